"""Scenes shared by tests/test_points_ref.py and tests/test_gpu_points.py (no sgnn_amd import, no GPU)."""
import functools

import numpy as np

import fusion_ref as FR
import render_ref as RR

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------
# the common set-up: a 24 x 20 x 16 grid of 5 cm voxels, rotated about a skew axis and shifted
# ---------------------------------------------------------------------------------------------------------
DIMS = (24, 20, 16)
VS = F32(0.05)
DMIN, DMAX = 0.1, 3.0


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def world2grid():
    m = np.eye(4)
    m[:3, :3] = rotation((0.3, -0.5, 0.8), 0.7) / float(VS)
    m[:3, 3] = (3.25, -1.5, 7.75)
    return m.astype(F32)


def to_world(grid_pts):
    g2w = np.linalg.inv(world2grid().astype(np.float64))
    return (np.asarray(grid_pts, np.float64) @ g2w[:3, :3].T + g2w[:3, 3]).astype(F32)


ORIGINS_GRID = np.array([[5.3, 4.1, 8.2], [-10.4, 8.3, 20.6]])       # the second one lies outside the grid
OBB = np.array([3.0, 1.5, 2.0, 17.0, 5.0, 0.0, -4.0, 13.6, 0.0, 0.0, 0.0, 11.0], F32)   # a, e0, e1, e2 (voxels)


@functools.lru_cache(maxsize=None)
def cloud(seed=0):
    """About 1 500 points on two walls and a box corner, in world metres: (points, origins, origin_id, rgba); a fifth
    of the colours have A == 0."""
    rng = np.random.default_rng(seed)
    u = rng.uniform
    wall_a = np.stack([np.full(600, 20.3), u(1.5, 18.5, 600), u(1.5, 14.5, 600)], 1)
    wall_b = np.stack([u(1.5, 20.3, 500), np.full(500, 17.2), u(1.5, 14.5, 500)], 1)
    lo, hi = np.array([9.0, 7.0, 3.0]), np.array([13.0, 11.0, 7.0])
    corner = []
    for ax in range(3):
        p = u(lo, hi, (130, 3))
        p[:, ax] = lo[ax]
        corner.append(p)
    grid_pts = np.concatenate([wall_a, wall_b] + corner)
    grid_pts = grid_pts[rng.permutation(len(grid_pts))]
    oid = (rng.random(len(grid_pts)) < 0.3).astype(np.int32)
    rgba = rng.integers(0, 256, (len(grid_pts), 4), dtype=np.uint8)
    rgba[:, 3] = np.where(rng.random(len(grid_pts)) < 0.2, 0, 255)
    return to_world(grid_pts), to_world(ORIGINS_GRID), oid, rgba


def ignored_rays(seed=1):
    """Rays that section P ignores or that never enter the grid, for the common set-up: (points, origin_id)."""
    pts, org, _, _ = cloud()
    far = org[0] + F32(DMAX + 0.5) * np.array([0.6, 0.0, 0.8], F32)
    near = org[0] + F32(DMIN * 0.5) * np.array([0.0, 1.0, 0.0], F32)
    away = org[1] + (org[1] - org[0]) * F32(0.2)                    # from the outer origin, away from the grid
    extra = np.array([[np.nan, 0, 0], [0, np.inf, 0], far, near, org[0], org[1], away, away * F32(1.01)], F32)
    return extra, np.array([0, 1, 0, 0, 0, 1, 1, 1], np.int32)


# ---------------------------------------------------------------------------------------------------------
# the cross-route scene: a closed box room with one box on the floor, seen from six poses inside it
# ---------------------------------------------------------------------------------------------------------
ROOM_EXT = (2.0, 1.6, 1.2)
ROOM_BOX = ((0.9, 0.5, 0.0), (1.4, 0.9, 0.4))
ROOM_PAD = 4
ROOM_HW = (60, 80)


@functools.lru_cache(maxsize=None)
def room():
    """dict: verts, faces (the mesh, world metres), dims, w2g, k (6, 4), poses (6, 4, 4)."""
    parts = [RR.box_mesh((0.0, 0.0, 0.0), ROOM_EXT, 2), RR.box_mesh(ROOM_BOX[0], ROOM_BOX[1], 2)]
    verts = np.concatenate([parts[0][0], parts[1][0]]).astype(F32)
    faces = np.concatenate([parts[0][1], parts[1][1] + len(parts[0][0])]).astype(np.int32)
    dims = tuple(int(round(e / float(VS))) + 2 * ROOM_PAD + 1 for e in ROOM_EXT)
    # the walls fall 0.37 of a voxel past a voxel centre: on a centre the sign of a voxel's sdf would be rounding noise
    w2g = FR.grid_transform((-(ROOM_PAD + 0.37) * float(VS),) * 3, float(VS))
    eyes = [(0.5, 0.5, 0.7), (1.5, 1.1, 0.8), (0.6, 1.2, 0.6), (1.6, 0.4, 0.9), (1.0, 0.8, 1.0), (0.45, 0.8, 0.5)]
    tgts = [(1.9, 1.5, 0.2), (0.1, 0.1, 0.1), (1.6, 0.3, 0.1), (0.2, 1.4, 0.3), (1.15, 0.7, 0.0), (1.9, 0.8, 0.4)]
    poses = np.stack([FR.look_at(e, t) for e, t in zip(eyes, tgts)])
    h, w = ROOM_HW
    k = np.tile(np.array([0.7 * w, 0.7 * w, (w - 1) / 2.0, (h - 1) / 2.0], F32), (6, 1))
    return {'verts': verts, 'faces': faces, 'dims': dims, 'w2g': w2g, 'k': k, 'poses': poses}


def cross_route_figures(sdf_a, w_a, sdf_b, w_b, vs):
    """(share of sign disagreements, max |sdf_A - sdf_B| / vs, voxels compared) over voxels where both routes have
    weight > 0 and |sdf| < vs."""
    a, b = np.asarray(sdf_a, np.float64), np.asarray(sdf_b, np.float64)
    with np.errstate(invalid='ignore'):
        sel = (np.asarray(w_a) > 0) & (np.asarray(w_b) > 0) & (np.abs(a) < float(vs)) & (np.abs(b) < float(vs))
    n = int(sel.sum())
    if n == 0:
        return 0.0, 0.0, 0
    return float(((a[sel] < 0) != (b[sel] < 0)).mean()), float(np.abs(a[sel] - b[sel]).max() / float(vs)), n
