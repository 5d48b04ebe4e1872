"""Cases shared by tests/test_regrid_ref.py and tests/test_gpu_regrid.py.  No GPU.  The only thing taken from sgnn_amd is
the host-only regrid.grid_for, for the yawed destination boxes (grid_b, e2e_grid_b); tests/test_cabi_regrid.py checks it
on its own."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import fusion_ref as FR  # noqa: E402
import mc_oracle  # noqa: E402
import meshdist_ref as MR  # noqa: E402
import points_scenes as PS  # noqa: E402
import regrid_ref as GR  # noqa: E402
import render_ref as RR  # noqa: E402
import voxelize_ref as VR  # noqa: E402

F32 = np.float32
# source world2grid of the exact maps: a power-of-two scale and integer shifts, so every matrix below is exact
EXACT_W2G = np.array([[16, 0, 0, 3], [0, 16, 0, -2], [0, 0, 16, 5], [0, 0, 0, 1]], np.float64)
EXACT_DIMS = ((7, 5, 1), (6, 4, 3))


def exact_source(dims_xyz):
    """The random source of the exact maps: holes, colour, and at least one voxel with a weight but no finite sdf."""
    v = GR.random_volume(dims_xyz, 3, color=True, world2grid=EXACT_W2G)
    z, y, x = (int(c[0]) for c in np.nonzero(np.isfinite(v.sdf)))
    v.sdf[z, y, x] = -np.inf
    return v


def normalised(v):
    """What the identity map gives: an unobserved voxel (rule 2) is unseen, the free counter stays."""
    obs = (v.weight > 0) & np.isfinite(v.sdf)
    out = v.copy()
    out.sdf = np.where(obs, v.sdf, F32(-np.inf)).astype(F32)
    out.weight = np.where(obs, v.weight, 0)
    if v.color is not None:
        out.color = np.where(obs[..., None], v.color, 0)
    return out


def arrays(v):
    return [v.sdf, v.weight, v.free] + ([] if v.color is None else [v.color])


def unseen_like(a):
    return np.full(a.shape, -np.inf, F32) if a.dtype == F32 else np.zeros(a.shape, a.dtype)


def rot_z(sx):
    """dst -> src voxel coordinates of np.rot90(arr, 1, axes=(1, 2)) on (z, y, x) arrays: out[z, y', x'] =
    arr[z, x', sx - 1 - y']."""
    return np.array([[0, -1, 0, sx - 1], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def exact_maps(dims_xyz):
    """[(name, dst dims_xyz, M (dst -> src voxel coordinates, integers), expect(arr) -> arr)] for a source of dims_xyz."""
    sx, sy, sz = dims_xyz
    eye = np.eye(4)

    def shifted(t):
        tx, ty, tz = t

        def f(a):
            out = unseen_like(a)
            zs, ys, xs = (slice(max(0, -o), min(n, n - o)) for o, n in ((tz, sz), (ty, sy), (tx, sx)))
            zd, yd, xd = (slice(max(0, o), min(n, n + o)) for o, n in ((tz, sz), (ty, sy), (tx, sx)))
            out[zd, yd, xd] = a[zs, ys, xs]
            return out
        m = eye.copy()
        m[:3, 3] = (-tx, -ty, -tz)                 # dst voxel i shows src voxel i - t
        return m, f

    cases = [('identity', dims_xyz, eye, lambda a: a)]
    for t in ((2, -1, 0), (-3, 2, 1 if sz > 1 else 0)):
        m, f = shifted(t)
        cases.append(('shift%s' % (t,), dims_xyz, m, f))
    for ax, n in ((0, sx), (1, sy), (2, sz)):
        m = eye.copy()
        m[ax, ax], m[ax, 3] = -1, n - 1
        cases.append(('flip%d' % ax, dims_xyz, m, functools.partial(np.flip, axis=2 - ax)))
    m, d = eye, (sx, sy)
    for k in (1, 2, 3):
        m = m @ rot_z(d[0])
        d = (d[1], d[0])
        cases.append(('rot%d' % (90 * k), (d[0], d[1], sz), m.copy(), functools.partial(np.rot90, k=k, axes=(1, 2))))
    return cases


def exact_dst_w2g(m):
    """The destination world2grid whose map back to the EXACT_W2G source is m."""
    return (np.linalg.inv(m) @ EXACT_W2G).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# the general similarity of the bit-equality cases: yaw + pitch, scale 0.7, shift
# ---------------------------------------------------------------------------------------------------------
SRC_DIMS = (20, 17, 13)
DST_DIMS = ((23, 11, 19), (9, 8, 1))
SRC_W2G = PS.world2grid()


def similarity_w2g(dims_xyz):
    """A destination grid whose centre sits near the source's centre, turned by a yaw and a pitch, with voxels 0.7 of
    the source's: part of it looks outside the source."""
    yaw, pitch = PS.rotation((0, 0, 1), 0.6), PS.rotation((0, 1, 0), -0.35)
    m = np.eye(4)
    m[:3, :3] = (yaw @ pitch) * 0.7                                   # dst voxel -> src voxel
    m[:3, 3] = (np.array(SRC_DIMS) - 1) / 2.0 + (2.3, -3.45, 1.2) - m[:3, :3] @ ((np.array(dims_xyz) - 1) / 2.0)
    return (np.linalg.inv(m) @ SRC_W2G.astype(np.float64)).astype(F32)


def planes_w2g():
    """Destination voxels exactly on the source's last plane and on half-integer positions: dst = 2 src - 1 on x (so odd
    dst voxels sit on integers, even ones on halves, and dst 2 (sx - 1) + 1 on the last plane), a half-voxel shift on y,
    identity on z, over the EXACT_W2G source."""
    m = np.eye(4)
    m[0, 0], m[0, 3] = 0.5, 0.5
    m[1, 3] = -0.5
    return (np.linalg.inv(m) @ EXACT_W2G).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# the cross-route scene: the room of points_scenes on grid A and on grid B = A yawed by 30 degrees about the up axis
# ---------------------------------------------------------------------------------------------------------
def yaw_about_room_centre(deg=30.0):
    c = np.array(PS.ROOM_EXT) / 2.0
    t = np.eye(4)
    t[:3, :3] = PS.rotation((0, 0, 1), np.deg2rad(deg))
    t[:3, 3] = c - t[:3, :3] @ c
    return t


class GridStub(object):
    """What regrid.grid_for looks at."""

    def __init__(self, dims_xyz, voxel_size, world2grid):
        self.dims_xyz, self.voxel_size, self.world2grid = tuple(dims_xyz), F32(voxel_size), np.asarray(world2grid, F32)


@functools.lru_cache(maxsize=None)
def grid_b():
    from sgnn_amd import regrid
    room = PS.room()
    return regrid.grid_for(GridStub(room['dims'], PS.VS, room['w2g']), yaw_about_room_centre(), pad=0)


def as_vol(g):
    """A fusion_ref.Grid as a regrid_ref.Vol."""
    return GR.from_state(g.dims, g.vs, g.w2g, g.sdf, g.weight, g.free, getattr(g, 'color', None))


# ---------------------------------------------------------------------------------------------------------
# one fold, two callers: a cloud fused directly, and fused on an empty volume that is then merged (rules P and Q.8)
# ---------------------------------------------------------------------------------------------------------
FOLD_HW = (30, 40)
FOLD_VOXEL = (16, 18, 12)       # 0.54 m from the eye of pose 2: every ray that ends in it weighs 4
FOLD_AIMED = 72                 # 72 x 4 = 288 > 255: the call's weight for that voxel saturates


@functools.lru_cache(maxsize=None)
def fold_scene():
    """The corner of the room of points_scenes on PS.DIMS voxels: two depth frames (poses 1 and 4) that fill the volume
    first, and a coloured cloud from two origins: every eighth pixel of the frames of poses 2 and 3 (300 rays, a fifth
    with A == 0) and FOLD_AIMED rays from pose 2 that end inside FOLD_VOXEL.  dict: dims, w2g, depth, k, poses, pts, org,
    oid, rgba."""
    import points_ref as PR
    room = PS.room()
    k = np.tile(np.array([28.0, 28.0, 19.5, 14.5], F32), (6, 1))
    depth = RR.render_ref(room['verts'], room['faces'], k, room['poses'], FOLD_HW)
    pts, org, oid = PR.from_depth(depth[2:4], k[2:4], room['poses'][2:4])
    pts, oid = pts[::8], oid[::8]
    rng = np.random.default_rng(17)
    centre = (np.array(FOLD_VOXEL, np.float64) - room['w2g'][:3, 3]) * float(PS.VS)     # w2g is a scale and a shift
    aimed = (centre + rng.uniform(-0.3, 0.3, (FOLD_AIMED, 3)) * float(PS.VS)).astype(F32)
    pts, oid = np.concatenate([pts, aimed]), np.concatenate([oid, np.zeros(FOLD_AIMED, np.int32)])
    rgba = rng.integers(0, 256, (len(pts), 4), dtype=np.uint8)
    rgba[:, 3] = np.where(rng.random(len(pts)) < 0.2, 0, 255)
    sel = [1, 4]
    return {'dims': PS.DIMS, 'w2g': room['w2g'], 'depth': depth[sel], 'k': k[sel], 'poses': room['poses'][sel],
            'pts': pts, 'org': org, 'oid': oid, 'rgba': rgba}


@functools.lru_cache(maxsize=None)
def cross_route_ref():
    """On the CPU: (A->B resampled, B fused directly, A[0:3] merged into B[3:6], the frames)."""
    room = PS.room()
    depth = RR.render_ref(room['verts'], room['faces'], room['k'], room['poses'], PS.ROOM_HW)
    dims_b, w2g_b = grid_b()

    def fuse(dims, w2g, sel):
        return FR.Grid(dims, PS.VS, w2g).integrate(depth[sel], room['k'][sel], room['poses'][sel])
    a_all, b_all = fuse(room['dims'], room['w2g'], slice(0, 6)), fuse(dims_b, w2g_b, slice(0, 6))
    merged = GR.merge(as_vol(fuse(dims_b, w2g_b, slice(3, 6))), as_vol(fuse(room['dims'], room['w2g'], slice(0, 3))))
    return GR.resample(as_vol(a_all), dims_b, w2g_b), as_vol(b_all), merged, depth



def cross_route_extra(sdf_a, w_a, sdf_b, w_b, vs):
    """Two figures that bite harder than points_scenes.cross_route_figures, over the same selection (both observed,
    |sdf| < vs on both): (mean |sdf_A - sdf_B| / vs, share of sign disagreements among the voxels that lie more than
    0.3 vs off the surface on both routes, the number of those voxels).  A shifted or mirrored map moves the first; the
    second leaves out the voxels whose sign the frame route's own noise decides."""
    a, b, vs = np.asarray(sdf_a, np.float64), np.asarray(sdf_b, np.float64), float(vs)
    with np.errstate(invalid='ignore'):
        sel = (np.asarray(w_a) > 0) & (np.asarray(w_b) > 0) & (np.abs(a) < vs) & (np.abs(b) < vs)
        far = sel & (np.abs(a) > 0.3 * vs) & (np.abs(b) > 0.3 * vs)
    return float(np.abs(a[sel] - b[sel]).mean() / vs), float(((a[far] < 0) != (b[far] < 0)).mean()), int(far.sum())


# ---------------------------------------------------------------------------------------------------------
# end to end: a box mesh voxelised on grid A, resampled to grid B = A yawed by 30 degrees about the box's centre, meshed
# by marching cubes and measured against the box (meshdist accuracy: mean distance from the extracted surface to the box)
# ---------------------------------------------------------------------------------------------------------
E2E_VS = F32(0.05)
E2E_DIMS = (26, 24, 20)
E2E_BAND = 4.0                      # voxels; the box is 7.4 voxels thin, so all of its inside is in the band
E2E_MC_ARGS = (0.0, 1.0, 10.0)      # metric sdf: no truncation inside the band, no jump test
E2E_SAMPLES = 20000
E2E_MAX_DIST = 0.5
E2E_LO, E2E_EXT = np.array([0.315, 0.335, 0.32]), np.array([0.66, 0.52, 0.37])


def e2e_box():
    """(verts (8, 3) fp32 in metres, faces (12, 3) int32 with outward normals); vertex c sits at bit 0 / 1 / 2 of c on
    x / y / z.  On grid A it spans voxels 6.3 .. 19.5, 6.7 .. 17.1 and 6.4 .. 13.8."""
    verts = np.array([[E2E_LO[a] + (c >> a & 1) * E2E_EXT[a] for a in range(3)] for c in range(8)], F32)
    faces = np.array([[0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5], [0, 1, 5], [0, 5, 4],
                      [2, 6, 7], [2, 7, 3], [0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6]], np.int32)
    return verts, faces


def e2e_w2g_a():
    m = np.eye(4, dtype=F32)
    m[:3, :3] /= E2E_VS
    return m


@functools.lru_cache(maxsize=None)
def e2e_grid_b():
    from sgnn_amd import regrid
    c = E2E_LO + E2E_EXT / 2.0
    t = np.eye(4)
    t[:3, :3] = PS.rotation((0, 0, 1), np.deg2rad(30.0))
    t[:3, 3] = c - t[:3, :3] @ c
    return regrid.grid_for(GridStub(E2E_DIMS, E2E_VS, e2e_w2g_a()), t, pad=0)


def e2e_world(verts_grid, w2g):
    """Marching-cubes vertices (x, y, z in voxels of the grid w2g) in world coordinates, fp32."""
    g2w = np.linalg.inv(np.asarray(w2g, F32).astype(np.float64)).astype(F32)
    return np.asarray(verts_grid, F32) @ g2w[:3, :3].T + g2w[:3, 3]


@functools.lru_cache(maxsize=None)
def e2e_ref():
    """The restatement route on the CPU: voxelize_ref -> regrid_ref -> mc_oracle -> meshdist_ref.  (accuracy in metres,
    faces of the extracted mesh, the volume on A, the volume on B)."""
    verts, faces = e2e_box()
    ref = VR.signed_distance_ref(VR.grid_coords_ref(verts, e2e_w2g_a()), faces, E2E_DIMS, E2E_BAND)
    inband = ref.face >= 0
    with np.errstate(invalid='ignore'):
        sdf = np.where(inband, ref.dist * E2E_VS, F32(-np.inf)).astype(F32)      # section L: one fp32 product
    on_a = GR.from_state(E2E_DIMS, E2E_VS, e2e_w2g_a(), sdf, inband.astype(np.int64), 0)
    dims_b, w2g_b = e2e_grid_b()
    on_b = GR.resample(on_a, dims_b, w2g_b)
    v, _, f = mc_oracle.run_marching_cubes(on_b.sdf, None, *E2E_MC_ARGS)
    world = e2e_world(v, w2g_b)
    pts, _ = MR.sample_ref(world, f, E2E_SAMPLES, 0, MR.areas_ref(world, f)[1])
    d, _ = MR.distance_ref(pts, verts, faces, E2E_MAX_DIST)
    return MR.compare_ref(d, d, max_dist=E2E_MAX_DIST)['accuracy'], len(f), on_a, on_b
