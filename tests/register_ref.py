"""Independent NumPy restatement of the point-to-SDF registration rules (rules 1-8), of
surface_points and of the align loop.

Nothing here imports sgnn_amd.register.  Rules 2-6 are fp32 with one rounding per operation in the evaluation orders
the rules give, vectorised over the points; the sums of rule 7 are math.fsum over the exact fp64 products, so they are
the exact sums rounded once; the step is fp64.  The device must match residuals and cells bit for bit, and the sums
within rule 7's bound.  The scenes of the tests are at the end.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as C  # noqa: E402  (room_sdf: the analytic room as a volume)
import track_ref as K  # noqa: E402  (section I rules 6 and 8, which section R takes over word for word)

F32 = np.float32
term_table, system_from_terms, sum_bound, unpack, exp_se3, step = (K.term_table, K.system_from_terms, K.sum_bound,
                                                                   K.unpack, K.exp_se3, K.step)


# ---------------------------------------------------------------------------------------------------------
# rules 1-8
# ---------------------------------------------------------------------------------------------------------
def rows32(m):
    """Rule 1: rows 0..2 of a 4x4 rounded to fp32; None where an entry is not finite."""
    m = np.asarray(m, np.float64)
    if not np.isfinite(m).all():
        return None
    with np.errstate(all='ignore'):
        r = m[:3].astype(F32)
    return r if np.isfinite(r).all() else None


def affine(m, x, y, z):
    """((m0 x + m1 y) + m2 z) + m3 per row -> three fp32 arrays."""
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]


def lerp(p, q, a):
    return p + a * (q - p)


def terms(points, sdf, world2grid, T, band, max_dist=None, min_grad=0.5):
    """Rules 1-6 and 8 for one transform -> (J (N, 6) fp32, r (N,) fp32, residual (P,) fp32, cell (P,) int32)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    sdf = np.asarray(sdf, F32)
    dz, dy, dx = sdf.shape
    band = F32(band)
    max_dist = band if max_dist is None else F32(max_dist)
    min_grad2 = F32(min_grad) * F32(min_grad)
    residual, cell = np.full(len(p), np.nan, F32), np.full(len(p), -1, np.int32)
    t, w = rows32(T), rows32(world2grid)
    if t is None or w is None:
        return np.zeros((0, 6), F32), np.zeros(0, F32), residual, cell
    with np.errstate(all='ignore'):
        q = affine(t, p[:, 0], p[:, 1], p[:, 2])                            # rule 2
        g = affine(w, q[0], q[1], q[2])
        ok = np.isfinite(p).all(1)
        for v in q + g:
            ok &= np.isfinite(v)
        f = [np.floor(v) for v in g]                                        # rule 3
        for v, d in zip(f, (dx, dy, dz)):
            ok &= (v >= 0) & (v <= d - 2)
        ix, iy, iz = (np.where(ok, v, 0).astype(np.int64) for v in f)
        c = {(k, j, i): sdf[iz + k, iy + j, ix + i] for k in (0, 1) for j in (0, 1) for i in (0, 1)}
        for v in c.values():
            ok &= np.isfinite(v) & (np.abs(v) < band)
        ax, ay, az = (g[a] - f[a] for a in range(3))
        value = lerp(lerp(lerp(c[0, 0, 0], c[0, 0, 1], ax), lerp(c[0, 1, 0], c[0, 1, 1], ax), ay),
                     lerp(lerp(c[1, 0, 0], c[1, 0, 1], ax), lerp(c[1, 1, 0], c[1, 1, 1], ax), ay), az)
        # rule 4
        gx = lerp(lerp(c[0, 0, 1] - c[0, 0, 0], c[0, 1, 1] - c[0, 1, 0], ay),
                  lerp(c[1, 0, 1] - c[1, 0, 0], c[1, 1, 1] - c[1, 1, 0], ay), az)
        gy = lerp(lerp(c[0, 1, 0] - c[0, 0, 0], c[0, 1, 1] - c[0, 0, 1], ax),
                  lerp(c[1, 1, 0] - c[1, 0, 0], c[1, 1, 1] - c[1, 0, 1], ax), az)
        gz = lerp(lerp(c[1, 0, 0] - c[0, 0, 0], c[1, 0, 1] - c[0, 0, 1], ax),
                  lerp(c[1, 1, 0] - c[0, 1, 0], c[1, 1, 1] - c[0, 1, 1], ax), ay)
        n = [(w[0, a] * gx + w[1, a] * gy) + w[2, a] * gz for a in range(3)]
        len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]                    # rule 5
        ok &= (np.abs(value) <= max_dist) & np.isfinite(len2) & (len2 >= min_grad2)
        J = np.stack([q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0],
                      n[0], n[1], n[2]], -1).astype(F32)                    # rule 6
    assert value.dtype == F32 and J.dtype == F32
    residual[ok] = value[ok]
    cell[ok] = ((iz * dy + iy) * dx + ix)[ok]
    return J[ok], value[ok], residual, cell


def normal_equations(points, sdf, world2grid, T, band, **kw):
    J, r, _, _ = terms(points, sdf, world2grid, T, band, **kw)
    return system_from_terms(term_table(J, r))


def interpolant(sdf, g):
    """Rule 3's value at grid positions g (P, 3) in fp64 from the fp32 corners (for the gradient check)."""
    g = np.asarray(g, np.float64)
    f = np.floor(g).astype(np.int64)
    a = g - f
    c = {(k, j, i): sdf[f[:, 2] + k, f[:, 1] + j, f[:, 0] + i].astype(np.float64)
         for k in (0, 1) for j in (0, 1) for i in (0, 1)}
    return lerp(lerp(lerp(c[0, 0, 0], c[0, 0, 1], a[:, 0]), lerp(c[0, 1, 0], c[0, 1, 1], a[:, 0]), a[:, 1]),
                lerp(lerp(c[1, 0, 0], c[1, 0, 1], a[:, 0]), lerp(c[1, 1, 0], c[1, 1, 1], a[:, 0]), a[:, 1]), a[:, 2])


# ---------------------------------------------------------------------------------------------------------
# surface_points, align, best, apply
# ---------------------------------------------------------------------------------------------------------
def surface_points(sdf, world2grid, band=None, stride=1):
    """(P, 3) fp32 world-space zero crossings: the x pairs, the y pairs, the z pairs, each by the linear index of the
    pair's first voxel; every stride-th one, through inv(world2grid) (fp64 inverse rounded to fp32, affine())."""
    s = np.asarray(sdf, F32)
    band = F32(np.inf) if band is None else F32(band)
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(s) & (np.abs(s) < band)
    found = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[2 - axis], hi[2 - axis] = slice(0, -1), slice(1, None)
        pv, v = s[tuple(lo)], s[tuple(hi)]
        with np.errstate(invalid='ignore'):
            cross = usable[tuple(lo)] & usable[tuple(hi)] & (((pv > 0) & (v <= 0)) | ((v > 0) & (pv <= 0)))
        idx = np.argwhere(cross)
        a, b = pv[cross], v[cross]
        g = idx[:, ::-1].astype(F32)
        g[:, axis] = g[:, axis] + a / (a - b)
        found.append(g)
    g = np.concatenate(found)[::stride]
    m = np.linalg.inv(np.asarray(world2grid, F32).astype(np.float64)).astype(F32)
    return np.stack(affine(m, g[:, 0], g[:, 1], g[:, 2]), 1).astype(F32)


class Result(object):
    def __init__(self, T, ok, pairs, rmse, history):
        self.T, self.ok, self.pairs, self.rmse, self.history = T, ok, pairs, rmse, tuple(history)


def align(points, sdf, world2grid, band, guess=None, iterations=30, max_dist=None, min_grad=0.5, min_pairs=64):
    """One guess (4, 4) -> Result; the loop of sgnn_amd.register.align."""
    guess = np.eye(4) if guess is None else np.asarray(guess, np.float64)
    T = guess.copy()
    history, rmse, n = [], float('nan'), 0
    for _ in range(iterations):
        s = normal_equations(points, sdf, world2grid, T, band, max_dist=max_dist, min_grad=min_grad)
        n = int(s[28])
        history.append(n)
        xi = step(s, min_pairs)
        if xi is None:
            return Result(guess.copy(), False, n, float('nan'), history)
        rmse = math.sqrt(s[27] / n)
        T = exp_se3(xi) @ T
    return Result(T, True, n, rmse, history)


def best(results):
    ok = [r for r in results if r.ok]
    if not ok:
        return None
    most = max(r.pairs for r in ok)
    return min((r for r in ok if 2 * r.pairs >= most), key=lambda r: r.rmse)


def moved_world2grid(world2grid, T):
    """register.apply: world2grid . inv(T) in fp64, rounded to fp32."""
    return (np.asarray(world2grid, F32).astype(np.float64) @ np.linalg.inv(np.asarray(T, np.float64))).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# errors and perturbations (tests)
# ---------------------------------------------------------------------------------------------------------
def transform_error(true, got, centre):
    """(metres, degrees) between two transforms: how far `centre` (a point of the source world) lands from where the
    true transform puts it, and the angle of the rotation between the two."""
    true, got = np.asarray(true, np.float64), np.asarray(got, np.float64)
    c = np.append(np.asarray(centre, np.float64), 1.0)
    rel = got[:3, :3] @ true[:3, :3].T
    sine = 0.5 * np.linalg.norm([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]])
    angle = math.atan2(sine, (np.trace(rel) - 1) / 2)                       # no cancellation at small angles
    return float(np.linalg.norm((got @ c - true @ c)[:3])), float(np.degrees(angle))


def perturbed(true, seed, centre, trans=0.03, rot_deg=1.5):
    """`true` followed by a turn of rot_deg about a seeded random axis through the image of `centre` and a shift of
    `trans` along a seeded random direction: transform_error(true, result, centre) is (trans, rot_deg)."""
    rng = np.random.default_rng(2000 + seed)
    axis, direction = rng.normal(size=3), rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction /= np.linalg.norm(direction)
    true = np.asarray(true, np.float64)
    c = (true @ np.append(np.asarray(centre, np.float64), 1.0))[:3]
    d = exp_se3(np.concatenate([axis * np.radians(rot_deg), np.zeros(3)]))
    d[:3, 3] = c - d[:3, :3] @ c + trans * direction
    return d @ true


# ---------------------------------------------------------------------------------------------------------
# the room scene (CPU accuracy figures; one seed of it on the device)
# ---------------------------------------------------------------------------------------------------------
VS = 0.05
ROOM_BAND = F32(3.0) * F32(VS)
ROOM_STRIDE = 4
# the source world is the room's world moved by inv(ROOM_TRUE): a 10 degree turn about a tilted axis and a shift
ROOM_TRUE = exp_se3(np.concatenate([np.radians(10.0) * np.array([0.6, -0.48, 0.64]), [0.4, -0.3, 0.2]]))


def room_scene():
    """(sdf (60, 72, 88) fp32 in metres, world2grid, source points (P, 3) fp32, centre of the points): the analytic
    room of raycast_ref.room_sdf at 5 cm with a band of 3 voxels; the points are every ROOM_STRIDE-th of its own
    surface_points, taken to the source world through inv(ROOM_TRUE) in fp64 and rounded to fp32."""
    sdf, w2g = C.room_sdf(VS, 4, ROOM_BAND)
    assert sdf.shape == (60, 72, 88)
    dst = surface_points(sdf, w2g, ROOM_BAND, ROOM_STRIDE).astype(np.float64)
    inv = np.linalg.inv(ROOM_TRUE)
    src = (dst @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    return sdf, w2g, src, src.astype(np.float64).mean(0)


# ---------------------------------------------------------------------------------------------------------
# the small scene of the device tests, in voxel units on a 24 x 20 x 16 grid: a tilted plane with a sphere resting on it
# and a second, smaller sphere (a plane and one sphere leave the turn about the plane's normal through the sphere's
# centre free; the second sphere closes it)
# ---------------------------------------------------------------------------------------------------------
SMALL_DIMS = (24, 20, 16)
SMALL_BAND = F32(3.0)
SMALL_W2G = np.array([[8.0, 0, 0, 3.25], [0, 8.0, 0, 2.5], [0, 0, 8.0, 1.75], [0, 0, 0, 1]], F32)   # 0.125 m voxels
SMALL_NAN = (10, 8, 7)              # x, y, z of the one NaN voxel
# x, y, z of a cell with f = d - 2 on one axis that lies in the band, per axis, and the cell of the voxel-centre point
SMALL_EDGE_CELLS = ((22, 9, 1), (11, 18, 3), (13, 10, 14))
SMALL_CENTRE = (12, 9, 4)


def small_volume():
    """(sdf (16, 20, 24) fp32 in voxels, SMALL_W2G): the smallest of the distance above the plane n.x = 9.5 and the
    distances outside two spheres, so the field is positive above the plane and outside the spheres.  Voxels beyond
    the band keep their values (unusable by rule 3), a sprinkle of voxels is -inf (unseen) except in the cells the
    edge cases of small_points need, one voxel is NaN."""
    dx, dy, dz = SMALL_DIMS
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing='ij')
    p = np.stack([x, y, z], -1).astype(np.float64)
    n = np.array([0.28, 0.16, 0.9466])
    n /= np.linalg.norm(n)
    d = np.minimum(p @ n - 9.5, np.linalg.norm(p - np.array([13.2, 10.4, 8.9]), axis=-1) - 4.6)
    d = np.minimum(d, np.linalg.norm(p - np.array([5.5, 14.0, 9.5]), axis=-1) - 2.7)
    sdf = d.astype(F32)
    rng = np.random.default_rng(11)
    unseen = rng.random(sdf.shape) < 0.03
    nan_cells = ((SMALL_NAN[0] - 1, SMALL_NAN[1] - 1, SMALL_NAN[2] - 1), SMALL_NAN)
    for cx, cy, cz in SMALL_EDGE_CELLS + (SMALL_CENTRE,) + nan_cells:
        unseen[cz:cz + 2, cy:cy + 2, cx:cx + 2] = False
    sdf[unseen] = -np.inf
    sdf[SMALL_NAN[2], SMALL_NAN[1], SMALL_NAN[0]] = np.nan
    return sdf, SMALL_W2G.copy()


SMALL_SPECIAL = 16                  # the last SMALL_SPECIAL slots of small_points(count >= 17) are the edge cases


def small_points(count, seed=0):
    """`count` source points for the small scene: surface points jittered by up to a voxel, then the edge cases in fixed
    slots at the end, as far as `count` allows (in this order; positions in voxels, exact under the identity)."""
    sdf, w2g = small_volume()
    base = surface_points(sdf, w2g, SMALL_BAND)
    rng = np.random.default_rng(100 + seed)
    pts = base[rng.integers(0, len(base), size=count)] + rng.uniform(-0.125, 0.125, size=(count, 3)).astype(F32)
    pts = pts.astype(F32)
    m = np.linalg.inv(w2g.astype(np.float64))                               # exact: powers of two and quarters

    def world(*g):
        return (m[:3, :3] @ np.array(g) + m[:3, 3]).astype(F32)

    dx, dy, dz = SMALL_DIMS
    (ex, ey, ez), c = SMALL_EDGE_CELLS, SMALL_CENTRE
    special = [world(*c),                                                   # exactly on a voxel centre
               world(ex[0] + 0.5, ex[1] + 0.25, ex[2] + 0.75), world(dx - 1 + 0.25, ex[1] + 0.25, ex[2] + 0.75),
               world(ey[0] + 0.5, ey[1] + 0.5, ey[2] + 0.5), world(ey[0] + 0.5, dy - 1 + 0.25, ey[2] + 0.5),
               world(ez[0] + 0.25, ez[1] + 0.5, ez[2] + 0.5), world(ez[0] + 0.25, ez[1] + 0.5, dz - 1 + 0.25),
               world(-0.5, 9.25, 5.25), world(11.5, -2.25, 5.25), world(11.5, 9.25, -0.0078125),   # negative coordinates
               np.array([np.nan, 0.5, 0.5], F32), np.array([0.5, np.inf, 0.5], F32), np.array([0.5, 0.5, -np.inf], F32),
               world(9.5, 7.5, 6.5), world(10.5, 8.5, 7.5),                 # cells with the NaN voxel as a corner
               np.array([3e38, 3e38, 3e38], F32)]                           # a finite p whose q overflows
    assert len(special) == SMALL_SPECIAL
    k = min(SMALL_SPECIAL, max(count - 1, 0))
    if k:
        pts[count - k:] = np.stack(special[:k])
    return pts


def small_transforms():
    """[non-finite, the identity, a centimetre and a third of a degree off, several centimetres and degrees off]"""
    bad = np.eye(4)
    bad[1, 2] = np.nan
    near = exp_se3([0.004, -0.003, 0.005, 0.01, -0.008, 0.006])
    far = exp_se3([0.03, 0.02, -0.025, -0.06, 0.04, 0.05])
    return [bad, np.eye(4), near, far]


# ---------------------------------------------------------------------------------------------------------
# two volumes of one box (align_volumes): the box of 0.66 x 0.52 x 0.37 m voxelised at 5 cm on a 26 x 24 x 20 grid, once
# as it is (source) and once moved by BOX_TRUE, 2 cm and 1 degree (destination)
# ---------------------------------------------------------------------------------------------------------
BOX_DIMS, BOX_VS, BOX_VOX_BAND = (26, 24, 20), F32(0.05), 4.0
BOX_LO, BOX_EXT = np.array([0.315, 0.335, 0.32]), np.array([0.66, 0.52, 0.37])
BOX_STRIDE = 2


def box_true():
    c = BOX_LO + BOX_EXT / 2
    axis, direction = np.array([0.36, 0.48, 0.8]), np.array([0.6, -0.64, 0.48])
    t = exp_se3(np.concatenate([np.radians(1.0) * axis, np.zeros(3)]))
    t[:3, 3] = c - t[:3, :3] @ c + 0.02 * direction
    return t


def box_mesh(T=None):
    """(verts (8, 3) fp32 metres, faces (12, 3) int32, outward normals) of the box, moved by T."""
    verts = np.array([[BOX_LO[a] + (c >> a & 1) * BOX_EXT[a] for a in range(3)] for c in range(8)], np.float64)
    if T is not None:
        verts = verts @ T[:3, :3].T + T[:3, 3]
    faces = np.array([[0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5], [0, 1, 5], [0, 5, 4],
                      [2, 6, 7], [2, 7, 3], [0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6]], np.int32)
    return verts.astype(F32), faces


def box_w2g():
    m = np.eye(4, dtype=F32)
    m[:3, :3] /= BOX_VS
    return m


def box_volume_ref(T=None):
    """The sdf (metres, -inf beyond 4 voxels) that voxelize.mesh_to_volume gives for box_mesh(T), by voxelize_ref."""
    import voxelize_ref as VR
    verts, faces = box_mesh(T)
    ref = VR.signed_distance_ref(VR.grid_coords_ref(verts, box_w2g()), faces, BOX_DIMS, BOX_VOX_BAND)
    with np.errstate(invalid='ignore'):
        return np.where(ref.face >= 0, ref.dist * BOX_VS, F32(-np.inf)).astype(F32)


# The accuracy the rules reach on the CPU: measured and held by tests/test_register_ref.py, quoted in INTEGRATION.md
# section R, asserted at 1.5x on the device by tests/test_gpu_register.py.
TRANS, ROT = 0.03, 1.5                  # the perturbation of the guesses: 3 cm and 1.5 degrees
EXACT_DRIFT = (1.058e-7, 2.541e-7)             # from the exact transform: metres, degrees
ALIGN_ERROR = (1.530e-7, 6.288e-7)             # worst final error over seeds 0-3 of the room: metres, degrees
BOX_ERROR = (0.0005611, 0.03567)             # align_volumes of the two box volumes against the true 2 cm / 1 degree
