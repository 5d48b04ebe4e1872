"""Independent NumPy restatement of register.search: the record, position, voxel, cost and
sum rules 1-5 in fp32 arithmetic with int64 sums, the seed rule of the field, the level-0 lattice, the selection and the
ladder.  Nothing here imports sgnn_amd.  The field stands on edt_ref's separable passes (held to its brute force by
tests/test_edt_ref.py), the finish on register_ref.align.  Matrices are formed entry by entry with Python floats in the
orders the rules give, so the device route's vectorised host code has to reach the same fp64 bits; the integer scores,
the kept poses of every level and the guesses handed to align are compared bit for bit.  The scene and the settings of
the tests are at the end.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_ref as E  # noqa: E402
import register_ref as R  # noqa: E402

F32 = np.float32
MAX_POSES = 1 << 24


# ---------------------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------------------
def seeds(sdf, band):
    """Both voxels of every pair of axis neighbours that are usable (finite, |v| < band) with pv > 0 >= v or
    v > 0 >= pv."""
    s = np.asarray(sdf, F32)
    out = np.zeros(s.shape, bool)
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(s) & (np.abs(s) < F32(band))
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            pv, v = s[lo], s[hi]
            cross = usable[lo] & usable[hi] & (((pv > 0) & (v <= 0)) | ((v > 0) & (pv <= 0)))
            out[lo] |= cross
            out[hi] |= cross
    return out


def dist2_of(seed_mask, reach_vox, slab=6):
    """edt_ref's three passes, run a slab of planes at a time to bound memory, then its cap: (Z, Y, X) int32, -1 = no
    seed within reach."""
    g = np.where(seed_mask, 0, E.NONE).astype(np.int64)
    feat = np.arange(g.size, dtype=np.int64).reshape(g.shape)
    for axis, along in ((2, 0), (1, 0), (0, 1)):                            # a pass is independent along the other axes
        for lo in range(0, g.shape[along], slab):
            sl = [slice(None)] * 3
            sl[along] = slice(lo, lo + slab)
            sl = tuple(sl)
            g[sl], feat[sl] = E._pass(g[sl], feat[sl], axis)
    none = g == E.NONE
    d = np.where(none, -1, g).astype(np.int32)
    return E.cap(d, d, reach_vox)[0]


class Field(object):
    def __init__(self, dist2, world2grid, cap2):
        self.dist2, self.world2grid, self.cap2 = dist2, np.asarray(world2grid, F32), cap2
        self.dims = dist2.shape


def distance_field(sdf, world2grid, band, reach_vox):
    cap2 = E.cap2_of(reach_vox)
    assert cap2 is not None and cap2 >= 1
    return Field(dist2_of(seeds(sdf, band), reach_vox), world2grid, cap2)


# ---------------------------------------------------------------------------------------------------------
# rules 1-5
# ---------------------------------------------------------------------------------------------------------
def pose_rows(world2grid, T):
    """Rule 1 for one transform: (12,) fp32, NaN all over where an entry is not finite before or after rounding."""
    w = np.asarray(world2grid, np.float64)
    with np.errstate(all='ignore'):
        w = w.astype(F32).astype(np.float64)
    t = np.asarray(T, np.float64)
    m = np.zeros((3, 4))
    with np.errstate(all='ignore'):
        for i in range(3):
            for j in range(4):
                m[i, j] = ((w[i, 0] * t[0, j] + w[i, 1] * t[1, j]) + w[i, 2] * t[2, j]) + w[i, 3] * t[3, j]
        r = m.astype(F32).reshape(12)
    if not (np.isfinite(w).all() and np.isfinite(t).all() and np.isfinite(m).all() and np.isfinite(r).all()):
        return np.full(12, np.nan, F32)
    return r


def pose_rows_many(world2grid, T):
    """pose_rows over (B, 4, 4), vectorised over B with the same expression per entry."""
    with np.errstate(all='ignore'):
        w = np.asarray(world2grid, np.float64).astype(F32).astype(np.float64)
    t = np.asarray(T, np.float64)
    m = np.zeros((len(t), 3, 4))
    with np.errstate(all='ignore'):
        for i in range(3):
            for j in range(4):
                m[:, i, j] = ((w[i, 0] * t[:, 0, j] + w[i, 1] * t[:, 1, j]) + w[i, 2] * t[:, 2, j]) + w[i, 3] * t[:, 3, j]
        r = m.reshape(-1, 12).astype(F32)
    ok = np.isfinite(t).all(axis=(1, 2)) & np.isfinite(m).all(axis=(1, 2)) & np.isfinite(r).all(axis=1) & \
        bool(np.isfinite(w).all())
    r[~ok] = np.nan
    return r


def score_rows(points, dist2, rows, cap2, inlier2):
    """Rules 2-5 for records rows (B, 12) fp32 -> (B, 3) int64: cost, inliers, outside."""
    p = np.asarray(points, F32).reshape(-1, 3)
    d2 = np.asarray(dist2, np.int32)
    dz, dy, dx = d2.shape
    flat = d2.reshape(-1).astype(np.int64)
    rows = np.asarray(rows, F32).reshape(-1, 12)
    out = np.zeros((len(rows), 3), np.int64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    half = F32(0.5)
    for b, m in enumerate(rows):
        if len(p) == 0:
            break
        if not m[0] == m[0]:                                                # rule 1: the kernel tests m[0]
            out[b] = (len(p) * cap2, 0, len(p))
            continue
        with np.errstate(all='ignore'):
            g = [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)]   # rule 2
            n = [np.floor(v + half) for v in g]                             # rule 3
            inside = np.ones(len(p), bool)
            for v, k, d in zip(g, n, (dx, dy, dz)):
                assert v.dtype == F32 and k.dtype == F32
                inside &= np.isfinite(v) & (k >= 0) & (k <= F32(d - 1))
        nx, ny, nz = (np.where(inside, k, 0).astype(np.int64) for k in n)
        d = flat[(nz * dy + ny) * dx + nx]
        cost = np.where(inside & (d >= 0), np.minimum(d, cap2), cap2)       # rule 4
        out[b] = (cost.sum(dtype=np.int64), (inside & (d >= 0) & (d <= inlier2)).sum(), (~inside).sum())   # rule 5
    return out


def score(points, field, T, inlier2=1):
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    return score_rows(points, field.dist2, pose_rows_many(field.world2grid, T), field.cap2, inlier2)


# ---------------------------------------------------------------------------------------------------------
# poses, entry by entry
# ---------------------------------------------------------------------------------------------------------
def rotation(u, angle):
    s, v = math.sin(angle), 1.0 - math.cos(angle)
    k = [[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]]
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    return [[(eye[i][j] + s * k[i][j]) + v * (u[i] * u[j] - eye[i][j]) for j in range(3)] for i in range(3)]


def mul3(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def pose(rot, centre_to, c):
    """The transform that turns by rot and takes c to centre_to: t = centre_to - rot . c."""
    t = np.eye(4)
    for i in range(3):
        for j in range(3):
            t[i, j] = rot[i][j]
        t[i, 3] = centre_to[i] - ((rot[i][0] * c[0] + rot[i][1] * c[1]) + rot[i][2] * c[2])
    return t


def unit(up):
    u = [float(v) for v in up]
    n = math.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return [v / n for v in u]


def lattice(dims, world2grid, step=None, up=(0, 0, 1), z_range=None):
    """(origin, (nx, ny, nz), pitch): the world box of the 8 corner voxel centres, k = 0 .. floor(span / pitch)."""
    w = np.asarray(world2grid, F32).astype(np.float64)
    inv = np.linalg.inv(w)
    dz, dy, dx = dims
    world = []
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                g = (float(i * (dx - 1)), float(j * (dy - 1)), float(k * (dz - 1)))
                world.append([((inv[a, 0] * g[0] + inv[a, 1] * g[1]) + inv[a, 2] * g[2]) + inv[a, 3] for a in range(3)])
    lo, hi = [min(p[a] for p in world) for a in range(3)], [max(p[a] for p in world) for a in range(3)]
    pitch = 4.0 / math.sqrt((w[0, 0] * w[0, 0] + w[0, 1] * w[0, 1]) + w[0, 2] * w[0, 2]) if step is None else float(step)
    if z_range is not None:
        a = int(np.argmax(np.abs(unit(up))))
        lo[a], hi[a] = float(z_range[0]), float(z_range[1])
    return lo, tuple(int(math.floor((hi[a] - lo[a]) / pitch)) + 1 for a in range(3)), pitch


def select(costs, decode, top, cyclic=0):
    """Ascending (cost, index); a candidate is dropped if a kept one has a rotation index within one (cyclically for
    cyclic = Nr) and a lattice position within one pitch on every axis."""
    order = np.argsort(np.asarray(costs), kind='stable')
    kept = []
    for i in order:
        r, kz, ky, kx = decode(int(i))
        clash = False
        for q in kept:
            qr, qz, qy, qx = decode(q)
            dr = abs(r - qr)
            if (dr <= 1 or (cyclic > 1 and dr == cyclic - 1)) and max(abs(kz - qz), abs(ky - qy), abs(kx - qx)) <= 1:
                clash = True
        if not clash:
            kept.append(int(i))
        if len(kept) == top:
            break
    return kept


class Trace(object):
    """What the ladder went through: level0 (B, 3), kept: per level (T (K, 4, 4), scores (K, 3)), guesses, results."""


def search(points, sdf, world2grid, band, field, rotations=None, yaw_step=10.0, up=(0, 0, 1), step=None, z_range=None,
           max_points=4096, top=16, levels=4, tilt=False, finish=True, **align_kwargs):
    """The ladder of section X -> (T or None, Trace)."""
    pts_all = np.asarray(points, F32).reshape(-1, 3)
    pts = pts_all[::-(-len(pts_all) // max_points)]
    fin = pts[np.isfinite(pts).all(axis=1)].astype(np.float64)
    c = [float(v) for v in np.ascontiguousarray(fin).sum(axis=0) / len(fin)]
    u = unit(up)
    if rotations is None:
        nr = int(math.ceil(360.0 / yaw_step))
        rots = [rotation(u, math.radians(k * yaw_step)) for k in range(nr)]
    else:
        rots = [[[float(v) for v in row] for row in m] for m in np.asarray(rotations, np.float64)]
        nr = len(rots)
    origin, (nx, ny, nz), pitch = lattice(field.dims, world2grid, step, up, z_range)

    def decode(i):
        return i // (nx * ny * nz), (i // (nx * ny)) % nz, (i // nx) % ny, i % nx

    def centre_of(i):
        _, kz, ky, kx = decode(i)
        return [origin[0] + kx * pitch, origin[1] + ky * pitch, origin[2] + kz * pitch]

    total = nr * nz * ny * nx
    tr = Trace()
    tr.lattice = (origin, (nx, ny, nz), pitch)
    tr.centroid = c
    T0 = np.stack([pose(rots[decode(i)[0]], centre_of(i), c) for i in range(total)])
    tr.level0 = score(pts, field, T0)
    kept = select(tr.level0[:, 0], decode, top, nr if rotations is None else 0)
    state = [(rots[decode(i)[0]], centre_of(i)) for i in kept]
    tr.kept = [(np.stack([pose(r, ctr, c) for r, ctr in state]), tr.level0[kept])]
    angles_of = lambda d: (-d, 0.0, d)                                      # noqa: E731
    for level in range(1, levels + 1):
        s, delta = pitch / 2.0 ** level, math.radians(yaw_step) / 2.0 ** level
        if tilt:
            ex, ey, ez = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
            turns = [mul3(rotation(ez, az), mul3(rotation(ey, ay), rotation(ex, ax)))
                     for ax in angles_of(delta) for ay in angles_of(delta) for az in angles_of(delta)]
        else:
            turns = [rotation(u, a) for a in angles_of(delta)]
        new_state, new_scores = [], []
        for rot, ctr in state:
            hood = [(mul3(d, rot), [ctr[0] + ox * s, ctr[1] + oy * s, ctr[2] + oz * s])
                    for d in turns for oz in (-1.0, 0.0, 1.0) for oy in (-1.0, 0.0, 1.0) for ox in (-1.0, 0.0, 1.0)]
            sc = score(pts, field, np.stack([pose(r, q, c) for r, q in hood]))
            k = int(np.argmin(sc[:, 0]))                                    # the first minimum: (cost, index)
            new_state.append(hood[k])
            new_scores.append(sc[k])
        state = new_state
        tr.kept.append((np.stack([pose(r, q, c) for r, q in state]), np.stack(new_scores)))
    tr.guesses = tr.kept[-1][0]
    if not finish:
        return None, tr
    tr.results = [R.align(pts_all, sdf, world2grid, band, guess=g, **align_kwargs) for g in tr.guesses]
    chosen = R.best(tr.results)
    return (None if chosen is None else chosen.T), tr


# ---------------------------------------------------------------------------------------------------------
# the scene of the tests: register_ref's room, its source points taken to a world 70 degrees and more than a metre away
# ---------------------------------------------------------------------------------------------------------
ROOM_REACH_VOX = 10.0
ROOM_SETTINGS = dict(yaw_step=30.0, max_points=512, top=3, levels=4)
ROOM_PITCH_VOX = 6.4                        # the level-0 pitch in voxels of 5 cm: the truth is 0.35 and 0.44 pitches off a node
ROOM_YAW = 70.0                             # two steps of 30 degrees and a third
ROOM_SHIFT = (1.3, -0.9, 0.35)


def room_true():
    """Source world -> room world: a turn of ROOM_YAW about the vertical through the origin, then ROOM_SHIFT."""
    t = np.eye(4)
    a = math.radians(ROOM_YAW)
    t[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    t[:3, 3] = ROOM_SHIFT
    return t


_ROOM = []


def room_search_scene():
    """(sdf, world2grid, band, source points (P, 3) fp32, their centre, the true transform, settings): the room of
    register_ref.room_scene(); its points are taken back to the room's world (register_ref.ROOM_TRUE) and from there
    through inv(room_true()) in fp64, rounded to fp32.  The pitch is 6.4 voxels; z_range starts a pitch and a third
    below where the true transform puts the scoring points' centroid and ends a pitch above it (three planes), so that
    the truth lies a third of a pitch off a lattice plane on that axis too.  Computed once and shared."""
    if not _ROOM:
        sdf, w2g, src, _ = R.room_scene()
        dst = src.astype(np.float64) @ R.ROOM_TRUE[:3, :3].T + R.ROOM_TRUE[:3, 3]
        true = room_true()
        inv = np.linalg.inv(true)
        pts = (dst @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
        pitch = ROOM_PITCH_VOX * R.VS
        sub = pts[::-(-len(pts) // ROOM_SETTINGS['max_points'])].astype(np.float64)
        cz = float((true[:3, :3] @ sub.mean(0) + true[:3, 3])[2])
        settings = dict(ROOM_SETTINGS, step=pitch, z_range=(cz - pitch - pitch / 3, cz + pitch))
        _ROOM.append((sdf, w2g, R.ROOM_BAND, pts, pts.astype(np.float64).mean(0), true, settings))
    return _ROOM[0]


_FIELD = []


def room_field():
    if not _FIELD:
        sdf, w2g, band = room_search_scene()[:3]
        _FIELD.append(distance_field(sdf, w2g, band, ROOM_REACH_VOX))
    return _FIELD[0]


BOX_SHIFT = np.array([0.08, -0.05, -0.285])     # 30 cm, mostly down: the turned box stays on register_ref's grid


def box_search_true():
    """The second box volume of the search_volumes test: the box of register_ref moved by 40 degrees about the vertical
    through its centre and by 30 cm."""
    c = R.BOX_LO + R.BOX_EXT / 2
    t = np.eye(4)
    a = math.radians(40.0)
    t[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    t[:3, 3] = c - t[:3, :3] @ c + BOX_SHIFT
    return t


def box_search_ref(finish=True):
    """The restatement's search of the two box volumes with the defaults of register.search_volumes -> (T, Trace, true,
    source points, their centre).  A TSDFVolume's band is 3 voxels and its reach 0.5 m."""
    true = box_search_true()
    src, dst = R.box_volume_ref(), R.box_volume_ref(true)
    band = F32(3.0) * R.BOX_VS
    pts = R.surface_points(src, R.box_w2g(), band, R.BOX_STRIDE)
    field = distance_field(dst, R.box_w2g(), band, 0.5 / float(R.BOX_VS))
    T, tr = search(pts, dst, R.box_w2g(), band, field, finish=finish)
    return T, tr, true, pts, pts.astype(np.float64).mean(0)


def nearest_twin(true, T, centre):
    """(metres, degrees) from T to the nearest of box_twins(true)."""
    return min((R.transform_error(t, T, centre) for t in box_twins(true)), key=lambda e: e[0] + math.radians(e[1]))


def box_twins(true):
    """The transforms that differ from `true` by a symmetry of the box (a cuboid: the identity and the half turns about
    its three axes through its centre), applied in the source world."""
    c = R.BOX_LO + R.BOX_EXT / 2
    out = []
    for signs in ((1, 1, 1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1)):
        s = np.eye(4)
        s[:3, :3] = np.diag(signs)
        s[:3, 3] = c - s[:3, :3] @ c
        out.append(true @ s)
    return out


# The accuracy the ladder reaches on the CPU: measured and held by tests/test_register_search_ref.py, quoted in
# INTEGRATION.md section X, asserted at 1.5x on the device by tests/test_gpu_register_search.py.
SEARCH_ERROR = (7.327e-8, 6.172e-7)         # final error of the room search: metres, degrees
BOX_SEARCH_ERROR = (0.0003386, 0.06985)             # search of the two box volumes against the nearest twin of the truth
