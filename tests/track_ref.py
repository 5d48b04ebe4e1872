"""Independent NumPy restatement of the frame-to-model tracking rules (rules 1-10).

Nothing here imports sgnn_amd.track.  Rules 2-5, 9 and 10 are fp32 with one rounding per operation in the evaluation
orders the rules give, vectorised over the pixels of a frame; the sums of rule 6 are math.fsum over the exact fp64
products, so they are the exact sums rounded once; rule 8 is fp64.  align() and track_sequence() run the whole loop on
the CPU with fusion_ref.Grid as the volume and raycast_ref.cast as the caster.  The device must match residuals,
associations, pyramid levels and normals bit for bit, and the sums within rule 6's bound.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402

F32 = np.float32
NINF = F32(-np.inf)
TRIU = [(a, b) for a in range(6) for b in range(a, 6)]


# ---------------------------------------------------------------------------------------------------------
# rules 1-7
# ---------------------------------------------------------------------------------------------------------
def pair_matrix(model_pose, live_pose):
    """Rule 1 in fp64: inv(model_pose) . live_pose."""
    return np.linalg.inv(np.asarray(model_pose, np.float64)) @ np.asarray(live_pose, np.float64)


def rows32(T):
    """Rows 0..2 of T rounded to fp32; None for an empty system."""
    T = np.asarray(T, np.float64)
    if not np.isfinite(T).all():
        return None
    with np.errstate(all='ignore'):
        t = T[:3].astype(F32)
    return t if np.isfinite(t).all() else None


def backproject(d, k):
    """Rule 2's p for every pixel of a frame d (h, w) -> three (h, w) fp32 arrays."""
    h, w = d.shape
    fx, fy, cx, cy = (F32(v) for v in k)
    i, j = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    return ((i - cx) / fx) * d, ((j - cy) / fy) * d, d


def terms(depth, k, model_depth, model_normal, k_model, T, max_dist=0.1, max_angle_deg=20.0, live_normal=None):
    """Rules 1-5 and 7 for one pair -> (J (N, 6) fp32, r (N,) fp32, residual (h, w) fp32, assoc (h, w) int32)."""
    d = np.asarray(depth, F32)
    md, mn = np.asarray(model_depth, F32), np.asarray(model_normal, F32)
    h, w = d.shape
    hm, wm = md.shape
    residual, assoc = np.full((h, w), np.nan, F32), np.full((h, w), -1, np.int32)
    t = rows32(T)
    if t is None:
        return np.zeros((0, 6), F32), np.zeros(0, F32), residual, assoc
    fxm, fym, cxm, cym = (F32(v) for v in k_model)
    with np.errstate(all='ignore'):
        ok = np.isfinite(d) & (d > 0)
        px, py, pz = backproject(d, k)
        q = [((t[r, 0] * px + t[r, 1] * py) + t[r, 2] * pz) + t[r, 3] for r in range(3)]
        ok &= q[2] > 0
        u = R.round_away((q[0] * fxm) / q[2] + cxm)
        v = R.round_away((q[1] * fym) / q[2] + cym)
        ok &= (u >= 0) & (u < wm) & (v >= 0) & (v < hm)
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        dm, n = md[vi, ui], mn[vi, ui]
        ok &= np.isfinite(dm) & (dm > 0) & np.isfinite(n).all(-1)
        m = [((u - cxm) / fxm) * dm, ((v - cym) / fym) * dm, dm]
        e = [q[c] - m[c] for c in range(3)]
        ok &= (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= F32(max_dist) * F32(max_dist)
        if live_normal is not None:
            ln = np.asarray(live_normal, F32)
            rot = [(t[r, 0] * ln[..., 0] + t[r, 1] * ln[..., 1]) + t[r, 2] * ln[..., 2] for r in range(3)]
            cos_min = F32(math.cos(math.radians(float(max_angle_deg))))
            ok &= (rot[0] * n[..., 0] + rot[1] * n[..., 1]) + rot[2] * n[..., 2] >= cos_min     # NaN fails
        r = (n[..., 0] * e[0] + n[..., 1] * e[1]) + n[..., 2] * e[2]
        J = np.stack([q[1] * n[..., 2] - q[2] * n[..., 1], q[2] * n[..., 0] - q[0] * n[..., 2],
                      q[0] * n[..., 1] - q[1] * n[..., 0], n[..., 0], n[..., 1], n[..., 2]], -1).astype(F32)
    residual[ok] = r[ok]
    assoc[ok] = (vi * wm + ui)[ok]
    return J[ok], r[ok].astype(F32), residual, assoc


def term_table(J, r):
    """The 28 columns of exact fp64 products of rule 6 -> (N, 28)."""
    J64, r64 = J.astype(np.float64), r.astype(np.float64)
    cols = [J64[:, a] * J64[:, b] for a, b in TRIU] + [J64[:, a] * r64 for a in range(6)] + [r64 * r64]
    return np.stack(cols, 1) if len(r) else np.zeros((0, 28))


def system_from_terms(table):
    """Rule 6: the 32 doubles, every sum exact and rounded once (math.fsum)."""
    out = np.zeros(32)
    out[:28] = [math.fsum(table[:, c]) for c in range(28)]
    out[28] = table.shape[0]
    return out


def sum_bound(table):
    """Rule 6's bound per sum: N 2^-52 sum |term|."""
    return table.shape[0] * 2.0 ** -52 * np.array([math.fsum(np.abs(table[:, c])) for c in range(28)])


def normal_equations(depth, k, model_depth, model_normal, k_model, T, **kw):
    J, r, _, _ = terms(depth, k, model_depth, model_normal, k_model, T, **kw)
    return system_from_terms(term_table(J, r))


# ---------------------------------------------------------------------------------------------------------
# rule 8, fp64
# ---------------------------------------------------------------------------------------------------------
def unpack(s):
    a = np.zeros((6, 6))
    for idx, (i, j) in enumerate(TRIU):
        a[i, j] = a[j, i] = s[idx]
    return a, np.array(s[21:27]), float(s[27]), int(s[28])


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def exp_se3(xi):
    """Closed form: R = I + sin(th)/th K + (1 - cos th)/th^2 K^2, V = I + (1 - cos th)/th^2 K + (th - sin th)/th^3 K^2;
    below th = 1e-8 the leading terms of the three series.  1 - cos th is formed as 2 sin^2(th / 2), which does not cancel."""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th = math.sqrt(float(w @ w))
    K = skew(w)
    if th < 1e-8:
        a, b, c = 1 - th ** 2 / 6, 0.5 - th ** 2 / 24, 1 / 6 - th ** 2 / 120
    else:
        a, b, c = math.sin(th) / th, 2 * math.sin(th / 2) ** 2 / th ** 2, (th - math.sin(th)) / th ** 3
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    m[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return m


def exp_series(xi, nterms=30):
    """The matrix exponential of the 4x4 twist matrix by its power series (the check of exp_se3)."""
    m = np.zeros((4, 4))
    m[:3, :3], m[:3, 3] = skew(xi[:3]), xi[3:]
    out, p = np.eye(4), np.eye(4)
    for n in range(1, nterms):
        p = p @ m / n
        out = out + p
    return out


def step(s, min_pairs=64):
    """-> xi, or None when the system is too small or not positive definite."""
    a, g, _, n = unpack(s)
    if n < min_pairs or not np.isfinite(s).all():
        return None
    try:
        low = np.linalg.cholesky(a)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(low.T, np.linalg.solve(low, -g))


# ---------------------------------------------------------------------------------------------------------
# rules 9 and 10
# ---------------------------------------------------------------------------------------------------------
def halve(depth, k, delta=0.05):
    """Rule 9 for one frame (h, w) -> ((h // 2, w // 2) fp32, level intrinsics fp32)."""
    d = np.asarray(depth, F32)
    h2, w2 = d.shape[0] // 2, d.shape[1] // 2
    v = [d[0:2 * h2:2, 0:2 * w2:2], d[0:2 * h2:2, 1:2 * w2:2], d[1:2 * h2:2, 0:2 * w2:2], d[1:2 * h2:2, 1:2 * w2:2]]
    fin = [np.isfinite(x) for x in v]
    c = np.full((h2, w2), np.inf, F32)
    for x, f in zip(v, fin):
        c = np.where(f & (x < c), x, c)
    s, n = np.zeros((h2, w2), F32), np.zeros((h2, w2), F32)
    with np.errstate(all='ignore'):
        for x, f in zip(v, fin):
            take = f & (x - c <= F32(delta))
            s = np.where(take, s + x, s).astype(F32)
            n = n + take.astype(F32)
        out = np.where(n > 0, s / n, NINF).astype(F32)
    k64 = np.asarray(k, F32).astype(np.float64)
    return out, np.array([k64[0] / 2, k64[1] / 2, (k64[2] - 0.5) / 2, (k64[3] - 0.5) / 2]).astype(F32)


def depth_normals(depth, k, delta=0.05):
    """Rule 10 for one frame -> (h, w, 3) fp32, NaN = none."""
    d = np.asarray(depth, F32)
    h, w = d.shape
    out = np.full((h, w, 3), np.nan, F32)
    if h < 3 or w < 3:
        return out
    with np.errstate(all='ignore'):
        p = backproject(d, k)
        ctr = (slice(1, h - 1), slice(1, w - 1))
        right, left = (slice(1, h - 1), slice(2, w)), (slice(1, h - 1), slice(0, w - 2))
        down, up = (slice(2, h), slice(1, w - 1)), (slice(0, h - 2), slice(1, w - 1))
        ok = np.isfinite(d[ctr])
        for nb in (right, left, down, up):
            ok &= np.isfinite(d[nb]) & (np.abs(d[nb] - d[ctr]) <= F32(delta))
        a = [c[right] - c[left] for c in p]
        b = [c[down] - c[up] for c in p]
        n = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).astype(F32)
        ok &= (length > 0) & np.isfinite(length)
        unit = np.stack([c / length for c in n], -1).astype(F32)
    inner = out[1:h - 1, 1:w - 1]
    inner[ok] = unit[ok]
    return out


# ---------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------
class Result(object):
    def __init__(self, pose, ok, pairs, rmse, history):
        self.pose, self.ok, self.pairs, self.rmse, self.history = pose, ok, pairs, rmse, tuple(history)
        self.iterations = len(self.history)


def cast_grid(grid, k, pose, hw):
    """Depth and normals of a fusion_ref.Grid (sdf in metres, band 3 voxels as one fp32 product) for one camera."""
    vs = F32(grid.vs)
    depth, normal = C.cast(np.asarray(grid.sdf, F32), grid.w2g, vs, np.asarray(k, F32)[None], np.asarray(pose)[None], hw,
                           F32(3.0) * vs, normals=True)
    return depth[0], normal[0]


def align(depth, k, model_pose, guess_pose, grid, iterations=(10, 5, 4), max_dist=0.1, max_angle_deg=20.0,
          min_pairs=64, delta=0.05, angle_gate=True):
    model_pose, guess_pose = np.asarray(model_pose, np.float64), np.asarray(guess_pose, np.float64)
    d, ks = [np.asarray(depth, F32)], [np.asarray(k, F32)]
    deltas = [F32(delta) * F32(2 ** lv) for lv in range(len(iterations))]         # exact: a power of two
    for lv in range(len(iterations) - 1):
        half, kh = halve(d[-1], ks[-1], deltas[lv])
        d.append(half)
        ks.append(kh)
    live_n = [depth_normals(dl, kl, dv) if angle_gate else None for dl, kl, dv in zip(d, ks, deltas)]
    model = [cast_grid(grid, kl, model_pose, dl.shape) for dl, kl in zip(d, ks)]
    with np.errstate(all='ignore'):
        T = pair_matrix(model_pose, guess_pose) if np.isfinite(model_pose).all() else np.full((4, 4), np.nan)
    history, rmse, n = [], float('nan'), 0
    for lv in range(len(iterations) - 1, -1, -1):
        for _ in range(iterations[lv]):
            s = normal_equations(d[lv], ks[lv], model[lv][0], model[lv][1], ks[lv], T, max_dist=max_dist,
                                 max_angle_deg=max_angle_deg, live_normal=live_n[lv])
            n = int(s[28])
            history.append(n)
            xi = step(s, min_pairs)
            if xi is None:
                return Result(guess_pose.copy(), False, n, float('nan'), history)
            rmse = math.sqrt(s[27] / n)
            T = exp_se3(xi) @ T
    return Result(model_pose @ T, True, n, rmse, history)


def track_sequence(grid, depth, k, first_pose, integrate=True, **kw):
    pose = np.asarray(first_pose, np.float64).copy()
    poses, results = [], []
    for f in range(len(depth)):
        if f == 0:
            res = Result(pose.copy(), True, 0, 0.0, [])
        else:
            res = align(depth[f], k[f], pose, pose, grid, **kw)
        results.append(res)
        poses.append(res.pose)
        if res.ok:
            pose = res.pose
            if integrate:
                grid.integrate(depth[f:f + 1], k[f:f + 1], pose[None])
    return np.stack(poses), results


# ---------------------------------------------------------------------------------------------------------
# pose errors and perturbations (tests)
# ---------------------------------------------------------------------------------------------------------
def pose_error(a, b):
    """(translation error in metres, rotation error in degrees) between two cam2world matrices."""
    rel = np.linalg.inv(a) @ b
    cosv = (np.trace(rel[:3, :3]) - 1) / 2
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0))))


def perturbed(pose, seed, trans=0.03, rot_deg=1.5):
    """pose moved by `trans` metres along a seeded random direction and turned by rot_deg about a seeded random axis
    through the camera centre."""
    rng = np.random.default_rng(1000 + seed)
    axis, direction = rng.normal(size=3), rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction /= np.linalg.norm(direction)
    delta = exp_se3(np.concatenate([axis * np.radians(rot_deg), np.zeros(3)]))
    out = np.asarray(pose, np.float64) @ delta
    out[:3, 3] = pose[:3, 3] + trans * direction
    return out


def sequence_poses(n, seed=0, step=0.02):
    """n poses of a hand-held sweep inside the room of fusion_ref: the eye moves `step` radians per frame along the
    circle of fusion_ref.room_trajectory (1.8 cm and 1.1 degrees a frame) with a slow bob, looking outwards and down."""
    rng = np.random.default_rng(seed)
    a0, c = rng.uniform(0, 2 * np.pi), np.array([2.0, 1.6, 1.2])
    poses = []
    for i in range(n):
        a = a0 + step * i
        eye = c + np.array([0.9 * np.cos(a), 0.9 * np.sin(a), 0.05 * np.sin(0.5 * i)])
        poses.append(R.look_at(eye, eye + np.array([np.cos(a + 0.6), np.sin(a + 0.6), -0.3])))
    return np.stack(poses)


def sequence_frames(n, hw, seed=0):
    """(depth (n, h, w) fp32, intrinsics (n, 4) fp32, poses (n, 4, 4)) of sequence_poses in the analytic room."""
    _, k, _ = R.room_frames(1, hw)
    poses = sequence_poses(n, seed)
    depth = np.stack([R.render(k[0], p, hw, R.ROOM_PLANES, R.ROOM_BOXES) for p in poses])
    return depth, np.tile(k[0], (n, 1)), poses


def room_volume(vs=0.05):
    """The analytic room of raycast_ref.room_sdf as a fusion_ref.Grid."""
    dims, _, w2g = C.room_grid(vs, 4)
    grid = R.Grid(dims, vs, w2g)
    grid.sdf = C.room_sdf(vs, 4)[0]
    return grid


def conditioning(depth, k, pose, grid):
    """Largest over smallest eigenvalue of the finest-level 6x6 matrix at the true pose: how well a view constrains all
    six degrees of freedom (a single plane leaves three free and gives 1e16 or a negative number)."""
    md, mn = cast_grid(grid, k, pose, depth.shape)
    s = normal_equations(depth, k, md, mn, k, np.eye(4), live_normal=depth_normals(depth, k))
    ev = np.linalg.eigvalsh(unpack(s)[0])
    return float(ev[-1] / ev[0]) if ev[0] > 0 else float('inf')


MAX_CONDITION = 200.0


def test_view(seed, hw, grid):
    """The first frame of fusion_ref.room_frames(6, hw, seed) whose view constrains the pose: conditioning() below
    MAX_CONDITION.  Half of the room's views show one wall or a wall and the floor, which no ICP can track.
    -> (depth, k, pose, frame index, condition number)."""
    depth, k, poses = R.room_frames(6, hw, seed=seed)
    for f in range(len(depth)):
        c = conditioning(depth[f], k[f], poses[f], grid)
        if c < MAX_CONDITION:
            return depth[f], k[f], poses[f], f, c
    raise AssertionError('no usable view for seed %d' % seed)


SEQUENCE_SEED = 1      # sequence_frames(6, (48, 64), 1): conditioning() of frame 0 is 165; seed 0 looks at a wall (15867)


# The accuracy the rules reach on the CPU: measured and pinned by tests/test_track_ref.py, quoted in INTEGRATION.md
# section I, asserted at 1.5x on the device by tests/test_gpu_track.py.
TRANS, ROT = 0.03, 1.5                  # the perturbation of the guesses: 3 cm and 1.5 degrees
ALIGN_ERROR = (0.000839, 0.02416)       # worst final error over seeds 0-3: metres, degrees
SEQUENCE_DRIFT = (0.002969, 0.03876)    # frame 5 of the six-frame sequence against the true trajectory
