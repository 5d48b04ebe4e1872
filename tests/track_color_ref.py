"""Independent NumPy restatement of tracking with colour (rules T1-T6), on the helpers of
tests/track_ref.py, tests/fusion_color_ref.py and tests/raycast_color_ref.py.  Nothing here imports sgnn_amd.track.

Rules T1-T4 are fp32 with one rounding per operation in the evaluation orders the rules give, vectorised over the pixels
of a frame; the sums of T5 are track_ref's (math.fsum over exact fp64 products); T6 is fp64.  align_color() and
track_sequence() run the whole loop on the CPU with fusion_color_ref.ColorGrid as the volume and
raycast_color_ref.cast_color as the caster.  The device must match intensities, residuals and cells bit for bit, and
the sums within rule 6's bound.

The textured wall at the end is the scene colour is for: one plane fills every view, so the geometry leaves the two
translations along the wall and the rotation about its normal open, and only the texture holds them.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_color_ref as FC  # noqa: E402
import fusion_ref as R  # noqa: E402
import raycast_color_ref as CC  # noqa: E402
import raycast_ref as C  # noqa: E402
import track_ref as T  # noqa: E402

F32 = np.float32
COLOR_WEIGHT = 1e-3        # lambda of rule T6, the default: one grey level counts like 1 mm
MAX_INTENSITY = 40.0       # the default gate on |r|, grey levels


# ---------------------------------------------------------------------------------------------------------
# rules T1 and T2
# ---------------------------------------------------------------------------------------------------------
def intensity(rgba):
    """T1: (.., 4) uint8 -> (..) fp32, NaN where A == 0."""
    c = np.asarray(rgba, np.uint8).astype(np.int64)
    y = 77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]
    return np.where(c[..., 3] == 0, F32(np.nan), y.astype(F32) / F32(256)).astype(F32)


def halve_intensity(depth, inten, delta=0.05):
    """T2 for one frame: (h, w) depth and intensity -> (h // 2, w // 2) fp32, NaN = none."""
    d, c = np.asarray(depth, F32), np.asarray(inten, F32)
    h2, w2 = d.shape[0] // 2, d.shape[1] // 2
    block = [(slice(0, 2 * h2, 2), slice(0, 2 * w2, 2)), (slice(0, 2 * h2, 2), slice(1, 2 * w2, 2)),
             (slice(1, 2 * h2, 2), slice(0, 2 * w2, 2)), (slice(1, 2 * h2, 2), slice(1, 2 * w2, 2))]     # raster order
    v, y = [d[b] for b in block], [c[b] for b in block]
    fin = [np.isfinite(x) for x in v]
    low = np.full((h2, w2), np.inf, F32)
    for x, f in zip(v, fin):
        low = np.where(f & (x < low), x, low)
    s, n = np.zeros((h2, w2), F32), np.zeros((h2, w2), F32)
    with np.errstate(all='ignore'):
        for x, f, yy in zip(v, fin, y):
            take = f & (x - low <= F32(delta)) & ~np.isnan(yy)
            s = np.where(take, s + yy, s).astype(F32)
            n = n + take.astype(F32)
        return np.where(n > 0, s / n, F32(np.nan)).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# rules T3-T5
# ---------------------------------------------------------------------------------------------------------
def color_terms(depth, inten, k, model_depth, model_normal, model_inten, k_model, Tm, max_dist=0.1, max_angle_deg=20.0,
                max_intensity=MAX_INTENSITY, live_normal=None):
    """T3 and T4 for one pair -> (J (N, 6) fp32, r (N,) fp32, residual (h, w) fp32, cell (h, w) int32)."""
    d, il = np.asarray(depth, F32), np.asarray(inten, F32)
    md, mi = np.asarray(model_depth, F32), np.asarray(model_inten, F32)
    h, w = d.shape
    hm, wm = md.shape
    residual, cell = np.full((h, w), np.nan, F32), np.full((h, w), -1, np.int32)
    t = T.rows32(Tm)
    if t is None:
        return np.zeros((0, 6), F32), np.zeros(0, F32), residual, cell
    # "passes rules 2-4 of section I": the pixels track_ref associates
    ok = T.terms(d, k, md, model_normal, k_model, Tm, max_dist=max_dist, max_angle_deg=max_angle_deg,
                 live_normal=live_normal)[3] >= 0
    fxm, fym, cxm, cym = (F32(v) for v in k_model)
    with np.errstate(all='ignore'):
        px, py, pz = T.backproject(d, k)
        q = [((t[r, 0] * px + t[r, 1] * py) + t[r, 2] * pz) + t[r, 3] for r in range(3)]
        ok = ok & ~np.isnan(il)
        x = (q[0] * fxm) / q[2] + cxm
        y = (q[1] * fym) / q[2] + cym
        x0, y0 = np.floor(x), np.floor(y)
        a, b = x - x0, y - y0
        ok &= (x0 >= 0) & (x0 + F32(1) < F32(wm)) & (y0 >= 0) & (y0 + F32(1) < F32(hm))       # a NaN fails
        xi, yi = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
        xj, yj = np.minimum(xi + 1, wm - 1), np.minimum(yi + 1, hm - 1)                       # read where ok
        corner = {}
        for name, (cy_, cx_) in (('00', (yi, xi)), ('10', (yi, xj)), ('01', (yj, xi)), ('11', (yj, xj))):   # (x, y)
            ik, dk = mi[cy_, cx_], md[cy_, cx_]
            ok &= ~np.isnan(ik) & np.isfinite(dk) & (np.abs(dk - q[2]) <= F32(max_dist))
            corner[name] = ik
        i00, i10, i01, i11 = corner['00'], corner['10'], corner['01'], corner['11']
        oma, omb = F32(1) - a, F32(1) - b
        im = (i00 * oma + i10 * a) * omb + (i01 * oma + i11 * a) * b
        gx = (i10 - i00) * omb + (i11 - i01) * b
        gy = (i01 - i00) * oma + (i11 - i10) * a
        r = im - il
        ok &= np.abs(r) <= F32(max_intensity)
        kx, ky = (gx * fxm) / q[2], (gy * fym) / q[2]
        kz = -((kx * q[0] + ky * q[1]) / q[2])
        J = np.stack([q[1] * kz - q[2] * ky, q[2] * kx - q[0] * kz, q[0] * ky - q[1] * kx, kx, ky, kz], -1).astype(F32)
    residual[ok] = r[ok]
    cell[ok] = (yi * wm + xi)[ok]
    return J[ok], r[ok].astype(F32), residual, cell


def color_equations(depth, inten, k, model_depth, model_normal, model_inten, k_model, Tm, **kw):
    J, r, _, _ = color_terms(depth, inten, k, model_depth, model_normal, model_inten, k_model, Tm, **kw)
    return T.system_from_terms(T.term_table(J, r))


# ---------------------------------------------------------------------------------------------------------
# rule T6 and the loop
# ---------------------------------------------------------------------------------------------------------
def combine(geo, col, color_weight=COLOR_WEIGHT):
    """T6: entries 0..27 are S_g + lambda^2 S_c with lambda^2 formed once in fp64; entry 28 is N_g."""
    out = np.array(geo, np.float64)
    out[:28] = geo[:28] + (float(color_weight) * float(color_weight)) * np.asarray(col, np.float64)[:28]
    return out


class ColorResult(T.Result):
    def __init__(self, pose, ok, pairs, rmse, history, color_pairs, color_rmse):
        T.Result.__init__(self, pose, ok, pairs, rmse, history)
        self.color_pairs, self.color_rmse = color_pairs, color_rmse


def grid_rgba(grid):
    """What raycast.cast_volume_color hands to the caster: colors() with A = 255 where the colour weight is positive."""
    alpha = np.where(grid.wc > 0, 255, 0).astype(np.uint8)
    return np.concatenate([grid.colors(), alpha[..., None]], -1)


def cast_grid_color(grid, k, pose, hw):
    """Depth, normals and intensity of a fusion_color_ref.ColorGrid for one camera (band: 3 voxels, one fp32 product)."""
    vs = F32(grid.vs)
    depth, normal, rgba = CC.cast_color(np.asarray(grid.sdf, F32), grid_rgba(grid), grid.w2g, vs, np.asarray(k, F32)[None],
                                        np.asarray(pose)[None], hw, F32(3.0) * vs, normals=True)
    return depth[0], normal[0], intensity(rgba[0])


def pyramid(depth, inten, k, levels, delta):
    d, c, ks = [np.asarray(depth, F32)], [np.asarray(inten, F32)], [np.asarray(k, F32)]
    deltas = [F32(delta) * F32(2 ** lv) for lv in range(levels)]
    for lv in range(levels - 1):
        c.append(halve_intensity(d[-1], c[-1], deltas[lv]))
        half, kh = T.halve(d[-1], ks[-1], deltas[lv])
        d.append(half)
        ks.append(kh)
    return d, c, ks, deltas


def align_color(depth, rgba, k, model_pose, guess_pose, grid, color_weight=COLOR_WEIGHT, max_intensity=MAX_INTENSITY,
                iterations=(10, 5, 4), max_dist=0.1, max_angle_deg=20.0, min_pairs=64, delta=0.05, angle_gate=True):
    model_pose, guess_pose = np.asarray(model_pose, np.float64), np.asarray(guess_pose, np.float64)
    d, c, ks, deltas = pyramid(depth, intensity(rgba), k, len(iterations), delta)
    live_n = [T.depth_normals(dl, kl, dv) if angle_gate else None for dl, kl, dv in zip(d, ks, deltas)]
    model = [cast_grid_color(grid, kl, model_pose, dl.shape) for dl, kl in zip(d, ks)]
    with np.errstate(all='ignore'):
        Tm = T.pair_matrix(model_pose, guess_pose) if np.isfinite(model_pose).all() else np.full((4, 4), np.nan)
    history, rmse, n, nc, crmse = [], float('nan'), 0, 0, float('nan')
    for lv in range(len(iterations) - 1, -1, -1):
        md, mn, mc = model[lv]
        for _ in range(iterations[lv]):
            gates = dict(max_dist=max_dist, max_angle_deg=max_angle_deg, live_normal=live_n[lv])
            sg = T.normal_equations(d[lv], ks[lv], md, mn, ks[lv], Tm, **gates)
            sc = color_equations(d[lv], c[lv], ks[lv], md, mn, mc, ks[lv], Tm, max_intensity=max_intensity, **gates)
            n, nc = int(sg[28]), int(sc[28])
            history.append(n)
            xi = T.step(combine(sg, sc, color_weight), min_pairs)
            if xi is None:
                return ColorResult(guess_pose.copy(), False, n, float('nan'), history, nc, float('nan'))
            rmse, crmse = math.sqrt(sg[27] / n), (math.sqrt(sc[27] / nc) if nc else float('nan'))
            Tm = T.exp_se3(xi) @ Tm
    return ColorResult(model_pose @ Tm, True, n, rmse, history, nc, crmse)


def track_sequence(grid, depth, rgba, k, first_pose, **kw):
    """track_ref.track_sequence with align_color and ColorGrid.integrate(.., rgba); frame 0 is fused with its colour."""
    pose = np.asarray(first_pose, np.float64).copy()
    poses, results = [], []
    for f in range(len(depth)):
        res = ColorResult(pose.copy(), True, 0, 0.0, [], 0, 0.0) if f == 0 else \
            align_color(depth[f], rgba[f], k[f], pose, pose, grid, **kw)
        results.append(res)
        poses.append(res.pose)
        if res.ok:
            pose = res.pose
            grid.integrate(depth[f:f + 1], k[f:f + 1], pose[None], rgba[f:f + 1])
    return np.stack(poses), results


def conditioning(depth, rgba, k, pose, grid, color_weight=COLOR_WEIGHT):
    """track_ref.conditioning's figure at the true pose for the geometric system and for the system of rule T6 ->
    (geometric, combined); inf for a matrix that is not positive definite."""
    md, mn, mc = cast_grid_color(grid, k, pose, depth.shape)
    ln = T.depth_normals(depth, k)
    sg = T.normal_equations(depth, k, md, mn, k, np.eye(4), live_normal=ln)
    sc = color_equations(depth, intensity(rgba), k, md, mn, mc, k, np.eye(4), live_normal=ln)
    out = []
    for s in (sg, combine(sg, sc, color_weight)):
        ev = np.linalg.eigvalsh(T.unpack(s)[0])
        out.append(float(ev[-1] / ev[0]) if ev[0] > 0 else float('inf'))
    return tuple(out)


def in_plane_error(true_pose, pose, normal):
    """Length of the translation error's component along the wall (metres)."""
    e = np.asarray(pose, np.float64)[:3, 3] - np.asarray(true_pose, np.float64)[:3, 3]
    n = np.asarray(normal, np.float64)
    return float(np.linalg.norm(e - (e @ n) * n))


# ---------------------------------------------------------------------------------------------------------
# the textured wall
# ---------------------------------------------------------------------------------------------------------
# The plane x = WALL_X seen from x < WALL_X; the wall's own coordinates are world (y, z).  Its intensity is
# WALL_MEAN + WALL_AMPLITUDE (sin(2 pi s1 / P1) + sin(2 pi s2 / P2)) with s1, s2 the coordinate along two directions
# 75 degrees apart, so the texture varies along every direction of the wall.  Limits on the periods: at least 8 voxels
# of the 5 cm volume (0.4 m), and at least 4 pixels at the coarsest pyramid level: a 48 x 64 frame has fx = 51.2, its
# level 2 has fx = 12.8, a pixel there spans 2 m / 12.8 = 0.156 m of a wall 2 m away, four of them 0.625 m.
WALL_X = 2.4
WALL_NORMAL = (-1.0, 0.0, 0.0)
WALL_VS = 0.05
WALL_DIMS = (60, 96, 80)                     # x, y, z: 3.0 x 4.8 x 4.0 m
WALL_ORIGIN = (-0.2, -2.4, -2.0)
WALL_MEAN, WALL_AMPLITUDE = 128.0, 60.0
WALL_PERIODS = (0.70, 0.90)                  # metres
WALL_DIRECTIONS = (np.radians(20.0), np.radians(95.0))
WALL_HW = (48, 64)


def wall_texture(y, z):
    """Intensity in [8, 248] at wall coordinates (fp64)."""
    out = np.full(np.shape(y), WALL_MEAN)
    for period, ang in zip(WALL_PERIODS, WALL_DIRECTIONS):
        out = out + WALL_AMPLITUDE * np.sin(2 * np.pi * (np.cos(ang) * y + np.sin(ang) * z) / period)
    return out


def wall_render(k, cam2world, hw=WALL_HW):
    """(depth (h, w) fp32, rgba (h, w, 4) uint8, R = G = B) of the wall, fp64 rays; A = 0 and -inf where a ray misses."""
    h, w = hw
    fx, fy, cx, cy = (float(v) for v in k)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c2w = np.asarray(cam2world, np.float64)
    dw, o = dirs @ c2w[:3, :3].T, c2w[:3, 3]
    with np.errstate(all='ignore'):
        t = (WALL_X - o[0]) / dw[..., 0]
    hit = np.isfinite(t) & (t > 0)
    p = o + np.where(hit, t, 0.0)[..., None] * dw
    grey = np.clip(np.rint(wall_texture(p[..., 1], p[..., 2])), 0, 255).astype(np.uint8)
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[hit] = np.stack([grey, grey, grey, np.full_like(grey, 255)], -1)[hit]
    return np.where(hit, t, -np.inf).astype(F32), rgba


def wall_intrinsics(hw=WALL_HW):
    h, w = hw
    return np.array([0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0], F32)


def wall_grid():
    """An empty ColorGrid around the wall."""
    return FC.ColorGrid(WALL_DIMS, WALL_VS, R.grid_transform(WALL_ORIGIN, WALL_VS))


def wall_volume():
    """The wall as an analytic ColorGrid: sdf = WALL_X - x in metres (fp64, rounded to fp32), -inf beyond 3 voxels;
    every voxel inside the band carries the texture at its foot point, rounded to 8 bits, with colour weight 1."""
    grid = wall_grid()
    dx, dy, dz = WALL_DIMS
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing='ij')
    p = np.asarray(WALL_ORIGIN) + np.stack([x, y, z], -1).astype(np.float64) * WALL_VS
    d = WALL_X - p[..., 0]
    band = np.abs(d) <= 3 * WALL_VS
    grid.sdf = np.where(band, d, -np.inf).astype(F32)
    grey = np.clip(np.rint(wall_texture(p[..., 1], p[..., 2])), 0, 255).astype(np.int64)
    grid.q = np.where(band[..., None], (grey * 256)[..., None], 0) * np.ones(3, np.int64)
    grid.wc = band.astype(np.int64)
    grid.weight = band.astype(np.int64)
    return grid


def wall_pose(seed):
    """A hand-held view of the wall from about 2 m: the eye near x = 0.4, looking at a seeded point of the wall, so the
    view is a few degrees off the normal and the wall fills the frame."""
    rng = np.random.default_rng(2000 + seed)
    eye = np.array([0.4 + rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
    target = np.array([WALL_X, eye[1] + rng.uniform(-0.25, 0.25), eye[2] + rng.uniform(-0.25, 0.25)])
    return R.look_at(eye, target)


def wall_view(seed, hw=WALL_HW):
    """-> (depth, rgba, k, pose) of wall_pose(seed)."""
    k, pose = wall_intrinsics(hw), wall_pose(seed)
    depth, rgba = wall_render(k, pose, hw)
    return depth, rgba, k, pose


def wall_sequence(n=6, hw=WALL_HW, step=0.02):
    """n frames of a sweep along the wall: 2 cm a frame sideways with a slow bob, turning 0.5 degrees a frame sideways
    and 1.1 degrees a frame downwards ->
    (depth (n, h, w), rgba (n, h, w, 4), k (n, 4), poses (n, 4, 4))."""
    k = wall_intrinsics(hw)
    poses = []
    for i in range(n):
        eye = np.array([0.4, -0.05 + step * i, 0.01 * math.sin(0.7 * i)])
        a = np.radians(0.5) * i
        poses.append(R.look_at(eye, eye + np.array([math.cos(a), math.sin(a), -0.02 * i])))
    frames = [wall_render(k, p, hw) for p in poses]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.tile(k, (n, 1)), np.stack(poses)


def painted_room_volume(vs=0.05):
    """track_ref.room_volume in colour: the analytic room as a ColorGrid whose voxels inside the band carry the colour
    of the nearest primitive of fusion_color_ref's painted room, with colour weight 1."""
    dims, _, w2g = C.room_grid(vs, 4)
    grid = FC.ColorGrid(dims, vs, w2g)
    grid.sdf = C.room_sdf(vs, 4)[0]
    dx, dy, dz = dims
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing='ij')
    own, _ = FC.painted_expectation(np.stack([x, y, z], -1).reshape(-1, 3), w2g, 0.0)
    band = np.isfinite(grid.sdf)
    grid.q = np.where(band[..., None], own.reshape(dz, dy, dx, 3).astype(np.int64) * 256, 0)
    grid.wc = band.astype(np.int64)
    grid.weight = band.astype(np.int64)
    return grid


# The accuracy the rules reach on the CPU: measured and pinned by tests/test_track_color_ref.py, quoted in
# INTEGRATION.md section T, asserted at 1.5x on the device by tests/test_gpu_track_color.py.
WALL_ALIGN_ERROR = (0.000143, 0.00959)     # worst final error over seeds 0-3 on the wall: metres, degrees
WALL_SEQUENCE_DRIFT = (0.001841, 0.02065)   # frame 5 of the six-frame wall sequence against the true trajectory
ROOM_ALIGN_ERROR = (0.001298, 0.2100)      # worst final error over seeds 0-3 in the painted room
