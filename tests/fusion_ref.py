"""Independent NumPy restatement of the TSDF fusion rules (INTEGRATION.md "TSDF fusion"; the reference's
datagen/GenerateScans Scene.cpp:167-200, CameraUtil.h:25-63, VoxelGrid.cpp:6-63, VoxelGrid.h:120-216,350-400).

Nothing here imports sgnn_amd.fusion: the frustum box, the voxel->camera matrix and the OBB test have their own
code.  `integrate(..., dtype=np.float32)` follows the operation order the kernel documents, one rounding per
operation, so the device result must match it bit for bit; dtype=np.float64 gives the physical answer for the
analytic checks.  The scene renderer at the bottom casts rays against axis-aligned boxes and planes in fp64.
"""
import numpy as np

F32 = np.float32


def round_away(x):
    """Round half away from zero in x's precision (C's round)."""
    a = np.abs(x)
    f = np.floor(a)
    r = f + (a - f >= 0.5).astype(a.dtype)          # a - f is exact
    return np.copysign(r, x)


# ---------------------------------------------------------------------------------------------------------
# 1. raw depth
# ---------------------------------------------------------------------------------------------------------
def raw_to_metric(raw, depth_shift, out_hw, min_depth=0.1, max_depth=12.0):
    raw = np.asarray(raw, dtype=np.uint16)
    single = raw.ndim == 2
    raw = raw[None] if single else raw
    _, hr, wr = raw.shape
    h, w = out_hw
    xs = round_away(np.arange(w, dtype=F32) * (F32(wr - 1) / F32(w - 1))).astype(np.int64)
    ys = round_away(np.arange(h, dtype=F32) * (F32(hr - 1) / F32(h - 1))).astype(np.int64)
    d = raw[:, ys][:, :, xs]
    fd = (F32(1.0) / F32(depth_shift)) * d.astype(F32)
    out = np.where((d == 0) | (fd < F32(min_depth)) | (fd > F32(max_depth)), F32(-np.inf), fd).astype(F32)
    return out[0] if single else out


def adapt_intrinsics(k, raw_hw, out_hw):
    k = np.array(k, dtype=F32)
    (hr, wr), (h, w) = raw_hw, out_hw
    k[..., 0] = k[..., 0] * (F32(w) / F32(wr))
    k[..., 1] = k[..., 1] * (F32(h) / F32(hr))
    k[..., 2] = k[..., 2] * (F32(w - 1) / F32(wr - 1))
    k[..., 3] = k[..., 3] * (F32(h - 1) / F32(hr - 1))
    return k


# ---------------------------------------------------------------------------------------------------------
# 2. bilateral filter, fp64
# ---------------------------------------------------------------------------------------------------------
def bilateral64(depth, sigma_d=2.0, sigma_r=0.1):
    d = np.asarray(depth, dtype=np.float64)
    single = d.ndim == 2
    d = d[None] if single else d
    nf, h, w = d.shape
    rad = int(np.ceil(2.0 * sigma_d))
    valid = np.isfinite(d)
    num = np.zeros_like(d)
    den = np.zeros_like(d)
    c = np.where(valid, d, 0.0)
    for oy in range(-rad, rad + 1):
        for ox in range(-rad, rad + 1):
            nb = np.full_like(d, np.nan)
            ys0, ys1 = max(0, -oy), min(h, h - oy)
            xs0, xs1 = max(0, -ox), min(w, w - ox)
            nb[:, ys0:ys1, xs0:xs1] = d[:, ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
            ok = np.isfinite(nb)
            nbv = np.where(ok, nb, 0.0)
            wt = np.exp(-(ox * ox + oy * oy) / (2.0 * sigma_d * sigma_d)) * \
                np.exp(-(nbv - c) ** 2 / (2.0 * sigma_r * sigma_r))
            wt = np.where(ok, wt, 0.0)
            num += wt * nbv
            den += wt
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.where(valid & (den > 0), num / den, -np.inf)
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------
# 3. integration
# ---------------------------------------------------------------------------------------------------------
def voxel_to_camera(cam2world, world2grid):
    """inv(cam2world) @ inv(world2grid) in fp64 -> fp32 rows 0..2."""
    m = np.linalg.inv(np.asarray(cam2world, np.float64)) @ np.linalg.inv(np.asarray(world2grid, np.float64))
    return m[:3].astype(F32)


def _apply(m, p, dt):
    out = []
    for r in range(3):
        acc = m[r, 0] * p[..., 0]
        acc = acc + m[r, 1] * p[..., 1]
        acc = acc + m[r, 2] * p[..., 2]
        out.append((acc + m[r, 3]).astype(dt))
    return np.stack(out, -1)


def frame_box(k, cam2world, hw, world2grid, dims_xyz, dmin=0.4, dmax=4.0):
    """Inclusive voxel box (x0, x1, y0, y1, z0, z1) or None."""
    c2w = np.asarray(cam2world, F32)
    if not np.isfinite(c2w).all():
        return None
    w2g = np.asarray(world2grid, F32)
    fx, fy, cx, cy = (F32(v) for v in k)
    h, w = hw
    corners = []
    for dep in (F32(dmin), F32(dmax)):
        for ux, uy in ((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)):
            corners.append((dep * ((F32(ux) - cx) / fx), dep * ((F32(uy) - cy) / fy), dep))
    wp = _apply(c2w, np.array(corners, F32), F32)
    g = round_away(_apply(w2g, np.concatenate([np.floor(wp), np.ceil(wp)]), F32))
    lo = np.maximum(g.min(0), 0).astype(np.int64)
    hi = np.minimum(g.max(0), np.array(dims_xyz) - 1).astype(np.int64)
    if (lo > hi).any():
        return None
    return np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]])


def in_obb(obb, q):
    o = np.asarray(obb, F32).reshape(4, 3)
    r = q.astype(F32) - o[0]
    ok = np.ones(q.shape[0], bool)
    for k in range(3):
        e = o[1 + k]
        dd = r[:, 0] * e[0]
        dd = dd + r[:, 1] * e[1]
        dd = dd + r[:, 2] * e[2]
        ee = e[0] * e[0]
        ee = ee + e[1] * e[1]
        ee = ee + e[2] * e[2]
        ok &= (dd >= 0) & (dd <= ee)
    return ok


class Grid(object):
    def __init__(self, dims_xyz, voxel_size, world2grid, dmin=0.4, dmax=4.0, obb=None, dtype=F32):
        dx, dy, dz = dims_xyz
        self.dims, self.dt = tuple(dims_xyz), dtype
        self.vs, self.w2g, self.dmin, self.dmax, self.obb = dtype(voxel_size), np.asarray(world2grid), dmin, dmax, obb
        self.sdf = np.full((dz, dy, dx), -np.inf, dtype)
        self.weight = np.zeros((dz, dy, dx), np.int64)
        self.free = np.zeros((dz, dy, dx), np.int64)
        self.behind_updates = 0

    def integrate(self, depth, intr, c2w):
        dt = self.dt
        depth = np.asarray(depth, dt)
        h, w = depth.shape[1:]
        for f in range(depth.shape[0]):
            box = frame_box(intr[f], c2w[f], (h, w), self.w2g, self.dims, self.dmin, self.dmax)
            if box is None:
                continue
            zz, yy, xx = np.meshgrid(np.arange(box[4], box[5] + 1), np.arange(box[2], box[3] + 1),
                                     np.arange(box[0], box[1] + 1), indexing='ij')
            q = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)
            if self.obb is not None:
                q = q[in_obb(self.obb, q)]
            if dt == F32:
                m = voxel_to_camera(c2w[f], self.w2g)
            else:
                m = (np.linalg.inv(np.asarray(c2w[f], np.float64)) @ np.linalg.inv(np.asarray(self.w2g, np.float64)))[:3]
            pf = _apply(m.astype(dt), q.astype(dt), dt)
            fx, fy, cx, cy = (dt(v) for v in intr[f])
            with np.errstate(all='ignore'):
                px = round_away((pf[:, 0] * fx) / pf[:, 2] + cx)
                py = round_away((pf[:, 1] * fy) / pf[:, 2] + cy)
            on = (px >= 0) & (px < w) & (py >= 0) & (py < h)       # NaN compares false
            q, pf, px, py = q[on], pf[on], px[on].astype(np.int64), py[on].astype(np.int64)
            d = depth[f, py, px]
            ok = np.isfinite(d) & (d >= dt(self.dmin)) & (d <= dt(self.dmax))
            q, pz, d = q[ok], pf[ok, 2], d[ok]
            iz, iy, ix = q[:, 2], q[:, 1], q[:, 0]
            self.free[iz, iy, ix] += (pz < d)
            sd = (d - pz).astype(dt)
            tr = (self.vs * dt(3.0) + d * self.vs).astype(dt)
            up = sd > -tr
            iz, iy, ix, sd, tr, d, pz = iz[up], iy[up], ix[up], sd[up], tr[up], d[up], pz[up]
            self.behind_updates += int((pz < 0).sum())
            sd = np.where(sd >= 0, np.minimum(tr, sd), np.maximum(-tr, sd)).astype(dt)
            z01 = ((d - dt(0.4)) / (dt(4.0) - dt(0.4))).astype(dt)
            wu = np.maximum(dt(4.5) * (dt(1.0) - z01), dt(1.0)).astype(dt)
            old = self.sdf[iz, iy, ix]
            ow = self.weight[iz, iy, ix].astype(dt)
            with np.errstate(invalid='ignore'):                    # the unselected branch of a first sample
                new = np.where(old == -np.inf, sd, (old * ow + sd * wu) / (ow + wu)).astype(dt)
            self.sdf[iz, iy, ix] = new
            self.weight[iz, iy, ix] = np.minimum(self.weight[iz, iy, ix] + wu.astype(np.int64), 255)
        return self

    # 4. sparse export
    def sparse(self, factor=6.0):
        keep = np.abs(self.sdf) <= F32(factor) * F32(self.vs)
        z, y, x = np.nonzero(keep)                                     # raster order, x fastest
        return np.stack([x, y, z], 1).astype(np.uint32), self.sdf[z, y, x].astype(F32)

    # 5. known codes
    def known(self):
        s, vs = self.sdf.astype(F32), F32(self.vs)
        out = np.zeros(s.shape, np.uint8)
        with np.errstate(all='ignore'):
            q = -s / vs
            code = np.clip(np.where(np.isfinite(q), q, 0).astype(np.int64) + 1, 2, 255)
        code = np.where(np.isfinite(q), code, 2)                     # -inf: x86's (int)inf = INT_MIN -> 2
        out[s < -vs] = code[s < -vs]
        out[(s >= -vs) & (s <= vs)] = 1
        return out


# ---------------------------------------------------------------------------------------------------------
# analytic scenes
# ---------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam2world of a camera at eye looking at target: camera x right, y down, z forward."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-9:
        right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, eye
    return m


def render(k, cam2world, hw, planes=(), boxes=()):
    """z-depth (fp64 rays, rounded to fp32) of planes (n, c: n.x = c) and axis-aligned boxes (lo, hi); -inf = miss."""
    h, w = hw
    fx, fy, cx, cy = (float(v) for v in k)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c2w = np.asarray(cam2world, np.float64)
    dw = dirs @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = np.full((h, w), np.inf)
    with np.errstate(all='ignore'):
        for n, c in planes:
            n = np.asarray(n, np.float64)
            tt = (c - n @ o) / (dw @ n)
            t = np.where((tt > 0) & (tt < t), tt, t)
        for lo, hi in boxes:
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            t0 = (lo - o) / dw
            t1 = (hi - o) / dw
            tn = np.minimum(t0, t1).max(-1)
            tf = np.maximum(t0, t1).min(-1)
            hit = (tf >= tn) & (tn > 0)
            t = np.where(hit & (tn < t), tn, t)
    return np.where(np.isfinite(t), t, -np.inf).astype(F32)


ROOM_PLANES = [((0, 0, 1), 0.0), ((0, 0, -1), -2.6), ((1, 0, 0), 0.0), ((-1, 0, 0), -4.0), ((0, 1, 0), 0.0),
               ((0, -1, 0), -3.2)]
ROOM_BOXES = [((1.0, 1.0, 0.0), (1.8, 1.6, 0.75)), ((2.6, 0.3, 0.0), (3.4, 0.9, 1.1)), ((0.4, 2.2, 0.0),
                                                                                           (1.2, 2.9, 0.45))]


def room_trajectory(n, seed=0, centre=(2.0, 1.6, 1.2), radius=0.9):
    """n poses on a wobbly circle inside ROOM_PLANES, looking outwards and down a little."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    poses = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1) + rng.uniform(-0.1, 0.1)
        eye = c + np.array([radius * np.cos(a), radius * np.sin(a), rng.uniform(-0.15, 0.15)])
        tgt = eye + np.array([np.cos(a + 0.6), np.sin(a + 0.6), rng.uniform(-0.5, -0.1)])
        poses.append(look_at(eye, tgt))
    return np.stack(poses)


def room_frames(n, hw, seed=0, k=None):
    """(depth (n,h,w) f32, intrinsics (n,4) f32, cam2world (n,4,4) f64) of the analytic room."""
    h, w = hw
    if k is None:
        k = np.array([0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0], F32)
    poses = room_trajectory(n, seed)
    depth = np.stack([render(k, p, hw, ROOM_PLANES, ROOM_BOXES) for p in poses])
    return depth, np.tile(np.asarray(k, F32), (n, 1)), poses


def grid_transform(origin, voxel_size):
    """world2grid = scale(1/vs) . translate(-origin), fp32 (Fuser.cpp:58)."""
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] /= voxel_size
    m[:3, 3] = -np.asarray(origin, np.float64) / voxel_size
    return m.astype(F32)
