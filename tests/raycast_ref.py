"""Independent NumPy restatement of the TSDF ray-casting rules (rules 1-6).

Nothing here imports sgnn_amd.raycast.  Everything is fp32 with one rounding per operation in the evaluation orders
the rules give, vectorised over the pixels of a frame with a plain loop over the samples k, and there is no
skipping: every sample of every ray goes through rule 4.  The device result must match it bit for bit.

room_sdf() is the analytic volume of the tests: the signed distance to the room of fusion_ref (ROOM_PLANES,
ROOM_BOXES), positive in free space.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_ref as R  # noqa: E402

F32 = np.float32
NINF = F32(-np.inf)


# ---------------------------------------------------------------------------------------------------------
# the analytic room as a volume
# ---------------------------------------------------------------------------------------------------------
def _box_sd(p, lo, hi):
    """Signed distance (fp64) of points p (.., 3) to the solid box [lo, hi]: negative inside."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    q = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def room_extent():
    """(lo, hi) of the room's interior, from the six planes n.x = c with axis-aligned inward normals."""
    lo, hi = np.zeros(3), np.zeros(3)
    for n, c in R.ROOM_PLANES:
        a = int(np.argmax(np.abs(n)))
        if n[a] > 0:
            lo[a] = c / n[a]
        else:
            hi[a] = c / n[a]
    return lo, hi


def room_grid(vs=0.05, pad=4):
    """(dims_xyz, origin, world2grid fp32) of the grid that covers the room with `pad` voxels around it; voxel
    (x, y, z) sits at origin + (x, y, z) * vs."""
    lo, hi = room_extent()
    dims = tuple(int(v) for v in np.rint((hi - lo) / vs).astype(np.int64) + 2 * pad)
    origin = lo - pad * vs
    return dims, origin, R.grid_transform(origin, vs)


def room_sdf(vs=0.05, pad=4, band=None):
    """The room as a (Z, Y, X) fp32 volume in metres: the signed distance to the walls and boxes, positive in free
    space (the smallest of: minus the box distance of the room's interior, the box distance of every ROOM_BOX),
    computed in fp64, rounded to fp32, -inf where |d| > band (None: 3 vs).  Returns (sdf, world2grid)."""
    band = 3 * vs if band is None else band
    (dx, dy, dz), origin, w2g = room_grid(vs, pad)
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing='ij')
    p = origin + np.stack([x, y, z], -1).astype(np.float64) * vs
    lo, hi = room_extent()
    d = -_box_sd(p, lo, hi)
    for blo, bhi in R.ROOM_BOXES:
        d = np.minimum(d, _box_sd(p, blo, bhi))
    return np.where(np.abs(d) > band, -np.inf, d).astype(F32), w2g


# ---------------------------------------------------------------------------------------------------------
# rules 1-6
# ---------------------------------------------------------------------------------------------------------
def frame_matrix(world2grid, cam2world):
    """Rule 1: rows 0..2 of world2grid . cam2world, fp64 product rounded to fp32; None for an empty frame."""
    c2w = np.asarray(cam2world, np.float64)
    if not np.isfinite(c2w).all():
        return None
    with np.errstate(all='ignore'):
        g = (np.asarray(world2grid, np.float64) @ c2w)[:3].astype(F32)
    return g if np.isfinite(g).all() else None


def sample_depths(depth_min, depth_max, dt):
    """Rule 3: t_k = depth_min + (float)k * dt while t_k <= depth_max."""
    dmin, dmax, dt = F32(depth_min), F32(depth_max), F32(dt)
    ts, k = [], 0
    while True:
        t = dmin + F32(k) * dt
        if not t <= dmax:
            return ts
        ts.append(t)
        k += 1


def lerp(p, q, a):
    return p + a * (q - p)


def sample(sdf, band, g):
    """Rule 4 at grid positions g (P, 3) fp32, x y z -> (valid (P,), value (P,) fp32, 0 where invalid)."""
    dz, dy, dx = sdf.shape
    with np.errstate(invalid='ignore'):
        f = np.floor(g)
        inside = np.ones(len(g), bool)
        for a, d in enumerate((dx, dy, dz)):
            inside &= (f[:, a] >= 0) & (f[:, a] <= d - 2)
    c = np.where(inside[:, None], f, 0).astype(np.int64)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    x1, y1, z1 = (np.minimum(v + 1, d - 1) for v, d in ((x, dx), (y, dy), (z, dz)))     # only read where inside
    corner = {(k, j, i): sdf[(z, z1)[k], (y, y1)[j], (x, x1)[i]] for k in (0, 1) for j in (0, 1) for i in (0, 1)}
    valid = inside.copy()
    for v in corner.values():
        with np.errstate(invalid='ignore'):
            valid &= np.isfinite(v) & (np.abs(v) < band)
    corner = {key: np.where(valid, v, F32(0)) for key, v in corner.items()}
    a = np.where(valid[:, None], g - f, F32(0)).astype(F32)
    along_x = {(k, j): lerp(corner[k, j, 0], corner[k, j, 1], a[:, 0]) for k in (0, 1) for j in (0, 1)}
    along_y = {k: lerp(along_x[k, 0], along_x[k, 1], a[:, 1]) for k in (0, 1)}
    value = lerp(along_y[0], along_y[1], a[:, 2]).astype(F32)
    return valid, value


def rays(g, k, hw):
    """Rule 2 -> (origin (3,), directions (h*w, 3)) in grid space, fp32."""
    h, w = hw
    fx, fy, cx, cy = (F32(v) for v in k)
    i, j = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    with np.errstate(all='ignore'):
        c0, c1 = ((i - cx) / fx).ravel(), ((j - cy) / fy).ravel()
        d = np.stack([(g[r, 0] * c0 + g[r, 1] * c1) + g[r, 2] for r in range(3)], -1).astype(F32)
    return g[:, 3].copy(), d


def cast_frame(sdf, band, g, k, hw, dt, ts, normals):
    h, w = hw
    n = h * w
    depth = np.full(n, NINF, F32)
    normal = np.full((n, 3), np.nan, F32)
    if g is None:
        return depth.reshape(h, w), normal.reshape(h, w, 3)
    o, d = rays(g, k, hw)
    alive = np.ones(n, bool)
    pvalid, pv = np.zeros(n, bool), np.zeros(n, F32)
    with np.errstate(all='ignore'):
        for idx, t in enumerate(ts):
            pos = (o + t * d).astype(F32)
            valid, v = sample(sdf, band, pos)
            both = alive & valid & pvalid
            hit = both & (pv > 0) & (v <= 0)
            if hit.any():
                tprev = ts[idx - 1]
                tstar = tprev + dt * (pv[hit] / (pv[hit] - v[hit]))
                depth[hit] = tstar
            alive &= ~(hit | (both & (pv < 0) & (v > 0)))
            pvalid, pv = valid, v
            if not alive.any():
                break
        if normals:
            hit = np.isfinite(depth)
            gs = (o + depth[hit, None] * d[hit]).astype(F32)
            ok = np.ones(len(gs), bool)
            grad = np.zeros((len(gs), 3), F32)
            for a in range(3):
                off = np.zeros(3, F32)
                off[a] = 0.5
                vp, plus = sample(sdf, band, gs + off)
                vm, minus = sample(sdf, band, gs - off)
                ok &= vp & vm
                grad[:, a] = plus - minus
            nc = np.stack([(g[0, c] * grad[:, 0] + g[1, c] * grad[:, 1]) + g[2, c] * grad[:, 2] for c in range(3)], -1)
            nc = nc.astype(F32)
            length = np.sqrt((nc[:, 0] * nc[:, 0] + nc[:, 1] * nc[:, 1]) + nc[:, 2] * nc[:, 2]).astype(F32)
            ok &= (length > 0) & np.isfinite(length)
            unit = (nc / length[:, None]).astype(F32)
            out = np.full((len(gs), 3), np.nan, F32)
            out[ok] = unit[ok]
            normal[hit] = out
    return depth.reshape(h, w), normal.reshape(h, w, 3)


def cast(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, step=0.5, depth_min=0.4, depth_max=4.0,
         normals=False):
    """(F, h, w) fp32 depth, -inf = no hit; with normals also (F, h, w, 3) fp32 camera-space normals."""
    sdf = np.ascontiguousarray(sdf, F32)
    band = F32(band)
    dt = F32(step) * F32(voxel_size)
    ts = sample_depths(depth_min, depth_max, dt)
    intr = np.asarray(intrinsics, F32).reshape(-1, 4)
    poses = np.asarray(cam2world, np.float64).reshape(-1, 4, 4)
    assert len(intr) == len(poses)
    frames = [cast_frame(sdf, band, frame_matrix(world2grid, p), k, hw, dt, ts, normals) for k, p in zip(intr, poses)]
    depth = np.stack([f[0] for f in frames]) if frames else np.zeros((0,) + tuple(hw), F32)
    if not normals:
        return depth
    return depth, (np.stack([f[1] for f in frames]) if frames else np.zeros((0,) + tuple(hw) + (3,), F32))
