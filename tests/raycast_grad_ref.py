"""Independent NumPy restatement of the differentiable cast, built on raycast_ref.

Nothing here imports sgnn_amd.raycast.  forward() is raycast_ref's walk (no skipping) that also keeps the sample
index k of every hit, the features at the hit and ok; terms() lists, pixel by pixel, what rule 4 adds to which voxel,
in fp32 with one rounding per operation in the orders the rule gives (or, with dtype=np.float64, the same expressions
in fp64); accumulate() sums such lists per voxel in fp64 and also returns rule 5's bound; forward64() is the forward
of single pixels in fp64 with k held fixed, as a function of the voxel values, for differentiation.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as C  # noqa: E402

F32 = np.float32
NINF = F32(-np.inf)
CORNERS = [(i >> 2, (i >> 1) & 1, i & 1) for i in range(8)]          # (z, y, x) of corner i: x fastest, then y, then z


def smooth_features(shape_zyx, channels=3):
    """A smooth feature field (Z, Y, X, channels <= 5) fp32 for the tests."""
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape_zyx], indexing='ij')
    f = [np.sin(0.21 * x + 0.13 * y) + 0.02 * z, np.cos(0.17 * y - 0.11 * z) + 0.01 * x, 0.03 * z + 0.02 * x - 0.01 * y,
         np.sin(0.09 * (x + y + z)), 0.5 + 0.01 * x * np.cos(0.2 * z)]
    return np.stack(f[:channels], -1).astype(F32)


def cell(g, dims_zyx):
    """Rule 3's cell of positions g (P, 3) x y z -> (inside (P,), f (P, 3) int64 x y z, 0 where outside, a (P, 3)
    fractions in g's dtype)."""
    dz, dy, dx = dims_zyx
    with np.errstate(invalid='ignore'):
        f = np.floor(g)
        inside = np.ones(len(g), bool)
        for a, d in enumerate((dx, dy, dz)):
            inside &= (f[:, a] >= 0) & (f[:, a] <= d - 2)
    fi = np.where(inside[:, None], f, 0).astype(np.int64)
    a = np.where(inside[:, None], g - f, 0).astype(g.dtype)
    return inside, fi, a


def axis_weights(a):
    """(wx, wy, wz), each (P, 2): 1 - a and a."""
    one = a.dtype.type(1)
    return tuple(np.stack([one - a[:, c], a[:, c]], 1) for c in range(3))


def corner_weights(a):
    """(P, 8): w_i = (wz . wy) . wx in corner order."""
    wx, wy, wz = axis_weights(a)
    return np.stack([(wz[:, z] * wy[:, y]) * wx[:, x] for z, y, x in CORNERS], 1)


def corner_index(f, dims_zyx):
    """(P, 8) flat voxel indices (z, y, x order of the volume) of the corners of the cells f (P, 3) x y z."""
    dz, dy, dx = dims_zyx
    return np.stack([((f[:, 2] + z) * dy + (f[:, 1] + y)) * dx + (f[:, 0] + x) for z, y, x in CORNERS], 1)


def usable(v, band):
    with np.errstate(invalid='ignore'):
        return np.isfinite(v) & (np.abs(v) < band)


def features_at(features, inside, f, a):
    """Rule 3: the left-to-right sum of w_i . c_i over all eight corners -> (P, C), 0 where the cell test fails."""
    dims = features.shape[:3]
    flat = features.reshape(-1, features.shape[3])
    idx, w = corner_index(f, dims), corner_weights(a)
    with np.errstate(all='ignore'):
        acc = w[:, 0, None] * flat[idx[:, 0]]
        for i in range(1, 8):
            acc = acc + w[:, i, None] * flat[idx[:, i]]
    return np.where(inside[:, None], acc, 0).astype(features.dtype)


def forward_frame(sdf, band, g, k, hw, dt, ts, features):
    """One frame -> (depth (h, w), hit (h, w) int32, feat (h, w, C) or None, ok (h, w) bool)."""
    h, w = hw
    n = h * w
    depth, hitk = np.full(n, NINF, F32), np.full(n, -1, np.int32)
    ch = 0 if features is None else features.shape[3]
    feat, ok = np.zeros((n, ch), F32), np.zeros(n, bool)
    if g is not None:
        o, d = C.rays(g, k, hw)
        alive = np.ones(n, bool)
        pvalid, pv = np.zeros(n, bool), np.zeros(n, F32)
        with np.errstate(all='ignore'):
            for idx, t in enumerate(ts):                                   # raycast_ref.cast_frame's walk
                valid, v = C.sample(sdf, band, (o + t * d).astype(F32))
                both = alive & valid & pvalid
                hit = both & (pv > 0) & (v <= 0)
                if hit.any():
                    depth[hit] = ts[idx - 1] + dt * (pv[hit] / (pv[hit] - v[hit]))
                    hitk[hit] = idx
                alive &= ~(hit | (both & (pv < 0) & (v > 0)))
                pvalid, pv = valid, v
                if not alive.any():
                    break
            has = hitk >= 0
            gs = (o + np.where(has, depth, F32(0))[:, None] * d).astype(F32)
        inside, f, a = cell(gs, sdf.shape)
        inside &= has
        ok = inside & usable(sdf.reshape(-1)[corner_index(f, sdf.shape)], band).all(1)
        if features is not None:
            feat = features_at(features, inside, f, a)
    return (depth.reshape(h, w), hitk.reshape(h, w), feat.reshape(h, w, ch) if features is not None else None,
            ok.reshape(h, w))


def setup(world2grid, voxel_size, intrinsics, cam2world, step, depth_min, depth_max):
    dt = F32(step) * F32(voxel_size)
    ts = C.sample_depths(depth_min, depth_max, dt)
    intr = np.asarray(intrinsics, F32).reshape(-1, 4)
    poses = np.asarray(cam2world, np.float64).reshape(-1, 4, 4)
    assert len(intr) == len(poses)
    return dt, ts, intr, [C.frame_matrix(world2grid, p) for p in poses]


def forward(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, features=None, step=0.5, depth_min=0.4,
            depth_max=4.0):
    """(depth (F, h, w) fp32, hit (F, h, w) int32, feat (F, h, w, C) fp32 or None, ok (F, h, w) bool)."""
    sdf = np.ascontiguousarray(sdf, F32)
    features = None if features is None else np.ascontiguousarray(features, F32)
    dt, ts, intr, mats = setup(world2grid, voxel_size, intrinsics, cam2world, step, depth_min, depth_max)
    frames = [forward_frame(sdf, F32(band), g, k, hw, dt, ts, features) for g, k in zip(mats, intr)]
    out = [np.stack([f[c] for f in frames]) for c in (0, 1, 3)]
    feat = None if features is None else np.stack([f[2] for f in frames])
    return out[0], out[1], feat, out[2]


def trilinear(c, a):
    """Rule H4's value from corners c (P, 8) and fractions a (P, 3): four lerps along x, two along y, one along z."""
    x = [C.lerp(c[:, 2 * e], c[:, 2 * e + 1], a[:, 0]) for e in range(4)]
    y = [C.lerp(x[0], x[1], a[:, 1]), C.lerp(x[2], x[3], a[:, 1])]
    return C.lerp(y[0], y[1], a[:, 2])


def feature_slopes(q, a):
    """(px, py, pz), each (P,): the gradient of rule 3's interpolant of corner values q (P, 8) in the weight form:
    four edges along each axis, left to right in corner order."""
    wx, wy, wz = axis_weights(a)
    px = (wz[:, 0] * wy[:, 0]) * (q[:, 1] - q[:, 0])
    px = px + (wz[:, 0] * wy[:, 1]) * (q[:, 3] - q[:, 2])
    px = px + (wz[:, 1] * wy[:, 0]) * (q[:, 5] - q[:, 4])
    px = px + (wz[:, 1] * wy[:, 1]) * (q[:, 7] - q[:, 6])
    py = (wz[:, 0] * wx[:, 0]) * (q[:, 2] - q[:, 0])
    py = py + (wz[:, 0] * wx[:, 1]) * (q[:, 3] - q[:, 1])
    py = py + (wz[:, 1] * wx[:, 0]) * (q[:, 6] - q[:, 4])
    py = py + (wz[:, 1] * wx[:, 1]) * (q[:, 7] - q[:, 5])
    pz = (wy[:, 0] * wx[:, 0]) * (q[:, 4] - q[:, 0])
    pz = pz + (wy[:, 0] * wx[:, 1]) * (q[:, 5] - q[:, 1])
    pz = pz + (wy[:, 1] * wx[:, 0]) * (q[:, 6] - q[:, 2])
    pz = pz + (wy[:, 1] * wx[:, 1]) * (q[:, 7] - q[:, 3])
    return px, py, pz


class Crossing:
    """The geometry of the hit pixels of one frame, rebuilt from k alone (rule 4) in `dtype`: pix (P,) pixel numbers
    in the frame, o (3,), d (P, 3), t0, f0 / f1 cells and a0 / a1 fractions of both samples, idx0 / idx1 (P, 8)."""

    def __init__(self, sdf_shape, g, k, hw, dt, depth_min, hitk, dtype=F32):
        T = dtype
        self.pix = np.nonzero(hitk.ravel() >= 1)[0]
        kk = hitk.ravel()[self.pix]
        o, d = C.rays(g, k, hw)                                            # rule H2 is fp32 in either case
        self.o, self.d = o.astype(T), d[self.pix].astype(T)
        self.dt = T(dt)
        self.t0 = T(depth_min) + (kk - 1).astype(T) * self.dt
        t1 = T(depth_min) + kk.astype(T) * self.dt
        g0 = (self.o + self.t0[:, None] * self.d).astype(T)
        g1 = (self.o + t1[:, None] * self.d).astype(T)
        in0, self.f0, self.a0 = cell(g0, sdf_shape)
        in1, self.f1, self.a1 = cell(g1, sdf_shape)
        assert in0.all() and in1.all()
        self.idx0, self.idx1 = corner_index(self.f0, sdf_shape), corner_index(self.f1, sdf_shape)


def pixel_terms(x, sdf, features, gd, gf):
    """Rule 4 for the pixels of a Crossing x, in x's dtype.  sdf (Z, Y, X), features (Z, Y, X, C) or None, gd (P,),
    gf (P, C) or None, all of that dtype -> (sdf_idx (P, 16), sdf_terms (P, 16), feat_idx (P, 8), feat_terms
    (P, 8, C) or None, inside (P,): rule 3's cell test, tstar (P,))."""
    T = x.d.dtype.type
    flat = sdf.reshape(-1)
    with np.errstate(all='ignore'):
        pv, v = trilinear(flat[x.idx0], x.a0), trilinear(flat[x.idx1], x.a1)
        den = pv - v
        tstar = x.t0 + x.dt * (pv / den)
        gs = (x.o + tstar[:, None] * x.d).astype(x.d.dtype)
        inside, fs, a = cell(gs, sdf.shape)
        G = gd.copy()
        fidx, fterms = corner_index(fs, sdf.shape), None
        if features is not None and gf is not None:
            ch = features.shape[3]
            fl = features.reshape(-1, ch)
            w = corner_weights(a)
            for c in range(ch):
                px, py, pz = feature_slopes(fl[fidx, c], a)
                D = (px * x.d[:, 0] + py * x.d[:, 1]) + pz * x.d[:, 2]
                G = np.where(inside, G + gf[:, c] * D, G)
            fterms = np.where(inside[:, None, None], gf[:, None, :] * w[:, :, None], T(0))
        A = (G * x.dt) / (den * den)
        cpv, cv = A * (-v), A * pv
        terms = np.concatenate([cpv[:, None] * corner_weights(x.a0), cv[:, None] * corner_weights(x.a1)], 1)
    return np.concatenate([x.idx0, x.idx1], 1), terms, fidx, fterms, inside, tstar


def terms(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, hitk, features=None, grad_depth=None, grad_feat=None,
          step=0.5, depth_min=0.4, dtype=F32):
    """All frames: a list with one entry (frame, Crossing, pixel_terms(..)) per non-empty frame.  hitk (F, h, w) is
    forward()'s record; grad_depth (F, h, w) and grad_feat (F, h, w, C) are the incoming gradients (None: zero)."""
    T, depth_min = dtype, F32(depth_min)
    sdf = np.ascontiguousarray(sdf, F32).astype(T)
    features = None if features is None else np.ascontiguousarray(features, F32).astype(T)
    dt, _, intr, mats = setup(world2grid, voxel_size, intrinsics, cam2world, step, depth_min, depth_min)
    out = []
    for f, (g, k) in enumerate(zip(mats, intr)):
        if g is None or not (hitk[f] >= 1).any():
            continue
        x = Crossing(sdf.shape, g, k, hw, dt, depth_min, hitk[f], T)
        gd = np.zeros(len(x.pix), T) if grad_depth is None else np.asarray(grad_depth[f], F32).ravel()[x.pix].astype(T)
        gf = None
        if grad_feat is not None and features is not None:
            gf = np.asarray(grad_feat[f], F32).reshape(-1, features.shape[3])[x.pix].astype(T)
        out.append((f, x, pixel_terms(x, sdf, features, gd, gf)))
    return out


def accumulate(lists, sdf_shape, channels=0):
    """Per-voxel sums of term lists in fp64 -> (grad_sdf, bound_sdf, grad_features, bound_features): the exact sums
    of the fp32 terms and rule 5's bound n . 2^-24 . sum |term| (features: None without channels)."""
    nv = int(np.prod(sdf_shape))
    gs, ab, cnt = np.zeros(nv), np.zeros(nv), np.zeros(nv)
    gfe = abf = cntf = None
    if channels:
        gfe, abf, cntf = np.zeros((nv, channels)), np.zeros((nv, channels)), np.zeros(nv)
    for _, _, (idx, t, fidx, ft, inside, _) in lists:
        t64 = t.astype(np.float64)
        np.add.at(gs, idx.ravel(), t64.ravel())
        np.add.at(ab, idx.ravel(), np.abs(t64).ravel())
        np.add.at(cnt, idx.ravel(), 1.0)
        if channels and ft is not None:
            ft64 = ft.astype(np.float64)[inside]
            np.add.at(gfe, fidx[inside].ravel(), ft64.reshape(-1, channels))
            np.add.at(abf, fidx[inside].ravel(), np.abs(ft64).reshape(-1, channels))
            np.add.at(cntf, fidx[inside].ravel(), 1.0)
    bound = cnt * 2.0 ** -24 * ab
    if not channels:
        return gs.reshape(sdf_shape), bound.reshape(sdf_shape), None, None
    shape = tuple(sdf_shape) + (channels,)
    return (gs.reshape(sdf_shape), bound.reshape(sdf_shape), gfe.reshape(shape),
            (cntf[:, None] * 2.0 ** -24 * abf).reshape(shape))


def scatter32(lists, sdf_shape, channels=0):
    """The term lists added one by one in fp32, in list order -> (grad_sdf, grad_features or None): what the device
    holds bit for bit when no voxel receives more than two terms (a two-term fp32 sum has no order)."""
    nv = int(np.prod(sdf_shape))
    gs = np.zeros(nv, F32)
    gfe = np.zeros((nv, channels), F32) if channels else None
    for _, _, (idx, t, fidx, ft, inside, _) in lists:
        np.add.at(gs, idx.ravel(), t.astype(F32).ravel())
        if channels and ft is not None:
            np.add.at(gfe, fidx[inside].ravel(), ft.astype(F32)[inside].reshape(-1, channels))
    return gs.reshape(sdf_shape), (gfe.reshape(tuple(sdf_shape) + (channels,)) if channels else None)


def forward64(x, c0, c1, features, cells=None):
    """The forward of the pixels of a Crossing x built with dtype=np.float64, k held fixed, as a function of the
    corner values of both samples c0, c1 (P, 8) and of the feature volume (Z, Y, X, C) fp64 or None -> (depth (P,),
    feat (P, C) or None).  cells (P, 3) x y z: the cell whose trilinear piece gives the features, wherever the hit
    moves (None: the cell the fp64 hit lies in, by rule 3's test)."""
    pv, v = trilinear(c0, x.a0), trilinear(c1, x.a1)
    tstar = x.t0 + x.dt * (pv / (pv - v))
    if features is None:
        return tstar, None
    gs = x.o + tstar[:, None] * x.d
    if cells is None:
        inside, fs, a = cell(gs, features.shape[:3])
    else:
        inside, fs, a = np.ones(len(gs), bool), cells, gs - cells
    return tstar, features_at(features, inside, fs, a)
