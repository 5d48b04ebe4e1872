"""Independent NumPy restatement of INTEGRATION.md section P (point clouds with sensor origins -> TSDF volumes).

Written from that text, not from csrc/points.hip, and it imports nothing of sgnn_amd.  Every float step is an fp32
NumPy operation of its own (one rounding per operation, the order the text gives); the per-voxel sums of a call are
exact integers (int64 arrays filled with np.add.at: no float sum anywhere; the fold checks that they convert to fp64
exactly, and folds the colour in integers).  The device result must therefore match bit for bit: sdf, weight, free
counter and colour record.

`integrate` works on a `Volume` of this file or on a `fusion_ref.Grid` (the same field names), so that the frame
route's restatement and this one can be chained on one state.
"""
import numpy as np

F32 = np.float32
FIXED = 4096            # fixed-point steps per voxel of the per-sample sdf
MAX_SAMPLES = 1 << 24


def round_away(x):
    """Round half away from zero in x's own precision."""
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5).astype(a.dtype), x)


def affine(m, p):
    """Rows 0..2 of the 4x4 m on points p (n, 3): ((m0 x + m1 y) + m2 z) + m3, in m's precision."""
    out = []
    for r in range(3):
        acc = m[r, 0] * p[:, 0]
        acc = acc + m[r, 1] * p[:, 1]
        acc = acc + m[r, 2] * p[:, 2]
        out.append(acc + m[r, 3])
    return np.stack(out, 1)


def dot3(a, b):
    acc = a[:, 0] * b[:, 0]
    acc = acc + a[:, 1] * b[:, 1]
    return acc + a[:, 2] * b[:, 2]


def in_obb(obb, q):
    o = np.asarray(obb, F32).reshape(4, 3)
    r = q - o[0]
    ok = np.ones(q.shape[0], bool)
    for k in range(3):
        e = np.broadcast_to(o[1 + k], r.shape)
        ee = dot3(o[1 + k][None], o[1 + k][None])[0]
        dd = dot3(r, e)
        ok &= (dd >= 0) & (dd <= ee)
    return ok


def grid2world(world2grid):
    """inv(world2grid) formed in fp64 from the fp32 matrix, rounded once."""
    return np.linalg.inv(np.asarray(world2grid, F32).astype(np.float64)).astype(F32)


class Volume(object):
    def __init__(self, dims_xyz, voxel_size, world2grid, dmin=0.4, dmax=4.0, obb=None, color=False):
        dx, dy, dz = dims_xyz
        self.dims, self.vs, self.w2g = tuple(dims_xyz), F32(voxel_size), np.asarray(world2grid, F32)
        self.dmin, self.dmax, self.obb = dmin, dmax, obb
        self.sdf = np.full((dz, dy, dx), -np.inf, F32)
        self.weight = np.zeros((dz, dy, dx), np.int64)
        self.free = np.zeros((dz, dy, dx), np.int64)
        self.color = np.zeros((dz, dy, dx, 4), np.int64) if color else None


def rays(vol, points, origins, origin_id, carve):
    """Rules 1-5 up to the sample count, for all rays: dict of per-ray arrays; n = 0 for an ignored ray."""
    p = np.asarray(points, F32).reshape(-1, 3)
    org = np.asarray(origins, F32).reshape(-1, 3)
    oid = np.zeros(p.shape[0], np.int64) if origin_id is None else np.asarray(origin_id, np.int64)
    assert oid.shape == (p.shape[0],) and (p.shape[0] == 0 or (oid.min() >= 0 and oid.max() < org.shape[0]))
    o = org[oid]
    vs, dmin, dmax = F32(vol.vs), F32(vol.dmin), F32(vol.dmax)
    with np.errstate(all='ignore'):
        v = p - o
        d = np.sqrt(dot3(v, v))
        ok = np.isfinite(p).all(1) & np.isfinite(o).all(1) & np.isfinite(d) & (d > 0) & (d >= dmin) & (d <= dmax)
        direction = v / d[:, None]
        trunc = vs * F32(3.0) + d * vs
        z01 = (d - F32(0.4)) / (F32(4.0) - F32(0.4))
        wu = np.maximum(F32(4.5) * (F32(1.0) - z01), F32(1.0))
        t0 = np.full_like(d, dmin) if carve else np.maximum(d - trunc, F32(0.0))
        te = d + trunc
        nf = np.floor((te - t0) / (vs * F32(0.5)))
        ok &= (nf >= 0) & (nf < MAX_SAMPLES)
    n = np.where(ok, np.where(ok, nf, 0).astype(np.int64) + 1, 0)
    wi = np.where(ok, wu, 0).astype(np.int64)                       # (int)wu: truncation
    return {'o': o, 'dir': direction, 'd': d, 'trunc': trunc, 't0': t0, 'n': n, 'wi': wi}


def sample_voxels(R, rr, n, w2g, half):
    t = R['t0'][rr] + n.astype(F32) * half
    w = R['o'][rr] + R['dir'][rr] * t[:, None]
    return round_away(affine(w2g, w))


def accumulate(vol, points, origins, origin_id=None, color=None, carve=True, batch=2048):
    """Rules 1-7: the call's integer accumulators, dense over the grid: S, W, free (dz, dy, dx) and C (dz, dy, dx, 4)
    or None."""
    dx, dy, dz = vol.dims
    S = np.zeros((dz, dy, dx), np.int64)
    W = np.zeros((dz, dy, dx), np.int64)
    Fr = np.zeros((dz, dy, dx), np.int64)
    C = None if color is None else np.zeros((dz, dy, dx, 4), np.int64)
    R = rays(vol, points, origins, origin_id, carve)
    col = None if color is None else np.asarray(color, np.uint8)
    w2g, g2w = np.asarray(vol.w2g, F32), grid2world(vol.w2g)
    vs = F32(vol.vs)
    half = vs * F32(0.5)
    live = np.nonzero(R['n'] > 0)[0]
    for b0 in range(0, live.shape[0], batch):
        ids = live[b0:b0 + batch]
        cnt = R['n'][ids]
        rr = np.repeat(ids, cnt)
        n = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        with np.errstate(all='ignore'):
            vox = sample_voxels(R, rr, n, w2g, half)
            prev = sample_voxels(R, rr, np.maximum(n - 1, 0), w2g, half)
            keep = (vox[:, 0] >= 0) & (vox[:, 0] < dx) & (vox[:, 1] >= 0) & (vox[:, 1] < dy) & (vox[:, 2] >= 0) & \
                (vox[:, 2] < dz)
            keep &= ~((n > 0) & (prev == vox).all(1))
        if vol.obb is not None:
            keep &= in_obb(vol.obb, vox)
        rr, vox = rr[keep], vox[keep]
        o, direction, d, trunc, wi = R['o'][rr], R['dir'][rr], R['d'][rr], R['trunc'][rr], R['wi'][rr]
        c = affine(g2w, vox)
        pz = dot3(c - o, direction)
        ix, iy, iz = (vox[:, a].astype(np.int64) for a in range(3))
        np.add.at(Fr, (iz, iy, ix), (pz < d).astype(np.int64))
        sd0 = d - pz
        up = sd0 > -trunc
        sd = np.where(sd0 >= 0, np.minimum(trunc, sd0), np.maximum(-trunc, sd0))
        q = round_away((sd / vs) * F32(FIXED)).astype(np.int64)
        np.add.at(S, (iz[up], iy[up], ix[up]), (q * wi)[up])
        np.add.at(W, (iz[up], iy[up], ix[up]), wi[up])
        if col is not None:
            has = up & (sd0 < trunc)                                  # free space gets no colour
            if col.shape[1] == 4:
                has &= col[rr, 3] != 0
            for ch in range(3):
                np.add.at(C[..., ch], (iz[has], iy[has], ix[has]), col[rr[has], ch].astype(np.int64) * wi[has])
            np.add.at(C[..., 3], (iz[has], iy[has], ix[has]), wi[has])
    return S, W, Fr, C


def fold(vol, S, W, Fr, C=None):
    """The fold of section P: the call as one observation per voxel."""
    vs = F32(vol.vs)
    assert np.abs(S).max(initial=0) < 2 ** 53 and W.max(initial=0) < 2 ** 32     # int64 -> fp64 below is exact
    vol.free += Fr
    m = W > 0
    obs = (S[m].astype(np.float64) / (W[m].astype(np.float64) * np.float64(4096.0))).astype(F32) * vs
    wu = np.minimum(W[m], 255)
    w = vol.weight[m]
    with np.errstate(invalid='ignore'):                                # the unselected branch of a first observation
        old = vol.sdf[m].astype(F32)
        mixed = (old * w.astype(F32) + obs * wu.astype(F32)) / (w.astype(F32) + wu.astype(F32))
    vol.sdf[m] = np.where(w == 0, obs, mixed)
    vol.weight[m] = np.minimum(w + wu, 255)
    if C is not None:
        m = C[..., 3] > 0
        cw = C[..., 3][m]
        wcu = np.minimum(cw, 255)
        wc = vol.color[..., 3][m]
        for ch in range(3):
            ci = (256 * C[..., ch][m] + cw // 2) // cw                  # the call's mean colour, 8.8 fixed point
            qo = vol.color[..., ch][m]
            vol.color[..., ch][m] = np.where(wc == 0, ci, (qo * wc + ci * wcu + (wc + wcu) // 2) // (wc + wcu))
        vol.color[..., 3][m] = np.minimum(wc + wcu, 255)
    return vol


def integrate(vol, points, origins, origin_id=None, color=None, carve=True):
    assert color is None or getattr(vol, 'color', None) is not None
    return fold(vol, *accumulate(vol, points, origins, origin_id, color, carve))


def from_depth(depth, intrinsics, cam2world):
    """Depth frames (F, h, w) as rays, fp32: (points (F h w, 3), origins (F, 3), origin_id); NaN points where the depth
    is not finite."""
    d = np.asarray(depth, F32)
    nf, h, w = d.shape
    k = np.asarray(intrinsics, F32).reshape(nf, 4)
    c2w = np.asarray(cam2world, np.float64).reshape(nf, 4, 4).astype(F32)
    u = np.arange(w, dtype=F32)[None, None, :]
    v = np.arange(h, dtype=F32)[None, :, None]
    z = np.where(np.isfinite(d), d, F32(np.nan))
    cam = np.stack([(u - k[:, 2, None, None]) * z / k[:, 0, None, None],
                    (v - k[:, 3, None, None]) * z / k[:, 1, None, None], z], -1).reshape(nf, h * w, 3)
    pts = np.einsum('fnc,frc->fnr', cam, c2w[:, :3, :3]) + c2w[:, None, :3, 3]
    return pts.reshape(-1, 3).astype(F32), c2w[:, :3, 3].copy(), np.repeat(np.arange(nf), h * w).astype(np.int32)
