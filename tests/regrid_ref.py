"""Independent NumPy restatement of INTEGRATION.md section Q (a TSDF volume's state on another grid).  Nothing here
imports sgnn_amd: the map, the rounding, the corner rules and the folds have their own code.  All float arithmetic is
fp32 with one rounding per operation (NumPy rounds every array operation once and never fuses), so the device result
must match bit for bit: sdf bits, weight, free counter and colour record as integers.
"""
import numpy as np

F32 = np.float32


class Vol(object):
    """The state of a volume on the host: sdf (dz, dy, dx) fp32, weight and free int64, color (dz, dy, dx, 4) int64
    (R, G, B in 8.8 fixed point and the colour weight) or None."""

    def __init__(self, dims_xyz, voxel_size, world2grid, color=False):
        dx, dy, dz = (int(d) for d in dims_xyz)
        self.dims_xyz, self.voxel_size = (dx, dy, dz), F32(voxel_size)
        self.world2grid = np.asarray(world2grid, F32).reshape(4, 4).copy()
        self.sdf = np.full((dz, dy, dx), -np.inf, F32)
        self.weight = np.zeros((dz, dy, dx), np.int64)
        self.free = np.zeros((dz, dy, dx), np.int64)
        self.color = np.zeros((dz, dy, dx, 4), np.int64) if color else None

    def copy(self):
        c = Vol(self.dims_xyz, self.voxel_size, self.world2grid, self.color is not None)
        c.sdf, c.weight, c.free = self.sdf.copy(), self.weight.copy(), self.free.copy()
        c.color = None if self.color is None else self.color.copy()
        return c


def from_state(dims_xyz, voxel_size, world2grid, sdf, weight, free, color=None):
    v = Vol(dims_xyz, voxel_size, world2grid, color is not None)
    v.sdf[...] = np.asarray(sdf, F32)
    v.weight[...] = weight
    v.free[...] = free
    if color is not None:
        v.color[...] = color
    return v


def random_volume(dims_xyz, seed, color=True, world2grid=None, voxel_size=0.05):
    """A volume with holes: about a third of the voxels never seen (-inf, weight 0) in blocks of 4 x 4 x 4, a sparse
    checkerboard of voxels with weight > 0 but sdf -inf (so one-bad-corner samples occur), free counts everywhere, colour
    on most seen voxels."""
    rng = np.random.default_rng(seed)
    v = Vol(dims_xyz, voxel_size, np.eye(4) if world2grid is None else world2grid, color)
    shape = v.sdf.shape
    z, y, x = np.indices(shape)
    seen = (x // 4 + 2 * (y // 4) + z // 4 + int(seed)) % 3 != 0
    v.sdf[...] = np.where(seen, rng.uniform(-0.3, 0.3, shape), -np.inf).astype(F32)
    v.weight[...] = np.where(seen, rng.integers(1, 256, shape), 0)
    odd = ((x + y + z) % 2 == 0) & (rng.random(shape) < 0.12)
    v.sdf[odd] = -np.inf                       # weight > 0 and not finite: unobserved by rule 2
    v.weight[odd] = np.maximum(v.weight[odd], 1)
    v.free[...] = rng.integers(0, 50, shape)
    if color:
        v.color[...] = rng.integers(0, 65536, shape + (4,))
        v.color[..., 3] = np.where(seen & (rng.random(shape) < 0.8), rng.integers(1, 256, shape), 0)
        v.color[v.color[..., 3] == 0] = 0
    return v


def round_away(x):
    """C's roundf: halves away from zero, exact (|x| - floor |x| is exact in fp32)."""
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= F32(0.5)).astype(F32), x).astype(F32)


def grid_map(src_w2g, dst_w2g):
    """Rule 1: rows 0..2 of src.world2grid . inv(dst.world2grid), fp64 from the fp32 matrices, rounded once; the
    identity where the two fp32 matrices are equal entry by entry."""
    s, d = (np.asarray(m, F32).astype(np.float64).reshape(4, 4) for m in (src_w2g, dst_w2g))
    a = (np.eye(4) if (s == d).all() else s @ np.linalg.inv(d))[:3].astype(F32)
    if not np.isfinite(a).all():
        raise ValueError('the map is not finite')
    return a


def positions(a, dims_xyz):
    """g = A . (i, j, k, 1) for every destination voxel, rows evaluated ((m0 i + m1 j) + m2 k) + m3 -> 3 x (dz, dy, dx)."""
    dx, dy, dz = dims_xyz
    k, j, i = np.meshgrid(np.arange(dz, dtype=F32), np.arange(dy, dtype=F32), np.arange(dx, dtype=F32), indexing='ij')
    out = []
    for r in range(3):
        t = a[r, 0] * i
        t = t + a[r, 1] * j
        t = t + a[r, 2] * k
        out.append((t + a[r, 3]).astype(F32))
    return out


def lerp(p, q, a):
    """l(p, q, a) = p + a (q - p); l(p, q, 0) = p by definition."""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(a == 0, p, p + a * (q - p)).astype(F32)


def sample(src, dims_xyz, a, mode='linear'):
    """Rules 2 - 6 for every destination voxel -> (s2 fp32, w2, f2, c2 or None), arrays (dz, dy, dx[, 4])."""
    if mode not in ('linear', 'nearest'):
        raise ValueError(mode)
    sx, sy, sz = src.dims_xyz
    top = [F32(sx - 1), F32(sy - 1), F32(sz - 1)]
    g = positions(a, dims_xyz)
    observed = (src.weight > 0) & np.isfinite(src.sdf)                                  # rule 2
    r = [round_away(v) for v in g]                                                      # rule 3
    r_in = np.ones(g[0].shape, bool)
    for c in range(3):
        r_in &= (r[c] >= 0) & (r[c] <= top[c])
    ri = [np.where(r_in, v, 0).astype(np.int64) for v in r]
    f2 = np.where(r_in, src.free[ri[2], ri[1], ri[0]], 0)                               # rule 6
    if mode == 'nearest':                                                               # rule 4
        valid = r_in & observed[ri[2], ri[1], ri[0]]
        s2 = np.where(valid, src.sdf[ri[2], ri[1], ri[0]], F32(-np.inf)).astype(F32)
        w2 = np.where(valid, src.weight[ri[2], ri[1], ri[0]], 0)
    else:                                                                               # rule 5
        f = [np.floor(v) for v in g]
        al = [(v - fl).astype(F32) for v, fl in zip(g, f)]
        two = [x != 0 for x in al]                                  # the axis has a second participating index
        inr = np.ones(g[0].shape, bool)
        for c in range(3):
            inr &= (f[c] >= 0) & (np.where(two[c], f[c] + F32(1), f[c]) <= top[c])
        fi = [np.where(inr, v, 0).astype(np.int64) for v in f]
        valid = inr.copy()
        w2 = np.full(g[0].shape, 255, np.int64)
        corner = {}
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    takes_part = inr & (two[0] | (cx == 0)) & (two[1] | (cy == 0)) & (two[2] | (cz == 0))
                    # a corner that does not take part is not looked at: index it at the cell's own voxel
                    ix = fi[0] + np.where(takes_part, cx, 0)
                    iy = fi[1] + np.where(takes_part, cy, 0)
                    iz = fi[2] + np.where(takes_part, cz, 0)
                    valid &= ~takes_part | observed[iz, iy, ix]
                    w2 = np.where(takes_part, np.minimum(w2, src.weight[iz, iy, ix]), w2)
                    corner[cx, cy, cz] = src.sdf[iz, iy, ix]
        x = {(cy, cz): lerp(corner[0, cy, cz], corner[1, cy, cz], al[0]) for cy in (0, 1) for cz in (0, 1)}
        y = {cz: lerp(x[0, cz], x[1, cz], al[1]) for cz in (0, 1)}
        s2 = np.where(valid, lerp(y[0], y[1], al[2]), F32(-np.inf)).astype(F32)
        w2 = np.where(valid, w2, 0)
    c2 = None
    if src.color is not None:
        c2 = np.where(valid[..., None], src.color[ri[2], ri[1], ri[0]], 0)
    return s2, w2, f2, c2


def resample(src, dims_xyz, world2grid, voxel_size=None, mode='linear'):
    out = Vol(dims_xyz, src.voxel_size if voxel_size is None else voxel_size, world2grid, src.color is not None)
    s2, w2, f2, c2 = sample(src, out.dims_xyz, grid_map(src.world2grid, out.world2grid), mode)
    out.sdf, out.weight, out.free = s2, w2, f2
    if c2 is not None:
        out.color = c2
    return out


def merge(dst, src, mode='linear'):
    """Rule 8, in place."""
    s2, w2, f2, c2 = sample(src, dst.dims_xyz, grid_map(src.world2grid, dst.world2grid), mode)
    dst.free = dst.free + f2
    s1, w1 = dst.sdf, dst.weight
    w1f, w2f = w1.astype(F32), w2.astype(F32)
    with np.errstate(all='ignore'):
        mean = ((s1 * w1f + s2 * w2f).astype(F32) / (w1f + w2f).astype(F32)).astype(F32)
    dst.sdf = np.where(w2 == 0, s1, np.where(w1 == 0, s2, mean)).astype(F32)
    dst.weight = np.where(w2 == 0, w1, np.where(w1 == 0, w2, np.minimum(w1 + w2, 255)))
    if dst.color is not None and c2 is not None:
        wcu, wc = c2[..., 3], dst.color[..., 3]
        upd = (w2 > 0) & (wcu > 0)
        den = np.maximum(wc + wcu, 1)
        for c in range(3):
            q, ci = dst.color[..., c], c2[..., c]
            new = np.where(wc == 0, ci, (q * wc + ci * wcu + (wc + wcu) // 2) // den)
            dst.color[..., c] = np.where(upd, new, q)
        dst.color[..., 3] = np.where(upd, np.minimum(wc + wcu, 255), wc)
    return dst
