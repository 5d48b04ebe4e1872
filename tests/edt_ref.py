"""Host restatement of sgnn_amd.edt in NumPy, by brute force: every voxel takes the minimum,
over the list of ALL seeds, of the key (squared distance, linear index of the seed).  Nothing here is separable, so the
three-pass kernels (sgnn_amd/csrc/edt.hip) and this file share no reasoning; tests/test_edt_ref.py checks that the
decomposition the kernels rely on gives the same answer.

    dist2, nearest = feature_transform(seeds, max_dist=None)     # (Z, Y, X) int32 each, -1 = none
    rgb = fill_colors(colors, nearest)                           # (Z, Y, X, 3) uint8

The key is one int64, dist2 * 2^31 + index (an index is < 2^31), so "smallest distance, then smallest linear index" is
one integer minimum.  Seeds are taken a chunk at a time to bound memory: a chunk costs dy * dx * chunk keys.
"""
import math

import numpy as np

SHIFT = 31
NONE = np.iinfo(np.int64).max


def cap2_of(max_dist):
    """floor(R * R) with the product in fp64, or None for no cap (None, or a square that no volume reaches)."""
    if max_dist is None:
        return None
    r = float(max_dist)
    if not r >= 0.0:
        raise ValueError('max_dist must be >= 0, got %r' % (max_dist,))
    rr = r * r
    return None if rr >= 2.0 ** 31 else int(math.floor(rr))


def brute(seeds, chunk_keys=1 << 19):
    """(dist2, nearest) int32 without a cap."""
    seeds = np.asarray(seeds) != 0
    if seeds.ndim != 3:
        raise ValueError('seeds must be (Z, Y, X)')
    dz, dy, dx = seeds.shape
    idx = np.flatnonzero(seeds.reshape(-1)).astype(np.int64)
    sz, sy, sx = idx // (dy * dx), (idx // dx) % dy, idx % dx
    best = np.full((dz, dy, dx), NONE, dtype=np.int64)
    chunk = max(1, chunk_keys // max(1, dy * dx))
    az, ay, ax = (np.arange(d, dtype=np.int64)[:, None] for d in (dz, dy, dx))
    for c in range(0, idx.size, chunk):
        s = slice(c, c + chunk)
        kz = ((az - sz[None, s]) ** 2) << SHIFT                         # (dz, S)
        ky = ((ay - sy[None, s]) ** 2) << SHIFT                         # (dy, S)
        kx = (((ax - sx[None, s]) ** 2) << SHIFT) + idx[None, s]        # (dx, S): carries the index
        plane = ky[:, None, :] + kx[None, :, :]                         # (dy, dx, S)
        for z in range(dz):
            np.minimum(best[z], (plane + kz[z]).min(axis=-1), out=best[z])
    none = best == NONE
    dist2 = np.where(none, -1, best >> SHIFT).astype(np.int32)
    nearest = np.where(none, -1, best & ((1 << SHIFT) - 1)).astype(np.int32)
    return dist2, nearest


def cap(dist2, nearest, max_dist):
    """The cap of the contract applied to an uncapped result: beyond floor(R * R) a voxel has no seed."""
    c2 = cap2_of(max_dist)
    if c2 is None:
        return dist2, nearest
    far = dist2 > c2
    return np.where(far, -1, dist2).astype(np.int32), np.where(far, -1, nearest).astype(np.int32)


def feature_transform(seeds, max_dist=None):
    return cap(*brute(seeds), max_dist)


def fill_colors(colors, nearest):
    """out[p] = colors[nearest[p]] where nearest[p] >= 0, else 0."""
    colors = np.asarray(colors)
    if colors.dtype != np.uint8 or colors.shape != nearest.shape + (3,):
        raise ValueError('colors must be %s uint8' % (nearest.shape + (3,),))
    flat = colors.reshape(-1, 3)
    out = flat[np.maximum(nearest.reshape(-1), 0)].copy()
    out[nearest.reshape(-1) < 0] = 0
    return out.reshape(colors.shape)


# ----------------------------------------------------------------------------------------------------------------------
# the three-pass decomposition of the kernels, restated on the host (tests/test_edt_ref.py holds it to brute())
# ----------------------------------------------------------------------------------------------------------------------
def _pass(g, feat, axis):
    """One pass along axis: g (partial squared distance, NONE = no seed yet) and feat (linear index of the partial
    nearest seed) -> the same after minimising g[a'] + (a - a')^2 over a', ties to the smaller a'."""
    n = g.shape[axis]
    g = np.moveaxis(g, axis, 0)
    feat = np.moveaxis(feat, axis, 0)
    a = np.arange(n, dtype=np.int64)
    off = ((a[:, None] - a[None, :]) ** 2).reshape((n, n) + (1,) * (g.ndim - 1))          # [a, a']
    cost = np.where(g[None] == NONE, NONE, g[None] + off)                                 # (a, a', ...)
    pick = cost.argmin(axis=1)                                                            # the first: smallest a'
    g2 = np.take_along_axis(cost, pick[:, None], axis=1)[:, 0]
    f2 = np.take_along_axis(np.broadcast_to(feat[None], cost.shape), pick[:, None], axis=1)[:, 0]
    return np.moveaxis(g2, 0, axis), np.moveaxis(f2, 0, axis)


def separable(seeds):
    """(dist2, nearest) int32 without a cap by the x, y, z passes."""
    seeds = np.asarray(seeds) != 0
    n = seeds.size
    g = np.where(seeds, 0, NONE).astype(np.int64)
    feat = np.arange(n, dtype=np.int64).reshape(seeds.shape)
    for axis in (2, 1, 0):
        g, feat = _pass(g, feat, axis)
    none = g == NONE
    return np.where(none, -1, g).astype(np.int32), np.where(none, -1, feat).astype(np.int32)
