"""Independent NumPy restatement of the mesh-distance rules.

Nothing here imports sgnn_amd.meshdist or touches a device.  Every fp32 value is produced by one NumPy operation per
rounding in the order section G states, so the device result must match `distance_ref` and `sample_ref` bit for bit.
`distance_ref` is brute force over all (point, face) pairs; `walk_ref` restates the grid and the shell walk of rule 5
and also returns the number of pairs the rule evaluates.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------
# rule 1: usable faces and their records
# ---------------------------------------------------------------------------------------------------------
def pack_ref(verts, faces, dtype=F32):
    """a, ab, ac (T, 3) in `dtype` (from the fp32 vertices) and usable (T,) bool; rule 1 is decided in fp32."""
    v = np.asarray(verts, F32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all='ignore'):
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    finite = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    usable = finite & ~((nx == 0) & (ny == 0) & (nz == 0))
    if dtype is not F32:
        a, b, c = a.astype(dtype), b.astype(dtype), c.astype(dtype)
        with np.errstate(all='ignore'):
            ab, ac = b - a, c - a
    return a, ab, ac, usable


# ---------------------------------------------------------------------------------------------------------
# rule 2: squared point-triangle distance; works elementwise on broadcastable (.., 3) arrays of one dtype
# ---------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _away(u, s, v):
    return u - s[..., None] * v


def tri_dist2(p, a, ab, ac):
    with np.errstate(all='ignore'):
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = ap - ab
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = ap - ac
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s, t = d4 - d3, d5 - d6
        den = (va + vb) + vc
        e = _away(_away(ap, vb / den, ab), vc / den, ac)                         # interior ...
        r1, r2 = _dot(ab, e), _dot(ac, e)                                        # ... and one refinement step
        g11, g12, g22 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
        e = _away(_away(e, (r1 * g22 - r2 * g12) / den, ab), (r2 * g11 - r1 * g12) / den, ac)
        e = np.where(((va <= 0) & (s >= 0) & (t >= 0))[..., None], _away(bp, s / (s + t), ac - ab), e)     # edge bc
        e = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], _away(ap, d2 / (d2 - d6), ac), e)     # edge ac
        e = np.where(((d6 >= 0) & (d5 <= d6))[..., None], cp, e)                                           # vertex c
        e = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], _away(ap, d1 / (d1 - d3), ab), e)     # edge ab
        e = np.where(((d3 >= 0) & (d4 <= d3))[..., None], bp, e)                                           # vertex b
        e = np.where(((d1 <= 0) & (d2 <= 0))[..., None], ap, e)                                            # vertex a
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


# ---------------------------------------------------------------------------------------------------------
# rules 3 and 4: brute force
# ---------------------------------------------------------------------------------------------------------
def _finish(best, face, max_dist, dtype):
    d = np.sqrt(best)
    if max_dist is not None:
        far = ~(d <= dtype(max_dist))
        d[far], face[far] = np.inf, -1
    return d, face.astype(np.int32)


def _distance(points, verts, faces, max_dist, dtype, block):
    pts = np.asarray(points, F32).astype(dtype).reshape(-1, 3)
    a, ab, ac, usable = pack_ref(verts, faces, dtype)
    ids = np.nonzero(usable)[0]
    a, ab, ac = a[ids], ab[ids], ac[ids]
    best = np.full(len(pts), np.inf, dtype)
    face = np.full(len(pts), -1, np.int64)
    ok = np.isfinite(pts).all(1)
    for s in range(0, len(pts), block):
        sel = np.nonzero(ok[s:s + block])[0] + s
        if not len(sel) or not len(ids):
            continue
        d2 = tri_dist2(pts[sel, None, :], a[None], ab[None], ac[None])
        d2 = np.where(np.isnan(d2), np.inf, d2)
        k = np.argmin(d2, 1)                                                    # first = lowest face index
        m = d2[np.arange(len(sel)), k]
        best[sel] = m
        face[sel] = np.where(m < np.inf, ids[k], -1)
    return _finish(best, face, max_dist, dtype)


def distance_ref(points, verts, faces, max_dist=None, block=256):
    """(P,) fp32 distance and (P,) int32 face: the minimum over all usable faces, lowest index among equals."""
    return _distance(points, verts, faces, max_dist, F32, block)


def distance_ref64(points, verts, faces, max_dist=None, block=256):
    """The same construction with every operation in fp64 (the inputs are the same fp32 numbers)."""
    return _distance(points, verts, faces, max_dist, F64, block)


# ---------------------------------------------------------------------------------------------------------
# rule 5: the grid and the shell walk
# ---------------------------------------------------------------------------------------------------------
def cell_of(x, lo, cell, n):
    with np.errstate(all='ignore'):
        q = np.floor(((np.asarray(x, F32) - F32(lo)) / F32(cell)).astype(F32))
    q = np.where(q >= 0, q, 0)                                                  # NaN -> 0
    return np.minimum(q, n - 1).astype(np.int64)


def default_cell_ref(verts, faces):
    a, ab, ac, usable = pack_ref(verts, faces)
    edges = np.concatenate([np.linalg.norm(x[usable].astype(F64), axis=1) for x in (ab, ac, ac - ab)])
    lo, hi = grid_box(verts, faces)
    median = np.sort(edges)[(len(edges) - 1) // 2]                              # the lower of two middle values
    return F32(max(2.0 * median, (hi.astype(F64) - lo.astype(F64)).max() / 256.0))


def grid_box(verts, faces):
    v = np.asarray(verts, F32)
    usable = pack_ref(verts, faces)[3]
    tri = v[np.asarray(faces, np.int64).reshape(-1, 3)[usable]]
    return tri.min((0, 1)), tri.max((0, 1))


class GridRef:
    """Cells of pitch `cell` over the box of the usable faces, every face listed in the cells its box touches (CSR)."""

    def __init__(self, verts, faces, cell):
        v = np.asarray(verts, F32)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        self.a, self.ab, self.ac, usable = pack_ref(verts, faces)
        self.lo, self.hi = grid_box(verts, faces)
        self.cell = F32(cell)
        self.dims = tuple(int(np.floor(((h - l) / self.cell).astype(F32))) + 1 for l, h in zip(self.lo, self.hi))
        nx, ny, nz = self.dims
        cells, ids = [], []
        for t in np.nonzero(usable)[0]:
            tri = v[f[t]]
            r = [np.arange(cell_of(tri[:, k].min(), self.lo[k], self.cell, self.dims[k]),
                           cell_of(tri[:, k].max(), self.lo[k], self.cell, self.dims[k]) + 1) for k in range(3)]
            c = ((r[2][:, None, None] * ny + r[1][None, :, None]) * nx + r[0][None, None, :]).ravel()
            cells.append(c)
            ids.append(np.full(len(c), t, np.int64))
        cells, ids = np.concatenate(cells), np.concatenate(ids)
        order = np.lexsort((ids, cells))
        self.refs = ids[order]
        self.offsets = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=nx * ny * nz))])


def _shell_offsets(r):
    k = np.arange(-r, r + 1)
    dz, dy, dx = np.meshgrid(k, k, k, indexing='ij')
    on = np.maximum(np.abs(dz), np.maximum(np.abs(dy), np.abs(dx))) == r
    return np.stack([dx[on], dy[on], dz[on]], 1)


def walk_ref(points, grid, max_dist=None):
    """The shell walk of rule 5 for all points: (distance fp32, face int32, pairs evaluated, cells visited)."""
    pts = np.asarray(points, F32).reshape(-1, 3)
    g, (nx, ny, nz) = grid, grid.dims
    dims = np.array(grid.dims)
    best = np.full(len(pts), INF, F32)
    face = np.full(len(pts), -1, np.int64)
    active = np.nonzero(np.isfinite(pts).all(1))[0]
    c = np.stack([cell_of(pts[:, k], g.lo[k], g.cell, dims[k]) for k in range(3)], 1)
    with np.errstate(all='ignore'):
        m = np.maximum(np.abs(pts - g.lo), np.abs(pts - g.hi)).max(1)
        slack = m * F32(2.0 ** -18)
    rmax = np.maximum(c, dims - 1 - c).max(1)
    md = INF if max_dist is None else F32(max_dist)
    pairs = cells = 0
    r = 0
    while len(active):
        for off in _shell_offsets(r):
            cc = c[active] + off
            inside = ((cc >= 0) & (cc < dims)).all(1)
            pi, cc = active[inside], cc[inside]
            lin = (cc[:, 2] * ny + cc[:, 1]) * nx + cc[:, 0]
            beg, cnt = g.offsets[lin], g.offsets[lin + 1] - g.offsets[lin]
            cells += len(lin)
            pairs += int(cnt.sum())
            if not cnt.sum():
                continue
            pp = np.repeat(pi, cnt)                                             # one row per (point, listed face)
            within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            tt = g.refs[np.repeat(beg, cnt) + within]
            d2 = tri_dist2(pts[pp], g.a[tt], g.ab[tt], g.ac[tt])
            d2 = np.where(np.isnan(d2), INF, d2)
            order = np.lexsort((tt, d2, pp))
            pp, tt, d2 = pp[order], tt[order], d2[order]
            first = np.concatenate([[True], pp[1:] != pp[:-1]])
            pp, tt, d2 = pp[first], tt[first], d2[first]
            better = (d2 < best[pp]) | ((d2 == best[pp]) & (tt < face[pp]))
            best[pp[better]], face[pp[better]] = d2[better], tt[better]
        # the bound after shell r
        a = active[r < rmax[active]]                                            # the others have seen the whole grid
        gap = np.full(len(a), INF, F32)
        for k in range(3):
            lo_side = c[a, k] - r > 0
            hi_side = c[a, k] + r < dims[k] - 1
            with np.errstate(all='ignore'):
                glo = pts[a, k] - (g.lo[k] + (c[a, k] - r).astype(F32) * g.cell)
                ghi = (g.lo[k] + (c[a, k] + r + 1).astype(F32) * g.cell) - pts[a, k]
            gap = np.where(lo_side, np.minimum(gap, glo), gap)
            gap = np.where(hi_side, np.minimum(gap, ghi), gap)
        with np.errstate(all='ignore'):
            bound = gap - slack[a]
            done = (bound > 0) & ((best[a] < bound * bound) | (bound > md))
        active = a[~done]
        r += 1
    d, face = _finish(best, face, max_dist, F32)
    return d, face, pairs, cells


def walk_pairs_ref(points, verts, faces, cell, max_dist=None):
    """Number of (point, face) pairs the walk of rule 5 evaluates."""
    return walk_ref(points, GridRef(verts, faces, cell), max_dist)[2]


# ---------------------------------------------------------------------------------------------------------
# rule 6: sampling
# ---------------------------------------------------------------------------------------------------------
def fmix64(k):
    k &= MASK64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k


def _fmix64_array(k):
    k = k.astype(np.uint64)
    with np.errstate(over='ignore'):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def fractions(seed, n):
    """(n, 3) int64 numerators m of the 24-bit fractions u_k = m / 2^24 of samples 0..n-1."""
    base = np.uint64(fmix64(int(seed)))
    with np.errstate(over='ignore'):
        counter = base + (np.uint64(3) * np.arange(n, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None])
    return (_fmix64_array(counter) >> np.uint64(40)).astype(np.int64)


def areas_ref(verts, faces):
    """fp64 areas from the fp32 records, 0 for an ignored face, and NumPy's cumulative sum."""
    _, ab, ac, usable = pack_ref(verts, faces)
    area = 0.5 * np.linalg.norm(np.cross(ab.astype(F64), ac.astype(F64)), axis=1)
    area = np.where(usable, area, 0.0)
    return area, np.cumsum(area)


def sample_ref(verts, faces, n, seed, cum):
    """(n, 3) fp32 points and (n,) int32 faces from the fp64 cumulative areas `cum` (T,)."""
    a, ab, ac, usable = pack_ref(verts, faces)
    cum = np.asarray(cum, F64)
    m = fractions(seed, n)
    u0 = int(fractions(seed, 1)[0, 0]) * 2.0 ** -24                             # one offset for all samples
    x = ((np.arange(n, dtype=F64) + u0) / F64(n)) * cum[-1]
    t = np.minimum(np.searchsorted(cum, x, side='right'), np.nonzero(usable)[0][-1])      # first cum[t] > x
    reflect = m[:, 1] + m[:, 2] > (1 << 24)
    u1 = (np.where(reflect, (1 << 24) - m[:, 1], m[:, 1]).astype(F32) * F32(2.0 ** -24))[:, None]
    u2 = (np.where(reflect, (1 << 24) - m[:, 2], m[:, 2]).astype(F32) * F32(2.0 ** -24))[:, None]
    pts = (a[t] + u1 * ab[t]) + u2 * ac[t]
    return pts.astype(F32), t.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------
def compare_ref(d_pred, d_target, thresholds=(0.05,), max_dist=None):
    rep = {}
    means = []
    for d in (d_pred, d_target):
        x = np.asarray(d, F32).astype(F64)
        if max_dist is not None:
            x = np.where(np.isinf(x), F64(F32(max_dist)), x)
        means.append(float(x.mean()))
    rep['accuracy'], rep['completeness'] = means
    rep['chamfer'] = means[0] + means[1]
    rep['hits_pred'] = [int((np.asarray(d_pred, F32) <= F32(t)).sum()) for t in thresholds]
    rep['hits_target'] = [int((np.asarray(d_target, F32) <= F32(t)).sum()) for t in thresholds]
    rep['precision'] = [h / len(d_pred) for h in rep['hits_pred']]
    rep['recall'] = [h / len(d_target) for h in rep['hits_target']]
    rep['fscore'] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(rep['precision'], rep['recall'])]
    return rep


# ---------------------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------
def clipped_soup(n, seed=0, big=0.1):
    """n random triangles with every coordinate in [-1, 5]: most from millimetres to decimetres, a share `big` of
    them up to metres."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.0, 4.0, (n, 1, 3))
    size = 10.0 ** np.where(rng.random((n, 1, 1)) < big, rng.uniform(-0.5, 0.3, (n, 1, 1)), rng.uniform(-3.0, -0.7, (n, 1, 1)))
    verts = np.clip(centre + rng.normal(size=(n, 3, 3)) * size, -1.0, 5.0).reshape(-1, 3).astype(F32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def near_surface_points(verts, faces, n, seed=0, off=1e-3):
    """n points `off` away (random direction) from random points of random faces."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, F64)
    f = np.asarray(faces, np.int64)[rng.integers(0, len(faces), n)]
    u = rng.random((n, 2))
    u = np.where((u.sum(1) > 1)[:, None], 1 - u, u)
    p = v[f[:, 0]] + u[:, :1] * (v[f[:, 1]] - v[f[:, 0]]) + u[:, 1:] * (v[f[:, 2]] - v[f[:, 0]])
    d = rng.normal(size=(n, 3))
    return (p + off * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def sliver_soup(n, aspect, seed=0):
    """n triangles 0.1 to 2 long and 1 / aspect of that wide, anywhere in [0, 4]^3."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 4.0, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    length = rng.uniform(0.1, 2.0, (n, 1))
    b = a + length * u
    c = a + length * (rng.uniform(0.2, 0.8, (n, 1)) * u + w / aspect)
    verts = np.stack([a, b, c], 1).reshape(-1, 3).astype(F32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def pruning_case():
    """A finely tessellated room (21 168 triangles) and 20 000 points 1 mm off its surface."""
    import render_ref as RR
    verts, faces = RR.tessellate_room(21)
    return verts, faces, near_surface_points(verts, faces, 20000, seed=5)
