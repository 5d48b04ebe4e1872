"""Looking inside a point cloud on the GPU: a uniform-grid index over a point set with exact k-nearest-neighbour and
radius queries, PCA normals, statistical and radius outlier filters, voxel down-sampling and cloud-to-cloud metrics.

The reference project has no counterpart; the rules this module follows are listed in INTEGRATION.md section Z, and
that text is the contract of the kernels (sgnn_amd/csrc/cloud.hip) and of the independent NumPy restatement of the
tests (tests/cloud_ref.py), which searches by brute force.  Every answer is a pure function of the points: it does not
depend on the grid pitch, and the same input gives the same bits on every run.

    index = PointIndex(points, cell=None)                  # built once; cell=None: the default pitch of rule C.1
    idx, d2 = index.knn(queries, k, max_dist=None)         # (Q,k) int32 / fp32, ascending by (d2, idx); -1 / +inf where fewer
    idx, d2 = index.knn(None, k)                           # the indexed points as queries, each WITHOUT its own row
    d, idx = index.nearest(queries, max_dist=None)         # k = 1: (Q,) fp32 distance and (Q,) int32
    cnt = index.radius_count(queries, radius)              # (Q,) int32, d2 <= radius * radius (the fp32 product)
    start, nbr = index.radius(queries, radius)             # CSR: (Q+1,) int64, (M,) int32 ascending per query
    res = normals(points, k=16, max_dist=None, toward=None, index=None)      # Normals(normal, variation, valid)
    keep, mean_d, thr = statistical_outliers(points, k=16, std_ratio=2.0, index=None)
    keep = radius_outliers(points, radius, min_neighbors, index=None)
    out = voxel_downsample(points, cell, colors=None, normals=None)          # Thinned(points, colors, normals, count, first, cell_of)
    rep = compare(pred_points, target_points, thresholds=(0.05,), max_dist=None)        # meshdist.summarise's report

Points are (N, 3) fp32, numpy arrays or torch tensors, host or device, as smooth and simplify take them; results are
device tensors and the inputs are not written.  A row with a non-finite coordinate is never a neighbour and gets the
empty answer as a query.  The host layer does plumbing only: the bounding box and the pitch, the sorts of the keys
(torch.sort), the scans of counts and _glue.compact; distances, normals and means come from the kernels.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._glue import compact, source_device, to_device

F32 = np.float32
LIMIT = 2 ** 31
MAX_K = 32
MAX_CELLS_AXIS = 1024       # rule C.2 rests on it (MAX_AXIS of csrc/cloud.hip)
STATUS_RANGE = 1            # SGNN_STATUS_COORD_RANGE
VOXEL_LIMIT = 2 ** 20       # cells of voxel_downsample lie in (-2^20, 2^20) on every axis

Normals = namedtuple('Normals', 'normal variation valid')
Thinned = namedtuple('Thinned', 'points colors normals count first cell_of')


def max_cells(n):
    """The most cells a grid over n finite points may have (rule C.1): 2 n + 64."""
    return 2 * n + 64


def _rows(name, x, cols=(3,)):
    shape = tuple(np.shape(x))
    if len(shape) != 2 or shape[1] not in cols:
        raise ValueError('%s must be (N, %s), got %s' % (name, ' | '.join(str(c) for c in cols), shape))
    if shape[0] >= LIMIT // MAX_K:
        raise ValueError('%s: %d rows do not fit (at most %d)' % (name, shape[0], LIMIT // MAX_K - 1))
    return shape[0]


def _k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError('k must be an integer in [1, %d], got %r' % (MAX_K, k))
    return int(k)


def _positive(name, v):
    f = F32(v)
    if not (f > 0 and np.isfinite(f)):
        raise ValueError('%s must be positive and finite, got %r' % (name, v))
    return f


def _limit2(name, v):
    """fp32 v * v of a distance bound that is not negative (None: +inf)."""
    if v is None:
        return float('inf')
    f = F32(v)
    if not f >= 0:
        raise ValueError('%s must be >= 0, got %r' % (name, v))
    with np.errstate(over='ignore'):
        return float(f * f)


def default_cell(lo, hi, n):
    """Rule C.1: the pitch at which a surface of the area of the bounding box's three faces holds four points a cell,
    sqrt(4 (ex ey + ey ez + ez ex) / n), not below 4 max(e) / n (points on a line), 1 where both are 0."""
    e = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    c = max(np.sqrt(4.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]) / max(n, 1)), 4.0 * e.max() / max(n, 1))
    c = F32(c)
    return c if c > 0 and np.isfinite(c) else F32(1.0)


def fit_cell(cell, lo, hi, n):
    """Rule C.1: (cell, dims) with cell doubled until the grid has at most MAX_CELLS_AXIS cells an axis and
    max_cells(n) in all.  dims are one more than the fp32 cell of hi, as the kernels compute it."""
    cell = F32(cell)
    while True:
        with np.errstate(all='ignore'):
            dims = np.floor((hi - lo).astype(F32) / cell).astype(np.int64) + 1
        if dims.max() <= MAX_CELLS_AXIS and int(dims.prod()) <= max_cells(n):
            return cell, tuple(int(d) for d in dims)
        cell = F32(cell * F32(2.0))


class PointIndex:
    """A uniform grid over the finite rows of points (N, 3), on the device: the points re-ordered by cell as
    (x, y, z, index) records and the first record of every cell.  cell: the pitch, None for default_cell; a pitch that
    would give more than max_cells(N) cells, or more than 1024 along an axis, is doubled until it does not (one far
    outlier must not make a grid of 10^9 cells).  No answer depends on the pitch.  Raises SgnnError when the extent of
    the finite points overflows fp32."""

    def __init__(self, points, cell=None):
        n = _rows('points', points)
        if cell is not None:
            cell = _positive('cell', cell)
        dev = source_device(points)
        p = to_device(points, torch.float32, dev)
        lo = hi = np.zeros(3, F32)
        nfin = 0
        if n:
            finite = torch.isfinite(p).all(1, keepdim=True)
            inf = torch.full_like(p, float('inf'))
            stats = torch.cat([torch.where(finite, p, inf).amin(0).double(), torch.where(finite, p, -inf).amax(0).double(),
                               finite.sum().double().reshape(1)]).tolist()      # the one read-back
            nfin = int(stats[6])
            if nfin:
                lo, hi = np.array(stats[:3], F32), np.array(stats[3:6], F32)
                with np.errstate(over='ignore'):
                    if not np.isfinite(hi - lo).all():
                        raise _lib.SgnnError('the extent of the points does not fit fp32')
        self.cell, self.dims = fit_cell(default_cell(lo, hi, nfin) if cell is None else cell, lo, hi, nfin)
        self.n, self.nfin, self.device, self.points, self.lo, self.hi = n, nfin, dev, p, lo, hi
        ncell = self.dims[0] * self.dims[1] * self.dims[2]
        self.packed = torch.empty((max(nfin, 1), 4), dtype=torch.float32, device=dev)
        self.start = torch.empty(ncell + 1, dtype=torch.int32, device=dev)
        keys = self._keys(p, n)
        _lib.call('sgnn_cloud_pack', _lib.ptr(p), n, _lib.ptr(keys), nfin, ncell, _lib.ptr(self.packed),
                  _lib.ptr(self.start))

    def _grid(self):
        return (float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), float(self.cell)) + self.dims

    def _keys(self, rows, n):
        """The sorted (cell << 32 | row) keys of n rows: cell order, non-finite rows last."""
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        if n == 0:
            return keys
        _lib.call('sgnn_cloud_keys', _lib.ptr(rows), n, *self._grid(), _lib.ptr(keys))
        return torch.sort(keys).values

    def _index_args(self):
        return (_lib.ptr(self.packed), self.nfin, _lib.ptr(self.start)) + self._grid()

    def _queries(self, queries):
        q = to_device(queries, torch.float32, self.device)
        nq = int(q.shape[0])
        return q, nq, self._keys(q, nq)

    def knn(self, queries, k, max_dist=None):
        """(idx (Q, k) int32, d2 (Q, k) fp32): for every query the first k of the finite indexed points ordered by
        (d2, index), d2 = (dx dx + dy dy) + dz dz in fp32, restricted to d2 <= max_dist * max_dist (the fp32 product)
        when max_dist is given; -1 and +inf where there are fewer.  queries=None: the indexed points themselves, each
        without its own row (duplicates of it stay, at d2 = 0)."""
        k = _k(k)
        if queries is not None:
            _rows('queries', queries)
        limit2 = _limit2('max_dist', max_dist)
        dev = self.device
        if queries is None:
            nq, q, qkeys, rows = self.nfin, None, None, self.n
        else:
            q, nq, qkeys = self._queries(queries)
            rows = nq
        idx = torch.empty((rows, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((rows, k), dtype=torch.float32, device=dev)
        if queries is None and self.nfin < self.n:      # the rows of the non-finite points
            idx.fill_(-1)
            d2.fill_(float('inf'))
        if nq:
            _lib.call('sgnn_cloud_knn', *self._index_args(), _lib.ptr(q), _lib.ptr(qkeys), nq, rows, k, limit2,
                      _lib.ptr(idx), _lib.ptr(d2))
        return idx, d2

    def nearest(self, queries, max_dist=None):
        """(d (Q,) fp32, idx (Q,) int32): the distance to the nearest indexed point, the correctly rounded root of d2,
        and that point; +inf and -1 where there is none within max_dist.  Like TriangleIndex.distance."""
        idx, d2 = self.knn(queries, 1, max_dist)
        return _mean_dist(idx, d2).float(), idx.reshape(-1)

    def radius_count(self, queries, radius):
        """(Q,) int32: the indexed points with d2 <= radius * radius (the fp32 product); a query that is an indexed
        point counts itself."""
        return self._radius(queries, radius)[0]

    def _radius(self, queries, radius):
        _rows('queries', queries)
        limit2 = _limit2('radius', radius)
        q, nq, qkeys = self._queries(queries)
        cnt = torch.empty(nq, dtype=torch.int32, device=self.device)
        if nq:
            _lib.call('sgnn_cloud_radius_count', *self._index_args(), _lib.ptr(q), _lib.ptr(qkeys), nq, limit2,
                      _lib.ptr(cnt))
        return cnt, q, nq, qkeys, limit2

    def radius(self, queries, radius):
        """CSR lists (start (Q+1,) int64, nbr (M,) int32): the indexed points with d2 <= radius * radius of query q are
        nbr[start[q]:start[q+1]], ascending."""
        cnt, q, nq, qkeys, limit2 = self._radius(queries, radius)
        start = torch.zeros(nq + 1, dtype=torch.int64, device=self.device)
        if nq:
            torch.cumsum(cnt, 0, out=start[1:])
        total = int(start[-1].item())
        if total >= LIMIT:
            raise ValueError('%d neighbours do not fit 31 bits: choose a smaller radius' % total)
        out = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
        if total:
            _lib.call('sgnn_cloud_radius_fill', *self._index_args(), _lib.ptr(q), _lib.ptr(qkeys), nq, limit2,
                      _lib.ptr(start), _lib.ptr(out))
            out = torch.sort(out).values
        return start, (out[:total] & 0xFFFFFFFF).to(torch.int32)


def _mean_dist(idx, d2):
    """sgnn_cloud_mean_dist: (N,) fp64 mean of the fp32 roots of every row of a knn answer, +inf for an empty row."""
    n, k = int(idx.shape[0]), int(idx.shape[1])
    mean = torch.empty(n, dtype=torch.float64, device=idx.device)
    if n:
        _lib.call('sgnn_cloud_mean_dist', _lib.ptr(idx), _lib.ptr(d2), n, k, _lib.ptr(mean))
    return mean


def _index(index, n, points):
    """index as a PointIndex over n points: itself, or built from the points."""
    if index is None:
        return PointIndex(points)
    return index


def _check_index(index, n):
    if index is not None and not (isinstance(index, PointIndex) and index.n == n):
        raise ValueError('index must be a PointIndex over the same %d points' % n)


def normals(points, k=16, max_dist=None, toward=None, index=None):
    """Normals(normal (N, 3) fp32 unit or 0, variation (N,) fp32, valid (N,) bool) by PCA over every point and its k
    nearest neighbours within max_dist (rule C.3): the eigenvector of the smallest eigenvalue of their fp64 covariance
    and variation = that eigenvalue over the trace (0 on a plane, 1/3 at most).  valid needs two neighbours and a
    positive trace.  toward: one viewpoint (3,) or one per point (N, 3) that the normals face; without it the component
    of largest magnitude is made positive, which is no consistent orientation.  index: the PointIndex of points."""
    n = _rows('points', points)
    k = _k(k)
    _limit2('max_dist', max_dist)
    mode = 0
    if toward is not None:
        shape = tuple(np.shape(toward))
        if shape != (3,) and shape != (n, 3):
            raise ValueError('toward must be (3,) or (%d, 3), got %s' % (n, shape))
        mode = 1 if shape == (3,) else 2
    _check_index(index, n)
    index = _index(index, n, points)
    dev = index.device
    idx, _ = index.knn(None, k, max_dist)
    tw = None if toward is None else to_device(toward, torch.float32, dev)
    normal = torch.empty((n, 3), dtype=torch.float32, device=dev)
    variation = torch.empty(n, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        _lib.call('sgnn_cloud_normals', _lib.ptr(index.points), n, _lib.ptr(idx), k, _lib.ptr(tw), mode, _lib.ptr(normal),
                  _lib.ptr(variation), _lib.ptr(valid))
    return Normals(normal, variation, valid.bool())


def statistical_outliers(points, k=16, std_ratio=2.0, index=None):
    """(keep (N,) bool, mean_d (N,) fp64, thr): mean_d is every point's mean distance to its k nearest neighbours
    (+inf without one), thr = mean + std_ratio * population standard deviation of the finite mean_d (fp64, on the
    device; NaN when there is none), keep = mean_d <= thr (rule C.4)."""
    n = _rows('points', points)
    k = _k(k)
    ratio = float(std_ratio)
    if not np.isfinite(ratio):
        raise ValueError('std_ratio must be finite, got %r' % (std_ratio,))
    _check_index(index, n)
    index = _index(index, n, points)
    mean_d = _mean_dist(*index.knn(None, k))
    fin = mean_d[torch.isfinite(mean_d)]
    thr = float((fin.mean() + ratio * fin.std(unbiased=False)).item()) if fin.numel() else float('nan')
    return mean_d <= thr, mean_d, thr


def radius_outliers(points, radius, min_neighbors, index=None):
    """(N,) bool: the points with at least min_neighbors other points within radius, radius_count(points, radius) - 1 >=
    min_neighbors (the count includes the point itself; a non-finite row counts nothing and is dropped)."""
    n = _rows('points', points)
    _positive('radius', radius)
    if isinstance(min_neighbors, bool) or int(min_neighbors) != min_neighbors or min_neighbors < 0:
        raise ValueError('min_neighbors must be a non-negative integer, got %r' % (min_neighbors,))
    _check_index(index, n)
    index = _index(index, n, points)
    return index.radius_count(index.points, radius) - 1 >= int(min_neighbors)


def voxel_downsample(points, cell, colors=None, normals=None):
    """One point per occupied cell of the world lattice of pitch cell (rule C.5), so that two clouds thin alike:
    Thinned(points (C, 3) fp32 the mean of the members, colors (C, 3 | 4) uint8 their rounded mean or None, normals
    (C, 3) fp32 the unit sum of theirs or None, count (C,) int32, first (C,) int32 the smallest member, cell_of (N,)
    int32 the output row of every input point, -1 for a non-finite one).  Rows are in ascending (z, y, x) cell order.
    A point at or beyond cell * 2^20 from the origin raises SgnnError."""
    n = _rows('points', points)
    cell = _positive('cell', cell)
    ncol = 0
    if colors is not None:
        if _rows('colors', colors, (3, 4)) != n:
            raise ValueError('colors must have %d rows, got %d' % (n, np.shape(colors)[0]))
        dtype = getattr(colors, 'dtype', None)
        if not (dtype is torch.uint8 or (not torch.is_tensor(colors) and dtype == np.uint8)):
            raise ValueError('colors must be uint8, got %s' % (dtype,))
        ncol = int(np.shape(colors)[1])
    if normals is not None and _rows('normals', normals) != n:
        raise ValueError('normals must have %d rows, got %d' % (n, np.shape(normals)[0]))
    dev = source_device(points, colors, normals)
    p = to_device(points, torch.float32, dev)
    col = None if colors is None else to_device(colors, torch.uint8, dev)
    nrm = None if normals is None else to_device(normals, torch.float32, dev)
    cell_of = torch.full((n,), -1, dtype=torch.int32, device=dev)
    nruns = nvalid = 0
    if n:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.call('sgnn_cloud_voxel_keys', _lib.ptr(p), n, float(cell), _lib.ptr(keys), _lib.ptr(status))
        keys, order = torch.sort(keys, stable=True)
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.call('sgnn_cloud_run_flags', _lib.ptr(keys), n, _lib.ptr(flags))
        sel, count = compact(flags, n, dev, read=False)
        nruns, nvalid, bad = torch.cat([count, (keys != 2 ** 63 - 1).sum().reshape(1), status.long()]).tolist()
        if bad & STATUS_RANGE:
            raise _lib.SgnnError('a point lies at or beyond cell * 2^20 = %g from the origin' % (float(cell) * VOXEL_LIMIT))
    out = Thinned(torch.empty((nruns, 3), dtype=torch.float32, device=dev),
                  None if col is None else torch.empty((nruns, ncol), dtype=torch.uint8, device=dev),
                  None if nrm is None else torch.empty((nruns, 3), dtype=torch.float32, device=dev),
                  torch.empty(nruns, dtype=torch.int32, device=dev), torch.empty(nruns, dtype=torch.int32, device=dev),
                  cell_of)
    if nruns:
        _lib.call('sgnn_cloud_voxel_reduce', _lib.ptr(p), n, _lib.ptr(col), ncol, _lib.ptr(nrm), _lib.ptr(order),
                  _lib.ptr(sel), nruns, nvalid, _lib.ptr(out.points), _lib.ptr(out.colors), _lib.ptr(out.normals),
                  _lib.ptr(out.count), _lib.ptr(out.first), _lib.ptr(cell_of))
    return out


def compare(pred_points, target_points, thresholds=(0.05,), max_dist=None):
    """Cloud-to-cloud comparison: the report of meshdist.summarise (accuracy, completeness, chamfer, precision, recall
    and fscore per threshold, the counts and the two distance tensors) from the nearest-neighbour distance of every
    pred point to the target points and of every target point to the pred points.  A non-finite row, and with max_dist
    a point farther than it, has the distance +inf."""
    from .meshdist import summarise
    _rows('pred_points', pred_points)
    _rows('target_points', target_points)
    _limit2('max_dist', max_dist)
    thresholds = tuple(float(t) for t in thresholds)
    dev = source_device(pred_points, target_points)
    pred = to_device(pred_points, torch.float32, dev)
    target = to_device(target_points, torch.float32, dev)
    d_pred = PointIndex(target).nearest(pred, max_dist)[0]
    d_target = PointIndex(pred).nearest(target, max_dist)[0]
    return summarise(d_pred, d_target, thresholds, max_dist)
