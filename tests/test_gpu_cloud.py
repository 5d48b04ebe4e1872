"""sgnn_amd.cloud on the GPU against the brute-force host restatement tests/cloud_ref.py:
every neighbour index equal and every distance, normal, mean and voxel row equal bit for bit (floats compared as
integers), whatever the grid pitch; every call runs twice, the runs are equal and the inputs come back unchanged.
The point sets are the smallest at which the walk can go wrong: ties, duplicates, points on the binning borders, whole
rings of empty cells, a grid stretched by far outliers, fewer points than k, rows that are not finite."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as CR  # noqa: E402

from sgnn_amd import _lib, cloud, meshdist  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
KS = (1, 5, 8, 16, 32)
PITCH = F32(0.1)        # the pitch of the border set: not a power of two, so that i * PITCH is rounded


def raw(x):
    """The bits of an array: floats as integers of their width."""
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize]) if x.dtype.kind == 'f' else x


def same(got, want, what=''):
    assert torch.is_tensor(got) and got.is_cuda, what
    want = np.asarray(want)
    assert tuple(got.shape) == want.shape and got.cpu().numpy().dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    g, w = raw(got), raw(want)
    differ = np.nonzero((g != w).reshape(len(w), -1).any(1))[0] if len(w) else []
    assert len(differ) == 0, '%s: %d of %d rows differ, first %d: %r against %r' % (
        what, len(differ), len(w), differ[0], got[int(differ[0])].cpu().numpy(), want[differ[0]])


def run(fn, *args, **kw):
    """fn twice: the two results hold the same bits and the array arguments are unchanged.  Returns a tuple."""
    arrays = [a for a in list(args) + list(kw.values()) if isinstance(a, np.ndarray) or torch.is_tensor(a)]
    before = [a.clone() if torch.is_tensor(a) else a.copy() for a in arrays]
    a, b = fn(*args, **kw), fn(*args, **kw)
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert x.data_ptr() != y.data_ptr() or x.numel() == 0
            assert np.array_equal(raw(x), raw(y)), 'two runs differ'
        else:
            assert x == y or (x != x and y != y), 'two runs differ'
    for x, y in zip(arrays, before):
        assert np.array_equal(raw(x), raw(y)), 'an input was written'
    return a


def sets():
    rng = np.random.default_rng(2024)
    out = {}
    out['uniform'] = rng.uniform(0, 1, (1500, 3)).astype(F32)
    g = np.arange(9, dtype=F32)
    out['lattice'] = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    out['duplicates'] = np.tile(rng.uniform(-1, 1, (300, 3)).astype(F32), (3, 1))[rng.permutation(900)]
    edge = np.array([F32(i) * PITCH for i in range(7)], F32)
    values = np.unique(np.concatenate([edge, np.nextafter(edge, F32(10)), np.nextafter(edge[1:], F32(-10))]))
    border = values[rng.integers(0, len(values), (420, 3))]
    border[0] = 0
    out['borders'] = border.astype(F32)
    out['plane'] = np.concatenate([rng.uniform(-2, 2, (600, 2)), rng.normal(0, 0.004, (600, 1))], 1).astype(F32)
    far = np.array([[50, 0, 0], [0, -50, 3], [-30, 30, 30]], F32)
    out['clustered'] = np.concatenate([rng.normal(0, 0.1, (1000, 3)).astype(F32), far])
    holes = rng.uniform(0, 1, (400, 3)).astype(F32)
    holes[rng.permutation(400)[:20]] = np.nan
    holes[7, 1] = np.inf
    out['holes'] = holes
    return out


SETS = sets()


def box(points):
    fin = points[np.isfinite(points).all(1)]
    if len(fin) == 0:
        return np.zeros(3, F32), np.ones(3, F32)
    return fin.min(0), fin.max(0)


def query_sets(points, seed):
    """Queries equal to the points, inside the box, and far outside it on every side and corner."""
    rng = np.random.default_rng(seed)
    lo, hi = box(points)
    ext = np.maximum(hi - lo, F32(1e-3))
    inside = (lo + rng.uniform(0, 1, (150, 3)) * ext).astype(F32)
    dirs = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if x or y or z], F32)
    mid = (lo + hi) / 2
    outside = np.concatenate([mid + dirs * ext * F32(0.75), mid + dirs * ext * F32(40)]).astype(F32)
    return {'points': points, 'inside': inside, 'outside': outside}


def cells_of(points):
    lo, hi = box(points)
    ext = float(max((hi - lo).max(), 1e-3))
    n = max(len(points), 1)
    return (None, ext * 1e-5, ext / n ** (1 / 3), ext * 4)


@functools.lru_cache(maxsize=None)
def reference(name, qname, max_dist):
    """The restatement at k = 32, whose first k columns are its answer at k (it sorts all keys and cuts)."""
    points = SETS[name]
    queries = None if qname is None else query_sets(points, 5)[qname]
    return CR.knn(points, queries, 32, max_dist)


def spacing(points):
    """The median distance to the nearest other point."""
    d2 = CR.knn(points, None, 1)[1][:, 0]
    return float(np.sqrt(np.median(d2[np.isfinite(d2)])))


@pytest.mark.parametrize('name', sorted(SETS))
def test_knn_is_the_brute_force_answer_at_every_pitch(name):
    points = SETS[name]
    dev_points = torch.from_numpy(points).cuda()
    queries = query_sets(points, 5)
    s = spacing(points)
    pitches = cells_of(points) + ((PITCH,) if name == 'borders' else ())
    indexes = [cloud.PointIndex(dev_points if i & 1 else points, cell=c) for i, c in enumerate(pitches)]
    assert indexes[1].cell > F32(pitches[1]), 'the small pitch was not enlarged'
    assert indexes[3].dims == (1, 1, 1)
    for index in indexes:
        assert max(index.dims) <= 1024 and np.prod(index.dims) <= cloud.max_cells(index.nfin)
    for max_dist in (None, 2.5 * s, 1e-3 * s if s > 0 else 0.0):
        for qname in (None, 'points', 'inside', 'outside'):
            want_idx, want_d2 = reference(name, qname, max_dist)
            q = None if qname is None else queries[qname]
            for index in indexes:
                for k in KS:
                    what = '%s %s k=%d max_dist=%r cell=%r' % (name, qname, k, max_dist, index.cell)
                    idx, d2 = run(index.knn, q, k, max_dist=max_dist)
                    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
                    same(idx, want_idx[:, :k], what + ' idx')
                    same(d2, want_d2[:, :k], what + ' d2')
    if name in ('uniform', 'holes'):
        for index in indexes[:2]:
            d, idx = run(index.nearest, queries['inside'], max_dist=2.5 * s)
            want_d, want_idx = CR.nearest(points, queries['inside'], 2.5 * s)
            same(d, want_d, name + ' nearest d')
            same(idx, want_idx, name + ' nearest idx')


@pytest.mark.parametrize('k', KS)
def test_fewer_points_than_k(k):
    rng = np.random.default_rng(k)
    queries = rng.uniform(-1, 2, (40, 3)).astype(F32)
    for n in (0, 1, 2, k, k + 1):
        points = rng.uniform(0, 1, (n, 3)).astype(F32)
        for cell in (None, 0.01, 10.0):
            index = cloud.PointIndex(points, cell=cell)
            for q in (None, points, queries):
                for max_dist in (None, 0.5):
                    idx, d2 = run(index.knn, q, k, max_dist=max_dist)
                    want_idx, want_d2 = CR.knn(points, q, k, max_dist)
                    same(idx, want_idx, 'n=%d k=%d idx' % (n, k))
                    same(d2, want_d2, 'n=%d k=%d d2' % (n, k))
        res = run(cloud.normals, points, k=k)
        for got, want in zip(res, CR.normals(points, k=k)):
            same(got, want, 'n=%d normals' % n)
        if n < 3:
            assert not res[2].any() and not res[0].any()


@pytest.mark.parametrize('name,radii', [('lattice', (0.0, 2.0, 3.0, 100.0)), ('uniform', (0.0, 0.11, 7.0)),
                                        ('holes', (0.2,)), ('clustered', (0.05, 60.0))])
def test_radius_counts_and_lists(name, radii):
    points = SETS[name]
    queries = query_sets(points, 9)
    for cell in cells_of(points)[:3]:
        index = cloud.PointIndex(points, cell=cell)
        for qname in ('points', 'inside', 'outside'):
            q = queries[qname][:300]
            for radius in radii:
                what = '%s %s radius=%r cell=%r' % (name, qname, radius, index.cell)
                want_cnt, want_start, want_nbr = CR.radius(points, q, radius)
                (cnt,) = run(index.radius_count, q, radius)
                same(cnt, want_cnt, what + ' count')
                start, nbr = run(index.radius, q, radius)
                assert start.dtype == torch.int64 and nbr.dtype == torch.int32 and int(start[-1]) == len(nbr)
                same(start, want_start, what + ' start')
                same(nbr, want_nbr, what + ' nbr')
    if name == 'lattice':      # the <= edge: the six points at the exact distance 2 are in
        index = cloud.PointIndex(points)
        centre = np.array([[4, 4, 4]], F32)
        assert int(index.radius_count(centre, 2.0)[0]) == 33 and int(index.radius_count(centre, 0.0)[0]) == 1
        assert int(index.radius_count(centre, np.nextafter(F32(2), F32(0)))[0]) == 27


def sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (np.array([3, -2, 1]) + v * (1 + rng.normal(0, 0.002, (n, 1)))).astype(F32)


def test_normals():
    shell = sphere(700, 1)
    centre = np.array([3, -2, 1], F32)
    eyes = (shell + np.random.default_rng(2).normal(0, 1, shell.shape)).astype(F32)
    cases = [('plane', SETS['plane'], dict(k=16)), ('plane k=5', SETS['plane'], dict(k=5, max_dist=0.4)),
             ('shell to centre', shell, dict(k=16, toward=centre)), ('shell per point', shell, dict(k=12, toward=eyes)),
             ('lattice', SETS['lattice'], dict(k=16)), ('lattice k=6', SETS['lattice'], dict(k=6)),
             ('holes', SETS['holes'], dict(k=8, toward=np.zeros(3, F32))),
             ('duplicates', SETS['duplicates'], dict(k=2))]
    for what, points, kw in cases:
        res = run(cloud.normals, points, **kw)
        assert isinstance(res, cloud.Normals) and res.valid.dtype == torch.bool
        want = CR.normals(points, **kw)
        for got, ref, part in zip(res, want, ('normal', 'variation', 'valid')):
            same(got, ref, what + ' ' + part)
    index = cloud.PointIndex(torch.from_numpy(shell).cuda(), cell=0.3)
    res = cloud.normals(shell, k=16, toward=centre, index=index)
    same(res.normal, CR.normals(shell, k=16, toward=centre)[0], 'normals with an index')
    n = res.normal.cpu().numpy().astype(np.float64)
    inward = centre.astype(np.float64) - shell
    assert res.valid.all() and ((n * inward).sum(1) > 0.9 * np.linalg.norm(inward, axis=1)).all()
    plane = cloud.normals(SETS['plane'], k=16)
    assert (plane.normal[:, 2] > 0.9).all() and (plane.variation < 0.01).all()


def test_outlier_filters():
    points = SETS['clustered']
    for k, ratio in ((16, 2.0), (5, 1.0)):
        keep, mean_d, thr = run(cloud.statistical_outliers, points, k=k, std_ratio=ratio)
        want = CR.mean_dist(*CR.knn(points, None, k))
        assert mean_d.dtype == torch.float64 and keep.dtype == torch.bool and isinstance(thr, float)
        same(mean_d, want, 'mean_d')
        fin = want[np.isfinite(want)]
        want_thr = fin.mean() + ratio * fin.std()
        assert abs(thr - want_thr) <= 1e-12 * abs(want_thr)
        assert np.array_equal(keep.cpu().numpy(), want <= thr)
        assert not keep[-3:].any()
        assert keep.cpu().numpy()[:1000][want[:1000] <= fin.mean() + fin.std()].all()
    holes = SETS['holes']
    keep, mean_d, thr = run(cloud.statistical_outliers, holes, k=4, index=cloud.PointIndex(holes, cell=0.5))
    want = CR.mean_dist(*CR.knn(holes, None, 4))
    same(mean_d, want, 'mean_d with holes')
    assert np.isinf(want).sum() == (~CR.finite_rows(holes)).sum() >= 20 and np.array_equal(keep.cpu().numpy(), want <= thr)
    for pts in (points, holes):
        (keep,) = run(cloud.radius_outliers, pts, 0.08, 4)
        assert np.array_equal(keep.cpu().numpy(), CR.radius(pts, pts, 0.08)[0] - 1 >= 4)
    assert not cloud.radius_outliers(points, 1.0, 1)[-3:].any() and cloud.radius_outliers(points, 1.0, 1)[:1000].all()


@pytest.mark.parametrize('ncol', [0, 3, 4])
def test_voxel_downsample(ncol):
    rng = np.random.default_rng(30 + ncol)
    points = np.concatenate([rng.uniform(-3, 3, (2000, 3)), rng.uniform(10.01, 10.49, (1000, 3)),
                             rng.uniform(-7.49, -7.01, (200, 3))]).astype(F32)[rng.permutation(3200)]
    points[rng.permutation(3200)[:40]] = np.nan
    colors = rng.integers(0, 256, (3200, ncol)).astype(np.uint8) if ncol else None
    nrm = rng.normal(size=(3200, 3)).astype(F32) if ncol != 3 else None
    if nrm is not None:
        nrm[:50] = 0
    res = run(cloud.voxel_downsample, points, 0.5, colors=colors, normals=nrm)
    assert isinstance(res, cloud.Thinned)
    want = CR.voxel_downsample(points, 0.5, colors, nrm)
    assert want[3].max() >= 900, 'no cell for the spread reduction'
    for got, ref, part in zip(res, want, cloud.Thinned._fields):
        if ref is None:
            assert got is None
        else:
            same(got, ref, part)
    dev = run(cloud.voxel_downsample, torch.from_numpy(points).cuda(), np.float32(0.37))
    for got, ref, part in zip(dev, CR.voxel_downsample(points, 0.37), cloud.Thinned._fields):
        assert (got is None) if ref is None else (same(got, ref, part) is None)
    empty = cloud.voxel_downsample(points[:0], 0.5)
    assert empty.points.shape == (0, 3) and empty.cell_of.shape == (0,)
    edge = np.array([[0, 0, 0], [0, 0.25 * (2 ** 20 - 1), 0]], F32)
    assert cloud.voxel_downsample(edge, 0.25).points.shape == (2, 3)
    for bad in (0.25 * 2 ** 20, -0.25 * 2 ** 20, 3e9):
        edge[1, 1] = bad
        assert CR.voxel_downsample(edge, 0.25) == 'range'
        with pytest.raises(_lib.SgnnError):
            cloud.voxel_downsample(edge, 0.25)


def test_compare():
    a = SETS['lattice']
    rep = cloud.compare(a, a, thresholds=(0.05, 0.5))
    assert rep['accuracy'] == 0 and rep['completeness'] == 0 and rep['chamfer'] == 0
    assert rep['fscore'] == [1.0, 1.0] and not rep['pred_to_target'].any() and not rep['target_to_pred'].any()
    b = (a + np.array([0.25, 0, 3], F32)).astype(F32)
    for max_dist in (None, 1.5):
        rep = cloud.compare(torch.from_numpy(a).cuda(), b, thresholds=(0.25, 0.3), max_dist=max_dist)
        d_pred, d_target = CR.nearest(b, a, max_dist)[0], CR.nearest(a, b, max_dist)[0]
        same(rep['pred_to_target'], d_pred, 'pred_to_target')
        same(rep['target_to_pred'], d_target, 'target_to_pred')
        want = meshdist.summarise(torch.from_numpy(d_pred).cuda(), torch.from_numpy(d_target).cuda(), (0.25, 0.3),
                                  max_dist)
        for key in ('accuracy', 'completeness', 'chamfer', 'thresholds', 'hits_pred', 'hits_target', 'precision',
                    'recall', 'fscore'):
            assert rep[key] == want[key], key
        assert rep['hits_pred'][0] == 9 * 9 * 6 and rep['hits_pred'][0] == rep['hits_pred'][1]
