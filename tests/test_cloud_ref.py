"""tests/cloud_ref.py, the host restatement the GPU tests of sgnn_amd.cloud compare with bit for bit, held to things it
was not written from: a plain fp64 sort, numpy.linalg.eigh and a dictionary of lists.  No GPU."""
import numpy as np
import pytest

import cloud_ref as ref

F32 = np.float32


def _dyadic(rng, n, scale=1.0):
    """Points on multiples of 2^-10: differences, squares and their sums are exact in fp32 and in fp64 alike."""
    return (rng.integers(0, 1024, (n, 3)) / 1024.0 * scale).astype(F32)


@pytest.mark.parametrize('k', [1, 5, 32])
def test_knn_is_the_fp64_sort(k):
    rng = np.random.default_rng(k)
    pts, qs = _dyadic(rng, 400), _dyadic(rng, 90)
    idx, d2 = ref.knn(pts, qs, k)
    exact = ((qs[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(2)
    order = np.argsort(exact, axis=1, kind='stable')[:, :k]
    assert np.array_equal(idx, order)
    assert np.array_equal(d2.astype(np.float64), np.take_along_axis(exact, order, 1))
    own_idx, own_d2 = ref.knn(pts, None, k)
    exact = ((pts[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(2)
    exact[np.arange(len(pts)), np.arange(len(pts))] = np.inf
    order = np.argsort(exact, axis=1, kind='stable')[:, :k]
    assert np.array_equal(own_idx, order)
    assert np.array_equal(own_d2.astype(np.float64), np.take_along_axis(exact, order, 1))


def test_knn_bounds_rows_and_empty_slots():
    rng = np.random.default_rng(7)
    pts = _dyadic(rng, 50)
    pts[[3, 17]] = np.nan
    qs = np.concatenate([_dyadic(rng, 10), np.array([[np.inf, 0, 0]], F32)])
    idx, d2 = ref.knn(pts, qs, 8, max_dist=0.25)
    assert not np.isin(idx, [3, 17]).any()
    assert (idx[-1] == -1).all() and np.isinf(d2[-1]).all()
    assert ((d2 <= F32(0.25) * F32(0.25)) | (idx < 0)).all()
    assert (np.isinf(d2) == (idx < 0)).all()
    idx, d2 = ref.knn(pts[:4], None, 5)
    assert (idx[3] == -1).all() and sorted(idx[0][:2]) == [1, 2] and (idx[0][2:] == -1).all()
    cnt, start, nbr = ref.radius(pts, qs, 0.25)
    assert start[-1] == len(nbr) == cnt.sum() and cnt[-1] == 0
    for q in range(len(qs)):
        assert np.array_equal(nbr[start[q]:start[q + 1]], np.sort(idx_within(pts, qs[q], 0.25)))


def idx_within(pts, q, r):
    with np.errstate(invalid='ignore'):
        d2 = ref.dist2(q[None], pts)[0]
        return np.nonzero(d2 <= F32(r) * F32(r))[0]


def _neighbourhoods():
    """Noisy planes, offset by 100, exactly flat ones and anisotropic blobs: every one has a gap between its two
    smallest eigenvalues far above 1e-3 of the trace."""
    rng = np.random.default_rng(11)
    out = []
    for case in range(240):
        m = int(rng.integers(3, 34))
        rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        kind = case % 4
        if kind == 3:
            x = rng.normal(size=(m, 3)) * np.array([1.0, 0.55, 0.12])
            while np.linalg.matrix_rank(x - x.mean(0)) < 3:
                x = rng.normal(size=(m, 3)) * np.array([1.0, 0.55, 0.12])
        else:
            x = np.concatenate([rng.uniform(-1, 1, (m, 2)), rng.normal(size=(m, 1)) * (0.0 if kind == 2 else 0.01)], 1)
            x[:3, :2] = [[-1, -1], [1, -0.8], [0.1, 1]]      # never collinear
        x = x @ rot.T + (100.0 if kind == 1 else 0.0)
        out.append(x.astype(F32))
    return out


def test_eigenvalues_and_normals_are_those_of_eigh():
    worst_l = worst_n = 0.0
    for rows in _neighbourhoods():
        x = rows.astype(np.float64)
        cov = (x - x.mean(0)).T @ (x - x.mean(0))
        w, v = np.linalg.eigh(cov)
        trace = w.sum()
        assert (w[1] - w[0]) / trace > 1e-3
        normal, variation, lam = ref.normal_of(rows)
        worst_l = max(worst_l, np.abs(np.sort(lam) - w).max() / trace)
        worst_n = max(worst_n, np.linalg.norm(np.cross(normal, v[:, 0])))
        assert abs(np.linalg.norm(normal) - 1.0) < 1e-15
        assert abs(variation - max(w[0], 0.0) / trace) <= 1e-12
        big = int(np.argmax(np.abs(normal)))
        assert normal[big] > 0
        eye = x.mean(0) + 5.0 * v[:, 0]
        toward, _, _ = ref.normal_of(rows, eye.astype(F32))
        assert np.dot(toward, eye.astype(F32).astype(np.float64) - x[0]) >= 0
        assert np.allclose(np.abs(toward), np.abs(normal), atol=0, rtol=0)
    assert worst_l <= 1e-12, worst_l
    assert worst_n <= 1e-9, worst_n


def test_normals_need_two_neighbours_and_a_spread():
    pts = np.array([[0, 0, 0], [1, 0, 0]], F32)
    normal, variation, valid = ref.normals(pts, k=4)
    assert not valid.any() and not normal.any() and not variation.any()
    same = np.ones((5, 3), F32)
    normal, variation, valid = ref.normals(same, k=4)
    assert not valid.any() and not normal.any()
    rng = np.random.default_rng(3)
    plane = np.concatenate([rng.uniform(-1, 1, (60, 2)), np.zeros((60, 1))], 1).astype(F32)
    normal, variation, valid = ref.normals(plane, k=8)
    assert valid.all() and np.array_equal(normal, np.tile(F32([0, 0, 1]), (60, 1))) and (variation < 1e-12).all()


def test_mean_dist_is_the_mean_of_the_roots():
    rng = np.random.default_rng(5)
    pts = _dyadic(rng, 80)
    idx, d2 = ref.knn(pts, None, 6, max_dist=0.2)
    got = ref.mean_dist(idx, d2)
    for i in range(len(pts)):
        kk = (idx[i] >= 0).sum()
        if kk == 0:
            assert np.isinf(got[i])
        else:
            want = np.sqrt(d2[i, :kk].astype(np.float64)).astype(F32).astype(np.float64).mean()
            assert abs(got[i] - want) <= 1e-15 * want


def _dict_downsample(points, cell, colors, normals):
    cells = {}
    for i, p in enumerate(points):
        if np.isfinite(p).all():
            c = tuple(int(np.floor(F32(p[a]) / F32(cell))) for a in (2, 1, 0))
            cells.setdefault(c, []).append(i)
    rows = []
    for c in sorted(cells):
        m = cells[c]
        pos = np.zeros(3)
        for i in m:
            pos = pos + points[i].astype(np.float64)
        col = None if colors is None else [(2 * sum(int(colors[i][a]) for i in m) + len(m)) // (2 * len(m))
                                            for a in range(colors.shape[1])]
        nrm = None
        if normals is not None:
            nrm = np.zeros(3)
            for i in m:
                nrm = nrm + normals[i].astype(np.float64)
            nrm = nrm / np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]) if nrm.any() else nrm
        rows.append((m, (pos / len(m)).astype(F32), col, nrm))
    return rows


@pytest.mark.parametrize('ncol', [0, 3, 4])
def test_voxel_downsample_is_the_dictionary_of_lists(ncol):
    rng = np.random.default_rng(20 + ncol)
    pts = rng.uniform(-2, 2, (500, 3)).astype(F32)
    pts[::50] = np.nan
    pts[5:8] = pts[4]
    colors = rng.integers(0, 256, (500, ncol)).astype(np.uint8) if ncol else None
    nrm = rng.normal(size=(500, 3)).astype(F32)
    nrm[10] = -nrm[11]
    pts[10] = pts[11]
    out_p, out_c, out_n, count, first, cell_of = ref.voxel_downsample(pts, 0.5, colors, nrm)
    rows = _dict_downsample(pts, 0.5, colors, nrm)
    assert len(rows) == len(count)
    for r, (members, pos, col, nr) in enumerate(rows):
        assert count[r] == len(members) and first[r] == members[0] and (cell_of[members] == r).all()
        assert np.array_equal(out_p[r], pos)
        if ncol:
            assert list(out_c[r]) == col
        assert np.array_equal(out_n[r], nr.astype(F32))
    assert (cell_of[::50] == -1).all() and (cell_of >= 0).sum() == count.sum()
    assert ref.voxel_downsample(np.array([[0, 0, 0.5 * 2 ** 20]], F32), 0.5) == 'range'
    assert ref.voxel_downsample(np.array([[0, 0, -0.5 * 2 ** 20]], F32), 0.5) == 'range'
    assert ref.voxel_downsample(np.array([[0, 0, 0.5 * (2 ** 20 - 1)]], F32), 0.5) != 'range'
