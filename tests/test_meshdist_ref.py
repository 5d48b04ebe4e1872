"""CPU: the NumPy restatement of the mesh-distance rules (tests/meshdist_ref.py) against
its fp64 twin, its shell walk against brute force, and the properties of the sampler."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshdist_ref as M  # noqa: E402

F32 = np.float32


def fp_bar(*arrays):
    """16 * 2^-24 * max |coordinate|: the rounding of one fp32 coordinate times a small constant (4.8e-6 at 5)."""
    return 16.0 * 2.0 ** -24 * max(float(np.abs(a[np.isfinite(a)]).max()) for a in arrays)


@pytest.mark.parametrize('seed,big', [(1, 0.0), (2, 0.1), (3, 0.6)])
def test_fp32_restatement_against_fp64_twin(seed, big):
    """800-triangle soups, 3 000 points 1 mm off the surface and a few hundred anywhere, coordinates in [-1, 5].
    Measured largest |d32 - d64| over the three cases: 3.4e-7 (bar 4.8e-6)."""
    verts, faces = M.clipped_soup(800, seed, big)
    rng = np.random.default_rng(seed)
    pts = np.concatenate([M.near_surface_points(verts, faces, 3000, seed), rng.uniform(-1, 5, (300, 3)).astype(F32)])
    pts = np.clip(pts, -1.0, 5.0)
    d32, f32 = M.distance_ref(pts, verts, faces)
    d64, f64 = M.distance_ref64(pts, verts, faces)
    err = np.abs(d32.astype(np.float64) - d64).max()
    bar = fp_bar(verts, pts)
    print('max |d32 - d64| = %.3g, bar %.3g, faces differ at %d of %d points' % (err, bar, (f32 != f64).sum(), len(pts)))
    assert bar <= 4.8e-6 and err <= bar
    assert (d32[:3000] < 1.01e-3).all() and (f32 >= 0).all()


def walk_case():
    verts, faces = M.clipped_soup(300, seed=4, big=0.05)
    faces = faces.copy()
    faces[7, 1] = faces[7, 0]                                                # ignored faces take part in no rule
    verts[3 * 11] = np.nan
    rng = np.random.default_rng(4)
    pts = np.concatenate([M.near_surface_points(verts, np.delete(faces, [7, 11], 0), 250, 4),
                          rng.uniform(-1, 5, (150, 3)), rng.uniform(-2, 6, (200, 3))]).astype(F32)
    pts[5] = np.nan
    pts[6, 1] = np.inf
    return verts, faces, pts


def test_shell_walk_equals_brute_force():
    verts, faces, pts = walk_case()
    d, f = M.distance_ref(pts, verts, faces)
    assert np.isinf(d[[5, 6]]).all() and (f[[5, 6]] == -1).all() and (np.delete(f, [5, 6]) >= 0).all()
    assert not np.isin(f, [7, 11]).any()
    seen = []
    for cell in (0.21, 100.0, 0.37, 1.3):
        grid = M.GridRef(verts, faces, cell)
        wd, wf, pairs, cells = M.walk_ref(pts, grid)
        assert np.array_equal(wd.view(np.int32), d.view(np.int32)) and np.array_equal(wf, f), cell
        seen.append((grid.dims, pairs))
    assert seen[1][0] == (1, 1, 1) and seen[1][1] == (len(pts) - 2) * 298   # one cell: every point meets every face


@pytest.mark.parametrize('aspect', [1e2, 1e3, 1e4])
def test_slivers_keep_the_walk_conservative(aspect):
    """Rule 5 rests on this: the fp32 distance of rule 2 is never below the true one by more than 2^-20 m, however
    thin the triangle (above it, it may be: the region tests of a sliver go wrong by far more than rounding), and so
    the walk equals brute force on slivers too.  Measured d32 - d64 over the 600 points, smallest / largest:
    aspect 1e2 -8.7e-8 / 1.3e-7, 1e3 -6.6e-8 / 1.6e-3, 1e4 -9.0e-8 / 0.44."""
    verts, faces = M.sliver_soup(200, aspect, seed=int(aspect))
    rng = np.random.default_rng(9)
    pts = np.concatenate([M.near_surface_points(verts, faces, 300, 9, off=0.0), M.near_surface_points(verts, faces, 150, 10),
                          rng.uniform(-0.5, 4.5, (150, 3))]).astype(F32)
    d32, f32 = M.distance_ref(pts, verts, faces)
    d64, _ = M.distance_ref64(pts, verts, faces)
    lo, hi = M.grid_box(verts, faces)
    m = np.maximum(np.abs(pts - lo), np.abs(pts - hi)).max(1).astype(np.float64)
    diff = d32.astype(np.float64) - d64
    print('aspect %g: d32 - d64 from %.3g to %.3g' % (aspect, diff.min(), diff.max()))
    assert (diff >= -(2.0 ** -20) * m).all()
    for cell in (0.37, 1.3):
        wd, wf, _, _ = M.walk_ref(pts, M.GridRef(verts, faces, cell))
        assert np.array_equal(wd.view(np.int32), d32.view(np.int32)) and np.array_equal(wf, f32), cell


def test_shell_walk_with_max_dist():
    verts, faces, pts = walk_case()
    d, f = M.distance_ref(pts, verts, faces)
    grid = M.GridRef(verts, faces, 0.37)
    full = M.walk_ref(pts, grid)[2]
    for md in (0.0, 0.02, 0.5):
        ed, ef = M.distance_ref(pts, verts, faces, max_dist=md)
        keep = d <= F32(md)
        assert np.array_equal(ed[keep], d[keep]) and np.array_equal(ef[keep], f[keep])
        assert np.isinf(ed[~keep]).all() and (ef[~keep] == -1).all()
        wd, wf, pairs, _ = M.walk_ref(pts, grid, max_dist=md)
        assert np.array_equal(wd.view(np.int32), ed.view(np.int32)) and np.array_equal(wf, ef), md
        assert pairs < full


def test_pruning_case_needs_under_a_twentieth():
    """The rule itself, on the case the GPU test caps at P T / 10.  Measured: 557 026 pairs = P T / 760."""
    verts, faces, pts = M.pruning_case()
    assert len(faces) >= 20000 and len(pts) == 20000
    grid = M.GridRef(verts, faces, M.default_cell_ref(verts, faces))
    d, f, pairs, cells = M.walk_ref(pts, grid)
    print('pairs %d = P T / %.1f, cells %d, dims %s' % (pairs, len(pts) * len(faces) / pairs, cells, grid.dims))
    assert pairs < len(pts) * len(faces) / 20
    assert (d < 1.01e-3).all() and (f >= 0).all()


def sampler_case():
    verts, faces = M.clipped_soup(500, seed=6, big=0.1)
    faces = faces.copy()
    faces[10, 2] = faces[10, 0]
    faces[499, 1] = faces[499, 2]                                            # the last face is ignored: the clamp target moves
    return verts, faces


def test_sampler_counts_within_one():
    """Every per-face count is within +-1 of n area / A: all samples share one stratum offset u0, so a face whose
    interval of the cumulative table has length L strata catches floor(L) or ceil(L) of them."""
    verts, faces = sampler_case()
    area, cum = M.areas_ref(verts, faces)
    n = 7001
    _, fid = M.sample_ref(verts, faces, n, 3, cum)
    dev = np.abs(np.bincount(fid, minlength=len(faces)) - n * area / cum[-1])
    print('largest |count - n area / A| = %.3f, %d faces above 1' % (dev.max(), (dev > 1).sum()))
    assert dev.max() <= 1.0


def test_sampler_properties():
    verts, faces = sampler_case()
    area, cum = M.areas_ref(verts, faces)
    assert area[10] == 0 and area[499] == 0 and (np.delete(area, [10, 499]) > 0).all()
    n = 7001
    pts, fid = M.sample_ref(verts, faces, n, 3, cum)
    counts = np.bincount(fid, minlength=len(faces))
    assert np.abs(counts - n * area / cum[-1]).max() <= 1.0
    assert counts[10] == 0 and counts[499] == 0
    a, ab, ac, _ = M.pack_ref(verts, faces, np.float64)
    d = np.sqrt(M.tri_dist2(pts.astype(np.float64), a[fid], ab[fid], ac[fid]))
    print('largest distance of a sample from its face: %.3g, bar %.3g' % (d.max(), fp_bar(verts)))
    assert d.max() <= fp_bar(verts)
    again, fid2 = M.sample_ref(verts, faces, n, 3, cum)
    assert np.array_equal(again.view(np.int32), pts.view(np.int32)) and np.array_equal(fid, fid2)
    other, _ = M.sample_ref(verts, faces, n, 4, cum)
    assert (other != pts).any(1).mean() > 0.99
    m = M.fractions(3, 4096)
    assert m.min() >= 0 and m.max() < 1 << 24 and abs(m.mean() / 2 ** 24 - 0.5) < 0.02
    assert len(M.sample_ref(verts, faces, 0, 0, cum)[0]) == 0


def test_compare_ref_counts_and_means():
    d0 = np.array([0.0, 0.01, 0.05, 0.2, np.inf], F32)
    d1 = np.array([0.0, 0.06, 0.04, np.inf], F32)
    rep = M.compare_ref(d0, d1, thresholds=(0.05, 0.1), max_dist=0.5)
    assert rep['hits_pred'] == [3, 3] and rep['hits_target'] == [2, 3]
    assert rep['precision'] == [0.6, 0.6] and rep['recall'] == [0.5, 0.75]
    acc = (0.0 + float(F32(0.01)) + float(F32(0.05)) + float(F32(0.2)) + 0.5) / 5
    assert abs(rep['accuracy'] - acc) < 1e-15 and abs(rep['chamfer'] - rep['accuracy'] - rep['completeness']) < 1e-15
    assert abs(rep['fscore'][1] - 2 * 0.6 * 0.75 / 1.35) < 1e-15
