"""GPU: point-to-SDF registration (sgnn_amd.register, csrc/register.hip) against the NumPy restatement of
tests/register_ref.py: residuals and cells bit for bit, the sums of the Gauss-Newton systems within the derived bound of
INTEGRATION.md section R rule 7, and align / align_volumes against the accuracy the restatement reaches on the CPU
(tests/test_register_ref.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import register_ref as G  # noqa: E402

from sgnn_amd import fusion, regrid, register, voxelize  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@functools.lru_cache(maxsize=None)
def small():
    sdf, w2g = G.small_volume()
    return sdf, w2g, torch.from_numpy(sdf).cuda()


@functools.lru_cache(maxsize=None)
def expected(count):
    """The restatement for small_points(count) under each of small_transforms(): one reference, shared."""
    sdf, w2g, _ = small()
    pts = G.small_points(count)
    return pts, [G.terms(pts, sdf, w2g, T, G.SMALL_BAND) for T in G.small_transforms()]


def run(pts, Ts, **kw):
    sdf, w2g, dev_sdf = small()
    res = torch.empty((len(Ts), len(pts)), dtype=torch.float32, device='cuda')
    cell = torch.empty((len(Ts), len(pts)), dtype=torch.int32, device='cuda')
    out = register.normal_equations(pts, dev_sdf, w2g, np.stack(Ts), G.SMALL_BAND, residual=res, cell=cell, **kw)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(Ts), 32)
    return out.cpu().numpy(), res.cpu().numpy(), cell.cpu().numpy()


@pytest.mark.parametrize('count', [1, 63, 257, 70001])
def test_systems_against_the_restatement(count):
    """70 001 points are more than the 65 536 lanes of the largest grid: the stride loop takes a second trip."""
    pts, exp = expected(count)
    Ts = G.small_transforms()
    got, res, cell = run(pts, Ts)
    total = 0
    for b, (J, r, exp_res, exp_cell) in enumerate(exp):
        assert np.array_equal(res[b].view(np.int32), exp_res.view(np.int32)), 'record %d' % b    # NaN positions included
        assert np.array_equal(cell[b], exp_cell)
        table = G.term_table(J, r)
        exact, bound = G.system_from_terms(table), G.sum_bound(table)
        err = np.abs(got[b, :28] - exact[:28])
        print('P %d record %d: N = %d, worst error / bound = %.3g' % (count, b, len(r),
                                                                     (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (err, bound)
        assert got[b, 28] == len(r) and not got[b, 29:].any()
        total += len(r)
    assert not got[0].any() and np.isnan(res[0]).all() and (cell[0] == -1).all()          # the non-finite record
    if count >= 257:
        assert total > 0.5 * 3 * count and np.isnan(res[1:]).any()
    again = run(pts, Ts)
    assert np.array_equal(again[0].view(np.int64), got.view(np.int64))                    # the same bits on every call
    one, res1, cell1 = run(pts, Ts[1:2])
    assert np.array_equal(one[0].view(np.int64), got[1].view(np.int64))                   # B does not show in a record
    assert np.array_equal(res1[0].view(np.int32), res[1].view(np.int32)) and np.array_equal(cell1[0], cell[1])


def test_gates_and_input_kinds():
    pts, _ = expected(257)
    sdf, w2g, dev_sdf = small()
    T = G.small_transforms()[3]
    for kw in (dict(max_dist=0.4), dict(min_grad=7.9), dict(min_grad=0.0), dict(max_dist=0.4, min_grad=8.2)):
        J, r, exp_res, exp_cell = G.terms(pts, sdf, w2g, T, G.SMALL_BAND, **kw)
        got, res, cell = run(pts, [T], **kw)
        assert np.array_equal(res[0].view(np.int32), exp_res.view(np.int32)) and np.array_equal(cell[0], exp_cell)
        assert got[0, 28] == len(r)
        print('%s: %d of %d points pass' % (sorted(kw.items()), len(r), len(pts)))
    wide = G.terms(pts, sdf, w2g, T, G.SMALL_BAND)[1]
    assert 0 < len(G.terms(pts, sdf, w2g, T, G.SMALL_BAND, max_dist=0.4)[1]) < len(wide)   # both outcomes of a gate
    assert 0 < len(G.terms(pts, sdf, w2g, T, G.SMALL_BAND, min_grad=7.9)[1]) < len(wide)
    # host arrays, host tensors and device tensors, one matrix or a stack of one
    plain = register.normal_equations(pts, sdf, w2g, T, G.SMALL_BAND).cpu().numpy()
    assert plain.shape == (1, 32) and np.array_equal(plain, run(pts, [T])[0])
    t = torch.from_numpy
    assert np.array_equal(register.normal_equations(t(pts.copy()), t(sdf.copy()), t(w2g.copy()), t(T.copy())[None],
                                                    G.SMALL_BAND).cpu().numpy(), plain)
    assert np.array_equal(register.normal_equations(t(pts.copy()).cuda(), dev_sdf, w2g, T, G.SMALL_BAND).cpu().numpy(),
                          plain)
    assert tuple(register.normal_equations(pts[:0], dev_sdf, w2g, T, G.SMALL_BAND).shape) == (1, 32)
    assert tuple(register.normal_equations(pts, dev_sdf, w2g, np.zeros((0, 4, 4)), G.SMALL_BAND).shape) == (0, 32)


def test_surface_points_match_the_restatement():
    sdf, w2g, dev_sdf = small()
    for band, stride in ((G.SMALL_BAND, 1), (None, 3), (1.5, 2)):
        got = register.surface_points(dev_sdf, w2g, band=band, stride=stride)
        exp = G.surface_points(sdf, w2g, band, stride)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == exp.shape and len(exp) > 50
        assert np.array_equal(got.cpu().numpy().view(np.int32), exp.view(np.int32))
    vol = fusion.TSDFVolume(G.SMALL_DIMS, 0.125, w2g)
    vol.sdf().copy_(dev_sdf * 0.125)
    exp = G.surface_points(sdf * F32(0.125), w2g, F32(3.0) * F32(0.125), 2)
    assert np.array_equal(register.surface_points(vol, stride=2).cpu().numpy().view(np.int32), exp.view(np.int32))


@pytest.fixture(scope='module')
def room():
    sdf, w2g, src, centre = G.room_scene()
    vol = fusion.TSDFVolume((88, 72, 60), G.VS, w2g)
    vol.sdf().copy_(torch.from_numpy(sdf))
    return vol, sdf, w2g, src, centre


def test_align_on_a_perturbed_guess(room):
    """The same steps as the restatement, summed in another order: the same number of pairs at every iteration and a
    final transform within 1.5 times the error the restatement reaches on the CPU (register_ref.ALIGN_ERROR, the worst
    of seeds 0-3)."""
    vol, sdf, w2g, src, centre = room
    guess = G.perturbed(G.ROOM_TRUE, 0, centre, G.TRANS, G.ROT)
    exp = G.align(src, sdf, w2g, G.ROOM_BAND, guess)
    got = register.align(src, vol, guess)
    dt, dr = G.transform_error(G.ROOM_TRUE, got.T, centre)
    print('pairs %s ... %d rmse %.4g error %.4g m %.4g deg (restatement %.4g m %.4g deg)'
          % ((got.history[:3], got.pairs, got.rmse, dt, dr) + G.transform_error(G.ROOM_TRUE, exp.T, centre)))
    assert got.ok and exp.ok and len(got.history) == 30 and got.T.dtype == np.float64
    assert got.history == exp.history and got.pairs == exp.pairs
    assert dt <= 1.5 * G.ALIGN_ERROR[0] and dr <= 1.5 * G.ALIGN_ERROR[1]


def test_several_guesses_in_one_call(room):
    vol, sdf, w2g, src, centre = room
    off = np.eye(4)
    off[:3, 3] = [0.4, 0.0, 0.0]
    far = np.eye(4)
    far[:3, 3] = 100.0
    bad = np.full((4, 4), np.nan)
    guesses = np.stack([G.ROOM_TRUE, G.perturbed(G.ROOM_TRUE, 1, centre, G.TRANS, G.ROT), off @ G.ROOM_TRUE, far, bad])
    results = register.align(src, (vol.sdf(), w2g, G.ROOM_BAND), guesses, iterations=12)
    assert isinstance(results, list) and len(results) == 5
    exp = [G.align(src, sdf, w2g, G.ROOM_BAND, g, iterations=12) for g in guesses[:2]]
    for r, e in zip(results, exp):
        assert r.ok and r.history == e.history
    chosen = register.best(results)
    assert chosen is results[0] or chosen is results[1]
    for r, g in zip(results[3:], guesses[3:]):                              # no pairs, no transform: the guess comes back
        assert not r.ok and r.pairs == 0 and len(r.history) == 1 and np.array_equal(r.T, g, equal_nan=True)
    assert register.best(results[3:]) is None
    single = register.align(src, vol, guesses[1], iterations=12)            # B does not show in a guess's steps
    assert np.array_equal(single.T, results[1].T) and single.history == results[1].history


def test_align_volumes_apply_and_merge():
    """Two volumes voxelised from one box, the second moved by 2 cm and 1 degree.  The bound on the recovered transform is
    1.5 times what the restatement route reaches for this very pair on the CPU (register_ref.BOX_ERROR, held by
    tests/test_register_ref.py): the two volumes sample the box on different lattices, so rounding-level agreement, the
    room's figure, is not there to be had.  Then the registered merge against the merge with the true transform."""
    true = G.box_true()
    src = voxelize.mesh_to_volume(*G.box_mesh(), G.BOX_DIMS, G.BOX_VS, G.box_w2g(), band=G.BOX_VOX_BAND)
    dst = voxelize.mesh_to_volume(*G.box_mesh(true), G.BOX_DIMS, G.BOX_VS, G.box_w2g(), band=G.BOX_VOX_BAND)
    assert np.array_equal(src.sdf().cpu().numpy().view(np.int32), G.box_volume_ref().view(np.int32))
    res = register.align_volumes(src, dst, stride=G.BOX_STRIDE)
    centre = register.surface_points(src, stride=G.BOX_STRIDE).double().mean(0).cpu().numpy()
    dt, dr = G.transform_error(true, res.T, centre)
    print('align_volumes: %d pairs, rmse %.6f m, %.6f m %.5f deg from the true transform' % (res.pairs, res.rmse, dt, dr))
    assert res.ok and dt <= 1.5 * G.BOX_ERROR[0] and dr <= 1.5 * G.BOX_ERROR[1]
    moved = register.apply(src, res.T)
    assert np.array_equal(moved.world2grid, G.moved_world2grid(src.world2grid, res.T))
    assert moved.sdf().data_ptr() != src.sdf().data_ptr() and np.array_equal(src.world2grid, G.box_w2g())
    merged = {name: regrid.merge(dst.copy(), register.apply(src, T)) for name, T in
              (('true', true), ('recovered', res.T), ('identity', np.eye(4)))}
    ref = merged['true'].sdf()
    near = (merged['true'].weight() > 0) & (ref.abs() < float(G.BOX_VS))
    for m in merged.values():
        near &= (m.weight() > 0) & torch.isfinite(m.sdf())
    mean = {name: float((m.sdf()[near] - ref[near]).abs().mean()) for name, m in merged.items()}
    print('mean |sdf - sdf merged with the true transform| over %d near-surface voxels: %s' % (int(near.sum()), mean))
    assert int(near.sum()) > 500 and mean['recovered'] < mean['identity']


def test_argument_errors():
    pts, _ = expected(257)
    sdf, w2g, dev_sdf = small()
    T = np.eye(4)
    launches = register._lib.load().sgnn_launch_count
    before = launches()
    base = dict(points=pts, sdf=sdf, w2g=w2g, T=T, band=3.0, max_dist=None, min_grad=0.5)
    bad = [dict(points=pts[:, :2]), dict(points=pts[0]), dict(sdf=sdf[0]), dict(sdf=sdf[:1]), dict(w2g=w2g[:3]),
           dict(T=T[:3]), dict(T=np.zeros((2, 3, 4))), dict(band=0.0), dict(band=-1.0), dict(band=float('nan')),
           dict(max_dist=0.0), dict(max_dist=-0.5), dict(min_grad=-0.1)]
    for change in bad:
        a = dict(base, **change)
        with pytest.raises(ValueError):
            register.normal_equations(a['points'], a['sdf'], a['w2g'], a['T'], a['band'], a['max_dist'], a['min_grad'])
    with pytest.raises(ValueError):
        register.normal_equations(pts, sdf, w2g, T, 3.0, residual=torch.empty((1, 257), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        register.normal_equations(pts, sdf, w2g, T, 3.0, cell=torch.empty((2, 257), dtype=torch.int32, device='cuda'))
    vol = (dev_sdf, w2g, 3.0)
    for kw in (dict(iterations=0), dict(max_dist=0.0), dict(guess=np.eye(3)), dict(guess=np.zeros((2, 4, 3))),
               dict(min_grad=-1.0)):
        with pytest.raises(ValueError):
            register.align(pts, vol, **kw)
    for v in ((dev_sdf, w2g), (dev_sdf, w2g, 0.0), (dev_sdf[0], w2g, 3.0), 'volume'):
        with pytest.raises(ValueError):
            register.align(pts, v)
    with pytest.raises(ValueError):
        register.align(pts[:, :2], vol)
    for args, kw in (((dev_sdf,), {}), ((dev_sdf, w2g), dict(stride=0)), ((dev_sdf, w2g), dict(band=0.0)),
                     ((dev_sdf[0], w2g), {}), ((dev_sdf, np.zeros((4, 4))), {})):
        with pytest.raises(ValueError):
            register.surface_points(*args, **kw)
    tsdf = fusion.TSDFVolume(G.SMALL_DIMS, 0.125, w2g)
    with pytest.raises(ValueError):
        register.align_volumes((dev_sdf, w2g, 3.0), tsdf)
    with pytest.raises(ValueError):
        register.align_volumes(tsdf, tsdf, stride=0)
    for bad_T in (np.eye(3), np.zeros((4, 4)), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            register.apply(tsdf, bad_T)
    assert launches() == before                                             # raised before any launch
    register.normal_equations(pts, dev_sdf, w2g, T, 3.0)
    assert launches() > before
