"""GPU: tracking with colour (sgnn_amd.track, csrc/track.hip) against the NumPy restatement
of tests/track_color_ref.py: intensities, residuals and cells bit for bit, the sums of the photometric systems within
the bound of section I rule 6, and align_color / track_sequence on the textured wall against the accuracy the
restatement reaches on the CPU (tests/test_track_color_ref.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402
import track_color_ref as TC  # noqa: E402
import track_ref as T  # noqa: E402

from sgnn_amd import fusion, track  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = 0.05
TRANS, ROT = T.TRANS, T.ROT
BAND = F32(3.0) * F32(VS)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == exp.shape
    g, e = bits(got), bits(exp)
    assert np.array_equal(g, e), '%d of %d values differ' % ((g != e).sum(), g.size)


def pattern(u, v):
    """A smooth intensity in [38, 218] over pixel coordinates."""
    return 128.0 + 50.0 * np.sin(0.45 * u + 0.2 * v) + 40.0 * np.sin(0.3 * v - 0.1 * u)


@functools.lru_cache(maxsize=None)
def pairs(hw, hw_model):
    """Three (live frame, model frame) pairs: test_gpu_track's room geometry (live frames rendered at hw, model frames
    cast by the restatement at hw_model from poses 3 cm and 1.5 degrees away), a smooth pattern as the model
    intensity, and the same pattern at the live frame's scale plus noise of 12 levels as the live intensity, so that
    residuals fall on both sides of the intensity gate.  3 % of either have no intensity, as have model pixels
    without a depth."""
    sdf, w2g = C.room_sdf(VS, 4, BAND)
    depth, k, poses = R.room_frames(3, hw, seed=1)
    _, km, _ = R.room_frames(3, hw_model, seed=1)
    model_poses = np.stack([T.perturbed(p, f, TRANS, ROT) for f, p in enumerate(poses)])
    md, mn = C.cast(sdf, w2g, VS, km, model_poses, hw_model, BAND, normals=True)
    Ts = np.stack([T.pair_matrix(m, p) for m, p in zip(model_poses, poses)])
    ln = np.stack([T.depth_normals(d, kk) for d, kk in zip(depth, k)])
    rng = np.random.default_rng(11)
    (h, w), (hm, wm) = hw, hw_model
    um, vm = np.meshgrid(np.arange(wm, dtype=np.float64), np.arange(hm, dtype=np.float64))
    ul, vl = np.meshgrid(np.arange(w) * (wm / w), np.arange(h) * (hm / h))
    mi = np.stack([pattern(um + 3 * f, vm) for f in range(3)]).astype(F32)
    li = np.stack([pattern(ul + 3 * f, vl) for f in range(3)]) + rng.normal(0, 12.0, (3, h, w))
    li = np.clip(li, 0, 255).astype(F32)
    mi[~np.isfinite(md) | (rng.random(mi.shape) < 0.03)] = np.nan
    li[rng.random(li.shape) < 0.03] = np.nan
    return dict(depth=depth, li=li, k=k, km=km, md=md, mn=mn, mi=mi, T=Ts, ln=ln)


def run(p, sel, **kw):
    """color_equations with both per-pixel outputs for the pairs `sel` -> (system on the host, residual, cell)."""
    sel = list(sel)
    h, w = p['depth'].shape[1:]
    res = torch.empty((len(sel), h, w), dtype=torch.float32, device='cuda')
    cell = torch.empty((len(sel), h, w), dtype=torch.int32, device='cuda')
    if 'live_normal' in kw:
        kw['live_normal'] = kw['live_normal'][sel]
    out = track.color_equations(p['depth'][sel], p['li'][sel], p['k'][sel], p['md'][sel], p['mn'][sel], p['mi'][sel],
                                p['km'][sel], p['T'][sel], residual=res, cell=cell, **kw)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(sel), 32)
    return out.cpu().numpy(), res, cell


def check_pair(p, f, got, res, cell, **kw):
    """One pair of a device result against rules T3-T5 -> (pixels that take part, the restatement's cells)."""
    if 'live_normal' in kw:
        kw['live_normal'] = kw['live_normal'][f]
    J, r, exp_res, exp_cell = TC.color_terms(p['depth'][f], p['li'][f], p['k'][f], p['md'][f], p['mn'][f], p['mi'][f],
                                             p['km'][f], p['T'][f], **kw)
    same(res, exp_res)                                                      # NaN positions included
    assert np.array_equal(cell.cpu().numpy(), exp_cell)
    table = T.term_table(J, r)
    exact, bound = T.system_from_terms(table), T.sum_bound(table)
    err = np.abs(got[:28] - exact[:28])
    print('pair %d: N = %d, worst error / bound = %.3g' % (f, len(r), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err, bound)
    assert got[28] == len(r) and not got[29:].any()
    return len(r), exp_cell


@pytest.mark.parametrize('hw,hw_model', [((5, 7), (5, 7)), ((37, 53), (24, 32)), ((48, 64), (48, 64)),
                                         ((260, 256), (48, 64))])
def test_systems_against_the_restatement(hw, hw_model):
    """(5, 7): one partial block; (37, 53): a tail block and another model size; (260, 256): 66560 pixels for 256
    blocks of 256 lanes, so lanes walk twice.  Pair 1 has a T that is not finite."""
    p = dict(pairs(hw, hw_model))
    p['T'] = p['T'].copy()
    p['T'][1, 0, 1] = np.nan
    for kw in ({}, dict(live_normal=p['ln'], max_angle_deg=20.0)):
        got3, res3, cell3 = run(p, range(3), **dict(kw))
        counts = [check_pair(p, f, got3[f], res3[f], cell3[f], **dict(kw))[0] for f in range(3)]
        assert counts[1] == 0 and not got3[1].any()
        if hw[0] > 5:
            assert counts[0] + counts[2] > 0.25 * 2 * hw[0] * hw[1]
        again, res_again, cell_again = run(p, range(3), **dict(kw))
        assert np.array_equal(again.view(np.int64), got3.view(np.int64))   # the same bits on every call
        assert torch.equal(res_again.view(torch.int32), res3.view(torch.int32)) and torch.equal(cell_again, cell3)
        got1, res1, cell1 = run(p, [2], **dict(kw))
        assert np.array_equal(got1[0].view(np.int64), got3[2].view(np.int64))   # B does not show in a pair's bits
        assert torch.equal(res1[0].view(torch.int32), res3[2].view(torch.int32)) and torch.equal(cell1[0], cell3[2])
    # host arrays, host tensors and device tensors give the same system; the per-pixel outputs are optional
    t = torch.from_numpy
    args = [p['depth'], p['li'], p['k'], p['md'], p['mn'], p['mi'], p['km'], p['T']]
    plain = track.color_equations(*args).cpu().numpy()
    assert np.array_equal(plain, run(p, range(3))[0])
    assert np.array_equal(track.color_equations(*[t(a.copy()) for a in args]).cpu().numpy(), plain)
    assert np.array_equal(track.color_equations(*[t(a.copy()).cuda() for a in args]).cpu().numpy(), plain)


def test_gates():
    """Each gate of rule T3 and the intensity gate of T4 removes exactly the pixels the restatement removes."""
    base = pairs((48, 64), (48, 64))
    hm, wm = base['md'].shape[1:]
    clean = dict(base, li=np.where(np.isnan(base['li']), F32(100), base['li']),
                 mi=np.where(np.isnan(base['mi']) & np.isfinite(base['md']), F32(100), base['mi']))
    wide = dict(max_intensity=1000.0)

    def cells(p, **kw):
        got, res, cell = run(p, range(3), **dict(kw))
        return np.stack([check_pair(p, f, got[f], res[f], cell[f], **dict(kw))[1] for f in range(3)])

    all_in = cells(clean, **wide)
    n_all = (all_in >= 0).sum()
    assert n_all > 0.5 * all_in.size
    # a live intensity that is NaN: those pixels and no others
    holes = np.random.default_rng(3).random(clean['li'].shape) < 0.1
    got = cells(dict(clean, li=np.where(holes, F32(np.nan), clean['li'])), **wide)
    assert np.array_equal(got, np.where(holes, -1, all_in)) and (got >= 0).sum() < n_all
    # a model intensity that is NaN at one pixel: the (up to four) cells that have it as a corner
    v, u = 20, 30
    assert np.isfinite(clean['md'][:, v, u]).all()
    mi = clean['mi'].copy()
    mi[:, v, u] = np.nan
    touched = np.isin(all_in, [v * wm + u, v * wm + u - 1, (v - 1) * wm + u, (v - 1) * wm + u - 1])
    got = cells(dict(clean, mi=mi), **wide)
    assert touched.sum() > 0 and np.array_equal(got, np.where(touched, -1, all_in))
    # a corner whose depth is more than max_dist from the point's: the same cells (the association of rule 3 to that
    # pixel fails the distance gate of rule 4 as well, and those pixels are inside `touched`)
    md = clean['md'].copy()
    md[:, v, u] += F32(0.5)
    got = cells(dict(clean, md=md), **wide)
    assert np.array_equal(got, np.where(touched, -1, all_in))
    # the last row and column hold no cell, although rule 3 associates pixels there
    assoc = torch.empty((3, 48, 64), dtype=torch.int32, device='cuda')
    track.normal_equations(clean['depth'], clean['k'], clean['md'], clean['mn'], clean['km'], clean['T'], assoc=assoc)
    assoc = assoc.cpu().numpy()
    edge = (assoc >= 0) & ((assoc % wm == wm - 1) | (assoc // wm == hm - 1))
    used = all_in[all_in >= 0]
    assert edge.sum() > 0 and (used % wm < wm - 1).all() and (used // wm < hm - 1).all()
    assert (edge & (all_in < 0)).sum() > 0                                  # associated by rule 3, without a cell
    # the intensity gate: both outcomes occur
    tight = cells(base, max_intensity=10.0)
    loose = cells(base, **wide)
    n_tight, n_loose = (tight >= 0).sum(), (loose >= 0).sum()
    print('max_intensity 10: %d of %d pixels pass' % (n_tight, n_loose))
    assert 0.1 * n_loose < n_tight < 0.9 * n_loose and (loose[tight >= 0] == tight[tight >= 0]).all()
    # no live intensity at all
    got, res, cell = run(dict(base, li=np.full_like(base['li'], np.nan)), range(3))
    assert not got.any() and torch.isnan(res).all() and (cell == -1).all()


@pytest.mark.parametrize('hw', [(48, 64), (37, 53), (2, 2), (1, 3)])
def test_intensity_and_halve_intensity(hw):
    rng = np.random.default_rng(hw[0])
    rgba = rng.integers(0, 256, size=(3,) + hw + (4,), dtype=np.uint8)
    rgba[..., 3] = np.where(rng.random((3,) + hw) < 0.1, 0, rgba[..., 3])
    assert (rgba[..., 3] == 0).any() or hw[0] < 3
    exp = TC.intensity(rgba)
    got = track.intensity(rgba)
    same(got, exp)
    same(track.intensity(torch.from_numpy(rgba).cuda()), exp)
    same(track.intensity(rgba[0, 0, 0]), exp[0, 0, 0])
    assert tuple(track.intensity(rgba[:0]).shape) == (0,) + hw
    depth, k, _ = R.room_frames(3, hw, seed=2)
    depth = depth.copy()
    depth[rng.random(depth.shape) < 0.1] = -np.inf                          # holes
    for delta in (0.05, 0.2):
        half = track.halve_intensity(depth, exp, delta)
        assert tuple(half.shape) == (3, hw[0] // 2, hw[1] // 2)
        same(half, np.stack([TC.halve_intensity(d, c, delta) for d, c in zip(depth, exp)]))
    same(track.halve_intensity(torch.from_numpy(depth).cuda(), got),
         np.stack([TC.halve_intensity(d, c) for d, c in zip(depth, exp)]))


def wall_volume_on_device(grid):
    vol = fusion.TSDFVolume(TC.WALL_DIMS, TC.WALL_VS, grid.w2g, color=True)
    vol.sdf().copy_(torch.from_numpy(grid.sdf))
    vol._color.copy_(torch.from_numpy(grid.state().view(np.int16)))
    return vol


@pytest.fixture(scope='module')
def wall():
    grid = TC.wall_volume()
    return wall_volume_on_device(grid), grid


@pytest.mark.parametrize('seed', range(4))
def test_align_color_on_the_wall(wall, seed):
    """The same steps as the restatement, summed in another order: the same number of pairs at every iteration and a
    final pose within 1.5 times the error the restatement reaches on the CPU (track_color_ref.WALL_ALIGN_ERROR, the
    worst of seeds 0-3; section I's margin).  Geometry alone is lost on the same frame, or no closer along the wall."""
    vol, grid = wall
    depth, rgba, k, pose = TC.wall_view(seed)
    guess = T.perturbed(pose, seed, TRANS, ROT)
    exp = TC.align_color(depth, rgba, k, guess, guess, grid)
    got = track.align_color(depth, rgba, k, guess, guess, vol)
    dt, dr = T.pose_error(pose, got.pose)
    print('seed %d: pairs %s colour pairs %d rmse %.6f colour rmse %.3f error %.6f m %.5f deg (restatement %.6f m %.5f deg)'
          % ((seed, got.history, got.color_pairs, got.rmse, got.color_rmse, dt, dr) + T.pose_error(pose, exp.pose)))
    assert isinstance(got, track.ColorTrackResult) and got.ok and exp.ok and got.iterations == 19
    assert got.history == exp.history and got.pairs == exp.pairs and got.color_pairs == exp.color_pairs
    assert abs(got.color_rmse - exp.color_rmse) <= 1e-6 * exp.color_rmse
    assert dt <= 1.5 * TC.WALL_ALIGN_ERROR[0] and dr <= 1.5 * TC.WALL_ALIGN_ERROR[1]
    geo = track.align(depth, k, guess, guess, vol)
    assert not geo.ok or TC.in_plane_error(pose, geo.pose, TC.WALL_NORMAL) >= TC.in_plane_error(pose, guess, TC.WALL_NORMAL)
    # colour frames without an alpha channel, on the device
    rgb = torch.from_numpy(rgba[..., :3].copy()).cuda()
    assert np.array_equal(track.align_color(torch.from_numpy(depth).cuda(), rgb, k, guess, guess, vol).pose, got.pose)


def test_track_sequence_on_the_wall():
    """Six wall frames tracked and fused with their colour into the empty volume: the drift at the last frame within
    1.5 times what the restatement and fusion_color_ref.ColorGrid reach on the CPU (WALL_SEQUENCE_DRIFT)."""
    depth, rgba, k, poses = TC.wall_sequence(6)
    w2g = TC.wall_grid().w2g
    vol = fusion.TSDFVolume(TC.WALL_DIMS, TC.WALL_VS, w2g, color=True)
    est, results = track.track_sequence(vol, depth, k[0], poses[0], color_frames=rgba)
    assert est.shape == (6, 4, 4) and est.dtype == np.float64 and np.array_equal(est[0], poses[0])
    assert all(isinstance(r, track.ColorTrackResult) for r in results)
    assert [r.ok for r in results] == [True] * 6 and all(np.array_equal(r.pose, e) for r, e in zip(results, est))
    dt, dr = T.pose_error(poses[5], est[5])
    print('drift at frame 5: %.6f m %.5f deg; pairs %s colour pairs %s' % (dt, dr, [r.pairs for r in results],
                                                                          [r.color_pairs for r in results]))
    assert dt <= 1.5 * TC.WALL_SEQUENCE_DRIFT[0] and dr <= 1.5 * TC.WALL_SEQUENCE_DRIFT[1]
    again = fusion.TSDFVolume(TC.WALL_DIMS, TC.WALL_VS, w2g, color=True).integrate(depth, k, est, color=rgba)
    assert torch.equal(again.sdf().view(torch.int32), vol.sdf().view(torch.int32))
    assert torch.equal(again.color_state().view(torch.int16), vol.color_state().view(torch.int16))   # frame 0 included
    # the same frames without colour: the depth-only route loses the wall at once and fuses frame 0 alone
    plain = fusion.TSDFVolume(TC.WALL_DIMS, TC.WALL_VS, w2g)
    _, lost = track.track_sequence(plain, depth, k[0], poses[0])
    assert [r.ok for r in lost] == [True] + [False] * 5 and all(type(r) is track.TrackResult for r in lost)


def test_argument_errors(wall):
    vol, _ = wall
    p = pairs((48, 64), (48, 64))
    launches = track._lib.load().sgnn_launch_count
    before = launches()
    base = dict(depth=p['depth'], li=p['li'], k=p['k'], md=p['md'], mn=p['mn'], mi=p['mi'], km=p['km'], T=p['T'],
                max_dist=0.1, max_angle_deg=20.0, max_intensity=40.0, live_normal=None)
    huge = np.broadcast_to(F32(1.0), (2, 1 << 15, 1 << 15))                 # B h w = 2^31, no memory behind it
    bad = [
        # normal_equations' own
        dict(depth=p['depth'][0]), dict(depth=p['depth'][:2]), dict(md=p['md'][:2]), dict(mn=p['mn'][..., :2]),
        dict(mn=p['mn'][:, :40]), dict(k=p['k'][:2]), dict(km=p['km'][:, :3]), dict(T=p['T'][:2]), dict(T=p['T'][0]),
        dict(max_dist=0.0), dict(max_dist=-0.1), dict(max_angle_deg=0.0), dict(max_angle_deg=-5.0),
        dict(live_normal=p['ln'][:2]), dict(live_normal=p['ln'][..., 0]), dict(depth=huge),
        # intensities that do not fit the depths, and the intensity gate
        dict(li=p['li'][:2]), dict(li=p['li'][:, :40]), dict(li=p['li'][0]), dict(mi=p['mi'][:2]),
        dict(mi=p['mi'][:, :, :60]), dict(mi=p['mn']), dict(max_intensity=0.0), dict(max_intensity=-1.0),
    ]
    for change in bad:
        a = dict(base)
        a.update(change)
        with pytest.raises(ValueError):
            track.color_equations(a['depth'], a['li'], a['k'], a['md'], a['mn'], a['mi'], a['km'], a['T'], a['max_dist'],
                                  a['max_angle_deg'], a['max_intensity'], a['live_normal'])
    args = (p['depth'], p['li'], p['k'], p['md'], p['mn'], p['mi'], p['km'], p['T'])
    with pytest.raises(ValueError):
        track.color_equations(*args, residual=torch.empty((3, 48, 64), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        track.color_equations(*args, cell=torch.empty((2, 48, 64), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        track.intensity(np.zeros((4, 4, 3), np.uint8))
    for a in ((p['depth'], p['li'][:2]), (p['depth'][0], p['li'][0]), (p['depth'], p['li'], 0.0), (p['depth'], p['li'], -1.0)):
        with pytest.raises(ValueError):
            track.halve_intensity(*a)
    depth, rgba, k, pose = TC.wall_view(0)
    plain = fusion.TSDFVolume(TC.WALL_DIMS, TC.WALL_VS, TC.wall_grid().w2g)
    with pytest.raises(ValueError):
        track.align_color(depth, rgba, k, pose, pose, plain)               # a volume without colour
    for kw in (dict(rgba=rgba[:40]), dict(rgba=rgba[..., :2]), dict(rgba=rgba[None]), dict(depth=depth[None]),
               dict(color_weight=0.0), dict(max_intensity=0.0), dict(iterations=()), dict(max_dist=0.0)):
        a = dict(depth=depth, rgba=rgba, color_weight=1e-3, max_intensity=40.0, iterations=(10, 5, 4), max_dist=0.1)
        a.update(kw)
        with pytest.raises(ValueError):
            track.align_color(a['depth'], a['rgba'], k, pose, pose, vol, color_weight=a['color_weight'],
                              max_intensity=a['max_intensity'], iterations=a['iterations'], max_dist=a['max_dist'])
    frames = np.stack([depth, depth])
    with pytest.raises(ValueError):
        track.track_sequence(plain, frames, k, pose, color_frames=np.stack([rgba, rgba]))
    with pytest.raises(ValueError):
        track.track_sequence(vol, frames, k, pose, color_frames=rgba[None])
    assert launches() == before                                             # raised before any launch
    track.color_equations(*args)
    assert launches() > before
