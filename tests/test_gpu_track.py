"""GPU: frame-to-model tracking (sgnn_amd.track, csrc/track.hip) against the NumPy restatement of tests/track_ref.py:
residuals, associations, pyramid levels and normals bit for bit, the sums of the Gauss-Newton systems within the
derived bound of INTEGRATION.md section I rule 6, and align / track_sequence against the accuracy the restatement
reaches on the CPU (tests/test_track_ref.py)."""
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
import track_ref as T  # noqa: E402

from sgnn_amd import fusion, track  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
VS = 0.05
TRANS, ROT, ALIGN_ERROR, SEQUENCE_DRIFT = T.TRANS, T.ROT, T.ALIGN_ERROR, T.SEQUENCE_DRIFT
BAND = F32(3.0) * F32(VS)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == exp.shape
    g, e = bits(got), bits(exp)
    assert np.array_equal(g, e), '%d of %d values differ' % ((g != e).sum(), g.size)


@functools.lru_cache(maxsize=None)
def room():
    return C.room_sdf(VS, 4, BAND)


@functools.lru_cache(maxsize=None)
def pairs(hw, hw_model):
    """Three (live frame, model frame) pairs of the room: live frames rendered at hw, model frames cast by the
    restatement at hw_model from poses 3 cm and 1.5 degrees away."""
    sdf, w2g = room()
    depth, k, poses = R.room_frames(3, hw, seed=1)
    _, km, _ = R.room_frames(3, hw_model, seed=1)
    model_poses = np.stack([T.perturbed(p, f, TRANS, ROT) for f, p in enumerate(poses)])
    md, mn = C.cast(sdf, w2g, VS, km, model_poses, hw_model, BAND, normals=True)
    Ts = np.stack([T.pair_matrix(m, p) for m, p in zip(model_poses, poses)])
    ln = np.stack([T.depth_normals(d, kk) for d, kk in zip(depth, k)])
    return dict(depth=depth, k=k, km=km, md=md, mn=mn, T=Ts, ln=ln)


def run(p, sel, **kw):
    """normal_equations with both per-pixel outputs for the pairs `sel` -> (system, residual, assoc) on the host."""
    sel = list(sel)
    h, w = p['depth'].shape[1:]
    res = torch.empty((len(sel), h, w), dtype=torch.float32, device='cuda')
    assoc = torch.empty((len(sel), h, w), dtype=torch.int32, device='cuda')
    if 'live_normal' in kw:
        kw['live_normal'] = kw['live_normal'][sel]
    out = track.normal_equations(p['depth'][sel], p['k'][sel], p['md'][sel], p['mn'][sel], p['km'][sel], p['T'][sel],
                                 residual=res, assoc=assoc, **kw)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(sel), 32)
    return out.cpu().numpy(), res, assoc


def check_pair(p, f, got, res, assoc, **kw):
    """One pair of a device result against rules 2-7."""
    if 'live_normal' in kw:
        kw['live_normal'] = kw['live_normal'][f]
    J, r, exp_res, exp_assoc = T.terms(p['depth'][f], p['k'][f], p['md'][f], p['mn'][f], p['km'][f], p['T'][f], **kw)
    same(res, exp_res)                                                      # NaN positions included
    assert np.array_equal(assoc.cpu().numpy(), exp_assoc)
    table = T.term_table(J, r)
    exact, bound = T.system_from_terms(table), T.sum_bound(table)
    err = np.abs(got[:28] - exact[:28])
    print('pair %d: N = %d, worst error / bound = %.3g' % (f, len(r), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err, bound)
    assert got[28] == len(r) and not got[29:].any()
    return len(r)


@pytest.mark.parametrize('hw,hw_model', [((48, 64), (48, 64)), ((37, 53), (37, 53)), ((1, 3), (1, 3)),
                                         ((37, 53), (48, 64))])
def test_systems_against_the_restatement(hw, hw_model):
    p = pairs(hw, hw_model)
    for kw in ({}, dict(live_normal=p['ln'], max_angle_deg=20.0)):
        got3, res3, assoc3 = run(p, range(3), **dict(kw))
        total = sum(check_pair(p, f, got3[f], res3[f], assoc3[f], **dict(kw)) for f in range(3))
        if hw[0] > 1:
            assert total > 0.5 * 3 * hw[0] * hw[1]
        again, res_again, _ = run(p, range(3), **dict(kw))
        assert np.array_equal(again.view(np.int64), got3.view(np.int64))   # the same bits on every call
        got1, res1, assoc1 = run(p, [0], **dict(kw))
        assert np.array_equal(got1[0].view(np.int64), got3[0].view(np.int64))   # B does not show in pair 0
        assert torch.equal(res1[0].view(torch.int32), res3[0].view(torch.int32)) and torch.equal(assoc1[0], assoc3[0])
    # host arrays, host tensors and device tensors give the same system
    t = torch.from_numpy
    args = [p['depth'], p['k'], p['md'], p['mn'], p['km'], p['T']]
    plain = track.normal_equations(*args).cpu().numpy()
    assert np.array_equal(plain, run(p, range(3))[0])
    assert np.array_equal(track.normal_equations(*[t(a.copy()) for a in args]).cpu().numpy(), plain)
    assert np.array_equal(track.normal_equations(*[t(a.copy()).cuda() for a in args]).cpu().numpy(), plain)


def test_gates():
    """A distance gate at 8 mm against guesses 3 cm off, and an angle gate at 2.5 degrees against pair matrices turned by
    a further 3 degrees about the camera's x axis (a normal turns by 3 degrees times the sine of its angle to that
    axis): the restatement passes some pixels and rejects others, and the device agrees pixel by pixel."""
    base = pairs((48, 64), (48, 64))
    turn = T.exp_se3([np.radians(3.0), 0, 0, 0, 0, 0])
    turned = dict(base, T=np.stack([turn @ m for m in base['T']]))
    for p, kw in ((base, dict(max_dist=0.008)), (turned, dict(max_dist=1.0, live_normal=base['ln'], max_angle_deg=2.5))):
        open_kw = dict(kw, max_dist=1.0, max_angle_deg=90.0)
        wide = sum(len(T.terms(p['depth'][f], p['k'][f], p['md'][f], p['mn'][f], p['km'][f], p['T'][f],
                               **dict(open_kw, **({'live_normal': p['ln'][f]} if 'live_normal' in kw else {})))[1])
                   for f in range(3))
        got, res, assoc = run(p, range(3), **dict(kw))
        n = sum(check_pair(p, f, got[f], res[f], assoc[f], **dict(kw)) for f in range(3))
        print('%s: %d of %d pixels pass' % (sorted(kw), n, wide))
        assert 0.25 * wide < n < 0.75 * wide                                # both outcomes of the gate occur
    p = base
    nan_normals = np.full_like(p['ln'], np.nan)                             # a NaN live normal fails the gate
    got, res, assoc = run(p, range(3), live_normal=nan_normals)
    assert not got.any() and torch.isnan(res).all() and (assoc == -1).all()


def test_degenerate_inputs():
    p = dict(pairs((48, 64), (48, 64)))
    sdf, w2g = room()
    empty = dict(p, depth=np.full_like(p['depth'], -np.inf))
    got, res, assoc = run(empty, range(3))
    assert not got.any() and torch.isnan(res).all() and (assoc == -1).all()
    bad = p['T'].copy()
    bad[1, 0, 1] = np.nan
    bad[2, 2, 3] = np.inf
    got, res, assoc = run(dict(p, T=bad), range(3))
    check_pair(p, 0, got[0], res[0], assoc[0])
    assert got[0, 28] > 0 and not got[1:].any() and torch.isnan(res[1:]).all() and (assoc[1:] == -1).all()
    # align: nothing to see, and no pose to start from
    dims, _, _ = C.room_grid(VS, 4)
    vol = fusion.TSDFVolume(dims, VS, w2g)
    vol.sdf().copy_(torch.from_numpy(sdf))
    _, k, poses = R.room_frames(1, (48, 64), seed=1)
    res = track.align(np.full((48, 64), -np.inf, F32), k[0], poses[0], poses[0], vol)
    assert not res.ok and res.pairs == 0 and res.iterations == 1 and np.array_equal(res.pose, poses[0])
    nan_pose = poses[0].copy()
    nan_pose[0, 0] = np.nan
    for model, guess in ((poses[0], nan_pose), (nan_pose, poses[0])):
        res = track.align(p['depth'][0], k[0], model, guess, vol)
        assert not res.ok and res.pairs == 0 and res.pose is not guess and np.array_equal(res.pose, guess, equal_nan=True)
    assert tuple(track.normal_equations(p['depth'][:0], p['k'][:0], p['md'][:0], p['mn'][:0], p['km'][:0],
                                        p['T'][:0]).shape) == (0, 32)


def test_a_frame_larger_than_the_grid():
    """64 x 4096 pixels are 1024 blocks' worth; the grid stops at 256, so every lane walks four pixels."""
    p = pairs((48, 64), (48, 64))
    hw = (64, 4096)
    k = np.array([[51.2 * 64, 51.2, (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0]], F32)   # the model's view, 64 columns a pixel
    _, _, poses = R.room_frames(3, (48, 64), seed=1)
    depth = R.render(k[0], poses[0], hw, R.ROOM_PLANES, R.ROOM_BOXES)[None]
    big = dict(depth=depth, k=k, km=p['km'][:1], md=p['md'][:1], mn=p['mn'][:1], T=p['T'][:1])
    got, res, assoc = run(big, [0])
    n = check_pair(big, 0, got[0], res[0], assoc[0])
    assert n > 0.5 * hw[0] * hw[1]
    assert np.array_equal(run(big, [0])[0].view(np.int64), got.view(np.int64))


@pytest.mark.parametrize('hw', [(48, 64), (37, 53), (2, 2), (1, 3)])
def test_halve_and_depth_normals(hw):
    depth, k, _ = R.room_frames(3, hw, seed=2)
    depth = depth.copy()
    rng = np.random.default_rng(5)
    depth[rng.random(depth.shape) < 0.1] = -np.inf                          # holes
    k = k * np.array([1.0, 1.1, 1.0, 0.9], F32)
    for delta in (0.05, 0.2):
        half, kh = track.halve(depth, k, delta)
        exp = [T.halve(d, kk, delta) for d, kk in zip(depth, k)]
        same(half, np.stack([e[0] for e in exp]))
        assert tuple(half.shape) == (3, hw[0] // 2, hw[1] // 2)
        assert kh.dtype == F32 and np.array_equal(kh, np.stack([e[1] for e in exp]))
        normal = track.depth_normals(depth, k, delta)
        exp_n = np.stack([T.depth_normals(d, kk, delta) for d, kk in zip(depth, k)])
        same(normal, exp_n)
        if min(hw) > 2:
            assert np.isnan(exp_n).any() and np.isfinite(exp_n).any() and (exp_n[np.isfinite(exp_n[..., 2]), 2] < 0).all()
    same(track.halve(torch.from_numpy(depth).cuda(), k[0])[0], np.stack([T.halve(d, k[0])[0] for d in depth]))
    assert np.array_equal(track.halve(depth, k[0])[1], T.halve(depth[0], k[0])[1])


@pytest.fixture(scope='module')
def room_volume():
    sdf, w2g = room()
    dims, _, _ = C.room_grid(VS, 4)
    vol = fusion.TSDFVolume(dims, VS, w2g)
    vol.sdf().copy_(torch.from_numpy(sdf))
    return vol, T.room_volume(VS)


@pytest.mark.parametrize('seed', range(4))
def test_align_on_perturbed_guesses(room_volume, seed):
    """The same steps as the restatement, summed in another order: the same number of pairs at every iteration, and a
    final pose within 1.5 times the error the restatement reaches on the CPU (track_ref.ALIGN_ERROR, the worst
    of seeds 0-3; the margin of section H's loop closure)."""
    vol, grid = room_volume
    depth, k, pose, f, cond = T.test_view(seed, (48, 64), grid)
    guess = T.perturbed(pose, seed, TRANS, ROT)
    exp = T.align(depth, k, guess, guess, grid)
    got = track.align(depth, k, guess, guess, vol)
    dt, dr = T.pose_error(pose, got.pose)
    print('seed %d frame %d: pairs %s rmse %.6f error %.6f m %.5f deg (restatement %.6f m %.5f deg)'
          % ((seed, f, got.history, got.rmse, dt, dr) + T.pose_error(pose, exp.pose)))
    assert got.ok and exp.ok and got.iterations == 19
    assert got.history == exp.history
    assert got.pairs == exp.pairs and abs(got.rmse - exp.rmse) <= 1e-6 * exp.rmse
    assert dt <= 1.5 * ALIGN_ERROR[0] and dr <= 1.5 * ALIGN_ERROR[1]


def test_track_sequence():
    """Six frames tracked and fused into the empty 88 x 72 x 60 volume: the drift at the last frame within 1.5 times
    what the restatement and fusion_ref.Grid reach on the CPU (track_ref.SEQUENCE_DRIFT)."""
    depth, k, poses = T.sequence_frames(6, (48, 64), T.SEQUENCE_SEED)
    dims, _, w2g = C.room_grid(VS, 4)
    assert dims == (88, 72, 60)
    vol = fusion.TSDFVolume(dims, VS, w2g)
    est, results = track.track_sequence(vol, depth, k[0], poses[0])
    assert est.shape == (6, 4, 4) and est.dtype == np.float64 and np.array_equal(est[0], poses[0])
    assert [r.ok for r in results] == [True] * 6 and all(np.array_equal(r.pose, e) for r, e in zip(results, est))
    dt, dr = T.pose_error(poses[5], est[5])
    print('drift at frame 5: %.6f m %.5f deg; pairs %s' % (dt, dr, [r.pairs for r in results]))
    assert dt <= 1.5 * SEQUENCE_DRIFT[0] and dr <= 1.5 * SEQUENCE_DRIFT[1]
    again = fusion.TSDFVolume(dims, VS, w2g).integrate(depth, k, est)
    assert torch.equal(again.sdf().view(torch.int32), vol.sdf().view(torch.int32))
    assert torch.equal(again.weight(), vol.weight())
    # a lost frame is reported and not fused; integrate=False leaves the volume alone
    lost = depth[:3].copy()
    lost[1] = -np.inf
    vol2 = fusion.TSDFVolume(dims, VS, w2g)
    est2, results2 = track.track_sequence(vol2, lost, k[:3], poses[0])
    assert [r.ok for r in results2] == [True, False, True] and np.array_equal(est2[1], est2[0])
    two = fusion.TSDFVolume(dims, VS, w2g).integrate(lost[[0, 2]], k[[0, 2]], est2[[0, 2]])
    assert torch.equal(two.sdf().view(torch.int32), vol2.sdf().view(torch.int32))
    before = vol2.sdf().clone()
    est3, results3 = track.track_sequence(vol2, depth[:2], k[:2], poses[0], integrate=False)
    assert results3[1].ok and torch.equal(before.view(torch.int32), vol2.sdf().view(torch.int32))


def test_argument_errors():
    p = pairs((48, 64), (48, 64))
    launches = track._lib.load().sgnn_launch_count
    before = launches()
    base = dict(depth=p['depth'], k=p['k'], md=p['md'], mn=p['mn'], km=p['km'], T=p['T'], max_dist=0.1,
                max_angle_deg=20.0, live_normal=None)
    huge = np.broadcast_to(F32(1.0), (2, 1 << 15, 1 << 15))                 # B h w = 2^31, no memory behind it
    bad = [
        dict(depth=p['depth'][0]), dict(depth=p['depth'][:2]), dict(md=p['md'][:2]), dict(mn=p['mn'][..., :2]),
        dict(mn=p['mn'][:, :40]), dict(k=p['k'][:2]), dict(km=p['km'][:, :3]), dict(T=p['T'][:2]), dict(T=p['T'][0]),
        dict(max_dist=0.0), dict(max_dist=-0.1), dict(max_angle_deg=0.0), dict(max_angle_deg=-5.0),
        dict(live_normal=p['ln'][:2]), dict(live_normal=p['ln'][..., 0]), dict(depth=huge),
    ]
    for change in bad:
        a = dict(base)
        a.update(change)
        with pytest.raises(ValueError):
            track.normal_equations(a['depth'], a['k'], a['md'], a['mn'], a['km'], a['T'], a['max_dist'],
                                   a['max_angle_deg'], a['live_normal'])
    with pytest.raises(ValueError):
        track.normal_equations(p['depth'], p['k'], p['md'], p['mn'], p['km'], p['T'],
                               residual=torch.empty((3, 48, 64), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        track.normal_equations(p['depth'], p['k'], p['md'], p['mn'], p['km'], p['T'],
                               assoc=torch.empty((2, 48, 64), dtype=torch.int32, device='cuda'))
    for fn in (track.halve, track.depth_normals):
        for args in ((p['depth'][0], p['k'][0]), (p['depth'], p['k'][:2]), (p['depth'], p['k'], 0.0),
                     (p['depth'], p['k'], -1.0), (huge, p['k'][0])):
            with pytest.raises(ValueError):
                fn(*args)
    sdf, w2g = room()
    vol = fusion.TSDFVolume(C.room_grid(VS, 4)[0], VS, w2g)
    pose = np.eye(4)
    for kw in (dict(depth=p['depth']), dict(iterations=()), dict(iterations=(4,) * 8), dict(max_dist=0.0),
               dict(delta=0.0)):
        a = dict(depth=p['depth'][0], iterations=(10, 5, 4), max_dist=0.1, delta=0.05)
        a.update(kw)
        with pytest.raises(ValueError):
            track.align(a['depth'], p['k'][0], pose, pose, vol, iterations=a['iterations'], max_dist=a['max_dist'],
                        delta=a['delta'])
    with pytest.raises(ValueError):
        track.track_sequence(vol, p['depth'], p['k'][:2], pose)
    assert launches() == before                                             # raised before any launch
    track.normal_equations(p['depth'], p['k'], p['md'], p['mn'], p['km'], p['T'])
    assert launches() > before
