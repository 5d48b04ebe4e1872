"""GPU: the differentiable cast (sgnn_amd.raycast.cast_diff, csrc/raycast.hip) against the
NumPy restatement of tests/raycast_grad_ref.py: depth bit for bit with raycast.cast, the hit record, features and ok
bit for bit, the backward of single pixels bit for bit, whole frames within rule 5's bound, and autograd."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402
import raycast_grad_ref as G  # noqa: E402

from sgnn_amd import raycast  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HW = (12, 16)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def dev(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def plane_scene():
    """A 16 x 20 x 24 (z, y, x) volume at 10 cm with a tilted plane that leaves it through the high-z face, band 3
    voxels, two oblique 12 x 16 frames, samples 0.9 voxel apart: crossings inside one cell, across neighbouring cells,
    with the hit in a third cell, and in the last cell of an axis."""
    vs, shape = 0.1, (16, 20, 24)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    n = np.array([0.35, 0.25, 0.9])
    n /= np.linalg.norm(n)
    d = (13.2 - (x * n[0] + y * n[1] + z * n[2])) * vs
    band = F32(3.0) * F32(vs)
    sdf = np.where(np.abs(d) > 0.999 * band, -np.inf, d).astype(F32)
    c = np.array(shape[::-1]) * vs / 2
    eyes = [c + np.array([-0.4, -0.5, -2.0]), c + np.array([0.9, 0.3, -1.7])]
    poses = np.stack([R.look_at(e, c + np.array([0.1, 0.0, 0.5]), up=(0.0, 1.0, 0.0)) for e in eyes])
    k = np.tile(np.array([14.0, 14.0, 7.5, 5.5], F32), (2, 1))
    return dict(sdf=sdf, w2g=R.grid_transform((0.0, 0.0, 0.0), vs), vs=vs, k=k, poses=poses, band=band, step=0.9)


def endcap_scene():
    """Hits whose cell test fails.  The hit lies between both samples, so it can leave the volume only by rounding:
    with v = 0 the hit is t0 + dt, which may be one ulp above t1 = depth_min + k . dt.  A camera looks along +x at
    16 voxels per metre (every factor a power of two, so positions are 16 t + o exactly); the last layer of cells of
    a 16 x 20 x 41 volume holds zeros and the voxels before it are positive; o.x is chosen so that the sample k with
    t0 + dt > t1 lands on the last float below d - 1 = 40 and the hit on 40 itself.  The second frame stands 0.3
    voxel further back: its hits are ordinary ones in the last cell of x."""
    vs, shape, step, dmin = 1.0 / 16, (16, 20, 41), 1.2, F32(0.4)
    dt = F32(step) * F32(vs)
    at = lambda k: dmin + F32(k) * dt  # noqa: E731
    kk = next(k for k in range(2, 60) if F32(2) <= at(k) < F32(4) and F32(at(k - 1) + dt) > at(k))
    ox = 40.0 - 16.0 * float(F32(at(kk - 1) + dt))
    x = np.arange(shape[2], dtype=np.float64)
    sdf = np.broadcast_to(np.maximum(39.0 - x, 0.0) * vs, shape).astype(F32)
    rot = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])       # camera z -> world x, x -> y, y -> z
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[:, :3, :3] = rot
    poses[0, :3, 3] = np.array([ox, 10.0, 8.0]) * vs
    poses[1, :3, 3] = np.array([ox - 0.3, 10.0, 8.0]) * vs
    k = np.tile(np.array([64.0, 64.0, 7.5, 5.5], F32), (2, 1))
    return dict(sdf=sdf, w2g=R.grid_transform((0.0, 0.0, 0.0), vs), vs=vs, k=k, poses=poses, band=F32(100.0),
                step=step, kk=kk)


def room_scene():
    """The room of the CPU test: 60 x 72 x 88 voxels at 5 cm, two 12 x 16 frames."""
    vs = 0.05
    band = F32(3.0) * F32(vs)
    sdf, w2g = C.room_sdf(vs, 4, band)
    _, k, poses = R.room_frames(2, HW, seed=1)
    return dict(sdf=sdf, w2g=w2g, vs=vs, k=k, poses=poses, band=band, step=0.5)


def geometry(s):
    return (s['sdf'], s['w2g'], s['vs'], s['k'], s['poses'], HW, s['band'])


def complete(s):
    """The restatement's forward with five channels (fewer channels are its leading ones), the term geometry, and
    the device plan of the scene."""
    s['fe'] = G.smooth_features(s['sdf'].shape, 5)
    s['depth'], s['hit'], s['feat'], s['ok'] = G.forward(*geometry(s), s['fe'], step=s['step'])
    _, _, band, dmin, dt, ns, table = raycast._plan(*geometry(s), s['step'], 0.4, 4.0)
    s['plan'] = (torch.from_numpy(table.view(np.uint8)).cuda(), HW, band, dmin, dt, ns)
    return s


@pytest.fixture(scope='module')
def scenes():
    return {name: complete(make()) for name, make in (('plane', plane_scene), ('endcap', endcap_scene),
                                                      ('room', room_scene))}


def ref_terms(s, channels, gd, gf):
    fe = None if not channels else np.ascontiguousarray(s['fe'][..., :channels])
    return G.terms(s['sdf'], s['w2g'], s['vs'], s['k'], s['poses'], HW, s['hit'], fe, gd, gf, step=s['step'])


def forward(s, channels, **kw):
    table, hw, band, dmin, dt, ns = s['plan']
    fe = dev(s['fe'][..., :channels]) if channels else None
    return raycast.diff_forward(dev(s['sdf']), fe, table, hw, band, dmin, dt, ns, **kw)


def backward(s, channels, gd, gf, hit=None, **kw):
    table, hw, band, dmin, dt, ns = s['plan']
    fe = dev(s['fe'][..., :channels]) if channels else None
    hit = s['hit'] if hit is None else hit
    gs, gfe = raycast.diff_backward(dev(s['sdf']), fe, table, hw, dmin, dt, ns, dev(hit, np.int32), dev(gd, F32),
                                    dev(gf, F32), **kw)
    return gs.cpu().numpy(), (None if gfe is None else gfe.cpu().numpy())


def categories(s):
    """Per frame (pixel numbers, dict of boolean arrays over them): where both samples and the hit lie."""
    out = []
    for f, x, t in ref_terms(s, 1, None, np.ones(s['hit'].shape + (1,), F32)):
        shape = s['sdf'].shape
        fs = np.stack(np.unravel_index(t[2][:, 0], shape)[::-1], 1)
        same = (x.f0 == x.f1).all(1)
        inside = t[4]
        third = inside & ~(fs == x.f0).all(1) & ~(fs == x.f1).all(1)
        last = inside & (fs == np.array(shape[::-1]) - 2).any(1)
        out.append((f, x.pix, dict(same=same & inside & ~third, neighbours=~same & inside & ~third, third=third,
                                   last=last, outside=~inside)))
    return out


def test_the_scenes_cover_the_cases(scenes):
    count = {}
    for name, s in scenes.items():
        for f, pix, cat in categories(s):
            for key, m in cat.items():
                count[name, f, key] = int(m.sum())
    print(count)
    for key in ('same', 'neighbours', 'third', 'last'):
        assert sum(count['plane', f, key] for f in (0, 1)) >= 3, key
    e = scenes['endcap']
    assert count['endcap', 0, 'outside'] == HW[0] * HW[1] == (e['hit'][0] == e['kk']).sum()
    assert not e['ok'][0].any() and (e['feat'][0] == 0).all() and np.isfinite(e['depth'][0]).all()
    assert count['endcap', 1, 'last'] == HW[0] * HW[1] and e['ok'][1].all()
    p = scenes['plane']
    assert 0.5 < np.isfinite(p['depth']).mean() < 1.0 and (p['ok'] == np.isfinite(p['depth'])).all()
    r = scenes['room']
    assert r['sdf'].shape == (60, 72, 88) and np.isfinite(r['depth']).mean() > 0.9


@pytest.mark.parametrize('name', ['plane', 'endcap', 'room'])
def test_forward_bitwise(scenes, name):
    s = scenes[name]
    for channels in (0, 1, 3, 5):
        for kw in (dict(), dict(skip=False), dict(chunk=1), dict(chunk=1, skip=False)):
            if name == 'room' and (channels not in (0, 3) or kw.get('chunk')):
                continue
            depth, hit, feat, ok = forward(s, channels, **kw)
            plain = raycast.cast(*geometry(s), step=s['step'], **kw)
            assert np.array_equal(bits(depth), bits(plain)) and np.array_equal(bits(depth), bits(s['depth'])), kw
            assert hit.dtype == torch.int32 and np.array_equal(hit.cpu().numpy(), s['hit']), kw
            assert np.array_equal(ok.cpu().numpy().astype(bool), s['ok']), kw
            if channels:
                assert tuple(feat.shape) == s['hit'].shape + (channels,)
                assert np.array_equal(bits(feat), bits(s['feat'][..., :channels])), (kw, channels)
            else:
                assert feat is None


def one_hot_cases(s):
    """(frame, pixel, what) for one pixel of every category the scene has: the nearest to the frame's centre."""
    out = []
    for f, pix, cat in categories(s):
        for key, m in cat.items():
            if m.any():
                cand = pix[m]
                out.append((f, int(cand[np.argmin((cand // HW[1] - HW[0] // 2) ** 2 + (cand % HW[1] - HW[1] // 2) ** 2)]),
                            key))
    return out


@pytest.mark.parametrize('name', ['plane', 'endcap'])
def test_one_hot_backward_bitwise(scenes, name):
    s = scenes[name]
    cases = one_hot_cases(s)
    assert {c[2] for c in cases} >= ({'same', 'neighbours', 'third', 'last'} if name == 'plane' else {'outside', 'last'})
    n = 0
    for f, px, what in cases:
        for channels in (1, 3, 5):
            for slot in [-1] + list(range(channels)):                      # gd, then each gf_c
                gd = np.zeros(s['hit'].shape, F32)
                gf = np.zeros(s['hit'].shape + (channels,), F32)
                if slot < 0:
                    gd[f].reshape(-1)[px] = F32(1.7)
                else:
                    gf[f].reshape(-1, channels)[px, slot] = F32(-0.6)
                lists = ref_terms(s, channels, gd, gf)
                exp_s, exp_f = G.scatter32(lists, s['sdf'].shape, channels)
                cnt = np.zeros(exp_s.size)
                for fr, x, t in lists:
                    here = (x.pix == px) & (fr == f)
                    np.add.at(cnt, t[0][here].ravel(), 1)
                assert cnt.max() <= 2                                       # a two-term sum has no order
                got_s, got_f = backward(s, channels, gd, gf)
                assert np.array_equal(bits(got_s), bits(exp_s)), (what, channels, slot)
                assert np.array_equal(bits(got_f), bits(exp_f)), (what, channels, slot)
                if what == 'outside':
                    assert not got_f.any() and (slot >= 0) == (not got_s.any())
                else:
                    assert got_s.any() and (slot < 0) == (not got_f.any())
                n += 1
    assert n >= 2 * 9


def within(got, exact, bound):
    return bool((np.abs(got.astype(np.float64) - exact) <= bound).all())


@pytest.mark.parametrize('name', ['plane', 'endcap', 'room'])
def test_full_frames_within_the_bound(scenes, name):
    s = scenes[name]
    rng = np.random.default_rng(7)
    for channels in ((0, 3) if name == 'room' else (0, 1, 3, 5)):
        gd = rng.normal(size=s['hit'].shape).astype(F32)
        gf = rng.normal(size=s['hit'].shape + (channels,)).astype(F32) if channels else None
        lists = ref_terms(s, channels, gd, gf)
        exact_s, bound_s, exact_f, bound_f = G.accumulate(lists, s['sdf'].shape, channels)
        assert np.abs(exact_s).max() > 0 and bound_s.max() < 1e-3 * np.abs(exact_s).max()
        for kw in (dict(), dict(chunk=1)):
            got_s, got_f = backward(s, channels, gd, gf, **kw)
            assert within(got_s, exact_s, bound_s), (channels, kw)
            assert (got_s[bound_s == 0] == 0).all()
            if channels:
                assert within(got_f, exact_f, bound_f), (channels, kw)
            else:
                assert got_f is None
        # either incoming gradient alone, and either output alone
        only_d = backward(s, channels, gd, None)
        ex = G.accumulate(ref_terms(s, channels, gd, None), s['sdf'].shape)
        assert within(only_d[0], ex[0], ex[1])
        if channels:
            assert not only_d[1].any()
            only_f = backward(s, channels, None, gf)
            ex = G.accumulate(ref_terms(s, channels, None, gf), s['sdf'].shape, channels)
            assert within(only_f[0], ex[0], ex[1]) and within(only_f[1], ex[2], ex[3])
            table, hw, band, dmin, dt, ns = s['plan']
            args = (dev(s['sdf']), dev(s['fe'][..., :channels]), table, hw, dmin, dt, ns, dev(s['hit']), dev(gd), dev(gf))
            a, b = raycast.diff_backward(*args, want_sdf=False)
            assert a is None and within(b.cpu().numpy(), exact_f, bound_f)
            a, b = raycast.diff_backward(*args, want_features=False)
            assert b is None and within(a.cpu().numpy(), exact_s, bound_s)


def test_edge_cases(scenes):
    s = scenes['plane']
    rng = np.random.default_rng(8)
    gd = rng.normal(size=s['hit'].shape).astype(F32)
    gf = rng.normal(size=s['hit'].shape + (3,)).astype(F32)
    exact_s, bound_s, exact_f, bound_f = G.accumulate(ref_terms(s, 3, gd, gf), s['sdf'].shape, 3)
    # NaN on the pixels without a hit changes nothing
    miss = s['hit'] < 0
    assert miss.any()
    gd_nan, gf_nan = gd.copy(), gf.copy()
    gd_nan[miss], gf_nan[miss] = np.nan, np.nan
    got_s, got_f = backward(s, 3, gd_nan, gf_nan)
    assert within(got_s, exact_s, bound_s) and within(got_f, exact_f, bound_f)
    # two calls agree within the bound of each
    again_s, again_f = backward(s, 3, gd, gf)
    assert (np.abs(got_s.astype(np.float64) - again_s) <= 2 * bound_s).all()
    assert (np.abs(got_f.astype(np.float64) - again_f) <= 2 * bound_f).all()
    # a frame with a non-finite pose: empty in the forward, nothing in the backward, whatever its record says
    broken = dict(s, poses=s['poses'].copy())
    broken['poses'][1, 0, 3] = np.inf
    complete(broken)
    assert (broken['hit'][1] == -1).all() and np.array_equal(broken['hit'][0], s['hit'][0])
    depth, hit, feat, ok = forward(broken, 3)
    assert np.array_equal(hit.cpu().numpy(), broken['hit']) and (depth[1] == -float('inf')).all()
    assert not ok[1].any() and not feat[1].any()
    ex = G.accumulate(ref_terms(broken, 3, gd, gf), s['sdf'].shape, 3)
    for record in (broken['hit'], s['hit']):
        got = backward(broken, 3, gd, gf, hit=record)
        assert within(got[0], ex[0], ex[1]) and within(got[1], ex[2], ex[3])
    # a record that names no crossing of the volume adds nothing
    wild = np.full(s['hit'].shape, 3, np.int32)
    wild[1] = 1 << 19
    got = backward(s, 3, gd, gf, hit=wild)
    assert not got[0].any() and not got[1].any()
    # no features: feat is None, and no frames at all
    depth, feat, ok = raycast.cast_diff(*geometry(s), step=s['step'])
    assert feat is None and ok.dtype == torch.bool and np.array_equal(bits(depth), bits(s['depth']))
    depth, feat, ok = raycast.cast_diff(s['sdf'], s['w2g'], s['vs'], s['k'][:0], s['poses'][:0], HW, s['band'],
                                        features=s['fe'])
    assert tuple(depth.shape) == (0,) + HW and tuple(feat.shape) == (0,) + HW + (5,) and tuple(ok.shape) == (0,) + HW


def test_autograd_dense_and_sparse(scenes):
    s = scenes['plane']
    rng = np.random.default_rng(9)
    gd = rng.normal(size=s['hit'].shape).astype(F32)
    gf = rng.normal(size=s['hit'].shape + (3,)).astype(F32)
    exact_s, bound_s, exact_f, bound_f = G.accumulate(ref_terms(s, 3, gd, gf), s['sdf'].shape, 3)
    sdf = dev(s['sdf']).requires_grad_()
    fe = dev(s['fe'][..., :3]).requires_grad_()
    depth, feat, ok = raycast.cast_diff(sdf, s['w2g'], s['vs'], s['k'], s['poses'], HW, s['band'], features=fe,
                                        step=s['step'])
    assert depth.requires_grad and feat.requires_grad and not ok.requires_grad
    assert np.array_equal(bits(depth.detach()), bits(s['depth'])) and np.array_equal(ok.cpu().numpy(), s['ok'])
    assert np.array_equal(bits(feat.detach()), bits(s['feat'][..., :3]))
    hit = torch.isfinite(depth)
    loss = (torch.where(hit, depth, torch.zeros_like(depth)) * dev(gd)).sum() + (feat * dev(gf)).sum()
    g_sdf, g_fe = torch.autograd.grad(loss, (sdf, fe))
    direct_s, direct_f = backward(s, 3, gd, gf)
    assert (np.abs(g_sdf.cpu().numpy().astype(np.float64) - direct_s) <= 2 * bound_s).all()
    assert (np.abs(g_fe.cpu().numpy().astype(np.float64) - direct_f) <= 2 * bound_f).all()
    assert within(g_sdf.cpu().numpy(), exact_s, bound_s) and within(g_fe.cpu().numpy(), exact_f, bound_f)
    # depth alone, features without a gradient
    depth, feat, ok = raycast.cast_diff(sdf, s['w2g'], s['vs'], s['k'], s['poses'], HW, s['band'],
                                        features=dev(s['fe'][..., :3]), step=s['step'])
    (only,) = torch.autograd.grad((torch.where(hit, depth, torch.zeros_like(depth)) * dev(gd)).sum(), (sdf,))
    ex = G.accumulate(ref_terms(s, 3, gd, None), s['sdf'].shape)
    assert within(only.cpu().numpy(), ex[0], ex[1])
    # sparse rows: the same frames, and per-row gradients = the dense gradient at the rows' voxels
    locs = np.stack(np.nonzero(np.isfinite(s['sdf'])), 1)
    perm = rng.permutation(len(locs))
    locs = locs[perm]
    vals = dev(s['sdf'][locs[:, 0], locs[:, 1], locs[:, 2]]).requires_grad_()
    rows = dev(s['fe'][locs[:, 0], locs[:, 1], locs[:, 2], :3]).requires_grad_()
    depth, feat, ok = raycast.cast_sparse_diff(dev(locs), vals, s['sdf'].shape, s['w2g'], s['vs'], s['k'], s['poses'],
                                               HW, s['band'], features=rows, step=s['step'])
    assert np.array_equal(bits(depth.detach()), bits(s['depth'])) and np.array_equal(ok.cpu().numpy(), s['ok'])
    # features of voxels without a row are 0, so feat differs from the dense call only where such a voxel is a corner
    hole = np.where(np.isfinite(s['sdf'])[..., None], s['fe'][..., :3], F32(0))
    exp = G.forward(*geometry(s), hole, step=s['step'])
    assert np.array_equal(bits(feat.detach()), bits(exp[2]))
    loss = (torch.where(hit, depth, torch.zeros_like(depth)) * dev(gd)).sum() + (feat * dev(gf)).sum()
    g_vals, g_rows = torch.autograd.grad(loss, (vals, rows))
    lists = G.terms(s['sdf'], s['w2g'], s['vs'], s['k'], s['poses'], HW, s['hit'], hole, gd, gf, step=s['step'])
    ex = G.accumulate(lists, s['sdf'].shape, 3)
    at = (locs[:, 0], locs[:, 1], locs[:, 2])
    assert within(g_vals.cpu().numpy(), ex[0][at], ex[1][at]) and within(g_rows.cpu().numpy(), ex[2][at], ex[3][at])
    assert g_vals.abs().sum().item() > 0 and g_rows.abs().sum().item() > 0


def test_argument_errors_before_any_launch(scenes):
    s = scenes['plane']
    launches = raycast._lib.load().sgnn_launch_count
    before = launches()
    fe = s['fe']
    for wrong in (fe[1:], fe[..., 0], fe.reshape(-1, 5), np.zeros(s['sdf'].shape + (0,), F32),
                  np.zeros(s['sdf'].shape + (17,), F32)):
        with pytest.raises(ValueError, match='features'):
            raycast.cast_diff(*geometry(s), features=wrong)
    for kw in (dict(step=0.0), dict(depth_min=2.0, depth_max=1.0), dict(step=1e-6)):
        with pytest.raises(ValueError):
            raycast.cast_diff(*geometry(s), features=fe, **kw)
    with pytest.raises(ValueError):
        raycast.cast_diff(s['sdf'][0], *geometry(s)[1:])
    with pytest.raises(ValueError):
        raycast.cast_diff(s['sdf'], s['w2g'], s['vs'], s['k'][:1], s['poses'], HW, s['band'])
    locs = np.stack(np.nonzero(np.isfinite(s['sdf'])), 1)
    vals = s['sdf'][np.isfinite(s['sdf'])]
    tail = (s['sdf'].shape,) + geometry(s)[1:]
    for a, b, kw in ((locs[:, :2], vals, {}), (locs, vals[1:], {}), (locs, vals, dict(features=np.zeros((3, 2), F32))),
                     (locs, vals, dict(features=np.zeros((len(vals), 17), F32))), (locs, vals, dict(step=-1.0))):
        with pytest.raises(ValueError):
            raycast.cast_sparse_diff(a, b, *tail, **kw)
    assert launches() == before
    # the library's own checks return before a launch too
    table, hw, band, dmin, dt, ns = s['plan']
    sdf, hit = dev(s['sdf']), dev(s['hit'])
    out = [torch.empty(s['hit'].shape, device='cuda') for _ in range(3)]
    with pytest.raises(raycast._lib.SgnnError):
        raycast._lib.call('sgnn_raygrad_cast', sdf.data_ptr(), 24, 20, 16, float(band), None, table.data_ptr(), 2, 0, 12,
                          16, float(dmin), float(dt), ns, dev(fe).data_ptr(), 17, out[0].data_ptr(), hit.data_ptr(),
                          out[1].data_ptr(), out[2].data_ptr())
    with pytest.raises(raycast._lib.SgnnError):
        raycast._lib.call('sgnn_raygrad_backward', sdf.data_ptr(), 24, 20, 16, table.data_ptr(), 2, 0, 12, 16, float(dmin),
                          float(dt), ns, hit.data_ptr(), None, 0, None, out[0].data_ptr(), out[1].data_ptr(), None)
    assert launches() == before
