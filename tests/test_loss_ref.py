"""CPU: tests/loss_ref.py (the float64 host reference the GPU tests of loss.hip and metrics.hip rely on) anchored to the
oracle's restatement of the reference (oracle/model_oracle.py, oracle/metrics_oracle.py), to the stored outputs of the
reference itself (tests/golden/targets_expected.npz, metrics_expected.npz), and to closed forms; and the properties of
tests/loss_cases.py's inputs that tests/test_gpu_loss_fp64.py takes for granted."""
import os

import numpy as np
import pytest
import torch

import loss_cases as C
import loss_ref as LR
import metrics_oracle as meto
import model_oracle as mo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _sites(rng, n, batch, dims):
    cells = rng.permutation(batch * int(np.prod(dims)))[:n]
    vol = int(np.prod(dims))
    b, v = cells // vol, cells % vol
    return np.stack([v // (dims[1] * dims[2]), (v // dims[2]) % dims[1], v % dims[2], b], 1).astype(np.int64)


def _small_scene(seed, L, dims, batch=2):
    rng = np.random.default_rng(seed)
    shape = lambda k: (batch, 1) + tuple(d >> k for d in dims)
    sdf = rng.uniform(-5, 5, shape(0)).astype(np.float32)
    sdf.reshape(-1)[:6] = [np.inf, -np.inf, 0.0, -0.0, 3.0, -3.0]
    known = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), shape(0))
    hierarchy = [rng.uniform(-5, 5, shape(L - 1 - h)).astype(np.float32) for h in range(L - 1)]
    locs = _sites(rng, 40, batch, dims)
    return sdf, known, hierarchy, locs


@pytest.mark.parametrize('L,dims', [(1, (3, 5, 7)), (2, (2, 6, 10)), (3, (4, 12, 20)), (4, (8, 24, 40)), (4, (16, 8, 8))])
@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('trunc', [3.0, 0.5])
def test_targets_equal_the_oracle(L, dims, masking, trunc):
    sdf, known, hierarchy, locs = _small_scene(L * 7 + masking, L, dims)
    ts, occs, hiers = mo.compute_targets(torch.from_numpy(sdf.copy()), [torch.from_numpy(h.copy()) for h in hierarchy], L, trunc,
                                         masking, torch.from_numpy(known))
    w = mo.compute_weights_missing_geo(5.0, torch.from_numpy(locs), occs, trunc)
    tsdf, rocc, rhier, rw = LR.targets(sdf, known, locs, None, hierarchy, L, trunc, masking, 5.0)
    assert np.array_equal(tsdf.view(np.int32), ts.numpy().view(np.int32))
    for h in range(L):
        assert np.array_equal(rocc[h], occs[h].numpy()), h
        assert np.array_equal(rhier[h].view(np.int32), hiers[h].numpy().view(np.int32)), h
        assert np.array_equal(rw[h], w[h].numpy()), h
    assert LR.targets(sdf, known, None, None, hierarchy, L, trunc, masking, None)[3] is None


def test_targets_keep_nan_like_torch_clamp_and_count_live_sites_only():
    sdf, known, hierarchy, locs = _small_scene(3, 2, (2, 6, 10))
    sdf.reshape(-1)[7] = np.nan
    hierarchy[0].reshape(-1)[3] = np.nan
    tsdf, occs, hiers, w = LR.targets(sdf, known, locs, 10, hierarchy, 2, 3.0, False, 5.0)
    want = torch.from_numpy(sdf.copy()).clamp_(-3.0, 3.0).numpy()
    assert np.array_equal(tsdf.view(np.int32), want.view(np.int32)) and np.isnan(tsdf.reshape(-1)[7])
    assert np.isnan(hiers[0].reshape(-1)[3]) and occs[1].reshape(-1)[7] == 0
    fl = LR.flat_index(locs, (2, 6, 10))
    assert (w[1].reshape(-1)[fl[:10]] == 1).all() and (w[1].reshape(-1)[fl[10:]] == 5).all()
    outside = np.array([[-1, 0, 0, 0], [0, 6, 0, 0], [0, 0, 0, 2]], np.int64)
    w2 = LR.targets(sdf, known, np.concatenate([outside, locs]), 13, hierarchy, 2, 3.0, False, 5.0)[3]
    assert np.array_equal(w2[1], w[1])


def _oracle_loss(levels, coef, g, use_log, masking, known):
    """The oracle's per-level functions in float64 torch: total, per-level (bce, l1) and the gradients of g x total."""
    total, grads, means = 0.0, [], []
    for lv, (cb, cl) in zip(levels, coef):
        v = torch.from_numpy(lv['vals'].astype(np.float64)).requires_grad_(True)
        locs = torch.from_numpy(lv['locs'])
        dense = lambda a: None if a is None else torch.from_numpy(np.asarray(a).astype(np.float64))
        w = dense(lv['weights'])
        bce = l1 = None
        if lv['occ_col'] >= 0:
            bce = mo.bce_sparse_dense(locs, v[:, lv['occ_col']], dense(lv['tgt_occ']), w, masking)
            total = total + cb * bce
        if lv['sdf_col'] >= 0:
            kn = torch.from_numpy(known) if lv['mask_mode'] == 2 else \
                (torch.from_numpy(lv['tgt_occ']) == -1) * 2 if masking else None
            l1 = mo.l1_predsurf_sparse_dense(locs, v[:, lv['sdf_col']], dense(lv['tgt_sdf']), w, use_log, masking, kn)
            total = total + cl * l1
        grads.append(v)
        means.append((bce, l1))
    (g * total).backward()
    return float(total.detach()), means, [v.grad.numpy() for v in grads]


@pytest.mark.parametrize('use_log', [0, 1])
@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('weights', [False, True])
def test_loss_equals_the_oracle_in_float64(use_log, masking, weights):
    vol = C.volumes()
    a, _ = C.level(700, (2, 0, 1), 1 if masking else 0, use_log, weights, key='oracle', ladder=False)
    b, _ = C.level(300, (1, -1, 0), 2 if masking else 0, use_log, weights, key='oracle')
    for lv in (a, b):
        lv['vals'] = np.where(np.isnan(lv['vals']), np.float32(0), lv['vals'])
    coef, g = ((0.5, 2.0), (0.0, 3.0)), 0.375
    ref = LR.loss_levels([a, b], coef, g)
    total, means, grads = _oracle_loss([a, b], coef, g, bool(use_log), masking, vol['known'])
    assert ref['total'] == pytest.approx(total, rel=1e-12)
    assert ref['out2s'][0, 0] == pytest.approx(float(means[0][0].detach()), rel=1e-12)
    assert ref['out2s'][0, 1] == pytest.approx(float(means[0][1].detach()), rel=1e-12)
    assert ref['out2s'][1, 1] == pytest.approx(float(means[1][1].detach()), rel=1e-12)
    for l in range(2):
        assert np.allclose(ref['dvals'][l], grads[l], rtol=1e-11, atol=1e-18), l


@pytest.mark.parametrize('use_log', [False, True])
@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('wgeo', [1.0, 5.0])
@pytest.mark.parametrize('lw', [(0.5, 2.0), (0.0, 3.0), (1.5, 0.0)])
def test_loss_equals_oracle_compute_loss(use_log, masking, wgeo, lw):
    """model_oracle.compute_loss itself (loss weights, the cur_known rule, skipped levels, weights from the input sites)
    in float64 torch: value, per-level values and autograd gradient of g x loss."""
    vol = C.volumes()
    a, _ = C.level(700, (2, 0, 1), 1 if masking else 0, int(use_log), False, key='compose')
    b, _ = C.level(300, (1, -1, 0), 2 if masking else 0, int(use_log), False, key='compose')
    t64 = lambda x: torch.from_numpy(np.asarray(x).astype(np.float64))
    occ, sdf, known = t64(vol['tgt_occ']), t64(vol['tgt_sdf']), torch.from_numpy(vol['known'])
    input_locs = torch.from_numpy(a['locs'][::7].copy())
    va, vb = t64(a['vals']).requires_grad_(True), t64(b['vals']).requires_grad_(True)
    loss, losses = mo.compute_loss([torch.from_numpy(b['locs']), vb], [[torch.from_numpy(a['locs']), va]], sdf, [occ], [sdf], lw,
                                   C.TRUNC, use_log, wgeo, input_locs, masking, known)
    g = 0.375
    if torch.is_tensor(loss):
        (g * loss).backward()
    w = mo.compute_weights_missing_geo(wgeo, input_locs, [occ], C.TRUNC)[0].numpy().astype(np.float32) if wgeo > 1 else None
    a['weights'] = b['weights'] = w
    ref = LR.loss_levels([a, b], [(lw[0], lw[0]), (0.0, lw[1])], g)
    assert ref['total'] == pytest.approx(float(loss.detach() if torch.is_tensor(loss) else loss), rel=1e-12)
    for l, (v, cur) in enumerate(zip((va, vb), losses)):
        if lw[l] == 0:
            assert cur == -1 and v.grad is None and (ref['dvals'][l] == 0).all() and ref['cur'][l] == 0
        else:
            assert ref['cur'][l] == pytest.approx(cur, rel=1e-12)
            assert np.allclose(ref['dvals'][l], v.grad.numpy(), rtol=1e-11, atol=1e-18), l


@pytest.mark.parametrize('tag', ['rect_mask_w5', 'rect_nomask_w1', 'cube64_mask_w5'])
def test_reference_goldens(tag):
    """Targets and weights exact, loss and gradients within the float32-vs-float64 bars test_oracle_targets.py carries."""
    from sgnn_amd import synth
    z = np.load(os.path.join(GOLD, 'targets_expected.npz'))
    d0, d1, d2, batch, cfg, masking = (int(v) for v in z[tag + '_cfg'])
    wgeo = float(z[tag + '_wgeo'])
    data = synth.make_batch(batch, (d0, d1, d2), cfg=cfg, occupancy=0.07)
    locs, known = data['input'][0].numpy(), data['known'].numpy()
    tsdf, occs, hiers, w = LR.targets(data['sdf'].numpy(), known, locs, None, [h.numpy() for h in data['hierarchy']], 4, 3.0,
                                      bool(masking), wgeo if wgeo > 1 else None)
    assert np.array_equal(tsdf, z[tag + '_tsdf'])
    for h in range(4):
        assert np.array_equal(occs[h], z['%s_occ%d' % (tag, h)].astype(np.float32))
        assert np.array_equal(hiers[h], z['%s_hier%d' % (tag, h)])
        if w is not None:
            assert np.array_equal(w[h], z['%s_w%d' % (tag, h)])
    lw = z[tag + '_lw']
    levels, coef = [], []
    for h in range(4):
        levels.append(dict(locs=z['%s_pred%d_locs' % (tag, h)], vals=z['%s_pred%d_vals' % (tag, h)], occ_col=0, sdf_col=1,
                           tgt_occ=occs[h], tgt_sdf=hiers[h], weights=None if w is None else w[h], known=None,
                           dims=occs[h].shape[2:], use_log=1, mask_mode=1 if masking else 0, m_dev=None))
        coef.append((lw[h], lw[h]))
    levels.append(dict(locs=z[tag + '_pred3_locs'], vals=z[tag + '_sdf_vals'], occ_col=-1, sdf_col=0, tgt_occ=None, tgt_sdf=tsdf,
                       weights=None if w is None else w[3], known=known, dims=(d0, d1, d2), use_log=1,
                       mask_mode=2 if masking else 0, m_dev=None))
    coef.append((0.0, lw[4]))
    ref = LR.loss_levels(levels, coef, 1.0)
    assert abs(ref['total'] - float(z[tag + '_loss'])) <= 1e-6 * abs(float(z[tag + '_loss']))
    assert np.allclose(ref['cur'], z[tag + '_losses'], rtol=1e-6)
    for h in range(4):
        assert np.allclose(ref['dvals'][h], z['%s_pred%d_grad' % (tag, h)], rtol=1e-5, atol=1e-9)
    assert np.allclose(ref['dvals'][4], z[tag + '_sdf_grad'], rtol=1e-5, atol=1e-9)


def test_metrics_equal_the_reference_goldens_and_the_oracle():
    g = np.load(os.path.join(GOLD, 'metrics_expected.npz'))
    for h in range(4):
        locs, vals = g['locs%d' % h], g['vals%d' % h]
        tgt = g['target_occ%d' % h]
        keep = 1.0 / (1.0 + np.exp(-vals[:, 0].astype(np.float32))) > 0.5
        pred = [locs[(locs[:, 3] == b) & keep][:, :3] for b in range(3)]
        for masking in (True, False):
            for t in (tgt[:, 0].astype(np.float32), tgt[:, 0].astype(np.uint8)):
                lo, hi, band = LR.iou_counts(locs, None, vals, 2, t, int(masking), 3)
                assert len(band) == 0 and np.array_equal(lo, hi)
                lo2 = LR.iou_counts(locs, keep.astype(np.uint8), None, 0, t, int(masking), 3)[0]
                assert np.array_equal(lo, lo2)
                P, Cc, T = lo.sum(0)
                assert Cc / (P + T - Cc) == float(g['iou%d_m%d' % (h, masking)])
                with np.errstate(divide='ignore', invalid='ignore'):
                    per = (lo[:, 1].astype(np.float32) / (lo[:, 0] + lo[:, 2] - lo[:, 1]).astype(np.float32))
                assert np.array_equal(per, g['iou%d_m%d_per' % (h, masking)], equal_nan=True)
                assert Cc / (P + T - Cc) == meto.compute_iou_sparse_dense(pred, tgt.astype(np.uint8), masking)
    for masking in (True, False):
        for thresh, tag in ((-1.0, 'n'), (1.0, '1')):
            s, n, terms, nterms, big = LR.l1_tgtsurf(g['sdf_locs'], g['sdf_vals'], g['target_sdf'][:, 0],
                                                     g['known'] if masking else None, 3.0, thresh)
            assert s / n == pytest.approx(float(g['l1tgt_m%d_t%s' % (int(masking), tag)]), rel=2e-6)
            want = meto.compute_l1_tgtsurf_sparse_dense(g['sdf_locs'], g['sdf_vals'], g['target_sdf'], 3.0, masking, g['known'],
                                                        thresh=None if thresh < 0 else thresh)
            assert s / n == pytest.approx(want, rel=1e-12)
            assert terms >= abs(s) and nterms >= n and big <= 6.0


def test_iou_band_and_rejected_rows():
    import glue_ref
    x = glue_ref.sigmoid_ladder()
    m = len(x)
    locs = np.zeros((m, 4), np.int64)
    tgt = np.ones((1, 2, 2, 4), np.float32)
    lo, hi, band = LR.iou_counts(locs, None, x, 1, tgt, 0, 1)
    keep, drop = glue_ref.sigmoid_rule(x)
    assert lo[0, 0] == keep.sum() and hi[0, 0] == m - drop.sum() and len(band) == m - keep.sum() - drop.sum() > 0
    assert lo[0, 2] == 16 and (lo[:, 1] == lo[:, 0]).all()
    bad = np.array([[-1, 0, 0, 0], [2, 0, 0, 0], [0, -1, 0, 0], [0, 2, 0, 0], [0, 0, -1, 0], [0, 0, 4, 0], [0, 0, 0, -1],
                    [0, 0, 0, 1], [1, 1, 3, 0]], np.int64)
    lo = LR.iou_counts(bad, None, None, 0, tgt, 0, 1)[0]
    assert lo.tolist() == [[1, 1, 16]]


def test_closed_forms():
    vol = dict(tgt_occ=np.array([0, 1, -1, 1], np.float32), tgt_sdf=np.array([0.5, -0.0, 3.0, -2.0], np.float32),
               weights=np.array([1, 5, 5, 1], np.float32), known=np.array([0, 1, 2, 255], np.uint8))
    locs = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 2, 0], [0, 0, 3, 0]], np.int64)
    vals = np.array([[0.0, 0.5], [-0.0, 0.0], [104.0, 1.0], [-1e4, -2.0]], np.float32)
    r = LR.loss_level(locs, vals, 0, 1, dims=(1, 1, 4), use_log=1, mask_mode=0, **vol)
    assert r['keep'].all()
    assert r['bce'][0] == pytest.approx(np.log(2.0), rel=1e-15) and r['bce'][1] == pytest.approx(5 * np.log(2.0), rel=1e-15)
    assert r['dbce'][0] == 0.5 and r['dbce'][1] == -2.5
    assert r['bce'][2] == pytest.approx(5 * 104.0, rel=1e-15) and r['dbce'][2] == pytest.approx(5.0, rel=1e-15)   # unknown counts as 0
    assert r['bce'][3] == pytest.approx(1e4, rel=1e-15) and r['dbce'][3] == pytest.approx(-1.0, rel=1e-15)
    assert (r['l1'][[0, 1, 3]] == 0).all() and (r['dl1'][[0, 1, 3]] == 0).all()                 # p == t, -0 == 0 included
    assert r['l1'][2] == pytest.approx(5 * (np.log(4.0) - np.log(2.0)), rel=1e-15) and r['dl1'][2] == -2.5
    assert r['mag_bce'][3] == pytest.approx(1e4) and r['mag_dbce'][1] == pytest.approx(5 * 1.5)
    assert LR.loss_level(locs, vals, 0, 1, dims=(1, 1, 4), use_log=1, mask_mode=1, **vol)['keep'].tolist() == [1, 1, 0, 1]
    assert LR.loss_level(locs, vals, 0, 1, dims=(1, 1, 4), use_log=1, mask_mode=2, **vol)['keep'].tolist() == [1, 1, 0, 0]
    lin = LR.loss_level(locs, vals, -1, 1, dims=(1, 1, 4), use_log=0, mask_mode=0, **vol)
    assert lin['l1'][2] == 10.0 and lin['dl1'][2] == -5.0 and (lin['bce'] == 0).all()
    # empty levels and zero coefficients
    lv = dict(locs=locs, vals=vals, occ_col=0, sdf_col=1, dims=(1, 1, 4), use_log=1, mask_mode=1, **vol)
    e = LR.loss_levels([dict(lv, m_dev=0), dict(lv, m_dev=None), dict(lv, m_dev=-3)], [(1, 1), (0, 2), (1, 0)], 1.0)
    assert (e['out2s'][[0, 2]] == 0).all() and e['total'] == 2 * e['out2s'][1, 1] and e['cur'][1] == e['out2s'][1, 1]
    masked = dict(lv, locs=locs[[2, 2]], vals=vals[:2], m_dev=None)
    e = LR.loss_levels([masked], [(1, 0)], 1.0)
    assert np.isnan(e['out2s']).all() and np.isnan(e['total']) and (e['dvals'][0] == 0).all()
    e = LR.loss_levels([masked], [(0, 0)], 1.0)
    assert e['total'] == 0 and e['cur'][0] == 0


def test_case_inputs_hit_every_class_and_keep_the_band_small():
    vol = C.volumes()
    v = C.row_voxels(2049)
    occ, kn, w = (vol[k].reshape(-1)[v] for k in ('tgt_occ', 'known', 'weights'))
    for o in (0, 1, -1):
        for k in (0, 1, 2, 255):
            for ww in (1, 5):
                assert ((occ == o) & (kn == k) & (w == ww)).sum() >= 16, (o, k, ww)
    sdf = vol['tgt_sdf'].reshape(-1)[v]
    for bits in (0x00000000, 0x80000000, 0x40400000, 0xC0400000):
        assert (sdf.view(np.uint32) == bits).sum() >= 16, hex(bits)
    cases = [dict(m=m, key=m, ladder=ld) for m in C.ROW_COUNTS for ld in (False, True) if m != C.BIG or not ld]
    cases += [dict(m=4099, key=C.BIG, ladder=True)]
    cases += [dict(m=1025, layout=lay, mask_mode=mm, ladder=True, key='layout') for lay in C.LAYOUTS for mm in (1, 2)]
    cases += [dict(m=1025, mask_mode=mm, use_log=ul, weights=ww, ladder=True, key='options') for mm in (0, 1, 2)
              for ul in (0, 1) for ww in (False, True)]
    import test_gpu_loss_fp64 as G
    cases += [dict(key=('five', k), **kw) for k, kw in enumerate(G.FIVE)]
    cases += [dict(m=m, m_dev=live, ladder=True, key='cap') for m in (257, 2049) for live in (-3, 0, 1, m - 1, m, m + 5)]
    cases += [dict(m=m, key='ws') for m in (C.BIG, 7, 1025)] + [dict(m=700, key='beside')]
    for kw in cases:
        lv, planted = C.level(**kw)
        live = lv.pop('m_dev')
        row = LR.loss_level(live=live, **lv)
        assert row['keep'].sum() >= 1 or (live is not None and live < 1), kw            # a live row 0 is always kept
        assert not lv['sdf_col'] >= 0 or C.band_rows(row, planted).sum() <= C.BAND_SHARE * row['keep'].sum(), kw
        if lv['sdf_col'] >= 0 and row['live'] >= 255:
            kept = int(row['keep'].sum())
            assert (planted['tie'] & row['keep']).sum() >= 4 and (planted['nb'] & row['keep']).sum() >= 2, kw
            assert C.band_rows(row, planted).sum() <= C.BAND_SHARE * kept, (kw, int(C.band_rows(row, planted).sum()), kept)
            # every planted neighbour lies inside the band, every tie has d == 0
            nb = planted['nb'] & row['keep']
            assert (np.abs(row['d'][nb]) <= C.BAND * LR.EPS32 * row['mag_l1'][nb]).all() and (row['d'][nb] != 0).all()
            assert (row['d'][planted['tie']] == 0).all()
        if lv['occ_col'] >= 0 and kw.get('ladder') and row['live'] >= 255:
            x = lv['vals'][:, lv['occ_col']]
            assert set(np.unique(C.LADDER.view(np.uint32))) <= set(np.unique(x.view(np.uint32)))


def test_five_level_case_has_a_finite_total_and_every_level_contributes():
    import test_gpu_loss_fp64 as G
    levels = [C.level(key=('five', k), **kw)[0] for k, kw in enumerate(G.FIVE)]
    for coef, lv in ((G.FIVE_COEF, levels), (G.FIVE_COEF[::-1], levels[::-1])):
        ref = LR.loss_levels(lv, coef, 0.375)
        assert np.isfinite(ref['total']) and np.isfinite(ref['cur']).all() and (ref['sums'][:, 2] >= 1).all()
    assert sum(c == 0 for pair in G.FIVE_COEF for c in pair) >= 3 and all(any(pair) for pair in G.FIVE_COEF)
    # each level's used means move the total by more than the total's bar would hide
    for l in range(5):
        for c in range(2):
            if G.FIVE_COEF[l][c] != 0:
                assert abs(G.FIVE_COEF[l][c] * ref['out2s'][::-1][l, c]) > 1e-3 * abs(ref['total'])


def test_comparison_rules_notice_the_deliberate_breaks():
    """check_backward on float32 emulations of two one-line kernel errors: d bce without the - t, 1 / (|p| + 2)."""
    lv, planted = C.level(1025, ladder=True, key='breaks')
    ref = LR.loss_levels([lv], (1.0, 1.0), 1.0)
    row, kept = ref['rows'][0], ref['sums'][0, 2]
    good = ref['dvals'][0].astype(np.float32)
    good[~row['keep']] = 0
    good[np.isnan(good)] = 0
    assert C.check_backward(ref, 0, lv, planted, (1.0, 1.0), 1.0, good.view(np.int32), 1, 'exact') <= 1.0
    x = lv['vals'][:, 0].astype(np.float64)
    no_t = good.copy()
    no_t[:, 0] = np.where(row['keep'], row['w'] * LR.sigmoid(x) / kept, 0)
    plus2 = good.copy()
    plus2[:, 1] = np.where(row['keep'], row['w'] * np.sign(row['d']) / (np.abs(lv['vals'][:, 1].astype(np.float64)) + 2) / kept, 0)
    for broken in (no_t, plus2):
        with pytest.raises(AssertionError):
            C.check_backward(ref, 0, lv, planted, (1.0, 1.0), 1.0, broken.view(np.int32), 16, 'broken')
