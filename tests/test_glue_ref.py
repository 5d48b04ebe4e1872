"""The host references of tests/glue_ref.py, on the CPU alone: they agree with each other and with torch where torch has
the operation, and the comparison helpers notice eight kinds of wrong kernel on the data the GPU tests
(test_gpu_rows.py, test_gpu_compaction.py, test_gpu_adam.py) run on."""
import numpy as np
import pytest
import torch

import glue_ref as R


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- agreement with torch and with each other ----

def test_row_references_agree_with_torch():
    src = R.real_data('t', (50, 5))
    idx = np.abs(R.mixed_index('t', 80, 50))
    assert np.array_equal(R.gather(src, idx), _t(src).index_select(0, _t(idx).long()).numpy())
    assert np.array_equal(R.repeat(src, 8), _t(src).repeat_interleave(8, 0).numpy())
    a, b, c = R.real_data('a', (9, 16)), R.real_data('b', (9, 2)), R.real_data('c', (9, 7))
    assert np.array_equal(R.concat([(a, 16, None), (b, 2, None)], 9), torch.cat([_t(a), _t(b)], 1).numpy())
    assert np.array_equal(R.concat([(a, 16, None), (b, 2, None), (c, 7, None)], 9), torch.cat([_t(a), _t(b), _t(c)], 1).numpy())
    assert np.array_equal(R.concat([(a, 16, None), (None, 0, None), (c, 7, None)], 9), torch.cat([_t(a), _t(c)], 1).numpy())
    i = np.array([3, -1, 0, 8, 8, -1, 2, 2, 1], np.int32)
    want = torch.cat([_t(a), _t(R.gather(b, i))], 1).numpy()
    assert np.array_equal(R.concat([(a, 16, None), (b, 2, i)], 9), want)


def test_gather_negative_index_and_scatter_round_trip():
    src = R.move_data(0, 40, 3)
    idx = R.unique_index('rt', 30, 40)
    assert (idx < 0).any() and (idx == 0).any() and (idx == 39).any() and len(set(idx[idx >= 0])) == (idx >= 0).sum()
    g = R.gather(src, idx)
    assert (R.bits(g[idx < 0]) == 0).all()
    back = R.scatter(g, idx, 40)
    hit = np.zeros(40, bool)
    hit[idx[idx >= 0]] = True
    R.assert_same_bits(back[hit], src[hit], 'scatter of a gather')
    assert (R.bits(back[~hit]) == 0).all()
    assert (R.bits(R.scatter(g, idx, 40, live=0)) == 0).all()
    R.assert_same_bits(R.scatter(g, idx, 40, live=99), back, 'live count above m')
    m = R.mixed_index('m', 300, 20)
    assert (m == -1).any() and (m == 0).any() and (m == 19).any()


@pytest.mark.parametrize('use_idx', [(False, False, False), (True, False, True), (True, True, True)])
def test_concat_adjoint_is_the_transpose(use_idx):
    m, widths = 65, (5, 0, 3)
    srcs, idxs, ns = [], [], []
    for w, (c, ui) in enumerate(zip(widths, use_idx)):
        n = m + 3
        ns.append(n)
        idxs.append(R.unique_index(('adj', w), m, n) if ui else None)
        srcs.append(R.int_data(('adj', w), (n, c)) if c else None)
    d = R.int_data('adj d', (m, sum(widths)))
    y = R.concat(list(zip(srcs, widths, idxs)), m)
    grads = R.concat_bwd(d, [(c, i, n, True) for c, i, n in zip(widths, idxs, ns)], m)
    lhs = float((y.astype(np.float64) * d).sum())
    rhs = sum(float((s.astype(np.float64) * g).sum()) for s, (g, _) in zip(srcs, grads) if g is not None)
    assert lhs == rhs and grads[1] == (None, None)
    for (g, written), i in zip(grads, idxs):
        if g is not None:
            assert written.all() if i is not None else (written[:m].all() and not written[m:].any())
    assert R.concat_bwd(d, [(5, None, m, False), (0, None, m, True), (3, None, m, True)], m)[0] == (None, None)


def test_sums_are_sequential_float32():
    src = R.int_data('s', (30, 4))
    table = np.random.default_rng(1).integers(-1, 30, (27, 12)).astype(np.int32)
    want = sum(np.where(table[k, :10, None] >= 0, src[np.maximum(table[k, :10], 0)], 0).astype(np.float64) for k in range(27))
    assert np.array_equal(R.gather_sum(src, table, 10), want.astype(np.float32))
    assert np.array_equal(R.sum_groups(R.int_data('g', (35, 3)), 7, 5), R.int_data('g', (35, 3)).reshape(7, 5, 3).sum(1))
    x = R.real_data('x', (16, 1))
    acc = np.float32(0)
    for t in range(16):
        acc = np.float32(acc + x[t, 0])
    assert R.sum_groups(x, 1, 16)[0, 0] == acc
    assert R.bits(R.gather_sum(x, np.full((3, 2), -1, np.int32), 2)).tolist() == [[0], [0]]          # +0, not -0
    assert np.array_equal(R.add(x, x), (_t(x) + _t(x)).numpy())


def test_sparse_dense_and_copy():
    coords = np.array([(0, 0, 0, 0), (2, 4, 6, 1), (3, 0, 0, 0), (0, 0, 0, 2), (1, -1, 0, 0), (1, 2, 3, 1)], np.int32)
    feats = R.move_data(4, 6, 3)
    dense = R.sparse_to_dense(feats, coords, 2, (3, 5, 7))
    assert dense.shape == (2, 3, 3, 5, 7) and np.count_nonzero(R.bits(dense)) <= 9
    R.assert_same_bits(dense[1, :, 2, 4, 6], feats[1], 'site')
    back = R.dense_to_sparse(dense, coords)
    R.assert_same_bits(back[[0, 1, 5]], feats[[0, 1, 5]], 'round trip')
    assert (R.bits(back[[2, 3, 4]]) == 0).all()
    mem = np.arange(100, dtype=np.uint8)
    out = R.copy_multi(mem, [(50, 0, 7), (60, 60, 5), (70, 10, 0)])
    assert out[50:57].tolist() == list(range(7)) and np.array_equal(np.delete(out, range(50, 57)), np.delete(mem, range(50, 57)))


def test_compaction_reference():
    for n in R.COMPACT_SIZES:
        for name, mask in R.masks(n).items():
            ref = R.compaction(mask)
            assert np.array_equal(ref['sel'], torch.arange(n)[_t(mask)].numpy())
            assert ref['total'] == int(mask.sum()) and not ref['overflow']
    assert 'hole' in R.masks(9000) and not R.masks(9000)['hole'][4096:6144].any() and R.masks(9000)['hole'][6144:].any()
    mask = R.masks(9000)['random']
    t = int(mask[:100].sum())
    assert R.compaction(mask, 100, t - 1)['overflow'] and R.compaction(mask, 100, t - 1)['count_mul'] == 8 * (t - 1)
    assert R.compaction(mask, 100, t - 1)['total'] == t and np.array_equal(R.compaction(mask, 100)['sel'], np.nonzero(mask[:100])[0])
    assert not R.compaction(mask, 100, t)['overflow'] and R.compaction(mask, -1)['total'] == 0
    assert R.compaction(mask, 9009)['total'] == int(mask.sum()) and R.compaction(mask, 0, 0)['overflow'] is False
    x = R.sigmoid_ladder()
    keep, drop = R.sigmoid_rule(x)
    assert not (keep & drop).any() and (~keep & ~drop).sum() > 500         # the band the test only measures
    s = torch.sigmoid(_t(x).double()) > 0.5
    assert s[_t(keep)].all() and not s[_t(drop)].any()


def test_coordinate_references():
    c = np.array([(1, 2, 3, 0), (32767, 32767, 32767, 5)], np.int32)
    e = R.expand8(c)
    assert e[5].tolist() == [3, 4, 7, 0] and e[15].tolist() == [65535, 65535, 65535, 5] and e[8].tolist() == [65534, 65534, 65534, 5]
    z, y, x = np.indices((3, 5, 7)).reshape(3, -1)
    want = np.concatenate([np.stack([z, y, x, np.full_like(z, b)], 1) for b in range(2)])
    assert np.array_equal(R.dense_coords(2, 3, 5, 7), want) and R.dense_coords(0, 3, 5, 7).shape == (0, 4)
    locs = R.clean_locs('c', 10)
    c32, bad = R.coords_from_i64(locs)
    assert not bad and np.array_equal(R.coords_to_i64(c32), locs) and locs[0].tolist() == list(R.COORD_MAX)
    assert len(R.range_cases()) == 8
    for name, col, value in R.range_cases():
        l2 = locs.copy()
        l2[4, col] = value
        assert R.coords_from_i64(l2)[1] and not R.coords_from_i64(l2, 4)[1], name
    sites = R.random_sites('h', 500)
    assert not R.has_duplicates(sites)
    q = np.concatenate([sites[::-1], sites[:3] + np.array([1000, 0, 0, 0], np.int32), [[-1, 0, 0, 0]]]).astype(np.int32)
    assert R.hash_rows(sites, q).tolist() == list(range(499, -1, -1)) + [-1] * 4


def _torch_adam(p, g, m, v, segs, steps, wd):
    """torch.optim.Adam in float64 with each segment's state preset (one parameter tensor per segment)."""
    ps = [torch.nn.Parameter(_t(p[b:e]).double()) for b, e in segs]
    opt = torch.optim.Adam(ps, lr=float(np.float32(1e-2)), betas=(float(np.float32(0.9)), float(np.float32(0.999))),
                           eps=float(np.float32(1e-8)), weight_decay=float(np.float32(wd)))
    for q, (b, e), s in zip(ps, segs, steps):
        q.grad = _t(g[b:e]).double()
        opt.state[q] = {'step': torch.tensor(float(s)), 'exp_avg': _t(m[b:e]).double(), 'exp_avg_sq': _t(v[b:e]).double()}
    opt.step()
    return ps, opt


@pytest.mark.parametrize('wd', [0.0, 1e-3])
def test_adam_reference_is_torch_adam(wd):
    n = 1031
    segs, steps = R.adam_segments(n), [0, 1, 9, 999]
    p, g, m, v = R.adam_state('torch', n)
    p64, m64, v64, steps_out, upd, U = R.adam_step(p, g, m, v, segs, steps, [True] * 4, 1e-2, 0.9, 0.999, 1e-8, wd, 1.0)
    ps, opt = _torch_adam(p, g, m, v, segs, steps, wd)
    for q, (b, e) in zip(ps, segs):
        assert np.allclose(q.detach().numpy(), p64[b:e], rtol=1e-13, atol=0)
        assert np.allclose(opt.state[q]['exp_avg'].numpy(), m64[b:e], rtol=1e-13, atol=0)
        assert np.allclose(opt.state[q]['exp_avg_sq'].numpy(), v64[b:e], rtol=1e-13, atol=0)
    assert steps_out == [1.0, 2.0, 10.0, 1000.0] and not upd[6] and upd.sum() == n - 1 and p64[6] == p[6] and (U[upd] > 0).all()
    half = R.adam_step(p, g, m, v, segs, steps, [True] * 4, 1e-2, 0.9, 0.999, 1e-8, wd, 0.5)
    same = R.adam_step(p, (g * np.float32(0.5)), m, v, segs, steps, [True] * 4, 1e-2, 0.9, 0.999, 1e-8, wd, 1.0)
    assert np.array_equal(half[0], same[0])                       # grad_scale is applied to the gradient first


def test_adam_rules():
    assert R.segment_active(None, None) and R.segment_active(5, None) and not R.segment_active(0, None)
    assert R.segment_active(0, 1.0) and not R.segment_active(5, 0.0) and not R.segment_active(None, 0.0)
    assert R.status_blocks(4) and R.status_blocks(6) and not R.status_blocks(2) and not R.status_blocks(None)
    p, g, m, v = R.adam_state('rules', 1031)
    out = R.adam_step(p, g, m, v, R.adam_segments(1031), [3] * 4, [True] * 4, 1e-2, 0.9, 0.999, 1e-8, 0, 1, status=4)
    assert not out[4].any() and out[3] == [3.0] * 4 and np.array_equal(out[0], p)
    out = R.adam_step(p, g, m, v, R.adam_segments(1031), [3] * 4, [True, False, False, True], 1e-2, 0.9, 0.999, 1e-8, 0, 1)
    assert out[3] == [4.0, 3.0, 3.0, 4.0] and out[4][:5].all() and not out[4][5:1030].any() and out[4][1030]


def _adam_f32(p, g, m, v, segs, steps, lr, b1, b2, eps, wd, scale):
    """The same step in float32 arithmetic, one rounding per operation (no contraction): a stand-in for a correct kernel."""
    f = np.float32
    p, m, v = p.copy(), m.copy(), v.copy()
    for (b, e), s in zip(segs, steps):
        bc1 = f(1.0 - float(f(b1)) ** (s + 1.0))
        bc2s = np.sqrt(f(1.0 - float(f(b2)) ** (s + 1.0)))
        gp = g[b:e] * f(scale)
        if wd:
            gp = gp + p[b:e] * f(wd)
        m[b:e] = m[b:e] + (gp - m[b:e]) * (f(1) - f(b1))
        v[b:e] = f(b2) * v[b:e] + (f(1) - f(b2)) * gp * gp
        p[b:e] = p[b:e] - (f(lr) / bc1) * m[b:e] / (np.sqrt(v[b:e]) / bc2s + f(eps))
    return p, m, v


ADAM_ARGS = (1e-2, 0.9, 0.999, 1e-8)


@pytest.mark.parametrize('wd,scale', [(0.0, 1.0), (1e-3, 0.125)])
def test_adam_bars_hold_for_a_float32_step_and_reject_wrong_ones(wd, scale):
    n = 4099
    segs, steps, on = R.adam_segments(n), [1, 9, 999, 100000], [True] * 4
    p, g, m, v = R.adam_state(('bars', wd), n)
    ref = R.adam_step(p, g, m, v, segs, steps, on, *ADAM_ARGS, wd, scale)
    ratio = R.assert_adam(*_adam_f32(p, g, m, v, segs, steps, *ADAM_ARGS, wd, scale), ref, (p, m, v), 'float32 step')
    assert ratio < 1.0
    # a segment that misses its last element
    short = [(b, e - 1) if t == 2 else (b, e) for t, (b, e) in enumerate(segs)]
    with pytest.raises(AssertionError, match='bound|ulp'):
        R.assert_adam(*_adam_f32(p, g, m, v, short, steps, *ADAM_ARGS, wd, scale), ref, (p, m, v), 'short segment')
    one = [(b, e - 1) if t == 1 else (b, e) for t, (b, e) in enumerate(segs)]        # the one-element segment: empty
    with pytest.raises(AssertionError):
        R.assert_adam(*_adam_f32(p, g, m, v, one, steps, *ADAM_ARGS, wd, scale), ref, (p, m, v), 'empty segment')
    # bias correction from `step` instead of `step + 1`
    with pytest.raises(AssertionError, match='bound'):
        R.assert_adam(*_adam_f32(p, g, m, v, segs, [s - 1 for s in steps], *ADAM_ARGS, wd, scale), ref, (p, m, v), 'bias')
    # element 6 updated although it lies in no segment
    with pytest.raises(AssertionError, match='outside the active segments'):
        R.assert_adam(*_adam_f32(p, g, m, v, [(0, 7)] + segs[2:], [1, 999, 100000], *ADAM_ARGS, wd, scale), ref, (p, m, v), 'gap')


# ---- the helpers notice wrong kernels on the GPU tests' data ----

def _as_output(arr, spoil=None):
    """arr as it would come back from the device: inside a guarded buffer (spoil(buffer array) edits it in place)."""
    g = R.guarded(arr.shape, arr.dtype)
    full = g.full.copy()
    g.inner(full)[...] = arr
    if spoil:
        spoil(g, full)
    return g, full


def test_helpers_accept_the_reference_and_see_guards():
    want = R.gather(R.move_data(0, 35, 5), R.mixed_index('x', 65, 35))
    g, full = _as_output(want)
    R.assert_same_bits(g.check(full, 'ok'), want, 'ok')
    for where in (g.lead - 1, g.lead + g.size):
        bad = full.copy()
        bad[where] = 0
        with pytest.raises(AssertionError, match='front of|past the end'):
            g.check(bad, 'guard')
    with pytest.raises(AssertionError, match='untouched'):
        g.check(full, 'rows', untouched=(np.arange(65) >= 64)[:, None])
    neg = want.copy()
    neg[want == 0] = -0.0
    if (want == 0).any():
        with pytest.raises(AssertionError, match='differ'):
            R.assert_same_bits(neg, want, '-0 for +0')
    for shift in (0, 1):
        assert R.guarded((3, 4), np.float32, shift).offset_bytes % 16 == 4 * shift


@pytest.mark.parametrize('c,m', [(1, 1), (5, 65), (16, 257), (48, 4097)])
def test_wrong_row_kernels_are_rejected(c, m):
    n_src = max(2, m // 2 + 3)
    src, idx = R.move_data(0, n_src, c), R.mixed_index('gather_rows c=%d m=%d shift=0' % (c, m), m, n_src)
    want = R.gather(src, idx)
    wrong = {}
    w = want.copy()
    w[:, -1] = 0                                                     # last element of a row dropped
    wrong['row tail dropped'] = w
    if m > 1:
        wrong['index off by one'] = R.gather(src, np.where(idx >= 0, (idx + 1) % n_src, idx))
        wrong['negative index read as row 0'] = R.gather(src, np.maximum(idx, 0))
        assert (idx < 0).any()
    for name, w in wrong.items():
        with pytest.raises(AssertionError, match='differ'):
            R.assert_same_bits(w, want, name)
    # the summing kernels on their integer data: a dropped last slice changes a sum
    x = R.int_data('sum_groups', (m * 5, c))
    short = R.sum_groups(x.reshape(m, 5, c)[:, :4].reshape(m * 4, c), m, 4)
    if m > 1:
        with pytest.raises(AssertionError, match='differ'):
            R.assert_same_bits(short, R.sum_groups(x, m, 5), 'last slice dropped')


@pytest.mark.parametrize('widths', [(16, 2), (3, 4), (16, 2, 8), (16, 2, 30), (16, 2, 47)])
def test_wrong_concat_boundary_is_rejected(widths):
    m = 65
    parts = [(R.move_data(w, m + 3, c), c, R.mixed_index(('cat', w), m, m + 3) if w != 1 else None) for w, c in enumerate(widths)]
    want = R.concat(parts, m)
    wrong = want.copy()
    wrong[:, widths[0] - 1] = want[:, widths[0]]          # the boundary one column early: b's first column taken for a's last
    with pytest.raises(AssertionError, match='differ'):
        R.assert_same_bits(wrong, want, 'boundary')
    d = R.move_data(7, m, sum(widths))
    spec = [(c, R.unique_index(('catb', w), m, m + 3) if w == 0 else None, m + 3, True) for w, c in enumerate(widths)]
    (va, wa), (vb, wb) = R.concat_bwd(d, spec, m)[:2]
    assert wa.all() and not wb[m:].any()
    g, full = _as_output(vb, lambda g, full: g.inner(full).__setitem__(slice(m, None), R.sentinel(np.float32)))
    g.check(full, 'direct destination', untouched=~wb)
    full2 = full.copy()
    g.inner(full2)[m] = 0                                                # a direct destination zero-filled past row m
    with pytest.raises(AssertionError, match='untouched'):
        g.check(full2, 'direct destination', untouched=~wb)


@pytest.mark.parametrize('n', [2049, 4096, 9000])
def test_wrong_compactions_are_rejected(n):
    mask = R.masks(n)['random']
    ref = R.compaction(mask)
    sel = np.full(n, R.SENT_INT, np.int32)
    sel[:ref['total']] = ref['sel']
    R.assert_compaction(sel, [ref['total']], ref, 'ok')
    k0 = int(mask[:R.SCAN_BLOCK].sum())
    off = np.full(n, R.SENT_INT, np.int32)                               # the second block's offset one too high
    off[:k0] = ref['sel'][:k0]
    off[k0 + 1:ref['total'] + 1] = ref['sel'][k0:]
    with pytest.raises(AssertionError):
        R.assert_compaction(off, [ref['total']], ref, 'offset + 1')
    low = sel.copy()                                                     # ... or one too low: a row overwritten
    low[k0 - 1:ref['total'] - 1] = ref['sel'][k0:]
    low[ref['total'] - 1] = R.SENT_INT
    with pytest.raises(AssertionError):
        R.assert_compaction(low, [ref['total']], ref, 'offset - 1')
    capped = R.compaction(mask, None, ref['total'] - 1)
    assert capped['overflow'] and capped['count'] == ref['total'] - 1
    R.assert_compaction(sel, [capped['count'], capped['count_mul']], capped, 'ok')
    with pytest.raises(AssertionError, match='counts'):
        R.assert_compaction(sel, [ref['total'], 8 * ref['total']], capped, 'count not clamped')
    with pytest.raises(AssertionError):
        R.assert_compaction(sel, [ref['total']], R.compaction(mask, n - 1 if mask[n - 1] else int(np.nonzero(mask)[0][-1])), 'n_dev ignored')
