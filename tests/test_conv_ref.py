"""The fp64 convolution reference of tests/conv_ref.py (used by test_gpu_conv_fp32.py) on CPU tensors with the oracle's
rulebooks: it equals torch's dense conv3d, and its comparators reject near-misses of a correct result."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scn_oracle as oscn
import conv_ref as R


def _dense_block(d, b=1):
    zz, yy, xx, bb = torch.meshgrid(torch.arange(d), torch.arange(d), torch.arange(d), torch.arange(b), indexing='ij')
    return torch.stack([zz, yy, xx, bb], -1).reshape(-1, 4)         # raster order: row = ((z * d + y) * d + x) * b + b_


def _to_dense(rows, d, c):
    return rows.reshape(d, d, d, c).permute(3, 0, 1, 2)[None]          # (1, c, d, d, d)


def _from_dense(t, c):
    return t[0].permute(1, 2, 3, 0).reshape(-1, c)


def _w3(w, k):
    """(k^3, cin, cout) rulebook weight -> conv3d weight (cout, cin, k, k, k)."""
    return w.reshape(k, k, k, w.shape[1], w.shape[2]).permute(4, 3, 0, 1, 2)


def test_walk_equals_dense_conv3d_with_adjoint_and_weight_gradient():
    d, cin, cout = 6, 5, 7
    coords = _dense_block(d)
    nbr = torch.from_numpy(oscn.Grid(coords.numpy()).subm_rules(3))
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(d ** 3, cin, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(27, cin, cout, generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(d ** 3, cout, generator=gen, dtype=torch.float64)
    dense = _from_dense(F.conv3d(_to_dense(x, d, cin), _w3(w, 3), padding=1), cout)
    y, mag = R.walk(x.detach(), w.detach(), nbr, 27, d ** 3, d ** 3)
    assert torch.allclose(y, dense, rtol=1e-12, atol=1e-12)
    assert (mag >= y.abs()).all()
    gx, gw = torch.autograd.grad(dense, (x, w), dy)
    dx, _ = R.walk_adjoint(dy, w.detach(), nbr, 27, d ** 3, d ** 3, d ** 3)
    dw, _ = R.walk_dw(x.detach(), dy, nbr, 27, d ** 3, d ** 3)
    assert torch.allclose(dx, gx, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dw, gw, rtol=1e-12, atol=1e-12)


def test_down2_walk_equals_strided_conv3d():
    d, cin, cout = 8, 4, 6
    coords = _dense_block(d)
    g = oscn.Grid(coords.numpy())
    coarse, parent, off = oscn.down2_rules(g)
    children, _, _ = oscn.down_tables(parent, off, coarse.n)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(d ** 3, cin, generator=gen, dtype=torch.float64)
    w = torch.randn(8, cin, cout, generator=gen, dtype=torch.float64)
    y, _ = R.walk(x, w, torch.from_numpy(children), 8, coarse.n, coarse.n)
    dense = _from_dense(F.conv3d(_to_dense(x, d, cin), _w3(w, 2), stride=2), cout)     # coarse rows in raster order
    cc = torch.from_numpy(coarse.coords)
    order = ((cc[:, 0] * (d // 2) + cc[:, 1]) * (d // 2) + cc[:, 2]).long()
    assert torch.allclose(y, dense[order], rtol=1e-12, atol=1e-12)


def test_grouped_walk_with_kmap_kadd_in_mul_and_in_shift():
    """The generalised walk restated entry by entry, straight from the sgnn_conv_fwd_ex contract."""
    gen = torch.Generator().manual_seed(2)
    n_in, n_out, cin, cout, K, groups, ld, in_mul, in_shift = 40, 9, 3, 2, 3, 2, 16, 2, 1
    table = torch.randint(-1, n_in // in_mul * 2, (5, ld), generator=gen)     # entries >> 1 stay below n_in / in_mul
    kmap = [4, 0, 2, 1, 3, 0]
    kadd = [0, 1, 1, 0, 1, 0]
    x = torch.randn(n_in, cin, generator=gen, dtype=torch.float64)
    w = torch.randn(groups * K, cin, cout, generator=gen, dtype=torch.float64)
    y, _ = R.walk(x, w, table, K, ld, n_out, kmap, kadd, in_mul, groups, in_shift)
    want = torch.zeros(n_out * groups, cout, dtype=torch.float64)
    for row in range(n_out):
        for g in range(groups):
            for k in range(K):
                e = int(table[kmap[g * K + k], row])
                if e >= 0:
                    want[row * groups + g] += x[(e >> in_shift) * in_mul + kadd[g * K + k]] @ w[g * K + k]
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)


def test_children_rulebook_equals_upsampled_dense_conv3d():
    """expand-then-submanifold: the 8N children and their 27-offset rulebook, built from coordinates only, against a
    dense conv3d of the nearest-neighbour up-sampled block; the tap sums of expand_taps against the same."""
    d, cin, cout = 3, 2, 3
    coords = _dense_block(d)
    ch = R.children_coords(coords)
    nbr = R.subm_rulebook(ch)
    assert torch.equal(torch.from_numpy(oscn.Grid(ch.numpy()).subm_rules(3)), nbr)    # same as the oracle's lookup
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(d ** 3, cin, generator=gen, dtype=torch.float64)
    w = torch.randn(27, cin, cout, generator=gen, dtype=torch.float64)
    y, _ = R.walk(x.repeat_interleave(8, 0), w, nbr, 27, ch.shape[0], ch.shape[0])
    up = _to_dense(x, d, cin).repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    dense = F.conv3d(up, _w3(w, 3), padding=1)[0]                                    # (cout, 2d, 2d, 2d)
    want = dense[:, ch[:, 0], ch[:, 1], ch[:, 2]].t()
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    # the same through the 64 pre-summed slices on the parent rulebook (the library's formulation)
    A = R.expand_taps()
    assert float(A.sum()) == 8 * 27 and (A.sum(0) == 8).all()
    wc = torch.einsum('st,tio->sio', A, w)
    pn = torch.from_numpy(oscn.Grid(coords.numpy()).subm_rules(3))
    S = []
    for g in range(8):
        for i in range(8):
            o = [((i >> s) & 1) - 1 + ((g >> s) & 1) for s in (2, 1, 0)]
            S.append((o[0] + 1) * 9 + (o[1] + 1) * 3 + (o[2] + 1))
    y8, _ = R.walk(x, wc, pn, 8, d ** 3, d ** 3, kmap=S, groups=8)
    assert torch.allclose(y8, want, rtol=1e-12, atol=1e-12)


@pytest.fixture(scope='module')
def case():
    locs = np.stack(np.nonzero(np.random.default_rng(4).random((9, 9, 9)) < 0.5), 1)
    coords = np.concatenate([locs, np.zeros((len(locs), 1), np.int64)], 1)
    nbr = torch.from_numpy(oscn.Grid(coords).subm_rules(3))
    n, c = len(locs), 6
    gen = torch.Generator().manual_seed(5)
    xi, wi = R.int_data((n, c), gen, 'cpu'), R.int_data((27, c, c), gen, 'cpu')
    xr, wr = R.real_data((n, c), gen, 'cpu'), R.real_data((27, c, c), gen, 'cpu') / 12
    return nbr, n, c, xi, wi, xr, wr


def _fp32_walk(x, w, nbr, n):
    """An fp32 walk of the same rules in another order (a stand-in for a correct kernel)."""
    y = torch.zeros(n, w.shape[2])
    for k in reversed(range(27)):
        m = nbr[k] >= 0
        y[m] += x[nbr[k][m]] @ w[k]
    return y


def test_comparators_accept_a_correct_fp32_result(case):
    nbr, n, c, xi, wi, xr, wr = case
    ref, mag = R.walk(xi, wi, nbr, 27, n, n)
    R.assert_exact(_fp32_walk(xi, wi, nbr, n), ref, mag)
    ref, mag = R.walk(xr, wr, nbr, 27, n, n)
    R.assert_close(_fp32_walk(xr, wr, nbr, n), ref, mag)


def test_comparators_reject_one_dropped_rule(case):
    nbr, n, c, xi, wi, xr, wr = case
    k, j = 4, int((nbr[4] >= 0).nonzero()[0])
    cut = nbr.clone()
    cut[k, j] = -1
    ref, mag = R.walk(xi, wi, nbr, 27, n, n)
    assert (xi[nbr[k, j]] @ wi[k]).abs().sum() > 0
    assert R.exact_mismatch(_fp32_walk(xi, wi, cut, n), ref, mag) is not None
    ref, mag = R.walk(xr, wr, nbr, 27, n, n)
    assert R.close_mismatch(_fp32_walk(xr, wr, cut, n), ref, mag) is not None


def test_comparators_reject_one_transposed_offset(case):
    nbr, n, c, xi, wi, xr, wr = case
    for x, w, check in ((xi, wi, R.exact_mismatch), (xr, wr, R.close_mismatch)):
        bad = w.clone()
        bad[20] = w[20].t()
        ref, mag = R.walk(x, w, nbr, 27, n, n)
        assert check(_fp32_walk(x, bad, nbr, n), ref, mag) is not None


def test_comparator_rejects_a_bf16_rounded_result(case):
    nbr, n, c, xi, wi, xr, wr = case
    ref, mag = R.walk(xr, wr, nbr, 27, n, n)
    y = _fp32_walk(xr, wr, nbr, n)
    assert R.close_mismatch(y.bfloat16().float(), ref, mag) is not None
    # and a NaN is never inside the bar
    y[3, 2] = float('nan')
    assert R.close_mismatch(y, ref, mag) is not None


def test_exact_comparison_refuses_data_past_the_fp32_integer_range():
    ref = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(AssertionError, match='2\\^24'):
        R.exact_mismatch(ref.float(), ref, torch.full_like(ref, 2.0 ** 24))
