"""CPU checks of tests/bn_ref.py: the fp64 restatement agrees with torch (batch_norm + leaky_relu, autograd, linear), and
its comparators reject near-misses of the kind a subtly wrong kernel would produce."""
import numpy as np
import torch
import torch.nn.functional as F

import bn_ref as B

EPS = 1e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _torch_bn(x, gamma, beta, rm, rv, momentum, training, leak):
    """torch float64 BatchNorm + leaky ReLU; torch's momentum is the weight of the NEW value."""
    y = F.batch_norm(x, rm, rv, gamma, beta, training=training, momentum=1 - momentum, eps=EPS)
    return F.leaky_relu(y, leak)


def test_forward_and_running_stats_match_torch():
    g = _gen(1)
    for n, c, leak in ((1, 3, 0.0), (2, 5, 0.25), (37, 16, 1.0), (1000, 7, 0.0)):
        x = torch.randn(n, c, generator=g, dtype=torch.float64) * 3 + 1
        gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
        for training in (True, False):
            rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
            rm_t, rv_t = rm.clone(), rv.clone()
            m = float(torch.tensor(0.9, dtype=torch.float32))
            if training and n == 1:      # torch refuses one row per channel in training; the library's factor is 1
                st = B.bn_stats(x, EPS, 0.9, rm, rv, True)
                assert torch.equal(st['var'], torch.zeros(c, dtype=torch.float64))
                assert torch.allclose(st['rv'], m * rv, rtol=0, atol=1e-15)
                continue
            want = _torch_bn(x, gamma, beta, rm_t, rv_t, m, training, leak)
            st = B.bn_stats(x, EPS, 0.9, rm, rv, training)
            y, _, _ = B.bn_apply(x, st['mean'], st['invstd'], gamma, beta, leak)
            assert torch.allclose(y, want, rtol=1e-12, atol=1e-12), (n, c, training)
            assert torch.allclose(st['rm'], rm_t, rtol=1e-12, atol=1e-14)
            assert torch.allclose(st['rv'], rv_t, rtol=1e-12, atol=1e-14)


def test_empty_level_leaves_running_stats():
    rm, rv = torch.randn(4, dtype=torch.float64), torch.rand(4, dtype=torch.float64)
    st = B.bn_stats(torch.zeros(0, 4), EPS, 0.9, rm, rv, True)
    assert torch.equal(st['mean'], torch.zeros(4, dtype=torch.float64)) and torch.equal(st['invstd'], st['mean'])
    assert torch.equal(st['rm'], rm) and torch.equal(st['rv'], rv)


def test_backward_matches_autograd():
    g = _gen(2)
    for n, c, leak, training, affine, add in ((50, 6, 0.0, True, True, False), (64, 4, 0.25, True, False, True),
                                              (33, 3, 1.0, False, True, True), (2, 8, 0.0, True, True, False)):
        x = (torch.randn(n, c, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
        gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True) if affine else None
        beta = (torch.randn(c, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True) if affine else None
        rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
        y = _torch_bn(x, gamma, beta, rm.clone(), rv.clone(), 0.9, training, leak)
        dy = torch.randn(n, c, generator=g, dtype=torch.float64)
        addend = torch.randn(n, c, generator=g, dtype=torch.float64) if add else None
        y.backward(dy)
        st = B.bn_stats(x.detach(), EPS, 0.9, rm, rv, training)
        r = B.bn_backward(x.detach(), dy, st['mean'], st['invstd'], None if gamma is None else gamma.detach(),
                          None if beta is None else beta.detach(), leak, training, addend)
        want_dx = x.grad + (addend if add else 0)
        assert torch.allclose(r['dx'], want_dx, rtol=1e-10, atol=1e-10)
        if affine:
            assert torch.allclose(r['dgamma'], gamma.grad, rtol=1e-10, atol=1e-10)
            assert torch.allclose(r['dbeta'], beta.grad, rtol=1e-10, atol=1e-10)
        assert (r['dx_mag'] >= r['dx'].abs() - 1e-12).all()


def test_linear_matches_torch():
    g = _gen(3)
    x = torch.randn(300, 12, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(2, 12, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(2, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.linear(x, w, b)
    dy = torch.randn(300, 2, generator=g, dtype=torch.float64)
    y.backward(dy)
    ry, mag = B.linear_fwd(x.detach(), w.detach(), b.detach())
    assert torch.allclose(ry, y.detach(), rtol=1e-13, atol=1e-13) and (mag >= ry.abs() - 1e-12).all()
    r = B.linear_bwd(x.detach(), dy, w.detach())
    assert torch.allclose(r['dx'], x.grad) and torch.allclose(r['dw'], w.grad) and torch.allclose(r['db'], b.grad)


# ---- near-misses: each must be rejected ----

def test_rejects_sequential_fp32_statistics():
    """Statistics summed row after row in fp32 over 10^6 rows of offset data (mean 8, spread 1)."""
    n = 10 ** 6
    x = B.offset_data((n, 1), _gen(4), 'cpu', 8.0)
    st = B.bn_stats(x, EPS)
    xs = x[:, 0].numpy()
    s1 = np.add.accumulate(xs, dtype=np.float32)[-1]           # sequential fp32 sums
    s2 = np.add.accumulate(xs * xs, dtype=np.float32)[-1]
    mean = s1 / np.float32(n)
    var = max(float(s2) / n - float(mean) ** 2, 0.0)
    sm = torch.tensor([mean], dtype=torch.float32)
    si = torch.tensor([1.0 / np.sqrt(var + EPS)], dtype=torch.float32)
    assert B.stats_mismatch(sm, si, st, EPS) is not None
    # while the kernel's scheme (fp32 pairs flushed into fp64) passes
    p1 = (x[0::2, 0] + x[1::2, 0]).double().sum()
    p2 = torch.addcmul(x[0::2, 0] * x[0::2, 0], x[1::2, 0], x[1::2, 0]).double().sum()
    m = p1 / n
    v = p2 / n - m * m
    assert B.stats_mismatch(m.float().reshape(1), (1 / torch.sqrt(v + EPS)).float().reshape(1), st, EPS) is None


def test_rejects_dropped_or_doubled_row_and_swapped_channels():
    g = _gen(5)
    x = torch.randn(4096, 6, generator=g) * 2 + 1
    st = B.bn_stats(x, EPS)
    ok = B.bn_stats(x, EPS)
    assert B.stats_mismatch(ok['mean'].float(), ok['invstd'].float(), st, EPS) is None
    for bad in (x[1:], torch.cat([x, x[:1]]), x[:, [0, 2, 1, 3, 4, 5]]):
        b = B.bn_stats(bad, EPS)
        assert B.stats_mismatch(b['mean'].float(), b['invstd'].float(), st, EPS) is not None
    # integer data: a dropped row moves dbeta, an exact comparison catches it
    xi = B.int_data((1000, 4), g, 'cpu')
    dy = B.int_data((1000, 4), g, 'cpu')
    dy[0] = 2.0                                         # the row that goes missing carries a gradient
    r = B.bn_backward(xi, dy, st['mean'][:4], st['invstd'][:4], leak=0.25)
    assert B.exact_mismatch(B.bn_backward(xi[1:], dy[1:], st['mean'][:4], st['invstd'][:4], leak=0.25)['dbeta'].float(),
                            r['dbeta'], r['dbeta_mag']) is not None


def test_rejects_bf16_invstd():
    x = torch.randn(5000, 8, generator=_gen(6)) * 3 + 0.7
    st = B.bn_stats(x, EPS)
    inv = st['invstd'].float()
    assert B.stats_mismatch(st['mean'].float(), inv, st, EPS) is None
    assert B.stats_mismatch(st['mean'].float(), inv.bfloat16().float(), st, EPS) is not None
    assert B.ulp_mismatch(inv.bfloat16().float(), st['invstd']) is not None
    # and applied with it, the rows leave the apply bar
    y16, _, _ = B.bn_apply(x, st['mean'].float(), inv.bfloat16().float())
    _, t, mag = B.bn_apply(x, st['mean'].float(), inv)
    assert B.apply_mismatch(y16, t, mag, 0.0) is not None


def test_rejects_flipped_mask_away_from_the_boundary():
    x = torch.randn(2000, 5, generator=_gen(7))
    st = B.bn_stats(x, EPS)
    mean, inv = st['mean'].float(), st['invstd'].float()
    y, t, mag = B.bn_apply(x, mean, inv, leak=0.25)
    assert B.apply_mismatch(y.float(), t, mag, 0.25) is None
    i = int((t[:, 2].abs() > 0.5).nonzero()[0])
    flipped = y.clone()
    flipped[i, 2] = t[i, 2] * 0.25 if t[i, 2] > 0 else t[i, 2]
    assert B.apply_mismatch(flipped.float(), t, mag, 0.25) is not None
    mask = t > 0
    assert B.mask_mismatch(mask, t, mag) is None
    mask[i, 2] = ~mask[i, 2]
    assert B.mask_mismatch(mask, t, mag) is not None
    dy = torch.randn(2000, 5, generator=_gen(8))
    r = B.bn_backward(x, dy, mean, inv, leak=0.25)
    rf = B.bn_backward(x, dy, mean, inv, leak=0.25, mask=mask)
    assert B.close_mismatch(rf['dx'], r['dx'], r['dx_mag'], B.SUM_BAR) is not None


def test_rejects_fp32_head_weight_gradient_over_a_million_rows():
    """dW summed in fp32 row after row over 10^6 rows of same-sign real data."""
    n = 10 ** 6
    g = _gen(9)
    x = torch.rand(n, 4, generator=g)
    dy = torch.rand(n, 1, generator=g)
    r = B.linear_bwd(x, dy, torch.ones(1, 4))
    seq = np.stack([np.add.accumulate((dy[:, 0] * x[:, k]).numpy(), dtype=np.float32)[-1] for k in range(4)])
    assert B.close_mismatch(torch.from_numpy(seq).reshape(1, 4), r['dw'], r['dw_mag'], B.SUM_BAR) is not None
    # one fp32 rounding of the exact value passes
    assert B.close_mismatch(r['dw'].float(), r['dw'], r['dw_mag'], B.SUM_BAR) is None


def test_exact_bound_is_asserted():
    import pytest
    with pytest.raises(AssertionError, match='2\\^24'):
        B.assert_int_bound(torch.tensor([2.0 ** 24]))
