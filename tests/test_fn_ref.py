"""The references of tests/fn_ref.py held themselves (no GPU): the dense k4/s2 restatement against torch's own fp64
ops, the up-sampling reference against the oracle's expand_children + SubmanifoldConvolution, and adjoint_gap on a
reference operator with a hand-written transpose, right and perturbed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import fn_ref as FR
import glue_ref as G
from util import random_sites


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- dense k4 / s2 / p1 ----

@pytest.mark.parametrize('batch,dims,cin,cout', [(2, (4, 8, 6), 3, 5), (1, (8, 8, 8), 4, 2), (3, (2, 2, 2), 2, 2)])
def test_k4s2_restatement_equals_torch_fp64(batch, dims, cin, cout):
    gen = _gen(cin * 10 + cout)
    # integer data: both sides are exact in fp64, so the comparison needs no bar
    x = R.int_data((batch, cin) + tuple(dims), gen, 'cpu').double()
    wd = R.int_data((cout, cin, 4, 4, 4), gen, 'cpu').double()          # nn.Conv3d layout
    wu = R.int_data((cout, cin, 4, 4, 4), gen, 'cpu').double()          # nn.ConvTranspose3d: (in, out, k, k, k)
    xl = x.permute(0, 2, 3, 4, 1).contiguous()
    w_taps = wd.permute(2, 3, 4, 1, 0).reshape(64, cin, cout)
    y, mag = FR.k4s2_down(xl, w_taps)
    want = F.conv3d(x, wd, stride=2, padding=1).permute(0, 2, 3, 4, 1)
    assert y.shape == want.shape
    R.assert_exact(y, want, mag, 'down')
    u_taps = wu.permute(2, 3, 4, 0, 1).reshape(64, cout, cin)
    z, zmag = FR.k4s2_up(y, u_taps)
    want_z = F.conv_transpose3d(want.permute(0, 4, 1, 2, 3), wu, stride=2, padding=1).permute(0, 2, 3, 4, 1)
    assert z.shape == want_z.shape == xl.shape
    R.assert_exact(z, want_z, zmag, 'up')
    # the weight gradient of the down layer, through autograd on torch's op
    wd_ = wd.clone().requires_grad_(True)
    dy = R.int_data(tuple(want.shape), gen, 'cpu').double()
    (F.conv3d(x, wd_, stride=2, padding=1).permute(0, 2, 3, 4, 1) * dy).sum().backward()
    dw, dmag = FR.k4s2_pair(xl, dy)
    R.assert_exact(dw, wd_.grad.permute(2, 3, 4, 1, 0).reshape(64, cin, cout), dmag, 'dW')


def test_k4s2_up_is_the_transpose_of_down_exactly():
    gen = _gen(4)
    x = R.int_data((2, 4, 6, 8, 3), gen, 'cpu')
    w = R.int_data((64, 3, 5), gen, 'cpu')
    dy = R.int_data((2, 2, 3, 4, 5), gen, 'cpu')
    y, _ = FR.k4s2_down(x.double(), w)
    dx, _ = FR.k4s2_up(dy.double(), w.transpose(1, 2))
    assert FR.adjoint_gap(x, dx.float(), y.float(), dy) == 0
    dw, _ = FR.k4s2_pair(x.double(), dy.double())
    assert FR.adjoint_gap(w, dw.float(), y.float(), dy) == 0


def test_slot_order_is_a_permutation_and_inverts():
    w = torch.arange(64.0).view(64, 1, 1)
    assert torch.equal(FR.taps_to_slots(FR.slots_to_taps(w)), w)
    P = FR.k4s2_taps()
    assert float(FR.slots_to_taps(w)[P[5]]) == 5.0          # slot 5 holds tap P[5]
    # parity group g of slot q = q // 8 is the parity of the fine voxel 2o - 1 + k for every tap of the group
    for q, t in enumerate(P):
        k = (t // 16, (t // 4) % 4, t % 4)
        assert tuple((kk - 1) % 2 for kk in k) == ((q >> 5) & 1, (q >> 4) & 1, (q >> 3) & 1)


# ---- up-sampling convolution ----

@pytest.mark.parametrize('cin,cout', [(3, 2), (5, 4)])
def test_expand_reference_equals_oracle_expand_then_subm(cin, cout):
    import model_oracle as mo
    import scn_oracle as oscn
    locs = random_sites(2, 8, 0.2, 4, surface=True)
    gen = _gen(cin)
    f = R.int_data((locs.shape[0], cin), gen, 'cpu')
    w = R.int_data((27, cin, cout), gen, 'cpu')
    conv = oscn.SubmanifoldConvolution(3, cin, cout, 3, False).double()
    with torch.no_grad():
        conv.weight.copy_(w.double())
    fo = f.double().requires_grad_(True)
    locs_c, feats_c = mo.expand_children(locs, fo)
    yo = conv(oscn.InputLayer(3, [16] * 3, mode=0)([locs_c, feats_c])).features
    dy = R.int_data(tuple(yo.shape), gen, 'cpu')
    yo.backward(dy.double())
    assert torch.equal(R.children_coords(locs), locs_c)
    rules = FR.expand_rulebook(locs)
    y, mag = FR.expand_fwd(f, w, rules)
    R.assert_exact(yo.detach(), y, mag, 'forward')
    R.assert_exact(fo.grad, *FR.expand_df(dy, w, rules), 'df')
    R.assert_exact(conv.weight.grad, *FR.expand_dw(f, dy, rules), 'dw')
    # the parent-rulebook form with the pre-summed weights states the same function
    prules = R.subm_rulebook(locs)
    wc = torch.einsum('st,tio->sio', R.expand_taps(), w.double())
    y2, _ = FR.expand_slot_fwd(f, wc, prules)
    assert torch.equal(y2, y)
    dwc, _ = FR.expand_slot_dwc(f, dy, prules)
    assert torch.equal(torch.einsum('st,sio->tio', R.expand_taps(), dwc), conv.weight.grad)


# ---- adjoint_gap ----

def _gather_pair(seed):
    rng = np.random.default_rng(seed)
    idx = G.unique_index('gap', 40, 64)
    x = rng.integers(-3, 4, (64, 5)).astype(np.float32)
    dy = rng.integers(-3, 4, (40, 5)).astype(np.float32)
    dy[np.abs(dy).sum(1) == 0] = 1
    x[np.abs(x).sum(1) == 0] = 1
    return idx, x, dy


def test_adjoint_gap_is_zero_for_an_operator_and_its_transpose():
    idx, x, dy = _gather_pair(1)
    y = G.gather(x, idx)
    dx = FR.gather_adjoint(dy, idx, 64)
    assert FR.adjoint_gap(x, dx, y, dy) == 0
    parent = np.array([0, 0, 1, 3, 3, 3, 4], np.int64)
    c = np.arange(15, dtype=np.float32).reshape(5, 3) - 6
    d = np.arange(21, dtype=np.float32).reshape(7, 3) - 9
    assert FR.adjoint_gap(c, FR.unpool_adjoint(d, parent, 5), FR.unpool(c, parent), d) == 0
    assert FR.adjoint_gap(c, FR.repeat_adjoint(np.tile(d[:5], (2, 1)), 2), G.repeat(c, 2), np.tile(d[:5], (2, 1))) == 0
    # several arguments jointly
    a, b = c, c[::-1].copy()
    y = G.add(a, b)
    assert FR.adjoint_gap([a, b], [d[:5], d[:5]], y, d[:5]) == 0


def test_adjoint_gap_sees_one_perturbed_index():
    idx, x, dy = _gather_pair(2)
    y = G.gather(x, idx)
    r = int(np.nonzero(idx >= 0)[0][3])
    free = sorted(set(range(64)) - set(idx[idx >= 0].tolist()))
    seen = 0
    for target in free[:8]:              # the row's gradient lands on another source row
        bad = idx.copy()
        bad[r] = target
        seen += FR.adjoint_gap(x, FR.gather_adjoint(dy, bad, 64), y, dy) != 0
    assert seen >= 7                     # (a coincidence needs <dy[r], x[idx[r]] - x[target]> = 0)
    scaled = FR.gather_adjoint(dy, idx, 64)
    scaled[idx[r]] *= 2
    assert FR.adjoint_gap(x, scaled, y, dy) != 0


def test_adjoint_gap_refuses_non_integers():
    x = np.ones((2, 2), np.float32)
    with pytest.raises(AssertionError):
        FR.adjoint_gap(x * 0.5, x, x, x)
    with pytest.raises(AssertionError):
        FR.adjoint_gap(x, x * np.float32('nan'), x, x)
    with pytest.raises(AssertionError):
        FR.adjoint_gap(x.astype(np.float64), x, x, x)
