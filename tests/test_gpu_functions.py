"""The autograd layer (sgnn_amd/scn/functions.py) Function by Function: forward against a host reference (tests/fn_ref.py
and the *_ref modules it builds on) and backward as the exact adjoint of forward.

Two checks on every case:
  a. forward (and every gradient) against the reference, bit for bit on integer data ({-3..3}: every sum here stays below
     2^24, the longest being a weight gradient over 65 536 rows x 9), within conv_ref.BAR / bn_ref's bars on real data;
  b. for every argument a Function is linear in: adjoint_gap(a, a.grad, y, dy) == 0 exactly.
The host-side routing is part of what is tested: the `calls` fixture records every library call a Function makes, and
each case asserts the route it is named after (tap split with G slices / plain call, in_shift + sum_groups, parity
groups / 64-offset walk, capacity-mode gather, ...), so a changed threshold fails the case instead of emptying it."""
import zlib

import numpy as np
import pytest
import torch

import bn_ref as B
import conv_ref as R
import fn_ref as FR
import glue_ref as G
from util import random_sites

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TRANSPOSE_W, FLIP_K = 1, 2
NAN = float('nan')


def _F():
    from sgnn_amd.scn import functions as F_
    return F_


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _data(shape, gen, integer, lim=3, scale=1.0):
    return R.int_data(shape, gen, DEV, lim) if integer else R.real_data(shape, gen, DEV, scale)


def _check(y, ref, mag, integer, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(ref.shape), '%s: %s %s' % (what, y.dtype, tuple(y.shape))
    (R.assert_exact if integer else R.assert_close)(y.detach(), ref, mag, what)


def _leaf(t, grad=True):
    return t.clone().requires_grad_(grad)


def _grid_from_locs(locs):
    from sgnn_amd.scn.metadata import Grid, coords_from_locs
    return Grid(coords_from_locs(locs, torch.device(DEV)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


# ---- the routes a Function took, read off its library calls ----

@pytest.fixture
def calls(monkeypatch):
    """Every _lib.call made while the test runs, as (name, args); the calls go through unchanged."""
    from sgnn_amd import _lib as L
    log, real = [], L.call

    def spy(name, *args):
        log.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(L, 'call', spy)
    return log


def routes(log):
    """The log's convolution and row-sum calls as tuples:
      ('plain', n_out, K, flags, in_shift)        sgnn_conv_fwd
      ('ex', n_out, K per group, groups, flags, table rows)   sgnn_conv_fwd_ex
      ('sum', n, rep)                             sgnn_sum_groups
      ('dw', n_out, K, in_shift) / ('dw_ex', n_out, K per group, groups)   the weight gradients
      ('gather', idx pointer) / ('gather_dn',) / ('scatter', has m_dev)"""
    out = []
    for name, a in log:
        if name == 'sgnn_conv_fwd':
            out.append(('plain', a[7], a[4], a[10], a[11]))
        elif name == 'sgnn_conv_fwd_ex':
            out.append(('ex', a[7], a[4], a[15], a[10], a[16]))
        elif name == 'sgnn_sum_groups':
            out.append(('sum', a[2], a[3]))
        elif name == 'sgnn_conv_bwd_weight':
            out.append(('dw', a[8], a[7], a[10]))
        elif name == 'sgnn_conv_bwd_weight_ex':
            out.append(('dw_ex', a[8], a[7], a[14]))
        elif name == 'sgnn_gather_rows':
            out.append(('gather', a[2]))
        elif name == 'sgnn_gather_rows_dn':
            out.append(('gather_dn',))
        elif name == 'sgnn_scatter_rows':
            out.append(('scatter', a[6] is not None))
    return out


def split_G(n_out, K=64):
    """The slice count conv_fwd_split is documented to choose: doubled while it divides K and tiles * G < 1024."""
    tiles, g = (n_out + 63) // 64, 1
    while g * 2 <= K and K % (g * 2) == 0 and tiles * g < 1024:
        g *= 2
    return g


def split_route(n_out, cin, cout, flags, K=64):
    """What a conv_fwd_split call over n_out rows must have issued."""
    g = split_G(n_out, K)
    if g == 1 or (cin, cout) not in _F()._SPLIT_SHAPES:
        return [('plain', n_out, K, flags, 0)]
    return [('ex', n_out, K // g, g, flags, K), ('sum', n_out, g)]


def assert_routes(got, want, what):
    for r in want:
        assert r in got, '%s: route %r not taken; calls were %r' % (what, r, got)


def test_split_rule_gives_the_documented_slice_counts():
    # tiles = ceil(n / 64): 31 tiles still take 64 slices, 32 tiles (1985 .. 2048 rows) 32
    assert [split_G(n) for n in (64, 512, 1984, 1985, 2048, 4096, 8192, 16384, 32768, 65536, 10 ** 6)] == \
        [64, 64, 64, 32, 32, 16, 8, 4, 2, 1, 1]
    S = _F()._SPLIT_SHAPES
    assert {(16, 24), (24, 16), (28, 56), (56, 28), (32, 64), (64, 32)} <= S and (16, 16) not in S


# ---- SparseConv ----

@pytest.fixture(scope='module')
def levels():
    from sgnn_amd.scn.metadata import build_down2
    g = _grid_from_locs(random_sites(2, 32, 0.1, 5, surface=True))
    d = build_down2(g)
    assert 500 < d.coarse.n < g.n < 16384
    return g, d


def _tables(levels, kind):
    g, d = levels
    if kind == 'K8':      # stride 2: forward over children (coarse rows), data gradient through ptable (fine rows)
        return dict(K=8, fwd=(d.children, d.ldc), n_in=g.n, n_out=d.coarse.n, bwd=(d.ptable, d.ldf), flags=TRANSPOSE_W)
    t = g.subm_table()
    return dict(K=27, fwd=(t, g.ld), n_in=g.n, n_out=g.n, bwd=(t, g.ld), flags=TRANSPOSE_W | FLIP_K)


def _sparse_case(T, cin, cout, needs, integer, calls, in_shift=0, tag=''):
    F_ = _F()
    K, (tf, ldf), (tb, ldb), n_in, n_out, flags = T['K'], T['fwd'], T['bwd'], T['n_in'], T['n_out'], T['flags']
    rep = 1 << in_shift
    assert n_in % rep == 0
    what = 'SparseConv K=%d (%d, %d) needs=%s in_shift=%d %s %s' % (K, cin, cout, needs, in_shift,
                                                                    'int' if integer else 'real', tag)
    gen = _gen('sparse', K, cin, cout, needs, integer, in_shift)
    x = _data((n_in // rep, cin), gen, integer)
    w = _data((K, cin, cout), gen, integer, scale=1.0 / np.sqrt(K * cin))
    dy = _data((n_out, cout), gen, integer)
    xl, wl = _leaf(x, 'x' in needs), _leaf(w, 'w' in needs)
    del calls[:]
    y = F_.SparseConv.apply(xl, wl, tf, ldf, n_out, tb, ldb, n_in, flags, in_shift)
    ref, mag = R.walk(x, w, tf, K, ldf, n_out, in_shift=in_shift)
    _check(y, ref, mag, integer, what + ' forward')
    assert_routes(routes(calls), [('plain', n_out, K, 0, in_shift)], what + ' forward')
    if needs == 'none':
        assert not y.requires_grad
        return
    del calls[:]
    y.backward(dy)
    got = routes(calls)
    if 'x' in needs:
        dref, dmag = R.walk_adjoint(dy, w, tf, K, ldf, n_out, n_in)          # w.r.t. the virtual rows
        want = [('plain', n_in, K, flags, 0)]
        if in_shift:
            dref, dmag = dref.view(n_in // rep, rep, cin).sum(1), dmag.view(n_in // rep, rep, cin).sum(1)
            want.append(('sum', n_in // rep, rep))
        assert_routes(got, want, what + ' dX')
        _check(xl.grad, dref, dmag, integer, what + ' dX')
        if integer:
            assert FR.adjoint_gap(x, xl.grad, y, dy) == 0, what + ': dX is not the adjoint of forward'
    else:
        assert xl.grad is None and not [r for r in got if r[0] in ('plain', 'ex')], what + ': dX computed unasked'
    if 'w' in needs:
        wref, wmag = R.walk_dw(x, dy, tf, K, ldf, n_out, in_shift)
        assert_routes(got, [('dw', n_out, K, in_shift)], what + ' dW')
        _check(wl.grad, wref, wmag, integer, what + ' dW')
        if integer:
            assert FR.adjoint_gap(w, wl.grad, y, dy) == 0, what + ': dW is not the adjoint of forward'
    else:
        assert wl.grad is None and not [r for r in got if r[0] == 'dw'], what + ': dW computed unasked'


@pytest.mark.parametrize('needs', ['x', 'w', 'xw', 'none'])
@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 12)])
@pytest.mark.parametrize('kind', ['K27-plain-flip_transpose', 'K8-plain-transpose'])
def test_sparse_conv_integer_exact_and_adjoint(levels, calls, kind, cin, cout, needs):
    _sparse_case(_tables(levels, kind.split('-')[0]), cin, cout, needs, True, calls)


@pytest.mark.parametrize('kind', ['K27-plain-flip_transpose', 'K8-plain-transpose'])
def test_sparse_conv_real_within_bar(levels, calls, kind):
    _sparse_case(_tables(levels, kind.split('-')[0]), 8, 12, 'xw', False, calls)


@pytest.fixture(scope='module')
def even_level():
    locs = random_sites(2, 24, 0.1, 11, surface=True)
    g = _grid_from_locs(locs[:locs.shape[0] // 4 * 4])
    assert g.n % 4 == 0 and g.n > 1000
    return g


@pytest.mark.parametrize('integer', [True, False], ids=['int', 'real'])
@pytest.mark.parametrize('route', ['in_shift0-plain', 'in_shift1-sum_groups2', 'in_shift2-sum_groups4'])
def test_sparse_conv_in_shift_routes(even_level, calls, route, integer):
    """Table entries are rows of a virtual level of 2^in_shift rows per feature row (x[e >> in_shift]); the data
    gradient is taken on the virtual rows and summed over each group."""
    g = even_level
    t = g.subm_table()
    T = dict(K=27, fwd=(t, g.ld), n_in=g.n, n_out=g.n, bwd=(t, g.ld), flags=TRANSPOSE_W | FLIP_K)
    _sparse_case(T, 8, 12, 'xw', integer, calls, in_shift=int(route[8]), tag=route)


# ---- DenseK4S2 ----

def _dense_case(batch, fdims, cin, cout, down, parity, integer, calls, what):
    """One DenseK4S2 forward + backward on the (batch, fdims) geometry against the strided-slice restatement.  (cin, cout)
    are the Function's: the down layer reads cin channels on the fine level, the up layer cin on the coarse level."""
    from sgnn_amd import model as M
    F_ = _F()
    lvl = M.dense_geometry(batch, fdims, torch.device(DEV)).level(0)
    cdims = [d // 2 for d in fdims]
    n_f, n_c = batch * fdims[0] * fdims[1] * fdims[2], batch * cdims[0] * cdims[1] * cdims[2]
    assert (lvl.n_f, lvl.n_c) == (n_f, n_c)
    n_in, n_out = (n_f, n_c) if down else (n_c, n_f)
    gen = _gen('dense', batch, tuple(fdims), cin, cout, down, parity, integer)
    x = _data((n_in, cin), gen, integer)
    w = _data((64, cin, cout), gen, integer, scale=1.0 / np.sqrt(8 * cin))        # slot order
    dy = _data((n_out, cout), gen, integer)
    xl, wl = _leaf(x), _leaf(w)
    del calls[:]
    y = F_.DenseK4S2.apply(xl, wl, lvl, down, parity)
    fwd = routes(calls)
    wt = FR.slots_to_taps(w)
    xv = FR.rows_to_vol(x, batch, fdims if down else cdims)
    dyv = FR.rows_to_vol(dy, batch, cdims if down else fdims)
    ref, mag = (FR.k4s2_down if down else FR.k4s2_up)(xv, wt)
    _check(y, FR.vol_to_rows(ref), FR.vol_to_rows(mag), integer, what + ' forward')
    del ref, mag
    del calls[:]
    y.backward(dy)
    bwd = routes(calls)
    dref, dmag = (FR.k4s2_up if down else FR.k4s2_down)(dyv, wt.transpose(1, 2))
    _check(xl.grad, FR.vol_to_rows(dref), FR.vol_to_rows(dmag), integer, what + ' dX')
    del dref, dmag
    if down:
        wref, wmag = FR.k4s2_pair(xv, dyv)
    else:
        wref, wmag = [t.transpose(1, 2) for t in FR.k4s2_pair(dyv, xv)]
    _check(wl.grad, FR.taps_to_slots(wref), FR.taps_to_slots(wmag), integer, what + ' dW')
    if integer:
        assert FR.adjoint_gap(x, xl.grad, y, dy) == 0, what + ': dX is not the adjoint of forward'
        assert FR.adjoint_gap(w, wl.grad, y, dy) == 0, what + ': dW is not the adjoint of forward'
    # ---- routes: the coarse side sees 64 taps (tdown), the fine side 8 parity groups or the 64-offset walk (tup) ----
    coarse_fwd = split_route(n_c, cin, cout, 0) if down else None
    coarse_bwd = None if down else split_route(n_c, cout, cin, TRANSPOSE_W)
    if parity:
        fine = lambda flags: [('ex', n_c, 8, 8, flags, 27), ('gather', lvl.child_of_raster.data_ptr())]
    else:
        fine = lambda flags: split_route(n_f, *((cout, cin) if down else (cin, cout)), flags)
    assert_routes(fwd, coarse_fwd if down else fine(0), what + ' forward')
    assert_routes(bwd, fine(TRANSPOSE_W) if down else coarse_bwd, what + ' dX')
    if down:
        assert_routes(bwd, [('dw', n_c, 64, 0)], what + ' dW')
    elif parity:
        assert_routes(bwd, [('dw_ex', n_c, 8, 8), ('gather', lvl.raster_of_child.data_ptr())], what + ' dW')
    else:
        assert_routes(bwd, [('dw', n_f, 64, 0)], what + ' dW')
    return fwd, bwd


SMALL_GEO = (2, (8, 16, 16))           # 512 coarse rows (G = 64), 4096 fine rows (G = 16)


@pytest.mark.parametrize('parity', [True, False], ids=['parity', 'tup64'])
@pytest.mark.parametrize('down', [True, False], ids=['down', 'up'])
@pytest.mark.parametrize('a,b,route', [(16, 24, 'split'), (16, 16, 'plain_outside_split_shapes'), (28, 56, 'split'),
                                       (32, 64, 'split')])
def test_dense_k4s2_shapes_and_directions(calls, a, b, route, down, parity):
    """The layer pair Conv3d(a -> b) / ConvTranspose3d(b -> a) at the smallest geometry."""
    F_ = _F()
    assert ((a, b) in F_._SPLIT_SHAPES) == (route == 'split') and ((b, a) in F_._SPLIT_SHAPES) == (route == 'split')
    assert split_G(512) == 64 and split_G(4096) == 16
    cin, cout = (a, b) if down else (b, a)
    what = 'DenseK4S2 (%d, %d) %s %s' % (cin, cout, 'down' if down else 'up', 'parity' if parity else 'tup64')
    fwd, bwd = _dense_case(SMALL_GEO[0], SMALL_GEO[1], cin, cout, down, parity, True, calls, what)
    ex = [r for r in fwd + bwd if r[0] == 'ex' and r[5] == 64]
    assert bool(ex) == (route == 'split'), what + ': %r' % (fwd + bwd,)


@pytest.mark.parametrize('parity', [True, False], ids=['parity', 'tup64'])
@pytest.mark.parametrize('down', [True, False], ids=['down', 'up'])
def test_dense_k4s2_real_within_bar(calls, down, parity):
    cin, cout = (16, 24) if down else (24, 16)
    _dense_case(SMALL_GEO[0], SMALL_GEO[1], cin, cout, down, parity, False, calls, 'DenseK4S2 real down=%s' % down)


# coarse rows -> (batch, fine dims, G on the coarse side)
COARSE_GEO = [(512, 2, (8, 16, 16), 64), (2048, 2, (16, 16, 32), 32), (4096, 2, (16, 32, 32), 16),
              (8192, 2, (32, 32, 32), 8), (16384, 2, (32, 32, 64), 4), (32768, 1, (64, 64, 64), 2),
              (65536, 2, (64, 64, 64), 1)]


@pytest.mark.parametrize('down', [True, False], ids=['down_fwd', 'up_dx'])
@pytest.mark.parametrize('n_c,batch,fdims,G', COARSE_GEO, ids=['coarse%d-G%d' % (c[0], c[3]) for c in COARSE_GEO])
def test_dense_k4s2_coarse_side_tap_split(calls, n_c, batch, fdims, G, down):
    """Every slice count of conv_fwd_split on the coarse side: Conv3d forward and ConvTranspose3d data gradient of the
    (16, 24) pair.  G = 4 and 8 are what the training batch sizes take; G = 1 is the plain call."""
    assert split_G(n_c) == G and (16, 24) in _F()._SPLIT_SHAPES and (24, 16) in _F()._SPLIT_SHAPES
    cin, cout = (16, 24) if down else (24, 16)
    fwd, bwd = _dense_case(batch, fdims, cin, cout, down, True, True, calls, 'DenseK4S2 coarse rows %d G=%d' % (n_c, G))
    got = fwd if down else bwd
    flags = 0 if down else TRANSPOSE_W
    if G == 1:
        assert ('plain', n_c, 64, flags, 0) in got and not [r for r in got if r[0] == 'ex' and r[5] == 64]
    else:
        assert ('ex', n_c, 64 // G, G, flags, 64) in got and ('sum', n_c, G) in got


FINE_GEO = [(16384, 1, (16, 32, 32), 4), (65536, 2, (32, 32, 32), 1)]


@pytest.mark.parametrize('down', [True, False], ids=['down_dx', 'up_fwd'])
@pytest.mark.parametrize('n_f,batch,fdims,G', FINE_GEO, ids=['fine%d-G%d' % (c[0], c[3]) for c in FINE_GEO])
def test_dense_k4s2_fine_side_tap_split(calls, n_f, batch, fdims, G, down):
    """The 64-offset walk over the fine rows (parity off): ConvTranspose3d forward and Conv3d data gradient."""
    assert split_G(n_f) == G
    cin, cout = (16, 24) if down else (24, 16)
    fwd, bwd = _dense_case(batch, fdims, cin, cout, down, False, True, calls, 'DenseK4S2 fine rows %d G=%d' % (n_f, G))
    got = bwd if down else fwd
    flags = TRANSPOSE_W if down else 0
    if G == 1:
        assert ('plain', n_f, 64, flags, 0) in got
    else:
        assert ('ex', n_f, 64 // G, G, flags, 64) in got and ('sum', n_f, G) in got


# ---- ExpandConv / ExpandWeights / expand_conv ----

@pytest.fixture(scope='module')
def expand_level():
    locs = random_sites(1, 24, 0.1, 9, surface=True).to(DEV)
    g = _grid_from_locs(locs)
    prules = R.subm_rulebook(locs)
    assert torch.equal(prules, g.subm_table().view(27, g.ld)[:, :g.n].long())
    return g, prules, FR.expand_rulebook(locs)


def _expand_case(expand_level, cin, cout, integer, calls, what):
    F_ = _F()
    g, _, crules = expand_level
    n = g.n
    gen = _gen('expand', cin, cout, integer)
    f = _data((n, cin), gen, integer)
    w = _data((27, cin, cout), gen, integer, scale=1.0 / np.sqrt(27 * cin))
    dy = _data((8 * n, cout), gen, integer)
    fl, wl = _leaf(f), _leaf(w)
    del calls[:]
    y = F_.expand_conv(fl, wl, g)
    assert_routes(routes(calls), [('ex', n, 8, 8, 0, 27)], what + ' forward')
    _check(y, *FR.expand_fwd(f, w, crules), integer, what + ' forward')
    del calls[:]
    y.backward(dy)
    G_ = F_.EXPAND_DX_SPLIT
    want = [('ex', n, 64 // G_, G_, TRANSPOSE_W, 27), ('dw_ex', n, 8, 8)] + ([('sum', n, G_)] if G_ > 1 else [])
    assert_routes(routes(calls), want, what + ' backward')
    assert 'sgnn_expand_weights_bwd' in [c[0] for c in calls], what + ': dw did not go through ExpandWeights.backward'
    _check(fl.grad, *FR.expand_df(dy, w, crules), integer, what + ' df')
    _check(wl.grad, *FR.expand_dw(f, dy, crules), integer, what + ' dw')
    if integer:
        assert FR.adjoint_gap(f, fl.grad, y, dy) == 0, what + ': df is not the adjoint of forward'
        assert FR.adjoint_gap(w, wl.grad, y, dy) == 0, what + ': dw is not the adjoint of forward'
    return fl.grad


@pytest.mark.parametrize('integer', [True, False], ids=['int', 'real'])
@pytest.mark.parametrize('cin,cout', [(48, 16), (12, 8)])
def test_expand_conv_against_children_reference(expand_level, calls, cin, cout, integer):
    _expand_case(expand_level, cin, cout, integer, calls, 'expand_conv (%d, %d)' % (cin, cout))


@pytest.mark.parametrize('cin,cout', [(48, 16), (12, 8)])
def test_expand_conv_dx_split_1_2_4_8_bit_identical(expand_level, calls, monkeypatch, cin, cout):
    F_ = _F()
    outs = []
    for G_ in (1, 2, 4, 8):
        monkeypatch.setattr(F_, 'EXPAND_DX_SPLIT', G_)
        outs.append(_expand_case(expand_level, cin, cout, True, calls, 'expand_conv (%d, %d) dx split %d' % (cin, cout, G_)))
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize('cin,cout', [(48, 16), (12, 8)])
def test_expand_conv_slot_weight_gradient(expand_level, calls, cin, cout):
    """ExpandConv on a free (64, cin, cout) slot weight: dwc slot by slot, before ExpandWeights.backward folds it."""
    F_ = _F()
    g, prules, _ = expand_level
    n = g.n
    gen = _gen('dwc', cin, cout)
    f, wc, dy = R.int_data((n, cin), gen, DEV), R.int_data((64, cin, cout), gen, DEV), R.int_data((8 * n, cout), gen, DEV)
    fl, wcl = _leaf(f), _leaf(wc)
    y = F_.ExpandConv.apply(fl, wcl, g.subm_table(), g.ld, n)
    R.assert_exact(y.detach(), *FR.expand_slot_fwd(f, wc, prules), 'slot forward')
    y.backward(dy)
    R.assert_exact(wcl.grad, *FR.expand_slot_dwc(f, dy, prules), 'dwc')
    assert FR.adjoint_gap(wc, wcl.grad, y, dy) == 0 and FR.adjoint_gap(f, fl.grad, y, dy) == 0


@pytest.mark.parametrize('cin,cout', [(48, 16), (12, 8)])
def test_expand_weights_and_its_backward(cin, cout):
    F_ = _F()
    A = R.expand_taps().to(DEV)
    gen = _gen('ew', cin, cout)
    w, dwc = R.int_data((27, cin, cout), gen, DEV), R.int_data((64, cin, cout), gen, DEV)
    wl = _leaf(w)
    wc = F_.ExpandWeights.apply(wl)
    R.assert_exact(wc.detach(), torch.einsum('st,tio->sio', A, w.double()), torch.einsum('st,tio->sio', A, w.double().abs()),
                   'ExpandWeights')
    wc.backward(dwc)
    R.assert_exact(wl.grad, torch.einsum('st,sio->tio', A, dwc.double()), torch.einsum('st,sio->tio', A, dwc.double().abs()),
                   'ExpandWeights backward')
    assert FR.adjoint_gap(w, wl.grad, wc, dwc) == 0


# ---- row Functions ----

def _rows_case(fn, src, dy, ref_y, ref_dx, what):
    """One linear row Function: forward and gradient bit for bit, and the adjoint identity."""
    sl = _leaf(_dev(src))
    y = fn(sl)
    G.assert_same_bits(_host(y), ref_y, what + ' forward')
    y.backward(_dev(dy))
    G.assert_same_bits(_host(sl.grad), ref_dx, what + ' gradient')
    assert FR.adjoint_gap(src, _host(sl.grad), _host(y), dy) == 0, what + ': backward is not the adjoint of forward'


@pytest.mark.parametrize('c', [16, 5])
def test_gather_rows(c):
    F_ = _F()
    n, m = 1500, 1000
    idx = G.unique_index('fn-gather', m, n)
    src, dy = G.int_data(('g', c), (n, c)), G.int_data(('gd', c), (m, c))
    _rows_case(lambda s: F_.GatherRows.apply(s, _dev(idx), m), src, dy, G.gather(src, idx), FR.gather_adjoint(dy, idx, n),
               'GatherRows c=%d' % c)


@pytest.mark.parametrize('c', [16, 5])
def test_scatter_rows_plain_gather_backward(calls, c):
    F_ = _F()
    m, n_dst = 1000, 1500
    idx = G.unique_index('fn-scatter', m, n_dst)
    src, dy = G.int_data(('s', c), (m, c)), G.int_data(('sd', c), (n_dst, c))
    _rows_case(lambda s: F_.ScatterRows.apply(s, _dev(idx), n_dst), src, dy, G.scatter(src, idx, n_dst), G.gather(dy, idx),
               'ScatterRows c=%d' % c)
    got = routes(calls)
    assert ('scatter', False) in got and ('gather_dn',) not in got


@pytest.mark.parametrize('c', [16, 5])
@pytest.mark.parametrize('live', ['below', 'equal', 'zero'])
def test_scatter_rows_capacity_mode_gather_dn_backward(calls, live, c):
    """m_cnt: only the first *m_cnt source rows are live.  Rows past the count must not reach dst.  Their gradient rows:
    sgnn_gather_rows_dn processes rows r < *m_dev only (sgnn_hip.h; test_gpu_rows.py holds the kernel to leaving the rest
    unwritten), so they are unspecified memory and nothing is asserted on them; the adjoint identity is taken over the
    live rows, the only ones forward reads."""
    F_ = _F()
    m, n_dst = 1000, 1500
    k = {'below': m - 3, 'equal': m, 'zero': 0}[live]
    idx = G.unique_index('fn-scatter-cap', m, n_dst)
    idx[m - 2] = sorted(set(range(n_dst)) - set(idx.tolist()))[0]      # a valid destination on a dead row
    src, dy = G.int_data(('sc', c), (m, c)), G.int_data(('scd', c), (n_dst, c))
    src[src == 0] = 1                                                  # a dead row that reached dst would show
    sl = _leaf(_dev(src))
    cnt = torch.tensor([k], dtype=torch.int64, device=DEV)
    y = F_.ScatterRows.apply(sl, _dev(idx), n_dst, cnt)
    G.assert_same_bits(_host(y), G.scatter(src, idx, n_dst, k), 'capacity scatter live=%d' % k)
    y.backward(_dev(dy))
    got = routes(calls)
    assert ('scatter', True) in got and ('gather_dn',) in got and not [r for r in got if r[0] == 'gather']
    assert sl.grad.shape == (m, c)
    G.assert_same_bits(_host(sl.grad)[:k], G.gather(dy, idx, k), 'capacity scatter gradient, live rows')
    assert FR.adjoint_gap(src[:k], _host(sl.grad)[:k], _host(y), dy) == 0


def _unpool_family():
    """Parents 0..7 with 1..8 children, parent 8 with none, parent 9 with 8, children in shuffled fine order."""
    rng = np.random.default_rng(5)
    parent, slot = [], []
    for p, k in enumerate([1, 2, 3, 4, 5, 6, 7, 8, 0, 8]):
        parent += [p] * k
        slot += rng.permutation(8)[:k].tolist()
    order = rng.permutation(len(parent))
    return np.array(parent, np.int32)[order], np.array(slot)[order], 10


@pytest.mark.parametrize('c', [16, 5])
def test_unpool_parents_of_0_to_8_children(c):
    F_ = _F()
    parent, slot, nc = _unpool_family()
    nf, ldc = len(parent), 256
    children = FR.children_table(parent, slot, nc, ldc)
    src, dy = G.int_data(('u', c), (nc, c)), G.int_data(('ud', c), (nf, c))
    ref_dx = FR.unpool_adjoint(dy, parent, nc)
    assert (ref_dx[8] == 0).all()
    _rows_case(lambda s: F_.UnPool.apply(s, _dev(parent), nf, _dev(children.reshape(-1)), ldc), src, dy,
               FR.unpool(src, parent), ref_dx, 'UnPool c=%d' % c)


def test_unpool_on_a_stride2_level(levels):
    F_ = _F()
    g, d = levels
    nf, nc = g.n, d.coarse.n
    parent = _host(d.parent)[:nf]
    src, dy = G.int_data('ul', (nc, 16)), G.int_data('uld', (nf, 16))
    _rows_case(lambda s: F_.UnPool.apply(s, d.parent, nf, d.children, d.ldc), src, dy, FR.unpool(src, parent),
               FR.unpool_adjoint(dy, parent, nc), 'UnPool level')


@pytest.mark.parametrize('c', [16, 5])
@pytest.mark.parametrize('rep', [2, 8])
def test_repeat_rows(rep, c):
    F_ = _F()
    n = 700
    src, dy = G.int_data(('r', rep, c), (n, c)), G.int_data(('rd', rep, c), (n * rep, c))
    _rows_case(lambda s: F_.RepeatRows.apply(s, rep), src, dy, G.repeat(src, rep), FR.repeat_adjoint(dy, rep),
               'RepeatRows rep=%d c=%d' % (rep, c))


def _concat_index(kind, m, n):
    if kind == 'none':
        return None
    if kind == 'perm':
        return np.random.default_rng(m + n).permutation(n)[:m].astype(np.int32)
    return G.unique_index('fn-concat', m, n)          # 'neg': some -1


@pytest.mark.parametrize('needs', ['a', 'b', 'ab', 'none'])
@pytest.mark.parametrize('kb', ['none', 'perm', 'neg'])
@pytest.mark.parametrize('ka', ['none', 'perm'])
def test_concat_rows(ka, kb, needs):
    F_ = _F()
    m, ca, cb = 900, 16, 12
    na, nb = (m if ka == 'none' else m + 300), (m if kb == 'none' else m + 200)
    ia, ib = _concat_index(ka, m, na), _concat_index(kb, m, nb)
    a, b = G.int_data(('ca', ka, kb), (na, ca)), G.int_data(('cb', ka, kb), (nb, cb))
    dy = G.int_data(('cd', ka, kb), (m, ca + cb))
    al, bl = _leaf(_dev(a), 'a' in needs), _leaf(_dev(b), 'b' in needs)
    y = F_.ConcatRows.apply(al, None if ia is None else _dev(ia), bl, None if ib is None else _dev(ib), m)
    what = 'ConcatRows ia=%s ib=%s needs=%s' % (ka, kb, needs)
    G.assert_same_bits(_host(y), G.concat([(a, ca, ia), (b, cb, ib)], m), what)
    if needs == 'none':
        assert not y.requires_grad
        return
    y.backward(_dev(dy))
    (da, _), (db, _) = G.concat_bwd(dy, [(ca, ia, na, True), (cb, ib, nb, True)], m)
    for name, leaf, ref in (('a', al, da), ('b', bl, db)):
        if name in needs:
            G.assert_same_bits(_host(leaf.grad), ref, what + ' d' + name)
        else:
            assert leaf.grad is None
    if needs == 'ab':     # linear in (a, b) jointly
        assert FR.adjoint_gap([a, b], [_host(al.grad), _host(bl.grad)], _host(y), dy) == 0, what


def test_add_rows():
    F_ = _F()
    a, b, dy = G.int_data('aa', (777, 12)), G.int_data('ab', (777, 12)), G.int_data('ad', (777, 12))
    al, bl = _leaf(_dev(a)), _leaf(_dev(b))
    y = F_.AddRows.apply(al, bl)
    G.assert_same_bits(_host(y), G.add(a, b), 'AddRows')
    y.backward(_dev(dy))
    G.assert_same_bits(_host(al.grad), dy, 'AddRows da')
    G.assert_same_bits(_host(bl.grad), dy, 'AddRows db')
    assert FR.adjoint_gap([a, b], [_host(al.grad), _host(bl.grad)], _host(y), dy) == 0


def test_sparse_to_dense_and_back_on_a_rectangular_volume():
    F_ = _F()
    batch, dims, c = 3, (4, 6, 5), 12
    vol = dims[0] * dims[1] * dims[2]
    cells = np.random.default_rng(8).permutation(batch * vol)[:200]
    bb, v = cells // vol, cells % vol
    coords = np.stack([v // (dims[1] * dims[2]), (v // dims[2]) % dims[1], v % dims[2], bb], 1).astype(np.int32)
    assert set(bb.tolist()) == {0, 1, 2}
    feats, dd = G.int_data('s2d', (200, c)), G.int_data('s2dd', (batch, c) + dims)
    cd = _dev(coords)
    _rows_case(lambda s: F_.SparseToDenseFn.apply(s, cd, batch, *dims), feats, dd,
               G.sparse_to_dense(feats, coords, batch, dims), G.dense_to_sparse(dd, coords), 'SparseToDenseFn')
    dense, dr = G.int_data('d2s', (batch, c) + dims), G.int_data('d2sd', (200, c))
    _rows_case(lambda s: F_.DenseToSparseFn.apply(s, cd), dense, dr, G.dense_to_sparse(dense, coords),
               G.sparse_to_dense(dr, coords, batch, dims), 'DenseToSparseFn')


# ---- non-contiguous inputs, the dtype guard ----

def _strided(x, dy):
    """x as a column slice of a wider leaf whose other columns hold NaN; dy as a transposed view."""
    base = torch.full((x.shape[0], x.shape[1] + 7), NAN, device=DEV)
    base[:, 3:3 + x.shape[1]] = x
    base.requires_grad_(True)
    xs = base[:, 3:3 + x.shape[1]]
    dyt = dy.t().contiguous().t()
    assert not xs.is_contiguous() and not dyt.is_contiguous()
    return base, xs, dyt


def _assert_strided_grad(base, cin, want, what):
    gb = base.grad
    assert torch.equal(gb[:, 3:3 + cin], want), what + ': gradient through the column slice differs'
    assert (gb[:, :3] == 0).all() and (gb[:, 3 + cin:] == 0).all(), what


@pytest.mark.parametrize('fn', ['SparseConv', 'DenseK4S2', 'ExpandConv'])
def test_conv_functions_take_non_contiguous_x_and_dy(levels, expand_level, fn):
    F_ = _F()
    gen = _gen('strided', fn)
    if fn == 'SparseConv':
        T = _tables(levels, 'K27')
        n_in, n_out, cin, cout = T['n_in'], T['n_out'], 8, 12
        w = R.int_data((27, cin, cout), gen, DEV)
        run = lambda x, w: F_.SparseConv.apply(x, w, T['fwd'][0], T['fwd'][1], n_out, T['bwd'][0], T['bwd'][1], n_in,
                                               T['flags'], 0)
    elif fn == 'DenseK4S2':
        from sgnn_amd import model as M
        lvl = M.dense_geometry(SMALL_GEO[0], SMALL_GEO[1], torch.device(DEV)).level(0)
        n_in, n_out, cin, cout = lvl.n_f, lvl.n_c, 16, 24
        w = R.int_data((64, cin, cout), gen, DEV)
        run = lambda x, w: F_.DenseK4S2.apply(x, w, lvl, True, True)
    else:
        g = expand_level[0]
        n_in, n_out, cin, cout = g.n, 8 * g.n, 12, 8
        w = R.int_data((27, cin, cout), gen, DEV)
        run = lambda x, w: F_.expand_conv(x, w, g)
    x, dy = R.int_data((n_in, cin), gen, DEV), R.int_data((n_out, cout), gen, DEV)
    xl, wl = _leaf(x), _leaf(w)
    y0 = run(xl, wl)
    y0.backward(dy)
    base, xs, dyt = _strided(x, dy)
    w2 = _leaf(w.transpose(1, 2).contiguous())
    y1 = run(xs, w2.transpose(1, 2))                  # the weight as a transposed view too
    assert torch.equal(y1, y0) and torch.isfinite(y1).all(), fn
    y1.backward(dyt)
    _assert_strided_grad(base, cin, xl.grad, fn)
    assert torch.equal(w2.grad.transpose(1, 2), wl.grad), fn + ': weight gradient through the transposed view'


@pytest.mark.parametrize('dtype', [torch.float64, torch.bfloat16])
def test_dtype_guard_raises(levels, dtype):
    F_ = _F()
    T = _tables(levels, 'K27')
    x = torch.zeros(T['n_in'], 8, device=DEV, dtype=dtype)
    w = torch.zeros(27, 8, 12, device=DEV)
    with pytest.raises(TypeError):
        F_.SparseConv.apply(x, w, T['fwd'][0], T['fwd'][1], T['n_out'], T['bwd'][0], T['bwd'][1], T['n_in'], T['flags'], 0)
    with pytest.raises(TypeError):
        F_.SparseConv.apply(x.float(), w.to(dtype), T['fwd'][0], T['fwd'][1], T['n_out'], T['bwd'][0], T['bwd'][1],
                            T['n_in'], T['flags'], 0)
    with pytest.raises(TypeError):
        F_.GatherRows.apply(x, torch.zeros(4, dtype=torch.int32, device=DEV), 4)
    with pytest.raises(TypeError):
        F_.AddRows.apply(x, x)
    with pytest.raises(TypeError):
        F_.BatchNormLeaky.apply(x, None, None, torch.zeros(8, device=DEV), torch.ones(8, device=DEV), 1e-4, 0.9, True, 0.0)


# ---- the memo caches and the shared workspace ----

def _cache_cases(levels, even_level, expand_level):
    """name -> callable returning a tuple of result tensors; together they touch _arange_cache (K = 64 and K = 8 on the
    same device), _expand_cache, _ws_cache (two widths of BatchNorm, two of the heads) and the shared workspace (weight
    gradients on two grids)."""
    from sgnn_amd import model as M
    F_ = _F()
    g, d = levels

    def conv_on(grid, cin, cout, tag):
        def run():
            gen = _gen('cache', tag)
            t = grid.subm_table()
            x, w = _leaf(R.int_data((grid.n, cin), gen, DEV)), _leaf(R.int_data((27, cin, cout), gen, DEV))
            y = F_.SparseConv.apply(x, w, t, grid.ld, grid.n, t, grid.ld, grid.n, TRANSPOSE_W | FLIP_K, 0)
            y.backward(R.int_data((grid.n, cout), gen, DEV))
            return y.detach(), x.grad, w.grad
        return run

    def dense(cin, cout):
        def run():
            gen = _gen('cache-dense', cin)
            lvl = M.dense_geometry(SMALL_GEO[0], SMALL_GEO[1], torch.device(DEV)).level(0)
            x, w = _leaf(R.int_data((lvl.n_f, cin), gen, DEV)), _leaf(R.int_data((64, cin, cout), gen, DEV))
            y = F_.DenseK4S2.apply(x, w, lvl, True, False)
            y.backward(R.int_data((lvl.n_c, cout), gen, DEV))
            return y.detach(), x.grad, w.grad
        return run

    def split_k8():
        gen = _gen('cache-k8')
        x, w = R.int_data((g.n, 16), gen, DEV), R.int_data((8, 16, 24), gen, DEV)
        assert split_G(d.coarse.n, 8) == 8
        return (F_.conv_fwd_split(x, 16, w, 8, d.children, d.ldc, d.coarse.n, 24, 0),)

    def expand(cin, cout):
        def run():
            gen = _gen('cache-expand', cin)
            eg = expand_level[0]
            f, w = _leaf(R.int_data((eg.n, cin), gen, DEV)), _leaf(R.int_data((27, cin, cout), gen, DEV))
            y = F_.expand_conv(f, w, eg)
            y.backward(R.int_data((8 * eg.n, cout), gen, DEV))
            return y.detach(), f.grad, w.grad
        return run

    def bn(c):
        def run():
            gen = _gen('cache-bn', c)
            x = _leaf(torch.randn(2000, c, device=DEV, generator=gen))
            gm, bt = _leaf(torch.rand(c, device=DEV, generator=gen) + 0.5), _leaf(torch.randn(c, device=DEV, generator=gen))
            rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
            y = F_.BatchNormLeaky.apply(x, gm, bt, rm, rv, 1e-4, 0.9, True, 0.0)
            y.backward(torch.randn(2000, c, device=DEV, generator=gen))
            return y.detach(), x.grad, gm.grad, bt.grad, rm, rv
        return run

    def head(cin, cout):
        def run():
            gen = _gen('cache-head', cin)
            x, w = _leaf(R.int_data((3000, cin), gen, DEV)), _leaf(R.int_data((cout, cin), gen, DEV))
            b = _leaf(R.int_data((cout,), gen, DEV))
            y = F_.RowLinear.apply(x, w, b)
            y.backward(R.int_data((3000, cout), gen, DEV))
            return y.detach(), x.grad, w.grad, b.grad
        return run

    return [('grid A (16, 16)', conv_on(g, 16, 16, 'A')), ('grid B (8, 12)', conv_on(even_level, 8, 12, 'B')),
            ('K64 split (16, 24)', dense(16, 24)), ('K8 split (16, 24)', split_k8), ('K64 split (32, 64)', dense(32, 64)),
            ('expand (48, 16)', expand(48, 16)), ('expand (12, 8)', expand(12, 8)), ('bn 16', bn(16)), ('bn 48', bn(48)),
            ('head (16, 2)', head(16, 2)), ('head (48, 1)', head(48, 1))]


def test_memo_caches_and_shared_workspace_do_not_leak_between_calls(levels, even_level, expand_level):
    """Each case first alone with all three caches emptied (what a fresh process computes), then all of them back to
    back on warm caches, in order and in reverse: every result bit-identical.  Then _ws_cache filled past its 4096
    entries with none of the real keys in it, so the next query misses and clears it."""
    F_ = _F()
    cases = _cache_cases(levels, even_level, expand_level)

    def cold():
        for c in (F_._ws_cache, F_._arange_cache, F_._expand_cache):
            c.clear()

    def same(got, want, what):
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s: result %d differs' % (what, i)

    fresh = {}
    for name, run in cases:
        cold()
        fresh[name] = [t.clone() for t in run()]
    cold()
    for order in (cases, cases[::-1], cases):
        for name, run in order:
            same(run(), fresh[name], name + ' on warm caches')
    assert F_._ws_cache and len(F_._arange_cache) >= 2 and F_._expand_cache
    F_._ws_cache.clear()
    for i in range(4200):
        F_._ws_cache[('filler', i)] = 0
    assert len(F_._ws_cache) > 4096
    for name, run in cases[-4:]:
        same(run(), fresh[name], name + ' after the workspace-size cache overflowed')
    assert 0 < len(F_._ws_cache) < 100 and not [k for k in F_._ws_cache if k[0] == 'filler']


# ---- nonlinear Functions: argument order, the saved rows, the gradient hand-over ----

EPS, MOM = 1e-4, 0.9


@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('leak', [0.0, 1.0 / 3.0], ids=['leak0', 'leak1/3'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_batchnorm_leaky(training, leak, affine):
    """BatchNormLeaky against bn_ref with the bars of test_gpu_bn_fp32.py (the kernels are held there)."""
    F_ = _F()
    n, c = 3001, 16
    gen = _gen('bn', training, leak, affine)
    what = 'BatchNormLeaky training=%s leak=%g affine=%s' % (training, leak, affine)
    x = B.offset_data((n, c), gen, DEV, 0.5, 2.0)
    dy = torch.randn(n, c, device=DEV, generator=gen)
    gamma = torch.rand(c, device=DEV, generator=gen) + 0.5 if affine else None
    beta = torch.randn(c, device=DEV, generator=gen) * 0.3 if affine else None
    rm, rv = torch.randn(c, device=DEV, generator=gen), torch.rand(c, device=DEV, generator=gen) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    xl = _leaf(x)
    gl, bl = (_leaf(gamma), _leaf(beta)) if affine else (None, None)
    y = F_.BatchNormLeaky.apply(xl, gl, bl, rm, rv, EPS, MOM, training, leak)
    save = y.grad_fn.saved_tensors[3]
    assert save.shape == (2, c)
    st = B.bn_stats(x, EPS, MOM, rm0, rv0, training)
    if training:        # row 0 the mean, row 1 the inverse standard deviation
        msg = B.stats_mismatch(save[0], save[1], st, EPS)
        assert msg is None, what + ' ' + msg
        m = 1 - float(np.float32(MOM))
        B.assert_close(rm, st['rm'], B.RUN_BAR * st['rm_mag'] + m * B.MEAN_BAR * st['mean_mag'], what + ' running mean', 1.0)
        B.assert_close(rv, st['rv'], B.RUN_BAR * st['rv_mag'] + m * n / (n - 1) * B.VAR_BAR * st['var_mag'],
                       what + ' running var', 1.0)
    else:
        assert torch.equal(save[0], rm0), what + ': eval mean is the running mean'
        B.assert_ulp(save[1], st['invstd'], what + ' eval invstd', 2)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), what + ': eval changed the running stats'
    _, t, mag = B.bn_pre(x, save[0], save[1], gamma, beta)
    msg = B.apply_mismatch(y.detach(), t, mag, leak)
    assert msg is None, what + ' apply: ' + msg
    mask = y.detach() > 0          # the kernel's own mask: y keeps the sign of t (leak >= 0)
    msg = B.mask_mismatch(mask, t, mag)
    assert msg is None, what + ' forward sign: ' + msg
    y.backward(dy)
    r = B.bn_backward(x, dy, save[0], save[1], gamma, beta, leak, training, None, mask)
    B.assert_close(xl.grad, r['dx'], r['dx_mag'], what + ' dx')
    if affine:
        B.assert_close(gl.grad, r['dgamma'], r['dgamma_mag'], what + ' dgamma')
        B.assert_close(bl.grad, r['dbeta'], r['dbeta_mag'], what + ' dbeta')
        assert gl.grad.untyped_storage().data_ptr() != bl.grad.untyped_storage().data_ptr(), \
            what + ': dgamma and dbeta share a storage'
        assert gl.grad.shape == bl.grad.shape == (c,)


@pytest.mark.parametrize('integer', [True, False], ids=['int', 'real'])
@pytest.mark.parametrize('x_grad', [True, False], ids=['dx', 'no_dx'])
@pytest.mark.parametrize('cin,cout,bias', [(16, 2, True), (48, 1, True), (16, 2, False)])
def test_row_linear(cin, cout, bias, x_grad, integer):
    F_ = _F()
    n = 5003
    gen = _gen('lin', cin, cout, bias, x_grad, integer)
    what = 'RowLinear (%d, %d) bias=%s dx=%s %s' % (cin, cout, bias, x_grad, 'int' if integer else 'real')
    if integer:
        x, dy = B.int_data((n, cin), gen, DEV, 1), B.int_data((n, cout), gen, DEV, 1)
        w, b = B.int_data((cout, cin), gen, DEV), B.int_data((cout,), gen, DEV)
    else:
        x, dy = torch.randn(n, cin, device=DEV, generator=gen), torch.randn(n, cout, device=DEV, generator=gen)
        w, b = torch.randn(cout, cin, device=DEV, generator=gen), torch.randn(cout, device=DEV, generator=gen)
    b = b if bias else None
    xl, wl, bl = _leaf(x, x_grad), _leaf(w), (_leaf(b) if bias else None)
    y = F_.RowLinear.apply(xl, wl, bl)
    chk = (lambda v, ref, mag, tag: B.assert_exact(v, ref, mag, what + tag)) if integer else \
        (lambda v, ref, mag, tag: B.assert_close(v, ref, mag, what + tag))
    chk(y.detach(), *B.linear_fwd(x, w, b), ' y')
    y.backward(dy)
    r = B.linear_bwd(x, dy, w)
    if x_grad:
        chk(xl.grad, r['dx'], r['dx_mag'], ' dx')
    else:
        assert xl.grad is None
    chk(wl.grad, r['dw'], r['dw_mag'], ' dW')
    if bias:
        chk(bl.grad, r['db'], r['db_mag'], ' db')
    if integer and not bias:        # linear in x and in w (with a bias: affine)
        assert FR.adjoint_gap(w, wl.grad, y, dy) == 0
        if x_grad:
            assert FR.adjoint_gap(x, xl.grad, y, dy) == 0
