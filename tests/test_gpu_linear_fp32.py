"""The per-site linear heads (linear.hip) against the fp64 restatement in tests/bn_ref.py.

All ten compiled (cin, cout) shapes (LIN_CASES) at row counts around both clamps: the backward gives each thread one row
up to 512 workgroups (131 072 rows), the forward up to 2 048 workgroups (524 288 rows); past a clamp a thread takes
several rows and the backward sums them in fp32 before the fp64 block partials.  Integer data ({-1, 0, 1} rows and
gradients, weights and biases in {-3..3}) keeps every fp32 partial sum an integer below 2^24, so outputs, dx, dW and db
must match fp64 bit for bit; a real-data subset is held to 2^-18 sum |terms|.  Buffers hold NaN past row n, which must
stay bit-unchanged; NULL bias, NULL dx (weights only) and NULL dbias go through the exported sgnn_linear_fwd / _bwd.
The dx-with-addend path (sgnn_tune.prog_lin_add) is reached through the executor."""
import zlib

import pytest
import torch

import bn_ref as B
from util import random_sites

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
LIN_CASES = [(16, 1), (16, 2), (48, 1), (48, 2), (8, 1), (8, 2), (32, 1), (32, 2), (12, 2), (4, 1)]
ROWS = [0, 1, 255, 256, 257, 131072, 131073, 524288, 524289]
BIG = [(16, 2), (48, 1), (12, 2)]           # the ~10^6-row level (a few shapes only: runtime)
REAL = [(16, 2), (48, 2), (12, 2), (4, 1), (8, 1)]
TAIL = 3


def _lib():
    from sgnn_amd import _lib as L
    return L


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _buf(n, c, fill=None):
    b = torch.full((n + TAIL, c), NAN, device=DEV)
    if fill is not None:
        b[:n] = fill
    return b


def _bits(t):
    return t.view(torch.int32).clone()


def run_heads(x, w, b, dy, n, with_dx=True, with_db=True):
    """sgnn_linear_fwd / _bwd on NaN-tailed buffers; returns (y, dx, dw, db) and checks the tails."""
    L = _lib()
    cout, cin = w.shape
    xb, yb, dyb = _buf(n, cin, x), _buf(n, cout), _buf(n, cout, dy)
    dxb = _buf(n, cin) if with_dx else None
    dw = torch.full((cout, cin), NAN, device=DEV)
    db = torch.full((cout,), NAN, device=DEV) if with_db else None
    ybits, dxbits = _bits(yb), None if dxb is None else _bits(dxb)
    L.call('sgnn_linear_fwd', xb.data_ptr(), n, cin, w.data_ptr(), None if b is None else b.data_ptr(), cout,
           yb.data_ptr())
    wsb = L.query('sgnn_linear_ws_bytes', n, cin, cout)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    L.call('sgnn_linear_bwd', xb.data_ptr(), dyb.data_ptr(), n, cin, w.data_ptr(), cout,
           None if dxb is None else dxb.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(),
           ws.data_ptr(), wsb)
    assert torch.equal(_bits(yb)[n:], ybits[n:]), 'y written past row n'
    if dxb is not None:
        assert torch.equal(_bits(dxb)[n:], dxbits[n:]), 'dx written past row n'
    return yb[:n], None if dxb is None else dxb[:n], dw, db


def check(cin, cout, n, integer, bias=True, with_dx=True, with_db=True):
    gen = _gen(cin, cout, n, integer, bias, with_dx, with_db)
    what = '(%d, %d) n=%d %s bias=%s dx=%s db=%s' % (cin, cout, n, 'int' if integer else 'real', bias, with_dx, with_db)
    if integer:
        x, dy = B.int_data((n, cin), gen, DEV, 1), B.int_data((n, cout), gen, DEV, 1)
        w, b = B.int_data((cout, cin), gen, DEV), B.int_data((cout,), gen, DEV)
    else:
        x, dy = torch.randn(n, cin, device=DEV, generator=gen), torch.randn(n, cout, device=DEV, generator=gen)
        w, b = torch.randn(cout, cin, device=DEV, generator=gen), torch.randn(cout, device=DEV, generator=gen)
    b = b if bias else None
    y, dx, dw, db = run_heads(x, w, b, dy, n, with_dx, with_db)
    yr, ymag = B.linear_fwd(x, w, b)
    r = B.linear_bwd(x, dy, w)
    if integer:
        for mag in (ymag, r['dx_mag'], r['dw_mag'], r['db_mag']):
            B.assert_int_bound(mag, what)
        chk = lambda v, ref, mag, tag: B.assert_exact(v, ref, mag, what + tag)
    else:
        chk = lambda v, ref, mag, tag: B.assert_close(v, ref, mag, what + tag)
    chk(y, yr, ymag, ' y')
    if dx is not None:
        chk(dx, r['dx'], r['dx_mag'], ' dx')
    chk(dw, r['dw'], r['dw_mag'], ' dW')
    if db is not None:
        chk(db, r['db'], r['db_mag'], ' db')


@pytest.mark.parametrize('cin,cout', LIN_CASES)
def test_heads_integer_every_shape_and_clamp(cin, cout):
    """Bit for bit at every row count; the NULL variants cycle over the row counts."""
    ns = ROWS + ([10 ** 6 + 3] if (cin, cout) in BIG else [])
    for i, n in enumerate(ns):
        check(cin, cout, n, True, bias=i % 3 != 1, with_dx=i % 4 != 2, with_db=i % 5 != 3)


@pytest.mark.parametrize('cin,cout', REAL)
def test_heads_real_data(cin, cout):
    for n in (257, 131073, 524289):
        check(cin, cout, n, False)


def test_empty_level_zeroes_the_weight_gradient():
    check(16, 2, 0, True)           # dw / db zeroed (exact 0 = fp64 of an empty sum), nothing else written


@pytest.mark.parametrize('cin,cout', [(5, 1), (16, 3), (24, 2)])
@pytest.mark.parametrize('n', [0, 300])
def test_uncompiled_shape_is_refused_and_writes_nothing(cin, cout, n):
    """Regression: with n = 0 an uncompiled shape returned success (and zeroed dW / db) while n > 0 failed."""
    L = _lib()
    x, w, b = torch.ones(n + TAIL, cin, device=DEV), torch.ones(cout, cin, device=DEV), torch.ones(cout, device=DEV)
    dy = torch.ones(n + TAIL, cout, device=DEV)
    y, dx = _buf(n, cout), _buf(n, cin)
    dw, db = torch.full((cout, cin), NAN, device=DEV), torch.full((cout,), NAN, device=DEV)
    before = [_bits(t) for t in (y, dx, dw, db)]
    wsb = L.query('sgnn_linear_ws_bytes', max(n, 1), cin, cout)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SgnnError, match='unsupported head shape'):
        L.call('sgnn_linear_fwd', x.data_ptr(), n, cin, w.data_ptr(), b.data_ptr(), cout, y.data_ptr())
    with pytest.raises(L.SgnnError, match='unsupported head shape'):
        L.call('sgnn_linear_bwd', x.data_ptr(), dy.data_ptr(), n, cin, w.data_ptr(), cout, dx.data_ptr(), dw.data_ptr(),
               db.data_ptr(), ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    for a, t in zip(before, (y, dx, dw, db)):
        assert torch.equal(a, _bits(t))


# ---- dx + addend (sgnn_tune.prog_lin_add), reachable only through the executor ----

def test_head_adds_the_gradient_its_input_rows_carry():
    """The smallest program whose head input rows already carry a gradient when the head's backward runs: an empty chain,
    then ('bn', BatchNormReLU(c)), ('linear', [nn.Linear(c, 1)] x 2), run with out_bufs = [heads, BatchNorm output].  The
    caller's gradient of the BatchNorm output is there before the head's pass (and the second reader turns BnLin off), so
    with prog_lin_add = 1 the head writes dy W + that gradient in one pass, with 0 an add launch follows.  The input
    gradient, dgamma / dbeta and dW / db against fp64; the two settings bit-identical."""
    from sgnn_amd import scn
    from sgnn_amd.scn import program as P
    from test_gpu_bn_fp32 import _head_reference, _program_input
    L = _lib()
    c = 16
    gen = _gen('linadd')
    bn = scn.BatchNormReLU(c).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=gen) + 0.5)
    torch.manual_seed(5)
    lins = [torch.nn.Linear(c, 1).to(DEV) for _ in range(2)]
    saved = {k: L.tune(k) for k in ('prog_lin_add', 'prog_lin_bn')}
    results = {}
    try:
        for lin_add in (1, 0):
            L.tune('prog_lin_add', lin_add)
            prog = P.Program([], c, tail=[('bn', bn), ('linear', lins)])
            bn_out = prog.taps[id(bn)][0]
            x, f = _program_input(c, _gen('linadd-in'))
            for m in [bn] + lins:
                m.zero_grad()
            bn.running_mean.zero_()
            bn.running_var.fill_(1.0)
            outs, _, _ = P.run_program(prog, x, True, out_bufs=[prog.tail_out, bn_out])
            h, ybn = outs
            gh = B.int_data(h.shape, _gen('linadd-dh'), DEV)
            gb = B.int_data(ybn.shape, _gen('linadd-db'), DEV)
            torch.autograd.backward([h, ybn], [gh, gb])
            torch.cuda.synchronize()
            results[lin_add] = [h.detach().clone(), ybn.detach().clone(), f.grad.clone(), bn.weight.grad.clone(),
                                bn.bias.grad.clone()] + [l.weight.grad.clone() for l in lins] + \
                [l.bias.grad.clone() for l in lins]
            href, hmag, lb, r = _head_reference(f, bn, lins, gh.double(), gb.double())
            tag = 'prog_lin_add=%d' % lin_add
            B.assert_close(h, href, hmag, tag + ' heads')
            B.assert_close(f.grad, r['dx'], r['dx_mag'], tag + ' input gradient')
            B.assert_close(bn.weight.grad, r['dgamma'], r['dgamma_mag'], tag + ' dgamma')
            B.assert_close(bn.bias.grad, r['dbeta'], r['dbeta_mag'], tag + ' dbeta')
            for o, l in enumerate(lins):
                B.assert_close(l.weight.grad[0], lb['dw'][o], lb['dw_mag'][o], tag + ' dW')
                B.assert_close(l.bias.grad[0], lb['db'][o], lb['db_mag'][o], tag + ' db')
    finally:
        for k, v in saved.items():
            L.tune(k, v)
    for a, b in zip(results[1], results[0]):
        assert torch.equal(a, b), 'prog_lin_add = 1 and 0 differ'
