"""Every BatchNorm(+leaky ReLU) kernel path of bn.hip against the fp64 restatement in tests/bn_ref.py.

The entry points (sgnn_bn_fwd / _fwd_ex / _bwd / _bwd_add / _bwd_ex) are called directly.  How each case reaches its path:
  * VEC (float4 or scalar rows) follows the host rule: float4 when c % 4 == 0, every row stride is a multiple of 4 floats
    and every pointer is 16-byte aligned.  The layouts below choose it: 'dense' and 'wide' (ld > c, the view at column 4)
    take float4 for c % 4 == 0; 'ld_odd' (ld = c + 1) and 'misaligned' (the view at column 1, one float off 16 bytes)
    take the scalar kernels for every c.
  * finalize: sgnn_tune.bn_fuse = 1 lets bn_fuse_ok decide (fused into the apply kernels for c <= 64 on small levels),
    0 forces k_bn_finalize_fwd / _bwd.  The fused totals read two channels per load for even c (the partial table is
    16-byte aligned here), one otherwise: the channel list has both.
  * rows: 0, 1, 2, 3, rpb - 1, rpb, 2 rpb + 1 (rpb as bn_geom computes it), then one count past the statistics clamp
    (BN_MAX_BLOCKS = 2048 workgroups: 4096 rpb rows) and one past the apply clamp (4096 workgroups: 8192 rpb rows); there a
    thread walks many row groups.  c = 48 (and 12, 24, 68, 255) leaves idle threads (256 % cq != 0); c > 128 makes 2c > 256
    in the partial reduce.
  * modes: training and eval, leak 0 / 0.25 / 1, gamma / beta given or NULL, running stats given or NULL, dgamma / dbeta
    NULL; backward addend as a separate buffer, in place (addend == dx) and with its own ld_add.  MODES cycles over them.
Integer data: save_mean and dbeta bit for bit, save_invstd within 1 fp32 ulp; apply, dgamma and dx to the bn_ref bars.
Every output lives in a buffer whose other columns, and the rows past n, hold NaN; they must be bit-unchanged."""
import zlib

import numpy as np
import pytest
import torch

import bn_ref as B
import conv_ref as R
from util import random_sites

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = float(np.float32(1e-4))       # the kernels add the fp32 eps
MOM = 0.9
NAN = float('nan')
CHANNELS = [1, 3, 4, 5, 8, 12, 16, 24, 26, 30, 34, 48, 64, 68, 128, 255, 256, 1024]
LAYOUTS = ['dense', 'wide', 'ld_odd', 'misaligned']
# (training, leak, gamma/beta, running stats, dgamma/dbeta NULL, addend)
MODES = [(1, 0.0, True, True, False, None), (1, 0.25, True, True, False, 'separate'),
         (1, 1.0, False, False, False, 'inplace'), (0, 0.0, True, True, False, 'own_ld'),
         (1, 0.0, False, True, True, None), (0, 0.25, False, True, False, 'separate'),
         (1, 1.0, True, False, False, 'own_ld'), (0, 1.0, True, True, True, 'inplace')]


def _lib():
    from sgnn_amd import _lib as L
    return L


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def r4(c):
    return (c + 3) // 4 * 4


def layout(name, c):
    """(ld, col0, float4?) of a layout."""
    if name == 'dense':
        return c, 0, c % 4 == 0
    if name == 'wide':
        return r4(c) + 8, 4, c % 4 == 0
    if name == 'ld_odd':
        return c + 1 if c % 4 == 0 else c + 2, 0, False
    return r4(c) + 4, 1, False


def rpb_of(c, vec4):
    """bn_geom / bn_geom_scalar: rows per block iteration."""
    cq = c // 4 if vec4 else c
    return max(1, 256 // cq)


def stat_blocks(n, rpb):
    return min(max(-(-n // (2 * rpb)), 1), 2048)


def apply_grid(n, rpb):
    return min(max(-(-n // (2 * rpb)), 1), 4096)


def fused(n, c, rpb):
    """bn_fuse_ok: finalize inside the apply kernels (sgnn_tune.bn_fuse = 1)."""
    nb = stat_blocks(n, rpb)
    return c <= 64 and nb <= 4096 and nb * apply_grid(n, rpb) * 2 * c * 8 <= (48 << 20)


class Rows(object):
    """n rows of c channels at column col0 of an (n + 2) x ld buffer; every other entry holds NaN."""

    def __init__(self, n, c, ld, col0, fill=None):
        self.n, self.c, self.ld, self.col0 = n, c, ld, col0
        self.buf = torch.full((n + 2, ld), NAN, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None:
            self.buf[:n, col0:col0 + c] = fill
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * col0

    def get(self):
        return self.buf[:self.n, self.col0:self.col0 + self.c]

    def assert_outside_untouched(self, what):
        keep = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        keep[:self.n, self.col0:self.col0 + self.c] = False
        assert torch.equal(self.buf.view(torch.int32)[keep], self.before.view(torch.int32)[keep]), \
            what + ': store outside the view'

    def assert_untouched(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), what + ': buffer written'


@pytest.fixture
def tune():
    """set(**knobs) on top of the library defaults; everything restored afterwards."""
    L = _lib()
    names = ('bn_fuse', 'conv_small', 'conv_small_rows', 'conv_unrolled', 'conv_wide_epi', 'conv_one_round',
             'prog_lin_bn', 'prog_lin_add')
    saved = {k: L.tune(k) for k in names}

    def set_(**kv):
        for k in names:
            L.tune(k, kv.get(k, saved[k]))
    try:
        yield set_
    finally:
        for k, v in saved.items():
            L.tune(k, v)


def _ws(n, c):
    wsb = _lib().query('sgnn_bn_ws_bytes', n, c)
    return torch.empty(wsb, dtype=torch.uint8, device=DEV), wsb


def _p(t):
    return None if t is None else t.data_ptr()


def bn_forward(x, n, c, lay, training, leak, gamma, beta, rm, rv, pre=None, pre_nblk=0):
    """Runs the forward in layout `lay`; returns (x rows, y rows, save (2, c))."""
    ld, col0, _ = layout(lay, c)
    xr, yr = Rows(n, c, ld, col0, x), Rows(n, c, ld, col0)
    save = torch.full((2, c), NAN, device=DEV)
    ws, wsb = _ws(n, c)
    L = _lib()
    if lay == 'dense' and pre is None:
        L.call('sgnn_bn_fwd', xr.ptr, n, c, _p(gamma), _p(beta), _p(rm), _p(rv), EPS, MOM, training, leak,
               save[0].data_ptr(), save[1].data_ptr(), yr.ptr, ws.data_ptr(), wsb)
    else:
        L.call('sgnn_bn_fwd_ex', xr.ptr, ld, n, c, _p(gamma), _p(beta), _p(rm), _p(rv), EPS, MOM, training, leak,
               save[0].data_ptr(), save[1].data_ptr(), yr.ptr, ld, _p(pre), pre_nblk, ws.data_ptr(), wsb)
    return xr, yr, save


def bn_backward(xr, dy, n, c, lay, training, leak, gamma, beta, save, addend_mode, addend, dgb_null, pre=None,
                pre_nblk=0):
    """Runs the backward on the forward's x rows; returns (dx rows, dgb (2, c) or None)."""
    ld, col0, _ = layout(lay, c)
    dyr = Rows(n, c, ld, col0, dy)
    dxr = Rows(n, c, ld, col0, addend if addend_mode == 'inplace' else None)
    ar, ld_add = None, 0
    if addend_mode == 'separate':
        ar, ld_add = Rows(n, c, ld, col0, addend), ld
    elif addend_mode == 'own_ld':
        ld_add = ld + (8 if ld % 4 == 0 else 3)
        ar = Rows(n, c, ld_add, col0, addend)
    elif addend_mode == 'inplace':
        ld_add = ld
    addp = ar.ptr if ar is not None else (dxr.ptr if addend_mode == 'inplace' else None)
    dgb = None if dgb_null else torch.full((2, c), NAN, device=DEV)
    dg, db = (None, None) if dgb is None else (dgb[0].data_ptr(), dgb[1].data_ptr())
    ws, wsb = _ws(n, c)
    L = _lib()
    if lay == 'dense' and pre is None and addend_mode is None:
        L.call('sgnn_bn_bwd', xr.ptr, dyr.ptr, n, c, _p(gamma), _p(beta), save[0].data_ptr(), save[1].data_ptr(),
               training, leak, dxr.ptr, dg, db, ws.data_ptr(), wsb)
    elif lay == 'dense' and pre is None and addend_mode == 'separate':
        L.call('sgnn_bn_bwd_add', xr.ptr, dyr.ptr, n, c, _p(gamma), _p(beta), save[0].data_ptr(), save[1].data_ptr(),
               training, leak, addp, dxr.ptr, dg, db, ws.data_ptr(), wsb)
    else:
        L.call('sgnn_bn_bwd_ex', xr.ptr, ld, dyr.ptr, ld, n, c, _p(gamma), _p(beta), save[0].data_ptr(),
               save[1].data_ptr(), training, leak, addp, ld_add, dxr.ptr, ld, dg, db, _p(pre), pre_nblk, ws.data_ptr(),
               wsb)
    dyr.assert_untouched('dy')
    if ar is not None:
        ar.assert_untouched('addend')
    return dxr, dgb


def check_case(c, n, lay, mode, integer=True, mu=0.0, seed=0):
    """One forward + backward in `lay` and `mode` against bn_ref."""
    training, leak, affine, running, dgb_null, addend_mode = mode
    gen = _gen(c, n, lay, mode, integer, mu, seed)
    what = 'c=%d n=%d %s mode=%r %s' % (c, n, lay, mode, 'int' if integer else 'real mu=%g' % mu)
    x = B.int_data((n, c), gen, DEV) if integer else B.offset_data((n, c), gen, DEV, mu)
    dy = B.int_data((n, c), gen, DEV) if integer else torch.randn(n, c, device=DEV, generator=gen)
    addend = (B.int_data((n, c), gen, DEV) if integer else torch.randn(n, c, device=DEV, generator=gen)) \
        if addend_mode else None
    gamma = torch.rand(c, device=DEV, generator=gen) + 0.5 if affine else None
    beta = torch.randn(c, device=DEV, generator=gen) * 0.3 if affine else None
    rm = torch.randn(c, device=DEV, generator=gen) if running else None
    rv = torch.rand(c, device=DEV, generator=gen) + 0.5 if running else None
    rm0, rv0 = (None, None) if rm is None else (rm.clone(), rv.clone())
    xr, yr, save = bn_forward(x, n, c, lay, training, leak, gamma, beta, rm, rv)
    xr.assert_untouched(what + ' x')
    yr.assert_outside_untouched(what + ' y')
    st = B.bn_stats(x, EPS, MOM, rm0, rv0, bool(training))
    # ---- statistics ----
    if not training:
        assert torch.equal(save[0], rm0), what + ': eval mean is the running mean'
        B.assert_ulp(save[1], st['invstd'], what + ' eval invstd', 2)    # fp32 1 / sqrtf(rv + eps): two roundings
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), what + ': eval changed the running stats'
    elif n == 0:
        assert (save == 0).all(), what + ': empty level saves zero statistics'
        if rm is not None:
            assert torch.equal(rm, rm0) and torch.equal(rv, rv0), what + ': empty level changed the running stats'
        yr.assert_untouched(what + ' y')
        dxr, dgb = bn_backward(xr, dy, n, c, lay, training, leak, gamma, beta, save, addend_mode, addend, dgb_null)
        dxr.assert_untouched(what + ' dx')
        if dgb is not None:
            assert (dgb == 0).all(), what + ': empty level dgamma / dbeta'
        return
    else:
        if integer:
            B.assert_int_bound((x.double() ** 2).sum(0), what)
            B.assert_rounded(save[0], st['mean'], x.double().abs().sum(0), what + ' mean')
            B.assert_ulp(save[1], st['invstd'], what + ' invstd')
        else:
            msg = B.stats_mismatch(save[0], save[1], st, EPS)
            assert msg is None, what + ' ' + msg
        if rm is not None:
            m = 1 - float(np.float32(MOM))
            unb = n / (n - 1) if n > 1 else 1.0
            lim_m = B.RUN_BAR * st['rm_mag'] + (0 if integer else m * B.MEAN_BAR * st['mean_mag'])
            lim_v = B.RUN_BAR * st['rv_mag'] + (0 if integer else m * unb * B.VAR_BAR * st['var_mag'])
            B.assert_close(rm, st['rm'], lim_m, what + ' running mean', 1.0)
            B.assert_close(rv, st['rv'], lim_v, what + ' running var', 1.0)
    # ---- apply, from the kernel's own saved statistics ----
    y = yr.get()
    _, t, mag = B.bn_pre(x, save[0], save[1], gamma, beta)
    msg = B.apply_mismatch(y, t, mag, leak)
    assert msg is None, what + ' apply: ' + msg
    mask = y > 0
    msg = B.mask_mismatch(mask, t, mag)
    assert msg is None, what + ' forward sign: ' + msg
    # ---- backward: its mask must be exactly the sign of the forward output the kernel wrote ----
    dxr, dgb = bn_backward(xr, dy, n, c, lay, training, leak, gamma, beta, save, addend_mode, addend, dgb_null)
    dxr.assert_outside_untouched(what + ' dx')
    r = B.bn_backward(x, dy, save[0], save[1], gamma, beta, leak, bool(training), addend, mask)
    if dgb is not None:
        if integer:
            B.assert_int_bound(r['dbeta_mag'], what)
            B.assert_exact(dgb[1], r['dbeta'], r['dbeta_mag'], what + ' dbeta')
        else:
            B.assert_close(dgb[1], r['dbeta'], r['dbeta_mag'], what + ' dbeta')
        B.assert_close(dgb[0], r['dgamma'], r['dgamma_mag'], what + ' dgamma')
    B.assert_close(dxr.get(), r['dx'], r['dx_mag'], what + ' dx')


def row_counts(c, lay, fuse):
    vec4 = layout(lay, c)[2]
    rpb = rpb_of(c, vec4)
    ns = {0, 1, 2, 3, rpb - 1, rpb, 2 * rpb + 1}
    if not fuse and lay in ('wide', 'misaligned'):    # past the clamps no level is fused: one fuse setting suffices
        ns |= {4096 * rpb + 1, 8192 * rpb + 1}
        if c == 16 and lay == 'wide':
            ns.add(10 ** 6)
    return sorted(ns)


@pytest.mark.parametrize('fuse', [1, 0])
@pytest.mark.parametrize('lay', LAYOUTS)
@pytest.mark.parametrize('c', CHANNELS)
def test_bn_paths_integer(tune, c, lay, fuse):
    """Every channel count x layout x finalize path at the row counts of row_counts(), modes cycling through MODES."""
    tune(bn_fuse=fuse)
    if not layout(lay, c)[2] and c > 256:       # scalar rows carry at most 256 channels: refused
        assert_refused(c, lay)
        return
    for i, n in enumerate(row_counts(c, lay, fuse)):
        check_case(c, n, lay, MODES[(i + CHANNELS.index(c)) % len(MODES)])


@pytest.mark.parametrize('fuse', [1, 0])
@pytest.mark.parametrize('c,lay', [(16, 'wide'), (26, 'misaligned'), (5, 'dense'), (48, 'wide'), (128, 'dense')])
def test_bn_every_mode(tune, c, lay, fuse):
    """Every entry of MODES at one small level (fused for c <= 64 with bn_fuse = 1) and one past the statistics clamp."""
    tune(bn_fuse=fuse)
    rpb = rpb_of(c, layout(lay, c)[2])
    for n in (3 * rpb + 5, 4096 * rpb + 7):
        if fuse:
            assert fused(n, c, rpb) == (c <= 64 and n < 4096 * rpb)
        for mode in MODES:
            check_case(c, n, lay, mode)


@pytest.mark.parametrize('fuse', [1, 0])
@pytest.mark.parametrize('c', [16, 5])
def test_bn_offset_real_data(tune, c, fuse):
    """x = mu + N(0, 1), mu in {0, 8, 64}: the statistics to the var bar 2^-20 (var + mean^2), everything else to the
    real-data bars.  Small levels (fused with bn_fuse = 1) and ~10^5 rows."""
    tune(bn_fuse=fuse)
    for mu in (0.0, 8.0, 64.0):
        for i, n in enumerate((2, 7, 33, 100003)):
            check_case(c, n, 'wide', MODES[i % 3], integer=False, mu=mu)


def test_scalar_rows_beyond_256_channels_are_refused():
    """Regression: the scalar kernels give one thread per channel of a 256-thread workgroup, so for c in (256, 1024]
    with unaligned rows (c % 4 == 0, an ld or a pointer off 16 bytes) channels 256.. were never normalised and their
    statistics were read from uninitialised LDS.  Such calls are now refused before anything is written; aligned rows of
    the same width take the float4 kernels (test_bn_paths_integer)."""
    for lay in ('ld_odd', 'misaligned'):
        assert_refused(260, lay)
    check_case(260, 4096 * 4 + 3, 'wide', MODES[0])      # the float4 kernels do take 260 channels


def assert_refused(c, lay, n=100):
    L = _lib()
    gen = _gen('refuse', c, lay)
    x = B.int_data((n, c), gen, DEV)
    ld, col0, vec4 = layout(lay, c)
    assert not vec4
    xr, yr, dxr = Rows(n, c, ld, col0, x), Rows(n, c, ld, col0), Rows(n, c, ld, col0)
    save = torch.full((2, c), NAN, device=DEV)
    before = save.clone()
    ws, wsb = _ws(n, c)
    with pytest.raises(L.SgnnError, match='16-byte aligned'):
        L.call('sgnn_bn_fwd_ex', xr.ptr, ld, n, c, None, None, None, None, EPS, MOM, 1, 0.0, save[0].data_ptr(),
               save[1].data_ptr(), yr.ptr, ld, None, 0, ws.data_ptr(), wsb)
    with pytest.raises(L.SgnnError, match='16-byte aligned'):
        L.call('sgnn_bn_bwd_ex', xr.ptr, ld, xr.ptr, ld, n, c, None, None, save[0].data_ptr(), save[1].data_ptr(),
               1, 0.0, None, 0, dxr.ptr, ld, None, None, None, 0, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert torch.equal(save.view(torch.int32), before.view(torch.int32))
    yr.assert_untouched('y')
    dxr.assert_untouched('dx')


# ---- statistics from a convolution epilogue (ConvEpi.stats = 1 and 2) ----

EPI_PATHS = [('small16', {}), ('tile64', {'conv_small': 0}),
             ('tile256', {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 0}),
             ('tile256_wide', {'conv_small_rows': 0, 'conv_wide_epi': 1, 'conv_unrolled': 0}),
             ('unrolled', {'conv_small_rows': 0, 'conv_unrolled': 1})]
TRANSPOSE_W, FLIP_K = 1, 2


@pytest.fixture(scope='module')
def level():
    from sgnn_amd.scn.metadata import Grid, coords_from_locs
    g = Grid(coords_from_locs(random_sites(2, 32, 0.1, 5, surface=True), torch.device(DEV)))
    return g, g.subm_table()


@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 12)])
@pytest.mark.parametrize('path', [p[0] for p in EPI_PATHS])
@pytest.mark.parametrize('fuse', [1, 0])
def test_bn_on_conv_epilogue_statistics(level, tune, path, cin, cout, fuse):
    """sgnn_conv_fwd_epi with stats = 1, then sgnn_bn_fwd_ex(pre_partial): save_mean bit for bit.  Then the data-gradient
    convolution with stats = 2 and sgnn_bn_bwd_ex(pre_partial): dbeta bit for bit (leak 0 and 0.25 keep dz exact).
    Each epilogue family produces the partials under its conv switches; bn_fuse picks the finalize path."""
    L = _lib()
    tune(bn_fuse=fuse, **dict(EPI_PATHS)[path])
    g, tab = level
    n = g.n
    gen = _gen('epi', path, cin, cout)
    x = B.int_data((n, cin), gen, DEV, 1)
    w = B.int_data((27, cin, cout), gen, DEV, 1)
    y_ref, y_mag = R.walk(x, w, tab, 27, g.ld, n)
    B.assert_int_bound((y_ref * y_ref).sum(0), 'conv output squares')
    nblk = L.query('sgnn_conv_stats_blocks', n)
    part = torch.full((nblk, 2, cout), NAN, dtype=torch.float64, device=DEV)
    y = torch.full((n, cout), NAN, device=DEV)
    L.call('sgnn_conv_fwd_epi', x.data_ptr(), n, cin, cin, w.data_ptr(), 27, tab.data_ptr(), g.ld, n, cout, y.data_ptr(),
           cout, 0, None, 0, 1, part.data_ptr(), None, 0, None, None, None, None, 0.0)
    R.assert_exact(y, y_ref, y_mag, path + ' conv')
    gamma = torch.rand(cout, device=DEV, generator=gen) + 0.5
    beta = torch.randn(cout, device=DEV, generator=gen) * 0.3
    xr, yr, save = bn_forward(y, n, cout, 'dense', 1, 0.0, gamma, beta, None, None, part, nblk)
    st = B.bn_stats(y_ref, EPS)
    B.assert_rounded(save[0], st['mean'], y_mag.sum(0), path + ' mean from epilogue partials')
    B.assert_ulp(save[1], st['invstd'], path + ' invstd from epilogue partials')
    _, t, mag = B.bn_pre(y, save[0], save[1], gamma, beta)
    msg = B.apply_mismatch(yr.get(), t, mag, 0.0)
    assert msg is None, path + ' apply: ' + msg
    # data gradient: dX = walk_adjoint(dy) (the layer's weight (27, c = cout here, cin)), BatchNorm over dX's rows with a
    # mask no rounding can flip: bn_x integer, mean 0.5, invstd 1, gamma in {1, 2}, beta 0 -> t = +-0.5, +-1.5, ...
    c = cout
    wl = B.int_data((27, c, cin), gen, DEV, 1)
    dyc = B.int_data((n, cin), gen, DEV, 1)
    dx_ref, dx_mag = R.walk_adjoint(dyc, wl, tab, 27, g.ld, n, n)
    bn_x = B.int_data((n, c), gen, DEV, 1)
    mean = torch.full((c,), 0.5, device=DEV)
    invstd = torch.ones(c, device=DEV)
    gm = torch.randint(1, 3, (c,), device=DEV, generator=gen).float()
    bt = torch.zeros(c, device=DEV)
    for leak in (0.0, 0.25):
        part2 = torch.full((nblk, 2, c), NAN, dtype=torch.float64, device=DEV)
        gbuf = torch.full((n, c), NAN, device=DEV)
        L.call('sgnn_conv_fwd_epi', dyc.data_ptr(), n, cin, 0, wl.data_ptr(), 27, tab.data_ptr(), g.ld, n, c,
               gbuf.data_ptr(), 0, TRANSPOSE_W | FLIP_K, None, 0, 2, part2.data_ptr(), bn_x.data_ptr(), 0,
               mean.data_ptr(), invstd.data_ptr(), gm.data_ptr(), bt.data_ptr(), leak)
        R.assert_exact(gbuf, dx_ref, dx_mag, path + ' data gradient')
        r = B.bn_backward(bn_x, dx_ref, mean, invstd, gm, bt, leak, True)
        B.assert_int_bound(r['dbeta_mag'], 'dz')
        xbr = Rows(n, c, c, 0, bn_x)
        save2 = torch.stack([mean, invstd])
        dxr, dgb = bn_backward(xbr, gbuf, n, c, 'dense', 1, leak, gm, bt, save2, None, None, False, part2, nblk)
        tag = '%s leak=%g' % (path, leak)
        B.assert_exact(dgb[1], r['dbeta'], r['dbeta_mag'], tag + ' dbeta from epilogue partials')
        B.assert_close(dgb[0], r['dgamma'], r['dgamma_mag'], tag + ' dgamma from epilogue partials')
        B.assert_close(dxr.get(), r['dx'], r['dx_mag'], tag + ' dx from epilogue partials')


# ---- BnLin: BatchNorm backward that forms the head's data gradient (sgnn_tune.prog_lin_bn), through the executor ----

def _program_input(c, gen):
    """Level-0 rows of a small scene (integer features whose per-channel mean is no integer: no t sits on the ReLU
    boundary) as a SparseConvNetTensor with a gradient."""
    from sgnn_amd import scn
    locs = random_sites(2, 16, 0.2, 3, surface=True)
    n = locs.shape[0]
    f = B.int_data((n, c), gen, DEV)
    for ch in range(c):
        if int(f[:, ch].sum().item()) % n == 0:
            f[0, ch] += 1 if f[0, ch] < 3 else -1
    f.requires_grad_(True)
    return scn.InputLayer(3, [16] * 3, mode=0)([locs.to(DEV), f]), f


def _head_reference(f, bn, lins, gy, gb=None):
    """fp64 BatchNormReLU (training, batch statistics) -> heads, and their gradients for head gradients gy (+ gb on the
    BatchNorm output)."""
    x = f.detach().double()
    st = B.bn_stats(x, bn.eps)
    gamma, beta = bn.weight.detach().double(), bn.bias.detach().double()
    y, t, ymag = B.bn_apply(x, st['mean'], st['invstd'], gamma, beta, 0.0)
    W = torch.cat([l.weight.detach() for l in lins]).double()
    b = torch.cat([l.bias.detach() for l in lins]).double()
    h, hmag = B.linear_fwd(y, W, b)
    hmag = hmag + W.abs().sum(1) * ymag.max()         # + the apply error of y, carried through W
    lb = B.linear_bwd(y, gy, W, gb)
    r = B.bn_backward(x, lb['dx'], st['mean'], st['invstd'], gamma, beta, 0.0, True)
    return h, hmag, lb, r


@pytest.mark.parametrize('nout', [1, 2])
def test_bn_linear_head_through_executor(tune, nout):
    """The smallest Program: an empty chain, then ('bn', BatchNormReLU(c)), ('linear', [nn.Linear(c, 1)] x nout), planned
    with prog_lin_bn = 1 (the head is the BatchNorm output's only reader: BnLin forms dy W inside both backward passes)
    and with prog_lin_bn = 0 (k_linear_bwd writes it).  Head outputs, the input gradient, dgamma / dbeta and the head's
    dW / db against an fp64 composition; the two plans bit-identical."""
    from sgnn_amd import scn
    from sgnn_amd.scn import program as P
    c = 16
    gen = _gen('bnlin', nout)
    torch.manual_seed(nout)
    bn = scn.BatchNormReLU(c).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device=DEV, generator=gen) + 0.5)     # beta 0: sign(t) = sign(x - mean)
    lins = [torch.nn.Linear(c, 1).to(DEV) for _ in range(nout)]
    results = {}
    for lin_bn in (1, 0):
        tune(prog_lin_bn=lin_bn)
        prog = P.Program([], c, tail=[('bn', bn), ('linear', lins)])
        x, f = _program_input(c, _gen('bnlin-in', nout))
        for m in [bn] + lins:
            m.zero_grad()
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0)
        outs, _, _ = P.run_program(prog, x, True, out_bufs=[prog.tail_out])
        h = outs[0]
        gy = B.int_data(h.shape, _gen('bnlin-dy', nout), DEV)
        h.backward(gy)
        torch.cuda.synchronize()
        results[lin_bn] = [h.detach().clone(), f.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()] + \
            [l.weight.grad.clone() for l in lins] + [l.bias.grad.clone() for l in lins]
        href, hmag, lb, r = _head_reference(f, bn, lins, gy.double())
        tag = 'prog_lin_bn=%d nout=%d' % (lin_bn, nout)
        B.assert_close(h, href, hmag, tag + ' heads')
        B.assert_close(f.grad, r['dx'], r['dx_mag'], tag + ' input gradient')
        B.assert_close(bn.weight.grad, r['dgamma'], r['dgamma_mag'], tag + ' dgamma')
        B.assert_close(bn.bias.grad, r['dbeta'], r['dbeta_mag'], tag + ' dbeta')
        for o, l in enumerate(lins):
            B.assert_close(l.weight.grad[0], lb['dw'][o], lb['dw_mag'][o], tag + ' dW')
            B.assert_close(l.bias.grad[0], lb['db'][o], lb['db_mag'][o], tag + ' db')
    for a, b in zip(results[1], results[0]):
        assert torch.equal(a, b), 'prog_lin_bn = 1 and 0 differ'
