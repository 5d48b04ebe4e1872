"""Every fp32 convolution kernel path (conv.hip, conv_unrolled.hip) against an fp64 rulebook walk (tests/conv_ref.py).

Each path is forced with the library's switch table (sgnn_tune: conv_small, conv_small_rows, conv_unrolled, conv_wide_epi,
conv_one_round, conv_dw_blocks, conv_dw_c1), so coverage follows from the set-up and not from row-count thresholds.
The rulebooks are the library's own (held bit-exact to the oracle in test_gpu_ops.py), except for the up-sampling
convolution, whose 8N children and their 27-offset rulebook are built here from coordinates.  The data-gradient
reference scatters over the forward table (its adjoint), never through the library's flip / transpose / parent table.

Integer data ({-3..3}; {-1, 0, 1} on very long sums) must match bit for bit: fp32 sums of integers below 2^24 are exact in
any order, so a dropped, doubled or misplaced rule, a wrong row or a leaked pad column fails at any level size.  Real
data is held to |y - ref| <= 2^-18 * sum|terms| per element (conv_ref.BAR; the rationale is written there)."""
import zlib

import numpy as np
import pytest
import torch

import conv_ref as R
from util import random_sites

pytestmark = pytest.mark.gpu

TRANSPOSE_W, FLIP_K = 1, 2

# conv.hip CONV_FWD_CASES, then widths only k_conv_fwd_generic takes
FWD_SHAPES = [(1, 8), (8, 8), (8, 12), (12, 12), (12, 16), (16, 16), (34, 16), (30, 16), (26, 16), (48, 16), (8, 1),
              (12, 8), (16, 12), (16, 34), (16, 30), (16, 26), (16, 48), (32, 16), (16, 32), (4, 16), (16, 4), (16, 24),
              (24, 16), (24, 32), (32, 24), (64, 32), (32, 64), (56, 28), (28, 56), (32, 32), (28, 16), (16, 28)]
GENERIC_SHAPES = [(5, 7), (72, 8)]
# conv.hip CONV_DW_CASES, then shapes only k_conv_dw_generic takes
DW_SHAPES = [(1, 8), (8, 8), (8, 12), (12, 12), (12, 16), (16, 16), (34, 16), (30, 16), (26, 16), (48, 16), (32, 16),
             (4, 16), (16, 24), (24, 32), (64, 32), (56, 28), (32, 32), (28, 16)]
DW_GENERIC = [(5, 7), (16, 12)]
# conv.hip CONV_EX_CASES (the up-sampling convolution and the offset-split dense k4s2 shapes), then a generic one
EX_SHAPES = [(48, 16), (16, 48), (24, 8), (8, 24), (16, 24), (24, 16), (24, 32), (32, 24), (64, 32), (32, 64), (56, 28),
             (28, 56)]
EX_GENERIC = [(16, 16)]
# real data: at least one shape per kernel family (small / 64-row / 256-row / wide epilogue / unrolled 27 and 8 /
# generic) and every path below
REAL_SHAPES = [(16, 16), (26, 16), (12, 8), (8, 12), (34, 16), (64, 32), (1, 8), (5, 7)]

# forward and data-gradient paths of a small level (a few thousand rows)
FWD_PATHS = [
    ('small16', {}),                                                  # k_conv_small (levels below conv_small_rows)
    ('tile64', {'conv_small': 0}),                                    # k_conv_fwd<.., 1, ..>
    ('tile256', {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 0}),   # k_conv_fwd<.., 4, ..>
    ('tile256_wide', {'conv_small_rows': 0, 'conv_wide_epi': 1, 'conv_unrolled': 0}),   # k_conv_fwd_w
    ('unrolled', {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 1}),       # k_conv_fwd_u
    ('unrolled_wide', {'conv_small_rows': 0, 'conv_wide_epi': 1, 'conv_unrolled': 1}),  # k_conv_fwd_uw (K = 8)
]
KNOBS = ('conv_small', 'conv_small_rows', 'conv_unrolled', 'conv_one_round', 'conv_wide_epi', 'conv_dw_blocks',
         'conv_dw_c1')


def _lib():
    from sgnn_amd import _lib as L
    return L


def _grid_from_locs(locs):
    from sgnn_amd.scn.metadata import Grid, coords_from_locs
    return Grid(coords_from_locs(locs, torch.device('cuda')))


def _cloud(n, side, seed):
    """n distinct sites of a dense side^3 cloud (every site has many neighbours), on one batch entry."""
    cells = torch.from_numpy(np.random.default_rng(seed).permutation(side ** 3)[:n])
    return _grid_from_locs(torch.stack([cells // (side * side), (cells // side) % side, cells % side,
                                        torch.zeros_like(cells)], 1))


@pytest.fixture(scope='module')
def levels():
    from sgnn_amd.scn.metadata import build_down2
    g = _grid_from_locs(random_sites(2, 32, 0.1, 5, surface=True))
    d = build_down2(g)
    assert 500 < d.coarse.n < g.n < 16384           # a small level: below conv_small_rows and DW_FINE_ROWS
    return g, d


@pytest.fixture
def tune():
    """set(**knobs) on top of the library defaults; everything restored afterwards."""
    L = _lib()
    saved = {k: L.tune(k) for k in KNOBS}

    def set_(**kv):
        for k in KNOBS:
            L.tune(k, kv.get(k, saved[k]))
    try:
        yield set_
    finally:
        for k, v in saved.items():
            L.tune(k, v)


def _gen(*key):
    return torch.Generator(device='cuda').manual_seed(zlib.crc32(repr(key).encode()))


def _data(shape, gen, integer, lim=3, scale=1.0):
    return R.int_data(shape, gen, 'cuda', lim) if integer else R.real_data(shape, gen, 'cuda', scale)


def _check(y, ref, mag, integer, what):
    (R.assert_exact if integer else R.assert_close)(y, ref, mag, what)


def conv(x, cin, w, K, table, ld, n_out, cout, flags=0, in_shift=0):
    """sgnn_conv_fwd into a NaN-filled buffer (a row the kernel never writes stays NaN and fails every comparison)."""
    y = torch.full((n_out, cout), float('nan'), device='cuda')
    _lib().call('sgnn_conv_fwd', x.data_ptr(), x.shape[0], cin, w.data_ptr(), K, table.data_ptr(), ld, n_out, cout,
                y.data_ptr(), flags, in_shift)
    return y


def conv_dw(x, cin, dy, cout, table, ld, K, n_out, in_shift=0):
    L = _lib()
    wsb = L.query('sgnn_conv_bwd_weight_ws_bytes', n_out, K, cin, cout)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    dw = torch.full((K, cin, cout), float('nan'), device='cuda')
    L.call('sgnn_conv_bwd_weight', x.data_ptr(), x.shape[0], cin, dy.data_ptr(), cout, table.data_ptr(), ld, K, n_out,
           dw.data_ptr(), in_shift, ws.data_ptr(), wsb)
    return dw


# ---- forward and data gradient: every shape under every path ----

def _tables(levels, down):
    g, d = levels
    if down:   # stride-2: forward over children (coarse rows), data gradient through ptable (fine rows)
        return dict(K=8, fwd=(d.children, d.ldc), n_in=g.n, n_out=d.coarse.n, dx=(d.ptable, d.ldf), flags=TRANSPOSE_W)
    t = g.subm_table()
    return dict(K=27, fwd=(t, g.ld), n_in=g.n, n_out=g.n, dx=(t, g.ld), flags=TRANSPOSE_W | FLIP_K)


def _fwd_dx_all_paths(levels, tune, cin, cout, integer, paths=FWD_PATHS):
    for down in (False, True):
        T = _tables(levels, down)
        K, (tab, ld), n_in, n_out = T['K'], T['fwd'], T['n_in'], T['n_out']
        gen = _gen(cin, cout, down, integer)
        x = _data((n_in, cin), gen, integer)
        w = _data((K, cin, cout), gen, integer, scale=1.0 / np.sqrt(K * cin))
        dy = _data((n_out, cout), gen, integer)
        ref, mag = R.walk(x, w, tab, K, ld, n_out)
        dref, dmag = R.walk_adjoint(dy, w, tab, K, ld, n_out, n_in)
        dtab, dld = T['dx']
        for name, knobs in paths:
            tune(**knobs)
            what = '(%d, %d) K=%d %s %s' % (cin, cout, K, name, 'int' if integer else 'real')
            _check(conv(x, cin, w, K, tab, ld, n_out, cout), ref, mag, integer, 'fwd ' + what)
            _check(conv(dy, cout, w, K, dtab, dld, n_in, cin, T['flags']), dref, dmag, integer, 'dX ' + what)


@pytest.mark.parametrize('cin,cout', FWD_SHAPES + GENERIC_SHAPES)
def test_fwd_and_dx_every_path_integer_exact(levels, tune, cin, cout):
    _fwd_dx_all_paths(levels, tune, cin, cout, True)


@pytest.mark.parametrize('cin,cout', REAL_SHAPES)
def test_fwd_and_dx_every_path_real_within_bar(levels, tune, cin, cout):
    _fwd_dx_all_paths(levels, tune, cin, cout, False)


@pytest.mark.parametrize('cin,cout', [(16, 16), (26, 16), (12, 12), (8, 12)])
def test_fwd_row_count_edges_every_path(tune, cin, cout):
    """Levels of 1 .. 257 rows (partial 16-, 64- and 256-row tiles) on every path, forward and data gradient."""
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        g = _cloud(n, 9, n)
        t = g.subm_table()
        gen = _gen('edge', n, cin, cout)
        x, w = R.int_data((n, cin), gen, 'cuda'), R.int_data((27, cin, cout), gen, 'cuda')
        dy = R.int_data((n, cout), gen, 'cuda')
        ref, mag = R.walk(x, w, t, 27, g.ld, n)
        dref, dmag = R.walk_adjoint(dy, w, t, 27, g.ld, n, n)
        for name, knobs in FWD_PATHS:
            tune(**knobs)
            R.assert_exact(conv(x, cin, w, 27, t, g.ld, n, cout), ref, mag, 'n=%d %s' % (n, name))
            R.assert_exact(conv(dy, cout, w, 27, t, g.ld, n, cin, TRANSPOSE_W | FLIP_K), dref, dmag, 'dX n=%d %s' % (n, name))


@pytest.mark.parametrize('n', [40700, 41200])
def test_fwd_both_sides_of_the_small_level_threshold(tune, n):
    """Default switches: 40 960 rows (conv_small_rows) is where k_conv_small hands over to the 256-row kernels."""
    tune()
    L = _lib()
    assert (n < L.tune('conv_small_rows')) == (n == 40700)
    g = _cloud(n, 40, 1)
    t = g.subm_table()
    for cin, cout in ((16, 16), (26, 16)):
        gen = _gen('threshold', n, cin)
        x, w = R.int_data((n, cin), gen, 'cuda'), R.int_data((27, cin, cout), gen, 'cuda')
        ref, mag = R.walk(x, w, t, 27, g.ld, n)
        R.assert_exact(conv(x, cin, w, 27, t, g.ld, n, cout), ref, mag, '(%d, %d) n=%d' % (cin, cout, n))


def test_one_round_tiling_on_a_level_of_two_million_rows(tune):
    """128^3 sites: 8 192 workgroups of 256 rows, several times any resident-workgroup count, so one-round tiling must
    walk J > 1 tiles per workgroup.  Forward against fp64 and against the one-round-off launch, on the wide-epilogue,
    plain 256-row and unrolled kernels; the weight gradient of the same level (coarse path, {-1, 0, 1} data)."""
    side = 128
    ar = torch.arange(side, device='cuda')
    zz, yy, xx = torch.meshgrid(ar, ar, ar, indexing='ij')
    locs = torch.stack([zz.reshape(-1), yy.reshape(-1), xx.reshape(-1), torch.zeros_like(zz).reshape(-1)], 1)
    g = _grid_from_locs(locs)
    del zz, yy, xx, locs
    n, t = g.n, g.subm_table()
    assert n == side ** 3
    for cin, cout, knob, on, off in ((16, 16, 'conv_wide_epi', 'wide', 'tile256'),
                                     (26, 16, 'conv_unrolled', 'unrolled', 'tile256')):
        gen = _gen('big', cin)
        x, w = R.int_data((n, cin), gen, 'cuda'), R.int_data((27, cin, cout), gen, 'cuda')
        ref, mag = R.walk(x, w, t, 27, g.ld, n)
        for val, name in ((1, on), (0, off)):
            outs = []
            for one_round in (1, 0):
                tune(**{knob: val, 'conv_one_round': one_round})
                outs.append(conv(x, cin, w, 27, t, g.ld, n, cout))
            assert torch.equal(outs[0], outs[1]), '(%d, %d) %s: one-round tiling changed rows' % (cin, cout, name)
            R.assert_exact(outs[0], ref, mag, '(%d, %d) %s n=%d' % (cin, cout, name, n))
            del outs
        del ref, mag
        tune()
        dy = R.int_data((n, cout), gen, 'cuda', lim=1)
        x1 = R.int_data((n, cin), gen, 'cuda', lim=1)
        dref, dmag = R.walk_dw(x1, dy, t, 27, g.ld, n)
        R.assert_exact(conv_dw(x1, cin, dy, cout, t, g.ld, 27, n), dref, dmag, 'dW (%d, %d) n=%d' % (cin, cout, n))


# ---- in_shift (SparseConv: table entries are child rows, features live on the parent level) ----

@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 12), (26, 16), (5, 7)])
def test_in_shift_walk_forward_and_weight_gradient(levels, tune, cin, cout):
    g = levels[0]
    base = g.subm_table().view(27, g.ld).long()
    j = torch.arange(g.ld, device='cuda')
    tab = torch.where(base >= 0, base * 8 + (j * 5 + torch.arange(27, device='cuda')[:, None]) % 8, base).int()
    gen = _gen('shift', cin, cout)
    x, w = R.int_data((g.n, cin), gen, 'cuda'), R.int_data((27, cin, cout), gen, 'cuda')
    dy = R.int_data((g.n, cout), gen, 'cuda')
    ref, mag = R.walk(x, w, tab, 27, g.ld, g.n, in_shift=3)
    dref, dmag = R.walk_dw(x, dy, tab, 27, g.ld, g.n, in_shift=3)
    for name, knobs in FWD_PATHS[:3]:
        tune(**knobs)
        R.assert_exact(conv(x, cin, w, 27, tab, g.ld, g.n, cout, 0, 3), ref, mag, 'in_shift (%d, %d) %s' % (cin, cout, name))
        R.assert_exact(conv_dw(x, cin, dy, cout, tab, g.ld, 27, g.n, 3), dref, dmag, 'in_shift dW (%d, %d) %s' % (cin, cout, name))


# ---- weight gradient ----

DW_BLOCKS = (1, 7, None, 4096)      # None: the default


def _dw_paths(cin, cout):
    paths = []
    for blocks in DW_BLOCKS:
        for small in (1, 0):           # fine (one offset per workgroup, below DW_FINE_ROWS) / coarse
            kv = {'conv_small': small}
            if blocks is not None:
                kv['conv_dw_blocks'] = blocks
            paths.append(kv)
    if (cin, cout) == (1, 8):
        paths += [dict(p, conv_dw_c1=0) for p in paths]
    return paths


def _dw_every_path(levels, tune, cin, cout, integer):
    for down in (False, True):
        T = _tables(levels, down)
        K, (tab, ld), n_in, n_out = T['K'], T['fwd'], T['n_in'], T['n_out']
        gen = _gen('dw', cin, cout, down, integer)
        x, dy = _data((n_in, cin), gen, integer), _data((n_out, cout), gen, integer)
        ref, mag = R.walk_dw(x, dy, tab, K, ld, n_out)
        for kv in _dw_paths(cin, cout):
            tune(**kv)
            _check(conv_dw(x, cin, dy, cout, tab, ld, K, n_out), ref, mag, integer,
                   'dW (%d, %d) K=%d %r' % (cin, cout, K, kv))


@pytest.mark.parametrize('cin,cout', DW_SHAPES + DW_GENERIC)
def test_dw_every_path_integer_exact(levels, tune, cin, cout):
    _dw_every_path(levels, tune, cin, cout, True)


@pytest.mark.parametrize('cin,cout', [(16, 16), (8, 8), (1, 8), (34, 16), (64, 32), (5, 7)])
def test_dw_every_path_real_within_bar(levels, tune, cin, cout):
    _dw_every_path(levels, tune, cin, cout, False)


@pytest.fixture(scope='module')
def level_20k():
    g = _cloud(20000, 30, 2)
    return g, g.subm_table()


@pytest.mark.parametrize('cin,cout', DW_SHAPES + DW_GENERIC[:1])
def test_dw_row_probe_at_row_block_boundaries(level_20k, tune, cin, cout):
    """dy is zero except on rows 0, 255, 256, the first and last row of every dW row block and n - 1: a dropped or
    doubled row at any of those boundaries changes dW.  20 000 rows: above DW_FINE_ROWS (the coarse path) at default."""
    g, t = level_20k
    n = g.n
    gen = _gen('probe', cin, cout)
    x, v = R.int_data((n, cin), gen, 'cuda'), R.int_data((n, cout), gen, 'cuda')
    v = torch.where(v == 0, torch.ones_like(v), v)          # no probe value is zero
    for blocks in DW_BLOCKS:
        tune(**({} if blocks is None else {'conv_dw_blocks': blocks}))
        b = _lib().tune('conv_dw_blocks')
        rpb = max(256, (n + b - 1) // b + 255) // 256 * 256   # dw_rows_per_block (conv.hip)
        rows = {0, 255, 256, n - 1}
        for s in range(0, n, rpb):
            rows |= {s, min(s + rpb, n) - 1}
        idx = torch.tensor(sorted(rows), device='cuda')
        dy = torch.zeros(n, cout, device='cuda')
        dy[idx] = v[idx]
        ref, mag = R.walk_dw(x, dy, t, 27, g.ld, n)
        R.assert_exact(conv_dw(x, cin, dy, cout, t, g.ld, 27, n), ref, mag,
                       'row probe (%d, %d) blocks=%d rows=%s' % (cin, cout, b, sorted(rows)[:12]))


# ---- up-sampling (EX) convolution against expand-then-submanifold ----

@pytest.fixture(scope='module')
def expand_level():
    locs = random_sites(1, 24, 0.1, 9, surface=True).cuda()       # [z, y, x, b]; grid row i is site i
    g = _grid_from_locs(locs)
    tab = g.subm_table().view(27, g.ld)[:, :g.n].long()
    assert torch.equal(R.subm_rulebook(locs), tab)                 # the coordinate-built rulebook agrees on the parents
    return g, R.subm_rulebook(R.children_coords(locs))


def _expand_weights(w):
    L = _lib()
    wc = torch.full((64,) + tuple(w.shape[1:]), float('nan'), device='cuda')
    L.call('sgnn_expand_weights', w.data_ptr(), w.shape[1], w.shape[2], wc.data_ptr())
    return wc


def _expand_weights_bwd(dwc):
    L = _lib()
    dw = torch.full((27,) + tuple(dwc.shape[1:]), float('nan'), device='cuda')
    L.call('sgnn_expand_weights_bwd', dwc.data_ptr(), dwc.shape[1], dwc.shape[2], dw.data_ptr())
    return dw


@pytest.mark.parametrize('integer', [True, False])
@pytest.mark.parametrize('cin,cout', [(16, 16), (48, 16), (5, 7), (64, 32)])
def test_expand_weights_and_their_gradient(cin, cout, integer):
    A = R.expand_taps().cuda()
    gen = _gen('ew', cin, cout, integer)
    w, dwc = _data((27, cin, cout), gen, integer), _data((64, cin, cout), gen, integer)
    ref = torch.einsum('st,tio->sio', A, w.double())
    mag = torch.einsum('st,tio->sio', A, w.double().abs())
    _check(_expand_weights(w), ref, mag, integer, 'expand_weights (%d, %d)' % (cin, cout))
    ref = torch.einsum('st,sio->tio', A, dwc.double())
    mag = torch.einsum('st,sio->tio', A, dwc.double().abs())
    _check(_expand_weights_bwd(dwc), ref, mag, integer, 'expand_weights_bwd (%d, %d)' % (cin, cout))


def _expand_case(expand_level, tune, cin, cout, integer):
    from sgnn_amd.scn.functions import expand_maps, sum_groups_raw
    L = _lib()
    g, cnbr = expand_level
    n, n8 = g.n, 8 * g.n
    tab = g.subm_table()
    _, S, ST, PAR = expand_maps(torch.device('cuda'))      # the call's arguments only; the reference never reads them
    gen = _gen('ex', cin, cout, integer)
    f = _data((n, cin), gen, integer)
    w = _data((27, cin, cout), gen, integer, scale=1.0 / np.sqrt(27 * cin))
    dy = _data((n8, cout), gen, integer)
    xc = f.repeat_interleave(8, 0)                             # every child carries its parent's features
    ref, mag = R.walk(xc, w, cnbr, 27, n8, n8)
    dxc, dxm = R.walk_adjoint(dy, w, cnbr, 27, n8, n8, n8)
    dref, dmag = dxc.view(n, 8, cin).sum(1), dxm.view(n, 8, cin).sum(1)
    wref, wmag = R.walk_dw(xc, dy, cnbr, 27, n8, n8)
    wc = _expand_weights(w)
    for name, knobs in (('tile64', {}), ('tile256', {'conv_small_rows': 0})):
        tune(**knobs)
        what = '(%d, %d) %s %s' % (cin, cout, name, 'int' if integer else 'real')
        y = torch.full((n8, cout), float('nan'), device='cuda')
        L.call('sgnn_conv_fwd_ex', f.data_ptr(), n, cin, wc.data_ptr(), 8, tab.data_ptr(), g.ld, n, cout, y.data_ptr(), 0,
               0, S.data_ptr(), None, 1, 8, 27)
        _check(y, ref, mag, integer, 'expand fwd ' + what)
        for G in (1, 2, 4, 8):
            part = torch.full((n, G * cin), float('nan'), device='cuda')
            L.call('sgnn_conv_fwd_ex', dy.data_ptr(), n8, cout, wc.data_ptr(), 64 // G, tab.data_ptr(), g.ld, n, cin,
                   part.data_ptr(), TRANSPOSE_W, 0, ST.data_ptr(), PAR.data_ptr(), 8, G, 27)
            _check(sum_groups_raw(part, cin, n, G), dref, dmag, integer, 'expand dX G=%d %s' % (G, what))
        wsb = L.query('sgnn_conv_bwd_weight_ws_bytes', n, 64, cin, cout)
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
        dwc = torch.full((64, cin, cout), float('nan'), device='cuda')
        L.call('sgnn_conv_bwd_weight_ex', f.data_ptr(), n, cin, dy.data_ptr(), cout, tab.data_ptr(), g.ld, 8, n,
               dwc.data_ptr(), 0, S.data_ptr(), None, 1, 8, 27, ws.data_ptr(), wsb)
        _check(_expand_weights_bwd(dwc), wref, wmag, integer, 'expand dW ' + what)


@pytest.mark.parametrize('cin,cout', EX_SHAPES + EX_GENERIC)
def test_expand_conv_fwd_dx_dw_integer_exact(expand_level, tune, cin, cout):
    _expand_case(expand_level, tune, cin, cout, True)


@pytest.mark.parametrize('cin,cout', [(48, 16), (24, 8), (16, 16)])
def test_expand_conv_fwd_dx_dw_real_within_bar(expand_level, tune, cin, cout):
    _expand_case(expand_level, tune, cin, cout, False)


# ---- fused epilogues (sgnn_conv_fwd_epi) ----

EPI_PATHS = [('small16', {}), ('tile256', {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 0}),
             ('tile256_wide', {'conv_small_rows': 0, 'conv_wide_epi': 1, 'conv_unrolled': 0}),
             ('unrolled', {'conv_small_rows': 0, 'conv_unrolled': 1})]
SENTINEL = -12345.5


def _view(n, c, ld, col0, fill):
    """A (n + 1, ld) buffer of `fill` and the pointer of the column range [col0, col0 + c) of its first n rows (the
    extra row keeps a 16-byte read past the last row's end inside the allocation, and shows a stray store)."""
    buf = torch.full((n + 1, ld), fill, device='cuda')
    return buf, buf.data_ptr() + 4 * col0


def _bn_inputs(n, c, gen, affine):
    """BatchNorm input rows whose pre-activation t = xhat * gamma + beta keeps |t| >= 0.05 (no sign decided by a
    rounding), with mean / invstd / gamma / beta (gamma, beta None: the kernel's 1 and 0)."""
    mean = torch.randn(c, device='cuda', generator=gen)
    invstd = torch.rand(c, device='cuda', generator=gen) + 0.5
    gamma = torch.rand(c, device='cuda', generator=gen) + 0.5 if affine else None
    beta = torch.randn(c, device='cuda', generator=gen) * 0.3 if affine else None
    t = (torch.rand(n, c, device='cuda', generator=gen) * 2 + 0.05) * (torch.randint(0, 2, (n, c), device='cuda',
                                                                                    generator=gen) * 2 - 1)
    xh = (t - (beta if affine else 0)) / (gamma if affine else 1)
    return xh / invstd + mean, mean, invstd, gamma, beta


@pytest.mark.parametrize('cin,cout', [(26, 16), (30, 16), (34, 16), (12, 12), (16, 16), (16, 34), (8, 12), (1, 8)])
def test_epilogue_strides_nan_pads_addend_and_statistics(levels, tune, cin, cout):
    L = _lib()
    g = levels[0]
    n, t = g.n, g.subm_table()
    gen = _gen('epi', cin, cout)
    x = R.int_data((n, cin), gen, 'cuda')
    w = R.int_data((27, cin, cout), gen, 'cuda')
    add = R.int_data((n, cout), gen, 'cuda')
    conv_ref, conv_mag = R.walk(x, w, t, 27, g.ld, n)
    r4 = lambda c: (c + 3) // 4 * 4
    layouts = {'aligned': dict(ldx=r4(cin) + 4, colx=4, ldy=r4(cout) + 8, coly=4, ld_add=r4(cout), cola=0),
               'odd': dict(ldx=cin + 3, colx=1, ldy=cout + 5, coly=3, ld_add=cout + 1, cola=1)}
    for (pname, knobs), (lname, lay) in [(p, l) for p in EPI_PATHS for l in layouts.items()]:
        tune(**knobs)
        what = '(%d, %d) %s %s' % (cin, cout, pname, lname)
        xb, xp = _view(n, cin, lay['ldx'], lay['colx'], float('nan'))     # NaN in every column but the rows
        xb[:n, lay['colx']:lay['colx'] + cin] = x
        ab, ap = _view(n, cout, lay['ld_add'], lay['cola'], float('nan'))
        ab[:n, lay['cola']:lay['cola'] + cout] = add
        nblk = L.query('sgnn_conv_stats_blocks', n)
        for mode in ('plain', 'addend', 'inplace', 'stats1', 'stats2', 'stats2_affine'):
            yb, yp = _view(n, cout, lay['ldy'], lay['coly'], SENTINEL)
            ycols = slice(lay['coly'], lay['coly'] + cout)
            addp, ld_add, ref, mag = None, 0, conv_ref, conv_mag
            if mode != 'plain':
                ref, mag = conv_ref + add.double(), conv_mag + add.double().abs()
                addp, ld_add = ap, lay['ld_add']
            if mode == 'inplace':
                yb[:n, ycols] = add
                addp, ld_add = yp, lay['ldy']
            stats = 1 if mode == 'stats1' else (2 if mode.startswith('stats2') else 0)
            part = torch.full((nblk, 2, cout), float('nan'), dtype=torch.float64, device='cuda')
            bn = (None,) * 5
            if stats == 2:
                bn = _bn_inputs(n, cout, gen, mode.endswith('affine'))
                bb, bp = _view(n, cout, lay['ld_add'], lay['cola'], float('nan'))
                bb[:n, lay['cola']:lay['cola'] + cout] = bn[0]
            for leak in ((0.0, 0.2) if stats == 2 else (0.0,)):
                if mode == 'inplace':
                    yb[:n, ycols] = add
                L.call('sgnn_conv_fwd_epi', xp, n, cin, lay['ldx'], w.data_ptr(), 27, t.data_ptr(), g.ld, n, cout, yp,
                       lay['ldy'], 0, addp, ld_add, stats, part.data_ptr() if stats else None,
                       bp if stats == 2 else None, lay['ld_add'] if stats == 2 else 0,
                       *[None if v is None else v.data_ptr() for v in bn[1:]], leak)
                tag = '%s %s leak=%g' % (what, mode, leak)
                R.assert_exact(yb[:n, ycols], ref, mag, tag)
                keep = torch.ones(lay['ldy'], dtype=torch.bool, device='cuda')
                keep[ycols] = False
                assert (yb[:n, keep] == SENTINEL).all() and (yb[n] == SENTINEL).all(), tag + ': store outside the view'
                if stats == 1:       # integer rows: fp64 sums of y and y^2 are exact in any order
                    s = part.sum(0)
                    assert torch.equal(s[0], ref.sum(0)) and torch.equal(s[1], (ref * ref).sum(0)), tag
                elif stats == 2:
                    bx, mean, invstd, gamma, beta = [None if v is None else v.double() for v in bn]
                    xhat = (bx - mean) * invstd
                    tt = xhat * (gamma if gamma is not None else 1) + (beta if beta is not None else 0)
                    slope = torch.where(tt > 0, torch.ones_like(tt), torch.full_like(tt, leak))
                    dz = ref * slope
                    s = part.sum(0)
                    # fp32 xhat in the kernel: each term carries ~2^-24 of |dz| (|x| + |mean|) invstd
                    m2 = (dz.abs() * (bx.abs() + mean.abs()) * invstd).sum(0)
                    R.assert_close(s[0], dz.sum(0), (ref.abs() * slope).sum(0), tag + ' sum dz')
                    R.assert_close(s[1], (dz * xhat).sum(0), m2, tag + ' sum dz*xhat')


# ---- regressions ----

def test_regression_single_input_channel_pad_quarters(levels, tune):
    """CIN = 1 (V = 1): lane quarters 1, 2 and 3 all hold pad channels, but the kernels zeroed quarter 3 only.
    k_conv_small then read the next columns' weights into quarters 1 and 2 for the data gradient of an (8, 1) layer
    (wrong rows), and every kernel multiplied NaN pad columns of a strided (1, 8) input by zero weights (NaN rows)."""
    L = _lib()
    g = levels[0]
    n, t = g.n, g.subm_table()
    gen = _gen('regression', 1)
    w81 = R.int_data((27, 8, 1), gen, 'cuda')
    dy = R.int_data((n, 1), gen, 'cuda')
    dref, dmag = R.walk_adjoint(dy, w81, t, 27, g.ld, n, n)
    x = R.int_data((n, 1), gen, 'cuda')
    w18 = R.int_data((27, 1, 8), gen, 'cuda')
    ref, mag = R.walk(x, w18, t, 27, g.ld, n)
    xb, xp = _view(n, 1, 4, 0, float('nan'))
    xb[:n, 0] = x[:, 0]
    for name, knobs in FWD_PATHS:
        tune(**knobs)
        R.assert_exact(conv(dy, 1, w81, 27, t, g.ld, n, 8, TRANSPOSE_W | FLIP_K), dref, dmag, 'dX (8, 1) ' + name)
        y = torch.full((n, 8), float('nan'), device='cuda')
        L.call('sgnn_conv_fwd_epi', xp, n, 1, 4, w18.data_ptr(), 27, t.data_ptr(), g.ld, n, 8, y.data_ptr(), 8, 0, None,
               0, 0, None, None, 0, None, None, None, None, 0.0)
        R.assert_exact(y, ref, mag, '(1, 8) NaN-padded rows ' + name)
