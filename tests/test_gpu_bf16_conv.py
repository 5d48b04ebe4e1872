"""bf16 inference kernels (infer_bf16.hip), one by one, against fp64 restatements computed from the same bf16-rounded
inputs and weights: the kernels accumulate in fp32 and round once, so a stored value may differ from the correctly
rounded reference by one bf16 ulp (plus the fp32 accumulation error of a sum that cancels).  The rulebooks are the
library's own (held to the oracle in test_gpu_ops.py); the reference walks them in fp64."""
import numpy as np
import pytest
import torch

from util import random_sites

pytestmark = pytest.mark.gpu

# every compiled forward shape of the fp32 convolution (conv.hip CONV_FWD_CASES) + widths only the generic kernel takes
FWD_SHAPES = [(1, 8), (8, 8), (8, 12), (12, 12), (12, 16), (16, 16), (34, 16), (30, 16), (26, 16), (48, 16), (8, 1),
              (12, 8), (16, 12), (16, 34), (16, 30), (16, 26), (16, 48), (32, 16), (16, 32), (4, 16), (16, 4), (16, 24),
              (24, 16), (24, 32), (32, 24), (64, 32), (32, 64), (56, 28), (28, 56), (32, 32), (28, 16), (16, 28)]
GENERIC_SHAPES = [(72, 8), (8, 80)]
EXPAND_SHAPES = [(16, 16), (48, 16), (24, 8), (8, 24), (16, 24), (32, 24), (28, 56), (64, 32), (72, 8)]


def _lib():
    from sgnn_amd import _lib as L
    return L


def _grid(batch, dim, seed, occupancy=0.1):
    from sgnn_amd.scn.metadata import Grid, coords_from_locs
    locs = random_sites(batch, dim, occupancy, seed, surface=True)
    return Grid(coords_from_locs(locs, torch.device('cuda')))


@pytest.fixture(scope='module')
def grids():
    from sgnn_amd.scn.metadata import build_down2
    g = _grid(2, 32, 5)
    return g, build_down2(g)


@pytest.fixture
def small_rows():
    """Run the test body once with the 16-row-tile kernel and once with the 64-row-tile kernel (the level-size switch
    sgnn_tune.conv_small_rows decides which one a launch takes)."""
    L = _lib()
    prev = L.tune('conv_small_rows')
    yield lambda v: L.tune('conv_small_rows', v)
    L.tune('conv_small_rows', prev)


def r8(c):
    return (c + 7) // 8 * 8


def bf(t):
    return t.to(torch.bfloat16)


def rows_bf16(n, c, ld, gen, col0=0, fill=float('nan')):
    """(values as fp64 [n, c], bf16 buffer [n, ld] with the rows in columns [col0, col0 + c), everything else `fill`)."""
    v = bf(torch.randn(n, c, device='cuda', generator=gen))
    buf = torch.full((n, ld), fill, dtype=torch.bfloat16, device='cuda')
    buf[:, col0:col0 + c] = v
    return v.double(), buf


def ulp(ref):
    """One bf16 ulp of the correctly rounded reference (8 significant bits)."""
    a = bf(ref).double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_bf16_close(y, ref, mag, what=''):
    """|y - bf16(ref)| <= 1 ulp + the fp32 accumulation error (2^-20 of the sum of |terms|)."""
    y = y.double()
    r = bf(ref).double()
    err = (y - r).abs()
    bar = ulp(ref) + 2.0 ** -20 * mag
    bad = err > bar
    assert torch.isfinite(y).all(), what
    assert not bad.any(), '%s: %d of %d values off, worst %g (bar %g)' % (
        what, int(bad.sum()), bad.numel(), float((err - bar).max()), float(bar.flatten()[int((err - bar).argmax())]))


def ref_conv(x, w, table, K, ld, n_out, kmap=None, groups=1):
    """fp64 rulebook walk: y[row * groups + g] = sum_k x[table[kmap[g, k], row]] @ w[g, k] (and the same with |x|, |w|)."""
    t = table.view(-1, ld)[:, :n_out].long()
    cout = w.shape[-1]
    y = torch.zeros(n_out, groups, cout, dtype=torch.float64, device='cuda')
    mag = torch.zeros_like(y)
    w = w.view(groups, K, w.shape[-2], cout)
    for g in range(groups):
        for k in range(K):
            idx = t[kmap[g * K + k] if kmap is not None else k]
            m = idx >= 0
            y[m, g] += x[idx[m]] @ w[g, k]
            mag[m, g] += x[idx[m]].abs() @ w[g, k].abs()
    return y.view(n_out * groups, cout), mag.view(n_out * groups, cout)


def run_conv(x_buf, n_in, cin, ldx, w, K, table, ld, n_out, cout, y_buf, ldy, addend=None, ld_add=0, n_dev=None,
             x_ptr=None, y_ptr=None):
    L = _lib()
    wsb = L.query('sgnn_bf16_conv_ws_bytes', cin, cout, K, 0)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    L.call('sgnn_bf16_conv_fwd', x_ptr or x_buf.data_ptr(), n_in, cin, ldx, w.data_ptr(), K, table.data_ptr(), ld, n_out,
           cout, y_ptr or y_buf.data_ptr(), ldy, None if addend is None else addend.data_ptr(), ld_add,
           None if n_dev is None else n_dev.data_ptr(), ws.data_ptr(), wsb)


def _conv_case(grids, cin, cout, down, seed):
    g, d = grids
    gen = torch.Generator(device='cuda').manual_seed(seed)
    K = 8 if down else 27
    table, ld = (d.children, d.ldc) if down else (g.subm_table(), g.ld)
    n_in, n_out = g.n, (d.coarse.n if down else g.n)
    x, xb = rows_bf16(n_in, cin, r8(cin), gen)
    w = torch.randn(K, cin, cout, device='cuda', generator=gen) / np.sqrt(K * cin)
    y = torch.full((n_out, r8(cout)), float('nan'), dtype=torch.bfloat16, device='cuda')
    run_conv(xb, n_in, cin, r8(cin), w, K, table, ld, n_out, cout, y, r8(cout))
    ref, mag = ref_conv(x, bf(w).double(), table, K, ld, n_out)
    assert_bf16_close(y[:, :cout], ref, mag, '(%d, %d) %s' % (cin, cout, 'down' if down else 'subm'))


@pytest.mark.parametrize('small', [True, False])
@pytest.mark.parametrize('cin,cout', FWD_SHAPES + GENERIC_SHAPES)
def test_conv_subm_and_down(grids, small_rows, cin, cout, small):
    small_rows(1 << 30 if small else 0)
    _conv_case(grids, cin, cout, False, cin * 100 + cout)
    _conv_case(grids, cin, cout, True, cin * 100 + cout + 1)


def expand_maps():
    S = []
    for g in range(8):
        for i in range(8):
            o = [((i >> s) & 1) - 1 + ((g >> s) & 1) for s in (2, 1, 0)]
            S.append((o[0] + 1) * 9 + (o[1] + 1) * 3 + (o[2] + 1))
    return S


def expand_weights(w):
    """The 64 pre-summed slices of the up-sampling convolution (conv.hip k_expand_weights), fp32, same summation order."""
    def taps(j, i):
        return ([-1] if i == 0 else [0, 1]) if j == 0 else ([-1, 0] if i == 0 else [1])
    out = []
    for g in range(8):
        for i in range(8):
            acc = torch.zeros_like(w[0])
            for dz in taps((g >> 2) & 1, (i >> 2) & 1):
                for dy in taps((g >> 1) & 1, (i >> 1) & 1):
                    for dx in taps(g & 1, i & 1):
                        acc = acc + w[(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)]
            out.append(acc)
    return torch.stack(out)


@pytest.mark.parametrize('small', [True, False])
@pytest.mark.parametrize('cin,cout', EXPAND_SHAPES)
def test_conv_expand(grids, small_rows, cin, cout, small):
    small_rows(1 << 30 if small else 0)
    L = _lib()
    g = grids[0]
    gen = torch.Generator(device='cuda').manual_seed(cin * 7 + cout)
    n = g.n
    x, xb = rows_bf16(n, cin, r8(cin), gen)
    w = torch.randn(27, cin, cout, device='cuda', generator=gen) / np.sqrt(8 * cin)
    y = torch.full((8 * n, r8(cout)), float('nan'), dtype=torch.bfloat16, device='cuda')
    wsb = L.query('sgnn_bf16_conv_ws_bytes', cin, cout, 27, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    tab = g.subm_table()
    L.call('sgnn_bf16_conv_expand', xb.data_ptr(), n, cin, r8(cin), w.data_ptr(), tab.data_ptr(), g.ld, cout, y.data_ptr(),
           r8(cout), None, ws.data_ptr(), wsb)
    wc = bf(expand_weights(w)).double()
    ref, mag = ref_conv(x, wc, tab, 8, g.ld, n, kmap=expand_maps(), groups=8)
    assert_bf16_close(y[:, :cout], ref, mag, 'expand (%d, %d)' % (cin, cout))


def test_conv_large_level_above_the_small_threshold():
    """A level of more rows than sgnn_tune.conv_small_rows, at its default: the 64-row-tile kernel as the executor runs it."""
    L = _lib()
    g = _grid(2, 128, 3)
    assert g.n > L.tune('conv_small_rows'), g.n
    gen = torch.Generator(device='cuda').manual_seed(1)
    x, xb = rows_bf16(g.n, 16, 16, gen)
    w = torch.randn(27, 16, 16, device='cuda', generator=gen) / 20
    y = torch.empty(g.n, 16, dtype=torch.bfloat16, device='cuda')
    tab = g.subm_table()
    run_conv(xb, g.n, 16, 16, w, 27, tab, g.ld, g.n, 16, y, 16)
    ref, mag = ref_conv(x, bf(w).double(), tab, 27, g.ld, g.n)
    assert_bf16_close(y, ref, mag, 'large level')


@pytest.mark.parametrize('small', [True, False])
def test_conv_capacity_mode_leaves_rows_past_the_live_count(grids, small_rows, small):
    small_rows(1 << 30 if small else 0)
    g = grids[0]
    gen = torch.Generator(device='cuda').manual_seed(2)
    x, xb = rows_bf16(g.n, 16, 16, gen)
    w = torch.randn(27, 16, 16, device='cuda', generator=gen) / 20
    live = g.n * 2 // 3
    n_dev = torch.tensor([live], dtype=torch.int64, device='cuda')
    sentinel = torch.full((g.n, 16), 7.0, dtype=torch.bfloat16, device='cuda')
    y = sentinel.clone()
    tab = g.subm_table()
    run_conv(xb, g.n, 16, 16, w, 27, tab, g.ld, g.n, 16, y, 16, n_dev=n_dev)
    ref, mag = ref_conv(x, bf(w).double(), tab, 27, g.ld, g.n)
    assert_bf16_close(y[:live], ref[:live], mag[:live], 'capacity')
    assert torch.equal(y[live:], sentinel[live:])


@pytest.mark.parametrize('small', [True, False])
@pytest.mark.parametrize('cin,cout', [(16, 16), (12, 12), (30, 16)])
def test_conv_strided_views_residual_and_nan_pads(grids, small_rows, cin, cout, small):
    """Input rows in a column range of a wider buffer whose other columns are NaN, output written into a column range of
    a join-style buffer (the rest untouched), bf16 residual added before the rounding."""
    small_rows(1 << 30 if small else 0)
    g = grids[0]
    gen = torch.Generator(device='cuda').manual_seed(cin + cout)
    ldx, colx = r8(cin + 10) + 8, 10
    x, xb = rows_bf16(g.n, cin, ldx, gen, col0=colx)
    w = torch.randn(27, cin, cout, device='cuda', generator=gen) / np.sqrt(27 * cin)
    add, addb = rows_bf16(g.n, cout, r8(cout) + 8, gen, col0=0)
    ldy, coly = r8(cout + 6), 6
    y = torch.full((g.n, ldy), 5.0, dtype=torch.bfloat16, device='cuda')
    before = y.clone()
    tab = g.subm_table()
    run_conv(xb, g.n, cin, ldx, w, 27, tab, g.ld, g.n, cout, y, ldy, addend=addb, ld_add=r8(cout) + 8,
             x_ptr=xb.data_ptr() + 2 * colx, y_ptr=y.data_ptr() + 2 * coly)
    ref, mag = ref_conv(x, bf(w).double(), tab, 27, g.ld, g.n)
    assert_bf16_close(y[:, coly:coly + cout], ref + add, mag + add.abs(), 'strided')
    assert torch.equal(y[:, :coly], before[:, :coly]) and torch.equal(y[:, coly + cout:], before[:, coly + cout:])


# ---- row ops ----

def test_bn_eval_bf16():
    L = _lib()
    gen = torch.Generator(device='cuda').manual_seed(3)
    n, c = 5000, 12
    x, xb = rows_bf16(n, c, 24, gen, col0=4)
    gamma, beta = torch.rand(c, device='cuda', generator=gen) + 0.5, torch.randn(c, device='cuda', generator=gen)
    rm, rv = torch.randn(c, device='cuda', generator=gen), torch.rand(c, device='cuda', generator=gen) + 0.2
    y = torch.full((n, 16), float('nan'), dtype=torch.bfloat16, device='cuda')
    L.call('sgnn_bf16_bn_eval', xb.data_ptr() + 8, 24, n, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
           1e-4, 0.01, y.data_ptr(), 16, None)
    invstd = 1.0 / torch.sqrt(rv.double() + 1e-4)
    t = (x - rm.double()) * invstd * gamma.double() + beta.double()
    ref = torch.where(t > 0, t, t * 0.01)
    mag = ((x.abs() + rm.double().abs()) * invstd * gamma.double() + beta.double().abs())
    assert_bf16_close(y[:, :c], ref, mag * 8, 'bn')


def test_gather_add_join_copy_out():
    L = _lib()
    gen = torch.Generator(device='cuda').manual_seed(4)
    n, m, c = 3000, 7000, 12
    x, xb = rows_bf16(n, c, 16, gen)
    idx = torch.randint(0, n, (m,), device='cuda', dtype=torch.int32, generator=gen)
    y = torch.full((m, 16), float('nan'), dtype=torch.bfloat16, device='cuda')
    L.call('sgnn_bf16_gather_rows', xb.data_ptr(), 16, c, idx.data_ptr(), m, y.data_ptr(), 16, None)
    assert torch.equal(y[:, :c], xb[idx.long(), :c])
    a, ab = rows_bf16(n, c, 16, gen)
    s = torch.empty(n, 24, dtype=torch.bfloat16, device='cuda')
    L.call('sgnn_bf16_add', xb.data_ptr(), 16, ab.data_ptr(), 16, n, c, s.data_ptr() + 4, 24, None)
    assert_bf16_close(s[:, 2:2 + c], x + a, x.abs() + a.abs(), 'add')
    j = torch.full((n, 32), float('nan'), dtype=torch.bfloat16, device='cuda')
    L.call('sgnn_bf16_join', xb.data_ptr(), 16, c, ab.data_ptr(), 16, c, n, j.data_ptr(), 32, None)
    assert torch.equal(j[:, :c], xb[:, :c]) and torch.equal(j[:, c:2 * c], ab[:, :c])
    f = torch.empty(n, 2 * c, device='cuda')
    L.call('sgnn_bf16_to_f32', j.data_ptr(), 32, n, 2 * c, f.data_ptr(), None)
    assert torch.equal(f, j[:, :2 * c].float())


def test_concat_in_with_index_arrays():
    L = _lib()
    gen = torch.Generator(device='cuda').manual_seed(5)
    m = 4000
    a = torch.randn(5000, 16, device='cuda', generator=gen)
    b = torch.randn(m, 2, device='cuda', generator=gen)
    c = torch.randn(3000, 8, device='cuda', generator=gen)
    ia = torch.randint(0, 5000, (m,), device='cuda', dtype=torch.int32, generator=gen)
    ic = torch.randint(-1, 3000, (m,), device='cuda', dtype=torch.int32, generator=gen)
    y = torch.full((m, 32), float('nan'), dtype=torch.bfloat16, device='cuda')
    L.call('sgnn_bf16_concat3', a.data_ptr(), 16, ia.data_ptr(), b.data_ptr(), 2, None, c.data_ptr(), 8, ic.data_ptr(), m,
           y.data_ptr(), 32, None)
    cc = torch.where((ic >= 0)[:, None], c[ic.clamp_min(0).long()], torch.zeros(1, device='cuda'))
    want = bf(torch.cat([a[ia.long()], b, cc], 1))
    assert torch.equal(y[:, :26], want)


@pytest.mark.parametrize('cin,cout', [(16, 1), (16, 2), (8, 2)])
def test_linear_heads(cin, cout):
    L = _lib()
    gen = torch.Generator(device='cuda').manual_seed(6)
    n = 6000
    x, xb = rows_bf16(n, cin, r8(cin) + 8, gen)
    w = torch.randn(cout, cin, device='cuda', generator=gen)
    bias = torch.randn(cout, device='cuda', generator=gen)
    y = torch.empty(n, cout, device='cuda')
    L.call('sgnn_bf16_linear', xb.data_ptr(), r8(cin) + 8, n, cin, w.data_ptr(), bias.data_ptr(), cout, y.data_ptr(), None)
    ref = x @ w.double().t() + bias.double()
    mag = x.abs() @ w.double().abs().t() + bias.double().abs()
    assert ((y.double() - ref).abs() <= 1e-5 * mag + 1e-6).all()
