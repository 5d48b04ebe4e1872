"""The wide-row 3x3x3 straight-line kernels (conv_unrolled.hip, k_conv_fwd_u<26|30|34,16,27> and <16,26|30|34,27>) with
their weight image resident in LDS for the whole workgroup, against the fp64 rulebook walk of tests/conv_ref.py.

What can go wrong when the image is staged once instead of once per chunk and row tile: a slice read from the wrong
place of the larger tile, pad columns of the image that are not zero, the statistics scratch or another LDS array
overlapping the tile, and — only on a workgroup's SECOND row tile — weights that are no longer there.  So every shape runs
at 1, 255, 256, 257 and 600 rows and at 140 000 rows: 547 tiles of 256 rows, more than the 512 workgroups that can be
resident (two per CU), so that one-round tiling gives every workgroup J >= 2 tiles.  Forward and the data-gradient form
(SGNN_CONV_TRANSPOSE_W | SGNN_CONV_FLIP_K), random rulebooks with ~10 % of the entries missing, integer data (bit-exact,
conv_ref.assert_exact) and real data (conv_ref.BAR); at 257 and 140 000 rows also the fused epilogues (statistics,
addend + BatchNorm-backward statistics, strided rows) and bit-equality of the rows with the looped k_conv_fwd.

Capacity mode (ConvEpi::n_dev: the launch sized for a capacity, the live row count in device memory) decides whether a
workgroup stages at all (workgroups past the live ones return before the staging) and how many tiles share the image (J
follows the device count).  No convolution entry point takes n_dev; the program executor sets it, so those cases run
one-convolution programs through sgnn_prog_forward / sgnn_prog_backward (lev_n = capacity, lev_cnt = live rows) at 257
and 140 000 live rows and at a live count of 0: rows against the fp64 walk, rows past the live count untouched, and —
through a BatchNorm fed from the convolution's statistics epilogue out of a NaN-filled workspace — zero partials from
the workgroups without rows."""
import zlib

import numpy as np
import pytest
import torch

import conv_ref as R
import prog_cases as C

pytestmark = pytest.mark.gpu

TRANSPOSE_W, FLIP_K = 1, 2
K = 27
SHAPES = [(26, 16), (30, 16), (34, 16), (16, 26), (16, 30), (16, 34)]
ROWS = (1, 255, 256, 257, 600, 140000)
EPI_ROWS = (257, 140000)
UNROLLED = {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 1}
LOOPED = {'conv_small_rows': 0, 'conv_wide_epi': 0, 'conv_unrolled': 0}
KNOBS = ('conv_small', 'conv_small_rows', 'conv_unrolled', 'conv_one_round', 'conv_wide_epi', 'prog_fusion')
SENTINEL = -12345.5


def _lib():
    from sgnn_amd import _lib as L
    return L


@pytest.fixture
def tune():
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


_TABLES = {}


def _table(n):
    """Random rulebook [27][ld] over n rows, ~10 % of the entries -1, the padding rows j >= n all -1 (ld: next multiple of 256)."""
    if n not in _TABLES:
        gen = _gen('table', n)
        ld = (n + 255) // 256 * 256
        t = torch.full((K, ld), -1, dtype=torch.int32, device='cuda')
        e = torch.randint(0, n, (K, n), generator=gen, device='cuda', dtype=torch.int32)
        miss = torch.rand((K, n), generator=gen, device='cuda') < 0.1
        t[:, :n] = torch.where(miss, torch.full_like(e, -1), e)
        _TABLES[n] = (t, ld)
    return _TABLES[n]


def _ref_weights(w, dgrad):
    """The (K, cin, cout) weights the walk applies: the data-gradient form reads a (K, cout, cin) tensor mirrored in k."""
    return w.flip(0).transpose(1, 2).contiguous() if dgrad else w


def _case(n, cin, cout, dgrad, integer):
    gen = _gen('case', n, cin, cout, dgrad, integer)
    t, ld = _table(n)
    make = (lambda s, sc=1.0: R.int_data(s, gen, 'cuda')) if integer else (lambda s, sc=1.0: R.real_data(s, gen, 'cuda', sc))
    x = make((n, cin))
    w = make((K, cout, cin) if dgrad else (K, cin, cout), 1.0 / np.sqrt(K * cin))
    ref, mag = R.walk(x, _ref_weights(w, dgrad), t, K, ld, n)
    return x, w, t, ld, ref, mag


def _epi(x, n, cin, ldx, w, t, ld, cout, y, ldy, flags, addend=None, ld_add=0, stats=0, part=None, bnx=None, ld_bnx=0,
         mean=None, invstd=None, gamma=None, beta=None, leak=0.0):
    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())
    _lib().call('sgnn_conv_fwd_epi', p(x), n, cin, ldx, w.data_ptr(), K, t.data_ptr(), ld, n, cout, p(y), ldy, flags,
                p(addend), ld_add, stats, p(part), p(bnx), ld_bnx, p(mean), p(invstd), p(gamma), p(beta), leak)


def _plain(x, n, cin, w, t, ld, cout, flags):
    y = torch.full((n, cout), float('nan'), device='cuda')
    _lib().call('sgnn_conv_fwd', x.data_ptr(), n, cin, w.data_ptr(), K, t.data_ptr(), ld, n, cout, y.data_ptr(), flags, 0)
    return y


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_rows_every_size_forward_and_data_gradient(tune, cin, cout):
    tune(**UNROLLED)
    for n in ROWS:
        for dgrad in (False, True):
            flags = TRANSPOSE_W | FLIP_K if dgrad else 0
            for integer in (True, False) if n in (257, 600, 140000) else (True,):
                x, w, t, ld, ref, mag = _case(n, cin, cout, dgrad, integer)
                y = _plain(x, n, cin, w, t, ld, cout, flags)
                what = '<%d,%d> n=%d %s %s' % (cin, cout, n, 'dX' if dgrad else 'fwd', 'int' if integer else 'real')
                (R.assert_exact if integer else R.assert_close)(y, ref, mag, what)


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_rows_bit_identical_to_the_looped_kernel(tune, cin, cout):
    """conv_unrolled.hip promises the arithmetic and summation order of k_conv_fwd: real data, rows equal bit for bit."""
    for n in EPI_ROWS:
        for dgrad in (False, True):
            flags = TRANSPOSE_W | FLIP_K if dgrad else 0
            x, w, t, ld, _, _ = _case(n, cin, cout, dgrad, False)
            tune(**UNROLLED)
            a = _plain(x, n, cin, w, t, ld, cout, flags)
            tune(**LOOPED)
            b = _plain(x, n, cin, w, t, ld, cout, flags)
            assert torch.equal(a, b), '<%d,%d> n=%d %s: unrolled and looped rows differ' % (cin, cout, n, 'dX' if dgrad else 'fwd')


def _strided(rows, ld, col0, fill):
    """rows (n, c) inside a (n + 1, ld) buffer of `fill` at column col0: (buffer, pointer of the view)."""
    n, c = rows.shape
    buf = torch.full((n + 1, ld), fill, device='cuda')
    buf[:n, col0:col0 + c] = rows
    return buf, buf.data_ptr() + 4 * col0


def _bn_inputs(n, c, gen):
    """BatchNorm input rows whose pre-activation keeps |t| >= 0.05 (no sign decided by a rounding), mean, invstd, gamma, beta."""
    mean = torch.randn(c, device='cuda', generator=gen)
    invstd = torch.rand(c, device='cuda', generator=gen) + 0.5
    gamma = torch.rand(c, device='cuda', generator=gen) + 0.5
    beta = torch.randn(c, device='cuda', generator=gen) * 0.3
    t = (torch.rand(n, c, device='cuda', generator=gen) * 2 + 0.05) * (
        torch.randint(0, 2, (n, c), device='cuda', generator=gen) * 2 - 1)
    return ((t - beta) / gamma) / invstd + mean, mean, invstd, gamma, beta


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_epilogues_statistics_addend_and_strides(tune, cin, cout):
    """Integer rows (exact), strided x / y / addend with NaN around the views; statistics partials summed on the host in
    fp64: stats = 1 exactly (integer rows), stats = 2 (addend, BatchNorm-backward sums) under conv_ref.BAR."""
    L = _lib()
    tune(**UNROLLED)
    for n in EPI_ROWS:
        for dgrad in (False, True):
            flags = TRANSPOSE_W | FLIP_K if dgrad else 0
            x, w, t, ld, conv, cmag = _case(n, cin, cout, dgrad, True)
            gen = _gen('epi', n, cin, cout, dgrad)
            add = R.int_data((n, cout), gen, 'cuda')
            nblk = L.query('sgnn_conv_stats_blocks', n)
            for ldx, colx, ldy, coly, lda, cola in ((cin, 0, cout, 0, cout, 0), (cin + 3, 1, cout + 5, 3, cout + 1, 1),
                                                    (cin + 6, 4, cout + 8, 4, cout + 4, 0)):
                what = '<%d,%d> n=%d %s ldx=%d ldy=%d' % (cin, cout, n, 'dX' if dgrad else 'fwd', ldx, ldy)
                xb, xp = _strided(x, ldx, colx, float('nan'))
                ab, ap = _strided(add, lda, cola, float('nan'))
                ycols = slice(coly, coly + cout)
                outside = torch.ones(ldy, dtype=torch.bool, device='cuda')
                outside[ycols] = False
                # stats = 1
                yb, yp = _strided(torch.full((n, cout), SENTINEL, device='cuda'), ldy, coly, SENTINEL)
                part = torch.full((nblk, 2, cout), float('nan'), dtype=torch.float64, device='cuda')
                _epi(xp, n, cin, ldx, w, t, ld, cout, yp, ldy, flags, stats=1, part=part)
                R.assert_exact(yb[:n, ycols], conv, cmag, what + ' stats1 rows')
                assert (yb[:n, outside] == SENTINEL).all() and (yb[n] == SENTINEL).all(), what + ': store outside the view'
                s = part.sum(0)
                assert torch.equal(s[0], conv.sum(0)) and torch.equal(s[1], (conv * conv).sum(0)), what + ' stats1 sums'
                # stats = 2 with an addend
                bx, mean, invstd, gamma, beta = _bn_inputs(n, cout, gen)
                bb, bp = _strided(bx, lda, cola, float('nan'))
                ref, mag = conv + add.double(), cmag + add.double().abs()
                for leak in (0.0, 0.2):
                    yb, yp = _strided(torch.full((n, cout), SENTINEL, device='cuda'), ldy, coly, SENTINEL)
                    part = torch.full((nblk, 2, cout), float('nan'), dtype=torch.float64, device='cuda')
                    _epi(xp, n, cin, ldx, w, t, ld, cout, yp, ldy, flags, addend=ap, ld_add=lda, stats=2, part=part,
                         bnx=bp, ld_bnx=lda, mean=mean, invstd=invstd, gamma=gamma, beta=beta, leak=leak)
                    tag = '%s stats2 leak=%g' % (what, leak)
                    R.assert_exact(yb[:n, ycols], ref, mag, tag + ' rows')
                    assert (yb[:n, outside] == SENTINEL).all() and (yb[n] == SENTINEL).all(), tag + ': store outside the view'
                    xhat = (bx.double() - mean.double()) * invstd.double()
                    tt = xhat * gamma.double() + beta.double()
                    slope = torch.where(tt > 0, torch.ones_like(tt), torch.full_like(tt, leak))
                    dz = ref * slope
                    s = part.sum(0)
                    # fp32 xhat in the kernel: each term carries ~2^-24 of |dz| (|x| + |mean|) invstd
                    m2 = (dz.abs() * (bx.double().abs() + mean.double().abs()) * invstd.double()).sum(0)
                    R.assert_close(s[0], dz.sum(0), (ref.abs() * slope).sum(0), tag + ' sum dz')
                    R.assert_close(s[1], (dz * xhat).sum(0), m2, tag + ' sum dz*xhat')


@pytest.mark.parametrize('cin,cout', SHAPES)
def test_second_row_tile_runs_at_140000_rows(tune, cin, cout):
    """The size above must give the workgroups of every shape more than one row tile (two workgroups per CU: J = 2, one:
    J = 3): with statistics on, workgroups past the live ones write all-zero partials, so at most half as many non-zero
    partial blocks as 256-row tiles means J >= 2."""
    L = _lib()
    tune(**UNROLLED)
    n = 140000
    assert L.tune('conv_one_round') == 1
    t, ld = _table(n)
    x = torch.ones(n, cin, device='cuda')
    w = torch.ones(K, cin, cout, device='cuda')
    y = torch.empty(n, cout, device='cuda')
    nblk = L.query('sgnn_conv_stats_blocks', n)
    part = torch.zeros(nblk, 2, cout, dtype=torch.float64, device='cuda')
    _epi(x, n, cin, cin, w, t, ld, cout, y, cout, 0, stats=1, part=part)
    live = int((part[:, 1].sum(1) > 0).sum())
    tiles = (n + 255) // 256
    assert nblk >= tiles and 0 < live <= (tiles + 1) // 2, (live, tiles)


# ---- capacity mode, through the program executor ----

_SITES = {}


def _sites(n):
    """(27, n) int64 submanifold rulebook of n distinct sites of a dense cube (the library's own grid and table)."""
    if n not in _SITES:
        from sgnn_amd.scn.metadata import Grid, coords_from_locs
        side = 9 if n <= 600 else 60
        cells = torch.from_numpy(np.random.default_rng(n).permutation(side ** 3)[:n])
        locs = torch.stack([cells // (side * side), (cells // side) % side, cells % side, torch.zeros_like(cells)], 1)
        g = Grid(coords_from_locs(locs, torch.device('cuda')))
        assert g.n == n
        _SITES[n] = g.subm_table().view(K, g.ld)[:, :n].long().clone()
    return _SITES[n]


def _ptrs(values):
    return np.ascontiguousarray(np.array([0 if v is None else v for v in values] + [0], dtype=np.uint64))


def _padded(t, rows, fill):
    out = torch.full((rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device='cuda')
    out[:t.shape[0]] = t
    return out


def _run_program(net, keep, nbr, cap, count, params, x, gout=None):
    """sgnn_prog_forward (training) of a one-level program at capacity `cap` with `count` live rows; with gout = (buffer,
    rows) also sgnn_prog_backward.  Workspace, arenas and gradients start as NaN.  Returns ({buffer: (cap, ch) rows},
    gradient of the external input or None)."""
    L = _lib()
    nops, nbuf, n_ext, ncls = len(net.ops), len(net.bufs), net.n_ext, net.n_classes
    assert ncls == 1 and net.nlev == 1 and n_ext == 1
    lev_n = np.array([cap], dtype=np.int64)
    ld = (cap + 255) // 256 * 256
    lev_ld = np.array([ld], dtype=np.int64)
    tab = torch.full((K, ld), -1, dtype=torch.int32, device='cuda')
    tab[:, :nbr.shape[1]] = nbr.int()
    cnt = torch.tensor([count], dtype=torch.int64, device='cuda')
    tabs = [_ptrs([tab.data_ptr()]), _ptrs([0]), _ptrs([0]), _ptrs([0]), _ptrs([cnt.data_ptr()])]
    nan = float('nan')
    P = [p.cuda().clone() for p in params]
    E = [_padded(x, cap, nan)]
    keepv = np.zeros(nbuf, dtype=np.int32)
    keepv[keep] = 1
    ops, opf, bufs = net.ops_np, net.opf_np, net.bufs_np
    qa = (ops.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data, ncls, keepv.ctypes.data)
    total = L.query('sgnn_prog_arena_floats', *qa, 0)
    fwd_total = L.query('sgnn_prog_arena_floats', *qa, 1)
    assert 0 <= fwd_total <= total
    wsb = L.query('sgnn_prog_ws_bytes', ops.ctypes.data, nops, lev_n.ctypes.data, ncls)
    arena = torch.full((max(total, 1),), nan, device='cuda')
    ws = torch.full((max(wsb, 256),), 0xFF, dtype=torch.uint8, device='cuda')      # every double in it a NaN
    pp, ep, ip = _ptrs([p.data_ptr() for p in P]), _ptrs([e.data_ptr() for e in E]), _ptrs([])
    L.call('sgnn_prog_forward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, len(P), ep.ctypes.data, ip.ctypes.data, 0, arena.data_ptr(),
           fwd_total, keepv.ctypes.data, 1, None, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    out = {}
    for b in keep:
        off = L.query('sgnn_prog_buffer_offset', *qa, 0, b)
        assert off >= 0, b
        ch = int(bufs[b, 1])
        out[b] = arena[off:off + cap * ch].view(cap, ch).clone()
    if gout is None:
        return out, None
    garena = torch.full((max(total, 1),), nan, device='cuda')
    G = _padded(gout[1], cap, nan)
    PG = [None if kind in ('rm', 'rv') else torch.full_like(p, nan) for p, (kind, _) in zip(P, net.slots)]
    GE = [torch.full_like(E[0], nan)]
    gp = _ptrs([G.data_ptr() if b == gout[0] else 0 for b in range(nbuf)])
    pgp = _ptrs([None if g is None else g.data_ptr() for g in PG])
    gep = _ptrs([GE[0].data_ptr()])
    L.call('sgnn_prog_backward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, pgp.ctypes.data, len(P), ep.ctypes.data, gep.ctypes.data,
           ip.ctypes.data, 0, arena.data_ptr(), garena.data_ptr(), total, gp.ctypes.data, keepv.ctypes.data, 1,
           ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    return out, GE[0]


_CAP_CASES = {}


def _cap_case(n, cin, cout):
    """Integer x, w, dy on the n-site level and the fp64 forward rows / input gradient (computed once per shape and size)."""
    key = (n, cin, cout)
    if key not in _CAP_CASES:
        nbr = _sites(n)
        gen = _gen('cap', n, cin, cout)
        x, w, dy = R.int_data((n, cin), gen, 'cuda'), R.int_data((K, cin, cout), gen, 'cuda'), R.int_data((n, cout), gen, 'cuda')
        ref, mag = R.walk(x, w, nbr, K, n, n)
        dref, dmag = R.walk_adjoint(dy, w, nbr, K, n, n, n)
        _CAP_CASES[key] = (nbr, x, w, dy, ref, mag, dref, dmag)
    return _CAP_CASES[key]


def _untouched(rows):
    return bool(torch.isnan(rows).all())


@pytest.mark.parametrize('n', EPI_ROWS)
@pytest.mark.parametrize('cin,cout', SHAPES)
def test_capacity_mode_forward_and_data_gradient(tune, cin, cout, n):
    """One SUBM op, capacity 1.3 n + 5, live count n and 0: forward through k_conv_fwd_u<cin,cout,27>, the gradient of
    the input through <cout,cin,27> (TRANSPOSE_W | FLIP_K), integer data bit-exact; rows past the live count keep their NaN."""
    tune(**UNROLLED)
    nbr, x, w, dy, ref, mag, dref, dmag = _cap_case(n, cin, cout)
    net = C.Net()
    xb = net.ext(0, cin)
    yb = net.subm(xb, cout)
    net.finish()
    cap = int(1.3 * n) + 5
    what = '<%d,%d> capacity %d live ' % (cin, cout, cap)
    out, gx = _run_program(net, [yb], nbr, cap, n, [w], x, gout=(yb, dy))
    R.assert_exact(out[yb][:n], ref, mag, what + '%d fwd' % n)
    assert _untouched(out[yb][n:]), what + '%d: forward wrote past the live rows' % n
    R.assert_exact(gx[:n], dref, dmag, what + '%d dX' % n)
    out, gx = _run_program(net, [yb], nbr, cap, 0, [w], x, gout=(yb, dy))
    assert _untouched(out[yb]), what + '0: forward wrote rows'
    touched = gx[~torch.isnan(gx)]
    assert bool((touched == 0).all()), what + '0: input gradient holds values'


@pytest.mark.parametrize('n', EPI_ROWS)
@pytest.mark.parametrize('cin,cout', SHAPES)
def test_capacity_mode_statistics_partials_feed_batchnorm(tune, cin, cout, n):
    """SUBM -> BatchNorm in training mode: the convolution's statistics epilogue feeds BatchNorm from a workspace that
    starts as NaN, so a partial block that a workgroup without rows did not zero would poison every output row.  Rows of
    the convolution exact; BatchNorm output against fp64 within 8 * 2^-24 of the magnitudes its fp32 steps round
    ((|h| + |mean|) invstd gamma, |beta|, the result): mean and invstd rounded to fp32, one subtraction, one
    multiplication and one fused multiply-add per element are at most 6 roundings of those magnitudes."""
    tune(**UNROLLED)
    assert _lib().tune('prog_fusion') == 1
    nbr, x, w, _, ref, mag, _, _ = _cap_case(n, cin, cout)
    net = C.Net()
    xb = net.ext(0, cin)
    hb = net.subm(xb, cout)
    yb = net.bn(hb)
    net.finish()
    gen = _gen('capbn', n, cin, cout)
    gamma = torch.rand(cout, generator=gen, device='cuda') + 0.5
    beta = torch.randn(cout, generator=gen, device='cuda') * 0.3
    params = [w, gamma, beta, torch.zeros(cout, device='cuda'), torch.ones(cout, device='cuda')]
    cap = int(1.3 * n) + 5
    what = '<%d,%d> capacity %d live ' % (cin, cout, cap)
    out, _ = _run_program(net, [hb, yb], nbr, cap, n, params, x)
    R.assert_exact(out[hb][:n], ref, mag, what + '%d conv rows' % n)
    assert _untouched(out[hb][n:]) and _untouched(out[yb][n:]), what + '%d: wrote past the live rows' % n
    eps = float(net.opf_np[1][0])
    mean = ref.mean(0)
    invstd = 1.0 / torch.sqrt(((ref - mean) ** 2).mean(0) + eps)
    pre = (ref - mean) * invstd * gamma.double() + beta.double()
    want = torch.where(pre > 0, pre, torch.zeros_like(pre))
    lim = 8 * 2.0 ** -24 * ((ref.abs() + mean.abs()) * invstd * gamma.double() + beta.double().abs() + pre.abs())
    err = (out[yb][:n].double() - want).abs()
    assert bool((err <= lim).all()), what + '%d BatchNorm rows: worst err / limit %g' % (n, float((err / lim).max()))
    out, _ = _run_program(net, [hb, yb], nbr, cap, 0, params, x)
    assert _untouched(out[hb]) and _untouched(out[yb]), what + '0: wrote rows'
