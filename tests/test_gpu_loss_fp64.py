"""sgnn_loss_levels_fwd / _bwd (loss.hip) driven at the C ABI against the float64 reference of tests/loss_ref.py, on the
data of tests/loss_cases.py (volumes, row values, ties, neighbours, ladder: described there).

Which case takes which branch:
  test_row_counts        m = 1 .. 2049: one block, 255 / 256 / 257 around the block width, several blocks; m = 524288 +
                         1031: loss_blocks() hits LOSS_MAX_BLOCKS = 512, k_loss_partial strides 5 times with a ragged
                         last pass, k_loss_bwd (2048 blocks) twice.  With and without the ladder 0, -0, +-1e-8, +-88,
                         +-104, +-1e4 (expf overflow and underflow on either side).
  test_layouts           vstride / occ_col / sdf_col other than compute_loss's (2,0,1) and (1,-1,0): the column loop of
                         k_loss_bwd, terms switched off by a column of -1.
  test_options           mask_mode 0 with unknown targets (counted as 0), 1, 2; use_log 0 / 1; weights NULL / given.
  test_five_levels       n = 5, m = (3, 2049, 1, 700, 524288 + 1031): blocks with blockIdx.x >= nblk[l] return early;
                         weights NULL next to weights given, zero coefficients, g != 1; the reverse order; every level
                         alone (n = 1, coefficient 1) gives bit-equal sums.
  test_capacity          m_dev in {-3, 0, 1, m - 1, m, m + 5}: the clamp of sgnn_dyn_n, rows past the live count keep the
                         sentinel, m_dev <= 0 takes the `empty` branch of k_loss_finalize (means exactly +0).
  test_all_masked        exact mode, nothing kept: NaN means, every dvals entry +0.
  test_zero_coefficient_drops_a_nan_level   a level with NaN means and coefficients (0, 0) next to a live one: total
                         and cur stay finite (the coef != 0 tests of k_loss_finalize).
  test_stale_workspace   a 1-block level straight after a 512-block level on one workspace (and every workspace is
                         pre-filled with NaN): partials past nblk must not be read.
  test_refusals          the return code of every argument check, nothing launched.

Bars.  Forward, per level: the kept count is exact;  |sum - ref| <= K_F x 2^-24 x sum of magnitudes,
the magnitudes being loss_ref's mag_bce / mag_l1.  Float32 roundings per row as loss_site is written:
  bce   x t is exact (t is 0 or 1); max(x, 0) - x t (1); + log1pf(..) (1); x w (1): R = 3, and two libm calls, expf
        and log1pf (the relative error of expf passes to log1p(e) undiminished at most, as e / (1 + e) <= log1p(e)).
  l1    |p| + 1 and |t| + 1 (1 each, but relative to 1 + |v|: an absolute 2^-24 in the logarithm, which is 1 / log1p|v|
        roundings in units of the magnitude; over the sums of these cases, 0.5 .. 1.5); the subtraction (1); x w (1):
        R = 4 and two logf calls.  Without the log: p - t (1), x w (1).
  The float64 accumulation (at most 525 319 terms) adds less than 1e-10 relative.
  means  (float)(sum / kept): the sum's bar / kept + 1 rounding.
  total  t = 0; t += coef[i] * out2s[i]: the bars of the means x |coef| + (1 + terms) roundings of sum |coef out2s|.
  cur    one addition: the two bars + 1 rounding of |bce mean| + |l1 mean|.
Backward, per entry of a kept row, g0 = g coef / kept:
  occ_col  |dvals - ref| <= K_B x (2^-24 x |g0| x mag_dbce + 2^-149): 2^-149, the float32 denormal spacing, is
           needed because sigmoid(-104) = 6.8e-46 is 0 in float32.  Roundings: g x coef (1), (float)(.. / kept) (1),
           expf (libm), 1 + e (1), 1 / .. (1), - t (1), x w (1), x g0 (1): R = 7 and one libm call.
  sdf_col  ref = g1 w sign(d) / (|p| + 1), bar K_B x (2^-24 x |ref| + 2^-149); |p| + 1 (1), 1 / .. (1), x w (1), x g1 (1)
           and g1's two: R = 6, no libm.  The sign is the reference's wherever |d| > 4 x 2^-24 x mag_l1 (an error of
           sign is 2 |ref|, far over the bar); inside that band either sign or 0 passes; planted ties give exactly 0.
           loss_cases.band_rows() is at most 0.1 % of the kept rows (asserted on the reference in test_loss_ref.py).
  Dropped rows and the other columns are +0.0 bit for bit; rows past the live count keep the sentinel.
K = R + A, A for the libm calls, measured: with SGNN_LOSS_RATIOS set to a file name every case appends its worst
error / (2^-24 x magnitude), forward and backward (profiles/loss_fp64_ratios.txt holds an MI355X run); each K is
the smallest integer at least twice the worst ratio recorded there.
  K_F = 5: worst forward ratio 2.37 (the l1 term of the one-row level, where the absolute 2^-24 of 1 + |v| weighs most;
           the sums over 255 rows and more stay below 0.5): R = 4, so the two logf calls cost A = 1 between them.
  K_B = 8: worst backward ratio 3.74 (one d bce entry among 525 319 rows; below 3 at every smaller size): R = 7, so
           expf costs A = 1.  Both A are far below 8 per libm call: nothing to explain in the device libm."""
import os

import numpy as np
import pytest

import glue_ref as R
import loss_cases as C
import loss_ref as LR

pytestmark = pytest.mark.gpu

K_F, K_B = 5, 8


def L():
    from sgnn_amd import _lib
    return _lib


def _record(what, fwd, bwd):
    path = os.environ.get('SGNN_LOSS_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write('%-64s fwd %8.4f (%.4f of K_F)  bwd %8.4f (%.4f of K_B)\n' % (what, fwd, fwd / K_F, bwd, bwd / K_B))


class Volumes:
    """The shared dense volumes on the device, uploaded once."""
    _dev = None

    @classmethod
    def get(cls):
        if cls._dev is None:
            cls._dev = {k: R.dev_in(v) for k, v in C.volumes().items()}
        return cls._dev


def _workspace():
    import torch
    nbytes = L().query('sgnn_loss_multi_ws_bytes')
    return torch.full((nbytes // 8 + 8,), float('nan'), dtype=torch.float64, device='cuda'), nbytes


class Call:
    """One set of levels on the device: descriptors, outputs in sentinel buffers."""

    def __init__(self, levels, coef, g=1.0):
        vol = Volumes.get()
        self.levels, self.n = levels, len(levels)
        self.coef = np.ascontiguousarray(np.asarray(coef, np.float32).reshape(-1))
        self.g = R.dev_in(np.array([g], np.float32))
        self.held, desc = [], np.zeros((self.n, 16), np.int64)
        for l, lv in enumerate(levels):
            locs, vals = R.dev_in(lv['locs']), R.dev_in(lv['vals'])
            assert locs.ptr % 16 == 0
            md = None if lv['m_dev'] is None else R.dev_in(np.array([lv['m_dev']], np.int64))
            m, vstride = lv['vals'].shape
            desc[l] = [locs.ptr, vals.ptr, vstride, lv['occ_col'], lv['sdf_col'], vol['tgt_occ'].ptr, vol['tgt_sdf'].ptr,
                       0 if lv['weights'] is None else vol['weights'].ptr, vol['known'].ptr, C.DIMS[0], C.DIMS[1], C.DIMS[2],
                       m, lv['use_log'], lv['mask_mode'], 0 if md is None else md.ptr]
            self.held.append((locs, vals, md))
        self.desc = np.ascontiguousarray(desc)

    def forward(self, ws=None):
        n = self.n
        self.sums, self.out2s = R.dev_out((n, 3), np.float64), R.dev_out((n, 2))
        self.total, self.cur = R.dev_out((1,)), R.dev_out((n,))
        self.ws, nbytes = ws if ws is not None else _workspace()
        L().call('sgnn_loss_levels_fwd', self.desc.ctypes.data, n, self.coef.ctypes.data, self.sums.ptr, self.out2s.ptr,
                 self.total.ptr, self.cur.ptr, self.ws.data_ptr(), nbytes)
        return (self.sums.check('sums'), self.out2s.check('out2s'), self.total.check('total')[0], self.cur.check('cur'))

    def backward(self):
        self.dvals = [R.dev_out(lv['vals'].shape) for lv in self.levels]
        ptrs = np.ascontiguousarray(np.array([d.ptr for d in self.dvals] + [0], np.uint64))
        L().call('sgnn_loss_levels_bwd', self.desc.ctypes.data, self.n, self.coef.ctypes.data, self.sums.ptr, self.g.ptr,
                 ptrs.ctypes.data)
        return [R.bits(d.check('dvals %d' % l)) for l, d in enumerate(self.dvals)]

    def check_inputs(self, what):
        for l, (lv, (locs, vals, _)) in enumerate(zip(self.levels, self.held)):
            assert np.array_equal(locs.check(what), lv['locs']), '%s: locs of level %d changed' % (what, l)
            R.assert_same_bits(vals.check(what), lv['vals'], '%s: vals of level %d' % (what, l))


def run(levels, planted, coef, g, what, ws=None):
    """Forward + backward of `levels` against the reference; returns (the call, the reference, sums, out2s)."""
    ref = LR.loss_levels(levels, coef, g)
    call = Call(levels, coef, g)
    sums, out2s, total, cur = call.forward(ws)
    dv = call.backward()
    call.check_inputs(what)
    fwd = bwd = 0.0
    bars = np.zeros((len(levels), 2))
    for l, lv in enumerate(levels):
        w = '%s level %d' % (what, l)
        empty = lv['m_dev'] is not None and lv['m_dev'] <= 0
        r, bars[l] = C.check_forward(ref, l, sums, out2s, K_F, w, empty)
        assert lv['sdf_col'] < 0 or C.band_rows(ref['rows'][l], planted[l]).sum() <= C.BAND_SHARE * ref['sums'][l, 2], \
            '%s: the either-sign band holds more than 0.1 %% of the kept rows' % w
        fwd = max(fwd, r)
        bwd = max(bwd, C.check_backward(ref, l, lv, planted[l], coef, g, dv[l], K_B, w))
    C.check_total(ref, coef, bars, total, cur, what)
    _record(what, fwd, bwd)
    return call, ref, sums, out2s


def one(m, what, coef=(1.0, 1.0), g=1.0, ws=None, **kw):
    lv, pl = C.level(m, **kw)
    return run([lv], [pl], coef, g, what, ws)


@pytest.mark.parametrize('ladder', [False, True])
@pytest.mark.parametrize('m', C.ROW_COUNTS)
def test_row_counts(m, ladder):
    if m == C.BIG and ladder:
        m = 4099                            # the big case runs once; the ladder gets a ragged multi-block size instead
    _, ref, _, _ = one(m, 'rows m=%d ladder=%d' % (m, ladder), ladder=ladder, key=m)
    assert ref['sums'][0, 2] >= 1                # the one-row case included: row 0 is kept under every mask mode


@pytest.mark.parametrize('layout', C.LAYOUTS)
def test_layouts(layout):
    for mask_mode in (1, 2):
        one(1025, 'layout %s mask=%d' % (layout, mask_mode), coef=(0.75, 1.5), g=-2.5, layout=layout, mask_mode=mask_mode,
            ladder=True, key='layout')


@pytest.mark.parametrize('mask_mode', [0, 1, 2])
@pytest.mark.parametrize('use_log', [0, 1])
@pytest.mark.parametrize('weights', [False, True])
def test_options(mask_mode, use_log, weights):
    one(1025, 'options mask=%d log=%d weights=%d' % (mask_mode, use_log, weights), mask_mode=mask_mode, use_log=use_log,
        weights=weights, ladder=True, key='options')


FIVE = (dict(m=3, layout=(2, 0, 1), mask_mode=0, use_log=1, weights=False),
        dict(m=2049, layout=(3, 2, 0), mask_mode=1, use_log=0, weights=True),
        dict(m=1, layout=(1, -1, 0), mask_mode=2, use_log=1, weights=True),
        dict(m=700, layout=(2, 1, -1), mask_mode=1, use_log=1, weights=False, ladder=True),
        dict(m=C.BIG, layout=(2, 0, 1), mask_mode=2, use_log=1, weights=True))
FIVE_COEF = ((1.0, 0.0), (0.5, 2.0), (0.0, 3.0), (1.25, 0.0), (0.25, 0.5))


def test_five_levels():
    made = [C.level(key=('five', k), **kw) for k, kw in enumerate(FIVE)]
    levels, planted = [a for a, _ in made], [b for _, b in made]
    _, ref, sums, out2s = run(levels, planted, FIVE_COEF, 0.375, 'five levels')
    assert np.isfinite(ref['total']) and (ref['sums'][:, 2] >= 1).all()
    _, _, rsums, rout2s = run(levels[::-1], planted[::-1], FIVE_COEF[::-1], 0.375, 'five levels reversed')
    assert np.array_equal(rsums[::-1].view(np.int64), sums.view(np.int64)), 'a level\'s sums depend on its place in the call'
    R.assert_same_bits(np.ascontiguousarray(rout2s[::-1]), out2s, 'means of the reversed call')
    for l in range(5):
        _, _, s1, _ = run(levels[l:l + 1], planted[l:l + 1], (1.0, 1.0), 1.0, 'five levels: level %d alone' % l)
        assert np.array_equal(s1.view(np.int64), sums[l:l + 1].view(np.int64)), 'level %d alone gives other sums' % l


@pytest.mark.parametrize('m', [257, 2049])
def test_capacity(m):
    for live in (-3, 0, 1, m - 1, m, m + 5):
        _, ref, _, out2s = one(m, 'capacity m=%d m_dev=%d' % (m, live), coef=(1.0, 0.5), g=2.0, m_dev=live, ladder=True,
                               key='cap')
        assert ref['rows'][0]['live'] == min(max(live, 0), m) and (live < 1 or ref['sums'][0, 2] >= 1)
        if live <= 0:
            assert (out2s.view(np.int32) == 0).all()


def test_all_masked():
    """Exact mode with every row on an unknown voxel: means NaN, dvals all +0 (the gradient scale is g coef / 0)."""
    lv, pl = C.level(300, mask_mode=1, key='masked')
    lv['locs'] = C.unknown_locs(300)
    pl = dict(tie=np.zeros(300, bool), nb=np.zeros(300, bool))
    call, ref, sums, out2s = run([lv], [pl], (1.0, 1.0), 1.0, 'all masked')
    assert sums[0, 2] == 0 and np.isnan(out2s).all() and np.isnan(ref['out2s']).all()
    assert (R.bits(call.dvals[0].check('dvals')) == 0).all()


def test_zero_coefficient_drops_a_nan_level():
    dead, pl0 = C.level(300, mask_mode=1, key='masked')
    dead['locs'] = C.unknown_locs(300)
    live, pl1 = C.level(700, key='beside')
    pl0 = dict(tie=np.zeros(300, bool), nb=np.zeros(300, bool))
    for order in (0, 1):
        lv, pl, coef = [dead, live], [pl0, pl1], [(0.0, 0.0), (0.5, 2.0)]
        _, ref, _, out2s = run(lv[::1 - 2 * order], pl[::1 - 2 * order], coef[::1 - 2 * order], 1.5, 'zero coefficient, order %d' % order)
        assert np.isnan(out2s[order]).all() and np.isfinite(ref['total']) and np.isfinite(ref['cur']).all()


def test_stale_workspace():
    ws = _workspace()
    one(C.BIG, 'workspace: 512 blocks first', key='ws', ws=ws)
    one(7, 'workspace: 1 block on the used workspace', key='ws', ws=ws)
    one(1025, 'workspace: 2 blocks on the used workspace', key='ws', ws=ws)


def _refusal_cases():
    ok = dict(n=1, vstride=2, occ_col=0, sdf_col=1, mask_mode=1, tgt_occ=True, known=True, ws=0)
    yield 'n=0', dict(ok, n=0)
    yield 'n=6', dict(ok, n=6)
    yield 'occ_col >= vstride', dict(ok, occ_col=2)
    yield 'both columns -1', dict(ok, occ_col=-1, sdf_col=-1)
    yield 'mask_mode=3', dict(ok, mask_mode=3)
    yield 'mask_mode=1 without tgt_occ', dict(ok, occ_col=-1, tgt_occ=False)
    yield 'mask_mode=2 without known', dict(ok, mask_mode=2, known=False)
    yield 'workspace too small', dict(ok, ws=-8)


@pytest.mark.parametrize('name,case', list(_refusal_cases()))
def test_refusals(name, case):
    lib = L().load()
    lv, _ = C.level(16, key='refuse')
    call = Call([lv], (1.0, 1.0))
    desc = np.zeros((6, 16), np.int64)
    desc[:] = call.desc[0]
    desc[:, 2:5] = case['vstride'], case['occ_col'], case['sdf_col']
    desc[:, 14] = case['mask_mode']
    if not case['tgt_occ']:
        desc[:, 5] = 0
    if not case['known']:
        desc[:, 8] = 0
    coef = np.ones(12, np.float32)
    sums, out2s, total, cur = R.dev_out((6, 3), np.float64), R.dev_out((6, 2)), R.dev_out((1,)), R.dev_out((6,))
    ws, nbytes = _workspace()
    rc = lib.sgnn_loss_levels_fwd(desc.ctypes.data, case['n'], coef.ctypes.data, sums.ptr, out2s.ptr, total.ptr, cur.ptr,
                                  ws.data_ptr(), nbytes + case['ws'], L().stream())
    assert rc != 0, '%s: accepted' % name
    assert lib.sgnn_last_error(), name
    for b in (sums, out2s, total, cur):
        assert R.unwritten(b.check(name)).all(), '%s: an output was written' % name
    if case['ws'] == 0:                     # the backward call shares the descriptor checks
        dv = R.dev_out((16, 3))
        ptrs = np.array([dv.ptr] * 6 + [0], np.uint64)
        rc = lib.sgnn_loss_levels_bwd(desc.ctypes.data, case['n'], coef.ctypes.data, sums.ptr, call.g.ptr, ptrs.ctypes.data,
                                      L().stream())
        assert rc != 0, '%s: backward accepted' % name
        assert R.unwritten(dv.check(name)).all()
