"""sgnn_iou_counts and sgnn_l1_tgtsurf (metrics.hip) at the C ABI against tests/loss_ref.py.

IoU: the counters {P, C, T} are integers and must be exact.  Which case takes which branch:
  nb 1, 3, 512       k_iou_sparse counts in LDS (nb <= MET_LDS_SAMPLES) and flushes per block;
  nb 513             the global-atomic path, never run by another test;
  targets            float and uint8, holding 0, 1, unknown (-1 / 255) and other values (2, 0.5 / 2, 7: empty);
  row selection      a `keep` byte array (values 0, 1, 2, 255), logits with lstride 1 and 2, neither (all rows);
  use_mask 0 / 1     rows on unknown voxels counted or not;
  rejected rows      outside the volume in each of the eight ways (met_flat);
  m = 0              no sparse launch; m = 262144 + 777: past the 1024-block cap of k_iou_sparse (a second, ragged trip);
  64 x 96 x 96       589 824 voxels per sample > 256 blocks x 256 threads x 8: k_iou_dense strides;
  sigmoid ladder     glue_ref.sigmoid_ladder(): rows with x >= 2^-20 must count, x <= 0 and NaN must not; the band
                     between may go either way, so the counters must lie between the two extremes (lo, hi of
                     loss_ref.iou_counts).  Elsewhere the band is at most 1 % of the rows (here: empty).
  Counters lie in a sentinel buffer: nothing past nb x 3 is written.

L1 on the target surface: out = {sum, count, mean} in float64.  count is exact.  Every term the kernel adds is one
float32 subtraction (fill - t for each surface voxel; p - t and fill - t for each site on the surface), correctly
rounded: at most 2^-24 relative each, so the sum of the float64 conversions is within 2^-24 x sum |terms| of the exact
one.  The float64 accumulation of n terms in any order adds at most (n - 1) x 2^-53 x sum |partial sums| <=
n x 2^-53 x n x max |term|; with n <= 2^22.3 here n x 2^-53 < 2^-30, and the bar takes the looser 2^-50 x n x max |term|
only when that is larger -- both are far below the first term.  out[2] is out[0] / out[1] in float64, bit for bit.
  thresh -1 / 0.0 / 1.0   |t| < truncation, |t| <= 0 (only +-0 voxels), |t| <= 1;  known NULL / given;
  m = 0, no surface voxel at all (count 0, mean NaN), rejected rows, a workspace pre-filled with NaN;
  2 x 128 x 96 x 96 voxels (> 256 x 8 x 1024) and 1024 x 1024 + 333 rows: both stride loops of k_l1_tgtsurf_partial."""
import numpy as np
import pytest

import glue_ref as R
import loss_ref as LR

pytestmark = pytest.mark.gpu


def L():
    from sgnn_amd import _lib
    return _lib


def _ptr(b):
    return None if b is None else b.ptr


def _outside(nb, dims):
    return np.array([(-1, 0, 0, 0), (dims[0], 0, 0, 0), (0, -1, 0, 0), (0, dims[1], 0, 0), (0, 0, -1, 0), (0, 0, dims[2], 0),
                     (0, 0, 0, -1), (0, 0, 0, nb)], np.int64)


def _random_locs(rng, m, nb, dims, outside=True):
    locs = np.stack([rng.integers(0, d, m) for d in dims] + [rng.integers(0, nb, m)], 1).astype(np.int64)
    if outside and m >= 16:
        locs[3:11] = _outside(nb, dims)
    return locs


def _target(rng, nb, dims, u8):
    vals = np.array([0, 1, 255, 2, 7], np.uint8) if u8 else np.array([0, 1, -1, 2, 0.5], np.float32)
    return vals[rng.choice(5, (nb,) + dims, p=[0.3, 0.3, 0.2, 0.1, 0.1])]


def _iou(locs, keep, logits, lstride, tgt, use_mask, what, band_share=0.01):
    nb, dims = tgt.shape[0], tgt.shape[1:]
    m = 0 if locs is None else len(locs)
    lo, hi, band = LR.iou_counts(locs, keep, logits, lstride, tgt, use_mask, nb)
    if band_share is not None:
        assert len(band) <= band_share * max(m, 1), '%s: %d of %d rows in the undetermined band' % (what, len(band), m)
    d_locs = None if locs is None else R.dev_in(locs)
    d_keep = None if keep is None else R.dev_in(keep)
    d_log = None if logits is None else R.dev_in(logits)
    d_tgt, out = R.dev_in(tgt), R.dev_out((nb, 3), np.int64)
    L().call('sgnn_iou_counts', _ptr(d_locs), _ptr(d_keep), _ptr(d_log), lstride, m, d_tgt.ptr, int(tgt.dtype == np.uint8), nb,
             dims[0], dims[1], dims[2], use_mask, out.ptr)
    got = out.check(what)
    assert np.array_equal(got[:, 2], lo[:, 2]), '%s: T differs' % what
    assert ((got >= lo) & (got <= hi)).all(), '%s: %d counters outside [lo, hi], first %s: got %s, lo %s, hi %s' % (
        what, int(((got < lo) | (got > hi)).sum()), np.argwhere((got < lo) | (got > hi))[0], got[(got < lo) | (got > hi)][0],
        lo[(got < lo) | (got > hi)][0], hi[(got < lo) | (got > hi)][0])
    assert ((got[:, 0] - lo[:, 0]) >= (got[:, 1] - lo[:, 1])).all(), what      # a band row adds to C only if it adds to P
    assert np.array_equal(d_tgt.check(what), tgt)
    return got


@pytest.mark.parametrize('nb', [1, 3, 512, 513])
@pytest.mark.parametrize('u8', [False, True])
def test_iou_counts(nb, u8):
    dims = (2, 2, 4)
    rng = np.random.default_rng(nb * 2 + u8)
    tgt = _target(rng, nb, dims, u8)
    m = 4099
    locs = _random_locs(rng, m, nb, dims)
    keep = np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, m)]
    logits = (rng.standard_normal((m, 2)) * 3).astype(np.float32)
    logits[rng.random(m) < 0.1, 0] = 0.0
    for use_mask in (0, 1):
        what = 'iou nb=%d u8=%d mask=%d' % (nb, u8, use_mask)
        _iou(locs, keep, None, 0, tgt, use_mask, what + ' keep')
        _iou(locs, keep, logits, 2, tgt, use_mask, what + ' keep over logits')         # keep wins when both are given
        _iou(locs, None, logits, 2, tgt, use_mask, what + ' logits stride 2')
        _iou(locs, None, np.ascontiguousarray(logits[:, 1]), 1, tgt, use_mask, what + ' logits stride 1')
        _iou(locs, None, None, 0, tgt, use_mask, what + ' all rows')
        _iou(None, None, None, 0, tgt, use_mask, what + ' m=0')


@pytest.mark.parametrize('nb', [3, 513])
def test_iou_counts_past_the_block_cap(nb):
    rng = np.random.default_rng(nb)
    tgt = _target(rng, nb, (2, 2, 4), False)
    m = 262144 + 777
    locs = _random_locs(rng, m, nb, (2, 2, 4))
    logits = (rng.standard_normal(m) * 3).astype(np.float32)
    _iou(locs, None, logits, 1, tgt, 1, 'iou m=%d nb=%d' % (m, nb))


@pytest.mark.parametrize('u8', [False, True])
def test_iou_counts_dense_stride(u8):
    rng = np.random.default_rng(5)
    dims = (64, 96, 96)
    tgt = _target(rng, 1, dims, u8)
    _iou(_random_locs(rng, 1000, 1, dims), None, None, 0, tgt, 1, 'iou dense stride u8=%d' % u8)


@pytest.mark.parametrize('nb', [3, 513])
def test_iou_counts_sigmoid_ladder(nb):
    x = R.sigmoid_ladder()
    m = len(x)
    rng = np.random.default_rng(nb)
    tgt = _target(rng, nb, (2, 2, 4), False)
    locs = _random_locs(rng, m, nb, (2, 2, 4), outside=False)
    got = _iou(locs, None, x, 1, tgt, 0, 'iou ladder nb=%d' % nb, band_share=None)
    keep, drop = R.sigmoid_rule(x)
    assert keep.sum() <= got[:, 0].sum() <= m - drop.sum()


def _l1(locs, vals, tgt, known, trunc, thresh, what):
    nb, dims = tgt.shape[0], tgt.shape[1:]
    m = 0 if locs is None else len(locs)
    s, count, terms, nterms, big = LR.l1_tgtsurf(locs, vals, tgt, known, trunc, thresh)
    import torch
    nbytes = L().query('sgnn_l1_tgtsurf_ws_bytes')
    ws = torch.full((nbytes // 8 + 8,), float('nan'), dtype=torch.float64, device='cuda')
    d_locs, d_vals = (None, None) if locs is None else (R.dev_in(locs), R.dev_in(vals))
    d_tgt, d_known = R.dev_in(tgt), None if known is None else R.dev_in(known)
    out = R.dev_out((3,), np.float64)
    L().call('sgnn_l1_tgtsurf', _ptr(d_locs), _ptr(d_vals), m, d_tgt.ptr, _ptr(d_known), nb, dims[0], dims[1], dims[2],
             float(trunc), float(thresh), out.ptr, ws.data_ptr(), nbytes)
    got = out.check(what)
    assert got[1] == count, '%s: count %r, expected %d' % (what, got[1], count)
    bar = 2.0 ** -24 * terms + 2.0 ** -50 * nterms * big
    assert abs(got[0] - s) <= bar, '%s: sum %.17g, expected %.17g: off by %.3g, bar %.3g' % (what, got[0], s, abs(got[0] - s), bar)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.float64(got[0]) / np.float64(got[1])
    if np.isnan(want):
        assert np.isnan(got[2]), '%s: mean %r, expected NaN' % (what, got[2])
    else:
        assert np.float64(got[2]).view(np.int64) == want.view(np.int64), '%s: mean %r is not sum / count = %r' % (what, got[2], want)
    if count == 0:
        assert np.isnan(got[2]) and got[1] == 0
    R.assert_same_bits(d_tgt.check(what), tgt, what + ': target')
    return got


def _l1_scene(rng, nb, dims, m):
    """Target sdf with +-0, +-trunc and values around them; m unique sites plus the eight kinds of outside rows."""
    vol = nb * int(np.prod(dims))
    tgt = rng.uniform(-4.0, 4.0, (nb,) + dims).astype(np.float32)
    flat = tgt.reshape(-1)
    sp = np.array([0.0, -0.0, 3.0, -3.0, 1.0, -1.0, np.nextafter(np.float32(3), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))], np.float32)
    at = rng.permutation(vol)[:vol // 8]
    flat[at] = sp[np.arange(len(at)) % len(sp)]
    known = rng.choice(np.array([0, 1, 2, 255], np.uint8), (nb,) + dims)
    cells = rng.permutation(vol)[:m] if m < vol // 2 else np.nonzero(rng.random(vol) < 1.05 * m / vol)[0][:m]
    per = int(np.prod(dims))
    b, v = cells // per, cells % per
    locs = np.stack([v // (dims[1] * dims[2]), (v // dims[2]) % dims[1], v % dims[2], b], 1).astype(np.int64)
    locs = np.concatenate([locs[:len(locs) // 2], _outside(nb, dims), locs[len(locs) // 2:]])
    vals = (flat[LR.flat_index(np.clip(locs, 0, None) % np.array(dims + (nb,)), dims)] +
            rng.normal(0, 0.5, len(locs))).astype(np.float32)
    return tgt, known, locs, vals


@pytest.mark.parametrize('thresh', [-1.0, 0.0, 1.0])
@pytest.mark.parametrize('masked', [False, True])
def test_l1_tgtsurf(thresh, masked):
    rng = np.random.default_rng(int(thresh * 2 + 5) * 2 + masked)
    for nb, dims, m in ((1, (3, 5, 7), 40), (3, (8, 12, 20), 1500)):
        tgt, known, locs, vals = _l1_scene(rng, nb, dims, m)
        what = 'l1 %s x%d thresh=%g known=%d' % (dims, nb, thresh, masked)
        got = _l1(locs, vals, tgt, known if masked else None, 3.0, thresh, what)
        assert got[1] > 0 or nb == 1
        _l1(None, None, tgt, known if masked else None, 3.0, thresh, what + ' m=0')


def test_l1_tgtsurf_without_surface():
    rng = np.random.default_rng(1)
    tgt, known, locs, vals = _l1_scene(rng, 2, (4, 6, 10), 100)
    far = np.where(np.abs(tgt) < 3, np.float32(3.5), tgt)
    assert _l1(locs, vals, far, None, 3.0, -1.0, 'l1 no surface')[1] == 0
    assert _l1(locs, vals, tgt, np.full(tgt.shape, 2, np.uint8), 3.0, 1.0, 'l1 nothing known')[1] == 0


def test_l1_tgtsurf_both_stride_loops():
    rng = np.random.default_rng(2)
    tgt, known, locs, vals = _l1_scene(rng, 2, (128, 96, 96), 1024 * 1024 + 333)
    assert len(locs) > 1024 * 1024 + 8 and tgt.size > 256 * 8 * 1024
    _l1(locs, vals, tgt, known, 3.0, -1.0, 'l1 2x128x96x96, %d rows' % len(locs))
