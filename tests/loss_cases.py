"""Data and comparison rules of tests/test_gpu_loss_fp64.py, numpy only, so that tests/test_loss_ref.py can check on the
CPU, on the very same inputs, what the GPU test takes for granted about them (classes hit, band size, closed forms).

Volumes: batch 2 of 8 x 12 x 20.  Voxel i (flat) carries
  tgt_occ  (0, 1, -1)[i % 3]            known (0, 1, 2, 255)[(i // 3) % 4]          weights (1, 5)[(i // 12) % 2]
  tgt_sdf  (+0, -0, +trunc, -trunc)[j] for j = (i // 24) % 8 < 4, a uniform draw from (-3, 3) otherwise
so 24 consecutive voxels hold every (occ, known, weight) combination once.  Row r sits on voxel (1543 r + 109) mod 3840
(1543 is coprime to 3840 and to 24: consecutive rows walk through all 24 combinations, sites repeat after 3840 rows;
the loss only gathers; row 0 sits on voxel 109 with tgt_occ 1, known 0, weight 5 and a generic sdf, so it is kept under
every mask mode and the one-row cases m = 1 and m_dev = 1 carry a value through the sums and the gradient).  Every row of locs lies inside the volume, rows past a live count included: loss_site does not
check bounds.

Row values: the logit is +-10^u, u uniform in [-4, log10 30]; the sdf prediction +-e^u over 0.05 .. 4.  Rows r % 32 == 3
predict the target's sdf bit for bit (ties); rows r % 32 == 19 predict its float32 neighbour, alternately above and
below, where the target is a normal non-zero number (the neighbour of +-0 is a denormal: log(|v| + 1) evaluated in
float32, which is the operation's definition, cannot tell it from 0, so it is no neighbour in any useful sense).  With
`ladder`, rows r % 16 == 5 cycle through LADDER.  Columns that are neither occ_col nor sdf_col hold NaN, and so does
every row past the live count: a kernel that reads them shows up as NaN in its sums."""
import zlib

import numpy as np

import loss_ref as LR

BATCH, DIMS, TRUNC = 2, (8, 12, 20), 3.0
NVOX = BATCH * DIMS[0] * DIMS[1] * DIMS[2]
LADDER = np.array([0.0, -0.0, 1e-8, -1e-8, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4], np.float32)
BIG = 524288 + 1031                     # > LOSS_MAX_BLOCKS x 1024 rows: the block cap, 5 stride passes forward, 2 backward
ROW_COUNTS = (1, 255, 256, 257, 1024, 1025, 2049, BIG)
LAYOUTS = ((2, 0, 1), (1, -1, 0), (3, 2, 0), (3, -1, 1), (2, 1, -1))          # vstride, occ_col, sdf_col
BAND = 4.0                              # rows with |d| <= BAND x 2^-24 x mag_l1 may take either sign
BAND_SHARE = 1e-3


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def volumes():
    i = np.arange(NVOX)
    rng = _rng('volumes')
    sdf = rng.uniform(-3.0, 3.0, NVOX).astype(np.float32)
    j = (i // 24) % 8
    for k, v in enumerate((0.0, -0.0, TRUNC, -TRUNC)):
        sdf[j == k] = np.float32(v)
    shape = (BATCH, 1) + DIMS
    return dict(tgt_occ=np.array([0, 1, -1], np.float32)[i % 3].reshape(shape),
                known=np.array([0, 1, 2, 255], np.uint8)[(i // 3) % 4].reshape(shape),
                weights=np.array([1, 5], np.float32)[(i // 12) % 2].reshape(shape),
                tgt_sdf=sdf.reshape(shape))


def row_voxels(m):
    return (np.arange(m, dtype=np.int64) * 1543 + 109) % NVOX


def unknown_locs(n):
    """n in-range sites on voxels whose occupancy target is unknown (-1): dropped under mask_mode 1."""
    d0, d1, d2 = DIMS
    v = np.nonzero(volumes()['tgt_occ'].reshape(-1) == -1)[0][:n]
    return np.stack([(v // (d1 * d2)) % d0, (v // d2) % d1, v % d2, v // (d0 * d1 * d2)], 1).astype(np.int64)


def rows(m, vstride, occ_col, sdf_col, key, ladder=False, live=None):
    """locs (m, 4) int64, vals (m, vstride) float32, and the boolean masks of planted ties and neighbours."""
    d0, d1, d2 = DIMS
    v = row_voxels(m)
    locs = np.stack([(v // (d1 * d2)) % d0, (v // d2) % d1, v % d2, v // (d0 * d1 * d2)], 1).astype(np.int64)
    rng = _rng('rows', key, m)
    vals = np.full((m, vstride), np.nan, np.float32)
    r = np.arange(m)
    tie, nb = np.zeros(m, bool), np.zeros(m, bool)
    if occ_col >= 0:
        x = np.where(rng.random(m) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-4.0, np.log10(30.0), m)
        x = x.astype(np.float32)
        if ladder:
            at = r % 16 == 5
            x[at] = LADDER[(r[at] // 16) % len(LADDER)]
        vals[:, occ_col] = x
    if sdf_col >= 0:
        p = np.where(rng.random(m) < 0.5, -1.0, 1.0) * np.exp(rng.uniform(np.log(0.05), np.log(4.0), m))
        p = p.astype(np.float32)
        t = volumes()['tgt_sdf'].reshape(-1)[v]
        tie = r % 32 == 3
        p[tie] = t[tie]
        nb = (r % 32 == 19) & (np.abs(t) >= np.finfo(np.float32).tiny)
        up = np.where((r // 32) % 2 == 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        p[nb] = np.nextafter(t[nb], up[nb])
        vals[:, sdf_col] = p
    if live is not None:
        vals[LR.live_count(m, live):] = np.nan
    return locs, vals, tie, nb


def level(m, layout=(2, 0, 1), mask_mode=1, use_log=1, weights=True, key=0, ladder=False, m_dev=None):
    """The loss_ref.loss_levels description of one level on the shared volumes, plus 'tie' / 'nb' (planted rows)."""
    vstride, occ_col, sdf_col = layout
    vol = volumes()
    locs, vals, tie, nb = rows(m, vstride, occ_col, sdf_col, (key, layout, mask_mode, use_log), ladder, m_dev)
    lv = dict(locs=locs, vals=vals, occ_col=occ_col, sdf_col=sdf_col, tgt_occ=vol['tgt_occ'], tgt_sdf=vol['tgt_sdf'],
              weights=vol['weights'] if weights else None, known=vol['known'], dims=DIMS, use_log=use_log,
              mask_mode=mask_mode, m_dev=m_dev)
    return lv, dict(tie=tie, nb=nb)


def band_rows(row, planted):
    """Kept rows, planted ones aside, whose l1 difference is too small for float32 to tell its sign."""
    inband = row['keep'] & (np.abs(row['d']) <= BAND * LR.EPS32 * row['mag_l1'])
    return inband & ~planted['tie'] & ~planted['nb']


# ---------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------
def _bad(err, bar):
    return ~(err <= bar)               # NaN counts as a miss


def check_forward(ref, l, sums, out2s, K, what, empty=False):
    """Level l of a forward call against loss_ref.loss_levels: the kept count exactly, either sum within
    K x 2^-24 x sum of magnitudes, the means with that bar divided by kept plus one rounding.
    Returns (largest error / (2^-24 x magnitudes), the bars of the two means)."""
    kept = ref['sums'][l, 2]
    assert sums[l, 2] == kept, '%s: kept count %r, expected %r' % (what, sums[l, 2], kept)
    ratio, mean_bar = 0.0, np.zeros(2)
    for c, name in enumerate(('bce', 'l1')):
        unit = LR.EPS32 * ref['mags'][l, c]
        err = abs(float(sums[l, c]) - ref['sums'][l, c])
        assert not _bad(err, K * unit), '%s: sum %s %.9g, expected %.9g: error %.3g is %.2f x (2^-24 x %.6g)' % (
            what, name, sums[l, c], ref['sums'][l, c], err, err / max(unit, 1e-300), ref['mags'][l, c])
        ratio = max(ratio, err / unit if unit > 0 else 0.0)
        want = ref['out2s'][l, c]
        got = out2s[l, c]
        if empty:
            assert got.view(np.int32) == 0, '%s: mean %s of an empty level is %r, expected +0' % (what, name, got)
        elif np.isnan(want):
            assert np.isnan(got), '%s: mean %s is %r, expected NaN (nothing kept)' % (what, name, got)
        else:
            mean_bar[c] = K * unit / kept + LR.EPS32 * abs(want)
            assert not _bad(abs(float(got) - want), mean_bar[c]), '%s: mean %s %.9g, expected %.9g' % (what, name, got, want)
    return ratio, mean_bar


def check_total(ref, coef, mean_bars, total, cur, what):
    """total and cur of a forward call: the bars of the means carried through coef, plus one rounding per multiplication
    and addition of  t = 0; t += coef[i] * out2s[i]  ((1 + terms) x 2^-24 x sum |coef out2s|), one addition for cur."""
    coef = np.asarray(coef, np.float32).astype(np.float64).reshape(-1, 2)
    used = coef != 0
    if np.isnan(ref['out2s'][used]).any():
        assert np.isnan(total), '%s: total %r, expected NaN' % (what, total)
    else:
        s = np.abs(coef * np.where(used, ref['out2s'], 0.0)).sum()
        bar = (np.abs(coef) * mean_bars).sum() + (1 + used.sum()) * LR.EPS32 * s
        assert not _bad(abs(float(total) - ref['total']), bar), '%s: total %.9g, expected %.9g (bar %.3g)' % (
            what, total, ref['total'], bar)
    for l in range(len(cur)):
        want = ref['cur'][l]
        if np.isnan(want):
            assert np.isnan(cur[l]), '%s: cur[%d] %r, expected NaN' % (what, l, cur[l])
        else:
            bar = (mean_bars[l] * used[l]).sum() + LR.EPS32 * np.abs(np.where(used[l], ref['out2s'][l], 0.0)).sum()
            assert not _bad(abs(float(cur[l]) - want), bar), '%s: cur[%d] %.9g, expected %.9g' % (what, l, cur[l], want)


def check_backward(ref, l, lv, planted, coef, g, dv_bits, K, what):
    """dvals of level l (int32 bit patterns of the (m, vstride) buffer, sentinel where nothing was written).
    Returns the largest error / (2^-24 x magnitude + 2^-149) over the entries of occ_col and sdf_col."""
    from glue_ref import SENT_BITS
    row = ref['rows'][l]
    m, vstride = np.asarray(lv['vals']).shape
    live, keep = row['live'], row['keep']
    sent = np.array([SENT_BITS], np.uint32).view(np.int32)[0]
    assert (dv_bits[live:] == sent).all(), '%s: dvals rows past the live count %d were written' % (what, live)
    dv_bits = dv_bits[:live]
    got = dv_bits.view(np.float32).astype(np.float64)
    zero = np.ones((live, vstride), bool)
    for c in (lv['occ_col'], lv['sdf_col']):
        if c >= 0:
            zero[keep[:live], c] = False
    assert (dv_bits[zero] == 0).all(), '%s: %d entries of dropped rows / unused columns are not +0.0' % (
        what, int((dv_bits[zero] != 0).sum()))
    kept = ref['sums'][l, 2]
    if kept == 0:
        return 0.0
    k = keep[:live]
    coef = np.asarray(coef, np.float32).astype(np.float64).reshape(-1, 2)
    scale = abs(float(np.float32(g))) / kept
    ratio = 0.0
    if lv['occ_col'] >= 0:
        unit = LR.EPS32 * scale * abs(coef[l, 0]) * row['mag_dbce'][:live][k] + LR.TINY32
        err = np.abs(got[k, lv['occ_col']] - ref['dvals'][l][:live][k, lv['occ_col']])
        bad = _bad(err, K * unit)
        assert not bad.any(), '%s: %d d bce entries off, worst %.2f x 2^-24 x magnitude (row %d)' % (
            what, int(bad.sum()), np.nanmax(err / unit), np.nonzero(k)[0][np.argmax(bad)])
        ratio = max(ratio, float((err / unit).max()))
    if lv['sdf_col'] >= 0:
        c = lv['sdf_col']
        want = ref['dvals'][l][:live][k, c]
        slope = 1.0 / (np.abs(np.asarray(lv['vals'], np.float32)[:live][k, c].astype(np.float64)) + 1.0) if lv['use_log'] else 1.0
        mag = scale * abs(coef[l, 1]) * row['w'][:live][k] * slope
        unit = LR.EPS32 * mag + LR.TINY32
        gk = got[k, c]
        tie = planted['tie'][:live][k]
        assert (gk[tie] == 0).all(), '%s: %d planted ties have a non-zero d l1' % (what, int((gk[tie] != 0).sum()))
        inband = (np.abs(row['d']) <= BAND * LR.EPS32 * row['mag_l1'])[:live][k]
        err = np.abs(gk - want)
        either = np.minimum(np.abs(np.abs(gk) - mag), np.where(gk == 0, 0.0, np.inf))
        err = np.where(inband, either, err)
        bad = _bad(err, K * unit)
        assert not bad.any(), '%s: %d d l1 entries off (%d of them sign errors outside the band), worst %.2f x 2^-24 x ' \
            'magnitude (row %d)' % (what, int(bad.sum()), int((bad & ~inband & (np.sign(gk) != np.sign(want))).sum()),
                                    np.nanmax(err / unit), np.nonzero(k)[0][np.argmax(bad)])
        ratio = max(ratio, float((err / unit).max()))
    return ratio
