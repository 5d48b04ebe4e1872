"""Host references for loss.hip and metrics.hip: the hierarchical loss and its gradient, the loss targets, the IoU
counters and the target-surface L1.

Plain numpy, float64 arithmetic on float32 inputs, written from the formulas in include/sgnn_hip.h (above
sgnn_loss_levels_*, sgnn_loss_targets, sgnn_iou_counts, sgnn_l1_tgtsurf) and in sgnn_amd/loss.py; nothing is derived
from a kernel and nothing is imported from sgnn_amd (glue_ref supplies the one shared rule, sigmoid_rule).
tests/test_loss_ref.py anchors every function to the oracle restatement of the reference (oracle/model_oracle.py, oracle/metrics_oracle.py) and to the stored reference outputs
under tests/golden/ before a GPU test relies on it.

Besides each value the loss reference returns the magnitude of the terms that cancel in it: a float32 evaluation can be
held to (roundings) x 2^-24 x magnitude, whatever the data's condition."""
import numpy as np

import glue_ref

UNK_ID = -1.0
UNK_THRESH = 2
EPS32 = 2.0 ** -24                  # half a float32 ulp, relative: the error of one correctly rounded operation
TINY32 = 2.0 ** -149                # the spacing of float32 denormals: what a result that underflows may be off by


def flat_index(locs, dims):
    locs = np.asarray(locs, np.int64)
    return ((locs[:, 3] * dims[0] + locs[:, 0]) * dims[1] + locs[:, 1]) * dims[2] + locs[:, 2]


def inside(locs, batch, dims):
    c = np.asarray(locs, np.int64)
    return ((c[:, 0] >= 0) & (c[:, 0] < dims[0]) & (c[:, 1] >= 0) & (c[:, 1] < dims[1]) & (c[:, 2] >= 0) &
            (c[:, 2] < dims[2]) & (c[:, 3] >= 0) & (c[:, 3] < batch))


def live_count(n, n_dev):
    return int(n) if n_dev is None else int(min(max(int(n_dev), 0), int(n)))


def sigmoid(x):
    """1 / (1 + e^-x) with full relative accuracy on either side."""
    return np.exp(-np.logaddexp(0.0, -np.asarray(x, np.float64)))


def logt(v):
    """sign(v) log(|v| + 1)."""
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.log1p(np.abs(v))


# ---------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------
def loss_level(locs, vals, occ_col, sdf_col, tgt_occ, tgt_sdf, weights, known, dims, use_log, mask_mode, live=None):
    """One level, row by row.  vals (m, vstride) float32; the dense volumes hold B x d0 x d1 x d2 elements (any shape).
    Rows >= live (None: all m rows are live) are dropped like masked rows.  Returns a dict of per-row arrays: keep;
    bce, l1 (the weighted terms) and dbce = d bce / d logit, dl1 = d l1 / d sdf, all float64 and 0 on dropped rows;
    mag_bce, mag_l1, mag_dbce = the sums of absolute values behind them; d = the signed difference inside l1."""
    vals = np.asarray(vals, np.float32)
    m = vals.shape[0]
    n_live = live_count(m, live)
    fl = flat_index(np.asarray(locs)[:m], dims)
    vol = lambda a: None if a is None else np.asarray(a).reshape(-1)
    tgt_occ, tgt_sdf, weights, known = vol(tgt_occ), vol(tgt_sdf), vol(weights), vol(known)
    keep = np.arange(m) < n_live
    to = np.zeros(m) if tgt_occ is None else tgt_occ[fl].astype(np.float64)
    if mask_mode == 1:
        keep &= to != UNK_ID
    elif mask_mode == 2:
        keep &= known[fl] < UNK_THRESH
    else:
        assert mask_mode == 0
    w = np.ones(m) if weights is None else weights[fl].astype(np.float64)
    out = {k: np.zeros(m) for k in ('bce', 'l1', 'dbce', 'dl1', 'mag_bce', 'mag_l1', 'mag_dbce', 'd')}
    out['keep'], out['w'], out['live'] = keep, w, n_live
    k = keep
    if occ_col >= 0:
        x = vals[k, occ_col].astype(np.float64)
        t = np.maximum(to[k], 0.0)                   # an unknown (-1) occupancy target that is kept counts as empty
        # -[t log s + (1 - t) log(1 - s)], s = sigmoid(x):  log s = -softplus(-x), log(1 - s) = -softplus(x)
        out['bce'][k] = w[k] * (t * np.logaddexp(0.0, -x) + (1.0 - t) * np.logaddexp(0.0, x))
        out['dbce'][k] = w[k] * (sigmoid(x) - t)
        out['mag_bce'][k] = w[k] * (np.maximum(x, 0.0) + np.abs(x * t) + np.log1p(np.exp(-np.abs(x))))
        out['mag_dbce'][k] = w[k] * (sigmoid(x) + t)
    if sdf_col >= 0:
        p = vals[k, sdf_col].astype(np.float64)
        t = tgt_sdf[fl][k].astype(np.float64)
        if use_log:
            d = logt(p) - logt(t)
            out['mag_l1'][k] = w[k] * (np.abs(logt(p)) + np.abs(logt(t)))
            slope = 1.0 / (np.abs(p) + 1.0)
        else:
            d = p - t
            out['mag_l1'][k] = w[k] * (np.abs(p) + np.abs(t))
            slope = np.ones_like(p)
        out['d'][k] = w[k] * d
        out['l1'][k] = w[k] * np.abs(d)
        out['dl1'][k] = w[k] * np.sign(d) * slope
    return out


def loss_levels(levels, coef, g=1.0):
    """levels: dicts with the arguments of loss_level plus 'm_dev' (None: exact mode).  coef: 2n floats (bce, l1 weight
    per level), g: d loss / d total; both are taken at their float32 values.  Returns a dict:
      rows[l]  the loss_level result;
      sums (n, 3) = {sum bce, sum l1, kept}; mags (n, 2) = the sums of mag_bce, mag_l1;
      out2s (n, 2) = the two means: 0 where m_dev is given and <= 0, NaN where nothing is kept otherwise;
      total = sum of coef * out2s over the slots with coef != 0; cur[l] = the level's two means over those slots;
      dvals[l] (m, vstride) float64: g coef / kept times dbce / dl1 in their columns, 0 elsewhere (rows past the live
      count included: `rows[l]['live']` says which rows the operation writes at all)."""
    n = len(levels)
    coef = np.asarray(coef, np.float32).astype(np.float64).reshape(n, 2)
    g = float(np.float32(g))
    res = dict(rows=[], sums=np.zeros((n, 3)), mags=np.zeros((n, 2)), out2s=np.zeros((n, 2)), cur=np.zeros(n), dvals=[])
    total = 0.0
    for l, lv in enumerate(levels):
        lv = dict(lv)
        m_dev = lv.pop('m_dev', None)
        r = loss_level(live=m_dev, **lv)
        kept = float(r['keep'].sum())
        res['rows'].append(r)
        res['sums'][l] = r['bce'].sum(), r['l1'].sum(), kept
        res['mags'][l] = r['mag_bce'].sum(), r['mag_l1'].sum()
        if m_dev is not None and m_dev <= 0:
            res['out2s'][l] = 0.0
        elif kept == 0:
            res['out2s'][l] = np.nan
        else:
            res['out2s'][l] = res['sums'][l, :2] / kept
        for c in range(2):
            if coef[l, c] != 0:
                total += coef[l, c] * res['out2s'][l, c]
                res['cur'][l] += res['out2s'][l, c]
        vals = np.asarray(lv['vals'])
        dv = np.zeros(vals.shape)
        if kept > 0:
            if lv['occ_col'] >= 0:
                dv[:, lv['occ_col']] = g * coef[l, 0] / kept * r['dbce']
            if lv['sdf_col'] >= 0:
                dv[:, lv['sdf_col']] = g * coef[l, 1] / kept * r['dl1']
        res['dvals'].append(dv)
    res['total'] = total
    return res


# ---------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------
def clamp_keep_nan(v, trunc):
    """torch.clamp_(-trunc, trunc): infinities go to +-trunc, -0 stays -0, NaN stays NaN (with its bits)."""
    v = np.asarray(v, np.float32)
    t = np.float32(trunc)
    with np.errstate(invalid='ignore'):
        c = np.where(v < -t, -t, np.where(v > t, t, v)).astype(np.float32)
    return c


def targets(sdf, known, input_locs, live, hierarchy, L, trunc, masking, wmg):
    """sdf, known: (B, 1, d0, d1, d2); hierarchy[h] for h < L - 1: (B, 1, d >> (L - 1 - h)).  wmg None: no weights.
    Returns tsdf, occs[L], hiers[L], weights[L] or None, all float32 and exact:
      tsdf = clamp(sdf); hiers[L-1] = tsdf; occs[L-1] = |tsdf| < trunc, -1 where known >= 2 (masking);
      weights[L-1] = wmg where |occ| <= trunc off the first clamp(live, 0, n) input sites that lie inside the volume, 1
      elsewhere; occs[h] = 2x2x2 maximum of occs[h+1]; weights[h] = weights[h+1][::2, ::2, ::2]; hiers[h] = clamp."""
    sdf = np.asarray(sdf, np.float32)
    B, _, d0, d1, d2 = sdf.shape
    t = np.float32(trunc)
    tsdf = clamp_keep_nan(sdf, trunc)
    occs, hiers = [None] * L, [None] * L
    weights = None if wmg is None else [None] * L
    hiers[L - 1] = tsdf.copy()
    with np.errstate(invalid='ignore'):
        occ = (np.abs(tsdf) < t).astype(np.float32)
    if masking:
        occ[np.asarray(known) >= UNK_THRESH] = UNK_ID
    occs[L - 1] = occ
    if wmg is not None:
        w = np.where(np.abs(occ) <= t, np.float32(wmg), np.float32(1)).astype(np.float32)
        if input_locs is not None:
            loc = np.asarray(input_locs, np.int64)[:live_count(len(input_locs), live)]
            loc = loc[inside(loc, B, (d0, d1, d2))]
            w.reshape(-1)[flat_index(loc, (d0, d1, d2))] = 1
        weights[L - 1] = w
    for h in range(L - 2, -1, -1):
        f = occs[h + 1]
        s = f.shape
        occs[h] = f.reshape(s[0], 1, s[2] // 2, 2, s[3] // 2, 2, s[4] // 2, 2).max(axis=(3, 5, 7))
        hiers[h] = clamp_keep_nan(hierarchy[h], trunc)
        if wmg is not None:
            weights[h] = np.ascontiguousarray(weights[h + 1][:, :, ::2, ::2, ::2])
    return tsdf, occs, hiers, weights


# ---------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------
def occ_class(tgt):
    """0 empty, 1 occupied, 2 unknown: float targets 1 / -1, uint8 targets 1 / 255; any other value is empty."""
    tgt = np.asarray(tgt)
    unknown = 255 if tgt.dtype == np.uint8 else -1
    return np.where(tgt == 1, 1, np.where(tgt == unknown, 2, 0))


def iou_counts(locs, keep, logits, lstride, tgt, use_mask, nb):
    """tgt (nb, d0, d1, d2) float32 or uint8.  Rows count when keep[r] != 0; without keep, when
    sigmoid(logits[r * lstride]) > 0.5; with neither, always.  Returns (lo, hi, band): int64 (nb, 3) counters {P, C, T}
    with the rows whose decision float32 rounding may flip (band, row numbers) left out (lo) and counted (hi)."""
    tgt = np.asarray(tgt)
    dims = tgt.shape[1:]
    m = 0 if locs is None else len(locs)
    cls = occ_class(tgt).reshape(-1)
    sure, maybe = np.ones(m, bool), np.zeros(m, bool)
    if keep is not None:
        sure = np.asarray(keep)[:m] != 0
    elif logits is not None:
        x = np.asarray(logits, np.float32).reshape(-1)[:m * lstride:lstride] if m else np.zeros(0, np.float32)
        must_keep, must_drop = glue_ref.sigmoid_rule(x)
        sure, maybe = must_keep, ~must_keep & ~must_drop
    out = []
    for sel in (sure, sure | maybe):
        c = np.zeros((nb, 3), np.int64)
        if m:
            ok = sel & inside(locs, nb, dims)
            l = np.asarray(locs, np.int64)[ok]
            k = cls[flat_index(l, dims)]
            if use_mask:
                l, k = l[k != 2], k[k != 2]
            c[:, 0] = np.bincount(l[:, 3], minlength=nb)
            c[:, 1] = np.bincount(l[k == 1][:, 3], minlength=nb)
        c[:, 2] = (cls.reshape(nb, -1) == 1).sum(1)
        out.append(c)
    return out[0], out[1], np.nonzero(maybe)[0]


def l1_tgtsurf(locs, vals, tgt, known, trunc, thresh):
    """Mean |pred - t| over the target's surface voxels, the prediction being -trunc wherever no site predicts.  tgt
    (nb, d0, d1, d2) float32; surface: |t| <= thresh, or |t| < trunc when thresh < 0; known drops voxels with known >= 2;
    rows outside the volume are ignored, sites are unique.  Returns (sum, count, sum of |terms|, number of terms, largest
    |term|), the terms being the differences fill - t of every surface voxel and p - t, fill - t of every site on it."""
    tgt = np.asarray(tgt, np.float32)
    nb, dims = tgt.shape[0], tgt.shape[1:]
    t = tgt.reshape(-1).astype(np.float64)
    thresh, trunc = float(np.float32(thresh)), float(np.float32(trunc))
    with np.errstate(invalid='ignore'):
        surf = (np.abs(t) <= thresh) if thresh >= 0 else (np.abs(t) < trunc)
    if known is not None:
        surf &= np.asarray(known).reshape(-1) < UNK_THRESH
    fill = -trunc
    base = np.abs(fill - t[surf])
    total, terms, biggest = base.sum(), base.sum(), base.max() if base.size else 0.0
    nterms = int(base.size)
    if locs is not None and len(locs):
        ok = inside(locs, nb, dims)
        fl = flat_index(np.asarray(locs)[ok], dims)
        assert len(np.unique(fl)) == len(fl), 'l1_tgtsurf: sites must be unique'
        p = np.asarray(vals, np.float32).reshape(-1)[:len(locs)][ok].astype(np.float64)
        on = surf[fl]
        a, b = np.abs(p[on] - t[fl][on]), np.abs(fill - t[fl][on])
        total += (a - b).sum()
        terms += a.sum() + b.sum()
        nterms += 2 * int(on.sum())
        if a.size:
            biggest = max(biggest, a.max(), b.max())
    return float(total), int(surf.sum()), float(terms), nterms, float(biggest)
