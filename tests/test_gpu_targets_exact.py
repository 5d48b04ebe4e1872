"""sgnn_loss_targets (loss.hip: k_targets_fine, k_targets_sites, k_targets_coarse) at the C ABI against
loss_ref.targets, bit for bit.

Which case takes which branch:
  ncoarse 0          only k_targets_fine (+ k_targets_sites with weights).
  ncoarse 1 (2,6,10), 2 (4,12,20), 3 (8,24,40) and (16,8,8): the level below the finest measures 1x3x5, 2x6x10, 4x12x20
                     and 8x4x4 voxels, so the 4x4x4 bricks of k_targets_coarse are partial on every axis (lanes with
                     `in` false feed -inf into the shuffles), coarse extents are odd, and the level L-4 of (16,8,8) is
                     2x1x1.  Batch 1 and 3.
  weights off        w_last NULL and every w[k] NULL; masking off: known NULL.
  trunc 0.5          |occ| <= trunc is false for occ = 1 and -1: the weight rule of the reference stops being trivial.
  sdf / hierarchy    +-inf, +-0, +-trunc, the float32 neighbours of +-trunc on either side, NaN (kept, like
                     torch.clamp_ in loss.compute_targets' tensor-op route), known from {0, 1, 2, 3, 255}.
  input sites        duplicates, rows outside the volume in each of the eight ways (skipped by the bounds check of
                     k_targets_sites), n_locs_dev in {0, 1, n - 1, n, n + 5, None} with in-range rows past the count whose
                     voxels must keep weight_missing_geo.
Every output lies in a sentinel buffer (writes outside are caught), 8-byte aligned as k_targets_coarse reads occ_last as
float2; the inputs must come back untouched."""
import itertools

import numpy as np
import pytest

import glue_ref as R
import loss_ref as LR

pytestmark = pytest.mark.gpu

SHAPES = {0: [(3, 5, 7)], 1: [(2, 6, 10)], 2: [(4, 12, 20)], 3: [(8, 24, 40), (16, 8, 8)]}
WMG = 5.0


def L():
    from sgnn_amd import _lib
    return _lib


def _special(trunc):
    t = np.float32(trunc)
    inf = np.float32(np.inf)
    return np.array([np.inf, -np.inf, 0.0, -0.0, t, -t, np.nextafter(t, inf), np.nextafter(t, -inf), np.nextafter(-t, inf),
                     np.nextafter(-t, -inf), np.nan, np.nan], np.float32)


def _volume(rng, shape, trunc):
    v = rng.uniform(-2 * trunc, 2 * trunc, shape).astype(np.float32)
    sp = _special(trunc)
    flat = v.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size // 2, 4 * len(sp))]
    flat[at] = sp[np.arange(len(at)) % len(sp)]
    return v


def _sites(rng, batch, dims, n_in):
    vol = int(np.prod(dims))
    cells = rng.permutation(batch * vol)[:n_in]
    b, v = cells // vol, cells % vol
    inside = np.stack([v // (dims[1] * dims[2]), (v // dims[2]) % dims[1], v % dims[2], b], 1).astype(np.int64)
    out = np.array([(-1, 0, 0, 0), (dims[0], 0, 0, 0), (0, -1, 0, 0), (0, dims[1], 0, 0), (0, 0, -1, 0), (0, 0, dims[2], 0),
                    (0, 0, 0, -1), (0, 0, 0, batch)], np.int64)
    half = n_in // 2
    # duplicates of the first rows in the middle, the eight kinds of outside rows, in-range rows at the end
    return np.concatenate([inside[:half], out, inside[:3], inside[half:]])


def _run(ncoarse, dims, batch, masking, weights, trunc, n_dev, what):
    Lv = ncoarse + 1
    rng = np.random.default_rng([ncoarse, batch, int(masking), int(weights), int(trunc * 2)] + list(dims))
    shape = lambda k: (batch, 1) + tuple(d >> k for d in dims)
    sdf = _volume(rng, shape(0), trunc)
    known = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), shape(0))
    hierarchy = [_volume(rng, shape(Lv - 1 - h), trunc) for h in range(Lv - 1)]
    locs = _sites(rng, batch, dims, 24)
    n = len(locs)
    live = {'none': None, 'n+5': n + 5, 'n': n, 'n-1': n - 1, '1': 1, '0': 0}[n_dev]
    tsdf, occs, hiers, ws = LR.targets(sdf, known, locs, live, hierarchy, Lv, trunc, masking, WMG if weights else None)

    d_sdf, d_known, d_locs = R.dev_in(sdf), R.dev_in(known), R.dev_in(locs)
    d_live = None if live is None else R.dev_in(np.array([live], np.int64))
    d_hin = [R.dev_in(h) for h in hierarchy]
    o_tsdf, o_occ = R.dev_out(shape(0)), [R.dev_out(shape(Lv - 1 - h)) for h in range(Lv)]
    o_hier = [R.dev_out(shape(Lv - 1 - h)) for h in range(Lv)]
    o_w = [R.dev_out(shape(Lv - 1 - h)) for h in range(Lv)] if weights else None
    for b in [o_tsdf] + o_occ + o_hier + (o_w or []) + d_hin + [d_sdf]:
        assert b.ptr % 8 == 0
    coarse = list(range(Lv - 2, -1, -1))                      # the ABI lists the coarser levels from L-2 downwards
    arr = lambda bufs: np.ascontiguousarray(np.array([0 if b is None else b.ptr for b in bufs] + [0], np.uint64))
    hin, occ, hier = arr([d_hin[h] for h in coarse]), arr([o_occ[h] for h in coarse]), arr([o_hier[h] for h in coarse])
    w = arr([o_w[h] if weights else None for h in coarse])
    L().call('sgnn_loss_targets', d_sdf.ptr, d_known.ptr if masking else None, d_locs.ptr if weights else None,
             n if weights else 0, None if d_live is None or not weights else d_live.ptr, batch, dims[0], dims[1], dims[2],
             float(trunc), int(masking), WMG, ncoarse, hin.ctypes.data, o_tsdf.ptr, o_hier[-1].ptr, o_occ[-1].ptr,
             o_w[-1].ptr if weights else None, occ.ctypes.data, w.ctypes.data if weights else None, hier.ctypes.data)
    R.assert_same_bits(o_tsdf.check(what + ' tsdf'), tsdf, what + ' tsdf')
    for h in range(Lv):
        R.assert_same_bits(o_occ[h].check('%s occ %d' % (what, h)), occs[h], '%s occ %d' % (what, h))
        R.assert_same_bits(o_hier[h].check('%s hier %d' % (what, h)), hiers[h], '%s hier %d' % (what, h))
        if weights:
            R.assert_same_bits(o_w[h].check('%s w %d' % (what, h)), ws[h], '%s w %d' % (what, h))
    R.assert_same_bits(d_sdf.check(what), sdf, what + ': the sdf input')
    assert np.array_equal(d_known.check(what), known) and np.array_equal(d_locs.check(what), locs), what + ': inputs changed'
    for h, b in enumerate(d_hin):
        R.assert_same_bits(b.check(what), hierarchy[h], '%s: hierarchy input %d' % (what, h))
    return occs, ws


@pytest.mark.parametrize('trunc', [3.0, 0.5])
@pytest.mark.parametrize('ncoarse', [0, 1, 2, 3])
def test_targets(ncoarse, trunc):
    for dims in SHAPES[ncoarse]:
        for batch, masking, weights in itertools.product((1, 3), (False, True), (False, True)):
            occs, ws = _run(ncoarse, dims, batch, masking, weights, trunc, 'none',
                            'targets %s x%d mask=%d w=%d trunc=%g' % (dims, batch, masking, weights, trunc))
            if weights and masking and trunc < 1:             # the quirk bites: unknown and occupied voxels keep weight 1
                assert ((ws[-1] == 1) & (occs[-1] != 0)).sum() > 24 and (ws[-1][occs[-1] != 0] == 1).all()


@pytest.mark.parametrize('n_dev', ['n+5', 'n', 'n-1', '1', '0'])
def test_targets_site_count_on_the_device(n_dev):
    for ncoarse, dims in ((0, (3, 5, 7)), (2, (4, 12, 20))):
        _run(ncoarse, dims, 3, True, True, 3.0, n_dev, 'targets %s n_locs_dev=%s' % (dims, n_dev))


@pytest.mark.parametrize('dims,ncoarse', [((8, 24, 36), 3), ((8, 12, 40), 3), ((4, 24, 40), 3), ((3, 6, 10), 1), ((16, 16, 16), 4)])
def test_targets_refusals(dims, ncoarse):
    lib = L().load()
    bufs = [R.dev_out((2, 1) + dims) for _ in range(12)]
    ptrs = np.array([b.ptr for b in bufs[:4]] + [0], np.uint64)
    rc = lib.sgnn_loss_targets(bufs[4].ptr, None, None, 0, None, 2, dims[0], dims[1], dims[2], 3.0, 0, 1.0, ncoarse,
                               ptrs.ctypes.data, bufs[5].ptr, bufs[6].ptr, bufs[7].ptr, None, ptrs.ctypes.data, None,
                               ptrs.ctypes.data, L().stream())
    assert rc != 0 and lib.sgnn_last_error()
    for b in bufs:
        assert R.unwritten(b.check('refusal')).all()
