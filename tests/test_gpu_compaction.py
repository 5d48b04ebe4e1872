"""The stream compaction, the coordinate kernels and the voxel hash of grid_rules.hip against tests/glue_ref.py.

Which set-up reaches which kernel:
  sgnn_compact_mask / _sigmoid / _dense and the four _cap / _cap_locs forms
      k_scan_count<F> -> k_scan_emit<F, Emit> with F = FlagMask / FlagSigmoid / FlagDense and Emit = EmitSel / EmitSelLocs.
      scan_inline = 1 (default) and <= 4096 blocks: k_scan_emit sums the raw block counts itself (scan_offsets_inline,
      scan_publish); scan_inline = 0: k_scan_block_sums between the two.  test_compact_mask_block_scan_carry
      (n = 1024 x 2048 + 2049, scan_inline = 0) runs the second iteration of k_scan_block_sums' 1024-wide loop and its carry;
      test_compact_mask_beyond_inline_limit (n = 4096 x 2048 + 1, default switches) takes the automatic fall-back to
      the three-launch form above SCAN_INLINE_MAX blocks.
  sgnn_coords_from_i64 / _to_i64, sgnn_expand8_coords / _i64, sgnn_dense_coords, sgnn_hash_build / _lookup: one kernel each.
  The test_wrapper* cases at the end go through sgnn_amd.scn.functions instead of the library: compact_sigmoid, compact_mask,
      compact_sigmoid_plan and compact_capped on 300 candidates of a batch-2 8x8x8 volume against a NumPy selection, each
      asserting which of the seven entry points its switches (teacher volume, capacity, FUSED_GLUE, metadata.CHAIN) chose.

Sizes sit on the 256-thread and 2048-item edges; masks are none / all / alternating / first / last / random / one whole
2048 block empty.  Outputs lie in sentinel buffers: sel past the total, locs past min(total, keep_cap) and rows past a
device count must still hold the sentinel.  The scan_inline switch is restored by a fixture.

The sigmoid predicate (test_sigmoid_threshold): on the ladder of glue_ref.sigmoid_ladder the kernel keeps exactly the
logits above one threshold; x <= 0 and NaN are dropped, x >= 2^-20 kept.  Measured on an MI355X: the smallest kept ladder
value is 8.288770914077759e-08 (2^-23.524; below it 1 / (1 + expf(-x)) rounds to exactly 0.5), and
torch.sigmoid(x) > 0.5 evaluated by torch on the same device agrees on all 1657 ladder values, so the agreement is
asserted: the kernel's "identical predicate" holds on the ladder, band included."""
import numpy as np
import pytest
import torch

import glue_ref as R

pytestmark = pytest.mark.gpu

DIMS, BATCH = (17, 17, 17), 2             # 9826 voxels: room for the 9000 candidates of the dense predicate


def L():
    from sgnn_amd import _lib
    return _lib


@pytest.fixture(params=[1, 0], ids=['inline', 'three_launch'])
def scan_inline(request):
    saved = L().tune('scan_inline')
    L().tune('scan_inline', request.param)
    try:
        yield request.param
    finally:
        L().tune('scan_inline', saved)


def _ws(n):
    wsb = L().query('sgnn_compact_ws_bytes', n)
    return torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda'), wsb


def _i64(v):
    return R.dev_in(np.array([v], np.int64))


def _sites(n):
    """n distinct sites of the volume in random order; a few replaced by sites outside it (never kept)."""
    vol = int(np.prod(DIMS))
    cells = np.random.default_rng(n).permutation(vol * BATCH)[:n]
    b, v = cells // vol, cells % vol
    coords = np.stack([v // (DIMS[1] * DIMS[2]), (v // DIMS[2]) % DIMS[1], v % DIMS[2], b], 1).astype(np.int32)
    if n >= 64:
        coords[7], coords[n // 2], coords[n - 2] = (-1, 0, 0, 0), (0, DIMS[1], 0, 1), (1, 1, 1, BATCH)
    return coords


def _volume(coords, mask):
    """A dense (B, d0, d1, d2) volume that is 1 at the kept sites, 0.5 (not > 0.5) or 0.25 elsewhere."""
    vol = np.where(np.random.default_rng(5).random((BATCH,) + DIMS) < 0.5, 0.5, 0.25).astype(np.float32)
    inside = R.dense_predicate(coords, np.ones((BATCH,) + DIMS, np.float32))
    c = coords[inside & mask]
    vol[c[:, 3], c[:, 0], c[:, 1], c[:, 2]] = 1.0
    return vol


def _logits(mask):
    """Stride-2 logits: column 0 decides (+-1 and a few +-0), column 1 says the opposite."""
    x = np.where(mask, 1.0, -1.0).astype(np.float32)
    x[~mask & (np.arange(len(mask)) % 5 == 0)] = 0.0
    return np.stack([x, -x + 0.5], 1).astype(np.float32)


def _check_sel(sel, count, ref, what, count_words=1):
    R.assert_compaction(sel.check(what + ' sel'), count.check(what + ' count'), ref, what)


def _run_plain(kind, mask, what):
    n = len(mask)
    ws, wsb = _ws(n)
    sel, count = R.dev_out((n,), np.int32), R.dev_out((1,), np.int64)
    if kind == 'mask':
        m = R.dev_in(mask.astype(np.uint8))
        L().call('sgnn_compact_mask', m.ptr, n, sel.ptr, count.ptr, ws.data_ptr(), wsb)
        pred = mask
    elif kind == 'sigmoid':
        x = R.dev_in(_logits(mask))
        L().call('sgnn_compact_sigmoid', x.ptr, 2, n, sel.ptr, count.ptr, ws.data_ptr(), wsb)
        pred = mask
    else:
        coords = _sites(n)
        vol = _volume(coords, mask)
        co, v = R.dev_in(coords), R.dev_in(vol)
        L().call('sgnn_compact_dense', co.ptr, n, v.ptr, BATCH, *DIMS, sel.ptr, count.ptr, ws.data_ptr(), wsb)
        pred = R.dense_predicate(coords, vol)
    _check_sel(sel, count, R.compaction(pred), what)


@pytest.mark.parametrize('kind', ['mask', 'sigmoid', 'dense'])
def test_compact(kind, scan_inline):
    for n in R.COMPACT_SIZES:
        for name, mask in R.masks(n).items():
            _run_plain(kind, mask, 'compact_%s n=%d %s inline=%d' % (kind, n, name, scan_inline))


def _run_cap(kind, locs, mask, n_dev, cap_rule, what):
    """cap_rule: offset from the total (of the live candidates), or None for keep_cap = 0."""
    n = len(mask)
    coords = _sites(n)
    if kind == 'sigmoid':
        pred, x = mask, R.dev_in(_logits(mask))
    else:
        vol = _volume(coords, mask)
        pred, v = R.dense_predicate(coords, vol), R.dev_in(vol)
    total = R.compaction(pred, n_dev)['total']
    keep_cap = 0 if cap_rule is None else max(total + cap_rule, 0)
    ref = R.compaction(pred, n_dev, keep_cap)
    ws, wsb = _ws(n)
    co, nd = R.dev_in(coords), (None if n_dev is None else _i64(n_dev))
    sel, count2 = R.dev_out((n,), np.int32), R.dev_out((2,), np.int64)
    status = R.dev_in(np.array([R.STATUS_DUPLICATE], np.int32))
    out = R.dev_out((keep_cap + 3, 4), np.int32)
    ndp = None if nd is None else nd.ptr
    tail = (count2.ptr, keep_cap, status.ptr, ws.data_ptr(), wsb)
    if kind == 'sigmoid' and locs:
        L().call('sgnn_compact_sigmoid_cap_locs', x.ptr, 2, n, ndp, co.ptr, sel.ptr, out.ptr, *tail)
    elif kind == 'sigmoid':
        L().call('sgnn_compact_sigmoid_cap', x.ptr, 2, n, ndp, sel.ptr, *tail)
    elif locs:
        L().call('sgnn_compact_dense_cap_locs', co.ptr, n, ndp, v.ptr, BATCH, *DIMS, sel.ptr, out.ptr, *tail)
    else:
        L().call('sgnn_compact_dense_cap', co.ptr, n, ndp, v.ptr, BATCH, *DIMS, sel.ptr, *tail)
    what = '%s n_dev=%s keep_cap=%d total=%d' % (what, n_dev, keep_cap, total)
    _check_sel(sel, count2, ref, what, 2)
    st = int(status.check(what + ' status')[0])
    assert st == R.STATUS_DUPLICATE | (R.STATUS_OVERFLOW if ref['overflow'] else 0), '%s: status %d' % (what, st)
    k = ref['count']
    got = out.check(what + ' locs', untouched=(np.arange(keep_cap + 3) >= (k if locs else 0))[:, None])
    if locs:
        R.assert_same_bits(got[:k], coords[ref['sel'][:k]], what + ' locs')


CAP_RULES = (None, -1, 0, 1)


@pytest.mark.parametrize('locs', [False, True], ids=['cap', 'cap_locs'])
@pytest.mark.parametrize('kind', ['sigmoid', 'dense'])
def test_compact_cap(kind, locs, scan_inline):
    k = 0
    for n in R.COMPACT_SIZES:
        for name, mask in R.masks(n).items():
            _run_cap(kind, locs, mask, None, CAP_RULES[k % 4], 'compact_%s_cap%s n=%d %s' % (kind, '_locs' * locs, n, name))
            k += 1
    for n in (257, 2049, 9000):
        mask = R.masks(n)['random']
        for n_dev in (None, 0, 1, n - 1, n, n + 9, -1):
            for rule in CAP_RULES:
                _run_cap(kind, locs, mask, n_dev, rule, 'compact_%s_cap%s n=%d random' % (kind, '_locs' * locs, n))


def _big_mask(n, what):
    mask = np.random.default_rng(n).random(n) < 0.3
    mask[n - 1] = True
    ws, wsb = _ws(n)
    m, sel, count = R.dev_in(mask.astype(np.uint8)), R.dev_out((n,), np.int32), R.dev_out((1,), np.int64)
    L().call('sgnn_compact_mask', m.ptr, n, sel.ptr, count.ptr, ws.data_ptr(), wsb)
    _check_sel(sel, count, R.compaction(mask), what)


def test_compact_mask_block_scan_carry():
    saved = L().tune('scan_inline')
    L().tune('scan_inline', 0)
    try:
        _big_mask(1024 * 2048 + 2049, 'compact_mask n=1024*2048+2049 three launches')    # 1026 blocks: two scan iterations
    finally:
        L().tune('scan_inline', saved)


def test_compact_mask_beyond_inline_limit():
    assert L().tune('scan_inline') == 1
    _big_mask(4096 * 2048 + 1, 'compact_mask n=4096*2048+1')                              # 4097 blocks > SCAN_INLINE_MAX


def test_sigmoid_threshold(capsys):
    """One threshold over the ladder, and the same answers as torch.sigmoid(x) > 0.5 from torch's own kernel (the module
    docstring holds the measured threshold)."""
    x = R.sigmoid_ladder()
    n = len(x)
    ws, wsb = _ws(n)
    d, sel, count = R.dev_in(x), R.dev_out((n,), np.int32), R.dev_out((1,), np.int64)
    L().call('sgnn_compact_sigmoid', d.ptr, 1, n, sel.ptr, count.ptr, ws.data_ptr(), wsb)
    total = int(count.check('count')[0])
    keep = np.zeros(n, bool)
    keep[sel.check('sel')[:total]] = True
    must_keep, must_drop = R.sigmoid_rule(x)
    assert keep[must_keep].all(), 'dropped %s' % x[must_keep & ~keep][:5]
    assert not keep[must_drop].any(), 'kept %s' % x[must_drop & keep][:5]
    pos = x > 0
    order = np.argsort(x[pos])
    k = keep[pos][order]
    assert (np.diff(k.astype(int)) >= 0).all(), 'the predicate is not monotone over the ladder'
    thr = x[pos][order][k][0]
    tk = (torch.sigmoid(torch.from_numpy(x).cuda()) > 0.5).cpu().numpy()
    diff = x[tk != keep]
    line = 'sigmoid predicate: smallest kept ladder value %s (2^%.3f); torch.sigmoid(x) > 0.5 on the device differs on %d of %d ' \
           'ladder values%s' % (repr(float(thr)), np.log2(float(thr)), len(diff), n,
                               '' if not len(diff) else ': %s .. %s' % (repr(float(diff.min())), repr(float(diff.max()))))
    with capsys.disabled():
        print('\n' + line)
    assert not len(diff), line


# ---- coordinates ----

def _from_i64(locs, n_dev, preset):
    n = len(locs)
    src, out, status = R.dev_in(locs), R.dev_out((n, 4), np.int32), R.dev_in(np.array([preset], np.int32))
    nd = None if n_dev is None else _i64(n_dev)
    L().call('sgnn_coords_from_i64', src.ptr, n, out.ptr, status.ptr, None if nd is None else nd.ptr)
    return out, int(status.check('status')[0])


def test_coords_from_i64_range_flags():
    for name, col, value in R.range_cases():
        for n, row in ((200, 0), (200, 199), (65, 64)):          # first, last, and alone in a ragged second wave
            locs = R.clean_locs(name, n)
            locs[row, col] = value
            what = 'coords_from_i64 %s at row %d of %d' % (name, row, n)
            want, bad = R.coords_from_i64(locs)
            assert bad
            out, st = _from_i64(locs, None, R.STATUS_DUPLICATE)
            assert st == R.STATUS_DUPLICATE | R.STATUS_COORD_RANGE, '%s: status %d' % (what, st)
            R.assert_same_bits(out.check(what), want, what)
        locs = R.clean_locs(name, 200)
        locs[150, col] = value                                   # beyond the device count: not converted, not flagged
        out, st = _from_i64(locs, 100, 0)
        assert st == 0, 'coords_from_i64 %s beyond n_dev: status %d' % (name, st)
        got = out.check(name, untouched=(np.arange(200) >= 100)[:, None])
        R.assert_same_bits(got[:100], R.coords_from_i64(locs, 100)[0], name)


def test_coords_from_i64_second_trip_flags_its_last_row():
    n = 4096 * 256 + 65
    locs = R.clean_locs('big', n)
    locs[n - 1, 3] = 32768
    out, st = _from_i64(locs, None, 0)
    assert st == R.STATUS_COORD_RANGE
    R.assert_same_bits(out.check('big'), R.coords_from_i64(locs)[0], 'coords_from_i64 n=%d' % n)


def test_coords_clean_round_trip():
    for n in (1, 65, 1000):
        locs = R.clean_locs('clean', n)                          # holds (65535, 65535, 65535, 32767) and zeros
        for preset in (0, R.STATUS_DUPLICATE):
            out, st = _from_i64(locs, None, preset)
            assert st == preset
        c32 = out.check('clean')
        R.assert_same_bits(c32, R.coords_from_i64(locs)[0], 'coords_from_i64 clean n=%d' % n)
        for n_dev in (None, n // 2):
            back = R.dev_out((n, 4), np.int64)
            nd = None if n_dev is None else _i64(n_dev)
            L().call('sgnn_coords_to_i64', out.ptr, n, back.ptr, None if nd is None else nd.ptr)
            k = R.live_count(n, n_dev)
            got = back.check('to_i64', untouched=(np.arange(n) >= k)[:, None])
            R.assert_same_bits(got[:k], locs[:k], 'coords_to_i64 n=%d n_dev=%s' % (n, n_dev))


def test_expand8():
    for n in (1, 31, 32, 33, 1234):
        rng = np.random.default_rng(n)
        coords = np.stack([rng.integers(0, 32768, n) for _ in range(3)] + [rng.integers(0, 4, n)], 1).astype(np.int32)
        coords[0, :3] = 32767                                    # children reach 65535
        for n_dev in (None, 0, n - 1, n + 3):
            src, nd = R.dev_in(coords), (None if n_dev is None else _i64(n_dev))
            ndp = None if nd is None else nd.ptr
            k = 8 * R.live_count(n, n_dev)
            want = R.expand8(coords)[:k]
            keep = (np.arange(8 * n) >= k)[:, None]
            a = R.dev_out((8 * n, 4), np.int32)
            L().call('sgnn_expand8_coords', src.ptr, n, a.ptr, ndp)
            what = 'expand8 n=%d n_dev=%s' % (n, n_dev)
            R.assert_same_bits(a.check(what, untouched=keep)[:k], want, what)
            b, l64 = R.dev_out((8 * n, 4), np.int32), R.dev_out((8 * n, 4), np.int64)
            L().call('sgnn_expand8_coords_i64', src.ptr, n, b.ptr, l64.ptr, ndp)
            R.assert_same_bits(b.check(what, untouched=keep)[:k], want, what + ' (i64 form)')
            R.assert_same_bits(l64.check(what, untouched=keep)[:k], want.astype(np.int64), what + ' int64 rows')
    assert R.expand8(np.array([[32767, 32767, 32767, 1]]))[7].tolist() == [65535, 65535, 65535, 1]


def test_dense_coords():
    for batch, dims in ((2, (3, 5, 7)), (1, (1, 5, 7)), (3, (4, 1, 1)), (1, (1, 1, 1)), (0, (3, 5, 7))):
        total = batch * int(np.prod(dims))
        out = R.dev_out((max(total, 1), 4), np.int32)
        L().call('sgnn_dense_coords', batch, *dims, out.ptr)
        what = 'dense_coords batch=%d dims=%s' % (batch, dims)
        got = out.check(what, untouched=np.arange(max(total, 1))[:, None] >= total)
        R.assert_same_bits(got[:total], R.dense_coords(batch, *dims), what)


# ---- hash ----

def _hash(sites, cap, queries, preset, what, m_dev=None):
    n, m = len(sites), len(queries)
    keys = torch.empty(cap, dtype=torch.int64, device='cuda')
    vals = torch.empty(cap, dtype=torch.int32, device='cuda')
    s, q, status = R.dev_in(sites), R.dev_in(queries), R.dev_in(np.array([preset], np.int32))
    L().call('sgnn_hash_build', s.ptr, n, keys.data_ptr(), vals.data_ptr(), cap, status.ptr, None)
    rows = R.dev_out((m,), np.int32)
    md = None if m_dev is None else _i64(m_dev)
    L().call('sgnn_hash_lookup', keys.data_ptr(), vals.data_ptr(), cap, q.ptr, m, rows.ptr, None if md is None else md.ptr)
    k = R.live_count(m, m_dev)
    got = rows.check(what, untouched=np.arange(m) >= k)
    return got[:k], int(status.check(what)[0])


def _queries(sites, key):
    rng = np.random.default_rng(key)
    absent = sites[rng.permutation(len(sites))[:200]].copy()
    absent[:, 0] += 1000                                          # no site has z >= 1000
    bad = np.array([(-1, 0, 0, 0), (0, -5, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1), (65536, 0, 0, 0), (0, 65536, 0, 0),
                    (0, 0, 70000, 0), (0, 0, 0, 32768), (sites[0][0] - 65536, sites[0][1], sites[0][2], sites[0][3])], np.int32)
    q = np.concatenate([sites, absent, bad])
    return q[rng.permutation(len(q))]


@pytest.mark.parametrize('cloud', ['random', 'cube'])
def test_hash_build_lookup(cloud):
    sites = R.random_sites('hash', 3000) if cloud == 'random' else R.dense_coords(1, 12, 12, 12)      # clustered keys
    n = len(sites)
    q = _queries(sites, n)
    want = R.hash_rows(sites, q)
    assert (want >= 0).sum() == n and (want < 0).sum() == 209
    small = 2
    while small < 2 * n:
        small *= 2
    for cap in (L().query('sgnn_hash_capacity', n), small):
        what = 'hash %s n=%d cap=%d' % (cloud, n, cap)
        got, st = _hash(sites, cap, q, R.STATUS_COORD_RANGE, what)
        assert st == R.STATUS_COORD_RANGE, '%s: status %d' % (what, st)           # no duplicate; the other bit survives
        R.assert_same_bits(got, want, what)
    got, _ = _hash(sites, small, q, 0, 'hash m_dev', m_dev=100)
    R.assert_same_bits(got, want[:100], 'hash lookup with a device count')
    dup = np.concatenate([sites, sites[3:4]])
    assert R.has_duplicates(dup) and not R.has_duplicates(sites)
    got, st = _hash(dup, 2 * small, q, R.STATUS_COORD_RANGE, 'hash duplicate')
    assert st == R.STATUS_COORD_RANGE | R.STATUS_DUPLICATE
    # either of the two rows of the repeated site may win; every other query answers as before
    assert set(np.nonzero(got != want)[0]) <= set(np.nonzero((q == sites[3]).all(1))[0])


# ---- the host wrappers of sgnn_amd.scn.functions: each of the seven entry points through the wrapper that chooses it ----

W_N, W_DIMS, W_BATCH, W_CAP = 300, (8, 8, 8), 2, 512


@pytest.fixture(scope='module')
def wrapper_case():
    """300 distinct candidate sites of a batch-2 8x8x8 volume in random order, with stride-2 logits and a teacher volume
    that keep two different subsets of them; everything the NumPy selections below need."""
    vol = int(np.prod(W_DIMS))
    cells = np.random.default_rng(300).permutation(vol * W_BATCH)[:W_N]
    b, v = cells // vol, cells % vol
    coords = np.stack([v // (W_DIMS[1] * W_DIMS[2]), (v // W_DIMS[2]) % W_DIMS[1], v % W_DIMS[2], b], 1).astype(np.int32)
    by_logit = R.masks(W_N)['random']
    teacher = np.where(np.random.default_rng(8).random((W_BATCH,) + W_DIMS) < 0.4, 1.0, 0.5).astype(np.float32)
    by_teacher = R.dense_predicate(coords, teacher)
    assert 0 < by_logit.sum() < W_CAP and 0 < by_teacher.sum() < W_CAP and (by_logit != by_teacher).any()
    assert by_logit[256:].any() and by_teacher[256:].any()
    return dict(coords=coords, dev_coords=torch.from_numpy(coords).cuda(), logits=torch.from_numpy(_logits(by_logit)).cuda(),
                teacher=torch.from_numpy(teacher[:, None].copy()).cuda(), keep={False: by_logit, True: by_teacher})


@pytest.fixture
def compact_names(monkeypatch):
    """The sgnn_compact_* entry points called while the test runs; the calls go through unchanged."""
    log, real = [], L().call

    def spy(name, *args):
        if name.startswith('sgnn_compact'):
            log.append(name)
        return real(name, *args)
    monkeypatch.setattr(L(), 'call', spy)
    return log


def test_wrappers_compact_sigmoid_and_compact_mask(wrapper_case, compact_names):
    from sgnn_amd.scn import functions as F_
    c = wrapper_case
    want = np.nonzero(c['keep'][False])[0].astype(np.int32)
    sel, count = F_.compact_sigmoid(c['logits'], 2, W_N)
    assert count == len(want)
    R.assert_same_bits(sel.cpu().numpy(), want, 'compact_sigmoid')
    sel, count = F_.compact_mask(torch.from_numpy(c['keep'][False].astype(np.uint8)).cuda(), W_N)
    assert count == len(want)
    R.assert_same_bits(sel.cpu().numpy(), want, 'compact_mask')
    assert compact_names == ['sgnn_compact_sigmoid', 'sgnn_compact_mask']


@pytest.mark.parametrize('teacher', [False, True], ids=['logits', 'teacher'])
@pytest.mark.parametrize('chain', [True, False], ids=['chain', 'one_level'])
def test_wrapper_compact_sigmoid_plan(wrapper_case, compact_names, monkeypatch, chain, teacher):
    from sgnn_amd.scn import functions as F_, metadata as MD
    from sgnn_amd.scn.sites import info
    monkeypatch.setattr(MD, 'CHAIN', chain)
    c = wrapper_case
    want = np.nonzero(c['keep'][teacher])[0].astype(np.int32)
    what = 'compact_sigmoid_plan chain=%s teacher=%s' % (chain, teacher)
    sel, count, locs = F_.compact_sigmoid_plan(c['logits'], 2, W_N, c['dev_coords'], 1, c['teacher'] if teacher else None)
    assert count == len(want), what
    R.assert_same_bits(sel.cpu().numpy(), want, what + ' sel')
    R.assert_same_bits(locs.cpu().numpy(), c['coords'][want], what + ' locs')
    assert (info(locs).plan is not None) == chain, what
    assert compact_names == ['sgnn_compact_dense' if teacher else 'sgnn_compact_sigmoid'], what


@pytest.mark.parametrize('teacher', [False, True], ids=['logits', 'teacher'])
@pytest.mark.parametrize('fused', [True, False], ids=['locs', 'gather'])
def test_wrapper_compact_capped(wrapper_case, compact_names, monkeypatch, fused, teacher):
    """Capacity 512 >= the kept count: no overflow status; the counts stay on the device until the test reads them."""
    from sgnn_amd.scn import functions as F_, metadata as MD
    from sgnn_amd.scn.capacity import Capacity
    from sgnn_amd.scn.sites import info
    monkeypatch.setattr(F_, 'FUSED_GLUE', fused)
    c = wrapper_case
    want = np.nonzero(c['keep'][teacher])[0].astype(np.int32)
    what = 'compact_capped fused=%s teacher=%s' % (fused, teacher)
    cap = Capacity('cuda', 1024, [], [(W_CAP, [W_CAP, W_CAP])])
    rt = MD.runtime(torch.device('cuda', torch.cuda.current_device()))
    syncs = rt.syncs
    sel, K, locs = F_.compact_capped(c['logits'], 2, W_N, c['dev_coords'], 0, cap, 0, c['teacher'] if teacher else None)
    assert rt.syncs == syncs, what + ': capacity mode must not read anything back'
    assert K == W_CAP and tuple(sel.shape) == (W_N,) and tuple(locs.shape) == (W_CAP, 4) and locs.dtype == torch.int32
    assert cap.kept2(0).cpu().tolist() == [len(want), 8 * len(want)], what
    assert info(locs).cnt.data_ptr() == cap.kept2(0).data_ptr() and int(info(locs).cnt8.item()) == 8 * len(want)
    R.assert_same_bits(sel.cpu().numpy()[:len(want)], want, what + ' sel')
    R.assert_same_bits(locs.cpu().numpy()[:len(want)], c['coords'][want], what + ' locs')
    rt.check_status()
    assert compact_names == ['sgnn_compact_%s_cap%s' % ('dense' if teacher else 'sigmoid', '_locs' if fused else '')], what
