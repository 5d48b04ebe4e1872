"""Every exported row kernel of rows.hip against the host references of tests/glue_ref.py, bit for bit.

Which set-up reaches which kernel (the entry points are called through sgnn_amd._lib.call, as scn/functions.py does):
  sgnn_gather_rows / _dn, sgnn_scatter_rows, sgnn_gather_sum, sgnn_repeat_rows, sgnn_sum_groups
      c % 4 == 0 and 16-byte aligned bases -> the <4> (float4) instantiation; any other width, or shift = 1 (every
      float pointer 4 bytes off alignment) -> the <1> instantiation.  WIDTHS holds both kinds.
  sgnn_concat3_rows / _bwd   total width <= 32 -> k_concat3_rg<8> / k_concat3_bwd_rg<8>; <= 64 -> <16>; above -> the
      element-per-thread k_concat3 / k_concat3_bwd (CAT3 lists widths per form).
  sgnn_concat_rows / _bwd    k_concat_rows / k_concat_rows_bwd (one form); index-reached gradients also run k_fill32_multi.
  sgnn_add                   aligned -> float4 body + scalar tail (counts around multiples of 4); shift = 1 -> scalar form.
  sgnn_copy_multi            regions 16-byte aligned on both sides -> 16-byte units + byte tail, else the byte path.
  sgnn_sparse_to_dense / sgnn_dense_to_sparse   one kernel each; the zero fill of the dense volume is k_fill32_multi with
      its scalar tail when the word count is no multiple of 4.
  BIG cases: one per kernel whose work exceeds the block cap of its sgnn_grid_for call x 256 threads, so that the
      grid-stride loop makes a second, ragged trip.

Pure-move kernels carry distinct bit patterns (glue_ref.move_data: a (source, row, column) counter mixed with -0,
denormals, infinities and NaN payloads) and are compared as int32.  The summing kernels run on integers in {-3..3} and on
NaN-free real data; both must equal the sequential float32 reference bit for bit.  Every output lies in a sentinel
buffer with guard elements on either side; rows the operation must not write must still hold the sentinel."""
import itertools

import numpy as np
import pytest

import glue_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 8, 12, 16, 26, 30, 48)
ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 4097)
SHIFT_WIDTHS, SHIFT_ROWS = (4, 16), (65, 257)           # the misaligned cases: widths that would otherwise take float4


def call(name, *args):
    from sgnn_amd import _lib as L
    L.call(name, *args)


def _sizes(shift):
    return list(itertools.product(SHIFT_WIDTHS, SHIFT_ROWS)) if shift else list(itertools.product(WIDTHS, ROWS))


def _i32(a):
    return R.dev_in(np.asarray(a, np.int32))


def _i64(v):
    return R.dev_in(np.array([v], np.int64))


def _ptr(b):
    return None if b is None else b.ptr


# ---- gather / scatter ----

def _gather(c, m, n_src, shift, what):
    src, idx = R.move_data(0, n_src, c), R.mixed_index(what, m, n_src)
    s, i, d = R.dev_in(src, shift), _i32(idx), R.dev_out((m, c), np.float32, shift)
    call('sgnn_gather_rows', s.ptr, c, i.ptr, m, d.ptr)
    R.assert_same_bits(d.check(what), R.gather(src, idx), what)


@pytest.mark.parametrize('shift', [0, 1])
def test_gather_rows(shift):
    for c, m in _sizes(shift):
        _gather(c, m, max(2, m // 2 + 3), shift, 'gather_rows c=%d m=%d shift=%d' % (c, m, shift))


def test_gather_rows_second_trip():
    _gather(16, 262144 + 77, 1000, 0, 'gather_rows c=16 m=262221')      # 4096 blocks x 256 threads = 262 144 rows of 4 float4


def test_gather_rows_copies_int32_coordinates_bit_for_bit():
    """gather_coords uses the kernel on (n, 4) int32 rows: small integers are denormal floats and must survive."""
    rng = np.random.default_rng(3)
    coords = rng.integers(0, 300, (777, 4)).astype(np.int32)
    coords[5] = (65535, 0, 1, 32767)
    idx = R.mixed_index('coords', 500, 777)
    s, i, d = R.dev_in(coords), _i32(idx), R.dev_out((500, 4), np.int32)
    call('sgnn_gather_rows', s.ptr, 4, i.ptr, 500, d.ptr)
    R.assert_same_bits(d.check('coords'), R.gather(coords, idx), 'gather_rows on int32 coordinates')


def _live_counts(m):
    return (0, 1, m - 1, m, m + 5, -3)


def _gather_dn(c, m, live, shift, what, n_src=None):
    n_src = n_src or max(2, m // 2 + 3)
    src, idx = R.move_data(1, n_src, c), R.mixed_index(what, m, n_src)
    s, i, n, d = R.dev_in(src, shift), _i32(idx), _i64(live), R.dev_out((m, c), np.float32, shift)
    call('sgnn_gather_rows_dn', s.ptr, c, i.ptr, n.ptr, m, d.ptr)
    k = R.live_count(m, live)
    got = d.check(what, untouched=(np.arange(m) >= k)[:, None])
    R.assert_same_bits(got[:k], R.gather(src, idx, k), what)


@pytest.mark.parametrize('shift', [0, 1])
def test_gather_rows_dn(shift):
    for c, m in ((c, m) for c in ((4, 16) if shift else (1, 5, 12, 16)) for m in (65, 257, 1023)):
        for live in _live_counts(m):
            _gather_dn(c, m, live, shift, 'gather_rows_dn c=%d m=%d live=%d shift=%d' % (c, m, live, shift))
    if not shift:
        for c, m in _sizes(0):
            _gather_dn(c, m, m, 0, 'gather_rows_dn c=%d m=%d' % (c, m))


def test_gather_rows_dn_second_trip():
    _gather_dn(16, 262144 + 77, 262144 + 70, 0, 'gather_rows_dn c=16 m=262221', n_src=1000)


def _scatter(c, m, live, shift, what):
    n_dst = m + 9
    src, idx = R.move_data(2, m, c), R.unique_index(what, m, n_dst)
    s, i, d = R.dev_in(src, shift), _i32(idx), R.dev_out((n_dst, c), np.float32, shift)
    n = None if live is None else _i64(live)
    call('sgnn_scatter_rows', s.ptr, c, i.ptr, m, d.ptr, n_dst, _ptr(n))
    R.assert_same_bits(d.check(what), R.scatter(src, idx, n_dst, live), what)     # rows past the live count stay zero


@pytest.mark.parametrize('shift', [0, 1])
def test_scatter_rows(shift):
    for c, m in _sizes(shift):
        _scatter(c, m, None, shift, 'scatter_rows c=%d m=%d shift=%d' % (c, m, shift))
    for c, m in ((c, m) for c in ((4, 16) if shift else (1, 5, 12, 16)) for m in (65, 257, 1023)):
        for live in _live_counts(m):
            _scatter(c, m, live, shift, 'scatter_rows c=%d m=%d live=%d shift=%d' % (c, m, live, shift))


def test_scatter_rows_second_trip():
    _scatter(16, 262144 + 77, None, 0, 'scatter_rows c=16 m=262221')


# ---- sums ----

def _sum_data(integer, key, shape):
    return R.int_data(key, shape) if integer else R.real_data(key, shape)


def _gather_sum(c, n_out, K, integer, shift, what, n_src=None, all_empty_column=True):
    n_src = n_src or max(2, n_out // 2 + 3)
    ld = n_out + 5
    src = _sum_data(integer, what, (n_src, c))
    rng = np.random.default_rng(n_out * 31 + K)
    table = rng.integers(0, n_src, (K, ld)).astype(np.int32)
    table[rng.random((K, ld)) < 0.3] = -1
    if all_empty_column:
        table[:, n_out // 2] = -1                      # an output row with no valid entry: +0
    table[0, n_out - 1], table[K - 1, 0] = n_src - 1, 0
    s, t, d = R.dev_in(src, shift), _i32(table), R.dev_out((n_out, c), np.float32, shift)
    call('sgnn_gather_sum', s.ptr, c, t.ptr, ld, K, n_out, d.ptr)
    R.assert_same_bits(d.check(what), R.gather_sum(src, table, n_out), what)


@pytest.mark.parametrize('integer', [True, False])
@pytest.mark.parametrize('shift', [0, 1])
def test_gather_sum(shift, integer):
    for K in (1, 8, 27):
        for c, m in _sizes(shift):
            if K == 8 or m in (1, 65, 257) or shift:
                _gather_sum(c, m, K, integer, shift, 'gather_sum c=%d n=%d K=%d int=%d shift=%d' % (c, m, K, integer, shift))


def test_gather_sum_second_trip():
    _gather_sum(16, 262144 + 77, 2, False, 0, 'gather_sum c=16 n=262221 K=2', n_src=1000)


def _repeat(c, n, rep, shift, what):
    src = R.move_data(3, n, c)
    s, d = R.dev_in(src, shift), R.dev_out((n * rep, c), np.float32, shift)
    call('sgnn_repeat_rows', s.ptr, c, n, rep, d.ptr)
    R.assert_same_bits(d.check(what), R.repeat(src, rep), what)


@pytest.mark.parametrize('shift', [0, 1])
def test_repeat_rows(shift):
    for rep in (1, 8):
        for c, m in _sizes(shift):
            _repeat(c, m, rep, shift, 'repeat_rows c=%d n=%d rep=%d shift=%d' % (c, m, rep, shift))


def test_repeat_rows_second_trip():
    _repeat(16, 32768 + 9, 8, 0, 'repeat_rows c=16 n=32777 rep=8')       # 32 777 x 8 rows x 4 float4 > 4096 x 256


def _sum_groups(c, n, rep, integer, shift, what):
    src = _sum_data(integer, what, (n * rep, c))
    s, d = R.dev_in(src, shift), R.dev_out((n, c), np.float32, shift)
    call('sgnn_sum_groups', s.ptr, c, n, rep, d.ptr)
    R.assert_same_bits(d.check(what), R.sum_groups(src, n, rep), what)


@pytest.mark.parametrize('integer', [True, False])
@pytest.mark.parametrize('shift', [0, 1])
def test_sum_groups(shift, integer):
    for rep in (1, 2, 3, 4, 5, 8, 16, 27):           # the 4-way unrolled body and its remainder of 0..3 slices
        for c, m in _sizes(shift):
            if rep == 5 or m in (1, 65, 257) or shift:
                _sum_groups(c, m, rep, integer, shift, 'sum_groups c=%d n=%d rep=%d int=%d shift=%d' % (c, m, rep, integer, shift))


def test_sum_groups_second_trip():
    _sum_groups(16, 262144 + 77, 2, False, 0, 'sum_groups c=16 n=262221 rep=2')


def _add(count, integer, shift, what):
    a, b = _sum_data(integer, what + 'a', (count,)), _sum_data(integer, what + 'b', (count,))
    da, db, y = R.dev_in(a, shift), R.dev_in(b, shift), R.dev_out((count,), np.float32, shift)
    call('sgnn_add', da.ptr, db.ptr, count, y.ptr)
    R.assert_same_bits(y.check(what), R.add(a, b), what)


@pytest.mark.parametrize('integer', [True, False])
@pytest.mark.parametrize('shift', [0, 1])
def test_add(shift, integer):
    for count in (1, 3, 4, 5, 1023, 1024, 1027):
        _add(count, integer, shift, 'add count=%d int=%d shift=%d' % (count, integer, shift))


def test_add_second_trip():
    _add(4 * 4096 * 256 + 7, False, 0, 'add count=4194311')           # float4 groups > 4096 x 256, and a 3-element tail


# ---- two-way concat and its adjoint ----

CAT2 = ((16, 2), (0, 5), (5, 0), (3, 4))


def _cat_parts(widths, use_idx, m, what):
    """Per source: (data or None, c, idx or None, rows)."""
    parts = []
    for w, (c, ui) in enumerate(zip(widths, use_idx)):
        n = max(2, m // 2 + 3) if ui else m + 3
        idx = R.mixed_index((what, w), m, n) if ui else None
        parts.append((R.move_data(w, n, c) if c else None, c, idx, n))
    return parts


def _concat(entry, widths, use_idx, m, what):
    parts = _cat_parts(widths, use_idx, m, what)
    bufs = [(R.dev_in(s) if c else None, _i32(i) if i is not None else None) for s, c, i, _ in parts]
    d = R.dev_out((m, sum(widths)))
    args = []
    for (s, c, i, _), (bs, bi) in zip(parts, bufs):
        args += [_ptr(bs), c, _ptr(bi)]
    call(entry, *args, m, d.ptr)
    R.assert_same_bits(d.check(what), R.concat([(s, c, i) for s, c, i, _ in parts], m), what)


def _concat_bwd(entry, widths, use_idx, present, m, what):
    ctot = sum(widths)
    ddst = R.move_data(7, m, ctot)
    parts = []
    for w, (c, ui, pr) in enumerate(zip(widths, use_idx, present)):
        n = m + 3                                                        # zero-filled regions are larger than m
        parts.append((c, R.unique_index((what, w), m, n) if ui else None, n, pr))
    g = R.dev_in(ddst)
    idx = [_i32(i) if i is not None else None for _, i, _, _ in parts]
    outs = [R.dev_out((n, c)) if (pr and c) else None for c, _, n, pr in parts]
    args = [g.ptr]
    for (c, _, _, _), bi in zip(parts, idx):
        args += [c, _ptr(bi)]
    args.append(m)
    for (_, _, n, _), o in zip(parts, outs):
        args += [_ptr(o), n]
    call(entry, *args)
    for w, ((val, written), o) in enumerate(zip(R.concat_bwd(ddst, parts, m), outs)):
        if o is None:
            continue
        got = o.check('%s: d%s' % (what, 'abc'[w]), untouched=~written)
        R.assert_same_bits(np.where(written, got, 0).astype(np.float32), val, '%s: d%s' % (what, 'abc'[w]))


def test_concat_rows():
    for widths in CAT2:
        for use_idx in itertools.product((False, True), repeat=2):
            for m in ROWS:
                _concat('sgnn_concat_rows', widths, use_idx, m, 'concat_rows %s idx=%s m=%d' % (widths, use_idx, m))


def test_concat_rows_bwd():
    for widths in CAT2:
        for use_idx in itertools.product((False, True), repeat=2):
            for k, present in enumerate(itertools.product((True, False), repeat=2)):
                for m in (ROWS if all(present) else ROWS[k::3]):
                    _concat_bwd('sgnn_concat_rows_bwd', widths, use_idx, present, m,
                                'concat_rows_bwd %s idx=%s dst=%s m=%d' % (widths, use_idx, present, m))


def test_concat_rows_second_trip():
    _concat('sgnn_concat_rows', (16, 2), (True, True), 58300, 'concat_rows (16,2) m=58300')      # 58 300 x 18 > 4096 x 256
    _concat_bwd('sgnn_concat_rows_bwd', (16, 2), (True, False), (True, True), 58300, 'concat_rows_bwd (16,2) m=58300')


# ---- three-way concat and its adjoint: the three kernel forms ----

CAT3 = {
    'rg8': ((1, 0, 0), (0, 1, 0), (0, 0, 1), (16, 2, 8), (5, 0, 21), (16, 2, 12), (0, 7, 23), (16, 8, 8), (13, 19, 0)),   # 1 26 30 32
    'rg16': ((16, 1, 16), (16, 2, 30), (0, 48, 0), (26, 30, 8), (31, 0, 33)),                                            # 33 48 64
    'element': ((16, 2, 47), (33, 32, 0), (0, 48, 32), (26, 30, 24)),                                                    # 65 80
}
CAT3_BIG = {'rg8': ((16, 2, 8), 262144 + 33), 'rg16': ((16, 2, 30), 131072 + 17), 'element': ((16, 2, 47), 16200)}


@pytest.mark.parametrize('form', list(CAT3))
def test_concat3_rows(form):
    k = 0
    for widths in CAT3[form]:
        assert {'rg8': sum(widths) <= 32, 'rg16': 32 < sum(widths) <= 64, 'element': sum(widths) > 64}[form]
        for use_idx in itertools.product((False, True), repeat=3):
            for m in ROWS[k % 3::3]:                      # every row count under every third combination
                _concat('sgnn_concat3_rows', widths, use_idx, m, 'concat3_rows %s idx=%s m=%d' % (widths, use_idx, m))
            k += 1


@pytest.mark.parametrize('form', list(CAT3))
def test_concat3_rows_bwd(form):
    k = 0
    for widths in CAT3[form]:
        for use_idx in itertools.product((False, True), repeat=3):
            for present in itertools.product((True, False), repeat=3):
                m = ROWS[k % len(ROWS)]
                _concat_bwd('sgnn_concat3_rows_bwd', widths, use_idx, present, m,
                            'concat3_rows_bwd %s idx=%s dst=%s m=%d' % (widths, use_idx, present, m))
                k += 1


@pytest.mark.parametrize('form', list(CAT3_BIG))
def test_concat3_second_trip(form):
    widths, m = CAT3_BIG[form]
    _concat('sgnn_concat3_rows', widths, (True, False, True), m, 'concat3_rows %s m=%d' % (widths, m))
    _concat_bwd('sgnn_concat3_rows_bwd', widths, (False, True, False), (True, True, True), m,
                'concat3_rows_bwd %s m=%d' % (widths, m))


# ---- multi-region copy ----

def _copy_multi(sizes, misaligned, same, what):
    """Regions laid out in one uint8 buffer, 64 guard bytes around each; region k is 1 byte off 16-byte alignment on the
    destination side if k is in `misaligned`; region `same` has dst == src."""
    rng = np.random.default_rng(len(sizes) * 7 + sum(sizes))
    lay, off = [], 256
    for k, nb in enumerate(sizes):
        s = off
        off = (s + nb + 64 + 15) // 16 * 16
        d = off + (1 if k in misaligned else 0)
        off = (d + nb + 64 + 15) // 16 * 16
        lay.append((s if k == same else d, s, nb))
    mem = np.full(off + 64, 0xA5, np.uint8)
    for d, s, nb in lay:
        mem[s:s + nb] = rng.integers(0, 256, nb, dtype=np.uint8)
    import torch
    t = torch.from_numpy(mem).cuda()
    base = t.data_ptr()
    assert base % 16 == 0
    n = len(lay)
    arr = lambda v: np.array(list(v) + [0], np.int64)              # host arrays (never empty)
    dst, src, nby = arr(base + d for d, _, _ in lay), arr(base + s for _, s, _ in lay), arr(nb for _, _, nb in lay)
    call('sgnn_copy_multi', dst.ctypes.data, src.ctypes.data, nby.ctypes.data, n)
    R.assert_same_bits(t.cpu().numpy(), R.copy_multi(mem, lay), what)        # guard bytes included


def test_copy_multi():
    sizes = (0, 1, 15, 16, 17, 4099, 16, 33)
    for n in range(0, 9):
        _copy_multi(sizes[:n], (), None, 'copy_multi %d aligned regions' % n)
        _copy_multi(sizes[::-1][:n], set(range(0, n, 2)), None, 'copy_multi %d regions, even ones misaligned' % n)
    _copy_multi(sizes, (1, 5), 3, 'copy_multi with a dst == src region')
    _copy_multi((4099,) * 8, (7,), 0, 'copy_multi 8 x 4099')


def test_copy_multi_second_trip():
    _copy_multi((16 * 8192 * 256 + 4099, 17), (), None, 'copy_multi 33 558 531 bytes')        # 16-byte units > 8192 x 256


# ---- sparse <-> dense ----

def _s2d_sites(key, n, batch, dims):
    """n sites: distinct voxels of the volume in random order, then some outside the volume and outside the batch."""
    rng = np.random.default_rng(key)
    vol = int(np.prod(dims))
    cells = rng.permutation(vol * batch)[:n]
    b, v = cells // vol, cells % vol
    coords = np.stack([v // (dims[1] * dims[2]), (v // dims[2]) % dims[1], v % dims[2], b], 1).astype(np.int32)
    out = np.array([(-1, 0, 0, 0), (dims[0], 0, 0, 0), (0, dims[1], 0, 1), (0, 0, -1, 0), (0, 0, dims[2], 1), (0, 0, 0, batch),
                    (1, 1, 1, -1), (0, -2, 0, 0)], np.int32)
    return np.concatenate([coords[:n // 2], out, coords[n // 2:]])


def _sparse_dense(c, batch, dims, n_in, what):
    coords = _s2d_sites(c + n_in, n_in, batch, dims)
    n = len(coords)
    feats = R.move_data(4, n, c)
    f, co, d = R.dev_in(feats), R.dev_in(coords), R.dev_out((batch, c) + dims)
    call('sgnn_sparse_to_dense', f.ptr, co.ptr, n, c, d.ptr, batch, *dims)
    dense = R.sparse_to_dense(feats, coords, batch, dims)
    R.assert_same_bits(d.check(what + ' to dense'), dense, what + ' to dense')
    vol = (np.arange(batch * c * int(np.prod(dims)), dtype=np.uint32) | np.uint32(6 << 26)).view(np.float32).reshape((batch, c) + dims)
    v, back = R.dev_in(vol), R.dev_out((n, c))
    call('sgnn_dense_to_sparse', v.ptr, co.ptr, n, c, back.ptr, batch, *dims)
    R.assert_same_bits(back.check(what + ' to sparse'), R.dense_to_sparse(vol, coords), what + ' to sparse')
    rt = R.dev_out((n, c))                                               # round trip of the first result
    call('sgnn_dense_to_sparse', d.ptr, co.ptr, n, c, rt.ptr, batch, *dims)
    inside = R.dense_predicate(coords, np.ones((batch,) + dims, np.float32))
    R.assert_same_bits(rt.check(what + ' round trip'), np.where(inside[:, None], feats, 0).astype(np.float32), what + ' round trip')


def test_sparse_dense():
    for c in (1, 3, 16):             # 2 x c x 105 words: 210 and 630 are no multiple of 4 (the fill's scalar tail)
        for n in (1, 100, 210):
            _sparse_dense(c, 2, (3, 5, 7), n, 'sparse/dense c=%d n=%d' % (c, n))


def test_sparse_dense_second_trip():
    _sparse_dense(16, 1, (41, 41, 41), 65536 + 5, 'sparse/dense c=16 n=65549')          # 65 549 x 16 > 4096 x 256
