"""Host references for the kernels between the arithmetic layers: row movement and short sums (rows.hip), stream
compaction, coordinate conversion / expansion and the voxel hash (grid_rules.hip), and the flat Adam step (optim.hip).

Plain numpy, written from the definitions in the header comments of include/sgnn_hip.h; nothing here is derived from a
kernel and nothing is imported from sgnn_amd.  Three parts:
  * the references (one function per operation);
  * the comparison helpers: assert_same_bits compares bit patterns, guarded() wraps an output in sentinel guard
    elements and checks that they, and every element the operation must not write, survive;
  * the data the GPU tests run on (move_data, mixed_index, masks, sigmoid_ladder, adam_state ...), so that
    test_glue_ref.py can show on the very same data that a wrong kernel would be noticed.

Sums (gather_sum, sum_groups, add) are sequential np.float32 additions in ascending k / slice order starting from +0:
the kernels contain only additions in that order, nothing can contract, so the match is bit for bit on NaN-free data."""
import numpy as np

STATUS_COORD_RANGE, STATUS_DUPLICATE, STATUS_OVERFLOW = 1, 2, 4
SCAN_BLOCK = 2048                       # items per workgroup of the compaction (256 threads x 8)
SENT_BITS = 0x7FC5A5A5                  # float sentinel: a quiet NaN with a payload no data generator produces
SENT_INT = -7                           # integer sentinel


# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------
def bits(a):
    """The array as integers of the same width (float32 -> int32), so that NaN payloads and -0 compare."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %s %s, expected %s %s' % (
        what, got.dtype, got.shape, want.dtype, want.shape)
    diff = bits(got) != bits(want)
    if diff.any():
        d2 = diff.reshape(diff.shape[0], -1) if diff.ndim else diff.reshape(1, 1)
        r, c = np.argwhere(d2)[0]
        g, w = bits(got).reshape(d2.shape)[r, c], bits(want).reshape(d2.shape)[r, c]
        raise AssertionError('%s: %d of %d elements differ, first at (row %d, column %d): got 0x%x, expected 0x%x' % (
            what, int(diff.sum()), diff.size, r, c, int(g) & 0xFFFFFFFFFFFFFFFF, int(w) & 0xFFFFFFFFFFFFFFFF))


def sentinel(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([SENT_BITS], np.uint32).view(np.float32)[0]
    if dtype == np.uint8:
        return np.uint8(0xA5)
    return dtype.type(SENT_INT)


class Guarded:
    """A flat buffer of sentinels: `lead` guard elements, the array, `tail` guard elements.  The array starts 256 bytes
    (+ shift elements) into the buffer, so shift = 1 on float data places it 4 bytes off 16-byte alignment."""
    GUARD = 64

    def __init__(self, shape, dtype, shift=0):
        self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        self.size = int(np.prod(self.shape)) if self.shape else 1
        self.lead = (256 // self.dtype.itemsize) + shift
        self.full = np.full(self.lead + self.size + self.GUARD, sentinel(dtype), self.dtype)

    @property
    def offset_bytes(self):
        return self.lead * self.dtype.itemsize

    def inner(self, full):
        return np.asarray(full)[self.lead:self.lead + self.size].reshape(self.shape)

    def check(self, full, what, untouched=None):
        """Guards intact, and so is every element of `untouched` (boolean, broadcast over the array).  Returns the array."""
        full = np.asarray(full)
        assert full.shape == self.full.shape and full.dtype == self.dtype, what
        s = bits(np.array([sentinel(self.dtype)]))[0]
        b = bits(full)
        assert (b[:self.lead] == s).all(), '%s: wrote in front of the buffer' % what
        assert (b[self.lead + self.size:] == s).all(), '%s: wrote past the end of the buffer' % what
        arr = self.inner(full)
        if untouched is not None:
            u = np.broadcast_to(untouched, self.shape)
            bad = u & (bits(arr) != s)
            assert not bad.any(), '%s: %d elements that must stay untouched were written, first at %s' % (
                what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
        return arr


def guarded(shape, dtype, shift=0):
    return Guarded(shape, dtype, shift)


def unwritten(arr):
    """Boolean: elements that still hold the sentinel."""
    return bits(arr) == bits(np.array([sentinel(arr.dtype)]))[0]


# ---------------------------------------------------------------------------
# row movement
# ---------------------------------------------------------------------------
def _rows_of(idx, m):
    return np.arange(m, dtype=np.int64) if idx is None else np.asarray(idx[:m], np.int64)


def gather(src, idx, m=None):
    """dst[r] = src[idx[r]], zeros where idx[r] < 0."""
    m = len(idx) if m is None else m
    src = np.asarray(src)
    dst = np.zeros((m,) + src.shape[1:], src.dtype)
    i = np.asarray(idx[:m], np.int64)
    dst[i >= 0] = src[i[i >= 0]]
    return dst


def scatter(src, idx, n_dst, live=None):
    """dst (n_dst rows of zeros); dst[idx[r]] = src[r] for r < live, idx[r] >= 0 (idx unique)."""
    src = np.asarray(src)
    m = len(idx) if live is None else int(min(max(live, 0), len(idx)))
    dst = np.zeros((n_dst,) + src.shape[1:], src.dtype)
    i = np.asarray(idx[:m], np.int64)
    dst[i[i >= 0]] = src[:m][i >= 0]
    return dst


def repeat(src, rep):
    """dst[r * rep + t] = src[r]."""
    src = np.asarray(src)
    return src[np.arange(src.shape[0] * rep) // rep]


def concat(parts, m):
    """parts: (src (rows, c) or None when c == 0, c, idx or None).  dst[r] = [part[idx ? idx[r] : r] ...], zeros for idx < 0."""
    ctot = sum(c for _, c, _ in parts)
    dst = np.zeros((m, ctot), np.float32)
    off = 0
    for src, c, idx in parts:
        if c > 0:
            i = _rows_of(idx, m)
            ok = i >= 0
            dst[ok, off:off + c] = np.asarray(src)[i[ok]]
        off += c
    return dst


def concat_bwd(ddst, parts, m):
    """Adjoint of concat.  parts: (c, idx or None, n rows, present).  Per part (values, written): NULL (absent or c == 0)
    destinations give (None, None); a destination reached through an index array is zero-filled (all n rows written);
    a direct one gets rows < m only."""
    out, off = [], 0
    for c, idx, n, present in parts:
        if not present or c == 0:
            out.append((None, None))
        else:
            val = np.zeros((n, c), np.float32)
            written = np.zeros((n, c), bool)
            if idx is not None:
                written[:] = True
            i = _rows_of(idx, m)
            ok = i >= 0
            val[i[ok]] = ddst[:m][ok, off:off + c]
            written[i[ok]] = True
            out.append((val, written))
        off += c
    return out


def sparse_to_dense(feats, coords, batch, dims):
    """dense (B, C, d0, d1, d2) of zeros; dense[b, :, z, y, x] = feats[r] at coords[r] = (z, y, x, b) inside the volume."""
    c = feats.shape[1]
    dense = np.zeros((batch, c) + tuple(dims), np.float32)
    for r, (z, y, x, b) in enumerate(np.asarray(coords).tolist()):
        if 0 <= z < dims[0] and 0 <= y < dims[1] and 0 <= x < dims[2] and 0 <= b < batch:
            dense[b, :, z, y, x] = feats[r]
    return dense


def dense_to_sparse(dense, coords):
    batch, c, d0, d1, d2 = dense.shape
    feats = np.zeros((len(coords), c), np.float32)
    for r, (z, y, x, b) in enumerate(np.asarray(coords).tolist()):
        if 0 <= z < d0 and 0 <= y < d1 and 0 <= x < d2 and 0 <= b < batch:
            feats[r] = dense[b, :, z, y, x]
    return feats


def copy_multi(mem, regions):
    """mem: uint8 array; regions: (dst offset, src offset, bytes), non-overlapping.  Returns the memory afterwards."""
    out = mem.copy()
    for d, s, nb in regions:
        out[d:d + nb] = mem[s:s + nb]
    return out


# ---------------------------------------------------------------------------
# sums: sequential float32, ascending order, from +0
# ---------------------------------------------------------------------------
def gather_sum(src, table, n_out):
    """dst[j] = sum_k src[table[k, j]] over entries >= 0; table is (K, ld), ld >= n_out."""
    src = np.asarray(src, np.float32)
    acc = np.zeros((n_out, src.shape[1]), np.float32)
    for k in range(table.shape[0]):
        i = np.asarray(table[k, :n_out], np.int64)
        ok = i >= 0
        acc[ok] = acc[ok] + src[i[ok]]
    return acc


def sum_groups(src, n, rep):
    """dst[r] = sum_t src[r * rep + t]."""
    src = np.asarray(src, np.float32).reshape(n, rep, -1)
    acc = np.zeros((n, src.shape[2]), np.float32)
    for t in range(rep):
        acc = acc + src[:, t]
    return acc


def add(a, b):
    return np.asarray(a, np.float32) + np.asarray(b, np.float32)


# ---------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------
def live_count(n, n_dev):
    return n if n_dev is None else int(min(max(n_dev, 0), n))


def compaction(pred, n_dev=None, keep_cap=None):
    """Stable compaction of the first clamp(n_dev, 0, n) candidates: sel = ascending kept rows (all `total` of them),
    count = total clamped to keep_cap, count_mul = 8 * count, overflow iff total > keep_cap."""
    pred = np.asarray(pred, bool)
    sel = np.nonzero(pred[:live_count(len(pred), n_dev)])[0].astype(np.int32)
    total = len(sel)
    count = total if keep_cap is None else min(total, keep_cap)
    return dict(sel=sel, total=total, count=count, count_mul=8 * count,
                overflow=keep_cap is not None and total > keep_cap)


def assert_compaction(sel, counts, ref, what):
    """sel: the whole output buffer as it came back (sentinel where nothing was written); counts: [total] of the plain
    forms or [count, count_mul] of the capacity forms."""
    total = ref['total']
    assert unwritten(sel[total:]).all(), '%s: sel was written past the %d kept rows' % (what, total)
    assert_same_bits(sel[:total], ref['sel'], what + ' sel')
    want = [total] if len(counts) == 1 else [ref['count'], ref['count_mul']]
    assert [int(c) for c in counts] == want, '%s: counts %s, expected %s' % (what, list(counts), want)


def dense_predicate(coords, vol):
    """Keep site (z, y, x, b) iff it lies inside the (B, d0, d1, d2) volume and the volume is > 0.5 there."""
    batch, d0, d1, d2 = vol.shape
    c = np.asarray(coords, np.int64)
    inside = (c[:, 0] >= 0) & (c[:, 0] < d0) & (c[:, 1] >= 0) & (c[:, 1] < d1) & (c[:, 2] >= 0) & (c[:, 2] < d2) & \
        (c[:, 3] >= 0) & (c[:, 3] < batch)
    keep = np.zeros(len(c), bool)
    ci = c[inside]
    keep[inside] = vol[ci[:, 3], ci[:, 0], ci[:, 1], ci[:, 2]] > 0.5
    return keep


def sigmoid_rule(x):
    """What sigmoid(x) > 0.5 must answer wherever float32 rounding cannot matter: (must_keep, must_drop).  x <= 0 and NaN
    are dropped (sigmoid <= 1/2 exactly), x >= 2^-20 is kept (sigmoid(x) - 1/2 ~ x / 4 >= 4 ulp of 1/2); the band in
    between belongs to the rounding of expf, the addition and the division."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid='ignore'):
        return x >= np.float32(2.0 ** -20), ~(x > 0)


# ---------------------------------------------------------------------------
# coordinates and hash
# ---------------------------------------------------------------------------
def expand8(coords):
    """Children of (z, y, x, b): row 8 i + j = (2z + (j >> 2), 2y + ((j >> 1) & 1), 2x + (j & 1), b)."""
    c = np.asarray(coords, np.int32)
    out = np.empty((len(c) * 8, 4), np.int32)
    for j in range(8):
        out[j::8, 0] = 2 * c[:, 0] + (j >> 2)
        out[j::8, 1] = 2 * c[:, 1] + ((j >> 1) & 1)
        out[j::8, 2] = 2 * c[:, 2] + (j & 1)
        out[j::8, 3] = c[:, 3]
    return out


def dense_coords(batch, d0, d1, d2):
    """Every voxel of a (B, d0, d1, d2) volume, batch-major raster order, as (z, y, x, b)."""
    return np.array([(z, y, x, b) for b in range(batch) for z in range(d0) for y in range(d1) for x in range(d2)],
                    np.int32).reshape(-1, 4)


COORD_MAX = (65535, 65535, 65535, 32767)


def coords_from_i64(locs, n_dev=None):
    """(int32 rows, range flag): the flag is raised iff a live row has z, y, x outside [0, 65535] or b outside [0, 32767]."""
    locs = np.asarray(locs, np.int64)
    live = locs[:live_count(len(locs), n_dev)]
    bad = bool(((live < 0) | (live > np.array(COORD_MAX, np.int64))).any())
    return live.astype(np.int32), bad


def coords_to_i64(coords):
    return np.asarray(coords, np.int32).astype(np.int64)


def hash_rows(sites, queries):
    """Row of each query site in `sites` (first occurrence), -1 if absent or outside the coordinate range."""
    table = {}
    for r, s in enumerate(map(tuple, np.asarray(sites).tolist())):
        table.setdefault(s, r)
    out = np.empty(len(queries), np.int32)
    for r, q in enumerate(map(tuple, np.asarray(queries).tolist())):
        ok = all(0 <= v <= hi for v, hi in zip(q, COORD_MAX))
        out[r] = table.get(q, -1) if ok else -1
    return out


def has_duplicates(sites):
    s = np.asarray(sites)
    return len(np.unique(s, axis=0)) < len(s)


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
def segment_active(cnt, flag):
    """A segment is updated iff it was reached: the flag (> 0) decides when there is one, else the row count (> 0),
    else always."""
    if flag is not None:
        return flag > 0
    if cnt is not None:
        return cnt > 0
    return True


def status_blocks(status):
    """Nothing is updated while the status word carries the overflow bit."""
    return status is not None and bool(status & STATUS_OVERFLOW)


def adam_step(p, g, m, v, segs, steps, active, lr, beta1, beta2, eps, weight_decay, grad_scale, status=None):
    """One torch.optim.Adam step (amsgrad off, weight_decay added to the gradient) in float64 from float32 inputs; the
    gradient is scaled by grad_scale first.  segs: [begin, end) ranges, steps: updates each has seen, active: reached.
    Hyper-parameters are taken at their float32 values (what crosses the C interface).  Returns p, m, v (float64),
    the new step counters, the boolean mask of updated elements and U (the update with absolute values)."""
    f = lambda x: float(np.float32(x))
    lr, beta1, beta2, eps, weight_decay, grad_scale = map(f, (lr, beta1, beta2, eps, weight_decay, grad_scale))
    p64, g64, m64, v64 = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    upd = np.zeros(len(p64), bool)
    U = np.zeros(len(p64))
    steps_out = [float(s) for s in steps]
    if status_blocks(status):
        return p64, m64, v64, steps_out, upd, U
    for t, (b, e) in enumerate(segs):
        if not active[t]:
            continue
        step = steps[t] + 1.0
        steps_out[t] = step
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        gp = g64[b:e] * grad_scale + weight_decay * p64[b:e]
        m0 = m64[b:e].copy()
        m64[b:e] = m0 + (gp - m0) * (1.0 - beta1)
        v64[b:e] = beta2 * v64[b:e] + (1.0 - beta2) * gp * gp
        denom = np.sqrt(v64[b:e]) / np.sqrt(bc2) + eps
        p64[b:e] = p64[b:e] - (lr / bc1) * m64[b:e] / denom
        U[b:e] = lr * (np.abs(m0) + np.abs(gp)) / (bc1 * denom)
        upd[b:e] = True
    return p64, m64, v64, steps_out, upd, U


def ulps(got32, want64):
    """|got - want| in units of the float32 spacing at |want|."""
    want32 = np.abs(want64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - want64) / np.spacing(np.maximum(want32, np.finfo(np.float32).tiny)).astype(np.float64)


ADAM_MV_ULPS = 4.0
ADAM_P_ROUNDINGS = 32.0


def adam_p_ratio(p32, p64, U):
    """|p - p64| / (2^-24 |p64| + 32 * 2^-24 * U) per element."""
    bound = 2.0 ** -24 * np.abs(p64) + ADAM_P_ROUNDINGS * 2.0 ** -24 * U
    return np.abs(p32.astype(np.float64) - p64) / np.maximum(bound, np.finfo(np.float64).tiny)


def assert_adam(p32, m32, v32, ref, before, what):
    """The comparison rules of the Adam test on one step: updated elements within the bars, all others bit-identical to
    `before` = (p, m, v).  Returns the largest p ratio."""
    p64, m64, v64, _, upd, U = ref
    for name, got, b in zip('pmv', (p32, m32, v32), before):
        assert_same_bits(got[~upd], b[~upd], '%s: %s outside the active segments' % (what, name))
    if not upd.any():
        return 0.0
    um, uv = ulps(m32[upd], m64[upd]).max(), ulps(v32[upd], v64[upd]).max()
    ratio = adam_p_ratio(p32[upd], p64[upd], U[upd]).max()
    print('%s: m %.2f ulp, v %.2f ulp, p ratio %.3f' % (what, um, uv, ratio))
    assert um <= ADAM_MV_ULPS, '%s: exp_avg is %.2f ulp from the float64 step' % (what, um)
    assert uv <= ADAM_MV_ULPS, '%s: exp_avg_sq is %.2f ulp from the float64 step' % (what, uv)
    assert ratio <= 1.0, '%s: |p - p64| is %.3f of its bound' % (what, ratio)
    return float(ratio)


# ---------------------------------------------------------------------------
# data of the GPU tests
# ---------------------------------------------------------------------------
def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


SPECIAL_BITS = (0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x00000001, 0x807FFFFF)


def move_data(tag, n, c, specials=True):
    """(n, c) float32 of distinct bit patterns: a counter of (tag, row, column), every 7th element replaced by -0, an
    infinity, a NaN with a payload or a denormal (small integers viewed as float, as int32 coordinates are)."""
    assert 0 <= tag < 8 and n < (1 << 19) and c < (1 << 7)
    r, k = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(c, dtype=np.uint32), indexing='ij')
    b = ((np.uint32(tag + 1) << 26) | (r << 7) | k).astype(np.uint32)
    if specials:
        flat = (r * np.uint32(c) + k)
        pick = flat % 7 == 3
        sp = np.array(SPECIAL_BITS, np.uint32)[(flat // 7) % len(SPECIAL_BITS)]
        small = ((flat * np.uint32(2654435761)) >> 12) & np.uint32(0xFFFF) | np.uint32(1)      # denormals: coordinates
        sp = np.where((flat // 7) % 3 == 2, small, sp)
        b = np.where(pick, sp, b).astype(np.uint32)
    return b.view(np.float32).reshape(n, c)


def int_data(key, shape, lim=3):
    return _rng('int', key).integers(-lim, lim + 1, shape).astype(np.float32)


def real_data(key, shape):
    return _rng('real', key).standard_normal(shape).astype(np.float32)


def mixed_index(key, m, n_src):
    """m indices into n_src rows: valid rows, -1, the first and the last source row."""
    rng = _rng('idx', key, m, n_src)
    idx = rng.integers(0, n_src, m).astype(np.int32)
    idx[rng.random(m) < 0.2] = -1
    if m >= 4:
        idx[0], idx[1], idx[m // 2] = -1, 0, 0
    idx[m - 1] = n_src - 1
    return idx


def unique_index(key, m, n_dst):
    """m distinct indices into n_dst >= m rows with some -1, the first and the last destination row among them."""
    assert n_dst >= m
    rng = _rng('uniq', key, m, n_dst)
    idx = rng.permutation(n_dst)[:m].astype(np.int32)
    if m >= 4:
        idx[rng.random(m) < 0.15] = -1
        idx[0] = -1
        for want, at in ((0, 1), (n_dst - 1, m - 1)):
            idx[idx == want] = -1
            idx[at] = want
    return idx


COMPACT_SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4096, 9000)


def masks(n):
    """name -> boolean keep mask of n candidates."""
    rng = _rng('mask', n)
    out = {'none': np.zeros(n, bool), 'all': np.ones(n, bool), 'alternating': np.arange(n) % 2 == 0,
           'first': np.arange(n) == 0, 'last': np.arange(n) == n - 1, 'random': rng.random(n) < 0.3}
    nblk = -(-n // SCAN_BLOCK)
    if nblk >= 3:                       # one whole workgroup's 2048 items empty in the middle
        hole = rng.random(n) < 0.5
        hole[(nblk // 2) * SCAN_BLOCK:(nblk // 2 + 1) * SCAN_BLOCK] = False
        out['hole'] = hole
    return out


def sigmoid_ladder():
    """Logits around the threshold of sigmoid(x) > 0.5: +-0, infinities, NaN, huge values, denormals, and per binade of
    +-2^-30 .. +-2^-18 the power of two, its two neighbours on either side and 64 evenly spaced mantissas."""
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, 100.0, -100.0, 1e38, -1e38]
    pos = [np.array([1, 2, 0x7FFFFF], np.uint32).view(np.float32)]          # denormals
    for e in range(-30, -17):
        b = np.array([2.0 ** e], np.float32).view(np.uint32)[0]
        pos.append((b + np.arange(-2, 3, dtype=np.int64)).astype(np.uint32).view(np.float32))
        if e < -18:
            pos.append((b + (np.arange(1, 64, dtype=np.int64) << 17)).astype(np.uint32).view(np.float32))
    pos = np.unique(np.concatenate(pos))
    return np.concatenate([np.array(vals, np.float32), pos, -pos]).astype(np.float32)


def range_cases():
    """(name, column, value): each of the eight bounds of the int64 -> int32 coordinate conversion violated alone."""
    out = []
    for col, (name, hi) in enumerate(zip('zyxb', COORD_MAX)):
        out += [('%s<0' % name, col, -1), ('%s>%d' % (name, hi), col, hi + 1)]
    return out


def clean_locs(key, n):
    """n int64 (z, y, x, b) rows inside the range, the extreme corners among them."""
    rng = _rng('locs', key, n)
    locs = np.stack([rng.integers(0, hi + 1, n) for hi in COORD_MAX], 1).astype(np.int64)
    locs[0] = COORD_MAX
    if n > 1:
        locs[n - 1] = 0
    return locs


def random_sites(key, n, side=40, batch=2):
    """n distinct int32 sites of a side^3 x batch volume, in random order."""
    cells = _rng('sites', key, n).permutation(side ** 3 * batch)[:n]
    b, v = cells // side ** 3, cells % side ** 3
    return np.stack([v // (side * side), (v // side) % side, v % side, b], 1).astype(np.int32)


def adam_segments(n):
    """[0,5) [5,6) [7,1030) [1030,n): boundaries off multiples of 4, a one-element segment, element 6 in no segment."""
    return [(0, 5), (5, 6), (7, 1030), (1030, n)]


ADAM_STEPS = (0, 1, 9, 999, 100000)


def adam_state(key, n):
    """p, g, m, v of a running optimisation: gradient, momentum and parameter of one sign per element (the momentum is an
    average of past gradients; with weight decay the decayed gradient keeps its sign), so that no sum on the path
    cancels and the ulp bars on m and v measure the kernel's roundings, not the data's condition."""
    rng = _rng('adam', key, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mag = lambda lo, hi: np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    g = (sign * mag(1e-3, 10.0)).astype(np.float32)
    m = (sign * mag(1e-3, 10.0)).astype(np.float32)
    p = (sign * mag(1e-2, 5.0)).astype(np.float32)
    v = (mag(1e-6, 100.0)).astype(np.float32)
    return p, g, m, v


# ---------------------------------------------------------------------------
# device side of guarded(): the only place that touches torch (imported late: the references above are numpy alone)
# ---------------------------------------------------------------------------
class DeviceBuf:
    """guarded(shape, dtype, shift) on the GPU.  With `data` the array holds it (an input at a chosen alignment);
    without, it holds the sentinel (an output).  .ptr is the device address of the array itself."""

    def __init__(self, shape, dtype, shift=0, data=None):
        import torch
        self.g = Guarded(shape, dtype, shift)
        if data is not None:
            self.g.inner(self.g.full)[...] = data
        self.t = torch.from_numpy(self.g.full).cuda()
        self.ptr = self.t.data_ptr() + self.g.offset_bytes
        assert self.t.data_ptr() % 256 == 0

    def host(self):
        return self.t.cpu().numpy()

    def check(self, what, untouched=None):
        return self.g.check(self.host(), what, untouched)


def dev_in(a, shift=0):
    a = np.ascontiguousarray(a)
    return DeviceBuf(a.shape, a.dtype, shift, a)


def dev_out(shape, dtype=np.float32, shift=0):
    return DeviceBuf(shape, dtype, shift)
