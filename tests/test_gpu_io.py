"""GPU: the three decode kernels of io.hip (sgnn_io_flag_entries, sgnn_io_emit_entries, sgnn_io_scatter_dense) called
directly through the C ABI and compared with tests/io_ref.py.  Bit for bit: integer coordinates and one correctly
rounded float32 division, so no tolerance appears anywhere (NaN compares equal to NaN, everything else by its bits).

Every output sits between two sentinel-filled guard regions, and rows past the expected count are sentinel-filled
too; all of them must come back untouched.  The packed coordinates and values are uploaded to addresses that are
4-byte but not 16-byte aligned.  Each case asserts the property of its own input that makes it a test."""
import numpy as np
import pytest
import torch

import io_ref
from sgnn_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 256                               # elements on either side of every output
SENT_U8 = 0xA5
SENT_I64 = -0x5A5A5A5A5A5A5A5B
SENT_F32 = 0x7FA5A5A5                      # bit pattern (a NaN payload no division produces), held as int32
NOLIMIT = 1 << 40
CAP = 4096 * 256                          # threads of the largest launch: beyond it the grid-stride loops wrap
F32 = np.float32


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype != np.float32:
        assert np.array_equal(a, b)
        return
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])     # -0.0 is not +0.0 here


def seg_of(counts):
    seg = np.zeros(len(counts) + 1, dtype=np.int64)
    seg[1:] = np.cumsum(counts)
    return seg


def _misaligned(arr):
    """Device copy of `arr` at an address that is 4 (mod 16).  Returns (owner tensor, address)."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    owner = torch.empty(raw.size + 32, dtype=torch.uint8, device='cuda')
    assert owner.data_ptr() % 16 == 0
    if raw.size:
        owner[4:4 + raw.size].copy_(torch.from_numpy(raw.copy()))
    return owner, owner.data_ptr() + 4


class Batch(object):
    """A packed batch on the host (what io_ref reads) and on the device (what the kernels read)."""

    def __init__(self, locs_xyz, vals, voxelsize, seg):
        self.locs = np.ascontiguousarray(locs_xyz, dtype=np.uint32).reshape(-1, 3)
        self.vals = np.ascontiguousarray(vals, dtype=np.float32)
        self.vs = np.ascontiguousarray(voxelsize, dtype=np.float32)
        self.seg = np.ascontiguousarray(seg, dtype=np.int64)
        self.n, self.nb = len(self.vals), len(self.vs)
        assert len(self.locs) == self.n and len(self.seg) == self.nb + 1
        assert self.seg[0] == 0 and self.seg[-1] == self.n and np.all(np.diff(self.seg) >= 0)
        assert self.locs.max(initial=0) < 2 ** 31
        self._l, self.p_locs = _misaligned(self.locs)
        self._v, self.p_vals = _misaligned(self.vals)
        assert self.p_locs % 16 == 4 and self.p_vals % 16 == 4
        self._vs, self._seg = torch.from_numpy(self.vs).cuda(), torch.from_numpy(self.seg).cuda()
        self.p_vs, self.p_seg = self._vs.data_ptr(), self._seg.data_ptr()

    @property
    def host(self):
        return self.locs, self.vals, self.vs, self.seg

    def sample(self):
        return io_ref.sample_of(self.seg, self.n)


class Guarded(object):
    """n elements of `dtype` between two guard regions, everything filled with `sentinel`."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.full = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()
        assert self.ptr % 16 == 0

    @property
    def body(self):
        return self.full[GUARD:GUARD + self.n]

    def read(self):
        torch.cuda.synchronize()
        host = self.full.cpu().numpy()
        assert np.all(host[:GUARD] == self.sentinel), 'the guard in front of the output was written'
        assert np.all(host[GUARD + self.n:] == self.sentinel), 'the guard behind the output was written'
        return host[GUARD:GUARD + self.n]

    def untouched(self):
        return bool(np.all(self.read() == self.sentinel))


def run_flag(b, truncation, max_z):
    out = Guarded(b.n, torch.uint8, SENT_U8)
    _lib.call('sgnn_io_flag_entries', b.p_locs, b.p_vals, b.p_vs, b.p_seg, b.nb, b.n, float(truncation), max_z, out.ptr)
    mask = out.read()
    assert np.all(mask <= 1), 'an entry of the mask was not written, or holds something other than 0 / 1'
    return mask


def run_emit(b, mask):
    """Rows and features of the entries selected by `mask`; sel and *count come from the host, so the kernel is on
    its own.  The launch is sized by n_max = n, the loop by *count: rows past it must stay sentinel."""
    kept = np.nonzero(mask)[0]
    m = len(kept)
    sel = np.zeros(b.n, dtype=np.int32)          # zeros past m: even a kernel that read them would stay in bounds
    sel[:m] = kept
    sel_d, count_d = torch.from_numpy(sel).cuda(), torch.tensor([m], dtype=torch.int64, device='cuda')
    rows, feats = Guarded(4 * b.n, torch.int64, SENT_I64), Guarded(b.n, torch.int32, SENT_F32)
    _lib.call('sgnn_io_emit_entries', b.p_locs, b.p_vals, b.p_vs, b.p_seg, b.nb, sel_d.data_ptr(), count_d.data_ptr(),
              b.n, rows.ptr, feats.ptr)
    r, f = rows.read().reshape(b.n, 4), feats.read()
    assert np.all(r[m:] == SENT_I64), 'a row at or beyond *count was written'
    assert np.all(f[m:] == SENT_F32), 'a feature at or beyond *count was written'
    return r[:m].copy(), f[:m].copy().view(np.float32)


def run_scatter(b, dims, max_z):
    d0, d1, d2 = dims
    out = Guarded(b.nb * d0 * d1 * d2, torch.int32, SENT_F32)
    out.body.view(torch.float32).fill_(-float('inf'))
    _lib.call('sgnn_io_scatter_dense', b.p_locs, b.p_vals, b.p_vs, b.p_seg, b.nb, b.n, d0, d1, d2, max_z, out.ptr)
    return out.read().copy().view(np.float32).reshape(b.nb, d0, d1, d2)


def check_all(b, truncation, dims, max_z_flag=NOLIMIT, max_z_scatter=NOLIMIT, emit_all=True):
    """All three kernels on one batch against io_ref.  Returns the reference mask and dense volume."""
    mask = io_ref.flag(*b.host, truncation, max_z_flag)
    bits_equal(run_flag(b, truncation, max_z_flag), mask)
    for mk in ([mask, np.ones(b.n, np.uint8)] if emit_all else [mask]):
        rows, feats = run_emit(b, mk)
        want_rows, want_feats = io_ref.emit(*b.host, mk)
        bits_equal(rows, want_rows)
        bits_equal(feats, want_feats)
    dense = io_ref.scatter(*b.host, dims, max_z_scatter)
    bits_equal(run_scatter(b, dims, max_z_scatter), dense)
    return mask, dense


def distinct_coords(rng, counts, grid_zyx):
    """Packed (x,y,z) of counts[s] distinct voxels of `grid_zyx` per sample."""
    vol = int(np.prod(grid_zyx))
    out = []
    for c in counts:
        assert c <= vol
        z, y, x = np.unravel_index(rng.permutation(vol)[:c], grid_zyx)
        out.append(np.stack([x, y, z], 1))
    return np.concatenate(out).astype(np.uint32).reshape(-1, 3)


def voxel_sizes(nb):
    """One voxel size per sample, all distinct, none a power of two."""
    vs = (F32(0.0173) + F32(0.00037) * np.arange(nb, dtype=np.float32)).astype(np.float32)
    assert len(np.unique(vs)) == nb and np.all(np.frexp(vs)[0] != 0.5)
    return vs


# ---- sample lookup ---------------------------------------------------------------------------------------------
def _counts300(single=None):
    rng = np.random.default_rng(300)
    if single is not None:
        c = np.zeros(300, dtype=np.int64)
        c[single] = 29
        return c
    c = rng.integers(1, 13, 300)
    c[rng.random(300) < 0.4] = 0
    c[[0, 2, 3, 150, 151, 152, 298, 299]] = 0
    c[[1, 4, 149, 153, 297]] = 5
    return c


# name -> (counts, properties its emptiness pattern must have)
LOOKUP = {
    'nb1': ([37], []),
    'nb2_first_empty': ([0, 41], ['first']),
    'nb2_last_empty': ([41, 0], ['last']),
    'nb5_first_and_run': ([0, 7, 0, 0, 9], ['first', 'middle', 'run']),
    'nb5_middle_and_last_run': ([3, 0, 5, 0, 0], ['middle', 'last', 'run']),
    'nb5_single': ([0, 0, 11, 0, 0], ['first', 'last', 'run', 'single']),
    'nb300_mixed': (_counts300(), ['first', 'middle', 'last', 'run']),
    'nb300_single': (_counts300(173), ['first', 'last', 'run', 'single']),
}


def _pattern(counts):
    e = np.asarray(counts) == 0
    props = set()
    if e[0]:
        props.add('first')
    if e[-1]:
        props.add('last')
    if np.any(e[1:-1]):
        props.add('middle')
    if np.any(e[1:] & e[:-1]):
        props.add('run')
    if np.count_nonzero(~e) == 1 and len(e) > 1:
        props.add('single')
    return props


@pytest.mark.parametrize('name', sorted(LOOKUP))
def test_sample_lookup(name):
    counts, props = LOOKUP[name]
    counts = np.asarray(counts, dtype=np.int64)
    nb, T, dims = len(counts), 3.0, (4, 5, 6)
    assert nb in (1, 2, 5, 300) and set(props) <= _pattern(counts), (_pattern(counts), props)
    rng = np.random.default_rng(nb * 1000 + int(counts.sum()))
    vs, seg = voxel_sizes(nb), seg_of(counts)
    s = io_ref.sample_of(seg, int(seg[-1]))
    assert np.array_equal(np.bincount(s, minlength=nb), counts)
    # quotients within 0.2 % of the truncation, on both sides: the voxel size of the wrong sample flips the mask
    q = T * (1 + rng.choice([-1, 1], len(s)) * rng.uniform(1e-4, 2e-3, len(s))) * rng.choice([-1, 1], len(s))
    vals = (q * vs[s]).astype(np.float32)
    b = Batch(distinct_coords(rng, counts, dims), vals, vs, seg)
    mask, dense = check_all(b, T, dims)
    assert 0 < mask.sum() < b.n
    assert np.count_nonzero(np.isfinite(dense)) == b.n
    if nb > 1:                                     # what a lookup that is one sample off would have produced
        filled = np.nonzero(counts)[0]
        for wrong in (np.roll(filled, 1)[np.searchsorted(filled, s)], np.clip(s + 1, 0, nb - 1), np.maximum(s - 1, 0)):
            moved = wrong != s
            if not moved.any():
                continue
            wq = vals / vs[wrong]
            assert np.all((wq.view(np.uint32) != (vals / vs[s]).view(np.uint32))[moved])
            assert np.count_nonzero(((np.abs(wq) < F32(T)) != mask.astype(bool))[moved]) >= 0.25 * moved.sum()


# ---- grid stride -----------------------------------------------------------------------------------------------
BIG = CAP + 257


@pytest.fixture(scope='module')
def big():
    rng = np.random.default_rng(7)
    counts = [400000, 0, BIG - 400000]
    vs = voxel_sizes(3)
    seg = seg_of(counts)
    s = io_ref.sample_of(seg, BIG)
    vals = (rng.uniform(-6, 6, BIG) * vs[s]).astype(np.float32)
    b = Batch(distinct_coords(rng, counts, (100, 100, 100)), vals, vs, seg)
    assert b.n == BIG > CAP and b.n % 256 != 0 and b.n < 2 * CAP      # a full first trip, then a partial wrap
    return b


def test_grid_stride_flag(big):
    for max_z in (NOLIMIT, 50):
        want = io_ref.flag(*big.host, 3.0, max_z)
        assert 0.1 < want.mean() < 0.9
        assert 0 < want[CAP:].sum() < BIG - CAP                       # the wrapped tail holds both answers
        bits_equal(run_flag(big, 3.0, max_z), want)


def test_grid_stride_emit_every_entry(big):
    mask = np.ones(BIG, dtype=np.uint8)
    rows, feats = run_emit(big, mask)
    want_rows, want_feats = io_ref.emit(*big.host, mask)
    assert len(want_rows) == BIG > CAP
    assert set(np.unique(want_rows[:, 3])) == {0, 2}                  # sample 1 is empty
    bits_equal(rows, want_rows)
    bits_equal(feats, want_feats)


def test_grid_stride_emit_few_entries(big):
    """The launch is sized for n_max = n entries, the loop runs to *count: a few hundred rows, the rest untouched."""
    rng = np.random.default_rng(8)
    mask = np.zeros(BIG, dtype=np.uint8)
    mask[rng.permutation(BIG)[:300]] = 1
    mask[[0, 255, 256, CAP - 1, CAP, BIG - 1]] = 1
    assert 256 < mask.sum() < 1000 and mask.sum() % 256 != 0
    rows, feats = run_emit(big, mask)
    want_rows, want_feats = io_ref.emit(*big.host, mask)
    bits_equal(rows, want_rows)
    bits_equal(feats, want_feats)


def test_grid_stride_scatter(big):
    dims = (96, 96, 96)
    want = io_ref.scatter(*big.host, dims, 90)
    kept = np.count_nonzero(np.isfinite(want))
    assert 0 < kept < BIG and np.count_nonzero(np.isfinite(want[1])) == 0
    z, y, x = big.locs[CAP:, 2], big.locs[CAP:, 1], big.locs[CAP:, 0]
    inside = (z < 90) & (y < 96) & (x < 96)
    assert 0 < inside.sum() < BIG - CAP                               # the wrapped tail both writes and skips
    bits_equal(run_scatter(big, dims, 90), want)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_block_edges(n):
    rng = np.random.default_rng(n)
    counts = [n // 2, n - n // 2]
    vs, seg, dims = voxel_sizes(2), seg_of(counts), (7, 7, 7)
    vals = (rng.uniform(-6, 6, n) * vs[io_ref.sample_of(seg, n)]).astype(np.float32)
    b = Batch(distinct_coords(rng, counts, dims), vals, vs, seg)
    assert b.n == n
    mask, dense = check_all(b, 3.0, dims)
    assert np.count_nonzero(np.isfinite(dense)) == n
    if n > 1:
        assert 0 < mask.sum() < n


# ---- value edges -----------------------------------------------------------------------------------------------
EDGE_VS = [0.03, 0.0199999, 0.02, 0.046875, 7.3, 0.0173]


def _raw_for(q, vs):
    """A raw float32 whose correctly rounded quotient by vs is exactly q, or None (not every q has one)."""
    r0 = F32(F32(q) * F32(vs))
    cand = [r0]
    for _ in range(4):
        cand = [np.nextafter(cand[0], F32(-np.inf))] + cand + [np.nextafter(cand[-1], F32(np.inf))]
    for r in cand:
        if (F32(r) / F32(vs)).view(np.uint32) == F32(q).view(np.uint32):
            return F32(r)
    return None


@pytest.mark.parametrize('T', [3.0, 1.7])
def test_value_edges(T):
    T = F32(T)
    below, above = np.nextafter(T, F32(0)), np.nextafter(T, F32(np.inf))
    targets = [T, below, above, -T, -below, -above]
    rng = np.random.default_rng(11)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 2e-38, -2e-38]
    vals, counts, hit = [], [], np.zeros(6, dtype=int)
    for vs in EDGE_VS:
        mine = list(specials)
        for k, q in enumerate(targets):
            r = _raw_for(q, F32(vs))
            if r is not None:
                mine.append(r)
                hit[k] += 1
        mine += list(rng.uniform(-0.2, 0.2, 200) * (vs / 0.02))
        vals.append(np.array(mine, dtype=np.float32))
        counts.append(len(mine))
    assert np.all(hit >= 1), hit                                      # every edge is reached by some voxel size
    vals, vs, seg, dims = np.concatenate(vals), np.array(EDGE_VS, dtype=np.float32), seg_of(counts), (8, 8, 8)
    s = io_ref.sample_of(seg, len(vals))
    with np.errstate(all='ignore'):
        q = vals / vs[s]
    qb, tiny = q.view(np.uint32), np.finfo(np.float32).tiny
    for k, t in enumerate(targets):                                   # exactly at, one ulp below, one ulp above; both signs
        assert np.count_nonzero(qb == F32(t).view(np.uint32)) >= hit[k] >= 1
    assert np.isnan(q).any() and (q == np.inf).any() and (q == -np.inf).any()
    assert ((q == 0) & np.signbit(q)).any() and ((q == 0) & ~np.signbit(q)).any()
    sub = (q != 0) & (np.abs(q) < tiny)
    assert (sub & (np.abs(vals) >= tiny)).any() and (sub & (np.abs(vals) < tiny)).any()    # normal and subnormal raw
    b = Batch(distinct_coords(rng, counts, dims), vals, vs, seg)
    mask, dense = check_all(b, T, dims)
    near = np.isin(qb, [F32(t).view(np.uint32) for t in targets])
    assert np.array_equal(mask[near].astype(bool), np.abs(q[near]) < T)
    assert mask[near].any() and not mask[near].all() and 0 < mask.sum() < b.n
    assert not mask[np.isnan(q) | np.isinf(q)].any() and mask[sub].all() and mask[q == 0].all()
    assert np.isnan(dense).sum() == len(EDGE_VS) and (dense == np.inf).sum() == len(EDGE_VS)


# ---- clips -----------------------------------------------------------------------------------------------------
CLIP_DIMS = [(3, 5, 7), (1, 1, 1), (1, 4, 1), (8, 8, 8)]
CLIP_MAX_Z = {'0': lambda d0: 0, '1': lambda d0: 1, 'd0-1': lambda d0: d0 - 1, 'd0': lambda d0: d0,
              'd0+1': lambda d0: d0 + 1, '2^32': lambda d0: 1 << 32, '2^40': lambda d0: 1 << 40}


def _clip_points(dims, max_z):
    d0, d1, d2 = dims
    pts = {(z, y, x) for z in (0, d0 - 1) for y in (0, d1 - 1) for x in (0, d2 - 1)}           # the eight corners
    for z, y, x in ((0, 0, 0), (d0 - 1, d1 - 1, d2 - 1)):                                       # just outside each face
        pts |= {(d0, y, x), (z, d1, x), (z, y, d2)}
    for far in (1000, 70000, 2 ** 31 - 1):
        pts |= {(far, 0, 0), (0, far, 0), (0, 0, far), (far, far, far), (d0 - 1, d1 - 1, far)}
    for z in (max_z - 1, max_z):
        if 0 <= z < 2 ** 31:
            pts |= {(z, 0, 0), (z, d1 - 1, d2 - 1), (z, d1, 0)}
    return np.array(sorted(pts), dtype=np.int64)


@pytest.mark.parametrize('which', sorted(CLIP_MAX_Z))
@pytest.mark.parametrize('dims', CLIP_DIMS, ids=lambda d: '%dx%dx%d' % d)
def test_clips(dims, which):
    d0, d1, d2 = dims
    max_z = CLIP_MAX_Z[which](d0)
    assert max_z >= 0
    rng = np.random.default_rng(d0 * 100 + d1 * 10 + d2)
    pts, nb, T = _clip_points(dims, max_z), 3, 3.0
    vs = voxel_sizes(nb)
    locs = np.concatenate([pts[rng.permutation(len(pts))][:, ::-1] for _ in range(nb)])
    seg = seg_of([len(pts)] * nb)
    s = io_ref.sample_of(seg, len(locs))
    vals = (rng.uniform(-2.9, 2.9, len(locs)) * vs[s]).astype(np.float32)     # every value passes the truncation
    b = Batch(locs, vals, vs, seg)
    z, y, x = pts[:, 0], pts[:, 1], pts[:, 2]
    assert (x == d2).any() and (y == d1).any() and (z == d0).any() and (pts == 2 ** 31 - 1).any()
    if max_z < 2 ** 31:
        assert (z == max_z).any() and (max_z == 0 or (z == max_z - 1).any())
    mask, dense = check_all(b, T, dims, max_z_flag=max_z, max_z_scatter=max_z)
    assert np.array_equal(mask.astype(bool), b.locs[:, 2].astype(np.int64) < max_z)
    inside = (z < min(d0, max_z)) & (y < d1) & (x < d2)
    assert 0 <= inside.sum() < len(pts)
    for k in range(nb):                              # each sample's volume holds its own values and nothing else
        assert np.count_nonzero(np.isfinite(dense[k])) == inside.sum()
    corners = len({(a, c, e) for a in (0, d0 - 1) for c in (0, d1 - 1) for e in (0, d2 - 1)})
    if max_z == 0:
        assert inside.sum() == 0 and not mask.any()
    elif max_z >= d0:
        assert inside.sum() == corners                # nothing else of the set lies inside the volume
    else:
        assert inside.sum() > 0 and (pts[inside][:, 0] == max_z - 1).any()


# ---- alignment -------------------------------------------------------------------------------------------------
def test_inputs_are_only_4_byte_aligned():
    rng = np.random.default_rng(5)
    counts, dims = [333, 0, 444], (10, 10, 10)
    vs, seg = voxel_sizes(3), seg_of(counts)
    vals = (rng.uniform(-6, 6, 777) * vs[io_ref.sample_of(seg, 777)]).astype(np.float32)
    b = Batch(distinct_coords(rng, counts, dims), vals, vs, seg)
    for p in (b.p_locs, b.p_vals):
        assert p % 4 == 0 and p % 8 != 0 and p % 16 != 0
    mask, _ = check_all(b, 3.0, dims)
    assert 0 < mask.sum() < b.n


# ---- contract --------------------------------------------------------------------------------------------------
def test_empty_work_is_ok_with_null_pointers():
    _lib.call('sgnn_io_flag_entries', None, None, None, None, 1, 0, 3.0, 5, None)
    _lib.call('sgnn_io_emit_entries', None, None, None, None, 1, None, None, 0, None, None)
    _lib.call('sgnn_io_scatter_dense', None, None, None, None, 1, 0, 1, 1, 1, 5, None)
    b = Batch(np.zeros((0, 3)), np.zeros(0), voxel_sizes(2), [0, 0, 0])
    mask, rows = Guarded(8, torch.uint8, SENT_U8), Guarded(32, torch.int64, SENT_I64)
    feats, dense = Guarded(8, torch.int32, SENT_F32), Guarded(8, torch.int32, SENT_F32)
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    _lib.call('sgnn_io_flag_entries', b.p_locs, b.p_vals, b.p_vs, b.p_seg, 2, 0, 3.0, 5, mask.ptr)
    _lib.call('sgnn_io_emit_entries', b.p_locs, b.p_vals, b.p_vs, b.p_seg, 2, mask.ptr, count.data_ptr(), 0, rows.ptr,
              feats.ptr)
    _lib.call('sgnn_io_scatter_dense', b.p_locs, b.p_vals, b.p_vs, b.p_seg, 2, 0, 2, 2, 1, 5, dense.ptr)
    assert mask.untouched() and rows.untouched() and feats.untouched() and dense.untouched()


def test_bad_arguments_raise_and_write_nothing():
    rng = np.random.default_rng(9)
    counts, dims = [5, 6], (2, 2, 3)
    vs, seg = voxel_sizes(2), seg_of(counts)
    b = Batch(distinct_coords(rng, counts, dims), rng.uniform(-0.1, 0.1, 11), vs, seg)
    n, nb = b.n, b.nb
    mask, rows = Guarded(n, torch.uint8, SENT_U8), Guarded(4 * n, torch.int64, SENT_I64)
    feats, dense = Guarded(n, torch.int32, SENT_F32), Guarded(nb * 12, torch.int32, SENT_F32)
    sel = torch.arange(n, dtype=torch.int32, device='cuda')
    count = torch.tensor([n], dtype=torch.int64, device='cuda')
    flag_ok = [b.p_locs, b.p_vals, b.p_vs, b.p_seg, nb, n, 3.0, 5, mask.ptr]
    emit_ok = [b.p_locs, b.p_vals, b.p_vs, b.p_seg, nb, sel.data_ptr(), count.data_ptr(), n, rows.ptr, feats.ptr]
    scat_ok = [b.p_locs, b.p_vals, b.p_vs, b.p_seg, nb, n, 2, 2, 3, 5, dense.ptr]

    def bad(name, ok, **changes):
        args = list(ok)
        for k, v in changes.items():
            args[int(k[1:])] = v
        with pytest.raises(_lib.SgnnError, match='invalid argument'):
            _lib.call(name, *args)

    for ptr_at in (0, 1, 2, 3, 8):
        bad('sgnn_io_flag_entries', flag_ok, **{'a%d' % ptr_at: None})
    bad('sgnn_io_flag_entries', flag_ok, a4=0)           # nb == 0
    bad('sgnn_io_flag_entries', flag_ok, a4=-1)
    bad('sgnn_io_flag_entries', flag_ok, a5=-1)          # negative n
    bad('sgnn_io_flag_entries', flag_ok, a7=-1)          # negative max_z
    for ptr_at in (0, 1, 2, 3, 5, 6, 8, 9):
        bad('sgnn_io_emit_entries', emit_ok, **{'a%d' % ptr_at: None})
    bad('sgnn_io_emit_entries', emit_ok, a4=0)
    bad('sgnn_io_emit_entries', emit_ok, a7=-1)          # negative n_max
    for ptr_at in (0, 1, 2, 3, 10):
        bad('sgnn_io_scatter_dense', scat_ok, **{'a%d' % ptr_at: None})
    bad('sgnn_io_scatter_dense', scat_ok, a4=0)
    bad('sgnn_io_scatter_dense', scat_ok, a5=-1)
    for dim_at in (6, 7, 8):
        bad('sgnn_io_scatter_dense', scat_ok, **{'a%d' % dim_at: 0})
        bad('sgnn_io_scatter_dense', scat_ok, **{'a%d' % dim_at: -3})
    bad('sgnn_io_scatter_dense', scat_ok, a9=-1)
    assert mask.untouched() and rows.untouched() and feats.untouched() and dense.untouched()
    # the same arguments, unchanged, are accepted
    dense.body.view(torch.float32).fill_(-float('inf'))
    _lib.call('sgnn_io_flag_entries', *flag_ok)
    _lib.call('sgnn_io_emit_entries', *emit_ok)
    _lib.call('sgnn_io_scatter_dense', *scat_ok)
    bits_equal(mask.read(), io_ref.flag(*b.host, 3.0, 5))
    want_rows, want_feats = io_ref.emit(*b.host, np.ones(n, np.uint8))
    bits_equal(rows.read().reshape(n, 4), want_rows)
    bits_equal(feats.read().copy().view(np.float32), want_feats)
    bits_equal(dense.read().copy().view(np.float32).reshape(nb, 2, 2, 3), io_ref.scatter(*b.host, (2, 2, 3), 5))
