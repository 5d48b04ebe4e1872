"""Host reference for the table builders of grid_rules.hip that sit on top of the voxel hash: the 3x3x3 submanifold
rulebook (sgnn_rulebook_subm3, _multi, _dense, _volume), the stride-2 level (sgnn_rulebook_down2, sgnn_down2_tables) and
the stride-2 pyramid (sgnn_down2_chain, sgnn_down2_chain_tables).

Plain numpy, written from the header comments of include/sgnn_hip.h; nothing here is derived from a kernel and nothing is
imported from sgnn_amd.  Three parts:
  * the references: subm_table, down2, down2_tables, pyramid (+ table_lds, the leading dimensions the header prescribes);
  * the comparisons: assert_table compares a table where the library is obliged to write, check_pyramid holds a whole
    pyramid (counts, parents, coarse sites, tables, status word) to the reference, lay_out writes a pyramid into
    sentinel buffers the way an entry point does, so that test_rules_ref.py can hand check_pyramid a wrong one;
  * the data of the GPU tests (cloud, one_parent, own_parent, collapse, dense_volume, limit_cloud, non_neighbours,
    clamp_caps), shared with the CPU self-tests.

Which table entries the library is obliged to write: rows [0, min(roundup256(live count), ld)) of every offset, the rows
in [live count, roundup256(live count)) as -1.  The convolution kernels read a table in tiles of at most 256 rows that
start below the live count, so nothing beyond is ever read; what lies beyond may or may not be written, inside the buffer."""
import functools

import numpy as np

from glue_ref import (Guarded, dev_in, dev_out, assert_same_bits, live_count, hash_rows, sentinel, unwritten,  # noqa: F401
                      expand8, dense_coords, _rng, COORD_MAX, SCAN_BLOCK, SENT_INT, STATUS_COORD_RANGE, STATUS_DUPLICATE,
                      STATUS_OVERFLOW)

SIZES = (1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 5000)   # wave, 256-row tile and 2048-row scan block boundaries
ORDERS = ('raster', 'shuffled', 'children', 'spread')


def roundup256(n):
    return (int(n) + 255) // 256 * 256


def pack(coords):
    """int64 keys of (z, y, x, b) rows, every coordinate inside its range: b, z, y, x from the high bits down."""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    return (c[:, 3] << 48) | (c[:, 0] << 32) | (c[:, 1] << 16) | c[:, 2]


def offset_index(dz, dy, dx):
    return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def written_rows(n_live, ld):
    """Boolean (ld,): the rows of a table the library is obliged to write for n_live live rows."""
    return np.arange(ld) < min(roundup256(n_live), ld)


def subm_table(coords, n_live, ld):
    """(table, must): table (27, ld) int32 with table[k][j] = row of the site at p_j + d_k among the first n_live rows of
    coords, k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), else -1.  A neighbour with z, y or x outside [0, 65535] is absent;
    the batch index is never shifted.  must (27, ld): entries the library is obliged to write."""
    c = np.asarray(coords, np.int64).reshape(-1, 4)[:n_live]
    assert ld >= n_live == len(c)
    table = np.full((27, ld), -1, np.int32)
    must = np.broadcast_to(written_rows(n_live, ld), (27, ld)).copy()
    if n_live == 0:
        return table, must
    keys = pack(c)
    order = np.argsort(keys, kind='stable')
    sk = keys[order]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = c + np.array([dz, dy, dx, 0], np.int64)
                ok = ((q[:, :3] >= 0) & (q[:, :3] <= 65535)).all(1)
                qk = pack(np.where(ok[:, None], q, 0))
                pos = np.minimum(np.searchsorted(sk, qk), n_live - 1)
                hit = ok & (sk[pos] == qk)
                table[offset_index(dz, dy, dx), :n_live][hit] = order[pos[hit]]
    return table, must


def down2(coords, n_live):
    """(parent, coarse, count) of the first n_live rows: coarse sites = unique(z >> 1, y >> 1, x >> 1, b), numbered in
    first-touch order (walking the fine rows in order, a parent gets the next free row the first time it is met);
    parent[i] = coarse row of fine row i."""
    rows = {}
    parent = np.empty(n_live, np.int32)
    for i, (z, y, x, b) in enumerate(np.asarray(coords).reshape(-1, 4)[:n_live].tolist()):
        parent[i] = rows.setdefault((z >> 1, y >> 1, x >> 1, b), len(rows))
    coarse = np.array(list(rows), np.int32).reshape(-1, 4)
    return parent, coarse, len(rows)


def child_offset(coords):
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    return (c[:, 0] & 1) * 4 + (c[:, 1] & 1) * 2 + (c[:, 2] & 1)


def down2_tables(coords, parent, nf, nc, ldc, ldf):
    """(children (8, ldc), ptable (8, ldf), must_c, must_f) of the nf live fine rows and nc live coarse rows:
    children[k][c] = fine row whose parent is c and whose offset (z & 1) * 4 + (y & 1) * 2 + (x & 1) is k, else -1;
    ptable[k][i] = parent[i] if offset(i) == k else -1.  A parent at or above nc (a clamped level) counts as -1."""
    assert ldc >= nc and ldf >= nf
    children = np.full((8, ldc), -1, np.int32)
    ptable = np.full((8, ldf), -1, np.int32)
    off = child_offset(coords[:nf])
    p = np.asarray(parent[:nf], np.int64).copy()
    p[p >= nc] = -1
    i = np.arange(nf)
    ptable[off, i] = p
    children[off[p >= 0], p[p >= 0]] = i[p >= 0]
    return (children, ptable, np.broadcast_to(written_rows(nc, ldc), (8, ldc)).copy(),
            np.broadcast_to(written_rows(nf, ldf), (8, ldf)).copy())


def pyramid(coords, n_live, depth, cap, level_caps=None):
    """The stride-2 chain, level by level.  Returns (levels, overflow); level l holds
      fine, nf     the live rows the level is built from (level 0: the first n_live of coords)
      parent       true coarse row of every fine row (what sgnn_down2_chain writes)
      clamped      the same with rows at or above `count` replaced by -1 (sgnn_down2_chain_tables, sgnn_down2_tables + nc_dev)
      coarse       all coarse sites in first-touch order, total = their number
      count        rows of level l + 1: min(total, level_caps[l], cap) with level_caps, else total
    The next level is built from exactly the first `count` coarse rows, in their order."""
    assert n_live <= cap
    fine = np.asarray(coords, np.int32).reshape(-1, 4)[:n_live]
    levels, overflow = [], False
    for l in range(depth):
        parent, coarse, total = down2(fine, len(fine))
        count = total if level_caps is None else min(total, int(level_caps[l]), cap)
        overflow |= count < total
        levels.append(dict(fine=fine, nf=len(fine), parent=parent, clamped=np.where(parent >= count, -1, parent).astype(np.int32),
                           coarse=coarse, total=total, count=count, over=count < total))
        fine = coarse[:count]
    return levels, overflow


def table_lds(cap, depth, level_caps):
    """(ldc, ldf) of sgnn_down2_chain_tables: ldc_l = roundup256(min(level_caps[l], cap)), ldf_0 = roundup256(cap),
    ldf_l = ldc_{l-1}."""
    ldc = [roundup256(min(int(level_caps[l]), cap)) for l in range(depth)]
    return ldc, [roundup256(cap)] + ldc[:-1]


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def assert_table(got, want, must, what):
    """Bit-exact where the library is obliged to write; the rest of the buffer may hold anything."""
    got = np.asarray(got)
    assert got.shape == want.shape == must.shape, '%s: table %s, expected %s' % (what, got.shape, want.shape)
    assert_same_bits(np.where(must, got, want), want, what)


def lookup_queries(coarse):
    """Queries for the hash of a coarse level: its own sites, the same sites moved where no site lies, and rows outside
    the coordinate range."""
    c = np.asarray(coarse, np.int32).reshape(-1, 4)
    away = c[:64].copy()
    away[:, 1] = (away[:, 1] + 33000) % 65536      # no generator places sites 33 000 apart in y
    bad = np.array([(-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1), (65536, 0, 0, 0), (0, 65536, 0, 0),
                    (0, 0, 65536, 0), (0, 0, 0, 32768)], np.int32)
    return np.concatenate([c, away, bad])


def check_pyramid(got, levels, overflow, clamp_parent, preset, what):
    """got: counts (depth), parent[l], coarse[l], optional children[l] / ptable[l] with ldc / ldf, optional rows[l]
    (sgnn_hash_lookup of lookup_queries(kept coarse sites) in the level's hash), status (None: no status word)."""
    for l, lv in enumerate(levels):
        w = '%s level %d' % (what, l)
        assert int(got['counts'][l]) == lv['count'], '%s: count %d, expected %d (true %d)' % (
            w, int(got['counts'][l]), lv['count'], lv['total'])
        nf, nc = lv['nf'], lv['count']
        parent = lv['clamped'] if clamp_parent else lv['parent']
        assert_same_bits(np.asarray(got['parent'][l])[:nf], parent, w + ' parent')
        assert_same_bits(np.asarray(got['coarse'][l])[:nc], lv['coarse'][:nc], w + ' coarse sites')
        if got.get('children') is not None:
            ldc, ldf = got['ldc'][l], got['ldf'][l]
            ch, pt, mc, mf = down2_tables(lv['fine'], lv['parent'], nf, nc, ldc, ldf)
            assert_table(got['children'][l], ch, mc, w + ' children')
            assert_table(got['ptable'][l], pt, mf, w + ' ptable')
        if got.get('rows') is not None:
            q = lookup_queries(lv['coarse'][:nc])
            assert_same_bits(np.asarray(got['rows'][l]), hash_rows(lv['coarse'][:nc], q), w + ' hash lookup')
    if got.get('status') is not None:
        want = preset | (STATUS_OVERFLOW if overflow else 0)
        assert int(got['status']) == want, '%s: status %d, expected %d' % (what, int(got['status']), want)


def _sent(shape):
    return np.full(shape, SENT_INT, np.int32)


def lay_out(levels, overflow, cap, clamp_parent, preset, lds=None):
    """The pyramid as a correct entry point leaves it in sentinel buffers sized as the header prescribes: parent[l] (cap),
    coarse[l] (cap, 4), and with lds = (ldc, ldf) the tables, written over the obliged rows only."""
    got = dict(counts=[], parent=[], coarse=[], rows=[], status=preset | (STATUS_OVERFLOW if overflow else 0))
    if lds is not None:
        got.update(children=[], ptable=[], ldc=lds[0], ldf=lds[1])
    for l, lv in enumerate(levels):
        nf, nc = lv['nf'], lv['count']
        p, c = _sent(cap), _sent((cap, 4))
        p[:nf] = lv['clamped'] if clamp_parent else lv['parent']
        c[:lv['total']] = lv['coarse']
        got['counts'].append(nc)
        got['parent'].append(p)
        got['coarse'].append(c)
        got['rows'].append(hash_rows(lv['coarse'][:nc], lookup_queries(lv['coarse'][:nc])))
        if lds is not None:
            nt = min(nf, lds[1][l])        # (a wrong pyramid may hold more rows than its table: the table's rows, as a kernel's loop would)
            ch, pt, mc, mf = down2_tables(lv['fine'], lv['parent'], nt, nc, lds[0][l], lds[1][l])
            got['children'].append(np.where(mc, ch, SENT_INT).astype(np.int32))
            got['ptable'].append(np.where(mf, pt, SENT_INT).astype(np.int32))
    return got


# ---------------------------------------------------------------------------
# data of the GPU tests
# ---------------------------------------------------------------------------
def _frozen(a):
    a = np.ascontiguousarray(a, np.int32).reshape(-1, 4)
    a.setflags(write=False)
    return a


def cloud_side(n):
    """Even side of the cubic, two-sample volume the clouds of n sites live in (about a third of it occupied)."""
    s = 2
    while 2 * s ** 3 * 0.3 < n:
        s += 2
    return s


def _cells(cells, s):
    cells = np.asarray(cells, np.int64)
    b, v = cells // s ** 3, cells % s ** 3
    return np.stack([v // (s * s), (v // s) % s, v % s, b], 1).astype(np.int32)


@functools.lru_cache(None)
def cloud(order, n):
    """n distinct sites of a cloud_side(n)^3 x 2 volume.
      raster    batch-major raster order
      shuffled  random order
      children  8 consecutive rows per parent (the last parent may be cut short), parents in random order
      spread    the siblings of a parent as far apart in row order as possible: candidate row j * P + p is child j of
                parent p (P parents), a random n of the 8 P candidates are kept in that order - so a parent is first met
                in any of the eight strata, and its other children lie whole waves, 256-row tiles and 2048-row scan
                blocks further on"""
    s, rng = cloud_side(n), _rng('cloud', order, n)
    h = s // 2
    if order in ('raster', 'shuffled'):
        cells = rng.permutation(2 * s ** 3)[:n]
        return _frozen(_cells(np.sort(cells) if order == 'raster' else cells, s))
    if order == 'children':
        parents = _cells(rng.permutation(2 * h ** 3)[:-(-n // 8)], h)
        return _frozen(expand8(parents)[:n])
    assert order == 'spread'
    P = min(int(np.ceil(n / 5.6)) + 1, 2 * h ** 3)
    assert 8 * P >= n
    kids = expand8(_cells(rng.permutation(2 * h ** 3)[:P], h)).reshape(P, 8, 4)
    cand = kids.transpose(1, 0, 2).reshape(8 * P, 4)
    return _frozen(cand[np.sort(rng.permutation(8 * P)[:n])])


def one_parent(n):
    """n <= 8 sites under the one parent (3, 2, 5, 1), in random order."""
    assert 1 <= n <= 8
    return _frozen(expand8(np.array([[3, 2, 5, 1]], np.int32))[_rng('one', n).permutation(8)[:n]])


def sparse(n, k):
    """cloud('shuffled', n) k levels up: n sites with n different ancestors down to level k, where the cloud itself appears."""
    c = cloud('shuffled', n).copy()
    c[:, :3] = (c[:, :3] << k) + _rng('sparse', n, k).integers(0, 1 << k, (n, 3))
    return _frozen(c)


def own_parent(n):
    """n sites with n different parents (random parities)."""
    return sparse(n, 1)


def collapse(n):
    """n sites of one aligned power-of-two block (side 2^k >= n^(1/3)) of one sample: k levels down a single site is left."""
    k = 0
    while (1 << k) ** 3 < n:
        k += 1
    s = 1 << k
    cells = _rng('collapse', n).permutation(s ** 3)[:n]
    return _frozen(_cells(cells, s) + np.array([64, 128, 192, 3], np.int32)), k


def dense_volume(batch, dims):
    """Every voxel of a batch x dims volume in raster order: every edge row is next to another one in linear memory."""
    return _frozen(dense_coords(batch, *dims))


DENSE_VOLUMES = ((2, (3, 5, 7)), (3, (1, 1, 9)))


def limit_cloud():
    """0, 1, 65534 and 65535 on every axis in sample 32767 (64 sites, parents at 0 and 32767), and the eight corners
    again in sample 0; random order."""
    v = (0, 1, 65534, 65535)
    a = [(z, y, x, 32767) for z in v for y in v for x in v] + [(z, y, x, 0) for z in (0, 65535) for y in (0, 65535) for x in (0, 65535)]
    a = np.array(a, np.int32)
    return _frozen(a[_rng('limit').permutation(len(a))])


NON_NEIGHBOUR_DIMS, NON_NEIGHBOUR_BATCH = (3, 5, 7), 2


def non_neighbours():
    """Pairs that must not be neighbours, inside a 2 x (3, 5, 7) volume: the same z, y and x +- 1 in another sample; the
    last x of a row and the first x of the next row; the last voxel of a z slab and the first of the next; the last voxel
    of sample 0 and the first of sample 1.  No site of it has any neighbour but itself."""
    return _frozen(np.array([(1, 2, 3, 0), (1, 2, 4, 1), (1, 2, 2, 1), (2, 1, 6, 0), (2, 2, 0, 0), (0, 4, 6, 0), (1, 0, 0, 0),
                             (2, 4, 6, 0), (0, 0, 0, 1)], np.int32))


def clamp_caps(coords, n, depth, cap, at):
    """level_caps for one overflow, sized from the reference's own unclamped pyramid: every level before `at` gets exactly
    the rows it produces, level `at` about two thirds of them, the levels after it the whole capacity.  at = None: every
    level fits exactly and no flag may be raised."""
    levels, _ = pyramid(coords, n, depth, cap)
    caps = [lv['total'] for lv in levels]
    if at is not None:
        assert levels[at]['total'] >= 2
        caps[at] = levels[at]['total'] - max(1, levels[at]['total'] // 3)
        caps[at + 1:] = [cap] * (depth - at - 1)
    return caps


def clamp_cloud(order, n, at):
    """Sites of an overflow case: a cloud in one of the ORDERS, or ('sparse') sites whose level at + 1 is the shuffled
    cloud - there the coarse rows an overflow at level `at` drops have parents no kept row has, so a level built from the
    dropped rows as well has more rows than it should."""
    return sparse(n, at + 1) if order == 'sparse' else cloud(order, n)


# (sites, n, depth, level the overflow is meant for or None): the cases of the overflow tests of sgnn_down2_chain(_tables)
CLAMP_CASES = (('shuffled', 9, 1, 0), ('sparse', 257, 3, 0), ('sparse', 2049, 3, 1), ('shuffled', 5000, 3, 2),
               ('spread', 5000, 4, 1), ('children', 2048, 2, 1), ('sparse', 255, 2, 0), ('shuffled', 2049, 3, None),
               ('spread', 257, 4, None))


def chain_cap(n):
    """Capacity of the pyramid tests: some head-room above the live rows, off every tile size."""
    return n + 37


def padded_fine(coords, cap):
    """coords followed by cap - n rows the entry points must not read (sites of their own, far from the cloud)."""
    n = len(coords)
    pad = np.stack([np.arange(cap - n) + 30000, np.full(cap - n, 7), np.arange(cap - n) % 5, np.full(cap - n, 9)], 1)
    return np.concatenate([np.asarray(coords, np.int32), pad.astype(np.int32)])
