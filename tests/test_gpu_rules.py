"""The table builders of grid_rules.hip against tests/rules_ref.py: the 3x3x3 rulebook through the hash
(sgnn_rulebook_subm3, _multi) and through the dense index volume (_dense, _volume), the stride-2 level
(sgnn_rulebook_down2 + sgnn_down2_tables) and the stride-2 pyramid (sgnn_down2_chain, sgnn_down2_chain_tables).

The C entry points are called the way sgnn_amd/scn/metadata.py calls them, host arrays of device pointers included.  Every
output, the hash storage and the workspaces lie in sentinel buffers sized exactly as include/sgnn_hip.h prescribes; all
comparisons are bit for bit.  A table is compared over the rows the library is obliged to write, [0, min(roundup256(live
count), ld)); beyond them only the guards count.  Hash grids are compared by behaviour: sgnn_hash_lookup must answer
with its row for every kept coarse site and with -1 for absent and out-of-range queries.

Sizes are rules_ref.SIZES (1 .. 5000: the boundaries of a wave, a 256-row tile and a 2048-row scan block); the other
launch forms are reached through the switches scan_inline (k_scan_block_sums between count and write kernel),
chain_merged (k_chain_tables_insert or k_chain_parent_tables + k_chain_insert) and rulebook_multi, restored by fixtures.

tests/test_rules_ref.py shows on the same data and with the same comparisons that a mirrored or transposed offset index,
sorted instead of first-touch coarse rows, swapped parity bits, a neighbour across samples or across a row wrap of the
volume, unwritten padding, an unclamped count and a level built from dropped rows would each fail here."""
import numpy as np
import pytest

import rules_ref as R

pytestmark = pytest.mark.gpu


def L():
    from sgnn_amd import _lib
    return _lib


def _switch(name):
    @pytest.fixture(params=[1, 0], ids=['%s=1' % name, '%s=0' % name])
    def fixture(request):
        saved = L().tune(name)
        L().tune(name, request.param)
        try:
            yield request.param
        finally:
            L().tune(name, saved)
    return fixture


scan_inline = _switch('scan_inline')
chain_merged = _switch('chain_merged')
rulebook_multi = _switch('rulebook_multi')


def _i64(v):
    return None if v is None else R.dev_in(np.array([v], np.int64))


def _ptr(buf):
    return None if buf is None else buf.ptr


def _ptrs(bufs):
    """Host array of device pointers (kept alive by the caller for the duration of the call)."""
    return np.ascontiguousarray(np.array([0 if b is None else b.ptr for b in bufs], np.uint64))


def _small_cap(n):
    """The smallest legal hash capacity: a power of two >= 2 n (load factor up to 1/2: long probe sequences)."""
    cap = 2
    while cap < 2 * n:
        cap *= 2
    return cap


def _hash(co, n, cap, nd):
    keys, vals, status = R.dev_out((cap,), np.int64), R.dev_out((cap,), np.int32), R.dev_in(np.zeros(1, np.int32))
    L().call('sgnn_hash_build', _ptr(co), n, keys.ptr, vals.ptr, cap, status.ptr, _ptr(nd))
    assert int(status.check('hash status')[0]) == 0
    return keys, vals


def _lookup(keys, vals, cap, queries, what):
    q, rows = R.dev_in(queries), R.dev_out((len(queries),), np.int32)
    L().call('sgnn_hash_lookup', keys.ptr, vals.ptr, cap, q.ptr, len(queries), rows.ptr, None)
    return rows.check(what + ' lookup')


# ---------------------------------------------------------------------------
# 3x3x3 rulebook through the hash
# ---------------------------------------------------------------------------
def _subm3(c, what):
    """sgnn_rulebook_subm3 over n_dev x hash capacity x ld for one cloud."""
    n = len(c)
    co = R.dev_in(c)
    ld0 = R.roundup256(n)
    for n_dev in (None, n, n // 2, 0, 1):
        live, nd = R.live_count(n, n_dev), _i64(n_dev)
        want, must = R.subm_table(c, live, ld0 + 512)
        for cap in sorted({L().query('sgnn_hash_capacity', n), _small_cap(n)}):
            keys, vals = _hash(co, n, cap, nd)
            for ld in (ld0, ld0 + 512):
                w = '%s n_dev=%s cap=%d ld=%d' % (what, n_dev, cap, ld)
                nbr = R.dev_out((27, ld), np.int32)
                L().call('sgnn_rulebook_subm3', keys.ptr, vals.ptr, cap, co.ptr, n, nbr.ptr, ld, _ptr(nd))
                R.assert_table(nbr.check(w), want[:, :ld], must[:, :ld], w)
            keys.check(what + ' keys'), vals.check(what + ' vals')


@pytest.mark.parametrize('order', R.ORDERS)
def test_rulebook_subm3(order):
    for n in R.SIZES:
        _subm3(R.cloud(order, n), 'subm3 %s n=%d' % (order, n))


def test_rulebook_subm3_edges():
    for batch, dims in R.DENSE_VOLUMES:
        _subm3(R.dense_volume(batch, dims), 'subm3 dense %d x %s' % (batch, dims))
    _subm3(R.limit_cloud(), 'subm3 coordinate limits')
    _subm3(R.non_neighbours(), 'subm3 non-neighbours')


# level sizes of the multi-level call; per set, one run with every level live (two thirds of the odd levels) and one with
# the live count of one level at 0
MULTI_SETS = ((257,), (2049, 255), (5000, 0, 9), (256, 2047, 7, 1))


def test_rulebook_subm3_multi(rulebook_multi):
    for si, ns in enumerate(MULTI_SETS):
        for dead in (None, max(range(len(ns)), key=lambda i: (ns[i] > 0, i))):
            lv = []
            for i, n in enumerate(ns):
                c = R.cloud(R.ORDERS[(si + i) % 4], n) if n else None
                live = 0 if i == dead else (n - n // 3 if i % 2 else n)
                co, nd = (R.dev_in(c) if n else None), _i64(live)
                cap = L().query('sgnn_hash_capacity', n)
                keys, vals = _hash(co, n, cap, nd)
                ld = R.roundup256(max(n, 1)) + (512 if i % 2 else 0)
                lv.append(dict(c=c, n=n, live=live, co=co, nd=nd, cap=cap, keys=keys, vals=vals, ld=ld,
                               nbr=R.dev_out((27, ld), np.int32)))
            args = [_ptrs([v['keys'] for v in lv]), _ptrs([v['vals'] for v in lv]), np.array([v['cap'] for v in lv], np.int64),
                    _ptrs([v['co'] for v in lv]), np.array(ns, np.int64), _ptrs([v['nbr'] for v in lv]),
                    np.array([v['ld'] for v in lv], np.int64), _ptrs([v['nd'] for v in lv])]
            L().call('sgnn_rulebook_subm3_multi', len(ns), *[a.ctypes.data for a in args])
            for i, v in enumerate(lv):
                w = 'subm3_multi levels %s dead=%s level %d' % (ns, dead, i)
                if v['n'] == 0:
                    v['nbr'].check(w, untouched=np.ones((27, v['ld']), bool))
                else:
                    want, must = R.subm_table(v['c'], v['live'], v['ld'])
                    R.assert_table(v['nbr'].check(w), want, must, w)


# ---------------------------------------------------------------------------
# 3x3x3 rulebook through the dense index volume
# ---------------------------------------------------------------------------
def _volume_call(c, dims, entries, n_dev, what, volume_only=False, preset=0):
    """One sgnn_rulebook_subm3_dense / _volume call; the volume must be all -1 afterwards.  Returns (table, status)."""
    n = len(c)
    co, nd = R.dev_in(c), _i64(n_dev)
    ld = R.roundup256(n)
    vol, nbr = R.dev_in(np.full(max(entries, 1), -1, np.int32)), R.dev_out((27, ld), np.int32)
    status = R.dev_in(np.array([preset], np.int32))
    if volume_only:
        L().call('sgnn_rulebook_subm3_volume', co.ptr, n, *dims, vol.ptr, entries, nbr.ptr, ld, _ptr(nd), status.ptr)
    else:
        cap = L().query('sgnn_hash_capacity', n)
        keys, vals = _hash(co, n, cap, nd)
        L().call('sgnn_rulebook_subm3_dense', keys.ptr, vals.ptr, cap, co.ptr, n, *dims, vol.ptr, entries, nbr.ptr, ld, _ptr(nd))
    assert (vol.check(what + ' volume') == -1).all(), '%s: the volume is not all -1 afterwards' % what
    return nbr.check(what), int(status.check(what + ' status')[0])


def _volume_case(c, dims, entries, what, volume_only=False):
    n = len(c)
    for n_dev in (None, n // 2):
        live = R.live_count(n, n_dev)
        w = '%s n_dev=%s' % (what, n_dev)
        got, st = _volume_call(c, dims, entries, n_dev, w, volume_only, R.STATUS_DUPLICATE)
        want, must = R.subm_table(c, live, R.roundup256(n))
        R.assert_table(got, want, must, w)
        assert st == R.STATUS_DUPLICATE, '%s: status %d' % (w, st)


def _edge_volumes():
    for batch, dims in R.DENSE_VOLUMES:
        yield 'dense %d x %s' % (batch, dims), R.dense_volume(batch, dims), dims, batch * int(np.prod(dims))
    yield 'non-neighbours', R.non_neighbours(), R.NON_NEIGHBOUR_DIMS, R.NON_NEIGHBOUR_BATCH * int(np.prod(R.NON_NEIGHBOUR_DIMS))


def test_rulebook_subm3_dense():
    for n in R.SIZES:
        c, s = R.cloud('shuffled', n), R.cloud_side(n)
        what = 'subm3_dense n=%d' % n
        _volume_case(c, (s, s, s), 2 * s ** 3, what + ' inside')
        small = (max(1, s // 2), s, max(1, s - 1))
        _volume_case(c, small, 2 * int(np.prod(small)), what + ' sites outside dims (hash fall-back)')
        _volume_case(c, (s, s, s), s ** 3 + 5, what + ' sample 1 beyond the volume')
        _volume_case(c, (s, s, s), s ** 3 - 1, what + ' volume smaller than one block')
    _volume_case(R.cloud('raster', 2049), (R.cloud_side(2049),) * 3, 2 * R.cloud_side(2049) ** 3, 'subm3_dense raster')
    _volume_case(R.cloud('children', 2049), (R.cloud_side(2049),) * 3, 2 * R.cloud_side(2049) ** 3, 'subm3_dense children')
    for name, c, dims, entries in _edge_volumes():
        _volume_case(c, dims, entries, 'subm3_dense ' + name)


def test_rulebook_subm3_volume():
    for n in R.SIZES:
        s = R.cloud_side(n)
        for order in ('shuffled', 'children'):
            _volume_case(R.cloud(order, n), (s, s, s), 2 * s ** 3 + 3, 'subm3_volume %s n=%d' % (order, n), volume_only=True)
    for name, c, dims, entries in _edge_volumes():
        _volume_case(c, dims, entries, 'subm3_volume ' + name, volume_only=True)


def test_rulebook_subm3_volume_flags_an_uncovered_site():
    for n in (9, 257, 2049):
        s = R.cloud_side(n)
        c = R.cloud('shuffled', n).copy()
        for row, site in ((n // 2, (s, 0, 0, 0)), (n - 1, (0, 0, 0, 2)), (0, (0, s - 1, s, 1))):     # z, sample, x outside
            bad = c.copy()
            bad[row] = site
            for preset in (0, R.STATUS_DUPLICATE):
                what = 'subm3_volume n=%d uncovered site %s' % (n, site)
                _, st = _volume_call(bad, (s, s, s), 2 * s ** 3, None, what, True, preset)
                assert st == preset | R.STATUS_COORD_RANGE, '%s: status %d' % (what, st)


# ---------------------------------------------------------------------------
# stride-2 level
# ---------------------------------------------------------------------------
def _down2(c, what):
    n = len(c)
    co = R.dev_in(c)
    ccap = L().query('sgnn_hash_capacity', n)
    wsb = L().query('sgnn_down2_ws_bytes', n)
    ckeys, cvals, ws = R.dev_out((ccap,), np.int64), R.dev_out((ccap,), np.int32), R.dev_out((wsb,), np.uint8)
    parent, coarse, cnt = R.dev_out((n,), np.int32), R.dev_out((n, 4), np.int32), R.dev_out((1,), np.int64)
    L().call('sgnn_rulebook_down2', co.ptr, n, ckeys.ptr, cvals.ptr, ccap, parent.ptr, coarse.ptr, cnt.ptr, ws.ptr, wsb)
    want_parent, want_coarse, nc = R.down2(c, n)
    ws.check(what + ' workspace'), ckeys.check(what + ' keys'), cvals.check(what + ' vals')
    assert int(cnt.check(what + ' count')[0]) == nc, '%s: %d coarse sites, expected %d' % (what, int(cnt.host()[cnt.g.lead]), nc)
    R.assert_same_bits(parent.check(what), want_parent, what + ' parent')
    R.assert_same_bits(coarse.check(what)[:nc], want_coarse, what + ' coarse sites')
    q = R.lookup_queries(want_coarse)
    R.assert_same_bits(_lookup(ckeys, cvals, ccap, q, what), R.hash_rows(want_coarse, q), what + ' hash lookup')
    for nf_dev, nc_dev, extra in ((None, None, 0), (None, None, 512), (n, nc, 512), (n - n // 3, nc, 0), (n, nc - 1, 0)):
        nf_live, nc_live = R.live_count(n, nf_dev), R.live_count(nc, nc_dev)
        ldc, ldf = R.roundup256(nc) + extra, R.roundup256(n) + extra
        w = '%s tables nf_dev=%s nc_dev=%s ldc=%d ldf=%d' % (what, nf_dev, nc_dev, ldc, ldf)
        children, ptable = R.dev_out((8, ldc), np.int32), R.dev_out((8, ldf), np.int32)
        nfd, ncd = _i64(nf_dev), _i64(nc_dev)
        L().call('sgnn_down2_tables', co.ptr, parent.ptr, n, children.ptr, ldc, nc, ptable.ptr, ldf, _ptr(nfd), _ptr(ncd))
        ch, pt, mc, mf = R.down2_tables(c, want_parent, nf_live, nc_live, ldc, ldf)
        R.assert_table(children.check(w), ch, mc, w + ' children')
        R.assert_table(ptable.check(w), pt, mf, w + ' ptable')


@pytest.mark.parametrize('order', R.ORDERS)
def test_down2_and_tables(order, scan_inline):
    for n in R.SIZES:
        _down2(R.cloud(order, n), 'down2 %s n=%d' % (order, n))


def test_down2_and_tables_edges(scan_inline):
    for n in (1, 7, 8):
        _down2(R.one_parent(n), 'down2 one parent n=%d' % n)
    for n in R.SIZES:
        _down2(R.own_parent(n), 'down2 every site its own parent n=%d' % n)
    _down2(R.limit_cloud(), 'down2 coordinate limits')


# ---------------------------------------------------------------------------
# stride-2 pyramid
# ---------------------------------------------------------------------------
def _chain(c, depth, caps, n0_on_device, tables, preset, what):
    """One sgnn_down2_chain (tables = False) or sgnn_down2_chain_tables call with every buffer sized as the header says,
    held to rules_ref.pyramid."""
    n = len(c)
    cap = R.chain_cap(n)
    ccap = L().query('sgnn_hash_capacity', cap)
    fine = R.dev_in(R.padded_fine(c, cap))
    ckeys = [R.dev_out((ccap,), np.int64) for _ in range(depth)]
    cvals = [R.dev_out((ccap,), np.int32) for _ in range(depth)]
    parent = [R.dev_out((cap,), np.int32) for _ in range(depth)]
    coarse = [R.dev_out((cap, 4), np.int32) for _ in range(depth)]
    counts, status = R.dev_out((depth,), np.int64), R.dev_in(np.array([preset], np.int32))
    n0 = _i64(n) if n0_on_device else None
    caps_np = None if caps is None else np.ascontiguousarray(np.array(caps, np.int64))
    keep = [_ptrs(ckeys), _ptrs(cvals), _ptrs(parent), _ptrs(coarse)]
    got = dict()
    if tables:
        ldc, ldf = R.table_lds(cap, depth, caps)
        children = [R.dev_out((8, ldc[l]), np.int32) for l in range(depth)]
        ptable = [R.dev_out((8, ldf[l]), np.int32) for l in range(depth)]
        keep += [_ptrs(children), _ptrs(ptable)]
        wsb = L().query('sgnn_down2_chain_tables_ws_bytes', cap, depth)
        ws = R.dev_out((wsb,), np.uint8)
        L().call('sgnn_down2_chain_tables', fine.ptr, n0.ptr, cap, depth, keep[0].ctypes.data, keep[1].ctypes.data, ccap,
                 keep[2].ctypes.data, keep[3].ctypes.data, counts.ptr, caps_np.ctypes.data, keep[4].ctypes.data,
                 keep[5].ctypes.data, status.ptr, ws.ptr, wsb)
        got.update(children=[b.check(what + ' children') for b in children], ptable=[b.check(what + ' ptable') for b in ptable],
                   ldc=ldc, ldf=ldf)
    else:
        wsb = L().query('sgnn_down2_chain_ws_bytes', cap)
        ws = R.dev_out((wsb,), np.uint8)
        L().call('sgnn_down2_chain', fine.ptr, 0 if n0_on_device else n, _ptr(n0), cap, depth, keep[0].ctypes.data,
                 keep[1].ctypes.data, ccap, keep[2].ctypes.data, keep[3].ctypes.data, counts.ptr,
                 None if caps is None else caps_np.ctypes.data, status.ptr, ws.ptr, wsb)
    ws.check(what + ' workspace')
    levels, over = R.pyramid(c, n, depth, cap, caps)
    got.update(counts=counts.check(what + ' counts'), status=int(status.check(what + ' status')[0]),
               parent=[b.check(what + ' parent') for b in parent], coarse=[b.check(what + ' coarse') for b in coarse], rows=[])
    for l, lv in enumerate(levels):
        ckeys[l].check(what + ' keys'), cvals[l].check(what + ' vals')
        got['rows'].append(_lookup(ckeys[l], cvals[l], ccap, R.lookup_queries(lv['coarse'][:lv['count']]), what))
    R.check_pyramid(got, levels, over, tables, preset, what)
    return over


def _chain_clouds(order):
    """(name, sites, depth): every size at depth 1 .. 4 in turn, and for one order each the pyramids that collapse to a
    single site before the last level and the coordinate-limit cloud."""
    for i, n in enumerate(R.SIZES):
        yield '%s n=%d' % (order, n), R.cloud(order, n), 1 + i % 4
    if order == 'shuffled':
        for n in (1, 9, 257):
            yield 'collapse n=%d' % n, R.collapse(n)[0], 4
    if order == 'spread':
        yield 'coordinate limits', R.limit_cloud(), 3
        yield 'spread n=5000', R.cloud(order, 5000), 4


@pytest.mark.parametrize('order', ['shuffled', 'spread'])
def test_down2_chain(order, scan_inline):
    for i, (name, c, depth) in enumerate(_chain_clouds(order)):
        for on_device in (False, True):
            what = 'down2_chain %s depth=%d n0 on the %s' % (name, depth, 'device' if on_device else 'host')
            assert not _chain(c, depth, None, on_device, False, 0, what)
            caps = [R.chain_cap(len(c))] * depth if (i + on_device) % 2 else R.clamp_caps(c, len(c), depth, R.chain_cap(len(c)), None)
            assert not _chain(c, depth, caps, on_device, False, R.STATUS_DUPLICATE, what + ' level_caps=%s' % caps)


@pytest.mark.parametrize('order', ['shuffled', 'spread'])
def test_down2_chain_tables(order, scan_inline, chain_merged):
    for i, (name, c, depth) in enumerate(_chain_clouds(order)):
        caps = [R.chain_cap(len(c))] * depth if i % 2 else R.clamp_caps(c, len(c), depth, R.chain_cap(len(c)), None)
        what = 'down2_chain_tables %s depth=%d level_caps=%s' % (name, depth, caps)
        assert not _chain(c, depth, caps, True, True, R.STATUS_COORD_RANGE * (i % 2), what)     # large enough: no flag


@pytest.mark.parametrize('order,n,depth,at', R.CLAMP_CASES)
def test_down2_chain_overflow(order, n, depth, at, scan_inline):
    c = R.clamp_cloud(order, n, at)
    caps = R.clamp_caps(c, n, depth, R.chain_cap(n), at)
    for on_device in (False, True):
        what = 'down2_chain %s n=%d depth=%d overflow at %s level_caps=%s' % (order, n, depth, at, caps)
        assert _chain(c, depth, caps, on_device, False, R.STATUS_DUPLICATE, what) == (at is not None)


@pytest.mark.parametrize('order,n,depth,at', R.CLAMP_CASES)
def test_down2_chain_tables_overflow(order, n, depth, at, scan_inline, chain_merged):
    c = R.clamp_cloud(order, n, at)
    caps = R.clamp_caps(c, n, depth, R.chain_cap(n), at)
    for preset in (0, R.STATUS_DUPLICATE):
        what = 'down2_chain_tables %s n=%d depth=%d overflow at %s level_caps=%s' % (order, n, depth, at, caps)
        assert _chain(c, depth, caps, True, True, preset, what) == (at is not None)


def test_down2_launch_counts(scan_inline, chain_merged, monkeypatch):
    """Kernel launches of the three stride-2 builders (sgnn_launch_count around each call), 300 sites at depth 2:
    sgnn_rulebook_down2 5 and sgnn_down2_chain 5 per level, one more each for the scan launch of scan_inline = 0;
    sgnn_down2_chain_tables 3 per level + 2 at the defaults, 5 per level + 1 with both switches off."""
    lib, launches = L(), {}
    real_call = lib.call

    def counting_call(name, *args):
        before = lib.query('sgnn_launch_count')
        real_call(name, *args)
        launches[name] = lib.query('sgnn_launch_count') - before

    monkeypatch.setattr(lib, 'call', counting_call)
    c, depth = R.cloud('shuffled', 300), 2
    caps = [R.chain_cap(len(c))] * depth
    _down2(c, 'launch counts: down2')
    _chain(c, depth, None, True, False, 0, 'launch counts: chain')
    _chain(c, depth, caps, True, True, 0, 'launch counts: chain_tables')
    scan = 0 if scan_inline else 1
    assert launches['sgnn_rulebook_down2'] == 5 + scan
    assert launches['sgnn_down2_chain'] == (5 + scan) * depth
    # one init, per level count (+ scan) + write + tables, and the insertions: one launch of their own for level 0 only
    # (chain_merged: the others ride in the tables launch of the level above) or for every level
    assert launches['sgnn_down2_chain_tables'] == 1 + (3 + scan) * depth + (1 if chain_merged else depth)
    if scan_inline and chain_merged:
        assert launches['sgnn_down2_chain_tables'] == 3 * depth + 2
    if not scan_inline and not chain_merged:
        assert launches['sgnn_down2_chain_tables'] == 5 * depth + 1
