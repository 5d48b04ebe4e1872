"""The host reference of tests/rules_ref.py, held to account on the CPU alone: it agrees with independent statements of
the same tables (a brute-force neighbour search, the oracle, tests/conv_ref.py, the symmetry of the rulebook, children and
ptable being each other's inverse), its comparisons notice nine kinds of wrong kernel on the very data test_gpu_rules.py
runs on, and the level capacities chosen for the overflow tests clamp exactly where they are meant to."""
import numpy as np
import pytest
import torch

import rules_ref as R


def _clouds(max_n=None):
    """(name, sites) of every cloud the GPU tests build a 3x3x3 rulebook of."""
    for order in R.ORDERS:
        for n in R.SIZES:
            if max_n is None or n <= max_n:
                yield '%s n=%d' % (order, n), R.cloud(order, n)
    for batch, dims in R.DENSE_VOLUMES:
        yield 'dense %d x %s' % (batch, dims), R.dense_volume(batch, dims)
    yield 'limit', R.limit_cloud()
    yield 'non-neighbours', R.non_neighbours()


def _table(c, ld=None):
    n = len(c)
    return R.subm_table(c, n, R.roundup256(n) if ld is None else ld)


# ---- agreement with independent statements ----

def _brute(c):
    """O(n^2): t[k][j] = i iff site i = site j + d_k and both lie in the same sample."""
    c = np.asarray(c, np.int64)
    n = len(c)
    t = np.full((27, n), -1, np.int32)
    d = c[:, None, :] - c[None, :, :]                     # d[i, j] = c_i - c_j
    near = (np.abs(d[:, :, :3]).max(2) <= 1) & (d[:, :, 3] == 0)
    for i, j in np.argwhere(near):
        t[R.offset_index(*d[i, j, :3]), j] = i
    return t


def test_subm_table_is_the_brute_force_search():
    seen = 0
    for name, c in _clouds(300):
        t, must = _table(c)
        R.assert_same_bits(t[:, :len(c)], _brute(c), name)
        assert (t[:, len(c):] == -1).all() and must.all()
        seen += 1
    assert seen >= 4 * 7 + 4
    assert (R.subm_table(R.non_neighbours(), 9, 256)[0][:, :9] >= 0).sum(0).tolist() == [1] * 9      # nobody but itself
    lim, _ = _table(R.limit_cloud())
    assert ((lim >= 0).sum(0)[:72] >= 1).all() and (lim[13, :72] == np.arange(72)).all()


def test_subm_table_is_the_oracle_and_conv_ref():
    import scn_oracle
    import conv_ref
    for name, c in _clouds():
        n = len(c)
        t, _ = _table(c)
        R.assert_same_bits(t[:, :n].astype(np.int64), np.asarray(scn_oracle.Grid(c.astype(np.int64)).subm_rules()), name + ' oracle')
        if c.max() < 64:
            R.assert_same_bits(t[:, :n].astype(np.int64), conv_ref.subm_rulebook(torch.from_numpy(c.copy())).numpy(), name + ' conv_ref')


def test_subm_table_symmetry_live_count_and_padding():
    for name, c in _clouds():
        n = len(c)
        t, _ = _table(c)
        k, j = np.nonzero(t[:, :n] >= 0)
        assert (t[26 - k, t[k, j]] == j).all(), name             # t[k][j] = i  <=>  t[26 - k][i] = j
        assert (t[13, :n] == np.arange(n)).all()
    c = R.cloud('shuffled', 257)
    for live in (0, 1, 128, 257):
        t, must = R.subm_table(c, live, 512 + 512)
        assert must[:, :R.roundup256(live)].all() and not must[:, R.roundup256(live):].any()
        assert (t[:, live:] == -1).all() and t[:, :live].max(initial=-1) < max(live, 0) or live == 0
        R.assert_same_bits(t[:, :live], R.subm_table(c[:live], live, live)[0], 'live rows only')
    assert not R.subm_table(c, 257, 300)[1][:, 300:].any() and R.subm_table(c, 257, 300)[1].all()     # ld below roundup256(n)


def test_down2_is_the_oracle_and_tables_are_inverse():
    import scn_oracle
    data = [(name, c) for name, c in _clouds()] + [('one parent %d' % n, R.one_parent(n)) for n in (1, 7, 8)] + \
        [('own parent %d' % n, R.own_parent(n)) for n in R.SIZES] + [('sparse 2049', R.sparse(2049, 2))]
    for name, c in data:
        n = len(c)
        parent, coarse, nc = R.down2(c, n)
        g, op, ooff = scn_oracle.down2_rules(scn_oracle.Grid(c.astype(np.int64)))
        R.assert_same_bits(parent.astype(np.int64), np.asarray(op), name + ' parent')
        R.assert_same_bits(coarse.astype(np.int64), g.coords, name + ' coarse')
        assert np.array_equal(R.child_offset(c), ooff)
        assert len(np.unique(R.pack(coarse))) == nc == parent.max() + 1
        assert np.array_equal(coarse[parent], np.concatenate([c[:, :3] >> 1, c[:, 3:]], 1))
        first = np.full(nc, n)
        np.minimum.at(first, parent, np.arange(n))
        assert (np.diff(first) > 0).all(), name                   # first-touch order
        ldc, ldf = R.roundup256(nc) + 512, R.roundup256(n)
        ch, pt, mc, mf = R.down2_tables(c, parent, n, nc, ldc, ldf)
        k, p = np.nonzero(ch >= 0)
        assert len(k) == n and (pt[k, ch[k, p]] == p).all() and (pt >= 0).sum() == n        # each other's inverse
        assert ((pt[:, :n] >= 0).sum(0) == 1).all() and (pt[:, n:] == -1).all() and (ch[:, nc:] == -1).all()
        assert mc[:, :R.roundup256(nc)].all() and not mc[:, R.roundup256(nc):].any() and mf.all()
    assert R.down2(R.one_parent(8), 8)[2] == 1 and R.down2(R.own_parent(257), 257)[2] == 257
    lim = R.down2(R.limit_cloud(), 72)[1]
    assert lim[:, :3].max() == 32767 and lim[:, 3].max() == 32767


def test_pyramid_is_repeated_down2():
    for order, n, depth in (('shuffled', 2049, 4), ('spread', 257, 3), ('children', 9, 2)):
        c = R.cloud(order, n)
        levels, over = R.pyramid(c, n, depth, R.chain_cap(n))
        fine = c
        for lv in levels:
            parent, coarse, nc = R.down2(fine, len(fine))
            assert lv['count'] == lv['total'] == nc and np.array_equal(lv['parent'], parent) and np.array_equal(lv['clamped'], parent)
            fine = coarse
        assert not over
    for n in (1, 9, 257):
        c, k = R.collapse(n)
        levels, _ = R.pyramid(c, n, 4, R.chain_cap(n))
        assert [lv['count'] for lv in levels][k:] == [1] * (4 - k) and (k == 0 or levels[k - 1]['nf'] > 1)
    assert R.collapse(257)[1] == 3
    assert R.table_lds(300, 3, [1000, 257, 5]) == ([512, 512, 256], [512, 512, 512])


# ---- every mutant is noticed on the data of the GPU tests ----

def _rejected(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def _mirror_as_k(t, n):
    """The mirror entry of offset k written to row k instead of row 26 - k."""
    m = t.copy()
    m[14:, :n] = -1
    for k in range(13):
        j = np.nonzero(t[k, :n] >= 0)[0]
        m[k, t[k, j]] = j
    return m


def _swap_dz_dx(t):
    m = t.copy()
    for k in range(27):
        dz, dy, dx = k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1
        m[R.offset_index(dx, dy, dz)] = t[k]
    return m


def _across_batches(c, ld):
    """The neighbour search with the sample index left out of the key."""
    table = {}
    for r, (z, y, x, b) in enumerate(c.tolist()):
        table[(z, y, x)] = r
    m = np.full((27, ld), -1, np.int32)
    for j, (z, y, x, b) in enumerate(c.tolist()):
        for k in range(27):
            m[k, j] = table.get((z + k // 9 - 1, y + (k // 3) % 3 - 1, x + k % 3 - 1), -1)
    return m


def _across_row_wrap(c, batch, dims, ld):
    """The dense-volume search without the bounds test: a neighbour is whatever lies at the shifted linear address."""
    Z, Y, X = dims
    vol = np.full(batch * Z * Y * X, -1, np.int32)
    lin = ((c[:, 3].astype(np.int64) * Z + c[:, 0]) * Y + c[:, 1]) * X + c[:, 2]
    vol[lin] = np.arange(len(c))
    m = np.full((27, ld), -1, np.int32)
    for k in range(27):
        a = lin + ((k // 9 - 1) * Y + ((k // 3) % 3 - 1)) * X + (k % 3 - 1)
        ok = (a >= 0) & (a < len(vol))
        m[k, :len(c)][ok] = vol[a[ok]]
    return m


def test_wrong_subm_tables_are_rejected():
    for name, c in _clouds():
        n = len(c)
        t, must = _table(c, R.roundup256(n) + 512)
        R.assert_table(t, t, must, name)
        if (t[:13] >= 0).any():                                   # at least one pair of neighbours
            _rejected(R.assert_table, _mirror_as_k(t, n), t, must, name)
        if n >= 255 or name.startswith('dense'):
            _rejected(R.assert_table, _swap_dz_dx(t), t, must, name)
        if n % 256:                                               # [n, roundup256(n)) left unwritten
            unpadded = np.where(np.arange(t.shape[1]) < n, t, R.SENT_INT).astype(np.int32)
            _rejected(R.assert_table, unpadded, t, must, name)
        beyond = np.where(must, t, R.SENT_INT).astype(np.int32)  # what lies past roundup256(n) is nobody's business
        R.assert_table(beyond, t, must, name)
    for name, c in list(_clouds(2049))[-4:] + [('shuffled 257', R.cloud('shuffled', 257)), ('raster 2049', R.cloud('raster', 2049))]:
        t, must = _table(c)
        _rejected(R.assert_table, _across_batches(c, t.shape[1]), t, must, name) if c[:, 3].max() > 0 and name != 'limit' else None
    for batch, dims in R.DENSE_VOLUMES:
        c = R.dense_volume(batch, dims)
        t, must = _table(c)
        _rejected(R.assert_table, _across_row_wrap(c, batch, dims, t.shape[1]), t, must, 'row wrap')
    c = R.non_neighbours()
    t, must = _table(c)
    _rejected(R.assert_table, _across_row_wrap(c, R.NON_NEIGHBOUR_BATCH, R.NON_NEIGHBOUR_DIMS, 256), t, must, 'row wrap')
    _rejected(R.assert_table, _across_batches(c, 256), t, must, 'batch')
    # each of the four pairs of non_neighbours() is what one of the two mutants finds
    w, a = _across_row_wrap(c, R.NON_NEIGHBOUR_BATCH, R.NON_NEIGHBOUR_DIMS, 256), _across_batches(c, 256)
    assert (w[:, 3] >= 0).sum() == 2 and (w[:, 5] >= 0).sum() == 2 and (w[:, 7] >= 0).sum() == 2 and (a[:, 0] >= 0).sum() == 3


def _sorted_order(levels):
    """Every level's coarse rows numbered in sorted key order instead of first-touch order (the following levels built
    from the renumbered rows)."""
    out, fine = [], levels[0]['fine']
    for lv in levels:
        parent, coarse, nc = R.down2(fine, len(fine))
        order = np.argsort(R.pack(coarse), kind='stable')
        rank = np.empty(nc, np.int32)
        rank[order] = np.arange(nc, dtype=np.int32)
        out.append(dict(lv, fine=fine, nf=len(fine), parent=rank[parent], clamped=rank[parent], coarse=coarse[order], total=nc, count=nc))
        fine = coarse[order]
    return out


def _xyz_parity(lv):
    """A level whose tables take the offset bits in x, y, z order."""
    f = lv['fine'][:, [2, 1, 0, 3]]
    return dict(lv, fine=f)


def _tables_of(levels, over, cap, lds, mutate=None):
    got = R.lay_out(levels, over, cap, True, 0, lds)
    if mutate:
        mutate(got)
    return got


def test_wrong_pyramids_are_rejected():
    for order in R.ORDERS:
        for n in R.SIZES:
            c = R.cloud(order, n)
            cap, depth = R.chain_cap(n), 2
            levels, over = R.pyramid(c, n, depth, cap)
            lds = R.table_lds(cap, depth, [cap] * depth)
            for clamp in (False, True):
                R.check_pyramid(R.lay_out(levels, over, cap, clamp, 2, lds), levels, over, clamp, 2, 'reference')
            wrong = _sorted_order(levels)
            if order != 'raster' and n >= 255:                    # (raster order meets the parents in sorted order)
                assert not np.array_equal(wrong[0]['parent'], levels[0]['parent']), (order, n)
            if not np.array_equal(wrong[0]['parent'], levels[0]['parent']):
                _rejected(R.check_pyramid, R.lay_out(wrong, over, cap, False, 0), levels, over, False, 0, 'sorted')
            if n >= 7:
                wrong = [_xyz_parity(levels[0])] + levels[1:]
                _rejected(R.check_pyramid, R.lay_out(wrong, over, cap, True, 0, lds), levels, over, True, 0, 'parity')
            if levels[0]['count'] % 256:                          # padding of children left unwritten

                def spoil(got, nc=levels[0]['count']):
                    got['children'][0][:, nc:] = R.SENT_INT
                _rejected(R.check_pyramid, _tables_of(levels, over, cap, lds, spoil), levels, over, True, 0, 'padding')

            def spoil(got, nf=n):
                got['ptable'][0][:, nf:] = R.SENT_INT
            if n % 256:
                _rejected(R.check_pyramid, _tables_of(levels, over, cap, lds, spoil), levels, over, True, 0, 'padding')


def _case(order, n, depth, at):
    c = R.clamp_cloud(order, n, at)
    cap = R.chain_cap(n)
    caps = R.clamp_caps(c, n, depth, cap, at)
    return c, cap, caps


def _next_from_all(c, n, depth, cap, caps):
    """The level after a clamped one built from all of its coarse rows instead of the kept ones."""
    levels, _ = R.pyramid(c, n, depth, cap, caps)
    out, fine = [], c[:n]
    for l in range(depth):
        parent, coarse, total = R.down2(fine, len(fine))
        count = min(total, caps[l], cap)
        out.append(dict(fine=fine, nf=len(fine), parent=parent, clamped=np.where(parent >= count, -1, parent).astype(np.int32),
                        coarse=coarse, total=total, count=count, over=count < total))
        fine = coarse
    return out


@pytest.mark.parametrize('order,n,depth,at', R.CLAMP_CASES)
def test_clamp_cases_are_real_and_wrong_clamps_are_rejected(order, n, depth, at):
    c, cap, caps = _case(order, n, depth, at)
    assert all(1 <= v <= cap for v in caps)
    free, _ = R.pyramid(c, n, depth, cap)
    levels, over = R.pyramid(c, n, depth, cap, caps)
    lds = R.table_lds(cap, depth, caps)
    assert [lv['over'] for lv in levels] == [l == at for l in range(depth)] and over == (at is not None)
    for clamp in (False, True):
        R.check_pyramid(R.lay_out(levels, over, cap, clamp, 1, lds), levels, over, clamp, 1, 'reference')
    if at is None:
        assert [lv['count'] for lv in levels] == caps == [lv['total'] for lv in free]     # an exact fit raises no flag
        _rejected(R.check_pyramid, R.lay_out(levels, True, cap, True, 1, lds), levels, over, True, 1, 'flag')
        return
    lv = levels[at]
    assert lv['count'] == caps[at] < lv['total'] == free[at]['total'] and (lv['clamped'] == -1).any()
    assert (lv['clamped'][lv['parent'] < lv['count']] >= 0).all() and levels[at]['nf'] == free[at]['nf']
    if at + 1 < depth:
        assert levels[at + 1]['nf'] == caps[at] and np.array_equal(levels[at + 1]['fine'], lv['coarse'][:caps[at]])
    # the overflow bit missing, or a preset bit lost
    _rejected(R.check_pyramid, R.lay_out(levels, False, cap, True, 1, lds), levels, over, True, 1, 'no flag')
    _rejected(R.check_pyramid, R.lay_out(levels, over, cap, True, 0, lds), levels, over, True, 1, 'preset bit lost')

    def unclamped(got):
        got['counts'][at] = lv['total']
    _rejected(R.check_pyramid, _tables_of(levels, over, cap, lds, unclamped), levels, over, True, 0, 'count not clamped')
    # parents past the kept count left in place where the entry point clamps them
    _rejected(R.check_pyramid, R.lay_out(levels, over, cap, False, 0, lds), levels, over, True, 0, 'parent not clamped')
    if at + 1 < depth:
        wrong = _next_from_all(c, n, depth, cap, caps)
        assert wrong[at + 1]['nf'] == lv['total']
        # with tables the extra rows show in children; without, in the next count - where they bring new parents along,
        # which the sparse clouds make sure of
        _rejected(R.check_pyramid, R.lay_out(wrong, over, cap, True, 0, lds), levels, over, True, 0, 'next level from all rows')
        if order == 'sparse':
            assert wrong[at + 1]['count'] > levels[at + 1]['count']
            _rejected(R.check_pyramid, R.lay_out(wrong, over, cap, False, 0), levels, over, False, 0, 'next level from all rows')


def test_overflow_cases_cover_first_middle_and_last_level():
    ats = {(at, depth) for _, _, depth, at in R.CLAMP_CASES}
    assert any(at == 0 and d > 1 for at, d in ats) and any(at is not None and 0 < at < d - 1 for at, d in ats)
    assert any(at is not None and at == d - 1 and d > 1 for at, d in ats) and any(at is None for at, _ in ats)
    pad = R.padded_fine(R.cloud('shuffled', 9), R.chain_cap(9))
    assert len(pad) == 46 and len(np.unique(R.pack(pad))) == 46 and np.array_equal(pad[:9], R.cloud('shuffled', 9))
