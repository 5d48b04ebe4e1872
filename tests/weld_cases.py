"""Seeded synthetic triangle soups for the welding tests (tests/test_gpu_weld.py), and two host restatements used
to check that a soup really has the property it was built for: the reference's sequential greedy merge with its
look-up table kept, and the synchronous form of the sweep rule of csrc/mc.hip (k_weld_sweep) with its sweep count.

A soup is written in cell units (coordinate / thresh) and placed at a pitch by place(): 0.25, where every product and
quotient is exact, and the reference's own 1e-5.
"""
import itertools

import numpy as np

F32 = np.float32
PITCHES = (0.25, 0.00001)
CHAIN = 300                     # cells per chain: dependency depth = CHAIN (asserted >= 256 by the tests)
UNDECIDED, IN, OUT = 0, 1, 2    # csrc/mc.hip: W_UNDECIDED, W_IN, W_OUT
OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3)]      # dx, dy, dz: hasNearestNeighborApprox's order


def _jitter(rng, n):
    """Offsets inside a cell, multiples of 1/64 in [-0.25, 0.25]: exact at pitch 0.25, far from a boundary at 1e-5."""
    return rng.integers(-16, 17, (n, 3)) / 64.0


def _with_second_pass(rng, cells):
    """One vertex per cell in the given order, then one more per cell in random order (every cell exists by then, so
    these resolve by the scan order of the look-up alone)."""
    cells = np.asarray(cells, np.int64)
    both = np.concatenate([cells, cells[rng.permutation(len(cells))]])
    return both + _jitter(rng, len(both))


def _line(n, step, start=(0, 0, 0)):
    return np.asarray(start, np.int64) + np.arange(n)[:, None] * np.asarray(step, np.int64)


def chain_up(rng):
    return _with_second_pass(rng, _line(CHAIN, (1, 0, 0), (3, 5, 7)))


def chain_down(rng):            # crosses zero
    return _with_second_pass(rng, _line(CHAIN, (1, 0, 0), (-CHAIN // 2, -2, 4))[::-1])


def chain_middle(rng):          # the first vertex in the middle: one chain runs up from it, then one runs down
    line = _line(2 * CHAIN + 42, (0, 1, 0), (2, -30, 2))
    m = len(line) // 2
    return _with_second_pass(rng, np.concatenate([line[m:], line[:m][::-1]]))


def chain_diagonal(rng):
    """Four chains far apart.  Along (1,-1,0), (0,1,-1) and (1,0,-1) the two neighbours of a cell differ in the sign of
    two offsets, so whether dx is scanned before dy, dy before dz and dx before dz decides which one a vertex of a
    cell that was not created resolves to; along (1,1,1) all three agree."""
    chains = [_line(CHAIN, (1, 1, 1), (0, 0, 0)), _line(CHAIN, (1, -1, 0), (0, 0, 1000))[::-1],
              _line(CHAIN, (0, 1, -1), (0, 0, 2000)), _line(CHAIN, (1, 0, -1), (-40, 9, 3000))[::-1]]
    return _with_second_pass(rng, np.concatenate(chains))


def dense(rng, side=12, per_cell=4):
    """Every cell of a side^3 block around zero, several vertices per cell, in one random permutation: a greedy maximal
    independent set in random order."""
    cells = np.array(list(itertools.product(range(-side // 2, side - side // 2), repeat=3)), np.int64)
    cells = np.repeat(cells, per_cell, 0)[rng.permutation(len(cells) * per_cell)]
    return cells + _jitter(rng, len(cells))


def large(rng):
    """24000 vertices spread at random over a 20^3 block of cells."""
    return rng.integers(0, 20, (24000, 3)) + _jitter(rng, 24000)


def late(rng):
    """By hand.  v0 creates A = (2,0,0).  v1 falls into C = (1,0,0) beside A: C is not created.  v2 creates S = (0,0,0):
    its only neighbour C does not exist.  v3 falls into C again and now finds S, which the scan meets before A; v1, in
    the same cell, had to pass S over, because S did not exist yet.  v4 creates D far away, v5 repeats A."""
    return np.array([[2, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [12, 0, 0], [2, 0, 0]], np.float64) + _jitter(rng, 6)


def signs(rng):
    """Every triple of: negative, zero, -0.0, positive, and values exactly on a cell boundary (k + 0.5), either side of
    zero on each axis."""
    axis = [-1.5, -1.0, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 1.5]
    pts = np.array(list(itertools.product(axis, repeat=3)), np.float64)
    assert len(pts) % 3 == 0
    return pts[rng.permutation(len(pts))]


def _points(rng, n):
    """n points in cells 10 apart, and a function giving a jittered copy of point k (same cell)."""
    base = np.array([[10 * k, -10 * k, 5] for k in range(n)], np.float64)
    return lambda k: base[k] + _jitter(rng, 1)[0]


def faces_orders(rng):
    """The six orders of one triangle (the first, (1,2,0), has to survive as it stands), a triangle that welding makes
    degenerate, a plain triangle and a rotated copy of it made of near-copies of its corners."""
    p = _points(rng, 6)
    tris = [(1, 2, 0), (0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 0, 1), (2, 1, 0), (3, 3, 4), (3, 4, 5), (5, 3, 4), (4, 4, 4)]
    return np.array([p(k) for t in tris for k in t])


def faces_all_dropped(rng):
    """Every face has two corners in one cell: the vertices stay, no face does."""
    p = _points(rng, 5)
    tris = [(0, 0, 1), (2, 3, 2), (4, 1, 1), (3, 3, 3)]
    return np.array([p(k) for t in tris for k in t])


def sized(nv):
    def build(rng):             # nv vertices in a handful of cells, so that some weld
        return rng.integers(-1, 3, (nv, 3)) * 2 + _jitter(rng, nv)
    return build


SOUPS = {
    'chain_up': chain_up, 'chain_down': chain_down, 'chain_middle': chain_middle, 'chain_diagonal': chain_diagonal,
    'dense': dense, 'late': late, 'signs': signs, 'faces_orders': faces_orders, 'faces_all_dropped': faces_all_dropped,
    'nv0': sized(0), 'nv3': sized(3), 'nv6': sized(6), 'nv9': sized(9), 'large': large,
}
CHAINS = ['chain_up', 'chain_down', 'chain_middle', 'chain_diagonal']


def place(units, thresh):
    """Cell units -> float32 coordinates at pitch thresh."""
    return (np.asarray(units, np.float64).reshape(-1, 3).astype(F32) * F32(thresh)).astype(F32)


def make_soup(name, thresh):
    """-> (verts (nv,3) float32, vcols (nv,3) uint8), nv a multiple of 3."""
    rng = np.random.default_rng(3000 + sorted(SOUPS).index(name))
    verts = place(SOUPS[name](rng), thresh)
    assert len(verts) % 3 == 0
    return verts, rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)


def cells_of(verts, thresh):
    """The reference's grid cell of a vertex: (int)(v / thresh + 0.5f * sgn(v)) per axis, in float32."""
    v = np.asarray(verts, F32)
    return np.trunc(v / F32(thresh) + F32(0.5) * np.sign(v).astype(F32)).astype(np.int64).reshape(-1, 3)


def greedy(cells):
    """The reference's merge_close_vertices(approx) as it runs, one vertex after the other -> (lookup (nv,) = the
    vertex whose cell vertex i resolves to, i itself where it creates its cell; created: cell -> creating vertex)."""
    created, lookup = {}, np.zeros(len(cells), np.int64)
    for i, c in enumerate(map(tuple, cells.tolist())):
        hit = -1
        for dx, dy, dz in OFFSETS:
            hit = created.get((c[0] + dx, c[1] + dy, c[2] + dz), -1)
            if hit >= 0:
                break
        if hit < 0:
            created[c] = hit = i
        lookup[i] = hit
    return lookup, created


def _key(c):
    return ((c[:, 0] + (1 << 20)) * (1 << 21) + (c[:, 1] + (1 << 20))) * (1 << 21) + (c[:, 2] + (1 << 20))


def sweeps(cells):
    """The sweep rule of k_weld_sweep run synchronously (every cell reads the states of the sweep before): a cell
    with an earlier neighbour that is IN goes OUT, one whose earlier neighbours are all OUT goes IN, any other waits.
    -> (number of sweeps until no cell waits, distinct cells (n,3), first vertex of each (n,), final states (n,))."""
    uniq, first = np.unique(cells, axis=0, return_index=True)
    n = len(uniq)
    if n == 0:
        return 0, uniq, first, np.zeros(0, np.int8)
    order = np.argsort(_key(uniq))
    sorted_keys = _key(uniq)[order]
    nb = np.full((n, 26), -1, np.int64)
    for j, off in enumerate(o for o in OFFSETS if o != (0, 0, 0)):
        q = _key(uniq + np.asarray(off))
        p = np.minimum(np.searchsorted(sorted_keys, q), n - 1)
        hit = sorted_keys[p] == q
        nb[hit, j] = order[p[hit]]
    earlier = (nb >= 0) & (first[nb] < first[:, None])
    state, count = np.zeros(n, np.int8), 0
    while (state == UNDECIDED).any():
        st = state[nb]
        any_in = (earlier & (st == IN)).any(1)
        all_out = (~earlier | (st == OUT)).all(1)
        waiting = state == UNDECIDED
        new = state.copy()
        new[waiting & any_in] = OUT
        new[waiting & ~any_in & all_out] = IN
        assert (new != state).any(), 'the sweep rule made no progress'
        state, count = new, count + 1
    return count, uniq, first, state
