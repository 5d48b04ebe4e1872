"""The host reference of sgnn_amd.edt (tests/edt_ref.py) against hand-written cases, against scipy where it is
installed, and against the three-pass decomposition that the kernels rely on.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_ref as ER  # noqa: E402


def mask(shape, seeds):
    m = np.zeros(shape, dtype=np.uint8)
    for s in seeds:
        m[s] = 1
    return m


def test_single_seed():
    d2, nr = ER.brute(mask((2, 3, 4), [(1, 2, 3)]))
    z, y, x = np.meshgrid(np.arange(2), np.arange(3), np.arange(4), indexing='ij')
    assert np.array_equal(d2, (z - 1) ** 2 + (y - 2) ** 2 + (x - 3) ** 2)
    assert (nr == 1 * 12 + 2 * 4 + 3).all()
    assert d2.dtype == np.int32 and nr.dtype == np.int32


def test_row_by_hand():
    #          x: 0  1  2  3  4  5  6
    m = np.array([0, 1, 0, 0, 0, 1, 0], dtype=np.uint8).reshape(1, 1, 7)
    d2, nr = ER.brute(m)
    assert d2.reshape(-1).tolist() == [1, 0, 1, 4, 1, 0, 1]
    assert nr.reshape(-1).tolist() == [1, 1, 1, 1, 5, 5, 5]          # x = 3 is 2 from both: the smaller x wins


def test_tie_between_lower_z_and_lower_x():
    # seeds (0, 0, 1) = index 1 and (1, 0, 0) = index 3; voxel (1, 0, 1) is at squared distance 1 from both
    d2, nr = ER.brute(mask((3, 1, 3), [(0, 0, 1), (1, 0, 0)]))
    assert d2[1, 0, 1] == 1 and nr[1, 0, 1] == 1                     # the lower z: the smaller linear index
    # (2, 0, 0): 4 + 1 from index 1, 1 from index 3; (0, 0, 0): 1 from both again
    assert d2[2, 0, 0] == 1 and nr[2, 0, 0] == 3
    assert d2[0, 0, 0] == 1 and nr[0, 0, 0] == 1
    # (2, 0, 2): 4 + 1 = 5 from index 1, 1 + 4 = 5 from index 3
    assert d2[2, 0, 2] == 5 and nr[2, 0, 2] == 1


def test_tie_between_lower_y_and_lower_x():
    d2, nr = ER.brute(mask((1, 3, 3), [(0, 0, 2), (0, 2, 0)]))       # indices 2 and 6
    assert d2[0, 1, 1] == 2 and nr[0, 1, 1] == 2
    assert d2[0, 2, 2] == 4 and nr[0, 2, 2] == 2
    assert d2[0, 0, 0] == 4 and nr[0, 0, 0] == 2


def test_seeds_are_their_own_nearest_and_no_seeds_is_minus_one():
    rng = np.random.default_rng(1)
    m = (rng.random((5, 6, 7)) < 0.2).astype(np.uint8)
    d2, nr = ER.brute(m)
    lin = np.arange(m.size).reshape(m.shape)
    assert (d2[m != 0] == 0).all() and np.array_equal(nr[m != 0], lin[m != 0])
    assert (d2[m == 0] > 0).all() and (m.reshape(-1)[nr[m == 0]] != 0).all()
    d2, nr = ER.brute(np.zeros((2, 3, 4), dtype=np.uint8))
    assert (d2 == -1).all() and (nr == -1).all()
    d2, nr = ER.brute(np.ones((2, 3, 4), dtype=np.uint8))
    assert (d2 == 0).all() and np.array_equal(nr.reshape(-1), np.arange(24))


def test_chunking_does_not_show():
    m = (np.random.default_rng(2).random((6, 7, 9)) < 0.3).astype(np.uint8)
    a = ER.brute(m)
    b = ER.brute(m, chunk_keys=1)                                     # one seed at a time
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cap():
    assert ER.cap2_of(None) is None and ER.cap2_of(0) == 0 and ER.cap2_of(1.5) == 2 and ER.cap2_of(2.5) == 6
    assert ER.cap2_of(1e30) is None
    with pytest.raises(ValueError):
        ER.cap2_of(-1.0)
    m = (np.random.default_rng(3).random((6, 7, 9)) < 0.03).astype(np.uint8)
    d2, nr = ER.brute(m)
    for r in (0, 1, 1.5, 2.5, 7, 1000):
        c2, cn = ER.feature_transform(m, r)
        near = d2 <= (ER.cap2_of(r) if ER.cap2_of(r) is not None else 1 << 40)
        assert np.array_equal(c2[near], d2[near]) and np.array_equal(cn[near], nr[near])
        assert (c2[~near] == -1).all() and (cn[~near] == -1).all()
    c2, cn = ER.feature_transform(m, 0)
    assert np.array_equal(c2 == 0, m != 0)


def test_fill():
    rng = np.random.default_rng(4)
    m = (rng.random((4, 5, 6)) < 0.1).astype(np.uint8)
    col = rng.integers(1, 256, size=m.shape + (3,), dtype=np.uint8)
    d2, nr = ER.feature_transform(m, 1.5)
    out = ER.fill_colors(col, nr)
    assert np.array_equal(out[m != 0], col[m != 0])
    assert (out[nr < 0] == 0).all() and (out[nr >= 0] != 0).all()
    p = (1, 2, 3)
    if nr[p] >= 0:
        assert np.array_equal(out[p], col.reshape(-1, 3)[nr[p]])


@pytest.mark.parametrize('shape', [(7, 9, 11), (1, 1, 13), (1, 12, 1), (12, 1, 1), (3, 4, 30)])
@pytest.mark.parametrize('density', [0.5, 0.05, 0.005])
def test_distances_equal_scipy(shape, density):
    ndi = pytest.importorskip('scipy.ndimage')
    m = np.random.default_rng(5).random(shape) < density
    if not m.any():
        m[tuple(s // 2 for s in shape)] = True                         # scipy needs a seed
    d2, _ = ER.brute(m)
    want = np.rint(ndi.distance_transform_edt(~m) ** 2).astype(np.int64)
    assert np.array_equal(d2, want)


def lattice(shape, step=4):
    m = np.zeros(shape, dtype=np.uint8)
    m[::step, ::step, ::step] = 1
    return m


@pytest.mark.parametrize('shape', [(7, 9, 11), (1, 1, 13), (1, 12, 1), (12, 1, 1), (10, 9, 13)])
def test_three_passes_equal_brute_force(shape):
    """x, then y, then z, each with ties to the smaller coordinate, picks the lexicographically smallest seed among
    the nearest: the decomposition of the kernels.  The lattice is all ties."""
    rng = np.random.default_rng(6)
    cases = [(rng.random(shape) < d).astype(np.uint8) for d in (0.4, 0.05, 0.01)]
    cases += [lattice(shape), np.zeros(shape, dtype=np.uint8), np.ones(shape, dtype=np.uint8)]
    for m in cases:
        a, b = ER.brute(m), ER.separable(m)
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1])
