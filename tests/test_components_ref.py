"""tests/components_ref.py, the host restatement that the GPU labelling is compared with, checked against brute force
(the transitive closure of the adjacency matrix), against the hand-written cases and, where it is installed, against
scipy.ndimage.label; and the selection rules.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as CR  # noqa: E402

TILE = (8, 8, 32)
SHAPE = CR.default_shape(TILE)


def closure_labels(mask, connectivity):
    """Brute force: adjacency matrix of the foreground, closed under composition; numbering by the smallest member."""
    mask = np.asarray(mask) != 0
    m4 = mask.reshape((-1,) + mask.shape[-3:])
    cells = [tuple(int(v) for v in c) for c in np.argwhere(m4)]           # raster order
    maxc = {6: 1, 18: 2, 26: 3}[connectivity]
    n = len(cells)
    reach = np.eye(n, dtype=bool)
    for i, a in enumerate(cells):
        for j, b in enumerate(cells):
            d = [abs(p - q) for p, q in zip(a[1:], b[1:])]
            reach[i, j] |= a[0] == b[0] and max(d) <= 1 and 0 < sum(d) <= maxc
    while True:
        nxt = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    labels = np.full(m4.shape, -1, np.int32)
    sizes = []
    for i, c in enumerate(cells):
        first = int(np.flatnonzero(reach[i])[0])
        if first == i:
            sizes.append(int(reach[i].sum()))
            labels[c] = len(sizes) - 1
        else:
            labels[c] = labels[cells[first]]
    return labels.reshape(mask.shape), np.asarray(sizes, np.int64).reshape(-1)


@pytest.mark.parametrize('connectivity', [6, 18, 26])
@pytest.mark.parametrize('shape', [(5, 4, 3), (3, 4, 5), (2, 3, 2, 4), (1, 1, 7), (1, 1, 1)])
def test_volume_reference_equals_the_closure(shape, connectivity):
    rng = np.random.default_rng(sum(shape) * 31 + connectivity)
    for density in (0.0, 0.2, 0.35, 0.6, 1.0):
        mask = rng.random(shape) < density
        labels, sizes = CR.label_volume(mask, connectivity)
        want_labels, want_sizes = closure_labels(mask, connectivity)
        assert labels.dtype == np.int32 and sizes.dtype == np.int64 and sizes.shape == (len(want_sizes),)
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)


@pytest.mark.parametrize('connectivity', [6, 18, 26])
def test_sparse_reference_equals_the_dense_one(connectivity):
    rng = np.random.default_rng(connectivity)
    mask = rng.random((2, 5, 6, 7)) < 0.3
    locs = np.argwhere(mask)[:, [1, 2, 3, 0]]
    locs = np.concatenate([locs, locs[::9]])[rng.permutation(len(locs) + len(locs[::9]))]
    labels, sizes = CR.label_sparse(locs, (5, 6, 7), connectivity)
    dense, dense_sizes = CR.label_volume(mask, connectivity)
    assert np.array_equal(labels, dense[locs[:, 3], locs[:, 0], locs[:, 1], locs[:, 2]])
    assert np.array_equal(sizes, dense_sizes) and sizes.sum() == mask.sum()
    with pytest.raises(ValueError):
        CR.label_sparse(np.array([[0, 6, 0]]), (5, 6, 7), connectivity)


def test_offsets():
    for connectivity, n in ((6, 6), (18, 18), (26, 26)):
        assert len(CR.offsets(connectivity)) == n and len(CR.offsets(connectivity, forward=True)) == n // 2
        assert sorted(CR.offsets(connectivity)) == sorted(
            CR.offsets(connectivity, True) + [tuple(-v for v in o) for o in CR.offsets(connectivity, True)])


def test_serpentine_is_one_chain():
    path = CR.serpentine(SHAPE)
    assert len(set(path)) == len(path)
    steps = np.abs(np.diff(np.asarray(path), axis=0)).sum(1)
    assert (steps == 1).all()
    mask = CR.mask_of(SHAPE, path)
    assert mask.sum() == len(path) and mask[::2, ::2].all() and mask[-1].any() and mask[:, -1].any()
    labels, sizes = CR.label_volume(mask, 6)
    assert sizes.tolist() == [len(path)]
    # a chain: every voxel has two face neighbours in the path, the two ends have one
    pad = np.pad(mask, 1).astype(np.int64)
    nb = sum(np.roll(pad, s, a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert sorted(nb[mask != 0].tolist()) == [1, 1] + [2] * (len(path) - 2)
    cut = len(path) // 2
    labels, sizes = CR.label_volume(CR.mask_of(SHAPE, path[:cut] + path[cut + 1:]), 6)
    assert sizes.tolist() == [cut, len(path) - cut - 1]
    assert labels[path[0]] == 0 and labels[path[-1]] == 1 and labels[path[cut]] == -1


@pytest.mark.parametrize('connectivity', [6, 18, 26])
def test_corner_contacts_and_row_ends(connectivity):
    maxc = {6: 1, 18: 2, 26: 3}[connectivity]
    cases = CR.corner_contacts(TILE)
    assert len(cases) == 13 and sorted(CR.offset_class(o) for o, _ in cases) == [1] * 3 + [2] * 6 + [3] * 4
    for o, voxels in cases:
        sizes = CR.label_volume(CR.mask_of(SHAPE, voxels), connectivity)[1]
        assert sizes.tolist() == ([2] if CR.offset_class(o) <= maxc else [1, 1]), o
    for voxels in CR.no_wrap_cases(SHAPE):
        assert CR.label_volume(CR.mask_of(SHAPE, voxels), connectivity)[1].tolist() == [1, 1]
    full = np.ones((2, 3, 4, 5), np.uint8)
    labels, sizes = CR.label_volume(full, connectivity)
    assert sizes.tolist() == [60, 60] and (labels[0] == 0).all() and (labels[1] == 1).all()
    labels, sizes = CR.label_volume(np.zeros((3, 4, 5), np.uint8), connectivity)
    assert sizes.shape == (0,) and (labels == -1).all()


@pytest.mark.parametrize('connectivity,structure', [(6, 1), (18, 2), (26, 3)])
def test_volume_reference_equals_scipy(connectivity, structure):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(connectivity)
    for density in (0.12, 0.3, 0.6):
        mask = rng.random((9, 10, 11)) < density
        labels, sizes = CR.label_volume(mask, connectivity)
        theirs, count = ndimage.label(mask, ndimage.generate_binary_structure(3, structure))
        assert count == len(sizes)
        pairs = np.unique(np.stack([labels[mask], theirs[mask]], 1), axis=0)      # a bijection up to renumbering
        assert len(pairs) == count and len(set(pairs[:, 0])) == count and len(set(pairs[:, 1])) == count


def test_mesh_reference():
    f, v, fs, vs = CR.label_mesh(5, [[0, 1, 2], [2, 3, 4]])                         # bow-tie
    assert f.tolist() == [0, 0] and v.tolist() == [0] * 5 and fs.tolist() == [2] and vs.tolist() == [5]
    f, v, fs, vs = CR.label_mesh(9, [[6, 7, 8], [1, 2, 4], [4, 2, 1]])
    assert f.tolist() == [1, 0, 0] and v.tolist() == [-1, 0, 0, -1, 0, -1, 1, 1, 1]
    assert fs.tolist() == [2, 1] and vs.tolist() == [3, 3]
    f, v, fs, vs = CR.label_mesh(3, np.zeros((0, 3), np.int32))
    assert f.shape == (0,) and v.tolist() == [-1] * 3 and fs.shape == (0,) and vs.shape == (0,)
    nverts, faces = CR.strip_mesh(500, 0)
    f, v, fs, vs = CR.label_mesh(nverts, faces)
    assert fs.tolist() == [500] and vs.tolist() == [502]
    nverts, faces = CR.cluster_mesh(12, 30, 1)
    f, v, fs, vs = CR.label_mesh(nverts, faces)
    assert 12 <= len(fs) and (v == -1).sum() >= 30 and fs.sum() == len(faces)
    roots = [int(np.flatnonzero(v == k)[0]) for k in range(len(vs))]
    assert roots == sorted(roots)
    for bad in (nverts, -1):
        with pytest.raises(ValueError):
            CR.label_mesh(nverts, [[0, 1, bad]])


def _module_select(sizes, **kw):
    import torch
    from sgnn_amd import components
    got = components.select(torch.as_tensor(sizes, dtype=torch.int64), **kw)
    assert got.dtype == torch.bool
    assert np.array_equal(components.select(np.asarray(sizes, np.int64), **kw), got.numpy())
    return got.numpy()


@pytest.mark.parametrize('select', [CR.select, _module_select], ids=['ref', 'module'])
def test_select_rules(select):
    sizes = [5, 9, 5, 1, 9, 2]
    assert select(sizes).tolist() == [True] * 6
    assert select(sizes, min_size=5).tolist() == [True, True, True, False, True, False]
    assert select(sizes, keep_largest=1).tolist() == [False, True, False, False, False, False]      # tie: lower label
    assert select(sizes, keep_largest=3).tolist() == [True, True, False, False, True, False]
    assert select(sizes, keep_largest=0).tolist() == [False] * 6
    assert select(sizes, keep_largest=10).tolist() == [True] * 6
    assert select(sizes, min_size=6, keep_largest=3).tolist() == [False, True, False, False, True, False]   # both apply
    assert select(sizes, min_size=10, keep_largest=3).tolist() == [False] * 6
    assert select([], min_size=2, keep_largest=1).shape == (0,)
