"""sgnn_amd.components on the GPU against the host restatement tests/components_ref.py: labels and sizes are integers
and must be equal, for the tile-local route (tiled=True), the one-level route (tiled=False) and between the two."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as CR  # noqa: E402

from sgnn_amd import _lib, components, marching_cubes as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = CR.default_shape(components.TILE_ZYX)       # two full tiles and a ragged remainder on every axis
CONNECTIVITIES = (6, 18, 26)
MAXC = {6: 1, 18: 2, 26: 3}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def random_mask(density, seed=0, shape=SHAPE):
    m = (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def random_ref(density, connectivity):
    return CR.label_volume(random_mask(density), connectivity)


def label_both(mask, connectivity, **kw):
    """Labels of the two routes, each run twice (determinism), checked against each other; returns the tiled one."""
    out = []
    for tiled in (True, False):
        a = components.label_volume(mask, connectivity=connectivity, tiled=tiled, **kw)
        b = components.label_volume(mask, connectivity=connectivity, tiled=tiled, **kw)
        assert a.labels.dtype == torch.int32 and a.sizes.dtype == torch.int64 and a.labels.shape == mask.shape
        assert torch.equal(a.labels, b.labels) and torch.equal(a.sizes, b.sizes), 'two runs differ (tiled=%s)' % tiled
        out.append(a)
    assert torch.equal(out[0].labels, out[1].labels) and torch.equal(out[0].sizes, out[1].sizes), 'the routes differ'
    return host(out[0].labels), host(out[0].sizes)


def check(mask, connectivity, want=None):
    want = CR.label_volume(mask, connectivity) if want is None else want
    labels, sizes = label_both(dev(mask), connectivity)
    assert sizes.shape == want[1].shape and np.array_equal(sizes, want[1])
    assert np.array_equal(labels, want[0])
    return labels, sizes


def test_tile():
    assert SHAPE == (19, 17, 69)


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
@pytest.mark.parametrize('density', [0.05, 0.12, 0.25, 0.32, 0.6])
def test_random_masks(density, connectivity):
    labels, sizes = check(random_mask(density), connectivity, random_ref(density, connectivity))
    assert sizes.sum() == random_mask(density).sum()


def test_long_chain():
    path = CR.serpentine(SHAPE)
    labels, sizes = check(CR.mask_of(SHAPE, path), 6)
    assert sizes.tolist() == [len(path)]
    cut = len(path) // 2
    labels, sizes = check(CR.mask_of(SHAPE, path[:cut] + path[cut + 1:]), 6)
    assert sizes.tolist() == [cut, len(path) - cut - 1]
    assert labels[path[0]] == 0 and labels[path[-1]] == 1


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_contacts_across_a_tile_corner(connectivity):
    for offset, voxels in CR.corner_contacts(components.TILE_ZYX):
        labels, sizes = label_both(dev(CR.mask_of(SHAPE, voxels)), connectivity)
        joined = CR.offset_class(offset) <= MAXC[connectivity]
        assert sizes.tolist() == ([2] if joined else [1, 1]), offset
        assert [int(labels[v]) for v in sorted(voxels)] == ([0, 0] if joined else [0, 1]), offset


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_no_wrap_at_row_and_slice_ends(connectivity):
    for voxels in CR.no_wrap_cases(SHAPE):
        labels, sizes = label_both(dev(CR.mask_of(SHAPE, voxels)), connectivity)
        assert sizes.tolist() == [1, 1]


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_degenerate_shapes(connectivity):
    labels, sizes = label_both(dev(np.zeros(SHAPE, np.uint8)), connectivity)
    assert sizes.shape == (0,) and (labels == -1).all()
    labels, sizes = label_both(dev(np.ones(SHAPE, np.uint8)), connectivity)
    assert sizes.tolist() == [int(np.prod(SHAPE))] and (labels == 0).all()
    tz, ty, tx = components.TILE_ZYX
    for shape in [(1, 1, 1), (1, SHAPE[1], 1), (tz - 3, ty - 1, tx - 5)]:
        for density in (0.0, 0.4, 1.0):
            check((np.random.default_rng(7).random(shape) < density).astype(np.uint8), connectivity)


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_batch(connectivity):
    mask = random_mask(0.25)
    want_labels, want_sizes = random_ref(0.25, connectivity)
    count = len(want_sizes)
    labels, sizes = label_both(dev(np.stack([mask, mask])), connectivity)
    assert len(sizes) == 2 * count and np.array_equal(sizes, np.concatenate([want_sizes, want_sizes]))
    assert np.array_equal(labels[0], want_labels)
    assert np.array_equal(labels[1], np.where(want_labels >= 0, want_labels + count, -1))


def test_mask_dtypes():
    mask = random_mask(0.25)
    want = random_ref(0.25, 26)
    for m in (dev(mask).bool(), dev(mask) * 200, dev(mask).bool()[:, ::1, :]):
        got = components.label_volume(m)
        assert np.array_equal(host(got.labels), want[0]) and np.array_equal(host(got.sizes), want[1])
    strided = dev(np.stack([mask, 1 - mask], -1))[..., 0]                 # not contiguous
    assert np.array_equal(host(components.label_volume(strided).labels), want[0])
    with pytest.raises(ValueError):
        components.label_volume(dev(mask), connectivity=8)
    with pytest.raises(ValueError):
        components.label_volume(dev(mask).float())                        # a float volume needs band
    with pytest.raises(_lib.SgnnError):
        components.label_volume(torch.from_numpy(mask.copy()))            # host tensor


def test_float_input():
    rng = np.random.default_rng(3)
    band = 0.06
    sdf = rng.uniform(-0.2, 0.2, SHAPE).astype(np.float32)
    special = rng.integers(0, 8, SHAPE)
    b32 = np.float32(band)
    for code, value in ((0, -np.inf), (1, np.inf), (2, np.nan), (3, b32), (4, -b32), (5, np.nextafter(b32, np.float32(1))),
                        (6, np.nextafter(-b32, np.float32(-1)))):
        sdf[special == code] = value
    fg = CR.foreground(sdf, band)
    assert fg[special == 3].all() and fg[special == 4].all() and not fg[special <= 2].any()
    assert not fg[special == 5].any() and not fg[special == 6].any() and 0 < fg[special == 7].sum() < (special == 7).sum()
    assert np.array_equal(host(components.foreground(dev(sdf), band)) != 0, fg)
    want = CR.label_volume(fg, 18)
    labels, sizes = label_both(dev(sdf), 18, band=band)
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[1])
    assert np.array_equal(labels >= 0, fg)


@pytest.mark.parametrize('connectivity', CONNECTIVITIES)
def test_sparse(connectivity):
    rng = np.random.default_rng(11)
    mask = np.stack([random_mask(0.12), random_mask(0.25)])
    locs = np.argwhere(mask)[:, [1, 2, 3, 0]]
    extra = locs[rng.permutation(len(locs))[:len(locs) // 20]]            # about 5 % of the rows twice
    locs = np.concatenate([locs, extra])
    locs = locs[rng.permutation(len(locs))]
    dense = components.label_volume(dev(mask), connectivity=connectivity)
    got = components.label_sparse(dev(locs), SHAPE, connectivity)
    again = components.label_sparse(dev(locs), SHAPE, connectivity)
    assert torch.equal(got.labels, again.labels) and torch.equal(got.sizes, again.sizes)
    assert got.labels.shape == (len(locs),) and got.labels.dtype == torch.int32
    assert np.array_equal(host(got.labels), host(dense.labels)[locs[:, 3], locs[:, 0], locs[:, 1], locs[:, 2]])
    assert torch.equal(got.sizes, dense.sizes) and int(got.sizes.sum()) == int(mask.sum())      # voxels, not rows
    want_labels, want_sizes = CR.label_sparse(locs, SHAPE, connectivity)
    assert np.array_equal(host(got.labels), want_labels) and np.array_equal(host(got.sizes), want_sizes)
    one = locs[locs[:, 3] == 0][:, :3]                                      # (N, 3): no batch column
    got3 = components.label_sparse(dev(one), SHAPE, connectivity)
    want3 = CR.label_sparse(one, SHAPE, connectivity)
    assert np.array_equal(host(got3.labels), want3[0]) and np.array_equal(host(got3.sizes), want3[1])
    for bad in ([SHAPE[0], 0, 0, 0], [0, -1, 0, 0], [0, 0, SHAPE[2], 1], [0, 0, 0, -1]):
        with pytest.raises(ValueError):
            components.label_sparse(dev(np.concatenate([locs[:5], np.array([bad])])), SHAPE, connectivity)
    empty = components.label_sparse(dev(np.zeros((0, 4), np.int64)), SHAPE, connectivity)
    assert empty.labels.shape == (0,) and empty.sizes.shape == (0,)


def check_mesh(nverts, faces):
    got = components.label_mesh(nverts, dev(faces))
    again = components.label_mesh(nverts, dev(faces))
    want = CR.label_mesh(nverts, faces)
    for g, a, w, dtype in zip(got, again, want, (torch.int32, torch.int32, torch.int64, torch.int64)):
        assert g.dtype == dtype and torch.equal(g, a)
        assert g.shape == w.shape and np.array_equal(host(g), w)
    return got


def test_mesh_strip():
    nverts, faces = CR.strip_mesh(5000, 5)
    got = check_mesh(nverts, faces)
    assert got.face_sizes.tolist() == [5000] and got.vertex_sizes.tolist() == [5002]


def test_mesh_clusters():
    nverts, faces = CR.cluster_mesh(40, 100, 9)
    got = check_mesh(nverts, faces)
    assert len(got.face_sizes) >= 40 and int((got.vertex_labels == -1).sum()) >= 100
    got64 = components.label_mesh(torch.zeros(nverts, 3), dev(faces.astype(np.int64)))       # (V, 3) array, int64 faces
    assert all(torch.equal(a, b) for a, b in zip(got, got64))


def test_mesh_small_cases():
    got = check_mesh(5, np.array([[0, 1, 2], [2, 3, 4]], np.int32))                           # bow-tie
    assert got.face_sizes.tolist() == [2] and got.vertex_labels.tolist() == [0] * 5
    got = check_mesh(4, np.zeros((0, 3), np.int32))                                           # F == 0
    assert got.face_labels.shape == (0,) and got.vertex_labels.tolist() == [-1] * 4
    assert got.face_sizes.shape == (0,) and got.vertex_sizes.shape == (0,)
    got = check_mesh(0, np.zeros((0, 3), np.int32))
    assert got.vertex_labels.shape == (0,)


def test_mesh_bad_index_is_an_error_not_an_access():
    nverts, faces = CR.cluster_mesh(6, 3, 2)
    for bad in (nverts, -1):
        broken = faces.copy()
        broken[len(broken) // 2, 1] = bad
        with pytest.raises(_lib.SgnnError):
            components.label_mesh(nverts, dev(broken))
        with pytest.raises(_lib.SgnnError):
            components.label_mesh(nverts, dev(broken.astype(np.int64)))
        check_mesh(nverts, faces)                                                             # the process is healthy


def test_filter_sparse():
    rng = np.random.default_rng(21)
    mask = random_mask(0.25)
    locs = np.argwhere(mask)
    locs = locs[rng.permutation(len(locs))]
    vals = rng.standard_normal((len(locs), 1)).astype(np.float32)
    ref_labels, ref_sizes = CR.label_sparse(locs, SHAPE, 18)
    for kw in (dict(min_size=4), dict(keep_largest=3), dict(min_size=30, keep_largest=5), dict()):
        out_locs, out_vals, rows = components.filter_sparse(dev(locs), dev(vals), SHAPE, connectivity=18, **kw)
        want_rows = np.flatnonzero(CR.select(ref_sizes, **kw)[ref_labels])
        assert rows.dtype == torch.int64 and np.array_equal(host(rows), want_rows)           # ascending: original order
        assert np.array_equal(host(out_locs), locs[want_rows]) and np.array_equal(host(out_vals), vals[want_rows])
    kept = CR.select(ref_sizes, min_size=30, keep_largest=5)
    assert 0 < kept.sum() < 5                     # at this density both criteria bite: fewer than 5 reach 30 voxels


def test_filter_volume():
    rng = np.random.default_rng(22)
    band = 0.5
    sdf = rng.uniform(-1.0, 1.0, SHAPE).astype(np.float32) * np.where(rng.random(SHAPE) < 0.35, 0.4, 3.0).astype(np.float32)
    sdf[rng.random(SHAPE) < 0.05] = -np.inf
    sdf[rng.random(SHAPE) < 0.01] = np.nan
    fg = CR.foreground(sdf, band)
    ref_labels, ref_sizes = CR.label_volume(fg, 6)
    x = dev(sdf)
    before = x.clone()
    for kw, fill in ((dict(min_size=5), -np.inf), (dict(keep_largest=2), 7.0), (dict(min_size=3, keep_largest=40), -np.inf)):
        out = components.filter_volume(x, band, connectivity=6, fill=fill, **kw)
        assert torch.equal(x.view(torch.int32), before.view(torch.int32))                     # the input is untouched
        keep = CR.select(ref_sizes, **kw)
        dropped = fg & ~keep[np.maximum(ref_labels, 0)]
        assert 0 < dropped.sum() < fg.sum()
        want = sdf.copy()
        want[dropped] = fill
        assert np.array_equal(host(out).view(np.int32), want.view(np.int32))


def test_filter_mesh():
    nverts, faces = CR.cluster_mesh(40, 100, 9)
    rng = np.random.default_rng(23)
    verts = rng.standard_normal((nverts, 3)).astype(np.float32)
    colors = rng.integers(0, 256, (nverts, 3)).astype(np.uint8)
    face_labels, vertex_labels, face_sizes, _ = CR.label_mesh(nverts, faces)
    for kw in (dict(min_size=20), dict(keep_largest=4), dict(min_size=25, keep_largest=30), dict(min_size=25, keep_largest=10),
               dict(keep_largest=0)):
        keep = CR.select(face_sizes, **kw)
        out_v, out_f, out_c = components.filter_mesh(dev(verts), dev(faces), dev(colors), **kw)
        assert out_v.dtype == torch.float32 and out_f.dtype == torch.int32 and out_c.dtype == torch.uint8
        kept_faces = np.flatnonzero(keep[face_labels])
        kept_verts = np.flatnonzero((vertex_labels >= 0) & keep[np.maximum(vertex_labels, 0)])
        assert out_f.shape == (len(kept_faces), 3) and out_v.shape == (len(kept_verts), 3)
        assert np.array_equal(host(out_v), verts[kept_verts]) and np.array_equal(host(out_c), colors[kept_verts])
        assert np.array_equal(host(out_v)[host(out_f).astype(np.int64)], verts[faces[kept_faces]])   # corners, in order
        again = components.label_mesh(out_v, out_f)
        assert int((again.vertex_labels == -1).sum()) == 0                                    # no unused vertex
        assert again.face_sizes.tolist() == face_sizes[keep].tolist()                         # exactly the kept ones
    assert 0 < CR.select(face_sizes, min_size=25, keep_largest=30).sum() < min(30, (face_sizes >= 25).sum() + 1)
    assert CR.select(face_sizes, min_size=25).sum() < 30                                      # so min_size bites there
    assert CR.select(face_sizes, min_size=25, keep_largest=10).sum() == 10                    # and keep_largest here
    two = components.filter_mesh(dev(verts), dev(faces), keep_largest=1)
    assert len(two) == 2 and two[1].shape[0] == int(face_sizes.max())


@functools.lru_cache(maxsize=None)
def spheres():
    """48^3 sdf in voxels, truncated at 3: two separate spheres of radius 10 and 2, and the large one alone."""
    z, y, x = np.meshgrid(*(np.arange(48, dtype=np.float32),) * 3, indexing='ij')

    def sphere(c, r):
        return np.sqrt((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2).astype(np.float32) - np.float32(r)
    big, small = sphere((20.3, 20.6, 20.1), 10), sphere((40.2, 39.7, 40.4), 2)
    return np.minimum(big, small), big


def mesh_of(sdf):
    return mc.run_marching_cubes(sdf, None, 0.0, 3.0, 10.0)


def test_end_to_end_two_spheres():
    both, big = (dev(a) for a in spheres())
    verts, colors, faces = mesh_of(both)
    alone = mesh_of(big)
    lab = components.label_mesh(verts, faces)
    assert len(lab.face_sizes) == 2 and int(lab.face_sizes.sum()) == faces.shape[0]
    assert lab.face_sizes[0] == alone[2].shape[0] > lab.face_sizes[1] > 0                     # the large sphere comes first
    out_v, out_f, out_c = components.filter_mesh(verts, faces, colors, keep_largest=1)
    assert out_f.shape[0] == alone[2].shape[0] and out_v.shape[0] == alone[0].shape[0]
    assert torch.equal(out_v[out_f.long()], alone[0][alone[2].long()])
    vol = components.label_volume(both, band=1.5)
    assert len(vol.sizes) == 2
    cleaned = components.filter_volume(both, 1.5, keep_largest=1)
    v2, _, f2 = mesh_of(cleaned)
    lab2 = components.label_mesh(v2, f2)
    assert len(lab2.face_sizes) == 1 and f2.shape[0] == alone[2].shape[0]
