"""sgnn_amd.simplify on the GPU against the host restatement tests/simplify_ref.py: faces,
maps and colours equal, vertices equal bit for bit, for both placements; every case runs twice and the runs are equal."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as SR  # noqa: E402

from sgnn_amd import _lib, components, marching_cubes as mc, meshdist, simplify  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


def host(t):
    return None if t is None else t.cpu().numpy()


def run(verts, faces, cell, **kw):
    """simplify.cluster twice; the two results must be the same tensors bit for bit."""
    a = simplify.cluster(verts, faces, cell, **kw)
    b = simplify.cluster(verts, faces, cell, **kw)
    for x, y in zip(a, b):
        assert (x is None and y is None) or (x.is_cuda and torch.equal(x, y)), 'two runs differ'
    assert torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32))
    assert a.verts.dtype == torch.float32 and a.faces.dtype == torch.int32
    assert a.vertex_map.dtype == torch.int32 and a.face_map.dtype == torch.int32
    return a


def check(verts, faces, cell, colors=None, origin=None):
    """Both placements against the restatement; returns the 'quadric' result."""
    out = None
    for placement in ('mean', 'quadric'):
        want = SR.cluster(verts, faces, cell, colors=colors, placement=placement, origin=origin)
        out = run(verts, faces, cell, colors=colors, placement=placement, origin=origin)
        assert tuple(out.verts.shape) == want.verts.shape and tuple(out.faces.shape) == want.faces.shape
        assert np.array_equal(host(out.faces), want.faces)
        assert np.array_equal(host(out.vertex_map), want.vertex_map)
        assert np.array_equal(host(out.face_map), want.face_map)
        got_bits, want_bits = host(out.verts).view(np.int32), want.verts.view(np.int32)
        differ = np.nonzero((got_bits != want_bits).any(1))[0]
        assert len(differ) == 0, '%s: %d of %d vertices differ, first %d: %r against %r' % (
            placement, len(differ), len(want_bits), differ[0], host(out.verts)[differ[0]], want.verts[differ[0]])
        if colors is None:
            assert out.colors is None
        else:
            assert out.colors.dtype == torch.uint8 and np.array_equal(host(out.colors), want.colors)
    return out


@functools.lru_cache(maxsize=None)
def sphere():
    """The project's own marching-cubes mesh of a sphere in a 24^3 distance volume, with random colours; voxel units."""
    z, y, x = np.meshgrid(*(np.arange(24, dtype=np.float64),) * 3, indexing='ij')
    sdf = np.sqrt((x - 11.3) ** 2 + (y - 11.7) ** 2 + (z - 12.1) ** 2) - 8.4
    colors = np.random.default_rng(7).integers(0, 256, (24, 24, 24, 3), dtype=np.uint8)
    v, c, f = mc.run_marching_cubes(torch.from_numpy(sdf.astype(F32)).cuda(), torch.from_numpy(colors).cuda(), 0.0, 3.0,
                                    10.0)
    v, c, f = host(v), host(c), host(f)
    assert len(v) > 1000 and len(f) > 2000
    for a in (v, c, f):
        a.setflags(write=False)
    return v, c, f


def test_tilted_plane():
    verts, faces, _, _ = SR.tilted_plane(12)
    out = check(verts, faces, 0.21)
    assert 10 < out.verts.shape[0] < len(verts)


def test_cube():
    verts, faces = SR.cube_surface(8)
    out = check(verts, faces, 2.5 / 8)
    assert 8 < out.verts.shape[0] <= 4 ** 3 - 2 ** 3        # cells of the 4 x 4 x 4 grid that touch the surface


@pytest.mark.parametrize('cell', [1.5, 3.0, 7.0])
def test_sphere_with_colours(cell):
    v, c, f = sphere()
    out = check(v, f, cell, colors=c)
    assert 0 < out.faces.shape[0] < len(f)


def test_inputs_on_the_device_and_int64_faces():
    v, c, f = sphere()
    want = SR.cluster(v, f, 3.0, colors=c)
    out = run(torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int64)).cuda(), 3.0,
              colors=torch.from_numpy(c).cuda())
    assert np.array_equal(host(out.verts).view(np.int32), want.verts.view(np.int32))
    assert np.array_equal(host(out.faces), want.faces) and np.array_equal(host(out.colors), want.colors)


def test_every_vertex_alone():
    """A cell near the weld distance of marching cubes, the smallest the 2^21 cells per axis allow here: the vertices
    come back bit for bit, the faces without their degenerates and duplicates (there are none in a cleaned mesh)."""
    v, c, f = sphere()
    out = check(v, f, 1.2e-5, colors=c)
    assert np.array_equal(host(out.verts).view(np.int32), v.view(np.int32))
    assert np.array_equal(host(out.colors), c)
    assert np.array_equal(host(out.faces), f[SR.kept_faces(f.astype(np.int64))])
    assert np.array_equal(host(out.vertex_map), np.arange(len(v)))


def test_cell_larger_than_the_mesh():
    v, c, f = sphere()
    out = check(v, f, 100.0, colors=c)
    assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3) and out.colors.shape == (0, 3)
    assert out.face_map.shape == (0,) and bool((out.vertex_map == -1).all()) and out.vertex_map.shape == (len(v),)


@pytest.mark.parametrize('nv,nf', [(0, 0), (5, 0), (1, 0)])
def test_empty_mesh(nv, nf):
    verts = np.random.default_rng(1).random((nv, 3)).astype(F32)
    out = check(verts, np.zeros((nf, 3), np.int32), 0.25, colors=np.zeros((nv, 3), np.uint8))
    assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3) and out.vertex_map.shape == (nv,)


def test_one_vertex():
    out = check(np.array([[0.5, 1.0, 2.0]], F32), np.array([[0, 0, 0]], np.int32), 0.25)
    assert out.verts.shape == (0, 3) and host(out.vertex_map).tolist() == [-1]


def messy_mesh():
    rng = np.random.default_rng(11)
    n = 9
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    grid = np.stack([i.reshape(-1), j.reshape(-1), np.zeros(i.size)], 1) + rng.uniform(-0.2, 0.2, (i.size, 3))
    verts = np.concatenate([grid, rng.uniform(0, n, (31, 3)),                 # vertices that no face uses
                            [[1.0, 1.0, 5.0], [3.0, 3.0, 5.0], [5.0, 5.0, 5.0]]]).astype(F32)      # three on a line
    base = SR.grid_faces(n, n)
    k = len(verts)
    faces = np.concatenate([base, base[10:30], base[40:70][:, ::-1], base[5:9][:, [1, 2, 0]],      # repeats, flips
                            [[3, 3, 17], [8, 20, 8], [4, 4, 4]],                                    # repeated indices
                            [[k - 3, k - 2, k - 1]], base[:3]]).astype(np.int32)                    # zero area
    assert len(verts) % 64 != 0
    return verts, faces


def test_repeated_flipped_degenerate_and_unused():
    verts, faces = messy_mesh()
    colors = np.random.default_rng(2).integers(0, 256, verts.shape, dtype=np.uint8)
    for cell in (0.01, 0.9, 2.3):
        check(verts, faces, cell, colors=colors)
    out = check(verts, faces, 0.01)
    k = len(verts)
    zero_area = int(np.nonzero((faces == [k - 3, k - 2, k - 1]).all(1))[0][0])
    assert zero_area in host(out.face_map).tolist()                   # it has three clusters, so it stays
    assert (host(out.vertex_map)[len(verts) - 34:len(verts) - 3] == -1).all()


def test_bad_face_index_raises_and_the_rest_still_works():
    verts, faces = messy_mesh()
    for bad in (-1, len(verts)):
        broken = faces.copy()
        broken[7, 1] = bad
        with pytest.raises(_lib.SgnnError, match='face index'):
            simplify.cluster(verts, broken, 0.9)
        with pytest.raises(_lib.SgnnError, match='face index'):
            simplify.cluster(verts, torch.from_numpy(broken.astype(np.int64)).cuda(), 0.9, placement='mean')
        with pytest.raises(_lib.SgnnError, match='face index'):
            simplify.cell_for_faces(verts, broken, 10)
    check(verts, np.delete(faces, 7, axis=0), 0.9)


def test_bad_coordinates_raise():
    verts, faces = messy_mesh()
    for value in (np.inf, -np.inf, np.nan):
        broken = verts.copy()
        broken[13, 2] = value
        with pytest.raises(_lib.SgnnError, match='vertex'):
            simplify.cluster(broken, faces, 0.9)
        with pytest.raises(SR.RangeError):
            SR.cluster(broken, faces, 0.9)
    with pytest.raises(_lib.SgnnError, match='vertex'):
        simplify.cluster(verts, faces, 0.9, origin=verts.min(0) + F32(1.0))      # negative cell indices
    with pytest.raises(_lib.SgnnError, match='vertex'):
        simplify.cluster(verts, faces, 1e-6)                                       # cell indices of 2^21 and more
    check(verts, faces, 0.9, origin=verts.min(0) - F32(0.37))
    check(verts, faces, 0.9)


def test_many_small_clusters():
    """More than 2^16 clusters of one to four vertices: 330 x 330 vertices, cells of 1.2 spacings."""
    n = 329
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    rng = np.random.default_rng(5)
    verts = np.stack([i.reshape(-1), j.reshape(-1), 3.0 * np.sin(i.reshape(-1) / 17.0)], 1)
    verts = (verts + rng.uniform(-0.1, 0.1, verts.shape)).astype(F32)
    out = check(verts, SR.grid_faces(n, n), 1.2)
    assert out.verts.shape[0] > 2 ** 16


def test_one_cluster_with_thousands_of_corners():
    """A 40 x 40-quad patch inside one cell (9 600 corners), held by two faces that reach three other cells."""
    n = 40
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    rng = np.random.default_rng(9)
    patch = np.stack([0.1 + 0.8 * i.reshape(-1) / n, 0.1 + 0.8 * j.reshape(-1) / n, 0.5 + 0.0 * i.reshape(-1)], 1)
    patch[:, 2] += 0.2 * np.sin(7.0 * patch[:, 0]) + rng.uniform(-0.003, 0.003, len(patch))
    far = np.array([[3.5, 0.5, 0.2], [0.5, 3.5, 0.7], [3.3, 3.4, 1.6]])
    verts = np.concatenate([patch, far]).astype(F32)
    k = len(patch)
    faces = np.concatenate([SR.grid_faces(n, n), [[0, k, k + 1], [k + 2, k + 1, k]]]).astype(np.int32)
    colors = rng.integers(0, 256, verts.shape, dtype=np.uint8)
    out = check(verts, faces, 1.0, colors=colors, origin=np.zeros(3, F32))
    assert out.verts.shape[0] == 4 and out.faces.shape[0] == 2
    assert int((out.vertex_map == 0).sum()) == k and 3 * 2 * n * n + 1 > 4096


def test_end_to_end_distance_and_components():
    """1.5 sqrt(3) cells is the bound that follows from rule 5's guard for the distance to a member of the cluster,
    and a member is a point of the original surface."""
    v, c, f = sphere()
    cell = 3.0
    out = run(v, f, cell, colors=c)
    d, _ = meshdist.TriangleIndex(v, f).distance(out.verts)
    worst = float(d.max())
    print('largest distance of a simplified vertex to the original mesh: %.4f cells' % (worst / cell))
    assert worst <= 1.5 * math.sqrt(3.0) * cell
    lab = components.label_mesh(out.verts, out.faces)
    assert lab.face_sizes.shape[0] == 1 and int(lab.face_sizes[0]) == out.faces.shape[0]


def test_cell_for_faces():
    v, c, f = sphere()
    target = 400
    cell = simplify.cell_for_faces(v, f, target)
    assert cell == float(F32(cell)) and cell > 0
    n_at, n_twice = simplify.cluster(v, f, cell).faces.shape[0], simplify.cluster(v, f, 2 * cell).faces.shape[0]
    print('cell %.5f keeps %d faces, twice the cell %d (target %d of %d)' % (cell, n_at, n_twice, target, len(f)))
    assert n_at >= target > n_twice
    assert simplify.count_faces(v, f, cell) == n_at == SR.count_faces(v, f, cell)
    assert simplify.cell_for_faces(v, f, target, lo=0.5, hi=16.0, iters=12) == SR.cell_for_faces(v, f, target, lo=0.5,
                                                                                                 hi=16.0, iters=12)
    assert simplify.cell_for_faces(v, f, 0) == simplify.cell_for_faces(v, f, 0, iters=0)       # hi itself is enough
    with pytest.raises(ValueError):
        simplify.cell_for_faces(v, f, len(f) + 1)
