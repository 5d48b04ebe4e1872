"""sgnn_amd.smooth on the GPU against the host restatement tests/smooth_ref.py: every
array of the adjacency equal, every vertex and normal equal bit for bit (compared as int32); every call runs twice, the
runs are equal and the inputs come back unchanged."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_ref as SR  # noqa: E402

from sgnn_amd import _lib, marching_cubes as mc, smooth  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == F32
    return np.ascontiguousarray(x).view(np.int32)


def same(got, want, what=''):
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g, w = bits(got), bits(want)
    differ = np.nonzero((g != w).reshape(len(w), -1).any(1))[0]
    assert len(differ) == 0, '%s: %d of %d rows differ, first %d: %r against %r' % (
        what, len(differ), len(w), differ[0], got[int(differ[0])].cpu().numpy(), want[differ[0]])


def run(fn, *args, **kw):
    """fn twice: the two results hold the same bits and the array arguments are unchanged."""
    arrays = [a for a in list(args) + list(kw.values()) if isinstance(a, np.ndarray) or torch.is_tensor(a)]
    before = [a.clone() if torch.is_tensor(a) else a.copy() for a in arrays]
    a, b = fn(*args, **kw), fn(*args, **kw)
    assert a.data_ptr() != b.data_ptr() or a.numel() == 0
    assert np.array_equal(bits(a), bits(b)), 'two runs differ'
    for x, y in zip(arrays, before):
        assert torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert not torch.is_tensor(x) or x.data_ptr() != a.data_ptr()
    return a


def check_all(verts, faces, boundary='curve', fixed=None, what=''):
    """Every public call against the restatement on one mesh."""
    adj = smooth.Adjacency(faces, len(verts))
    same(run(smooth.taubin, verts, adj, 10, boundary=boundary, fixed=fixed),
         SR.taubin(verts, faces, 10, boundary=boundary, fixed=fixed), what + ' taubin(10)')
    same(run(smooth.laplacian, verts, faces, 3, lam=0.63, boundary=boundary, fixed=fixed),
         SR.laplacian(verts, faces, 3, lam=0.63, boundary=boundary, fixed=fixed), what + ' laplacian(3)')
    same(run(smooth.face_normals, verts, faces), SR.face_normals(verts, faces), what + ' face_normals')
    same(run(smooth.vertex_normals, verts, faces), SR.vertex_normals(verts, faces), what + ' vertex_normals')
    same(run(smooth.denoise, verts, faces, 3, 5, adj=adj, fixed=fixed), SR.denoise(verts, faces, 3, 5, fixed=fixed),
         what + ' denoise(3, 5)')
    return adj


def check_adjacency(adj, want):
    assert adj.start.dtype == torch.int64 and adj.neighbor.dtype == torch.int32
    assert adj.mult.dtype == torch.uint8 and adj.kind.dtype == torch.uint8
    assert np.array_equal(adj.start.cpu().numpy(), want.start)
    assert np.array_equal(adj.neighbor.cpu().numpy(), want.neighbor)
    assert np.array_equal(adj.mult.cpu().numpy(), want.mult)
    assert np.array_equal(adj.kind.cpu().numpy(), want.kind)
    edges = adj.boundary_edges()
    assert edges.dtype == torch.int32 and np.array_equal(edges.cpu().numpy(), SR.boundary_edges(want))


@functools.lru_cache(maxsize=None)
def sphere():
    """The project's own marching-cubes mesh of a sphere in a noisy 24^3 distance volume; voxel units."""
    z, y, x = np.meshgrid(*(np.arange(24, dtype=np.float64),) * 3, indexing='ij')
    sdf = np.sqrt((x - 11.3) ** 2 + (y - 11.7) ** 2 + (z - 12.1) ** 2) - 8.4
    sdf += 0.2 * np.random.default_rng(7).standard_normal(sdf.shape)
    colors = np.zeros((24, 24, 24, 3), dtype=np.uint8)
    v, _, f = mc.run_marching_cubes(torch.from_numpy(sdf.astype(F32)).cuda(), torch.from_numpy(colors).cuda(), 0.0, 3.0,
                                    10.0)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert len(v) > 1000 and len(f) > 2000 and len(v) % 256 != 0
    for a in (v, f):
        a.setflags(write=False)
    return v, f


def test_every_kind():
    verts, faces = SR.kinds_mesh()
    want = SR.adjacency(faces, len(verts))
    assert want.kind.tolist() == SR.KINDS_KIND
    still = np.isin(want.kind, (SR.ISOLATED, SR.NONMANIFOLD))
    for boundary in smooth.BOUNDARIES:
        adj = check_all(verts, faces, boundary=boundary, what=boundary)
        check_adjacency(adj, want)
        for out in (smooth.taubin(verts, adj, 4, boundary=boundary), smooth.laplacian(verts, adj, 4, boundary=boundary),
                    smooth.denoise(verts, faces, adj=adj)):
            assert np.array_equal(bits(out)[still], bits(verts)[still])
    assert np.array_equal(bits(smooth.laplacian(verts, faces, 2, boundary='fixed'))[want.kind == SR.BOUNDARY],
                          bits(verts)[want.kind == SR.BOUNDARY])
    many = np.tile(np.int32([[0, 1, 2]]), (300, 1))
    check_adjacency(smooth.Adjacency(many, 4), SR.adjacency(many, 4))


def test_tetrahedron():
    verts = np.random.default_rng(1).uniform(-1, 1, (4, 3)).astype(F32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=np.int32)
    adj = check_all(verts, faces)
    check_adjacency(adj, SR.adjacency(faces, 4))
    assert adj.kind.tolist() == [smooth.INTERIOR] * 4 and adj.boundary_edges().shape == (0, 2)


def test_open_patch_with_a_curve_boundary():
    verts, faces = SR.flat_patch(5, 4, z=0.0, pitch=0.3)
    verts = (verts + 0.05 * np.random.default_rng(2).standard_normal(verts.shape)).astype(F32)
    for boundary in smooth.BOUNDARIES:
        adj = check_all(verts, faces, boundary=boundary, what=boundary)
    check_adjacency(adj, SR.adjacency(faces, len(verts)))
    assert adj.boundary_edges().shape == (2 * (5 + 4), 2)
    flat, _ = SR.flat_patch(6, 5, z=2.0, pitch=0.25)
    inner = SR.adjacency(SR.grid_faces(6, 5), len(flat)).kind == SR.INTERIOR
    for out in (smooth.taubin(flat, SR.grid_faces(6, 5)), smooth.denoise(flat, SR.grid_faces(6, 5))):
        assert np.array_equal(bits(out)[inner, 2], bits(flat)[inner, 2])


def test_fan_of_seventy():
    """A valence above the 64 lanes of a wavefront changes nothing: one lane still walks the whole list in order."""
    verts, faces = SR.fan(70)
    adj = check_all(verts, faces)
    assert int(adj.start[1] - adj.start[0]) == 70 and adj.kind.tolist() == [smooth.INTERIOR] + [smooth.BOUNDARY] * 70
    check_all(verts, faces, boundary='free', what='free')


def test_marching_cubes_sphere():
    verts, faces = sphere()
    adj = check_all(verts, faces)
    check_adjacency(adj, SR.adjacency(faces, len(verts)))


def test_one_vertex_past_a_block():
    verts, faces = sphere()
    faces = faces[(faces < 257).all(1)][:257]
    verts = verts[:257]
    assert 64 < len(faces) <= 257
    adj = check_all(verts, faces)
    check_adjacency(adj, SR.adjacency(faces, 257))


def test_padded_rows_give_the_same_bits(monkeypatch):
    verts, faces = sphere()
    want = bits(smooth.taubin(verts, faces, 3))
    monkeypatch.setattr(smooth, 'ROW_FLOATS', 4)
    got = run(smooth.taubin, verts, faces, 3)
    assert got.shape == (len(verts), 3) and got.is_contiguous() and np.array_equal(bits(got), want)


@pytest.mark.parametrize('nv', [0, 5])
def test_no_faces(nv):
    verts = np.random.default_rng(1).random((nv, 3)).astype(F32)
    faces = np.zeros((0, 3), np.int32)
    adj = smooth.Adjacency(faces, nv)
    check_adjacency(adj, SR.adjacency(faces, nv))
    assert adj.kind.tolist() == [smooth.ISOLATED] * nv and adj.neighbor.shape == (0,) and adj.start.shape == (nv + 1,)
    for out in (run(smooth.laplacian, verts, adj), run(smooth.taubin, verts, faces), run(smooth.denoise, verts, faces)):
        assert out.shape == (nv, 3) and np.array_equal(bits(out), bits(verts))
    assert smooth.face_normals(verts, faces).shape == (0, 3)
    vn = smooth.vertex_normals(verts, faces)
    assert vn.shape == (nv, 3) and not bool(vn.any())


def test_fixed_vertices_stay():
    verts, faces = sphere()
    fixed = np.random.default_rng(3).random(len(verts)) < 0.4
    adj = smooth.Adjacency(faces, len(verts))
    for out, want in ((run(smooth.taubin, verts, adj, 4, fixed=fixed), SR.taubin(verts, faces, 4, fixed=fixed)),
                      (run(smooth.denoise, verts, faces, 2, 3, fixed=torch.from_numpy(fixed).cuda()),
                       SR.denoise(verts, faces, 2, 3, fixed=fixed))):
        same(out, want)
        assert np.array_equal(bits(out)[fixed], bits(verts)[fixed])
        assert (bits(out)[~fixed] != bits(verts)[~fixed]).any()


def test_no_iterations_is_a_copy():
    verts, faces = sphere()
    dv = torch.from_numpy(verts).cuda()
    for out in (run(smooth.laplacian, dv, faces, 0), run(smooth.taubin, dv, faces, iterations=0),
                run(smooth.denoise, dv, faces, 3, 0)):
        assert out.data_ptr() != dv.data_ptr() and torch.equal(out, dv)


def test_status_words_raise():
    verts, faces = sphere()
    adj = smooth.Adjacency(faces, len(verts))
    for value in (np.nan, np.inf):
        broken = verts.copy()
        broken[len(verts) - 3, 1] = value
        for call in (lambda: smooth.laplacian(broken, adj), lambda: smooth.taubin(broken, faces, 2),
                     lambda: smooth.denoise(broken, faces, 1, 2)):
            with pytest.raises(_lib.SgnnError, match='not finite'):
                call()
        with pytest.raises(SR.RangeError):
            SR.taubin(broken, faces, 1)
    broken = faces.copy()
    broken[5, 2] = len(verts)
    for f in (broken, torch.from_numpy(broken.astype(np.int64)).cuda()):
        for call in (lambda: smooth.Adjacency(f, len(verts)), lambda: smooth.laplacian(verts, f),
                     lambda: smooth.face_normals(verts, f), lambda: smooth.vertex_normals(verts, f),
                     lambda: smooth.denoise(verts, f), lambda: smooth.denoise(verts, f, adj=adj)):
            with pytest.raises(_lib.SgnnError, match='face index'):
                call()
    with pytest.raises(SR.RangeError):
        SR.adjacency(broken, len(verts))
    with pytest.raises(ValueError):
        smooth.laplacian(verts[:-1], adj)
    same(smooth.taubin(verts, adj, 2), SR.taubin(verts, faces, 2))       # and the device is as good as before


def test_numpy_host_and_device_inputs_agree():
    verts, faces = sphere()
    forms = [(verts, faces), (torch.from_numpy(verts.copy()), torch.from_numpy(faces.copy())),
             (torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()),
             (verts.astype(np.float64), torch.from_numpy(faces.astype(np.int64)).cuda())]
    want = None
    for v, f in forms:
        got = [bits(run(smooth.taubin, v, f, 2)), bits(run(smooth.denoise, v, f, 1, 2)),
               bits(run(smooth.vertex_normals, v, f)), bits(run(smooth.face_normals, v, f))]
        want = want or got
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
