"""The host restatement of sgnn_amd.smooth (tests/smooth_ref.py) held to ground truth that
needs no device: exact invariance of a flat patch, shrinkage and noise removal on a sphere, kept edges on a cube, and
the adjacency of one hand-written mesh.  No GPU."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_ref as SR  # noqa: E402

F32 = np.float32


def test_flat_patch_is_invariant():
    """All sums are exact on multiples of 0.25 at z = 2: an interior vertex keeps z bit for bit, under every call."""
    verts, faces = SR.flat_patch(6, 5, z=2.0, pitch=0.25)
    adj = SR.adjacency(faces, len(verts))
    inner = adj.kind == SR.INTERIOR
    assert inner.sum() == 5 * 4 and (adj.kind[~inner] == SR.BOUNDARY).all()
    for out in (SR.laplacian(verts, faces, 5), SR.taubin(verts, faces, 10), SR.denoise(verts, faces),
                SR.laplacian(verts, faces, 3, boundary='free'), SR.laplacian(verts, faces, 3, boundary='fixed')):
        assert out.dtype == F32 and out.shape == verts.shape
        assert np.array_equal(out[inner, 2].view(np.int32), verts[inner, 2].view(np.int32))
    assert np.array_equal(SR.face_normals(verts, faces), np.tile(F32([0, 0, 1]), (len(faces), 1)))
    assert np.array_equal(SR.vertex_normals(verts, faces), np.tile(F32([0, 0, 1]), (len(verts), 1)))
    # 'curve' keeps the rim on its lines: in one step a vertex inside a straight side moves along the side only (the
    # corners round off, so later steps pull their neighbours after them)
    side = (verts[:, 0] == 0) & (verts[:, 1] > 0) & (verts[:, 1] < 1.25)
    assert side.sum() == 4 and (SR.laplacian(verts, faces, 1, boundary='curve')[side, 0] == 0).all()
    assert (SR.laplacian(verts, faces, 1, boundary='free')[side, 0] > 0).all()


@functools.lru_cache(maxsize=None)
def sphere():
    verts, faces = SR.icosphere(3)
    assert len(verts) == 642 and len(faces) == 1280
    return verts, faces


def test_taubin_shrinks_less_than_laplacian():
    verts, faces = sphere()
    v0 = SR.enclosed_volume(verts, faces)
    adj = SR.adjacency(faces, len(verts))
    assert (adj.kind == SR.INTERIOR).all()
    lap = SR.enclosed_volume(SR.laplacian(verts, adj, 50), faces) / v0
    tau = SR.enclosed_volume(SR.taubin(verts, adj), faces) / v0
    print('enclosed volume after laplacian(50): %.4f of the input, after taubin(10): %.4f' % (lap, tau))
    assert lap < 1.0 and lap < tau


def radial_rms(x):
    return float(np.sqrt(np.mean((np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1) - 1.0) ** 2)))


def test_noise_removal_on_a_sphere():
    verts, faces = sphere()
    noise = np.random.default_rng(17).standard_normal(len(verts))
    noisy = (verts.astype(np.float64) * (1.0 + 0.02 * noise)[:, None]).astype(F32)
    before = radial_rms(noisy)
    tau, den = radial_rms(SR.taubin(noisy, faces, 10)), radial_rms(SR.denoise(noisy, faces))
    print('RMS radial error: input %.5f, taubin(10) %.5f, denoise() %.5f' % (before, tau, den))
    assert tau < before and den < before


def test_denoise_keeps_the_edges_of_a_cube():
    """The reason denoise exists: the filtered normals do not mix across a sharp edge, the umbrella does."""
    verts, faces, on_edge = SR.cube_surface(8)
    assert on_edge.sum() == 12 * 7 + 8
    noisy = (verts + 0.01 * np.random.default_rng(23).standard_normal(verts.shape)).astype(F32)
    before = SR.cube_edge_distance(noisy[on_edge]).mean()
    tau = SR.cube_edge_distance(SR.taubin(noisy, faces, 10)[on_edge]).mean()
    den = SR.cube_edge_distance(SR.denoise(noisy, faces)[on_edge]).mean()
    print('mean distance of the edge vertices to the edge lines: input %.5f, taubin(10) %.5f, denoise() %.5f'
          % (before, tau, den))
    assert den < tau


def test_kinds():
    verts, faces = SR.kinds_mesh()
    adj = SR.adjacency(faces, len(verts))
    assert adj.kind.tolist() == SR.KINDS_KIND
    assert adj.start.tolist() == np.concatenate([[0], np.cumsum([len(n) for n in SR.KINDS_NEIGHBOR])]).tolist()
    assert adj.neighbor.tolist() == sum(SR.KINDS_NEIGHBOR, [])
    assert adj.mult.tolist() == sum(SR.KINDS_MULT, [])
    assert SR.boundary_edges(adj).tolist() == [list(e) for e in SR.KINDS_BOUNDARY_EDGES]
    for boundary in SR.BOUNDARIES:
        out = SR.taubin(verts, faces, 3, boundary=boundary)
        still = np.isin(adj.kind, (SR.ISOLATED, SR.NONMANIFOLD))
        assert np.array_equal(out[still].view(np.int32), verts[still].view(np.int32))
        moved = (out != verts).any(1)
        assert moved[adj.kind == SR.INTERIOR].all()
        assert moved[adj.kind == SR.BOUNDARY].all() == (boundary != 'fixed')
    fixed = np.zeros(len(verts), dtype=bool)
    fixed[[1, 5]] = True
    out = SR.denoise(verts, faces, 2, 3, fixed=fixed)
    assert np.array_equal(out[[1, 5, 8, 9, 13]].view(np.int32), verts[[1, 5, 8, 9, 13]].view(np.int32))
    many = np.tile(np.int32([[0, 1, 2]]), (300, 1))
    assert SR.adjacency(many, 3).mult.tolist() == [255] * 6
