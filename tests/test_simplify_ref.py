"""The NumPy restatement of INTEGRATION.md section K (tests/simplify_ref.py) is right on its own terms, whatever the
kernels do: its solve against numpy.linalg, planes, edges and corners kept, the cell guard, and the maps.  No GPU."""
import numpy as np
import pytest

import simplify_ref as ref

F32, F64 = np.float32, np.float64


def bumpy_sheet(n=20, seed=3):
    """An n x n-quad height field with noise in all three coordinates: nothing planar, nothing degenerate."""
    rng = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    pts = np.stack([i.reshape(-1) / n, j.reshape(-1) / n, 0.2 * np.sin(5.0 * i.reshape(-1) / n)], 1)
    return (pts + rng.uniform(-0.01, 0.01, pts.shape)).astype(F32), ref.grid_faces(n, n)


def _sums(verts, faces, cell):
    c, origin = ref.cells(verts, cell)
    vcluster, first = ref.clusters(c)
    return ref.cluster_sums(verts, faces.astype(np.int64), vcluster, first, origin, cell), vcluster


def test_solve_agrees_with_numpy_linalg():
    verts, faces = bumpy_sheet()
    sums, _ = _sums(verts, faces, 0.13)
    has = sums.count > 0
    A, b, m = sums.A[has], sums.b[has], sums.s[has] / sums.count[has, None]
    delta = ref.delta_of(A)
    assert np.all(delta > 0) and len(A) > 30
    M = A + delta[:, None, None] * np.eye(3)
    r = b - np.einsum('cij,cj->ci', A, m)
    y = ref.solve_ldl(M, r)
    want = np.linalg.solve(M, r[..., None])[..., 0]
    err = np.linalg.norm(y - want, axis=1) / np.linalg.norm(want, axis=1)
    print('largest relative difference to numpy.linalg.solve: %.3g' % err.max())
    assert err.max() <= 1e-9


def test_tilted_plane_stays_on_its_plane():
    """The grid's vertices are exact in fp32 and lie exactly on the plane, so the mean of a cluster does too, and the
    quadric term moves it by fp64 rounding only.  What is left is the final rounding of rule 5: half an fp32 ulp of the
    largest coordinate on each axis, sqrt(3) / 2 ulp in distance."""
    verts, faces, p0, normal = ref.tilted_plane(12)
    assert np.array_equal(verts.astype(F64), verts.astype(F64).astype(F32).astype(F64))
    assert np.abs((verts.astype(F64) - p0) @ normal).max() < 1e-15
    bound = np.sqrt(3.0) / 2 * float(np.spacing(F32(np.abs(verts).max()))) * 1.001
    for placement in ('quadric', 'mean'):
        out = ref.cluster(verts, faces, 0.21, placement=placement)
        assert 10 < len(out.verts) < len(verts) and len(out.faces) > 10
        dist = np.abs((out.verts.astype(F64) - p0) @ normal)
        print('%s: largest distance to the plane %.3g, bound %.3g' % (placement, dist.max(), bound))
        assert dist.max() <= bound


def cube_errors(out_verts, vertex_map, verts, faces):
    """For every output vertex: the cube sides (axis, value) its cluster's faces lie on, and its distance to the edge
    or corner where those sides meet (clusters on two or three sides only)."""
    sides = {}
    for t in faces:
        p = verts[t].astype(F64)
        for axis in range(3):
            for val in (0.0, 1.0):
                if np.all(p[:, axis] == val):
                    for k in t:
                        if vertex_map[k] >= 0:
                            sides.setdefault(int(vertex_map[k]), set()).add((axis, val))
    edge, corner = [], []
    for k, on in sides.items():
        axes = sorted(on)
        if len({a for a, _ in axes}) != len(axes) or len(axes) < 2:
            continue
        err = max(abs(float(out_verts[k][a]) - val) for a, val in axes)
        (edge if len(axes) == 2 else corner).append(err)
    return np.array(edge), np.array(corner)


def test_cube_edges_and_corners_are_kept_by_quadric_and_not_by_mean():
    """8 quads per edge, cell 2.5 quads: the vertex of a cluster on two sides lies on their edge and that of a cluster
    on three sides on the corner, to 1e-5 of the edge length, under 'quadric'; under 'mean' it does not.

    Rule 5's regulariser delta = f trace(A) / 3 leaves the vertex delta / (lambda + delta) of the way from the edge
    to the mean, lambda being the quadric's eigenvalue across the edge (trace / 2 on an edge, trace / 3 on a corner),
    and the mean lies about a quad inside.  This bound is what fixes f = 1e-5: it gives 2.5e-6 of the edge length on
    an edge and 7.5e-6 on a corner, where f = 1e-3 gave 2.5e-4 and 7.5e-4."""
    q = 8
    verts, faces = ref.cube_surface(q)
    cell = 2.5 / q
    got = {}
    for placement in ('quadric', 'mean'):
        out = ref.cluster(verts, faces, cell, placement=placement)
        edge, corner = cube_errors(out.verts, out.vertex_map, verts, faces)
        assert len(corner) == 8 and len(edge) >= 12
        got[placement] = (edge.max(), corner.max())
        print('%s: largest distance to its edge %.3g, to its corner %.3g' % (placement, edge.max(), corner.max()))
    assert min(got['mean']) > 1e-2          # the mean of a cluster on two sides lies inside the cube
    assert max(got['quadric']) <= 1e-5


@pytest.mark.parametrize('placement', ['quadric', 'mean'])
def test_output_vertices_stay_near_their_cluster(placement):
    """Rule 5's guard keeps x within one cell of the cell centre on every axis and every member lies in the cell, so
    the two are at most 1.5 cells apart per axis."""
    for verts, faces, cell in (bumpy_sheet() + (0.13,), bumpy_sheet(seed=5) + (0.3,), ref.cube_surface(8) + (2.5 / 8,)):
        out = ref.cluster(verts, faces, cell, placement=placement)
        assert len(out.verts)
        worst = 0.0
        for k in range(len(out.verts)):
            members = verts[out.vertex_map == k].astype(F64)
            assert len(members)
            worst = max(worst, np.linalg.norm(members - out.verts[k].astype(F64), axis=1).min())
        print('largest distance to the nearest member: %.3g cells' % (worst / cell))
        assert worst <= 1.5 * np.sqrt(3.0) * cell


def test_maps_say_what_went_where():
    verts, faces = bumpy_sheet()
    faces = np.concatenate([faces, faces[:40][:, ::-1], faces[5:9]])      # flipped and repeated copies
    out = ref.cluster(verts, faces, 0.13)
    src = faces[out.face_map]
    assert np.array_equal(out.faces, out.vertex_map[src])
    assert out.faces.min() == 0 and out.faces.max() == len(out.verts) - 1
    assert np.all(np.diff(out.face_map) > 0)
    assert set(np.unique(out.vertex_map)) - {-1} == set(range(len(out.verts)))
    triples = np.sort(out.faces, axis=1)
    assert len(np.unique(triples, axis=0)) == len(triples)                 # one face per set of three clusters
    assert np.all((triples[:, 0] != triples[:, 1]) & (triples[:, 1] != triples[:, 2]))
    assert ref.count_faces(verts, faces, 0.13) == len(out.faces)
