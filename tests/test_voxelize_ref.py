"""The NumPy restatement of the voxelisation rules (tests/voxelize_ref.py) against fp64:
distances against a separately written fp64 point-triangle distance, signs against the generalised winding number,
and the two meshes on which the sign of the winning face's own normal goes wrong while the pseudo-normal of the closest
feature does not.  No GPU."""
import functools

import numpy as np
import pytest

import voxelize_ref as VR

BAND = 3.0
CASES = {
    'needle': (VR.needle_tetrahedron, (24, 24, 32)),
    'l_prism': (VR.l_prism, (40, 40, 28)),
    'sphere': (lambda: VR.uv_sphere((7.31, 8.13, 6.77), 4.6, 9, 6), (16, 17, 15)),
}
# A voxel whose sign is ambiguous is left out of sign comparisons; no case may leave out more than this share of its
# in-band voxels, here or on the device (tests/test_gpu_voxelize.py)
AMBIGUOUS_CAP = 0.01


@functools.lru_cache(maxsize=None)
def case(name):
    make, dims = CASES[name]
    verts, faces = make()
    ref = VR.signed_distance_ref(verts, faces, dims, BAND)
    pts = VR.centres(dims)
    return verts, faces, dims, ref, pts


@pytest.mark.parametrize('name', sorted(CASES))
def test_distances_match_fp64_within_the_rounding_of_section_g(name):
    """Section G, rule 5: rule 2 in fp32 is within about 16 * 2^-24 * m = 2^-20 * m of the true distance, m the largest
    coordinate magnitude involved; these meshes have no slivers, so the bound holds both ways."""
    verts, faces, dims, ref, pts = case(name)
    d64 = VR.exact_distance64(pts, verts, faces).reshape(ref.dist.shape)       # written apart from rule 2
    m = max(float(np.abs(verts).max()), float(max(dims)))
    tol = 2.0 ** -20 * m
    # rule 2 itself in fp64 is the same distance up to fp64 rounding
    assert np.abs(VR.distance64(pts, verts, faces).reshape(ref.dist.shape) - d64).max() <= 1e-9 * m
    inband = ref.face >= 0
    assert inband.sum() > 1000
    assert np.abs(np.abs(ref.dist[inband]).astype(np.float64) - d64[inband]).max() <= tol
    # the band itself: only a voxel within the rounding of the boundary may be on the other side of it
    assert (d64[inband] <= BAND + tol).all() and (d64[~inband] > BAND - tol).all()
    assert np.isposinf(ref.dist[~inband]).all() and (ref.face[~inband] == -1).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_signs_match_the_winding_number(name):
    verts, faces, dims, ref, pts = case(name)
    inband = ref.face >= 0
    share = ref.ambiguous[inband].mean()
    print('%s: %d in-band voxels, %d ambiguous (%.4f)' % (name, inband.sum(), ref.ambiguous.sum(), share))
    assert share <= AMBIGUOUS_CAP
    sel = inband & ~ref.ambiguous
    w = VR.winding_number(pts[sel.ravel()], verts, faces)
    assert (np.abs(w - np.rint(w)) < 1e-6).all() and set(np.rint(w).astype(int)) <= {0, 1}     # closed, outward
    inside = np.rint(w) == 1
    assert inside.sum() > 50 and (~inside).sum() > 50
    assert np.array_equal(np.signbit(ref.dist[sel]), inside)


def test_the_test_meshes_are_what_they_claim():
    verts, faces = VR.needle_tetrahedron()
    assert sum(a < 30.0 for a in VR.dihedral_angles(verts, faces).values()) >= 2
    verts, faces = VR.l_prism()
    angles = VR.dihedral_angles(verts, faces)
    assert sum(a > 260.0 for a in angles.values()) == 1            # the re-entrant edge
    assert min(angles.values()) < 80.0                             # slanted: sharper than a right prism
    for make in (VR.needle_tetrahedron, VR.l_prism):
        v = make()[0]
        assert (np.abs(v - np.rint(v)) > 1e-3).all()               # off the lattice


@pytest.mark.parametrize('name', ['needle', 'l_prism'])
def test_the_winning_faces_normal_gives_wrong_signs_where_the_pseudo_normal_does_not(name):
    verts, faces, dims, ref, pts = case(name)
    sel = (ref.face >= 0) & ~ref.ambiguous
    w = np.rint(VR.winding_number(pts[sel.ravel()], verts, faces))
    outside = w == 0
    naive_wrong = np.signbit(ref.naive_dist[sel]) != (w == 1)
    assert naive_wrong.sum() > 0 and outside[naive_wrong].any()    # the test has teeth: outside voxels signed inside
    assert not (np.signbit(ref.dist[sel]) != (w == 1)).any()       # rules 4 to 6 sign every one of them right
    # and they sit where the rule says: the closest feature of a wrongly signed voxel is an edge or a vertex
    a, ab, ac, _ = VR.pack_ref(verts, faces)
    t = ref.face[sel][naive_wrong]
    _, feature = VR.residual_ref(pts[sel.ravel()][naive_wrong], a[t], ab[t], ac[t])
    assert (feature != VR.INTERIOR).all()


def test_flip_negates_every_non_zero_value_and_nothing_else():
    verts, faces, dims, ref, _ = case('needle')
    flipped = VR.signed_distance_ref(verts, faces, dims, BAND, flip=True)
    inband = ref.face >= 0
    assert np.array_equal(flipped.face, ref.face)
    assert np.array_equal(flipped.dist[inband], -ref.dist[inband]) and np.isposinf(flipped.dist[~inband]).all()


def test_a_voxel_on_the_surface_keeps_plus_zero():
    verts = np.array([[2, 2, 3], [9, 2, 3], [2, 9, 3]], np.float32)
    for flip in (False, True):
        ref = VR.signed_distance_ref(verts, [[0, 1, 2]], (12, 12, 6), 1.0, flip=flip)
        assert ref.dist[3, 4, 4] == 0 and not np.signbit(ref.dist[3, 4, 4])
        assert ref.dist[4, 4, 4] == (-1 if flip else 1) and ref.dist[2, 4, 4] == (1 if flip else -1)


def test_grid_coordinates_follow_fusion_affine():
    from sgnn_amd import fusion
    rng = np.random.default_rng(3)
    m = np.eye(4, dtype=np.float32)
    m[:3] = rng.normal(size=(3, 4)).astype(np.float32) * 37
    v = rng.normal(size=(100, 3)).astype(np.float32)
    assert np.array_equal(VR.grid_coords_ref(v, m), fusion._affine(m, v))


def test_pseudo_normals_do_not_depend_on_the_face_order():
    verts, faces = VR.l_prism()
    perm = np.random.default_rng(0).permutation(len(faces))
    _, v0, e0 = VR.pseudo_normals_ref(verts, faces)
    _, v1, e1 = VR.pseudo_normals_ref(verts, faces[perm])
    assert np.array_equal(v0, v1) and e0.keys() == e1.keys() and all(np.array_equal(e0[k], e1[k]) for k in e0)
    # a closed manifold: every edge sees two faces, so its sum is at most 2 long
    assert all(np.linalg.norm(s / VR.Q32) <= 2.0 + 1e-9 for s in e0.values())
