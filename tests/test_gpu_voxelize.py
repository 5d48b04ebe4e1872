"""sgnn_amd.voxelize on the GPU against the host restatement tests/voxelize_ref.py and against
meshdist: distance magnitudes and faces equal bit for bit, signs equal wherever the restatement is not ambiguous; every
case runs twice and the runs are equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxelize_ref as VR  # noqa: E402

from sgnn_amd import chunks, data, fusion, marching_cubes as mc, meshdist, voxelize  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
AMBIGUOUS_CAP = 0.01        # as in tests/test_voxelize_ref.py


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def run(verts, faces, dims, band, flip=False):
    """voxelize.signed_distance twice; the two results must be the same bits."""
    a = voxelize.signed_distance(verts, faces, dims, band, flip=flip)
    b = voxelize.signed_distance(verts, faces, dims, band, flip=flip)
    assert a.dist.is_cuda and a.dist.dtype == torch.float32 and a.face.dtype == torch.int32
    assert tuple(a.dist.shape) == tuple(a.face.shape) == tuple(dims)[::-1]
    assert torch.equal(a.dist.view(torch.int32), b.dist.view(torch.int32)) and torch.equal(a.face, b.face), 'two runs differ'
    return a.dist.cpu().numpy(), a.face.cpu().numpy()


def check(verts, faces, dims, band, flip=False, index=True):
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int32).reshape(-1, 3)
    ref = VR.signed_distance_ref(verts, faces, dims, band, flip=flip)
    dist, face = run(verts, faces, dims, band, flip)
    inband = ref.face >= 0
    assert np.array_equal(face, ref.face)
    assert np.array_equal(bits(np.abs(dist)), bits(np.abs(ref.dist)))
    assert np.isposinf(dist[~inband]).all()
    if index:       # the existing route to the same unsigned distances
        d, f = meshdist.TriangleIndex(verts, faces).distance(VR.centres(dims), max_dist=band)
        d, f = d.cpu().numpy().reshape(dist.shape), f.cpu().numpy().reshape(dist.shape)
        assert np.array_equal(np.isfinite(d), inband) and np.array_equal(f, face)
        assert np.array_equal(bits(d), bits(np.abs(dist)))
    sel = inband & ~ref.ambiguous
    share = ref.ambiguous[inband].mean() if inband.any() else 0.0
    print('%d in-band voxels, %d ambiguous' % (inband.sum(), ref.ambiguous.sum()))
    assert share <= AMBIGUOUS_CAP
    assert np.array_equal(np.signbit(dist[sel]), np.signbit(ref.dist[sel]))
    return dist, face, ref


def small_sphere(nfaces=None):
    """A sphere of 3 * FACE_BATCH faces, or its first nfaces, that lies in the middle of brick 0."""
    assert voxelize.FACE_BATCH == 128 and voxelize.BRICK == 8
    verts, faces = VR.uv_sphere((3.62, 3.41, 3.73), 2.23, 16, 13)
    assert len(faces) == 3 * voxelize.FACE_BATCH
    return verts, faces if nfaces is None else faces[:nfaces]


@pytest.mark.parametrize('band', [0.5, 3.0])
def test_dims_that_are_no_multiple_of_the_brick(band):
    verts, faces = VR.uv_sphere((17.3, 10.6, 6.2), 5.4, 7, 5)
    dist, face, _ = check(verts, faces, (37, 22, 13), band)
    assert (face >= 0).sum() > 300 and (dist < 0).any() and (dist > 0).any()


def test_one_triangle_spanning_the_volume():
    verts = [[-3.2, -2.1, 1.3], [44.7, 5.2, 20.9], [10.4, 43.3, 38.8]]
    dist, face, _ = check(verts, [[0, 1, 2]], (40, 40, 40), 3.0)
    touched = {(z // 8, y // 8, x // 8) for z, y, x in zip(*np.nonzero(face == 0))}
    assert len(touched) > 30


def bricks_touched(verts, face, dims, band):
    """Bricks that hold a voxel of the face's vertex box grown by band (the kernel's box is a hair larger)."""
    tri = np.asarray(verts, np.float64)[list(face)]
    n = 1
    for k in range(3):
        lo, hi = max(np.ceil(tri[:, k].min() - band), 0), min(np.floor(tri[:, k].max() + band), dims[k] - 1)
        n *= max(int(hi) // 8 - int(lo) // 8 + 1, 0) if lo <= hi else 0
    return n


@pytest.mark.parametrize('dims', [(72, 72, 56), (136, 136, 8)])
def test_a_face_that_touches_more_bricks_than_one_thread_lists(dims):
    """Such a face is spread over the 64 lanes of its wave in the count and in the fill pass."""
    assert voxelize.WAVE_BRICKS == 256
    s = np.array(dims, np.float64)
    verts = np.array([[-3.2, -2.1, 1.3], [1.12, 0.13, 0.52], [0.26, 1.08, 0.97]]) * [[1, 1, 1], s, s]
    assert bricks_touched(verts, (0, 1, 2), dims, 3.0) > voxelize.WAVE_BRICKS
    dist, face, _ = check(verts, [[0, 1, 2]], dims, 3.0)
    touched = {(z // 8, y // 8, x // 8) for z, y, x in zip(*np.nonzero(face == 0))}
    assert len(touched) > 60


def wave_mix():
    """Eight faces for a (72, 72, 56) volume: 2 and 6 are big, the others small."""
    needle, nf = VR.needle_tetrahedron(offset=(40.37, 8.61, 20.29))
    quad = np.array([[50.3, 52.7, 4.1], [61.6, 53.9, 6.3], [60.2, 64.8, 8.9], [49.4, 63.1, 6.2]], F32)
    big = np.array([[-3.2, -2.1, 1.3], [80.7, 9.2, 29.9], [18.4, 77.3, 54.8],
                    [21.3, 70.9, 3.2], [69.8, 66.1, 50.7], [66.2, 18.4, 47.5]], F32)
    verts = np.concatenate([needle, quad, big])
    faces = np.concatenate([nf[:2], [[8, 9, 10]], nf[2:], [[4, 5, 6]], [[11, 12, 13]], [[4, 6, 7]]]).astype(np.int32)
    return verts, faces


def test_big_and_small_faces_in_one_wave():
    """Two faces over the threshold, small faces before, between and after them, all listed by the same wave; the
    second big face is listed only in part of the volume."""
    dims = (72, 72, 56)
    verts, faces = wave_mix()
    assert len(faces) < 64
    for t in (2, 6):
        assert bricks_touched(verts, faces[t], dims, 3.0) > voxelize.WAVE_BRICKS
    assert bricks_touched(verts, faces[6], dims, 3.0) < 9 * 9 * 7
    assert all(bricks_touched(verts, faces[t], dims, 3.0) <= 64 for t in (0, 1, 3, 4, 5, 7))
    dist, face, _ = check(verts, faces, dims, 3.0)
    assert set(np.unique(face)) == {-1} | set(range(8))


def sorted_lists(offsets, refs):
    """The refs of a CSR list in ascending order inside every cell: the order inside a cell is the atomics'."""
    cell = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return refs[np.lexsort((refs, cell))]


@pytest.mark.parametrize('band', [0.0, 3.0])
@pytest.mark.parametrize('dims', [(20, 9, 33), (69, 75, 53)])
def test_the_brick_lists_themselves(dims, band):
    """voxelize._brick_lists against voxelize_ref.brick_lists_ref: offsets equal, every brick's faces equal as sets.
    One wave holds faces that span the volume (listed by the wave in the larger volume, where they touch more than
    WAVE_BRICKS bricks, by their lane in the smaller), small faces, one face wholly outside, one overhanging the
    x = 0 side and one with a NaN vertex.  Neither volume is a multiple of the brick."""
    verts, faces = wave_mix()
    verts = verts * (np.array(dims, F32) / np.array([72, 72, 56], F32))              # made for a (72, 72, 56) volume
    nv = len(verts)
    more = np.array([[100.5, 3, 3], [104, 9.1, 3], [101, 4, 8.3],                     # wholly outside
                     [-9.2, 4.1, 10.3], [2.6, 6.2, 12.9], [-4.1, 7.7, 17.2],          # overhangs x = 0
                     [np.nan, 3, 3]], F32)
    faces = np.concatenate([faces, [[nv, nv + 1, nv + 2], [nv + 3, nv + 4, nv + 5], [nv + 6, 0, 1]]]).astype(np.int32)
    verts = np.concatenate([verts, more])
    outside, overhang, ignored = 8, 9, 10
    tri = verts[faces]
    boxes = np.concatenate([tri.min(1), tri.max(1)], 1)
    boxes[ignored] = [np.inf] * 3 + [-np.inf] * 3
    packed = meshdist._Packed(verts, faces)
    assert np.array_equal(bits(packed.boxes.cpu().numpy()), bits(boxes))
    want_offsets, want_refs = VR.brick_lists_ref(boxes, dims, band)
    per_face = np.bincount(want_refs, minlength=len(faces))
    assert per_face[outside] == per_face[ignored] == 0 and per_face[overhang] > 0
    assert (per_face[:8] > 0).all() if band else (per_face[[2, 5, 6, 7]] > 0).all()      # a thin face may hold no voxel
    assert per_face.max() == -(-dims[0] // 8) * -(-dims[1] // 8) * -(-dims[2] // 8)         # the whole volume
    if dims == (69, 75, 53):
        assert (per_face[[2, 6]] > voxelize.WAVE_BRICKS).all() and (per_face[[0, 1, 3, 4, 5, 7]] <= 64).all()
    else:
        assert per_face.max() <= voxelize.WAVE_BRICKS
    for _ in range(2):
        offsets, refs, n_refs = voxelize._brick_lists(packed.boxes, len(faces), float(F32(band)), dims, packed.device)
        assert offsets.dtype == torch.int32 and refs.dtype == torch.int32 and n_refs == want_offsets[-1]
        offsets, refs = offsets.cpu().numpy(), refs.cpu().numpy()[:n_refs]
        assert np.array_equal(offsets, want_offsets)
        assert np.array_equal(sorted_lists(offsets, refs), want_refs)


@pytest.mark.parametrize('nfaces,band', [(voxelize.FACE_BATCH + 1, 3.0), (3 * voxelize.FACE_BATCH, 1.5)])
def test_more_faces_in_a_brick_than_one_batch(nfaces, band):
    verts, faces = small_sphere(nfaces)
    dist, face, _ = check(verts, faces, (13, 12, 11), band)
    assert len(np.unique(face[:8, :8, :8])) > 40             # many of the brick's faces win somewhere in it


def test_a_mesh_that_overhangs_the_volume_on_every_side():
    verts, faces = VR.l_prism(offset=(-6.3, -5.2, -4.4), scale=14.1, height=30.7)
    dims = (20, 18, 16)
    assert (verts.min(0) < -3).all() and (verts.max(0) > np.array(dims) + 3).all()
    check(verts, faces, dims, 3.0)


def test_faces_wholly_outside_the_volume():
    verts, faces = VR.needle_tetrahedron()
    far = np.array([[100.5, 3, 3], [104, 9.1, 3], [101, 4, 8.3], [-30.2, -9, -8], [-35, -9.5, -3], [-31, -14, -7.7]], F32)
    faces = np.concatenate([[[4, 5, 6], [7, 8, 9]], faces])
    dist, face, _ = check(np.concatenate([verts, far]), faces, (24, 24, 32), 3.0)
    assert face.max() > 1 and not np.isin(face, (0, 1)).any()


def test_nan_degenerate_and_duplicate_faces_and_the_shared_edge_tie():
    verts = np.array([[2.5, 2.5, 2.5], [13.2, 2.6, 5.1], [12.7, 12.9, 6.3], [2.9, 13.4, 5.2], [np.nan, 3, 3], [5, 5, 5],
                      [7.5, 7.5, 7.5]], F32)
    faces = [[4, 0, 1],             # a NaN vertex: ignored
             [0, 0, 1],             # a repeated vertex: ignored
             [0, 5, 6],             # three vertices on one line: no area, ignored
             [0, 2, 3], [0, 1, 2],  # a quad: the voxels nearest the diagonal tie, the lower index wins
             [0, 1, 2], [0, 2, 3]]  # duplicates of both
    dist, face, ref = check(verts, faces, (16, 16, 10), 3.0)
    assert set(np.unique(face)) == {-1, 3, 4}
    a, ab, ac, usable = VR.pack_ref(verts, faces)
    assert list(usable) == [False, False, False, True, True, True, True]
    pts = VR.centres((16, 16, 10))
    d3 = VR._sq(VR.residual_ref(pts, a[3], ab[3], ac[3])[0])
    d4 = VR._sq(VR.residual_ref(pts, a[4], ab[4], ac[4])[0])
    tie = (d3 == d4).reshape(face.shape) & (face >= 0)
    assert tie.sum() > 5 and (face[tie] == 3).all()


def test_an_empty_mesh_and_a_mesh_without_a_usable_face():
    for verts, faces in ((np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)),
                         (np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]], F32), np.array([[0, 1, 2], [0, 0, 1]], np.int32))):
        dist, face, _ = check(verts, faces, (9, 8, 7), 3.0, index=False)
        assert np.isposinf(dist).all() and (face == -1).all()


def test_flip_negates_every_non_zero_value_and_nothing_else():
    verts, faces = VR.needle_tetrahedron()
    dist, face, _ = check(verts, faces, (24, 24, 32), 3.0)
    flipped, face2, _ = check(verts, faces, (24, 24, 32), 3.0, flip=True, index=False)
    inband = face >= 0
    assert np.array_equal(face, face2) and (dist[inband] != 0).all()
    assert np.array_equal(bits(flipped[inband]), bits(-dist[inband])) and np.isposinf(flipped[~inband]).all()


def test_a_voxel_on_the_surface_keeps_plus_zero():
    verts = np.array([[2, 2, 3], [9, 2, 3], [2, 9, 3]], F32)
    for flip in (False, True):
        dist, _ = run(verts, np.array([[0, 1, 2]], np.int32), (12, 12, 6), 1.0, flip=flip)
        assert dist[3, 4, 4] == 0 and not np.signbit(dist[3, 4, 4])
        assert dist[4, 4, 4] == (-1 if flip else 1) and dist[2, 4, 4] == (1 if flip else -1)


def test_an_open_mesh_a_single_quad():
    """Boundary edges see one face, the two boundary-only corners one angle."""
    verts = np.array([[3.3, 2.7, 4.1], [14.6, 3.9, 6.3], [13.2, 14.8, 8.9], [2.4, 13.1, 6.2]], F32)
    dist, face, _ = check(verts, [[0, 1, 2], [0, 2, 3]], (18, 18, 13), 3.0)
    assert (dist < 0).sum() > 200 and (np.isfinite(dist) & (dist > 0)).sum() > 200


def test_the_sharp_edges_where_a_face_normal_goes_wrong():
    """The two host cases with teeth (tests/test_voxelize_ref.py): the device signs them as the restatement does."""
    for (verts, faces), dims in ((VR.needle_tetrahedron(), (24, 24, 32)), (VR.l_prism(), (40, 40, 28))):
        dist, face, ref = check(verts, faces, dims, 3.0)
        sel = (face >= 0) & ~ref.ambiguous
        wrong = np.signbit(ref.naive_dist[sel]) != np.signbit(ref.dist[sel])
        assert wrong.sum() > 0 and np.array_equal(np.signbit(dist[sel][wrong]), np.signbit(ref.dist[sel][wrong]))


def test_device_inputs_are_taken_as_they_are():
    verts, faces = VR.needle_tetrahedron()
    want = run(verts, faces, (24, 24, 32), 3.0)
    got = run(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), (24, 24, 32), 3.0)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        voxelize.signed_distance(torch.from_numpy(verts).cuda(), torch.from_numpy(faces + 2).cuda(), (24, 24, 32), 3.0)
    with pytest.raises(ValueError):
        voxelize.signed_distance(verts, faces + 2, (24, 24, 32), 3.0)
    with pytest.raises(ValueError):
        voxelize.signed_distance(verts, faces, (24, 24, 32), -1.0)


# ---------------------------------------------------------------------------------------------------------
# volumes
# ---------------------------------------------------------------------------------------------------------
VS = F32(0.05)


def world_case():
    """The L prism in metres and a world2grid that is not the identity."""
    verts, faces = VR.l_prism()
    w2g = np.eye(4, dtype=F32)
    w2g[:3, :3] = np.array(VR.rotation((0.2, -0.1, 1.0), 0.05), F32) / VS
    w2g[:3, 3] = [1.7, -2.2, 0.9]
    g2w = np.linalg.inv(w2g.astype(np.float64))
    world = (np.concatenate([verts.astype(np.float64), np.ones((len(verts), 1))], 1) @ g2w.T)[:, :3].astype(F32)
    return world, faces, w2g


def expected_sdf(world, faces, dims, w2g, vs, band, flip=False):
    ref = VR.signed_distance_ref(VR.grid_coords_ref(world, w2g), faces, dims, band, flip=flip)
    inband = ref.face >= 0
    with np.errstate(invalid='ignore'):
        return np.where(inband, ref.dist * F32(vs), F32(-np.inf)).astype(F32), inband, ref


def test_mesh_to_volume(tmp_path):
    world, faces, w2g = world_case()
    dims = (40, 40, 28)
    vol = voxelize.mesh_to_volume(world, faces, dims, VS, w2g, band=3.0)
    again = voxelize.mesh_to_volume(world, faces, dims, VS, w2g, band=3.0)
    assert isinstance(vol, fusion.TSDFVolume) and vol.dims_xyz == dims
    assert torch.equal(vol._sdf.view(torch.int32), again._sdf.view(torch.int32))
    want, inband, ref = expected_sdf(world, faces, dims, w2g, VS, 3.0)
    sdf = vol.sdf().cpu().numpy()
    assert np.array_equal(bits(np.abs(sdf)), bits(np.abs(want)))
    sel = inband & ~ref.ambiguous
    assert ref.ambiguous[inband].mean() <= AMBIGUOUS_CAP and np.array_equal(np.signbit(sdf[sel]), np.signbit(want[sel]))
    assert np.isneginf(sdf[~inband]).all()
    assert np.array_equal(vol.weight().cpu().numpy(), inband.astype(np.uint8)) and not vol.free_count().any()
    # the consumers of a fused volume run on it unchanged
    known = vol.known().cpu().numpy()
    assert known.shape == sdf.shape and (known[~inband] == 2).all() and (known[np.abs(sdf) <= VS] == 1).all()
    locs, vals = vol.sparse()
    assert locs.shape[0] == inband.sum() and np.array_equal(bits(vals.cpu().numpy()), bits(sdf[inband]))
    assert fusion.scan_sample(vol)['input'][0].shape[0] > 1000
    path = vol.save(str(tmp_path / 'mesh.sdf'))
    (zyx, feats), dims_zyx, w = data.load_scene(path)
    assert list(dims_zyx) == list(dims[::-1]) and np.array_equal(np.asarray(w, F32).reshape(4, 4), w2g)
    assert np.array_equal(np.asarray(zyx)[:, ::-1], locs.cpu().numpy())
    assert np.array_equal(bits(feats), bits(vals.cpu().numpy() / VS))
    assert np.array_equal(data.load_scene_known(os.path.splitext(path)[0] + '.knw').reshape(known.shape), known)


@functools.lru_cache(maxsize=None)
def sphere():
    """The marching-cubes sphere of tests/test_gpu_simplify.py: a 24^3 distance volume, voxel units."""
    z, y, x = np.meshgrid(*(np.arange(24, dtype=np.float64),) * 3, indexing='ij')
    centre, radius = np.array([11.3, 11.7, 12.1]), 8.4
    sdf = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    v, _, f = mc.run_marching_cubes(torch.from_numpy(sdf.astype(F32)).cuda(), None, 0.0, 3.0, 10.0)
    assert v.shape[0] > 1000 and f.shape[0] > 2000
    return v, f, sdf, centre, radius


MC_FLIP = False     # README "Volumes from a mesh": run_marching_cubes output needs no flip


def test_round_trip_through_marching_cubes():
    """Volume -> mesh -> volume.  Every in-band voxel is as far from the mesh as from the sphere up to the distance
    between the two surfaces, measured here on the mesh itself: vertices lie within dev = max | |v - c| - r | of the
    sphere, and a point of a triangle lies at most the chord sag further in.  For q = sum l_i v_i in a triangle,
    |q - c|^2 = sum l_i |v_i - c|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= (r - dev)^2 - L^2 / 3 with L the longest edge of
    the mesh (sum_{i<j} l_i l_j <= 1/3), so sag = (r - dev) - sqrt((r - dev)^2 - L^2 / 3): the sag of a chord of
    half-length L / sqrt(3), which for a marching-cubes triangle inside one voxel is at most half a voxel's diagonal
    and a bit.  The mesh is star-shaped about c, so the sphere is within the same bound of the mesh.

    Measured on an MI355X: vertex deviation 0.04453, longest edge 1.7077, bound 0.10290, largest difference 0.07390,
    72 % of the bound.  Read as the sag of a chord whose half-length is half a voxel (0.0149), the bound would be
    0.0594 and would not hold: marching-cubes edges reach 1.7 voxels, and their triangles dip further than that."""
    v, f, analytic, centre, radius = sphere()
    vh, fh = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
    dev = np.abs(np.linalg.norm(vh - centre, axis=1) - radius).max()
    tri = vh[fh]
    longest = max(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1).max() for i in range(3))
    rho = radius - dev
    bound = dev + (rho - np.sqrt(rho * rho - longest * longest / 3.0))
    vol = voxelize.mesh_to_volume(v, f, (24, 24, 24), 1.0, np.eye(4), band=3.0, flip=MC_FLIP)
    sdf = vol.sdf().cpu().numpy().astype(np.float64)
    inband = np.isfinite(sdf)
    err = np.abs(sdf[inband] - analytic[inband]).max()
    half = radius - np.sqrt(radius * radius - 0.25)            # the sag of a chord whose half-length is half a voxel
    print('vertex deviation %.5f, longest edge %.4f, bound %.5f, largest difference %.5f (%.0f %% of the bound); '
          'with the sag of a half-voxel half-chord the bound would be %.5f'
          % (dev, longest, bound, err, 100 * err / bound, dev + half))
    assert inband.sum() > 3000 and err <= bound
    assert np.isneginf(sdf[np.abs(analytic) > 3.0 + bound]).all() and inband[np.abs(analytic) < 3.0 - bound].all()
    sure = inband & (np.abs(analytic) > bound)
    assert np.array_equal(sdf[sure] < 0, analytic[sure] < 0)
    # the other flip is the wrong one
    other = voxelize.mesh_to_volume(v, f, (24, 24, 24), 1.0, np.eye(4), band=3.0, flip=not MC_FLIP).sdf().cpu().numpy()
    assert np.array_equal(other[sure] < 0, analytic[sure] > 0)


def test_mesh_to_pyramid_and_a_training_chunk():
    world, faces, w2g = world_case()
    dims = (32, 32, 64)
    pyr = voxelize.mesh_to_pyramid(world, faces, dims, VS, w2g, levels=4, band=3.0)
    assert isinstance(pyr, fusion.TSDFPyramid) and len(pyr) == 4
    for k, level in enumerate(pyr.volumes):
        assert level.dims_xyz == tuple(-(-d // 2 ** k) for d in dims)
        alone = voxelize.mesh_to_volume(world, faces, level.dims_xyz, level.voxel_size, level.world2grid, band=3.0)
        assert torch.equal(level.sdf().view(torch.int32), alone.sdf().view(torch.int32))
        assert torch.equal(level.weight(), alone.weight()) and int(level.weight().sum()) > 0
        want, inband, ref = expected_sdf(world, faces, level.dims_xyz, level.world2grid, level.voxel_size, 3.0)
        assert np.array_equal(bits(np.abs(level.sdf().cpu().numpy())), bits(np.abs(want)))
    # a sparsely seen input beside the complete target: the same mesh, a thinner band
    inp = voxelize.mesh_to_volume(world, faces, dims, VS, w2g, band=1.0)
    cutter = chunks.ChunkCutter(inp, pyr, crop_zyx=(32, 32, 32), stride_zyx=(32, 32, 32))
    cand = cutter.candidates()
    assert len(cand.origins) >= 1
    batch = cutter.batch(cand.origins[:1])
    oz, oy, ox = (int(o) for o in cand.origins[0])
    fine = pyr[0].sdf().cpu().numpy()[oz:oz + 32, oy:oy + 32, ox:ox + 32]
    with np.errstate(invalid='ignore'):
        want = np.where(np.abs(fine) <= F32(6.0) * VS, fine / VS, F32(-np.inf)).astype(F32)
    got = batch['sdf'].cpu().numpy()[0, 0]
    assert np.isfinite(want).sum() > 1000 and np.array_equal(bits(got), bits(want))
    assert batch['input'][0].shape[0] > 100 and [tuple(h.shape[2:]) for h in batch['hierarchy']] == [(4,) * 3, (8,) * 3, (16,) * 3]
