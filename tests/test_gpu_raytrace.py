"""GPU: rays against meshes (sgnn_amd.raytrace, csrc/raytrace.hip) against the brute-force NumPy restatement of
tests/raytrace_ref.py: t and uv bit for bit, faces and hit flags exactly, whatever the grid; then the rasteriser, a
LiDAR sweep fused into a volume, and visibility."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshdist_ref as M  # noqa: E402
import raytrace_ref as T  # noqa: E402
import render_ref as RR  # noqa: E402

from sgnn_amd import fusion, meshdist, points, raytrace, render, voxelize  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
# rasteriser cross-check: four times the largest |t - depth| between tests/render_ref.py and the restatement on the
# interior pixels of the four 60 x 80 frames below, which tests/test_raytrace_ref.py measures and asserts on the CPU
RENDER_BAR = 4.0 * T.MEASURED_RENDER_ERR


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    t, f, uv = exp
    assert got.t.is_cuda and got.t.dtype == torch.float32 and got.face.dtype == torch.int32
    assert tuple(got.t.shape) == t.shape and tuple(got.uv.shape) == uv.shape
    gf = got.face.cpu().numpy()
    assert np.array_equal(gf, f), '%d of %d faces differ' % ((gf != f).sum(), f.size)
    assert np.array_equal(bits(got.t), bits(t)), '%d of %d t differ' % ((bits(got.t) != bits(t)).sum(), t.size)
    assert np.array_equal(bits(got.uv), bits(uv)), '%d of %d uv differ' % ((bits(got.uv) != bits(uv)).any(1).sum(), t.size)


def counted(scene, o, d, **kw):
    c = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = scene.closest(o, d, counters=c, **kw)
    return out, [int(v) for v in c.cpu()]


@functools.lru_cache(None)
def soup_case():
    """render_ref.triangle_soup(3000) and 5 000 rays: a third start inside the box, a third outside and aimed at it, a
    third aimed past it; the brute-force result."""
    verts, faces = RR.triangle_soup(3000)
    o, d = T.soup_rays(verts, faces, 5000, seed=11)
    exp = T.closest_ref(o, d, verts, faces)
    for x in (verts, faces, o, d) + exp:
        x.setflags(write=False)
    return verts, faces, o, d, exp


def test_soup_for_three_pitches():
    verts, faces, o, d, exp = soup_case()
    a, ab, ac, usable = M.pack_ref(verts, faces)
    median = float(np.median(np.concatenate([np.linalg.norm(x, axis=1) for x in (ab, ac, ac - ab)])))
    assert 1000 < (exp[1] >= 0).sum() < 4000
    seen = []
    for cell in (None, 1000.0, 0.8 * median):
        scene = raytrace.Scene(verts, faces, cell)
        got, (cells, pairs) = counted(scene, o, d)
        same(got, exp)
        same(scene.closest(o, d, sort=True), exp)
        seen.append((scene.index.dims, cells, pairs))
    print('dims, cells, pairs per cell value:', seen)
    scene = raytrace.Scene(verts, faces, 1000.0)
    enter = T.enters_ref(o, d, scene.index.lo, scene.index.dims, scene.index.cell, scene.index.guard)
    assert seen[1][0] == (1, 1, 1) and 0 < enter.sum() < len(o)
    assert seen[1][1:] == (int(enter.sum()), int(enter.sum()) * int(usable.sum()))
    assert seen[2][0][0] > seen[0][0][0] > 1 and seen[0][2] < len(o) * len(faces) // 10
    # the order of the rays and of the faces (remapped) changes no bit
    rng = np.random.default_rng(0)
    rp, fp = rng.permutation(len(o)), rng.permutation(len(faces))
    scene = raytrace.Scene(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())
    same(scene.closest(torch.from_numpy(o[rp]).cuda(), torch.from_numpy(d[rp]).cuda()), tuple(x[rp] for x in exp))
    got = raytrace.Scene(verts, faces[fp]).closest(o, d)
    assert np.array_equal(bits(got.t), bits(exp[0]))
    f = got.face.cpu().numpy()
    orig = np.where(f >= 0, fp[np.maximum(f, 0)], -1)
    ties = orig != exp[1]                                         # another face at exactly the same t
    det, u, v, t = T.ray_face(o[ties], d[ties], a[orig[ties]], ab[orig[ties]], ac[orig[ties]])
    assert np.array_equal(bits(t), bits(exp[0][ties])) and (f[ties] < np.argsort(fp)[exp[1][ties]]).all()
    assert np.array_equal(bits(got.uv)[~ties], bits(exp[2])[~ties])


def test_gates_culling_and_points():
    verts, faces, o, d, exp = soup_case()
    o, d = o[:1500], d[:1500]
    scene = raytrace.Scene(verts, faces)
    for kw in (dict(t_min=0.5, t_max=6.0), dict(cull_back=True), dict(t_min=-2.0, t_max=0.75, cull_back=True)):
        e = T.closest_ref(o, d, verts, faces, **kw)
        assert 0 < (e[1] >= 0).sum() and not np.array_equal(e[1], exp[1][:1500])
        same(scene.closest(o, d, **kw), e)
    got = scene.closest(o, d)
    p = got.points(o, d)
    assert np.array_equal(bits(p), bits(T.points_ref(o, d, exp[0][:1500])))
    assert np.isnan(p.cpu().numpy()[exp[1][:1500] < 0]).all()
    for bad in (dict(t_min=1.0, t_max=1.0), dict(t_min=float('nan')), dict(t_min=float('-inf'))):
        with pytest.raises(ValueError):
            scene.closest(o, d, **bad)
    with pytest.raises(ValueError):
        scene.closest(o[:, :2], d)
    with pytest.raises(ValueError):
        scene.closest(o, d[:7])
    with pytest.raises(ValueError):
        scene.closest(o, d, counters=torch.zeros(2))
    with pytest.raises(ValueError):
        scene.occluded(o, o[:5])
    with pytest.raises(ValueError):
        raytrace.Scene(verts, faces, colors=np.zeros((3, 3), np.uint8))
    none = scene.closest(o[:0], d[:0])
    assert none.t.shape == (0,) and none.face.shape == (0,) and none.uv.shape == (0, 2)
    assert scene.occluded(o[:0], o[:0]).shape == (0,)


@pytest.mark.parametrize('nrays', [1, 63, 64, 65])
def test_one_face_and_few_rays(nrays):
    verts = np.array([[0.25, 0.5, 1.0], [1.5, 0.5, 1.0], [0.25, 2.0, 1.25]], F32)
    faces = np.array([[0, 1, 2]], np.int32)
    rng = np.random.default_rng(nrays)
    o = np.concatenate([rng.uniform(0, 2, (nrays, 2)), np.full((nrays, 1), -1.0)], 1).astype(F32)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], F32), (nrays, 1))
    d[::3] = rng.normal(size=d[::3].shape) * 0.1 + [0, 0, 1]
    exp = T.closest_ref(o, d, verts, faces)
    for cell in (None, 0.1):
        same(raytrace.Scene(verts, faces, cell).closest(o, d), exp)
    assert nrays < 10 or 0 < (exp[1] == 0).sum() < nrays


def awkward_mesh():
    """The room with n = 2, whose walls lie in grid planes at cell = 0.4, with degenerate, non-finite and duplicate
    faces mixed in: the duplicates of faces 0..9 come first, so the copies at the end never win."""
    verts, faces = RR.tessellate_room(2)
    nv = len(verts)
    verts = np.concatenate([verts, [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]]]).astype(F32)
    extra = np.array([[0, 0, 1], [3, 3, 3], [0, 1, nv], [nv + 1, 2, 3], [nv, nv, nv]], np.int32)
    faces = np.concatenate([faces[:7], extra[:3], faces[7:], extra[3:], faces[:10]]).astype(np.int32)
    return verts, faces


def test_awkward_rays_and_faces():
    verts, faces = awkward_mesh()
    usable = M.pack_ref(verts, faces)[3]
    assert (~usable).sum() == 5
    eye = np.array([2.0, 1.6, 1.3])
    v, room_faces = (x.astype(np.float64) if x.dtype == F32 else x for x in RR.tessellate_room(2))
    aims = np.concatenate([v[room_faces[:20]].mean(1), v, (v[room_faces[:40, 0]] + v[room_faces[:40, 1]]) / 2])
    for cell in (0.4, None):
        scene = raytrace.Scene(verts, faces, cell)
        grid = T.GuardGrid(verts, faces, scene.index.cell)
        assert grid.dims == scene.index.dims
        ao, ad = T.awkward_rays(grid)
        # from the middle of the room at face centres, vertices and edge midpoints; and origins exactly on a wall
        on_wall = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 0.7], [2.0, 1.0, 0.0]])
        o = np.concatenate([ao, np.repeat(eye[None], len(aims), 0), on_wall, on_wall]).astype(F32)
        d = np.concatenate([ad, aims - eye, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0.5, 0], [0, 1, 0.5], [0.5, 0, 1]]]).astype(F32)
        exp = T.closest_ref(o, d, verts, faces)
        got, (cells, pairs) = counted(scene, o, d)
        same(got, exp)
        assert not np.isin(exp[1], np.nonzero(~usable)[0]).any() and (exp[1] < len(faces) - 10).all()
        assert (exp[1][len(ao) - 6:len(ao)] == -1).all()              # zero and non-finite rays
        assert (exp[0][-6:] > 0.01).all() and (exp[1][-6:] >= 0).all()    # t = 0 on the wall is excluded
        same(scene.closest(o, d, cull_back=True), T.closest_ref(o, d, verts, faces, cull_back=True))
        e_hit = T.occluded_ref(o, o + d, verts, faces, eps=1e-4)
        assert np.array_equal(scene.occluded(o, o + d, eps=1e-4).cpu().numpy(), e_hit)
    # a two-sided pair: the same triangle with both windings; culling picks the one that faces the ray
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    pair = np.array([[0, 2, 1], [0, 1, 2]], np.int32)
    o = np.array([[0.2, 0.2, 1.0], [0.2, 0.2, -1.0]], F32)
    d = np.array([[0, 0, -1.0], [0, 0, 1.0]], F32)
    scene = raytrace.Scene(tri, pair)
    assert scene.closest(o, d).face.tolist() == [0, 0]
    culled = scene.closest(o, d, cull_back=True)
    same(culled, T.closest_ref(o, d, tri, pair, cull_back=True))
    assert sorted(culled.face.tolist()) == [0, 1]


@functools.lru_cache(None)
def soup_boundary():
    verts, faces, o, d, exp = soup_case()
    hit = np.nonzero(exp[1] >= 0)[0]                              # every closest hit
    return hit, T.boundary64(o[hit], d[hit], verts, faces)


def test_any_hit():
    verts, faces, o, d, exp = soup_case()
    scene = raytrace.Scene(verts, faces)
    sel = slice(0, 5000, 3)
    targets = (o[sel] + d[sel] * F32(8.0)).astype(F32)
    e = T.occluded_ref(o[sel], targets, verts, faces, eps=1e-4)
    assert 50 < e.sum() < len(e) - 50, e.sum()
    c = torch.zeros(2, dtype=torch.int64, device='cuda')
    assert np.array_equal(scene.occluded(o[sel], targets, counters=c).cpu().numpy(), e)
    assert np.array_equal(scene.occluded(o[sel], targets, sort=True).cpu().numpy(), e)
    full = torch.zeros(2, dtype=torch.int64, device='cuda')
    scene.closest(o[sel], d[sel], t_min=1e-4, t_max=8.0, counters=full)
    print('any-hit cells, pairs %s against closest %s' % (c.tolist(), full.tolist()))
    assert int(c[1]) < int(full[1])                               # the early exit
    # every closest hit blocks the segment that passes it and not the one that stops short of it
    hit, near = soup_boundary()
    assert near.mean() <= 0.01
    eps = 1e-4
    t = exp[0][hit][:, None].astype(np.float64)
    oo, dd = o[hit].astype(np.float64), d[hit].astype(np.float64)
    short = scene.occluded(o[hit], (oo + t * dd * (1 - 2 * eps)).astype(F32), eps=eps).cpu().numpy()
    far = scene.occluded(o[hit], (oo + 2 * t * dd).astype(F32), eps=eps).cpu().numpy()
    assert not short[~near].any() and far[~near].all()


def test_closest_through_pixel_centres_sees_the_depth_of_the_rasteriser():
    hw, n = (60, 80), 4
    verts, faces = RR.tessellate_room(4)
    k, poses, o, d = T.room_camera_rays(n, hw)
    assert np.array_equal(bits(raytrace.camera_dirs(k[0], hw)), bits(T.camera_dirs_ref(k[0], hw)))
    depth = render.render_depth(verts, faces, k, poses, hw).cpu().numpy().reshape(-1)
    got = raytrace.Scene(verts, faces).closest(o, d)
    t, f = got.t.cpu().numpy(), got.face.cpu().numpy()
    interior = T.interior_pixels(f, n, hw)
    assert interior.sum() >= 0.5 * (f >= 0).sum() and (f >= 0).sum() > 0.9 * f.size
    both = interior & (depth > 0)
    assert both.sum() >= 0.9 * interior.sum()
    err = np.abs(t[both].astype(np.float64) - depth[both])
    print('largest |t - depth| on %d interior pixels: %.4e, bar %.4e' % (both.sum(), err.max(), RENDER_BAR))
    assert err.max() <= RENDER_BAR


def test_a_lidar_sweep_becomes_a_volume():
    """The sweep is what points.integrate takes, and the volume it gives agrees with the voxelised mesh: every voxel of
    the fused sweep's surface band (known() == 1, observed) lies within vs (1 + sqrt(3) / 2), under two voxels, of the
    mesh as voxelize.mesh_to_volume measures it, except at true depth discontinuities, where section P's running mean
    mixes rays that see different surfaces.  That region is computed from the restated sampling rules and holds 17 of
    the 6 841 band voxels, 9 of them beyond the bound: tests/test_raytrace_ref.py derives the bound and measures both."""
    case = T.lidar_room_case()
    verts, faces, pose, vs = case['verts'], case['faces'], case['pose'], T.SWEEP_VS
    rng = np.random.default_rng(4)
    colors = rng.integers(0, 256, (len(verts), 4), dtype=np.uint8)
    dirs = raytrace.lidar_dirs(16, 256)
    assert np.array_equal(bits(dirs), bits(case['dirs']))
    scene = raytrace.Scene(verts, faces, colors=colors)
    pts, org, oid, cols = raytrace.sweep(scene, pose[None], dirs, t_min=0.1, t_max=12.0)
    keep = case['keep']
    print('%d of %d rays of the sweep slip through a shared edge' % ((~keep).sum(), len(keep)))
    assert keep.sum() >= 0.99 * len(keep)                         # a closed room: only edge slips are lost
    assert tuple(pts.shape) == (keep.sum(), 3) and np.array_equal(bits(pts), bits(case['points']))
    assert oid.dtype == torch.int32 and not oid.any() and np.array_equal(bits(org), bits(case['origins']))
    assert cols.dtype == torch.uint8
    assert np.array_equal(cols.cpu().numpy(), T.colors_ref(case['face'], case['uv'], faces, colors)[keep])
    assert raytrace.sweep(raytrace.Scene(verts, faces), pose, dirs)[3] is None
    # the sweep through the point entrance against the mesh through the mesh entrance
    vol = points.integrate(fusion.TSDFVolume(T.SWEEP_DIMS, vs, case['w2g'], color=True), pts, org, origin_id=oid, color=cols)
    exact = voxelize.mesh_to_volume(verts, faces, T.SWEEP_DIMS, vs, case['w2g'], band=3.0)
    band = (vol.known() == 1) & (vol.weight() > 0)
    far = band & ~(exact.sdf().abs() <= T.SWEEP_BOUND * vs)       # beyond the mesh volume's own band counts as far
    region = torch.from_numpy(T.discontinuity_voxels(case)).to(band.device)
    print('%d band voxels, %d of them in the discontinuity region, %d beyond the bound, %d of those outside the region'
          % (int(band.sum()), int((band & region).sum()), int(far.sum()), int((far & ~region).sum())))
    assert int(band.sum()) > 2000 and not (far & ~region).any()
    assert int((band & region).sum()) <= T.SWEEP_REGION_VOXELS and int(far.sum()) <= T.SWEEP_FAR_VOXELS


def test_visible_from():
    quad = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    scene = raytrace.Scene(quad, faces)
    rng = np.random.default_rng(1)
    xy = rng.uniform(-0.5, 0.5, (300, 2))
    below = np.concatenate([xy, np.zeros((300, 1))], 1)           # behind the quad for eyes above it
    above = np.concatenate([xy, np.full((300, 1), 2.0)], 1)
    beside = below + [6.0, 0.0, 0.0]
    samples = np.concatenate([below, above, beside]).astype(F32)
    eyes = np.array([[0.0, 0.0, 3.0], [0.2, -0.1, 4.0], [-0.3, 0.2, 3.5]], F32)
    for max_rays in (1 << 22, 1000):                              # all eyes at once; one eye per chunk
        seen = raytrace.visible_from(scene, samples, eyes, max_rays=max_rays).cpu().numpy()
        assert not seen[:300].any() and seen[300:].all()
    assert raytrace.visible_from(scene, samples, np.array([[0.0, 0.0, -3.0]], F32)).cpu().numpy()[:300].all()
    ref = ~T.occluded_ref(np.repeat(samples, 3, 0), np.tile(eyes, (len(samples), 1)), quad, faces).reshape(-1, 3).all(1)
    assert np.array_equal(raytrace.visible_from(scene, samples, eyes).cpu().numpy(), ref)


def test_the_distance_index_is_unchanged_by_the_guard_keyword():
    """TriangleIndex without a guard lists faces exactly as before; with one it lists them in more cells and answers
    distance queries with the same bits."""
    verts, faces = RR.triangle_soup(300)
    plain = meshdist.TriangleIndex(verts, faces)
    grid = M.GridRef(verts, faces, plain.cell)
    assert plain.guard == 0 and np.array_equal(plain.offsets.cpu().numpy(), grid.offsets)
    guarded = raytrace.Scene(verts, faces).index
    assert guarded.n_refs > plain.n_refs and guarded.dims == plain.dims
    pts = M.near_surface_points(verts, faces, 500, 3)
    (d0, f0), (d1, f1) = plain.distance(pts), guarded.distance(pts)
    assert torch.equal(d0, d1) and torch.equal(f0, f1)
