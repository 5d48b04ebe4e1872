"""No GPU: the NumPy restatement of the ray-tracing rules (tests/raytrace_ref.py) against the same construction in
fp64, its grid walk against its brute force, and the ray patterns of sgnn_amd.raytrace against their stated formulas."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshdist_ref as M  # noqa: E402
import raytrace_ref as T  # noqa: E402
import render_ref as RR  # noqa: E402

F32 = np.float32
# the largest |t32 - t64| of the restatement on the fixed case below, measured on the CPU, and the bar: 4 times that,
# as headroom for other seeds (INTEGRATION.md section W quotes both)
MEASURED_T_ERR = 1.6925e-4
T_BAR = 4.0 * MEASURED_T_ERR


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def test_restatement_against_fp64():
    """render_ref.triangle_soup(300), 2 000 rays: hit / miss and the face agree with fp64 on every ray that fp64 does
    not place near a decision boundary; t within the bar where the ray meets its face at a cosine of 0.1 or more."""
    verts, faces = RR.triangle_soup(300)
    o, d = T.soup_rays(verts, faces, 2000, seed=3)
    t32, f32, uv32 = T.closest_ref(o, d, verts, faces)
    t64, f64, uv64 = T.closest_ref(o, d, verts, faces, dtype=np.float64)
    near = T.boundary64(o, d, verts, faces)
    print('%d of %d rays hit, %d near a boundary' % ((f64 >= 0).sum(), len(o), near.sum()))
    assert near.mean() <= 0.01
    assert (f64 >= 0).sum() >= 300 and (f64 < 0).sum() >= 300
    assert np.array_equal(f32[~near], f64[~near])
    steep = ~near & (f64 >= 0) & (T.incidence_cos(d, verts, faces, f64) >= 0.1)
    err = np.abs(t32[steep].astype(np.float64) - t64[steep])
    print('largest |t32 - t64| over %d rays: %.4e (t up to %.1f), bar %.4e' % (steep.sum(), err.max(), t64[steep].max(), T_BAR))
    assert steep.sum() >= 250 and err.max() <= T_BAR
    assert np.abs(uv32[steep] - uv64[steep]).max() <= 1e-3
    # any-hit agrees with the closest hit, segment by segment
    assert np.array_equal(T.any_hit(o, d, verts, faces, 0.0, np.where(f32 >= 0, t32 * F32(2), F32(1))), f32 >= 0)
    hit_before = T.any_hit(o, d, verts, faces, 0.0, t32)           # nothing lies in front of the closest hit
    assert not hit_before[f32 >= 0].any()


def test_walk_equals_brute_force_in_the_restatement():
    """The walk of rule 4, restated ray by ray, returns the brute-force result bit for bit for three pitches, and in a
    one-cell grid it tests every usable face for every ray that enters the grid."""
    verts, faces = RR.triangle_soup(300)
    o, d = T.soup_rays(verts, faces, 300, seed=5)
    for cell in (M.default_cell_ref(verts, faces), 1000.0, 0.3):
        grid = T.GuardGrid(verts, faces, cell)
        ao, ad = T.awkward_rays(grid)
        oo, dd = np.concatenate([o, ao]), np.concatenate([d, ad])
        for kw in (dict(), dict(t_min=0.5, t_max=6.0), dict(cull_back=True)):
            exp = T.closest_ref(oo, dd, verts, faces, **kw)
            t, f, uv, _, cells, pairs = T.walk_ref(oo, dd, grid, **kw)
            assert np.array_equal(bits(t), bits(exp[0])) and np.array_equal(f, exp[1])
            assert np.array_equal(bits(uv), bits(exp[2]))
            if grid.dims == (1, 1, 1):
                assert pairs == cells * len(faces) and 0 < cells < len(oo)
        assert (exp[1][-6:] == -1).all()                          # the rays that cannot hit anything
        seg = np.where(np.isfinite(exp[0]), exp[0], F32(1.0))
        for scale in (F32(0.5), F32(2.0)):
            hit = T.walk_ref(oo, dd, grid, t_max=seg * scale, first=True)[3]
            assert np.array_equal(hit, T.any_hit(oo, dd, verts, faces, 0.0, seg * scale))


def test_room_walk_and_shared_edges():
    """The closed room seen from inside: rays through the middle of faces hit; the walk equals brute force for rays
    aimed exactly at vertices and edge midpoints, where a ray may slip between two faces (rule 5)."""
    verts, faces = RR.tessellate_room(2)
    eye = np.array([2.0, 1.6, 1.3])
    v = verts.astype(np.float64)
    mids = v[faces].mean(1)
    edges = ((v[faces] + v[faces[:, [1, 2, 0]]]) / 2).reshape(-1, 3)
    targets = np.concatenate([mids, v, edges])
    d = (targets - eye).astype(F32)
    o = np.repeat(eye[None], len(d), 0).astype(F32)
    exp = T.closest_ref(o, d, verts, faces)
    assert (exp[1][:len(mids)] >= 0).all()
    grid = T.GuardGrid(verts, faces, 0.4)
    t, f, uv = T.walk_ref(o, d, grid)[:3]
    assert np.array_equal(bits(t), bits(exp[0])) and np.array_equal(f, exp[1]) and np.array_equal(bits(uv), bits(exp[2]))
    print('%d of %d rays at vertices and edge midpoints slip through' % ((exp[1][len(mids):] < 0).sum(), len(d) - len(mids)))


def test_a_fine_grid_under_grazing_rays():
    """The limit of rule 4's argument: 1000 cells per axis over 30 m, rays that meet a face at an incidence cosine of
    0.002 to 0.1.  The walk still equals brute force; rule 1's error along the ray, measured against fp64, reaches 0.85
    of the guard cell / 64 here (0.08 at 250 cells), which is where section W puts the limit: n cells per axis cover
    incidence cosines down to about n / 2^19."""
    for ncell, measured in ((1000, 0.8502), (250, 0.0799)):
        verts, faces, o, d, cell = T.grazing_case(30.0, ncell)
        grid = T.GuardGrid(verts, faces, cell)
        assert min(grid.dims) >= ncell
        exp = T.closest_ref(o, d, verts, faces)
        t, f, uv = T.walk_ref(o, d, grid)[:3]
        assert (exp[1] >= 0).sum() >= 0.9 * len(o)
        assert np.array_equal(bits(t), bits(exp[0])) and np.array_equal(f, exp[1]) and np.array_equal(bits(uv), bits(exp[2]))
        e64 = T.closest_ref(o, d, verts, faces, dtype=np.float64)
        both = (exp[1] >= 0) & (e64[1] == exp[1])
        err = np.abs(exp[0][both] - e64[0][both]) * np.linalg.norm(d[both].astype(np.float64), axis=1)
        print('%d cells: largest error along the ray %.4f of the guard %.3g' % (ncell, err.max() / float(grid.guard), grid.guard))
        assert err.max() / float(grid.guard) <= 1.01 * measured


def test_the_rasteriser_bar_comes_from_the_restatements():
    """render_ref against the brute-force restatement on the interior pixels of the four 60 x 80 room frames: the source
    of MEASURED_RENDER_ERR in tests/test_gpu_raytrace.py, whose bar is four times that."""
    hw, n = (60, 80), 4
    verts, faces = RR.tessellate_room(4)
    k, poses, o, d = T.room_camera_rays(n, hw)
    depth = RR.render_ref(verts, faces, k, poses, hw).reshape(-1)
    t, f, _ = T.closest_ref(o, d, verts, faces)
    interior = T.interior_pixels(f, n, hw)
    assert interior.sum() == 13981 and interior.sum() >= 0.5 * (f >= 0).sum() and (depth[interior] > 0).all()
    err = np.abs(t[interior].astype(np.float64) - depth[interior]).max()
    print('largest |t - depth| on %d interior pixels: %.4e' % (interior.sum(), err))
    assert err <= T.MEASURED_RENDER_ERR


def test_sweep_voxels_away_from_the_mesh_lie_at_depth_discontinuities():
    """The sweep-to-volume check of tests/test_gpu_raytrace.py with every part restated on the CPU (points_ref,
    meshdist_ref).  A voxel of the fused sweep's surface band (|sdf| <= vs, observed) whose rays all see one plane lies
    within vs (1 + sqrt(3) / 2) of the mesh: the voxel centre is at most sqrt(3) / 2 vs off each ray that samples it,
    and either some ray has |sdf| <= vs, or rays of both signs bracket the plane.  Measured: 1.0000002 vs.  The
    exceptions are voxels fed by rays that hit different planes more than a voxel apart in range (section P's mean mixes
    a carved value with one from behind the nearer surface): 17 of the 6 841 band voxels, 9 of them beyond the bound."""
    import points_ref as PR
    case = T.lidar_room_case()
    assert case['keep'].all()                                       # a closed room, and no ray slips through an edge
    vol = PR.integrate(PR.Volume(T.SWEEP_DIMS, T.SWEEP_VS, case['w2g']), case['points'], case['origins'],
                       np.zeros(len(case['points']), np.int64), carve=True)
    vs = F32(T.SWEEP_VS)
    band = (vol.weight > 0) & (vol.sdf <= vs) & (vol.sdf >= -vs)
    region = T.discontinuity_voxels(case)
    iz, iy, ix = np.nonzero(band)
    centres = PR.affine(PR.grid2world(case['w2g']), np.stack([ix, iy, iz], 1).astype(F32))
    dist = M.distance_ref(centres, case['verts'], case['faces'])[0]
    far = dist > T.SWEEP_BOUND * T.SWEEP_VS
    inside = region[iz, iy, ix]
    print('%d band voxels, %d in the discontinuity region, %d beyond the bound, largest distance outside the region %.7f vs'
          % (band.sum(), inside.sum(), far.sum(), dist[~inside].max() / T.SWEEP_VS))
    assert band.sum() == 6841 and not (far & ~inside).any()
    assert inside.sum() <= T.SWEEP_REGION_VOXELS and far.sum() <= T.SWEEP_FAR_VOXELS


def test_lidar_dirs():
    from sgnn_amd import raytrace
    for channels, steps, up, down in ((32, 1024, 15.0, -25.0), (16, 256, 15.0, -15.0), (1, 7, 10.0, -30.0), (5, 1, 90.0, -90.0)):
        d = raytrace.lidar_dirs(channels, steps, up, down).numpy()
        assert d.dtype == F32 and d.shape == (channels * steps, 3)
        assert np.array_equal(bits(d), bits(T.lidar_dirs_ref(channels, steps, up, down)))
        d64 = d.astype(np.float64).reshape(channels, steps, 3)
        assert np.abs(np.linalg.norm(d64, axis=-1) - 1).max() <= 2.0 ** -22
        el, az = T.lidar_angles(channels, steps, up, down)
        assert np.abs(np.arcsin(d64[..., 2]) - el[:, None]).max() <= 1e-6
        flat = np.hypot(d64[..., 0], d64[..., 1]) > 1e-6          # the azimuth of a vertical ray is arbitrary
        diff = np.angle(np.exp(1j * (np.arctan2(d64[..., 1], d64[..., 0]) - az[None])))
        assert np.abs(diff[flat]).max() <= 1e-6
        if channels > 1:
            assert abs(np.degrees(el[0]) - up) < 1e-12 and abs(np.degrees(el[-1]) - down) < 1e-12
    assert np.array_equal(bits(raytrace.lidar_dirs()), bits(T.lidar_dirs_ref()))


def test_panorama_dirs_cover_the_sphere():
    from sgnn_amd import raytrace
    for h, w in ((32, 64), (5, 3), (1, 1)):
        d = raytrace.panorama_dirs(h, w).numpy()
        assert d.shape == (h * w, 3) and np.array_equal(bits(d), bits(T.panorama_dirs_ref(h, w)))
        d64 = d.astype(np.float64)
        assert np.abs(np.linalg.norm(d64, axis=1) - 1).max() <= 2.0 ** -22
        # solid angle of a pixel: cos(lat) dlat dlon; the midpoint rule sums cos over the rows to x / sin(x) of the
        # exact 2 / dlat, x = pi / 2h, so the total is 4 pi x / sin(x)
        x = np.pi / (2 * h)
        total = (np.hypot(d64[:, 0], d64[:, 1]) * (np.pi / h) * (2 * np.pi / w)).sum()
        assert abs(total / (4 * np.pi) - x / np.sin(x)) <= 1e-6
    d64 = raytrace.panorama_dirs(32, 64).numpy().astype(np.float64)
    assert abs(total_solid(d64, 32, 64) / (4 * np.pi) - 1) <= (np.pi / 64) ** 2 / 5
    octant = (d64 > 0) @ np.array([1, 2, 4])
    assert np.array_equal(np.bincount(octant, minlength=8), np.full(8, 32 * 64 // 8))
    top_left = d64.reshape(32, 64, 3)[0, 0]
    assert top_left[2] > 0.99 and top_left[1] > 0 and top_left[0] < 0    # up; just left of straight behind


def total_solid(d64, h, w):
    return (np.hypot(d64[:, 0], d64[:, 1]) * (np.pi / h) * (2 * np.pi / w)).sum()


def test_camera_dirs_times_depth_is_the_back_projection_of_from_depth():
    import torch
    from sgnn_amd import points, raytrace
    h, w = 24, 32
    k = np.array([28.875, 29.125, 15.5, 11.25], F32)
    d = raytrace.camera_dirs(k, (h, w)).numpy()
    assert d.shape == (h * w, 3) and np.array_equal(bits(d), bits(T.camera_dirs_ref(k, (h, w)))) and (d[:, 2] == 1).all()
    rng = np.random.default_rng(0)
    depth = rng.uniform(0.4, 6.0, (1, h, w)).astype(F32)
    pts = points.from_depth(torch.from_numpy(depth), k[None], np.eye(4)[None])[0].numpy()
    mine = d * depth.reshape(-1, 1)
    # both are the exact point up to two roundings per component
    assert np.abs(mine - pts).max() <= 4 * 2.0 ** -24 * np.abs(pts).max()
    assert np.array_equal(mine[:, 2], pts[:, 2])


def test_malformed_patterns_raise():
    import pytest
    from sgnn_amd import raytrace
    for call in (lambda: raytrace.lidar_dirs(0, 4), lambda: raytrace.lidar_dirs(4, 0), lambda: raytrace.lidar_dirs(4, 4, -5.0, 5.0),
                 lambda: raytrace.panorama_dirs(0, 4), lambda: raytrace.camera_dirs([1.0, 1.0, 0.0], (4, 4)),
                 lambda: raytrace.camera_dirs([1.0, 1.0, 0.0, 0.0], (0, 4))):
        with pytest.raises(ValueError):
            call()
