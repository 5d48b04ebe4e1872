"""CPU: the NumPy restatement of the TSDF fusion rules (tests/fusion_ref.py) against analytic geometry, the host
helpers of sgnn_amd.fusion (frustum box, voxel->camera matrix, OBB, rounding) against the restatement, and the
.sdf / .knw writer against the readers."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402

from sgnn_amd import data, fusion  # noqa: E402

F32 = np.float32


def wall_setup(D=1.3, vs=0.02, dims=(40, 40, 120), dtype=np.float64):
    """A fronto-parallel wall at depth D in front of a camera at the world origin looking along +z; the grid's
    world origin sits at (-0.4, -0.4, 0), so voxel (i, j, k) is at z = k * vs."""
    h, w = 48, 64
    k = np.array([40.0, 40.0, (w - 1) / 2.0, (h - 1) / 2.0], F32)
    c2w = np.eye(4)[None]
    depth = R.render(k, c2w[0], (h, w), planes=[((0, 0, 1), D)])[None]
    w2g = R.grid_transform((-0.4, -0.4, 0.0), vs)
    g = R.Grid(dims, vs, w2g, dtype=dtype).integrate(depth, k[None], c2w)
    return g, D, vs


def test_round_away_is_c_round():
    x = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 0.49999997, -0.49999997, 7.0], F32)
    exp = np.array([-3, -2, -1, 1, 2, 3, 0, -0, 7], F32)
    assert np.array_equal(R.round_away(x), exp)
    assert np.array_equal(fusion.round_half_away(x), exp)
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(10000) * 100).astype(F32)
    y[::7] = np.floor(y[::7]) + F32(0.5)
    assert np.array_equal(R.round_away(y), fusion.round_half_away(y))


def test_wall_gives_its_distance_in_the_band():
    g, D, vs = wall_setup()
    # the column on the optical axis: voxel (20, 20, k) sits at camera (0, 0, k*vs)
    col_sdf, col_free, col_w = g.sdf[:, 20, 20], g.free[:, 20, 20], g.weight[:, 20, 20]
    z = np.arange(len(col_sdf)) * vs
    trunc = 3 * vs + D * vs
    band = (z > 0.0) & (D - z > -trunc)                                # z = 0 projects to 0/0: outside
    seen = band & (D - z <= trunc)
    assert seen.sum() >= 8
    assert np.allclose(col_sdf[seen], (D - z)[seen], rtol=0, atol=1e-6)     # D is rendered to fp32
    assert np.allclose(col_sdf[band & ~seen], trunc)                   # clamped in front of the band
    assert (col_sdf[~band & (z > D)] == -np.inf).all()                 # nothing behind -trunc
    assert (col_w[~band & (z > D)] == 0).all()
    front = (z < D) & (z > 0)
    assert (col_free[front] == 1).all() and (col_free[z > D] == 0).all()
    wu = max(4.5 * (1 - (D - 0.4) / 3.6), 1.0)
    assert (col_w[band] == int(wu)).all()


def test_wall_fp32_restatement_agrees_with_fp64():
    g64, _, vs = wall_setup()
    g32, _, _ = wall_setup(dtype=F32)
    # voxels that sit on a pixel or band boundary may fall to either side in fp32
    differ = np.isfinite(g64.sdf) != np.isfinite(g32.sdf)
    assert differ.sum() <= 1e-3 * np.isfinite(g64.sdf).sum()
    fin = np.isfinite(g64.sdf) & np.isfinite(g32.sdf)
    assert fin.sum() > 1000 and np.abs(g64.sdf[fin] - g32.sdf[fin]).max() < 1e-5
    assert (g64.weight[fin] == g32.weight[fin]).mean() > 0.999


def test_running_average_and_saturation():
    """Repeating one frame keeps the sdf (a weighted mean of equal values) and saturates the weight at 255."""
    h, w = 24, 32
    k = np.array([20.0, 20.0, (w - 1) / 2.0, (h - 1) / 2.0], F32)
    depth = R.render(k, np.eye(4), (h, w), planes=[((0, 0, 1), 0.5)])
    w2g = R.grid_transform((-0.2, -0.2, 0.0), 0.02)
    g1 = R.Grid((20, 20, 40), 0.02, w2g).integrate(depth[None], k[None], np.eye(4)[None])
    g = R.Grid((20, 20, 40), 0.02, w2g).integrate(np.repeat(depth[None], 70, 0), np.tile(k, (70, 1)),
                                                    np.repeat(np.eye(4)[None], 70, 0))
    assert g.weight.max() == 255 and g1.weight.max() == 4
    fin = np.isfinite(g1.sdf)
    assert np.abs(g.sdf[fin] - g1.sdf[fin]).max() < 1e-6


def test_camera_matrix_and_boxes_match_the_restatement():
    d, k, poses = R.room_frames(16, (48, 64), seed=3)
    w2g = R.grid_transform((0.0, 0.0, 0.0), 0.085)
    dims = (48, 48, 48)
    m = fusion.camera_matrix(poses, w2g)
    for f in range(len(poses)):
        assert np.array_equal(m[f], R.voxel_to_camera(poses[f], w2g))
        exp = R.frame_box(k[f], poses[f], (48, 64), w2g, dims)
        got = fusion.frustum_box(k[f], poses[f], (48, 64), w2g, dims)
        assert exp is not None and np.array_equal(got, exp), (f, got, exp)
    # a frame looking away from a grid it is outside of, and an invalid pose, touch nothing
    away = R.look_at((-5.0, 1.0, 1.0), (-9.0, 1.0, 1.0))
    assert R.frame_box(k[0], away, (48, 64), w2g, dims) is None
    assert np.array_equal(fusion.frustum_box(k[0], away, (48, 64), w2g, dims), fusion.EMPTY_BOX)
    bad = poses[0].copy()
    bad[0, 0] = -np.inf
    assert np.array_equal(fusion.frustum_box(k[0], bad, (48, 64), w2g, dims), fusion.EMPTY_BOX)


def test_obb_matches_the_restatement():
    rng = np.random.default_rng(1)
    obb = np.array([3.3, -2.0, 1.5, 30.0, 12.0, 0.0, -8.0, 20.0, 0.0, 0.0, 0.0, 25.5], F32)
    q = rng.integers(-10, 50, size=(20000, 3))
    got = fusion.obb_contains(obb, q)
    assert np.array_equal(got, R.in_obb(obb, q))
    assert 0.05 < got.mean() < 0.95


def test_raw_depth_restatement():
    raw = np.array([[0, 100, 5000], [65535, 1000, 12001]], np.uint16)
    out = R.raw_to_metric(raw, 1000.0, (2, 3))
    assert out[0, 0] == -np.inf and out[1, 0] == -np.inf and out[1, 2] == -np.inf   # 0, 65.5 m, 12.001 m
    assert out[0, 1] == F32(0.001) * F32(100) and out[1, 1] == F32(0.001) * F32(1000)
    k = R.adapt_intrinsics([577.6, 578.7, 318.9, 242.7], (480, 640), (240, 320))
    assert np.array_equal(k, fusion.adapt_intrinsics([577.6, 578.7, 318.9, 242.7], (480, 640), (240, 320)))


def test_known_codes():
    g = R.Grid((4, 1, 1), 0.1, np.eye(4))
    g.sdf[0, 0] = np.array([-np.inf, -0.35, 0.05, 0.2], F32)
    assert g.known()[0, 0].tolist() == [2, 4, 1, 0]


def test_writer_round_trip(tmp_path):
    d, k, poses = R.room_frames(12, (48, 64), seed=5)
    w2g = R.grid_transform((0.0, 0.0, 0.0), 0.1)
    g = R.Grid((41, 33, 27), 0.1, w2g).integrate(d, k, poses)
    locs, vals = g.sparse(6.0)
    known = g.known()
    assert len(vals) > 100 and (known == 1).any() and (known == 2).any()
    path = str(tmp_path / 'scan.sdf')
    fusion.write_scan(path, (27, 33, 41), g.vs, w2g, locs, vals, known)
    (rl, rv), dims, rw = data.load_scene(path)
    assert dims == [27, 33, 41] and np.array_equal(rw, w2g)
    assert np.array_equal(rl, locs[:, ::-1].astype(np.int32))
    assert np.array_equal(rv, vals / F32(0.1))
    assert np.array_equal(data.load_scene_known(str(tmp_path / 'scan.knw')), known)
    raw = open(path, 'rb').read()
    n = int(np.frombuffer(raw, '<u8', 1, data.HEADER_BYTES)[0])
    assert n == len(vals)
    assert raw[data.HEADER_BYTES + 8:data.HEADER_BYTES + 8 + 12 * n] == locs.astype('<u4').tobytes()
