"""CPU: tracking with colour as restated in tests/track_color_ref.py: that the Jacobian of
rule T4 is the derivative of its residual, that the combined step of rule T6 holds a view of one textured plane that
geometry alone loses, that colour does no harm where geometry suffices, and the accuracy figures the GPU tests assert
against.  No GPU, no sgnn_amd.track kernels; the device side is compared with this restatement in
tests/test_gpu_track_color.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_color_ref as FC  # noqa: E402
import track_color_ref as TC  # noqa: E402
import track_ref as T  # noqa: E402

F32 = np.float32
HW = TC.WALL_HW
TRANS, ROT = T.TRANS, T.ROT


@pytest.fixture(scope='module')
def wall():
    return TC.wall_volume()


@pytest.fixture(scope='module')
def wall_views():
    return [TC.wall_view(seed) for seed in range(4)]


def test_the_wall_is_what_the_issue_asks_for(wall, wall_views):
    """One plane about 2 m away fills every view; every period of the texture is at least 8 voxels and at least 4
    pixels of the coarsest level; the geometric system at the true pose is above track_ref.MAX_CONDITION (a plane: not
    even positive definite) and the system of rule T6 at the default weight is below it.  The texture first tried
    (periods 0.7 m and 0.9 m, amplitude 60 each, directions 75 degrees apart) met this; neither it nor the weight was
    changed afterwards."""
    k = TC.wall_intrinsics()
    coarsest = 2.0 / (float(k[0]) / 4)                                      # metres per pixel of level 2 at 2 m
    assert min(TC.WALL_PERIODS) >= 8 * TC.WALL_VS and min(TC.WALL_PERIODS) >= 4 * coarsest
    assert TC.WALL_MEAN - 2 * TC.WALL_AMPLITUDE >= 0 and TC.WALL_MEAN + 2 * TC.WALL_AMPLITUDE <= 255
    for seed, (depth, rgba, k, pose) in enumerate(wall_views):
        assert np.isfinite(depth).all() and (rgba[..., 3] == 255).all() and 1.8 < depth.min() and depth.max() < 2.6
        assert (rgba[..., 0] == rgba[..., 1]).all() and (rgba[..., 0] == rgba[..., 2]).all()
        geo, both = TC.conditioning(depth, rgba, k, pose, wall)
        print('seed %d: condition %.3g with geometry alone, %.1f with colour at lambda = %g' % (seed, geo, both,
                                                                                               TC.COLOR_WEIGHT))
        assert geo > T.MAX_CONDITION and both < T.MAX_CONDITION


def test_intensity_and_halving_by_hand():
    rgba = np.array([[255, 255, 255, 255], [0, 0, 0, 255], [10, 20, 30, 0], [1, 2, 3, 7], [200, 200, 200, 1]], np.uint8)
    got = TC.intensity(rgba)
    assert got.dtype == F32 and np.isnan(got[2])
    assert got[0] == 255 and got[1] == 0 and got[3] == F32((77 + 300 + 87) / 256.0) and got[4] == 200
    nan, inf = np.nan, np.inf
    d = np.array([[1.00, 1.02, 2.00, -inf],
                  [1.04, 1.50, -inf, -inf],
                  [-inf, -inf, 3.00, 3.02],
                  [1.00, -inf, 3.04, 3.06]], F32)
    c = np.array([[10, 20, 7, 9],
                  [nan, 90, 9, 9],
                  [1, 2, 30, nan],
                  [nan, 5, 50, 70]], F32)
    out = TC.halve_intensity(d, c, 0.05)
    assert out.shape == (2, 2) and out.dtype == F32
    assert out[0, 0] == (F32(10) + F32(20)) / F32(2)        # 1.50 is beyond delta, 1.04 has no intensity
    assert out[0, 1] == 7                                   # the one pixel with a depth
    assert np.isnan(out[1, 0])                              # the one pixel with a depth has no intensity
    assert out[1, 1] == (F32(30) + F32(50)) / F32(2)        # 3.02 has no intensity, 3.06 - 3.00 > 0.05 in fp32
    assert TC.halve_intensity(np.ones((5, 3), F32), np.ones((5, 3), F32)).shape == (2, 1)


def residual64(depth, inten, k, md, mi, Tm):
    """The residual of rule T4 in fp64 for every pixel, no gates: the bilinear interpolant of the model intensity at
    the projection of the moved live point, minus the live intensity; NaN outside the model frame."""
    k64 = np.asarray(k, np.float64)
    h, w = depth.shape
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = depth.astype(np.float64)
    p = np.stack([(i - k64[2]) / k64[0] * d, (j - k64[3]) / k64[1] * d, d, np.ones_like(d)], -1)
    q = p @ np.asarray(Tm, np.float64)[:3].T
    x, y = q[..., 0] * k64[0] / q[..., 2] + k64[2], q[..., 1] * k64[1] / q[..., 2] + k64[3]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ok = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    x0, y0 = np.where(ok, x0, 0), np.where(ok, y0, 0)
    a, b = x - x0, y - y0
    m = mi.astype(np.float64)
    im = (m[y0, x0] * (1 - a) + m[y0, x0 + 1] * a) * (1 - b) + (m[y0 + 1, x0] * (1 - a) + m[y0 + 1, x0 + 1] * a) * b
    return np.where(ok, im - inten, np.nan), x0 + w * y0


def test_jacobian_against_central_differences(wall, wall_views):
    """J of rule T4 is d r / d xi of the left-multiplied twist: central differences of the residual in fp64 with a step
    of 1e-6 (the interpolant is piecewise bilinear, so pixels whose cell changes under the step are left out) agree
    with the fp32 Jacobian to fp32 rounding.  The bound: intensities up to 255 carry half an ulp, 8e-6, and a gradient is
    built from four of them in about eight operations, 6e-5; times fx / q.z = 26 for k, times |q| < 2.6 m for the
    rotational entries: 5e-3 absolute, plus 1e-4 of the row's largest entry for the products.  A wrong sign or a wrong
    row misses by the row's scale, hundreds."""
    depth, rgba, k, pose = wall_views[0]
    inten = TC.intensity(rgba)
    md, mn, mc = TC.cast_grid_color(wall, k, pose, HW)
    T0 = T.pair_matrix(pose, T.perturbed(pose, 0, 0.01, 0.5))
    J, r, residual, cell = TC.color_terms(depth, inten, k, md, mn, mc, k, T0)
    used = cell >= 0
    assert used.sum() > 0.5 * HW[0] * HW[1]
    r0, c0 = residual64(depth, inten, k, md, mc, T0)
    assert np.array_equal(c0[used], cell[used]) and np.abs(r0[used] - residual[used]).max() < 1e-3
    step = 1e-6
    numeric, same_cell = np.zeros(HW + (6,)), used.copy()
    for a in range(6):
        xi = np.zeros(6)
        xi[a] = step
        plus, cp = residual64(depth, inten, k, md, mc, T.exp_se3(xi) @ T0)
        minus, cm = residual64(depth, inten, k, md, mc, T.exp_se3(-xi) @ T0)
        numeric[..., a] = (plus - minus) / (2 * step)
        same_cell &= (cp == c0) & (cm == c0)
    keep = same_cell[used]
    assert keep.mean() > 0.99
    err = np.abs(numeric[used][keep] - J[keep].astype(np.float64))
    scale = np.abs(J[keep]).max(1, keepdims=True).astype(np.float64)
    print('Jacobian: %d pixels, worst |numeric - J| / row scale = %.3g' % (keep.sum(), (err / scale).max()))
    assert (err <= 5e-3 + 1e-4 * scale).all()


def test_gauss_newton_model(wall, wall_views):
    """Section I's linear-model check on the photometric energy: after a step of |xi| = 1e-3 along the Gauss-Newton
    direction of rule T6's combined system, the new E_c is the colour system's linear model E + 2 g.xi + xi^T A xi
    within 25 % of the predicted change."""
    depth, rgba, k, pose = wall_views[0]
    inten = TC.intensity(rgba)
    md, mn, mc = TC.cast_grid_color(wall, k, pose, HW)
    T0 = T.pair_matrix(pose, T.perturbed(pose, 0, TRANS, ROT))
    sg = T.normal_equations(depth, k, md, mn, k, T0)
    sc = TC.color_equations(depth, inten, k, md, mn, mc, k, T0)
    a, g, e0, n0 = T.unpack(sc)
    xi = T.step(TC.combine(sg, sc))
    xi = xi * (1e-3 / np.linalg.norm(xi))
    predicted = e0 + 2 * g @ xi + xi @ a @ xi
    s1 = TC.color_equations(depth, inten, k, md, mn, mc, k, T.exp_se3(xi) @ T0)
    e1, n1 = s1[27], int(s1[28])
    print('E_c %.3f -> %.3f, linear model %.3f; pairs %d -> %d' % (e0, e1, predicted, n0, n1))
    assert predicted < e0 and abs(n1 - n0) <= 0.01 * n0
    assert abs(e1 - predicted) <= 0.25 * (e0 - predicted)
    wrong = TC.color_equations(depth, inten, k, md, mn, mc, k, T.exp_se3(-xi) @ T0)[27]
    assert wrong > e0


def test_wall_alignment(wall, wall_views):
    worst = [0.0, 0.0]
    for seed, (depth, rgba, k, pose) in enumerate(wall_views):
        guess = T.perturbed(pose, seed, TRANS, ROT)
        res = TC.align_color(depth, rgba, k, guess, guess, wall)
        dt, dr = T.pose_error(pose, res.pose)
        slide, slide0 = TC.in_plane_error(pose, res.pose, TC.WALL_NORMAL), TC.in_plane_error(pose, guess, TC.WALL_NORMAL)
        print('seed %d: pairs %d, colour pairs %d, rmse %.6f m, colour rmse %.3f levels, error %.6f m %.5f deg, '
              'in-plane %.6f m (guess %.6f m)' % (seed, res.pairs, res.color_pairs, res.rmse, res.color_rmse, dt, dr,
                                                 slide, slide0))
        assert res.ok and res.iterations == 19 and res.color_pairs > 0.5 * HW[0] * HW[1]
        assert dt < TRANS and dr < ROT and slide < slide0                   # the condition of the issue
        geo = T.align(depth, k, guess, guess, wall)                         # geometry alone: lost, or no closer in-plane
        assert not geo.ok or TC.in_plane_error(pose, geo.pose, TC.WALL_NORMAL) >= slide0
        worst = [max(worst[0], dt), max(worst[1], dr)]
    print('worst over the seeds: %.6f m %.5f deg' % tuple(worst))
    # the record the GPU test relies on is this run's result (5 %: the host's LAPACK and libm may differ in the last bits)
    assert abs(worst[0] - TC.WALL_ALIGN_ERROR[0]) <= 0.05 * TC.WALL_ALIGN_ERROR[0]
    assert abs(worst[1] - TC.WALL_ALIGN_ERROR[1]) <= 0.05 * TC.WALL_ALIGN_ERROR[1]


def test_wall_sequence_drift():
    depth, rgba, k, poses = TC.wall_sequence(6)
    grid = TC.wall_grid()
    est, results = TC.track_sequence(grid, depth, rgba, k, poses[0])
    assert all(r.ok for r in results) and np.array_equal(est[0], poses[0])
    for f in range(6):
        print('frame %d: %d pairs, %d colour pairs, error %.6f m %.5f deg' % ((f, results[f].pairs, results[f].color_pairs)
                                                                              + T.pose_error(poses[f], est[f])))
    dt, dr = T.pose_error(poses[5], est[5])
    step_t, step_r = T.pose_error(poses[0], poses[5])
    assert dt < step_t and dr < step_r                                      # tracking beats standing still
    assert abs(dt - TC.WALL_SEQUENCE_DRIFT[0]) <= 0.05 * TC.WALL_SEQUENCE_DRIFT[0]
    assert abs(dr - TC.WALL_SEQUENCE_DRIFT[1]) <= 0.05 * TC.WALL_SEQUENCE_DRIFT[1]
    # the volume holds what integrating at the tracked poses gives, colour included
    again = TC.wall_grid().integrate(depth, k, est, rgba)
    assert np.array_equal(again.sdf.view(np.int32), grid.sdf.view(np.int32)) and np.array_equal(again.state(), grid.state())
    # without colour the second frame is already lost
    _, plain = T.track_sequence(TC.wall_grid(), depth, k, poses[0])
    assert [r.ok for r in plain] == [True] + [False] * 5


def test_colour_does_no_harm_in_the_room():
    """track_ref's four conditioned views of the painted room (flat colours, so the only gradients are the borders
    between primitives, blurred by 5 cm voxels): the error shrinks for every seed; the worst value is recorded."""
    room = TC.painted_room_volume()
    worst = [0.0, 0.0]
    for seed in range(4):
        depth, k, pose, f, cond = T.test_view(seed, HW, room)
        painted, rgba = FC.painted_frames(k[None], pose[None], HW)
        assert np.array_equal(painted[0], depth)
        guess = T.perturbed(pose, seed, TRANS, ROT)
        res = TC.align_color(depth, rgba[0], k, guess, guess, room)
        dt, dr = T.pose_error(pose, res.pose)
        print('seed %d frame %d: pairs %d, colour pairs %d, colour rmse %.3f levels, error %.6f m %.5f deg (geometry '
              'alone %.6f m %.5f deg)' % ((seed, f, res.pairs, res.color_pairs, res.color_rmse, dt, dr) +
                                          T.pose_error(pose, T.align(depth, k, guess, guess, room).pose)))
        assert res.ok and dt < TRANS and dr < ROT
        worst = [max(worst[0], dt), max(worst[1], dr)]
    print('worst over the seeds: %.6f m %.5f deg' % tuple(worst))
    assert abs(worst[0] - TC.ROOM_ALIGN_ERROR[0]) <= 0.05 * TC.ROOM_ALIGN_ERROR[0]
    assert abs(worst[1] - TC.ROOM_ALIGN_ERROR[1]) <= 0.05 * TC.ROOM_ALIGN_ERROR[1]


def test_empty_systems(wall, wall_views):
    depth, rgba, k, pose = wall_views[0]
    inten = TC.intensity(rgba)
    md, mn, mc = TC.cast_grid_color(wall, k, pose, HW)
    bad = np.eye(4)
    bad[1, 2] = np.nan
    for d, c, m in ((np.full(HW, -np.inf, F32), inten, np.eye(4)), (depth, inten, bad),
                    (depth, np.full(HW, np.nan, F32), np.eye(4))):
        J, r, residual, cell = TC.color_terms(d, c, k, md, mn, mc, k, m)
        assert len(r) == 0 and np.isnan(residual).all() and (cell == -1).all()
        assert not TC.color_equations(d, c, k, md, mn, mc, k, m).any()
    res = TC.align_color(depth, rgba, k, pose, bad, wall)
    assert not res.ok and res.pairs == 0 and res.color_pairs == 0 and res.iterations == 1
