"""CPU: the tracking rules of INTEGRATION.md section I as restated in tests/track_ref.py: that they converge, that the
linear model they build is the right one, and the accuracy figures the GPU tests assert against.  No GPU, no
sgnn_amd.track kernels; the device side is compared with this restatement in tests/test_gpu_track.py."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402
import track_ref as T  # noqa: E402

F32 = np.float32
HW = (48, 64)
VS = 0.05
TRANS, ROT, ALIGN_ERROR, SEQUENCE_DRIFT = T.TRANS, T.ROT, T.ALIGN_ERROR, T.SEQUENCE_DRIFT


@pytest.fixture(scope='module')
def grid():
    return T.room_volume(VS)


@pytest.fixture(scope='module')
def views(grid):
    return [T.test_view(seed, HW, grid) for seed in range(4)]


def test_exact_pose_stays(grid, views):
    """From the exact pose the iteration has nowhere to go but the bias of the model: a surface interpolated from
    5 cm voxels.  Section H records that bias per pixel (p99 of |cast - analytic| 0.13 voxel = 6.5 mm); a pose
    averaged over thousands of pixels must stay inside it, and inside the angle it subtends at 2 m (0.19 degrees)."""
    for seed, (depth, k, pose, f, cond) in enumerate(views):
        res = T.align(depth, k, pose, pose, grid)
        dt, dr = T.pose_error(pose, res.pose)
        print('seed %d frame %d (condition %.0f): %d pairs, rmse %.6f m, pose error %.6f m %.5f deg'
              % (seed, f, cond, res.pairs, res.rmse, dt, dr))
        assert res.ok and res.iterations == 19 and res.pairs > 0.5 * HW[0] * HW[1]
        assert dt <= 0.13 * VS and dr <= math.degrees(0.13 * VS / 2.0)


def test_perturbed_guesses_converge(grid, views):
    worst = [0.0, 0.0]
    for seed, (depth, k, pose, f, cond) in enumerate(views):
        guess = T.perturbed(pose, seed, TRANS, ROT)
        g_dt, g_dr = T.pose_error(pose, guess)
        assert abs(g_dt - TRANS) < 1e-9 and abs(g_dr - ROT) < 1e-6
        res = T.align(depth, k, guess, guess, grid)
        dt, dr = T.pose_error(pose, res.pose)
        print('seed %d frame %d: pairs %s, rmse %.6f m, error %.6f m %.5f deg' % (seed, f, res.history, res.rmse, dt, dr))
        assert res.ok
        assert dt < TRANS and dr < ROT                                      # the condition of the issue
        worst = [max(worst[0], dt), max(worst[1], dr)]
    print('worst over the seeds: %.6f m %.5f deg' % tuple(worst))
    # the record the GPU test relies on is this run's result (5 %: the host's LAPACK and libm may differ in the last bits)
    assert abs(worst[0] - ALIGN_ERROR[0]) <= 0.05 * ALIGN_ERROR[0] and abs(worst[1] - ALIGN_ERROR[1]) <= 0.05 * ALIGN_ERROR[1]


def test_sequence_drift():
    depth, k, poses = T.sequence_frames(6, HW, T.SEQUENCE_SEED)
    dims, _, w2g = C.room_grid(VS, 4)
    assert dims == (88, 72, 60)
    first = R.Grid(dims, VS, w2g).integrate(depth[:1], k[:1], poses[:1])
    assert T.conditioning(depth[0], k[0], poses[0], first) < T.MAX_CONDITION
    grid = R.Grid(dims, VS, w2g)
    est, results = T.track_sequence(grid, depth, k, poses[0])
    assert all(r.ok for r in results) and np.array_equal(est[0], poses[0])
    for f in range(6):
        print('frame %d: %d pairs, rmse %.6f, error %.6f m %.5f deg' % ((f, results[f].pairs, results[f].rmse) +
                                                                        T.pose_error(poses[f], est[f])))
    dt, dr = T.pose_error(poses[5], est[5])
    step_t, step_r = T.pose_error(poses[0], poses[5])
    assert dt < step_t and dr < step_r                                      # tracking beats standing still
    assert abs(dt - SEQUENCE_DRIFT[0]) <= 0.05 * SEQUENCE_DRIFT[0] and abs(dr - SEQUENCE_DRIFT[1]) <= 0.05 * SEQUENCE_DRIFT[1]
    # the volume holds what integrating at the tracked poses gives
    again = R.Grid(dims, VS, w2g).integrate(depth, k, est)
    assert np.array_equal(again.sdf.view(np.int32), grid.sdf.view(np.int32))


def test_lost_frames_are_skipped(grid):
    depth, k, poses = T.sequence_frames(3, HW, T.SEQUENCE_SEED)
    depth[1] = -np.inf                                                      # nothing to track
    dims, _, w2g = C.room_grid(VS, 4)
    g = R.Grid(dims, VS, w2g)
    est, results = T.track_sequence(g, depth, k, poses[0])
    assert [r.ok for r in results] == [True, False, True]
    assert np.array_equal(est[1], est[0]) and results[1].pairs == 0
    two = R.Grid(dims, VS, w2g).integrate(depth[[0, 2]], k[[0, 2]], est[[0, 2]])
    assert np.array_equal(two.sdf.view(np.int32), g.sdf.view(np.int32))


def test_gauss_newton_model(grid, views):
    """r(xi) = r + J xi + O(|xi|^2): after a step xi of length 1e-3 along the Gauss-Newton direction the new E is the
    linear model's E + 2 g.xi + xi^T A xi up to second order.  |xi| = 1e-3 moves a point at 3 m by 3 mm against
    residuals of a few centimetres, so the second-order part is a few per cent of the first-order change; a wrong sign
    or a wrong Jacobian row misses by 100 % or more.  Asserted at 25 %."""
    depth, k, pose, _, _ = views[0]
    guess = T.perturbed(pose, 0, TRANS, ROT)
    md, mn = T.cast_grid(grid, k, pose, HW)
    T0 = T.pair_matrix(pose, guess)
    s0 = T.normal_equations(depth, k, md, mn, k, T0, max_dist=0.3)
    a, g, e0, n0 = T.unpack(s0)
    xi = T.step(s0)
    xi = xi * (1e-3 / np.linalg.norm(xi))
    predicted = e0 + 2 * g @ xi + xi @ a @ xi
    s1 = T.normal_equations(depth, k, md, mn, k, T.exp_se3(xi) @ T0, max_dist=0.3)
    e1, n1 = s1[27], int(s1[28])
    print('E %.6f -> %.6f, linear model %.6f; pairs %d -> %d' % (e0, e1, predicted, n0, n1))
    assert predicted < e0 and abs(n1 - n0) <= 0.01 * n0
    assert abs(e1 - predicted) <= 0.25 * (e0 - predicted)
    wrong = T.normal_equations(depth, k, md, mn, k, T.exp_se3(-xi) @ T0, max_dist=0.3)[27]
    assert wrong > e0                                                       # the other way is uphill


def test_halve_by_hand():
    inf = np.inf
    k = np.array([40.0, 44.0, 1.5, 1.5], F32)
    d = np.array([[1.00, 1.02, 2.00, -inf],
                  [1.04, 1.50, -inf, -inf],
                  [-inf, -inf, 3.00, 3.02],
                  [-inf, -inf, 3.04, 3.06]], F32)
    out, kh = T.halve(d, k, 0.05)
    assert out.shape == (2, 2) and out.dtype == F32
    assert out[0, 0] == ((F32(1.00) + F32(1.02)) + F32(1.04)) / F32(3)      # 1.50 is a step beyond delta: left out
    assert out[0, 1] == F32(2.00)                                           # one finite value
    assert out[1, 0] == -inf                                                # no finite value
    assert out[1, 1] == ((F32(3.00) + F32(3.02)) + F32(3.04)) / F32(3)      # 3.06 - 3.00 > 0.05 in fp32
    assert np.array_equal(kh, np.array([20.0, 22.0, 0.5, 0.5], F32))
    # (5, 3): the odd row and column are dropped
    d53 = np.arange(15, dtype=F32).reshape(5, 3) * F32(0.01) + F32(1)
    out53, _ = T.halve(d53, k, 0.05)
    assert out53.shape == (2, 1)
    assert out53[0, 0] == (((d53[0, 0] + d53[0, 1]) + d53[1, 0]) + d53[1, 1]) / F32(4)
    assert out53[1, 0] == (((d53[2, 0] + d53[2, 1]) + d53[3, 0]) + d53[3, 1]) / F32(4)
    assert T.halve(np.ones((1, 3), F32), k)[0].shape == (0, 1)
    # a pixel centre of the next level sits between four of this one: (cx - 0.5) / 2
    assert np.array_equal(T.halve(d, np.array([51.2, 51.2, 31.5, 23.5], F32))[1], np.array([25.6, 25.6, 15.5, 11.5], F32))


def test_depth_normals_by_hand():
    k = np.array([50.0, 50.0, 2.0, 1.0], F32)
    wall = np.full((4, 4), 2.0, F32)                                        # seen head-on
    n = T.depth_normals(wall, k, 0.05)
    assert np.isnan(n[0]).all() and np.isnan(n[-1]).all() and np.isnan(n[:, 0]).all() and np.isnan(n[:, -1]).all()
    assert np.array_equal(n[1:3, 1:3], np.broadcast_to(np.array([0, 0, -1], F32), (2, 2, 3)))   # faces the camera
    hole = wall.copy()
    hole[1, 2] = -np.inf
    n = T.depth_normals(hole, k, 0.05)
    assert np.isnan(n[1, 1]).all() and np.isnan(n[1, 2]).all() and np.isnan(n[2, 2]).all() and np.isfinite(n[2, 1]).all()
    step = np.full((5, 3), 2.0, F32)
    step[3:] = 2.2                                                          # a depth step larger than delta
    n = T.depth_normals(step, k, 0.05)
    assert np.isfinite(n[1, 1]).all() and np.isnan(n[2, 1]).all() and np.isnan(n[3, 1]).all()
    assert np.isfinite(T.depth_normals(step, k, 0.25)[2, 1]).all()
    # a plane z = 2 + 0.5 x: normal along (0.5, 0, -1), unit length, towards the camera
    i = np.arange(5, dtype=np.float64)
    x_over_z = (i - 2.0) / 50.0
    z = 2.0 / (1.0 - 0.5 * x_over_z)
    tilted = np.tile(z.astype(F32), (3, 1))
    n = T.depth_normals(tilted, k, 0.05)[1, 1:4].astype(np.float64)
    assert np.abs(n - np.array([0.5, 0.0, -1.0]) / math.sqrt(1.25)).max() < 1e-5
    assert np.isnan(T.depth_normals(np.ones((2, 2), F32), k)).all()


def test_rule_6_bound_for_any_order(grid, views):
    depth, k, pose, _, _ = views[1]
    md, mn = T.cast_grid(grid, k, pose, HW)
    J, r, residual, assoc = T.terms(depth, k, md, mn, k, T.pair_matrix(pose, T.perturbed(pose, 1)))
    table = T.term_table(J, r)
    n = table.shape[0]
    assert n > 1000 and (assoc >= 0).sum() == n and np.isfinite(residual).sum() == n
    exact = T.system_from_terms(table)[:28]
    bound = T.sum_bound(table)
    rng = np.random.default_rng(0)
    for _ in range(5):
        order = rng.permutation(n)
        naive = np.zeros(28)
        for row in table[order]:
            naive += row                                                    # fp64, left to right
        assert (np.abs(naive - exact) <= bound).all()
        pairwise = table[order].sum(0)                                      # numpy's blocked pairwise order
        assert (np.abs(pairwise - exact) <= bound).all()
    assert (bound > 0).all() and (bound < 1e-9 * np.abs(table).sum(0) + 1e-300).all()   # tight: 12 digits and more


def test_exp_against_the_series():
    rng = np.random.default_rng(3)
    for scale in (1.0, 1e-3, 1e-7, 1e-9, 0.0):
        for _ in range(5):
            xi = np.concatenate([rng.normal(size=3) * scale, rng.normal(size=3)])
            assert np.abs(T.exp_se3(xi) - T.exp_series(xi)).max() < 1e-14
    m = T.exp_se3([0.3, -0.2, 0.5, 1.0, 2.0, 3.0])
    assert np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(m[:3, :3]) - 1) < 1e-15


def test_empty_systems(grid, views):
    depth, k, pose, _, _ = views[0]
    md, mn = T.cast_grid(grid, k, pose, HW)
    bad = np.eye(4)
    bad[1, 2] = np.nan
    for d, m in ((np.full(HW, -np.inf, F32), np.eye(4)), (depth, bad)):
        J, r, residual, assoc = T.terms(d, k, md, mn, k, m)
        assert len(r) == 0 and np.isnan(residual).all() and (assoc == -1).all()
        assert not T.normal_equations(d, k, md, mn, k, m).any()
    assert not T.align(np.full(HW, -np.inf, F32), k, pose, pose, grid).ok
    res = T.align(depth, k, pose, bad, grid)
    assert not res.ok and res.pairs == 0 and res.iterations == 1
