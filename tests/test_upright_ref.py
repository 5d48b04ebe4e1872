"""The NumPy restatement of INTEGRATION.md section S (tests/upright_ref.py) on the tilted analytic room, and the host
functions of sgnn_amd.upright run on the restatement's integers.  No GPU.

The 0.25 degree bounds are a usefulness condition, not a measurement: over a 5 m room 0.25 degrees is 2 cm, under half
a voxel.  The restatement reaches 0.05 degrees on both ("Accuracy")."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import points_scenes as PS  # noqa: E402
import regrid_ref as RG  # noqa: E402
import upright_ref as U  # noqa: E402

from sgnn_amd import regrid, upright  # noqa: E402

F32 = np.float32
BAND, SURFACE = F32(3.0) * U.VS, U.VS
HALF_VOXEL = 0.5 * float(U.VS)


@pytest.fixture(scope='module')
def room():
    sdf, w2g, dims, up, walls = U.room_scene()
    assert dims == (63, 58, 45)
    return sdf, w2g, dims, up, walls


@pytest.fixture(scope='module')
def found(room):
    sdf, w2g, dims, up, walls = room
    return U.find(sdf, w2g, U.VS, U.room_hint())


@pytest.fixture(scope='module')
def solved(room):
    sdf, w2g, dims, up, walls = room
    return upright.solve(U.Passes(sdf, w2g, BAND, SURFACE), dims, w2g, U.VS, up_hint=U.room_hint())


# ---- the restatement alone ------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', [8, 16, 32])
def test_histogram_total_is_the_number_of_surface_voxels(room, bins):
    sdf, w2g = room[:2]
    n = len(U.surface_voxels(sdf, w2g, BAND, SURFACE)['v'])
    hist = U.histogram(sdf, w2g, BAND, SURFACE, bins)
    assert n > 10000 and hist.shape == (6, bins, bins) and hist.dtype == np.int32 and int(hist.sum()) == n


def test_peak_with_a_hint_20_degrees_off(room, found):
    up = room[3]
    assert abs(U.angle_deg(U.room_hint(), up) - 20.0) < 1e-9
    diagonal = math.degrees(2.0 * math.atan(math.sqrt(2.0) / 16))          # a cell's diagonal where it is widest
    print('peak %.3f degrees from the true up (cell diagonal %.2f)' % (U.angle_deg(found['peak'], up), diagonal))
    assert U.angle_deg(found['peak'], up) <= diagonal


def test_cone_means_and_wall_yaw_reach_a_quarter_degree(room, found):
    up, walls = room[3], room[4]
    print('cone means %s degrees; wall axis %.3f degrees, confidence %.3f; votes %s' % (
        ['%.3f' % U.angle_deg(u, up) for u in found['ups']], U.wall_error_deg(found['x'], walls), found['confidence'],
        found['votes']))
    assert found['ok'] and found['yaw_ok'] and found['confidence'] > 0.8
    assert U.angle_deg(found['up'], up) <= 0.25
    assert U.wall_error_deg(found['x'], walls) <= 0.25
    assert -math.pi / 4 < found['yaw'] <= math.pi / 4


def test_straightened_floor_lies_in_two_layers(room, solved):
    """The share the GPU test asks of upright.straighten, met by the restatement alone through tests/regrid_ref.py."""
    sdf, w2g, dims = room[:3]
    src = RG.from_state(dims, U.VS, w2g, sdf, np.isfinite(sdf).astype(np.int64), 0)
    T = upright.transform(solved, floor_at=0.0)
    new_dims, new_w2g = regrid.grid_for(src, world_transform=T, pad=2)
    level = RG.resample(src, new_dims, new_w2g)
    box = (new_w2g.astype(np.float64) @ np.linalg.inv(T)).astype(F32)       # the upright world -> the new grid
    share, n = U.floor_layer_share(level.sdf, box, U.VS)
    tilted, _ = U.floor_layer_share(sdf, w2g, U.VS, up=room[3])
    print('%.4f of %d up-facing floor voxels in two adjacent layers (%.4f before)' % (share, n, tilted))
    assert n > 1000 and share >= 0.95 and tilted < 0.5


# ---- the host functions of sgnn_amd.upright on the restatement's integers ---------------------------------
def test_solve_agrees_with_the_restatements_own_host_steps(found, solved):
    assert solved.ok and solved.yaw_ok and solved.votes == found['votes']
    assert np.allclose(solved.up, found['up'], rtol=0, atol=1e-12) and np.array_equal(solved.R[2], solved.up)
    assert np.allclose(solved.R[0], found['x'], rtol=0, atol=1e-12)
    assert abs(solved.yaw - found['yaw']) < 1e-12 and abs(solved.yaw_confidence - found['confidence']) < 1e-12
    assert abs(solved.floor - found['floor']) < 1e-12 and abs(solved.ceiling - found['ceiling']) < 1e-12


def test_floor_and_ceiling_levels(room, solved):
    """The room's floor is the plane through the world origin normal to the true up; the ceiling lies 1.2 m above."""
    print('floor %.4f m, ceiling %.4f m' % (solved.floor, solved.ceiling))
    assert abs(solved.floor) <= HALF_VOXEL
    assert abs(solved.ceiling - PS.ROOM_EXT[2]) <= HALF_VOXEL


def test_transform_is_rigid_and_puts_the_floor_where_asked(solved):
    for floor_at in (0.0, -1.25):
        T = upright.transform(solved, floor_at=floor_at)
        R = T[:3, :3]
        assert T.dtype == np.float64 and np.array_equal(T[3], [0, 0, 0, 1])
        assert np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.allclose(R @ solved.up, [0, 0, 1], rtol=0, atol=1e-14)
        on_floor = solved.floor * solved.up + 0.3 * solved.R[0] - 0.2 * solved.R[1]
        assert abs((T @ np.append(on_floor, 1.0))[2] - floor_at) < 1e-14
    assert np.array_equal(upright.transform(solved, floor_at=None)[:3, 3], np.zeros(3))


def test_peak_choice_and_ties():
    bins = 8
    hist = np.zeros((6, bins, bins), np.int32)
    centres = upright.bin_centres(bins)
    assert centres.shape == (6 * bins * bins, 3) and np.allclose(np.linalg.norm(centres, axis=1), 1.0)
    for i in (0, 77, 200, 383):
        assert np.allclose(centres[i], U.centre(i, bins), rtol=0, atol=1e-15) and U.bin_of(centres[i], bins) == i
    assert upright.peak(hist) is None and upright.peak(hist, up_hint=(0, 0, 1)) is None
    up_bin, down_bin, x_bin = U.bin_of((0.05, 0.05, 1), bins), U.bin_of((-0.05, -0.05, -1), bins), U.bin_of((1, 0.05, 0.05), bins)
    hist.ravel()[[up_bin, down_bin, x_bin]] = (40, 50, 70)
    assert upright.peak(hist) == up_bin == U.peak(hist)                     # 90 as a pair beats 70; the lower of the pair
    assert upright.peak(hist, up_hint=(0, 0, -1)) == down_bin == U.peak(hist, (0, 0, -1))
    assert upright.peak(hist, up_hint=(0, 0, 1)) == up_bin
    assert upright.peak(hist, up_hint=(0.9, 0, 0.1), max_tilt=30.0) == x_bin
    assert upright.peak(hist, up_hint=(0, 1, 0), max_tilt=30.0) is None     # no vote within the tilt
    hist.ravel()[x_bin] = 90
    assert upright.peak(hist) == min(x_bin, up_bin)                         # a tie of scores: the lowest index
    tie = np.zeros((6, bins, bins), np.int32)
    a, b = U.bin_of((0.05, 0.05, 1), bins), U.bin_of((0.3, 0.05, 1), bins)
    tie.ravel()[[a, b]] = 9
    assert upright.peak(tie, up_hint=(0, 0, 1)) == min(a, b) == U.peak(tie, (0, 0, 1))


def test_hint_from_poses():
    poses = np.stack([np.eye(4)] * 3)
    poses[0, :3, :3] = PS.rotation((1, 0, 0), 0.2)
    poses[1, :3, :3] = PS.rotation((0, 0, 1), -0.3)
    poses[2, :3, :3] = PS.rotation((1, 1, 0), 0.1)
    mean = -poses[:, :3, 1].mean(0)
    assert np.allclose(upright.hint_from_poses(poses), mean / np.linalg.norm(mean), rtol=0, atol=1e-15)
    assert np.allclose(upright.hint_from_poses(np.eye(4)), [0, -1, 0])
    flipped = np.stack([np.eye(4), np.diag([1.0, -1.0, -1.0, 1.0])])
    for bad in (flipped, np.eye(3), np.zeros((0, 4, 4))):
        with pytest.raises(ValueError):
            upright.hint_from_poses(bad)


def test_gates_on_an_empty_volume_and_on_a_single_plane(room):
    w2g, dims = room[1], room[2]
    empty = np.full(dims[::-1], -np.inf, F32)
    res = upright.solve(U.Passes(empty, w2g, BAND, SURFACE), dims, w2g, U.VS, up_hint=U.room_hint())
    assert not res.ok and not res.yaw_ok and np.array_equal(res.R, np.eye(3)) and res.votes == (0, 0, 0)
    assert res.yaw == 0.0 and res.floor is None and res.ceiling is None
    assert np.array_equal(upright.transform(res), np.eye(4))
    assert U.find(empty, w2g, U.VS, U.room_hint()) is None
    # one tilted plane, free space above it: the up axis is found, the yaw is not
    k, j, i = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims[::-1]), indexing='ij')
    g2w = np.linalg.inv(w2g.astype(np.float64))
    world = np.stack([i, j, k], -1) @ g2w[:3, :3].T + g2w[:3, 3]
    up = U.ROOM_TILT[:, 2]
    d = world @ up - 0.4
    t = 3.0 * float(U.VS)
    plane = np.where(d < -t, -np.inf, np.minimum(d, t)).astype(F32)
    res = upright.solve(U.Passes(plane, w2g, BAND, SURFACE), dims, w2g, U.VS, up_hint=U.room_hint())
    print('single plane: up %.4f degrees off, votes %s, floor %.4f' % (U.angle_deg(res.up, up), res.votes, res.floor))
    assert res.ok and not res.yaw_ok and res.yaw == 0.0 and res.votes[0] > 1000 and res.votes[1:] == (0, 0)
    assert U.angle_deg(res.up, up) <= 0.25 and abs(res.floor - 0.4) <= HALF_VOXEL and res.ceiling is None
    assert abs(np.linalg.det(res.R) - 1.0) < 1e-14 and np.array_equal(res.R[2], res.up)
    few = upright.solve(U.Passes(plane, w2g, BAND, SURFACE), dims, w2g, U.VS, up_hint=U.room_hint(), min_votes=10 ** 6)
    assert not few.ok and np.array_equal(few.R, np.eye(3)) and few.votes == res.votes


def test_host_argument_errors(room):
    sdf, w2g, dims = room[:3]
    passes = U.Passes(sdf, w2g, BAND, SURFACE)
    singular = w2g.copy()
    singular[2] = singular[1]
    for kw in (dict(bins=12), dict(up_hint=(0, 0, 0)), dict(up_hint=(1, 2)), dict(cones=()), dict(cones=(20.0, 95.0)),
               dict(wall_tol=-1.0), dict(min_votes=0), dict(floor_share=0.0), dict(max_tilt=0.0, up_hint=(0, 0, 1))):
        with pytest.raises(ValueError):
            upright.solve(passes, dims, w2g, U.VS, **kw)
    with pytest.raises(ValueError):
        upright.solve(passes, dims, singular, U.VS)
    with pytest.raises(ValueError):
        upright.peak(np.zeros((6, 12, 12), np.int32))
    with pytest.raises(ValueError):
        upright.axis_table(np.zeros((2, 3)), np.zeros((3, 3)), np.zeros((2, 3)), 0.9, 0.1)
