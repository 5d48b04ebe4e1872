"""tests/points_ref.py, the NumPy restatement of INTEGRATION.md section P, against itself and against the frame
route's restatement (tests/fusion_ref.py).  No GPU."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_ref as FR  # noqa: E402
import points_ref as PR  # noqa: E402
import points_scenes as PS  # noqa: E402
import render_ref as RR  # noqa: E402

F32 = np.float32

# the cross-route limits of tests/test_gpu_points.py: the figures measured below on the CPU, plus half again
#   5 327 voxels compared; 26 of them (0.488 %) differ in sign; max |sdf_A - sdf_B| / vs = 1.898, at a voxel on the
#   ceiling's edge that the frames saw 9 times and the rays 33 times.  Both values lie within one voxel of zero by
#   selection, so no difference can reach 2: the second limit cannot bind on this scene, the first one does the work.
SIGN_SHARE_MEASURED, DIFF_MEASURED = 0.0048808, 1.8983825
SIGN_SHARE_LIMIT = 1.5 * SIGN_SHARE_MEASURED
DIFF_LIMIT = max(1.5 * DIFF_MEASURED, DIFF_MEASURED + 1.0 / PR.FIXED)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def state(v):
    return [bits(v.sdf), v.weight.copy(), v.free.copy()] + ([] if v.color is None else [v.color.copy()])


def common_volume(color=True, obb=None):
    return PR.Volume(PS.DIMS, PS.VS, PS.world2grid(), PS.DMIN, PS.DMAX, obb=obb, color=color)


def test_permuting_the_points_changes_no_bit():
    pts, org, oid, rgba = PS.cloud()
    perm = np.random.default_rng(5).permutation(len(pts))
    for carve in (True, False):
        a = PR.integrate(common_volume(), pts, org, oid, rgba, carve)
        b = PR.integrate(common_volume(), pts[perm], org, oid[perm], rgba[perm], carve)
        assert (a.weight > 0).sum() > 300 and (a.color[..., 3] > 0).sum() > 100
        assert all(np.array_equal(x, y) for x, y in zip(state(a), state(b)))
    assert (a.free > 0).sum() < (PR.integrate(common_volume(), pts, org, oid, rgba, True).free > 0).sum()


def axis_ray():
    vs = F32(0.05)
    w2g = FR.grid_transform((0.0, 0.0, 0.0), float(vs))
    origin = np.array([[2, 5, 5]], np.float64) * float(vs)
    point = np.array([[10, 5, 5]], np.float64) * float(vs)
    return vs, w2g, origin.astype(F32), point.astype(F32)


def test_one_ray_along_a_grid_axis_updates_the_voxels_one_can_list_by_hand():
    """d = 8 voxels = 0.4 m, trunc = 3 vs + d vs = 3.4 voxels, so without carving the samples start 4.6 voxels from the
    origin and come every half voxel up to 11.4: positions x = 6.6, 7.1, .., 13.1, which round to the voxels 7 .. 13,
    every one of them twice (the second sample is the duplicate that rule 6 drops).  Voxel x has sdf (10 - x) vs, all
    inside the band; wu = 4.5 at d = 0.4, so the weight is 4; voxels 7, 8, 9 lie in front of the point."""
    vs, w2g, origin, point = axis_ray()
    v = PR.integrate(PR.Volume((16, 10, 10), vs, w2g), point, origin, carve=False)
    z, y, x = np.nonzero(v.weight)
    assert x.tolist() == list(range(7, 14)) and set(y) == {5} and set(z) == {5}
    assert (v.weight[5, 5, 7:14] == 4).all()
    assert np.abs(v.sdf[5, 5, 7:14] / vs - (10 - np.arange(7, 14))).max() <= 1.0 / PR.FIXED
    assert v.free[5, 5].tolist() == [0] * 7 + [1, 1, 1] + [0] * 6 and v.free.sum() == 3
    assert np.isneginf(v.sdf).sum() == v.sdf.size - 7
    # with carving the walk starts at depth_min = 0.4 m = 8 voxels from the origin: voxel 10 on
    c = PR.integrate(PR.Volume((16, 10, 10), vs, w2g), point, origin, carve=True)
    assert np.nonzero(c.weight)[2].tolist() == list(range(10, 14)) and c.free[5, 5, 11:].sum() == 0
    # and from a closer depth_min it carves every voxel from there to the point
    c = PR.integrate(PR.Volume((16, 10, 10), vs, w2g, dmin=0.1), point, origin, carve=True)
    assert np.nonzero(c.weight)[2].tolist() == list(range(4, 14)) and c.free[5, 5, 4:10].tolist() == [1] * 6
    assert bits(c.sdf[5, 5, 4]) == bits(c.sdf[5, 5, 5]) and abs(c.sdf[5, 5, 4] / vs - 3.4) <= 1.0 / PR.FIXED   # +trunc


def test_300_identical_rays_saturate_the_weight_and_keep_the_value():
    vs, w2g, origin, point = axis_ray()
    one = PR.integrate(PR.Volume((16, 10, 10), vs, w2g), point, origin, carve=False)
    many = PR.integrate(PR.Volume((16, 10, 10), vs, w2g), np.repeat(point, 300, 0), origin, carve=False)
    assert (many.weight[5, 5, 7:14] == 255).all() and (many.free[5, 5, 7:10] == 300).all()
    assert np.array_equal(bits(many.sdf), bits(one.sdf))
    # a second call is a second observation: the running mean of two equal values, weight 4 + 4
    PR.integrate(one, point, origin, carve=False)
    assert (one.weight[5, 5, 7:14] == 8).all() and np.abs(one.sdf[5, 5, 7:14] - many.sdf[5, 5, 7:14]).max() < 1e-7


def test_ignored_rays_and_an_empty_call_change_nothing():
    pts, org, oid, rgba = PS.cloud()
    extra, extra_id = PS.ignored_rays()
    a = PR.integrate(common_volume(color=False), pts, org, oid)
    b = PR.integrate(common_volume(color=False), np.concatenate([extra, pts]), org, np.concatenate([extra_id, oid]))
    assert all(np.array_equal(x, y) for x, y in zip(state(a), state(b)))
    assert PR.rays(common_volume(), extra, org, extra_id, True)['n'][:6].tolist() == [0] * 6
    before = state(a)
    PR.integrate(a, np.zeros((0, 3), F32), org[:1])
    PR.integrate(a, extra, org, extra_id)
    assert all(np.array_equal(x, y) for x, y in zip(before, state(a)))


@functools.lru_cache(maxsize=None)
def cross_route():
    """Both routes on the room of points_scenes, on the CPU: the frames are render_ref's (bit for bit the device
    renderer's), route A is fusion_ref, route B sgnn_amd.points.from_depth (torch on the host) and points_ref."""
    from sgnn_amd import points
    room = PS.room()
    depth = RR.render_ref(room['verts'], room['faces'], room['k'], room['poses'], PS.ROOM_HW)
    a = FR.Grid(room['dims'], PS.VS, room['w2g']).integrate(depth, room['k'], room['poses'])
    pts, org, oid = (t.numpy() for t in points.from_depth(depth, room['k'], room['poses']))
    want = PR.from_depth(depth, room['k'], room['poses'])
    assert np.allclose(pts, want[0], rtol=0, atol=1e-5, equal_nan=True) and np.array_equal(oid, want[2])
    assert np.array_equal(org, want[1]) and np.isfinite(depth).mean() > 0.9
    b = PR.integrate(PR.Volume(room['dims'], PS.VS, room['w2g']), pts, org, oid, carve=True)
    return a, b


def test_the_point_route_agrees_with_the_frame_route_on_the_room():
    """Measured here (CPU, fusion_ref against points_ref, 6 frames of 60 x 80): see SIGN_SHARE_MEASURED and
    DIFF_MEASURED at the top of this file; the limits are those figures plus half again, at least one fixed-point
    step."""
    a, b = cross_route()
    share, diff, n = PS.cross_route_figures(a.sdf, a.weight, b.sdf, b.weight, PS.VS)
    print('cross-route on the CPU: %d voxels, sign disagreements %.5f, max |sdf_A - sdf_B| / vs %.5f' % (n, share, diff))
    assert n > 2000
    assert share <= SIGN_SHARE_LIMIT and diff <= DIFF_LIMIT
    # the point route carves what the frame route sees as free: most voxels the frames call free are free for the rays
    free_a = (a.free > 0) & (a.sdf > PS.VS)
    assert (b.free[free_a] > 0).mean() > 0.9
