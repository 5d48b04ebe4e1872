"""sgnn_amd.points on the device against tests/points_ref.py, bit for bit, and against the frame route (INTEGRATION.md
section P).  The scenes are tests/points_scenes.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_ref as FR  # noqa: E402
import points_ref as PR  # noqa: E402
import points_scenes as PS  # noqa: E402
from test_points_ref import DIFF_LIMIT, SIGN_SHARE_LIMIT  # noqa: E402

from sgnn_amd import data, fusion, marching_cubes as mc, meshdist, points, render  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

# mean distance of the extracted surface to the room mesh, route B over route A, measured on an MI355X (section P)
#   frames 0.009559 m, points 0.002301 m, ratio 0.2407: the rays' range distances average to a surface closer to the mesh
#   than the frames' projective z distances do on this scene
SURFACE_RATIO_MEASURED = 0.2407
SURFACE_MARGIN = 1.25


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def device_state(v):
    out = [bits(v.sdf().cpu().numpy()), v.weight().cpu().numpy().astype(np.int64),
           v.free_count().cpu().numpy().astype(np.int64)]
    if v.color_state() is not None:
        out.append(v.color_state().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64))
    return out


def ref_state(v):
    return [bits(v.sdf), v.weight, v.free] + ([] if getattr(v, 'color', None) is None else [v.color])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def volumes(color=False, obb=None):
    dev = fusion.TSDFVolume(PS.DIMS, PS.VS, PS.world2grid(), PS.DMIN, PS.DMAX, obb=obb, color=color)
    return dev, PR.Volume(PS.DIMS, PS.VS, PS.world2grid(), PS.DMIN, PS.DMAX, obb=obb, color=color)


@functools.lru_cache(maxsize=None)
def reference(carve, obb, color):
    """The host restatement of one variant of the common cloud, computed once."""
    pts, org, oid, rgba = PS.cloud()
    return PR.integrate(volumes(color, PS.OBB if obb else None)[1], pts, org, oid, rgba if color else None, carve)


@pytest.mark.parametrize('color', [False, True])
@pytest.mark.parametrize('obb', [False, True])
@pytest.mark.parametrize('carve', [True, False])
def test_bit_exact_against_the_restatement(carve, obb, color):
    pts, org, oid, rgba = PS.cloud()
    assert (rgba[:, 3] == 0).sum() > 100
    dev, _ = volumes(color, PS.OBB if obb else None)
    assert points.integrate(dev, pts, org, oid, color=rgba if color else None, carve=carve) is dev
    want = reference(carve, obb, color)
    assert (want.weight > 0).sum() > 200 and (not color or (want.color[..., 3] > 0).sum() > 100)
    assert same(device_state(dev), ref_state(want))
    if obb and not color:
        assert (want.weight > 0).sum() < (reference(carve, False, False).weight > 0).sum()


def test_a_three_channel_colour_is_a_colour_everywhere():
    pts, org, oid, rgba = PS.cloud()
    dev, ref = volumes(True)
    points.integrate(dev, torch.from_numpy(pts).cuda(), torch.from_numpy(org), torch.from_numpy(oid).cuda(),
                     color=torch.from_numpy(rgba[:, :3].copy()).cuda(), carve=False)
    assert same(device_state(dev), ref_state(PR.integrate(ref, pts, org, oid, rgba[:, :3], False)))


@pytest.mark.parametrize('carve', [True, False])
def test_ignored_rays_leave_the_bits_alone(carve):
    pts, org, oid, _ = PS.cloud()
    extra, extra_id = PS.ignored_rays()
    where = np.random.default_rng(3).permutation(len(pts) + len(extra))
    allp, alli = np.concatenate([extra, pts])[where], np.concatenate([extra_id, oid])[where]
    dev, _ = volumes()
    points.integrate(dev, allp, org, alli, carve=carve)
    assert same(device_state(dev), ref_state(reference(carve, False, False)))
    # a call of ignored rays only, and an empty call, change nothing
    before = device_state(dev)
    points.integrate(dev, extra, org, extra_id, carve=carve)
    points.integrate(dev, np.zeros((0, 3), F32), org[:1], carve=carve)
    assert same(device_state(dev), before)
    with pytest.raises(ValueError):
        points.integrate(dev, torch.from_numpy(pts).cuda(), org, torch.full((len(pts),), 2, dtype=torch.int32).cuda())
    assert same(device_state(dev), before)


def test_order_chunk_and_rerun_independence():
    pts, org, oid, rgba = PS.cloud()
    perm = np.random.default_rng(11).permutation(len(pts))
    want = ref_state(reference(True, False, True))
    for p, i, c, chunk in ((pts, oid, rgba, None), (pts, oid, rgba, None), (pts, oid, rgba, 7),
                           (pts[perm], oid[perm], rgba[perm], None), (pts[perm], oid[perm], rgba[perm], 100)):
        dev, _ = volumes(True)
        points.integrate(dev, p, org, i, color=c, carve=True, chunk=chunk)
        assert same(device_state(dev), want)


def test_contention_4096_rays_into_a_patch_of_27_voxels():
    """Every ray ends in the 3 x 3 x 3 voxels around (12, 10, 8): the sums of those voxels collect thousands of atomic
    adds each, and the folded state shows S / W (the sdf), W (the weight, saturated) and the free count."""
    rng = np.random.default_rng(2)
    pts = PS.to_world(np.array([12.0, 10.0, 8.0]) + rng.uniform(-1.4, 1.4, (4096, 3)))
    org = PS.to_world(PS.ORIGINS_GRID[:1])
    for carve in (True, False):
        dev, ref = volumes()
        points.integrate(dev, pts, org, carve=carve)
        PR.integrate(ref, pts, org, carve=carve)
        assert same(device_state(dev), ref_state(ref))
        patch = ref.weight[7:10, 9:12, 11:14]
        assert (patch == 255).all() and ref.free.max() > (2000 if carve else 1000)


def test_frames_then_points_then_points_is_one_running_mean():
    import render_ref as RR
    room = PS.room()
    k = np.tile(np.array([28.0, 28.0, 19.5, 14.5], F32), (3, 1))
    poses, dims, w2g = room['poses'][:3], room['dims'], room['w2g']
    depth = RR.render_ref(room['verts'], room['faces'], k, poses, (30, 40))
    dev = fusion.TSDFVolume(dims, PS.VS, w2g)
    ref = FR.Grid(dims, PS.VS, w2g)
    dev.integrate(depth, k, poses)
    ref.integrate(depth, k, poses)
    assert same(device_state(dev), ref_state(ref)) and (ref.weight > 0).sum() > 1000
    pts, org, oid = (t.numpy() for t in points.from_depth(depth[:2], k[:2], poses[:2]))
    for sel, carve in ((slice(0, None, 2), True), (slice(1, None, 2), False)):
        points.integrate(dev, pts[sel], org, oid[sel], carve=carve)
        PR.integrate(ref, pts[sel], org, oid[sel], carve=carve)
        assert same(device_state(dev), ref_state(ref))
    assert ref.weight.max() > 30
    # and frames again, on top of the points
    dev.integrate(depth[2:], k[2:], poses[2:])
    ref.integrate(depth[2:], k[2:], poses[2:])
    assert same(device_state(dev), ref_state(ref))


def test_every_pyramid_level_is_a_volume_fused_on_its_own():
    pts, org, oid, rgba = PS.cloud()
    kw = dict(depth_min=PS.DMIN, depth_max=PS.DMAX, color=True)
    pyr = fusion.TSDFPyramid(PS.DIMS, PS.VS, PS.world2grid(), levels=3, obb=PS.OBB, **kw)
    assert points.integrate(pyr, pts, org, oid, color=rgba) is pyr
    for k, level in enumerate(pyr.volumes):
        w2g = (fusion.level_transform(k) @ PS.world2grid().astype(np.float64)).astype(F32)
        alone = fusion.TSDFVolume(level.dims_xyz, F32(2 ** k) * PS.VS, w2g, obb=level.obb, **kw)
        assert np.array_equal(alone.world2grid, level.world2grid) and alone.voxel_size == level.voxel_size
        points.integrate(alone, pts, org, oid, color=rgba)
        assert same(device_state(alone), device_state(level)) and int((level.weight() > 0).sum()) > 20
    ref = PR.Volume(pyr[1].dims_xyz, pyr[1].voxel_size, pyr[1].world2grid, PS.DMIN, PS.DMAX, obb=pyr[1].obb, color=True)
    assert same(device_state(pyr[1]), ref_state(PR.integrate(ref, pts, org, oid, rgba)))


def test_the_volume_is_handed_on_like_any_other(tmp_path):
    pts, org, oid, _ = PS.cloud()
    dev, _ = volumes()
    points.integrate(dev, pts, org, oid, carve=True)
    known = dev.known().cpu().numpy()
    assert (known == 0).any() and (known == 1).any() and (known >= 2).any()
    assert (known[reference(True, False, False).sdf > PS.VS] == 0).all()
    locs, vals = dev.sparse()
    path = dev.save(str(tmp_path / 'cloud.sdf'))
    (zyx, feats), dims_zyx, w = data.load_scene(path)
    assert list(dims_zyx) == list(PS.DIMS[::-1]) and np.array_equal(np.asarray(w, F32).reshape(4, 4), PS.world2grid())
    assert np.array_equal(np.asarray(zyx)[:, ::-1], locs.cpu().numpy()) and locs.shape[0] > 500
    assert np.array_equal(bits(feats), bits(vals.cpu().numpy() / PS.VS))
    assert np.array_equal(data.load_scene_known(os.path.splitext(path)[0] + '.knw').reshape(known.shape), known)
    assert fusion.scan_sample(dev)['input'][0].shape[0] > 200


@functools.lru_cache(maxsize=None)
def routes():
    """The room through both entrances on the device: (volume A from frames, volume B from the frames' rays)."""
    room = PS.room()
    depth = render.render_depth(room['verts'], room['faces'], room['k'], room['poses'], PS.ROOM_HW)
    a = fusion.TSDFVolume(room['dims'], PS.VS, room['w2g']).integrate(depth, room['k'], room['poses'])
    pts, org, oid = points.from_depth(depth, room['k'], room['poses'])
    b = points.integrate(fusion.TSDFVolume(room['dims'], PS.VS, room['w2g']), pts, org, oid, carve=True)
    return a, b


def test_cross_route_the_room_from_frames_and_from_their_rays():
    """Limits from tests/test_points_ref.py, where both routes run on the CPU (fusion_ref, points_ref) on this scene:
    measured there 0.488 % sign disagreements among 5 327 voxels and max |sdf_A - sdf_B| / vs = 1.898; the limits are
    those figures plus half again (0.732 %, 2.848)."""
    a, b = routes()
    share, diff, n = PS.cross_route_figures(a.sdf().cpu().numpy(), a.weight().cpu().numpy(), b.sdf().cpu().numpy(),
                                            b.weight().cpu().numpy(), PS.VS)
    print('cross-route on the device: %d voxels, sign disagreements %.5f, max |sdf_A - sdf_B| / vs %.5f' % (n, share, diff))
    assert n > 2000 and share <= SIGN_SHARE_LIMIT and diff <= DIFF_LIMIT


def surface_accuracy(vol):
    room = PS.room()
    v, _, f = mc.run_marching_cubes(vol.sdf(), None, 0.0, 3.0 * float(PS.VS), 10.0)
    g2w = torch.from_numpy(np.linalg.inv(room['w2g'].astype(np.float64)).astype(F32)).to(v.device)
    world = v @ g2w[:3, :3].T + g2w[:3, 3]
    assert f.shape[0] > 1000
    return meshdist.compare((world, f), (room['verts'], room['faces']), n=20000, max_dist=0.5)['accuracy']


def test_the_surface_of_the_point_route_is_as_good_as_the_frame_route():
    """Marching cubes of both volumes, mean distance of the extracted surface to the room mesh (meshdist accuracy).
    The bound is SURFACE_MARGIN over the ratio measured on an MI355X (0.2407: frames 0.009559 m, points 0.002301 m),
    which absorbs the corner-clipping rule of the half-voxel walk."""
    a, b = routes()
    acc_a, acc_b = surface_accuracy(a), surface_accuracy(b)
    print('surface accuracy: frames %.6f m, points %.6f m, ratio %.4f' % (acc_a, acc_b, acc_b / acc_a))
    assert acc_a < float(PS.VS)
    assert acc_b <= acc_a * SURFACE_MARGIN * SURFACE_RATIO_MEASURED
