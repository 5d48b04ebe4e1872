"""GPU: TSDF ray casting (sgnn_amd.raycast, csrc/raycast.hip) against the NumPy restatement of tests/raycast_ref.py,
bit for bit, with and without empty-space skipping, and the loop from depth frames through fusion back to depth."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402

from sgnn_amd import fusion, raycast  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HW = (48, 64)
VS = 0.05
BAND = F32(3.0) * F32(VS)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == exp.shape
    g, e = bits(got), bits(exp)
    assert np.array_equal(g, e), '%d of %d values differ' % ((g != e).sum(), g.size)


def counted(*args, **kw):
    c = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = raycast.cast(*args, counters=c, **kw)
    return out, [int(v) for v in c.cpu()]


@pytest.fixture(scope='module')
def room():
    sdf, w2g = C.room_sdf(VS, 4, BAND)
    _, k, poses = R.room_frames(6, HW, seed=1)
    depth, normal = C.cast(sdf, w2g, VS, k, poses, HW, BAND, normals=True)
    return dict(sdf=sdf, w2g=w2g, k=k, poses=poses, depth=depth, normal=normal)


def test_room_bitwise(room):
    depth, normal = raycast.cast(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, BAND, normals=True)
    same(depth, room['depth'])
    same(normal, room['normal'])                                            # NaN positions included
    assert np.isnan(room['normal']).any() and np.isfinite(room['normal']).any()
    for f in range(5):
        assert np.isfinite(room['depth'][f]).mean() > 0.9
    same(raycast.cast(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, BAND), room['depth'])


def test_skipping_changes_no_bit(room):
    args = (room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, BAND)
    (d1, n1), (ev1, sk1) = counted(*args, normals=True, skip=True)
    (d0, n0), (ev0, sk0) = counted(*args, normals=True, skip=False)
    same(d1, room['depth'])
    same(d0, room['depth'])
    same(n1, room['normal'])
    same(n0, room['normal'])
    print('samples evaluated / skipped: with skipping %d / %d, without %d / %d' % (ev1, sk1, ev0, sk0))
    assert sk0 == 0 and 0 < ev1 < ev0 and ev1 + sk1 == ev0


@pytest.mark.parametrize('nf,hw', [(1, (48, 64)), (37, (37, 53)), (5, (1, 3))])
def test_frame_lists_and_odd_sizes(room, nf, hw):
    k = np.array([0.8 * hw[1], 0.8 * hw[1], (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0], F32)
    poses = R.room_trajectory(nf, seed=4)
    if nf > 10:
        poses[3, 1, 2] = np.nan                                          # non-finite pose: an empty frame
        poses[9, 0, 3] = np.inf
        poses[20] = R.look_at((-5.0, 1.0, 1.0), (-9.0, 1.0, 1.0))        # outside the volume, looking away
    kk = np.tile(k, (nf, 1))
    sdf, w2g = room['sdf'], room['w2g']
    exp, exp_n = C.cast(sdf, w2g, VS, kk, poses, hw, BAND, normals=True)
    if nf > 10:
        assert (exp[[3, 9, 20]] == -np.inf).all() and np.isfinite(exp[4]).any()
    for skip in (True, False):
        got, got_n = raycast.cast(sdf, w2g, VS, kk, poses, hw, BAND, normals=True, skip=skip)
        same(got, exp)
        same(got_n, exp_n)
    if nf > 10:
        for chunk in (1, 5, 37, None):
            same(raycast.cast(sdf, w2g, VS, kk, poses, hw, BAND, chunk=chunk), exp)
    # host arrays, host tensors and device tensors give the same frames
    t = torch.from_numpy
    same(raycast.cast(t(sdf.copy()), t(w2g), VS, t(kk), t(poses), hw, BAND), exp)
    same(raycast.cast(t(sdf.copy()).cuda(), t(w2g).cuda(), VS, t(kk).cuda(), t(poses).cuda(), hw, BAND), exp)


def slab(shape_zyx, plane, vs):
    """sdf (Z, Y, X) = (plane - z) * vs: a surface at grid height `plane`, seen from the front from below."""
    z = np.arange(shape_zyx[0], dtype=np.float64)[:, None, None]
    return np.broadcast_to((plane - z) * vs, shape_zyx).astype(F32)


def slab_views(shape_zyx, vs, front):
    """Three cameras 2.5 m from the slab's centre plane, below it (front) or above it (back), (12, 16) pixels."""
    dz, dy, dx = shape_zyx
    centre = np.array([(dx - 1) / 2.0, (dy - 1) / 2.0, (dz - 1) / 2.0]) * vs
    sign = -1.0 if front else 1.0
    eyes = [centre + (0.0, 0.0, sign * 2.5), centre + (0.3, -0.2, sign * 2.5), centre + (-0.4, 0.1, sign * 2.4)]
    poses = np.stack([R.look_at(e, centre + (0.01, 0.02, 0.0), up=(0.0, 1.0, 0.0)) for e in eyes])
    k = np.tile(np.array([12.8, 12.8, 7.5, 5.5], F32), (3, 1))
    return k, poses


@pytest.mark.parametrize('shape', [(2, 2, 2), (9, 8, 17)])
def test_small_volumes_and_the_back_face_rule(shape):
    vs = 0.5
    w2g = R.grid_transform((0.0, 0.0, 0.0), vs)
    sdf = slab(shape, (shape[0] - 1) // 2 + 0.5, vs)
    band = F32(1.01 * vs)                                                  # the two layers next to the surface only
    if shape[0] > 2:
        assert (np.abs(sdf) < band).any(axis=(1, 2)).sum() == 2
    for front in (True, False):
        k, poses = slab_views(shape, vs, front)
        exp, exp_n = C.cast(sdf, w2g, vs, k, poses, (12, 16), band, step=0.2, normals=True)
        assert np.isfinite(exp).any() if front else (exp == -np.inf).all()
        for skip in (True, False):
            got, got_n = raycast.cast(sdf, w2g, vs, k, poses, (12, 16), band, step=0.2, normals=True, skip=skip)
            same(got, exp)
            same(got_n, exp_n)
    # a band below every |v|: nothing is usable
    k, poses = slab_views(shape, vs, True)
    small = F32(0.4 * vs)
    assert (np.abs(sdf) >= small).all()
    for skip in (True, False):
        got, (ev, sk) = counted(sdf, w2g, vs, k, poses, (12, 16), small, step=0.2, skip=skip)
        assert (got == -float('inf')).all()
        assert ev == 0 if skip else sk == 0


def test_degenerate_volumes():
    vs = 0.5
    w2g = R.grid_transform((0.0, 0.0, 0.0), vs)
    band = F32(3.0 * vs)
    for shape in ((1, 8, 17), (9, 1, 17), (9, 8, 1)):                       # a dimension of 1: no cell at all
        sdf = np.zeros(shape, F32)
        k, poses = slab_views(shape, vs, True)
        for skip in (True, False):
            depth, normal = raycast.cast(sdf, w2g, vs, k, poses, (12, 16), band, normals=True, skip=skip)
            assert (depth == -float('inf')).all() and torch.isnan(normal).all()
    empty = np.full((9, 8, 17), -np.inf, F32)
    k, poses = slab_views(empty.shape, vs, True)
    got, (ev, sk) = counted(empty, w2g, vs, k, poses, (12, 16), band, skip=True)
    assert (got == -float('inf')).all() and ev == 0 and sk > 0
    got, (ev0, sk0) = counted(empty, w2g, vs, k, poses, (12, 16), band, skip=False)
    assert (got == -float('inf')).all() and ev0 == sk and sk0 == 0
    assert tuple(raycast.cast(empty, w2g, vs, k[:0], poses[:0], (12, 16), band).shape) == (0, 12, 16)


def test_from_fusion_and_back():
    """Depth frames -> TSDFVolume -> cast_volume at the same poses.  The cast equals the restatement run on the
    fused volume bit for bit, and the loop closes: the median |cast - input depth| over the pixels where both are
    finite is 0.000901 m (0.018 voxel; 0.0167 to 0.0184 voxel for trajectory seeds 0 to 3) when fusion_ref.Grid and
    the restatement do both halves on the CPU; asserted at 1.5 times that, 0.00135 m."""
    dims, _, w2g = C.room_grid(VS, 4)
    depth, k, poses = R.room_frames(24, HW)
    vol = fusion.TSDFVolume(dims, VS, w2g).integrate(depth, k, poses)
    got = raycast.cast_volume(vol, k, poses, HW)
    exp = C.cast(vol.sdf().cpu().numpy(), w2g, VS, k, poses, HW, F32(3.0) * F32(VS))
    same(got, exp)
    both = np.isfinite(exp) & np.isfinite(depth)
    assert both.sum() > 0.8 * depth.size
    median = float(np.median(np.abs(exp[both].astype(np.float64) - depth[both])))
    print('loop closure: %d pixels, median |cast - input| %.6f m' % (both.sum(), median))
    assert median <= 1.5 * 0.000901
    # a cast frame is a depth frame: fusion takes it back
    again = fusion.TSDFVolume(dims, VS, w2g).integrate(got, k, poses)
    assert torch.isfinite(again.sdf()).sum().item() > 0.5 * torch.isfinite(vol.sdf()).sum().item()


def test_sparse_route(room):
    sdf, w2g, k, poses = room['sdf'], room['w2g'], room['k'], room['poses']
    locs = np.stack(np.nonzero(np.isfinite(sdf)), 1)                        # z, y, x
    vals = sdf[locs[:, 0], locs[:, 1], locs[:, 2]]
    same(raycast.cast_sparse(locs, vals, sdf.shape, w2g, VS, k, poses, HW, BAND), room['depth'])
    voxels = raycast.cast_sparse(torch.from_numpy(locs).cuda(), torch.from_numpy(vals / F32(VS)).cuda(), sdf.shape, w2g,
                                 VS, k, poses, HW, 3.0)
    assert np.array_equal(np.isfinite(voxels.cpu().numpy()), np.isfinite(room['depth']))


def test_argument_errors(room):
    sdf, w2g, k, poses = room['sdf'], room['w2g'], room['k'], room['poses']
    launches = raycast._lib.load().sgnn_launch_count
    before = launches()
    bad = [
        dict(sdf=sdf[0]), dict(sdf=sdf[None]), dict(band=0.0), dict(band=-1.0), dict(step=0.0), dict(step=-0.5),
        dict(voxel_size=0.0), dict(voxel_size=-VS), dict(depth_min=2.0, depth_max=1.0), dict(k=k[:5]),
        dict(poses=poses[:2]), dict(k=np.tile(k[:1], (2, 1)), poses=poses[:2], hw=(1 << 15, 1 << 15)),
        dict(step=1e-6), dict(depth_min=0.0, depth_max=1e6, step=0.01),
    ]
    for change in bad:
        a = dict(sdf=sdf, w2g=w2g, voxel_size=VS, k=k, poses=poses, hw=HW, band=BAND, step=0.5, depth_min=0.4,
                 depth_max=4.0)
        a.update(change)
        with pytest.raises(ValueError):
            raycast.cast(a['sdf'], a['w2g'], a['voxel_size'], a['k'], a['poses'], a['hw'], a['band'], step=a['step'],
                         depth_min=a['depth_min'], depth_max=a['depth_max'])
    assert launches() == before                                             # raised before any launch
    same(raycast.cast(sdf, w2g, VS, k, poses, HW, BAND), room['depth'])
    assert launches() > before
