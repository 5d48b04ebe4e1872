"""GPU: colour in TSDF fusion (sgnn_amd.fusion, csrc/fusion.hip) against the NumPy
restatement of tests/fusion_color_ref.py, as integers: pack_color, the colour state of k_fuse_integrate<true> on the
two scenes of tests/test_gpu_fusion.py, the export rule, chunking, and the coloured volume through marching cubes."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_color_ref as C  # noqa: E402
from test_gpu_fusion import CASES, scene  # noqa: E402

from sgnn_amd import fusion, marching_cubes as mc  # noqa: E402

pytestmark = pytest.mark.gpu
UNIFORM = (10, 200, 77)


@pytest.fixture(scope='module')
def fused():
    out = {}
    for case in CASES:
        dims, vs, w2g, obb, depth, k, poses = scene(case)
        filt = fusion.bilateral(torch.from_numpy(depth).cuda())
        rgba = C.noise_frames(depth.shape, 11)
        ref = C.ColorGrid(dims, vs, w2g, obb=obb).integrate(filt.cpu().numpy(), k, poses, rgba)
        vol = fusion.TSDFVolume(dims, vs, w2g, obb=obb, color=True)
        vol.integrate(filt, k, poses, chunk=len(poses), color=fusion.pack_color(rgba))
        out[case] = dict(dims=dims, vs=vs, w2g=w2g, obb=obb, filt=filt, k=k, poses=poses, rgba=rgba, ref=ref, vol=vol)
    return out


def same_color(vol, ref):
    got = vol.color_state()
    assert got.dtype == torch.uint16 and tuple(got.shape) == ref.sdf.shape + (4,)
    assert np.array_equal(got.cpu().numpy(), ref.state())


def same_geometry(vol, other):
    assert torch.equal(vol.sdf().view(torch.int32), other.sdf().view(torch.int32))
    assert torch.equal(vol.weight(), other.weight()) and torch.equal(vol.free_count(), other.free_count())


def mesh_colors(sdf, colors, vs):
    """(vertices in voxels, vertex colours) of the coloured volume, as numpy."""
    v, c, _ = mc.run_marching_cubes(sdf, colors, *C.mc_args(vs))
    return v.cpu().numpy(), c.cpu().numpy()


def test_pack_color_bitwise():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, size=(3, 97, 131, 3), dtype=np.uint8)
    got = fusion.pack_color(rgb, (61, 83))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 61, 83, 4)
    assert np.array_equal(got.cpu().numpy(), C.pack(rgb, (61, 83)))
    rgba = rng.integers(0, 256, size=(2, 48, 64, 4), dtype=np.uint8)
    rgba[..., 3] = np.where(rng.random(rgba.shape[:3]) < 0.3, 0, 255)
    for src in (rgba, torch.from_numpy(rgba), torch.from_numpy(rgba).cuda()):       # numpy, host and device tensors
        same = fusion.pack_color(src, (48, 64))
        assert np.array_equal(same.cpu().numpy(), rgba) and np.array_equal(C.pack(rgba, (48, 64)), rgba)
    rgba[..., 3] = rng.integers(0, 3, size=rgba.shape[:3])                          # any a != 0 becomes 255
    assert np.array_equal(fusion.pack_color(rgba).cpu().numpy(), C.pack(rgba))
    assert np.array_equal(fusion.pack_color(rgba, (31, 77)).cpu().numpy(), C.pack(rgba, (31, 77)))
    one = fusion.pack_color(rgb[0], (61, 83))
    assert tuple(one.shape) == (1, 61, 83, 4) and np.array_equal(one.cpu().numpy(), C.pack(rgb[0], (61, 83)))
    with pytest.raises(ValueError):
        fusion.pack_color(np.zeros((4, 4, 2), np.uint8))


@pytest.mark.parametrize('case', CASES)
def test_colour_integration_bitwise(fused, case):
    c = fused[case]
    ref, vol = c['ref'], c['vol']
    same_color(vol, ref)
    assert np.array_equal(vol.colors().cpu().numpy(), ref.colors())
    assert np.array_equal(vol.color_weight().cpu().numpy().astype(np.int64), ref.wc)
    assert vol.colors().dtype == torch.uint8 and tuple(vol.colors().shape) == ref.sdf.shape + (3,)
    plain = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb']).integrate(c['filt'], c['k'], c['poses'])
    same_geometry(vol, plain)
    assert np.array_equal(vol.sdf().cpu().numpy().view(np.int32), ref.sdf.view(np.int32))
    fin = np.isfinite(ref.sdf)
    assert (fin & (ref.wc > 0)).sum() > 1000 and (fin & (ref.wc == 0)).sum() > 100
    if case == 'odd37x53x29':
        assert ref.wc.max() == 255
    assert plain.color_state() is None


@pytest.mark.parametrize('case', CASES)
def test_chunking_and_split_calls_are_bit_identical(fused, case):
    c = fused[case]
    col = fusion.pack_color(c['rgba'])
    for chunk in (1, 7, len(c['poses']), None):
        vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'], color=True)
        vol.integrate(c['filt'], c['k'], c['poses'], chunk=chunk, color=col)
        same_color(vol, c['ref'])
        same_geometry(vol, c['vol'])
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'], color=True)
    vol.integrate(c['filt'][:9], c['k'][:9], c['poses'][:9], color=c['rgba'][:9])    # raw frames are packed on the way in
    vol.integrate(c['filt'][9:], c['k'][9:], c['poses'][9:], color=col[9:])
    same_color(vol, c['ref'])
    same_geometry(vol, c['vol'])
    # a call without colour in between changes the geometry only
    a, b = 9, 15
    ref = C.ColorGrid(c['dims'], c['vs'], c['w2g'], obb=c['obb'])
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'], color=True)
    filt = c['filt'].cpu().numpy()
    for lo, hi, with_color in ((0, a, True), (a, b, False), (b, len(c['poses']), True)):
        ref.integrate(filt[lo:hi], c['k'][lo:hi], c['poses'][lo:hi], c['rgba'][lo:hi] if with_color else None)
        before = vol.color_state().view(torch.int16).clone()
        vol.integrate(c['filt'][lo:hi], c['k'][lo:hi], c['poses'][lo:hi], color=col[lo:hi] if with_color else None)
        assert with_color or torch.equal(vol.color_state().view(torch.int16), before)
    same_color(vol, ref)
    same_geometry(vol, c['vol'])
    assert not np.array_equal(ref.state(), c['ref'].state())


@pytest.mark.parametrize('case', CASES)
def test_uniform_frames_and_the_mesh(fused, case):
    c = fused[case]
    rgba = C.uniform_frames(c['rgba'].shape[:3], UNIFORM, 12)
    ref = C.ColorGrid(c['dims'], c['vs'], c['w2g'], obb=c['obb']).integrate(c['filt'].cpu().numpy(), c['k'], c['poses'],
                                                                           rgba)
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'], color=True)
    vol.integrate(c['filt'], c['k'], c['poses'], color=rgba)
    same_color(vol, ref)
    wc, cols = vol.color_weight().cpu().numpy(), vol.colors().cpu().numpy()
    assert (wc > 0).sum() > 1000 and (cols[wc > 0] == np.array(UNIFORM)).all() and not cols[wc == 0].any()
    _, vc = mesh_colors(vol.sdf(), vol.colors(), c['vs'])
    black = (vc == 0).all(1)
    assert len(vc) > 400 and (vc[~black] == np.array(UNIFORM)).all()
    # the cap is the reference's own share, from ColorGrid through the same mesher
    _, rc = mesh_colors(torch.from_numpy(ref.sdf).cuda(), torch.from_numpy(ref.colors()).cuda(), c['vs'])
    print('%s: %d vertices, black share %.4f, reference %.4f' % (case, len(vc), black.mean(), C.black_share(rc)))
    assert C.black_share(vc) <= C.black_share(rc) <= C.BLACK_SHARE_CAP


def test_painted_room(fused):
    c = fused['cube48']
    _, rgba = C.painted_frames(c['k'], c['poses'], tuple(c['filt'].shape[1:]))
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], color=True).integrate(c['filt'], c['k'], c['poses'], color=rgba)
    v, vc = mesh_colors(vol.sdf(), vol.colors(), c['vs'])
    own, keep = C.painted_expectation(v, c['w2g'], C.painted_margin(c['vs'], c['k'][0][0]))
    print('painted room: %d vertices, kept share %.4f, wrong among kept %d' % (
        len(v), keep.mean(), (vc[keep] != own[keep]).any(1).sum()))
    # this grid has the room's other walls on its border, where no cell has all its neighbours: the mesh is mostly
    # the wall y = 3.2 m, with the mixed colours of its corners and of the boxes among the vertices left out
    assert len(v) > 400 and len(np.unique(vc, axis=0)) >= 2 and len(np.unique(rgba[..., :3].reshape(-1, 3), axis=0)) >= 8
    assert keep.mean() >= C.KEPT_SHARE_MIN
    assert (vc[keep] == own[keep]).all()
    # the whole colour state is the restatement's
    ref = C.ColorGrid(c['dims'], c['vs'], c['w2g']).integrate(c['filt'].cpu().numpy(), c['k'], c['poses'], rgba)
    same_color(vol, ref)


def test_copy_pyramid_padding_and_errors(fused):
    c = fused['cube48']
    col = fusion.pack_color(c['rgba'])
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], color=True)
    vol.integrate(c['filt'][:10], c['k'][:10], c['poses'][:10], color=col[:10])
    snap = vol.copy()
    before = snap.color_state().view(torch.int16).clone()
    vol.integrate(c['filt'][10:], c['k'][10:], c['poses'][10:], color=col[10:])
    assert torch.equal(snap.color_state().view(torch.int16), before)
    assert not torch.equal(vol.color_state().view(torch.int16), before)
    same_color(vol, c['ref'])

    # every pyramid level is the volume built with that level's dims, voxel size and transform
    pyr = fusion.TSDFPyramid(c['dims'], c['vs'], c['w2g'], levels=3, color=True)
    pyr.integrate(c['filt'], c['k'], c['poses'], color=c['rgba'])
    for k in range(3):
        lv = pyr[k]
        one = fusion.TSDFVolume(lv.dims_xyz, lv.voxel_size, lv.world2grid, color=True)
        one.integrate(c['filt'], c['k'], c['poses'], color=col)
        assert torch.equal(lv.color_state().view(torch.int16), one.color_state().view(torch.int16))
        same_geometry(lv, one)
        assert int(lv.color_weight().max()) > 0
    same_color(pyr[0], c['ref'])
    assert pyr.copy()[1].color_state().data_ptr() != pyr[1].color_state().data_ptr()

    full = vol.colors()
    dz, dy, dx = full.shape[:3]
    pad = vol.colors((dz + 16, dy, dx + 5))
    assert tuple(pad.shape) == (dz + 16, dy, dx + 5, 3) and torch.equal(pad[:dz, :, :dx], full)
    assert not pad[dz:].any() and not pad[:, :, dx:].any()
    crop = vol.colors((dz - 7, dy + 3, dx - 1))
    assert tuple(crop.shape) == (dz - 7, dy + 3, dx - 1, 3) and torch.equal(crop[:, :dy], full[:dz - 7, :, :dx - 1])
    assert not crop[:, dy:].any()
    assert vol.colors((dz, dy, dx)).data_ptr() != 0 and torch.equal(vol.colors((dz, dy, dx)), full)

    plain = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'])
    with pytest.raises(ValueError):
        plain.integrate(c['filt'][:2], c['k'][:2], c['poses'][:2], color=col[:2])
    with pytest.raises(ValueError):
        plain.colors()
    with pytest.raises(ValueError):
        vol.integrate(c['filt'][:2], c['k'][:2], c['poses'][:2], color=col[:3])                   # frame count
    with pytest.raises(ValueError):
        vol.integrate(c['filt'][:2], c['k'][:2], c['poses'][:2], color=col[:2, :, :-1].contiguous())   # width
    with pytest.raises(ValueError):
        vol.integrate(c['filt'][:2], c['k'][:2], c['poses'][:2], color=np.zeros((2, 48, 64, 2), np.uint8))
