"""GPU: colour ray casting (sgnn_amd.raycast.cast_color, csrc/raycast.hip; INTEGRATION.md section N part B) against
the NumPy restatement of tests/raycast_color_ref.py, bit for bit, against raycast.cast, and the loop in colour: a
coloured mesh rendered to frames, fused, and cast back at the same poses."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import fusion_color_ref as FC  # noqa: E402
import raycast_ref as C  # noqa: E402
import raycast_color_ref as CC  # noqa: E402
import render_ref as RR  # noqa: E402
import render_color_ref as RC  # noqa: E402

from sgnn_amd import fusion, raycast, render  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HW = (24, 32)
VS = 0.18
BAND = F32(3.0) * F32(VS)
DIMS = (24, 20, 28)                                 # x, y, z
ORIGIN = (-0.05, -0.1, -0.9)                        # the room's four walls fall into the first and last cells of x and y


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


@pytest.fixture(scope='module')
def scene():
    """A 24 x 20 x 28 volume fused by the restatements from five painted 24 x 32 frames, a fifth of whose pixels
    have no colour, with further holes punched into the colour volume; the restatement's frames, computed once."""
    w2g = R.grid_transform(ORIGIN, VS)
    depth, k, poses = R.room_frames(5, HW, seed=2)
    painted = FC.painted_frames(k, poses, HW)[1]
    painted[..., 3] = np.where(np.random.default_rng(1).random(painted.shape[:3]) < 0.2, 0, painted[..., 3])
    grid = FC.ColorGrid(DIMS, VS, w2g).integrate(depth, k, poses, painted)
    sdf = grid.sdf.copy()
    rgba = np.concatenate([grid.colors(), np.where(grid.wc > 0, 255, 0).astype(np.uint8)[..., None]], -1)
    rng = np.random.default_rng(3)
    rgba[rng.random(sdf.shape) < 0.35, 3] = 0
    # a cell whose eight corners all lack a colour: the cell of the hit nearest to the centre of frame 0
    d0 = C.cast(sdf, w2g, VS, k[:1], poses[:1], HW, BAND)[0]
    o, d = C.rays(C.frame_matrix(w2g, poses[0]), k[0], HW)
    hits = np.nonzero(np.isfinite(d0).ravel())[0]
    px = int(hits[np.argmin((hits // HW[1] - HW[0] // 2) ** 2 + (hits % HW[1] - HW[1] // 2) ** 2)])
    x, y, z = (int(v) for v in np.floor((o + d0.ravel()[px] * d[px]).astype(F32)))
    rgba[z:z + 2, y:y + 2, x:x + 2, 3] = 0
    exp_d, exp_n, exp_c = CC.cast_color(sdf, rgba, w2g, VS, k, poses, HW, BAND, normals=True)
    return dict(sdf=sdf, rgba=rgba, w2g=w2g, k=k, poses=poses, depth=exp_d, normal=exp_n, color=exp_c, blank=(0, px))


def test_the_scene_covers_the_cases(scene):
    d, c = scene['depth'], scene['color']
    hit = np.isfinite(d)
    assert hit.mean() > 0.3 and (c[~hit] == 0).all()
    f, px = scene['blank']
    assert hit[f].ravel()[px] and (c[f].reshape(-1, 4)[px] == 0).all()          # all eight corners without a colour
    assert (c[hit][:, 3] == 0).sum() > 1 and (c[hit][:, 3] == 255).mean() > 0.8
    # hits in cells next to the volume border
    border = 0
    for f in range(len(d)):
        o, dirs = C.rays(C.frame_matrix(scene['w2g'], scene['poses'][f]), scene['k'][f], HW)
        m = hit[f].ravel()
        cell = np.floor((o + d[f].ravel()[m][:, None] * dirs[m]).astype(F32))
        border += int(((cell == 0) | (cell == np.array(DIMS) - 2)).any(1).sum())
    assert border > 20, border


def test_bitwise_with_normals_skip_and_chunks(scene):
    args = (scene['sdf'], scene['rgba'], scene['w2g'], VS, scene['k'], scene['poses'], HW, BAND)
    plain_d, plain_n = raycast.cast(args[0], *args[2:], normals=True)
    assert np.array_equal(bits(plain_d), bits(scene['depth'])) and np.array_equal(bits(plain_n), bits(scene['normal']))
    for kw in (dict(), dict(skip=False), dict(chunk=1), dict(chunk=2, skip=False)):
        depth, normal, rgba = raycast.cast_color(*args, normals=True, **kw)
        assert rgba.is_cuda and rgba.dtype == torch.uint8 and tuple(rgba.shape) == scene['color'].shape
        assert np.array_equal(bits(depth), bits(plain_d)), kw
        assert np.array_equal(bits(normal), bits(plain_n)), kw                 # NaN positions included
        diff = (rgba.cpu().numpy() != scene['color']).any(-1)
        assert not diff.any(), '%s: %d of %d pixels differ' % (kw, diff.sum(), diff.size)
        depth, rgba = raycast.cast_color(*args, **kw)
        assert np.array_equal(bits(depth), bits(plain_d)) and np.array_equal(rgba.cpu().numpy(), scene['color']), kw
    # device tensors, and an odd frame size
    t = torch.from_numpy
    depth, rgba = raycast.cast_color(t(scene['sdf']).cuda(), t(scene['rgba']).cuda(), *args[2:])
    assert np.array_equal(bits(depth), bits(plain_d)) and np.array_equal(rgba.cpu().numpy(), scene['color'])
    k = np.tile(np.array([20.0, 20.0, 12.0, 8.0], F32), (2, 1))
    exp = CC.cast_color(args[0], args[1], args[2], VS, k, scene['poses'][:2], (17, 25), BAND)
    got = raycast.cast_color(args[0], args[1], args[2], VS, k, scene['poses'][:2], (17, 25), BAND)
    assert np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(got[1].cpu().numpy(), exp[1])


def test_three_channels_count_every_voxel(scene):
    rgb = np.ascontiguousarray(scene['rgba'][..., :3])
    exp_d, exp_c = CC.cast_color(scene['sdf'], rgb, scene['w2g'], VS, scene['k'], scene['poses'], HW, BAND)
    hit = np.isfinite(exp_d)
    assert (exp_c[hit][:, 3] == 255).all() and (exp_c[..., :3] != scene['color'][..., :3]).any()
    depth, rgba = raycast.cast_color(scene['sdf'], rgb, scene['w2g'], VS, scene['k'], scene['poses'], HW, BAND)
    assert np.array_equal(bits(depth), bits(exp_d)) and np.array_equal(rgba.cpu().numpy(), exp_c)


def test_argument_errors(scene):
    args = (scene['w2g'], VS, scene['k'], scene['poses'], HW, BAND)
    for wrong in (scene['rgba'][1:], scene['rgba'][..., :2], scene['rgba'][..., 0], scene['rgba'].reshape(-1, 4)):
        with pytest.raises(ValueError, match='colors'):
            raycast.cast_color(scene['sdf'], wrong, *args)
    with pytest.raises(ValueError):
        raycast.cast_color(scene['sdf'], scene['rgba'], *args, step=0.0)
    vol = fusion.TSDFVolume(DIMS, VS, scene['w2g'])
    with pytest.raises(ValueError, match='colour'):
        raycast.cast_volume_color(vol, scene['k'], scene['poses'], HW)
    depth, rgba = raycast.cast_color(scene['sdf'], scene['rgba'], scene['w2g'], VS, scene['k'][:0], scene['poses'][:0], HW,
                                     BAND)
    assert tuple(depth.shape) == (0,) + HW and tuple(rgba.shape) == (0,) + HW + (4,)


def test_loop_closure_in_colour():
    """The analytic room as a mesh with affine vertex colours -> render_color at 24 poses of 48 x 64 ->
    TSDFVolume(color=True) of 88 x 72 x 60 voxels at 5 cm -> cast_volume_color at the same poses.

    Measured with the restatements alone (render_color_ref -> fusion_color_ref.ColorGrid -> raycast_color_ref) for
    trajectory seeds 0 to 3: over the 64 392 to 67 089 pixels with A = 255 in both stacks the median of
    |cast - rendered| is 0 in every channel for every seed (means 0.11 to 0.31 of a colour unit, 90th percentile 1),
    so the asserted value, 1.5 times the largest of the four medians, is 0.  Of the pixels finite in the rendered depth
    92.6 % to 93.8 % have A = 255 in the cast; 90 % is required."""
    hw, vs = (48, 64), 0.05
    dims, _, w2g = C.room_grid(vs, 4)
    assert dims == (88, 72, 60)
    _, k, poses = R.room_frames(24, hw)
    verts, faces = RR.tessellate_room(8)
    depth, rgba = render.render_color(verts, faces, RC.affine_vertex_colors(verts), k, poses, hw)
    vol = fusion.TSDFVolume(dims, vs, w2g, color=True).integrate(depth, k, poses, color=rgba)
    cast_d, cast_c = raycast.cast_volume_color(vol, k, poses, hw)
    # the cast is the restatement's on the fused volume, and its geometry is cast_volume's
    alpha = (vol.color_weight() > 0).to(torch.uint8) * 255
    colors = torch.cat([vol.colors(), alpha[..., None]], 3).cpu().numpy()
    exp_d, exp_c = CC.cast_color(vol.sdf().cpu().numpy(), colors, w2g, vs, k, poses, hw, F32(3.0) * F32(vs))
    assert np.array_equal(bits(cast_d), bits(exp_d)) and np.array_equal(cast_c.cpu().numpy(), exp_c)
    assert np.array_equal(bits(cast_d), bits(raycast.cast_volume(vol, k, poses, hw)))
    rendered, cast = rgba.cpu().numpy(), cast_c.cpu().numpy()
    both = (rendered[..., 3] == 255) & (cast[..., 3] == 255)
    diff = np.abs(cast[..., :3].astype(np.int64) - rendered[..., :3].astype(np.int64))[both]
    medians = [float(np.median(diff[:, c])) for c in range(3)]
    share = float((cast[..., 3] == 255)[np.isfinite(depth.cpu().numpy())].mean())
    print('colour loop closure: %d pixels, median |cast - rendered| per channel %s, means %s, coloured share %.4f' % (
        both.sum(), medians, [round(float(diff[:, c].mean()), 4) for c in range(3)], share))
    assert both.sum() > 0.8 * both.size
    assert all(m <= 1.5 * 0.0 for m in medians), medians
    assert share >= 0.90, share
