"""GPU: colour rendering (sgnn_amd.render.render_color, csrc/render.hip; INTEGRATION.md section N part A) against the
NumPy restatement of tests/render_color_ref.py, bit for bit in depth and colour, and against render_depth."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402
import render_color_ref as RC  # noqa: E402

from sgnn_amd import render  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HW = (37, 53)                                       # a multiple of no tile
WIDE = dict(depth_min=0.1, depth_max=50.0)
EYE = np.eye(4)[None]                               # camera at the origin: x right, y down, z forward


def intrinsics(hw, n=1):
    return np.tile(np.array([0.8 * hw[1], 0.8 * hw[1], (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0], F32), (n, 1))


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def check(verts, faces, vcol, k, poses, hw, counters=None, **kw):
    """render_color == the restatement in every bit, and its depth == render_depth's.  Returns the restatement."""
    exp_d, exp_c = RC.render_color_ref(verts, faces, vcol, k, poses, hw, **kw)
    depth, rgba = render.render_color(verts, faces, vcol, k, poses, hw, counters=counters, **kw)
    assert depth.is_cuda and depth.dtype == torch.float32 and tuple(depth.shape) == exp_d.shape
    assert rgba.is_cuda and rgba.dtype == torch.uint8 and tuple(rgba.shape) == exp_c.shape
    d, c = bits(depth), rgba.cpu().numpy()
    assert np.array_equal(d, bits(exp_d)), '%d of %d depth pixels differ' % ((d != bits(exp_d)).sum(), d.size)
    assert np.array_equal(c, exp_c), '%d of %d colour pixels differ' % ((c != exp_c).any(-1).sum(), d.size)
    assert np.array_equal(d, bits(render.render_depth(verts, faces, k, poses, hw, **kw)))
    assert np.array_equal(c[..., 3], np.where(np.isfinite(exp_d), 255, 0))
    return exp_d, exp_c


@pytest.fixture(scope='module')
def soup():
    """About 200 random triangles, two large ones among them, seen from 9 poses (more than the 8 frames a thread
    walks) of 37 x 53."""
    verts, faces = RR.triangle_soup(200, seed=11)
    big = np.array([[0.2, 0.2, 0.1], [3.8, 0.3, 0.2], [2.0, 3.0, 0.3], [0.3, 0.2, 2.4], [3.7, 0.4, 2.5], [0.4, 3.0, 2.3]], F32)
    faces = np.concatenate([faces, len(verts) + np.array([[0, 1, 2], [3, 5, 4]], np.int32)])
    verts = np.concatenate([verts, big])
    vcol = np.random.default_rng(2).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    _, _, poses = R.room_frames(9, HW, seed=5)
    return verts, faces, vcol, intrinsics(HW, 9), poses


def test_soup_bitwise_on_both_raster_paths(soup):
    verts, faces, vcol, k, poses = soup
    c = torch.zeros(3, dtype=torch.int64, device='cuda')
    exp_d, exp_c = check(verts, faces, vcol, k, poses, HW, counters=c, **WIDE)
    lane, wave, pixels = (int(v) for v in c.cpu())
    assert lane > 50 and wave > 0, (lane, wave)                         # pixel boxes of at most and of more than 128 pixels
    assert pixels >= np.isfinite(exp_d).sum() > 0.2 * exp_d.size
    assert len(np.unique(exp_c.reshape(-1, 4), axis=0)) > 500
    old = render.WAVE_PIXELS
    try:
        for wave_pixels in (1, 1 << 30):                                # everything per wave, everything per lane
            render.WAVE_PIXELS = wave_pixels
            c.zero_()
            check(verts, faces, vcol, k, poses, HW, counters=c, **WIDE)
            assert (int(c[1]) == 0) if wave_pixels > 1 else (int(c[1]) > int(c[0]))
    finally:
        render.WAVE_PIXELS = old


def test_chunks_residence_and_face_order_change_no_bit(soup):
    verts, faces, vcol, k, poses = soup
    exp_d, exp_c = RC.render_color_ref(verts, faces, vcol, k, poses, HW, **WIDE)
    t = torch.from_numpy
    rng = np.random.default_rng(0)
    shuffled = faces[rng.permutation(len(faces))]
    shuffled[::2] = shuffled[::2, ::-1]
    for args, kw in (((verts, faces, vcol, k, poses), dict(chunk=1)),
                     ((verts, faces, vcol, k, poses), dict(chunk=4)),
                     ((verts, shuffled, vcol, k, poses), {}),
                     ((t(verts).cuda(), t(faces).cuda(), t(vcol).cuda(), t(k).cuda(), t(poses).cuda()), {}),
                     ((t(verts), t(faces).to(torch.int64), t(vcol), k, poses), {})):
        depth, rgba = render.render_color(*args, HW, **WIDE, **kw)
        assert np.array_equal(bits(depth), bits(exp_d)) and np.array_equal(rgba.cpu().numpy(), exp_c)


def test_near_plane_clipping_carries_colour():
    # camera-space = world: z is the depth.  Faces 0 and 1 share the edge 0-2, which crosses the near plane: face 0
    # keeps two vertices, face 1 one.  Face 2 keeps one vertex, face 3 two.
    verts = np.array([[-0.5, 0.3, 0.8], [0.5, 0.3, 0.9], [0.4, -0.2, -0.4], [-0.4, -0.3, -0.5],
                      [0.0, -0.5, 1.2], [-0.4, -0.4, -0.3], [0.4, -0.45, -0.2],
                      [-0.6, 0.5, 1.0], [0.6, 0.5, 1.0], [0.0, 0.45, -0.5]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 9, 8]], np.int32)
    kept = (verts[faces][:, :, 2] >= 0.1).sum(1)
    assert kept.tolist() == [2, 1, 1, 2]
    vcol = np.random.default_rng(5).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    k = intrinsics(HW)
    exp_d, exp_c = check(verts, faces, vcol, k, EYE, HW, **WIDE)
    assert np.isfinite(exp_d).sum() > 100 and exp_d[np.isfinite(exp_d)].min() < 0.15   # drawn up to the near plane
    for order in ([1, 0, 2, 3], [3, 2, 1, 0]):
        d2, c2 = render.render_color(verts, faces[order][:, [1, 2, 0]], vcol, k, EYE, HW, **WIDE)
        assert np.array_equal(bits(d2), bits(exp_d)) and np.array_equal(c2.cpu().numpy(), exp_c)
    check(verts, faces, vcol, k, EYE, HW, z_clip=0.3, depth_min=0.3, depth_max=2.5)


def test_coincident_triangles_the_smaller_colour_wins():
    tri = np.array([[-0.6, -0.4, 1.0], [0.6, -0.4, 1.4], [0.0, 0.5, 1.2]], F32)
    verts = np.concatenate([tri, tri])
    ca, cb = (10, 200, 30), (10, 199, 250)                                # cb packs to the smaller number
    vcol = np.array([ca] * 3 + [cb] * 3, np.uint8)
    k = intrinsics(HW)
    for faces in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]], [[2, 1, 0], [4, 5, 3]]):
        exp_d, exp_c = check(verts, np.array(faces, np.int32), vcol, k, EYE, HW)
        seen = np.isfinite(exp_d)
        assert seen.sum() > 100 and (exp_c[seen] == np.array(cb + (255,), np.uint8)).all()


def test_empty_frames_and_the_range_test():
    verts, faces = RR.tessellate_room(2)
    vcol = RC.affine_vertex_colors(verts)
    _, _, poses = R.room_frames(3, HW, seed=4)
    poses[1, 1, 2] = np.nan                                               # a NaN pose: an empty frame
    exp_d, exp_c = check(verts, faces, vcol, intrinsics(HW, 3), poses, HW)
    assert (exp_d[1] == -np.inf).all() and (exp_c[1] == 0).all() and np.isfinite(exp_d[0]).mean() > 0.8
    # a small triangle between z_clip and depth_min hides the wall behind it: depth -inf, A = 0
    verts = np.array([[-0.05, -0.05, 0.25], [0.05, -0.05, 0.25], [0.0, 0.06, 0.25],
                      [-2.0, -2.0, 1.5], [2.0, -2.0, 1.5], [0.0, 3.0, 1.5]], F32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    vcol = np.array([[255, 0, 0]] * 3 + [[0, 0, 255]] * 3, np.uint8)
    exp_d, exp_c = check(verts, faces, vcol, intrinsics(HW), EYE, HW)
    centre = (HW[0] // 2, HW[1] // 2)
    assert exp_d[0][centre] == -np.inf and (exp_c[0][centre] == 0).all()
    assert exp_d[0, 2, 2] == F32(1.5) and (exp_c[0, 2, 2] == (0, 0, 255, 255)).all()
    assert 5 < (exp_d[0] == -np.inf).sum() < 200


def test_empty_mesh_and_no_frames():
    k, hw = intrinsics(HW, 2), HW
    poses = np.tile(EYE, (2, 1, 1))
    none_v, none_f, none_c = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8)
    exp_d, exp_c = check(none_v, none_f, none_c, k, poses, hw)
    assert (exp_d == -np.inf).all() and (exp_c == 0).all()
    verts, faces = RR.tessellate_room(1)
    depth, rgba = render.render_color(verts, faces, RC.affine_vertex_colors(verts), k[:0], poses[:0], hw)
    assert tuple(depth.shape) == (0,) + hw and tuple(rgba.shape) == (0,) + hw + (4,) and rgba.dtype == torch.uint8


def test_argument_errors():
    verts, faces = RR.tessellate_room(2)
    vcol = RC.affine_vertex_colors(verts)
    _, _, poses = R.room_frames(2, HW, seed=1)
    k = intrinsics(HW, 2)
    t = torch.from_numpy
    for index in (len(verts), -1):
        bad = faces.copy()
        bad[7, 1] = index
        with pytest.raises(ValueError, match='face index'):
            render.render_color(verts, bad, vcol, k, poses, HW)                       # host arrays
        with pytest.raises(ValueError, match='face index'):
            render.render_color(t(verts).cuda(), t(bad).cuda(), t(vcol).cuda(), k, poses, HW)   # device arrays
    for wrong in (vcol[:-1], vcol[:, :2], vcol.ravel(), np.concatenate([vcol, vcol[:, :1]], 1)):
        with pytest.raises(ValueError, match='vcolors'):
            render.render_color(verts, faces, wrong, k, poses, HW)
    with pytest.raises(ValueError):
        render.render_color(verts[:, :2], faces, vcol, k, poses, HW)
    with pytest.raises(ValueError):
        render.render_color(verts, faces, vcol, k, poses[:1], HW)
    with pytest.raises(ValueError):
        render.render_color(verts, faces, vcol, k, poses, HW, z_clip=0.0)
    check(verts, faces, vcol, k, poses, HW)
