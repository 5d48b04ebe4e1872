"""The NumPy restatement of colour rendering (tests/render_color_ref.py, INTEGRATION.md section N part A) against
facts that do not come from it: the colour of an affine colour function at the back-projected point, the depth of
tests/render_ref.py, and the independence of the image from how the faces are listed.  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402
import render_color_ref as RC  # noqa: E402

F32 = np.float32
HW = (48, 64)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def back_projected(depth, k, cam2world):
    """World points (h, w, 3) fp64 of the pixel centres at the rendered depth."""
    h, w = depth.shape
    fx, fy, cx, cy = (float(v) for v in k)
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = depth.astype(np.float64)
    cam = np.stack([(i - cx) / fx * z, (j - cy) / fy * z, z], -1)
    c2w = np.asarray(cam2world, np.float64)
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def colour_tolerance(depth, k):
    """What may separate a rendered channel from the affine colour at the back-projected point, per pixel.

    One colour unit: the vertex colours are the function rounded to integers (at most 0.5 off, and so is any convex
    combination of them) and the result is rounded once more (0.5).  The point the rasteriser interpolates lies on the
    triangle at the rendered depth, but the vertices were snapped to 1/256 pixel (each at most 1/512 pixel off per
    axis), so its image is at most 1/256 pixel from the pixel centre per axis: sqrt(2) z / (256 f) metres sideways at
    depth z, times the largest gradient of the function.  The fp32 roundings of depth and colour (a dozen operations
    of 2^-24 relative on values up to 255 and on a depth of a few metres) are covered by 0.001."""
    grad = float(np.abs(RC.AFFINE_GRAD).sum(0).max())
    f = float(min(k[0], k[1]))
    return 1.0 + grad * np.sqrt(2.0) * depth.astype(np.float64) / (256.0 * f) + 0.001


def oblique_scene():
    """One large triangle seen at a grazing angle (depth from 0.6 to 3.9 m across it) plus the room around it."""
    verts = np.array([[0.2, 0.3, 0.2], [3.9, 0.4, 0.3], [2.0, 3.0, 2.4]], F32)
    faces = np.array([[0, 1, 2]], np.int32)
    pose = R.look_at((0.1, 0.05, 0.15), (3.0, 1.6, 1.2))
    k = np.array([0.8 * HW[1], 0.8 * HW[1], (HW[1] - 1) / 2.0, (HW[0] - 1) / 2.0], F32)
    return verts, faces, k[None], pose[None]


def worst_excess(depth, rgba, k, poses):
    """The largest (|channel - affine colour at the back-projected point| - tolerance) over the finite pixels."""
    worst = -np.inf
    for f in range(len(depth)):
        seen = np.isfinite(depth[f])
        if not seen.any():
            continue
        want = RC.affine_color(back_projected(np.where(seen, depth[f], 1.0), k[f], poses[f]))
        err = np.abs(rgba[f, :, :, :3].astype(np.float64) - want).max(-1)
        worst = max(worst, float((err - colour_tolerance(depth[f], k[f]))[seen].max()))
    return worst


def test_colour_is_perspective_correct():
    # the room along a trajectory: thousands of triangles, near-plane clipping included
    _, k, poses = R.room_frames(6, HW, seed=2)
    near = np.stack([R.look_at((0.05, 0.5, 1.3), (0.6, 3.0, 1.2)), R.look_at((1.85, 1.3, 0.5), (1.6, 0.0, 0.4))])
    poses = np.concatenate([poses, near])
    k = np.tile(k[:1], (len(poses), 1))
    verts, faces = RR.tessellate_room(3)
    depth, rgba = RC.render_color_ref(verts, faces, RC.affine_vertex_colors(verts), k, poses, HW)
    seen = np.isfinite(depth)
    assert seen.mean() > 0.8 and (rgba[..., 3] == np.where(seen, 255, 0)).all()
    assert (rgba[~seen] == 0).all()
    assert worst_excess(depth, rgba, k, poses) <= 0.0
    # one oblique large triangle: the rule holds, and interpolation in screen space (the negative control) does not
    verts, faces, k, poses = oblique_scene()
    vcol = RC.affine_vertex_colors(verts)
    depth, rgba = RC.render_color_ref(verts, faces, vcol, k, poses, HW)
    assert np.isfinite(depth).sum() > 300 and np.nanmax(np.where(np.isfinite(depth), depth, np.nan)) > 2.0
    assert worst_excess(depth, rgba, k, poses) <= 0.0
    depth_s, rgba_s = RC.render_color_ref(verts, faces, vcol, k, poses, HW, perspective=False)
    assert np.array_equal(bits(depth_s), bits(depth))
    assert worst_excess(depth_s, rgba_s, k, poses) > 5.0


def test_depth_is_render_refs_depth():
    _, k, poses = R.room_frames(4, HW, seed=1)
    verts, faces = RR.tessellate_room(4)
    depth, _ = RC.render_color_ref(verts, faces, RC.affine_vertex_colors(verts), k, poses, HW)
    assert np.array_equal(bits(depth), bits(RR.render_ref(verts, faces, k, poses, HW)))
    verts, faces = RR.triangle_soup(400, seed=5)
    vcol = np.random.default_rng(1).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    kw = dict(depth_min=0.1, depth_max=50.0)
    depth, rgba = RC.render_color_ref(verts, faces, vcol, k[:2], poses[:2], (37, 53), **kw)
    assert np.isfinite(depth).mean() > 0.1
    assert np.array_equal(bits(depth), bits(RR.render_ref(verts, faces, k[:2], poses[:2], (37, 53), **kw)))


def test_order_of_faces_and_indices_changes_no_bit():
    verts, faces = RR.triangle_soup(300, seed=9)
    rng = np.random.default_rng(3)
    vcol = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    # coincident triangles of different colours: copies of some faces on copies of their vertices
    dup = faces[:40]
    verts = np.concatenate([verts, verts[dup.ravel()]])
    vcol = np.concatenate([vcol, rng.integers(0, 256, (dup.size, 3), dtype=np.uint8)])
    faces = np.concatenate([faces, len(verts) - dup.size + np.arange(dup.size, dtype=np.int32).reshape(-1, 3)])
    _, k, poses = R.room_frames(2, (37, 53), seed=3)
    near = R.look_at((0.05, 0.5, 1.3), (0.6, 3.0, 1.2))[None]
    poses, k = np.concatenate([poses, near]), np.tile(k[:1], (3, 1))
    kw = dict(depth_min=0.1, depth_max=50.0)
    depth, rgba = RC.render_color_ref(verts, faces, vcol, k, poses, (37, 53), **kw)
    assert np.isfinite(depth).mean() > 0.1 and len(np.unique(rgba.reshape(-1, 4), axis=0)) > 100
    variants = {
        'permuted': faces[rng.permutation(len(faces))],
        'reversed': faces[::-1],
        'windings': faces[:, ::-1],
        'rotated': np.roll(faces, 1, axis=1),
        'rotated twice': np.roll(faces, 2, axis=1),
    }
    for name, other in variants.items():
        d2, c2 = RC.render_color_ref(verts, other, vcol, k, poses, (37, 53), **kw)
        assert np.array_equal(bits(d2), bits(depth)), name
        assert np.array_equal(c2, rgba), name
