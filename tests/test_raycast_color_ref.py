"""The NumPy restatement of colour ray casting (tests/raycast_color_ref.py, INTEGRATION.md section N part B) against
facts that do not come from it: a constant colour comes back unchanged, no colour gives nothing, and a hole in the
colour volume narrows the corners used and never darkens the result.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402
import raycast_color_ref as CC  # noqa: E402

F32 = np.float32
HW = (24, 32)
VS = 0.05
BAND = F32(3.0) * F32(VS)


@pytest.fixture(scope='module')
def room():
    sdf, w2g = C.room_sdf(VS, 4, BAND)
    _, k, poses = R.room_frames(3, HW, seed=1)
    depth = C.cast(sdf, w2g, VS, k, poses, HW, BAND)
    assert np.isfinite(depth).mean() > 0.9
    return dict(sdf=sdf, w2g=w2g, k=k, poses=poses, depth=depth)


def cast(room, colors, **kw):
    return CC.cast_color(room['sdf'], colors, room['w2g'], VS, room['k'], room['poses'], HW, BAND, **kw)


def test_constant_colour_comes_back(room):
    hit = np.isfinite(room['depth'])
    for rgb in ((200, 40, 30), (0, 0, 0), (255, 255, 255), (1, 128, 254)):
        colors = np.empty(room['sdf'].shape + (3,), np.uint8)
        colors[:] = rgb
        depth, rgba = cast(room, colors)
        assert np.array_equal(depth.view(np.int32), room['depth'].view(np.int32))
        assert (rgba[hit] == np.array(rgb + (255,), np.uint8)).all()
        assert (rgba[~hit] == 0).all()
    # the same through four channels, and with normals: the geometry is raycast_ref's
    colors = np.empty(room['sdf'].shape + (4,), np.uint8)
    colors[:] = (9, 99, 199, 1)
    depth, normal, rgba = cast(room, colors, normals=True)
    d0, n0 = C.cast(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, BAND, normals=True)
    assert np.array_equal(depth.view(np.int32), d0.view(np.int32)) and np.array_equal(normal.view(np.int32), n0.view(np.int32))
    assert (rgba[hit] == np.array((9, 99, 199, 255), np.uint8)).all()


def test_no_colour_gives_nothing(room):
    colors = np.random.default_rng(0).integers(0, 256, room['sdf'].shape + (4,), dtype=np.uint8)
    colors[..., 3] = 0
    depth, rgba = cast(room, colors)
    assert np.isfinite(depth).any() and (rgba == 0).all()


def test_holes_narrow_the_corners_and_do_not_darken(room):
    rng = np.random.default_rng(4)
    colors = rng.integers(0, 256, room['sdf'].shape + (4,), dtype=np.uint8)
    colors[..., 3] = np.where(rng.random(room['sdf'].shape) < 0.6, 0, rng.integers(1, 256, room['sdf'].shape))
    depth, rgba = cast(room, colors)
    h, w = HW
    some = none = 0
    for f in range(len(depth)):
        g = C.frame_matrix(room['w2g'], room['poses'][f])
        o, d = C.rays(g, room['k'][f], HW)
        for px in np.nonzero(np.isfinite(depth[f]).ravel())[0]:
            p = (o + depth[f].ravel()[px] * d[px]).astype(F32)
            x, y, z = (int(v) for v in np.floor(p))
            corners = colors[z:z + 2, y:y + 2, x:x + 2].reshape(8, 4)
            used = corners[corners[:, 3] != 0]
            got = rgba[f].reshape(h * w, 4)[px]
            if len(used) == 0:
                assert (got == 0).all()
                none += 1
                continue
            # a corner of weight zero (a hit exactly on a cell face) may be the only coloured one: then S == 0
            if got[3] == 0:
                assert (p == np.floor(p)).any()
                continue
            some += 1
            assert got[3] == 255
            assert (got[:3] >= used[:, :3].min(0)).all() and (got[:3] <= used[:, :3].max(0)).all()
    assert some > 1000 and none > 5, (some, none)
