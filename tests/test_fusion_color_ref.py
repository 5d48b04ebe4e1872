"""The NumPy restatement of the colour rules (tests/fusion_color_ref.py) checked on its own,
on the two scenes of tests/test_gpu_fusion.py: its geometry is fusion_ref.Grid's, the colour state obeys the rules'
invariants, and the conditions that tests/test_gpu_fusion_color.py puts on the coloured meshes hold for the
reference alone (meshes from oracle/mc_oracle.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import fusion_color_ref as C  # noqa: E402
import fusion_ref as R  # noqa: E402
import mc_oracle  # noqa: E402
from test_gpu_fusion import CASES, scene  # noqa: E402

F32 = np.float32
UNIFORM = (10, 200, 77)


@pytest.fixture(scope='module')
def scenes():
    out = {}
    for case in CASES:
        dims, vs, w2g, obb, depth, k, poses = scene(case)
        filt = R.bilateral64(depth).astype(F32)
        c = dict(dims=dims, vs=vs, w2g=w2g, obb=obb, filt=filt, k=k, poses=poses)
        c['geom'] = R.Grid(dims, vs, w2g, obb=obb).integrate(filt, k, poses)
        c['noise'] = C.ColorGrid(dims, vs, w2g, obb=obb).integrate(filt, k, poses, C.noise_frames(filt.shape, 11))
        c['uniform'] = C.ColorGrid(dims, vs, w2g, obb=obb).integrate(filt, k, poses,
                                                                    C.uniform_frames(filt.shape, UNIFORM, 12))
        out[case] = c
    return out


@pytest.mark.parametrize('case', CASES)
def test_geometry_is_the_depth_only_reference(scenes, case):
    c = scenes[case]
    for g in (c['noise'], c['uniform']):
        assert np.array_equal(g.sdf.view(np.int32), c['geom'].sdf.view(np.int32))
        assert np.array_equal(g.weight, c['geom'].weight)
        assert np.array_equal(g.free, c['geom'].free)
    # without colour frames the colour state is never touched
    plain = C.ColorGrid(c['dims'], c['vs'], c['w2g'], obb=c['obb']).integrate(c['filt'][:6], c['k'][:6], c['poses'][:6])
    assert not plain.q.any() and not plain.wc.any() and np.isfinite(plain.sdf).any()


@pytest.mark.parametrize('case', CASES)
def test_colour_state_invariants(scenes, case):
    g = scenes[case]['noise']
    fin = np.isfinite(g.sdf)
    assert (g.wc <= g.weight).all()
    assert not (g.wc[~fin] > 0).any()
    assert (fin & (g.wc > 0)).sum() > 1000 and (fin & (g.wc == 0)).sum() > 100
    assert g.q.min() >= 0 and g.q.max() <= 255 * 256 and not g.q[g.wc == 0].any()
    if case == 'odd37x53x29':
        assert g.wc.max() == 255
    st = g.state()
    assert st.dtype == np.uint16 and st.shape == g.sdf.shape + (4,)
    assert np.array_equal(st[..., :3].astype(np.int64), g.q) and np.array_equal(st[..., 3].astype(np.int64), g.wc)


@pytest.mark.parametrize('case', CASES)
def test_uniform_frames_give_exactly_that_colour(scenes, case):
    g = scenes[case]['uniform']
    assert (g.wc > 0).sum() > 1000
    assert (g.q[g.wc > 0] == np.array(UNIFORM) * 256).all()
    assert (g.colors()[g.wc > 0] == np.array(UNIFORM)).all() and not g.colors()[g.wc == 0].any()
    # the mesh condition of the GPU test: only that colour or black, and few black vertices
    v, col, f = mc_oracle.run_marching_cubes(g.sdf, g.colors(), *C.mc_args(scenes[case]['vs']))
    assert len(v) > 400 and len(f) > 400
    black = (col == 0).all(1)
    assert (col[~black] == np.array(UNIFORM)).all()
    print('%s: %d vertices, black share %.4f' % (case, len(v), black.mean()))
    assert C.black_share(col) <= C.BLACK_SHARE_CAP


def test_pack_rules():
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, size=(2, 48, 64, 4), dtype=np.uint8)
    raw[..., 3] = np.where(rng.random(raw.shape[:3]) < 0.3, 0, 255)
    assert np.array_equal(C.pack(raw), raw)                              # equal sizes: the identity
    raw[0, 0, 0, 3] = 7
    assert C.pack(raw)[0, 0, 0, 3] == 255
    rgb = rng.integers(0, 256, size=(3, 97, 131, 3), dtype=np.uint8)
    out = C.pack(rgb, (61, 83))
    assert out.shape == (3, 61, 83, 4) and (out[..., 3] == 255).all()
    assert np.array_equal(out[:, 0, 0, :3], rgb[:, 0, 0]) and np.array_equal(out[:, -1, -1, :3], rgb[:, -1, -1])
    assert np.array_equal(out[1, 30, 41, :3], rgb[1, 48, 65])           # round(30 * 96/60) = 48, round(41 * 130/82) = 65
    assert C.pack(rgb[0], (61, 83)).shape == (1, 61, 83, 4)


def test_painted_room_conditions(scenes):
    c = scenes['cube48']
    hw = c['filt'].shape[1:]
    depth, rgba = C.painted_frames(c['k'], c['poses'], hw)
    for f in (0, 7):                                                     # the painted depth is fusion_ref.render's
        assert np.array_equal(depth[f], R.render(c['k'][f], c['poses'][f], hw, R.ROOM_PLANES, R.ROOM_BOXES))
    assert (rgba[..., 3] == 255).all() and len(np.unique(rgba[..., :3].reshape(-1, 3), axis=0)) >= 8
    g = C.ColorGrid(c['dims'], c['vs'], c['w2g']).integrate(c['filt'], c['k'], c['poses'], rgba)
    v, col, _ = mc_oracle.run_marching_cubes(g.sdf, g.colors(), *C.mc_args(c['vs']))
    own, keep = C.painted_expectation(v, c['w2g'], C.painted_margin(c['vs'], c['k'][0][0]))
    print('painted room: %d vertices, kept share %.4f, wrong among kept %d' % (
        len(v), keep.mean(), (col[keep] != own[keep]).any(1).sum()))
    assert len(v) > 400
    assert keep.mean() >= C.KEPT_SHARE_MIN
    assert (col[keep] == own[keep]).all()
