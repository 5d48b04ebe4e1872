"""The scoring entry point of register.search (csrc/register_search.hip) is declared, exported by the built library and
bound with the header's argument count; the record has the header's size and field; the host pose table turns
non-finite input into NaN records; every ValueError of the section is raised without a device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_register_score']


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_score_symbol_is_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_score_prototype_matches_the_header():
    from sgnn_amd import _lib
    src = header()
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params) == 12, name


def test_pose_dtype():
    from sgnn_amd import register
    record = re.search(r'typedef struct sgnn_register_pose \{(.*?)\}', header(), flags=re.S).group(1)
    fields = re.findall(r'float (\w+)\[(\d+)\]', record)
    assert fields == [('m', '12')]
    assert register.POSE_DTYPE.itemsize == 48 and register.POSE_DTYPE.names == ('m',)
    assert register.POSE_DTYPE['m'].shape == (12,) and register.POSE_DTYPE['m'].base == np.dtype('<f4')
    assert int(re.search(r'#define SGNN_REGISTER_SCORE_MAX_POSES \(1 << (\d+)\)', header()).group(1)) == 24
    assert register.MAX_POSES == 1 << 24


def test_non_finite_input_gives_nan_records():
    from sgnn_amd import register
    w2g = np.diag([20.0, 20.0, 20.0, 1.0])
    w2g[:3, 3] = [1.5, -2.0, 0.25]
    move = np.eye(4)
    move[:3, 3] = [0.5, 0.25, -1.0]
    bad, big, low = np.eye(4), np.eye(4), np.eye(4)
    bad[0, 3] = np.inf
    big[2, 3] = 1e300                                                       # finite in fp64, its product not in fp32
    low[3, 0] = np.nan                                                      # the last row counts too
    table = register.pose_table(w2g, np.stack([np.eye(4), move, bad, big, low]))
    assert table.dtype == register.POSE_DTYPE and table.shape == (5,)
    assert np.array_equal(table['m'][0], w2g[:3].astype(np.float32).ravel())
    assert np.array_equal(table['m'][1], (w2g @ move)[:3].astype(np.float32).ravel())     # exact: small dyadic numbers
    assert np.isnan(table['m'][2:]).all()
    for value in (np.nan, np.inf, 1e300):                                   # 1e300 is not finite once world2grid is fp32
        w = w2g.copy()
        w[1, 1] = value
        assert np.isnan(register.pose_table(w, np.eye(4)[None])['m']).all()
    with pytest.raises(ValueError):
        register.pose_table(w2g, np.eye(4))
    with pytest.raises(ValueError):
        register.pose_table(np.eye(3), np.eye(4)[None])


def no_device(monkeypatch):
    """From here on any attempt to get at a device fails the test."""
    from sgnn_amd import _lib

    def refuse():
        raise AssertionError('a device was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'require_gpu', refuse)


def volume():
    sdf = np.ones((6, 7, 8), np.float32)
    sdf[:, :, 4:] = -1.0
    return sdf, np.diag([20.0, 20.0, 20.0, 1.0]).astype(np.float32), 3.0


def test_search_checks_its_arguments_without_a_device(monkeypatch):
    from sgnn_amd import register
    no_device(monkeypatch)
    pts = np.zeros((10, 3), np.float32)
    vol = volume()
    for kwargs in (dict(yaw_step=0), dict(yaw_step=-5.0), dict(yaw_step=float('nan')), dict(step=0), dict(step=-1.0),
                   dict(reach=0), dict(reach=-2.0), dict(top=0), dict(top=1.5), dict(levels=0), dict(levels=-1),
                   dict(max_points=0), dict(up=(0, 0, 0)), dict(up=(0, 1)), dict(z_range=(1.0, 0.0)),
                   dict(z_range=(0.0,)), dict(rotations=np.eye(3)), dict(rotations=np.zeros((0, 3, 3))),
                   dict(rotations=np.full((2, 3, 3), np.nan))):
        with pytest.raises(ValueError):
            register.search(pts, vol, **kwargs)
    for bad_points in (np.zeros((10, 2), np.float32), np.zeros(3, np.float32), np.zeros((0, 3), np.float32)):
        with pytest.raises(ValueError):
            register.search(bad_points, vol)
    for bad_vol in ((np.ones((6, 7), np.float32),) + vol[1:], (np.ones((2, 2, 1025), np.float32),) + vol[1:],
                    (vol[0], np.eye(3), 3.0), (vol[0], np.zeros((4, 4)), 3.0), 'room'):
        with pytest.raises(ValueError):
            register.search(pts, bad_vol)
    with pytest.raises(ValueError):
        register.search_volumes(vol, vol)                                   # the source must be a TSDFVolume


def test_level_0_has_a_limit_and_names_the_count(monkeypatch):
    from sgnn_amd import register
    no_device(monkeypatch)

    class Shape(object):                                                    # the check comes before the sdf is touched
        shape = (512, 1024, 1024)
    vol = (Shape(), np.diag([50.0, 50.0, 50.0, 1.0]).astype(np.float32), 0.06)
    origin, counts, pitch = register.lattice(Shape.shape, vol[1], 0.02)
    total = 720 * counts[0] * counts[1] * counts[2]
    assert total > register.MAX_POSES * register.MAX_LAUNCHES
    with pytest.raises(ValueError, match=str(total)):
        register.search(np.zeros((10, 3), np.float32), vol, yaw_step=0.5, step=0.02)


def test_score_and_distance_field_check_their_arguments_without_a_device(monkeypatch):
    import torch
    from sgnn_amd import register
    no_device(monkeypatch)
    vol = volume()
    for reach in (0, -1.0, float('inf'), float('nan'), 0.5, 1e6):           # 0.5 voxels: cap2 = 0; 1e6: its square >= 2^31
        with pytest.raises(ValueError):
            register.distance_field(vol, reach)
    for bad_vol in ((np.ones((6, 7), np.float32),) + vol[1:], (np.ones((1, 1, 1025), np.float32),) + vol[1:], None):
        with pytest.raises(ValueError):
            register.distance_field(bad_vol)
    field = register.SearchField(torch.zeros((2, 3, 5), dtype=torch.int32), vol[1], (2, 3, 5), 9)
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        register.score(np.zeros((4, 2), np.float32), field, np.eye(4))
    with pytest.raises(ValueError):
        register.score(pts, field, np.eye(3))
    with pytest.raises(ValueError):
        register.score(pts, field, np.eye(4), inlier=-1.0)
    with pytest.raises(ValueError):
        register.score(pts, field, np.eye(4), inlier=1e6)
    for bad_field in (None, field._replace(dist2=field.dist2.float()), field._replace(dims=(2, 3, 4)),
                      field._replace(cap2=0)):
        with pytest.raises(ValueError):
            register.score(pts, bad_field, np.eye(4))


def test_lattice_by_hand():
    """An 8 x 7 x 6 grid of 5 cm voxels from the origin: the box of the voxel centres is 0.35 x 0.30 x 0.25 m."""
    from sgnn_amd import register
    w2g = np.diag([20.0, 20.0, 20.0, 1.0]).astype(np.float32)
    origin, counts, pitch = register.lattice((6, 7, 8), w2g)
    assert np.allclose(origin, 0) and abs(pitch - 0.2) < 1e-12 and counts == (2, 2, 2)
    origin, counts, pitch = register.lattice((6, 7, 8), w2g, 0.1, (0, 0, 1), (0.05, 0.16))
    assert counts == (4, 4, 2) and abs(origin[2] - 0.05) < 1e-15
    origin, counts, _ = register.lattice((6, 7, 8), w2g, 0.1, (0.1, -2.0, 0.3), (0.05, 0.16))   # up is mostly y
    assert counts == (4, 2, 3) and abs(origin[1] - 0.05) < 1e-15
