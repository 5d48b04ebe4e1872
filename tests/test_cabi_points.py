"""The point-cloud entry points (sgnn_amd.points, csrc/points.hip) are declared, exported by the built library and
bound with the header's argument counts; the unit is built with its contract line; the public calls check their
arguments before they need a device and need one after.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_points_'
F32 = np.float32


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % PREFIX, _header())))


def _library():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_the_header_declares_the_three_passes():
    assert _declared() == ['sgnn_points_count', 'sgnn_points_fold', 'sgnn_points_walk']


def test_declared_names_are_the_exported_names():
    from sgnn_amd import _lib
    lib = _library()
    declared = _declared()
    assert [n for n in declared if not hasattr(lib, n)] == []
    # the other half, with no tool: a symbol's name is a NUL-terminated string of the library's string tables, so every
    # name under the prefix that the file holds must be a declared one (kernels are mangled and do not begin with it)
    data = open(_lib.LIB_PATH, 'rb').read()
    held = sorted(set(m.decode() for m in re.findall(rb'\0(%s[a-z0-9_]+)(?=\0)' % PREFIX.encode(), data)))
    assert held == declared


def test_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    declared = _declared()
    assert declared == sorted(n for n in _lib.PROTOTYPES if n.startswith(PREFIX))
    for name in declared:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name


def test_the_unit_is_built_with_its_contract_line_and_the_limit_of_the_header():
    from sgnn_amd import points
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'points.hip' in srcs
    assert re.search(r'^#.*tests/points_ref\.py.*\n\.\./lib/points\.o:\s*CXXFLAGS \+= -ffp-contract=off$', mk, flags=re.M)
    assert int(re.search(r'#define SGNN_POINTS_MAX_RAYS \(1ll << (\d+)\)', _header()).group(1)) == 28
    assert points.MAX_RAYS == 1 << 28


def _stub(color=False, voxel_size=0.05, depth_max=4.0):
    """A TSDFVolume without its device arrays: what the argument checks look at."""
    from sgnn_amd import fusion
    v = fusion.TSDFVolume.__new__(fusion.TSDFVolume)
    v.device, v.dims_xyz, v.voxel_size, v.world2grid = None, (8, 8, 8), F32(voxel_size), np.eye(4, dtype=F32)
    v.depth_min, v.depth_max, v.obb, v._color = F32(0.4), F32(depth_max), None, (object() if color else None)
    return v


def test_integrate_needs_a_device(monkeypatch):
    from sgnn_amd import _lib, fusion, points
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    pts = np.zeros((5, 3), F32)
    with pytest.raises(_lib.SgnnError):
        points.integrate(_stub(), pts, np.zeros((1, 3), F32))
    with pytest.raises(_lib.SgnnError):
        points.integrate(_stub(color=True), torch.from_numpy(pts), np.zeros(3, F32), color=np.zeros((5, 4), np.uint8))
    with pytest.raises(_lib.SgnnError):
        points.integrate(_stub(), pts, np.zeros((2, 3), F32), origin_id=np.array([0, 1, 1, 0, 1]), carve=False, chunk=2)
    with pytest.raises(_lib.SgnnError):
        fusion.TSDFVolume((8, 8, 8), 0.05, np.eye(4))                 # the snippet's volume needs one as before


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import points
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    pts, one, two = np.zeros((5, 3), F32), np.zeros((1, 3), F32), np.zeros((2, 3), F32)
    bad = [
        dict(points=np.zeros((5, 2), F32), origins=one),                        # wrong shapes
        dict(points=np.zeros(15, F32), origins=one),
        dict(points=pts, origins=np.zeros((1, 4), F32)),
        dict(points=pts, origins=np.zeros((1, 1, 3), F32)),
        dict(points=pts, origins=two),                                          # two origins and no origin_id
        dict(points=pts, origins=two, origin_id=np.zeros(4, np.int32)),         # P does not match
        dict(points=pts, origins=two, origin_id=np.zeros((5, 1), np.int32)),
        dict(points=pts, origins=two, origin_id=np.array([0, 1, 2, 0, 0])),     # outside [0, S)
        dict(points=pts, origins=two, origin_id=np.array([0, -1, 1, 0, 0])),
        dict(points=pts, origins=one, color=np.zeros((5, 3), np.uint8)),        # colour for a volume without
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            points.integrate(_stub(), **kw)
    for color in (np.zeros((4, 3), np.uint8), np.zeros((5, 2), np.uint8), np.zeros((5, 3), F32), np.zeros(15, np.uint8)):
        with pytest.raises(ValueError):
            points.integrate(_stub(color=True), pts, one, color=torch.from_numpy(color))
    with pytest.raises(ValueError):
        points.integrate(_stub(voxel_size=1e-6, depth_max=12.0), pts, one)      # more samples on a ray than fp32 counts


def test_grid_for_and_from_depth_and_load_ply_points_run_on_the_host(tmp_path):
    from sgnn_amd import marching_cubes as mc, points
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.3, 2.1, (50, 3)).astype(F32)
    pts[7] = np.nan
    dims, w2g = points.grid_for(pts, 0.02, pad=8)
    g = pts[np.isfinite(pts).all(1)].astype(np.float64) @ w2g[:3, :3].T + w2g[:3, 3]
    assert g.min() >= 8 - 1e-9 and (g.max(0) <= np.array(dims) - 1 - 8 + 1e-9).all()
    assert (g.min(0) < 9).all() and (g.max(0) > np.array(dims) - 10).all()
    assert np.allclose(w2g[:3, :3], np.eye(3) / 0.02) and np.array_equal(w2g[:3, 3], np.round(w2g[:3, 3]))
    for args in ((np.zeros((0, 3)), 0.02), (pts, 0.0), (np.full((3, 3), np.nan), 0.02)):
        with pytest.raises(ValueError):
            points.grid_for(*args)
    # PLY files with and without faces, with and without colours
    path = str(tmp_path / 'cloud.ply')
    mc.write_points_ply(pts[:7], path)
    got, cols = points.load_ply_points(path)
    assert np.array_equal(got, pts[:7]) and cols is None
    rgb = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    mc.save_to_ply(path, torch.from_numpy(pts[:7]), torch.from_numpy(rgb), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    got, cols = points.load_ply_points(path)
    assert np.array_equal(got, pts[:7]) and np.array_equal(cols, rgb)
    # one frame, by hand: pixel (u, v) at depth z -> ((u - cx) z / fx, (v - cy) z / fy, z), then the pose
    depth = np.array([[1.0, 2.0, -np.inf], [0.5, 1.5, 1.0]], F32)
    pose = np.eye(4)
    pose[:3, 3] = (1.0, 2.0, 3.0)
    p, o, i = points.from_depth(depth, np.array([2.0, 4.0, 1.0, 0.5], F32), pose)
    assert p.shape == (6, 3) and o.tolist() == [[1.0, 2.0, 3.0]] and i.tolist() == [0] * 6 and i.dtype == torch.int32
    assert torch.isnan(p[2]).all() and p[3].tolist() == [1.0 - 0.25, 2.0 + 0.0625, 3.5]
    assert p[1].tolist() == [1.0, 2.0 - 0.25, 5.0]
