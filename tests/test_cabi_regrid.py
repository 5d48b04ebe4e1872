"""The regrid entry points (sgnn_amd.regrid, csrc/regrid.hip) are declared, exported by the built library and bound
with the header's argument counts; the unit is built with its contract line; the public calls check their arguments
before they need a device and need one after; grid_for runs on the host.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_regrid_'
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


def test_the_header_declares_the_store_and_the_fold():
    assert _declared() == ['sgnn_regrid_merge', 'sgnn_regrid_resample']


def test_declared_names_are_the_exported_names():
    from sgnn_amd import _lib
    lib = _library()
    declared = _declared()
    assert [n for n in declared if not hasattr(lib, n)] == []
    # a symbol's name is a NUL-terminated string of the library's string tables, so every name under the prefix that
    # the file holds must be a declared one (kernels are mangled and do not begin with it)
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


def test_the_unit_is_built_with_its_contract_line():
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'regrid.hip' in srcs
    assert re.search(r'^#.*tests/regrid_ref\.py.*\n\.\./lib/regrid\.o:\s*CXXFLAGS \+= -ffp-contract=off$', mk, flags=re.M)


def _stub(dims=(8, 7, 6), color=False, world2grid=None, device=None, voxel_size=0.05):
    """A TSDFVolume without its device arrays: what the argument checks look at."""
    from sgnn_amd import fusion
    v = fusion.TSDFVolume.__new__(fusion.TSDFVolume)
    v.device, v.dims_xyz, v.voxel_size = device, tuple(dims), F32(voxel_size)
    v.world2grid = np.eye(4, dtype=F32) if world2grid is None else np.asarray(world2grid, F32)
    v.depth_min, v.depth_max, v.obb, v._color = F32(0.4), F32(4.0), None, (object() if color else None)
    return v


def _yaw(deg=30.0):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0, 0.5], [s, c, 0, -1.0], [0, 0, 1, 0.25], [0, 0, 0, 1]])


def test_valid_calls_need_a_device(monkeypatch):
    from sgnn_amd import _lib, fusion, regrid
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.SgnnError):
        regrid.resample(_stub(), (9, 9, 9), _yaw())
    with pytest.raises(_lib.SgnnError):
        regrid.resample(_stub(color=True), (1, 1, 1), np.eye(4), voxel_size=0.1, mode='nearest', skip=False)
    with pytest.raises(_lib.SgnnError):
        regrid.merge(_stub(), _stub(color=True, world2grid=_yaw()), mode='nearest')
    pyr = fusion.TSDFPyramid.__new__(fusion.TSDFPyramid)
    pyr.volumes = [_stub(), _stub((4, 4, 3))]
    with pytest.raises(_lib.SgnnError):
        regrid.resample_pyramid(pyr, (9, 9, 9), _yaw())


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import regrid
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    nan, sing = np.eye(4), np.eye(4)
    nan[1, 2] = np.nan
    sing[2, 2] = 0.0
    huge = np.eye(4)
    huge[:3, :3] *= 1e-40                                       # invertible, but the map overflows fp32
    vol = _stub()
    bad = [
        dict(dims_xyz=(9, 9, 9), world2grid=nan),                               # non-finite matrices
        dict(dims_xyz=(9, 9, 9), world2grid=np.full((4, 4), np.inf)),
        dict(dims_xyz=(9, 9, 9), world2grid=sing),                              # singular destination
        dict(dims_xyz=(9, 9, 9), world2grid=np.zeros((4, 4))),
        dict(dims_xyz=(9, 9, 9), world2grid=huge),                              # a non-finite A
        dict(dims_xyz=(0, 9, 9), world2grid=np.eye(4)),                         # dims outside TSDFVolume's limits
        dict(dims_xyz=(65536, 1, 1), world2grid=np.eye(4)),
        dict(dims_xyz=(2048, 1024, 1024), world2grid=np.eye(4)),
        dict(dims_xyz=(9, 9), world2grid=np.eye(4)),
        dict(dims_xyz=(9, 9, 9), world2grid=np.eye(4), mode='cubic'),           # mode
        dict(dims_xyz=(9, 9, 9), world2grid=np.eye(4), voxel_size=0.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            regrid.resample(vol, **kw)
    with pytest.raises(ValueError):
        regrid.resample(_stub(world2grid=nan), (9, 9, 9), np.eye(4))
    with pytest.raises(ValueError):
        regrid.merge(vol, vol)                                                  # dst is src
    with pytest.raises(ValueError):
        regrid.merge(vol, _stub(), mode='cubic')
    with pytest.raises(ValueError):
        regrid.merge(_stub(world2grid=sing), _stub())
    with pytest.raises(ValueError):
        regrid.merge(_stub(device=torch.device('cuda', 0)), _stub(device=torch.device('cuda', 1)))
    from sgnn_amd import fusion
    pyr = fusion.TSDFPyramid.__new__(fusion.TSDFPyramid)
    pyr.volumes = [_stub(), _stub((4, 4, 3))]
    for args in (((9, 9, 9), sing), ((0, 1, 1), np.eye(4)), ((9, 9, 9), nan)):
        with pytest.raises(ValueError):
            regrid.resample_pyramid(pyr, *args)


def test_grid_for_runs_on_the_host_and_holds_the_moved_volume():
    from sgnn_amd import regrid
    w2g = np.eye(4)
    w2g[:3, :3] *= 16.0                                          # 6.25 cm voxels: every figure below is exact
    w2g[:3, 3] = (4.0, -2.0, 1.0)
    vol = _stub((24, 20, 16), world2grid=w2g, voxel_size=0.0625)
    dims, m = regrid.grid_for(vol)
    assert dims == (24, 20, 16) and m.dtype == np.float32 and np.array_equal(m, w2g.astype(F32))
    dims, m = regrid.grid_for(vol, pad=3)
    assert dims == (30, 26, 22) and np.array_equal(m[:3, 3], w2g[:3, 3].astype(F32) + 3)
    dims2, m2 = regrid.grid_for(vol, voxel_size=0.125)
    assert dims2 == (13, 11, 9)                                  # 23 / 2 -> floor and ceil: 0 .. 12
    t = _yaw()
    dims, m = regrid.grid_for(vol, t, pad=1)
    # every corner of the source grid, moved, lies at least `pad` voxels inside the box, and the box is tight
    g2w = np.linalg.inv(w2g)
    hi = np.array(vol.dims_xyz) - 1.0
    corners = np.array([[(c >> a & 1) * hi[a] for a in range(3)] + [1.0] for c in range(8)])
    g = (corners @ g2w.T @ m.astype(np.float64).T)[:, :3]
    assert g.min() >= 1 - 1e-4 and (g.max(0) <= np.array(dims) - 2 + 1e-4).all()
    assert (g.min(0) < 2 + 1e-4).all() and (g.max(0) > np.array(dims) - 3 - 1e-4).all()
    # the matrix takes the original world to the new grid: box . T, so resampling reads the volume where it was
    assert np.allclose(m[:3, :3], t[:3, :3] * 16.0, rtol=1e-6)
    for kw in (dict(voxel_size=0.0), dict(pad=-1), dict(world_transform=np.full((4, 4), np.nan))):
        with pytest.raises(ValueError):
            regrid.grid_for(vol, **kw)
