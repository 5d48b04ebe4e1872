"""The point-cloud entry points (sgnn_amd.cloud, csrc/cloud.hip) are declared, exported by the built library and bound
with the header's argument counts; the public calls check their arguments before they need a device and need one
after.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_cloud_'
NAMES = ['sgnn_cloud_keys', 'sgnn_cloud_knn', 'sgnn_cloud_mean_dist', 'sgnn_cloud_normals', 'sgnn_cloud_pack',
         'sgnn_cloud_radius_count', 'sgnn_cloud_radius_fill', 'sgnn_cloud_run_flags', 'sgnn_cloud_voxel_keys',
         'sgnn_cloud_voxel_reduce']


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


def test_the_header_declares_the_passes():
    assert _declared() == NAMES


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
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name
        for param, arg in zip(params, args):      # pointers, 64-bit counts, ints and floats sit where the header has them
            kind = (_lib.c_vp if '*' in param else _lib.c_i64 if 'int64_t' in param else _lib.c_f32 if 'float' in param
                    else _lib.c_vp if 'sgnn_stream_t' in param else _lib.c_i32)
            assert arg is kind, (name, param)


def test_the_unit_is_built_without_contraction():
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'cloud.hip' in srcs
    assert re.search(r'^\.\./lib/cloud\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off\s*$', mk, flags=re.M)
    assert re.search(r'^#.*tests/cloud_ref\.py.*\n\.\./lib/cloud\.o:', mk, flags=re.M)


def test_the_module_is_exported_like_the_other_tools():
    import sgnn_amd
    assert sgnn_amd.cloud.PointIndex is not None and 'cloud.py' in sgnn_amd.__doc__


def _cloud():
    rng = np.random.default_rng(0)
    return rng.uniform(0, 1, (12, 3)).astype(np.float32)


def test_every_public_call_needs_a_device(monkeypatch):
    from sgnn_amd import _lib, cloud
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    pts = _cloud()
    colors = np.zeros((12, 3), np.uint8)
    for call in (lambda: cloud.PointIndex(pts),
                 lambda: cloud.PointIndex(torch.from_numpy(pts), cell=0.5),
                 lambda: cloud.PointIndex(pts[:0]),
                 lambda: cloud.normals(pts),
                 lambda: cloud.normals(pts, k=4, max_dist=0.5, toward=np.zeros(3, np.float32)),
                 lambda: cloud.statistical_outliers(pts),
                 lambda: cloud.radius_outliers(pts, 0.5, 2),
                 lambda: cloud.voxel_downsample(pts, 0.25),
                 lambda: cloud.voxel_downsample(pts, 0.25, colors=colors, normals=pts),
                 lambda: cloud.voxel_downsample(pts[:0], 0.25),
                 lambda: cloud.compare(pts, pts),
                 lambda: cloud.compare(pts[:0], pts, max_dist=1.0)):
        with pytest.raises(_lib.SgnnError):
            call()


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import cloud
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    pts = _cloud()
    for bad in (pts[:, :2], pts.reshape(-1), np.zeros((4, 4), np.float32), np.zeros((2, 2, 3), np.float32)):
        for call in (cloud.PointIndex, cloud.normals, cloud.statistical_outliers,
                     lambda p: cloud.radius_outliers(p, 0.5, 1), lambda p: cloud.voxel_downsample(p, 0.5),
                     lambda p: cloud.compare(p, pts), lambda p: cloud.compare(pts, p)):
            with pytest.raises(ValueError):
                call(bad)
    for cell in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            cloud.PointIndex(pts, cell=cell)
        with pytest.raises(ValueError):
            cloud.voxel_downsample(pts, cell)
        with pytest.raises(ValueError):
            cloud.radius_outliers(pts, cell, 1)
    for k in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError):
            cloud.normals(pts, k=k)
        with pytest.raises(ValueError):
            cloud.statistical_outliers(pts, k=k)
    for md in (-1.0, float('nan')):
        with pytest.raises(ValueError):
            cloud.normals(pts, max_dist=md)
        with pytest.raises(ValueError):
            cloud.compare(pts, pts, max_dist=md)
    for toward in (np.zeros(2, np.float32), np.zeros((11, 3), np.float32), np.zeros((12, 2), np.float32),
                   np.zeros((1, 3), np.float32)):
        with pytest.raises(ValueError):
            cloud.normals(pts, toward=toward)
    for ratio in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            cloud.statistical_outliers(pts, std_ratio=ratio)
    for m in (-1, 1.5):
        with pytest.raises(ValueError):
            cloud.radius_outliers(pts, 0.5, m)
    with pytest.raises(ValueError):
        cloud.voxel_downsample(pts, 0.5, colors=np.zeros((12, 3), np.float32))
    with pytest.raises(ValueError):
        cloud.voxel_downsample(pts, 0.5, colors=torch.zeros((12, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        cloud.voxel_downsample(pts, 0.5, colors=np.zeros((11, 3), np.uint8))
    with pytest.raises(ValueError):
        cloud.voxel_downsample(pts, 0.5, colors=np.zeros((12, 2), np.uint8))
    with pytest.raises(ValueError):
        cloud.voxel_downsample(pts, 0.5, normals=np.zeros((11, 3), np.float32))

    class Other(cloud.PointIndex):
        def __init__(self, n):
            self.n = n

    for call in (cloud.normals, cloud.statistical_outliers, lambda p, index: cloud.radius_outliers(p, 0.5, 1, index=index)):
        with pytest.raises(ValueError):
            call(pts, index=Other(11))
        with pytest.raises(ValueError):
            call(pts, index='index')


def test_query_arguments_are_checked_before_the_library_is_called(monkeypatch):
    from sgnn_amd import _lib, cloud
    index = cloud.PointIndex.__new__(cloud.PointIndex)      # no device: the checks come before anything is touched
    index.n = index.nfin = 12
    monkeypatch.setattr(_lib, 'call', lambda *a: pytest.fail('the library was called'))
    pts = _cloud()
    for k in (0, 33, 1.5):
        with pytest.raises(ValueError):
            index.knn(pts, k)
        with pytest.raises(ValueError):
            index.knn(None, k)
    for bad in (pts[:, :2], pts.reshape(-1)):
        with pytest.raises(ValueError):
            index.knn(bad, 3)
        with pytest.raises(ValueError):
            index.nearest(bad)
        with pytest.raises(ValueError):
            index.radius_count(bad, 0.5)
        with pytest.raises(ValueError):
            index.radius(bad, 0.5)
    for md in (-0.5, float('nan')):
        with pytest.raises(ValueError):
            index.knn(pts, 3, max_dist=md)
        with pytest.raises(ValueError):
            index.nearest(pts, max_dist=md)
        with pytest.raises(ValueError):
            index.radius_count(pts, md)
        with pytest.raises(ValueError):
            index.radius(pts, md)


def test_the_limits_are_those_of_the_kernels():
    from sgnn_amd import cloud
    src = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'cloud.hip')).read()
    assert cloud.MAX_CELLS_AXIS == int(re.search(r'MAX_AXIS = (\d+);', src).group(1)) == 1024
    assert cloud.VOXEL_LIMIT == 2 ** 20 and 'VOXEL_LIMIT = 1 << 20;' in src
    assert cloud.MAX_K == 32 and cloud.max_cells(100) == 264
    lo, hi = np.zeros(3, np.float32), np.array([100, 1, 1], np.float32)
    cell, dims = cloud.fit_cell(np.float32(1e-3), lo, hi, 1000)      # enlarged: at most 1024 an axis, 2 n + 64 in all
    assert max(dims) <= 1024 and dims[0] * dims[1] * dims[2] <= cloud.max_cells(1000)
    assert float(cell) / float(np.float32(1e-3)) == 512.0      # doubled, exactly
    assert cloud.fit_cell(np.float32(0.5), lo, hi, 1000) == (np.float32(0.5), (201, 3, 3))
    assert cloud.default_cell(lo, lo, 5) == 1 and cloud.default_cell(lo, hi, 0) > 0
