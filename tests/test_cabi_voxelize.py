"""The mesh voxelisation entry points (sgnn_amd.voxelize, csrc/voxelize.hip) are declared, exported by the built
library and bound with the header's argument counts; without a device the module raises.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_vox_grid_coords', 'sgnn_vox_bricks_count', 'sgnn_vox_bricks_fill', 'sgnn_vox_normals', 'sgnn_vox_nearest',
         'sgnn_vox_tsdf']


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_voxelize_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_voxelize_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    declared = sorted(set(re.findall(r'\b(sgnn_vox_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(n for n in _lib.PROTOTYPES if n.startswith('sgnn_vox_'))
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name


def test_the_batch_constant_is_the_headers():
    from sgnn_amd import voxelize
    assert voxelize.FACE_BATCH == int(re.search(r'^#define SGNN_VOX_BATCH (\d+)$', _header(), flags=re.M).group(1))


def test_the_object_is_built_without_contraction():
    """The bit-for-bit comparison with meshdist and with tests/voxelize_ref.py rests on it."""
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bvoxelize\.hip\b', mk, flags=re.M)
    assert re.search(r'^\.\./lib/voxelize\.o: CXXFLAGS \+= -ffp-contract=off$', mk, flags=re.M)
    # the point-triangle routine is shared through a header, not copied
    csrc = os.path.join(ROOT, 'sgnn_amd', 'csrc')
    for name in ('meshdist.hip', 'voxelize.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "tri_dist.h"' in text and 'tri_residual(const' not in text, name


def test_voxelize_needs_a_device(monkeypatch):
    import numpy as np
    import pytest
    import torch
    from sgnn_amd import _lib, voxelize
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    verts = np.array([[1, 1, 1], [5, 1, 1], [1, 5, 2]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(_lib.SgnnError):
        voxelize.signed_distance(verts, faces, (8, 8, 8), 3.0)
    with pytest.raises(_lib.SgnnError):
        voxelize.mesh_to_volume(torch.from_numpy(verts), torch.from_numpy(faces), (8, 8, 8), 0.02, np.eye(4), band=3.0)
    with pytest.raises(_lib.SgnnError):
        voxelize.mesh_to_pyramid(verts, faces, (8, 8, 8), 0.02, np.eye(4), levels=2, flip=True)
