"""The mesh-simplification entry points (sgnn_amd.simplify, csrc/simplify.hip) are declared, exported by the built
library and bound with the header's argument counts; without a device the module raises.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_simp_keys', 'sgnn_simp_clusters', 'sgnn_simp_corners', 'sgnn_simp_mark', 'sgnn_simp_place']


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_simplify_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_simplify_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    declared = sorted(set(re.findall(r'\b(sgnn_simp_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(n for n in _lib.PROTOTYPES if n.startswith('sgnn_simp_'))
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name


def test_the_object_is_built_without_contraction():
    """The bit-for-bit comparison with tests/simplify_ref.py rests on it."""
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bsimplify\.hip\b', mk, flags=re.M)
    assert re.search(r'^\.\./lib/simplify\.o: CXXFLAGS \+= -ffp-contract=off$', mk, flags=re.M)


def test_simplify_needs_a_device(monkeypatch):
    import numpy as np
    import pytest
    import torch
    from sgnn_amd import _lib, simplify
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    verts = np.zeros((3, 3), np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(_lib.SgnnError):
        simplify.cluster(verts, faces, cell=0.06)
    with pytest.raises(_lib.SgnnError):
        simplify.cluster(torch.from_numpy(verts), torch.from_numpy(faces), cell=0.06, placement='mean')
    with pytest.raises(_lib.SgnnError):
        simplify.cell_for_faces(verts, faces, 1)
