"""The mesh-fairing entry points (sgnn_amd.smooth, csrc/smooth.hip) are declared, exported by the built library and
bound with the header's argument counts; the public calls check their arguments before they need a device and need
one after.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_smooth_'
NAMES = ['sgnn_smooth_classify', 'sgnn_smooth_corners', 'sgnn_smooth_face_normals', 'sgnn_smooth_filter',
         'sgnn_smooth_keys', 'sgnn_smooth_run_flags', 'sgnn_smooth_runs', 'sgnn_smooth_step', 'sgnn_smooth_update',
         'sgnn_smooth_vertex_normals']


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


def test_the_unit_is_built_without_contraction():
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'smooth.hip' in srcs
    assert re.search(r'^\.\./lib/smooth\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off\s*$', mk, flags=re.M)
    assert re.search(r'^#.*tests/smooth_ref\.py.*\n\.\./lib/smooth\.o:', mk, flags=re.M)


def _mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=np.int32)
    return verts, faces


def test_every_public_call_needs_a_device(monkeypatch):
    from sgnn_amd import _lib, smooth
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    verts, faces = _mesh()
    for call in (lambda: smooth.Adjacency(faces, 4),
                 lambda: smooth.laplacian(verts, faces),
                 lambda: smooth.taubin(torch.from_numpy(verts), torch.from_numpy(faces), fixed=np.zeros(4, bool)),
                 lambda: smooth.face_normals(verts, faces),
                 lambda: smooth.vertex_normals(verts, faces),
                 lambda: smooth.denoise(verts, faces),
                 lambda: smooth.laplacian(verts, faces, iterations=0),
                 lambda: smooth.denoise(verts[:0], faces[:0])):
        with pytest.raises(_lib.SgnnError):
            call()


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import smooth
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    verts, faces = _mesh()
    for bad_verts in (verts[:, :2], verts.reshape(-1), np.zeros((4, 4), np.float32), np.zeros((2, 2, 3), np.float32)):
        for call in (smooth.laplacian, smooth.taubin, smooth.face_normals, smooth.vertex_normals, smooth.denoise):
            with pytest.raises(ValueError):
                call(bad_verts, faces)
    for bad_faces in (faces[:, :2], faces.reshape(-1), np.zeros((4, 4), np.int32)):
        for call in (smooth.laplacian, smooth.taubin, smooth.face_normals, smooth.vertex_normals, smooth.denoise):
            with pytest.raises(ValueError):
                call(verts, bad_faces)
        with pytest.raises(ValueError):
            smooth.Adjacency(bad_faces, 4)
    with pytest.raises(ValueError):
        smooth.Adjacency(faces, -1)
    for call in (smooth.laplacian, smooth.taubin):
        with pytest.raises(ValueError):
            call(verts, faces, boundary='pinned')
        with pytest.raises(ValueError):
            call(verts, faces, iterations=-1)
        with pytest.raises(ValueError):
            call(verts, faces, lam=float('nan'))
        with pytest.raises(ValueError):
            call(verts, faces, fixed=np.zeros(5, bool))
        with pytest.raises(ValueError):
            call(verts, faces, fixed=np.zeros((4, 1), bool))
    with pytest.raises(ValueError):
        smooth.taubin(verts, faces, mu=float('inf'))
    with pytest.raises(ValueError):
        smooth.denoise(verts, faces, normal_iterations=-1)
    with pytest.raises(ValueError):
        smooth.denoise(verts, faces, vertex_iterations=-2)
    with pytest.raises(ValueError):
        smooth.denoise(verts, faces, threshold=float('nan'))
    with pytest.raises(ValueError):
        smooth.denoise(verts, faces, fixed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        smooth.denoise(verts, faces, adj=faces)


def test_the_kinds_and_modes_are_the_numbers_of_the_header():
    from sgnn_amd import smooth
    assert (smooth.ISOLATED, smooth.INTERIOR, smooth.BOUNDARY, smooth.NONMANIFOLD) == (0, 1, 2, 3)
    assert smooth.BOUNDARIES == ('fixed', 'curve', 'free') and smooth.ROW_FLOATS == 3
