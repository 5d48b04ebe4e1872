"""The feature-transform entry points (sgnn_amd.edt, csrc/edt.hip) are declared, exported by the built library and
bound with the header's argument counts; the public calls check their arguments before they need a device and need
one after.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_edt_'


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
    assert {'sgnn_edt_rows', 'sgnn_edt_axis', 'sgnn_edt_fill'} <= set(_declared())


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


def test_the_unit_is_built_and_the_limit_of_the_header_is_the_limit_of_the_module():
    from sgnn_amd import edt
    mk = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'edt.hip' in srcs
    assert not re.search(r'edt\.o:\s*CXXFLAGS', mk)                  # integer work only: no -ffp-contract line
    assert int(re.search(r'#define SGNN_EDT_MAX_DIM (\d+)', _header()).group(1)) == edt.MAX_DIM == 1024


def test_edt_needs_a_device(monkeypatch):
    from sgnn_amd import _lib, edt
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    seeds = np.zeros((2, 3, 4), dtype=np.uint8)
    with pytest.raises(_lib.SgnnError):
        edt.feature_transform(seeds)
    with pytest.raises(_lib.SgnnError):
        edt.distance(torch.from_numpy(seeds), max_dist=2.0, voxel_size=0.05)
    with pytest.raises(_lib.SgnnError):
        edt.fill_colors(np.zeros((2, 3, 4, 3), dtype=np.uint8), seeds.astype(bool))
    with pytest.raises(_lib.SgnnError):
        edt.volume_colors(None)


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import edt
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for shape in ((1, 1, 1025), (1025, 1, 1), (1, 1025, 2)):
        with pytest.raises(ValueError):
            edt.feature_transform(np.zeros(shape, dtype=np.uint8))
        with pytest.raises(ValueError):
            edt.distance(np.zeros(shape, dtype=bool))
        with pytest.raises(ValueError):
            edt.fill_colors(np.zeros(shape + (3,), dtype=np.uint8), np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError):
        edt.feature_transform(np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        edt.feature_transform(np.zeros((2, 3, 4), dtype=np.uint8), max_dist=-1.0)
    with pytest.raises(ValueError):
        edt.fill_colors(np.zeros((2, 3, 4, 3), dtype=np.float32), np.zeros((2, 3, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        edt.fill_colors(np.zeros((2, 3, 5, 3), dtype=np.uint8), np.zeros((2, 3, 4), dtype=np.uint8))
