"""The colour entry points of TSDF fusion (sgnn_amd.fusion, csrc/fusion.hip) are declared,
exported by the built library and bound with the header's argument counts; without a device the module raises.
No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_fusecol_pack', 'sgnn_fusecol_integrate', 'sgnn_fusecol_export']


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_fusion_colour_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_fusion_colour_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    declared = sorted(set(re.findall(r'\b(sgnn_fusecol_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(n for n in _lib.PROTOTYPES if n.startswith('sgnn_fusecol_'))
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name
    # the depth-only entry point keeps its signature
    assert len(_lib.PROTOTYPES['sgnn_fuse_integrate'][1]) == 17
    assert len(_lib.PROTOTYPES['sgnn_fusecol_integrate'][1]) == 19


def test_one_integrate_kernel_built_without_contraction():
    csrc = os.path.join(ROOT, 'sgnn_amd', 'csrc')
    assert re.search(r'^\.\./lib/fusion\.o: CXXFLAGS \+= -ffp-contract=off$', open(os.path.join(csrc, 'Makefile')).read(),
                     flags=re.M)
    text = open(os.path.join(csrc, 'fusion.hip')).read()
    assert len(re.findall(r'__global__[^;{]*\bk_fuse_integrate\s*\(', text)) == 1        # one text, two instantiations
    assert 'k_fuse_integrate<true>' in text and 'k_fuse_integrate<false>' in text


def test_fusion_colour_needs_a_device(monkeypatch):
    import numpy as np
    import pytest
    import torch
    from sgnn_amd import _lib, fusion
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.SgnnError):
        fusion.pack_color(np.zeros((2, 8, 8, 3), np.uint8))
    with pytest.raises(_lib.SgnnError):
        fusion.pack_color(torch.zeros((8, 8, 4), dtype=torch.uint8), (4, 4))
    with pytest.raises(_lib.SgnnError):
        fusion.TSDFVolume((8, 8, 8), 0.05, np.eye(4), color=True)
    with pytest.raises(_lib.SgnnError):
        fusion.TSDFPyramid((8, 8, 8), 0.05, np.eye(4), levels=2, color=True)
