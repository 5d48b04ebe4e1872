"""The connected-component entry points (sgnn_amd.components, csrc/components.hip) are declared, exported by the
built library and bound with the header's argument counts; the tile of the header is the tile of the module.
No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_cc_volume_link', 'sgnn_cc_mesh_link', 'sgnn_cc_flatten', 'sgnn_cc_relabel', 'sgnn_cc_face_labels']


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_component_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_component_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    declared = sorted(set(re.findall(r'\b(sgnn_cc_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(n for n in _lib.PROTOTYPES if n.startswith('sgnn_cc_'))
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name


def test_tile_of_the_header_is_the_tile_of_the_module():
    from sgnn_amd import components
    src = _header()
    tile = tuple(int(re.search(r'#define SGNN_CC_TILE_%s (\d+)' % a, src).group(1)) for a in 'ZYX')
    assert tile == components.TILE_ZYX
    assert tile[1] * tile[2] == 256          # one z slice of a tile per 256-thread workgroup (csrc/components.hip)


def test_components_need_a_device():
    import pytest
    import torch
    from sgnn_amd import _lib, components
    with pytest.raises(_lib.SgnnError):
        components.label_volume(torch.zeros(2, 2, 2, dtype=torch.uint8))
    with pytest.raises(_lib.SgnnError):
        components.label_mesh(3, torch.zeros(1, 3, dtype=torch.int32))
