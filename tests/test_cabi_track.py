"""The tracking entry points (sgnn_amd.track, csrc/track.hip) are declared, exported by the built library and bound
with the header's argument counts; the pair record has the header's size.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_track_halve', 'sgnn_track_normals', 'sgnn_track_system']


def test_track_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_track_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
    record = re.search(r'typedef struct sgnn_track_pair \{(.*?)\}', src, flags=re.S).group(1)
    floats = sum(int(n) for n in re.findall(r'float \w+\[(\d+)\]', record))
    assert floats * 4 == 96


def test_track_pair_dtype():
    import numpy as np
    from sgnn_amd import track
    assert track.PAIR_DTYPE.itemsize == 96 and track.PAIR_DTYPE.names == ('t', 'intr_live', 'intr_model', 'pad')
    bad = np.eye(4)
    bad[0, 3] = np.inf
    table = track.pair_table(np.ones(4, np.float32), np.ones((2, 4), np.float32), np.stack([np.eye(4), bad]))
    assert np.array_equal(table['t'][0], np.eye(4, dtype=np.float32)[:3].ravel()) and np.isnan(table['t'][1]).all()
