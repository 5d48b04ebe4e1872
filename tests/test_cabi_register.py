"""The registration entry point (sgnn_amd.register, csrc/register.hip) is declared, exported by the built library and
bound with the header's argument count; the record has the header's size and fields.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_register_system']


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_register_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_register_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = header()
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name


def test_register_pair_dtype():
    from sgnn_amd import register
    record = re.search(r'typedef struct sgnn_register_pair \{(.*?)\}', header(), flags=re.S).group(1)
    fields = re.findall(r'float (\w+)\[(\d+)\]', record)
    assert sum(int(n) for _, n in fields) * 4 == register.PAIR_DTYPE.itemsize == 96
    assert tuple(name for name, _ in fields) == register.PAIR_DTYPE.names == ('t', 'w')
    assert [register.PAIR_DTYPE[name].shape for name in register.PAIR_DTYPE.names] == [(int(n),) for _, n in fields]
    assert int(re.search(r'#define SGNN_REGISTER_MAX_BLOCKS (\d+)', header()).group(1)) == register.MAX_BLOCKS


def test_a_non_finite_transform_is_a_nan_record():
    from sgnn_amd import register
    w2g = np.diag([20.0, 20.0, 20.0, 1.0])
    bad, big = np.eye(4), np.eye(4)
    bad[0, 3] = np.inf
    big[2, 3] = 1e300                                                       # finite in fp64, not in fp32
    table = register.pair_table(w2g, np.stack([np.eye(4), bad, big]))
    assert np.array_equal(table['t'][0], np.eye(4, dtype=np.float32)[:3].ravel())
    assert np.isnan(table['t'][1]).all() and np.isnan(table['t'][2]).all()
    assert all(np.array_equal(w, w2g[:3].astype(np.float32).ravel()) for w in table['w'])
    w2g[1, 1] = np.nan                                                      # a non-finite world2grid empties every record
    assert np.isnan(register.pair_table(w2g, np.eye(4)[None])['t']).all()
