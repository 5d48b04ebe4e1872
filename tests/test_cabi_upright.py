"""The upright entry points (sgnn_amd.upright, csrc/upright.hip) are declared, exported by the built library and bound
with the header's argument counts; the axis record has the header's size and fields.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_upright_histogram', 'sgnn_upright_sums', 'sgnn_upright_heights']


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_upright_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_upright_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = header()
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert args[0] is _lib.c_vp and args[1:4] == [_lib.c_i32] * 3 and args[-1] is _lib.c_vp, name


def test_upright_axis_dtype():
    from sgnn_amd import upright
    record = re.search(r'typedef struct sgnn_upright_axis \{(.*?)\}', header(), flags=re.S).group(1)
    fields = [(name, int(n) if n else None) for name, n in re.findall(r'float (\w+)(?:\[(\d+)\])?;', record)]
    assert sum(n or 1 for _, n in fields) * 4 == upright.AXIS_DTYPE.itemsize == 48
    assert tuple(name for name, _ in fields) == upright.AXIS_DTYPE.names == ('u', 'e1', 'e2', 'cos_cone', 'sin_wall', 'pad')
    assert [upright.AXIS_DTYPE[name].shape for name, _ in fields] == [() if n is None else (n,) for _, n in fields]
    assert [upright.AXIS_DTYPE.fields[name][1] for name, _ in fields] == [0, 12, 24, 36, 40, 44]
    assert int(re.search(r'#define SGNN_UPRIGHT_MAX_HEIGHT_BINS (\d+)', header()).group(1)) == upright.MAX_HEIGHT_BINS


def test_a_non_finite_axis_is_a_nan_record():
    from sgnn_amd import upright
    z, x, y = np.eye(3)[2], np.eye(3)[0], np.eye(3)[1]
    u = np.stack([z, z, z, z])
    e1 = np.stack([x, x, x, x])
    u[1, 0] = np.inf
    e1[2, 1] = 1e300                                                        # finite in fp64, not in fp32
    table = upright.axis_table(u, e1, np.stack([y] * 4), [0.9, 0.9, 0.9, np.nan], -1.0)
    assert table.dtype == upright.AXIS_DTYPE and table.shape == (4,)
    assert np.array_equal(table['u'][0], z.astype(np.float32)) and np.array_equal(table['e2'][0], y.astype(np.float32))
    assert table['cos_cone'][0] == np.float32(0.9) and table['sin_wall'][0] == -1.0 and table['pad'][0] == 0
    for b in (1, 2, 3):
        assert all(np.isnan(table[name][b]).all() for name in ('u', 'e1', 'e2', 'cos_cone', 'sin_wall'))
    one = upright.axis_table(z, x, y, 1.5, 0.2)                             # a cone no normal can enter is still a record
    assert one.shape == (1,) and one['cos_cone'][0] == 1.5 and np.isfinite(one['u']).all()
