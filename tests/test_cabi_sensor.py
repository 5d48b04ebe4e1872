"""The sensor entry points (sgnn_amd.sensor, csrc/sensor.hip) are declared, exported by the built library and bound
with the header's argument counts; the model record has the header's size, fields and offsets.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_sensor_shadow', 'sgnn_sensor_degrade']


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_sensor_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_sensor_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = header()
    kinds = {'int': _lib.c_i32, 'float': _lib.c_f32, 'uint64_t': _lib.c_u64, 'sgnn_stream_t': _lib.c_vp}
    for name in NAMES:
        params = [p.strip() for p in re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')]
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        for param, arg in zip(params, args):
            want = _lib.c_vp if '*' in param else kinds[param.rsplit(' ', 1)[0]]
            assert arg is want, (name, param)


def test_sensor_model_dtype():
    from sgnn_amd import sensor
    record = re.search(r'typedef struct sgnn_sensor_model \{(.*?)\}', header(), flags=re.S).group(1)
    fields = re.findall(r'float (\w+);', record)
    assert len(fields) * 4 == sensor.MODEL_DTYPE.itemsize == 48
    assert tuple(fields) == sensor.MODEL_DTYPE.names == sensor.SensorModel._fields
    assert [sensor.MODEL_DTYPE.fields[name][1] for name in fields] == list(range(0, 48, 4))
    assert all(sensor.MODEL_DTYPE[name].shape == () and sensor.MODEL_DTYPE[name].str == '<f4' for name in fields)


def test_the_library_checks_the_model_before_it_touches_the_device():
    """Argument errors are the library's usual codes, and an empty call launches nothing: both without a GPU."""
    import numpy as np
    from sgnn_amd import _lib, sensor
    lib = _lib.load()
    ok = sensor.SensorModel().record()
    before = lib.sgnn_launch_count()
    assert lib.sgnn_sensor_degrade(None, None, 0, 4, 4, None, None, ok.ctypes.data, 0, None, None) == 0
    assert lib.sgnn_sensor_degrade(None, None, 3, 0, 4, None, None, ok.ctypes.data, 0, None, None) == 0
    assert lib.sgnn_sensor_shadow(None, 2, 4, 0, None, 0.075, None, None) == 0
    einval = -1
    assert lib.sgnn_sensor_degrade(None, None, 1, 4, 4, None, None, ok.ctypes.data, 0, None, None) == einval   # NULL frames
    assert lib.sgnn_sensor_degrade(None, None, 0, 4, 4, None, None, None, 0, None, None) == einval             # no model
    assert lib.sgnn_sensor_degrade(None, None, -1, 4, 4, None, None, ok.ctypes.data, 0, None, None) == einval
    assert lib.sgnn_sensor_degrade(None, None, 1 << 15, 1 << 8, 1 << 8, None, None, ok.ctypes.data, 0, None, None) == einval
    assert lib.sgnn_sensor_shadow(None, 1, 4, 4, None, 0.075, None, None) == einval
    assert lib.sgnn_sensor_shadow(None, 0, 4, 4, None, float('inf'), None, None) == einval
    for field, value in (('lateral_sigma', -1.0), ('min_depth', 7.0), ('baseline', np.inf), ('cos_min', 1.5),
                         ('edge_drop', -0.5), ('drop', np.nan), ('a0', np.inf), ('disparity_quantum', -0.125)):
        bad = ok.copy()
        bad[field] = value
        assert lib.sgnn_sensor_degrade(None, None, 0, 4, 4, None, None, bad.ctypes.data, 0, None, None) == einval, field
        assert field in lib.sgnn_last_error().decode()
    assert lib.sgnn_launch_count() == before
