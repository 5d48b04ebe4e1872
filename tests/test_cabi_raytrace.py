"""The ray-tracing entry points (sgnn_amd.raytrace, csrc/raytrace.hip) are declared, exported by the built library and
bound with the header's argument types; argument errors are the library's usual code and launch nothing.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_raytrace_closest', 'sgnn_raytrace_occluded']
EINVAL = -1


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def test_raytrace_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_raytrace_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = header()
    kinds = {'int': _lib.c_i32, 'float': _lib.c_f32, 'int64_t': _lib.c_i64, 'sgnn_stream_t': _lib.c_vp}
    for name in NAMES:
        params = [p.strip() for p in re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')]
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].startswith('sgnn_stream_t')
        for param, arg in zip(params, args):
            want = _lib.c_vp if '*' in param else kinds[param.rsplit(' ', 1)[0]]
            assert arg is want, (name, param)


# argument positions of the two entry points (include/sgnn_hip.h)
CLOSEST = ['origins', 'dirs', 'nrays', 't_min', 't_max', 'records', 'offsets', 'refs', 'lox', 'loy', 'loz', 'cell', 'nx',
           'ny', 'nz', 'guard', 'cull_back', 't', 'face', 'uv', 'counters', 'stream']
OCCLUDED = ['origins', 'dirs', 'nrays', 't_min', 't_max', 'records', 'offsets', 'refs', 'lox', 'loy', 'loz', 'cell', 'nx',
            'ny', 'nz', 'guard', 'cull_back', 'hit', 'counters', 'stream']


def test_the_library_checks_its_arguments_before_it_touches_the_device():
    """Every argument error returns SGNN_EINVAL and an empty call returns 0, both without a launch and without a GPU.
    The pointers below are host addresses that a call which got as far as a launch would hand to a kernel; none does."""
    import numpy as np
    from sgnn_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16               # 16-byte aligned, never dereferenced
    inf, nan = float('inf'), float('nan')
    good = dict(origins=p, dirs=p, nrays=5, t_min=0.0, records=p, offsets=p, refs=p, lox=0.0, loy=0.0, loz=0.0,
                cell=0.5, nx=4, ny=4, nz=4, guard=0.5 / 64, cull_back=0, counters=None, stream=None)
    cases = {'sgnn_raytrace_closest': (CLOSEST, dict(good, t_max=inf, t=p, face=p, uv=p)),
             'sgnn_raytrace_occluded': (OCCLUDED, dict(good, t_max=p, hit=p))}
    before = lib.sgnn_launch_count()
    for name, (order, args) in cases.items():
        fn = getattr(lib, name)

        def call(**change):
            return fn(*[dict(args, **change)[k] for k in order])

        assert call(nrays=0) == 0, name
        assert call(nrays=0, origins=None, dirs=None, records=None, offsets=None, refs=None) == 0, name
        pointers = [k for k in order if args[k] == p]
        assert len(pointers) == (8 if name.endswith('closest') else 7)
        for k in pointers:                                        # NULL with R > 0
            assert call(**{k: None}) == EINVAL, (name, k)
            assert name in lib.sgnn_last_error().decode()
        assert call(records=p + 4) == EINVAL, name                # records not 16-byte aligned
        bad = [dict(nrays=-1), dict(nx=0), dict(ny=-3), dict(nz=0), dict(nx=1 << 11, ny=1 << 11, nz=1 << 11),
               dict(cell=0.0), dict(cell=-1.0), dict(cell=inf), dict(cell=nan), dict(lox=nan), dict(loy=inf),
               dict(loz=-inf), dict(guard=-0.1), dict(guard=nan), dict(guard=inf), dict(t_min=nan), dict(t_min=-inf),
               dict(cull_back=2), dict(cull_back=-1)]
        if name.endswith('closest'):
            bad += [dict(t_min=1.0, t_max=1.0), dict(t_min=2.0, t_max=1.0), dict(t_max=nan)]
        for change in bad:
            assert call(**change) == EINVAL, (name, change)
            assert call(nrays=0, **{k: v for k, v in change.items() if k != 'nrays'}) == (0 if 'nrays' in change else EINVAL)
    assert lib.sgnn_launch_count() == before
