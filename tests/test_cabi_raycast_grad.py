"""The entry points of the differentiable cast (sgnn_amd.raycast.cast_diff, csrc/raycast.hip; INTEGRATION.md section
U) are declared, exported by the built library and bound with the header's argument counts; the recording cast is
k_raycast's text once more; the public calls check their arguments before they need a device and need one after.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = 'sgnn_raygrad_'
F32 = np.float32


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % PREFIX, _header())))


def _params(name):
    return [' '.join(p.split()) for p in re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, _header()).group(1).split(',')]


def test_the_header_declares_a_forward_and_a_gradient():
    assert _declared() == ['sgnn_raygrad_backward', 'sgnn_raygrad_cast']


def test_declared_names_are_the_exported_names():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in _declared() if not hasattr(lib, n)] == []
    data = open(_lib.LIB_PATH, 'rb').read()
    held = sorted(set(m.decode() for m in re.findall(rb'\0(%s[a-z0-9_]+)(?=\0)' % PREFIX.encode(), data)))
    assert held == _declared()


def test_prototypes_match_the_header():
    from sgnn_amd import _lib
    assert _declared() == sorted(n for n in _lib.PROTOTYPES if n.startswith(PREFIX))
    for name in _declared():
        params = _params(name)
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1] == 'sgnn_stream_t stream', name
        for p, a in zip(params, args):
            assert a is (_lib.c_vp if '*' in p or p.startswith('sgnn_stream_t') else
                         _lib.c_f32 if p.startswith('float') else _lib.c_i32), (name, p)
    # the forward takes the geometry of sgnn_raycast_cast, then its own arguments
    plain, diff = _params('sgnn_raycast_cast'), _params('sgnn_raygrad_cast')
    assert diff[:14] == plain[:14]
    assert diff[14:] == ['const float *features', 'int channels', 'float *depth', 'int32_t *hit', 'float *feat',
                         'uint8_t *ok', 'sgnn_stream_t stream']
    assert _params('sgnn_raygrad_backward')[-5:] == ['const float *grad_depth', 'const float *grad_feat',
                                                     'float *grad_sdf', 'float *grad_features', 'sgnn_stream_t stream']
    assert len(plain) == 18                                             # the cast keeps its signature


def test_one_walk_and_one_backward_kernel():
    text = open(os.path.join(ROOT, 'sgnn_amd', 'csrc', 'raycast.hip')).read()
    assert len(re.findall(r'__global__[^;{]*\bk_raycast\s*\(', text)) == 1
    assert re.search(r'template\s*<[^>]*\bbool DIFF\b[^>]*>\s*__global__[^;{]*\bk_raycast\s*\(', text)
    assert len(re.findall(r'__global__[^;{]*\bk_raycast_grad\s*\(', text)) == 1
    # floating-point atomics: the backward's scatter and nothing else in this unit
    body = text[text.index('void k_raycast_grad('):]
    body = body[:body.index('\n}\n')]
    assert len(re.findall(r'atomicAdd\(grad_', body)) == 3
    assert len(re.findall(r'atomicAdd\(', text)) == 3 + 2               # and the two sample counters (integers)


def _scene():
    sdf = np.zeros((6, 7, 8), F32)
    k, pose = np.array([[50.0, 50.0, 15.5, 11.5]], F32), np.eye(4)[None]
    return sdf, np.eye(4), 0.05, k, pose, (24, 32), 0.15


def test_arguments_are_checked_before_a_device_is_needed(monkeypatch):
    from sgnn_amd import raycast
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    sdf, w2g, vs, k, pose, hw, band = _scene()
    fe = np.zeros(sdf.shape + (3,), F32)
    for wrong in (fe[1:], fe[..., 0], fe.reshape(-1, 3), np.zeros(sdf.shape + (0,), F32),
                  np.zeros(sdf.shape + (17,), F32)):
        with pytest.raises(ValueError, match='features'):
            raycast.cast_diff(sdf, w2g, vs, k, pose, hw, band, features=wrong)
    bad = [dict(sdf=sdf[0]), dict(band=0.0), dict(step=0.0), dict(step=-0.5), dict(voxel_size=0.0),
           dict(depth_min=2.0, depth_max=1.0), dict(k=np.tile(k, (2, 1))), dict(hw=(0, 4)), dict(step=1e-6),
           dict(k=np.tile(k, (2, 1)), pose=np.tile(pose, (2, 1, 1)), hw=(1 << 15, 1 << 15))]
    for change in bad:
        a = dict(sdf=sdf, w2g=w2g, voxel_size=vs, k=k, pose=pose, hw=hw, band=band, step=0.5, depth_min=0.4,
                 depth_max=4.0)
        a.update(change)
        with pytest.raises(ValueError):
            raycast.cast_diff(a['sdf'], a['w2g'], a['voxel_size'], a['k'], a['pose'], a['hw'], a['band'], features=None,
                              step=a['step'], depth_min=a['depth_min'], depth_max=a['depth_max'])
    locs = np.stack(np.nonzero(np.ones(sdf.shape, bool)), 1)
    vals = sdf.reshape(-1)
    tail = (sdf.shape, w2g, vs, k, pose, hw, band)
    for a, b, kw in ((locs[:, :2], vals, {}), (locs, vals[1:], {}), (locs, vals, dict(features=np.zeros((3, 2), F32))),
                     (locs, vals, dict(features=np.zeros((len(vals), 17), F32))),
                     (locs, vals, dict(features=np.zeros(len(vals), F32))), (locs, vals, dict(step=-1.0)),
                     (locs, vals, dict(depth_min=3.0, depth_max=1.0))):
        with pytest.raises(ValueError):
            raycast.cast_sparse_diff(a, b, *tail, **kw)


def test_valid_calls_need_a_device(monkeypatch):
    from sgnn_amd import _lib, raycast
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    sdf, w2g, vs, k, pose, hw, band = _scene()
    with pytest.raises(_lib.SgnnError):
        raycast.cast_diff(sdf, w2g, vs, k, pose, hw, band)
    with pytest.raises(_lib.SgnnError):
        raycast.cast_diff(torch.zeros(sdf.shape, requires_grad=True), w2g, vs, k, pose, hw, band,
                          features=np.zeros(sdf.shape + (16,), F32), skip=False, chunk=1)
    locs = np.stack(np.nonzero(np.ones(sdf.shape, bool)), 1)
    with pytest.raises(_lib.SgnnError):
        raycast.cast_sparse_diff(locs, sdf.reshape(-1), sdf.shape, w2g, vs, k, pose, hw, band,
                                 features=np.zeros((len(locs), 2), F32))
