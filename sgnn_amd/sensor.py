"""A depth sensor simulated on rendered frames: the stage between "mesh" and "scan" of a virtual scan.

render.render_depth and raycast.cast_volume give perfect z-buffers; a network trained on scans fused from them sees
none of the holes a sensor makes.  degrade() turns clean metric depth into what a structured-light sensor with a
horizontal baseline would have returned: lateral jitter at edges, a range gate, the projector's shadow beside a
foreground object, loss at depth edges and at grazing angles, random dropout, axial noise that grows with distance and
incidence, and the steps of a quantised disparity.  The rules are INTEGRATION.md section V; that text is the contract
of the kernels (sgnn_amd/csrc/sensor.hip) and of the independent NumPy restatement of the tests (tests/sensor_ref.py).

    depth = render.render_depth(verts, faces, K, poses, (240, 320))
    model = SensorModel()                                    # every stage can be switched off on its own
    noisy = degrade(depth, K, model, seed=0)                 # (F, h, w) fp32 on the device, -inf = nothing
    vol.integrate(fusion.bilateral(noisy), K, poses)
    shadow = shadow_mask(depth, K, baseline=0.075)           # (F, h, w) bool: seen by the camera, not by the projector
    keep = keep_frames(len(poses), chance_drop=0.65, seed=0) # the frames an incomplete scan keeps

The result is a function of the pixel, its frame id and the seed: the same seed gives the same bits on every run, and
degrade(depth[a:b], ..., frame_ids=arange(a, b)) gives the bits of the whole call.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._glue import host as _host, source_device as _source_device, to_device as _to_device

# struct sgnn_sensor_model (include/sgnn_hip.h)
MODEL_DTYPE = np.dtype([('lateral_sigma', '<f4'), ('min_depth', '<f4'), ('max_depth', '<f4'), ('baseline', '<f4'),
                        ('cos_min', '<f4'), ('edge_drop', '<f4'), ('drop', '<f4'), ('a0', '<f4'), ('a1', '<f4'),
                        ('a2', '<f4'), ('a3', '<f4'), ('disparity_quantum', '<f4')])
assert MODEL_DTYPE.itemsize == 48

_FIELDS = MODEL_DTYPE.names
_DEFAULTS = (0.5, 0.4, 6.0, 0.075, 0.173648178, 0.5, 0.0, 0.0012, 0.0019, 0.4, 0.05, 0.125)
_KEEP_SALT = 0x6b6565705f66726d
_M64 = (1 << 64) - 1


class SensorModel(collections.namedtuple('SensorModel', _FIELDS)):
    """The sensor of degrade(): the fields of struct sgnn_sensor_model, in its order (rules V.3 - V.9).

    lateral_sigma 0.5 pixel; min_depth 0.4 and max_depth 6.0 metres (the reference's s_minDepth / s_maxDepth);
    baseline 0.075 m, the projector at (baseline, 0, 0) in the camera frame; cos_min cos 80 degrees; edge_drop 0.5;
    drop 0; a0 0.0012, a1 0.0019, a2 0.4: sigma(z) = a0 + a1 (z - a2)^2 metres, times 1 + a3 tan^2(incidence) with a3
    0.05; disparity_quantum 1/8 pixel.  A stage is off at: lateral_sigma 0; min_depth -inf and max_depth inf; baseline
    0 (no shadow, no disparity steps); cos_min 0; edge_drop 0; drop 0; a0 = a1 = 0; disparity_quantum 0.  off() has
    them all off; SensorModel.off()._replace(...) switches one on."""
    __slots__ = ()

    def __new__(cls, *args, **kwargs):
        values = dict(zip(_FIELDS, _DEFAULTS))
        if len(args) > len(_FIELDS):
            raise TypeError('SensorModel takes at most %d values' % len(_FIELDS))
        values.update(zip(_FIELDS, args))
        for k in kwargs:
            if k not in values:
                raise TypeError('SensorModel has no field %r' % k)
        values.update(kwargs)
        return super().__new__(cls, *(float(values[k]) for k in _FIELDS))

    @classmethod
    def off(cls):
        """Every stage off: degrade() returns its input (finite or -inf pixels) bit for bit."""
        return cls(0.0, -math.inf, math.inf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)

    @classmethod
    def constant(cls, sigma, **kwargs):
        """The defaults with the same axial noise at every distance and angle: a0 = sigma, a1 = a3 = 0.  That is the
        reference's s_depthNoiseSigma (0.01), which no line of its code reads."""
        return cls(**kwargs)._replace(a0=float(sigma), a1=0.0, a3=0.0)

    def record(self):
        """The model as one MODEL_DTYPE record, rounded to fp32 and checked against the ranges of the header."""
        r = np.zeros((), dtype=MODEL_DTYPE)
        for k in _FIELDS:
            r[k] = np.float32(getattr(self, k))
        unit = lambda v: 0 <= v <= 1                                # noqa: E731 (a NaN fails)
        if not (0 <= r['lateral_sigma'] < np.inf):
            raise ValueError('lateral_sigma must be finite and not negative')
        if not r['min_depth'] <= r['max_depth']:
            raise ValueError('min_depth must not exceed max_depth')
        if not (np.isfinite(r['baseline']) and all(np.isfinite(r[k]) for k in ('a0', 'a1', 'a2', 'a3'))):
            raise ValueError('baseline, a0, a1, a2 and a3 must be finite')
        if not (unit(r['cos_min']) and unit(r['edge_drop']) and unit(r['drop'])):
            raise ValueError('cos_min, edge_drop and drop must lie in [0, 1]')
        if not (0 <= r['disparity_quantum'] < np.inf):
            raise ValueError('disparity_quantum must be finite and not negative')
        return r


def hash64(k):
    """sgnn_hash64 of csrc/common.h (the murmur3 finaliser) on a Python integer."""
    k &= _M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    return k ^ (k >> 33)


def _seed(seed):
    seed = int(seed)
    if not 0 <= seed <= _M64:
        raise ValueError('seed must be an integer in [0, 2^64)')
    return seed


def _frames(depth, intrinsics):
    """(device, depth (F, h, w) fp32 on it, intrinsics (F, 4) fp32 on it, whether depth came as (h, w))."""
    shape = tuple(int(v) for v in getattr(depth, 'shape', ()))
    if len(shape) not in (2, 3):
        raise ValueError('depth must be (F, h, w) or (h, w), got %s' % (shape,))
    single = len(shape) == 2
    nf, h, w = (1,) + shape if single else shape
    if nf * h * w >= 2 ** 31:
        raise ValueError('F h w = %d does not fit 31 bits' % (nf * h * w))
    k = _host(intrinsics, np.float32)
    if k.shape == (4,):
        k = np.broadcast_to(k, (nf, 4))
    if k.shape != (nf, 4):
        raise ValueError('intrinsics must be (4,) or (F, 4) for %d frames, got %s' % (nf, k.shape))
    if not np.isfinite(k).all() or (k[:, :2] == 0).any():
        raise ValueError('intrinsics must be finite, fx and fy not 0')
    dev = _source_device(depth)
    d = _to_device(depth, torch.float32, dev).reshape(nf, h, w)
    return dev, d, _to_device(np.ascontiguousarray(k), torch.float32, dev), single


def _shadow(d, k, baseline):
    nf, h, w = d.shape
    mask = torch.empty((nf, h, w), dtype=torch.uint8, device=d.device)
    _lib.call('sgnn_sensor_shadow', d.data_ptr(), nf, h, w, k.data_ptr(), float(baseline), mask.data_ptr())
    return mask


def shadow_mask(depth, intrinsics, baseline=0.075):
    """The pixels the camera sees and the projector at (baseline, 0, 0) does not (rule V.5) -> (F, h, w) bool on the
    device ((h, w) for one frame).  depth: clean metric z-depth, (F, h, w) or (h, w), -inf = nothing; intrinsics (4,)
    or (F, 4) fx, fy, cx, cy; numpy arrays or torch tensors, host or device.  baseline 0 gives an empty mask."""
    baseline = np.float32(baseline)
    if not np.isfinite(baseline):
        raise ValueError('baseline must be finite')
    dev, d, k, single = _frames(depth, intrinsics)
    mask = _shadow(d, k, baseline).view(torch.bool)
    return mask[0] if single else mask


def degrade(depth, intrinsics, model=None, seed=0, frame_ids=None):
    """Clean depth frames as the sensor `model` (None: SensorModel()) would have returned them -> (F, h, w) fp32 on
    the device ((h, w) for one frame), -inf = nothing.

    depth, intrinsics: as shadow_mask.  seed: an integer in [0, 2^64); the same seed gives the same bits.  frame_ids:
    None (0 .. F - 1) or F integers >= 0, the frame numbers that enter the random draws: frames [a:b] with
    frame_ids=arange(a, b) get the bits they have in the whole call."""
    model = SensorModel() if model is None else model
    if not isinstance(model, SensorModel):
        raise ValueError('model must be a sensor.SensorModel')
    rec, seed = model.record(), _seed(seed)
    dev, d, k, single = _frames(depth, intrinsics)
    nf, h, w = d.shape
    ids = None
    if frame_ids is not None:
        ids_host = _host(frame_ids, np.int64).reshape(-1)
        if ids_host.shape != (nf,) or (ids_host < 0).any():
            raise ValueError('frame_ids must be %d integers >= 0' % nf)
        ids = _to_device(ids_host, torch.int64, dev)
    out = torch.empty_like(d)
    mask = _shadow(d, k, rec['baseline']) if rec['baseline'] != 0 else None
    _lib.call('sgnn_sensor_degrade', d.data_ptr(), _lib.ptr(mask), nf, h, w, k.data_ptr(), _lib.ptr(ids),
              rec.ctypes.data, seed, out.data_ptr())
    return out[0] if single else out


def keep_frames(n, chance_drop=0.65, seed=0):
    """The frames an incomplete scan keeps, reproducibly -> increasing int64 indices into range(n) (host).  Frame i is
    kept iff its uniform draw exceeds chance_drop, as in the reference's generateIncompleteFramesMatterport
    (Visualizer.h:28-35; s_chanceDropFrames = 0.65).  The draw of frame i is ((hash64((hash64(seed) ^ salt) + i) >> 12)
    + 0.5) / 2^52 in fp64, strictly between 0 and 1: chance_drop 0 keeps every frame and 1 none (rule V.10)."""
    n, chance_drop = int(n), float(chance_drop)
    if n < 0 or not 0 <= chance_drop <= 1:
        raise ValueError('n must not be negative and chance_drop must lie in [0, 1]')
    base = hash64(_seed(seed)) ^ _KEEP_SALT
    draws = np.array([((hash64(base + i) >> 12) + 0.5) / 2.0 ** 52 for i in range(n)], dtype=np.float64)
    return np.nonzero(draws > chance_drop)[0].astype(np.int64)
