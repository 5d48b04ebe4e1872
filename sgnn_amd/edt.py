"""Exact Euclidean feature transform of dense volumes on the GPU, and what it is for here: carrying the colours of a
fused scan to the voxels the sensor never saw, so that a completed scene is meshed in colour on both halves.

For every voxel of a (Z, Y, X) seed mask the transform gives the nearest seed voxel and the squared distance to it, in
integers and exactly; among seeds at the same distance the one with the smallest linear index wins, so the result is a
pure function of the input.  The reference project has no counterpart; the rules are listed in INTEGRATION.md section
O, and that text is the contract of the kernels (sgnn_amd/csrc/edt.hip) and of the brute-force host restatement of the
tests (tests/edt_ref.py), which agree bit for bit.

    ft = feature_transform(seeds, max_dist=None)              # FeatureTransform(dist2, nearest): int32, -1 = none
    d = distance(seeds, max_dist=None, voxel_size=1.0)        # fp32 sqrt(dist2) * voxel_size, +inf where none
    rgb = fill_colors(colors, valid, max_dist=None)           # (Z, Y, X, 3) uint8: colors[nearest], 0 where none
    rgb = volume_colors(vol, dims_zyx=None, max_dist=None)    # a TSDFVolume(color=True): colors(dims), filled

nearest is the linear index (z * Y + y) * X + x of the seed.  max_dist = R, in voxels, keeps seeds within
dist2 <= floor(R * R) only (every voxel within reach gets what it gets without a cap) and bounds the work: prefer it
where seeds are sparse.  Dilation and erosion by a radius are dist2 <= r * r of a mask and of its complement.  Inputs
may be numpy or torch, on the host or the device; results stay on the device.  Without a device every call raises
_lib.SgnnError.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._glue import device, to_device

MAX_DIM = 1024              # SGNN_EDT_MAX_DIM of include/sgnn_hip.h: a coordinate is 10 bits of the packed feature
LIMIT = 2 ** 31

FeatureTransform = namedtuple('FeatureTransform', 'dist2 nearest')


def _dims(shape, what):
    if len(shape) != 3:
        raise ValueError('%s must be (Z, Y, X), got %s' % (what, tuple(shape)))
    dims = tuple(int(v) for v in shape)
    if max(dims) > MAX_DIM or dims[0] * dims[1] * dims[2] >= LIMIT:
        raise ValueError('%s %s: every axis must be <= %d and there must be fewer than 2^31 voxels'
                         % (what, dims, MAX_DIM))
    return dims


def _cap2(max_dist):
    """floor(R * R), the product in fp64; -1 = no cap (None, or a square that no volume reaches)."""
    if max_dist is None:
        return -1
    r = float(max_dist)
    if not r >= 0.0:
        raise ValueError('max_dist must be None or >= 0, got %r' % (max_dist,))
    rr = r * r
    return -1 if rr >= float(LIMIT) else int(math.floor(rr))


def _mask(seeds, dev):
    """The contiguous uint8 device mask of a checked seed volume: non-zero = seed."""
    t = seeds if torch.is_tensor(seeds) else torch.from_numpy(seeds if seeds.flags.writeable else seeds.copy())
    t = t.to(dev)
    return (t if t.dtype == torch.bool else t != 0).to(torch.uint8).contiguous()


def _as_array(x):
    return x if torch.is_tensor(x) else np.ascontiguousarray(x)


def _transform(mask, dims, cap2):
    dz, dy, dx = dims
    dev = mask.device
    dist2 = torch.empty(dims, dtype=torch.int32, device=dev)
    nearest = torch.empty(dims, dtype=torch.int32, device=dev)      # holds the x pass's features until the last pass
    if dz * dy * dx == 0:
        return FeatureTransform(dist2, nearest)
    tmp = torch.empty(dims, dtype=torch.int32, device=dev)
    _lib.call('sgnn_edt_rows', _lib.ptr(mask), dz, dy, dx, cap2, _lib.ptr(nearest))
    _lib.call('sgnn_edt_axis', _lib.ptr(nearest), dz, dy, dx, 1, cap2, _lib.ptr(tmp), None, None)
    _lib.call('sgnn_edt_axis', _lib.ptr(tmp), dz, dy, dx, 0, cap2, None, _lib.ptr(dist2), _lib.ptr(nearest))
    return FeatureTransform(dist2, nearest)


def feature_transform(seeds, max_dist=None):
    """FeatureTransform(dist2, nearest) of a (Z, Y, X) seed volume (bool, or any number type: non-zero = seed), each
    (Z, Y, X) int32 on the device: the squared distance, in voxels, to the nearest seed and that seed's linear index;
    -1 and -1 where there is no seed, or none within max_dist."""
    seeds = _as_array(seeds)
    dims = _dims(seeds.shape, 'seeds')
    cap2 = _cap2(max_dist)
    dev = seeds.device if torch.is_tensor(seeds) and seeds.is_cuda else device()
    _lib.require_gpu()
    return _transform(_mask(seeds, dev), dims, cap2)


def distance(seeds, max_dist=None, voxel_size=1.0):
    """(Z, Y, X) float32 on the device: sqrt(dist2) * voxel_size, +inf where feature_transform has -1."""
    dist2 = feature_transform(seeds, max_dist).dist2
    d = torch.sqrt(dist2.clamp(min=0).float()) * voxel_size
    return torch.where(dist2 < 0, torch.full_like(d, float('inf')), d)


def fill_colors(colors, valid, max_dist=None):
    """(Z, Y, X, 3) uint8 on the device: every voxel takes the colour of the nearest voxel of the seed mask valid
    ((Z, Y, X) bool or uint8), a byte copy; 0 where there is none, or none within max_dist.  Seeds keep their own."""
    colors, valid = _as_array(colors), _as_array(valid)
    dims = _dims(valid.shape, 'valid')
    if tuple(colors.shape) != dims + (3,) or str(colors.dtype) not in ('torch.uint8', 'uint8'):
        raise ValueError('colors must be %s uint8, got %s %s' % (dims + (3,), tuple(colors.shape), colors.dtype))
    cap2 = _cap2(max_dist)
    dev = colors.device if torch.is_tensor(colors) and colors.is_cuda else device()
    _lib.require_gpu()
    colors = to_device(colors, torch.uint8, dev)
    nearest = _transform(_mask(valid, dev), dims, cap2).nearest
    out = torch.empty_like(colors)
    _lib.call('sgnn_edt_fill', _lib.ptr(colors), _lib.ptr(nearest), dims[0] * dims[1] * dims[2], _lib.ptr(out))
    return out


def volume_colors(vol, dims_zyx=None, max_dist=None):
    """The colour volume of a fusion.TSDFVolume(color=True) with the voxels that no colour frame reached filled from
    the nearest one that has a colour (color_weight() > 0): what marching_cubes.run_marching_cubes takes next to a
    predicted geometry.  dims_zyx pads or crops exactly as vol.colors(dims_zyx) does; padding holds no seed."""
    _lib.require_gpu()
    if vol.color_state() is None:
        raise ValueError('the volume was built without color=True')
    if dims_zyx is not None:
        _dims(tuple(dims_zyx), 'dims_zyx')
    rgb = vol.colors(dims_zyx)
    wc = vol.color_weight()
    valid = torch.zeros(tuple(rgb.shape[:3]), dtype=torch.uint8, device=rgb.device)
    z, y, x = (min(int(a), int(b)) for a, b in zip(valid.shape, wc.shape))
    valid[:z, :y, :x] = wc[:z, :y, :x] != 0
    return fill_colors(rgb, valid, max_dist)
