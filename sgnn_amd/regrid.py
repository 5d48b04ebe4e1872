"""A TSDF volume's state on another grid: resample a fusion.TSDFVolume, or merge one volume into another, across any
pair of grids that look at the same world (gravity or axis alignment after tracking, two registered sessions of one
room, another resolution or extent, rotated copies of a scan / target pair).

    dims, w2g = grid_for(vol, world_transform=R, pad=2)      # the box around the volume after moving the world by R
    moved = resample(vol, dims, w2g)                         # a new TSDFVolume: sdf, weight, free counter and colour
    merge(room, other_session)                               # fold a volume on any grid into `room` in place
    pyr2 = resample_pyramid(pyr, dims, w2g)                  # every level, level transforms as TSDFPyramid forms them

The rules are INTEGRATION.md section Q; the kernel (csrc/regrid.hip) and the independent NumPy restatement of the tests
(tests/regrid_ref.py) both follow that text, and the device matches the restatement bit for bit.  Never-seen voxels
stay never seen (no NaN, no smeared infinities), the weight is the smallest of the corners that took part, the free
counter and the 8.8 fixed-point colour record are copied whole from the nearest voxel.  Metric values are not
rescaled: the band of the result is the source's band, whatever the destination's voxel size.
"""
import numpy as np

from . import _lib, fusion
from ._glue import host as _host

MODES = ('linear', 'nearest')
# the destination brick of a wave: 0 = 4 x 4 x 4, 1 = 8 x 8 x 1, 2 = 64 x 1 x 1; the row won the measurement of section Q
# ("Wave shape", profiles/regrid_bench.json: the stores dominate and a row keeps them coalesced); the result
# does not depend on it
_DEFAULT_SHAPE = 2


def _matrix(m, what):
    m = _host(m, np.float32)
    if m.size != 16 or not np.isfinite(m).all():
        raise ValueError('%s must be a finite 4x4 matrix' % what)
    return m.reshape(4, 4)


def grid_map(src_world2grid, dst_world2grid):
    """Rule Q.1: rows 0..2 of A = src.world2grid . inv(dst.world2grid), formed in fp64 from the two fp32 matrices and
    rounded once to fp32, (3, 4); the identity where the two fp32 matrices are equal entry by entry (a crop or a pad).
    A takes a destination voxel to source voxel coordinates."""
    s = _matrix(src_world2grid, 'the source world2grid').astype(np.float64)
    d = _matrix(dst_world2grid, 'the destination world2grid').astype(np.float64)
    try:
        with np.errstate(all='ignore'):
            inv = np.linalg.inv(d)
    except np.linalg.LinAlgError:
        raise ValueError('the destination world2grid is singular')
    if not np.isfinite(inv).all():
        raise ValueError('the destination world2grid is singular')
    with np.errstate(all='ignore'):
        # equal matrices: the product is the identity, which the rounded inverse would miss by an ulp of the shift
        a = (np.eye(4) if np.array_equal(s, d) else s @ inv)[:3].astype(np.float32)
    if not np.isfinite(a).all():
        raise ValueError('the map between the two grids is not finite')
    return np.ascontiguousarray(a)


def _mode(mode):
    if mode not in MODES:
        raise ValueError('mode must be one of %s, got %r' % (MODES, mode))
    return int(mode == 'linear')


def grid_for(vol, world_transform=None, voxel_size=None, pad=0):
    """(dims_xyz, world2grid (4, 4) fp32) of the axis-aligned box around `vol` after the world has been moved by the 4x4
    `world_transform` T (None: not moved).  Host only, fp64: the 8 corners of the source grid (voxel centres 0 and
    d - 1 per axis) go to world space through inv(vol.world2grid) and through T; divided by the voxel size (None: the
    volume's own), lo = floor(min) - pad and hi = ceil(max) + pad per axis, dims = hi - lo + 1, the rounding rules of
    points.grid_for.  The matrix returned is box . T with box = scale(1 / voxel_size), translate(-lo): it takes the
    *original* world to the new grid, so its inverse, which rule Q.1 uses, holds inv(T), and resample(vol, dims,
    world2grid) is the moved volume."""
    w2g = _matrix(vol.world2grid, 'the volume\'s world2grid').astype(np.float64)
    t = np.eye(4) if world_transform is None else _host(world_transform, np.float64)
    if t.size != 16 or not np.isfinite(t).all():
        raise ValueError('world_transform must be a finite 4x4 matrix')
    t = t.reshape(4, 4)
    vs = float(vol.voxel_size if voxel_size is None else voxel_size)
    if not (vs > 0 and np.isfinite(vs)) or int(pad) < 0:
        raise ValueError('grid_for needs a positive voxel size and pad >= 0')
    try:
        g2w = np.linalg.inv(w2g)
    except np.linalg.LinAlgError:
        raise ValueError('the volume\'s world2grid is singular')
    hi_idx = np.array(vol.dims_xyz, np.float64) - 1.0
    corners = np.array([[(c >> a & 1) * hi_idx[a] for a in range(3)] + [1.0] for c in range(8)])
    moved = (corners @ g2w.T @ t.T)[:, :3] / vs
    if not np.isfinite(moved).all():
        raise ValueError('the moved volume is not finite')
    lo = np.floor(moved.min(0)) - int(pad)
    hi = np.ceil(moved.max(0)) + int(pad)
    box = np.eye(4, dtype=np.float64)
    box[:3, :3] /= vs
    box[:3, 3] = -lo
    return tuple(int(d) for d in hi - lo + 1), (box @ t).astype(np.float32)


def resample(vol, dims_xyz, world2grid, voxel_size=None, mode='linear', skip=True, _shape=None):
    """`vol` on the grid (dims_xyz, world2grid): a new fusion.TSDFVolume.  voxel_size: the
    result's (None: the source's; values are metres and are not rescaled).  Colour is carried iff the source has it;
    depth_min / depth_max are copied, the result has no obb.  mode: 'linear' (rule Q.5) or 'nearest' (rule Q.4).  skip: a
    launch detail, the result does not depend on it.  _shape picks the wave brick for the benchmark and the tests; it is
    not part of the interface and may go."""
    dims = fusion.check_dims(dims_xyz)
    linear = _mode(mode)
    a = grid_map(vol.world2grid, world2grid)
    vs = vol.voxel_size if voxel_size is None else np.float32(voxel_size)
    if not (vs > 0 and np.isfinite(vs)):
        raise ValueError('the voxel size must be positive')
    _lib.require_gpu()
    color = vol._color is not None
    out = fusion.TSDFVolume(dims, vs, _matrix(world2grid, 'world2grid'), vol.depth_min, vol.depth_max, device=vol.device,
                            color=color)
    sx, sy, sz = vol.dims_xyz
    _lib.call('sgnn_regrid_resample', *vol._state(color), sx, sy, sz, a.ctypes.data, linear, int(bool(skip)),
              int(_DEFAULT_SHAPE if _shape is None else _shape), *out._state(color), *dims)
    return out


def merge(dst, src, mode='linear', skip=True, _shape=None):
    """Fold `src`, a volume on any grid, into `dst` in place (rule Q.8: the resampled state is one more observation of
    each destination voxel); returns dst.  No intermediate volume is made.  Colour is folded only where both volumes
    carry it."""
    if dst is src:
        raise ValueError('a volume cannot be merged into itself')
    linear = _mode(mode)
    fusion.check_dims(dst.dims_xyz)
    fusion.check_dims(src.dims_xyz)
    a = grid_map(src.world2grid, dst.world2grid)
    if dst.device != src.device:
        raise ValueError('the volumes are on different devices (%s, %s)' % (dst.device, src.device))
    _lib.require_gpu()
    color = dst._color is not None and src._color is not None
    sx, sy, sz = src.dims_xyz
    _lib.call('sgnn_regrid_merge', *src._state(color), sx, sy, sz, a.ctypes.data, linear, int(bool(skip)),
              int(_DEFAULT_SHAPE if _shape is None else _shape), *dst._state(color), *dst.dims_xyz)
    return dst


def resample_pyramid(pyr, dims_xyz, world2grid, mode='linear', skip=True):
    """Every level of a fusion.TSDFPyramid on the grid (dims_xyz, world2grid) of its level 0: level k goes to dims
    ceil(d / 2**k) and world2grid_k = level_transform(k) @ world2grid (fp64 from the fp32 matrix, rounded once), the
    way TSDFPyramid forms its levels, with one resample per level; each level keeps its voxel size."""
    dims = fusion.check_dims(dims_xyz)
    w2g = _matrix(world2grid, 'world2grid').astype(np.float64)
    _mode(mode)
    levels = [([-(-d // 2 ** k) for d in dims], (fusion.level_transform(k) @ w2g).astype(np.float32))
              for k in range(len(pyr))]
    for (d, m), v in zip(levels, pyr.volumes):
        grid_map(v.world2grid, m)
    out = fusion.TSDFPyramid.__new__(fusion.TSDFPyramid)
    out.volumes = [resample(v, d, m, None, mode, skip) for (d, m), v in zip(levels, pyr.volumes)]
    return out
