"""Point sets and TSDF volumes registered against a TSDF volume on the GPU: the transform that regrid.merge and
points.integrate take for granted.

track.align is projective frame-to-model ICP: it needs a depth frame with intrinsics.  This module aligns anything that
is a set of surface points (a second session's volume, a LiDAR sweep, the vertices of a mesh, a voxelised model) with a
volume by point-to-SDF Gauss-Newton: the destination is already a distance field, so a source point needs no
nearest-neighbour search.  Its residual is the trilinear sample of the sdf at its transformed position, its Jacobian the
gradient of the same interpolant.  The rules are INTEGRATION.md section R; that text is the contract of the kernel
(sgnn_amd/csrc/register.hip) and of the independent NumPy restatement of the tests (tests/register_ref.py).

    res = align(points, room, guess)                          # RegisterResult; res.T: source world -> room's world
    res = best(align(points, room, guesses))                  # (B, 4, 4) guesses advance together, one launch a step
    res = align_volumes(other, room, guess)                   # surface_points(other, stride=2) against room
    regrid.merge(room, apply(other, res.T))                   # the registered merge
    sys = normal_equations(points, sdf, world2grid, T, band)  # (B, 32) fp64 on the device

align needs a guess within about one band of the truth (None is the identity).  search produces the guesses: it scores
a lattice of candidate transforms against an integer distance field of the destination, refines the best of them on a
ladder of halved pitches and hands them to align (csrc/register_search.hip and the restatement
tests/register_search_ref.py agree on every integer):

    res = search(points, room)                                # SearchResult; res.T where res.ok, res.candidates
    res = search_volumes(other, room, yaw_step=10.0)          # surface_points(other, stride=2) against room
    s = score(points, distance_field(room), T)                # (B, 3) int64: cost, inliers, outside

The device builds the Gauss-Newton systems and the scores; the 6x6 solve and the update of the transform are
track.solve_step and track.se3_exp, on the host in fp64.
"""
import collections
import math

import numpy as np
import torch

from . import _gn, _lib, edt, fusion  # noqa: F401  (_lib: the tests count launches through it)
from ._glue import (host as _host, invertible as _invertible, positive as _gate, source_device as _source_device,
                    to_device as _to_device)
from ._gn import se3_exp, solve_step, unpack  # noqa: F401  (the layout of a system is shared with track)

# struct sgnn_register_pair (include/sgnn_hip.h)
PAIR_DTYPE = np.dtype([('t', '<f4', (12,)), ('w', '<f4', (12,))])
assert PAIR_DTYPE.itemsize == 96

MAX_BLOCKS = 256            # SGNN_REGISTER_MAX_BLOCKS
MAX_PAIRS = 65535
MAX_POINTS = 2 ** 31 - MAX_BLOCKS * 256

RegisterResult = collections.namedtuple('RegisterResult', 'T ok pairs rmse history')
RegisterResult.__doc__ = """What align() found for one guess: T (4, 4) fp64, source world -> destination world (the
guess when ok is false), ok, pairs and rmse (the sdf's unit) of the last iteration, and history: the number of
associated points of every iteration run."""


def _matrices(T, name):
    """(B, 4, 4) fp64 host matrices from (4, 4) or (B, 4, 4) -> (matrices, whether a single one came in)."""
    t = _host(T, np.float64)
    if t.shape == (4, 4):
        return t[None], True
    if t.ndim != 3 or t.shape[1:] != (4, 4):
        raise ValueError('%s must be (4, 4) or (B, 4, 4), got %s' % (name, t.shape))
    return t, False


def pair_table(world2grid, T):
    """Host table of sgnn_register_pair records (rule 1): rows 0..2 of T (B, 4, 4) and of world2grid rounded to fp32.
    A record with a non-finite entry (in fp64 or after rounding) gets NaN rows of T: its system stays empty."""
    t64 = _host(T, np.float64)
    if t64.ndim != 3 or t64.shape[1:] != (4, 4):
        raise ValueError('T must be (B, 4, 4), got %s' % (t64.shape,))
    w64 = _host(world2grid, np.float64)
    if w64.shape != (4, 4):
        raise ValueError('world2grid must be (4, 4), got %s' % (w64.shape,))
    nb = t64.shape[0]
    table = np.zeros(nb, dtype=PAIR_DTYPE)
    with np.errstate(all='ignore'):
        w = w64[:3, :].astype(np.float32)
    w_ok = np.isfinite(w).all() and np.isfinite(w64).all()
    table['t'] = _gn.record_rows(t64[:, :3, :].reshape(nb, 12), np.isfinite(t64[:, 3]).all(axis=1) & w_ok)
    table['w'] = w.reshape(12) if w_ok else 0
    return table


def _check_points(points):
    shape = tuple(int(v) for v in points.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('points must be (P, 3), got %s' % (shape,))
    if shape[0] >= MAX_POINTS:
        raise ValueError('%d points in one call (limit %d)' % (shape[0], MAX_POINTS - 1))
    return shape[0]


def _check_sdf(sdf):
    shape = tuple(int(v) for v in sdf.shape)
    if len(shape) != 3 or min(shape) < 2 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('sdf must be (Z, Y, X) with every dimension >= 2 and fewer than 2^31 voxels, got %s' % (shape,))
    return shape


def _system(pts, sdf, table, band, max_dist, min_grad2, residual, cell, dev):
    """The launch: device fp32 points and sdf, a host record table -> (B, 32) fp64 on the device."""
    npts, nb = int(pts.shape[0]), int(table.shape[0])
    dz, dy, dx = (int(v) for v in sdf.shape)
    if nb == 0 or npts == 0:                                                # no launch: nothing writes the outputs
        if residual is not None:
            residual.fill_(float('nan'))
        if cell is not None:
            cell.fill_(-1)
    head = (pts.data_ptr(), npts, sdf.data_ptr(), dx, dy, dz)
    return _gn.launch('sgnn_register_system', head, table, (band, max_dist, min_grad2), npts, MAX_BLOCKS,
                      (residual, cell), dev)


def _gates(band, max_dist, min_grad):
    band = _gate('band', band)
    max_dist = band if max_dist is None else _gate('max_dist', max_dist)
    g = np.float32(min_grad)
    if not (g >= 0 and np.isfinite(g)):
        raise ValueError('min_grad must not be negative')
    return band, max_dist, g * g                                            # one fp32 product (rule 5)


def normal_equations(points, sdf, world2grid, T, band, max_dist=None, min_grad=0.5, residual=None, cell=None):
    """One Gauss-Newton system of point-to-SDF alignment per transform -> (B, 32) fp64 on the device: the 21 sums of the
    upper triangle of J^T J (row-major), the 6 of J^T r, the sum of r^2, the number of associated points, three zeros
    (rules 1-7; track.unpack gives A, g, E, N).

    points (P, 3) in the source world; sdf (Z, Y, X) of the destination in any unit, band and max_dist (None: band) in
    that unit; world2grid (4, 4) of the destination; T (4, 4) or (B, 4, 4): source world -> destination world, every
    one against the same points and volume in one launch.  min_grad: the smallest length of the world-space gradient
    an association may have.  residual: None or a device fp32 tensor (B, P) that receives r, NaN where a point has no
    association; cell: None or a device int32 tensor (B, P) that receives the linear index of the sample's cell, or
    -1.  numpy arrays or torch tensors, host or device."""
    dev = _source_device(points)
    npts = _check_points(points)
    _check_sdf(sdf)
    band, max_dist, min_grad2 = _gates(band, max_dist, min_grad)
    t64, _ = _matrices(T, 'T')
    nb = t64.shape[0]
    if nb > MAX_PAIRS:
        raise ValueError('more than %d transforms in one call' % MAX_PAIRS)
    table = pair_table(world2grid, t64)
    _gn.check_per_item((nb, npts), residual, cell, 'cell')
    pts = _to_device(points, torch.float32, dev)
    return _system(pts, _to_device(sdf, torch.float32, dev), table, band, max_dist, min_grad2, residual, cell, dev)


def _volume(vol):
    """(sdf, world2grid, band) of a fusion.TSDFVolume (band = 3 vs as one fp32 product, as raycast.cast_volume forms
    it) or of such a triple."""
    if isinstance(vol, fusion.TSDFVolume):
        return vol.sdf(), vol.world2grid, np.float32(3.0) * vol.voxel_size
    try:
        sdf, world2grid, band = vol
    except (TypeError, ValueError):
        raise ValueError('vol must be a fusion.TSDFVolume or (sdf, world2grid, band)')
    return sdf, world2grid, band


def align(points, vol, guess=None, iterations=30, max_dist=None, min_grad=0.5, min_pairs=64, timers=None):
    """The transform that takes `points` (P, 3), source world, onto the surface of `vol` -> RegisterResult, or a list of
    B of them for a (B, 4, 4) guess.

    vol: a fusion.TSDFVolume or (sdf, world2grid, band).  guess: (4, 4), (B, 4, 4) or None (the identity): where the
    iteration starts; it has to be close (INTEGRATION.md section R says how close).  iterations: Gauss-Newton steps,
    a fixed number with no early exit; all B guesses advance in one launch per step.  A guess whose system has fewer
    than min_pairs associations or is not positive definite ends with ok false and T = the guess; it rides along as an
    empty record.  timers: None or a dict whose 'system' and 'solve' entries get seconds added (measurements; switches on
    a device synchronisation per stage)."""
    sdf, world2grid, band = _volume(vol)
    npts = _check_points(points)
    _check_sdf(sdf)
    band, max_dist, min_grad2 = _gates(band, max_dist, min_grad)
    if int(iterations) < 1:
        raise ValueError('iterations = %s' % (iterations,))
    guess64, single = _matrices(np.eye(4) if guess is None else guess, 'guess')
    nb = guess64.shape[0]
    if nb > MAX_PAIRS:
        raise ValueError('more than %d guesses in one call' % MAX_PAIRS)
    w64 = _host(world2grid, np.float64)
    if w64.shape != (4, 4):
        raise ValueError('world2grid must be (4, 4), got %s' % (w64.shape,))
    dev = _source_device(sdf, points)
    pts = _to_device(points, torch.float32, dev)
    field = _to_device(sdf, torch.float32, dev)
    run = _gn.Steps(guess64, min_pairs)
    tick = _gn.Timer(timers)
    for _ in range(int(iterations)):
        if not any(run.alive):
            break
        current = np.where(np.array(run.alive)[:, None, None], run.T, np.nan)
        systems = _system(pts, field, pair_table(w64, current), band, max_dist, min_grad2, None, None,
                          dev).cpu().numpy()                                 # 256 bytes per guess
        tick('system')
        run.step(systems)
        tick('solve')
    out = [RegisterResult(run.T[b].copy(), run.alive[b], run.pairs[b], run.rmse[b], tuple(run.history[b]))
           for b in range(nb)]
    return out[0] if single else out


def best(results):
    """The ok result of lowest rmse among those with at least half as many pairs as the ok result with the most; None
    when no result is ok.  (A guess far off can end on a few points that happen to fit well; the pair count keeps it
    from winning.  The rule is a choice, not a measurement.)"""
    ok = [r for r in results if r.ok]
    if not ok:
        return None
    most = max(r.pairs for r in ok)
    return min((r for r in ok if 2 * r.pairs >= most), key=lambda r: r.rmse)


def surface_points(vol_or_sdf, world2grid=None, band=None, stride=1):
    """The zero crossings of a volume as world-space points -> (P, 3) fp32 on the device.

    vol_or_sdf: a fusion.TSDFVolume (world2grid and band = 3 vs are its own unless given) or an sdf (Z, Y, X) with its
    world2grid; band None for a bare sdf: every finite voxel is usable.  Each pair of axis neighbours that are both
    usable (finite, |v| < band) with pv > 0 >= v or v > 0 >= pv gives the point at the linear zero crossing,
    pv / (pv - v) of the way from the first voxel to the second.  Order: the x pairs, the y pairs, the z pairs, each by
    the linear index of the pair's first voxel; every stride-th point of that list is kept and mapped through
    inv(world2grid) (fp64 inverse, rounded to fp32, applied in the order of fusion._affine).  Plain torch ops."""
    if isinstance(vol_or_sdf, fusion.TSDFVolume):
        sdf = vol_or_sdf.sdf()
        world2grid = vol_or_sdf.world2grid if world2grid is None else world2grid
        band = np.float32(3.0) * vol_or_sdf.voxel_size if band is None else band
    else:
        sdf = vol_or_sdf
        if world2grid is None:
            raise ValueError('an sdf needs its world2grid')
    if len(tuple(sdf.shape)) != 3:
        raise ValueError('sdf must be (Z, Y, X), got %s' % (tuple(sdf.shape),))
    if int(stride) < 1:
        raise ValueError('stride = %s' % (stride,))
    band = np.float32(np.inf) if band is None else np.float32(band)
    if not band > 0:
        raise ValueError('band must be positive')
    m = np.linalg.inv(_invertible(world2grid, 'world2grid', np.float32).astype(np.float64)).astype(np.float32)
    dev = _source_device(sdf)
    s = _to_device(sdf, torch.float32, dev)
    usable = torch.isfinite(s) & (s.abs() < float(band))
    found = []
    for axis in range(3):                                                   # x, y, z: dims 2, 1, 0 of the tensor
        dim = 2 - axis
        n = int(s.shape[dim])
        if n < 2:
            continue
        pv, v = s.narrow(dim, 0, n - 1), s.narrow(dim, 1, n - 1)
        cross = usable.narrow(dim, 0, n - 1) & usable.narrow(dim, 1, n - 1) & (((pv > 0) & (v <= 0)) |
                                                                               ((v > 0) & (pv <= 0)))
        idx = torch.nonzero(cross)                                          # row-major: the first voxel's linear order
        a, b = pv[cross], v[cross]
        g = idx.flip(1).to(torch.float32)                                   # x, y, z
        g[:, axis] = g[:, axis] + a / (a - b)
        found.append(g)
    g = torch.cat(found)[::int(stride)] if found else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    x, y, z = g[:, 0], g[:, 1], g[:, 2]
    rows = [((float(m[r, 0]) * x + float(m[r, 1]) * y) + float(m[r, 2]) * z) + float(m[r, 3]) for r in range(3)]
    return torch.stack(rows, 1).contiguous()


def align_volumes(src_vol, dst_vol, guess=None, stride=2, **align_kwargs):
    """align(surface_points(src_vol, stride=stride), dst_vol, guess, **align_kwargs): the transform from the world of
    one fusion.TSDFVolume to that of another."""
    if not isinstance(src_vol, fusion.TSDFVolume):
        raise ValueError('src_vol must be a fusion.TSDFVolume')
    return align(surface_points(src_vol, stride=stride), dst_vol, guess, **align_kwargs)


def apply(vol, T):
    """vol.copy() moved by T (4, 4), source world -> destination world: its world2grid becomes
    vol.world2grid . inv(T), formed in fp64 and rounded to fp32, so regrid.merge(room, apply(other, res.T)) is the
    registered merge."""
    t = _invertible(T, 'T')
    moved = vol.copy()
    moved.world2grid = (vol.world2grid.astype(np.float64) @ np.linalg.inv(t)).astype(np.float32)
    return moved


# ---------------------------------------------------------------------------------------------------------
# search: guesses by exhaustive integer scoring
# ---------------------------------------------------------------------------------------------------------
# struct sgnn_register_pose (include/sgnn_hip.h)
POSE_DTYPE = np.dtype([('m', '<f4', (12,))])
assert POSE_DTYPE.itemsize == 48

MAX_POSES = 1 << 24         # SGNN_REGISTER_SCORE_MAX_POSES: records of one launch
MAX_LAUNCHES = 64           # launches search allows its level 0
SCORE_MAX_POINTS = 2 ** 31 - 65536
_TABLE_BLOCK = 1 << 18      # records whose fp64 matrices the host holds at a time

SearchField = collections.namedtuple('SearchField', 'dist2 world2grid dims cap2')
SearchField.__doc__ = """What score() samples: dist2 (Z, Y, X) int32 on the device, the squared distance in voxels to
the nearest seed voxel of the destination's surface, -1 = none within reach; the destination's world2grid (4, 4) fp32 on
the host; dims (Z, Y, X); cap2 = floor(reach^2) in voxels, what a point beyond reach or outside the volume costs."""

SearchResult = collections.namedtuple('SearchResult', 'T ok result candidates field')
SearchResult.__doc__ = """What search() found: T (4, 4) fp64, source world -> destination world (the identity when ok is
false), ok, result: the RegisterResult that best() chose (None when none is ok), candidates: the poses kept after the
last level as (T, cost, inliers, outside), best score first as selected at level 0, and the SearchField."""


def _positive(name, v, integer=False):
    """v as a float (or an int) that must be positive and finite: ValueError otherwise, no device involved."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError('%s must be a positive number, got %r' % (name, v))
    if not (f > 0 and math.isfinite(f)) or (integer and f != int(f)):
        raise ValueError('%s must be a positive %s, got %r' % (name, 'integer' if integer else 'number', v))
    return int(f) if integer else f


def _field_volume(vol, reach):
    """The checks of distance_field that need no device -> (is a TSDFVolume, dims, reach in voxels, cap2)."""
    is_vol = isinstance(vol, fusion.TSDFVolume)
    if is_vol:
        shape = tuple(vol.dims_xyz[::-1])
    else:
        try:
            sdf, _, _ = vol
            shape = tuple(sdf.shape)
        except (TypeError, ValueError, AttributeError):
            raise ValueError('vol must be a fusion.TSDFVolume or (sdf, world2grid, band)')
    dims = edt._dims(shape, 'sdf')
    if min(dims) < 1:
        raise ValueError('sdf %s has an empty axis' % (dims,))
    reach = _positive('reach', (0.5 if is_vol else 10.0) if reach is None else reach)
    reach_vox = reach / float(vol.voxel_size) if is_vol else reach
    cap2 = edt._cap2(reach_vox)
    if cap2 < 1:
        raise ValueError('reach = %r is %r voxels: it must be at least one voxel and its square below 2^31'
                         % (reach, reach_vox))
    return is_vol, dims, reach_vox, cap2


def distance_field(vol, reach=None):
    """The integer distance field score() samples -> SearchField(dist2, world2grid, dims, cap2).

    vol: a fusion.TSDFVolume or (sdf, world2grid, band).  A voxel is a seed if it is usable (finite, |v| < band) and has
    an axis neighbour that is usable with pv > 0 >= v or v > 0 >= pv (both voxels of a pair of surface_points); dist2 is
    edt.feature_transform(seeds, max_dist=reach in voxels).dist2.  reach: metres for a TSDFVolume (None: 0.5), voxels
    for a triple (None: 10); a choice, not a measurement.  edt's limits apply (every axis <= 1024, fewer than 2^31
    voxels).  Torch ops and edt; no kernel of its own."""
    _, dims, reach_vox, cap2 = _field_volume(vol, reach)
    sdf, world2grid, band = _volume(vol)
    band = _gate('band', band)
    w = _host(world2grid, np.float32)
    if w.shape != (4, 4):
        raise ValueError('world2grid must be (4, 4), got %s' % (w.shape,))
    dev = _source_device(sdf)
    s = _to_device(sdf, torch.float32, dev)
    usable = torch.isfinite(s) & (s.abs() < float(band))
    seeds = torch.zeros(dims, dtype=torch.bool, device=dev)
    for dim in range(3):
        n = dims[dim]
        if n < 2:
            continue
        pv, v = s.narrow(dim, 0, n - 1), s.narrow(dim, 1, n - 1)
        cross = usable.narrow(dim, 0, n - 1) & usable.narrow(dim, 1, n - 1) & (((pv > 0) & (v <= 0)) |
                                                                               ((v > 0) & (pv <= 0)))
        seeds.narrow(dim, 0, n - 1).logical_or_(cross)
        seeds.narrow(dim, 1, n - 1).logical_or_(cross)
    dist2 = edt.feature_transform(seeds, max_dist=reach_vox).dist2
    return SearchField(dist2, w.copy(), dims, cap2)


def _compose(w64, t64):
    """Rows 0..2 of W . T for T (B, 4, 4) -> (B, 3, 4) fp64, every entry ((Wi0 T0j + Wi1 T1j) + Wi2 T2j) + Wi3 T3j
    (rule 1: the order is part of the contract, so that the restatement forms the same bits)."""
    w = w64[None, :3, :, None]                                              # (1, 3, 4, 1)
    t = t64[:, None, :, :]                                                  # (B, 1, 4, 4)
    return ((w[:, :, 0] * t[:, :, 0] + w[:, :, 1] * t[:, :, 1]) + w[:, :, 2] * t[:, :, 2]) + w[:, :, 3] * t[:, :, 3]


def pose_table(world2grid, T):
    """Host table of sgnn_register_pose records (rule 1): rows 0..2 of world2grid . T, with world2grid rounded to fp32
    first and the product formed in fp64, then rounded to fp32.  A record with a non-finite entry (in T, in world2grid,
    in the product or after rounding) is NaN all over: every point of it is outside."""
    t64 = _host(T, np.float64)
    if t64.ndim != 3 or t64.shape[1:] != (4, 4):
        raise ValueError('T must be (B, 4, 4), got %s' % (t64.shape,))
    with np.errstate(all='ignore'):
        w32 = _host(world2grid, np.float64).astype(np.float32)
    if w32.shape != (4, 4):
        raise ValueError('world2grid must be (4, 4), got %s' % (w32.shape,))
    w_ok = bool(np.isfinite(w32).all())
    w64 = w32.astype(np.float64)
    nb = t64.shape[0]
    table = np.zeros(nb, dtype=POSE_DTYPE)
    for lo in range(0, nb, _TABLE_BLOCK):
        t = t64[lo:lo + _TABLE_BLOCK]
        with np.errstate(all='ignore'):
            m = _compose(w64, t).reshape(-1, 12)
        ok = np.isfinite(t).all(axis=(1, 2)) & np.isfinite(m).all(axis=1) & w_ok
        table['m'][lo:lo + _TABLE_BLOCK] = _gn.record_rows(m, ok)
    return table


def _check_field(field):
    if not (isinstance(field, SearchField) and torch.is_tensor(field.dist2) and field.dist2.dtype == torch.int32 and
            field.dist2.is_contiguous() and tuple(field.dist2.shape) == tuple(field.dims)):
        raise ValueError('field must be a SearchField of distance_field()')
    dz, dy, dx = (int(v) for v in field.dims)
    if min(dz, dy, dx) < 1 or dz * dy * dx >= 2 ** 31 or int(field.cap2) < 1:
        raise ValueError('field: dims %s, cap2 %s' % (tuple(field.dims), field.cap2))


def _check_score_points(points):
    shape = tuple(int(v) for v in points.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('points must be (P, 3), got %s' % (shape,))
    if shape[0] >= SCORE_MAX_POINTS:
        raise ValueError('%d points in one call (limit %d)' % (shape[0], SCORE_MAX_POINTS - 1))
    return shape[0]


def _inlier2(inlier):
    """floor(inlier^2) in voxels, as edt forms a cap; None: 1 voxel (a choice, not a measurement)."""
    try:
        i2 = edt._cap2(1.0 if inlier is None else inlier)
    except (TypeError, ValueError):
        i2 = -1
    if i2 < 0:
        raise ValueError('inlier must be None or a distance in voxels >= 0 with a square below 2^31, got %r' % (inlier,))
    return i2


def _score_table(pts, field, table, inlier2):
    """The launches: device fp32 points, a host record table -> (B, 3) int64 on the device, MAX_POSES records a launch."""
    _lib.require_gpu()
    dev = field.dist2.device
    nb = int(table.shape[0])
    dz, dy, dx = (int(v) for v in field.dims)
    out = torch.empty((nb, 3), dtype=torch.int64, device=dev)
    for lo in range(0, nb, MAX_POSES):
        part = table[lo:lo + MAX_POSES]
        dev_table = torch.from_numpy(part.view(np.uint8)).to(dev)
        _lib.call('sgnn_register_score', _lib.ptr(pts), int(pts.shape[0]), field.dist2.data_ptr(), dx, dy, dz,
                  dev_table.data_ptr(), int(part.shape[0]), int(field.cap2), inlier2, out[lo:].data_ptr())
    return out


def score(points, field, T, inlier=None):
    """(B, 3) int64 on the device: cost, inliers, outside of every transform T (4, 4) or (B, 4, 4), source world ->
    the field's world, against the SearchField of distance_field (rules 1-5 of section X).  A point costs the squared
    distance, in voxels, from the voxel it rounds to to the nearest surface voxel, at most cap2; it is an inlier where
    that distance is at most `inlier` voxels (None: 1) and outside where it leaves the volume.  More than MAX_POSES
    transforms take several launches."""
    npts = _check_score_points(points)
    t64, _ = _matrices(T, 'T')
    inlier2 = _inlier2(inlier)
    _check_field(field)
    table = pose_table(field.world2grid, t64)
    _lib.require_gpu()
    pts = _to_device(points, torch.float32, field.dist2.device)
    assert int(pts.shape[0]) == npts
    return _score_table(pts, field, table, inlier2)


def _rotation(axis, angle):
    """Rodrigues about a unit axis, entry by entry: (d_ij + sin a K_ij) + (1 - cos a) (u_i u_j - d_ij); sine and cosine
    are math.sin and math.cos of the fp64 angle.  An angle of 0 gives the identity exactly."""
    u = [float(v) for v in axis]
    s, v = math.sin(angle), 1.0 - math.cos(angle)
    k = [[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]]
    return np.array([[((1.0 if i == j else 0.0) + s * k[i][j]) + v * (u[i] * u[j] - (1.0 if i == j else 0.0))
                      for j in range(3)] for i in range(3)], np.float64)


def _mul3(a, b):
    """a . b for (..., 3, 3) fp64, every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j."""
    a, b = a[..., :, :, None], b[..., None, :, :]
    return (a[..., 0, :] * b[..., 0, :] + a[..., 1, :] * b[..., 1, :]) + a[..., 2, :] * b[..., 2, :]


def _apply3(r, c):
    """r . c for r (..., 3, 3), c (3,): (r_i0 c0 + r_i1 c1) + r_i2 c2."""
    return (r[..., 0] * c[0] + r[..., 1] * c[1]) + r[..., 2] * c[2]


def _poses(rot, centre_to, c):
    """(B, 4, 4) fp64: the transforms that turn by rot (B, 3, 3) and take the centroid c to centre_to (B, 3):
    t = centre_to - rot . c."""
    t = np.zeros(rot.shape[:-2] + (4, 4), np.float64)
    t[..., :3, :3] = rot
    t[..., :3, 3] = centre_to - _apply3(rot, c)
    t[..., 3, 3] = 1.0
    return t


def _unit(up):
    u = _host(up, np.float64)
    if u.shape != (3,) or not np.isfinite(u).all():
        raise ValueError('up must be three finite numbers, got %r' % (up,))
    n = math.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    if not n > 0:
        raise ValueError('up must not be zero')
    return u / n


def lattice(dims, world2grid, step=None, up=(0, 0, 1), z_range=None):
    """The level-0 lattice of a destination volume -> (origin (3,) fp64, counts (3,) ints, pitch), x, y, z.  The world
    box is the smallest axis-aligned box around the volume's 8 corner voxel centres taken through inv(world2grid) (fp64
    inverse of the fp32 matrix); position k of axis a is origin_a + k * pitch, k = 0 .. floor((hi_a - lo_a) / pitch).
    pitch None: 4 voxels, a voxel being 1 / |row 0 of world2grid's 3x3| (a choice, not a measurement).  z_range
    (lo, hi) replaces the span of the world axis on which `up` has its largest component.  Host only."""
    w = _invertible(world2grid, 'world2grid', np.float32).astype(np.float64)
    inv = np.linalg.inv(w)
    dz, dy, dx = (int(v) for v in dims)
    corners = np.array([[i * (dx - 1), j * (dy - 1), k * (dz - 1), 1.0] for k in (0, 1) for j in (0, 1)
                        for i in (0, 1)], np.float64)
    world = np.stack([_apply3(inv[:3, :3], g[:3]) + inv[:3, 3] for g in corners])
    lo, hi = world.min(0), world.max(0)
    if step is None:
        pitch = 4.0 / math.sqrt((w[0, 0] * w[0, 0] + w[0, 1] * w[0, 1]) + w[0, 2] * w[0, 2])
    else:
        pitch = _positive('step', step)
    if z_range is not None:
        z = _host(z_range, np.float64)
        if z.shape != (2,) or not np.isfinite(z).all() or z[1] < z[0]:
            raise ValueError('z_range must be (lo, hi) with lo <= hi, got %r' % (z_range,))
        a = int(np.argmax(np.abs(_unit(up))))
        lo[a], hi[a] = z[0], z[1]
    counts = tuple(int(math.floor((hi[a] - lo[a]) / pitch)) + 1 for a in range(3))
    return lo, counts, pitch


def select(cost_order, decode, top, cyclic=0):
    """The selection rule: walk candidate indices in ascending (cost, index) order and keep one unless a kept one has
    the same or an adjacent rotation index (with cyclic = Nr, index 0 and Nr - 1 are adjacent too) and a lattice
    position within one pitch on every axis; stop at `top` -> the kept indices.  decode(index) -> (r, kz, ky, kx)."""
    kept, where = [], []
    for i in cost_order:
        r, kz, ky, kx = decode(int(i))
        for q, qz, qy, qx in where:
            dr = abs(r - q)
            near = dr <= 1 or (cyclic > 1 and dr == cyclic - 1)
            if near and abs(kz - qz) <= 1 and abs(ky - qy) <= 1 and abs(kx - qx) <= 1:
                break
        else:
            kept.append(int(i))
            where.append((r, kz, ky, kx))
            if len(kept) == top:
                break
    return kept


def _neighbourhood(axis, delta, tilt):
    """The rotations of a refinement level, slowest first -> (3, 3, 3) about `axis`, or with tilt (27, 3, 3): about the
    world axes, Rz(az) . (Ry(ay) . Rx(ax)) with ax slowest; every angle runs over -delta, 0, +delta."""
    angles = (-delta, 0.0, delta)
    if not tilt:
        return np.stack([_rotation(axis, a) for a in angles])
    ex, ey, ez = np.eye(3)
    return np.stack([_mul3(_rotation(ez, az), _mul3(_rotation(ey, ay), _rotation(ex, ax)))
                     for ax in angles for ay in angles for az in angles])


_OFFSETS = np.array([[ox, oy, oz] for oz in (-1.0, 0.0, 1.0) for oy in (-1.0, 0.0, 1.0) for ox in (-1.0, 0.0, 1.0)])


def search(points, vol, rotations=None, yaw_step=10.0, up=(0, 0, 1), step=None, z_range=None, reach=None,
           max_points=4096, top=16, levels=4, tilt=False, field=None, trace=None, **align_kwargs):
    """The transform that takes `points` (P, 3), source world, onto the surface of `vol` without a guess ->
    SearchResult.  Both worlds are expected level (upright), so the unknown is a turn about `up` and a shift.

    Level 0 scores, in one launch, every rotation (rotations (Nr, 3, 3), or the ceil(360 / yaw_step) turns of yaw_step
    degrees about up) about the centroid of the scoring points, for every position of the centroid on a lattice of pitch
    `step` (None: 4 destination voxels) over the destination's world box (z_range: the span on the up axis).  The `top`
    best that are no lattice neighbours are kept; `levels` times each moves to the best of its 81 neighbours (729 with
    tilt) at half the pitch and half the angle; align polishes the kept poses from all the points and best chooses.
    Scoring takes every ceil(P / max_points)-th point.  reach: distance_field's; field: a SearchField of `vol` to
    reuse.  trace: None or a dict that receives 'lattice', 'level0' (the (B, 3) scores), 'kept' (per level, 0 first:
    (T (K, 4, 4), scores (K, 3))) and 'guesses'.  The rules are INTEGRATION.md section X."""
    npts = _check_points(points)
    if npts < 1:
        raise ValueError('no points')
    yaw_step = _positive('yaw_step', yaw_step)
    top, levels = _positive('top', top, True), _positive('levels', levels, True)
    max_points = _positive('max_points', max_points, True)
    if step is not None:
        _positive('step', step)
    if reach is not None:
        _positive('reach', reach)
    axis = _unit(up)
    if rotations is None:
        nr = int(math.ceil(360.0 / yaw_step))
        rots = np.stack([_rotation(axis, math.radians(k * yaw_step)) for k in range(nr)])
    else:
        rots = _host(rotations, np.float64)
        if rots.ndim != 3 or rots.shape[1:] != (3, 3) or rots.shape[0] < 1 or not np.isfinite(rots).all():
            raise ValueError('rotations must be (Nr, 3, 3), finite, Nr >= 1, got %s' % (rots.shape,))
        nr = rots.shape[0]
    if field is None:
        _, dims, _, _ = _field_volume(vol, reach)
        world2grid = vol.world2grid if isinstance(vol, fusion.TSDFVolume) else vol[1]
    else:
        _check_field(field)
        dims, world2grid = tuple(field.dims), field.world2grid
    origin, counts, pitch = lattice(dims, world2grid, step, axis, z_range)
    nx, ny, nz = counts
    total = nr * nz * ny * nx
    if total > MAX_POSES * MAX_LAUNCHES:
        raise ValueError('level 0 has %d poses (%d rotations x %d x %d x %d positions); the limit is %d: raise step or '
                         'yaw_step, or give z_range' % (total, nr, nz, ny, nx, MAX_POSES * MAX_LAUNCHES))

    # from here on a device is needed
    if field is None:
        field = distance_field(vol, reach)
    dev = field.dist2.device
    pts_all = _to_device(points, torch.float32, dev)
    pts = pts_all[::-(-npts // max_points)].contiguous()
    host_pts = pts.cpu().numpy().astype(np.float64)
    host_pts = np.ascontiguousarray(host_pts[np.isfinite(host_pts).all(axis=1)])
    if host_pts.shape[0] == 0:
        raise ValueError('no finite scoring point')
    c = host_pts.sum(axis=0) / host_pts.shape[0]
    inlier2 = _inlier2(None)

    # level 0: rotation slowest, then z, y, x
    rc = _apply3(rots, c)                                                   # (Nr, 3)
    table = np.zeros(total, dtype=POSE_DTYPE)
    for lo in range(0, total, _TABLE_BLOCK):
        i = np.arange(lo, min(lo + _TABLE_BLOCK, total), dtype=np.int64)
        k = np.stack([i % nx, (i // nx) % ny, (i // (nx * ny)) % nz], 1).astype(np.float64)
        r = i // (nx * ny * nz)
        table[lo:lo + _TABLE_BLOCK] = pose_table(field.world2grid, _poses(rots[r], origin + k * pitch, c))
    scores0 = _score_table(pts, field, table, inlier2)
    del table

    def decode(i):
        return i // (nx * ny * nz), (i // (nx * ny)) % nz, (i // nx) % ny, i % nx

    order = torch.sort(scores0[:, 0], stable=True).indices                  # ascending (cost, index)
    kept, taken = [], 0
    while len(kept) < top and taken < total:                                # the walk seldom needs more than a few
        taken = min(total, max(4096, 4 * taken))
        kept = select(order[:taken].cpu().numpy(), decode, top, nr if rotations is None else 0)
    picked = np.array(kept, np.int64)
    rot = rots[picked // (nx * ny * nz)]                                    # the kept poses as (rotation, centre)
    centre = origin + np.stack([picked % nx, (picked // nx) % ny, (picked // (nx * ny)) % nz], 1).astype(np.float64) * pitch
    kept_scores = scores0[torch.from_numpy(picked).to(dev)].cpu().numpy()
    if trace is not None:
        trace.update(lattice=(origin, counts, pitch), level0=scores0, kept=[(_poses(rot, centre, c), kept_scores)])

    # levels 1..levels: each kept pose moves to the best of its neighbourhood at half the pitch and half the angle
    nk = len(kept)
    for level in range(1, levels + 1):
        s, delta = pitch / 2.0 ** level, math.radians(yaw_step) / 2.0 ** level
        turns = _neighbourhood(axis, delta, tilt)                           # (n_rot, 3, 3)
        n_rot = turns.shape[0]
        cand_rot = _mul3(turns[None, :], rot[:, None])                      # (K, n_rot, 3, 3): D . R
        cand_rot = np.broadcast_to(cand_rot[:, :, None], (nk, n_rot, 27, 3, 3))
        cand_centre = np.broadcast_to((centre[:, None] + _OFFSETS[None] * s)[:, None], (nk, n_rot, 27, 3))
        hood = n_rot * 27
        T = _poses(cand_rot.reshape(-1, 3, 3), cand_centre.reshape(-1, 3), c)
        sc = _score_table(pts, field, pose_table(field.world2grid, T), inlier2).cpu().numpy().reshape(nk, hood, 3)
        pick = sc[:, :, 0].argmin(axis=1)                                   # the first minimum: (cost, index)
        rows = np.arange(nk)
        rot = cand_rot.reshape(nk, hood, 3, 3)[rows, pick]
        centre = cand_centre.reshape(nk, hood, 3)[rows, pick]
        kept_scores = sc[rows, pick]
        if trace is not None:
            trace['kept'].append((_poses(rot, centre, c), kept_scores))

    guesses = _poses(rot, centre, c)
    if trace is not None:
        trace['guesses'] = guesses.copy()
    results = align(pts_all, vol, guess=guesses, **align_kwargs)
    chosen = best(results)
    candidates = [(guesses[k].copy(),) + tuple(int(v) for v in kept_scores[k]) for k in range(nk)]
    if chosen is None:
        return SearchResult(np.eye(4), False, None, candidates, field)
    return SearchResult(chosen.T.copy(), True, chosen, candidates, field)


def search_volumes(src_vol, dst_vol, stride=2, **kwargs):
    """search(surface_points(src_vol, stride=stride), dst_vol, **kwargs): the transform from the world of one
    fusion.TSDFVolume to that of another, without a guess."""
    if not isinstance(src_vol, fusion.TSDFVolume):
        raise ValueError('src_vol must be a fusion.TSDFVolume')
    return search(surface_points(src_vol, stride=stride), dst_vol, **kwargs)
