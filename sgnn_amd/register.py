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

A guess is required (None is the identity): there is no global search.  The device builds the Gauss-Newton systems; the
6x6 solve and the update of the transform are track.solve_step and track.se3_exp, on the host in fp64.
"""
import collections

import numpy as np
import torch

from . import _gn, _lib, fusion  # noqa: F401  (_lib: the tests count launches through it)
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
