"""The gravity-aligned room frame of a scan volume: the matrix that regrid.grid_for(vol, world_transform=) takes.

A sequence tracked with track.track_sequence lives in the frame of its first camera, tilted by whatever the hand did;
the chunk cutter, the height clamp of the data layer and the network all take z for the up axis and the walls for x
and y.  The volume already holds the answer: its surface normals cluster on the floor / ceiling direction and on two
wall directions, and a TSDF gives a normal per surface voxel by central differences, with no search.  The rules are
INTEGRATION.md section S; that text is the contract of the kernels (sgnn_amd/csrc/upright.hip) and of the independent
NumPy restatement of the tests (tests/upright_ref.py).

    hint = hint_from_poses(cam2world)                         # cameras look x right, y down: up is about -y
    res = find(vol, up_hint=hint)                             # UprightResult: R, up, yaw, floor, ceiling, votes, ok
    T = transform(res, floor_at=0.0)                          # (4, 4) fp64: old world -> upright world
    dims, w2g = regrid.grid_for(vol, world_transform=T, pad=2)
    level = regrid.resample(vol, dims, w2g)                   # the upright volume; poses become T @ cam2world
    level, T, res = straighten(vol, up_hint=hint)             # the four lines above in one call

The device counts: a cube-map histogram of the normals (normal_histogram), fixed-point sums of the normals inside a
cone about a candidate axis and of the 4-fold angle of the wall normals (axis_sums), and histograms of the heights of
the floor- and ceiling-facing voxels (height_histogram).  Every device result is an integer, so it depends on no launch
detail.  The peak search, the cone iteration, the yaw and the levels are host arithmetic in fp64 on those integers
(solve), a few kilobytes per pass.
"""
import collections
import math

import numpy as np
import torch

from . import _lib, fusion, regrid
from ._glue import (host as _host, invertible as _invertible, positive as _gate, source_device as _source_device,
                    to_device as _to_device)
from ._gn import record_rows as _record_rows

# struct sgnn_upright_axis (include/sgnn_hip.h)
AXIS_DTYPE = np.dtype([('u', '<f4', (3,)), ('e1', '<f4', (3,)), ('e2', '<f4', (3,)), ('cos_cone', '<f4'),
                       ('sin_wall', '<f4'), ('pad', '<f4', (1,))])
assert AXIS_DTYPE.itemsize == 48

BINS = (8, 16, 32)
MAX_HEIGHT_BINS = 4096      # SGNN_UPRIGHT_MAX_HEIGHT_BINS
MAX_RECORDS = 65535
FIX = float(2 ** 20)        # the fixed point of the sums

UprightResult = collections.namedtuple('UprightResult', 'R up yaw yaw_confidence floor ceiling votes ok yaw_ok')
UprightResult.__doc__ = """What find() found: R (3, 3) fp64 whose rows are the new x, y, z axes in the old world
(right-handed, det +1; the identity when ok is false), up = R[2], yaw (radians, the turn about up from the old x axis
projected off up to the new x axis; 0 when yaw_ok is false) and its confidence in [0, 1], floor and ceiling: heights
along up in metres (None where no such level was seen), votes: the up-facing, down-facing and wall counts of the last
pass, ok, yaw_ok."""


# ---------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------
def _volume(vol):
    """(sdf, world2grid, voxel_size) of a fusion.TSDFVolume or of such a triple."""
    if isinstance(vol, fusion.TSDFVolume):
        return vol.sdf(), vol.world2grid, vol.voxel_size
    try:
        sdf, world2grid, voxel_size = vol
    except (TypeError, ValueError):
        raise ValueError('vol must be a fusion.TSDFVolume or (sdf, world2grid, voxel_size)')
    return sdf, world2grid, voxel_size


def _check_sdf(sdf):
    shape = tuple(int(v) for v in getattr(sdf, 'shape', ()))
    if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('sdf must be (Z, Y, X) with fewer than 2^31 voxels, got %s' % (shape,))
    return shape[::-1]


def grid_matrices(world2grid):
    """(world2grid, grid2world), each rows 0..2 as (3, 4) fp32: the matrix as given, and its inverse formed in fp64 from
    the fp32 matrix and rounded once (rule S.1)."""
    w = _invertible(world2grid, 'world2grid', np.float32)
    with np.errstate(all='ignore'):
        inv = np.linalg.inv(w.astype(np.float64)).astype(np.float32)
    if not np.isfinite(inv).all():
        raise ValueError('world2grid must be an invertible (4, 4) matrix')
    return np.ascontiguousarray(w[:3]), np.ascontiguousarray(inv[:3])


def _unit(v, name):
    v = _host(v, np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0:
        raise ValueError('%s must be a non-zero vector of 3 finite numbers' % name)
    return v / np.linalg.norm(v)


def _bins(bins):
    if bins not in BINS:
        raise ValueError('bins must be one of %s, got %r' % (BINS, bins))
    return int(bins)


def axis_table(u, e1, e2, cos_cone, sin_wall):
    """Host table of sgnn_upright_axis records (rule S.4) from (B, 3) or (3,) axes and frames and B or one cone cosine
    and wall sine, rounded to fp32.  A record with a non-finite entry (in fp64 or after rounding) is NaN all over: it
    stays empty."""
    u64, a64, b64 = (_host(v, np.float64).reshape(-1, 3) for v in (u, e1, e2))
    nb = u64.shape[0]
    if a64.shape[0] != nb or b64.shape[0] != nb:
        raise ValueError('u, e1 and e2 must have the same number of rows')
    c64 = np.broadcast_to(_host(cos_cone, np.float64).reshape(-1), (nb,))
    s64 = np.broadcast_to(_host(sin_wall, np.float64).reshape(-1), (nb,))
    flat = _record_rows(np.concatenate([u64, a64, b64, c64[:, None], s64[:, None]], 1))
    table = np.zeros(nb, dtype=AXIS_DTYPE)
    table['u'], table['e1'], table['e2'] = flat[:, 0:3], flat[:, 3:6], flat[:, 6:9]
    table['cos_cone'], table['sin_wall'] = flat[:, 9], flat[:, 10]
    return table


# ---------------------------------------------------------------------------------------------------------
# the three device passes
# ---------------------------------------------------------------------------------------------------------
class _Passes(object):
    """The three launches against one volume: what solve() asks for, answered by the device."""

    def __init__(self, sdf, world2grid, band, surface):
        self.dims = _check_sdf(sdf)
        self.w2g, self.g2w = grid_matrices(world2grid)
        self.band, self.surface = _gate('band', band), _gate('surface', surface)
        self.dev = _source_device(sdf)
        self.sdf = _to_device(sdf, torch.float32, self.dev)

    def _head(self):
        return (self.sdf.data_ptr(),) + self.dims + (self.w2g.ctypes.data,)

    def histogram(self, bins):
        out = torch.zeros((6, bins, bins), dtype=torch.int32, device=self.dev)
        _lib.call('sgnn_upright_histogram', *self._head(), float(self.band), float(self.surface), bins, out.data_ptr())
        return out

    def sums(self, table):
        nb = int(table.shape[0])
        out = torch.zeros((nb, 8), dtype=torch.int64, device=self.dev)
        if nb:
            dev_table = torch.from_numpy(table.view(np.uint8)).to(self.dev)
            _lib.call('sgnn_upright_sums', *self._head(), float(self.band), float(self.surface), dev_table.data_ptr(), nb,
                      out.data_ptr())
        return out

    def heights(self, up, cos_cone, h0, bin_size, nbins):
        out = torch.zeros((2, nbins), dtype=torch.int32, device=self.dev)
        _lib.call('sgnn_upright_heights', *self._head(), self.g2w.ctypes.data, float(self.band), float(self.surface),
                  up.ctypes.data, float(cos_cone), float(h0), float(bin_size), nbins, out.data_ptr())
        return out


def normal_histogram(sdf, world2grid, band, surface, bins=16):
    """The cube-map histogram of the surface normals of an sdf (Z, Y, X) -> (6, bins, bins) int32 on the device (rules
    S.1, S.2).  band, surface: the gates of a surface voxel, in the sdf's unit.  numpy arrays or torch tensors, host or
    device."""
    bins = _bins(bins)
    return _Passes(sdf, world2grid, band, surface).histogram(bins)


def axis_sums(sdf, world2grid, band, surface, records):
    """The sums of rule S.4 for every record of an axis_table (or an array of AXIS_DTYPE) -> (B, 8) int64 on the
    device: the fixed-point sums x, y, z of the folded normals inside the cone, n_up, n_down, the fixed-point sums of
    cos 4a and sin 4a of the wall normals, n_wall.  Every record runs against the same volume in one launch."""
    table = np.ascontiguousarray(records)
    if table.dtype != AXIS_DTYPE or table.ndim != 1:
        raise ValueError('records must be a one-dimensional array of upright.AXIS_DTYPE (axis_table makes one)')
    if table.shape[0] > MAX_RECORDS:
        raise ValueError('more than %d records in one call' % MAX_RECORDS)
    return _Passes(sdf, world2grid, band, surface).sums(table)


def _height_args(up, cos_cone, h0, bin_size, nbins):
    up = np.ascontiguousarray(_host(up, np.float32).reshape(-1))
    cos_cone, h0, bin_size = np.float32(cos_cone), np.float32(h0), np.float32(bin_size)
    if up.shape != (3,) or not np.isfinite(up).all():
        raise ValueError('up must be 3 finite numbers')
    if not (cos_cone > 0 and np.isfinite(cos_cone) and np.isfinite(h0) and bin_size > 0 and np.isfinite(bin_size)):
        raise ValueError('cos_cone and bin must be positive, h0 finite')
    if not 1 <= int(nbins) <= MAX_HEIGHT_BINS:
        raise ValueError('nbins must be 1 .. %d' % MAX_HEIGHT_BINS)
    return up, cos_cone, h0, bin_size, int(nbins)


def height_histogram(sdf, world2grid, band, surface, up, cos_cone, h0, bin, nbins):
    """The heights along `up` of the up-facing (row 0) and down-facing (row 1) surface voxels, each carried to the zero
    crossing along its normal -> (2, nbins) int32 on the device (rule S.5): bin floor((h - h0) / bin)."""
    args = _height_args(up, cos_cone, h0, bin, nbins)
    return _Passes(sdf, world2grid, band, surface).heights(*args)


# ---------------------------------------------------------------------------------------------------------
# host arithmetic on the integers (fp64)
# ---------------------------------------------------------------------------------------------------------
def bin_centres(bins):
    """(6 * bins * bins, 3) fp64: the unit vector through the centre of every cell of the cube map, in bin order."""
    bins = _bins(bins)
    f, iv, iu = np.meshgrid(np.arange(6), np.arange(bins), np.arange(bins), indexing='ij')
    f, a, b = f.ravel(), (iu.ravel() + 0.5) * (2.0 / bins) - 1.0, (iv.ravel() + 0.5) * (2.0 / bins) - 1.0
    out = np.zeros((f.size, 3))
    rows = np.arange(f.size)
    axis = f // 2
    out[rows, axis] = np.where(f % 2 == 1, -1.0, 1.0)
    out[rows, (axis + 1) % 3] = a
    out[rows, (axis + 2) % 3] = b
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def peak(hist, up_hint=None, max_tilt=45.0):
    """The bin the cone iteration starts from (rule S.3) -> its index in the flattened histogram, or None when no
    eligible bin has a vote.  With a hint: the bin of greatest count among those whose centre lies within max_tilt
    degrees of the hint.  Without: the bin of greatest count + count of the bin that holds the opposite centre; the two
    bins of a pair tie, so the lower one, on the positive half of its axis, is taken.  That is a guess (the largest
    pair of facing flat areas is usually floor and ceiling, and nothing tells which of the two is the floor), not a
    measurement.  Ties go to the lowest index."""
    h = _host(hist, np.int64)
    if h.ndim != 3 or h.shape[0] != 6 or h.shape[1] != h.shape[2]:
        raise ValueError('hist must be (6, bins, bins), got %s' % (h.shape,))
    bins = _bins(h.shape[1])
    if up_hint is None:
        score = h + h.reshape(3, 2, bins, bins)[:, ::-1, ::-1, ::-1].reshape(6, bins, bins)
        score = score.ravel()
    else:
        hint = _unit(up_hint, 'up_hint')
        if not 0 < float(max_tilt) <= 180:
            raise ValueError('max_tilt must be in (0, 180] degrees')
        eligible = bin_centres(bins) @ hint >= math.cos(math.radians(float(max_tilt)))
        score = np.where(eligible, h.ravel(), 0)
    best = int(np.argmax(score))
    return best if score[best] > 0 else None


def plane_frame(up):
    """(e1, e2) fp64 of rule S.4: the old world x axis (the y axis when |x . up| > 0.9) projected off up and
    normalised, and up x e1."""
    up = _unit(up, 'up')
    base = np.array([0.0, 1.0, 0.0]) if abs(up[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = base - (base @ up) * up
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(up, e1)


def height_bins(dims_xyz, world2grid, up, voxel_size):
    """(h0, bin, nbins) of rule S.5 for a grid: the heights along up of the 8 grid corners (fp64) span [lo, hi]; bin =
    voxel_size / 2, doubled until ceil((hi - lo) / bin) + 5 <= 4096; h0 = lo - 2 bin.  h0 and bin are fp32."""
    _, g2w = grid_matrices(world2grid)
    top = np.array(dims_xyz, np.float64) - 1.0
    corners = np.array([[(c >> a & 1) * top[a] for a in range(3)] for c in range(8)])
    h = (corners @ g2w[:, :3].astype(np.float64).T + g2w[:, 3].astype(np.float64)) @ _unit(up, 'up')
    lo, hi = float(h.min()), float(h.max())
    size = np.float32(voxel_size) * np.float32(0.5)
    if not (size > 0 and np.isfinite(size)):
        raise ValueError('voxel_size must be positive')
    while math.ceil((hi - lo) / float(size)) + 5 > MAX_HEIGHT_BINS:
        size = size * np.float32(2.0)
    return np.float32(lo - 2.0 * float(size)), size, int(math.ceil((hi - lo) / float(size)) + 5)


def level(row, h0, bin_size, share, from_top=False):
    """The first bin k from the bottom (from the top: from_top) with row[k] >= share * max(row), refined to the
    count-weighted mean of the centres of bins k - 1 .. k + 1 -> a height (fp64), or None for an empty row."""
    row = _host(row, np.int64)
    if row.max(initial=0) <= 0:
        return None
    hits = np.nonzero(row >= share * row.max())[0]
    k = int(hits[-1] if from_top else hits[0])
    ks = np.arange(max(k - 1, 0), min(k + 2, len(row)))
    centres = float(h0) + (ks + 0.5) * float(bin_size)
    return float((centres * row[ks]).sum() / row[ks].sum())


def _failed(votes=(0, 0, 0)):
    return UprightResult(np.eye(3), np.array([0.0, 0.0, 1.0]), 0.0, 0.0, None, None, tuple(int(v) for v in votes), False,
                         False)


def solve(passes, dims_xyz, world2grid, voxel_size, up_hint=None, max_tilt=45.0, cones=(20.0, 10.0, 5.0),
          wall_tol=10.0, bins=16, min_votes=256, floor_share=0.25):
    """find() on the integers that `passes` hands out: an object with histogram(bins) -> (6, bins, bins),
    sums(table) -> (B, 8) and heights(up (3,) fp32, cos_cone, h0, bin, nbins) -> (2, nbins), arrays or tensors.  find()
    passes the device; the tests pass the NumPy restatement, and the two agree bit for bit because the passes do."""
    bins = _bins(bins)
    cones = [float(c) for c in (cones if np.ndim(cones) else [cones])]
    if not cones or not all(0 < c < 90 for c in cones):
        raise ValueError('cones must be angles in (0, 90) degrees')
    if not 0 <= float(wall_tol) < 90:
        raise ValueError('wall_tol must be in [0, 90) degrees')
    if int(min_votes) < 1 or not 0 < float(floor_share) <= 1:
        raise ValueError('min_votes must be at least 1 and floor_share in (0, 1]')
    if up_hint is not None:
        _unit(up_hint, 'up_hint')
    if not 0 < float(max_tilt) <= 180:
        raise ValueError('max_tilt must be in (0, 180] degrees')
    grid_matrices(world2grid)
    start = peak(passes.histogram(bins), up_hint, max_tilt)
    if start is None:
        return _failed()
    up = bin_centres(bins)[start]
    cosines = [np.float32(math.cos(math.radians(c))) for c in cones]
    for cos_cone in cosines:
        e1, e2 = plane_frame(up)
        s = _host(passes.sums(axis_table(up, e1, e2, cos_cone, -1.0)), np.int64)[0]
        vec = s[:3].astype(np.float64)
        if s[3] + s[4] == 0 or not np.linalg.norm(vec) > 0:
            return _failed()
        up = vec / np.linalg.norm(vec)
    e1, e2 = plane_frame(up)
    sin_wall = np.float32(math.sin(math.radians(float(wall_tol))))
    s = _host(passes.sums(axis_table(up, e1, e2, cosines[-1], sin_wall)), np.int64)[0]
    votes = (int(s[3]), int(s[4]), int(s[7]))
    if votes[0] + votes[1] < int(min_votes):
        return _failed(votes)
    yaw, confidence, yaw_ok = 0.0, 0.0, False
    if votes[2] > 0:
        confidence = math.hypot(float(s[5]), float(s[6])) / (votes[2] * FIX)
        yaw_ok = votes[2] >= int(min_votes) and confidence >= 0.2
        if yaw_ok:
            yaw = math.atan2(float(s[6]), float(s[5])) / 4.0
    new_x = math.cos(yaw) * e1 + math.sin(yaw) * e2
    R = np.stack([new_x, np.cross(up, new_x), up])
    h0, size, nbins = height_bins(dims_xyz, world2grid, up, voxel_size)
    rows = _host(passes.heights(up.astype(np.float32), cosines[-1], h0, size, nbins), np.int64)
    floor = level(rows[0], h0, size, float(floor_share))
    ceiling = level(rows[1], h0, size, float(floor_share), from_top=True)
    if ceiling is not None and floor is not None and ceiling <= floor:
        ceiling = None
    return UprightResult(R, up, yaw, confidence, floor, ceiling, votes, True, yaw_ok)


# ---------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------
def hint_from_poses(cam2world):
    """-(mean of the cameras' y axes), normalised -> (3,) fp64: cameras look x right, y down, and a hand-held camera is
    level on average.  cam2world: (4, 4) or (F, 4, 4)."""
    c = _host(cam2world, np.float64)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[1:] != (4, 4) or c.shape[0] == 0:
        raise ValueError('cam2world must be (4, 4) or (F, 4, 4), got %s' % (c.shape,))
    return _unit(-c[:, :3, 1].mean(0), 'the mean of the cameras\' y axes')


def find(vol, up_hint=None, max_tilt=45.0, cones=(20.0, 10.0, 5.0), wall_tol=10.0, bins=16, band=None, surface=None,
         min_votes=256, floor_share=0.25):
    """The upright frame of a volume -> UprightResult.

    vol: a fusion.TSDFVolume or (sdf (Z, Y, X) in metres, world2grid, voxel_size).  up_hint: a vector within max_tilt
    degrees of the true up (hint_from_poses gives one); None: the largest pair of facing flat areas is taken for floor
    and ceiling, which is a guess.  cones: the half-angles in degrees of the cone means that refine the histogram's
    peak, one launch each.  wall_tol: how far in degrees from horizontal a wall normal may be.  bins: 8, 16 or 32
    cells along a side of a cube-map face.  band (None: 3 voxel sizes) and surface (None: one voxel size): the gates of
    a surface voxel.  ok is false, and R the identity, when no histogram bin within max_tilt of the hint has a vote or
    the last cone holds fewer than min_votes voxels; yaw_ok is false, and yaw 0, with fewer than min_votes wall voxels
    or a confidence below 0.2: the up axis is still good.  floor_share: the share of the fullest height bin that the
    lowest up-facing (highest down-facing) level must reach to be the floor (ceiling)."""
    sdf, world2grid, voxel_size = _volume(vol)
    vs = _gate('voxel_size', voxel_size)
    band = np.float32(3.0) * vs if band is None else band
    surface = vs if surface is None else surface
    passes = _Passes(sdf, world2grid, band, surface)
    return solve(passes, passes.dims, world2grid, vs, up_hint, max_tilt, cones, wall_tol, bins, min_votes, floor_share)


def transform(res, floor_at=0.0):
    """(4, 4) fp64: old world -> upright world (z up, walls along x and y, the floor at z = floor_at).  A rotation by
    res.R and a shift along z; floor_at None, or a result without a floor, leaves the shift out.  Camera poses become
    transform @ cam2world."""
    R = _host(res.R, np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError('res.R must be a finite (3, 3) matrix')
    T = np.eye(4)
    T[:3, :3] = R
    if floor_at is not None and res.floor is not None:
        T[2, 3] = float(floor_at) - float(res.floor)
    return T


def straighten(vol, up_hint=None, pad=2, mode='linear', floor_at=0.0, **find_kwargs):
    """find, transform, regrid.grid_for and regrid.resample in one call -> (the upright fusion.TSDFVolume, T, the
    UprightResult).  vol: a fusion.TSDFVolume.  With res.ok false T is the identity and the volume is only padded."""
    if not isinstance(vol, fusion.TSDFVolume):
        raise ValueError('vol must be a fusion.TSDFVolume')
    res = find(vol, up_hint=up_hint, **find_kwargs)
    T = transform(res, floor_at)
    dims, w2g = regrid.grid_for(vol, world_transform=T, pad=pad)
    return regrid.resample(vol, dims, w2g, mode=mode), T, res
