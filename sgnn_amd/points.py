"""Point clouds with known sensor positions -> scan volumes: the third entrance next to depth frames (fusion) and
triangle meshes (voxelize), for tripod and LiDAR sweeps, registered scanner exports and the points of a
photogrammetry or SLAM map.

    pts, cols = load_ply_points('sweep.ply')                 # vertices (+ colours) of a PLY with or without faces
    dims, world2grid = grid_for(pts, 0.02, pad=8)            # axis-aligned grid around the cloud
    vol = fusion.TSDFVolume(dims, 0.02, world2grid, depth_max=12.0, color=True)
    integrate(vol, pts, origins, origin_id=None, color=cols, carve=True)        # returns vol
    pyr = fusion.TSDFPyramid(dims, 0.02, world2grid); integrate(pyr, pts, origins)   # every level, level voxel size
    pts, origins, origin_id = from_depth(depth, K, cam2world)   # back-projected frames as rays

Every ray origin -> point is sampled each half voxel; a sample's voxel gets the signed distance of its centre along the
ray, free space in front of the point is carved, and one call is ONE observation per voxel, folded into the volume's
running mean the way a depth frame is.  The rules are INTEGRATION.md section P; the kernels (csrc/points.hip) and the
independent NumPy restatement of the tests (tests/points_ref.py) both follow that text.  The per-sample sums are
integers added with atomics, so the result depends neither on the order of the points nor on `chunk`.

Two documented deviations from the frame route: a ray is gated by its RANGE |p - o| against the volume's depth_min /
depth_max (a frame by its z-depth), and the half-voxel walk is no full voxel traversal: it can miss a voxel that the
ray only clips at a corner.
"""
import numpy as np
import torch

from . import _lib, fusion, render
from ._glue import host as _host, to_device as _to_device

MAX_RAYS = 1 << 28              # SGNN_POINTS_MAX_RAYS: the 32-bit weight sums of a call cannot overflow below it
MAX_SAMPLES_PER_RAY = 1 << 24   # the sample index is exact in fp32 below it


def load_ply_points(path):
    """(points (V, 3) fp32, colors (V, 3) uint8 or None) of a binary little-endian PLY, with or without a face element:
    the vertices through render.load_ply's parser, the colours from uchar red, green, blue where the file has them."""
    v, vprops, _ = render._read_ply(path, need_faces=False)
    pts = np.stack([v['x'], v['y'], v['z']], 1).astype(np.float32).reshape(-1, 3)
    types = dict(vprops)
    if all(types.get(c) in ('uchar', 'uint8') for c in ('red', 'green', 'blue')):
        return pts, np.stack([v['red'], v['green'], v['blue']], 1).astype(np.uint8).reshape(-1, 3)
    return pts, None


def grid_for(points, voxel_size, pad=8):
    """(dims_xyz, world2grid (4, 4) fp64) of an axis-aligned grid around the finite points: voxel coordinates are
    world / voxel_size - lo.  Rounding rule, in fp64: lo = floor(min / voxel_size) - pad and hi = ceil(max / voxel_size)
    + pad per axis, dims = hi - lo + 1; the cloud therefore lies at least `pad` voxels inside every face.  The matrix is
    rounded to fp32 by the volume that takes it."""
    p = _host(points, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    vs = float(voxel_size)
    if p.shape[0] == 0 or not vs > 0 or int(pad) < 0:
        raise ValueError('grid_for needs at least one finite point, a positive voxel size and pad >= 0')
    lo = np.floor(p.min(0) / vs) - int(pad)
    hi = np.ceil(p.max(0) / vs) + int(pad)
    w2g = np.eye(4, dtype=np.float64)
    w2g[:3, :3] /= vs
    w2g[:3, 3] = -lo
    return tuple(int(d) for d in hi - lo + 1), w2g


def from_depth(depth, intrinsics, cam2world):
    """Depth frames as rays: (points (F h w, 3) fp32, origins (F, 3) fp32, origin_id (F h w,) int32), torch tensors on
    the depth stack's device.  Pixel (u, v) of frame f with depth z goes to cam2world_f . ((u - cx) z / fx,
    (v - cy) z / fy, z) in fp32; a pixel without a finite depth becomes a NaN point, which integrate ignores, so row
    f h w + v w + u is that pixel whatever the frames hold (colours: rgb.reshape(-1, 3))."""
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth))
    d = d.to(torch.float32)
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise ValueError('depth must be (F, h, w) or (h, w), got %s' % (tuple(d.shape),))
    nf, h, w = (int(v) for v in d.shape)
    k = torch.from_numpy(_host(intrinsics, np.float32).reshape(-1, 4)).to(d.device)
    c2w = torch.from_numpy(_host(cam2world, np.float32).reshape(-1, 4, 4)).to(d.device)
    if k.shape[0] != nf or c2w.shape[0] != nf:
        raise ValueError('%d depth frames for %d intrinsics and %d poses' % (nf, k.shape[0], c2w.shape[0]))
    u = torch.arange(w, dtype=torch.float32, device=d.device)[None, None, :]
    v = torch.arange(h, dtype=torch.float32, device=d.device)[None, :, None]
    z = torch.where(torch.isfinite(d), d, torch.full_like(d, float('nan')))
    cam = torch.stack([(u - k[:, 2, None, None]) * z / k[:, 0, None, None],
                       (v - k[:, 3, None, None]) * z / k[:, 1, None, None], z], -1).reshape(nf, h * w, 3)
    pts = cam @ c2w[:, :3, :3].transpose(1, 2) + c2w[:, None, :3, 3]
    oid = torch.arange(nf, dtype=torch.int32, device=d.device)[:, None].expand(nf, h * w)
    return pts.reshape(-1, 3).contiguous(), c2w[:, :3, 3].contiguous(), oid.reshape(-1).contiguous()


def max_samples_per_ray(voxel_size, depth_min, depth_max, carve):
    """An upper bound on rule P.5's N for any ray the volume accepts (fp64, two samples of slack)."""
    vs, dmin, dmax = float(voxel_size), float(depth_min), float(depth_max)
    trunc = 3.0 * vs + dmax * vs
    span = (dmax + trunc - dmin) if carve else 2.0 * trunc
    return int(np.ceil(2.0 * span / vs)) + 3


def _check(volumes, points, origins, origin_id, color):
    """The argument errors, before a device is needed -> (P, S)."""
    shape = tuple(points.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('points must be (P, 3), got %s' % (shape,))
    if tuple(origins.shape)[-1:] != (3,) or len(origins.shape) != 2:
        raise ValueError('origins must be (S, 3), got %s' % (tuple(origins.shape),))
    p, s = int(shape[0]), int(origins.shape[0])
    if p > MAX_RAYS:
        raise ValueError('%d points in one call (at most %d)' % (p, MAX_RAYS))
    if origin_id is None:
        if s != 1:
            raise ValueError('%d origins need an origin_id per point' % s)
    else:
        if tuple(origin_id.shape) != (p,):
            raise ValueError('origin_id %s for %d points' % (tuple(origin_id.shape), p))
        if not (torch.is_tensor(origin_id) and origin_id.is_cuda) and p:
            ids = _host(origin_id, np.int64)
            if ids.min() < 0 or ids.max() >= s:
                raise ValueError('origin_id outside [0, %d)' % s)
    if color is not None:
        cs = tuple(color.shape)
        if len(cs) != 2 or cs[0] != p or cs[1] not in (3, 4):
            raise ValueError('color must be (%d, 3|4), got %s' % (p, cs))
        if color.dtype != (torch.uint8 if torch.is_tensor(color) else np.uint8):
            raise ValueError('color must be uint8')
        if any(v._color is None for v in volumes):
            raise ValueError('point colours for a volume built without color=True')
    for v in volumes:
        if max_samples_per_ray(v.voxel_size, v.depth_min, v.depth_max, True) > MAX_SAMPLES_PER_RAY:
            raise ValueError('depth_max / voxel_size gives more than %d samples on a ray' % MAX_SAMPLES_PER_RAY)
    return p, s


def count_scan(vol, pts, org, oid, carve, r0, r1):
    """Rays r0 .. r1-1: sgnn_points_count and the exclusive scan -> (offsets (n + 1,) int64, box (8,) int32 of those
    rays), both on the device."""
    n = r1 - r0
    counts = torch.empty(max(n, 1), dtype=torch.int32, device=vol.device)
    box = torch.empty(8, dtype=torch.int32, device=vol.device)
    dx, dy, dz = vol.dims_xyz
    _lib.call('sgnn_points_count', pts[r0:].data_ptr(), org.data_ptr(), None if oid is None else oid[r0:].data_ptr(), n,
              int(org.shape[0]), vol.world2grid.ctypes.data, dx, dy, dz, float(vol.voxel_size), float(vol.depth_min),
              float(vol.depth_max), int(bool(carve)), counts.data_ptr(), box.data_ptr())
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=vol.device)
    if n:
        torch.cumsum(counts[:n], 0, out=offsets[1:])
    return offsets, box


def walk(vol, pts, org, oid, col, carve, r0, r1, offsets, box, grid2world, acc):
    """sgnn_points_walk for rays r0 .. r1-1 into the accumulators acc = (acc_s, acc_wf, acc_c or None)."""
    n = r1 - r0
    dx, dy, dz = vol.dims_xyz
    bound = n * max_samples_per_ray(vol.voxel_size, vol.depth_min, vol.depth_max, carve)
    _lib.call('sgnn_points_walk', pts[r0:].data_ptr(), org.data_ptr(), None if oid is None else oid[r0:].data_ptr(),
              None if col is None else col[r0:].data_ptr(), 0 if col is None else int(col.shape[1]), n,
              int(org.shape[0]), offsets.data_ptr(), bound, vol.world2grid.ctypes.data, grid2world.ctypes.data,
              None if vol.obb is None else vol.obb.ctypes.data, dx, dy, dz, float(vol.voxel_size),
              float(vol.depth_min), float(vol.depth_max), int(bool(carve)), box.ctypes.data, acc[0].data_ptr(),
              acc[1].data_ptr(), _lib.ptr(acc[2]))


def fold(vol, box, acc):
    """sgnn_points_fold: the call's accumulators into the volume, one observation per voxel."""
    dx, dy, dz = vol.dims_xyz
    _lib.call('sgnn_points_fold', *vol._state(acc[2] is not None), dx, dy, dz, float(vol.voxel_size), box.ctypes.data,
              acc[0].data_ptr(), acc[1].data_ptr(), _lib.ptr(acc[2]))


def accumulators(vol, box, color):
    """Zeroed scratch for the box (x0, x1, y0, y1, z0, z1): 16 bytes per box voxel, 48 with colour."""
    nb = int(box[1] - box[0] + 1) * int(box[3] - box[2] + 1) * int(box[5] - box[4] + 1)
    return (torch.zeros(nb, dtype=torch.int64, device=vol.device), torch.zeros(nb, dtype=torch.int64, device=vol.device),
            torch.zeros((nb, 4), dtype=torch.int64, device=vol.device) if color else None)


def _integrate_volume(vol, pts, org, oid, col, carve, chunk):
    p = int(pts.shape[0])
    if p == 0:
        return
    grid2world = np.ascontiguousarray(np.linalg.inv(vol.world2grid.astype(np.float64)).astype(np.float32))
    chunk = p if not chunk or int(chunk) <= 0 else min(int(chunk), p)
    # the whole call's box first (the accumulators are sized by it); with one chunk its scan is the walk's scan
    offsets, dev_box = count_scan(vol, pts, org, oid, carve, 0, p)
    box = dev_box.cpu().numpy()                                     # the one read-back of a call
    if box[6] & 1:
        raise ValueError('origin_id outside [0, %d)' % int(org.shape[0]))
    if box[0] > box[1] or box[2] > box[3] or box[4] > box[5]:
        return                                                      # no ray can touch the grid
    box = np.ascontiguousarray(box[:6])
    acc = accumulators(vol, box, col is not None)
    for r0 in range(0, p, chunk):
        r1 = min(r0 + chunk, p)
        if chunk < p:
            offsets, _ = count_scan(vol, pts, org, oid, carve, r0, r1)
        walk(vol, pts, org, oid, col, carve, r0, r1, offsets, box, grid2world, acc)
    fold(vol, box, acc)


def integrate(volume, points, origins, origin_id=None, color=None, carve=True, chunk=None):
    """Fuse the rays origins[origin_id[r]] -> points[r] into a fusion.TSDFVolume, or into every level of a
    fusion.TSDFPyramid, as one observation; returns the volume.

    points (P, 3) and origins (S, 3) world metres, origin_id (P,) integers in [0, S) (None: S == 1), color (P, 3|4)
    uint8 for a volume built with color=True (A == 0 = the point has no colour); numpy or torch, host or device.
    carve: also sample the free space from depth_min on (else only the band around the point).  chunk: rays per walk
    launch (None: all at once); the result does not depend on it.  A ray whose range |p - o| is outside the volume's
    [depth_min, depth_max], or that has a non-finite coordinate, is ignored."""
    volumes = list(volume.volumes) if isinstance(volume, fusion.TSDFPyramid) else [volume]
    points, origins, origin_id, color = (x if x is None or torch.is_tensor(x) else np.asarray(x)
                                         for x in (points, origins, origin_id, color))
    org_in = origins.reshape(1, -1) if len(origins.shape) == 1 else origins      # one origin may come as (3,)
    _check(volumes, points, org_in, origin_id, color)
    _lib.require_gpu()
    dev = volumes[0].device
    pts = _to_device(points, torch.float32, dev)
    org = _to_device(org_in, torch.float32, dev)
    oid = None if origin_id is None else _to_device(origin_id, torch.int32, dev)
    col = None if color is None else _to_device(color, torch.uint8, dev)
    for v in volumes:
        _integrate_volume(v, pts, org, oid, col, carve, chunk)
    return volume
