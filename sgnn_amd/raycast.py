"""TSDF volumes ray-cast to depth and normal frames on the GPU: the way back from a volume to images.

sgnn_amd.render turns a mesh into depth frames and sgnn_amd.fusion turns depth frames into a volume; this module
closes the loop without a mesh in between: a scan volume, a target volume or a prediction seen from any camera pose,
compared in depth space with the frames it was fused from (or with render.render_depth of a ground-truth mesh), or
scanned again for fusion.  The reference project has no counterpart; the rules this follows are listed in
INTEGRATION.md section H, and that text is the contract of the kernels (sgnn_amd/csrc/raycast.hip) and of the
independent NumPy restatement of the tests (tests/raycast_ref.py).

    vol = fusion.TSDFVolume(dims, 0.02, world2grid).integrate(depth, K, poses)
    again = cast_volume(vol, K, poses, (240, 320))                      # (F, h, w) fp32 on the device, -inf = no hit
    depth, normal = cast(sdf, world2grid, vs, K, poses, (240, 320), band, normals=True)
    depth = cast_sparse(locs_zyx, vals, dims_zyx, world2grid, vs, K, poses, (240, 320), band)
    depth, rgba = cast_volume_color(vol, K, poses, (240, 320))          # a TSDFVolume(color=True): colour frames too
    depth, rgba = cast_color(sdf, colors, world2grid, vs, K, poses, (240, 320), band)

The host does per-frame geometry only (one 3x4 matrix per frame).
"""
import numpy as np
import torch

from . import _lib
from ._glue import camera_shapes, cameras, device as _device, host as _host, to_device as _to_device

# struct sgnn_raycast_frame (include/sgnn_hip.h)
FRAME_DTYPE = np.dtype([('g', '<f4', (12,)), ('intr', '<f4', (4,))])
assert FRAME_DTYPE.itemsize == 64

DEFAULT_CHUNK = 0           # frames per launch, 0 = all in one
MAX_SAMPLES = 1 << 20       # per ray


def frame_table(intrinsics, cam2world, world2grid):
    """Host table of sgnn_raycast_frame records (rule 1): rows 0..2 of world2grid . cam2world, formed in fp64 and
    rounded to fp32, and fx, fy, cx, cy.  A pose that is not finite (or whose product is not finite in fp32) gets NaN
    rows: its frame stays empty."""
    k, c2w = cameras(intrinsics, cam2world)
    w2g = _host(world2grid, np.float64).reshape(4, 4)
    t = np.zeros(k.shape[0], dtype=FRAME_DTYPE)
    with np.errstate(all='ignore'):
        g = (w2g @ c2w)[:, :3, :].astype(np.float32)
    g[~np.isfinite(g).all(axis=(1, 2)) | ~np.isfinite(c2w).all(axis=(1, 2))] = np.nan
    t['g'] = g.reshape(-1, 12)
    t['intr'] = k
    return t


def sample_count(depth_min, depth_max, dt):
    """Samples per ray (rule 3): the number of k = 0, 1, .. with depth_min + (float)k * dt <= depth_max, all fp32."""
    f32 = np.float32
    dmin, dmax, dt = f32(depth_min), f32(depth_max), f32(dt)
    est = (float(dmax) - float(dmin)) / float(dt)
    if not est < 4 * MAX_SAMPLES:
        return 4 * MAX_SAMPLES
    at = lambda k: dmin + f32(k) * dt  # noqa: E731
    k = int(est)
    while k < MAX_SAMPLES and at(k + 1) <= dmax:
        k += 1
    while k > 0 and at(k) > dmax:
        k -= 1
    return k + 1


def cast(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, step=0.5, depth_min=0.4, depth_max=4.0,
         normals=False, skip=True, chunk=None, counters=None):
    """z-depth of the zero crossing of a signed-distance volume seen from F cameras -> (F, h, w) fp32 on the device,
    -inf where a ray meets no front-facing crossing; with normals=True also (F, h, w, 3) fp32 unit normals in camera
    space, facing the camera, NaN where there is no hit or no gradient.

    sdf (Z, Y, X) fp32 in any unit, positive in front of surfaces (TSDFVolume.sdf(), marching_cubes.dense_from_sparse),
    band in the same unit: voxels with |sdf| >= band, NaN or an infinity are unknown.  world2grid (4, 4): world metres
    -> voxel coordinates; voxel_size in metres; step: sample spacing in voxels (z-depth); intrinsics (F, 4) fx, fy,
    cx, cy; cam2world (F, 4, 4); numpy arrays or torch tensors, host or device.  skip: pass over empty space through a
    brick table; chunk: frames per launch (None: DEFAULT_CHUNK); the result depends on neither.  counters: None, or a
    device int64 tensor of 2 that receives samples evaluated and samples skipped (measurements)."""
    return _cast(sdf, None, world2grid, voxel_size, intrinsics, cam2world, hw, band, step, depth_min, depth_max, normals,
                 skip, chunk, counters)


def cast_color(sdf, colors, world2grid, voxel_size, intrinsics, cam2world, hw, band, step=0.5, depth_min=0.4,
               depth_max=4.0, normals=False, skip=True, chunk=None, counters=None):
    """cast() of a volume that also has a colour per voxel -> (depth, rgba), or (depth, normal, rgba) with
    normals=True; rgba (F, h, w, 4) uint8 on the device, the layout TSDFVolume.integrate(color=) takes.

    colors (Z, Y, X, 4) uint8 R, G, B, A, A != 0 = the voxel has a colour, or (Z, Y, X, 3), the layout of
    TSDFVolume.colors() and of marching cubes: every voxel then counts as coloured.  At a hit the colour is the
    weighted mean of the coloured corners of the hit's cell with A = 255; a ray without a
    hit, or a hit whose cell has no coloured corner, gets (0, 0, 0, 0).  depth and normal are cast()'s, bit for bit;
    every other argument as cast()."""
    shape = tuple(colors.shape)
    if len(shape) != 4 or shape[:3] != tuple(sdf.shape) or shape[3] not in (3, 4):
        raise ValueError('colors must be (Z, Y, X, 3 | 4) for sdf %s, got %s' % (tuple(sdf.shape), shape))
    return _cast(sdf, colors, world2grid, voxel_size, intrinsics, cam2world, hw, band, step, depth_min, depth_max,
                 normals, skip, chunk, counters)


def _plan(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, step, depth_min, depth_max):
    """The argument checks of every cast, on the host -> ((dz, dy, dx), (h, w), band, depth_min, dt, samples per ray,
    frame table)."""
    if len(tuple(sdf.shape)) != 3:
        raise ValueError('sdf must be (Z, Y, X), got %s' % (tuple(sdf.shape),))
    dz, dy, dx = (int(v) for v in sdf.shape)
    if min(dx, dy, dz) < 1 or max(dx, dy, dz) > 65535:
        raise ValueError('unsupported volume dimensions %s' % ((dz, dy, dx),))
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError('unsupported frame size %s' % ((h, w),))
    f32 = np.float32
    band, step, vs = f32(band), f32(step), f32(voxel_size)
    dmin, dmax = f32(depth_min), f32(depth_max)
    for name, v in (('band', band), ('step', step), ('voxel_size', vs)):
        if not v > 0:
            raise ValueError('%s must be positive' % name)
    if not (np.isfinite(dmin) and np.isfinite(dmax)) or dmax < dmin:
        raise ValueError('depth_min = %s, depth_max = %s is not a range' % (depth_min, depth_max))
    camera_shapes(intrinsics, cam2world)
    table = frame_table(intrinsics, cam2world, world2grid)
    nf = int(table.shape[0])
    if nf * h * w >= 2 ** 31:
        raise ValueError('F h w = %d does not fit 31 bits' % (nf * h * w))
    dt = step * vs                                                       # one fp32 product (rule 3)
    if not (dt > 0 and np.isfinite(dt)):
        raise ValueError('step * voxel_size = %s is not a usable sample spacing' % dt)
    ns = sample_count(dmin, dmax, dt)
    if ns > MAX_SAMPLES:
        raise ValueError('more than %d samples per ray' % MAX_SAMPLES)
    return (dz, dy, dx), (h, w), band, dmin, dt, ns, table


def _cast(sdf, colors, world2grid, voxel_size, intrinsics, cam2world, hw, band, step, depth_min, depth_max, normals,
          skip, chunk, counters):
    dev = _device(next((x.device for x in (sdf, colors) if torch.is_tensor(x) and x.is_cuda), None))
    (dz, dy, dx), (h, w), band, dmin, dt, ns, table = _plan(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band,
                                                            step, depth_min, depth_max)
    nf = int(table.shape[0])
    vol = _to_device(sdf, torch.float32, dev)
    depth = torch.empty((nf, h, w), dtype=torch.float32, device=dev)
    normal = torch.empty((nf, h, w, 3), dtype=torch.float32, device=dev) if normals else None
    rgba = None
    if colors is not None:
        col = _to_device(colors, torch.uint8, dev)
        if col.shape[3] == 3:                                            # every voxel counts as coloured
            col = torch.cat([col, torch.full_like(col[..., :1], 255)], 3).contiguous()
        rgba = torch.empty((nf, h, w, 4), dtype=torch.uint8, device=dev)
    if nf:
        bricks = None
        if skip:
            bricks = torch.empty(((dz + 7) // 8, (dy + 7) // 8, (dx + 7) // 8), dtype=torch.uint8, device=dev)
            _lib.call('sgnn_raycast_bricks', vol.data_ptr(), dx, dy, dz, float(band), bricks.data_ptr())
        dev_table = torch.from_numpy(table.view(np.uint8)).to(dev)
        args = (vol.data_ptr(), dx, dy, dz, float(band), _lib.ptr(bricks), dev_table.data_ptr(), nf,
                int(DEFAULT_CHUNK if chunk is None else chunk), h, w, float(dmin), float(dt), ns, depth.data_ptr(),
                _lib.ptr(normal), _lib.ptr(counters))
        if colors is not None:
            _lib.call('sgnn_raycol_cast', *args, col.data_ptr(), rgba.data_ptr())
        else:
            _lib.call('sgnn_raycast_cast', *args)
    out = (depth, normal) if normals else (depth,)
    if colors is not None:
        return out + (rgba,)
    return out if normals else depth


def cast_volume(vol, intrinsics, cam2world, hw, band=None, **kwargs):
    """cast() of a fusion.TSDFVolume: its sdf in metres, its world2grid and voxel size; band: 3 voxel sizes (one fp32
    product) unless given.  depth_min / depth_max default to cast()'s, not to the volume's."""
    band = np.float32(3.0) * vol.voxel_size if band is None else band
    return cast(vol.sdf(), vol.world2grid, vol.voxel_size, intrinsics, cam2world, hw, band, **kwargs)


def cast_volume_color(vol, intrinsics, cam2world, hw, band=None, **kwargs):
    """cast_color() of a fusion.TSDFVolume(color=True): cast_volume's geometry, colours from vol.colors() with
    A = 255 where vol.color_weight() > 0.  ValueError for a volume without colour."""
    _lib.require_gpu()
    if vol.color_state() is None:
        raise ValueError('the volume has no colour: TSDFVolume(..., color=True)')
    band = np.float32(3.0) * vol.voxel_size if band is None else band
    alpha = (vol.color_weight() > 0).to(torch.uint8) * 255
    rgba = torch.cat([vol.colors(), alpha[..., None]], 3).contiguous()
    return cast_color(vol.sdf(), rgba, vol.world2grid, vol.voxel_size, intrinsics, cam2world, hw, band, **kwargs)


def cast_sparse(locs_zyx, vals, dims_zyx, world2grid, voxel_size, intrinsics, cam2world, hw, band, **kwargs):
    """cast() of sparse rows (locs (N, 3) z, y, x and vals (N,)), through marching_cubes.dense_from_sparse: voxels
    without a row are unknown."""
    from .marching_cubes import dense_from_sparse
    return cast(dense_from_sparse(locs_zyx, vals, dims_zyx), world2grid, voxel_size, intrinsics, cam2world, hw, band,
                **kwargs)


# ---------------------------------------------------------------------------------------------------------
# the differentiable cast
# ---------------------------------------------------------------------------------------------------------
MAX_CHANNELS = 16


def diff_forward(sdf, features, table, hw, band, depth_min, dt, ns, skip=True, chunk=None):
    """sgnn_raygrad_cast on device tensors: sdf (Z, Y, X) fp32, features (Z, Y, X, C) fp32 or None, table the
    device bytes of frame_table() -> (depth, hit, feat or None, ok as uint8).  hit (F, h, w) int32 is the record the
    backward takes: the sample index of each pixel's hit, -1 = none."""
    dz, dy, dx = (int(v) for v in sdf.shape)
    nf, (h, w) = int(table.numel()) // FRAME_DTYPE.itemsize, hw
    dev, ch = sdf.device, (0 if features is None else int(features.shape[3]))
    depth = torch.empty((nf, h, w), dtype=torch.float32, device=dev)
    hit = torch.empty((nf, h, w), dtype=torch.int32, device=dev)
    ok = torch.empty((nf, h, w), dtype=torch.uint8, device=dev)
    feat = None if features is None else torch.empty((nf, h, w, ch), dtype=torch.float32, device=dev)
    if nf:
        bricks = None
        if skip:
            bricks = torch.empty(((dz + 7) // 8, (dy + 7) // 8, (dx + 7) // 8), dtype=torch.uint8, device=dev)
            _lib.call('sgnn_raycast_bricks', sdf.data_ptr(), dx, dy, dz, float(band), bricks.data_ptr())
        _lib.call('sgnn_raygrad_cast', sdf.data_ptr(), dx, dy, dz, float(band), _lib.ptr(bricks), table.data_ptr(), nf,
                  int(DEFAULT_CHUNK if chunk is None else chunk), h, w, float(depth_min), float(dt), ns,
                  _lib.ptr(features), ch, depth.data_ptr(), hit.data_ptr(), _lib.ptr(feat), ok.data_ptr())
    return depth, hit, feat, ok


def diff_backward(sdf, features, table, hw, depth_min, dt, ns, hit, grad_depth, grad_feat, want_sdf=True,
                  want_features=True, chunk=None):
    """sgnn_raygrad_backward into fresh zeroed volumes -> (grad_sdf or None, grad_features or None).  grad_depth
    (F, h, w) and grad_feat (F, h, w, C) are fp32 device tensors or None."""
    dz, dy, dx = (int(v) for v in sdf.shape)
    nf, (h, w) = int(table.numel()) // FRAME_DTYPE.itemsize, hw
    ch = 0 if features is None else int(features.shape[3])
    grad_sdf = torch.zeros_like(sdf) if want_sdf else None
    grad_features = torch.zeros_like(features) if want_features and features is not None else None
    if nf:
        _lib.call('sgnn_raygrad_backward', sdf.data_ptr(), dx, dy, dz, table.data_ptr(), nf,
                  int(DEFAULT_CHUNK if chunk is None else chunk), h, w, float(depth_min), float(dt), ns, hit.data_ptr(),
                  _lib.ptr(features), ch, _lib.ptr(grad_depth), _lib.ptr(grad_feat if features is not None else None),
                  _lib.ptr(grad_sdf), _lib.ptr(grad_features))
    return grad_sdf, grad_features


class CastDiff(torch.autograd.Function):
    """depth, feat, ok = cast of (sdf, features); the gradients of depth and feat go to sdf and features by
    sgnn_raygrad_backward (see sgnn_hip.h).  geom = (device frame table, (h, w), band, depth_min, dt, samples per ray,
    skip, chunk)."""

    @staticmethod
    def forward(ctx, sdf, features, geom):
        table, hw, band, dmin, dt, ns, skip, chunk = geom
        depth, hit, feat, ok = diff_forward(sdf, features, table, hw, band, dmin, dt, ns, skip, chunk)
        ok = ok.bool()
        ctx.save_for_backward(sdf, features, hit)
        ctx.geom = geom
        ctx.mark_non_differentiable(ok)
        ctx.set_materialize_grads(False)
        return depth, feat, ok

    @staticmethod
    def backward(ctx, grad_depth, grad_feat, _):
        sdf, features, hit = ctx.saved_tensors
        table, hw, band, dmin, dt, ns, skip, chunk = ctx.geom
        gd = None if grad_depth is None else grad_depth.to(torch.float32).contiguous()
        gf = None if grad_feat is None else grad_feat.to(torch.float32).contiguous()
        grad_sdf, grad_features = diff_backward(sdf, features, table, hw, dmin, dt, ns, hit, gd, gf,
                                                ctx.needs_input_grad[0], ctx.needs_input_grad[1], chunk)
        return grad_sdf, grad_features, None


def cast_diff(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, features=None, step=0.5, depth_min=0.4,
              depth_max=4.0, skip=True, chunk=None):
    """cast() with a backward -> (depth, feat, ok): depth (F, h, w) fp32, cast()'s bit for bit, -inf = no hit; feat
    (F, h, w, C) fp32, the per-voxel features read at the hit, or None without features; ok (F, h, w) bool, no gradient.

    sdf (Z, Y, X) fp32 and features (Z, Y, X, C) fp32, 1 <= C <= 16, are tensors (host arrays are taken too) and either
    may require grad: the gradient of depth goes to the sixteen voxels of the crossing, the gradient of feat to the
    eight voxels of the hit's cell of features and, through the hit position, to the same sixteen voxels of sdf.  Poses,
    intrinsics and world2grid get no gradient.  feat is the plain trilinear sum over all eight corners of the hit's
    cell: a voxel without a feature should hold 0 and then darkens the result (unlike cast_color, which renormalises);
    it is 0 where there is no hit or the hit's cell lies outside the volume.  ok is True where the pixel has a hit whose
    own cell lies in the volume with eight usable corners of sdf: mask the loss with it.  The incoming gradient of a
    pixel without a hit is ignored (NaN included); a non-finite one at a hit propagates, and a crossing with a tiny
    pv - v gives large gradients.  Gradient volumes are summed with fp32 atomic adds: two runs may differ in the last
    bits (INTEGRATION.md section U rule 5).  The other arguments, and every ValueError, as cast()."""
    if features is not None:
        shape = tuple(features.shape)
        if len(shape) != 4 or shape[:3] != tuple(sdf.shape):
            raise ValueError('features must be (Z, Y, X, C) for sdf %s, got %s' % (tuple(sdf.shape), shape))
        if not 1 <= shape[3] <= MAX_CHANNELS:
            raise ValueError('features must have 1 to %d channels, got %d' % (MAX_CHANNELS, shape[3]))
    _, hw, band, dmin, dt, ns, table = _plan(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, step,
                                             depth_min, depth_max)
    dev = _device(next((x.device for x in (sdf, features) if torch.is_tensor(x) and x.is_cuda), None))
    vol = _to_device(sdf, torch.float32, dev)
    fea = None if features is None else _to_device(features, torch.float32, dev)
    geom = (torch.from_numpy(table.view(np.uint8)).to(dev), hw, band, dmin, dt, ns, bool(skip), chunk)
    return CastDiff.apply(vol, fea, geom)


def cast_sparse_diff(locs_zyx, vals, dims_zyx, world2grid, voxel_size, intrinsics, cam2world, hw, band, features=None,
                     **kwargs):
    """cast_diff() of sparse rows: locs (N, 3) z, y, x (distinct rows), vals (N,) or (N, 1) and features (N, C), put
    into dense volumes with torch operations that autograd follows, so gradients come back per row.  A voxel without a
    row is unknown (-inf) in the sdf and 0 in the features."""
    d0, d1, d2 = (int(v) for v in dims_zyx)
    if np.ndim(locs_zyx) != 2 or tuple(np.shape(locs_zyx))[1:] != (3,):
        raise ValueError('locs must be (N, 3), got %s' % (tuple(np.shape(locs_zyx)),))
    n = int(np.shape(locs_zyx)[0])
    if int(np.prod(np.shape(vals))) != n:
        raise ValueError('%d values for %d rows' % (int(np.prod(np.shape(vals))), n))
    if features is not None:
        shape = tuple(np.shape(features))
        if len(shape) != 2 or shape[0] != n:
            raise ValueError('features must be (N, C) for %d rows, got %s' % (n, shape))
        if not 1 <= shape[1] <= MAX_CHANNELS:
            raise ValueError('features must have 1 to %d channels, got %d' % (MAX_CHANNELS, shape[1]))
    # the checks of cast_diff before anything is put on the device (only the shape of the volume is looked at)
    _plan(np.broadcast_to(np.float32(0), (d0, d1, d2)), world2grid, voxel_size, intrinsics, cam2world, hw, band, kwargs.get('step', 0.5),
          kwargs.get('depth_min', 0.4), kwargs.get('depth_max', 4.0))
    dev = _device(next((x.device for x in (vals, features, locs_zyx) if torch.is_tensor(x) and x.is_cuda), None))
    locs = torch.as_tensor(locs_zyx).to(dev).long()
    flat = ((locs[:, 0] * d1 + locs[:, 1]) * d2 + locs[:, 2],)
    rows = torch.as_tensor(vals).to(device=dev, dtype=torch.float32).reshape(-1)
    sdf = torch.full((d0 * d1 * d2,), -float('inf'), dtype=torch.float32, device=dev).index_put(flat, rows)
    fea = None
    if features is not None:
        rows = torch.as_tensor(features).to(device=dev, dtype=torch.float32)
        fea = torch.zeros((d0 * d1 * d2, rows.shape[1]), dtype=torch.float32, device=dev).index_put(flat, rows)
        fea = fea.reshape(d0, d1, d2, -1)
    return cast_diff(sdf.reshape(d0, d1, d2), world2grid, voxel_size, intrinsics, cam2world, hw, band, features=fea,
                     **kwargs)
