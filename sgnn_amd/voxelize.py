"""Triangle meshes to signed distance volumes on the GPU: the exact signed distance of every voxel centre within a
narrow band of a mesh, as a fusion.TSDFVolume, a TSDFPyramid or raw arrays.

The reference project has no counterpart; the rules this module follows are listed in INTEGRATION.md section L, and
that text is the contract of the kernels (sgnn_amd/csrc/voxelize.hip) and of the independent NumPy restatement of the
tests (tests/voxelize_ref.py).

    vol = mesh_to_volume(verts, faces, (dx, dy, dz), 0.02, world2grid, band=3.0)      # a fusion.TSDFVolume
    pyr = mesh_to_pyramid(verts, faces, (dx, dy, dz), 0.02, world2grid, levels=4)      # a fusion.TSDFPyramid
    res = signed_distance(verts_grid, faces, (dx, dy, dz), band=3.0)                   # dist, face: (dz, dy, dx)

verts (V, 3) fp32 and faces (T, 3) int32 may be numpy arrays or torch tensors, host or device.  Distances are true
distances to the nearest triangle (meshdist's, bit for bit), positive on the side the face normals point to (free
space, as in fusion); the far field stays "never seen" (-inf in a volume).  The host layer does plumbing only: the
scan between the count and the fill pass and the allocation of the tables.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, fusion
from ._glue import binned_lists, compact, host as _host, mesh_shape, mesh_upload, pack_faces

BRICK = 8               # voxels per brick axis (csrc/voxelize.hip)
FACE_BATCH = 128        # SGNN_VOX_BATCH of include/sgnn_hip.h: face records a brick stages through LDS at a time
WAVE_BRICKS = 256       # a face whose voxel box touches more bricks is listed by its whole wave (csrc/box_lists.h)
MAX_BAND = 65535.0
F32 = np.float32

Result = namedtuple('Result', ['dist', 'face'])


def _check(verts, faces, dims_xyz, band):
    dev, (nv, nt) = mesh_shape(verts, faces)
    dims = tuple(int(d) for d in dims_xyz)
    if len(dims) != 3 or min(dims) < 1 or max(dims) > 65535 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('unsupported volume dimensions %s' % (dims,))
    band = float(F32(band))
    if not 0.0 <= band <= MAX_BAND:
        raise ValueError('band must be in [0, %g] voxels, got %r' % (MAX_BAND, band))
    if nt * 3 >= 2 ** 31 or nv >= 2 ** 31:
        raise ValueError('the mesh does not fit 31-bit indices')
    return mesh_upload(verts, faces, nv, dev) + (dims, band, dev)


def _brick_lists(boxes, nt, band, dims, dev):
    """The faces of every 8x8x8 brick (CSR): (offsets (bricks + 1,) int32, refs int32, n_refs)."""
    dx, dy, dz = dims
    nbricks = -(-dx // BRICK) * -(-dy // BRICK) * -(-dz // BRICK)
    return binned_lists('sgnn_vox_bricks_count', 'sgnn_vox_bricks_fill', (boxes.data_ptr(), nt, band, dx, dy, dz),
                        nbricks, dev,
                        '%d (face, brick) references do not fit 31 bits: voxelise a coarser volume or a smaller band')


def _signed_distance(v, f, on_device, dims, band, flip, dev):
    dx, dy, dz = dims
    nv, nt = int(v.shape[0]), int(f.shape[0])
    dist = torch.full((dz, dy, dx), float('inf'), dtype=torch.float32, device=dev)
    face = torch.full((dz, dy, dx), -1, dtype=torch.int32, device=dev)
    if nt == 0:
        return Result(dist, face)
    records, boxes, usable = pack_faces(v, f, on_device, dev)
    offsets, refs, n_refs = _brick_lists(boxes, nt, band, dims, dev)
    if n_refs == 0:                                                 # no brick holds a face
        return Result(dist, face)
    sel, nsel = compact((offsets[1:] != offsets[:-1]).to(torch.uint8), offsets.numel() - 1, dev)
    # pseudo-normal tables
    cap = _lib.query('sgnn_weld_slots', 3 * nt)
    vsum = torch.empty((max(nv, 1), 3), dtype=torch.int64, device=dev)
    ekeys = torch.empty(cap, dtype=torch.int64, device=dev)
    efirst = torch.empty(cap, dtype=torch.int32, device=dev)
    esum = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    _lib.call('sgnn_vox_normals', records.data_ptr(), f.data_ptr(), usable.data_ptr(), nt, nv, vsum.data_ptr(),
              ekeys.data_ptr(), efirst.data_ptr(), esum.data_ptr(), cap)
    _lib.call('sgnn_vox_nearest', records.data_ptr(), boxes.data_ptr(), f.data_ptr(), offsets.data_ptr(), refs.data_ptr(),
              sel.data_ptr(), nsel, dx, dy, dz, band, int(bool(flip)), vsum.data_ptr(), ekeys.data_ptr(), esum.data_ptr(),
              cap, dist.data_ptr(), face.data_ptr())
    return Result(dist, face)


def signed_distance(verts_grid, faces, dims_xyz, band, flip=False):
    """Signed distance, in voxels, from every voxel centre of a (dx, dy, dz) volume to a mesh given in grid
    coordinates (voxel (i, j, k) is centred on the integer point): Result(dist (dz, dy, dx) fp32, +inf beyond the band;
    face (dz, dy, dx) int32, the nearest face, -1 beyond the band), on the device.

    |dist| and face equal meshdist.TriangleIndex(verts_grid, faces).distance(centres, max_dist=band) bit for bit.  The
    sign comes from the angle-weighted pseudo-normal of the closest feature: positive on the side the face normals
    point to, flip=True for the other convention.  Inconsistently oriented or non-manifold meshes get whatever the
    normal sums give.  A mesh without a usable face gives +inf everywhere."""
    v, f, on_device, dims, band, dev = _check(verts_grid, faces, dims_xyz, band)
    return _signed_distance(v, f, on_device, dims, band, flip, dev)


def _to_grid(v, world2grid, dev):
    m = _host(world2grid, np.float32).reshape(4, 4)
    out = torch.empty_like(v)
    _lib.call('sgnn_vox_grid_coords', v.data_ptr(), int(v.shape[0]), m.ctypes.data, out.data_ptr())
    return out


def _fill_volume(vol, v, f, on_device, band, flip):
    res = _signed_distance(_to_grid(v, vol.world2grid, vol.device), f, on_device, vol.dims_xyz, band, flip, vol.device)
    _lib.call('sgnn_vox_tsdf', res.dist.data_ptr(), res.face.data_ptr(), res.dist.numel(), float(vol.voxel_size),
              vol._sdf.data_ptr(), vol._weight.data_ptr())
    vol._free.zero_()
    return vol


def mesh_to_volume(verts, faces, dims_xyz, voxel_size, world2grid, band=3.0, flip=False):
    """A fusion.TSDFVolume holding the true signed distance to a mesh in world coordinates (metres) within `band`
    voxels of it: _sdf = signed distance in voxels x voxel_size (one fp32 product), -inf ("never seen") beyond the
    band; _weight = 1 inside the band, 0 elsewhere; _free = 0.  flip: see signed_distance."""
    v, f, on_device, dims, band, dev = _check(verts, faces, dims_xyz, band)
    return _fill_volume(fusion.TSDFVolume(dims, voxel_size, world2grid, device=dev), v, f, on_device, band, flip)


def mesh_to_pyramid(verts, faces, dims_xyz, voxel_size, world2grid, levels=4, band=3.0, flip=False):
    """A fusion.TSDFPyramid whose every level is voxelised on its own with the level's world2grid, dims and voxel
    size, `band` measured in that level's voxels."""
    v, f, on_device, dims, band, dev = _check(verts, faces, dims_xyz, band)
    pyr = fusion.TSDFPyramid(dims, voxel_size, world2grid, levels=levels, device=dev)
    for vol in pyr.volumes:
        _fill_volume(vol, v, f, on_device, band, flip)
    return pyr
