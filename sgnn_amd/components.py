"""Connected components of volumes, sparse rows and meshes on the GPU, and the filters built on them: drop the small
detached fragments ("floaters") of a prediction or of a fused scan before it is meshed, shown or scored.

The reference project has no counterpart; the rules this module follows are listed in INTEGRATION.md section J, and
that text is the contract of the kernels (sgnn_amd/csrc/components.hip) and of the independent host restatement of
the tests (tests/components_ref.py).  Results are integers, so the two agree exactly.

    lab = label_volume(sdf, band=0.06)                          # Labels(labels (Z,Y,X) int32, sizes (C,) int64)
    lab = label_sparse(locs, dims_zyx)                          # labels (N,) in row order
    m = label_mesh(verts, faces)                                # MeshLabels(face_labels, vertex_labels, face_sizes, vertex_sizes)
    keep = select(lab.sizes, min_size=50, keep_largest=3)       # (C,) bool
    sdf2 = filter_volume(sdf, band=0.06, min_size=50)           # dropped components become -inf ("never seen")
    locs2, vals2, rows = filter_sparse(locs, vals, dims_zyx, min_size=50)
    verts2, faces2 = filter_mesh(verts, faces, keep_largest=1)

Component k is the one with the k-th smallest minimum index (raster index of a voxel, index of a vertex); background
voxels and vertices that no face uses are -1.  Everything runs on the device and raises _lib.SgnnError otherwise;
each labelling call reads one number back, the component count.  Mesh connectivity is by shared vertex index: pass a
welded mesh from marching_cubes.clean_mesh / run_marching_cubes, not a triangle soup, whose every face is a
component of its own.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._glue import compact, number, take3

TILE_ZYX = (8, 8, 32)       # SGNN_CC_TILE_Z, _Y, _X of include/sgnn_hip.h: the tile that one workgroup labels in LDS
STATUS_INDEX_RANGE = 1      # SGNN_STATUS_COORD_RANGE
LIMIT = 2 ** 31

Labels = namedtuple('Labels', 'labels sizes')
MeshLabels = namedtuple('MeshLabels', 'face_labels vertex_labels face_sizes vertex_sizes')


def _device_tensor(x, what):
    _lib.require_gpu()
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.SgnnError('sgnn_amd.components runs on the GPU only (%s is %s)' % (
            what, 'a %s tensor' % x.device if torch.is_tensor(x) else type(x).__name__))
    return x


def _number(parent, n, dev):
    """Flatten, enumerate the roots in ascending order and relabel: labels (n,) int32 and sizes (C,) int64."""
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    is_root = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_cc_flatten', _lib.ptr(parent), n, _lib.ptr(is_root))
    sel, ncomp = compact(is_root, n, dev)                      # stable: sel[k] = k-th smallest root
    rank = number(sel, ncomp, n, dev)                          # read at roots only
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.zeros(max(ncomp, 1), dtype=torch.int64, device=dev)
    _lib.call('sgnn_cc_relabel', _lib.ptr(parent), n, _lib.ptr(rank), ncomp, _lib.ptr(labels), _lib.ptr(sizes))
    return labels, sizes[:ncomp]


def _connectivity(connectivity):
    if connectivity not in (6, 18, 26):
        raise ValueError('connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    return int(connectivity)


def _label_mask(mask, connectivity, tiled):
    """mask: contiguous device uint8 (B, Z, Y, X) -> labels (B*Z*Y*X,) int32, sizes (C,) int64."""
    nb, dz, dy, dx = (int(v) for v in mask.shape)
    n = nb * dz * dy * dx
    if n >= LIMIT:
        raise ValueError('%d voxels do not fit 31 bits' % n)
    parent = torch.empty(max(n, 1), dtype=torch.int32, device=mask.device)
    _lib.call('sgnn_cc_volume_link', _lib.ptr(mask), nb, dz, dy, dx, connectivity, 1 if tiled else 0, _lib.ptr(parent))
    return _number(parent, n, mask.device)


def foreground(mask_or_sdf, band=None):
    """The uint8 foreground of a labelling input: a bool or uint8 tensor is a mask (non-zero = foreground); a float
    tensor needs band, and its foreground is isfinite(sdf) & (|sdf| <= band), compared in the tensor's precision."""
    x = mask_or_sdf
    if x.dtype in (torch.bool, torch.uint8):
        if band is not None:
            raise ValueError('band goes with a float volume, not with a mask')
        return (x != 0).to(torch.uint8) if x.dtype == torch.uint8 else x.to(torch.uint8)
    if not x.dtype.is_floating_point:
        raise ValueError('a volume must be bool, uint8 or float, got %s' % x.dtype)
    if band is None:
        raise ValueError('a float volume needs band')
    return (torch.isfinite(x) & (x.abs() <= torch.tensor(float(band), dtype=x.dtype, device=x.device))).to(torch.uint8)


def label_volume(mask_or_sdf, band=None, connectivity=26, tiled=True):
    """Components of a (Z, Y, X) or (B, Z, Y, X) volume: Labels(labels int32 of the input's shape, sizes (C,) int64).

    Voxels are neighbours inside one sample only, across 6 faces, 18 faces and edges, or all 26.  tiled=False takes
    the one-level path (every pair merged in global memory); the result is the same."""
    x = _device_tensor(mask_or_sdf, 'the volume')
    connectivity = _connectivity(connectivity)
    if x.dim() not in (3, 4):
        raise ValueError('a volume must be (Z, Y, X) or (B, Z, Y, X), got %s' % (tuple(x.shape),))
    mask = foreground(x, band).contiguous()
    labels, sizes = _label_mask(mask.reshape((-1,) + tuple(mask.shape[-3:])), connectivity, tiled)
    return Labels(labels.reshape(x.shape), sizes)


def _sparse_cells(locs, dims_zyx):
    """Checked rows -> (linear cell of every row, batch size)."""
    locs = _device_tensor(locs, 'locs')
    if locs.dim() != 2 or locs.shape[1] not in (3, 4):
        raise ValueError('locs must be (N, 3) z,y,x or (N, 4) z,y,x,b, got %s' % (tuple(locs.shape),))
    dz, dy, dx = (int(v) for v in dims_zyx)
    locs = locs.long()
    nb = 1
    if locs.shape[0]:
        hi = torch.tensor([dz, dy, dx], device=locs.device)
        bad = ((locs[:, :3] < 0) | (locs[:, :3] >= hi)).any()
        bmax = locs[:, 3].max() if locs.shape[1] == 4 else bad.long() * 0
        bmin = locs[:, 3].min() if locs.shape[1] == 4 else bad.long() * 0
        bad, bmax, bmin = (int(v) for v in torch.stack([bad.long(), bmax, bmin]).tolist())
        if bad or bmin < 0:
            raise ValueError('a row of locs lies outside dims %s' % ((dz, dy, dx),))
        nb = bmax + 1
    if nb * dz * dy * dx >= LIMIT:
        raise ValueError('%d voxels do not fit 31 bits' % (nb * dz * dy * dx))
    cell = (locs[:, 0] * dy + locs[:, 1]) * dx + locs[:, 2]
    if locs.shape[1] == 4:
        cell = cell + locs[:, 3] * (dz * dy * dx)
    return cell, nb


def label_sparse(locs, dims_zyx, connectivity=26, tiled=True):
    """Components of sparse rows: locs (N, 3) z, y, x or (N, 4) with the batch index last (as output_sdf[0]) are
    scattered into a dense index volume of dims_zyx, labelled there and gathered back.  labels (N,) follow the rows;
    duplicate rows get the same label and count once in sizes.  A row outside dims_zyx raises ValueError."""
    connectivity = _connectivity(connectivity)
    cell, nb = _sparse_cells(locs, dims_zyx)
    dz, dy, dx = (int(v) for v in dims_zyx)
    mask = torch.zeros((nb, dz, dy, dx), dtype=torch.uint8, device=cell.device)
    mask.view(-1)[cell] = 1
    labels, sizes = _label_mask(mask, connectivity, tiled)
    return Labels(labels[cell], sizes)


def _faces(verts_or_nverts, faces):
    faces = _device_tensor(faces, 'faces')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('faces must be (F, 3), got %s' % (tuple(faces.shape),))
    nv = int(verts_or_nverts) if isinstance(verts_or_nverts, (int, np.integer)) else int(verts_or_nverts.shape[0])
    nt = int(faces.shape[0])
    if nv < 0 or nv >= LIMIT or nt * 3 >= LIMIT:
        raise ValueError('%d vertices / %d faces do not fit 31 bits' % (nv, nt))
    if faces.dtype != torch.int32:
        big = faces.long()
        if nt and bool(((big < 0) | (big >= nv)).any().item()):
            raise _lib.SgnnError('face index out of range [0, %d)' % nv)
        faces = big.to(torch.int32)
    return faces.contiguous(), nv, nt


def label_mesh(verts_or_nverts, faces):
    """Components of a mesh whose faces share vertex indices: MeshLabels(face_labels (F,) int32, vertex_labels (V,)
    int32, face_sizes (C,) int64, vertex_sizes (C,) int64).  Components are numbered by their smallest referenced
    vertex index; a vertex that no face uses is -1.  A face index outside [0, V) raises SgnnError.  The first
    argument is the (V, 3) vertex array or just V: positions play no part, so weld first (marching_cubes.clean_mesh)."""
    faces, nv, nt = _faces(verts_or_nverts, faces)
    dev = faces.device
    parent = torch.empty(max(nv, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call('sgnn_cc_mesh_link', _lib.ptr(faces), nt, nv, _lib.ptr(parent), _lib.ptr(status))
    if nt and int(status.item()) & STATUS_INDEX_RANGE:          # such a face was skipped, not dereferenced
        raise _lib.SgnnError('face index out of range [0, %d)' % nv)
    vertex_labels, vertex_sizes = _number(parent, nv, dev)
    ncomp = int(vertex_sizes.shape[0])
    face_labels = torch.empty(nt, dtype=torch.int32, device=dev)
    face_sizes = torch.zeros(max(ncomp, 1), dtype=torch.int64, device=dev)
    _lib.call('sgnn_cc_face_labels', _lib.ptr(faces), nt, nv, _lib.ptr(vertex_labels), ncomp, _lib.ptr(face_labels),
              _lib.ptr(face_sizes))
    return MeshLabels(face_labels, vertex_labels, face_sizes[:ncomp], vertex_sizes)


def select(sizes, min_size=None, keep_largest=None):
    """(C,) bool: the components to keep.  min_size keeps sizes >= min_size; keep_largest keeps the k largest, ties
    going to the lower label.  With both, a component must pass both; with neither, all are kept.  sizes may be a
    torch tensor (the result lives on its device) or a numpy array (numpy result)."""
    as_numpy = not torch.is_tensor(sizes)
    s = torch.as_tensor(np.asarray(sizes)) if as_numpy else sizes
    keep = torch.ones(s.shape, dtype=torch.bool, device=s.device)
    if min_size is not None:
        keep &= s >= int(min_size)
    if keep_largest is not None:
        if int(keep_largest) < 0:
            raise ValueError('keep_largest must be >= 0')
        order = torch.sort(s, descending=True, stable=True).indices[:int(keep_largest)]
        top = torch.zeros_like(keep)
        top[order] = True
        keep &= top
    return keep.numpy() if as_numpy else keep


def _kept(labels, keep):
    """keep[labels] with -1 -> False."""
    if keep.numel() == 0:
        return torch.zeros(labels.shape, dtype=torch.bool, device=labels.device)
    return (labels >= 0) & keep[labels.clamp(min=0).long()]


def filter_volume(sdf, band, min_size=None, keep_largest=None, connectivity=26, fill=-float('inf')):
    """A copy of a float (Z, Y, X) or (B, Z, Y, X) volume in which the foreground voxels (isfinite & |sdf| <= band)
    of dropped components hold fill; -inf is what fusion.TSDFVolume holds where nothing was seen.  Every other voxel,
    and the input, are unchanged."""
    lab = label_volume(sdf, band, connectivity)
    drop = (lab.labels >= 0) & ~_kept(lab.labels, select(lab.sizes, min_size, keep_largest))
    out = sdf.clone()
    out[drop] = fill
    return out


def filter_sparse(locs, vals, dims_zyx, min_size=None, keep_largest=None, connectivity=26):
    """(locs, vals, rows) of the rows whose component is kept, in their original order; rows (M,) int64 indexes the
    input.  Sizes count voxels, not rows."""
    lab = label_sparse(locs, dims_zyx, connectivity)
    rows = torch.nonzero(_kept(lab.labels, select(lab.sizes, min_size, keep_largest))).reshape(-1)
    vals = _device_tensor(vals, 'vals')
    if vals.shape[0] != locs.shape[0]:
        raise ValueError('locs has %d rows and vals %d' % (locs.shape[0], vals.shape[0]))
    return locs[rows], vals[rows], rows


def filter_mesh(verts, faces, colors=None, min_size=None, keep_largest=None):
    """(verts, faces) or, with colors, (verts, faces, colors) of the kept components of a welded mesh; sizes are face
    counts.  Kept faces stay in order; vertices that no kept face uses are removed and the others keep their order;
    faces are re-indexed.  verts (V, 3) float32, colors (V, 3) uint8 and faces (F, 3) int32, as clean_mesh returns
    them."""
    verts = _device_tensor(verts, 'verts')
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError('verts must be (V, 3) float32')
    if colors is not None:
        colors = _device_tensor(colors, 'colors')
        if tuple(colors.shape) != tuple(verts.shape) or colors.dtype != torch.uint8:
            raise ValueError('colors must be (V, 3) uint8')
    lab = label_mesh(verts, faces)
    faces, nv, nt = _faces(verts, faces)
    dev = faces.device
    keep = select(lab.face_sizes, min_size, keep_largest)
    vsel, n_new = compact(_kept(lab.vertex_labels, keep).to(torch.uint8), nv, dev)
    fsel, n_faces = compact(_kept(lab.face_labels, keep).to(torch.uint8), nt, dev)
    newid = number(vsel, n_new, nv, dev)                       # read at kept vertices only
    out_f = take3(faces, 4, fsel, n_faces, torch.int32)
    out_f = newid[out_f.long()] if n_faces else out_f
    out = (take3(verts.contiguous(), 4, vsel, n_new, torch.float32), out_f)
    return out if colors is None else out + (take3(colors.contiguous(), 1, vsel, n_new, torch.uint8),)
