"""Host glue shared by the device-side tools (fusion, render, meshdist, raycast, track, marching_cubes, components,
simplify, voxelize, edt, chunks, data): where an input ends up; the checks and the upload of a triangle mesh (mesh_shape,
mesh_upload) and of cameras (camera_shapes, cameras); and the allocate-and-call wrappers of sgnn_meshdist_pack
(pack_faces), of a count / fill pair of CSR list passes (binned_lists), of the shared mesh entry points
(csrc/mesh_tables.hip) and of sgnn_compact_mask.  Plumbing only; every helper does what its callers wrote out before.
"""
import numpy as np
import torch

from . import _lib

STATUS_INDEX_RANGE = 1      # SGNN_STATUS_COORD_RANGE


def device(device=None):
    _lib.require_gpu()
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def to_device(x, dtype, dev):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def host(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))


def source_device(*inputs):
    """The device the inputs name: that of the first device tensor among them, the current one if there is none."""
    for x in inputs:
        if torch.is_tensor(x) and x.is_cuda:
            return device(x.device)
    return device()


def positive(name, v):
    """v as fp32, which must be positive and finite."""
    v = np.float32(v)
    if not (v > 0 and np.isfinite(v)):
        raise ValueError('%s must be positive' % name)
    return v


def invertible(m, name, dtype=np.float64):
    """m as a host (4, 4) matrix of dtype, which must be finite with a determinant (fp64) that is not 0."""
    m = host(m, dtype)
    if m.shape != (4, 4) or not np.isfinite(m).all() or abs(np.linalg.det(m.astype(np.float64))) == 0:
        raise ValueError('%s must be an invertible (4, 4) matrix' % name)
    return m


def mesh_shape(verts, faces, *more):
    """First half of a mesh hand-over: the device the inputs (and `more`, which may be None) name, and (nv, nt) once
    verts and faces are (N, 3).  The caller's own limits come between this and mesh_upload."""
    dev = source_device(verts, faces, *more)
    for name, x in (('verts', verts), ('faces', faces)):
        shape = tuple(x.shape)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError('%s must be (N, 3), got %s' % (name, shape))
    return dev, (int(verts.shape[0]), int(faces.shape[0]))


def mesh_upload(verts, faces, nv, dev):
    """Second half: (verts fp32, faces int32, on_device) on dev.  Host faces are range-checked here; faces that came
    from the device (on_device) are checked by the kernel that reads them, through a status word."""
    on_device = torch.is_tensor(faces) and faces.is_cuda
    if not on_device and faces.shape[0]:
        fh = host(faces, np.int64)
        if fh.min() < 0 or fh.max() >= nv:
            raise ValueError('face index out of range [0, %d)' % nv)
    return to_device(verts, torch.float32, dev), to_device(faces, torch.int32, dev), on_device


def pack_faces(v, f, on_device, dev):
    """sgnn_meshdist_pack: (records (T, 12) fp32, boxes (T, 6) fp32, usable (T,) uint8) of a mesh_upload mesh."""
    nv, nt = int(v.shape[0]), int(f.shape[0])
    records = torch.empty((nt, 12), dtype=torch.float32, device=dev)
    boxes = torch.empty((nt, 6), dtype=torch.float32, device=dev)
    usable = torch.empty(nt, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev) if on_device else None
    _lib.call('sgnn_meshdist_pack', v.data_ptr(), nv, f.data_ptr(), nt, records.data_ptr(), boxes.data_ptr(),
              usable.data_ptr(), _lib.ptr(status))
    if status is not None and int(status.item()) & STATUS_INDEX_RANGE:
        raise ValueError('face index out of range [0, %d)' % nv)
    return records, boxes, usable


def binned_lists(count, fill, args, ncell, dev, too_many):
    """CSR lists from a count / fill pair of entry points that share the leading arguments `args`: (offsets
    (ncell + 1,) int32, refs int32, n_refs).  Count pass, scan, one read-back of the total, fill pass.  too_many: the
    ValueError text, with one %d, for a total that does not fit 31 bits."""
    counts = torch.zeros(ncell, dtype=torch.int32, device=dev)
    _lib.call(count, *args, counts.data_ptr())
    offsets = torch.zeros(ncell + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    n_refs = int(offsets[-1].item())
    if n_refs >= 2 ** 31:
        raise ValueError(too_many % n_refs)
    offsets = offsets.to(torch.int32)
    refs = torch.empty(max(n_refs, 1), dtype=torch.int32, device=dev)
    if n_refs:
        counts.zero_()
        _lib.call(fill, *args, offsets.data_ptr(), counts.data_ptr(), refs.data_ptr())
    return offsets, refs, n_refs


def cameras(intrinsics, cam2world):
    """(k (F, 4) host fp32, cam2world (F, 4, 4) host fp64): what every frame table starts from."""
    k = host(intrinsics, np.float32).reshape(-1, 4)
    c2w = host(cam2world, np.float64).reshape(-1, 4, 4)
    if c2w.shape[0] != k.shape[0]:
        raise ValueError('%d intrinsics for %d poses' % (k.shape[0], c2w.shape[0]))
    return k, c2w


def camera_shapes(intrinsics, cam2world):
    if np.ndim(intrinsics) != 2 or tuple(np.shape(intrinsics))[1:] != (4,):
        raise ValueError('intrinsics must be (F, 4), got %s' % (tuple(np.shape(intrinsics)),))
    if np.ndim(cam2world) != 3 or tuple(np.shape(cam2world))[1:] != (4, 4):
        raise ValueError('cam2world must be (F, 4, 4), got %s' % (tuple(np.shape(cam2world)),))


def compact(mask, n, dev, read=True, ws=None):
    """sgnn_compact_mask: (sel int32, count): sel[:count] = the rows of the uint8 mask (n,) that are set, in order.
    count is an int, or with read=False the device int64[1], so that the caller can read it back later.  ws: a uint8
    workspace of at least sgnn_compact_ws_bytes(n) that the caller keeps (default: a fresh one)."""
    sel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    if ws is None:
        ws = torch.empty(max(_lib.query('sgnn_compact_ws_bytes', n), 1), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_compact_mask', _lib.ptr(mask), n, _lib.ptr(sel), _lib.ptr(cnt), _lib.ptr(ws), ws.numel())
    return sel, (int(cnt.item()) if read else cnt)


def take3(src, elem_bytes, sel, n, dtype):
    """sgnn_take_rows3: rows sel[:n] of a (., 3) array of 1- or 4-byte elements."""
    out = torch.empty((n, 3), dtype=dtype, device=src.device)
    if n:
        _lib.call('sgnn_take_rows3', _lib.ptr(src), elem_bytes, _lib.ptr(sel), n, _lib.ptr(out))
    return out


def number(sel, n, size, dev, fill=None):
    """sgnn_weld_number: newid (size,) int32 with newid[sel[p]] = p for p < n.  The other rows hold fill; with
    fill=None they are uninitialised, for callers that read selected rows only."""
    newid = torch.empty(max(size, 1), dtype=torch.int32, device=dev)
    if fill is not None:
        newid.fill_(fill)
    if n:
        _lib.call('sgnn_weld_number', _lib.ptr(sel), n, _lib.ptr(newid))
    return newid


def dedup_faces(corner_ids, newid, ntri, dev):
    """sgnn_mesh_faces: (faces (ntri, 3) int32 = newid[corner_ids], keep (ntri,) uint8 = not degenerate and the first
    face of its unordered vertex triple)."""
    cap = _lib.query('sgnn_weld_slots', ntri)
    faces = torch.empty((max(ntri, 1), 3), dtype=torch.int32, device=dev)
    frep = torch.empty(cap, dtype=torch.int32, device=dev)
    ffirst = torch.empty(cap, dtype=torch.int32, device=dev)
    keep = torch.empty(max(ntri, 1), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_mesh_faces', _lib.ptr(corner_ids), _lib.ptr(newid), ntri, _lib.ptr(faces), _lib.ptr(frep),
              _lib.ptr(ffirst), cap, _lib.ptr(keep))
    return faces, keep
