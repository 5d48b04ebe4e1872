"""Host glue shared by the device-side tools (fusion, render, meshdist, raycast, track, marching_cubes,
components, simplify, voxelize, edt): where an input ends up, and the allocate-and-call wrappers of the shared mesh
entry points (csrc/mesh_tables.hip) and of sgnn_compact_mask.  Plumbing only; every helper does what its callers wrote
out before.
"""
import numpy as np
import torch

from . import _lib


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


def compact(mask, n, dev, read=True):
    """sgnn_compact_mask: (sel int32, count): sel[:count] = the rows of the uint8 mask (n,) that are set, in order.
    count is an int, or with read=False the device int64[1], so that the caller can read it back later."""
    sel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = _lib.query('sgnn_compact_ws_bytes', n)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_compact_mask', _lib.ptr(mask), n, _lib.ptr(sel), _lib.ptr(cnt), _lib.ptr(ws), wsb)
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
