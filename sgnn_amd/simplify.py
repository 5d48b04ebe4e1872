"""Triangle-mesh simplification on the GPU: vertex clustering on a uniform grid (Rossignac-Borrel) with every cluster's
vertex placed at the minimiser of its regularised quadric (Lindstrom), or at the mean of its corners.

Marching cubes gives a mesh at voxel resolution, a handful of triangles per surface voxel however flat the wall; this
makes it coarser without taking it off the device.  The reference project has no counterpart; the rules this module
follows are listed in INTEGRATION.md section K, and that text is the contract of the kernels
(sgnn_amd/csrc/simplify.hip) and of the independent NumPy restatement of the tests (tests/simplify_ref.py).  The result
is a pure function of the input, the same bits on every run.

    out = cluster(verts, faces, cell=0.06, colors=None, placement='quadric', origin=None)
    # Simplified(verts (V',3) f32, faces (F',3) i32, colors (V',3) u8 or None,
    #            vertex_map (V,) i32: output vertex of every input vertex, -1 if its cluster has no surviving face,
    #            face_map (F',) i32: the input face each output face came from)
    cell = cell_for_faces(verts, faces, target_faces)          # bisection on the face count

verts (V, 3) fp32 and faces (F, 3) int32 may be numpy arrays or torch tensors, host or device, as meshdist takes them;
results are device tensors.  The host layer does plumbing only: the bounding-box minimum, the stable sort of the corners
by cluster (torch.sort) and the scan of their counts, and the index gathers of the maps.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._glue import compact, dedup_faces, device as _device, number, take3, to_device as _to_device

STATUS_RANGE = 1            # SGNN_STATUS_COORD_RANGE
CELLS_AXIS = 1 << 21        # cells per axis that a key holds
LIMIT = 2 ** 31
PLACEMENTS = ('mean', 'quadric')

Simplified = namedtuple('Simplified', 'verts faces colors vertex_map face_map')


def _inputs(verts, faces, colors=None):
    """Device tensors verts fp32 (V, 3), faces int32 (F, 3), colors uint8 (V, 3) or None."""
    dev = _device(next((x.device for x in (verts, faces) if torch.is_tensor(x) and x.is_cuda), None))
    for name, x in (('verts', verts), ('faces', faces)) + ((('colors', colors),) if colors is not None else ()):
        shape = tuple(x.shape)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError('%s must be (N, 3), got %s' % (name, shape))
    nv, nt = int(verts.shape[0]), int(faces.shape[0])
    if nv >= LIMIT or nt * 3 >= LIMIT:
        raise ValueError('%d vertices / %d faces do not fit 31 bits' % (nv, nt))
    if colors is not None and int(colors.shape[0]) != nv:
        raise ValueError('colors has %d rows and verts %d' % (colors.shape[0], nv))
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.array(faces))       # a copy: the input may be read-only
    if f.dtype != torch.int32:      # an index that int32 cannot hold is out of range whatever V is
        f = f.to(dev).long().clamp(-1, LIMIT - 1)
    return (_to_device(verts, torch.float32, dev), _to_device(f, torch.int32, dev),
            None if colors is None else _to_device(colors, torch.uint8, dev), dev)


def _cell32(cell):
    c = float(np.float32(cell))
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError('cell must be a positive finite fp32 number, got %r' % (cell,))
    return c


def _origin(v, origin):
    if origin is not None:
        return _to_device(np.asarray(origin, dtype=np.float32).reshape(3), torch.float32, v.device)
    return v.min(0).values if v.shape[0] else torch.zeros(3, dtype=torch.float32, device=v.device)


class _Clusters:
    """Rules 1, 2 and 3 with nothing read back: a cluster is named by its first member (rule 6 is _glue.dedup_faces).
    A vertex or a face that raises a status word is passed over by every stage, so the words can be read late."""

    def __init__(self, v, f, origin, cell):
        dev = v.device
        nv, nt = int(v.shape[0]), int(f.shape[0])
        self.nv, self.nt, self.dev = nv, nt, dev
        self.status = torch.zeros(2, dtype=torch.int32, device=dev)          # [0] coordinates, [1] face indices
        self.keys = torch.empty(max(nv, 1), dtype=torch.int64, device=dev)
        _lib.call('sgnn_simp_keys', _lib.ptr(v), nv, _lib.ptr(origin), cell, _lib.ptr(self.keys), _lib.ptr(self.status))
        cap = _lib.query('sgnn_weld_slots', nv)
        tkeys = torch.empty(cap, dtype=torch.int64, device=dev)
        tfirst = torch.empty(cap, dtype=torch.int32, device=dev)
        self.first_of = torch.empty(max(nv, 1), dtype=torch.int32, device=dev)
        self.is_first = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)
        _lib.call('sgnn_simp_clusters', _lib.ptr(self.keys), nv, _lib.ptr(tkeys), _lib.ptr(tfirst), cap,
                  _lib.ptr(self.first_of), _lib.ptr(self.is_first))
        self.corner_first = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
        _lib.call('sgnn_simp_corners', _lib.ptr(f), nt, nv, _lib.ptr(self.first_of), _lib.ptr(self.corner_first),
                  _lib.ptr(self.status[1:]))

    def read(self, count):
        """One read-back: the device count as an int, after the two status words have been checked."""
        count, coords, indices = torch.cat([count, self.status.long()]).tolist()
        if coords & STATUS_RANGE:
            raise _lib.SgnnError('a vertex is not finite or its cell index lies outside [0, %d)' % CELLS_AXIS)
        if indices & STATUS_RANGE:
            raise _lib.SgnnError('face index out of range [0, %d)' % self.nv)
        return count


def cluster(verts, faces, cell=0.06, colors=None, placement='quadric', origin=None):
    """Simplified(verts, faces, colors, vertex_map, face_map) of the mesh clustered on a grid of pitch cell.

    Vertices in one grid cell (counted from origin, default the componentwise minimum of verts) become one vertex, placed
    by placement 'quadric' (the minimiser of the cluster's regularised plane quadric: flat regions stay flat, edges and
    corners stay where they are) or 'mean' (the mean of the cluster's corners).  Faces with two corners in one cluster
    and later copies of a face, either orientation, are dropped; clusters that no face is left on are dropped with them.
    colors (V, 3) uint8 are averaged per cluster.  A non-finite vertex, a cell index outside [0, 2^21) (an origin above
    a vertex, or a cell too small for the extent) and a face index outside [0, V) raise SgnnError.  INTEGRATION.md
    section K has the rules in full."""
    if placement not in PLACEMENTS:
        raise ValueError('placement must be one of %s, got %r' % (PLACEMENTS, placement))
    v, f, col, dev = _inputs(verts, faces, colors)
    cell = _cell32(cell)
    nv, nt = int(v.shape[0]), int(f.shape[0])
    org = _origin(v, origin)
    cl = _Clusters(v, f, org, cell)
    sel, nclust = compact(cl.is_first, nv, dev, read=False)    # stable: sel[k] = first member of cluster k
    nclust = cl.read(nclust)
    rank = number(sel, nclust, nv, dev)                        # read at first members only
    cfaces, keep = dedup_faces(cl.corner_first, rank, nt, dev)      # faces in cluster numbers, kept-face mask
    fsel, n_faces = compact(keep, nt, dev)
    kept = take3(cfaces, 4, fsel, n_faces, torch.int32)        # surviving faces in cluster numbers
    used = torch.zeros(max(nclust, 1), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_simp_mark', _lib.ptr(kept), n_faces, nclust, _lib.ptr(used))
    csel, nout = compact(used, nclust, dev)                    # output vertex p is cluster csel[p]
    newc = number(csel, nout, nclust, dev, fill=-1)
    out_v = torch.empty((nout, 3), dtype=torch.float32, device=dev)
    out_c = None if col is None else torch.empty((nout, 3), dtype=torch.uint8, device=dev)
    if nout:
        corner_cluster = cfaces[:nt].reshape(-1)
        order = torch.sort(corner_cluster, stable=True).indices            # a cluster's corners in ascending number
        start = torch.zeros(nclust + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(corner_cluster, minlength=nclust), 0, out=start[1:])
        _lib.call('sgnn_simp_place', _lib.ptr(v), nv, _lib.ptr(f), nt, _lib.ptr(col), _lib.ptr(order), _lib.ptr(start),
                  _lib.ptr(csel), nout, _lib.ptr(sel), _lib.ptr(cl.keys), _lib.ptr(org), cell,
                  PLACEMENTS.index(placement), _lib.ptr(out_v), _lib.ptr(out_c))
    out_f = newc[kept.long()] if n_faces else kept
    vertex_map = newc[rank[cl.first_of[:nv].long()].long()] if nv else newc[:0]
    return Simplified(out_v, out_f, out_c, vertex_map, fsel[:n_faces])


def count_faces(verts, faces, cell, origin=None):
    """The number of faces cluster(verts, faces, cell, origin=origin) would return, without placing a vertex."""
    v, f, _, dev = _inputs(verts, faces)
    identity = torch.arange(max(int(v.shape[0]), 1), dtype=torch.int32, device=dev)
    return _count(v, f, _origin(v, origin), _cell32(cell), identity)


def _count(v, f, org, cell, identity):
    """Rules 1, 2 and 6 with a cluster named by its first member (the kept faces are the same); one read-back."""
    cl = _Clusters(v, f, org, cell)
    _, keep = dedup_faces(cl.corner_first, identity, cl.nt, cl.dev)
    return cl.read(compact(keep, cl.nt, cl.dev, read=False)[1])


def cell_for_faces(verts, faces, target_faces, lo=None, hi=None, iters=16):
    """The largest cell tried by a bisection whose clustering keeps at least target_faces faces.

    The search runs between lo (default: the bounding-box diagonal / 2^20) and hi (default: the diagonal) on a
    count-only route.  hi is returned if it already keeps enough faces; ValueError if even lo does not.  Otherwise the
    interval is halved iters times and the lower end, which always keeps enough, is returned (a Python float that is
    exact in fp32).  This is a convenience, not a guarantee: the face count is not strictly monotonic in the cell, so a
    larger cell than the one returned may also keep target_faces faces."""
    v, f, _, dev = _inputs(verts, faces)
    target = int(target_faces)
    org = _origin(v, None)
    if lo is None or hi is None:
        ext = (v.max(0).values - org).double() if v.shape[0] else torch.zeros(3, dtype=torch.float64, device=dev)
        diag = float(ext.pow(2).sum().sqrt().item())
        lo = diag / 2 ** 20 if lo is None else lo
        hi = diag if hi is None else hi
    lo, hi = _cell32(lo), _cell32(hi)
    if not lo <= hi:
        raise ValueError('lo %r is above hi %r' % (lo, hi))
    identity = torch.arange(max(int(v.shape[0]), 1), dtype=torch.int32, device=dev)
    if _count(v, f, org, hi, identity) >= target:
        return hi
    if _count(v, f, org, lo, identity) < target:
        raise ValueError('the mesh keeps fewer than %d faces even at cell %g' % (target, lo))
    for _ in range(int(iters)):
        mid = float(np.float32(0.5 * (lo + hi)))
        if mid <= lo or mid >= hi:
            break
        if _count(v, f, org, mid, identity) >= target:
            lo = mid
        else:
            hi = mid
    return lo
