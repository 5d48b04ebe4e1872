"""Fairing triangle meshes on the GPU: vertex adjacency with edge multiplicities and boundary vertices, Laplacian and
Taubin smoothing, face and vertex normals, and feature-preserving denoising by filtered face normals (Sun et al. 2007).

Marching cubes gives a mesh that carries the staircase of the grid and the noise of the sensor or of the network; this
takes both out without taking the mesh off the device.  Topology never changes: faces and colours pass through, only
vertex positions are returned.  The reference project has no counterpart; the rules this module follows are listed in
INTEGRATION.md section Y, and that text is the contract of the kernels (sgnn_amd/csrc/smooth.hip) and of the independent
NumPy restatement of the tests (tests/smooth_ref.py).  The result is a pure function of the input, the same bits on
every run.

    adj = Adjacency(faces, num_verts)            # built once, reused by every call below
    #   adj.start (V+1,) i64, adj.neighbor (E2,) i32 ascending per vertex, adj.mult (E2,) u8,
    #   adj.kind (V,) u8: ISOLATED / INTERIOR / BOUNDARY / NONMANIFOLD, adj.boundary_edges() -> (B,2) i32
    v1 = laplacian(verts, adj, iterations=5, lam=0.5, boundary='curve', fixed=None)
    v1 = taubin(verts, adj, iterations=10, lam=0.5, mu=-0.53, boundary='curve', fixed=None)
    fn = face_normals(verts, faces)              # (F,3) unit, 0 for a face without area
    vn = vertex_normals(verts, faces)            # (V,3) unit, area-weighted, 0 where no face has area
    v1 = denoise(verts, faces, normal_iterations=5, vertex_iterations=10, threshold=0.4, adj=None, fixed=None)

verts (V, 3) fp32 and faces (F, 3) int32 may be numpy arrays or torch tensors, host or device, as simplify takes them;
results are device tensors and the inputs are not written.  Every call that takes adj also takes the faces in its place
and builds the adjacency itself.  The host layer does plumbing only: the sort of the edge keys and of the corners
(torch.sort), the scans of their counts and _glue.compact; it does no arithmetic on coordinates.
"""
import numpy as np
import torch

from . import _lib
from ._glue import compact, source_device, to_device

ISOLATED, INTERIOR, BOUNDARY, NONMANIFOLD = 0, 1, 2, 3
BOUNDARIES = ('fixed', 'curve', 'free')        # the mode numbers of sgnn_smooth_step
STATUS_RANGE = 1            # SGNN_STATUS_COORD_RANGE
LIMIT = 2 ** 31
# floats per row of the ping-pong buffers of the umbrella steps: 3, or 4 for rows padded to 16 bytes.  The result does
# not depend on it; scripts/bench_smooth.py measures both.
ROW_FLOATS = 3


def _rows(name, x):
    shape = tuple(np.shape(x))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('%s must be (N, 3), got %s' % (name, shape))
    return shape[0]


def _mesh_shape(verts, faces):
    nv, nt = _rows('verts', verts), _rows('faces', faces)
    if nv >= LIMIT or nt * 6 >= LIMIT:
        raise ValueError('%d vertices / %d faces do not fit 31 bits' % (nv, nt))
    return nv, nt


def _count(name, n):
    if int(n) != n or n < 0:
        raise ValueError('%s must be a non-negative integer, got %r' % (name, n))
    return int(n)


def _factor(name, x):
    f = float(np.float32(x))
    if not np.isfinite(f):
        raise ValueError('%s must be a finite fp32 number, got %r' % (name, x))
    return f


def _fixed_shape(fixed, nv):
    if fixed is not None and tuple(np.shape(fixed)) != (nv,):
        raise ValueError('fixed must be (%d,), got %s' % (nv, tuple(np.shape(fixed))))


def _faces(faces, dev):
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.array(faces))       # a copy: the input may be read-only
    if f.dtype != torch.int32:      # an index that int32 cannot hold is out of range whatever V is
        f = f.to(dev).long().clamp(-1, LIMIT - 1)
    return to_device(f, torch.int32, dev)


def _mask(fixed, dev):
    if fixed is None:
        return None
    t = fixed if torch.is_tensor(fixed) else torch.from_numpy(np.ascontiguousarray(np.asarray(fixed)))
    return (t.to(dev) != 0).to(torch.uint8).contiguous()


class Adjacency:
    """Rules 1 to 3: the neighbours of every vertex in ascending order (CSR: start, neighbor), the number of faces on
    every edge (mult, clamped to 255) and the kind of every vertex.  Built once per topology; one read-back."""

    def __init__(self, faces, num_verts):
        nt, nv = _rows('faces', faces), _count('num_verts', num_verts)
        if nv >= LIMIT or nt * 6 >= LIMIT:
            raise ValueError('%d vertices / %d faces do not fit 31 bits' % (nv, nt))
        dev = source_device(faces)
        f = _faces(faces, dev)
        n = 6 * nt
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nruns = 0
        if n:
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.call('sgnn_smooth_keys', _lib.ptr(f), nt, nv, _lib.ptr(keys), _lib.ptr(status))
            keys = torch.sort(keys).values
            flags = torch.empty(n, dtype=torch.uint8, device=dev)
            _lib.call('sgnn_smooth_run_flags', _lib.ptr(keys), n, _lib.ptr(flags))
            sel, count = compact(flags, n, dev, read=False)
            nruns, bad = torch.cat([count, status.long()]).tolist()      # the one read-back
            if bad & STATUS_RANGE:
                raise _lib.SgnnError('face index out of range [0, %d)' % nv)
        source = torch.empty(max(nruns, 1), dtype=torch.int32, device=dev)
        neighbor = torch.empty(max(nruns, 1), dtype=torch.int32, device=dev)
        mult = torch.empty(max(nruns, 1), dtype=torch.uint8, device=dev)
        start = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
        if nruns:
            _lib.call('sgnn_smooth_runs', _lib.ptr(keys), n, _lib.ptr(sel), nruns, _lib.ptr(source), _lib.ptr(neighbor),
                      _lib.ptr(mult))
            torch.cumsum(torch.bincount(source[:nruns], minlength=nv), 0, out=start[1:])
        kind = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)
        _lib.call('sgnn_smooth_classify', _lib.ptr(start), _lib.ptr(mult), nv, _lib.ptr(kind))
        self.num_verts, self.device = nv, dev
        self.start, self.kind = start, kind[:nv]
        self.source, self.neighbor, self.mult = source[:nruns], neighbor[:nruns], mult[:nruns]
        self._tables = (start, neighbor, mult, kind)       # never empty: a mesh without an edge still passes pointers

    def _ptrs(self):
        return tuple(_lib.ptr(t) for t in self._tables)

    def boundary_edges(self):
        """(B, 2) int32: the edges of multiplicity 1 as (a, b) with a < b, in ascending order."""
        n = int(self.neighbor.shape[0])
        if n == 0:
            return torch.empty((0, 2), dtype=torch.int32, device=self.device)
        mask = ((self.mult == 1) & (self.source < self.neighbor)).to(torch.uint8)
        sel, count = compact(mask, n, self.device)
        idx = sel[:count].long()
        return torch.stack([self.source[idx], self.neighbor[idx]], 1)


def _adjacency(adj, nv, dev_of):
    """adj as an Adjacency of nv vertices: itself, or built from the faces given in its place."""
    if isinstance(adj, Adjacency):
        if adj.num_verts != nv:
            raise ValueError('the adjacency has %d vertices and verts %d' % (adj.num_verts, nv))
        return adj
    return Adjacency(_faces(adj, source_device(*dev_of)), nv)


def _umbrella(verts, adj, iterations, factors, boundary, fixed):
    nv = _rows('verts', verts)
    if not isinstance(adj, Adjacency):
        _mesh_shape(verts, adj)
    if boundary not in BOUNDARIES:
        raise ValueError('boundary must be one of %s, got %r' % (BOUNDARIES, boundary))
    iterations = _count('iterations', iterations)
    factors = [_factor(name, x) for name, x in factors]
    _fixed_shape(fixed, nv)
    adj = _adjacency(adj, nv, (verts, adj))
    dev = adj.device
    v = to_device(verts, torch.float32, dev)
    if iterations == 0 or nv == 0:
        return v.clone()
    fx = _mask(fixed, dev)
    rows = ROW_FLOATS
    if rows == 4:
        src = torch.zeros((nv, 4), dtype=torch.float32, device=dev)
        src[:, :3] = v
    else:
        src = v
    bufs = [torch.empty((nv, rows), dtype=torch.float32, device=dev) for _ in range(2)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    step = 0
    for _ in range(iterations):
        for f in factors:
            dst = bufs[step & 1]
            _lib.call('sgnn_smooth_step', _lib.ptr(src), _lib.ptr(dst), nv, rows, *adj._ptrs(), _lib.ptr(fx),
                      BOUNDARIES.index(boundary), f, _lib.ptr(status) if step == 0 else None)
            src = dst
            step += 1
    out = src[:, :3].contiguous() if rows == 4 else src
    if int(status.item()) & STATUS_RANGE:
        raise _lib.SgnnError('a vertex coordinate is not finite')
    return out


def laplacian(verts, adj, iterations=5, lam=0.5, boundary='curve', fixed=None):
    """verts after `iterations` umbrella steps x += lam * (mean of the neighbours - x): (V, 3) fp32 on the device.

    boundary says what a vertex on an open rim does: 'fixed' it stays, 'curve' it averages its rim neighbours only (the
    rim shrinks along itself and does not slide inwards), 'free' it moves like an interior vertex.  Vertices on an edge
    of more than two faces, vertices without an edge and vertices with fixed[i] set never move.  adj: an Adjacency, or
    the faces.  A non-finite coordinate and a face index outside [0, V) raise SgnnError."""
    return _umbrella(verts, adj, iterations, [('lam', lam)], boundary, fixed)


def taubin(verts, adj, iterations=10, lam=0.5, mu=-0.53, boundary='curve', fixed=None):
    """verts after `iterations` pairs of umbrella steps, one with lam and one with mu < -lam, which puts back the volume
    the first takes away (Taubin 1995).  Everything else as laplacian."""
    return _umbrella(verts, adj, iterations, [('lam', lam), ('mu', mu)], boundary, fixed)


def _mesh(verts, faces, *more):
    nv, nt = _mesh_shape(verts, faces)
    dev = source_device(verts, faces, *more)
    return to_device(verts, torch.float32, dev), _faces(faces, dev), nv, nt, dev


def _raw_normals(v, f, nv, nt, unit, status):
    out = torch.empty((nt, 3), dtype=torch.float32, device=v.device)
    _lib.call('sgnn_smooth_face_normals', _lib.ptr(v), nv, _lib.ptr(f), nt, int(unit), _lib.ptr(out), _lib.ptr(status))
    return out


def _corner_lists(f, nv, nt, status):
    """(order (3F,) i64, cstart (V+2,) i64): every vertex's corners in ascending number (rule 10)."""
    dev = f.device
    cstart = torch.zeros(nv + 2, dtype=torch.int64, device=dev)
    if nt == 0:
        return torch.empty(1, dtype=torch.int64, device=dev), cstart
    ckeys = torch.empty(3 * nt, dtype=torch.int32, device=dev)
    _lib.call('sgnn_smooth_corners', _lib.ptr(f), nt, nv, _lib.ptr(ckeys), _lib.ptr(status))
    order = torch.sort(ckeys, stable=True).indices
    torch.cumsum(torch.bincount(ckeys, minlength=nv + 1), 0, out=cstart[1:])
    return order, cstart


def _raise_faces(status, nv):
    if int(status.item()) & STATUS_RANGE:
        raise _lib.SgnnError('face index out of range [0, %d)' % nv)


def face_normals(verts, faces):
    """(F, 3) fp32 unit normals (b - a) x (c - a) / length; (0, 0, 0) for a face without area or with a repeated
    index.  A face index outside [0, V) raises SgnnError."""
    v, f, nv, nt, dev = _mesh(verts, faces)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _raw_normals(v, f, nv, nt, True, status)
    _raise_faces(status, nv)
    return out


def vertex_normals(verts, faces):
    """(V, 3) fp32 unit normals: the sum of the unnormalised face normals on every vertex, which weights them by area;
    (0, 0, 0) where that sum has no length."""
    v, f, nv, nt, dev = _mesh(verts, faces)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    raw = _raw_normals(v, f, nv, nt, False, None)
    order, cstart = _corner_lists(f, nv, nt, status)
    out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    _lib.call('sgnn_smooth_vertex_normals', _lib.ptr(raw), nt, _lib.ptr(order), _lib.ptr(cstart), nv, _lib.ptr(out))
    _raise_faces(status, nv)
    return out


def denoise(verts, faces, normal_iterations=5, vertex_iterations=10, threshold=0.4, adj=None, fixed=None):
    """verts after feature-preserving denoising: the unit face normals are filtered normal_iterations times, every face
    taking the mean of the normals round it weighted by max(0, n_i . n_j - threshold)^2, so that normals across a sharp
    edge do not mix; then every vertex moves vertex_iterations times towards the planes of its faces' filtered normals.
    Vertices on an edge of more than two faces, vertices without an edge and vertices with fixed[i] set do not move; rim
    vertices do.  adj: the Adjacency of faces if there is one already.  (V, 3) fp32 on the device."""
    nv, nt = _mesh_shape(verts, faces)
    normal_iterations = _count('normal_iterations', normal_iterations)
    vertex_iterations = _count('vertex_iterations', vertex_iterations)
    threshold = _factor('threshold', threshold)
    _fixed_shape(fixed, nv)
    if adj is not None and not isinstance(adj, Adjacency):
        raise ValueError('adj must be an Adjacency or None')
    v, f, nv, nt, dev = _mesh(verts, faces, None if adj is None else adj.kind)
    adj = _adjacency(f if adj is None else adj, nv, (v,))
    if vertex_iterations == 0 or nv == 0:
        return v.clone()
    fx = _mask(fixed, dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)          # [0] coordinates, [1] face indices
    order, cstart = _corner_lists(f, nv, nt, status[1:])
    normals = _raw_normals(v, f, nv, nt, True, None)
    other = torch.empty_like(normals)
    for _ in range(normal_iterations if nt else 0):
        _lib.call('sgnn_smooth_filter', _lib.ptr(normals), _lib.ptr(other), _lib.ptr(f), nt, nv, _lib.ptr(order),
                  _lib.ptr(cstart), threshold)
        normals, other = other, normals
    src = v
    bufs = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    for step in range(vertex_iterations):
        dst = bufs[step & 1]
        _lib.call('sgnn_smooth_update', _lib.ptr(src), _lib.ptr(dst), nv, _lib.ptr(f), nt, _lib.ptr(normals),
                  _lib.ptr(order), _lib.ptr(cstart), adj._ptrs()[3], _lib.ptr(fx),
                  _lib.ptr(status) if step == 0 else None)
        src = dst
    coords, indices = status.tolist()
    if indices & STATUS_RANGE:
        raise _lib.SgnnError('face index out of range [0, %d)' % nv)
    if coords & STATUS_RANGE:
        raise _lib.SgnnError('a vertex coordinate is not finite')
    return src
