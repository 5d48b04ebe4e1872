"""Mesh-to-mesh distances on the GPU: the exact nearest triangle for many points, area-weighted surface samples,
and the mesh-level numbers completion papers report (accuracy, completeness, Chamfer distance, F-score).

The reference project has no counterpart; the rules this module follows are listed in INTEGRATION.md section G, and
that text is the contract of the kernels (sgnn_amd/csrc/meshdist.hip) and of the independent NumPy restatement of the
tests (tests/meshdist_ref.py).

    index = TriangleIndex(verts, faces)                       # uniform grid of triangle lists, on the device
    d, face = index.distance(points)                          # (P,) fp32 distance, (P,) int32 nearest face
    pts, fid = sample_surface(verts, faces, 100000)           # area-weighted, one sample per stratum, counter-based
    rep = compare(pred=(v0, f0), target=(v1, f1), n=1_000_000, thresholds=(0.05,))

verts (V, 3) fp32 and faces (T, 3) int32 may be numpy arrays or torch tensors, host or device, as render.render_depth
takes them; device meshes straight from marching cubes are not copied.  The host layer does plumbing only: the
bounding box, the scan between the count and the fill pass, areas and their cumulative sum, and the final means.
"""
import numpy as np
import torch

from . import _lib
from ._glue import binned_lists, mesh_shape, mesh_upload, pack_faces, to_device as _to_device

MAX_CELLS_AXIS = 1024       # cells per axis and in all that an index accepts (rule 5)
MAX_CELLS = 1 << 26
F32 = np.float32


def _mesh(verts, faces):
    """Checked device tensors (verts fp32 (V, 3), faces int32 (T, 3)) and whether the faces came from the device."""
    dev, (nv, nt) = mesh_shape(verts, faces)
    if nt == 0:
        raise ValueError('the mesh has no faces')
    if nt * 3 >= 2 ** 31:
        raise ValueError('3 T = %d does not fit 31 bits' % (nt * 3))
    return mesh_upload(verts, faces, nv, dev) + (dev,)


class _Packed:
    """Rule 1 and the per-face records of a mesh: records (T, 12) fp32, boxes (T, 6) fp32, usable (T,) uint8."""

    def __init__(self, verts, faces):
        v, f, on_device, dev = _mesh(verts, faces)
        nt = int(f.shape[0])
        self.device, self.ntri = dev, nt
        self.records, self.boxes, self.usable = pack_faces(v, f, on_device, dev)
        ids = torch.nonzero(self.usable).reshape(-1)
        self.n_usable = int(ids.numel())
        if self.n_usable == 0:
            raise ValueError('the mesh has no usable face (all %d have a non-finite vertex or no area)' % nt)
        self.last_usable = int(ids[-1].item())


def default_cell(packed, lo, hi):
    """Twice the median edge length of the usable faces, not below the largest extent / 256 (fp32)."""
    r = packed.records[packed.usable.bool()]
    ab, ac = r[:, 4:7], r[:, 8:11]
    edges = torch.cat([ab.norm(dim=1), ac.norm(dim=1), (ac - ab).norm(dim=1)])
    med = float(edges.median().item())
    floor = float(np.max(hi.astype(np.float64) - lo.astype(np.float64))) / 256.0
    cell = max(2.0 * med, floor) if np.isfinite(med) else floor
    return F32(cell)


class TriangleIndex:
    """Uniform grid of triangle lists over a mesh, on the device (rule 5).

    cell: grid pitch in the units of verts; None takes default_cell.  Raises ValueError for a malformed mesh, a face
    index out of range, a mesh without a usable face, and a pitch so small that the grid or its (face, cell)
    reference list would not fit.  guard: every face is listed in the cells of its box grown by guard * cell on every
    side (raytrace.Scene, section W rule 4); 0 lists it in the cells its own box touches, all that `distance` needs."""

    def __init__(self, verts, faces, cell=None, guard=0.0):
        self._build(_Packed(verts, faces), cell, guard)

    @classmethod
    def _from_packed(cls, packed, cell=None):
        index = cls.__new__(cls)
        index._build(packed, cell)
        return index

    def _build(self, p, cell, guard=0.0):
        self.packed, self.device = p, p.device
        self.lo = p.boxes[:, :3].amin(0).cpu().numpy().astype(F32)          # ignored faces hold (+inf, -inf)
        self.hi = p.boxes[:, 3:].amax(0).cpu().numpy().astype(F32)
        if cell is None:
            cell = default_cell(p, self.lo, self.hi)
        self.cell = F32(cell)
        if not (np.isfinite(self.cell) and self.cell > 0):
            raise ValueError('cell must be positive and finite, got %r' % (cell,))
        with np.errstate(all='ignore'):
            span = np.floor(((self.hi - self.lo).astype(F32) / self.cell).astype(F32)).astype(np.float64) + 1
        if not np.isfinite(span).all() or span.max() > MAX_CELLS_AXIS or span.prod() > MAX_CELLS:
            raise ValueError('cell = %g gives a grid of %s cells (at most %d per axis and %d in all): choose a larger cell'
                             % (self.cell, 'x'.join('%.0f' % s for s in span), MAX_CELLS_AXIS, MAX_CELLS))
        self.dims = tuple(int(s) for s in span)                              # nx, ny, nz
        ncell = self.dims[0] * self.dims[1] * self.dims[2]
        grid = (float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), float(self.cell)) + self.dims
        self.guard = F32(F32(guard) * self.cell)
        if not (np.isfinite(self.guard) and self.guard >= 0):
            raise ValueError('guard must be finite and not negative, got %r' % (guard,))
        boxes = p.boxes
        if self.guard > 0:                                                   # ignored faces keep (+inf, -inf)
            boxes = torch.cat([boxes[:, :3] - float(self.guard), boxes[:, 3:] + float(self.guard)], 1).contiguous()
        self.offsets, self.refs, self.n_refs = binned_lists(
            'sgnn_meshdist_count', 'sgnn_meshdist_fill', (boxes.data_ptr(), p.ntri) + grid, ncell, self.device,
            '%%d (face, cell) references do not fit 31 bits at cell = %g: choose a larger cell' % self.cell)

    def _keys(self, pts):
        """Approximate linear cell of every point: the order of the sorted hand-over only."""
        lo = torch.from_numpy(self.lo).to(pts.device)
        dims = torch.tensor(self.dims, device=pts.device, dtype=torch.float32)
        c = torch.nan_to_num(((pts - lo) / float(self.cell)).floor(), nan=0.0, posinf=3e9, neginf=-3e9)
        c = torch.minimum(c.clamp_(min=0.0), dims - 1).to(torch.int64)
        return (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]

    def distance(self, points, max_dist=None, counters=None, sort=False):
        """Distance to the mesh and the nearest face for points (P, 3): (P,) fp32 and (P,) int32 on the device.

        The result is the minimum over all usable faces, the lowest face index among equals; a non-finite point
        gives +inf and -1.  max_dist: results above it become +inf and -1, the others are unchanged (None: exact and
        unbounded).  A point far from every face walks shells until the bound reaches its distance, so pass max_dist
        whenever the mesh may cover only part of the points (a partial scan against the full scene).  counters: None,
        or a device int64 tensor of 2 that receives cells visited and (point, face) pairs evaluated.  sort: hand the
        points to the kernel ordered by cell; the result does not depend on it.  Off by default: measured at 1 M
        points it costs 0.97 against 0.64 ms where points lie near the surface and gains 7 % where walks are long."""
        shape = tuple(points.shape)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError('points must be (P, 3), got %s' % (shape,))
        if max_dist is not None and not float(max_dist) >= 0.0:
            raise ValueError('max_dist must be >= 0')
        if counters is not None and not (torch.is_tensor(counters) and counters.is_cuda and counters.dtype == torch.int64
                                         and counters.numel() == 2 and counters.is_contiguous()):
            raise ValueError('counters must be a contiguous device int64 tensor of 2')
        pts = _to_device(points, torch.float32, self.device)
        n = int(pts.shape[0])
        d = torch.empty(n, dtype=torch.float32, device=self.device)
        face = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return d, face
        order = None
        if sort:
            order = torch.argsort(self._keys(pts))
            pts = pts[order].contiguous()
        md = float('inf') if max_dist is None else float(F32(max_dist))
        _lib.call('sgnn_meshdist_query', pts.data_ptr(), n, self.packed.records.data_ptr(), self.offsets.data_ptr(),
                  self.refs.data_ptr(), float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), float(self.hi[0]),
                  float(self.hi[1]), float(self.hi[2]), float(self.cell), *self.dims, md, d.data_ptr(), face.data_ptr(),
                  _lib.ptr(counters))
        if order is not None:
            d, face = torch.empty_like(d).index_copy_(0, order, d), torch.empty_like(face).index_copy_(0, order, face)
        return d, face


def face_areas(packed):
    """fp64 areas of the faces from the fp32 records (0 for an ignored face) and their cumulative sum, on the device."""
    r = packed.records.double()
    area = 0.5 * torch.linalg.cross(r[:, 4:7], r[:, 8:11]).norm(dim=1)
    area = torch.where(packed.usable.bool(), area, torch.zeros_like(area))
    return area, torch.cumsum(area, 0)


def sample_surface(verts, faces, n, seed=0, return_table=False):
    """n area-weighted points on the usable faces, one per stratum of the cumulative area: (n, 3) fp32 points and
    (n,) int32 faces on the device (rule 6).  The same seed gives the same bits.
    return_table adds the fp64 cumulative areas the kernel searched."""
    return _sample(_Packed(verts, faces), n, seed, return_table)


def _sample(p, n, seed, return_table=False):
    n = int(n)
    if n < 0 or n >= 2 ** 31:
        raise ValueError('n must be in [0, 2^31), got %d' % n)
    pts = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    fid = torch.empty(n, dtype=torch.int32, device=p.device)
    _, cum = face_areas(p)
    if n:
        _lib.call('sgnn_mesh_sample', p.records.data_ptr(), cum.data_ptr(), p.ntri, p.last_usable, n,
                  int(np.uint64(int(seed) & (2 ** 64 - 1)).astype(np.int64)), pts.data_ptr(), fid.data_ptr())
    return (pts, fid, cum) if return_table else (pts, fid)


def summarise(d_pred, d_target, thresholds=(0.05,), max_dist=None):
    """The report of compare() from the two distance tensors: fp64 means, exact integer counts."""
    rep = {'pred_to_target': d_pred, 'target_to_pred': d_target}
    cap = float('inf') if max_dist is None else float(F32(max_dist))
    means = []
    for d in (d_pred, d_target):
        x = d.double()
        x = torch.where(torch.isinf(x), torch.full_like(x, cap), x) if max_dist is not None else x
        means.append(float(x.mean().item()) if x.numel() else float('nan'))
    rep['accuracy'], rep['completeness'] = means
    rep['chamfer'] = means[0] + means[1]
    rep['thresholds'] = tuple(float(t) for t in thresholds)
    rep['hits_pred'] = [int((d_pred <= float(F32(t))).sum().item()) for t in thresholds]
    rep['hits_target'] = [int((d_target <= float(F32(t))).sum().item()) for t in thresholds]
    rep['precision'] = [h / max(d_pred.numel(), 1) for h in rep['hits_pred']]
    rep['recall'] = [h / max(d_target.numel(), 1) for h in rep['hits_target']]
    rep['fscore'] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(rep['precision'], rep['recall'])]
    return rep


def compare(pred, target, n=1_000_000, thresholds=(0.05,), seed=0, max_dist=None, cell=None):
    """Mesh-level comparison of a predicted mesh with a target mesh, both (verts, faces).

    n points are sampled on each surface (seed on pred, seed + 1 on target) and measured against the other mesh.
    Returns a dict: accuracy (mean pred -> target distance), completeness (mean target -> pred), chamfer (their sum),
    per threshold precision (share of pred points within it), recall (share of target points) and fscore, the exact
    counts behind them (hits_pred, hits_target) and the two distance tensors (pred_to_target, target_to_pred).  With
    max_dist, distances above it count as max_dist in the means and as misses.  Pass max_dist when one mesh covers
    only part of the other (a partial scan): without it the points far from every face dominate the run time (879 ms
    against 1.8 ms with max_dist = 0.1 for 1 M points in scripts/bench_meshdist.py)."""
    packs = [_Packed(*pred), _Packed(*target)]
    samples = [_sample(pk, n, seed + k)[0] for k, pk in enumerate(packs)]
    d_pred = TriangleIndex._from_packed(packs[1], cell).distance(samples[0], max_dist)[0]
    d_target = TriangleIndex._from_packed(packs[0], cell).distance(samples[1], max_dist)[0]
    return summarise(d_pred, d_target, thresholds, max_dist)
