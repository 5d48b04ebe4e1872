"""Arbitrary rays against a triangle mesh on the GPU: closest hits, shadow rays, and from them virtual scanner sweeps
and visibility.  Where render.render_depth looks at a mesh through a pinhole camera, this module takes any origin and
direction: the spinning LiDAR, the panoramic rig and the single "can this eye see that sample" query.

The reference project has no counterpart; the rules this module follows are listed in INTEGRATION.md section W, and that
text is the contract of the kernel (sgnn_amd/csrc/raytrace.hip) and of the independent NumPy restatement of the tests
(tests/raytrace_ref.py).

    scene = Scene(verts, faces, cell=None, colors=None)            # wraps a meshdist.TriangleIndex with a guard
    hits = scene.closest(origins, dirs, t_min=0.0, t_max=inf)      # Hits(t (R,), face (R,), uv (R, 2)) on the device
    blocked = scene.occluded(origins, targets, eps=1e-4)           # (R,) bool: something between origin and target
    dirs = lidar_dirs(32, 1024) | panorama_dirs(h, w) | camera_dirs(K, (h, w))
    pts, org, oid, cols = sweep(scene, sensor2world, dirs)         # what points.integrate takes
    seen = visible_from(scene, samples, eyes)                      # (P,) bool: unoccluded from at least one eye

verts (V, 3) fp32 and faces (T, 3) int32 may be numpy arrays or torch tensors, host or device, as meshdist takes them.
The host layer does plumbing only: the pattern tables, the rotation of a pattern by each pose, the compaction of the
hits and the barycentric colour mix, each as single-rounded elementwise fp32 operations in the order section W states.

Deviation, stated in section W rule 5: every face is tested on its own, so a ray within rounding of an edge that two
faces share can miss both.  Nothing here is watertight.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._glue import host as _host, to_device as _to_device
from .meshdist import TriangleIndex

GUARD = 1.0 / 64.0          # the guard of rule W.4 in cells
F32 = np.float32


class Hits(NamedTuple):
    """t (R,) fp32 ray parameter (+inf: miss), face (R,) int32 (-1: miss), uv (R, 2) fp32 barycentrics of b and c."""
    t: torch.Tensor
    face: torch.Tensor
    uv: torch.Tensor

    def points(self, origins, dirs):
        """(R, 3) fp32 hit points origin + t dir (one product, one sum per component); NaN where the ray missed."""
        o = _to_device(origins, torch.float32, self.t.device)
        d = _to_device(dirs, torch.float32, self.t.device)
        p = o + self.t[:, None] * d
        return torch.where((self.face >= 0)[:, None], p, torch.full_like(p, float('nan')))


def _rays(name, x):
    shape = tuple(x.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError('%s must be (R, 3), got %s' % (name, shape))
    return shape[0]


def _counters_ok(counters):
    if counters is not None and not (torch.is_tensor(counters) and counters.is_cuda and counters.dtype == torch.int64
                                     and counters.numel() == 2 and counters.is_contiguous()):
        raise ValueError('counters must be a contiguous device int64 tensor of 2')


class Scene:
    """A mesh ready for ray queries: a meshdist.TriangleIndex whose faces are listed with a guard of cell / 64.

    cell: grid pitch, None takes the index's default.  colors: per-vertex (V, 3|4) uint8, mixed at the hits by `sweep`.
    Raises ValueError as TriangleIndex does."""

    def __init__(self, verts, faces, cell=None, colors=None):
        if colors is not None:
            cs = tuple(colors.shape)
            if len(cs) != 2 or cs[0] != int(verts.shape[0]) or cs[1] not in (3, 4):
                raise ValueError('colors must be (%d, 3|4), got %s' % (int(verts.shape[0]), cs))
            if colors.dtype != (torch.uint8 if torch.is_tensor(colors) else np.uint8):
                raise ValueError('colors must be uint8')
        self.index = TriangleIndex(verts, faces, cell, guard=GUARD)
        self.device = self.index.device
        self.colors = self.faces = None
        if colors is not None:
            self.colors = _to_device(colors, torch.uint8, self.device)
            self.faces = _to_device(faces, torch.int64, self.device)

    def _grid(self):
        ix = self.index
        return (ix.packed.records.data_ptr(), ix.offsets.data_ptr(), ix.refs.data_ptr(), float(ix.lo[0]),
                float(ix.lo[1]), float(ix.lo[2]), float(ix.cell)) + ix.dims + (float(ix.guard),)

    def _keys(self, o, d, t_min):
        """Approximate linear cell in which every ray enters the grid: the order of the sorted hand-over only."""
        ix = self.index
        lo = torch.from_numpy(ix.lo).to(o.device) - float(ix.guard)
        hi = lo + torch.tensor(ix.dims, device=o.device, dtype=torch.float32) * float(ix.cell) + 2 * float(ix.guard)
        a, b = (lo - o) / d, (hi - o) / d
        near = torch.nan_to_num(torch.minimum(a, b), nan=-3e38, posinf=3e38, neginf=-3e38).amax(1)
        t0 = near.clamp_(min=float(t_min))
        return ix._keys(o + t0[:, None] * d)

    def _trace(self, entry, o, d, t_min, t_max, cull_back, outs, counters, sort):
        n = int(o.shape[0])
        if n == 0:
            return outs
        order = None
        if sort:
            order = torch.argsort(self._keys(o, d, t_min))
            o, d = o[order].contiguous(), d[order].contiguous()
            if torch.is_tensor(t_max):
                t_max = t_max[order].contiguous()
        _lib.call(entry, o.data_ptr(), d.data_ptr(), n, float(t_min),
                  t_max.data_ptr() if torch.is_tensor(t_max) else float(t_max), *self._grid(), int(bool(cull_back)),
                  *[x.data_ptr() for x in outs], _lib.ptr(counters))
        if order is not None:
            outs = tuple(torch.empty_like(x).index_copy_(0, order, x) for x in outs)
        return outs

    def closest(self, origins, dirs, t_min=0.0, t_max=float('inf'), cull_back=False, counters=None, sort=False):
        """The closest hit of every ray origin + t dir with t_min < t < t_max: Hits on the device.

        dirs are used as given, not normalised: t is the ray parameter (the range for unit dirs, the z-depth for
        camera_dirs).  The result is the smallest t over all usable faces, the lowest face index among equal t; a miss,
        a non-finite ray and a zero direction give +inf, -1 and uv = 0.  cull_back: only faces seen from their front
        (counter-clockwise) side.  counters: None, or a device int64 tensor of 2 that receives cells visited and (ray,
        face) pairs tested.  sort: hand the rays to the kernel ordered by entry cell; the result does not depend on it.
        Off by default: on coherent camera rays the sort costs more than it gains (Speed)."""
        n = _rays('origins', origins)
        if _rays('dirs', dirs) != n:
            raise ValueError('%d origins for %d dirs' % (n, int(dirs.shape[0])))
        t_min, t_max = float(F32(t_min)), float(F32(t_max))
        if not (np.isfinite(t_min) and t_min < t_max):
            raise ValueError('t_min must be finite and below t_max')
        _counters_ok(counters)
        o = _to_device(origins, torch.float32, self.device)
        d = _to_device(dirs, torch.float32, self.device)
        outs = (torch.empty(n, dtype=torch.float32, device=self.device),
                torch.empty(n, dtype=torch.int32, device=self.device),
                torch.empty((n, 2), dtype=torch.float32, device=self.device))
        return Hits(*self._trace('sgnn_raytrace_closest', o, d, t_min, t_max, cull_back, outs, counters, sort))

    def occluded(self, origins, targets, eps=1e-4, counters=None, sort=False):
        """(R,) bool on the device: some face is hit on the segment origin -> target, at a parameter t of
        origin + t (target - origin) with eps < t < 1 - eps, so that a surface the segment starts or ends on does not
        block it.  origins and targets are (R, 3); either may be (1, 3) and is then shared by all rays."""
        no, nt = _rays('origins', origins), _rays('targets', targets)
        if no != nt and 1 not in (no, nt):
            raise ValueError('%d origins for %d targets' % (no, nt))
        eps = float(F32(eps))
        if not 0.0 <= eps < 0.5:
            raise ValueError('eps must be in [0, 0.5)')
        _counters_ok(counters)
        n = max(no, nt) if min(no, nt) else 0
        o = _to_device(origins, torch.float32, self.device).expand(n, 3).contiguous()
        d = _to_device(targets, torch.float32, self.device).expand(n, 3) - o
        t_max = torch.full((n,), float(F32(1.0) - F32(eps)), dtype=torch.float32, device=self.device)
        hit = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._trace('sgnn_raytrace_occluded', o, d, eps, t_max, False, (hit,), counters, sort)[0].bool()

    def hit_colors(self, hits):
        """(R, C) uint8 barycentric mix of the vertex colours at the hits (rule W.6); rows of missed rays are 0."""
        if self.colors is None:
            raise ValueError('the scene was built without colors')
        f = self.faces[hits.face.long().clamp(min=0)]
        c0, c1, c2 = (self.colors[f[:, k]].float() for k in range(3))
        u, v = hits.uv[:, :1], hits.uv[:, 1:]
        w = (1.0 - u) - v
        mix = ((w * c0 + u * c1) + v * c2 + 0.5).floor().clamp(0.0, 255.0).to(torch.uint8)
        return torch.where((hits.face >= 0)[:, None], mix, torch.zeros_like(mix))


# ---------------------------------------------------------------------------------------------------------
# ray patterns in the sensor frame (fp64 tables rounded once to fp32)
# ---------------------------------------------------------------------------------------------------------
def lidar_dirs(channels=32, steps=1024, fov_up=15.0, fov_down=-25.0):
    """(channels * steps, 3) fp32 unit directions of a spinning scanner, x forward, y left, z up: channel c has the
    elevation fov_up + (fov_down - fov_up) c / (channels - 1) degrees (the middle of the two for one channel), step s
    the azimuth 2 pi s / steps; row c * steps + s is (cos el cos az, cos el sin az, sin el)."""
    channels, steps = int(channels), int(steps)
    if channels < 1 or steps < 1 or not (-90.0 <= float(fov_down) <= float(fov_up) <= 90.0):
        raise ValueError('lidar_dirs needs channels, steps >= 1 and -90 <= fov_down <= fov_up <= 90')
    c = np.arange(channels, dtype=np.float64) / (channels - 1) if channels > 1 else np.array([0.5])
    el = np.radians(float(fov_up) + (float(fov_down) - float(fov_up)) * c)
    az = 2.0 * np.pi * np.arange(steps, dtype=np.float64) / steps
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None], np.cos(el)[:, None] * np.sin(az)[None],
                  np.repeat(np.sin(el)[:, None], steps, 1)], -1)
    return torch.from_numpy(d.reshape(-1, 3).astype(F32))


def panorama_dirs(h, w):
    """(h * w, 3) fp32 unit directions through the pixel centres of an equirectangular image, x forward, y left, z up:
    pixel (u, v) has the longitude pi - 2 pi (u + 0.5) / w (left to right) and the latitude pi / 2 - pi (v + 0.5) / h
    (top to bottom); row v * w + u is (cos lat cos lon, cos lat sin lon, sin lat)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError('panorama_dirs needs h, w >= 1')
    lon = np.pi - 2.0 * np.pi * (np.arange(w, dtype=np.float64) + 0.5) / w
    lat = np.pi / 2.0 - np.pi * (np.arange(h, dtype=np.float64) + 0.5) / h
    d = np.stack([np.cos(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.sin(lon)[None],
                  np.repeat(np.sin(lat)[:, None], w, 1)], -1)
    return torch.from_numpy(d.reshape(-1, 3).astype(F32))


def camera_dirs(K, hw):
    """(h * w, 3) fp32 directions ((u - cx) / fx, (v - cy) / fy, 1) of a pinhole camera K = (fx, fy, cx, cy), fp32
    operations, row v * w + u: with z = 1 the ray parameter of a hit is its z-depth, as render.render_depth writes it."""
    k = _host(K, np.float32).reshape(-1)
    h, w = int(hw[0]), int(hw[1])
    if k.shape != (4,) or h < 1 or w < 1:
        raise ValueError('camera_dirs needs K = (fx, fy, cx, cy) and h, w >= 1')
    x = (np.arange(w, dtype=F32) - k[2]) / k[0]
    y = (np.arange(h, dtype=F32) - k[3]) / k[1]
    d = np.stack([np.repeat(x[None], h, 0), np.repeat(y[:, None], w, 1), np.ones((h, w), F32)], -1)
    return torch.from_numpy(d.reshape(-1, 3).astype(F32))


# ---------------------------------------------------------------------------------------------------------
# sweeps and visibility
# ---------------------------------------------------------------------------------------------------------
def sweep(scene, sensor2world, dirs, t_min=0.1, t_max=12.0):
    """Virtual scans of the scene: (points (P, 3) fp32, origins (S, 3) fp32, origin_id (P,) int32, colors (P, C) uint8
    or None), on the device, what points.integrate takes.

    sensor2world: (S, 4, 4) poses (or one (4, 4)); dirs: (D, 3) sensor-frame directions.  Ray s * D + j starts at the
    translation of pose s and runs along the rotated direction ((R0.x dx + R0.y dy) + R0.z dz, ...), fp32; all S * D
    rays are traced in one call, the misses are dropped and the order of the rest is kept."""
    poses = _host(sensor2world, np.float64)
    poses = poses[None] if poses.ndim == 2 else poses
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError('sensor2world must be (S, 4, 4), got %s' % (poses.shape,))
    nd = _rays('dirs', dirs)
    ns = poses.shape[0]
    dev = scene.device
    rot = torch.from_numpy(poses[:, :3, :3].astype(F32)).to(dev)
    org = torch.from_numpy(np.ascontiguousarray(poses[:, :3, 3].astype(F32))).to(dev)
    d = _to_device(dirs, torch.float32, dev)
    dx, dy, dz = d[None, :, 0, None], d[None, :, 1, None], d[None, :, 2, None]          # (1, D, 1)
    world = (rot[:, None, :, 0] * dx + rot[:, None, :, 1] * dy) + rot[:, None, :, 2] * dz   # (S, D, 3)
    world = world.reshape(-1, 3).contiguous()
    o = org[:, None, :].expand(ns, nd, 3).reshape(-1, 3).contiguous()
    hits = scene.closest(o, world, t_min=t_min, t_max=t_max)
    keep = torch.nonzero(hits.face >= 0).reshape(-1)
    pts = (o + hits.t[:, None] * world)[keep]
    oid = torch.arange(ns, dtype=torch.int32, device=dev)[:, None].expand(ns, nd).reshape(-1)[keep]
    cols = scene.hit_colors(hits)[keep].contiguous() if scene.colors is not None else None
    return pts.contiguous(), org, oid.contiguous(), cols


def visible_from(scene, samples, eyes, eps=1e-4, max_rays=1 << 22):
    """(P,) bool on the device: sample p is seen, without anything in between, from at least one of the eyes (E, 3).
    The eyes are taken in chunks of at most max_rays / P, so memory stays bounded."""
    npts, _ = _rays('samples', samples), _rays('eyes', eyes)
    s = _to_device(samples, torch.float32, scene.device)
    e = _to_device(eyes, torch.float32, scene.device)
    seen = torch.zeros(npts, dtype=torch.bool, device=scene.device)
    if npts == 0:
        return seen
    step = max(1, int(max_rays) // npts)
    for e0 in range(0, int(e.shape[0]), step):
        chunk = e[e0:e0 + step]
        ne = int(chunk.shape[0])
        o = s[:, None, :].expand(npts, ne, 3).reshape(-1, 3)
        t = chunk[None, :, :].expand(npts, ne, 3).reshape(-1, 3)
        seen |= ~scene.occluded(o, t, eps=eps).reshape(npts, ne).all(1)
    return seen
