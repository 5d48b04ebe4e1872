"""TSDF fusion on the GPU: depth frames -> scan volume -> .sdf / .knw files or a model input.

The reference makes its scan volumes with datagen/GenerateScans (Scene.cpp:167-200 raw depth, CameraUtil.h:25-63
bilateral filter, VoxelGrid.cpp:6-63 / VoxelGrid.h:120-216,350-400 integration, export and known codes, Fuser.cpp
the subset / all-frames pair).  That tool depends on a Windows-only library; the rules it follows are restated in
INTEGRATION.md "TSDF fusion", and that text is the contract these kernels (sgnn_amd/csrc/fusion.hip) and the
independent NumPy restatement of the tests (tests/fusion_ref.py) both follow.

    depth, K = raw_depth_to_metric(raw_u16, 1000.0, (240, 320), intrinsics=K_raw)
    vol = TSDFVolume((dx, dy, dz), 0.02, world2grid)
    vol.integrate(bilateral(depth), K, cam2world)           # all frames in one call, no per-frame host loop
    # with TSDFVolume(..., color=True): vol.integrate(..., color=pack_color(rgb, (240, 320))); vol.colors()
    vol.save('scene.sdf')                                    # + scene.knw, readable by data.load_scene / loaders
    sample = scan_sample(vol)                                # or straight to a model input on the device

The host does per-frame geometry only (a 3x4 matrix and a voxel box per frame); every per-voxel and per-pixel
step runs on the device.
"""
import numpy as np
import torch

from . import _lib, data
from ._glue import (cameras, compact, device as _device, host as _host, source_device as _source_device,
                    to_device as _to_device)

# struct sgnn_fuse_frame (include/sgnn_hip.h)
FRAME_DTYPE = np.dtype([('m', '<f4', (12,)), ('intr', '<f4', (4,)), ('box', '<i4', (6,)), ('offset', '<i8')])
assert FRAME_DTYPE.itemsize == 96

# frames per integration launch, 0 = all in one.  scripts/bench_fusion.py on the MI355X (1000 frames, 512x512x128):
# 1 -> 108 ms, 8 -> 71, 64 -> 66, all -> 53 (profiles/fusion_bench.json)
DEFAULT_CHUNK = 0
EMPTY_BOX = np.array([0, -1, 0, -1, 0, -1], dtype=np.int32)


def round_half_away(x):
    """std::round in the array's own precision: halves go away from zero (numpy's round goes to even)."""
    x = np.asarray(x)
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0).astype(x.dtype)


def _affine(m, p):
    """m (.., 3|4, 4) applied to points p (.., 3) in m's precision, order ((m0 x + m1 y) + m2 z) + m3 per row."""
    return np.stack([((m[..., r, 0] * p[..., 0] + m[..., r, 1] * p[..., 1]) + m[..., r, 2] * p[..., 2]) + m[..., r, 3]
                     for r in range(3)], -1)


# ---------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------
def adapt_intrinsics(intrinsics, raw_hw, out_hw):
    """(fx, fy, cx, cy) of a (h_raw, w_raw) sensor for frames resampled to (h, w) (Scene.cpp:180-183), fp32."""
    k = _host(intrinsics, np.float32).copy()
    (hr, wr), (h, w) = raw_hw, out_hw
    f32 = np.float32
    k[..., 0] *= f32(w) / f32(wr)
    k[..., 1] *= f32(h) / f32(hr)
    k[..., 2] *= f32(w - 1) / f32(wr - 1)
    k[..., 3] *= f32(h - 1) / f32(hr - 1)
    return k


def raw_depth_to_metric(raw_u16, depth_shift, out_hw, min_depth=0.1, max_depth=12.0, intrinsics=None):
    """uint16 frames (h_raw, w_raw) or (F, h_raw, w_raw) -> (metric fp32 depth on the device, (F,) h, w, with -inf
    for no data; the adapted intrinsics (fx, fy, cx, cy) as fp32 numpy, or None when none were given)."""
    dev = _source_device(raw_u16)
    if torch.is_tensor(raw_u16) and raw_u16.is_cuda and raw_u16.dtype in (torch.int16, getattr(torch, 'uint16', None)):
        raw = raw_u16.contiguous()
    else:
        arr = _host(raw_u16, np.uint16) if not torch.is_tensor(raw_u16) else raw_u16.cpu().numpy().astype(np.uint16)
        raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.int16)).to(dev)
    single = raw.dim() == 2
    raw3 = raw[None] if single else raw
    nf, hr, wr = (int(v) for v in raw3.shape)
    h, w = (int(v) for v in out_hw)
    out = torch.empty((nf, h, w), dtype=torch.float32, device=dev)
    _lib.call('sgnn_fuse_depth_raw', raw3.data_ptr(), nf, hr, wr, h, w, float(np.float32(depth_shift)),
              float(np.float32(min_depth)), float(np.float32(max_depth)), out.data_ptr())
    k = None if intrinsics is None else adapt_intrinsics(intrinsics, (hr, wr), (h, w))
    return (out[0] if single else out), k


def pack_color(rgb, out_hw=None):
    """uint8 colour frames (h_raw, w_raw, c) or (F, h_raw, w_raw, c), c = 3 (R, G, B) or 4 (R, G, B, A), numpy or
    torch, host or device -> the (F, h, w, 4) uint8 device stack TSDFVolume.integrate(color=) takes, resampled to
    out_hw = (h, w) by raw_depth_to_metric's nearest-index rule (None: the frames' own size).  A = 255 where the pixel
    has a colour (every pixel of 3-channel input, a != 0 of 4-channel input), else 0."""
    dev = _source_device(rgb)
    raw = _to_device(rgb if torch.is_tensor(rgb) else _host(rgb, np.uint8), torch.uint8, dev)
    if raw.dim() == 3:
        raw = raw[None]
    if raw.dim() != 4 or int(raw.shape[3]) not in (3, 4):
        raise ValueError('colour frames must be (F, h, w, 3|4) or (h, w, 3|4), got %s' % (tuple(raw.shape),))
    nf, hr, wr, ch = (int(v) for v in raw.shape)
    h, w = (hr, wr) if out_hw is None else (int(v) for v in out_hw)
    out = torch.empty((nf, h, w, 4), dtype=torch.uint8, device=dev)
    _lib.call('sgnn_fusecol_pack', raw.data_ptr(), nf, hr, wr, ch, h, w, out.data_ptr())
    return out


def bilateral(depth, sigma_d=2.0, sigma_r=0.1):
    """Bilateral filter of (h, w) or (F, h, w) metric depth (CameraUtil.h:25-63); -inf stays -inf."""
    dev = _source_device(depth)
    d = _to_device(depth, torch.float32, dev)
    d3 = d[None] if d.dim() == 2 else d
    out = torch.empty_like(d3)
    _lib.call('sgnn_fuse_bilateral', d3.data_ptr(), int(d3.shape[0]), int(d3.shape[1]), int(d3.shape[2]),
              float(sigma_d), float(sigma_r), out.data_ptr())
    return out[0] if d.dim() == 2 else out


def color_stack(color, dev):
    """What integrate(color=) was given -> the (F, h, w, 4) uint8 stack on dev: a stack that is already there is
    used as it is (the kernel only asks whether A != 0), anything else goes through pack_color at its own size."""
    if torch.is_tensor(color) and color.is_cuda and color.dtype == torch.uint8 and color.dim() == 4 and \
            int(color.shape[3]) == 4 and color.device == dev:
        return color.contiguous()
    return pack_color(color.to(dev) if torch.is_tensor(color) else color)


# ---------------------------------------------------------------------------------------------------------
# per-frame geometry (host)
# ---------------------------------------------------------------------------------------------------------
def camera_matrix(cam2world, world2grid):
    """Rows 0..2 of inv(cam2world) . inv(world2grid) (voxel -> camera), formed in fp64, rounded to fp32: (.., 3, 4)."""
    c2w = _host(cam2world, np.float64)
    g2w = np.linalg.inv(_host(world2grid, np.float64).reshape(4, 4))
    return (np.linalg.inv(c2w) @ g2w)[..., :3, :].astype(np.float32)


def frustum_box(intrinsics, cam2world, hw, world2grid, dims_xyz, depth_min=0.4, depth_max=4.0):
    """Voxel box (x0, x1, y0, y1, z0, z1), inclusive, that one frame can touch (VoxelGrid.h:350-377), all in fp32:
    the 8 image-corner points at depth_min / depth_max to world space, floor and ceil, round(world2grid . p), the
    box of those 16 points clamped to the grid.  A frame with a non-finite pose, or one that misses the grid, gets
    EMPTY_BOX (touches nothing)."""
    f32 = np.float32
    fx, fy, cx, cy = _host(intrinsics, f32).reshape(4)
    c2w = _host(cam2world, f32).reshape(4, 4)
    w2g = _host(world2grid, f32).reshape(4, 4)
    if not np.isfinite(c2w).all():
        return EMPTY_BOX.copy()
    h, w = hw
    pts = []
    for depth in (f32(depth_min), f32(depth_max)):
        for ux, uy in ((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)):
            x = (f32(ux) - cx) / fx
            y = (f32(uy) - cy) / fy
            pts.append([depth * x, depth * y, depth])
    world = _affine(c2w, np.array(pts, dtype=f32))
    grid = round_half_away(_affine(w2g, np.concatenate([np.floor(world), np.ceil(world)])))
    if not np.isfinite(grid).all():
        return EMPTY_BOX.copy()
    lo = np.maximum(grid.min(0), 0)
    hi = np.minimum(grid.max(0), np.array(dims_xyz, dtype=f32) - 1)
    if (lo > hi).any():
        return EMPTY_BOX.copy()
    return np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], dtype=np.int32)


def obb_contains(obb, q):
    """0 <= dot(q - a, e_k) <= dot(e_k, e_k) for the three edges of obb = (a, e0, e1, e2) (12 floats, voxel
    coordinates), in fp32; q (.., 3) voxel coordinates."""
    o = _host(obb, np.float32).reshape(4, 3)
    r = np.asarray(q, dtype=np.float32) - o[0]
    inside = np.ones(r.shape[:-1], dtype=bool)
    for e in o[1:]:
        d = (r[..., 0] * e[0] + r[..., 1] * e[1]) + r[..., 2] * e[2]
        ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        inside &= (d >= 0) & (d <= ee)
    return inside


# ---------------------------------------------------------------------------------------------------------
# the volume
# ---------------------------------------------------------------------------------------------------------
def check_dims(dims_xyz):
    """The limits of a volume's dims, before a device is needed -> the dims as a tuple of ints."""
    dims = tuple(int(d) for d in dims_xyz)
    if len(dims) != 3 or min(dims) < 1 or max(dims) > 65535 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('unsupported volume dimensions %s' % (dims,))
    return dims


class TSDFVolume(object):
    """A dense truncated signed-distance volume on the device, (dz, dy, dx) like the readers' arrays.

    dims_xyz: (dx, dy, dz) voxels; voxel_size in metres; world2grid: 4x4 (world metres -> voxel coordinates);
    depth_min / depth_max: the depths an observation may have; obb: optional (a, e0, e1, e2) in voxel
    coordinates, voxels outside it are never updated; color: also keep a colour per voxel,
    8 more bytes per voxel, fed by integrate(color=) and read with colors()."""

    def __init__(self, dims_xyz, voxel_size, world2grid, depth_min=0.4, depth_max=4.0, obb=None, device=None,
                 color=False):
        self.device = _device(device)
        self.dims_xyz = tuple(int(d) for d in dims_xyz)
        dx, dy, dz = check_dims(self.dims_xyz)
        self.voxel_size = np.float32(voxel_size)
        self.world2grid = _host(world2grid, np.float32).reshape(4, 4).copy()
        self.depth_min, self.depth_max = np.float32(depth_min), np.float32(depth_max)
        self.obb = None if obb is None else _host(obb, np.float32).reshape(12).copy()
        self._sdf = torch.full((dz, dy, dx), -float('inf'), dtype=torch.float32, device=self.device)
        self._weight = torch.zeros((dz, dy, dx), dtype=torch.uint8, device=self.device)
        self._free = torch.zeros((dz, dy, dx), dtype=torch.int32, device=self.device)
        # R, G, B in 8.8 fixed point and the colour weight, or None; held as int16 (torch fills and copies that type
        # everywhere), handed out as uint16
        self._color = torch.zeros((dz, dy, dx, 4), dtype=torch.int16, device=self.device) if color else None

    @property
    def dims_zyx(self):
        return self.dims_xyz[::-1]

    def _state(self, color):
        """The four pointers every entrance to the volume hands to the library (csrc/tsdf.h, TsdfVol); color False:
        None for the colour record."""
        return (self._sdf.data_ptr(), self._weight.data_ptr(), self._free.data_ptr(),
                self._color.data_ptr() if color else None)

    def frame_table(self, intrinsics, cam2world, hw):
        """Host table of sgnn_fuse_frame records for F frames of size hw = (h, w)."""
        k, c2w = cameras(intrinsics, cam2world)
        nf = k.shape[0]
        t = np.zeros(nf, dtype=FRAME_DTYPE)
        with np.errstate(all='ignore'):
            ok = np.isfinite(c2w).all(axis=(1, 2))
            m = np.zeros((nf, 3, 4), dtype=np.float32)
            if ok.any():
                m[ok] = camera_matrix(c2w[ok], self.world2grid)
        t['m'] = m.reshape(nf, 12)
        t['intr'] = k
        for f in range(nf):
            t['box'][f] = frustum_box(k[f], c2w[f], hw, self.world2grid, self.dims_xyz, self.depth_min,
                                      self.depth_max) if ok[f] else EMPTY_BOX
        t['offset'] = np.arange(nf, dtype=np.int64) * (int(hw[0]) * int(hw[1]))
        return t

    def integrate(self, depth, intrinsics, cam2world, chunk=None, color=None):
        """Fuse F frames in order.  depth (F, h, w) metres (-inf = invalid), intrinsics (F, 4) fx, fy, cx, cy,
        cam2world (F, 4, 4); torch tensors (host or device) or numpy arrays.  chunk: frames per launch (the result
        does not depend on it; None: DEFAULT_CHUNK).  color: the frames' colours for a volume built with color=True,
        a pack_color() stack or raw (F, h, w, 3|4) uint8 frames of the depth frames' size; None leaves the colours
        as they are."""
        d = _to_device(depth, torch.float32, self.device)
        if d.dim() == 2:
            d = d[None]
        nf, h, w = (int(v) for v in d.shape)
        if color is not None:
            if self._color is None:
                raise ValueError('colour frames for a volume built without color=True')
            color = color_stack(color, self.device)
            if tuple(color.shape) != (nf, h, w, 4):
                raise ValueError('colour frames %s for depth frames %s' % (tuple(color.shape[:3]), (nf, h, w)))
        table = self.frame_table(intrinsics, cam2world, (h, w))
        if table.shape[0] != nf:
            raise ValueError('%d depth frames for %d poses' % (nf, table.shape[0]))
        if nf == 0:
            return self
        dev_table = torch.from_numpy(table.view(np.uint8)).to(self.device)
        dx, dy, dz = self.dims_xyz
        obb = None if self.obb is None else self.obb.ctypes.data
        tail = (h, w, dev_table.data_ptr(), nf, int(DEFAULT_CHUNK if chunk is None else chunk),
                float(self.voxel_size), float(self.depth_min), float(self.depth_max), obb)
        if color is None:
            _lib.call('sgnn_fuse_integrate', *self._state(False)[:3], dx, dy, dz, d.data_ptr(), *tail)
        else:
            _lib.call('sgnn_fusecol_integrate', *self._state(True), dx, dy, dz, d.data_ptr(), color.data_ptr(), *tail)
        return self

    def sdf(self):
        return self._sdf

    def weight(self):
        return self._weight

    def free_count(self):
        return self._free

    def color_state(self):
        """(dz, dy, dx, 4) uint16: R, G, B in 8.8 fixed point and the colour weight; None without color=True."""
        return None if self._color is None else self._color.view(torch.uint16)

    def _export_color(self, want_weight):
        if self._color is None:
            raise ValueError('the volume was built without color=True')
        dx, dy, dz = self.dims_xyz
        rgb = torch.empty((dz, dy, dx, 3), dtype=torch.uint8, device=self.device)
        wc = torch.empty((dz, dy, dx), dtype=torch.uint8, device=self.device) if want_weight else None
        _lib.call('sgnn_fusecol_export', self._color.data_ptr(), dx * dy * dz, rgb.data_ptr(), _lib.ptr(wc))
        return rgb, wc

    def color_weight(self):
        """(dz, dy, dx) uint8: the weight behind each voxel's colour, 0 = no colour."""
        return self._export_color(True)[1]

    def colors(self, dims_zyx=None):
        """(dz, dy, dx, 3) uint8 R, G, B, black where a voxel has no colour: the colour volume that
        marching_cubes.run_marching_cubes takes next to sdf().  dims_zyx: zero-padded or cropped to those dims (the
        padded dense volume of a prediction)."""
        rgb = self._export_color(False)[0]
        if dims_zyx is None or tuple(int(v) for v in dims_zyx) == tuple(rgb.shape[:3]):
            return rgb
        out = torch.zeros(tuple(int(v) for v in dims_zyx) + (3,), dtype=torch.uint8, device=self.device)
        z, y, x = (min(int(a), int(b)) for a, b in zip(dims_zyx, rgb.shape[:3]))
        out[:z, :y, :x] = rgb[:z, :y, :x]
        return out

    def copy(self):
        """An independent snapshot (the input half of a subset / all-frames pair, Fuser.cpp:71-100)."""
        c = TSDFVolume.__new__(TSDFVolume)
        c.__dict__.update(self.__dict__)
        c._sdf, c._weight, c._free = self._sdf.clone(), self._weight.clone(), self._free.clone()
        c._color = None if self._color is None else self._color.clone()
        return c

    def _compact(self, keep_abs, truncation=0.0, max_z=1 << 40):
        dx, dy, dz = self.dims_xyz
        n = dx * dy * dz
        mask = torch.empty(n, dtype=torch.uint8, device=self.device)
        _lib.call('sgnn_fuse_flag', self._sdf.data_ptr(), dx, dy, dz, float(keep_abs), float(truncation),
                  float(self.voxel_size), int(max_z), mask.data_ptr())
        sel, count = compact(mask, n, self.device, read=False)
        return sel, count, int(count.item())

    def sparse(self, trunc_factor=6.0):
        """The .sdf block (VoxelGrid.h:120-150): voxels with |sdf| <= trunc_factor * voxel_size (fp32 product) in
        raster order, x fastest -> (locs (n, 3) int32 x, y, z; sdf (n,) fp32 metres), on the device."""
        keep = np.float32(trunc_factor) * self.voxel_size
        sel, count, m = self._compact(keep)
        locs = torch.empty((max(m, 1), 3), dtype=torch.int32, device=self.device)
        vals = torch.empty(max(m, 1), dtype=torch.float32, device=self.device)
        dx, dy, _ = self.dims_xyz
        _lib.call('sgnn_fuse_emit_block', self._sdf.data_ptr(), dx, dy, sel.data_ptr(), count.data_ptr(), m,
                  locs.data_ptr(), vals.data_ptr())
        return locs[:m], vals[:m]

    def known(self):
        """The .knw codes (VoxelGrid.h:199-216), (dz, dy, dx) uint8 on the device."""
        out = torch.empty_like(self._weight)
        _lib.call('sgnn_fuse_known', self._sdf.data_ptr(), self._sdf.numel(), float(self.voxel_size), out.data_ptr())
        return out

    def save(self, path_sdf, trunc_factor=6.0, known=True):
        """Write the sparse .sdf (data.write_scene) and, with known, the .knw next to it (data.write_known)."""
        locs, vals = self.sparse(trunc_factor)
        return write_scan(path_sdf, self.dims_zyx, self.voxel_size, self.world2grid, locs.cpu().numpy(),
                          vals.cpu().numpy(), self.known().cpu().numpy() if known else None)


def level_transform(level):
    """S_k (4x4, fp64) of pyramid level k, factor f = 2**k: fine voxel coordinates g0 -> (g0 - (f-1)/2) / f, the
    coordinates of the level whose voxel c is centred on the f**3 fine voxels f*c .. f*c + f-1 it covers."""
    f = float(2 ** int(level))
    s = np.eye(4, dtype=np.float64)
    s[:3, :3] /= f
    s[:3, 3] = -(f - 1.0) / (2.0 * f)
    return s


class TSDFPyramid(object):
    """The same frames fused at 1x, 2x, 4x, ... the voxel size: `levels` TSDFVolumes, the target hierarchy of a
    training chunk (chunks.ChunkCutter).  Host plumbing over the existing kernels: every level is an ordinary
    TSDFVolume and integrate() calls each level's integrate; there is no pyramid kernel.

    Level k (factor f = 2**k) has dims ceil(d / f), voxel size f * voxel_size (fp32 product) and world2grid_k =
    level_transform(k) @ world2grid, formed in fp64 from the fp32 world2grid that level 0 holds and rounded once to
    fp32.  An obb (a, e0, e1, e2 in fine voxel coordinates) is carried along: corner through S_k, edges / f, in fp64,
    rounded to fp32.  The integration kernel truncates at 3 voxel sizes of the volume it is given, so every level's
    band is three of its own voxels; a level-f value divided by f and by the fine voxel size (what the .sdfs route
    does) is the distance in level-f voxels, the convention of synth.block_arrays."""

    def __init__(self, dims_xyz, voxel_size, world2grid, levels=4, obb=None, **volume_kwargs):
        if int(levels) < 1:
            raise ValueError('a pyramid needs at least one level')
        w2g = _host(world2grid, np.float32).reshape(4, 4).astype(np.float64)
        vs = np.float32(voxel_size)
        self.volumes = []
        for k in range(int(levels)):
            f = 2 ** k
            s = level_transform(k)
            o = None
            if obb is not None:
                o64 = _host(obb, np.float64).reshape(4, 3)
                o = np.concatenate([o64[:1] @ s[:3, :3].T + s[:3, 3], o64[1:] / f]).astype(np.float32)
            self.volumes.append(TSDFVolume([-(-int(d) // f) for d in dims_xyz], np.float32(f) * vs,
                                           (s @ w2g).astype(np.float32), obb=o, **volume_kwargs))

    def __len__(self):
        return len(self.volumes)

    def __getitem__(self, k):
        return self.volumes[k]

    def integrate(self, depth, intrinsics, cam2world, chunk=None, color=None):
        """TSDFVolume.integrate on every level (the depth and colour stacks are moved to the device, and the colour
        stack packed, once)."""
        d = _to_device(depth, torch.float32, self.volumes[0].device)
        if color is not None:
            color = color_stack(color, self.volumes[0].device)
        for v in self.volumes:
            v.integrate(d, intrinsics, cam2world, chunk, color)
        return self

    def copy(self):
        """An independent snapshot of every level."""
        c = TSDFPyramid.__new__(TSDFPyramid)
        c.volumes = [v.copy() for v in self.volumes]
        return c


def write_scan(path_sdf, dims_zyx, voxel_size, world2grid, locs_xyz, vals, known=None):
    """Host arrays -> the .sdf (data.write_scene: (x, y, z) u32 + metric sdf) and, given known (dz, dy, dx) u8, the
    .knw next to it (data.write_known)."""
    import os
    xyz = np.asarray(locs_xyz).reshape(-1, 3)
    data.write_scene(path_sdf, dims_zyx, voxel_size, world2grid, (xyz[:, ::-1], np.asarray(vals, np.float32)))
    if known is not None:
        data.write_known(os.path.splitext(path_sdf)[0] + '.knw', dims_zyx, voxel_size, world2grid, known)
    return path_sdf


def scan_sample(volume, truncation=3.0, num_hierarchy_levels=4, max_input_height=0):
    """The target-less scene sample of a fused volume, on the device: what SceneDataset + collate and
    DeviceBatchLoader (scene mode) yield for the files volume.save() writes, with the volume as input and target.

    Returns {'name', 'input': [locs (n, 4) int64 z, y, x, 0; feats (n, 1) sdf / voxel_size], 'orig_dims' (1, 3),
    'padded_dims' (3,) (data._padded_dims), 'world2grid' (1, 4, 4), 'known' (1, 1, *padded_dims) uint8 padded with
    255}.  The file's |sdf| <= 6 voxel_size filter applies before |sdf / voxel_size| < truncation."""
    dx, dy, dz = volume.dims_xyz
    h = int(max_input_height)
    pd = tuple(int(v) for v in data._padded_dims((dz, dy, dx), num_hierarchy_levels, h))
    in_limit = h if (h > 0 and dz > h) else 1 << 40           # scene_dataloader.py:83-86
    tgt_limit = max(0, min(h, dz))
    sel, count, m = volume._compact(np.float32(6.0) * volume.voxel_size, np.float32(truncation), in_limit)
    dev = volume.device
    locs = torch.empty((max(m, 1), 4), dtype=torch.int64, device=dev)
    feats = torch.empty((max(m, 1), 1), dtype=torch.float32, device=dev)
    _lib.call('sgnn_fuse_emit_rows', volume._sdf.data_ptr(), dx, dy, float(volume.voxel_size), sel.data_ptr(),
              count.data_ptr(), m, locs.data_ptr(), feats.data_ptr())
    known = torch.full((1, 1) + pd, 255, dtype=torch.uint8, device=dev)
    known[0, 0, :tgt_limit, :dy, :dx] = volume.known()[:tgt_limit]
    return {'name': ['scan'], 'input': [locs[:m], feats[:m]],
            'orig_dims': torch.tensor([[dz, dy, dx]], dtype=torch.long), 'padded_dims': pd,
            'world2grid': torch.from_numpy(volume.world2grid[None].copy()).to(dev), 'known': known}
