"""Depth frames rendered from a triangle mesh on the GPU: mesh + camera poses -> the frames sgnn_amd.fusion fuses.

The reference's scan generator has two sources of depth (datagen/GenerateScans Scene.cpp:160-165): sensor frames
(fusion.raw_depth_to_metric) and virtual scans, depth rendered from the scene's mesh along the camera trajectory
(Scene::renderDepthFrame, Scene.cpp:107-158).  Its renderer is a Direct3D rasteriser that is not part of this
project; the rules this one follows are listed in INTEGRATION.md section F, and that text is the contract of the
kernels (sgnn_amd/csrc/render.hip) and of the independent NumPy restatement of the tests (tests/render_ref.py).

    verts, faces = load_ply('room.ply')                     # or device tensors straight from marching cubes
    poses = look_at(eyes, targets)                          # (F, 4, 4) cam2world: x right, y down, z forward
    depth = render_depth(verts, faces, K, poses, (240, 320))          # (F, h, w) fp32 on the device, -inf = nothing
    vol = fusion.TSDFVolume(dims, 0.02, world2grid).integrate(depth, K, poses)

Rendered depth goes to integrate() unfiltered: the reference applies its bilateral filter to sensor frames only
(Fuser.cpp:31).  The host does per-frame geometry only (one 3x4 matrix per frame).
"""
import numpy as np
import torch

from . import _lib
from ._glue import camera_shapes, cameras, mesh_shape, mesh_upload, to_device as _to_device

# struct sgnn_render_frame (include/sgnn_hip.h)
FRAME_DTYPE = np.dtype([('m', '<f4', (12,)), ('intr', '<f4', (4,))])
assert FRAME_DTYPE.itemsize == 64

DEFAULT_CHUNK = 0           # frames per triangle launch, 0 = all in one
WAVE_PIXELS = 0             # pixel boxes above this are drawn by a whole wave; 0 = the library's constant
STATUS_INDEX_RANGE = 1      # SGNN_STATUS_COORD_RANGE


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam2world (F, 4, 4) fp64 of cameras at eye (F, 3) looking at target (F, 3): camera x right, y down, z
    forward.  A single eye / target gives one (4, 4) matrix.  A view direction parallel to `up` takes (0, 1, 0)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    single = eye.ndim == 1 and target.ndim == 1
    eye, target = np.broadcast_arrays(np.atleast_2d(eye), np.atleast_2d(target))
    up = np.asarray(up, np.float64)
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd, axis=1, keepdims=True)
    right = np.cross(fwd, up)
    flat = np.linalg.norm(right, axis=1) < 1e-9
    right[flat] = np.cross(fwd[flat], (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    down = np.cross(fwd, right)
    m = np.tile(np.eye(4), (len(eye), 1, 1))
    m[:, :3, 0], m[:, :3, 1], m[:, :3, 2], m[:, :3, 3] = right, down, fwd, eye
    return m[0] if single else m


_PLY_SIZES = {'char': 1, 'uchar': 1, 'int8': 1, 'uint8': 1, 'short': 2, 'ushort': 2, 'int16': 2, 'uint16': 2, 'int': 4,
              'uint': 4, 'int32': 4, 'uint32': 4, 'float': 4, 'float32': 4, 'double': 8, 'float64': 8}


def load_ply(path):
    """Host reader for the PLY files marching_cubes.save_to_ply writes: binary little-endian, float x y z vertices
    (further vertex properties are skipped by their declared sizes), `list uchar int vertex_indices` triangles.
    Returns (verts (V, 3) fp32, faces (T, 3) int32).  ValueError names the first header line it cannot handle."""
    v, _, faces = _read_ply(path)
    return np.stack([v['x'], v['y'], v['z']], 1).astype(np.float32).reshape(-1, 3), faces


def load_ply_colors(path):
    """load_ply with the vertex colours: (verts (V, 3) fp32, faces (T, 3) int32, vcolors (V, 3) uint8) from the uchar
    properties red, green, blue that save_to_ply writes: what render_color takes.  ValueError if the file has none."""
    v, vprops, faces = _read_ply(path)
    types = dict(vprops)
    for want in ('red', 'green', 'blue'):
        if types.get(want) not in ('uchar', 'uint8'):
            raise ValueError('%s: no uchar vertex property %r (the file has no colours)' % (path, want))
    verts = np.stack([v['x'], v['y'], v['z']], 1).astype(np.float32).reshape(-1, 3)
    return verts, faces, np.stack([v['red'], v['green'], v['blue']], 1).astype(np.uint8).reshape(-1, 3)


def _read_ply(path, need_faces=True):
    """(vertex records, [(property, type)], faces (T, 3) int32) of a PLY file as load_ply describes it.  need_faces
    False (points.load_ply_points): the face element may be missing, and faces is then (0, 3)."""
    with open(path, 'rb') as fh:
        blob = fh.read()
    end = blob.find(b'end_header\n')
    if not blob.startswith(b'ply') or end < 0:
        raise ValueError('%s: not a PLY file' % path)
    lines = blob[:end].decode('ascii', 'replace').split('\n')
    body = end + len(b'end_header\n')
    element, counts, vprops, face_ok = None, {}, [], False
    for line in lines[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            if tok[1:] != ['binary_little_endian', '1.0']:
                raise ValueError('%s: unsupported header line %r (binary_little_endian 1.0 only)' % (path, line))
        elif tok[0] == 'element' and len(tok) == 3 and tok[1] in ('vertex', 'face') and tok[1] not in counts:
            if tok[1] == 'vertex' and 'face' in counts:
                raise ValueError('%s: unsupported header line %r (vertices must come first)' % (path, line))
            element = tok[1]
            counts[element] = int(tok[2])
        elif tok[0] == 'property' and element == 'vertex' and len(tok) == 3 and tok[1] in _PLY_SIZES:
            vprops.append((tok[2], tok[1]))
        elif tok[0] == 'property' and element == 'face' and not face_ok and tok[1:] in (
                ['list', 'uchar', 'int', 'vertex_indices'], ['list', 'uint8', 'int32', 'vertex_indices'],
                ['list', 'uchar', 'int', 'vertex_index'], ['list', 'uint8', 'int32', 'vertex_index']):
            face_ok = True
        else:
            raise ValueError('%s: unsupported header line %r' % (path, line))
    names = [n for n, _ in vprops]
    for want in ('x', 'y', 'z'):
        if want not in names or dict(vprops)[want] not in ('float', 'float32'):
            raise ValueError('%s: vertex property %r must be a float' % (path, want))
    if not need_faces and 'vertex' in counts and 'face' not in counts:
        counts['face'] = 0
    elif 'vertex' not in counts or 'face' not in counts or not face_ok:
        raise ValueError('%s: needs a vertex element and a face element with vertex_indices' % path)
    vdt = np.dtype({'names': names, 'formats': ['<f4' if n in ('x', 'y', 'z') else 'u1' if _PLY_SIZES[t] == 1 else
                                                'V%d' % _PLY_SIZES[t] for n, t in vprops]})
    nv, nf = counts['vertex'], counts['face']
    fdt = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    if len(blob) < body + nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError('%s: truncated' % path)
    v = np.frombuffer(blob, vdt, nv, body)
    f = np.frombuffer(blob, fdt, nf, body + nv * vdt.itemsize)
    if nf and (f['n'] != 3).any():
        raise ValueError('%s: unsupported face %d: %d vertices (triangles only)' % (
            path, int(np.argmax(f['n'] != 3)), int(f['n'][np.argmax(f['n'] != 3)])))
    return v, vprops, np.ascontiguousarray(f['i']).astype(np.int32).reshape(-1, 3)


def frame_table(intrinsics, cam2world):
    """Host table of sgnn_render_frame records: rows 0..2 of inv(cam2world), formed in fp64 and rounded to fp32, and
    fx, fy, cx, cy.  A non-finite pose gets NaN rows (its frame stays empty)."""
    k, c2w = cameras(intrinsics, cam2world)
    t = np.zeros(k.shape[0], dtype=FRAME_DTYPE)
    ok = np.isfinite(c2w).all(axis=(1, 2))
    m = np.full((k.shape[0], 3, 4), np.nan, dtype=np.float32)
    if ok.any():
        try:
            m[ok] = np.linalg.inv(c2w[ok])[:, :3, :].astype(np.float32)
        except np.linalg.LinAlgError:
            raise ValueError('a cam2world matrix is singular')
    t['m'] = m.reshape(-1, 12)
    t['intr'] = k
    return t


def render_depth(verts, faces, intrinsics, cam2world, hw, z_clip=0.1, depth_min=0.4, depth_max=4.0, chunk=None,
                 counters=None):
    """z-depth of a triangle mesh seen from F cameras -> (F, h, w) fp32 on the device, -inf where nothing is seen or
    the nearest surface is outside [depth_min, depth_max].

    verts (V, 3) fp32 world metres, faces (T, 3) int32, intrinsics (F, 4) fx, fy, cx, cy, cam2world (F, 4, 4); numpy
    arrays or torch tensors, host or device.  Pixel (i, j) is sampled at u = i, v = j, the convention of
    TSDFVolume.integrate.  chunk: frames per launch (the result does not depend on it; None: DEFAULT_CHUNK).
    counters: None, or a device int64 tensor of 3 that receives triangles drawn per lane, triangles drawn per wave
    and covered pixels (measurements; slower)."""
    return _render(verts, faces, None, intrinsics, cam2world, hw, z_clip, depth_min, depth_max, chunk, counters)


def render_color(verts, faces, vcolors, intrinsics, cam2world, hw, z_clip=0.1, depth_min=0.4, depth_max=4.0,
                 chunk=None, counters=None):
    """render_depth of a mesh whose vertices carry a colour -> (depth (F, h, w) fp32, rgba (F, h, w, 4) uint8), both
    on the device: the pair TSDFVolume(color=True).integrate(depth, K, cam2world, color=rgba) takes.

    vcolors (V, 3) uint8 R, G, B, numpy or torch, host or device; every other argument, and every error, as
    render_depth.  depth is render_depth's, bit for bit.  The colour is interpolated perspective-correctly between
    the vertices; A = 255 where depth is finite, (0, 0, 0, 0) elsewhere."""
    if vcolors is None or len(tuple(vcolors.shape)) != 2 or tuple(vcolors.shape) != (int(verts.shape[0]), 3):
        raise ValueError('vcolors must be (V, 3) for verts %s, got %s' % (
            tuple(verts.shape), None if vcolors is None else tuple(vcolors.shape)))
    return _render(verts, faces, vcolors, intrinsics, cam2world, hw, z_clip, depth_min, depth_max, chunk, counters)


def _render(verts, faces, vcolors, intrinsics, cam2world, hw, z_clip, depth_min, depth_max, chunk, counters):
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1 or h > 16384 or w > 16384:
        raise ValueError('unsupported frame size %s' % ((h, w),))
    dev, (nv, nt) = mesh_shape(verts, faces, vcolors)
    camera_shapes(intrinsics, cam2world)
    if not float(z_clip) > 0.0:
        raise ValueError('z_clip must be positive')
    table = frame_table(intrinsics, cam2world)
    nf = int(table.shape[0])
    if nt * 3 >= 2 ** 31 or nf * h * w >= 2 ** 31:
        raise ValueError('3 T = %d or F h w = %d does not fit 31 bits' % (nt * 3, nf * h * w))
    v, f, on_device = mesh_upload(verts, faces, nv, dev)
    out = torch.empty((nf, h, w), dtype=torch.float32, device=dev)
    color = vcolors is not None
    rgba = torch.empty((nf, h, w, 4), dtype=torch.uint8, device=dev) if color else None
    if nf == 0:
        return (out, rgba) if color else out
    status = torch.zeros(1, dtype=torch.int32, device=dev) if on_device else None
    dev_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    args = (v.data_ptr(), nv, f.data_ptr(), nt, dev_table.data_ptr(), nf,
            int(DEFAULT_CHUNK if chunk is None else chunk), h, w, float(np.float32(z_clip)),
            float(np.float32(depth_min)), float(np.float32(depth_max)), int(WAVE_PIXELS), out.data_ptr(),
            _lib.ptr(status), _lib.ptr(counters))
    if color:
        c = _to_device(vcolors, torch.uint8, dev)
        keys = torch.empty((nf, h, w), dtype=torch.int64, device=dev)       # the depth buffer of the call
        _lib.call('sgnn_rendercol_draw', *args, c.data_ptr(), keys.data_ptr(), rgba.data_ptr())
    else:
        _lib.call('sgnn_render_depth', *args)
    if status is not None and int(status.item()) & STATUS_INDEX_RANGE:
        raise ValueError('face index out of range [0, %d)' % nv)
    return (out, rgba) if color else out
