"""Depth frames tracked against a TSDF volume on the GPU: camera poses for sequences that arrive without any.

sgnn_amd.raycast is the "model to frame" half of a KinectFusion-style system; this module is the other half, frame to
model: projective point-to-plane ICP of a live depth frame against the depth and normal maps that
raycast.cast_volume(..., normals=True) returns, giving the cam2world that fusion.TSDFVolume.integrate takes.  The
reference project has no counterpart; the rules this follows are listed in INTEGRATION.md section I, and that text is
the contract of the kernels (sgnn_amd/csrc/track.hip) and of the independent NumPy restatement of the tests
(tests/track_ref.py).

    vol = fusion.TSDFVolume(dims, 0.02, world2grid)
    poses, results = track_sequence(vol, depth_frames, K, first_pose)      # tracks and fuses, frame by frame
    res = align(depth, K, model_pose, guess_pose, vol)                      # one frame: TrackResult
    res = align_color(depth, rgba, K, model_pose, guess_pose, color_vol)    # depth and colour: ColorTrackResult
    sys = normal_equations(depth, K, model_depth, model_normal, K_model, T)  # (B, 32) fp64 on the device

The device builds the Gauss-Newton systems, the depth pyramid and the live normals; the 6x6 solve and the pose update
run on the host in fp64 (one 256-byte read-back per iteration), in the same spirit as raycast.frame_table.
"""
import collections
import math

import numpy as np
import torch

from . import _gn, _lib, fusion, raycast
from ._glue import host as _host, positive as _positive, source_device as _source_device, to_device as _to_device
from ._gn import A_SLICE, E_INDEX, G_SLICE, N_INDEX, se3_exp, solve_step, unpack  # noqa: F401  (public here)

# struct sgnn_track_pair (include/sgnn_hip.h)
PAIR_DTYPE = np.dtype([('t', '<f4', (12,)), ('intr_live', '<f4', (4,)), ('intr_model', '<f4', (4,)),
                       ('pad', '<f4', (4,))])
assert PAIR_DTYPE.itemsize == 96

MAX_BLOCKS = 256            # SGNN_TRACK_MAX_BLOCKS
MAX_PAIRS = 65535

TrackResult = collections.namedtuple('TrackResult', 'pose ok pairs rmse iterations history')
TrackResult.__doc__ = """What align() found for one frame: pose (4, 4) fp64 cam2world (the guess when ok is false), ok,
pairs and rmse (metres) of the finest level's last iteration, iterations run, and history: the number of associated
pixels of every iteration in the order they ran (coarse to fine)."""

ColorTrackResult = collections.namedtuple('ColorTrackResult', TrackResult._fields + ('color_pairs', 'color_rmse'))
ColorTrackResult.__doc__ = """What align_color() found for one frame: TrackResult's fields (pairs and rmse are the
geometric system's), and color_pairs and color_rmse (grey levels) of the photometric system of the same iteration."""


def _frames(x, name, tail=()):
    """Shape of a (B, h, w) + tail stack, checked."""
    shape = tuple(int(v) for v in x.shape)
    if len(shape) != 3 + len(tail) or shape[3:] != tuple(tail):
        raise ValueError('%s must be (B, h, w%s), got %s' % (name, ''.join(', %d' % t for t in tail), shape))
    if shape[1] < 1 or shape[2] < 1:
        raise ValueError('unsupported frame size %s' % (shape[1:3],))
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('B h w = %d does not fit 31 bits' % (shape[0] * shape[1] * shape[2]))
    return shape


def _intrinsics(k, nb, name):
    """(nb, 4) fp32 host intrinsics from (4,) or (nb, 4)."""
    k = _host(k, np.float32)
    if k.shape == (4,):
        k = np.tile(k, (nb, 1))
    if k.ndim != 2 or k.shape[1] != 4:
        raise ValueError('%s must be (B, 4) or (4,), got %s' % (name, k.shape))
    if k.shape[0] != nb:
        raise ValueError('%d %s for %d frames' % (k.shape[0], name, nb))
    return np.ascontiguousarray(k)


def pair_table(intrinsics, model_intrinsics, T):
    """Host table of sgnn_track_pair records (rule 1): rows 0..2 of T rounded to fp32 and the two sets of fx, fy, cx,
    cy.  A T that is not finite (in fp64 or after rounding) gets NaN rows: its system stays empty."""
    t64 = _host(T, np.float64)
    if t64.ndim != 3 or t64.shape[1:] != (4, 4):
        raise ValueError('T must be (B, 4, 4), got %s' % (t64.shape,))
    nb = t64.shape[0]
    table = np.zeros(nb, dtype=PAIR_DTYPE)
    table['t'] = _gn.record_rows(t64[:, :3, :].reshape(nb, 12), np.isfinite(t64[:, 3]).all(axis=1))
    table['intr_live'] = _intrinsics(intrinsics, nb, 'intrinsics')
    table['intr_model'] = _intrinsics(model_intrinsics, nb, 'model intrinsics')
    return table


def normal_equations(depth, K, model_depth, model_normal, K_model, T, max_dist=0.1, max_angle_deg=20.0,
                     live_normal=None, residual=None, assoc=None):
    """One Gauss-Newton system of point-to-plane ICP per (live frame, model frame) pair -> (B, 32) fp64 on the device:
    the 21 sums of the upper triangle of J^T J (row-major), the 6 of J^T r, the sum of r^2, the number of associated
    pixels, three zeros (rules 2-6; unpack() gives A, g, E, N).

    depth (B, h, w) live z-depths, -inf = none; K (B, 4) or (4,) fx, fy, cx, cy; model_depth (B, hm, wm) and
    model_normal (B, hm, wm, 3) as raycast.cast(..., normals=True) returns them, K_model their intrinsics; T (B, 4, 4):
    live camera -> model camera, inv(model_pose) . live_pose.  max_dist: the distance gate in metres; live_normal
    (B, h, w, 3) switches the angle gate on (max_angle_deg between the rotated live normal and the model normal).
    residual: None or a device fp32 tensor (B, h, w) that receives r, NaN where a pixel has no association; assoc:
    None or a device int32 tensor (B, h, w) that receives v * wm + u, or -1.  numpy arrays or torch tensors, host or
    device."""
    dev = _source_device(depth)
    nb, h, w = _frames(depth, 'depth')
    mb, hm, wm = _frames(model_depth, 'model_depth')
    _frames(model_normal, 'model_normal', (3,))
    if mb != nb or tuple(int(v) for v in model_normal.shape[:3]) != (mb, hm, wm):
        raise ValueError('%d live frames, model depth %s, model normals %s' % (nb, tuple(model_depth.shape),
                                                                              tuple(model_normal.shape)))
    if live_normal is not None and _frames(live_normal, 'live_normal', (3,))[:3] != (nb, h, w):
        raise ValueError('live_normal %s for depth %s' % (tuple(live_normal.shape), (nb, h, w)))
    if nb > MAX_PAIRS:
        raise ValueError('more than %d pairs in one call' % MAX_PAIRS)
    _positive('max_dist', max_dist)
    _positive('max_angle_deg', max_angle_deg)
    max_dist2 = np.float32(max_dist) * np.float32(max_dist)             # one fp32 product (rule 4)
    if not (max_dist2 > 0 and np.isfinite(max_dist2)):
        raise ValueError('max_dist = %s is not a usable gate' % max_dist)
    cos_min = np.float32(math.cos(math.radians(float(max_angle_deg))))
    table = pair_table(K, K_model, T)
    if table.shape[0] != nb:
        raise ValueError('%d matrices for %d frames' % (table.shape[0], nb))
    _gn.check_per_item((nb, h, w), residual, assoc, 'assoc')
    d = _to_device(depth, torch.float32, dev)
    md = _to_device(model_depth, torch.float32, dev)
    mn = _to_device(model_normal, torch.float32, dev)
    ln = None if live_normal is None else _to_device(live_normal, torch.float32, dev)
    head = (d.data_ptr(), _lib.ptr(ln), h, w, md.data_ptr(), mn.data_ptr(), hm, wm)
    return _gn.launch('sgnn_track_system', head, table, (max_dist2, cos_min), h * w, MAX_BLOCKS, (residual, assoc), dev)


def intensity(rgba):
    """The intensity of R, G, B, A pixels (.., 4) uint8 -> (..) fp32 on the device: (77 R + 150 G + 29 B) / 256, exact,
    NaN where A == 0 (section T rule T1).  numpy array or torch tensor, host or device."""
    dev = _source_device(rgba)
    c = _to_device(rgba if torch.is_tensor(rgba) else _host(rgba, np.uint8), torch.uint8, dev)
    if c.dim() < 1 or int(c.shape[-1]) != 4:
        raise ValueError('rgba must be (.., 4) uint8, got %s' % (tuple(c.shape),))
    out = torch.empty(tuple(c.shape[:-1]), dtype=torch.float32, device=dev)
    if out.numel() >= 2 ** 31 - 256:
        raise ValueError('%d pixels do not fit 31 bits' % out.numel())
    if out.numel():
        _lib.call('sgnn_track_intensity', c.data_ptr(), out.numel(), out.data_ptr())
    return out


def halve_intensity(depth, intensity, delta=0.05):
    """The next pyramid level of (B, h, w) intensity frames -> (B, h // 2, w // 2) fp32 on the device: per 2x2 block the
    mean intensity of the pixels that halve(depth, ., delta) averages and whose intensity is not NaN, NaN if there are
    none (rule T2).  Colour is never averaged across a depth edge."""
    dev = _source_device(depth)
    nb, h, w = _frames(depth, 'depth')
    if _frames(intensity, 'intensity') != (nb, h, w):
        raise ValueError('intensity %s for depth %s' % (tuple(intensity.shape), (nb, h, w)))
    _positive('delta', delta)
    d = _to_device(depth, torch.float32, dev)
    c = _to_device(intensity, torch.float32, dev)
    out = torch.empty((nb, h // 2, w // 2), dtype=torch.float32, device=dev)
    if out.numel():
        _lib.call('sgnn_track_halve_intensity', d.data_ptr(), c.data_ptr(), nb, h, w, float(np.float32(delta)),
                  out.data_ptr())
    return out


def color_equations(depth, intensity, K, model_depth, model_normal, model_intensity, K_model, T, max_dist=0.1,
                    max_angle_deg=20.0, max_intensity=40.0, live_normal=None, residual=None, cell=None):
    """One photometric Gauss-Newton system per (live frame, model frame) pair -> (B, 32) fp64 on the device, in
    normal_equations' layout (section T rules T3-T5).  A live pixel takes part when it passes normal_equations' gates
    for the same T, max_dist, max_angle_deg and live_normal, has an intensity, and falls into a cell of four model
    pixels that all have an intensity and a depth within max_dist of the point's; its residual is the bilinear sample
    of the model intensity minus the live intensity, gated at max_intensity (grey levels).

    intensity (B, h, w) and model_intensity (B, hm, wm) fp32 as intensity() returns them, NaN = none; every other
    argument as normal_equations.  residual: None or a device fp32 tensor (B, h, w) that receives r, NaN where a pixel
    takes no part; cell: None or a device int32 tensor (B, h, w) that receives y0 * wm + x0, or -1."""
    dev = _source_device(depth)
    nb, h, w = _frames(depth, 'depth')
    mb, hm, wm = _frames(model_depth, 'model_depth')
    _frames(model_normal, 'model_normal', (3,))
    if mb != nb or tuple(int(v) for v in model_normal.shape[:3]) != (mb, hm, wm):
        raise ValueError('%d live frames, model depth %s, model normals %s' % (nb, tuple(model_depth.shape),
                                                                              tuple(model_normal.shape)))
    if live_normal is not None and _frames(live_normal, 'live_normal', (3,))[:3] != (nb, h, w):
        raise ValueError('live_normal %s for depth %s' % (tuple(live_normal.shape), (nb, h, w)))
    if _frames(intensity, 'intensity') != (nb, h, w):
        raise ValueError('intensity %s for depth %s' % (tuple(intensity.shape), (nb, h, w)))
    if _frames(model_intensity, 'model_intensity') != (mb, hm, wm):
        raise ValueError('model intensity %s for model depth %s' % (tuple(model_intensity.shape), (mb, hm, wm)))
    if nb > MAX_PAIRS:
        raise ValueError('more than %d pairs in one call' % MAX_PAIRS)
    _positive('max_dist', max_dist)
    _positive('max_angle_deg', max_angle_deg)
    _positive('max_intensity', max_intensity)
    max_dist2 = np.float32(max_dist) * np.float32(max_dist)             # one fp32 product (rule 4)
    if not (max_dist2 > 0 and np.isfinite(max_dist2)):
        raise ValueError('max_dist = %s is not a usable gate' % max_dist)
    cos_min = np.float32(math.cos(math.radians(float(max_angle_deg))))
    table = pair_table(K, K_model, T)
    if table.shape[0] != nb:
        raise ValueError('%d matrices for %d frames' % (table.shape[0], nb))
    _gn.check_per_item((nb, h, w), residual, cell, 'cell')
    d, md, mn = (_to_device(x, torch.float32, dev) for x in (depth, model_depth, model_normal))
    li, mi = _to_device(intensity, torch.float32, dev), _to_device(model_intensity, torch.float32, dev)
    ln = None if live_normal is None else _to_device(live_normal, torch.float32, dev)
    head = (d.data_ptr(), _lib.ptr(ln), li.data_ptr(), h, w, md.data_ptr(), mn.data_ptr(), mi.data_ptr(), hm, wm)
    gates = (max_dist2, cos_min, np.float32(max_dist), np.float32(max_intensity))
    return _gn.launch('sgnn_track_color_system', head, table, gates, h * w, MAX_BLOCKS, (residual, cell), dev)


def level_intrinsics(K):
    """Intrinsics of the next pyramid level (rule 9): fx/2, fy/2, (cx - 0.5)/2, (cy - 0.5)/2, formed in fp64 and rounded
    to fp32; (.., 4) -> (.., 4) fp32 numpy."""
    k = _host(K, np.float32).astype(np.float64)
    return np.stack([k[..., 0] / 2, k[..., 1] / 2, (k[..., 2] - 0.5) / 2, (k[..., 3] - 0.5) / 2], -1).astype(np.float32)


def halve(depth, K, delta=0.05):
    """The next pyramid level of (B, h, w) depth frames -> ((B, h // 2, w // 2) fp32 on the device, its intrinsics as
    fp32 numpy).  A 2x2 block gives the mean of its finite values within delta of the smallest finite one, -inf if it
    has none (rule 9): a depth edge is not blurred into a surface that is not there."""
    dev = _source_device(depth)
    nb, h, w = _frames(depth, 'depth')
    _positive('delta', delta)
    k = _host(K, np.float32)
    if k.shape != (4,):
        k = _intrinsics(k, nb, 'intrinsics')
    d = _to_device(depth, torch.float32, dev)
    out = torch.empty((nb, h // 2, w // 2), dtype=torch.float32, device=dev)
    if out.numel():
        _lib.call('sgnn_track_halve', d.data_ptr(), nb, h, w, float(np.float32(delta)), out.data_ptr())
    return out, level_intrinsics(k)


def depth_normals(depth, K, delta=0.05):
    """Camera-space unit normals of (B, h, w) depth frames -> (B, h, w, 3) fp32 on the device, facing the camera (the
    sign raycast gives), NaN where a pixel or one of its four axis neighbours is missing or more than delta away in
    depth (rule 10)."""
    dev = _source_device(depth)
    nb, h, w = _frames(depth, 'depth')
    _positive('delta', delta)
    k = _intrinsics(K, nb, 'intrinsics')
    d = _to_device(depth, torch.float32, dev)
    out = torch.empty((nb, h, w, 3), dtype=torch.float32, device=dev)
    if nb:
        _lib.call('sgnn_track_normals', d.data_ptr(), torch.from_numpy(k).to(dev).data_ptr(), nb, h, w,
                  float(np.float32(delta)), out.data_ptr())
    return out


def align(depth, K, model_pose, guess_pose, volume, iterations=(10, 5, 4), max_dist=0.1, max_angle_deg=20.0,
          min_pairs=64, delta=0.05, angle_gate=True, timers=None, **cast_kwargs):
    """The pose of one depth frame against a fusion.TSDFVolume -> TrackResult.

    depth (h, w) metres, -inf = none; K (4,) fx, fy, cx, cy; model_pose: the cam2world the volume is cast at (the
    previous frame's pose); guess_pose: where the iteration starts.  iterations: Gauss-Newton steps per pyramid level,
    finest first; the live frame is halved len(iterations) - 1 times, the volume is cast once per level at that
    level's size and intrinsics (raycast.cast_volume(..., normals=True, **cast_kwargs)), and the levels run coarse to
    fine with no early exit.  delta is the depth step of halve() and depth_normals() at the finest level; level l uses
    delta * 2**l, since neighbouring pixels of one surface are twice as far apart.  angle_gate: compare
    depth_normals() of the live level with the model normal.  ok is false when an iteration has fewer than min_pairs
    associations or a system that is not positive definite; the pose returned is then the guess.  timers: None or a dict whose 'cast', 'system' and 'solve' entries get seconds added
    (measurements; switches on a device synchronisation per stage)."""
    dev = volume.device
    if len(tuple(depth.shape)) != 2:
        raise ValueError('depth must be (h, w), got %s' % (tuple(depth.shape),))
    levels = len(iterations)
    if levels < 1 or any(int(n) < 0 for n in iterations):
        raise ValueError('iterations = %s' % (iterations,))
    if int(depth.shape[0]) >> (levels - 1) < 1 or int(depth.shape[1]) >> (levels - 1) < 1:
        raise ValueError('a %s frame has no %d levels' % (tuple(depth.shape), levels))
    for name, v in (('max_dist', max_dist), ('max_angle_deg', max_angle_deg), ('delta', delta)):
        _positive(name, v)
    model_pose = _host(model_pose, np.float64).reshape(4, 4)
    guess_pose = _host(guess_pose, np.float64).reshape(4, 4)
    tick = _gn.Timer(timers)
    d = [_to_device(depth, torch.float32, dev)[None]]
    k = [_host(K, np.float32).reshape(4)]
    deltas = [np.float32(delta) * np.float32(2 ** lv) for lv in range(levels)]     # the pixel pitch doubles per level
    for lv in range(levels - 1):
        half, kh = halve(d[-1], k[-1], deltas[lv])
        d.append(half)
        k.append(kh)
    live_n = [depth_normals(dl, kl[None], dv) if angle_gate else None for dl, kl, dv in zip(d, k, deltas)]
    tick('system')
    model = [raycast.cast_volume(volume, kl[None], model_pose[None], tuple(dl.shape[1:]), normals=True, **cast_kwargs)
             for dl, kl in zip(d, k)]
    tick('cast')
    with np.errstate(all='ignore'):
        T = np.linalg.inv(model_pose) @ guess_pose if np.isfinite(model_pose).all() else np.full((4, 4), np.nan)
    run = _gn.Steps(T[None], min_pairs)
    history = run.history[0]
    for lv in range(levels - 1, -1, -1):
        for _ in range(int(iterations[lv])):
            systems = normal_equations(d[lv], k[lv], model[lv][0], model[lv][1], k[lv], run.T, max_dist,
                                       max_angle_deg, live_n[lv]).cpu().numpy()         # 256 bytes
            tick('system')
            run.step(systems)
            tick('solve')
            if not run.alive[0]:
                return TrackResult(guess_pose.copy(), False, run.pairs[0], float('nan'), len(history), tuple(history))
    return TrackResult(model_pose @ run.T[0], True, run.pairs[0], run.rmse[0], len(history), tuple(history))


def align_color(depth, rgba, K, model_pose, guess_pose, volume, color_weight=1e-3, max_intensity=40.0,
                iterations=(10, 5, 4), max_dist=0.1, max_angle_deg=20.0, min_pairs=64, delta=0.05, angle_gate=True,
                timers=None, **cast_kwargs):
    """The pose of one depth and colour frame against a fusion.TSDFVolume(color=True) -> ColorTrackResult: align()'s
    point-to-plane term plus a photometric term in one 6x6 step (section T), for views whose geometry leaves the pose
    open: a wall, a floor, a table top.

    rgba (h, w, 4) uint8, A == 0 = no colour (a fusion.pack_color frame), or (h, w, 3); every other argument as
    align().  The volume is cast once per level with raycast.cast_volume_color(..., normals=True); the live
    intensity() is halved next to the depth with halve_intensity().  Each iteration launches normal_equations and
    color_equations on the same T and solves S_g + color_weight^2 . S_c (rule T6): color_weight is metres per grey
    level, 1e-3 = one grey level counts like 1 mm; max_intensity gates |r| in grey levels.  Both are choices, not
    measurements; brightness constancy is assumed.  ok, pairs and rmse are taken from the geometric system as in
    align(); color_pairs and color_rmse from the photometric one.  ValueError for a volume without colour."""
    dev = volume.device
    if volume.color_state() is None:
        raise ValueError('the volume has no colour: TSDFVolume(..., color=True)')
    if len(tuple(depth.shape)) != 2:
        raise ValueError('depth must be (h, w), got %s' % (tuple(depth.shape),))
    if tuple(int(v) for v in rgba.shape[:2]) != tuple(int(v) for v in depth.shape) or len(tuple(rgba.shape)) != 3 or \
            int(rgba.shape[2]) not in (3, 4):
        raise ValueError('rgba must be (h, w, 3 | 4) for depth %s, got %s' % (tuple(depth.shape), tuple(rgba.shape)))
    levels = len(iterations)
    if levels < 1 or any(int(n) < 0 for n in iterations):
        raise ValueError('iterations = %s' % (iterations,))
    if int(depth.shape[0]) >> (levels - 1) < 1 or int(depth.shape[1]) >> (levels - 1) < 1:
        raise ValueError('a %s frame has no %d levels' % (tuple(depth.shape), levels))
    for name, v in (('max_dist', max_dist), ('max_angle_deg', max_angle_deg), ('delta', delta),
                    ('color_weight', color_weight), ('max_intensity', max_intensity)):
        _positive(name, v)
    weight2 = float(color_weight) * float(color_weight)                 # lambda^2, formed once in fp64 (rule T6)
    model_pose = _host(model_pose, np.float64).reshape(4, 4)
    guess_pose = _host(guess_pose, np.float64).reshape(4, 4)
    tick = _gn.Timer(timers)
    d = [_to_device(depth, torch.float32, dev)[None]]
    c = [intensity(fusion.color_stack(rgba, dev))]
    k = [_host(K, np.float32).reshape(4)]
    deltas = [np.float32(delta) * np.float32(2 ** lv) for lv in range(levels)]     # the pixel pitch doubles per level
    for lv in range(levels - 1):
        c.append(halve_intensity(d[-1], c[-1], deltas[lv]))
        half, kh = halve(d[-1], k[-1], deltas[lv])
        d.append(half)
        k.append(kh)
    live_n = [depth_normals(dl, kl[None], dv) if angle_gate else None for dl, kl, dv in zip(d, k, deltas)]
    tick('system')
    model = []
    for dl, kl in zip(d, k):
        md, mn, mc = raycast.cast_volume_color(volume, kl[None], model_pose[None], tuple(dl.shape[1:]), normals=True,
                                               **cast_kwargs)
        model.append((md, mn, intensity(mc)))
    tick('cast')
    with np.errstate(all='ignore'):
        T = np.linalg.inv(model_pose) @ guess_pose if np.isfinite(model_pose).all() else np.full((4, 4), np.nan)
    run = _gn.Steps(T[None], min_pairs)
    history = run.history[0]
    color_pairs, color_rmse = 0, float('nan')
    for lv in range(levels - 1, -1, -1):
        md, mn, mc = model[lv]
        for _ in range(int(iterations[lv])):
            geo = normal_equations(d[lv], k[lv], md, mn, k[lv], run.T, max_dist, max_angle_deg, live_n[lv])
            col = color_equations(d[lv], c[lv], k[lv], md, mn, mc, k[lv], run.T, max_dist, max_angle_deg,
                                  max_intensity, live_n[lv])
            geo, col = torch.stack([geo, col]).cpu().numpy()                            # one read-back: 512 bytes
            tick('system')
            both = geo.copy()
            both[:, :28] = geo[:, :28] + weight2 * col[:, :28]                          # rule T6; entry 28 stays N_g
            run.step(both, geo)
            color_pairs = int(col[0, N_INDEX])
            color_rmse = math.sqrt(col[0, E_INDEX] / color_pairs) if color_pairs else float('nan')
            tick('solve')
            if not run.alive[0]:
                return ColorTrackResult(guess_pose.copy(), False, run.pairs[0], float('nan'), len(history),
                                        tuple(history), color_pairs, float('nan'))
    return ColorTrackResult(model_pose @ run.T[0], True, run.pairs[0], run.rmse[0], len(history), tuple(history),
                            color_pairs, color_rmse)


def track_sequence(volume, depth_frames, K, first_pose, integrate=True, timers=None, color_frames=None, **align_kwargs):
    """Track a depth-only sequence against the volume it builds -> (poses (F, 4, 4) fp64 numpy, [TrackResult] * F).

    With integrate, frame 0 is fused at first_pose; each later frame is aligned against a cast at the last tracked
    frame's pose, with that pose as the guess, and fused when its result is ok.  A lost frame is skipped: it is
    reported (ok false, pose = the guess) and not fused, and the next frame starts from the same pose again.
    integrate=False tracks against the volume as it is and leaves it unchanged.  K (4,) or (F, 4); depth_frames
    (F, h, w), host or device.  color_frames: None, or the frames' colours as TSDFVolume.integrate(color=) takes them
    (F, h, w, 3 | 4) uint8 for a volume built with color=True: frames are then aligned with align_color() and fused
    with their colour, and the results are ColorTrackResults."""
    nf, h, w = _frames(depth_frames, 'depth_frames')
    k = _intrinsics(K, nf, 'intrinsics')
    d = _to_device(depth_frames, torch.float32, volume.device)
    rgba = None
    if color_frames is not None:
        if volume.color_state() is None:
            raise ValueError('colour frames for a volume built without color=True')
        if tuple(int(v) for v in color_frames.shape[:3]) != (nf, h, w):
            raise ValueError('colour frames %s for depth frames %s' % (tuple(color_frames.shape[:3]), (nf, h, w)))
        rgba = fusion.color_stack(color_frames, volume.device)
    pose = _host(first_pose, np.float64).reshape(4, 4).copy()
    poses = np.tile(pose, (nf, 1, 1))
    results = []
    tick = _gn.Timer(timers)
    for f in range(nf):
        if f == 0:
            res = TrackResult(pose.copy(), True, 0, 0.0, 0, ())
            if rgba is not None:
                res = ColorTrackResult(*res, 0, 0.0)
        elif rgba is not None:
            res = align_color(d[f], rgba[f], k[f], pose, pose, volume, timers=timers, **align_kwargs)
            tick = _gn.Timer(timers)
        else:
            res = align(d[f], k[f], pose, pose, volume, timers=timers, **align_kwargs)
            tick = _gn.Timer(timers)
        results.append(res)
        poses[f] = res.pose
        if res.ok:
            pose = res.pose
            if integrate:
                volume.integrate(d[f:f + 1], k[f:f + 1], pose[None], color=None if rgba is None else rgba[f:f + 1])
                tick('integrate')
    return poses, results
