"""Sensor simulation cost at scene size: 1000 frames of 240 x 320 cast from the 128 x 512 x 512 volume (z, y, x, 2 cm)
of synth.make_scene along the room trajectory of scripts/bench_render.py, the stack fusion's integrate takes.

Timed, warm, median of --rounds with min - max, from device events around the public calls (so the upload of the
intrinsics and the allocation of the result are inside): sensor.shadow_mask alone, sensor.degrade with the default
model (two launches), the same on the frames with every empty pixel filled at 2.5 m (the cast frames of this scene
are mostly empty, and an empty pixel leaves at the range gate), sensor.degrade with every stage off (one launch).
Comparison legs in the same run: (a) a device-to-device copy of the frames' bytes, the floor of a pass that reads and
writes each pixel once; (b) rules V.4, V.8 (without the incidence term) and V.9 by plain torch ops (randn, where,
round), the route a user has without this module.  Also the share of pixels the default model leaves.  No time is a
pass / fail criterion.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import fusion, raycast, render, sensor, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
H, W, F = 240, 320, args.frames
dev = torch.device('cuda')


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


locs, feats = synth.make_scene((Z, Y, X))
w2g = np.eye(4, dtype=np.float32)
w2g[:3, :3] /= np.float32(args.voxel)
vol = fusion.TSDFVolume((X, Y, Z), args.voxel, w2g)
locs = locs.to(dev)
vol._sdf[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0] * args.voxel
vol._weight.copy_(torch.isfinite(vol._sdf))
ext = np.array([X, Y, Z]) * args.voxel
K = np.tile(np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], np.float32), (F, 1))
c = ext / 2
a = 2 * np.pi * 2 * np.arange(F) / F                                          # two loops
r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
eyes = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), np.full(F, min(1.5, ext[2] * 0.6))], 1)
poses = render.look_at(eyes, eyes + np.stack([np.cos(a + 1.2), np.sin(a + 1.2), np.full(F, -0.35)], 1))
depth = raycast.cast_volume(vol, K, poses, (H, W), depth_max=8.0)
del vol
model, off = sensor.SensorModel(), sensor.SensorModel.off()
fx = torch.from_numpy(K[:, 0]).to(dev).reshape(-1, 1, 1)


def torch_ops():
    z = torch.where(torch.isfinite(depth) & (depth >= model.min_depth) & (depth <= model.max_depth), depth, -np.inf)
    dz = z - model.a2
    z1 = z + (model.a0 + model.a1 * dz * dz) * torch.randn_like(z)
    B = fx * abs(model.baseline)
    dq = torch.round(B / z1 / model.disparity_quantum) * model.disparity_quantum
    z2 = B / dq
    return torch.where((dq > 0) & torch.isfinite(z2), z2, -np.inf)


copy_dst = torch.empty_like(depth)
filled = torch.where(torch.isfinite(depth), depth, 2.5)
jobs = {
    'shadow_mask': lambda: sensor.shadow_mask(depth, K, model.baseline),
    'degrade_default': lambda: sensor.degrade(depth, K, model, seed=0),
    'degrade_default_filled': lambda: sensor.degrade(filled, K, model, seed=0),
    'degrade_all_off': lambda: sensor.degrade(depth, K, off, seed=0),
    'copy_frame_bytes': lambda: copy_dst.copy_(depth),
    'torch_ops_gate_noise_disparity': torch_ops,
}
for job in jobs.values():
    job()
torch.cuda.synchronize()
times = {n: [] for n in jobs}
for _ in range(args.rounds):
    for n, job in jobs.items():
        times[n].append(timed(job)[0])
res = {'frames': F, 'frame_hw': [H, W], 'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'rounds': args.rounds,
       'frame_bytes': int(depth.numel() * 4)}
for n, runs in times.items():
    res[n + '_ms'] = round(statistics.median(runs), 4)
    res[n + '_ms_min_max'] = [round(min(runs), 4), round(max(runs), 4)]
out = jobs['degrade_default']()
res['finite_share_clean'] = round(torch.isfinite(depth).float().mean().item(), 4)
res['finite_share_degraded'] = round(torch.isfinite(out).float().mean().item(), 4)
res['finite_share_degraded_filled'] = round(torch.isfinite(jobs['degrade_default_filled']()).float().mean().item(), 4)
res['shadow_share'] = round(jobs['shadow_mask']().float().mean().item(), 5)
res['all_off_equals_input'] = bool(torch.equal(jobs['degrade_all_off']().view(torch.int32), depth.view(torch.int32)))
res['gb_per_s_degrade_default'] = round((2 * depth.numel() * 4 + 2 * depth.numel()) / res['degrade_default_ms'] / 1e6, 1)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
