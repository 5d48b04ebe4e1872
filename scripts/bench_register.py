"""Registration cost at scene size: the 128 x 512 x 512 volume (z, y, x, 2 cm) of synth.make_scene and its own
register.surface_points at strides 1 and 4 as the source, a few millimetres and a fraction of a degree off.

Timed, warm, median of --rounds with min - max, from device events: one register.normal_equations launch at B = 1 and
B = 8 (table upload, system kernel, finish kernel), and a 30-iteration register.align split into launches with their
read-back and the host solve (wall clock).  Comparison legs in the same run: (a) torch.nn.functional.grid_sample plus
autograd for the same values and gradients (no gates, no sums; -inf voxels set to 0, which it would turn into NaN);
(b) sgnn_track_system on a frame with as many pixels as there are points, every pixel associated: the same 28-sum
reduction behind coalesced loads; (c) a device-to-device copy of the bytes the gather touches, 12 per point and 32 of
corners.  No time is a pass / fail criterion.  Prints one JSON line; --out also writes it.
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
from sgnn_amd import fusion, register, synth, track  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
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
band = np.float32(3.0) * vol.voxel_size
off = track.se3_exp([0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
guesses = np.stack([track.se3_exp(np.array([0.002, -0.001, 0.0015, 0.004, -0.003, 0.002]) * (0.5 + 0.1 * b))
                    for b in range(8)])
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'rounds': args.rounds,
       'observed_share': round(float(torch.isfinite(vol._sdf).float().mean()), 4)}
clean = torch.where(torch.isfinite(vol._sdf), vol._sdf, torch.zeros_like(vol._sdf))[None, None]
scale = torch.tensor([2.0 / (X - 1), 2.0 / (Y - 1), 2.0 / (Z - 1)], device=dev)

jobs, aligns = {}, {}
for stride in (1, 4):
    pts = register.surface_points(vol, stride=stride)
    npts = int(pts.shape[0])
    res['points_stride%d' % stride] = npts
    res['associated_stride%d' % stride] = int(register.normal_equations(pts, vol.sdf(), w2g, off, band)[0, 28])
    tag = 'stride%d' % stride
    jobs['system_B1_' + tag] = lambda pts=pts: register.normal_equations(pts, vol.sdf(), w2g, off, band)
    jobs['system_B8_' + tag] = lambda pts=pts: register.normal_equations(pts, vol.sdf(), w2g, guesses, band)
    aligns[tag] = pts

    def sampled(pts=pts):
        g = (pts / args.voxel).requires_grad_(True)
        v = torch.nn.functional.grid_sample(clean, (g * scale - 1.0)[None, None, None], mode='bilinear',
                                            padding_mode='zeros', align_corners=True)
        v.sum().backward()
        return g.grad
    jobs['grid_sample_autograd_' + tag] = sampled

    h = 512
    w = (npts + h - 1) // h
    depth = torch.full((1, h, w), 2.0, device=dev)
    normal = torch.zeros((1, h, w, 3), device=dev)
    normal[..., 2] = -1.0
    K = np.array([w * 0.8, w * 0.8, (w - 1) / 2.0, (h - 1) / 2.0], np.float32)
    res['track_pixels_' + tag] = h * w
    jobs['track_system_equal_lanes_' + tag] = (
        lambda depth=depth, normal=normal, K=K: track.normal_equations(depth, K, depth, normal, K, np.eye(4)[None]))
    a = torch.empty(npts * 44 // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    res['gather_bytes_' + tag] = npts * 44
    jobs['copy_gather_bytes_' + tag] = lambda a=a, b=b: b.copy_(a)

for job in jobs.values():
    job()
torch.cuda.synchronize()
times = {n: [] for n in jobs}
for _ in range(args.rounds):
    for n, job in jobs.items():
        times[n].append(timed(job)[0])
for n, runs in times.items():
    res[n + '_ms'] = round(statistics.median(runs), 4)
    res[n + '_ms_min_max'] = [round(min(runs), 4), round(max(runs), 4)]

for tag, pts in aligns.items():
    register.align(pts, vol, off)
    split = {'system': [], 'solve': []}
    for _ in range(args.rounds):
        timers = {}
        out = register.align(pts, vol, off, timers=timers)
        for k in split:
            split[k].append(1e3 * timers.get(k, 0.0))
    res['align30_%s_ok' % tag] = bool(out.ok)
    for k, runs in split.items():
        res['align30_%s_%s_ms' % (tag, k)] = round(statistics.median(runs), 3)
        res['align30_%s_%s_ms_min_max' % (tag, k)] = [round(min(runs), 3), round(max(runs), 3)]

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
