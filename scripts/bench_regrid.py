"""Regrid cost at scene size: the 128 x 512 x 512 volume (z, y, x, 2 cm) of synth.make_scene resampled under a 30
degree yaw about the up axis into its regrid.grid_for box.  The source's state is filled from the scene directly
(sdf = the scene's values in metres, weight 1..255 and free counts from a generator, an 8.8 colour record on every
observed voxel); it is not fused from frames, which changes no byte count and no access pattern.

Timed, warm, median of --rounds with min - max, from device events: resample linear / nearest, with and without colour,
skip on and off, the three wave shapes (0 = 4 x 4 x 4, 1 = 8 x 8 x 1, 2 = 64 x 1 x 1), merge; against a device-to-device
copy of the same number of bytes (source state read once + destination state written once: the floor) and against
torch.nn.functional.grid_sample on sdf() alone, the stop-gap, which carries no weight, free counter or colour and turns
-inf into NaN.  No time is a pass / fail criterion.  Prints one JSON line; --out also writes it.
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
from sgnn_amd import fusion, regrid, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--yaw', type=float, default=30.0, help='degrees')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')


def scene_volume(color):
    locs, feats = synth.make_scene((Z, Y, X))
    w2g = np.eye(4, dtype=np.float32)
    w2g[:3, :3] /= np.float32(args.voxel)
    vol = fusion.TSDFVolume((X, Y, Z), args.voxel, w2g, color=color)
    locs = locs.to(dev)
    vol._sdf[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0] * args.voxel
    gen = torch.Generator(device=dev).manual_seed(0)
    seen = torch.isfinite(vol._sdf)
    vol._weight[...] = torch.randint(1, 256, (Z, Y, X), generator=gen, device=dev, dtype=torch.uint8) * seen
    vol._free[...] = torch.randint(0, 50, (Z, Y, X), generator=gen, device=dev, dtype=torch.int32)
    if color:
        rec = torch.randint(-32768, 32767, (Z, Y, X, 4), generator=gen, device=dev, dtype=torch.int16)
        rec[..., 3] = torch.randint(1, 256, (Z, Y, X), generator=gen, device=dev, dtype=torch.int16)
        vol._color[...] = rec * seen[..., None]
    return vol


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


vols = {True: scene_volume(True), False: None}
vols[False] = vols[True].copy()
vols[False]._color = None
c, s = np.cos(np.deg2rad(args.yaw)), np.sin(np.deg2rad(args.yaw))
T = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
dims_b, w2g_b = regrid.grid_for(vols[True], T)
n_src, n_dst = X * Y * Z, int(np.prod(dims_b))
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'yaw_deg': args.yaw, 'dst_dims_xyz': list(dims_b), 'rounds': args.rounds,
       'src_voxels': n_src, 'dst_voxels': n_dst, 'observed_share': round(float((vols[True]._weight > 0).float().mean()), 4)}

jobs = {}
for color in (True, False):
    tag = 'color' if color else 'plain'
    for mode in ('linear', 'nearest'):
        for skip in (True, False):
            jobs['resample_%s_%s_%s' % (mode, tag, 'skip' if skip else 'noskip')] = (
                lambda color=color, mode=mode, skip=skip: regrid.resample(vols[color], dims_b, w2g_b, mode=mode, skip=skip))
    for shape in (0, 1, 2):
        jobs['resample_linear_%s_shape%d' % (tag, shape)] = (
            lambda color=color, shape=shape: regrid.resample(vols[color], dims_b, w2g_b, _shape=shape))
        jobs['resample_nearest_%s_shape%d' % (tag, shape)] = (
            lambda color=color, shape=shape: regrid.resample(vols[color], dims_b, w2g_b, mode='nearest', _shape=shape))
merge_dst = regrid.resample(vols[True], dims_b, w2g_b)
for skip in (True, False):
    jobs['merge_linear_color_%s' % ('skip' if skip else 'noskip')] = (
        lambda skip=skip: regrid.merge(merge_dst, vols[True], skip=skip))
del_bytes = {True: 17, False: 9}                                 # sdf 4 + weight 1 + free 4 (+ colour 8) per voxel
for color in (True, False):
    nbytes = del_bytes[color] * (n_src + n_dst) // 2             # a copy reads and writes its size
    a, b = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    jobs['copy_floor_%s' % ('color' if color else 'plain')] = lambda a=a, b=b: b.copy_(a)
    res['bytes_%s' % ('color' if color else 'plain')] = 2 * nbytes

# the stop-gap: grid_sample on sdf() alone, positions from the same map, normalised to [-1, 1] with align_corners
A = torch.from_numpy(regrid.grid_map(vols[True].world2grid, w2g_b)).to(dev)
k, j, i = torch.meshgrid(torch.arange(dims_b[2], device=dev, dtype=torch.float32),
                         torch.arange(dims_b[1], device=dev, dtype=torch.float32),
                         torch.arange(dims_b[0], device=dev, dtype=torch.float32), indexing='ij')
grid = torch.stack([(A[r, 0] * i + A[r, 1] * j + A[r, 2] * k + A[r, 3]) * (2.0 / (d - 1)) - 1.0
                    for r, d in zip(range(3), (X, Y, Z))], -1)[None]
del i, j, k
sdf5 = vols[True]._sdf[None, None]
jobs['grid_sample_sdf_only'] = lambda: torch.nn.functional.grid_sample(sdf5, grid, mode='bilinear', padding_mode='zeros',
                                                                       align_corners=True)

for job in jobs.values():
    job()
torch.cuda.synchronize()
times = {n: [] for n in jobs}
for _ in range(args.rounds):
    for n, job in jobs.items():
        times[n].append(timed(job)[0])
for n, runs in times.items():
    res[n + '_ms'] = round(statistics.median(runs), 3)
    res[n + '_ms_min_max'] = [round(min(runs), 3), round(max(runs), 3)]
res['default_shape'] = regrid._DEFAULT_SHAPE
res['observed_after_linear'] = int((regrid.resample(vols[False], dims_b, w2g_b).weight() > 0).sum())
res['observed_after_nearest'] = int((regrid.resample(vols[False], dims_b, w2g_b, mode='nearest').weight() > 0).sum())

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
