"""Feature-transform cost at scene size: the 128 x 512 x 512 volume (z, y, x) of synth.make_scene, seeds = the voxels
with |sdf| < 1 voxel.

Timed: edt.feature_transform without a cap and with max_dist 8 and 32; edt.fill_colors of a random colour volume;
the worst case of the outward walk, a volume that is empty but for ONE seed, without a cap and with max_dist 32; the
three passes of the uncapped transform one by one; and, for scale, marching cubes of the same scene.  Every job is
warmed up, then all are timed in turn for --rounds rounds with device events around the whole call, so that drift of a
shared machine hits all of them alike; the median, the minimum and the maximum are reported.  If scipy imports, the
host leg (.cpu() + scipy.ndimage.distance_transform_edt(return_indices=True)) is timed once with a wall clock and its
squared distances are compared with the device's.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import _lib, edt, marching_cubes as mc, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--no-host', action='store_true', help='skip the scipy leg')
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
_lib.require_gpu()
dev = torch.device('cuda')

locs, feats = synth.make_scene((Z, Y, X))
dense = torch.full((Z, Y, X), -float('inf'), dtype=torch.float32, device=dev)
locs = locs.to(dev)
dense[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0]
seeds = (dense.abs() < 1.0).to(torch.uint8).contiguous()
one = torch.zeros_like(seeds)
one[Z // 2, Y // 2, X // 2] = 1
colors = torch.randint(0, 256, (Z, Y, X, 3), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()

dims = (Z, Y, X)
feat_a = torch.empty(dims, dtype=torch.int32, device=dev)
feat_b = torch.empty_like(feat_a)
dist2 = torch.empty_like(feat_a)


def pass_x():
    _lib.call('sgnn_edt_rows', _lib.ptr(seeds), Z, Y, X, -1, _lib.ptr(feat_a))


def pass_y():
    _lib.call('sgnn_edt_axis', _lib.ptr(feat_a), Z, Y, X, 1, -1, _lib.ptr(feat_b), None, None)


def pass_z():
    _lib.call('sgnn_edt_axis', _lib.ptr(feat_b), Z, Y, X, 0, -1, None, _lib.ptr(dist2), _lib.ptr(feat_a))


jobs = {
    'transform': lambda: edt.feature_transform(seeds),
    'transform_max8': lambda: edt.feature_transform(seeds, 8),
    'transform_max32': lambda: edt.feature_transform(seeds, 32),
    'fill_colors': lambda: edt.fill_colors(colors, seeds),
    'one_seed': lambda: edt.feature_transform(one),
    'one_seed_max32': lambda: edt.feature_transform(one, 32),
    'pass_x': pass_x, 'pass_y': pass_y, 'pass_z': pass_z,                  # in this order: each reads the one before
    'marching_cubes': lambda: mc.run_marching_cubes(dense, None, 0.0, 3.0, 10.0),
}
res = {'dims_zyx': [Z, Y, X], 'voxels': Z * Y * X, 'rounds': args.rounds, 'seeds': int(seeds.sum().item()),
       'seed_share': round(float(seeds.float().mean().item()), 5)}

for job in jobs.values():                                                   # warm-up
    job()
    job()
torch.cuda.synchronize()
ft = edt.feature_transform(seeds)
res['max_dist2'] = int(ft.dist2.max().item())
for r in (8, 32):
    capped = edt.feature_transform(seeds, r)
    near = ft.dist2 <= r * r
    res['max%d_equal_within_reach' % r] = bool(
        torch.equal(capped.dist2[near], ft.dist2[near]) and torch.equal(capped.nearest[near], ft.nearest[near]) and
        bool((capped.dist2[~near] == -1).all()))
    del capped, near

times = {n: [] for n in jobs}
for _ in range(args.rounds):
    for n, job in jobs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        job()
        e.record()
        torch.cuda.synchronize()
        times[n].append(s.elapsed_time(e))
for n in jobs:
    res[n] = {'ms': round(statistics.median(times[n]), 3), 'ms_min': round(min(times[n]), 3),
              'ms_max': round(max(times[n]), 3), 'ms_runs': [round(t, 3) for t in times[n]]}
res['one_seed_over_transform'] = round(res['one_seed']['ms'] / res['transform']['ms'], 2)

ndimage = None
if not args.no_host:
    try:
        from scipy import ndimage
    except ImportError:
        pass
if ndimage is None:
    res['host_scipy'] = None
else:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = seeds.cpu().numpy()
    d, idx = ndimage.distance_transform_edt(host == 0, return_indices=True)
    t = time.perf_counter() - t0
    res['host_scipy'] = {'ms': round(t * 1e3, 1), 'over_transform': round(t * 1e3 / res['transform']['ms'], 1),
                         'dist2_equal': bool(np.array_equal(np.rint(d * d).astype(np.int64), ft.dist2.cpu().numpy()))}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
