"""Point-cloud fusion cost at scene size: the marching-cubes surface of synth.make_scene (128 x 512 x 512 voxels, z, y,
x, at 2 cm) rendered to --poses frames of 240 x 320 from a ring of cameras (the frames of scripts/bench_voxelize.py) and
back-projected by points.from_depth to about 7.7 M rays.

Timed, warm, median of --rounds with min - max, from device events: points.integrate with carving on and off, and its
three stages apart (count + scan, walk, fold); the depth-frame TSDFVolume.integrate of the same frames as the
comparison leg; tests/points_ref.py on a --host-share subsample of the rays as the host NumPy leg (wall clock, once).
No time is a pass / fail criterion.  Prints one JSON line; --out also writes it.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import points_ref as PR  # noqa: E402
from sgnn_amd import fusion, marching_cubes as mc, points, render, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--poses', type=int, default=100)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--host-share', type=float, default=0.01, help='share of the rays the host NumPy leg fuses')
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')

locs, feats = synth.make_scene((Z, Y, X))
dense = torch.full((Z, Y, X), -float('inf'), dtype=torch.float32, device=dev)
locs = locs.to(dev)
dense[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0]
verts, _, faces = mc.run_marching_cubes(dense, None, 0.0, 3.0, 10.0)         # x, y, z in voxels
del dense
dims = (X, Y, Z)
world = verts * args.voxel
w2g = np.eye(4, dtype=np.float32)
w2g[:3, :3] /= np.float32(args.voxel)
ang = np.linspace(0.0, 2.0 * np.pi, args.poses, endpoint=False)
centre = np.array([X / 2, Y / 2, Z / 2]) * args.voxel
eye = centre + np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.0 * ang], 1)
poses = render.look_at(eye, eye + np.stack([np.cos(ang), np.sin(ang), -0.2 + 0.0 * ang], 1))
K = np.tile(np.array([[290.0, 290.0, 159.5, 119.5]], np.float32), (args.poses, 1))
far = float(np.hypot(X, Y) * args.voxel)
depth = render.render_depth(world, faces, K, poses, (240, 320), depth_max=far)
pts, org, oid = points.from_depth(depth, K, poses)


def volume():
    return fusion.TSDFVolume(dims, args.voxel, w2g, depth_max=far)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def stages(carve):
    """One integrate call stage by stage: ms of (count + scan, walk, fold) and the number of samples walked."""
    vol = volume()
    g2w = np.ascontiguousarray(np.linalg.inv(vol.world2grid.astype(np.float64)).astype(np.float32))
    n = int(pts.shape[0])
    t_count, (offsets, dev_box) = timed(lambda: points.count_scan(vol, pts, org, oid, carve, 0, n))
    box = np.ascontiguousarray(dev_box.cpu().numpy()[:6])
    acc = points.accumulators(vol, box, False)
    torch.cuda.synchronize()
    t_walk, _ = timed(lambda: points.walk(vol, pts, org, oid, None, carve, 0, n, offsets, box, g2w, acc))
    t_fold, _ = timed(lambda: points.fold(vol, box, acc))
    return (t_count, t_walk, t_fold), int(offsets[-1].item()), box


res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'poses': args.poses, 'rounds': args.rounds, 'frame_hw': [240, 320],
       'rays': int(pts.shape[0]), 'rays_with_depth': int(torch.isfinite(depth).sum()), 'depth_max_m': round(far, 3)}
jobs = {
    'points_carve': lambda: points.integrate(volume(), pts, org, oid, carve=True),
    'points_band': lambda: points.integrate(volume(), pts, org, oid, carve=False),
    'frames': lambda: volume().integrate(depth, K, poses),
}
for job in jobs.values():                                                   # warm-up of every shape that is timed
    job()
for carve in (True, False):
    stages(carve)
torch.cuda.synchronize()
times = {n: [] for n in jobs}
split = {True: [], False: []}
for _ in range(args.rounds):
    for n, job in jobs.items():
        times[n].append(timed(job)[0])
    for carve in (True, False):
        t, samples, box = stages(carve)
        split[carve].append(t)
        res['samples_%s' % ('carve' if carve else 'band')] = samples
        res['box_voxels_%s' % ('carve' if carve else 'band')] = int(np.prod(box[1::2] - box[0::2] + 1))
for n, runs in times.items():
    res[n + '_ms'] = round(statistics.median(runs), 3)
    res[n + '_ms_min_max'] = [round(min(runs), 3), round(max(runs), 3)]
for carve, runs in split.items():
    for k, stage in enumerate(('count_scan', 'walk', 'fold')):
        col = [r[k] for r in runs]
        key = '%s_%s_ms' % (stage, 'carve' if carve else 'band')
        res[key] = round(statistics.median(col), 3)
        res[key + '_min_max'] = [round(min(col), 3), round(max(col), 3)]
res['gsamples_per_s_carve'] = round(res['samples_carve'] / res['walk_carve_ms'] / 1e6, 3)
res['gsamples_per_s_band'] = round(res['samples_band'] / res['walk_band_ms'] / 1e6, 3)
res['points_carve_over_frames'] = round(res['points_carve_ms'] / res['frames_ms'], 3)

# the host NumPy leg: the restatement of the tests on a subsample of the rays (every 1 / share-th ray)
step = max(1, int(round(1.0 / args.host_share)))
hp, ho, hi = pts[::step].cpu().numpy(), org.cpu().numpy(), oid[::step].cpu().numpy()
t0 = time.perf_counter()
PR.integrate(PR.Volume(dims, args.voxel, w2g, dmax=far), hp, ho, hi, carve=True)
res['host_numpy_carve_s'] = round(time.perf_counter() - t0, 2)
res['host_numpy_rays'] = int(hp.shape[0])
res['host_numpy_s_per_mray'] = round(res['host_numpy_carve_s'] / hp.shape[0] * 1e6, 1)
res['device_carve_s_per_mray'] = round(res['points_carve_ms'] / 1e3 / pts.shape[0] * 1e6, 4)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
