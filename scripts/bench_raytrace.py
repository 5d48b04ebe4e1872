"""Ray tracing cost at scene size (sgnn_amd.raytrace), next to the rasteriser and to a copy of the ray bytes.

The mesh is the marching-cubes surface of synth.make_scene (128 x 512 x 512 voxels, z, y, x) in metres, the mesh that
scripts/bench_voxelize.py uses.  Legs: `closest` for --poses pinhole frames of 240 x 320 through camera_dirs from a ring
of cameras (sort=False and sort=True), render.render_depth of the same frames, a device copy of the rays' 24 bytes each;
one 64 x 2048 LiDAR sweep from the middle of the volume; `occluded` for 1 M pairs of surface samples and camera eyes.
The counters give cells visited and (ray, face) pairs tested per ray.

Timed warm, with device events around the whole call and the median of --rounds rounds taken in turn.  Prints one JSON
line; --out also writes it.
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
from sgnn_amd import marching_cubes as mc, meshdist, raytrace, render, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--poses', type=int, default=100)
ap.add_argument('--pairs', type=int, default=1 << 20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')
H, W = 240, 320

locs, feats = synth.make_scene((Z, Y, X))
dense = torch.full((Z, Y, X), -float('inf'), dtype=torch.float32, device=dev)
locs = locs.to(dev)
dense[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0]
verts, _, faces = mc.run_marching_cubes(dense, None, 0.0, 3.0, 10.0)         # x, y, z in voxels
del dense
world = (verts * args.voxel).contiguous()

ang = np.linspace(0.0, 2.0 * np.pi, args.poses, endpoint=False)
centre = np.array([X / 2, Y / 2, Z / 2]) * args.voxel
eye = centre + np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.0 * ang], 1)
poses = render.look_at(eye, eye + np.stack([np.cos(ang), np.sin(ang), -0.2 + 0.0 * ang], 1))
K = np.tile(np.array([[290.0, 290.0, 159.5, 119.5]], np.float32), (args.poses, 1))
far = float(np.hypot(X, Y) * args.voxel)

scene = raytrace.Scene(world, faces)
cam = raytrace.camera_dirs(K[0], (H, W)).to(dev)
rot = torch.from_numpy(poses[:, :3, :3].astype(np.float32)).to(dev)
dirs = ((rot[:, None, :, 0] * cam[None, :, 0, None] + rot[:, None, :, 1] * cam[None, :, 1, None])
        + rot[:, None, :, 2] * cam[None, :, 2, None]).reshape(-1, 3).contiguous()
orig = torch.from_numpy(poses[:, :3, 3].astype(np.float32)).to(dev)[:, None].expand(-1, H * W, 3).reshape(-1, 3).contiguous()
lidar = raytrace.lidar_dirs(64, 2048)
lidar_pose = np.eye(4)
lidar_pose[:3, 3] = centre
samples = meshdist.sample_surface(world, faces, args.pairs, seed=1)[0]
eyes = torch.from_numpy(eye.astype(np.float32)).to(dev)[torch.arange(args.pairs, device=dev) % args.poses]
sink = torch.empty_like(dirs), torch.empty_like(orig)


def copy_rays():
    sink[0].copy_(dirs)
    sink[1].copy_(orig)


jobs = {
    'closest_frames': lambda: scene.closest(orig, dirs, t_min=0.1, t_max=far),
    'closest_frames_sorted': lambda: scene.closest(orig, dirs, t_min=0.1, t_max=far, sort=True),
    'render_depth': lambda: render.render_depth(world, faces, K, poses, (H, W), depth_min=0.1, depth_max=far),
    'copy_ray_bytes': copy_rays,
    'lidar_sweep': lambda: raytrace.sweep(scene, lidar_pose[None], lidar, t_min=0.1, t_max=far),
    'occluded_pairs': lambda: scene.occluded(samples, eyes),
    'scene_build': lambda: raytrace.Scene(world, faces),
}
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'poses': args.poses, 'frame_hw': [H, W], 'rounds': args.rounds,
       'verts': int(verts.shape[0]), 'faces': int(faces.shape[0]), 'grid': list(scene.index.dims),
       'cell': float(scene.index.cell), 'refs': int(scene.index.n_refs), 'frame_rays': int(dirs.shape[0]),
       'lidar_rays': int(lidar.shape[0]), 'pairs': args.pairs}

plain = jobs['closest_frames']()
ordered = jobs['closest_frames_sorted']()
res['sorted_equal'] = bool(all(torch.equal(a, b) for a, b in zip(plain, ordered)))
res['frame_hit_share'] = round(float((plain.face >= 0).float().mean()), 4)
depth = jobs['render_depth']().reshape(-1)
both = (plain.face >= 0) & (depth > 0)
res['frames_median_abs_t_minus_depth'] = float((plain.t[both] - depth[both]).abs().median())
del plain, ordered, depth, both
counters = torch.zeros(2, dtype=torch.int64, device=dev)
scene.closest(orig, dirs, t_min=0.1, t_max=far, counters=counters)
res['frames_cells_per_ray'], res['frames_pairs_per_ray'] = [round(int(c) / dirs.shape[0], 3) for c in counters]
counters.zero_()
scene.occluded(samples, eyes, counters=counters)
res['occluded_cells_per_ray'], res['occluded_pairs_per_ray'] = [round(int(c) / args.pairs, 3) for c in counters]
res['occluded_share'] = round(float(jobs['occluded_pairs']().float().mean()), 4)
res['lidar_hits'] = int(jobs['lidar_sweep']()[0].shape[0])

for job in jobs.values():                                                  # warm-up of every shape that is timed
    job()
torch.cuda.synchronize()
times = {n: [] for n in jobs}
for _ in range(args.rounds):
    for n, job in jobs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        job()
        e.record()
        torch.cuda.synchronize()
        times[n].append(s.elapsed_time(e))
for n, runs in times.items():
    res[n + '_ms'] = round(statistics.median(runs), 3)
    res[n + '_ms_runs'] = [round(t, 3) for t in runs]
res['closest_mrays_per_s'] = round(dirs.shape[0] / res['closest_frames_ms'] / 1e3, 1)
res['closest_over_render'] = round(res['closest_frames_ms'] / res['render_depth_ms'], 3)
res['closest_over_copy'] = round(res['closest_frames_ms'] / res['copy_ray_bytes_ms'], 3)
res['sorted_over_unsorted'] = round(res['closest_frames_sorted_ms'] / res['closest_frames_ms'], 3)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
