"""Tracking cost at scene size: the analytic room of scripts/bench_raycast.py in a configs[3]-sized volume
(512 x 512 x 128 voxels at 2 cm), 100 rendered 240 x 320 depth frames along a hand-held sweep, tracked and fused
frame by frame with track.track_sequence from the first frame's true pose.

Reports milliseconds per frame split into the casts of the model (one per pyramid level), the system launches with
their 256-byte read-backs (pyramid and live normals included), the host solve and the integration, from host clocks
around device synchronisations (track's timers), after a warm-up run on a second volume; and the drift against the true
trajectory.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402
from sgnn_amd import fusion, track  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=100)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--step', type=float, default=0.01, help='radians of the sweep per frame')
ap.add_argument('--out', default='')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W = 240, 320

# the room fills the volume: walls, floor, ceiling and furniture boxes (the scene of bench_raycast.py)
planes = [((0, 0, 1), 0.05), ((0, 0, -1), -(ext[2] - 0.05)), ((1, 0, 0), 0.1), ((-1, 0, 0), -(ext[0] - 0.1)),
          ((0, 1, 0), 0.1), ((0, -1, 0), -(ext[1] - 0.1))]
rng = np.random.default_rng(0)
boxes = []
for _ in range(14):
    lo = np.array([rng.uniform(0.3, ext[0] - 1.5), rng.uniform(0.3, ext[1] - 1.5), 0.05])
    boxes.append((lo, lo + np.array([rng.uniform(0.4, 1.4), rng.uniform(0.4, 1.4), rng.uniform(0.3, 1.6)])))
K = np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], np.float32)
c = ext / 2
poses = []
for i in range(args.frames):
    a = args.step * i                                                      # about 3 cm and 0.6 degrees a frame
    r = 0.3 * min(ext[0], ext[1])
    eye = np.array([c[0] + r * np.cos(a), c[1] + r * np.sin(a), min(1.5, ext[2] * 0.6) + 0.05 * np.sin(0.2 * i)])
    poses.append(R.look_at(eye, eye + np.array([np.cos(a + 1.2), np.sin(a + 1.2), -0.35])))
poses = np.stack(poses)


def _render(p):
    return R.render(K, p, (H, W), planes, boxes)


t0 = time.perf_counter()
import multiprocessing  # noqa: E402
with multiprocessing.get_context('fork').Pool(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:   # before CUDA
    depth = np.stack(pool.map(_render, list(poses), chunksize=4))
render_s = time.perf_counter() - t0
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
F = args.frames
dev_depth = torch.from_numpy(depth).cuda()

track.track_sequence(fusion.TSDFVolume(dims, args.voxel, w2g), dev_depth[:3], K, poses[0])      # warm-up
torch.cuda.synchronize()

# one run without timers (no synchronisation but the read-backs), one with the stages split
vol = fusion.TSDFVolume(dims, args.voxel, w2g)
torch.cuda.synchronize()
t0 = time.perf_counter()
est, results = track.track_sequence(vol, dev_depth, K, poses[0])
torch.cuda.synchronize()
total_s = time.perf_counter() - t0

timers = {}
est2, _ = track.track_sequence(fusion.TSDFVolume(dims, args.voxel, w2g), dev_depth, K, poses[0], timers=timers)


def pose_error(a, b):
    rel = np.linalg.inv(a) @ b
    return (float(np.linalg.norm(a[:3, 3] - b[:3, 3])),
            float(np.degrees(np.arccos(np.clip((np.trace(rel[:3, :3]) - 1) / 2, -1.0, 1.0)))))


tracked = max(F - 1, 1)
errs = [pose_error(p, e) for p, e in zip(poses, est)]
res = {'frames': F, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W], 'render_host_s': round(render_s, 2),
       'iterations': [10, 5, 4], 'lost_frames': int(sum(not r.ok for r in results)),
       'ms_per_frame': round(1e3 * total_s / F, 3),
       'ms_per_frame_split': {k: round(1e3 * v / (F if k == 'integrate' else tracked), 3) for k, v in sorted(timers.items())},
       'pairs_mean': round(float(np.mean([r.pairs for r in results[1:]])) if F > 1 else 0.0, 1),
       'rmse_mean_m': round(float(np.mean([r.rmse for r in results[1:] if r.ok])) if F > 1 else 0.0, 6),
       'drift_last_m': round(errs[-1][0], 5), 'drift_last_deg': round(errs[-1][1], 4),
       'drift_max_m': round(max(e[0] for e in errs), 5), 'drift_max_deg': round(max(e[1] for e in errs), 4),
       'same_poses_with_timers': bool(np.array_equal(est, est2))}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
