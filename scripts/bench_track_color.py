"""Tracking with colour at scene size: the scene of scripts/bench_track.py (the analytic room in a 512 x 512 x 128
volume at 2 cm, 100 rendered 240 x 320 frames along a hand-held sweep) with a texture on every surface, tracked and
fused frame by frame with track.track_sequence(color_frames=) from the first frame's true pose; and, as the yardstick,
the same depth frames through the depth-only track_sequence in the same run.

Reports milliseconds per frame split into the casts of the model (one per pyramid level, in colour), the system
launches with their read-backs (both systems, the pyramids and the live normals), the host solve and the integration,
from host clocks around device synchronisations (track's timers), after a warm-up on a second volume; and the drift
against the true trajectory.  The frames are rendered on the host once; each of the two GPU steps then runs as a child
process under its own time limit, and the second is not started when the first fails.  Prints one JSON line; --out
also writes it (profiles/track_color_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=100)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--step', type=float, default=0.01, help='radians of the sweep per frame')
ap.add_argument('--limit', type=float, default=240.0, help='seconds each GPU step may take')
ap.add_argument('--out', default='')
ap.add_argument('--child', default='', help='(internal) depth | color: run one GPU step on the frames of --scene')
ap.add_argument('--scene', default='', help='(internal) the .npz of rendered frames')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
H, W = 240, 320


def pose_error(a, b):
    rel = np.linalg.inv(a) @ b
    return (float(np.linalg.norm(a[:3, 3] - b[:3, 3])),
            float(np.degrees(np.arccos(np.clip((np.trace(rel[:3, :3]) - 1) / 2, -1.0, 1.0)))))


def gpu_step(kind):
    """One GPU step in this process: a warm-up, a run without timers, a run with the stages split -> dict."""
    import torch
    from sgnn_amd import fusion, track
    scene = np.load(args.scene)
    depth, K, poses = torch.from_numpy(scene['depth']).cuda(), scene['K'], scene['poses']
    color = kind == 'color'
    kw = [dict(color_frames=torch.from_numpy(scene['rgba'][lo:hi]).cuda()) if color else {}
          for lo, hi in ((0, 3), (0, len(poses)))]
    w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
    F = len(poses)

    def volume():
        return fusion.TSDFVolume(dims, args.voxel, w2g, color=color)

    track.track_sequence(volume(), depth[:3], K, poses[0], **kw[0])                               # warm-up
    torch.cuda.synchronize()
    vol = volume()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est, results = track.track_sequence(vol, depth, K, poses[0], **kw[1])
    torch.cuda.synchronize()
    total_s = time.perf_counter() - t0
    timers = {}
    est2, _ = track.track_sequence(volume(), depth, K, poses[0], timers=timers, **kw[1])
    tracked = max(F - 1, 1)
    errs = [pose_error(p, e) for p, e in zip(poses, est)]
    out = {'lost_frames': int(sum(not r.ok for r in results)), 'ms_per_frame': round(1e3 * total_s / F, 3),
           'ms_per_frame_split': {k: round(1e3 * v / (F if k == 'integrate' else tracked), 3) for k, v in sorted(timers.items())},
           'pairs_mean': round(float(np.mean([r.pairs for r in results[1:]])) if F > 1 else 0.0, 1),
           'drift_last_m': round(errs[-1][0], 5), 'drift_last_deg': round(errs[-1][1], 4),
           'drift_max_m': round(max(e[0] for e in errs), 5), 'drift_max_deg': round(max(e[1] for e in errs), 4),
           'same_poses_with_timers': bool(np.array_equal(est, est2))}
    if color:
        out['color_pairs_mean'] = round(float(np.mean([r.color_pairs for r in results[1:]])) if F > 1 else 0.0, 1)
        out['color_weight'], out['max_intensity'] = 1e-3, 40.0
    return out


if args.child:
    print(json.dumps(gpu_step(args.child)))
    sys.exit(0)

# the room fills the volume: walls, floor, ceiling and furniture boxes (the scene of bench_track.py)
ext = np.array(dims) * args.voxel
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
    """bench_track's depth, and a grey texture of the hit point: three sinusoids along the world axes with periods of
    0.5 to 0.7 m (25 voxels and more), so every surface varies along both of its directions."""
    depth = R.render(K, p, (H, W), planes, boxes)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dirs = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1)
    hit = np.isfinite(depth)
    x = p[:3, 3] + np.where(hit, depth, 0.0)[..., None].astype(np.float64) * (dirs @ p[:3, :3].T)
    grey = 128 + 40 * (np.sin(2 * np.pi * x[..., 0] / 0.5) + np.sin(2 * np.pi * x[..., 1] / 0.6) +
                       np.sin(2 * np.pi * x[..., 2] / 0.7))
    grey = np.clip(np.rint(grey), 0, 255).astype(np.uint8)
    return depth, np.where(hit[..., None], np.stack([grey, grey, grey, np.full_like(grey, 255)], -1), 0).astype(np.uint8)


t0 = time.perf_counter()
import multiprocessing  # noqa: E402
with multiprocessing.get_context('fork').Pool(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
    frames = pool.map(_render, list(poses), chunksize=4)
render_s = time.perf_counter() - t0
res = {'frames': args.frames, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W],
       'render_host_s': round(render_s, 2), 'iterations': [10, 5, 4]}
with tempfile.TemporaryDirectory() as tmp:
    scene = os.path.join(tmp, 'scene.npz')
    np.savez(scene, depth=np.stack([f[0] for f in frames]), rgba=np.stack([f[1] for f in frames]), K=K, poses=poses)
    for kind in ('depth', 'color'):                                        # the yardstick first
        cmd = [sys.executable, os.path.abspath(__file__), '--child', kind, '--scene', scene, '--dims', args.dims,
               '--voxel', str(args.voxel)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit('the %s step did not finish in %g s' % (kind, args.limit))
        if done.returncode != 0:
            sys.exit('the %s step ended with status %d' % (kind, done.returncode))
        res[kind + '_only' if kind == 'depth' else kind] = json.loads(done.stdout.decode().strip().splitlines()[-1])
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
