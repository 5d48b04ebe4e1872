"""What colour costs in TSDF fusion, on the volume and frames of scripts/bench_fusion.py: 512 x 512 x 128 voxels at
2 cm, synthetic 320 x 240 depth frames through an analytic room, noise colour frames from a 640 x 480 sensor.

Warm medians of 5 runs each, from device events: depth-only integration (sgnn_fuse_integrate), colour integration
(sgnn_fusecol_integrate), pack_color of the raw frames, and the ratio colour / depth-only; min and max of the 5 runs
are the spread.  With --parent-lib PATH (a libsgnn_hip.so built from the parent commit, e.g. in a git worktree) a
fresh process times depth-only integration with that library on the same frames, to show whether the depth-only path
has moved.  Prints one JSON line; --out also writes it (profiles/fusion_color_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--parent-lib', default='', help='libsgnn_hip.so of the parent commit')
ap.add_argument('--out', default='')
ap.add_argument('--depth-only-on', default='', help='(internal) .npz of frames: time depth-only integration, print JSON')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
H, W = 240, 320


def stats(times):
    return {'median_s': round(float(np.median(times)), 5), 'min_s': round(min(times), 5), 'max_s': round(max(times), 5),
            'runs_s': [round(t, 5) for t in times]}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 1e3


def time_integrate(fusion, filt, kk, poses, w2g, color=None):
    """Warm-up, then args.runs timed integrations of all frames into a fresh volume each."""
    times = []
    for rep in range(args.runs + 1):
        vol = fusion.TSDFVolume(dims, args.voxel, w2g, color=color is not None)
        t = timed(lambda: vol.integrate(filt, kk, poses, color=color))
        if rep:
            times.append(t)
    return stats(times), vol


if args.depth_only_on:                                                       # the child: whatever library SGNN_LIB names
    from sgnn_amd import fusion
    z = np.load(args.depth_only_on)
    filt = torch.from_numpy(z['filt']).cuda()
    print(json.dumps(time_integrate(fusion, filt, z['kk'], z['poses'], z['w2g'])[0]))
    sys.exit(0)

# the scene of scripts/bench_fusion.py: a room that fills the volume, furniture boxes, two loops of a wobbly circle
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
    a = 2 * np.pi * 2 * i / args.frames
    r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
    eye = np.array([c[0] + r * np.cos(a), c[1] + r * np.sin(a), min(1.5, ext[2] * 0.6)])
    poses.append(R.look_at(eye, eye + np.array([np.cos(a + 1.2), np.sin(a + 1.2), -0.35])))
poses = np.stack(poses)


def _render(p):
    return R.render(K, p, (H, W), planes, boxes)


import multiprocessing  # noqa: E402
with multiprocessing.get_context('fork').Pool(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:   # before CUDA
    depth = np.stack(pool.map(_render, list(poses), chunksize=8))
raw_rgb = np.random.default_rng(1).integers(0, 256, size=(args.frames, 2 * H, 2 * W, 3), dtype=np.uint8)
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
kk = np.tile(K, (args.frames, 1))

from sgnn_amd import fusion  # noqa: E402
filt = fusion.bilateral(torch.from_numpy(depth).cuda())
raw_d = torch.from_numpy(raw_rgb).cuda()
fusion.pack_color(raw_d[:4], (H, W))                                         # warm-up
pack_times = [timed(lambda: fusion.pack_color(raw_d, (H, W))) for _ in range(args.runs)]
col = fusion.pack_color(raw_d, (H, W))
del raw_d

res = {'frames': args.frames, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W],
       'raw_color_hw': [2 * H, 2 * W], 'runs': args.runs}
res['depth_only'], plain = time_integrate(fusion, filt, kk, poses, w2g)
res['color'], vol = time_integrate(fusion, filt, kk, poses, w2g, color=col)
res['depth_only_again'], _ = time_integrate(fusion, filt, kk, poses, w2g)   # the same code twice: the drift of the box
res['pack_color'] = stats(pack_times)
res['pack_color_ms_per_frame'] = round(res['pack_color']['median_s'] * 1e3 / args.frames, 5)
res['color_over_depth_only'] = round(res['color']['median_s'] / res['depth_only']['median_s'], 4)
res['same_geometry'] = bool(torch.equal(vol.sdf().view(torch.int32), plain.sdf().view(torch.int32)) and
                            torch.equal(vol.weight(), plain.weight()))
res['colored_voxels'] = int((vol.color_weight() > 0).sum())
res['parent_depth_only'] = None                                              # not measured without --parent-lib
if args.parent_lib:
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'frames.npz')
        np.savez(path, filt=filt.cpu().numpy(), kk=kk, poses=poses, w2g=w2g)
        env = dict(os.environ, SGNN_LIB=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--depth-only-on', path, '--dims', args.dims,
                              '--voxel', str(args.voxel), '--runs', str(args.runs)], env=env, check=True,
                             stdout=subprocess.PIPE, timeout=600).stdout.decode()
    res['parent_depth_only'] = json.loads(out.strip().splitlines()[-1])
    res['depth_only_over_parent'] = round(res['depth_only']['median_s'] / res['parent_depth_only']['median_s'], 4)
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
