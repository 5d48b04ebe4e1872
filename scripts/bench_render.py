"""Depth rendering cost at scene size: 1000 frames of 320 x 240 along the room trajectory of scripts/bench_fusion.py
over (a) the tessellated room (walls and 14 furniture boxes, about 500 k triangles) and (b) the marching-cubes mesh
of those frames fused into the 512 x 512 x 128 bench volume.

Times come from device events, the median of 9 calls after a warm-up; a separate call with counters gives the work:
(frame, triangle) pairs, triangles drawn per lane and per wave, covered pixels (= atomic minima issued).  The split
between the kernels comes from a kernel trace of `--once` (one call per mesh, no counters).  Prints one JSON line;
--out also writes it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402
from sgnn_amd import fusion, marching_cubes as mc, render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--tess', type=int, default=53, help='quads per box edge: 15 boxes x 12 n^2 triangles')
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--once', action='store_true', help='one timed call per mesh, for a kernel trace')
ap.add_argument('--out', default='')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W = 240, 320
F = args.frames

rng = np.random.default_rng(0)
boxes = [(np.array([0.1, 0.1, 0.05]), np.array([ext[0] - 0.1, ext[1] - 0.1, ext[2] - 0.05]))]
for _ in range(14):
    lo = np.array([rng.uniform(0.3, ext[0] - 1.5), rng.uniform(0.3, ext[1] - 1.5), 0.05])
    boxes.append((lo, lo + np.array([rng.uniform(0.4, 1.4), rng.uniform(0.4, 1.4), rng.uniform(0.3, 1.6)])))
parts, base = [], 0
for lo, hi in boxes:
    p, t = RR.box_mesh(lo, hi, args.tess)
    parts.append((p, t + base))
    base += len(p)
verts_a = np.concatenate([p for p, _ in parts]).astype(np.float32)
faces_a = np.concatenate([t for _, t in parts]).astype(np.int32)

K = np.tile(np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], np.float32), (F, 1))
c = ext / 2
a = 2 * np.pi * 2 * np.arange(F) / F                                          # two loops
r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
eyes = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), np.full(F, min(1.5, ext[2] * 0.6))], 1)
poses = render.look_at(eyes, eyes + np.stack([np.cos(a + 1.2), np.sin(a + 1.2), np.full(F, -0.35)], 1))

dev = torch.device('cuda')
res = {'frames': F, 'frame_hw': [H, W], 'dims_xyz': list(dims), 'voxel_size': args.voxel}


def measure(tag, verts, faces):
    v, f = verts.to(dev) if torch.is_tensor(verts) else torch.from_numpy(verts).to(dev), \
        faces.to(dev) if torch.is_tensor(faces) else torch.from_numpy(faces).to(dev)
    call = lambda **kw: render.render_depth(v, f, K, poses, (H, W), **kw)    # noqa: E731
    out = call()                                                               # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(1 if args.once else args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = call()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    ms = float(np.median(times))
    res[tag] = {'verts': int(v.shape[0]), 'triangles': int(f.shape[0]), 'ms': round(ms, 3),
                'ms_runs': [round(t, 3) for t in times], 'finite_share': round(torch.isfinite(out).float().mean().item(), 4)}
    if not args.once:
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        call(counters=cnt)
        lane, wave, pixels = (int(x) for x in cnt.cpu())
        pairs = F * int(f.shape[0])
        res[tag].update({'frame_triangle_pairs': pairs, 'gpairs_per_s': round(pairs / ms / 1e6, 2),
                         'drawn_per_lane': lane, 'drawn_per_wave': wave,
                         'wave_share_of_drawn': round(wave / max(lane + wave, 1), 5),
                         'drawn_share_of_pairs': round((lane + wave) / pairs, 5),
                         'covered_pixels': pixels, 'gatomics_per_s': round(pixels / ms / 1e6, 3),
                         'overdraw': round(pixels / (F * H * W), 3)})
    return out


depth = measure('room_tessellated', verts_a, faces_a)
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
vol = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(depth, K, poses)
del depth
vv, _, ff = mc.run_marching_cubes(vol.sdf() / args.voxel, None, 0.0, 3.0, 10.0)
del vol
measure('marching_cubes_mesh', vv * args.voxel, ff)                            # world2grid is a pure scale here
res['context'] = {'fusion_integrate_ms_same_frames': 22.2, 'output_bytes': F * H * W * 4}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
