"""Mesh-distance cost at scene size: the two meshes of scripts/bench_render.py, (a) the tessellated room (walls and
14 furniture boxes, about 500 k triangles) and (b) the marching-cubes mesh of 1000 rendered frames of (a) fused into
the 512 x 512 x 128 bench volume.  Each mesh is indexed and queried with 1 M points sampled on the other.

Times come from device events, the median of 9 calls after a warm-up, for the unbounded query with and without the
sort by cell and for a query bounded by --max-dist; separate calls with counters give cells and pairs per point.
Context: the time a copy of the inputs takes at the HBM copy rate, and pairs/s against the fp32 vector rate.  Prints one JSON line; --out also writes it.
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
from sgnn_amd import fusion, marching_cubes as mc, meshdist, render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--tess', type=int, default=53, help='quads per box edge: 15 boxes x 12 n^2 triangles')
ap.add_argument('--points', type=int, default=1000000)
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--max-dist', type=float, default=0.1, help='bound of the third query (metres)')
ap.add_argument('--out', default='')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W, F = 240, 320, args.frames
HBM_COPY_TBS, FP32_VECTOR_TFLOPS = 6.29, 157.3        # measured copy rate; data-sheet vector fp32
PAIR_FLOPS = 90                                       # rule 2, all branches taken once: about 90 fp32 operations

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
dev = torch.device('cuda')
verts_a = torch.from_numpy(np.concatenate([p for p, _ in parts]).astype(np.float32)).to(dev)
faces_a = torch.from_numpy(np.concatenate([t for _, t in parts]).astype(np.int32)).to(dev)

K = np.tile(np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], np.float32), (F, 1))
c = ext / 2
a = 2 * np.pi * 2 * np.arange(F) / F
r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
eyes = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), np.full(F, min(1.5, ext[2] * 0.6))], 1)
poses = render.look_at(eyes, eyes + np.stack([np.cos(a + 1.2), np.sin(a + 1.2), np.full(F, -0.35)], 1))
depth = render.render_depth(verts_a, faces_a, K, poses, (H, W))
vol = fusion.TSDFVolume(dims, args.voxel, R.grid_transform((0.0, 0.0, 0.0), args.voxel)).integrate(depth, K, poses)
del depth
vv, _, faces_b = mc.run_marching_cubes(vol.sdf() / args.voxel, None, 0.0, 3.0, 10.0)
del vol
verts_b = (vv * args.voxel).contiguous()


def timed(fn):
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return out, float(np.median(times)), [round(t, 3) for t in times]


res = {'points': args.points, 'frames': F, 'dims_xyz': list(dims), 'voxel_size': args.voxel}
meshes = {'room_tessellated': (verts_a, faces_a), 'marching_cubes_mesh': (verts_b, faces_b)}
for tag, other in (('room_tessellated', 'marching_cubes_mesh'), ('marching_cubes_mesh', 'room_tessellated')):
    v, f = meshes[tag]
    (pts, _), sample_ms, _ = timed(lambda: meshdist.sample_surface(*meshes[other], args.points, seed=1))
    index, build_ms, build_runs = timed(lambda: meshdist.TriangleIndex(v, f))
    row = {'verts': int(v.shape[0]), 'triangles': int(f.shape[0]), 'queried_with': other, 'cell': float(index.cell),
           'grid': list(index.dims), 'references': index.n_refs, 'build_ms': round(build_ms, 3), 'build_ms_runs': build_runs,
           'sample_ms': round(sample_ms, 3)}
    for name, sort in (('sorted', True), ('unsorted', False)):                  # unsorted is the default
        (d, _), ms, runs = timed(lambda: index.distance(pts, sort=sort))
        row['query_ms_' + name], row['query_ms_runs_' + name] = round(ms, 3), runs
        row['mpoints_per_s_' + name] = round(args.points / ms / 1e3, 2)
    (dm, _), ms, runs = timed(lambda: index.distance(pts, max_dist=args.max_dist))
    row['max_dist'], row['query_ms_max_dist'], row['query_ms_runs_max_dist'] = args.max_dist, round(ms, 3), runs
    row['share_beyond_max_dist'] = round(torch.isinf(dm).float().mean().item(), 4)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    index.distance(pts, counters=cnt, max_dist=args.max_dist)
    row['cells_per_point_max_dist'], row['pairs_per_point_max_dist'] = (round(int(x) / args.points, 2) for x in cnt.cpu())
    cnt.zero_()
    index.distance(pts, counters=cnt)
    cells, pairs = (int(x) for x in cnt.cpu())
    best = min(row['query_ms_sorted'], row['query_ms_unsorted'])
    in_bytes = int(v.numel() * 4 + f.numel() * 4 + pts.numel() * 4 + args.points * 8)
    row.update({'cells_per_point': round(cells / args.points, 2), 'pairs_per_point': round(pairs / args.points, 2),
                'gpairs_per_s': round(pairs / best / 1e6, 2), 'mean_distance': float(d.double().mean().item()),
                'context_copy_inputs_ms': round(in_bytes / (HBM_COPY_TBS * 1e9), 4),
                'context_share_of_fp32_vector_rate': round(pairs * PAIR_FLOPS / (best * 1e-3) / (FP32_VECTOR_TFLOPS * 1e12), 4)})
    res[tag] = row
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
