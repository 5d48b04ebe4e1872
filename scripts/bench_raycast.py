"""TSDF ray-casting cost at scene size: a configs[3]-sized volume (512 x 512 x 128 voxels at 2 cm) fused from
320 x 240 depth frames rendered along a trajectory through an analytic room (the scene of scripts/bench_fusion.py),
cast back to 100 frames of 240 x 320 at the same poses.

Every variant (skip on / off, normals on / off) is warmed up, then the four are timed in turn for --rounds rounds
with device events around raycast.cast (brick pass, frame table upload and cast launch), so that drift of a shared
machine hits all of them alike; the best and all runs are reported as rays per second.  The sample counters come
from one extra call per variant outside the timed ones, and the four outputs are compared bit for bit.  Prints one
JSON line; --out also writes it.
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
from sgnn_amd import fusion, raycast  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=100)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--step', type=float, default=0.5)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W = 240, 320

# the room fills the volume: walls, floor, ceiling and furniture boxes
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
    a = 2 * np.pi * 2 * i / args.frames                                    # two loops
    r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
    eye = np.array([c[0] + r * np.cos(a), c[1] + r * np.sin(a), min(1.5, ext[2] * 0.6)])
    tgt = eye + np.array([np.cos(a + 1.2), np.sin(a + 1.2), -0.35])
    poses.append(R.look_at(eye, tgt))
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
kk = np.tile(K, (F, 1))

vol = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(depth, kk, poses)
sdf = vol.sdf()
band = np.float32(3.0) * vol.voxel_size
torch.cuda.synchronize()
res = {'frames': F, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W], 'step': args.step,
       'rays': F * H * W, 'render_host_s': round(render_s, 2),
       'samples_per_ray': raycast.sample_count(0.4, 4.0, np.float32(args.step) * vol.voxel_size),
       'usable_voxel_share': round(float((sdf.abs() < float(band)).float().mean().item()), 4)}

variants = [(skip, normals) for normals in (False, True) for skip in (True, False)]


def name(skip, normals):
    return '%s_%s' % ('skip' if skip else 'noskip', 'normals' if normals else 'depth')


def run(skip, normals, counters=None):
    return raycast.cast(sdf, w2g, args.voxel, kk, poses, (H, W), band, step=args.step, normals=normals, skip=skip,
                        counters=counters)


outs = {}
for skip, normals in variants:                                            # warm-up, counters, outputs to compare
    ctr = torch.zeros(2, dtype=torch.int64, device='cuda')
    outs[skip, normals] = run(skip, normals, ctr)
    ev, sk = (int(v) for v in ctr.cpu())
    res[name(skip, normals)] = {'samples_evaluated': ev, 'samples_skipped': sk}
    run(skip, normals)
torch.cuda.synchronize()


def bits(t):
    return t.view(torch.int32)


d_ref = outs[False, False]
res['hit_share'] = round(float(torch.isfinite(d_ref).float().mean().item()), 4)
res['identical_bits'] = bool(
    all(torch.equal(bits(outs[s, False]), bits(d_ref)) for s in (True, False)) and
    all(torch.equal(bits(outs[s, True][0]), bits(d_ref)) for s in (True, False)) and
    torch.equal(bits(outs[True, True][1]), bits(outs[False, True][1])))
both = torch.isfinite(d_ref) & torch.isfinite(torch.from_numpy(depth).cuda())
res['median_abs_cast_minus_input_m'] = round(float((d_ref - torch.from_numpy(depth).cuda())[both].abs().median().item()), 6)
del outs

times = {v: [] for v in variants}
for _ in range(args.rounds):
    for v in variants:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run(*v)
        e.record()
        torch.cuda.synchronize()
        times[v].append(s.elapsed_time(e) / 1e3)
for v in variants:
    r = res[name(*v)]
    r['s_runs'] = [round(t, 5) for t in times[v]]
    r['s'] = round(min(times[v]), 5)
    r['grays_per_s'] = round(res['rays'] / min(times[v]) / 1e9, 3)
res['skip_not_slower'] = bool(res['skip_depth']['s'] <= res['noskip_depth']['s'] and
                              res['skip_normals']['s'] <= res['noskip_normals']['s'])
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
