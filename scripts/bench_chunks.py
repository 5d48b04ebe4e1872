"""Chunk cutting cost at scene size: the 512 x 512 x 128 room of scripts/bench_fusion.py (2 cm voxels, synthetic
320 x 240 frames), fused once into an input volume (every third frame) and a four-level target pyramid (all frames).

Timed, with device events after an untimed warm-up, median of --reps runs: ChunkCutter.candidates() and
ChunkCutter.batch() for 32 crops of 128 x 64 x 64, their kernels one by one with the bytes each moves and the
fraction of the measured HBM copy rate that makes, and beside them the route that existed before: the same 32 crops
as .sdfs files on disk read by DeviceBatchLoader (whole: read + pack + copy + decode, host clock; decode alone:
device events).  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402
from sgnn_amd import _lib, chunks, data, fusion  # noqa: E402

HBM_TBS = 6.29                       # MI355X: measured HBM copy rate (MI355X_MICROARCH)

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=150)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--crops', type=int, default=32)
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--out', default='')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W = 240, 320
CROP, STRIDE = (128, 64, 64), (128, 32, 32)

# the room of bench_fusion.py: walls, floor, ceiling and furniture boxes, two loops of a wobbly circle
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
kk = np.tile(K, (args.frames, 1))
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)


def median_ms(fn, reps=args.reps, device=True):
    """Median over reps of one call: device events (launch to completion on the stream) or the host clock."""
    fn()
    fn()                                                                   # untimed warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        if device:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e))
        else:
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def rate(nbytes, ms):
    return {'ms': round(ms, 4), 'MB': round(nbytes / 1e6, 2), 'GBps': round(nbytes / ms / 1e6, 1),
            'share_of_HBM': round(nbytes / (ms * 1e-3) / (HBM_TBS * 1e12), 3)}


filt = fusion.bilateral(torch.from_numpy(depth).cuda())
sub = slice(0, None, 3)
target = fusion.TSDFPyramid(dims, args.voxel, w2g).integrate(filt[sub], kk[sub], poses[sub])
scan = target[0].copy()
rest = np.setdiff1d(np.arange(args.frames), np.arange(args.frames)[sub])
target.integrate(filt[rest], kk[rest], poses[rest])
cutter = chunks.ChunkCutter(scan, target, CROP, STRIDE)
res = {'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frames': args.frames, 'crop_zyx': list(CROP),
       'stride_zyx': list(STRIDE), 'reps': args.reps}

origins, counts = cutter.scores()
order = np.argsort(-counts[:, 1], kind='stable')[:args.crops]              # the windows with most input sites
pick = origins[np.sort(order)]
nb = len(pick)
res.update(windows=int(len(origins)), crops=nb, target_voxels_in_band=int(counts[order, 0].sum()),
           input_sites=int(counts[order, 1].sum()))

nvox = dims[0] * dims[1] * dims[2]
nbricks = -(-dims[0] // 8) * -(-dims[1] // 8) * -(-dims[2] // 8)
bricks = torch.empty((nbricks, 2), dtype=torch.int32, device='cuda')
table = torch.empty((len(origins), 2), dtype=torch.int32, device='cuda')
dx, dy, dz = dims
res['candidates_ms'] = round(median_ms(lambda: cutter.candidates(1000, 100)), 4)
res['candidates_host_ms'] = round(median_ms(lambda: cutter.candidates(1000, 100), device=False), 4)
res['kernel_score'] = rate(8.0 * nvox + 8.0 * nbricks, median_ms(lambda: _lib.call(
    'sgnn_chunk_score', target[0].sdf().data_ptr(), scan.sdf().data_ptr(), dx, dy, dz, float(cutter.voxel_size), 3.0,
    cutter._keep(0), *CROP, *STRIDE, *cutter.grid, bricks.data_ptr(), table.data_ptr())))

res['batch_ms'] = round(median_ms(lambda: cutter.batch(pick)), 4)
res['batch_host_ms'] = round(median_ms(lambda: cutter.batch(pick), device=False), 4)
b = cutter.batch(pick)
rows = int(b['input'][0].shape[0])
res['batch_input_rows'] = rows
ncrop = nb * CROP[0] * CROP[1] * CROP[2]
_, dev_o = cutter._origins(pick)
mask = torch.empty(ncrop, dtype=torch.uint8, device='cuda')
res['kernel_flag'] = rate(5.0 * ncrop, median_ms(lambda: _lib.call(
    'sgnn_chunk_flag', scan.sdf().data_ptr(), dx, dy, dz, dev_o.data_ptr(), nb, *CROP, cutter._keep(0), 3.0,
    float(cutter.voxel_size), mask.data_ptr())))
for k in range(4):                                                         # read f32, write f32 (+ u8 known at level 0)
    n_k = ncrop // 8 ** k
    res['kernel_crop_level%d' % k] = rate((9.0 if k == 0 else 8.0) * n_k, median_ms(
        lambda: cutter._dense(target[k], k, dev_o, nb, float(cutter.voxel_size), known=(k == 0))))

# the route that existed before: the same crops as files, read by DeviceBatchLoader
with tempfile.TemporaryDirectory() as tmp:
    t = time.perf_counter()
    files = cutter.save(pick, tmp, 'bench')
    res['save_host_ms'] = round((time.perf_counter() - t) * 1e3, 1)
    res['file_bytes'] = int(sum(os.path.getsize(f) for f in files))
    loader = data.DeviceBatchLoader(files, nb, 3.0, 4, prefetch=1, workers=1)
    res['file_route_ms'] = round(median_ms(lambda: next(iter(loader)), device=False), 4)
    staging, plan = loader._stage(files)
    res['file_route_decode_ms'] = round(median_ms(lambda: loader._decode(staging, plan)), 4)
    fb = loader._decode(staging, plan)
    same = (torch.equal(fb['input'][0], b['input'][0]) and torch.equal(fb['sdf'], b['sdf']) and
            torch.equal(fb['known'], b['known']) and all(torch.equal(x, y) for x, y in zip(fb['hierarchy'], b['hierarchy'])))
    res['file_route_batch_identical'] = bool(same)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
