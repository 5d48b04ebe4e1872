"""TSDF fusion cost at scene size: a configs[3]-sized volume (512 x 512 x 128 voxels at 2 cm) and synthetic
320 x 240 depth frames along a trajectory through an analytic room (tests/fusion_ref.py renders them).

Times come from device events after a warm-up of every launch shape: raw conversion and bilateral filter per
frame, integration at chunk sizes 1, 8, 64 and all frames, sparse export, scan_sample, and frames -> model input
end to end.  Work is counted from the frame boxes (voxel-frame visits).  Prints one JSON line; --out also writes it.
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
from sgnn_amd import fusion  # noqa: E402

HBM_TBS, L2_TBS = 6.29, 34.5          # MI355X: measured HBM copy rate, aggregate L2 rate (MI355X_MICROARCH)

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--chunks', default='1,8,64,0', help='0 = all frames in one launch')
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
    depth = np.stack(pool.map(_render, list(poses), chunksize=8))
render_s = time.perf_counter() - t0
raw = np.where(np.isfinite(depth), np.round(depth * 1000.0), 0).astype(np.uint16)
raw = np.repeat(np.repeat(raw, 2, 1), 2, 2)                                 # a 640 x 480 sensor
k_raw = np.array([2 * K[0], 2 * K[1], 2 * K[2] + 0.5, 2 * K[3] + 0.5], np.float32)
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)

dev = torch.device('cuda')
raw_d = torch.from_numpy(raw.view(np.int16)).to(dev)
torch.cuda.synchronize()


def ev_time(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps / 1e3, out


def host_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


res = {'frames': args.frames, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W],
       'render_host_s': round(render_s, 2)}
F = args.frames
# warm-up of every launch shape used below
metric, k_adapt = fusion.raw_depth_to_metric(raw_d[:4], 1000.0, (H, W), intrinsics=k_raw)
fusion.bilateral(metric)
small = fusion.TSDFVolume(dims, args.voxel, w2g)
table = small.frame_table(np.tile(k_adapt, (F, 1)), poses, (H, W))
box = table['box'].astype(np.int64)
visits = int(np.sum(np.clip(box[:, 1] - box[:, 0] + 1, 0, None) * np.clip(box[:, 3] - box[:, 2] + 1, 0, None) *
                    np.clip(box[:, 5] - box[:, 4] + 1, 0, None)))
res['voxel_frame_visits'] = visits
res['mean_box_voxels'] = visits / F

t_raw, (metric, k_adapt) = ev_time(lambda: fusion.raw_depth_to_metric(raw_d, 1000.0, (H, W), intrinsics=k_raw), 3)
t_bil, filt = ev_time(lambda: fusion.bilateral(metric), 3)
res['raw_ms_per_frame'] = t_raw * 1e3 / F
res['bilateral_ms_per_frame'] = t_bil * 1e3 / F
kk = np.tile(k_adapt, (F, 1))

for chunk in [int(v) for v in args.chunks.split(',')]:
    ch = chunk or F
    fusion.TSDFVolume(dims, args.voxel, w2g).integrate(filt[:min(F, 2 * ch)], kk[:min(F, 2 * ch)],
                                                       poses[:min(F, 2 * ch)], chunk=ch)
    times = []
    for rep in range(2):
        vol = fusion.TSDFVolume(dims, args.voxel, w2g)
        torch.cuda.synchronize()
        t, _ = ev_time(lambda: vol.integrate(filt, kk, poses, chunk=ch))
        times.append(t)
    t = min(times)
    key = 'integrate_chunk_%s' % (chunk or 'all')
    res[key + '_s'] = round(t, 4)
    res[key + '_s_runs'] = [round(v, 4) for v in times]
    res[key + '_gvisits_per_s'] = round(visits / t / 1e9, 2)

best = min((res['integrate_chunk_%s_s' % (c or 'all')], c) for c in [int(v) for v in args.chunks.split(',')])
res['integrate_best_chunk'] = best[1] or 'all'
t_best = best[0]
# traffic model: one 4-byte depth gather per visit; state (sdf f32 + weight u8 + free i32) read and written once
# per launch for every voxel the launches touch (upper bound: the whole volume per launch)
gather_bytes = 4.0 * visits
res['gather_GBps'] = round(gather_bytes / t_best / 1e9, 1)
res['gather_share_of_L2'] = round(gather_bytes / t_best / (L2_TBS * 1e12), 4)
res['gather_share_of_HBM'] = round(gather_bytes / t_best / (HBM_TBS * 1e12), 4)

vol = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(filt, kk, poses)
t_sp, (locs, vals) = host_time(lambda: vol.sparse())
t_sp2, _ = host_time(lambda: vol.sparse())
t_ss, sample = host_time(lambda: fusion.scan_sample(vol, 3.0, 4, 128))
t_ss2, sample = host_time(lambda: fusion.scan_sample(vol, 3.0, 4, 128))
res['sparse_export_s'] = round(min(t_sp, t_sp2), 4)
res['sparse_entries'] = int(len(vals))
res['scan_sample_s'] = round(min(t_ss, t_ss2), 4)
res['scan_input_rows'] = int(len(sample['input'][0]))


def end_to_end():
    m, k2 = fusion.raw_depth_to_metric(raw_d, 1000.0, (H, W), intrinsics=k_raw)
    v = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(fusion.bilateral(m), np.tile(k2, (F, 1)), poses)
    return fusion.scan_sample(v, 3.0, 4, 128)


host_time(end_to_end)
res['frames_to_model_input_s'] = round(min(host_time(end_to_end)[0], host_time(end_to_end)[0]), 4)
res['default_chunk'] = fusion.DEFAULT_CHUNK
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
