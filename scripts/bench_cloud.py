"""Point-cloud neighbourhood cost at scene size: register.surface_points of the 128 x 512 x 512 volume (z, y, x, 2 cm)
of synth.make_scene, about 371 k points on surfaces, goes through every entrance of sgnn_amd.cloud.

Timed, warm, with device events around the public calls, the median of --rounds rounds taken in turn with the minimum
and the maximum: the PointIndex build; knn(None, 16) and knn(None, 1) on a built index; normals(k=16) and
statistical_outliers(k=16) on a built index (each includes its knn); voxel_downsample at 2 voxels; compare against a
copy shifted by half a voxel (two index builds and two nearest passes).  Comparison legs in the same run: torch.cdist
plus topk(16) in query chunks that fit memory, over all points; a device copy of the point bytes; and
scipy.spatial.cKDTree on the host (build and a 16-neighbour query, wall clock) where scipy can be imported.  The
registers and scratch bytes of the kNN instantiations come from the compiler's resource remarks on csrc/cloud.hip.
Only the lane-per-query kernel exists; the workgroup-per-cell kernel staging cells in LDS
is not built, so there is no second shape to time.  No time is a pass / fail criterion.  Prints one JSON line; --out
also writes it.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import cloud, fusion, register, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--chunk', type=int, default=4096, help='queries per torch.cdist call')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cloud_bench.json'))
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')

locs, feats = synth.make_scene((Z, Y, X))
w2g = np.eye(4, dtype=np.float32)
w2g[:3, :3] /= np.float32(args.voxel)
vol = fusion.TSDFVolume((X, Y, Z), args.voxel, w2g)
locs = locs.to(dev)
vol._sdf[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0] * args.voxel
pts = register.surface_points(vol).contiguous()
del vol, locs, feats
n = int(pts.shape[0])
shifted = (pts + torch.tensor([0.5 * args.voxel, 0.0, 0.0], device=dev)).contiguous()
index = cloud.PointIndex(pts)
occupied = int((index.start[1:] > index.start[:-1]).sum())
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'rounds': args.rounds, 'points': n, 'cell_m': float(index.cell),
       'grid': list(index.dims), 'occupied_cells': occupied, 'points_per_occupied_cell': round(n / max(occupied, 1), 2)}


def cdist_topk(k=16):
    out = []
    for q0 in range(0, n, args.chunk):
        d = torch.cdist(pts[q0:q0 + args.chunk], pts)
        out.append(torch.topk(d, k + 1, dim=1, largest=False).indices[:, 1:])
    return torch.cat(out)


jobs = {'index_build': lambda: cloud.PointIndex(pts),
        'knn16': lambda: index.knn(None, 16),
        'knn1': lambda: index.knn(None, 1),
        'normals16': lambda: cloud.normals(pts, k=16, index=index),
        'statistical_outliers16': lambda: cloud.statistical_outliers(pts, k=16, index=index),
        'voxel_downsample_2vox': lambda: cloud.voxel_downsample(pts, 2 * args.voxel),
        'compare_shifted': lambda: cloud.compare(pts, shifted, thresholds=(args.voxel,)),
        'copy': lambda: pts.clone(),
        'torch_cdist_topk16': cdist_topk}
try:      # the two routes name the same neighbours wherever distances are not tied
    a, b = index.knn(None, 16)[0][:args.chunk].long().sort(1).values, cdist_topk()[:args.chunk].sort(1).values
    res['torch_route_rows_equal_share'] = round(float((a == b).all(1).float().mean()), 4)
except RuntimeError as e:
    res['torch_cdist_topk16_error'] = str(e).splitlines()[0]
    del jobs['torch_cdist_topk16']
res['thinned_points'] = int(cloud.voxel_downsample(pts, 2 * args.voxel).points.shape[0])
for job in jobs.values():                                                  # warm-up of every shape that is timed
    job()
torch.cuda.synchronize()
times = {name: [] for name in jobs}
for _ in range(args.rounds):
    for name, job in jobs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        job()
        e.record()
        torch.cuda.synchronize()
        times[name].append(s.elapsed_time(e))
for name, runs in times.items():
    res[name] = {'ms': round(statistics.median(runs), 4), 'ms_min': round(min(runs), 4), 'ms_max': round(max(runs), 4)}
res['knn16_over_copy'] = round(res['knn16']['ms'] / res['copy']['ms'], 1)
if 'torch_cdist_topk16' in res:
    res['torch_cdist_topk16_over_knn16'] = round(res['torch_cdist_topk16']['ms'] / res['knn16']['ms'], 1)
res['kernel_shape_b'] = 'not built: unmeasured'

try:
    from scipy.spatial import cKDTree
    host = pts.cpu().numpy()
    runs = {'build': [], 'query16': []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        tree = cKDTree(host)
        t1 = time.perf_counter()
        tree.query(host, k=17, workers=16)
        t2 = time.perf_counter()
        runs['build'].append((t1 - t0) * 1e3)
        runs['query16'].append((t2 - t1) * 1e3)
    res['scipy_ckdtree_host'] = {name: {'ms': round(statistics.median(r), 2), 'ms_min': round(min(r), 2),
                                        'ms_max': round(max(r), 2)} for name, r in runs.items()}
    res['scipy_ckdtree_host']['workers'] = 16
except ImportError:
    res['scipy_ckdtree_host'] = 'skipped: scipy is not installed'

# registers and scratch of the kNN kernels, from the compiler (nothing is run)
try:
    csrc = os.path.join(ROOT, 'sgnn_amd', 'csrc')
    text = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '-std=c++17', '--offload-arch=gfx950',
                           '-ffp-contract=off', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
                           'cloud.hip', '-o', os.devnull], cwd=csrc, capture_output=True, text=True, timeout=300).stderr
    usage = {}
    for name, body in re.findall(r'Function Name: (\S+)(.*?)(?=Function Name:|\Z)', text, flags=re.S):
        m = re.search(r'k_cloud_knnILi(\d+)ELb(\d)E', name)
        if m:
            usage['K%s_%s' % (m.group(1), 'self' if m.group(2) == '1' else 'queries')] = {
                'vgprs': int(re.search(r' VGPRs: (\d+)', body).group(1)),
                'scratch_bytes_per_lane': int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', body).group(1)),
                'waves_per_simd': int(re.search(r'Occupancy \[waves/SIMD\]: (\d+)', body).group(1))}
    res['knn_kernel'] = usage or 'unmeasured'
except (OSError, subprocess.SubprocessError, AttributeError) as e:
    res['knn_kernel'] = 'unmeasured: %s' % e

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
