"""Mesh fairing cost at scene size: the marching-cubes mesh of a configs[3]-sized volume (128 x 512 x 512 voxels of
2 cm, z, y, x), the analytic room of scripts/bench_simplify.py (walls, floor, ceiling, furniture boxes), about 1.7 M
faces, is smoothed by every entrance of sgnn_amd.smooth.

Timed, warm, with device events around the public calls, the median of --rounds rounds taken in turn with the minimum
and the maximum: the Adjacency build; taubin(10) on 12-byte rows and on rows padded to 16 bytes (per call and per
half-step), and the same 20 step launches replayed from a captured graph, which leaves out the host's cost per launch;
vertex_normals; denoise(); a copy of the vertex bytes; and the plain-torch route to the umbrella step, a
torch.sparse CSR matrix of 1 / deg times the vertex array, lambda and mu as two products, 10 iterations (it treats
every vertex as an interior one: no kinds, no rim rule).  The registers and the scratch bytes of the step kernels come
from the compiler's resource remarks on csrc/smooth.hip.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import _lib, marching_cubes as mc, smooth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smooth_bench.json'))
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')
rng = np.random.default_rng(0)


def box_sdf(z, y, x, lo, hi):
    """Signed distance (voxels) to an axis-aligned box, negative inside."""
    c = [(a + b) / 2 for a, b in zip(lo, hi)]
    h = [(b - a) / 2 for a, b in zip(lo, hi)]
    q = [(g - ci).abs() - hi_ for g, ci, hi_ in zip((z, y, x), c, h)]
    outside = torch.sqrt(sum(v.clamp(min=0) ** 2 for v in q))
    return outside + torch.maximum(torch.maximum(q[0], q[1]), q[2]).clamp(max=0)


z = torch.arange(Z, dtype=torch.float32, device=dev).view(Z, 1, 1)
y = torch.arange(Y, dtype=torch.float32, device=dev).view(1, Y, 1)
x = torch.arange(X, dtype=torch.float32, device=dev).view(1, 1, X)
sdf = -box_sdf(z, y, x, (2.5, 5.0, 5.0), (Z - 3.5, Y - 6.0, X - 6.0)).expand(Z, Y, X).contiguous()
for _ in range(14):
    lo = (2.5, float(rng.uniform(15, Y - 90)), float(rng.uniform(15, X - 90)))
    hi = (lo[0] + float(rng.uniform(15, min(80, Z - 10))), lo[1] + float(rng.uniform(20, 70)), lo[2] + float(rng.uniform(20, 70)))
    sdf = torch.minimum(sdf, box_sdf(z, y, x, lo, hi))
sdf = sdf.clamp(-3.0, 3.0).contiguous()
verts, _, faces = mc.run_marching_cubes(sdf, None, 0.0, 3.0, 10.0)
verts = (verts * args.voxel).contiguous()
del sdf
nv, nt = int(verts.shape[0]), int(faces.shape[0])

adj = smooth.Adjacency(faces, nv)
kinds = torch.bincount(adj.kind.long(), minlength=4).tolist()
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'rounds': args.rounds, 'verts': nv, 'faces': nt,
       'directed_edges': int(adj.neighbor.shape[0]),
       'kinds': dict(zip(('isolated', 'interior', 'boundary', 'nonmanifold'), kinds))}

# the plain-torch route: row i of A holds 1 / deg(i) at its neighbours
deg = adj.start[1:] - adj.start[:-1]
A = torch.sparse_csr_tensor(adj.start, adj.neighbor.long(), (1.0 / deg.clamp(min=1).float()).repeat_interleave(deg),
                            size=(nv, nv))


def torch_taubin(iterations=10, lam=0.5, mu=-0.53):
    p = verts
    for _ in range(iterations):
        for f in (lam, mu):
            p = p + f * (A @ p - p)
    return p


def padded(rows):
    def job():
        smooth.ROW_FLOATS = rows
        try:
            return smooth.taubin(verts, adj, 10)
        finally:
            smooth.ROW_FLOATS = 3
    return job


def graph_steps(rows):
    """The 20 step launches of taubin(10) captured once and replayed: the kernels without the host's cost per launch."""
    src = torch.zeros((nv, rows), dtype=torch.float32, device=dev)
    src[:, :3] = verts
    bufs = [torch.empty_like(src), torch.empty_like(src)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cur = src
        for k in range(20):
            _lib.call('sgnn_smooth_step', _lib.ptr(cur), _lib.ptr(bufs[k & 1]), nv, rows, *adj._ptrs(), None, 1,
                      -0.53 if k & 1 else 0.5, None)
            cur = bufs[k & 1]
    graph.keep = (src, bufs)
    return graph


jobs = {'adjacency': lambda: smooth.Adjacency(faces, nv),
        'taubin10_rows12': padded(3),
        'taubin10_rows16': padded(4),
        'vertex_normals': lambda: smooth.vertex_normals(verts, faces),
        'denoise': lambda: smooth.denoise(verts, faces, adj=adj),
        'copy': lambda: verts.clone(),
        'torch_sparse_taubin10': torch_taubin}
assert torch.equal(jobs['taubin10_rows12']().view(torch.int32), jobs['taubin10_rows16']().view(torch.int32))
try:
    worst = float((torch_taubin() - smooth.taubin(verts, adj, 10, boundary='free'))[adj.kind == smooth.INTERIOR].abs().max())
    res['torch_route_max_abs_difference_m'] = worst       # interior vertices far from a rim agree up to rounding
except RuntimeError as e:
    res['torch_sparse_taubin10_error'] = str(e).splitlines()[0]
    del jobs['torch_sparse_taubin10']

try:
    for rows in (3, 4):
        jobs['graph_steps20_rows%d' % (4 * rows)] = graph_steps(rows).replay
except RuntimeError as e:
    res['graph_steps20_error'] = str(e).splitlines()[0]
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
    res[n] = {'ms': round(statistics.median(runs), 4), 'ms_min': round(min(runs), 4), 'ms_max': round(max(runs), 4)}
for n in [n for n in res if n.startswith(('taubin10_rows', 'graph_steps20_rows'))]:
    res[n]['half_step_ms'] = round(res[n]['ms'] / 20.0, 4)
    res[n]['half_step_over_copy'] = round(res[n]['half_step_ms'] / res['copy']['ms'], 2)
if 'torch_sparse_taubin10' in res:
    res['torch_sparse_over_taubin10'] = round(res['torch_sparse_taubin10']['ms'] / res['taubin10_rows12']['ms'], 2)
if 'graph_steps20_rows16' in res:
    res['graph_rows16_over_rows12'] = round(res['graph_steps20_rows16']['ms'] / res['graph_steps20_rows12']['ms'], 3)
res['rows16_over_rows12'] = round(res['taubin10_rows16']['ms'] / res['taubin10_rows12']['ms'], 3)

# registers and scratch of the step kernels, from the compiler (nothing is run)
try:
    csrc = os.path.join(ROOT, 'sgnn_amd', 'csrc')
    text = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '-std=c++17', '--offload-arch=gfx950',
                           '-ffp-contract=off', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
                           'smooth.hip', '-o', os.devnull], cwd=csrc, capture_output=True, text=True, timeout=300).stderr
    usage = {}
    for name, body in re.findall(r'Function Name: (\S+)(.*?)(?=Function Name:|\Z)', text, flags=re.S):
        m = re.search(r'k_smooth_stepILi(\d)E', name)
        if m:
            usage['rows%d' % (4 * int(m.group(1)))] = {
                'vgprs': int(re.search(r' VGPRs: (\d+)', body).group(1)),
                'scratch_bytes_per_lane': int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', body).group(1)),
                'waves_per_simd': int(re.search(r'Occupancy \[waves/SIMD\]: (\d+)', body).group(1))}
    res['step_kernel'] = usage or 'unmeasured'
except (OSError, subprocess.SubprocessError, AttributeError) as e:
    res['step_kernel'] = 'unmeasured: %s' % e

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
