"""Mesh simplification cost at scene size, and what it saves downstream: the marching-cubes mesh of a configs[3]-sized
volume (128 x 512 x 512 voxels of 2 cm, z, y, x) built on the device, an analytic room (walls, floor, ceiling,
furniture boxes), is clustered at cells of 2, 4 and 8 voxels with both placements.

Timed, warm, with device events around the whole call and the median of --rounds rounds taken in turn, so that drift of
a shared machine hits every variant alike: the extraction (run_marching_cubes), every simplify.cluster variant, and for
the original and every 'quadric' result the two consumers a coarser mesh is for, meshdist.TriangleIndex build + 1 M
queries and render.render_depth of 16 frames of 240 x 320.  Face counts before and after go with the times.  Prints one
JSON line; --out also writes it.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import marching_cubes as mc, meshdist, render, simplify  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--cells', default='2,4,8', help='voxels')
ap.add_argument('--queries', type=int, default=1_000_000)
ap.add_argument('--frames', type=int, default=16)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
cells = [float(c) for c in args.cells.split(',')]
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
# the room: empty space is positive, walls are 2.5 voxels inside the volume
sdf = -box_sdf(z, y, x, (2.5, 5.0, 5.0), (Z - 3.5, Y - 6.0, X - 6.0)).expand(Z, Y, X).contiguous()
for _ in range(14):                                                        # furniture standing on the floor (z = 2.5)
    lo = (2.5, float(rng.uniform(15, Y - 90)), float(rng.uniform(15, X - 90)))
    hi = (lo[0] + float(rng.uniform(15, min(80, Z - 10))), lo[1] + float(rng.uniform(20, 70)), lo[2] + float(rng.uniform(20, 70)))
    sdf = torch.minimum(sdf, box_sdf(z, y, x, lo, hi))
sdf = sdf.clamp(-3.0, 3.0).contiguous()
torch.cuda.synchronize()


def extract():
    """The mesh in metres: marching cubes returns x, y, z in voxels."""
    v, _, f = mc.run_marching_cubes(sdf, None, 0.0, 3.0, 10.0)
    return v * args.voxel, f


verts, faces = extract()
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'queries': args.queries, 'frames': args.frames, 'rounds': args.rounds,
       'original': {'verts': int(verts.shape[0]), 'faces': int(faces.shape[0])}}

# queries: points near the surface; cameras: a ring in the middle of the room looking outwards and slightly down
points = verts[torch.randint(0, verts.shape[0], (args.queries,), device=dev, generator=torch.Generator(dev).manual_seed(0))]
points = points + 0.05 * torch.randn(points.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))
ang = np.linspace(0.0, 2.0 * np.pi, args.frames, endpoint=False)
centre = np.array([X / 2, Y / 2, Z / 2]) * args.voxel
eye = centre + np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.0 * ang], 1)
poses = render.look_at(eye, eye + np.stack([np.cos(ang), np.sin(ang), -0.2 + 0.0 * ang], 1))
K = np.tile(np.array([[290.0, 290.0, 159.5, 119.5]], np.float32), (args.frames, 1))
far = float(np.hypot(X, Y) * args.voxel)

meshes = {'original': (verts, faces)}
jobs = {'extract': extract}
for c in cells:
    for placement in ('quadric', 'mean'):
        name = 'cell%g_%s' % (c, placement)
        jobs['simplify_' + name] = (lambda c=c, p=placement: simplify.cluster(verts, faces, c * args.voxel, placement=p))
        out = jobs['simplify_' + name]()
        res[name] = {'cell_voxels': c, 'verts': int(out.verts.shape[0]), 'faces': int(out.faces.shape[0])}
        if placement == 'quadric':
            meshes[name] = (out.verts, out.faces)
for name, (v, f) in meshes.items():
    jobs['meshdist_' + name] = (lambda v=v, f=f: meshdist.TriangleIndex(v, f).distance(points))
    jobs['render_' + name] = (lambda v=v, f=f: render.render_depth(v, f, K, poses, (240, 320), depth_max=far))

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
    kind, _, mesh = n.partition('_')
    target = res.setdefault(mesh or 'original', {})
    target[kind + '_ms'] = round(statistics.median(runs), 3)
    target[kind + '_ms_runs'] = [round(t, 3) for t in runs]
for c in cells:
    for placement in ('quadric', 'mean'):
        r = res['cell%g_%s' % (c, placement)]
        r['simplify_over_extract'] = round(r['simplify_ms'] / res['original']['extract_ms'], 3)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
