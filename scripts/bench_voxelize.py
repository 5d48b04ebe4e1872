"""Mesh voxelisation cost at scene size, against the two existing routes from a mesh to a volume.

The mesh is the marching-cubes surface of synth.make_scene (128 x 512 x 512 voxels, z, y, x), in voxel units; it is
voxelised at band 3 by voxelize.signed_distance.  Leg (a) is the existing route to the same unsigned distances:
meshdist.TriangleIndex.distance on every voxel centre with max_dist = band (index build timed apart).  Leg (b) is the
route to a projective, view-dependent volume: render.render_depth of --poses frames of 240 x 320 from a ring of cameras
plus TSDFVolume.integrate.

Timed warm, with device events around the whole call and the median of --rounds rounds taken in turn.  Prints one JSON
line; --out also writes it.
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
from sgnn_amd import fusion, marching_cubes as mc, meshdist, render, synth, voxelize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--band', type=float, default=3.0)
ap.add_argument('--poses', type=int, default=100)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
Z, Y, X = (int(v) for v in args.dims.split(','))
dev = torch.device('cuda')

locs, feats = synth.make_scene((Z, Y, X))
dense = torch.full((Z, Y, X), -float('inf'), dtype=torch.float32, device=dev)
locs = locs.to(dev)
dense[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0]
verts, _, faces = mc.run_marching_cubes(dense, None, 0.0, 3.0, 10.0)         # x, y, z in voxels
del dense
dims = (X, Y, Z)
z, y, x = torch.meshgrid(torch.arange(Z, device=dev), torch.arange(Y, device=dev), torch.arange(X, device=dev), indexing='ij')
centres = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).float()
del x, y, z

# leg (b): cameras on a ring in the middle of the volume, looking outwards and slightly down, in metres
world = verts * args.voxel
w2g = np.eye(4, dtype=np.float32)
w2g[:3, :3] /= np.float32(args.voxel)
ang = np.linspace(0.0, 2.0 * np.pi, args.poses, endpoint=False)
centre = np.array([X / 2, Y / 2, Z / 2]) * args.voxel
eye = centre + np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.0 * ang], 1)
poses = render.look_at(eye, eye + np.stack([np.cos(ang), np.sin(ang), -0.2 + 0.0 * ang], 1))
K = np.tile(np.array([[290.0, 290.0, 159.5, 119.5]], np.float32), (args.poses, 1))
far = float(np.hypot(X, Y) * args.voxel)

index = meshdist.TriangleIndex(verts, faces)


def render_and_fuse():
    depth = render.render_depth(world, faces, K, poses, (240, 320), depth_max=far)
    return fusion.TSDFVolume(dims, args.voxel, w2g, depth_max=far).integrate(depth, K, poses)


jobs = {
    'voxelize': lambda: voxelize.signed_distance(verts, faces, dims, args.band),
    'mesh_to_volume': lambda: voxelize.mesh_to_volume(world, faces, dims, args.voxel, w2g, band=args.band),
    'index_build': lambda: meshdist.TriangleIndex(verts, faces),
    'index_distance': lambda: index.distance(centres, max_dist=args.band),
    'render_and_fuse': render_and_fuse,
}
res = {'dims_zyx': [Z, Y, X], 'voxel_m': args.voxel, 'band': args.band, 'poses': args.poses, 'rounds': args.rounds,
       'verts': int(verts.shape[0]), 'faces': int(faces.shape[0])}
out = jobs['voxelize']()
d, f = jobs['index_distance']()
res['in_band_voxels'] = int((out.face >= 0).sum())
res['equal_to_index'] = bool(torch.equal(out.dist.abs().reshape(-1), d) and torch.equal(out.face.reshape(-1), f))
del out, d, f
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
    res[n + '_ms'] = round(statistics.median(runs), 3)
    res[n + '_ms_runs'] = [round(t, 3) for t in runs]
res['index_distance_over_voxelize'] = round(res['index_distance_ms'] / res['voxelize_ms'], 3)
res['index_total_over_voxelize'] = round((res['index_build_ms'] + res['index_distance_ms']) / res['voxelize_ms'], 3)
res['render_and_fuse_over_mesh_to_volume'] = round(res['render_and_fuse_ms'] / res['mesh_to_volume_ms'], 3)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
