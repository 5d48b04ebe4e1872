"""What colour costs in rendering and ray casting, on the setups of scripts/bench_render.py and scripts/bench_raycast.py:
the tessellated room (walls and 14 furniture boxes, about 500 k triangles) rendered to 1000 frames of 240 x 320, those
frames fused into 512 x 512 x 128 voxels at 2 cm, and the volume cast back at every tenth pose (100 frames).

Four timings, warm, from device events, the median of 5 with min and max: render_depth, render_color, cast and
cast_color (the whole call each: clear, triangles and finish; brick pass, table upload and cast).  The four are timed
in turn, round by round, so that drift of a shared machine hits all of them alike.  With --parent-lib PATH (a
libsgnn_hip.so built from the parent commit) a fresh process times the two depth-only calls with that library on the
same scene, to show whether the depth-only paths have moved; --variant-lib NAME=PATH times all four with another build
of this commit (the recorded one, hint_load: render.hip with a plain load of a key's z word in front of the colour
arithmetic and the atomic, skipping fragments behind what it returns).
Prints one JSON line; --out also writes it (profiles/render_color_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--cast-every', type=int, default=10, help='cast at every n-th pose')
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--tess', type=int, default=53, help='quads per box edge: 15 boxes x 12 n^2 triangles')
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--parent-lib', default='', help='libsgnn_hip.so of the parent commit')
ap.add_argument('--variant-lib', default='', help='NAME=PATH of another build of this commit')
ap.add_argument('--out', default='')
ap.add_argument('--child', default='', help='(internal) depth: time the depth-only calls; all: all four; print JSON')
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))
ext = np.array(dims) * args.voxel
H, W = 240, 320
F = args.frames

from sgnn_amd import fusion, raycast, render  # noqa: E402  (whatever library SGNN_LIB names)

# the scene of scripts/bench_render.py
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
verts = torch.from_numpy(np.concatenate([p for p, _ in parts]).astype(np.float32)).to(dev)
faces = torch.from_numpy(np.concatenate([t for _, t in parts]).astype(np.int32)).to(dev)
vcol = (verts * torch.tensor([23.0, 23.0, 90.0], device=dev) + 10.0).clamp(0, 255).round().to(torch.uint8)   # a smooth colour
K = np.tile(np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], np.float32), (F, 1))
c = ext / 2
a = 2 * np.pi * 2 * np.arange(F) / F                                          # two loops
r = 0.3 * min(ext[0], ext[1]) * (1 + 0.3 * np.sin(5 * a))
eyes = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), np.full(F, min(1.5, ext[2] * 0.6))], 1)
poses = render.look_at(eyes, eyes + np.stack([np.cos(a + 1.2), np.sin(a + 1.2), np.full(F, -0.35)], 1))
w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
Kc, pc = K[::args.cast_every], poses[::args.cast_every]


def stats(times):
    return {'median_s': round(float(np.median(times)), 6), 'min_s': round(min(times), 6), 'max_s': round(max(times), 6),
            'runs_s': [round(t, 6) for t in times]}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 1e3, out


def measure(color):
    """The calls of this library on the scene: {name: stats}, and the outputs of the last round."""
    calls = {'render_depth': lambda: render.render_depth(verts, faces, K, poses, (H, W))}
    if color:
        calls['render_color'] = lambda: render.render_color(verts, faces, vcol, K, poses, (H, W))
        depth, rgba = calls['render_color']()
        vol = fusion.TSDFVolume(dims, args.voxel, w2g, color=True).integrate(depth, K, poses, color=rgba)
        alpha = (vol.color_weight() > 0).to(torch.uint8) * 255
        colors = torch.cat([vol.colors(), alpha[..., None]], 3).contiguous()
        del rgba, alpha
    else:
        depth = calls['render_depth']()
        vol = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(depth, K, poses)
    del depth
    sdf, band = vol.sdf(), np.float32(3.0) * vol.voxel_size
    calls['cast'] = lambda: raycast.cast(sdf, w2g, args.voxel, Kc, pc, (H, W), band)
    if color:
        calls['cast_color'] = lambda: raycast.cast_color(sdf, colors, w2g, args.voxel, Kc, pc, (H, W), band)
    times, outs = {n: [] for n in calls}, {}
    for rep in range(args.runs + 1):                                           # round 0 is the warm-up
        for n, fn in calls.items():
            t, outs[n] = timed(fn)
            if rep:
                times[n].append(t)
    return {n: stats(t) for n, t in times.items()}, outs


if args.child:
    print(json.dumps(measure(args.child == 'all')[0]))
    sys.exit(0)


def child(lib, mode):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--frames', str(F), '--cast-every',
           str(args.cast_every), '--dims', args.dims, '--voxel', str(args.voxel), '--tess', str(args.tess), '--runs',
           str(args.runs)]
    out = subprocess.run(cmd, env=dict(os.environ, SGNN_LIB=os.path.abspath(lib)), check=True, stdout=subprocess.PIPE,
                         timeout=600).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


res = {'frames': F, 'cast_frames': len(pc), 'frame_hw': [H, W], 'dims_xyz': list(dims), 'voxel_size': args.voxel,
       'triangles': int(faces.shape[0]), 'runs': args.runs}
timings, outs = measure(True)
res.update(timings)
bits = lambda t: t.view(torch.int32)  # noqa: E731
res['same_depth'] = bool(torch.equal(bits(outs['render_color'][0]), bits(outs['render_depth'])) and
                         torch.equal(bits(outs['cast_color'][0]), bits(outs['cast'])))
res['rendered_share'] = round(float((outs['render_color'][1][..., 3] == 255).float().mean().item()), 4)
res['cast_coloured_share'] = round(float((outs['cast_color'][1][..., 3] == 255).float().mean().item()), 4)
cnt = torch.zeros(3, dtype=torch.int64, device=dev)
render.render_color(verts, faces, vcol, K, poses, (H, W), counters=cnt)
res['covered_pixels'] = int(cnt[2])
res['overdraw'] = round(int(cnt[2]) / (F * H * W), 3)
del outs
res['render_color_over_render_depth'] = round(res['render_color']['median_s'] / res['render_depth']['median_s'], 4)
res['cast_color_over_cast'] = round(res['cast_color']['median_s'] / res['cast']['median_s'], 4)
res['parent'] = None                                                         # not measured without --parent-lib
if args.parent_lib:
    res['parent'] = child(args.parent_lib, 'depth')
    for n in ('render_depth', 'cast'):
        res['%s_over_parent' % n] = round(res[n]['median_s'] / res['parent'][n]['median_s'], 4)
if args.variant_lib:
    tag, _, path = args.variant_lib.partition('=')
    res['variant'] = {'name': tag, **child(path, 'all')}
    res['render_color_over_variant'] = round(res['render_color']['median_s'] / res['variant']['render_color']['median_s'], 4)
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
