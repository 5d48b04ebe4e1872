"""Connected-component labelling cost at scene size: the band |sdf| <= 1.5 voxels of a configs[3]-sized volume
(128 x 512 x 512 voxels, z, y, x) built on the device: an analytic room (walls, floor, ceiling, furniture boxes)
with a few hundred small detached spheres, the floaters a filter is there to remove.

label_volume runs with tiled=True (tile-local pass in LDS, then tile borders) and tiled=False (every pair merged in
global memory) at connectivity 6 and 26; label_mesh runs on the mesh that marching cubes extracts from the same
volume.  Every variant is warmed up, then all are timed in turn for --rounds rounds with device events around the
whole call (foreground, link, flatten, compaction, count read-back, relabel), so that drift of a shared machine hits
all of them alike; the best and all runs are reported.  The two routes' outputs are compared for equality.  If scipy
imports, the host leg (.cpu() + scipy.ndimage.label) is timed with a wall clock.  Prints one JSON line; --out also
writes it.
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
from sgnn_amd import components, marching_cubes as mc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--floaters', type=int, default=300)
ap.add_argument('--band', type=float, default=1.5, help='voxels')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default='')
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
# the room: empty space is positive, walls are 2.5 voxels inside the volume
sdf = -box_sdf(z, y, x, (2.5, 5.0, 5.0), (Z - 3.5, Y - 6.0, X - 6.0)).expand(Z, Y, X).contiguous()
for _ in range(14):                                                        # furniture standing on the floor (z = 2.5)
    lo = (2.5, float(rng.uniform(15, Y - 90)), float(rng.uniform(15, X - 90)))
    hi = (lo[0] + float(rng.uniform(15, min(80, Z - 10))), lo[1] + float(rng.uniform(20, 70)), lo[2] + float(rng.uniform(20, 70)))
    sdf = torch.minimum(sdf, box_sdf(z, y, x, lo, hi))
for _ in range(args.floaters):                                             # small spheres, stamped into their own boxes
    r = float(rng.uniform(0.8, 3.0))
    c = [float(rng.uniform(8, n - 9)) for n in (Z, Y, X)]
    sl = [slice(int(ci - r - 4), int(ci + r + 5)) for ci in c]
    d = torch.sqrt((z[sl[0]] - c[0]) ** 2 + (y[:, sl[1]] - c[1]) ** 2 + (x[:, :, sl[2]] - c[2]) ** 2) - r
    sdf[sl[0], sl[1], sl[2]] = torch.minimum(sdf[sl[0], sl[1], sl[2]], d)
sdf = sdf.clamp(-3.0, 3.0).contiguous()
torch.cuda.synchronize()

band = args.band
res = {'dims_zyx': [Z, Y, X], 'voxels': Z * Y * X, 'band_voxels': band, 'floaters': args.floaters,
       'tile_zyx': list(components.TILE_ZYX),
       'foreground_share': round(float(components.foreground(sdf, band).float().mean().item()), 5)}

verts, _, faces = mc.run_marching_cubes(sdf, None, 0.0, 3.0, 10.0)
res['mesh'] = {'verts': int(verts.shape[0]), 'faces': int(faces.shape[0])}

variants = [('volume_c%d_%s' % (c, 'tiled' if t else 'onelevel'), c, t) for c in (6, 26) for t in (True, False)]


def run(name):
    if name == 'mesh':
        return components.label_mesh(verts, faces)
    _, c, t = next(v for v in variants if v[0] == name)
    return components.label_volume(sdf, band=band, connectivity=c, tiled=t)


names = [v[0] for v in variants] + ['mesh']
outs = {}
for name in names:                                                         # warm-up and the outputs to compare
    outs[name] = run(name)
    run(name)
torch.cuda.synchronize()
for c in (6, 26):
    a, b = outs['volume_c%d_tiled' % c], outs['volume_c%d_onelevel' % c]
    res['c%d' % c] = {'components': int(a.sizes.shape[0]), 'largest': int(a.sizes.max().item()),
                      'routes_equal': bool(torch.equal(a.labels, b.labels) and torch.equal(a.sizes, b.sizes))}
res['mesh'].update(components=int(outs['mesh'].face_sizes.shape[0]), largest_faces=int(outs['mesh'].face_sizes.max().item()))

times = {n: [] for n in names}
for _ in range(args.rounds):
    for n in names:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run(n)
        e.record()
        torch.cuda.synchronize()
        times[n].append(s.elapsed_time(e))
for n in names:
    target = res['mesh'] if n == 'mesh' else res.setdefault(n, {})
    target['ms_runs'] = [round(t, 3) for t in times[n]]
    target['ms'] = round(min(times[n]), 3)
for c in (6, 26):
    res['c%d' % c]['tiled_over_onelevel'] = round(res['volume_c%d_tiled' % c]['ms'] / res['volume_c%d_onelevel' % c]['ms'], 3)
res['tiled_beats_onelevel'] = bool(all(res['c%d' % c]['tiled_over_onelevel'] < 1.0 for c in (6, 26)))

try:
    from scipy import ndimage
except ImportError:
    res['host_scipy'] = None
else:
    res['host_scipy'] = {}
    for c, structure in ((6, 1), (26, 3)):
        runs = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fg = components.foreground(sdf, band).cpu().numpy()
            _, count = ndimage.label(fg, ndimage.generate_binary_structure(3, structure))
            runs.append(time.perf_counter() - t0)
        res['host_scipy']['c%d' % c] = {'ms_runs': [round(t * 1e3, 1) for t in runs], 'ms': round(min(runs) * 1e3, 1),
                                        'components': int(count),
                                        'same_count': bool(count == res['c%d' % c]['components'])}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
