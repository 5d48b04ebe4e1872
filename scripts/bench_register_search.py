"""register.search at scene size: the 128 x 512 x 512 volume (z, y, x, 2 cm) of synth.make_scene against a moved copy of
its own register.surface_points (a turn about the vertical and a shift that align alone cannot undo).

Legs, each a child process under its own `timeout -k 10` (a leg that faults or hangs ends there and the legs after it
are not started): `field` (register.distance_field), `level0` (the one level-0 score launch: B, P, ms, lookups/s),
`level` (one refinement level: top x 81 records), `search` (the whole ladder with align, wall clock) and `copy` (a device
copy of the dist2 bytes, the floor of anything that reads the field once).  Warm, median of --rounds with min - max from
device events.  No time is a pass / fail criterion.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = (('field', 120), ('level0', 300), ('level', 120), ('search', 420), ('copy', 60))

ap = argparse.ArgumentParser()
ap.add_argument('--dims', default='128,512,512', help='z,y,x voxels')
ap.add_argument('--voxel', type=float, default=0.02, help='metres')
ap.add_argument('--yaw-step', type=float, default=30.0, help='degrees')
ap.add_argument('--step', type=float, default=0.16, help='level-0 pitch, metres')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--leg', default='', help='internal: run one leg in this process')
ap.add_argument('--out', default='')
args = ap.parse_args()


def parent():
    os.environ.setdefault('OMP_NUM_THREADS', '16')                          # at most 16 worker threads
    res = {'dims_zyx': [int(v) for v in args.dims.split(',')], 'voxel_m': args.voxel, 'rounds': args.rounds,
           'yaw_step_deg': args.yaw_step, 'pitch_m': args.step}
    for leg, limit in LEGS:
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', leg, '--dims', args.dims,
               '--voxel', str(args.voxel), '--yaw-step', str(args.yaw_step), '--step', str(args.step), '--rounds',
               str(args.rounds)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if run.returncode != 0:
            res[leg + '_failed_rc'] = run.returncode
            break                                                           # nothing more on a device that may have faulted
        res.update(json.loads(run.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 0 if not any(k.endswith('_failed_rc') for k in res) else 1


def child(leg):
    import numpy as np
    import torch
    from sgnn_amd import fusion, register, synth
    torch.set_num_threads(16)
    Z, Y, X = (int(v) for v in args.dims.split(','))
    dev = torch.device('cuda')
    locs, feats = synth.make_scene((Z, Y, X))
    w2g = np.eye(4, dtype=np.float32)
    w2g[:3, :3] /= np.float32(args.voxel)
    vol = fusion.TSDFVolume((X, Y, Z), args.voxel, w2g)
    locs = locs.to(dev)
    vol._sdf[locs[:, 0], locs[:, 1], locs[:, 2]] = feats.to(dev)[:, 0] * args.voxel
    a = np.radians(70.0)
    true = np.eye(4)
    true[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    true[:3, 3] = [1.3, -0.9, 0.1]
    inv = torch.from_numpy(np.linalg.inv(true)).to(dev)
    dst = register.surface_points(vol, stride=4).double()
    pts = (dst @ inv[:3, :3].T + inv[:3, 3]).float().contiguous()
    settings = dict(yaw_step=args.yaw_step, step=args.step)
    res = {}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.rounds):
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            runs.append(s.elapsed_time(e))
        return round(statistics.median(runs), 4), [round(min(runs), 4), round(max(runs), 4)]

    if leg == 'field':
        res['field_ms'], res['field_ms_min_max'] = timed(lambda: register.distance_field(vol))
    else:
        field = register.distance_field(vol)
    if leg == 'copy':
        other = torch.empty_like(field.dist2)
        res['dist2_bytes'] = field.dist2.numel() * 4
        res['copy_dist2_ms'], res['copy_dist2_ms_min_max'] = timed(lambda: other.copy_(field.dist2))
    if leg in ('level0', 'level'):
        trace = {}
        register.search(pts, vol, field=field, trace=trace, levels=1, iterations=1, **settings)
        sub = pts[::-(-int(pts.shape[0]) // 4096)].contiguous()
        if leg == 'level0':
            origin, (nx, ny, nz), pitch = trace['lattice']
            nb = int(trace['level0'].shape[0])
            i = np.arange(nb)
            c = sub.double().mean(0).cpu().numpy()
            nr = nb // (nx * ny * nz)
            rots = np.stack([register._rotation((0.0, 0.0, 1.0), np.radians(k * args.yaw_step)) for k in range(nr)])
            k = np.stack([i % nx, (i // nx) % ny, (i // (nx * ny)) % nz], 1).astype(np.float64)
            table = register.pose_table(field.world2grid, register._poses(rots[i // (nx * ny * nz)], origin + k * pitch, c))
        else:
            guesses = np.repeat(trace['guesses'], 81, axis=0)               # top x 81 records, the size of a level
            table = register.pose_table(field.world2grid, guesses)
            nb = int(table.shape[0])
        ms, span = timed(lambda: register._score_table(sub, field, table, 1))
        res.update({leg + '_B': nb, leg + '_P': int(sub.shape[0]), leg + '_ms': ms, leg + '_ms_min_max': span,
                    leg + '_lookups_per_s': round(nb * int(sub.shape[0]) / (ms * 1e-3), 1)})
    if leg == 'search':
        register.search(pts, vol, field=field, **settings)
        runs = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = register.search(pts, vol, field=field, **settings)
            torch.cuda.synchronize()
            runs.append(1e3 * (time.perf_counter() - t0))
        rel = out.T @ np.linalg.inv(true)
        res.update({'search_ok': bool(out.ok), 'search_wall_ms': round(statistics.median(runs), 2),
                    'search_wall_ms_min_max': [round(min(runs), 2), round(max(runs), 2)],
                    'search_points': int(pts.shape[0]),
                    'search_shift_error_m': round(float(np.linalg.norm(rel[:3, 3])), 6)})
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(child(args.leg) if args.leg else parent())
