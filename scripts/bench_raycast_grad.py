"""Cost of the differentiable cast at scene size: the volume and the 100 poses of scripts/bench_raycast.py (512 x 512 x
128 voxels at 2 cm fused from rendered 240 x 320 frames of an analytic room), cast_diff forward + backward with a
depth loss and with a 3-channel feature loss, against raycast.cast alone in the same run.

Each GPU step (one variant: warm-up, then --rounds timed runs with device events) runs in a child process of its own
under its own time limit; the parent renders the frames once on the host, hands them over in a temporary .npz, and
collects the children's JSON lines.  `floor_ms` is the backward's atomic traffic (4 bytes per add: 16 adds per hit
pixel into grad_sdf, 8 per channel into grad_features) over the chip-wide rate of global float atomics, 1.3 TB/s of
added bytes.  No time is a pass/fail criterion.  Prints one JSON line; --out also writes it
(profiles/raycast_grad_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fusion_ref as R  # noqa: E402

ATOMIC_BYTES_PER_S = 1.3e12
H, W = 240, 320
VARIANTS = ('cast', 'diff_depth', 'diff_depth_features')

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=100)
ap.add_argument('--dims', default='512,512,128', help='x,y,z voxels')
ap.add_argument('--voxel', type=float, default=0.02)
ap.add_argument('--step', type=float, default=0.5)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--limit', type=float, default=240.0, help='seconds per child process')
ap.add_argument('--out', default='')
ap.add_argument('--child', default='', help=argparse.SUPPRESS)
ap.add_argument('--scene', default='', help=argparse.SUPPRESS)
args = ap.parse_args()
dims = tuple(int(v) for v in args.dims.split(','))


def scene():
    """bench_raycast.py's room, trajectory and intrinsics -> (K, poses, planes, boxes)."""
    ext = np.array(dims) * args.voxel
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
    return K, np.stack(poses), planes, boxes


K, poses, planes, boxes = scene()


def _render(p):
    return R.render(K, p, (H, W), planes, boxes)


def child(variant):
    import torch
    from sgnn_amd import fusion, raycast
    depth_in = np.load(args.scene)['depth']
    w2g = R.grid_transform((0.0, 0.0, 0.0), args.voxel)
    kk = np.tile(K, (args.frames, 1))
    vol = fusion.TSDFVolume(dims, args.voxel, w2g).integrate(depth_in, kk, poses)
    sdf = vol.sdf()
    band = np.float32(3.0) * vol.voxel_size
    target = torch.from_numpy(depth_in).cuda()
    res = {'variant': variant}
    channels = 3 if variant == 'diff_depth_features' else 0
    fe = None
    if channels:
        fe = torch.rand(tuple(sdf.shape) + (channels,), device='cuda').requires_grad_()
        colour = torch.rand((args.frames, H, W, channels), device='cuda')
    leaf = sdf.clone().requires_grad_()

    def run():
        if variant == 'cast':
            return raycast.cast(sdf, w2g, args.voxel, kk, poses, (H, W), band, step=args.step)
        depth, feat, ok = raycast.cast_diff(leaf, w2g, args.voxel, kk, poses, (H, W), band, features=fe, step=args.step)
        m = ok & torch.isfinite(target)
        loss = ((torch.where(m, depth - target, torch.zeros_like(depth))) ** 2).sum()
        if channels:
            loss = loss + (((feat - colour) * m[..., None]) ** 2).sum()
        grads = torch.autograd.grad(loss, (leaf, fe) if channels else (leaf,))
        res['hit_pixels'] = int(torch.isfinite(depth).sum().item())
        return grads

    run()
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    res['ms_runs'] = [round(t, 3) for t in times]
    res['ms'] = round(float(np.median(times)), 3)
    if variant != 'cast':
        nbytes = 4 * res['hit_pixels'] * (16 + 8 * channels)
        res['atomic_bytes'] = nbytes
        res['floor_ms'] = round(nbytes / ATOMIC_BYTES_PER_S * 1e3, 4)
    print(json.dumps(res))


if args.child:
    child(args.child)
    sys.exit(0)

t0 = time.perf_counter()
import multiprocessing  # noqa: E402
with multiprocessing.get_context('fork').Pool(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
    depth = np.stack(pool.map(_render, list(poses), chunksize=4))
out = {'frames': args.frames, 'dims_xyz': list(dims), 'voxel_size': args.voxel, 'frame_hw': [H, W], 'step': args.step,
       'rays': args.frames * H * W, 'render_host_s': round(time.perf_counter() - t0, 2),
       'atomic_bytes_per_s': ATOMIC_BYTES_PER_S}
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, 'scene.npz')
    np.savez(path, depth=depth)
    for variant in VARIANTS:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', variant, '--scene', path, '--frames', str(args.frames),
               '--dims', args.dims, '--voxel', str(args.voxel), '--step', str(args.step), '--rounds', str(args.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out[variant] = {'error': 'time limit of %.0f s' % args.limit}
            break                                                          # nothing more on a device that hung
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        if p.returncode != 0 or not lines:
            out[variant] = {'error': 'exit status %d' % p.returncode, 'stderr': p.stderr[-400:]}
            break                                                          # nor after a fault
        out[variant] = json.loads(lines[-1])
if all('ms' in out.get(v, {}) for v in VARIANTS):
    for v in VARIANTS[1:]:
        out[v]['ratio_to_cast'] = round(out[v]['ms'] / out['cast']['ms'], 3)
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
