"""Whole-scene inference (BASELINE configs[3], the (128, 512, 512) scene of scripts/run_configs.py c4), fp32 against the bf16
inference mode (sgnn_amd.bf16_inference) in one process: forward ms (device events, median), peak allocated memory,
sites per level, and the per-level Jaccard index of the predicted site sets.  Prints one JSON line.

    python scripts/bench_infer_bf16.py [--dims 128 512 512] [--iters 10] [--warmup 2]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_infer_bf16.py --iters 3`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sgnn_amd  # noqa: E402
from sgnn_amd import synth  # noqa: E402
from sgnn_amd.model import GenModel  # noqa: E402
from sgnn_amd.scn import program as P_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dims', type=int, nargs=3, default=[128, 512, 512])
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--warmup', type=int, default=2)
args = ap.parse_args()

lw = np.ones(5, dtype=np.float32)
dims = tuple(args.dims)
locs, feats = synth.make_scene(dims, cfg=4, occupancy=0.05)[:2]
torch.manual_seed(0)
m = GenModel(8, (128, 128, 128), 1, 16, 16, 4, True, True, 1, 1).cuda()
m.update_sizes(np.array(dims), np.array(dims) // 8)
inp = [locs.cuda(), feats.cuda()]
# running statistics from one training-mode pass with "replace" momentum (as scripts/run_configs.py c4)
saved = []
for mod in m.modules():
    if isinstance(mod, torch.nn.BatchNorm3d):
        saved.append((mod, mod.momentum)); mod.momentum = 1.0
    elif hasattr(mod, 'running_mean') and hasattr(mod, 'momentum'):
        saved.append((mod, mod.momentum)); mod.momentum = 0.0
with torch.no_grad():
    m.train()
    m(inp, lw)
for mod, mom in saved:
    mod.momentum = mom
m.eval()


def forward(bf16):
    with torch.no_grad():
        if bf16:
            with sgnn_amd.bf16_inference():
                return m(inp, lw)
        return m(inp, lw)


res = {'sites_in': int(locs.shape[0]), 'dims': list(dims)}
outs = {}
for name, bf16 in (('fp32', False), ('bf16', True)):
    for _ in range(args.warmup):
        forward(bf16)
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = forward(bf16)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    P_.release_arenas()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = forward(bf16)
    torch.cuda.synchronize()
    outs[name] = out
    res[name] = {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)),
                 'peak_gb': torch.cuda.max_memory_allocated() / 2 ** 30,
                 'sites': [int(o[0].shape[0]) if torch.is_tensor(o[0]) and o[0].numel() else 0 for o in out[1]],
                 'arena_floats': [int(p.last_arena_floats[0]) for p in P_.programs_of(m)]}
jac = []
for (la, _), (lb, _) in zip(outs['fp32'][1], outs['bf16'][1]):
    sa = set(map(tuple, la.cpu().numpy().tolist())) if torch.is_tensor(la) and la.numel() else set()
    sb = set(map(tuple, lb.cpu().numpy().tolist())) if torch.is_tensor(lb) and lb.numel() else set()
    jac.append(len(sa & sb) / max(1, len(sa | sb)))
res['jaccard'] = jac
res['speedup'] = res['fp32']['ms_median'] / res['bf16']['ms_median']
print(json.dumps(res))
