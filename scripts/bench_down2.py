"""Stride-2 builder timings on the level-0 cloud of bench.py's default batch (32 blocks of 64^3, 366 085 sites):
sgnn_rulebook_down2 and sgnn_down2_tables (one level), sgnn_down2_chain and sgnn_down2_chain_tables (the three encoder
levels, capacities = the row count).  One line per entry point, then all four as one JSON line (us per call)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import _lib, synth  # noqa: E402
from sgnn_amd._lib import ptr  # noqa: E402

dev = torch.device('cuda:0')
DEPTH = 3
locs = synth.make_batch(32, (64,) * 3, cfg=2, occupancy=0.05)['input'][0]
fine = locs.to(torch.int32).to(dev).contiguous()
n = int(fine.shape[0])
ccap = _lib.query('sgnn_hash_capacity', n)
ld = (n + 255) // 256 * 256
mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
ckeys, cvals = [mk(ccap, torch.int64) for _ in range(DEPTH)], [mk(ccap, torch.int32) for _ in range(DEPTH)]
parent, coarse = [mk(n, torch.int32) for _ in range(DEPTH)], [mk((n, 4), torch.int32) for _ in range(DEPTH)]
children, ptable = [mk(8 * ld, torch.int32) for _ in range(DEPTH)], [mk(8 * ld, torch.int32) for _ in range(DEPTH)]
counts, n0 = torch.zeros(DEPTH, dtype=torch.int64, device=dev), torch.tensor([n], dtype=torch.int64, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)
wsb = max(_lib.query('sgnn_down2_ws_bytes', n), _lib.query('sgnn_down2_chain_ws_bytes', n),
          _lib.query('sgnn_down2_chain_tables_ws_bytes', n, DEPTH))
ws = mk(wsb, torch.uint8)
arr = lambda ts: np.ascontiguousarray(np.array([t.data_ptr() for t in ts], dtype=np.uint64))  # noqa: E731
keep = [arr(v) for v in (ckeys, cvals, parent, coarse, children, ptable)]
caps = np.full(DEPTH, n, dtype=np.int64)

_lib.call('sgnn_rulebook_down2', ptr(fine), n, ptr(ckeys[0]), ptr(cvals[0]), ccap, ptr(parent[0]), ptr(coarse[0]),
          ptr(counts), ptr(ws), wsb)
nc = int(counts[0].item())


def down2():
    _lib.call('sgnn_rulebook_down2', ptr(fine), n, ptr(ckeys[0]), ptr(cvals[0]), ccap, ptr(parent[0]), ptr(coarse[0]),
              ptr(counts), ptr(ws), wsb)


def tables():
    _lib.call('sgnn_down2_tables', ptr(fine), ptr(parent[0]), n, ptr(children[0]), ld, nc, ptr(ptable[0]), ld, None, None)


def chain():
    _lib.call('sgnn_down2_chain', ptr(fine), n, None, n, DEPTH, keep[0].ctypes.data, keep[1].ctypes.data, ccap,
              keep[2].ctypes.data, keep[3].ctypes.data, ptr(counts), None, None, ptr(ws), wsb)


def chain_tables():
    _lib.call('sgnn_down2_chain_tables', ptr(fine), ptr(n0), n, DEPTH, keep[0].ctypes.data, keep[1].ctypes.data, ccap,
              keep[2].ctypes.data, keep[3].ctypes.data, ptr(counts), caps.ctypes.data, keep[4].ctypes.data,
              keep[5].ctypes.data, ptr(status), ptr(ws), wsb)


res = {}
for name, f in (('sgnn_rulebook_down2', down2), ('sgnn_down2_tables', tables), ('sgnn_down2_chain', chain),
                ('sgnn_down2_chain_tables', chain_tables)):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(1000):
        f()
    e1.record()
    torch.cuda.synchronize()
    res[name] = round(e0.elapsed_time(e1) / 1000 * 1e3, 2)
    print('N=%d %-24s %8.1f us' % (n, name, res[name]))
assert int(status.item()) == 0, 'status %d' % int(status.item())
print(json.dumps({'rows': n, 'coarse_rows': [int(v) for v in counts.tolist()], 'us': res}))
