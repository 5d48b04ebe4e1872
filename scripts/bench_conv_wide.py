"""Stand-alone timing of the wide-row 3x3x3 convolutions (k_conv_fwd_u<26|30|34,16,27> and <16,26|30|34,27>,
conv_unrolled.hip) on synthetic levels of the benchmark's kind (needs GPU): forward, forward + statistics and the data
gradient per shape, and how many workgroups the one-round tiling keeps live (the non-zero statistics partials), from which
the resident workgroups per CU follow.  Prints one JSON line; SGNN_LIB selects a kernel-variant build for an A/B.
  python scripts/bench_conv_wide.py [--batches 32 52] [--dim 64] [--iters 50]"""
import argparse, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgnn_amd import synth, _lib
from sgnn_amd.scn import functions as F_
from sgnn_amd.scn.metadata import Grid, coords_from_locs

ap = argparse.ArgumentParser()
ap.add_argument('--batches', type=int, nargs='+', default=[32, 52], help='blocks per level: 32 -> 366 k sites, 52 -> ~600 k')
ap.add_argument('--dim', type=int, default=64)
ap.add_argument('--iters', type=int, default=50)
args = ap.parse_args()
dev = torch.device('cuda')
lib = _lib.load()
SHAPES = [(26, 16), (16, 26), (30, 16), (16, 30), (34, 16), (16, 34)]
FL = F_.CONV_TRANSPOSE_W | F_.CONV_FLIP_K


def timeit(fn, iters=args.iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


out = {'lib': os.environ.get('SGNN_LIB', 'default'), 'levels': []}
torch.manual_seed(0)
for batch in args.batches:
    data = synth.make_batch(batch, (args.dim,) * 3, cfg=2, occupancy=0.05)
    g = Grid(coords_from_locs(data['input'][0], dev))
    tab, n = g.subm_table(), g.n
    level = {'sites': n, 'tiles': (n + 255) // 256, 'us': {}, 'live_workgroups': {}}
    nblk = _lib.query('sgnn_conv_stats_blocks', n)
    for cin, cout in SHAPES:
        x = torch.randn(n, cin, device=dev)
        dy = torch.randn(n, cout, device=dev)
        w = torch.randn(27, cin, cout, device=dev) * 0.1
        y, dx = torch.empty(n, cout, device=dev), torch.empty(n, cin, device=dev)
        part = torch.zeros(nblk, 2, cout, dtype=torch.float64, device=dev)

        def run(src, ci, dst, co, flags, stats):
            _lib.call('sgnn_conv_fwd_epi', src.data_ptr(), n, ci, 0, w.data_ptr(), 27, tab.data_ptr(), g.ld, n, co,
                      dst.data_ptr(), 0, flags, None, 0, stats, part.data_ptr() if stats else None, None, 0, None, None,
                      None, None, 0.0)

        key = '%d,%d' % (cin, cout)
        level['us'][key] = {'fwd': round(timeit(lambda: run(x, cin, y, cout, 0, 0)), 2),
                            'fwd_stats': round(timeit(lambda: run(x, cin, y, cout, 0, 1)), 2),
                            'dx': round(timeit(lambda: run(dy, cout, dx, cin, FL, 0)), 2)}
        # the workgroups past the live ones write all-zero partials (k_conv_fwd_u): live = tiles / J
        live = int((part.abs().sum((1, 2)) > 0).sum())
        level['live_workgroups'][key] = live
    out['levels'].append(level)
print(json.dumps(out))
