"""sgnn_tune.prog_bn_fold_small: a small-level BatchNormReLU whose only reader is a <= 16-channel convolution is applied
by that convolution (k_conv_small<.., ConvPre> forward, k_conv_dw<.., 1, DwPre> for the weight gradient) instead of running
as a pass.  Through the C ABI, as tests/test_gpu_prog_fp64.py drives it.

The program: x -> conv a -> BN b1 -> conv c1 -> BN b2 -> conv c2 -> add(a, c2) = y -> BN b3 -> Convolution(2,2) z; y and
z are kept and carry gradients.  a feeds b1 and the add (two readers, stays a buffer); b1, b2, b3 each have one reader.

  * switch 0 against 1 in one process, bit for bit: kept outputs, running statistics, every parameter and input gradient,
    and the whole forward arena wherever the folded run wrote it (that covers save_mean / save_invstd, which live in the
    arena's per-op areas); what the folded run left unwritten must lie inside the folded layers' output buffers;
  * the folded forward and backward against the fp64 interpreter under the bars of tests/prog_ref.py;
  * the planner: launches saved = layers folded, counted through sgnn_launch_count; a reader that is not the next op, two
    readers and a table past the bn_fuse_ok budget do not fold.
The program has no loss; the loss is compared in the GraphStep test."""
import numpy as np
import pytest
import torch

import prog_cases as C
import prog_ref as R
import test_gpu_prog_fp64 as T

pytestmark = pytest.mark.gpu


class SizedCase(C.Case):
    """A case with an exact number of level-0 sites: the first n cells of a seeded permutation of side^3."""

    def __init__(self, n, *a, **kw):
        C.Case.__init__(self, *a, **kw)
        self.n_sites = n

    def coords(self):
        rng = np.random.default_rng(1000 + self.seed)
        s = self.side
        cells = rng.permutation(s ** 3)[:self.n_sites]
        return np.stack([cells // (s * s), (cells // s) % s, cells % s, np.zeros_like(cells)], 1).astype(np.int64)


def two_block(n, c, d, d2, side=8, seed=0):
    net = C.Net()
    x = net.ext(0, c)
    a = net.subm(x, c)
    c1 = net.subm(net.bn(a), d)
    c2 = net.subm(net.bn(c1), c)
    y = net.add(a, c2)
    z = net.down(net.bn(y), d2)
    net.finish()
    return SizedCase(n, 'fold_%d_%d_%d_%d' % (n, c, d, d2), net, False, [y, z], [y, z], {}, side=side, seed=seed)


def bn_ops(net):
    return [i for i, o in enumerate(net.ops) if o[0] == C.OP_BN]


@pytest.fixture
def fold():
    L = T._lib()
    saved = L.tune('prog_bn_fold_small')
    try:
        yield lambda v: L.tune('prog_bn_fold_small', v)
    finally:
        L.tune('prog_bn_fold_small', saved)


def forward_arena(case, lv, data, training, capacity=None, counts=None):
    """One forward call in the training layout, as T.execute makes it; returns (the whole NaN-prefilled forward arena on
    the CPU, {buffer: float offset in it}, rows per class)."""
    L = T._lib()
    net, geom = case.net, lv.geom
    params, ext, idx, _ = data
    live = case.rows(geom)
    ncls, nops, nbuf, n_ext = net.n_classes, len(net.ops), len(net.bufs), net.n_ext
    rows = T.capacity_rows(net, live, capacity) if capacity else list(live)
    lev_n, lev_ld, tabs, held = T.level_tables(net, geom, rows, live, capacity, counts)
    nan = float('nan')
    P = [p.cuda().clone() for p in params]
    E = [T._pad_rows(e, rows[net.bufs[b][0]], nan) for b, e in enumerate(ext)]
    I = [T._pad_rows(i.int(), rows[0], -1) for i in idx]
    keep = np.zeros(nbuf, dtype=np.int32)
    keep[case.keep] = 1
    ops, opf, bufs = net.ops_np, net.opf_np, net.bufs_np
    qa = (ops.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data, ncls, keep.ctypes.data)
    fwd_total = L.query('sgnn_prog_arena_floats', *qa, 1)
    wsb = L.query('sgnn_prog_ws_bytes', ops.ctypes.data, nops, lev_n.ctypes.data, ncls)
    arena = torch.full((max(fwd_total, 1),), nan, device='cuda')
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    pp, ep, ip = T._ptrs([p.data_ptr() for p in P]), T._ptrs([e.data_ptr() for e in E]), T._ptrs([i.data_ptr() for i in I])
    L.call('sgnn_prog_forward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, len(P), ep.ctypes.data, ip.ctypes.data, len(I), arena.data_ptr(),
           fwd_total, keep.ctypes.data, int(training), None, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    offs = dict((b, L.query('sgnn_prog_buffer_offset', *qa, 0, b)) for b in range(n_ext, nbuf))
    return arena.cpu(), offs, rows


def run(case, lv, data, training, capacity=None, counts=None):
    """(T.execute's outputs and gradients, the library launches of its two calls)."""
    lib = T._lib().load()
    before = lib.sgnn_launch_count()
    out = T.execute(case, lv, data, training, capacity=capacity, counts=counts)
    return out, lib.sgnn_launch_count() - before


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def assert_identical(case, lv, data, training, fold, folded_bns, capacity=None, counts=None):
    """folded_bns: which of the program's BatchNorm ops (in program order: 0, 1, ...) must fold; every other one must run."""
    tag = '%s training=%s capacity=%s counts=%s' % (case.name, training, capacity, counts)
    empty = counts is not None and not any(counts)
    fold(0)
    off, n0 = run(case, lv, data, training, capacity, counts)
    arena0, offs0, rows = forward_arena(case, lv, data, training, capacity, counts)
    fold(1)
    on, n1 = run(case, lv, data, training, capacity, counts)
    arena1, offs1, _ = forward_arena(case, lv, data, training, capacity, counts)
    # training: the apply launch goes; eval: the statistics copy and the apply launch go
    if not empty:
        assert n0 - n1 == len(folded_bns) * (1 if training else 2), (tag, n0, n1)
    for b in case.keep:
        assert same(on['bufs'][b], off['bufs'][b]), (tag, 'buffer', b)
    for key in ('params', 'gparams', 'gext'):
        for k, (u, v) in enumerate(zip(on[key], off[key])):
            assert (u is None) == (v is None) and (u is None or same(u, v)), (tag, key, k)
    assert arena0.shape == arena1.shape and offs0 == offs1, tag
    wrote = ~torch.isnan(arena1)
    assert bool((arena1[wrote] == arena0[wrote]).all()), (tag, 'forward arena (save_mean / save_invstd included)')
    # what only the unfolded run wrote: exactly the live rows of the folded layers' output buffers
    inside = torch.zeros_like(wrote)
    net = case.net
    live = case.rows(lv.geom) if counts is None else list(counts)
    for k, i in enumerate(bn_ops(net)):
        if k in folded_bns:
            b, lev, ch = net.ops[i][3], net.ops[i][5], net.ops[i][6]
            assert offs1[b] >= 0, (tag, b)
            inside[offs1[b]:offs1[b] + live[lev] * ch] = True
    only_off = (~wrote) & ~torch.isnan(arena0)
    assert bool((only_off == inside).all()), (tag, 'unwritten cells', int(only_off.sum()), int(inside.sum()))
    return on


def make(n, c, d, d2, side=8):
    case = two_block(n, c, d, d2, side)
    lv = T.Levels(case)
    return case, lv, case.data(lv.geom)


# rows: 1; the 16-row workgroup edge; 219 (the smallest level of the flagship step).  Every size below 512 cells of an 8^3
# grid has sites without some neighbour, one site has none at all: rows of missing rules must stay zero, not act(0).
@pytest.mark.parametrize('n', [1, 15, 16, 17, 219])
@pytest.mark.parametrize('chan', [(8, 8, 12), (12, 12, 16), (16, 16, 16), (8, 12, 12)])
def test_fold_is_bit_identical_to_the_pass(fold, n, chan):
    case, lv, data = make(n, *chan)
    # (8, 12, 12): conv c2 is 12 -> 8, no folded kernel of that shape: b2 stays a pass
    folded = [0, 2] if chan == (8, 12, 12) else [0, 1, 2]
    for training in (True, False):
        assert_identical(case, lv, data, training, fold, folded)


@pytest.mark.parametrize('chan', [(8, 8, 12), (16, 16, 16)])
def test_fold_in_capacity_mode(fold, chan):
    case, lv, data = make(219, *chan)
    for training in (True, False):
        assert_identical(case, lv, data, training, fold, [0, 1, 2], capacity=1.5)
    # live count 0 at non-zero capacity: nothing is written, no gradient is NaN
    on = assert_identical(case, lv, data, True, fold, [0, 1, 2], capacity=1.5, counts=[0] * case.net.n_classes)
    for g in on['gparams']:
        assert g is None or bool((g == 0).all())


@pytest.mark.parametrize('n, chan', [(17, (12, 12, 16)), (219, (16, 16, 16)), (219, (8, 8, 12))])
def test_folded_run_against_fp64_interpreter(fold, n, chan):
    case, lv, data = make(n, *chan)
    fold(1)
    check_fp64(case, lv, data)


def check_fp64(case, lv, data):
    """Forward and backward under the current switches against tests/prog_ref.py's fp64 interpreter, its own bars."""
    params, ext, idx, gouts = data
    net = case.net
    rows = case.rows(lv.geom)
    bad = []
    for training in (True, False):
        kw = dict(idx=idx, training=training, gouts=gouts)
        args = (net.ops_np, net.bufs_np, net.opf_np, net.n_ext, rows, lv.geom, params, ext)
        ref = R.run(*args, **kw)
        ref32 = R.run(*args, dtype=torch.float32, **kw)
        got = T.execute(case, lv, data, training)
        # (a program without fused adds or joins has every buffer read back: a folded layer's output was never written)
        got['bufs'] = dict((b, got['bufs'][b]) for b in case.keep)
        bad += T.compare(case, got, ref, ref32, training, 'fold train=%d' % training, data)
    assert not bad, '\n'.join(bad)


def test_planner_at_the_table_limit(fold):
    """bn_fuse_ok with the consumer's grid, 16 channels: blocks(producer) x blocks(consumer) x 256 bytes <= 48 MiB, i.e.
    443 x 443 sixteen-row blocks pass and 444 x 444 do not.  7088 rows: b1, b2 and b3 fold.  7104 rows: b1 and b2 stay
    passes; b3 still folds, its consumer (the stride-2 convolution) has the coarse level's far smaller grid."""
    for n, folded in ((7088, [0, 1, 2]), (7104, [2])):
        case, lv, data = make(n, 16, 16, 16, side=32)
        assert case.rows(lv.geom)[0] == n and (case.rows(lv.geom)[1] + 15) // 16 * 444 * 256 <= 48 << 20
        assert_identical(case, lv, data, True, fold, folded)


def test_two_readers_are_not_folded(fold):
    """u3: every BatchNorm output is read by a JoinTable and a convolution, or by an UnPooling."""
    case = T.CASES['u3']
    lv = T.Levels(case)
    assert_identical(case, lv, case.data(lv.geom), True, fold, [])


def test_reader_that_is_not_the_next_op_is_not_folded(fold):
    """b = bn(conv(x)); e = bn(conv(x)); g = conv(b): the convolution in front of e writes its statistics partials where
    those of b were — b's only reader is not the op behind it, so b runs as a pass (and reads its table in time).  e is
    kept.  Bit-identical to the switch off, nothing folds, and the values hold against the fp64 interpreter."""
    net = C.Net()
    x = net.ext(0, 8)
    b = net.bn(net.subm(x, 8))
    e = net.bn(net.subm(x, 8))
    g = net.subm(b, 8)
    net.finish()
    case = SizedCase(219, 'fold_far_reader', net, False, [e, g], [e, g], {}, side=8)
    lv = T.Levels(case)
    data = case.data(lv.geom)
    for training in (True, False):
        assert_identical(case, lv, data, training, fold, [])
    fold(1)
    check_fp64(case, lv, data)


@pytest.mark.parametrize('n', [17, 219])
def test_fold_of_a_four_channel_layer(fold, n):
    """16 -> 4 -> BN -> 4 -> 16: one float per lane quarter in the forward kernel, the fragment-mapped gathers in the
    weight gradient."""
    net = C.Net()
    x = net.ext(0, 16)
    y = net.subm(net.bn(net.subm(x, 4)), 16)
    net.finish()
    case = SizedCase(n, 'fold_4_16_%d' % n, net, False, [y], [y], {}, side=8)
    lv = T.Levels(case)
    data = case.data(lv.geom)
    for training in (True, False):
        assert_identical(case, lv, data, training, fold, [0])
    fold(1)
    check_fp64(case, lv, data)


def test_graph_step_replay_equals_eager_unfolded(fold):
    """GraphStep at batch 2 of 32^3 with a learning rate of 0: the parameters never move, so every step of one model
    computes the same loss and the same gradients (the running statistics move; a training-mode step does not read them).
    Switch off: the classic step, then the EAGER capacity step — its loss and flat gradient are the reference.  Switch on:
    classic, eager, capture + replay, two more replays — loss and the whole flat gradient of each of the three replayed
    steps equal the reference bit for bit.  The eager step with the switch on launches fewer kernels: the model folds."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
    from util import param_fill
    from sgnn_amd import synth
    from sgnn_amd.model import GenModel
    from sgnn_amd.train import GraphStep
    lib = T._lib().load()
    dims, cfg = (32, 32, 32), 11
    data = synth.make_batch(2, dims, cfg=cfg, occupancy=0.08)
    locs, feats = data['input']
    lw = np.ones(5, dtype=np.float32)
    batch = {'input': [locs.cuda(), feats.cuda()], 'sdf': data['sdf'].cuda(), 'known': data['known'].cuda(),
             'hierarchy': [h.cuda() for h in data['hierarchy']]}

    def steps(on, count):
        fold(on)
        gm = param_fill(GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().to('cuda:0')
        gs = GraphStep(gm, lr=0.0, settle=False)
        out = []
        for _ in range(count):
            before = lib.sgnn_launch_count()
            loss = float(gs(batch, lw))
            torch.cuda.synchronize()
            out.append((loss, gs.opt.flat_g.detach().cpu().clone(), lib.sgnn_launch_count() - before))
        return out, gs.stats

    ref, st0 = steps(0, 2)
    assert st0['eager_steps'] == 1 and st0['replays'] == 0, st0
    got, st1 = steps(1, 5)
    assert st1['captures'] == 1 and st1['replays'] == 3 and st1['overflows'] == 0, st1
    assert got[1][2] < ref[1][2], ('nothing folds in the eager step', got[1][2], ref[1][2])
    assert bool(ref[1][1].abs().sum() > 0)
    for loss, g, _ in got[2:]:
        assert loss == ref[1][0], (loss, ref[1][0])
        assert torch.equal(g, ref[1][1])
