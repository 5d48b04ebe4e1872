"""The bf16 program executor (forward_bf16 in prog.hip: sgnn_prog_forward with training = 2 | 4) op by op and branch by
branch against the interpreters of tests/prog_ref.py, on the programs of tests/prog_cases.py.

The test drives the C ABI as test_gpu_prog_fp64.py does (its helpers are imported): it owns the descriptor arrays, keep
and the arena, which it pre-fills with NaN through a bf16 view (an fp32 NaN leaves every other bf16 element zero), and
it reads a kept buffer itself: the bytes at 4 x sgnn_prog_buffer_offset(infer = 2) are [rows, round8(channels)] bf16,
columns [:channels]; a LINEAR output is fp32 [rows, channels].

Every case runs (a) with its own keep and the fusions on, the plan asserted against sgnn_prog_plan mode 3, (b) with
prog_fusion = 0, (c) with every non-external buffer kept, which compares every intermediate and stops fusion, views and
the recycling of arena slots; cases with heads also under the prog_lin_bn / prog_lin_add settings of the fp32 test.

Comparison rules
  * exact cases (the integer cases under data(geom, bf16=True); test_prog_ref.py shows that every value they store is a
    bf16 value and every sum of |terms| below 2^24): every compared buffer equals the fp64 interpreter bit for bit.
    Their externals are +-(1 + 2^-8), no bf16 values: the fp64 interpreter is fed them rounded (to +-1), the executor
    unrounded, so a reader that takes the fp32 tensor instead of its bf16 copy differs in the sums.
  * real cases, per compared tensor: err = max |y - ref64| / max |ref64| <= max(k x e_bf, 2^-8), e_bf the same distance
    of the rounding interpreter (run(..., storage='bf16')) from the fp64 one, 2^-8 one bf16 ulp of the largest value;
    k = prog_ref.BAR_K_BF16, the smallest power of two that covers the worst err / e_bf measured with prog_fusion = 0
    (profiles/prog_bf16_ratios.txt); runs (a) and (c) meet the same k.  Every value is finite.
  * one of the four mutations of test_prog_ref.py (external_not_rounded) moves no real case by 2 bars from the fp64 run,
    so, as the rule for a mutation that hides asks, the real cases are ALSO held to the rounding interpreter itself,
    under the same bar: |y - ref_bf| / max |ref_bf| <= max(k x e_bf, 2^-8).
Set SGNN_PROG_RATIOS to a file name to have every measured ratio appended to it."""
import numpy as np
import pytest
import torch

import prog_cases as C
import prog_ref as R
from test_gpu_prog_fp64 import (CAPACITY_CASES, Levels, _lib, _log, _pad_rows, _ptrs, capacity_rows, level_tables,
                                tune)  # noqa: F401  (tune: fixture)

pytestmark = pytest.mark.gpu

CASES = dict((c.name, c) for c in C.cases() if c.knobs is None)      # (the knobs switch fp32 kernels only)
NEW_JOINS = [n for n in CASES if n.startswith(('join_int_6', 'join_int_10', 'join_int_12', 'nested_int_6', 'join_bn_6',
                                               'join_bn_10', 'join_bn_12', 'nested_bn_6'))]
BF16_FLAGS = 2 | 4
SLACK = 256


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def execute(case, lv, data, keep=None, capacity=None, counts=None, flags=BF16_FLAGS):
    """One bf16 forward call under the current switches; keep: the buffers to read (default: the case's).  Returns
    {'bufs': {buffer: all rows, bf16 or (LINEAR) fp32, on the CPU}, 'live': live rows per class, 'tenant': {buffer: per
    element, whether its arena bytes also lie in the live rows of another buffer's slot or of an external's bf16 copy},
    'stale': {buffer: what its bf16 elements hold if nothing but the externals' bf16 copies was ever written there}} —
    the arena is liveness-packed, so a kept buffer may take over the slot of a buffer or of a bf16 copy that died before
    it was first written, and then its rows past the count hold that tenant's live rows instead of the pre-fill."""
    L = _lib()
    net, geom = case.net, lv.geom
    params, ext, idx, _ = data
    live = case.rows(geom)
    ncls, nops, nbuf, n_ext = net.n_classes, len(net.ops), len(net.bufs), net.n_ext
    rows = capacity_rows(net, live, capacity) if capacity else list(live)
    lev_n, lev_ld, tabs, held = level_tables(net, geom, rows, live, capacity, counts)
    nan = float('nan')
    P = [p.cuda().clone() for p in params]
    E = [_pad_rows(e, rows[net.bufs[b][0]], nan) for b, e in enumerate(ext)]
    E0 = [e.clone() for e in E]
    I = [_pad_rows(i.int(), rows[0], -1) for i in idx]
    kept = np.zeros(nbuf, dtype=np.int32)
    kept[list(case.keep if keep is None else keep)] = 1
    ops, opf, bufs = net.ops_np, net.opf_np, net.bufs_np
    qa = (ops.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data, ncls, kept.ctypes.data)
    total = L.query('sgnn_prog_arena_floats', *qa, 3)
    assert total >= 0
    wsb = L.query('sgnn_prog_ws_bytes', ops.ctypes.data, nops, lev_n.ctypes.data, ncls)
    arena = torch.empty(max(total, 1) + SLACK, device='cuda')      # SLACK floats behind what the layout asked for
    arena.view(torch.bfloat16).fill_(nan)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    pp, ep, ip = _ptrs([p.data_ptr() for p in P]), _ptrs([e.data_ptr() for e in E]), _ptrs([i.data_ptr() for i in I])
    L.call('sgnn_prog_forward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, len(P), ep.ctypes.data, ip.ctypes.data, len(I), arena.data_ptr(),
           total, kept.ctypes.data, flags, None, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert bool(torch.isnan(arena[max(total, 1):].view(torch.bfloat16).float()).all()), 'written behind the arena'
    for b, (e, e0) in enumerate(zip(E, E0)):
        assert torch.equal(_bits(e), _bits(e0)), 'external %d was written' % b
    for s, (p, p0) in enumerate(zip(P, params)):
        assert torch.equal(p.cpu(), p0), 'parameter slot %d was written' % s
    heads = set(o[3] for o in net.ops if o[0] == C.OP_LINEAR)
    out = {'bufs': {}, 'live': live if counts is None else list(counts), 'tenant': {}, 'stale': {}}
    # the arena as the externals' bf16 copies alone leave it (their offsets: the same query), on the CPU
    image = torch.full((2 * max(total, 1),), nan, dtype=torch.bfloat16)
    shadows = {}
    for b in range(n_ext):
        off = L.query('sgnn_prog_buffer_offset', *qa, 2, b)
        if off >= 0:
            n, ch = out['live'][bufs[b, 0]], int(bufs[b, 1])
            ld = (ch + 7) // 8 * 8
            shadows[b] = (4 * off, 2 * ld)
            image[2 * off:2 * off + n * ld].view(n, ld)[:, :ch] = E[b][:n].cpu().bfloat16()
    readers = set(b for o in net.ops if o[0] != C.OP_CONCAT_IN for b in (o[1], o[2]) if 0 <= b < n_ext)
    assert set(shadows) == readers, (sorted(shadows), sorted(readers))
    plan = C.read_plan(L.query, case, rows, 3, keep=np.nonzero(kept)[0])
    unwritten = set(int(net.ops[i][3]) for i, d in enumerate(plan['add_dst']) if d >= 0)      # fused-away conv outputs
    slots = {}
    for b in range(n_ext, nbuf):
        off = L.query('sgnn_prog_buffer_offset', *qa, 2, b)
        if off >= 0 and b not in unwritten:
            ch = int(bufs[b, 1])
            slots[b] = (4 * off, 4 * ch if b in heads else 2 * ((ch + 7) // 8 * 8))      # byte offset, bytes per row
    for b in np.nonzero(kept)[0].tolist():
        assert b in slots, b
        off, rb = slots[b]
        r, ch = rows[bufs[b, 0]], int(bufs[b, 1])
        assert off + r * rb <= 4 * max(total, 1)
        other = torch.zeros(4 * arena.numel(), dtype=torch.bool)
        for b2, (off2, rb2) in list(slots.items()) + list(shadows.items()):
            if b2 != b:
                other[off2:off2 + out['live'][bufs[b2, 0]] * rb2] = True
        es = 4 if b in heads else 2
        view = arena.view(torch.float32 if b in heads else torch.bfloat16)
        out['bufs'][b] = view[off // es:off // es + r * (rb // es)].view(r, rb // es)[:, :ch].cpu()
        out['tenant'][b] = other[off:off + r * rb].view(r, rb // es, es).all(2)[:, :ch]
        if b not in heads:
            out['stale'][b] = image[off // 2:off // 2 + r * (rb // 2)].view(r, rb // 2)[:, :ch]
    return out


def references(case, lv, data):
    net = case.net
    params, ext, idx, _ = data
    args = (net.ops_np, net.bufs_np, net.opf_np, net.n_ext, case.rows(lv.geom), lv.geom, params)
    if case.integer:      # the externals are no bf16 values (prog_cases.BF16_EXT_SCALE): the executor has to round them
        return R.run(*args, R.bf16_externals(ext), idx, training=False)['bufs'], None
    return R.run(*args, ext, idx, training=False)['bufs'], R.run(*args, ext, idx, training=False, storage='bf16')['bufs']


def compare(case, got, r64, rbf, tag):
    bad = []
    for b, y in got['bufs'].items():
        want = r64[b]
        y = y[:want.shape[0]]
        if case.integer:
            if not torch.equal(y.double(), want):
                bad.append('%s buf%d: %d of %d values differ' % (tag, b, int((y.double() != want).sum()), want.numel()))
            continue
        err, err_bf, e_bf = R.max_norm_error(y, want), R.max_norm_error(y, rbf[b]), R.max_norm_error(rbf[b], want)
        ratio = err / e_bf if e_bf > 0 else (0.0 if err == 0 else float('inf'))
        bar = R.bar_bf16(e_bf)
        _log('%-28s %-34s buf%-7d err %.3e  e_bf %.3e  ratio %8.3f  bar %.3e  err_vs_rounding %.3e' % (
            case.name, tag, b, err, e_bf, ratio, bar, err_bf))
        if not err <= bar:
            bad.append('%s buf%d: err %.3e > bar %.3e (e_bf %.3e, ratio %.2f)' % (tag, b, err, bar, e_bf, ratio))
        if not err_bf <= bar:
            bad.append('%s buf%d: %.3e from the rounding interpreter > bar %.3e' % (tag, b, err_bf, bar))
    return bad


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if not c.empty])
def test_bf16_executor_against_the_interpreters(tune, name):
    L = _lib()
    case = CASES[name]
    lv = Levels(case)
    data = case.data(lv.geom, bf16=True)
    net = case.net
    rows = case.rows(lv.geom)
    r64, rbf = references(case, lv, data)
    has_head = any(o[0] == C.OP_LINEAR for o in net.ops)
    settings = [dict(prog_fusion=1), dict(prog_fusion=0)]
    if has_head:
        settings += [dict(prog_fusion=1, prog_lin_bn=0), dict(prog_fusion=1, prog_lin_bn=0, prog_lin_add=0)]
    bad = []
    for st in settings:
        tune(**st)
        tag = 'fusion=%d lin_bn=%d lin_add=%d' % (st['prog_fusion'], st.get('prog_lin_bn', 1), st.get('prog_lin_add', 1))
        want = C.expected_plan(case, st['prog_fusion'], bf16=True)
        if not st.get('prog_lin_bn', 1):
            want['lin_bn'] = [-1] * len(net.ops)
        assert C.read_plan(L.query, case, rows, 3) == want, tag
        bad += compare(case, execute(case, lv, data), r64, rbf, tag)
    tune(prog_fusion=1)
    bad += compare(case, execute(case, lv, data, keep=range(net.n_ext, len(net.bufs))), r64, rbf, 'all kept')
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('name', CAPACITY_CASES + NEW_JOINS)
def test_capacity_mode_equals_the_exact_size_run(tune, name, fused):
    """lev_n = about 1.5 x the true rows, the true counts in device memory (lev_cnt).  Inputs and index arrays past the
    count are NaN / -1.  Two pairs of runs, each an exact-size run against a capacity run:
      * every non-external buffer kept (no buffer dies, so none is placed over another's rows): the live rows of EVERY
        buffer are bit-identical to the exact-size run and every row past the count is still bf16 NaN (fp32 NaN for a
        LINEAR output: stage_lin_add buf7), strictly.  One tenant remains even then: the bf16 copy of an external dies
        behind its last reader, and in join_bn_5_7, join_bn_5_8 and join_bn_10_12 buf4 takes its slot.  Its content is
        known to the bit (execute: 'stale'), so the rule stays strict: every element past the count equals, bit for
        bit, what the pre-fill and the externals' copies alone leave there;
      * the case's own keep, which leaves fusion, views and recycling on: live rows bit-identical; a row past the count
        is still NaN or lies in bytes that another buffer's live rows occupy (execute: 'tenant').  The liveness-packed
        arena puts a kept buffer into the slot of a buffer that died before it, and that tenant's live rows show
        through there.  This mask is wide: at capacity 1.5 it covers the whole region past the count for residual_8_12
        (fused), nested_int_6_12_8, join_bn_6_12 and join_bn_12_12 buf6 (fusion off) and stage_lin_add buf7 (both), and
        most of it for u3 (fusion off), so for those the second pair checks the live rows only and the strict rule
        rests on the first pair."""
    case = CASES[name]
    net = case.net
    lv = Levels(case)
    data = case.data(lv.geom, bf16=True)
    tune(prog_fusion=fused)
    bad = []
    for keep in (range(net.n_ext, len(net.bufs)), None):
        exact = execute(case, lv, data, keep=keep)
        cap = execute(case, lv, data, keep=keep, capacity=1.5)
        for b in (case.keep if keep is None else keep):
            n = exact['live'][net.bufs[b][0]]
            y = cap['bufs'][b]
            assert y.shape[0] > n and exact['bufs'][b].shape[0] == n
            tag = 'buffer %d (%s)' % (b, 'own keep' if keep is None else 'all kept')
            if not torch.equal(_bits(y[:n]), _bits(exact['bufs'][b])):
                bad.append('%s: %d live values differ' % (tag, int((_bits(y[:n]) != _bits(exact['bufs'][b])).sum())))
            if not bool(torch.isfinite(y[:n].float()).all()):
                bad.append('%s: live values are not finite' % tag)
            if keep is None:
                untouched = torch.isnan(y[n:].float()) | cap['tenant'][b][n:]
            elif b in cap['stale']:
                untouched = _bits(y[n:]) == _bits(cap['stale'][b][n:])
            else:
                untouched = torch.isnan(y[n:])
            if not bool(untouched.all()):
                bad.append('%s: %d values past the count were written' % (tag, int((~untouched).sum())))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['u3_all_levels_empty', 'stage_level0_empty', 'stage_empty_source'])
def test_empty_rows_classes(tune, name):
    """Every level empty, level 0 empty under sources with rows, a source without rows: no error.  Nothing is written
    where it must not be: execute() asserts that externals and parameters keep their bits and that the floats behind
    the arena keep their NaN; a program without level-0 sites has no row in any buffer, so its arena is the per-op
    weight areas alone.  The case
    with sites is compared like any real case."""
    case = CASES[name]
    lv = Levels(case)
    data = case.data(lv.geom, bf16=True)
    for fused in (1, 0):
        tune(prog_fusion=fused)
        got = execute(case, lv, data)
        if case.empty:
            assert all(v.shape[0] == 0 for v in got['bufs'].values())
            assert all(lv.geom.n[l] == 0 for l in range(case.net.nlev))
        else:
            r64, rbf = references(case, lv, data)
            bad = compare(case, got, r64, rbf, 'fusion=%d' % fused)
            assert not bad, '\n'.join(bad)


def test_zero_live_rows_at_nonzero_capacity(tune):
    """Every device row count is zero while the capacities are not: no error and no row of a kept buffer written."""
    case = CASES['u3']
    lv = Levels(case)
    data = case.data(lv.geom, bf16=True)
    for fused in (1, 0):
        tune(prog_fusion=fused)
        for keep in (None, range(case.net.n_ext, len(case.net.bufs))):
            got = execute(case, lv, data, keep=keep, capacity=1.5, counts=[0] * case.net.n_classes)
            for b, y in got['bufs'].items():
                assert y.shape[0] > 0 and bool(torch.isnan(y.float()).all()), (fused, b)


@pytest.mark.parametrize('flags', [4, 4 | 1, 4 | 2 | 1])
def test_bf16_storage_outside_eval_inference_is_refused(tune, flags):
    from sgnn_amd._lib import SgnnError
    case = CASES['residual_8_12']
    lv = Levels(case)
    with pytest.raises(SgnnError):
        execute(case, lv, case.data(lv.geom, bf16=True), flags=flags)


# ---- the Python side once: run_program inside sgnn_amd.bf16_inference() ----

def test_run_program_reads_back_what_the_rounding_interpreter_computes(monkeypatch):
    """A module graph with an in-place join at a 12-channel column, a residual add, an up-sampling stage and a two-logit
    head, compiled by Program and run in eval under no_grad() inside bf16_inference(): what run_program returns (through
    the offset query, the sgnn_bf16_to_f32 read-back with its round8 stride, and the fp32 head path) against the
    interpreters, under the bar of the real cases."""
    import sgnn_amd
    import sgnn_amd.scn as s
    from sgnn_amd.scn.program import Program, run_program
    gen = torch.Generator().manual_seed(11)
    res = s.Sequential().add(s.ConcatTable().add(s.Identity()).add(
        s.Sequential().add(s.SubmanifoldConvolution(3, 16, 16, 3, False)).add(s.BatchNormReLU(16))
        .add(s.SubmanifoldConvolution(3, 16, 16, 3, False)))).add(s.AddTable())
    inner = s.Sequential().add(s.Convolution(3, 12, 16, 2, 2, False)).add(s.BatchNormReLU(16)).add(res) \
        .add(s.BatchNormReLU(16)).add(s.UnPooling(3, 2, 2))
    mid = s.BatchNormReLU(16)
    chain = s.Sequential().add(s.SubmanifoldConvolution(3, 8, 12, 3, False)).add(s.BatchNormReLU(12)) \
        .add(s.ConcatTable().add(s.Identity()).add(inner)).add(s.JoinTable()) \
        .add(s.SubmanifoldConvolution(3, 28, 16, 3, False)).add(mid)
    up, ubn = s.SubmanifoldConvolution(3, 16, 8, 3, False), s.BatchNormReLU(8)
    lins = torch.nn.ModuleList([torch.nn.Linear(8, 1), torch.nn.Linear(8, 1)])
    mods = torch.nn.ModuleList([chain, up, ubn, lins])
    for p in mods.parameters():
        p.data = torch.randn(p.shape, generator=gen) * (0.2 if p.dim() > 1 else 0.3) + (1.0 if p.dim() == 1 and p.numel() > 1 else 0.0)
    for n, b in mods.named_buffers():
        b.data = torch.rand(b.shape, generator=gen) + (0.5 if n.endswith('var') else -0.5)
    mods.cuda().eval()
    prog = Program([chain], 8, tail=[('expand', up), ('bn', ubn), ('linear', list(lins))])
    assert sorted(set(int(o[0]) for o in prog.ops)) == sorted([R.OP_SUBM, R.OP_DOWN, R.OP_UNPOOL, R.OP_BN, R.OP_ADD,
                                                               R.OP_JOIN, R.OP_EXPAND, R.OP_LINEAR])
    rng = np.random.default_rng(5)
    cells = rng.permutation(np.nonzero(rng.random(12 ** 3) < 0.3)[0])
    coords = np.stack([cells // 144, (cells // 12) % 12, cells % 12, np.zeros_like(cells)], 1).astype(np.int64)
    feats = torch.randn(len(cells), 8, generator=gen)
    x = s.InputLayer(3, [12, 12, 12], mode=0)([torch.from_numpy(coords), feats.cuda()])
    out_bufs = [prog.out, prog.taps[id(ubn)][0], prog.tail_out]
    # what _run hands to sgnn_prog_forward (n_ext, row counts, keep, flags), read from the call itself
    import ctypes
    from sgnn_amd.scn import program as prog_mod
    real_call, seen = prog_mod._lib.call, []

    def spy(fn, *a):
        if fn == 'sgnn_prog_forward':
            seen.append(dict(n_ext=a[5], flags=a[22],
                             lev_n=np.ctypeslib.as_array(ctypes.cast(a[6], ctypes.POINTER(ctypes.c_int64)), (a[13],)).copy(),
                             keep=np.ctypeslib.as_array(ctypes.cast(a[21], ctypes.POINTER(ctypes.c_int32)), (a[4],)).copy()))
        return real_call(fn, *a)
    monkeypatch.setattr(prog_mod._lib, 'call', spy)
    with torch.no_grad(), sgnn_amd.bf16_inference():
        outs, grids, downs = run_program(prog, x, False, out_bufs=out_bufs)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen) == 1 and seen[0]['flags'] == BF16_FLAGS and seen[0]['n_ext'] == 1
    # the plan this run took: the JoinTable in place, its second input at column 12 (byte 24 of a 32-element row)
    L = _lib()
    rows = [g.n for g in grids] + [8 * grids[0].n]
    keep, lev_n = np.ascontiguousarray(seen[0]['keep']), np.ascontiguousarray(seen[0]['lev_n'])
    assert lev_n.tolist() == rows and np.nonzero(keep)[0].tolist() == sorted(out_bufs)
    plan = np.full(4 * len(prog.ops) + 3 * len(prog.bufs), -7, dtype=np.int32)
    assert L.query('sgnn_prog_plan', prog.ops_np.ctypes.data, len(prog.ops), prog.bufs_np.ctypes.data, len(prog.bufs), seen[0]['n_ext'],
                   lev_n.ctypes.data, prog.n_classes, keep.ctypes.data, 3, plan.ctypes.data) == 0
    jop = [i for i, o in enumerate(prog.ops) if o[0] == R.OP_JOIN][0]
    pb = plan[4 * len(prog.ops):].reshape(-1, 3)
    assert plan[4 * jop + 2] == 1 and pb[prog.ops[jop][2]].tolist() == [prog.ops[jop][3], 12, 32]
    assert max(plan[1:4 * len(prog.ops):4]) >= 0          # the residual add is fused
    geom = R.Geometry(coords, [g.subm_table().view(27, g.ld)[:, :g.n].cpu() for g in grids],
                      [d.children.view(8, d.ldc)[:, :d.coarse.n].cpu() for d in downs], [d.parent.cpu() for d in downs])
    params = [getattr(m, nm).detach().cpu() for m, nm in prog.slots]
    args = (prog.ops_np, prog.bufs_np, prog.opf_np, 1, rows, geom, params, [feats])
    r64 = R.run(*args, training=False)['bufs']
    rbf = R.run(*args, training=False, storage='bf16')['bufs']
    for b, y in zip(out_bufs, outs):
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(r64[b].shape)
        e_bf = R.max_norm_error(rbf[b], r64[b])
        err, err_bf = R.max_norm_error(y, r64[b]), R.max_norm_error(y, rbf[b])
        _log('%-28s %-34s buf%-7d err %.3e  e_bf %.3e  ratio %8.3f  bar %.3e  err_vs_rounding %.3e' % (
            'run_program', 'python side', b, err, e_bf, err / e_bf, R.bar_bf16(e_bf), err_bf))
        assert err <= R.bar_bf16(e_bf) and err_bf <= R.bar_bf16(e_bf), (b, err, err_bf, e_bf)
        if b != prog.tail_out:      # a bf16 buffer read back: every value is a bf16 value
            assert torch.equal(y.cpu().bfloat16().float(), y.cpu())
