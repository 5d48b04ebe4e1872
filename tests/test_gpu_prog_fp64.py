"""The native program executor (sgnn_prog_forward / sgnn_prog_backward, prog.hip) op by op and branch by branch against
the fp64 interpreter of tests/prog_ref.py, on the small programs of tests/prog_cases.py.

The test drives the C ABI itself: it owns the descriptor arrays, keep, gout, gext and the arenas.  Every case runs with
the fusions on and off (sgnn_tune prog_fusion; the heads' prog_lin_bn / prog_lin_add too), in training and in eval, and
asserts through sgnn_prog_plan that it takes the branch it is meant to take (fused AddTable, in-place JoinTable at an
aligned or unaligned column offset, head folded into its BatchNorm, or none of them).  The level tables are the
library's own (held bit-exact to the oracle in test_gpu_ops.py) and are handed to the interpreter as integer arrays.

Comparison rules
  * integer cases: outputs and all gradients bit for bit (test_prog_ref.py asserts the 2^24 bound on the sums of |terms|).
  * real cases, per checked tensor: err = max |y - ref64| / max |ref64| <= max(k x e_ref32, floor), where e_ref32
    is the same distance of the float32 interpreter from the float64 one and floor the per-op bar behind the tensor
    (prog_ref.floor_of: 2^-18 for sums, 2^-20 for BatchNorm outputs and running statistics).  k = prog_ref.BAR_K = 16:
    the smallest power of two that covers the worst err / e_ref32 measured with the fusions off, 10.8 (a head's bias
    gradient, itself at 1.3e-7); the fused runs meet the same k.  profiles/prog_fp64_ratios.txt holds the ratios.  test_prog_ref.py shows that six kinds of wrong executor move a checked tensor by at
    least 10 bars, and that no BatchNorm pre-activation of any case lies near zero (no element is excluded).
  * unwritten elements: both arenas, every gext and every parameter-gradient buffer are pre-filled with NaN.
  * inference layout (training | 2, liveness-packed arena): outputs bit-identical to the eval outputs of the training
    layout.
Set SGNN_PROG_RATIOS to a file name to have every measured ratio appended to it."""
import os

import numpy as np
import pytest
import torch

import prog_cases as C
import prog_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ('prog_fusion', 'prog_lin_bn', 'prog_lin_add', 'conv_small', 'conv_small_rows', 'conv_unrolled', 'conv_wide_epi')
CASES = dict((c.name, c) for c in C.cases())


def _lib():
    from sgnn_amd import _lib as L
    return L


@pytest.fixture
def tune():
    L = _lib()
    saved = dict((k, L.tune(k)) for k in KNOBS)

    def set_(**kv):
        for k in KNOBS:
            L.tune(k, kv.get(k, saved[k]))
    try:
        yield set_
    finally:
        for k, v in saved.items():
            L.tune(k, v)


class Levels(object):
    """The level tables of a case as integer arrays (prog_ref.Geometry), taken from the library's own grids and stride-2
    rulebooks.  A case without sites gets zero-row tables and calls nothing."""

    def __init__(self, case):
        from sgnn_amd.scn.metadata import Grid, build_down2, coords_from_locs
        coords = case.coords()
        nlev = case.net.nlev
        if coords.shape[0] == 0:
            z = lambda *shape: torch.zeros(shape, dtype=torch.long)
            self.geom = R.Geometry(coords, [z(27, 0)] * nlev, [z(8, 0)] * (nlev - 1), [z(0)] * (nlev - 1))
            return
        grids, downs = [Grid(coords_from_locs(torch.from_numpy(coords), torch.device('cuda')))], []
        for _ in range(nlev - 1):
            downs.append(build_down2(grids[-1]))
            grids.append(downs[-1].coarse)
        nbr = [g.subm_table().view(27, g.ld)[:, :g.n].cpu() for g in grids]
        children = [d.children.view(8, d.ldc)[:, :d.coarse.n].cpu() for d in downs]
        parent = [d.parent.cpu() for d in downs]
        self.geom = R.Geometry(coords, nbr, children, parent)


def _ptrs(values):
    return np.ascontiguousarray(np.array([0 if v is None else v for v in values] + [0], dtype=np.uint64))


def _pad_rows(t, n, fill):
    """t with its rows padded to n (at least one row of storage, so that the pointer is never NULL)."""
    out = torch.full((max(n, 1),) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out.cuda()


def _table(t, K, ld):
    """(K, n) integer table -> int32 [K][ld] on the device, -1 past the n columns."""
    out = torch.full((K, ld), -1, dtype=torch.int32)
    out[:, :t.shape[1]] = t.int()
    return out.cuda()


def level_tables(net, geom, rows, live, capacity=None, counts=None):
    """(lev_n, lev_ld, the five pointer tables of sgnn_prog_forward, the device tensors behind them) for `rows` rows per
    class; capacity: the live counts (or `counts`) go to device memory through lev_cnt."""
    ncls, nlev = net.n_classes, net.nlev
    lev_n = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    lev_ld = np.zeros(ncls, dtype=np.int64)
    for l in range(nlev):
        lev_ld[l] = (max(rows[l], 1) + 255) // 256 * 256
    nbr = [_table(geom.nbr[l], 27, int(lev_ld[l])) for l in range(nlev)]
    children = [_table(geom.children[l], 8, int(lev_ld[l + 1])) for l in range(nlev - 1)]
    ptable, parent = [], []
    for l in range(nlev - 1):
        pt = torch.full((8, int(lev_ld[l])), -1, dtype=torch.int32)
        for k in range(8):
            j = (geom.children[l][k] >= 0).nonzero()[:, 0]
            pt[k, geom.children[l][k][j]] = j.int()
        ptable.append(pt.cuda())
        parent.append(_pad_rows(geom.parent[l].int(), rows[l], 0))
    pad = lambda v: [t.data_ptr() for t in v] + [0] * (ncls - len(v))
    cnt = []
    if capacity:
        cnt = [torch.tensor([live[c] if counts is None else counts[c]], dtype=torch.int64, device='cuda') for c in range(ncls)]
    held = (nbr, children, ptable, parent, cnt)
    return lev_n, lev_ld, [_ptrs(pad(v)) for v in held], held


def capacity_rows(net, live, capacity):
    rows = [int(capacity * r) + 5 for r in live]
    if 'child' in net.class_ids:
        rows[net.class_ids['child']] = 8 * rows[0]
    return rows


def execute(case, lv, data, training, infer=False, capacity=None, counts=None):
    """One forward (+ backward) call under the current switches.  capacity: factor by which every rows class is
    over-allocated (lev_n = capacities, the live counts in device memory through lev_cnt; counts overrides them).
    Returns a dict of CPU tensors: 'bufs' {buffer: all rows} (the kept buffers; every buffer the layout stores on its
    own when nothing is fused), 'gparams', 'gext', 'params', 'live' {rows class: live rows}."""
    L = _lib()
    net, geom = case.net, lv.geom
    params, ext, idx, gouts = data
    live = case.rows(geom)
    ncls, nops, nbuf, n_ext, nlev = net.n_classes, len(net.ops), len(net.bufs), net.n_ext, net.nlev
    rows = list(live)
    if capacity:
        rows = capacity_rows(net, live, capacity)
    lev_n, lev_ld, tabs, held = level_tables(net, geom, rows, live, capacity, counts)
    nan = float('nan')
    P = [p.cuda().clone() for p in params]
    PG = [None if kind in ('rm', 'rv') else torch.full_like(p, nan) for p, (kind, _) in zip(P, net.slots)]
    E = [_pad_rows(e, rows[net.bufs[b][0]], nan) for b, e in enumerate(ext)]
    GE = [None if b in case.gext_null else torch.full_like(e, nan) for b, e in enumerate(E)]
    I = [_pad_rows(i.int(), rows[0], -1) for i in idx]
    keep = np.zeros(nbuf, dtype=np.int32)
    keep[case.keep] = 1
    ops, opf, bufs = net.ops_np, net.opf_np, net.bufs_np
    qa = (ops.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data, ncls, keep.ctypes.data)
    total = L.query('sgnn_prog_arena_floats', *qa, 0)
    fwd_total = L.query('sgnn_prog_arena_floats', *qa, 2 if infer else 1)
    assert total >= 0 and 0 <= fwd_total <= total
    wsb = L.query('sgnn_prog_ws_bytes', ops.ctypes.data, nops, lev_n.ctypes.data, ncls)
    arena = torch.full((max(fwd_total, 1),), nan, device='cuda')
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    pp, ep, ip = _ptrs([p.data_ptr() for p in P]), _ptrs([e.data_ptr() for e in E]), _ptrs([i.data_ptr() for i in I])
    flags = int(training) | (2 if infer else 0)
    L.call('sgnn_prog_forward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, len(P), ep.ctypes.data, ip.ctypes.data, len(I), arena.data_ptr(),
           fwd_total, keep.ctypes.data, flags, None, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    plan = C.read_plan(L.query, case, rows)
    plain = not infer and all(plan['root'][b] == b for b in range(nbuf)) and max(plan['add_dst'] + [-1]) < 0
    out = {'bufs': {}, 'live': live if counts is None else list(counts)}
    for b in range(n_ext, nbuf):
        if not (keep[b] or plain):
            continue
        off = L.query('sgnn_prog_buffer_offset', *qa, int(infer), b)
        assert off >= 0, b
        r, ch = rows[bufs[b, 0]], int(bufs[b, 1])
        out['bufs'][b] = arena[off:off + r * ch].view(r, ch).cpu()
    out['params'] = [p.cpu() for p in P]
    if infer:
        return out
    garena = torch.full((max(total, 1),), nan, device='cuda')
    G = dict((b, _pad_rows(g, rows[net.bufs[b][0]], nan)) for b, g in gouts.items())
    gp = _ptrs([0 if b not in G else G[b].data_ptr() for b in range(nbuf)])
    pgp = _ptrs([None if g is None else g.data_ptr() for g in PG])
    gep = _ptrs([None if g is None else g.data_ptr() for g in GE])
    L.call('sgnn_prog_backward', ops.ctypes.data, opf.ctypes.data, nops, bufs.ctypes.data, nbuf, n_ext, lev_n.ctypes.data,
           lev_ld.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
           tabs[4].ctypes.data, ncls, pp.ctypes.data, pgp.ctypes.data, len(P), ep.ctypes.data, gep.ctypes.data,
           ip.ctypes.data, len(I), arena.data_ptr(), garena.data_ptr(), total, gp.ctypes.data, keep.ctypes.data,
           int(training), ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    out['gparams'] = [None if g is None else g.cpu() for g in PG]
    out['gext'] = [None if g is None else g.cpu()[:ext[b].shape[0]] for b, g in enumerate(GE)]
    return out


def _log(line):
    path = os.environ.get('SGNN_PROG_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def compare(case, got, ref, ref32, training, tag, data):
    """Every kept (or separately stored) buffer, every parameter gradient, every wanted input gradient and the running
    statistics against the fp64 run; returns the failures as a list of strings."""
    net = case.net
    pairs = [('buf%d' % b, y[:ref['bufs'][b].shape[0]], ref['bufs'][b], ref32['bufs'][b] if ref32 else None)
             for b, y in got['bufs'].items()]
    for s, g in enumerate(got['gparams']):
        if g is not None:
            pairs.append(('dparam%d' % s, g, ref['gparams'][s], ref32['gparams'][s] if ref32 else None))
    for b, g in enumerate(got['gext']):
        if g is not None:
            pairs.append(('dext%d' % b, g, ref['gext'][b], ref32['gext'][b] if ref32 else None))
    for s, (kind, _) in enumerate(net.slots):
        if kind in ('rm', 'rv'):
            want = ref['running'][s] if training else data[0][s].double()
            pairs.append(('running%d' % s, got['params'][s], want, ref32['running'][s] if training else data[0][s]))
        else:
            assert torch.equal(got['params'][s], data[0][s]), 'parameter slot %d was written' % s
    bad = []
    for name, y, want, want32 in pairs:
        if case.integer:
            if not torch.equal(y.double(), want):
                bad.append('%s %s: %d of %d values differ' % (tag, name, int((y.double() != want).sum()), want.numel()))
            continue
        err, e32 = R.max_norm_error(y, want), R.max_norm_error(want32, want)
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float('inf'))
        bar = R.bar(e32, R.floor_of(name, net.ops))
        _log('%-28s %-34s %-10s err %.3e  e_ref32 %.3e  ratio %8.3f  bar %.3e' % (case.name, tag, name, err, e32, ratio,
                                                                                   bar))
        if not err <= bar:
            bad.append('%s %s: err %.3e > bar %.3e (e_ref32 %.3e, ratio %.2f)' % (tag, name, err, bar, e32, ratio))
    for s in case.zero_slots:
        if not bool((got['gparams'][s] == 0).all()):
            bad.append('%s dparam%d: not exactly zero although no gradient reaches it' % (tag, s))
    return bad


@pytest.mark.parametrize('name', C.case_names())
def test_executor_against_fp64_interpreter(tune, name):
    L = _lib()
    case = CASES[name]
    lv = Levels(case)
    data = case.data(lv.geom)
    params, ext, idx, gouts = data
    net = case.net
    rows = case.rows(lv.geom)
    if case.empty:
        assert max(rows[:net.nlev]) == 0
    knobs = dict(case.knobs or {})
    has_head = any(o[0] == C.OP_LINEAR for o in net.ops)
    settings = [dict(prog_fusion=1), dict(prog_fusion=0)]
    if has_head:
        settings += [dict(prog_fusion=1, prog_lin_bn=0), dict(prog_fusion=1, prog_lin_bn=0, prog_lin_add=0)]
    bad = []
    for training in (True, False):
        kw = dict(idx=idx, training=training, gouts=gouts)
        args = (net.ops_np, net.bufs_np, net.opf_np, net.n_ext, rows, lv.geom, params, ext)
        ref = R.run(*args, **kw)
        ref32 = None if case.integer else R.run(*args, dtype=torch.float32, **kw)
        eval_out = None
        for st in settings:
            tune(**dict(knobs, **st))
            tag = '%s fusion=%d lin_bn=%d lin_add=%d' % ('train' if training else 'eval', st['prog_fusion'],
                                                         st.get('prog_lin_bn', 1), st.get('prog_lin_add', 1))
            want = C.expected_plan(case, st['prog_fusion'])
            if not st.get('prog_lin_bn', 1):
                want['lin_bn'] = [-1] * len(net.ops)
            assert C.read_plan(L.query, case, rows) == want, tag
            got = execute(case, lv, data, training)
            bad += compare(case, got, ref, ref32, training, tag, data)
            if not training and eval_out is None:
                eval_out = got
        if not training:                     # inference layout under the default switches of the case
            tune(**knobs)
            inf = execute(case, lv, data, False, infer=True)
            for b in case.keep:
                if not torch.equal(inf['bufs'][b], eval_out['bufs'][b]):
                    bad.append('inference layout: buffer %d differs from the training layout in eval' % b)
    assert not bad, '\n'.join(bad)


CAPACITY_CASES = ['join_int_8_12', 'nested_joins', 'two_readers', 'stage_int', 'residual_8_12', 'join_bn_5_7', 'join_bn_5_8',
                  'u3', 'stage_lin_add']


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('name', CAPACITY_CASES)
def test_capacity_mode_equals_the_exact_size_run(tune, name, fused):
    """lev_n = about 1.5 x the true rows, the true counts in device memory (lev_cnt): the live rows of every output and
    every parameter and input gradient are bit-identical to the exact-size run, and output rows past the count are
    untouched (still NaN).  Inputs, index arrays and output gradients past the count are NaN / -1."""
    case = CASES[name]
    lv = Levels(case)
    data = case.data(lv.geom)
    tune(**dict(case.knobs or {}, prog_fusion=fused))
    bad = []
    for training in (True, False):
        exact = execute(case, lv, data, training)
        cap = execute(case, lv, data, training, capacity=1.5)
        for b in case.keep:
            n = exact['live'][case.net.bufs[b][0]]
            y = cap['bufs'][b]
            assert y.shape[0] > n
            if not torch.equal(y[:n], exact['bufs'][b][:n]):
                bad.append('training=%s buffer %d: %d live values differ (max %g)' % (
                    training, b, int((y[:n] != exact['bufs'][b][:n]).sum()), float((y[:n] - exact['bufs'][b][:n]).abs().max())))
            if not bool(torch.isnan(y[n:]).all()):
                bad.append('training=%s buffer %d: rows past the count were written' % (training, b))
        for key in ('gparams', 'gext'):
            for k, (u, v) in enumerate(zip(cap[key], exact[key])):
                if u is not None and not torch.equal(u, v):
                    bad.append('training=%s %s[%d]: %d values differ (max %g)' % (training, key, k, int((u != v).sum()),
                                                                                  float((u - v).abs().max())))
    assert not bad, '\n'.join(bad)


def test_zero_live_rows_at_nonzero_capacity(tune):
    """Every device row count is zero while the capacities are not (a level the network generated no sites for): no
    error, no output row written, every parameter gradient exactly zero (no NaN read from the unwritten arenas)."""
    case = CASES['u3']
    lv = Levels(case)
    data = case.data(lv.geom)
    for fused in (1, 0):
        tune(prog_fusion=fused)
        got = execute(case, lv, data, True, capacity=1.5, counts=[0] * case.net.n_classes)
        for b in case.keep:
            assert bool(torch.isnan(got['bufs'][b]).all()), (fused, b)
        for s, g in enumerate(got['gparams']):
            assert g is None or bool((g == 0).all()), (fused, s, g.flatten()[:4])


def test_gradient_for_an_in_place_join_input_is_refused(tune):
    """A caller's gradient (gout) for a buffer that lives as a column range of a JoinTable output and is not kept has no
    contiguous storage to be copied into: the executor must refuse the call instead of spreading it over the rows."""
    from sgnn_amd._lib import SgnnError
    case = CASES['join_int_8_12']
    lv = Levels(case)
    params, ext, idx, gouts = case.data(lv.geom)
    plan = C.expected_plan(case, 1)
    view = [b for b in range(len(case.net.bufs)) if plan['root'][b] != b][0]
    gouts = dict(gouts)
    gouts[view] = torch.ones(lv.geom.n[0], case.net.bufs[view][1])
    tune(prog_fusion=1)
    with pytest.raises(SgnnError):
        execute(case, lv, (params, ext, idx, gouts), True)
