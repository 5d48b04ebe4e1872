"""The fp64 program interpreter of tests/prog_ref.py, on the CPU alone: it agrees with the oracle's modules on compiled
scn containers, the cases of tests/prog_cases.py respect what the comparison rules of test_gpu_prog_fp64.py assume
(integer sums below 2^24, no BatchNorm pre-activation near zero), the bars are tight enough to notice six kinds of
wrong executor, and every case takes the plan it is meant to take (sgnn_prog_plan is host-only)."""
import numpy as np
import pytest
import torch

import conv_ref
import bn_ref
import prog_cases as C
import prog_ref as R


# ---- oracle agreement ----

def _stack(s):
    return s.Sequential().add(s.SubmanifoldConvolution(3, 6, 8, 3, False)).add(s.BatchNormReLU(8)) \
        .add(s.Convolution(3, 8, 12, 2, 2, False)).add(s.BatchNormReLU(12)).add(s.SubmanifoldConvolution(3, 12, 12, 3, False))


def _fcn(s):
    return s.Sequential().add(s.FullyConvolutionalNet(3, 1, [6, 8, 12], True)).add(s.BatchNormReLU(26))


@pytest.mark.parametrize('build,cin', [(_stack, 6), (_fcn, 6)])
@pytest.mark.parametrize('training', [True, False])
def test_interpreter_agrees_with_the_oracle_modules(build, cin, training):
    import scn_oracle as oscn
    import sgnn_amd.scn as scn
    from sgnn_amd.scn.program import Program
    gen = torch.Generator().manual_seed(3)
    hm = build(scn)
    for p in hm.parameters():
        p.data = torch.randn(p.shape, generator=gen) * (0.2 if p.dim() > 1 else 0.5) + (1.0 if p.dim() == 1 else 0.0)
    for n, b in hm.named_buffers():
        b.data = torch.rand(b.shape, generator=gen) + (0.5 if n.endswith('var') else -0.5)
    om = build(oscn).double()
    om.load_state_dict(dict((k, v.double()) for k, v in hm.state_dict().items()))
    om.train(training)
    prog = Program([hm], cin)
    rng = np.random.default_rng(5)
    cells = rng.permutation(np.nonzero(rng.random(12 ** 3) < 0.3)[0])
    coords = np.stack([cells // 144, (cells // 12) % 12, cells % 12, np.zeros_like(cells)], 1).astype(np.int64)
    x = torch.randn(len(cells), cin, generator=gen, dtype=torch.float64)
    geom = R.oracle_geometry(coords, prog.nlev)
    rows = geom.n
    params = [getattr(m, nm).detach() for m, nm in prog.slots]
    dy = torch.randn(rows[prog.bufs[prog.out][0]], prog.bufs[prog.out][1], generator=gen, dtype=torch.float64)
    got = R.run(prog.ops_np, prog.bufs_np, prog.opf_np, prog.n_ext, rows, geom, params, [x], training=training,
                gouts={prog.out: dy})
    xo = x.clone().requires_grad_(True)
    yo = om(oscn.InputLayer(3, [12, 12, 12], mode=0)([torch.from_numpy(coords), xo])).features
    names = dict((id(m), n) for n, m in hm.named_modules())
    opar, obuf = dict(om.named_parameters()), dict(om.named_buffers())
    grads = torch.autograd.grad((yo * dy).sum(), [xo] + list(opar.values()))
    ograd = dict(zip(opar.keys(), grads[1:]))
    close = lambda a, b: R.max_norm_error(a, b) <= 1e-9      # (the program carries eps as fp32: 1e-4f)
    assert close(got['bufs'][prog.out], yo.detach())
    assert close(got['gext'][0], grads[0])
    seen = 0
    for s, (m, nm) in enumerate(prog.slots):
        key = names[id(m)] + '.' + nm
        if prog.grad_slot[s]:
            assert close(got['gparams'][s], ograd[key]), key
            seen += 1
        elif training:      # the interpreter takes the program's fp32 momentum (0.9f, as the kernels do), the oracle 0.9
            assert torch.allclose(got['running'][s], obuf[key], rtol=1e-6, atol=1e-7), key
    assert seen == len(opar)


# ---- the cases ----

@pytest.fixture(scope='module')
def refs():
    """name -> (case, geometry, data, fp64 run in training mode), computed once."""
    out = {}
    for c in C.cases():
        if c.knobs is not None:          # same program and data as the case it repeats under other kernel switches
            continue
        geom = R.oracle_geometry(c.coords(), c.net.nlev)
        data = c.data(geom)
        out[c.name] = (c, geom, data, _run(c, geom, data))
    return out


def _run(c, geom, data, **kw):
    params, ext, idx, gouts = data
    n = c.net
    return R.run(n.ops_np, n.bufs_np, n.opf_np, n.n_ext, c.rows(geom), geom, params, ext, idx, gouts=gouts, **kw)


def test_case_names_are_unique_and_sizes_small():
    names = C.case_names()
    assert len(set(names)) == len(names)
    for c in C.cases():
        geom = R.oracle_geometry(c.coords(), c.net.nlev)
        assert max(c.rows(geom)) <= 4096, c.name
        types = set(o[0] for o in c.net.ops)
        assert c.integer == (not (types & {C.OP_BN, C.OP_LINEAR})), c.name


def test_integer_cases_stay_below_2_to_24(refs):
    """Every value and every gradient of an integer case is a sum of integer terms whose |terms| add up to less than 2^24:
    fp32 is exact in any summation order, so the executor must match the fp64 interpreter bit for bit."""
    n_int = 0
    for name, (c, geom, data, ref) in refs.items():
        if not c.integer:
            continue
        n_int += 1
        mag = _run(c, geom, data, abs_terms=True)
        for what, vals, mags in (('buffer', ref['bufs'], mag['bufs']), ('dparam', ref['gparams'], mag['gparams']),
                                 ('dext', ref['gext'], mag['gext'])):
            for k, (v, m) in enumerate(zip(vals, mags)):
                if v is None or not v.numel():
                    continue
                assert float(m.max()) < conv_ref.EXACT_LIMIT, '%s %s %d: sum of |terms| %g' % (name, what, k, float(m.max()))
                assert bool((m >= v.abs()).all()) and bool((v == v.round()).all())
        checked = [ref['bufs'][b] for b in c.keep] + [g for g in ref['gparams'] if g is not None]
        assert all(float(v.abs().max()) > 0 for v in checked), name      # the thinned-out data still reaches everything
    assert n_int >= 8


def test_no_batchnorm_preactivation_near_zero(refs):
    """ReLU guard: the gradients of a BatchNormReLU network jump where a pre-activation changes sign, so a comparison of
    gradients is only meaningful if the executor takes every ReLU decision the reference takes.  Held for every real
    case (training and eval): no pre-activation of the fp64 reference lies within 64 x the forward bar of the BatchNorm
    apply pass (bn_ref.APPLY_BAR x (|xhat gamma| + |beta|)) of zero.  No element is excluded anywhere."""
    n_real = 0
    for name, (c, geom, data, ref) in refs.items():
        if c.integer:
            continue
        n_real += 1
        for training, r in ((True, ref), (False, _run(c, geom, data, training=False))):
            for op, t in r['pre'].items():
                margin = (t.abs() / (64 * bn_ref.APPLY_BAR * r['pre_mag'][op]).clamp_min(1e-300))
                assert t.numel() == 0 or float(margin.min()) > 1.0, \
                    '%s (training=%s) op %d: a pre-activation at %.3g of the guard' % (name, training, op, float(margin.min()))
    assert n_real >= 8


# ---- sensitivity: the bars notice a wrong executor ----

def _quantities(c, r):
    q = dict(('buf%d' % b, r['bufs'][b]) for b in c.keep)
    q.update(('dparam%d' % s, g) for s, g in enumerate(r['gparams']) if g is not None and c.net.slots[s][0] not in ('rm', 'rv'))
    q.update(('dext%d' % b, g) for b, g in enumerate(r['gext']) if g is not None and b not in c.gext_null)
    q.update(('running%d' % s, v) for s, v in r['running'].items())
    return q


@pytest.mark.parametrize('mutation,case', [
    ('add_drops_addend', 'residual_8_12'), ('join_swaps_columns', 'join_bn_5_7'),
    ('second_reader_gradient_dropped', 'residual_8_12'), ('running_stats_in_training', 'residual_8_12'),
    ('unpool_gradient_drops_a_child', 'join_bn_5_7'), ('head_data_gradient_dropped', 'stage_lin_bn'),
    ('add_drops_addend', 'two_readers'), ('join_swaps_columns', 'join_int_8_12'),
    ('second_reader_gradient_dropped', 'two_joins_read_one_buffer'), ('unpool_gradient_drops_a_child', 'join_int_8_12')])
def test_each_mutation_moves_a_checked_quantity_ten_bars(refs, mutation, case):
    """A mutated interpreter stands in for an executor with that bug.  Real cases: some checked tensor moves by at least
    10 x its bar (prog_ref.bar: BAR_K x the fp32 interpreter's own error, floored at 2^-18).  Integer cases are compared
    bit for bit: any difference is a failure."""
    c, geom, data, ref = refs[case]
    bad = _quantities(c, _run(c, geom, data, mutate=mutation))
    good = _quantities(c, ref)
    if c.integer:
        assert any(not torch.equal(bad[k], good[k]) for k in good)
        return
    f32 = _quantities(c, _run(c, geom, data, dtype=torch.float32))
    worst = max(R.max_norm_error(bad[k], good[k]) / R.bar(R.max_norm_error(f32[k], good[k]), R.floor_of(k, c.net.ops)) for k in good if k in bad)
    assert worst >= 10.0, worst


def test_the_float32_interpreter_is_a_sane_yardstick(refs):
    for name, (c, geom, data, ref) in refs.items():
        if c.integer:
            continue
        good, f32 = _quantities(c, ref), _quantities(c, _run(c, geom, data, dtype=torch.float32))
        for k in good:
            assert R.max_norm_error(f32[k], good[k]) < 2.0 ** -14, (name, k)


# ---- plans (host-only: no GPU needed) ----

def test_every_case_takes_the_plan_it_is_meant_to_take(refs):
    """Needs the built library (build() precedes the suite, as for test_cabi_symbols.py) but no GPU: sgnn_prog_plan is
    host code.  Also shows that between them the cases reach every planned branch and its absence; a storage root is
    never itself a view (case nested_joins), so the multi-step walk of make_plan's root resolution is never taken."""
    from sgnn_amd import _lib
    saved = dict((k, _lib.tune(k)) for k in ('prog_fusion', 'prog_lin_bn', 'prog_lin_add'))
    shown = set()
    try:
        for name, (c, geom, data, ref) in refs.items():
            for fused in (1, 0):
                _lib.tune('prog_fusion', fused)
                got, want = C.read_plan(_lib.query, c, c.rows(geom)), C.expected_plan(c, fused)
                assert got == want, (name, fused, dict((k, (got[k], want[k])) for k in want if got[k] != want[k]))
                if not fused:
                    continue
                shown.add('add_dst' if max(got['add_dst']) >= 0 else 'no add_dst')
                shown.add('lin_bn' if max(got['lin_bn']) >= 0 else 'no lin_bn')
                shown.add('join_view' if max(got['join_view']) else 'no join_view')
                if any(v and got['col'][c.net.ops[i][2]] % 4 for i, v in enumerate(got['join_view'])):
                    shown.add('unaligned join_view')
                # a storage root is never itself a view: make_plan accepts only convolution, BatchNorm and UnPooling
                # producers for an in-place JoinTable input, so a join buffer cannot live inside another join buffer
                assert all(got['root'][r] == r for r in got['root'])
            _lib.tune('prog_fusion', 1)
            _lib.tune('prog_lin_bn', 0)
            assert max(C.read_plan(_lib.query, c, c.rows(geom))['lin_bn']) == -1
            _lib.tune('prog_lin_bn', saved['prog_lin_bn'])
    finally:
        for k, v in saved.items():
            _lib.tune(k, v)
    assert shown >= {'add_dst', 'no add_dst', 'lin_bn', 'no lin_bn', 'join_view', 'no join_view', 'unaligned join_view'}


# ---- the bf16 executor's yardstick: the rounding interpreter (run(..., storage='bf16')), CPU alone ----

@pytest.fixture(scope='module')
def refs_bf16():
    """name -> (case, geometry, data for the bf16 executor, fp64 eval run, rounding-interpreter eval run), computed once.
    The fp64 run of an exact case is fed the externals rounded to bf16 (their own values are no bf16 values)."""
    out = {}
    for c in C.cases():
        if c.knobs is not None:
            continue
        geom = R.oracle_geometry(c.coords(), c.net.nlev)
        data = c.data(geom, bf16=True)
        fed = (data[0], R.bf16_externals(data[1])) + tuple(data[2:]) if c.integer else data
        out[c.name] = (c, geom, data, _fwd(c, geom, fed), _fwd(c, geom, data, storage='bf16'))
    return out


def _fwd(c, geom, data, **kw):
    params, ext, idx, _ = data
    n = c.net
    return R.run(n.ops_np, n.bufs_np, n.opf_np, n.n_ext, c.rows(geom), geom, params, ext, idx, training=False, **kw)


def test_round_bf16_is_torchs_rounding_without_the_float32_step():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=gen)
    assert torch.equal(R.round_bf16(x.double()), x.bfloat16().double())
    one, ulp = 1.0, 2.0 ** -7
    ties = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, -(one + ulp / 2), one + ulp / 2 + 2.0 ** -40, 0.0, 256.0, 257.0], dtype=torch.float64)
    want = torch.tensor([one, one + 2 * ulp, -one, one + ulp, 0.0, 256.0, 256.0], dtype=torch.float64)
    assert torch.equal(R.round_bf16(ties), want)
    # float64 -> float32 -> bf16 would round 1 + ulp/2 + 2^-40 to a tie first and then down to 1
    assert float(ties[3].float().bfloat16()) == one


def test_exact_cases_store_nothing_but_bf16_values(refs_bf16):
    """The exact cases of test_gpu_prog_bf16.py (the integer cases, under data(geom, bf16=True)): the externals are
    +-(1 + 2^-8), which every reader must round to +-1; from there on every value the fp64 interpreter computes is a bf16
    value, so no executor rounds again, whatever its plan, and the rounding interpreter (fed the unrounded externals)
    reproduces the fp64 one (fed the rounded ones) bit for bit; the sums of |terms| stay below 2^24, so fp32
    accumulation is exact in any order.  A condition on the inputs, not a tolerance."""
    n_exact = 0
    for name, (c, geom, data, r64, rbf) in refs_bf16.items():
        if not c.integer:
            continue
        n_exact += 1
        assert all(not torch.equal(e.bfloat16().float(), e) for e in data[1]), name
        mag = _fwd(c, geom, (data[0], R.bf16_externals(data[1])) + tuple(data[2:]), abs_terms=True)
        for b, (v, m) in enumerate(zip(r64['bufs'], mag['bufs'])):
            assert torch.equal(R.round_bf16(v), v), '%s buffer %d: %d values are no bf16 values' % (
                name, b, int((R.round_bf16(v) != v).sum()))
            assert b < c.net.n_ext or torch.equal(rbf['bufs'][b], v), (name, b)
            assert not v.numel() or float(m.max()) < conv_ref.EXACT_LIMIT, (name, b)
        for p in data[0]:
            assert torch.equal(R.round_bf16(p.double()), p.double()), name
        assert all(float(r64['bufs'][b].abs().max()) > 0 for b in c.keep), name
    assert n_exact >= 12


BF16_BRANCHES = ('fused add', 'join view at byte 0 mod 16', 'join view at byte 4 mod 16', 'join view at byte 8 mod 16',
                 'join view at byte 12 mod 16', 'join refused for odd cin', 'copying join writes at byte 4 mod 16',
                 'shadowed external', 'external read only by CONCAT_IN', 'head on a bf16 buffer')


def bf16_branches(c, plan, plan32):
    """The branches of forward_bf16 a case reaches under `plan` (sgnn_prog_plan mode 3, fusions on)."""
    net, out = c.net, set()
    if max(plan['add_dst']) >= 0:
        out.add('fused add')
    for i, o in enumerate(net.ops):
        if o[0] == C.OP_JOIN and plan['join_view'][i]:
            out.add('join view at byte %d mod 16' % (2 * plan['col'][o[2]] % 16))
        if o[0] == C.OP_JOIN and not plan['join_view'][i]:
            if plan32['join_view'][i] and o[6] % 2:
                out.add('join refused for odd cin')
            if 2 * o[6] % 16 == 4:
                out.add('copying join writes at byte 4 mod 16')
        if o[0] == C.OP_LINEAR:
            out.add('head on a bf16 buffer')
    readers = dict((b, set(o[0] for o in net.ops if b in (o[1], o[2], o[8]))) for b in range(net.n_ext))
    for b, r in readers.items():
        if r - {C.OP_CONCAT_IN}:
            out.add('shadowed external')
        elif r:
            out.add('external read only by CONCAT_IN')
    return out


def test_every_case_takes_its_bf16_plan(refs):
    """sgnn_prog_plan mode 3 (host code): the plan of the bf16 layout is the fp32 plan, except that a JoinTable whose
    first input has an odd channel count is not in place and that row strides are round8(channels) bf16 elements (fp32
    rows of their own width for LINEAR outputs).  Between them the cases reach every branch of BF16_BRANCHES.  An
    in-place view never lies inside another (see test_every_case_takes_the_plan_it_is_meant_to_take), so the column
    6 + 12 of nested_*_6_12_8 is written by the copying JoinTable, not resolved through two views."""
    from sgnn_amd import _lib
    saved = _lib.tune('prog_fusion')
    shown = {}
    try:
        for name, (c, geom, data, ref) in refs.items():
            rows = c.rows(geom)
            for fused in (1, 0):
                _lib.tune('prog_fusion', fused)
                got, want = C.read_plan(_lib.query, c, rows, 3), C.expected_plan(c, fused, bf16=True)
                assert got == want, (name, fused, dict((k, (got[k], want[k])) for k in want if got[k] != want[k]))
                heads = set(o[3] for o in c.net.ops if o[0] == C.OP_LINEAR)
                assert all(v % 8 == 0 for b, v in enumerate(got['ld']) if got['root'][b] not in heads), name
                if fused and not c.empty:
                    for br in bf16_branches(c, got, C.read_plan(_lib.query, c, rows, 0)):
                        shown.setdefault(br, name)
    finally:
        _lib.tune('prog_fusion', saved)
    _lib.tune('prog_fusion', 1)
    try:
        for name in ('join_bn_5_7', 'join_bn_5_8'):
            c, geom = refs[name][:2]
            assert max(C.read_plan(_lib.query, c, c.rows(geom), 0)['join_view']) == 1, name
            assert max(C.read_plan(_lib.query, c, c.rows(geom), 3)['join_view']) == 0, name
    finally:
        _lib.tune('prog_fusion', saved)
    print('\n'.join('%-40s %s' % kv for kv in sorted(shown.items())))
    assert set(shown) >= set(BF16_BRANCHES), set(BF16_BRANCHES) - set(shown)


def _applies(mutation, net):
    """add / join mutations: the program holds the op; external_not_rounded: an op other than CONCAT_IN reads an external."""
    if mutation == 'external_not_rounded':
        return any(o[0] != C.OP_CONCAT_IN and 0 <= b < net.n_ext for o in net.ops for b in (o[1], o[2]))
    return any(o[0] == {'add_drops_addend': C.OP_ADD, 'join_swaps_columns': C.OP_JOIN}[mutation] for o in net.ops)


@pytest.mark.parametrize('mutation', ['add_drops_addend', 'join_swaps_columns', 'external_not_rounded'])
def test_bf16_mutation_changes_every_exact_case_it_applies_to(refs_bf16, mutation):
    """Exact cases are compared bit for bit: the mutated rounding interpreter must differ from the fp64 run in a kept
    buffer of every exact case it applies to.  (batch_stats_in_eval needs BatchNorm, which no exact case has.)"""
    n = 0
    for name, (c, geom, data, r64, rbf) in refs_bf16.items():
        if not c.integer or not _applies(mutation, c.net):
            continue
        n += 1
        bad = _fwd(c, geom, data, storage='bf16', mutate=mutation)
        assert any(not torch.equal(bad['bufs'][b], r64['bufs'][b]) for b in c.keep), name
    assert n >= 4


def _bars_moved(c, geom, data, r64, rbf, mutation, against):
    bad = _fwd(c, geom, data, storage='bf16', mutate=mutation)
    return max(R.max_norm_error(bad['bufs'][b], against['bufs'][b]) / R.bar_bf16(R.max_norm_error(rbf['bufs'][b], r64['bufs'][b]))
               for b in c.keep)


@pytest.mark.parametrize('mutation,case', [('add_drops_addend', 'residual_8_12'), ('join_swaps_columns', 'join_bn_6_12'),
                                           ('join_swaps_columns', 'u3'), ('batch_stats_in_eval', 'residual_8_12'),
                                           ('batch_stats_in_eval', 'stage_lin_bn')])
def test_bf16_mutation_moves_a_real_case_two_bars(refs_bf16, mutation, case):
    """A mutated rounding interpreter stands in for a bf16 executor with that bug: some kept tensor of a real case moves
    by at least 2 bars (prog_ref.bar_bf16) from the fp64 run.  batch_stats_in_eval is what a wrong choice of BatchNorm
    statistics looks like in eval, the only mode the bf16 executor has: running_stats_in_training itself changes
    nothing there (asserted)."""
    c, geom, data, r64, rbf = refs_bf16[case]
    assert _bars_moved(c, geom, data, r64, rbf, mutation, r64) >= 2.0
    same = _fwd(c, geom, data, storage='bf16', mutate='running_stats_in_training')
    assert all(torch.equal(same['bufs'][b], rbf['bufs'][b]) for b in c.keep)


def test_an_unrounded_external_changes_the_real_cases_too(refs_bf16):
    """external_not_rounded on real data is a sub-ulp change of the inputs that no tolerance tells from honest bf16
    rounding (it moved no real case by 2 bars when measured: at most 1.13 x 2^-8 / bar from the fp64 run, 1.63 from the
    rounding interpreter), so the exact cases carry its detection (above: their externals are no bf16 values).  As the
    rule for a mutation that hides asks, test_gpu_prog_bf16.py holds the real cases to the rounding interpreter as well,
    under the same bar.  Asserted here: the mutation is live on real data, it changes a kept tensor of some case."""
    worst = 0.0
    for name, (c, geom, data, r64, rbf) in refs_bf16.items():
        if not (c.integer or c.empty):
            worst = max(worst, _bars_moved(c, geom, data, r64, rbf, 'external_not_rounded', rbf))
    assert worst > 0.0
