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
