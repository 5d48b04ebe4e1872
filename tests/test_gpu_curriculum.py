"""The training step at the loss weights real training spends its time at: the curriculum of train.get_loss_weights
(trailing zeros, one fractional weight while a level fades in, an L1 weight of zero / a fraction / factor_l1_loss), held to
the CPU oracle in fp64 with the oracle's own fp32 run as the yardstick (tests/curriculum_ref.py), on both paths:
  classic   train.train_step with train.make_optimizer
  graph     train.GraphStep(teacher_forced=True, settle=False, keep_outputs=True): probe, eager capacity step, capture, replay
What only such weights reach: GraphStep._seg_cnts / _active_segments / _opt_step, the reached / cnt gating of
FlatAdam.step (sgnn_adam_flat's segment table), the weighted per-level fold of the fused loss (sgnn_loss_levels_*).

Stages S0..S4 come out of get_loss_weights itself (N = 2000, factor_l1_loss = 0.5); every stage runs on two batches, one of
which ('empty') leaves the last Refinement and the SurfacePrediction without a single site.  The oracle's masks are forced
into both paths (teacher volumes), so every site list must equal the oracle's bit for bit.

Bars.  Forward: logits / sdf within max(1e-4, 1.25 x oracle-fp32-vs-fp64), rms 5e-5 (tests/test_gpu_graphstep_parity.py).
Loss, total and per level: max(1e-4 |l64|, 2 |l32 - l64|); a zero-weight level is reported as -1 and adds nothing.
Gradients as Adam consumes them: every tensor of a reached segment within 3 e_ref + 5e-3 of its scale from fp64, at most
3 % of them beyond 2 e_ref + 1e-3 (e_ref: the fp32 oracle's own distance; that run meets the share by construction, a second
independent fp32 evaluation of the reference to confirm it with does not exist on the host).  A segment the oracle leaves
without a gradient must be ABSENT for the optimizer: grad None / no state (classic), step counter and moments untouched
(graph).  One Adam step at lr 1e-3 from zero moments: skipped segments bit-identical, reached ones against the fp64 Adam of
the fp64 gradient — the parameter delta over the entries with |g| > 100 (eps + e_ref x scale), within 2 x the yardstick of
curriculum_ref.adam_reference, where at most 20 % of a tensor's entries are excluded by that threshold; on the other tensors
(most of them at these sizes: one flipped ReLU in the oracle's fp32 run puts e_ref at 1e-2 and the threshold above the whole
tensor) the moments, read back as a gradient, against the gradient bar.  Host-only checks of the stage scan, of the reached
sets and of that 20 % cap run without a GPU."""
import numpy as np
import pytest
import torch

import curriculum_ref as R
from util import param_fill

gpu = pytest.mark.gpu
PHASES = ['probe (classic path)', 'eager capacity-mode step', 'capture + first replay', 'replay']
LR = 1e-3
DECAY_CASE = ('S2', 'empty')        # the one case that runs its optimizer step with weight_decay = 1e-2
REACHED = {'full': {'S0': 1, 'S1': 2, 'S2': 4, 'S3': 5, 'S4': 5}, 'empty': {'S0': 1, 'S1': 2, 'S2': 3, 'S3': 3, 'S4': 3}}


def report(msg):
    """One line to stdout and to the parity report the other oracle tests append to."""
    import test_gpu_configs as C
    C.report(msg)


# ---------------------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------------------
def test_stages_come_out_of_get_loss_weights():
    found = R.scan_stages()
    for s in R.STAGES:
        assert found[s], 'get_loss_weights(it, 4, %d, %g) never returns a stage %s vector' % (R.ITERS_PER_LEVEL, R.FACTOR_L1, s)
        w = R.stage_weights(s)
        assert R.classify(w) == s and w.dtype == np.float32 and w.shape == (5,)
    for s in ('S1', 'S3'):
        a, b = R.stage_weights(s), R.stage_weights(s, alt=True)
        assert R.classify(b) == s and not np.array_equal(a, b) and np.array_equal(a > 0, b > 0)
    assert R.FACTOR_L1 != 1.0 and float(R.stage_weights('S4')[-1]) == R.FACTOR_L1
    # with N = 400 the fade never starts (fade_level >= N - 20 + 20): no fractional vector at all
    from sgnn_amd.train import get_loss_weights
    assert all(float(v) in (0.0, 1.0, R.FACTOR_L1) for it in range(6 * 400) for v in get_loss_weights(it, 4, 400, R.FACTOR_L1))


def _oracle_params():
    import model_oracle as mo
    om = param_fill(mo.GenModel(8, R.DIMS, 1, 16, 16, 4, True, True, 1, 1), R.PARAM_SEED)
    return dict((n, p.detach().numpy().copy()) for n, p in om.named_parameters())


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_oracle_reached_sets_and_exclusion_cap(variant):
    """Oracle alone: every level the stage trains has sites ('full'), the reached sets are the reference's (a stage with
    zero weight or without input sites leaves its parameters at grad None), every reached gradient is non-zero, and the
    |g| threshold of the Adam-delta comparison leaves tensors on both sides of the 20 % cap (the others compare moments)."""
    params = _oracle_params()
    for s in R.STAGES:
        ora = R.oracle_stage(R.stage_weights(s), variant)
        want = R.SEGMENTS[:REACHED[variant][s]]
        assert [k for k in R.SEGMENTS if ora['reached'][k]] == list(want), (variant, s, ora['reached'])
        lw = ora['lw']
        for h in range(4):
            n = len(ora['f64']['occ'][h][0])
            runs = h == 0 or lw[h] > 0
            assert (n > 0) == bool(runs and not (variant == 'empty' and h == 3)), (variant, s, h, n)
            assert (ora['f64']['losses'][h] == -1) == (n == 0 or lw[h] == 0)
        assert all(np.isfinite(e) for e in ora['eref'].values())
        for wd in (0.0, 1e-2):
            ref = R.adam_reference(ora, params, LR, wd)
            under = [n for n, r in ref.items() if r['excluded'] <= 0.2]
            assert under and len(under) < len(ref), (variant, s, len(under), len(ref))
            assert all(r['scale'] > 0 for r in ref.values())
            assert max(ref[n]['yard'] for n in under) < 1e-3
        print('%s %s: oracle %.1f s, %d of %d reached tensors under the 20 %% exclusion cap, worst e_ref %.2e'
              % (variant, s, ora['seconds'], len(under), len(ref), max(ora['eref'].values())))


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _live(t, v=None):
    from sgnn_amd.scn.capacity import trim
    if not torch.is_tensor(t):
        return np.zeros((0, 4), dtype=np.int64), np.zeros((0, 1), dtype=np.float32)
    s = trim(t)
    n = int(s.shape[0])
    return s.cpu().numpy(), (None if v is None else v.detach()[:n].cpu().numpy())


def _device_batch(data):
    return {'input': [data['input'][0].cuda(), data['input'][1].cuda()], 'sdf': data['sdf'].cuda(),
            'known': data['known'].cuda(), 'hierarchy': [h.cuda() for h in data['hierarchy']]}


_BATCHES = {}


def _setup(ora, variant):
    """A fresh HIP model with the oracle's weights, the device batch and the oracle's masks as teacher volumes."""
    from sgnn_amd.model import GenModel
    hm = param_fill(GenModel(8, R.DIMS, 1, 16, 16, 4, True, True, 1, 1), R.PARAM_SEED).train().cuda()
    if variant not in _BATCHES:
        _BATCHES[variant] = _device_batch(ora['data'])
    return hm, _BATCHES[variant], [v.cuda() for v in R.teacher_volumes(ora)]


def _ref_layout(hm):
    """name -> function taking a tensor shaped like the parameter to a float64 array in the reference's layout."""
    conv = {}
    for n, p in hm.named_parameters():
        dense = getattr(p, '_sgnn_dense', None)
        conv[n] = (lambda t, d=dense: (d.to_torch(t) if d is not None else t).detach().cpu().double().numpy())
    return conv


def _params(hm):
    conv = _ref_layout(hm)
    return dict((n, conv[n](p.detach())) for n, p in hm.named_parameters())


def _check_forward(tag, ora, outputs):
    hsdf, hocc = outputs
    o32, o64 = ora['f32'], ora['f64']
    for h in range(5):
        if h < 4:
            hs, hv, os_, ov, dv, what = hocc[h][0], hocc[h][1], o32['occ'][h][0], o32['occ'][h][1], o64['occ'][h][1], 'level %d logits' % h
        else:
            hs, hv, os_, ov, dv, what = hsdf[0], hsdf[1], o32['sdf'][0], o32['sdf'][1], o64['sdf'][1], 'final sdf'
        sites, vals = _live(hs, hv)
        if len(os_) == 0:
            assert sites.shape[0] == 0, '%s: %s should have no site' % (tag, what)
            continue
        assert np.array_equal(sites, os_.numpy()), '%s: %s site list differs' % (tag, what)
        hv64, ov64, dv64 = vals.astype(np.float64).reshape(-1), ov.detach().double().numpy().reshape(-1), dv.detach().numpy().reshape(-1)
        e_h, e_o = np.abs(hv64 - dv64), np.abs(ov64 - dv64)
        assert e_h.max() <= max(1e-4, 1.25 * e_o.max()), (tag, what, e_h.max(), e_o.max())
        assert np.sqrt((e_h ** 2).mean()) <= 5e-5, (tag, what)


def _loss_bar(l64, l32):
    return max(1e-4 * abs(l64), 2 * abs(l32 - l64))


def _check_loss(tag, ora, loss, losses):
    o32, o64, lw = ora['f32'], ora['f64'], ora['lw']
    loss = float(loss.detach()) if torch.is_tensor(loss) else float(loss)
    assert abs(loss - o64['loss']) <= _loss_bar(o64['loss'], o32['loss']), (tag, loss, o64['loss'], o32['loss'])
    assert len(losses) == 5
    folded = 0.0
    for h in range(5):
        l64, l32 = o64['losses'][h], o32['losses'][h]
        got = losses[h] if isinstance(losses[h], (int, float)) else float(losses[h])
        if lw[h] == 0:
            assert isinstance(losses[h], int) and losses[h] == -1, '%s: level %d has weight 0 but reports %r' % (tag, h, losses[h])
        elif l64 == -1:         # weight > 0 but no site: skipped like a missing level (capacity mode: a device-side 0)
            assert got in (-1, 0.0), (tag, h, got)
        else:
            assert abs(got - l64) <= _loss_bar(l64, l32), '%s: level %d term %r, fp64 %r, fp32 %r' % (tag, h, got, l64, l32)
            folded += float(lw[h]) * got
    # the total is the weighted sum of exactly the levels with weight > 0: a float32 fold of at most ten weighted means
    # (10 products, 10 additions, 5 roundings of the per-level values read back here: 32 x 2^-24 covers them)
    assert abs(loss - folded) <= 32 * 2.0 ** -24 * max(abs(folded), 1.0), (tag, loss, folded)
    return loss


def _check_grads(tag, ora, grads, absent):
    """grads: name -> tensor in the reference layout (or None).  absent(name): the optimizer does not see this tensor."""
    g64s, eref = ora['f64']['grads'], ora['eref']
    worst, loose, total = (0.0, '', 0.0), 0, 0
    for n, g64 in g64s.items():
        if g64 is None:
            assert absent(n), '%s: %s has no gradient in the reference but the optimizer sees one' % (tag, n)
            continue
        assert grads[n] is not None and not absent(n), '%s: %s is reached in the reference' % (tag, n)
        gh = grads[n].detach().cpu().double().numpy()
        scale = float(np.abs(g64).max()) + 1e-30
        eh, eo = float(np.abs(gh - g64).max()) / scale, eref[n]
        worst = max(worst, (eh, n, eo))
        total += 1
        loose += eh > 2 * eo + 1e-3
        assert eh <= 3 * eo + 5e-3, '%s %s: HIP %.3e of scale vs fp64, reference fp32 %.3e' % (tag, n, eh, eo)
    assert loose <= 0.03 * total, '%s: %d of %d tensors beyond 2 e_ref + 1e-3' % (tag, loose, total)
    return worst


def _check_adam(tag, ora, ref, before, after, moments, wd):
    """One step from zero moments.  before / after: name -> parameter values (reference layout, float64 arrays); moments:
    name -> (exp_avg, exp_avg_sq) arrays or None where the optimizer holds no state."""
    worst, n_delta, n_mom = 0.0, 0, 0
    for n, g64 in ora['f64']['grads'].items():
        if g64 is None:
            assert np.array_equal(before[n], after[n]), '%s: skipped parameter %s moved' % (tag, n)
            if moments[n] is not None:
                assert not moments[n][0].any() and not moments[n][1].any(), '%s: skipped parameter %s has moments' % (tag, n)
            continue
        r = ref[n]
        m, v = moments[n]
        if r['excluded'] <= 0.2:
            keep = r['keep']
            rel = float((np.abs((after[n] - before[n]) - r['delta'])[keep] / np.abs(r['delta'][keep])).max())
            worst = max(worst, rel / r['yard'])
            n_delta += 1
            assert rel <= 2 * r['yard'], '%s %s: delta %.3e from the fp64 Adam step, fp32 yardstick %.3e' % (tag, n, rel, r['yard'])
        else:
            # first step: exp_avg = (1 - b1) g', exp_avg_sq = (1 - b2) g'^2 with g' = g + wd p
            ge = g64 + wd * before[n]
            bar = (3 * ora['eref'][n] + 5e-3) * r['scale']
            n_mom += 1
            assert float(np.abs(m / (1 - R.BETA1) - ge).max()) <= bar, '%s %s: exp_avg' % (tag, n)
            assert float(np.abs(np.sqrt(v / (1 - R.BETA2)) - np.abs(ge)).max()) <= bar, '%s %s: exp_avg_sq' % (tag, n)
            assert not np.array_equal(before[n], after[n]) or not ge.any(), '%s %s: reached parameter did not move' % (tag, n)
    return worst, n_delta, n_mom


def _force_teacher(hm, vols):
    """train_step(teacher_forced=True) hands the model the batch's target occupancies; the parity run needs the oracle's
    masks instead (what GraphStep.teacher_volumes does for the graph path)."""
    inner = hm.forward

    def forward(x, loss_weights, **kw):
        assert kw.get('teacher') is not None
        kw['teacher'] = vols
        return inner(x, loss_weights, **kw)
    hm.forward = forward


def _classic(ora, variant, lr, wd):
    """One train_step on a fresh model.  Returns what the checks need."""
    from sgnn_amd.train import train_step, make_optimizer
    from sgnn_amd.model import named_gradients
    hm, batch, vols = _setup(ora, variant)
    _force_teacher(hm, vols)
    opt = make_optimizer(hm.parameters(), lr=lr, weight_decay=wd)
    before = _params(hm)
    loss, losses, outputs = train_step(hm, opt, batch, ora['lw'], teacher_forced=True)
    torch.cuda.synchronize()
    conv = _ref_layout(hm)
    named = dict(hm.named_parameters())
    moments = dict((n, (conv[n](opt.state[p]['exp_avg']), conv[n](opt.state[p]['exp_avg_sq'])) if len(opt.state[p]) else None)
                   for n, p in named.items())
    stepped = dict((n, float(opt.state[p]['step']) if len(opt.state[p]) else 0.0) for n, p in named.items())
    grads = named_gradients(hm)
    absent = lambda n: grads[n] is None and moments[n] is None and stepped[n] == 0.0
    reached = [s for s in R.SEGMENTS if any(stepped[n] > 0 for n in named if R.segment_of(n) == s)]
    assert all(stepped[n] == 1.0 for n in named if R.segment_of(n) in reached)
    return dict(loss=loss, losses=losses, outputs=outputs, grads=grads, absent=absent, reached=reached, before=before,
                after=_params(hm), moments=moments)


class _Graph(object):
    """A GraphStep on a fresh model, with the optimizer's flat state readable by parameter name."""

    def __init__(self, ora, variant, lr, wd):
        from sgnn_amd.train import GraphStep
        self.hm, self.batch, vols = _setup(ora, variant)
        self.gs = GraphStep(self.hm, lr=lr, weight_decay=wd, teacher_forced=True, settle=False, keep_outputs=True)
        self.gs.teacher_volumes = vols
        self.kept = [vols]           # (volumes a captured graph may still read)
        self.opt = self.gs.opt
        assert tuple(n for n, _ in self.opt.segments) == R.SEGMENTS
        self.conv = _ref_layout(self.hm)
        self.names = dict((id(p), n) for n, p in self.hm.named_parameters())
        self.p0 = self.opt.flat_p.clone()

    def set_teacher(self, ora):
        vols = [v.cuda() for v in R.teacher_volumes(ora)]
        self.kept.append(vols)
        self.gs.teacher_volumes = vols

    def fresh(self):
        """Back to the initial parameters, zero moments and step counters."""
        torch.cuda.synchronize()
        self.opt.flat_p.copy_(self.p0)
        self.opt.flat_m.zero_()
        self.opt.flat_v.zero_()
        self.opt.steps.zero_()

    def named(self, flat):
        out, o = {}, 0
        for p in self.opt.params:
            n = p.numel()
            out[self.names[id(p)]] = self.conv[self.names[id(p)]](flat[o:o + n].view_as(p))
            o += n
        return out

    def steps(self):
        return [float(v) for v in self.opt.steps[:len(R.SEGMENTS)].cpu()]

    def call(self, lw):
        loss = float(self.gs(self.batch, lw))
        torch.cuda.synchronize()
        return loss

    def absent_after(self, steps_before):
        """name -> True where this call's optimizer step did not touch the tensor's segment (counter unchanged)."""
        now = self.steps()
        moved = dict((s, b != a) for s, b, a in zip(R.SEGMENTS, steps_before, now))
        assert all(a - b in (0.0, 1.0) for b, a in zip(steps_before, now)), (steps_before, now)
        return (lambda n: not moved[R.segment_of(n)]), [s for s in R.SEGMENTS if moved[s]]


CASES = [(s, v) for v in R.VARIANTS for s in R.STAGES]


@gpu
@pytest.mark.parametrize('stage,variant', CASES)
def test_curriculum_stage_vs_oracle(stage, variant):
    lw = R.stage_weights(stage)
    ora = R.oracle_stage(lw, variant)
    want_reached = [s for s in R.SEGMENTS if ora['reached'][s]]
    tag = '%s/%s' % (stage, variant)
    wd = 1e-2 if (stage, variant) == DECAY_CASE else 0.0

    # -- lr = 0: forward, loss, consumed gradients; classic path, then every phase of the graph path
    c = _classic(ora, variant, 0.0, 0.0)
    _check_forward(tag + ' classic', ora, c['outputs'])
    loss_c = _check_loss(tag + ' classic', ora, c['loss'], c['losses'])
    worst_c = _check_grads(tag + ' classic', ora, c['grads'], c['absent'])
    assert c['reached'] == want_reached, (tag, c['reached'], want_reached)
    g = _Graph(ora, variant, 0.0, 0.0)
    worst_g = (0.0, '', 0.0)
    for it, phase in enumerate(PHASES):
        t = '%s graph, %s' % (tag, phase)
        before = g.steps()
        loss = g.call(lw)
        absent, reached = g.absent_after(before)
        _check_forward(t, ora, g.gs.outputs)
        loss_g = _check_loss(t, ora, loss, g.gs.losses)
        worst_g = max(worst_g, _check_grads(t, ora, g.opt.named_gradients(g.hm), absent))
        assert reached == want_reached, (t, reached, want_reached)
        assert abs(loss_g - loss_c) <= _loss_bar(ora['f64']['loss'], ora['f32']['loss']), (t, loss_g, loss_c)
        # lr = 0 moves no parameter; a skipped segment's moments stay bit-identical zeros, its counter at 0
        assert torch.equal(g.opt.flat_p, g.p0), t
        for (b, e), s in zip(g.opt.bounds, R.SEGMENTS):
            if s not in want_reached:
                assert not g.opt.flat_m[b:e].any() and not g.opt.flat_v[b:e].any(), (t, s)
        assert g.steps() == [float(it + 1) if s in want_reached else 0.0 for s in R.SEGMENTS], (t, g.steps())
    assert g.gs.stats['probe_steps'] == 1 and g.gs.stats['eager_steps'] == 1 and g.gs.stats['captures'] == 1, g.gs.stats
    assert g.gs.stats['replays'] == 2 and g.gs.stats['overflows'] == 0, g.gs.stats

    # -- lr = 1e-3: one optimizer step from fresh moments, classic path and every phase of the graph path
    c = _classic(ora, variant, LR, wd)
    ref = R.adam_reference(ora, dict((n, v.astype(np.float32)) for n, v in c['before'].items()), LR, wd)
    yard = max([r['yard'] for r in ref.values() if r['excluded'] <= 0.2] or [0.0])
    assert c['reached'] == want_reached
    adam_worst, n_delta, n_mom = _check_adam(tag + ' classic step', ora, ref, c['before'], c['after'], c['moments'], wd)
    g = _Graph(ora, variant, LR, wd)
    p_before = g.named(g.p0)
    for it, phase in enumerate(PHASES):
        t = '%s graph step, %s' % (tag, phase)
        g.fresh()
        g.call(lw)
        ms, vs = g.named(g.opt.flat_m), g.named(g.opt.flat_v)
        aw, _, _ = _check_adam(t, ora, ref, p_before, g.named(g.opt.flat_p), dict((n, (ms[n], vs[n])) for n in ms), wd)
        adam_worst = max(adam_worst, aw)
        assert g.steps() == [1.0 if s in want_reached else 0.0 for s in R.SEGMENTS], (t, g.steps())
    assert g.gs.stats['captures'] == 1 and g.gs.stats['replays'] == 2 and g.gs.stats['overflows'] == 0, g.gs.stats
    report('curriculum %-8s w=%s loss %.7f classic / %.7f graph (fp64 %.7f, oracle fp32 %+.1e); worst gradient tensor %.2e of '
           'scale (%s, e_ref %.2e); Adam delta yardstick %.2e (fp32 step vs fp64), worst HIP delta %.2f of it over %d tensors, '
           '%d by moments, wd %g; reached %s; oracle %.1f s'
           % (tag, np.round(lw, 3).tolist(), loss_c, loss_g, ora['f64']['loss'], ora['f32']['loss'] - ora['f64']['loss'],
              max(worst_c, worst_g)[0], max(worst_c, worst_g)[1], max(worst_c, worst_g)[2], yard, adam_worst, n_delta, n_mom,
              wd, ','.join(want_reached), ora['seconds']))


@gpu
def test_stage_change_on_a_live_graph_step():
    """S1 -> S2 -> S1 -> S1 with another fraction on ONE GraphStep (lr = 0).  A change of which levels are switched on is a
    new key: the step probes, warms up and captures again.  A change of a weight's VALUE alone keeps capacities and stage:
    the loss weights are baked into the captured launches, so the graph is captured again (no probe, no eager step) — in
    neither case may a replay apply the weights of the stage before.  Every call is held to the oracle run of its own
    weights; a segment the current stage skips keeps its counter, whatever an earlier stage left in its gradient slice."""
    variant = 'full'
    seq = [('S1', False, 3), ('S2', False, 3), ('S1', False, 3), ('S1', True, 2)]
    g = None
    want_stats = {'probe_steps': 0, 'eager_steps': 0, 'captures': 0, 'replays': 0}
    want_steps = [0.0] * len(R.SEGMENTS)
    for k, (stage, alt, calls) in enumerate(seq):
        lw = R.stage_weights(stage, alt=alt)
        ora = R.oracle_stage(lw, variant)
        if g is None:
            g = _Graph(ora, variant, 0.0, 0.0)
        elif not alt:        # (another fraction of the same stage walks the same masks)
            g.set_teacher(ora)
        want_reached = [s for s in R.SEGMENTS if ora['reached'][s]]
        for it in range(calls):
            t = 'stage change %d: %s%s call %d' % (k, stage, ' (other fraction)' if alt else '', it)
            before = g.steps()
            loss = g.call(lw)
            absent, reached = g.absent_after(before)
            _check_forward(t, ora, g.gs.outputs)
            _check_loss(t, ora, loss, g.gs.losses)
            _check_grads(t, ora, g.opt.named_gradients(g.hm), absent)
            assert reached == want_reached, (t, reached, want_reached)
            want_steps = [v + (1.0 if s in want_reached else 0.0) for v, s in zip(want_steps, R.SEGMENTS)]
            assert g.steps() == want_steps, (t, g.steps(), want_steps)
        if alt:      # same key, new values: re-capture only
            want_stats['captures'] += 1
            want_stats['replays'] += calls
        else:        # new key: probe, eager capacity step, capture + replay
            want_stats = dict(probe_steps=want_stats['probe_steps'] + 1, eager_steps=want_stats['eager_steps'] + 1,
                              captures=want_stats['captures'] + 1, replays=want_stats['replays'] + calls - 2)
        got = dict((key, g.gs.stats[key]) for key in want_stats)
        assert got == want_stats and g.gs.stats['overflows'] == 0, (stage, alt, g.gs.stats, want_stats)
    assert torch.equal(g.opt.flat_p, g.p0)
