"""The native program executor (sgnn_prog_forward/backward) must reproduce the per-layer path.  With the epilogue
fusions off it launches the same kernels in the same order (logits agree to 1e-6, bit-identical except for the
order of two-term gradient sums); with the fusions on (default) the only arithmetic difference is the summation
order of the BatchNorm statistics (fp64 over convolution tiles instead of fp32 row pairs flushed into fp64), which
moves mean / invstd by an ulp in some channels; ~60 stacked conv/BN layers amplify that to ~5e-6 of the logit scale
(measured, scripts/diag_fuse.py; two fused runs are bit-identical): site lists stay identical, logits are held to
3e-5 of the logit scale — the oracle comparison in test_gpu_model.py is the accuracy test."""
import numpy as np
import pytest
import torch

from util import param_fill
from sgnn_amd import synth

pytestmark = pytest.mark.gpu


def _run(enabled, train=True):
    from sgnn_amd.model import GenModel
    from sgnn_amd import loss as L
    from sgnn_amd.scn import program as P
    P.ENABLED = enabled
    try:
        dims, cfg = (32, 32, 32), 17
        data = synth.make_batch(2, dims, cfg=cfg, occupancy=0.08)
        m = param_fill(GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train(train).cuda()
        lw = np.ones(5, dtype=np.float32)
        t = L.compute_targets(data['sdf'].clone().cuda(), [h.clone().cuda() for h in data['hierarchy']], 4, 3, True,
                              data['known'].cuda())
        if not train:
            with torch.no_grad():
                osdf, oocc = m([data['input'][0].cuda(), data['input'][1].cuda()], lw)
            return m, osdf, oocc, None
        osdf, oocc = m([data['input'][0].cuda(), data['input'][1].cuda()], lw)
        loss, _ = L.compute_loss(osdf, oocc, t[0], t[1], t[2], lw, 3, True, 5.0, data['input'][0].cuda(), True,
                                 data['known'].cuda())
        loss.backward()
        return m, osdf, oocc, loss.item()
    finally:
        P.ENABLED = True


@pytest.mark.parametrize('train,fused', [(True, True), (True, False), (False, True)])
def test_program_path_equals_layer_path(train, fused):
    from sgnn_amd import _lib
    prev = _lib.tune('prog_fusion', int(fused))
    try:
        ma, sa, oa, la = _run(True, train)
    finally:
        _lib.tune('prog_fusion', prev)
    mb, sb, ob, lb = _run(False, train)
    tol = 3e-5 if (fused and train) else 1e-6
    assert ma.encoder._sparse_program() is not None
    if train:
        assert all(p is not None for m in (ma.refinement[0], ma.surfacepred) for p in m._stage_progs.values())
        assert len(ma.refinement[0]._stage_progs) == 1 and len(ma.surfacepred._stage_progs) == 1
    def same(a, b):   # a level that received no sites is reported as empty lists (torch/model.py:211)
        if len(a[0]) == 0 or len(b[0]) == 0:
            assert len(a[0]) == 0 and len(b[0]) == 0
            return
        assert torch.equal(a[0], b[0])
        assert (a[1] - b[1]).abs().max().item() <= tol * max(1.0, b[1].abs().max().item())

    for h in range(4):
        same(oa[h], ob[h])
    same(sa, sb)
    if train:
        assert abs(la - lb) <= tol * max(1.0, abs(lb))
        pb = dict(mb.named_parameters())
        for n, p in ma.named_parameters():
            assert p.grad is not None and pb[n].grad is not None, n
            scale = max(1.0, pb[n].grad.abs().max().item())
            # gradients of a ReLU network are discontinuous in the activations: a summation-order-only change (1e-6
            # on the activations) flips ~100 of the 1e8 ReLU decisions of this step, and one flipped row moves a weight-
            # gradient entry (a sum over ~1e5 rows of mixed sign) by ~3e-3 of the largest entry.  Measured
            # (scripts/diag_fuse_grads.py): swapping only the small-level conv kernel changes the loss by 2.5e-7 and the
            # gradients by up to 1.7e-2 (median 4e-3) of each tensor's largest entry; the fusions by up to 3.3e-2.  The
            # tight checks of the fused arithmetic are op-level (tests/test_gpu_fused.py, 1e-5) and the [True-False]
            # case here (identical arithmetic: 1e-5); this case gets the tolerance of the golden fixtures (5 %).
            assert (p.grad - pb[n].grad).abs().max().item() <= (5e-2 if (fused and train) else 1e-5) * scale, n
        bb = dict(mb.named_buffers())
        for n, b in ma.named_buffers():
            assert torch.allclose(b.float(), bb[n].float(), atol=10 * tol, rtol=10 * tol), \
                (n, (b.float() - bb[n].float()).abs().max().item())


def test_program_compiler_rejects_what_it_cannot_run():
    import sgnn_amd.scn as scn
    from sgnn_amd.scn import program as P
    assert P.compile_or_none([scn.SubmanifoldConvolution(3, 4, 8, 3, True)], 4) is None      # bias
    assert P.compile_or_none([scn.UnPooling(3, 2, 2)], 4) is None                            # above level 0
    p = P.compile_or_none([scn.FullyConvolutionalNet(3, 1, [8, 8], True)], 8)
    assert p is not None and p.nlev == 2 and p.bufs[p.out][1] == 16


@pytest.mark.parametrize('masking,wgeo', [(True, 5.0), (False, 1.0), (True, 1.0)])
def test_fused_level_loss_equals_torch_loss(masking, wgeo):
    """sgnn_loss_levels_fwd/bwd vs the torch-op restatement of torch/loss.py:58-157 (value and gradients); without
    precomputed weights the (True, 5.0) case goes level by level, one n = 1 call each."""
    from sgnn_amd import loss as L
    torch.manual_seed(2)
    data = synth.make_batch(2, (16, 16, 16), cfg=9, occupancy=0.1)
    dims = data['sdf'].shape[2:]
    outs = []
    for h, f in enumerate((8, 4, 2, 1)):
        d = [v // f for v in dims]
        n = 300
        locs = torch.stack([torch.randint(0, d[0], (n,)), torch.randint(0, d[1], (n,)), torch.randint(0, d[2], (n,)),
                            torch.randint(0, 2, (n,))], 1).cuda()
        outs.append([locs, torch.randn(n, 2).cuda()])
    sdf_locs, sdf_vals = outs[3][0], torch.randn(outs[3][0].shape[0], 1).cuda()
    lw = np.array([1, 0.5, 1, 1, 2], dtype=np.float32)
    res = []
    for fused in (True, False):
        L.FUSED = fused
        try:
            t = L.compute_targets(data['sdf'].clone().cuda(), [h.clone().cuda() for h in data['hierarchy']], 4, 3,
                                  masking, data['known'].cuda())
            vs = [o[1].clone().requires_grad_(True) for o in outs]
            sv = sdf_vals.clone().requires_grad_(True)
            loss, losses = L.compute_loss([sdf_locs, sv], [[o[0], v] for o, v in zip(outs, vs)], t[0], t[1], t[2], lw, 3,
                                          True, wgeo, data['input'][0].cuda(), masking, data['known'].cuda())
            g = torch.autograd.grad(loss, vs + [sv])
            res.append((loss.item(), [float(x) for x in losses], g))
        finally:
            L.FUSED = True
    (la, lsa, ga), (lb, lsb, gb) = res
    assert abs(la - lb) < 1e-5 * max(1.0, abs(lb))
    assert np.allclose(lsa, lsb, rtol=1e-5, atol=1e-6)
    for x, y in zip(ga, gb):
        assert (x - y).abs().max().item() < 1e-6


def test_one_level_calls_equal_the_all_levels_call_bit_for_bit():
    """A level's value and gradient do not depend on which other levels share the sgnn_loss_levels_* call: the
    level-by-level route of compute_loss (no precomputed weights; one n = 1 call per level, coefficient 1) gives the
    same bits as the one all-levels call of the training step.  1500 sites on the finest and on the sdf level make
    loss_blocks() two workgroups there, so the two-stage reduction and the per-level stride take part.  The totals
    weight differently (sum lw*bce + lw*l1 slot by slot vs sum lw*(bce + l1)) and are held to 1e-6 relative."""
    from sgnn_amd import loss as L
    torch.manual_seed(3)
    data = synth.make_batch(2, (16, 16, 16), cfg=9, occupancy=0.1)
    dims = data['sdf'].shape[2:]
    sites = lambda n, d: torch.stack([torch.randint(0, d[0], (n,)), torch.randint(0, d[1], (n,)),
                                      torch.randint(0, d[2], (n,)), torch.randint(0, 2, (n,))], 1).cuda()
    outs = [[sites(n, [v // f for v in dims]), torch.randn(n, 2).cuda()]
            for f, n in ((8, 300), (4, 300), (2, 300), (1, 1500))]
    sdf_locs, sdf_vals = outs[3][0], torch.randn(1500, 1).cuda()
    lw = np.array([1, 0.5, 1, 1, 2], dtype=np.float32)
    sdf, hier, known = data['sdf'].cuda(), [h.cuda() for h in data['hierarchy']], data['known'].cuda()
    in_locs = data['input'][0].cuda()
    (ts, occs, hiers), w = L.compute_targets_and_weights(sdf, hier, 4, 3.0, True, known, 5.0, in_locs)
    res = []
    for weights in (w, None):
        vs = [o[1].clone().requires_grad_(True) for o in outs]
        sv = sdf_vals.clone().requires_grad_(True)
        loss, losses = L.compute_loss([sdf_locs, sv], [[o[0], v] for o, v in zip(outs, vs)], ts, occs, hiers, lw, 3.0,
                                      True, 5.0, in_locs, True, known, weights=weights)
        if weights is not None:
            assert 'TotalLoss' in type(loss.grad_fn).__name__          # one all-levels launch each way
        res.append((loss.detach(), [x.detach() for x in losses], torch.autograd.grad(loss, vs + [sv])))
    (la, lsa, ga), (lb, lsb, gb) = res
    assert len(lsa) == len(lsb) == 5
    for h, (x, y) in enumerate(zip(lsa, lsb)):
        assert torch.equal(x, y), (h, float(x), float(y))
    for h, (x, y) in enumerate(zip(ga, gb)):
        assert torch.equal(x, y), (h, (x - y).abs().max().item())
    assert abs(la.item() - lb.item()) <= 1e-6 * abs(lb.item()), (la.item(), lb.item())


def test_training_step_is_bitwise_reproducible():
    """No atomics on floats anywhere, the weight-gradient lane joins before gradients are read, aliased gradients are
    never written: two runs of the same step give identical bits (loss, every gradient, BN buffers)."""
    import numpy as np
    from sgnn_amd import synth, loss as L
    from sgnn_amd.model import GenModel
    from util import param_fill
    dims = (32, 32, 32)
    data = synth.make_batch(3, dims, cfg=21, occupancy=0.08)
    lw = np.ones(5, dtype=np.float32)
    runs = []
    for _ in range(2):
        m = param_fill(GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), 21).train().cuda()
        t = L.compute_targets(data['sdf'].clone().cuda(), [h.clone().cuda() for h in data['hierarchy']], 4, 3, True,
                              data['known'].cuda())
        locs, feats = data['input'][0].cuda(), data['input'][1].cuda()
        osdf, oocc = m([locs, feats], lw)
        loss, _ = L.compute_loss(osdf, oocc, t[0], t[1], t[2], lw, 3, True, 5.0, locs, True, data['known'].cuda())
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), [p.grad.clone() for p in m.parameters()],
                     [b.clone() for b in m.buffers()]))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dims', [(32, 32, 32), (64, 32, 48)])
@pytest.mark.parametrize('masking,wgeo', [(True, 5.0), (False, 1.0), (False, 3.0)])
def test_fused_targets_equal_tensor_op_targets(dims, masking, wgeo):
    """sgnn_loss_targets (three launches) vs the tensor-op restatement of torch/loss.py:15-48: every target volume,
    every weight volume, every level — bit for bit (clamps, comparisons and maxima are exact)."""
    from sgnn_amd import loss as L
    data = synth.make_batch(3, dims, cfg=31, occupancy=0.08)
    sdf, hier, known = data['sdf'].cuda(), [h.cuda() for h in data['hierarchy']], data['known'].cuda()
    locs = data['input'][0].cuda()
    sdf_before = sdf.clone()
    (ts, occs, hiers), w = L.compute_targets_and_weights(sdf, hier, 4, 3.0, masking, known, wgeo, locs)
    assert torch.equal(sdf, sdf_before)                      # inputs untouched
    rs, roccs, rhiers = L.compute_targets(sdf.clone(), [h.clone() for h in hier], 4, 3.0, masking, known)
    assert torch.equal(ts, rs)
    for h in range(4):
        assert torch.equal(occs[h], roccs[h]), h
        assert torch.equal(hiers[h], rhiers[h]), h
    if wgeo > 1:
        rw = L.compute_weights_missing_geo(wgeo, locs, roccs, 3.0)
        for h in range(4):
            assert torch.equal(w[h], rw[h]), h
        assert float(w[3].min()) == 1.0 and float(w[3].max()) == wgeo
    else:
        assert w is None


def prog_params(chain):
    return [p for m in chain for p in m.parameters()]


def test_teacher_forced_geometry_first_is_the_same_computation():
    """Teacher-forced step with all level geometry built up front (model.TEACHER_GEOMETRY_FIRST: one burst of cheap
    read-backs, then a synchronisation-free step) == the interleaved order: same site lists, same logits, same loss,
    same gradients, bit for bit; and the up-front variant does not touch the host between encoder and optimizer."""
    from sgnn_amd import model as M
    from sgnn_amd.train import train_step, to_device, make_optimizer
    from sgnn_amd.scn.metadata import runtime
    dims, cfg = (32, 32, 32), 17
    batch = to_device(synth.make_batch(2, dims, cfg=cfg, occupancy=0.08), 'cuda')
    lw = np.ones(5, dtype=np.float32)
    res = []
    for first in (False, True):
        prev = M.TEACHER_GEOMETRY_FIRST
        M.TEACHER_GEOMETRY_FIRST = first
        try:
            m = param_fill(M.GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().cuda()
            opt = make_optimizer(m.parameters(), lr=1e-3)
            rt = runtime(torch.device('cuda', torch.cuda.current_device()))
            s0 = rt.syncs
            loss, _, (osdf, oocc) = train_step(m, opt, batch, lw, teacher_forced=True)
            res.append((loss.item(), osdf[0].clone(), osdf[1].clone(), [o[1].clone() for o in oocc],
                        [p.detach().clone() for p in m.parameters()], rt.syncs - s0))
        finally:
            M.TEACHER_GEOMETRY_FIRST = prev
    a, b = res
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[4]))     # parameters after the Adam step
    assert a[5] == b[5]                                            # same number of read-backs, only earlier


def test_prefetched_geometry_is_the_same_training_run():
    """Eight teacher-forced steps over two alternating batches with train.GeometryPrefetcher (batch i+1's targets and
    geometry built on a second stream during step i) == the same steps without it: losses and final parameters bit
    for bit; the main lane never reads back from the device."""
    from sgnn_amd import model as M
    from sgnn_amd.train import train_step, to_device, make_optimizer, GeometryPrefetcher
    from sgnn_amd.scn.metadata import runtime
    dims, cfg = (32, 32, 32), 17
    batches = [to_device(synth.make_batch(2, dims, cfg=cfg + j, occupancy=0.08), 'cuda') for j in range(2)]
    lw = np.ones(5, dtype=np.float32)
    res = []
    for use in (None, 'after', 'thread'):       # no prefetcher / plan built after the step / on a worker thread
        m = param_fill(M.GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().cuda()
        opt = make_optimizer(m.parameters(), lr=1e-3)
        pre = GeometryPrefetcher(m, threaded=(use == 'thread')) if use else None
        rt = runtime(torch.device('cuda', torch.cuda.current_device()))
        losses, mem = [], []
        for i in range(8):
            if i == 1:
                s0 = rt.syncs
            loss, _, _ = train_step(m, opt, batches[i % 2], lw, teacher_forced=True, prefetch=pre,
                                    next_batch=batches[(i + 1) % 2] if use else None)
            losses.append(loss.detach())
            del loss
            if i in (3, 5, 7):              # same batch parity each time: the live set must not grow step over step
                if pre is not None and pre.pending is not None and pre.pending.get('thread') is not None:
                    pre.pending['thread'].join()        # a builder in flight holds temporaries
                torch.cuda.synchronize()
                mem.append(torch.cuda.memory_allocated())
        syncs = rt.syncs - s0
        torch.cuda.synchronize()
        res.append(([l.item() for l in losses], [p.detach().clone() for p in m.parameters()], syncs, mem))
    a = res[0]
    assert a[2] == 35                            # 5 read-backs per step on the main lane without the prefetcher
    # live bytes are counted in allocator blocks: a request served from a larger cached block (torch does not split
    # large-pool blocks for a remainder under 1 MB) moves the figure by up to 1 MB per tensor depending on what earlier
    # tests left in the cache.  A leak would be >= 1.5 MB per step, i.e. >= 6 MB over the four steps spanned here.
    assert max(a[3]) - min(a[3]) < (2 << 20), a[3]
    for b in res[1:]:
        assert a[0] == b[0], (a[0], b[0])
        assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
        assert b[2] == 0                         # ... none with it
        # no plan may outlive its step by more than the retention window (a plan hung on a tensor its own Grid views
        # is an uncollectable cycle); the kept loss scalars account for 512 bytes per step
        assert max(b[3]) - min(b[3]) < (2 << 20), b[3]      # a leaked plan is >= 1.5 MB per step here (6 MB over the span)


def test_input_errors_still_surface_with_the_prefetcher():
    """With the geometry prefetcher the training stream has no read-back that would report a duplicate input site
    (flagged on the device by the level-0 hash build); the end-of-step status copy must raise it within two steps."""
    from sgnn_amd import model as M
    from sgnn_amd._lib import SgnnError
    from sgnn_amd.train import train_step, to_device, make_optimizer, GeometryPrefetcher
    dims, cfg = (32, 32, 32), 17
    batch = to_device(synth.make_batch(2, dims, cfg=cfg, occupancy=0.08), 'cuda')
    locs, feats = batch['input']
    batch['input'] = [torch.cat([locs, locs[:1]]), torch.cat([feats, feats[:1]])]      # site 0 twice
    m = param_fill(M.GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().cuda()
    opt = make_optimizer(m.parameters(), lr=1e-3)
    pre = GeometryPrefetcher(m)
    lw = np.ones(5, dtype=np.float32)
    with pytest.raises(SgnnError, match='duplicate'):
        for _ in range(4):
            train_step(m, opt, batch, lw, teacher_forced=True, prefetch=pre, next_batch=batch)
    torch.cuda.synchronize()


def test_teacher_forced_hierarchy_is_the_target_hierarchy():
    """Teacher-forced forward (bench.py's workload): the candidate sites of level h+1 are exactly the 8 children (order
    4dz+2dy+dx, model.py:195-207) of the level-h candidates whose target occupancy is 1, in stable order, and the
    final sites are the last level's candidates with target occupancy 1 — checked with tensor ops on the outputs."""
    from sgnn_amd import model as M, loss as L
    dims, cfg = (32, 32, 32), 17
    data = synth.make_batch(2, dims, cfg=cfg, occupancy=0.08)
    m = param_fill(M.GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().cuda()
    lw = np.ones(5, dtype=np.float32)
    tgt = L.compute_targets(data['sdf'].clone().cuda(), [h.clone().cuda() for h in data['hierarchy']], 4, 3, True,
                            data['known'].cuda())
    occs = tgt[1]
    with torch.no_grad():
        osdf, oocc = m([data['input'][0].cuda(), data['input'][1].cuda()], lw, batch_size=2, teacher=occs)
    offs = torch.tensor([[dz, dy, dx, 0] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    prev = None
    for h, (locs, out) in enumerate(oocc):
        locs = locs.cpu()
        assert out.shape[0] == locs.shape[0] > 0
        if prev is not None:
            assert torch.equal(locs, prev)
        t = occs[h].cpu()
        keep = t[locs[:, 3], 0, locs[:, 0], locs[:, 1], locs[:, 2]] > 0.5
        kept = locs[keep]
        assert 0 < kept.shape[0] < locs.shape[0]
        prev = (kept[:, None, :] * torch.tensor([2, 2, 2, 1]) + offs[None]).reshape(-1, 4)
    assert torch.equal(osdf[0].cpu(), kept) and osdf[1].shape[0] == kept.shape[0]
