"""One training step and the data-parallel wrapper — counterpart of torch/train.py:245-268 (H2D copies,
compute_targets, forward, compute_loss, backward, optimizer.step).

Multi-GPU (an addition of this build; the reference is single-process): one process
per GPU, each rank owns `batch_size` independent TSDF blocks (batch index is part of every voxel key, so
blocks never interact in a sparse op), BatchNorm statistics stay per replica, and the only exchange is one
all-reduce of a flat fp32 gradient buffer (643 735 floats = 2.57 MB) over RCCL/xGMI after backward.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import loss as loss_util
from .scn.sites import attach, carry


def _parse_cpulist(text):
    cpus = set()
    for part in text.strip().split(','):
        if not part:
            continue
        lo, _, hi = part.partition('-')
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def bind_to_device_numa(device=None):
    """One process per GPU: run it on the CPUs of the NUMA node that GPU hangs off (sysfs local_cpulist of its PCI
    function).  The training step is a stream of ~1 350 kernel launches; issued from the remote socket every launch
    and every count read-back crosses the inter-socket link (measured on a 2-socket MI355X host: 9.4 vs 10.4 ms per
    step, at random, until pinned).  Returns the CPU set, or None when the topology cannot be read (then nothing is
    changed).  SGNN_NO_BIND=1 disables it."""
    import os
    if os.environ.get('SGNN_NO_BIND') == '1' or not torch.cuda.is_available() or not hasattr(os, 'sched_setaffinity'):
        return None
    try:
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        p = torch.cuda.get_device_properties(idx)
        bdf = '%04x:%02x:%02x.0' % (getattr(p, 'pci_domain_id', 0), p.pci_bus_id, p.pci_device_id)
        with open('/sys/bus/pci/devices/%s/local_cpulist' % bdf) as f:
            cpus = _parse_cpulist(f.read()) & os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return cpus
    except (OSError, ValueError, AttributeError, RuntimeError):
        return None


class FlatGradAllReduce(object):
    """Averages gradients across ranks with a single collective on one flat buffer.

    The buffer carries one extra float per parameter tensor: 1 where this rank produced a gradient.  A parameter no
    rank reached this step (a generative level whose loss weight is still 0, train.py:203-231) keeps ``grad = None``
    on every rank, so Adam skips it exactly as the single-process run does (no step-counter advance, no weight
    decay).  A parameter only SOME ranks reached (rank-local empty level) receives sum / world_size — the mean over
    all replicas, the missing ones contributing zero — on every rank."""

    def __init__(self, params, group=None):
        self.params = [p for p in params if p.requires_grad]
        self.group = group
        self.numel = sum(p.numel() for p in self.params)
        self.flat = None

    def __call__(self):
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self.group) == 1:
            return
        ps = self.params
        dev, dt = ps[0].device, ps[0].dtype
        have_local = [p.grad is not None for p in ps]
        zeros = None
        if not all(have_local):
            zeros = torch.zeros(max(p.numel() for p, h in zip(ps, have_local) if not h), dtype=dt, device=dev)
        flags = torch.tensor([1.0 if h else 0.0 for h in have_local], dtype=dt).to(dev, non_blocking=True)
        grads = [p.grad.reshape(-1) if h else zeros[:p.numel()] for p, h in zip(ps, have_local)]
        self.flat = torch.cat(grads + [flags])           # one gather kernel instead of one copy per tensor
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        world = dist.get_world_size(self.group)
        if all(have_local):
            have_any = have_local                          # every rank sees >= 1 contributor: no read-back needed
        else:
            have_any = (self.flat[self.numel:] > 0).tolist()   # one small D2H, only on steps with a local gap
        self.flat[:self.numel].div_(world)
        pieces = self.flat[:self.numel].split([p.numel() for p in ps])
        dst, src = [], []
        for p, v, hl, ha in zip(ps, pieces, have_local, have_any):
            if not ha:
                p.grad = None
            elif hl:
                dst.append(p.grad)
                src.append(v.view_as(p))
            else:
                p.grad = v.view_as(p).clone()
        if dst:
            torch._foreach_copy_(dst, src)


class FastAdam(torch.optim.Adam):
    """torch.optim.Adam(fused=True) with the per-step Python bookkeeping removed: same state layout (state_dict /
    load_state_dict / lr schedulers work unchanged) and the same fused multi-tensor kernel, but the per-parameter
    Python loop of Adam.step (_init_group over 307 tensors, grouping by device/dtype: ~1.2 ms of a 10 ms step) runs
    once; a step is then one _foreach_add_ on the step counters and one _fused_adam_ call."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True)
        self._fast = None

    def _lists(self, group):
        """Parameters that carry a gradient this step (the others are skipped, as Adam.step does), with their state
        tensors (created like Adam._init_group does for fused=True: device step counter, zero moments)."""
        ps, avgs, sqs, steps = [], [], [], []
        for p in group['params']:
            if p.grad is None:
                continue
            st = self.state[p]
            if len(st) == 0:
                st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            ps.append(p)
            avgs.append(st['exp_avg'])
            sqs.append(st['exp_avg_sq'])
            steps.append(st['step'])
        return ps, avgs, sqs, steps

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._fast = None                 # the cached moment / step tensors were replaced

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._fast = None

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        if any(g['amsgrad'] or g['maximize'] or g.get('capturable') or g.get('differentiable')
               for g in self.param_groups):
            return super().step()         # decided before any group was touched: no double step
        for gi, group in enumerate(self.param_groups):
            n_with_grad = sum(p.grad is not None for p in group['params'])
            cache = self._fast.get(gi) if self._fast else None
            if cache is None or cache[0] != n_with_grad or any(p.grad is None for p in cache[1][0]) or \
                    any(self.state[p].get('exp_avg') is not a for p, a in zip(cache[1][0][:1], cache[1][1][:1])):
                cache = (n_with_grad, self._lists(group))      # first step, or a level (dis)appeared
                self._fast = dict(self._fast or {})
                self._fast[gi] = cache
            ps, avgs, sqs, steps = cache[1]
            if not ps:
                continue
            grads = [p.grad for p in ps]
            beta1, beta2 = group['betas']
            torch._foreach_add_(steps, 1)
            torch._fused_adam_(ps, grads, avgs, sqs, [], steps, amsgrad=False, lr=group['lr'], beta1=beta1, beta2=beta2,
                               weight_decay=group['weight_decay'], eps=group['eps'], maximize=False, grad_scale=None,
                               found_inf=None)


def make_optimizer(params, lr=1e-3, weight_decay=0.0):
    """Adam as train.py:81 (fused multi-tensor kernel, see FastAdam)."""
    return FastAdam(params, lr=lr, weight_decay=weight_decay)


def to_device(batch, device, non_blocking=False, record_ready=False):
    """train.py:256-262: move one collated sample to the GPU.  record_ready: also record a torch.cuda.Event after the
    copies (out['ready']) so that a consumer on another stream (GeometryPrefetcher) can order itself behind them."""
    out = dict(batch)
    mv = lambda t: t.to(device, non_blocking=non_blocking)
    out['input'] = [mv(batch['input'][0]), mv(batch['input'][1])]
    out['sdf'] = mv(batch['sdf'])
    out['known'] = mv(batch['known']) if batch.get('known') is not None else None
    out['hierarchy'] = [mv(h) for h in batch['hierarchy']] if batch.get('hierarchy') is not None else None
    if record_ready and torch.device(device).type == 'cuda':
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device(device)))
        out['ready'] = ev
    return out


OVERLAP_TARGETS = True
_target_streams = {}


def _target_stream(dev):
    s = _target_streams.get(dev)
    if s is None:
        s = _target_streams[dev] = torch.cuda.Stream(device=dev)
    return s


class StepPlan(object):
    """What a teacher-forced step needs from its batch alone: targets + loss weights, input coordinates with the
    encoder pyramid, site / index lists of every generative level.  `ready` is recorded on the stream that built it."""
    __slots__ = ('batch', 'loss_weights', 'targets', 'weights', 'geometry', 'ready')


class GeometryPrefetcher(object):
    """Teacher-forced training, one batch ahead: the geometry of a step (every host read-back it has) is a function of
    the batch, so batch i+1's StepPlan is built on a second stream while batch i occupies the GPU, and the main stream
    never drains at a step boundary.

        pre = GeometryPrefetcher(model)
        for i, batch in enumerate(batches):
            train_step(model, opt, batch, lw, teacher_forced=True, prefetch=pre, next_batch=batches[i + 1])

    threaded=False (default) builds the next plan after the optimizer step has been issued (1.6 ms of host time per
    step at the BASELINE batch); threaded=True builds it on a worker thread started at the head of the step — correct and
    tested, but measured slower on this workload (7.8 vs 7.3–7.4 ms/step: the builder is Python-bound, its 3.3 ms under
    the GIL slow the issuing thread by more than the five read-back waits it hides).

    Memory discipline: plan tensors are allocated on the prefetch stream's pool and read by main-stream kernels of
    their step.  A plan is retained until the host has seen its step finish on the GPU (end-of-step events, `_retire`),
    only then may the pool hand its blocks to a new plan; the same wait keeps the host at most two steps ahead of the
    device.  The prefetch stream uses scratch lane 1 of the runtime (scn.metadata.lane): its workspace and count block
    are not shared with main-stream kernels."""

    def __init__(self, model, num_hierarchy_levels=4, truncation=3.0, weight_missing_geo=5.0, use_loss_masking=True,
                 threaded=None):
        self.model = model
        self.args = (num_hierarchy_levels, truncation, use_loss_masking, weight_missing_geo)
        self.threaded = (os.environ.get('SGNN_PREFETCH_THREAD', '0') == '1') if threaded is None else bool(threaded)
        self.stream = None
        self.pending = None            # the announced next batch's plan: {'plan' | 'error', 'thread'}
        self.issued = []               # [(end-of-step event on the main stream, plan of that step, status copy)]
        self.t_build = self.t_throttle = 0.0   # host seconds spent building plans / waiting for old steps
        self._status, self._n, self._rt = [], 0, None   # pinned copies of the training lane's status word, per step

    def build(self, batch, loss_weights):
        """StepPlan of `batch` on the prefetch stream (the calling thread blocks for its five read-backs only)."""
        from .scn.metadata import lane
        dev = batch['sdf'].device
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)    # (a high-priority stream measured no different)
        nl, trunc, masking, wgeo = self.args
        plan = StepPlan()
        plan.batch, plan.loss_weights = batch, np.array(loss_weights, copy=True)
        known = batch['known'] if masking else None
        # the batch may still be in flight on the stream that produced it (non-blocking H2D copies, a device-side
        # collate): order the prefetch stream behind it — batch['ready'] (a torch.cuda.Event recorded by the producer,
        # e.g. to_device(..., record_ready=True)) if present, else the current stream of the calling thread
        ready = batch.get('ready') if isinstance(batch, dict) else None
        if ready is not None:
            self.stream.wait_event(ready)
        else:
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(self.stream), lane(1):
            plan.targets, plan.weights = loss_util.compute_targets_and_weights(
                batch['sdf'], batch['hierarchy'], nl, trunc, masking, known, wgeo, batch['input'][0])
            plan.geometry = self.model.plan_geometry(batch['input'][0], loss_weights, int(batch['sdf'].shape[0]),
                                                     plan.targets[1])
            plan.ready = torch.cuda.Event()
            plan.ready.record(self.stream)
        return plan

    def _retire(self, keep):
        """Wait for all but the `keep` most recently issued steps to leave the GPU and let go of their plans."""
        import time
        t0 = time.perf_counter()
        while len(self.issued) > keep:
            ev, _plan, status, index = self.issued.pop(0)
            ev.synchronize()
            if status is not None and int(status[0]):
                # the training stream has no read-back of its own any more: input errors its kernels flagged during
                # that step (duplicate / out-of-range sites) surface here, two steps later at most — named by the
                # step they belong to (its optimizer update has already been applied)
                self._rt.raise_status(int(status[0]), 'raised by train_step call %d of this prefetcher (0-based), %d call(s) '
                                      'ago; that step\'s parameter update was applied' % (index, self._n - 1 - index))
        self.t_throttle += time.perf_counter() - t0

    def _start(self, batch, loss_weights):
        import threading
        import time
        box = {}

        def work():
            t0 = time.perf_counter()
            try:
                box['plan'] = self.build(batch, loss_weights)
            except BaseException as e:          # re-raised by take() on the training thread
                box['error'] = e
            self.t_build += time.perf_counter() - t0

        if not self.threaded:
            work()
            return box
        th = threading.Thread(target=work, name='sgnn-geometry-prefetch', daemon=True)
        box['thread'] = th
        th.start()
        return box

    @staticmethod
    def _result(box):
        if box.get('thread') is not None:
            box['thread'].join()
        if 'error' in box:
            raise box['error']
        return box['plan']

    def take(self, batch, loss_weights):
        """The plan announced for `batch` (built now when it was not announced); the main stream waits for it."""
        box, self.pending = self.pending, None
        plan = self._result(box) if box is not None else None
        if plan is None or plan.batch is not batch or not np.array_equal(plan.loss_weights, loss_weights):
            plan = self._result(self._start(batch, loss_weights))
        torch.cuda.current_stream(batch['sdf'].device).wait_event(plan.ready)
        return plan

    def announce(self, next_batch, loss_weights):
        """Head of a step, right after take(): start building `next_batch`'s plan on the worker thread."""
        if self.threaded and next_batch is not None:
            self._retire(1)     # the pool may recycle plans older than the previous step's from here on
            self.pending = self._start(next_batch, loss_weights)

    def step_issued(self, dev, plan, next_batch, loss_weights):
        """Call after the optimizer step of a step has been issued: remember when it ends, keep its plan until then."""
        from .scn.metadata import runtime
        self._rt = runtime(dev)
        if not self._status:
            self._status = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in range(4)]
        status = self._status[self._n % len(self._status)]
        self._n += 1
        status.copy_(self._rt.state[1:2], non_blocking=True)       # rides the training stream, no synchronisation
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.issued.append((ev, plan, status, self._n - 1))
        if not self.threaded and next_batch is not None:
            self._retire(1)
            self.pending = self._start(next_batch, loss_weights)
        self._retire(2)


def train_step(model, optimizer, batch, loss_weights, num_hierarchy_levels=4, truncation=3.0,
               use_log_transform=True, weight_missing_geo=5.0, use_loss_masking=True, grad_sync=None,
               teacher_forced=False, prefetch=None, next_batch=None):
    """batch: device-resident dict in scene_dataloader.collate layout.  Returns (loss, losses, outputs).
    prefetch / next_batch (teacher-forced only): a GeometryPrefetcher and the batch of the following step."""
    inputs = batch['input']
    known = batch['known'] if use_loss_masking else None
    dev = batch['sdf'].device

    def targets():    # three launches on the device (sgnn_loss_targets); the batch tensors stay untouched
        return loss_util.compute_targets_and_weights(batch['sdf'], batch['hierarchy'], num_hierarchy_levels, truncation,
                                                     use_loss_masking, known, weight_missing_geo, inputs[0])

    optimizer.zero_grad(set_to_none=True)
    if teacher_forced and prefetch is not None:
        if tuple(prefetch.args) != (num_hierarchy_levels, truncation, use_loss_masking, weight_missing_geo):
            # the plan's targets / weights were built with the prefetcher's own settings
            raise ValueError('GeometryPrefetcher was built with (levels, truncation, masking, weight_missing_geo) = %r '
                             'but train_step was called with %r' % (tuple(prefetch.args), (
                                 num_hierarchy_levels, truncation, use_loss_masking, weight_missing_geo)))
        plan = prefetch.take(batch, loss_weights)
        prefetch.announce(next_batch, loss_weights)
        (tgt_sdf, tgt_occs, tgt_hier), weights = plan.targets, plan.weights
        output_sdf, output_occs = model(inputs, loss_weights, batch_size=int(batch['sdf'].shape[0]), teacher=tgt_occs,
                                        geometry=plan.geometry)
    elif teacher_forced:
        # generative masks come from the target occupancy pyramid: the targets are needed before the model runs
        (tgt_sdf, tgt_occs, tgt_hier), weights = targets()
        output_sdf, output_occs = model(inputs, loss_weights, batch_size=int(batch['sdf'].shape[0]), teacher=tgt_occs)
    elif dev.type == 'cuda' and OVERLAP_TARGETS:
        # targets and loss weights depend on the batch only (a dozen dense element-wise / pooling passes over the
        # (B,1,D,D,D) volumes): they run on a second stream underneath the encoder, whose small launches leave the
        # memory system idle; the loss waits for them
        side = _target_stream(dev)
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            (tgt_sdf, tgt_occs, tgt_hier), weights = targets()
        output_sdf, output_occs = model(inputs, loss_weights, batch_size=int(batch['sdf'].shape[0]))
        main.wait_stream(side)
    else:
        (tgt_sdf, tgt_occs, tgt_hier), weights = targets()
        output_sdf, output_occs = model(inputs, loss_weights, batch_size=int(batch['sdf'].shape[0]))
    loss, losses = loss_util.compute_loss(output_sdf, output_occs, tgt_sdf, tgt_occs, tgt_hier, loss_weights,
                                          truncation, use_log_transform, weight_missing_geo, inputs[0],
                                          use_loss_masking, known, weights=weights)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    optimizer.step()
    if teacher_forced and prefetch is not None:
        prefetch.step_issued(dev, plan, next_batch, loss_weights)
    return loss, losses, (output_sdf, output_occs)


def get_loss_weights(it, num_hierarchy_levels, num_iters_per_level, factor_l1_loss):
    """Curriculum of train.py:203-231 (level k fades in every num_iters_per_level iterations)."""
    w = np.zeros(num_hierarchy_levels + 1, dtype=np.float32)
    cur_level = it // num_iters_per_level
    if cur_level > num_hierarchy_levels:
        w.fill(1)
        w[-1] = factor_l1_loss
        return w
    w[:cur_level + 1] = 1.0
    step_factor = 20
    fade_amount = max(1.0, min(100, num_iters_per_level // step_factor))
    fade_level = it % num_iters_per_level
    cur_weight = 0.0
    if fade_level >= num_iters_per_level - fade_amount + step_factor:
        fade_level_step = (fade_level - num_iters_per_level + fade_amount) // step_factor
        cur_weight = float(fade_level_step) / float(fade_amount // step_factor)
    l1_weight = 0.0
    if cur_level + 1 < num_hierarchy_levels:
        w[cur_level + 1] = cur_weight
    elif cur_level < num_hierarchy_levels:
        l1_weight = factor_l1_loss * cur_weight
    else:
        l1_weight = 1.0
    w[-1] = l1_weight
    return w


# ---------------------------------------------------------------------------------------------------------------
# Flat-buffer Adam + the whole training step as a replayed HIP graph (capacity mode, scn/capacity.py)
# ---------------------------------------------------------------------------------------------------------------
def genmodel_segments(model):
    """Parameter segments of a GenModel in the order the optimizer lays them out: the encoder (always reached), one
    per Refinement and the SurfacePrediction — a generative stage without input sites leaves its parameters without a
    gradient in the reference (torch/model.py:211, 260), which Adam then skips."""
    segs = [('encoder', list(model.encoder.parameters()))]
    for h, r in enumerate(model.refinement):
        segs.append(('refinement.%d' % h, list(r.parameters())))
    segs.append(('surfacepred', list(model.surfacepred.parameters())))
    seen = set(id(p) for _, ps in segs for p in ps)
    rest = [p for p in model.parameters() if id(p) not in seen]
    if rest:
        segs[0] = ('encoder', segs[0][1] + rest)
    return segs


class FlatAdam(object):
    """Adam (torch/train.py:81) over ONE flat buffer: every parameter becomes a view of `flat_p`, gradients / moments
    live in `flat_g` / `flat_m` / `flat_v` with the same layout, and a step is one launch (sgnn_adam_flat) instead
    of torch's eight multi-tensor launches + host list walk.  Segments (see genmodel_segments) carry torch's "skip a
    parameter without gradient" rule to the device: a segment is updated iff it was reached this step.  Same update
    rule as torch.optim.Adam (bias-corrected, eps outside the square root, L2 weight decay added to the gradient);
    state_dict() / load_state_dict() speak torch.optim.Adam's format, so checkpoints move both ways."""

    def __init__(self, segments, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if segments and not isinstance(segments[0], (tuple, list)):
            segments = [('all', list(segments))]
        self.segments = [(name, [p for p in ps if p.requires_grad]) for name, ps in segments]
        self.params = [p for _, ps in self.segments for p in ps]
        assert self.params and len(self.segments) <= 7      # flag slot 7 of the gradient tail carries the overflow bit
        dev, dt = self.params[0].device, torch.float32
        self.numel = sum(p.numel() for p in self.params)
        nseg = len(self.segments)
        self.flat_p = torch.empty(self.numel, dtype=dt, device=dev)
        self.flat_g = torch.zeros(self.numel + 8, dtype=dt, device=dev)       # tail: per-segment "reached" flags
        self.flat_m = torch.zeros(self.numel, dtype=dt, device=dev)
        self.flat_v = torch.zeros(self.numel, dtype=dt, device=dev)
        self.steps = torch.zeros(8, dtype=dt, device=dev)                     # per-segment update counters
        self.lr_dev = torch.full((1,), float(lr), dtype=dt, device=dev)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.bounds, self.views_g, o = [], [], 0
        with torch.no_grad():
            for _, ps in self.segments:
                b = o
                for p in ps:
                    n = p.numel()
                    self.flat_p[o:o + n].copy_(p.detach().reshape(-1))
                    p.data = self.flat_p[o:o + n].view_as(p)
                    self.views_g.append(self.flat_g[o:o + n].view_as(p))
                    o += n
                self.bounds.append((b, o))
        self.flags = self.flat_g[self.numel:self.numel + nseg]
        self._direct = set()
        self.param_groups = [{'lr': float(lr), 'params': self.params}]        # what schedulers / loggers look at

    # -- learning rate (device scalar: a captured graph picks up changes) -------------------------------------
    def set_lr(self, lr):
        self.param_groups[0]['lr'] = float(lr)
        self.lr_dev.fill_(float(lr))

    # -- gradient plumbing ---------------------------------------------------------------------------------
    def bind_programs(self, model):
        """Parameters of compiled native programs get their gradient written straight into flat_g by the program's
        backward pass (scn/program.py).  Call after the model's first forward pass (programs compile lazily)."""
        from .scn import program as P_
        by_id = dict((id(p), v) for p, v in zip(self.params, self.views_g))
        for prog in P_.programs_of(model):
            for (m, nm), trainable in zip(prog.slots, prog.grad_slot):
                p = getattr(m, nm)
                if trainable and id(p) in by_id:
                    p._sgnn_flat_grad = by_id[id(p)]
                    p.grad = by_id[id(p)]
                    self._direct.add(id(p))

    def unbind(self):
        for p in self.params:
            if id(p) in self._direct:
                del p._sgnn_flat_grad
                p.grad = None
        self._direct = set()

    def zero_grad(self):
        """Before backward: autograd-delivered gradients start from None (set_to_none), direct ones are overwritten."""
        for p in self.params:
            if id(p) not in self._direct:
                p.grad = None

    def collect(self):
        """After backward: copy the autograd-delivered gradients into flat_g (one multi-tensor launch) and zero the slices
        of parameters that received none.  Returns the per-segment "some parameter has a gradient" list (host knowledge,
        exact mode).  Semantics are per SEGMENT (torch.optim.Adam skips per parameter): a parameter without a gradient
        inside a reached segment is updated from a zero gradient — its moments decay and weight decay applies; in GenModel
        a stage's parameters are reached together (torch/model.py:211, 260), so the two rules coincide there."""
        dst, src, reached, stale = [], [], [], []
        i = 0
        for _, ps in self.segments:
            any_grad = False
            for p in ps:
                v = self.views_g[i]
                i += 1
                if id(p) in self._direct:
                    any_grad = True
                elif p.grad is not None:
                    any_grad = True
                    dst.append(v)
                    src.append(p.grad)
                else:
                    stale.append(v)
            reached.append(any_grad)
        if dst:
            torch._foreach_copy_(dst, src)
        if stale:
            # a parameter nothing reached this step: its slice of flat_g still holds an EARLIER step's gradient (capacity
            # mode writes program gradients straight into the buffer).  Nothing may read that: a data-parallel all-reduce
            # sums the whole buffer, and a segment another rank reached is updated from the sum on every rank.
            torch._foreach_zero_(stale)
        return reached

    def zero_segments(self, which):
        """Zero the gradient slices of the segments flagged in `which` (one fill per segment; capturable)."""
        for (b, e), z in zip(self.bounds, which):
            if z and e > b:
                self.flat_g[b:e].zero_()

    def named_gradients(self, model):
        """{parameter name: what flat_g holds for it} — the gradients Adam consumes (after collect(): autograd-delivered
        ones copied in, program gradients written there by the backward kernels) — in the REFERENCE's layout (dense
        convolutions store (K, Cin, Cout), model.DenseConv).  For tests and tools; clones."""
        from .model import DenseConv
        view = dict((id(p), v) for p, v in zip(self.params, self.views_g))
        owners = {}
        for mn, mod in model.named_modules():
            if isinstance(mod, DenseConv):
                owners[(mn + '.' if mn else '') + 'weight'] = mod
        out = {}
        for n, p in model.named_parameters():
            g = view.get(id(p))
            if g is not None:
                g = g.detach().clone()
                g = owners[n].to_torch(g) if n in owners else g
            out[n] = g
        return out

    def _seg_table(self, cnts, use_flags):
        seg = np.zeros((len(self.segments), 5), dtype=np.int64)
        for t, (b, e) in enumerate(self.bounds):
            seg[t, 0], seg[t, 1] = b, e
            c = cnts[t] if cnts is not None else None
            seg[t, 2] = 0 if c is None else c.data_ptr()
            seg[t, 3] = (self.flags.data_ptr() + 4 * t) if use_flags else 0
            seg[t, 4] = self.steps.data_ptr() + 4 * t
        return np.ascontiguousarray(seg)

    def step(self, reached=None, cnts=None, status=None, grad_scale=1.0, flags_in_grads=False):
        """One update from flat_g.  Exactly one of: `reached` (host list of bools per segment, exact mode), `cnts`
        (device int64[1] row counts per segment or None = always, capacity mode), flags_in_grads (the flags at the tail
        of flat_g were filled by sgnn_seg_flags and summed by the all-reduce).  status: device int32 status word."""
        from . import _lib
        use_flags = flags_in_grads
        if reached is not None:
            self.flags.copy_(torch.tensor([1.0 if r else 0.0 for r in reached], dtype=torch.float32), non_blocking=True)
            use_flags = True
        seg = self._seg_table(cnts, use_flags)
        _lib.call('sgnn_adam_flat', self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(),
                  self.flat_v.data_ptr(), self.numel, seg.ctypes.data, len(self.segments), self.lr_dev.data_ptr(),
                  self.betas[0], self.betas[1], self.eps, self.weight_decay, float(grad_scale),
                  None if status is None else status.data_ptr())

    def write_flags(self, cnts, status=None):
        """flags tail of flat_g from the device row counts (before a data-parallel all-reduce of flat_g); with `status`
        (device int32 status word) slot 7 carries this rank's capacity-overflow bit."""
        from . import _lib
        ptrs = np.ascontiguousarray(np.array([0 if c is None else c.data_ptr() for c in cnts], dtype=np.int64))
        _lib.call('sgnn_seg_flags', ptrs.ctypes.data, len(self.segments), self.flags.data_ptr(),
                  None if status is None else status.data_ptr())

    def merge_overflow(self, status):
        """After the all-reduce: an overflow on any rank (summed flag in slot 7) becomes every rank's overflow."""
        from . import _lib
        _lib.call('sgnn_status_merge', self.flat_g.data_ptr() + 4 * (self.numel + 7), status.data_ptr())

    # -- torch.optim.Adam checkpoint format ------------------------------------------------------------------
    def state_dict(self):
        steps = self.steps.cpu().tolist()
        state, i, o = {}, 0, 0
        for t, (_, ps) in enumerate(self.segments):
            for p in ps:
                n = p.numel()
                if steps[t] > 0:
                    # (dense convolutions store (K, Cin, Cout): checkpoints carry the reference's layout)
                    conv = getattr(p, '_sgnn_dense', None)
                    ea, es = self.flat_m[o:o + n].view_as(p), self.flat_v[o:o + n].view_as(p)
                    state[i] = {'step': torch.tensor(float(steps[t])),
                                'exp_avg': conv.to_torch(ea) if conv is not None else ea.clone(),
                                'exp_avg_sq': conv.to_torch(es) if conv is not None else es.clone()}
                i += 1
                o += n
        group = {'lr': self.param_groups[0]['lr'], 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay,
                 'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False,
                 'fused': None, 'params': list(range(len(self.params)))}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        self.set_lr(g['lr'])
        self.betas, self.eps, self.weight_decay = (float(g['betas'][0]), float(g['betas'][1])), float(g['eps']), float(g['weight_decay'])
        self.flat_m.zero_()
        self.flat_v.zero_()
        steps = [0.0] * 8
        i, o = 0, 0
        for t, (_, ps) in enumerate(self.segments):
            for p in ps:
                n = p.numel()
                st = sd['state'].get(i)
                if st is not None:
                    conv = getattr(p, '_sgnn_dense', None)
                    ea, es = st['exp_avg'], st['exp_avg_sq']
                    if conv is not None and ea.dim() == 5:
                        ea, es = conv.to_native(ea), conv.to_native(es)
                    self.flat_m[o:o + n].copy_(ea.reshape(-1))
                    self.flat_v[o:o + n].copy_(es.reshape(-1))
                    steps[t] = max(steps[t], float(st['step']))
                i += 1
                o += n
        self.steps.copy_(torch.tensor(steps, dtype=torch.float32))


class GraphStep(object):
    """The training step of torch/train.py:245-268 (targets, forward, loss, backward, Adam) in CAPACITY MODE, captured
    once in a HIP graph and replayed: no host read-back, no Python, no per-kernel launch cost in the steady state.

        step = GraphStep(model, lr=1e-3)
        for batch in loader:                       # device-resident dicts in scene_dataloader.collate layout
            loss = step(batch, loss_weights)       # device scalar (valid until the next call)

    Life cycle per loss-weight pattern: (1) one classic step with read-backs, which also measures every level's row
    count -> capacities = counts x headroom (scn.capacity.Capacity); (2) one eager capacity-mode step (warm-up: lazy
    allocations, program compilation); (3) capture; (4) replay per batch — the batch is copied into the graph's static
    input buffers first (or written there directly: `buffers()`).  Every step's status word is checked one step late:
    after a capacity overflow (SGNN_STATUS_OVERFLOW: the step did not update the parameters) the capacities grow, the
    affected batch is run again and the graph is re-captured.  Masks are the reference's (sigmoid(pred) > 0.5) unless
    teacher_forced.  grad_sync (data parallel): called between backward and the optimizer with the flat gradient
    buffer; the step then replays as two graphs around it.  BatchNorm running statistics of an overflowed step are not
    rolled back (they see that batch twice; weights are exact)."""

    def __init__(self, model, lr=1e-3, weight_decay=0.0, num_hierarchy_levels=4, truncation=3.0, use_log_transform=True,
                 weight_missing_geo=5.0, use_loss_masking=True, teacher_forced=False, headroom=1.3, use_graph=True,
                 grad_sync=None, world_size=1, optimizer=None, settle=True, keep_outputs=False):
        self.model = model
        # keep_outputs: `self.outputs` = (output_sdf, output_occs) of the last step, detached, as the model returned them (capacity-
        # sized tensors whose live prefix is scn.capacity.trim(t); inside a replayed graph they are the graph's own static
        # tensors, valid until the next call).  teacher_volumes (with teacher_forced): dense occupancy volumes that decide
        # the generative masks INSTEAD of the batch's target hierarchy (parity tests force the oracle's masks this way);
        # the loss still uses the batch's targets.
        self.keep_outputs, self.outputs, self.teacher_volumes = bool(keep_outputs), None, None
        self.opt = optimizer if optimizer is not None else FlatAdam(genmodel_segments(model), lr=lr, weight_decay=weight_decay)
        self.args = (num_hierarchy_levels, truncation, use_log_transform, weight_missing_geo, use_loss_masking)
        self.teacher_forced, self.headroom, self.use_graph = teacher_forced, float(headroom), bool(use_graph)
        self.settle = bool(settle)      # False: capture right after the warm-up step (row counts known to be stable)
        self.grad_sync, self.world_size = grad_sync, int(world_size)
        self.capacity = None
        self.key = None                 # (which stages run, batch shape) the capacities / static buffers belong to
        self.weights = None             # the loss weights the captured graph has baked in
        self.stage = 0                  # 0: needs a probe step, 1: needs the eager capacity step, 2: captured
        self.graphs = None
        self.static = None
        self.loss = None
        self.losses = None
        self.pending = []               # [(event, pinned status, batch, loss_weights, ...)] of issued steps, oldest first
        self.slot_batch = None          # the batch whose gradients the current slot's grad_sync call carries ...
        self.slot_kind = None           # ... and the kind of step that produced them: 'probe' | 'eager' | 'replay'
        self.stats = {'probe_steps': 0, 'eager_steps': 0, 'captures': 0, 'replays': 0, 'overflows': 0, 'replans': 0,
                      'replay_host_ms': 0.0}
        self._pins, self._npin = None, 0
        self.overflow_log = []          # diagnostics: which levels were full in the steps that overflowed (see _check)
        self._bound = False
        try:
            hwq = int(os.environ.get('GPU_MAX_HW_QUEUES', '4'))
        except ValueError:
            hwq = 4
        if self.use_graph and hwq > 4:
            import warnings
            warnings.warn('GPU_MAX_HW_QUEUES=%d: with more than 4 hardware queues two concurrently active branches of the '
                          'replayed step (training chain / side lane) were measured to share one hardware pipe on MI355X — '
                          '17-19 ms instead of 6 ms per step (HISTORY.md section 5a).  Leave it at the default of 4.' % hwq)

    # -- pieces --------------------------------------------------------------------------------------------
    @staticmethod
    def _detached(out_sdf, out_occs):
        """The model's outputs without their autograd graph (same storage, live counts kept).  A caller that holds
        the graph of an earlier step across a capturing call makes autograd re-use AccumulateGrad nodes created on another
        stream — a cross-stream synchronisation inside the capture, which HIP answers with a crash in hipStreamEndCapture."""
        def d(t):
            return carry(t.detach(), t, 'cnt', 'cnt8') if torch.is_tensor(t) else t
        return [d(t) for t in out_sdf], [[d(t) for t in o] for o in out_occs]

    def _teacher(self, toccs):
        if not self.teacher_forced:
            return None
        return self.teacher_volumes if self.teacher_volumes is not None else toccs

    def _probe(self, batch, loss_weights):
        """Classic step (read-backs) that also sizes the capacities."""
        from .scn import metadata as MD
        nl, trunc, use_log, wgeo, masking = self.args
        self.slot_batch, self.slot_kind = batch, 'probe'       # (what this slot's all-reduce carries: tests log it)
        self.opt.unbind()
        self._bound = False
        MD.runtime(batch['sdf'].device).state[1:2].zero_()     # a discarded capacity step may have left its overflow flag
        MD.COUNT_LOG = []
        try:
            self.opt.zero_grad()
            known = batch['known'] if masking else None
            (tsdf, toccs, thier), weights = loss_util.compute_targets_and_weights(
                batch['sdf'], batch['hierarchy'], nl, trunc, masking, known, wgeo, batch['input'][0])
            B = int(batch['sdf'].shape[0])
            out_sdf, out_occs = self.model(batch['input'], loss_weights, batch_size=B, teacher=self._teacher(toccs))
            if self.keep_outputs:
                self.outputs = self._detached(out_sdf, out_occs)
            loss, losses = loss_util.compute_loss(out_sdf, out_occs, tsdf, toccs, thier, loss_weights, trunc, use_log, wgeo,
                                                  batch['input'][0], masking, known, weights=weights)
            loss.backward()
            reached = self.opt.collect()
            if self.grad_sync is not None:
                # A probe step takes part in the SAME protocol as a capacity step (one all-reduce of flat_g + flags, merged
                # overflow bit, status-gated update, status word retired one step late): whatever kind of step a peer runs
                # in this slot, both ranks issue one collective, apply or skip the same update, and re-run their own batch
                # if ANY rank overflowed (a probe used to apply its update while an overflowing peer skipped it).
                rt = MD.runtime(batch['sdf'].device)
                self.opt.flat_g[self.opt.numel:].zero_()          # flag slots (slot 7: overflow, none on the classic path)
                self.opt.flags.copy_(torch.tensor([1.0 if r else 0.0 for r in reached], dtype=torch.float32))
                self.grad_sync(self.opt.flat_g)
                self.opt.merge_overflow(rt.status32)
                self.opt.step(flags_in_grads=True, grad_scale=1.0 / self.world_size, status=rt.status32)
                self._issue_status(batch, loss_weights, probe=True)
            else:
                self.opt.step(reached=reached)
            log = MD.COUNT_LOG
        finally:
            MD.COUNT_LOG = None
        from .scn.capacity import Capacity
        dev = batch['sdf'].device
        runs = self.model._runs(loss_weights)
        n_gen = 1 + sum(1 for r in runs[:-1] if r)      # the coarse compaction + one per running refinement
        new = Capacity.from_log(dev, log, self.headroom, n_gen=n_gen)
        if self.capacity is not None:        # never shrink below what an earlier batch needed
            old = self.capacity
            new = Capacity(dev, max(new.input_rows, old.input_rows),
                           [max(a, b) for a, b in zip(new.enc, old.enc)] if len(old.enc) == len(new.enc) else new.enc,
                           [(max(k, ko), [max(a, b) for a, b in zip(p, po)]) for (k, p), (ko, po) in zip(new.gen, old.gen)]
                           if len(old.gen) == len(new.gen) else new.gen)
        self.capacity = new
        self._live, self._hist = None, []        # counts read back so far belong to the plan this one replaces
        self.stats['probe_steps'] += 1
        self.loss, self.losses = loss.detach(), losses
        return self.loss

    def _make_static(self, batch):
        cap = self.capacity
        dev = batch['sdf'].device
        locs, feats = batch['input']
        st = {'locs': torch.zeros(cap.input_rows, 4, dtype=torch.int64, device=dev),
              'feats': torch.zeros(cap.input_rows, feats.shape[1], dtype=torch.float32, device=dev),
              'sdf': torch.empty_like(batch['sdf']),
              'known': torch.empty_like(batch['known']) if batch.get('known') is not None else None,
              'hierarchy': [torch.empty_like(h) for h in (batch.get('hierarchy') or [])]}
        attach(st['locs'], cnt=cap.input_cnt())
        self.static = st

    def buffers(self):
        """The graph's static input buffers (read-only view for tools and tests: a step always takes its batch as an
        argument and copies it in — `_load` also publishes the live input row count, which a writer into these buffers could
        not do)."""
        return self.static

    def _load(self, batch):
        st = self.static
        locs, feats = batch['input']
        n = int(locs.shape[0])
        self.capacity.set_input_rows(n)
        pairs = [(st['locs'][:n], locs), (st['feats'][:n], feats), (st['sdf'], batch['sdf'])]
        if st['known'] is not None:
            pairs.append((st['known'], batch['known']))
        pairs += list(zip(st['hierarchy'], batch.get('hierarchy') or []))
        ok = len(pairs) <= 8 and all(d.dtype == s_.dtype and d.shape == s_.shape and d.is_contiguous() and s_.is_contiguous()
                                     and s_.device == d.device for d, s_ in pairs)
        if ok:     # one launch instead of one copy kernel per tensor (each ~6 us in front of the replayed step)
            from . import _lib
            dst = np.ascontiguousarray(np.array([d.data_ptr() for d, _ in pairs], dtype=np.uint64))
            src = np.ascontiguousarray(np.array([s_.data_ptr() for _, s_ in pairs], dtype=np.uint64))
            nb = np.ascontiguousarray(np.array([d.numel() * d.element_size() for d, _ in pairs], dtype=np.int64))
            _lib.call('sgnn_copy_multi', dst.ctypes.data, src.ctypes.data, nb.ctypes.data, len(pairs))
        else:      # host-resident or non-contiguous pieces: torch's copies (dtype / layout conversion, H2D)
            for d, s_ in pairs:
                d.copy_(s_, non_blocking=True)

    def _fwd_bwd(self, loss_weights):
        """Capacity-mode targets + forward + loss + backward on the static buffers (capturable)."""
        from .scn.metadata import runtime
        nl, trunc, use_log, wgeo, masking = self.args
        st, cap = self.static, self.capacity
        rt = runtime(st['sdf'].device)
        rt.state[1:2].zero_()                       # status word of THIS step
        self.opt.zero_grad()
        known = st['known'] if masking else None
        # (the targets were tried on the side lane, under the encoder: no gain, profiles/r03w_hw_queues.txt)
        (tsdf, toccs, thier), weights = loss_util.compute_targets_and_weights(
            st['sdf'], st['hierarchy'], nl, trunc, masking, known, wgeo, st['locs'])
        B = int(st['sdf'].shape[0])
        out_sdf, out_occs = self.model([st['locs'], st['feats']], loss_weights, batch_size=B, capacity=cap,
                                       teacher=self._teacher(toccs))
        if self.keep_outputs:
            self.outputs = self._detached(out_sdf, out_occs)
        loss, losses = loss_util.compute_loss(out_sdf, out_occs, tsdf, toccs, thier, loss_weights, trunc, use_log, wgeo,
                                              st['locs'], masking, known, weights=weights)
        from .scn import metadata as MD, program as P_
        # program weight gradients land in the flat buffer nobody reads before Adam: ONE join of the lane at the end of the
        # backward pass instead of one per program (scn.program.DEFER_JOIN / sgnn_prog_defer_join; a program's last weight
        # gradient otherwise holds up the next program's chain).  (The dense bottleneck's six weight gradients were tried on
        # the lane as well: no gain, profiles/r03w_hw_queues.txt.)
        defer = MD.SIDE_LANE and os.environ.get('SGNN_DEFER_JOIN', '1') != '0'
        prev_defer, P_.DEFER_JOIN = P_.DEFER_JOIN, defer
        try:
            loss.backward()
        finally:
            P_.DEFER_JOIN = prev_defer
            MD.join_pyramid_lane(st['sdf'].device)      # (also after an exception: nothing may outlive the keep-alive list)
            del P_._deferred[:]
        self.opt.collect()           # gradients autograd delivered (dense bottleneck); program gradients are in flat_g already
        if self.grad_sync is not None:
            # a stage these loss weights switch off runs no kernel at all, so nothing writes its slice of flat_g: make sure
            # the all-reduce sums zeros there, not whatever an earlier curriculum stage left
            self.opt.zero_segments([not a for a in self._active_segments(loss_weights)])
        return loss.detach(), losses, rt

    def _seg_cnts(self, loss_weights):
        """Device row count deciding whether a segment was reached: encoder always; Refinement h <- kept rows of
        generative level h; SurfacePrediction <- kept rows of the last level."""
        cap = self.capacity
        R = len(self.model.refinement)
        cnts = [None]
        for h in range(R + 1):
            cnts.append(cap.kept2(h)[0:1] if h < len(cap.gen) else None)
        return cnts[:len(self.opt.segments)]

    def _active_segments(self, loss_weights):
        """Segments whose stage runs at all with these loss weights (static per graph)."""
        runs = self.model._runs(loss_weights)
        return [True] + [bool(r) for r in runs]

    def _opt_step(self, loss_weights, rt):
        cnts = self._seg_cnts(loss_weights)
        active = self._active_segments(loss_weights)
        # a stage that does not run at all has no gradient: park its segment on a zero count
        zero = self.capacity.counts[SLOT_ZERO:SLOT_ZERO + 1]
        cnts = [(c if a else zero) for c, a in zip(cnts, active)]
        if self.grad_sync is not None:
            self.opt.step(flags_in_grads=True, status=rt.status32, grad_scale=1.0 / self.world_size)
        else:
            self.opt.step(cnts=cnts, status=rt.status32)

    def _capacity_step_eager(self, loss_weights):
        loss, losses, rt = self._fwd_bwd(loss_weights)
        if self.grad_sync is not None:
            cnts = self._seg_cnts(loss_weights)
            active = self._active_segments(loss_weights)
            zero = self.capacity.counts[SLOT_ZERO:SLOT_ZERO + 1]
            self.opt.write_flags([(c if a else zero) for c, a in zip(cnts, active)], rt.status32)
            self.grad_sync(self.opt.flat_g)
            self.opt.merge_overflow(rt.status32)
        self._opt_step(loss_weights, rt)
        return loss, losses, rt

    def _issue_status(self, batch, loss_weights, probe=False):
        """Queue this step's status word (+ the live row counts) for a read one step late.  probe: a classic step under
        data parallelism — it has no row counts of its own, only the merged overflow bit of its all-reduce slot.
        (Everything device-specific of a slot lives in this method and in the step kinds it follows — _probe,
        _capacity_step_eager, _capture / _replay: tests/test_dp_protocol_sim.py replaces exactly those and drives the
        protocol logic of __call__ / _check / _overflow / _maybe_replan with two simulated ranks on the CPU.)"""
        from .scn.metadata import runtime
        rt = runtime(batch['sdf'].device)
        if self._pins is None:      # [status word | the capacity's 64 live row counts], per in-flight step
            self._pins = [torch.zeros(65, dtype=torch.int64).pin_memory() for _ in range(8)]
        pin = self._pins[self._npin % len(self._pins)]
        self._npin += 1
        pin[0:1].copy_(rt.state[1:2], non_blocking=True)
        if not probe:
            pin[1:].copy_(self.capacity.counts, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(rt.device))
        self._n_issued = getattr(self, '_n_issued', 0) + 1
        # (the entry also keeps what the step's kernels touch alive until the host has seen the step end: under data
        # parallelism a rank-local re-plan drops self.graphs / self.static while their last replay may still be in flight)
        alive = None if probe else (self.graphs, self.static, getattr(self, '_keep', None))
        self.pending.append((ev, pin, batch, loss_weights, None if probe else self.capacity, self._n_issued - 1, alive))

    def _check(self, keep):
        """Retire all but the `keep` newest issued steps; returns the batches whose step overflowed."""
        redo = []
        while len(self.pending) > keep:
            ev, pin, batch, lw, cap, index, _alive = self.pending.pop(0)
            ev.synchronize()
            word = int(pin[0]) & 0xFFFFFFFF
            if cap is not None and cap is self.capacity and not (word & 4):
                # (never from a step that overflowed: its producers CLAMPED their counts to the capacities, and a re-plan
                #  sized from clamped counts shrinks exactly the levels that were too small — tests/test_gpu_dp_protocol.py
                #  scenario C found a plan re-sized to 2 x 1024 rows for a 10 k-row level this way)
                self._live = pin[1:].tolist()
            if word & 4 and not (word & 3):
                redo.append((batch, lw))
                # which of THIS rank's levels hit their capacity (a producer clamps its count to the capacity when it
                # overflows; none = the overflow came from a peer's merged bit): [(step index, [(level, rows, capacity)])]
                full = [] if cap is None else [(i, int(n), int(c)) for i, (n, c) in
                                                enumerate(self._levels(pin[1:].tolist(), cap)) if n >= c]
                self.overflow_log.append((index, full))
                del self.overflow_log[:-32]
            elif word:
                from .scn.metadata import runtime
                runtime(batch['sdf'].device).raise_status(
                    word, 'raised by capacity-mode step %d of this GraphStep (0-based), %d step(s) ago; that step\'s '
                          'parameter update was applied' % (index, self._n_issued - 1 - index))
        return redo

    def _capture(self, loss_weights):
        from .scn.metadata import runtime
        dev = self.static['sdf'].device
        rt = runtime(dev)
        torch.cuda.synchronize(dev)
        from . import _lib
        if _lib.STAMPS:
            _lib.load().sgnn_stamp_reset()             # (scripts/lane_stamps.py) slots in capture order
        if self.grad_sync is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss, losses, _ = self._fwd_bwd(loss_weights)
                self._opt_step(loss_weights, rt)
            self.graphs = (g,)
        else:
            g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):
                loss, losses, _ = self._fwd_bwd(loss_weights)
                cnts = self._seg_cnts(loss_weights)
                active = self._active_segments(loss_weights)
                zero = self.capacity.counts[SLOT_ZERO:SLOT_ZERO + 1]
                self.opt.write_flags([(c if a else zero) for c, a in zip(cnts, active)], rt.status32)
            with torch.cuda.graph(g2, pool=g1.pool()):
                self.opt.merge_overflow(rt.status32)
                self._opt_step(loss_weights, rt)
            self.graphs = (g1, g2)
        self._graph_out = (loss, losses)
        self._graph_outputs = self.outputs       # (keep_outputs) the graph's own static output tensors
        # everything the captured kernels touch outside the graph's own pool must outlive the graph
        self._keep = (rt.ws, getattr(rt, '_side_ws', None), getattr(rt, '_volume', None), self.capacity, self.static)
        self.stats['captures'] += 1

    def _replay(self):
        import time
        t0 = time.perf_counter()
        if len(self.graphs) == 1:
            self.graphs[0].replay()
        else:
            self.graphs[0].replay()
            self.grad_sync(self.opt.flat_g)
            self.graphs[1].replay()
        self.stats['replay_host_ms'] += 1e3 * (time.perf_counter() - t0)     # host time inside hipGraphLaunch
        self.stats['replays'] += 1
        self.outputs = self._graph_outputs
        return self._graph_out

    # -- the step -------------------------------------------------------------------------------------------
    def __call__(self, batch, loss_weights):
        """One training step = one SLOT.  Under data parallelism (grad_sync) every slot is exactly one all-reduce on every
        rank, whatever kind of step the rank runs in it (probe / eager capacity step / replay), and every rank retires its
        status words at the same depth: slot k's word is read right after slot k+1 has been issued, never earlier — so the
        common decisions (skip the update, re-run the batch) happen at the same point of every rank's collective sequence.
        Rank-local decisions (this rank's input outgrew its capacity, this rank re-plans) only choose the KIND of step the
        rank runs in a slot; they neither retire anything nor issue a collective.  What must be common to all ranks of a
        slot: the loss weights and the batch SHAPE (they decide `key`), and calls to replan()."""
        loss_weights = np.asarray(loss_weights, dtype=np.float32)
        self.outputs = None
        dp = self.grad_sync is not None
        key = (tuple(bool(w > 0) for w in loss_weights), tuple(batch['sdf'].shape))
        wkey = tuple(float(w) for w in loss_weights)
        if key != self.key:                          # new curriculum stage / batch shape: re-size and re-capture
            self._drain()                            # (common to all ranks: see above)
            self.key, self.stage, self.graphs, self.capacity = key, 0, None, None
        if wkey != self.weights:                     # the loss weights are baked into the captured launches
            self._drain()
            self.weights, self.graphs = wkey, None
        n_in = int(batch['input'][0].shape[0])
        if self.stage == 0 or n_in > self.capacity.input_rows:
            # no plan yet, or (known on the host before anything is launched) the input level outgrew it: a classic step
            # that also measures every level.  Rank-local under data parallelism: nothing in flight is retired here (the
            # step before may carry a merged overflow that the peers will only see after THEIR next slot) — the pending
            # entries keep the graph / buffers of their step alive instead.
            if self.stage != 0 and not dp:
                self._drain()
            self.graphs = None
            self._probe(batch, loss_weights)
            self.stage = 1
            if not dp:
                return self.loss
        else:
            if self.stage == 1:
                self._make_static(batch)
            self._load(batch)
            if not self._bound:                          # programs were compiled by the probe step
                self.opt.bind_programs(self.model)
                self._bound = True
            self.slot_batch, self.slot_kind = batch, ('eager' if self.stage in (1, 2) else 'replay')
            if self.stage in (1, 2):                     # eager capacity steps: warm-up, and while the row counts settle
                loss, losses, _ = self._capacity_step_eager(loss_weights)     # (use_graph=False: forever)
                self.stats['eager_steps'] += 1
                if self.stage == 1:
                    self.stage = 3 if (self.use_graph and self.settle is False) else 2
            else:
                if self.graphs is None:
                    self._capture(loss_weights)
                loss, losses = self._replay()
            self._issue_status(batch, loss_weights)
            self.loss, self.losses = loss, losses
        redo = self._check(1)
        if redo:
            self._overflow(redo)
        else:
            self._maybe_replan()
        return self.loss

    def _levels(self, live, cap=None):
        """[(live rows, capacity)] of every count the plan (default: the current one) tracks."""
        from .scn.capacity import ENC0
        cap = self.capacity if cap is None else cap
        pairs = [(live[0], cap.input_rows)] + [(live[ENC0 + l], c) for l, c in enumerate(cap.enc)]
        for g, (k, pyr) in enumerate(cap.gen):
            b = cap.gen_base(g)
            pairs.append((live[b], k))
            pairs += [(live[b + 2 + l], c) for l, c in enumerate(pyr)]
        return pairs

    def _maybe_replan(self):
        """Row counts drift while the weights train (the masks are predictions) — fast right after initialisation, slowly
        later.  Capturing a graph costs a few hundred ms, an eager capacity-mode step about what a classic step costs.
        So: while the live counts (they ride back with every step's status word, one step late) are still moving or do
        not fit the plan, steps run eagerly and the plan follows the counts for free; once the counts of the last three
        steps agree within 15 % and fit, the step is captured and replayed.  A replaying step drops back to the eager
        phase when a level comes close to its capacity (before it overflows) or the plan has become more than twice as
        large as needed (kernels are launched for the capacities)."""
        live, cap = getattr(self, '_live', None), self.capacity
        if live is None or self.stage < 2:
            return
        from .scn.capacity import Capacity, ENC0, _round
        self._live = None
        pairs = self._levels(live)
        need = lambda n: _round(max(int(n * self.headroom), 1024))
        tight = any(n > (1.0 - 0.2 * min(self.headroom - 1.0, 0.4)) * c for n, c in pairs)
        have, want = sum(c for _, c in pairs), sum(need(n) for n, _ in pairs)
        hist = self.__dict__.setdefault('_hist', [])
        hist.append([n for n, _ in pairs])
        del hist[:-3]
        stable = len(hist) == 3 and all(max(v) <= 1.15 * max(min(v), 256) for v in zip(*hist))
        replaying = self.stage == 3 and self.graphs is not None
        if replaying:
            self._loose = (getattr(self, '_loose', 0) + 1) if have > 2.0 * want else 0
            if not (tight or self._loose >= 5):
                return
        else:
            if self.use_graph and self.stage == 2 and stable and not tight and have <= 1.5 * want:
                self.stage = 3                      # settled and fitting: capture on the next call
                return
            if not (tight or have > 1.5 * want):
                return
        # re-size from the live counts (moving up: leave more room than the steady-state headroom)
        self._loose = 0
        if self.grad_sync is None:
            self._drain()
            if self.stage < 2:                 # the drain found an overflow and re-planned already
                return
        # (data parallel: a re-plan is THIS rank's decision, so it must not retire the newest step's status word — that
        # word may carry a merged overflow, and acting on it one slot before the peers do would put this rank's re-run
        # all-reduce opposite the peers' next batch ("What's weak" 1).  The step in flight finishes on the
        # old plan — its pending entry keeps graph and buffers alive — and a late overflow grows the NEW plan.)
        self._resize(live, 1.25 if tight else 1.0)

    def _resize(self, live, grow=1.0):
        from .scn.capacity import Capacity, ENC0, _round
        cap = self.capacity
        nn = lambda n: _round(max(int(n * self.headroom * grow), 1024))
        b = cap.gen_base
        self.capacity = Capacity(cap.device, nn(live[0]), [nn(live[ENC0 + l]) for l in range(len(cap.enc))],
                                 [(nn(live[b(g)]), [nn(live[b(g) + 2 + l]) for l in range(len(pyr))])
                                  for g, (k, pyr) in enumerate(cap.gen)])
        self.graphs, self.stage = None, 1
        self._hist = []
        self.stats['replans'] += 1

    def replan(self):
        """Re-size every capacity to `headroom` x the current live row counts NOW (one synchronisation), e.g. before a
        phase that should not be interrupted by a re-plan of its own: the following calls run eagerly until the counts
        are stable again, then the step is re-captured."""
        if self.capacity is None or self.stage < 2:
            return
        self._drain()
        if self.stage < 2:
            return
        torch.cuda.synchronize(self.capacity.device)
        self._live = None
        self._resize(self.capacity.counts.tolist())

    def _drain(self):
        redo = self._check(0)
        if redo:
            self._overflow(redo)

    def _overflow(self, redo):
        """Some issued step overflowed a capacity (it left the parameters untouched): finish what is in flight, grow,
        run the affected batches again through the classic path, re-capture on the next call."""
        redo = redo + self._check(0)
        self.stats['overflows'] += len(redo)
        self.graphs = None
        self.capacity = self.capacity.grown(1.5)
        for batch, lw in redo:
            self._probe(batch, lw)
        self.stage = 1


SLOT_ZERO = 63      # a count slot that is always 0 (Capacity.counts is zero-initialised and nothing writes there)
