"""A plain interpreter of a compiled program (sgnn_amd/scn/program.py: ops_np / bufs_np / opf_np) in torch float64 on the
CPU: the yardstick for the native executor (sgnn_prog_forward / sgnn_prog_backward, prog.hip).

It shares nothing with the executor's plan: every op is evaluated into a fresh tensor (no fusion, no views, no gradient
state machine) and every gradient comes from torch.autograd over that forward.

  SUBM / DOWN   rulebook walks over the 27-column neighbour table / the 8-column children table
  UNPOOL        out[i] = in[parent[i]]
  BN            bn_ref's rules: batch statistics (biased variance) in training with the running-statistics update
                (momentum = weight of the OLD value, unbiased variance), running statistics in eval; leaky ReLU
  ADD / JOIN    sum / column concatenation
  CONCAT_IN     [in0[ia] | in1[ib] | in2[ic]]; a negative index gives a zero row, no index array = rows as they are
  EXPAND        a true 27-offset submanifold convolution over the 8N children (row 8p + g at 2 c_p + (g>>2&1, g>>1&1, g&1))
                whose rulebook is built here from the parents' coordinates — never through the 64 pre-summed slices
  LINEAR        out[:, q] = x w_q^T + b_q  (weight slot par + 2q, bias par + 2q + 1)

run(..., dtype=torch.float32) is the same interpreter in float32: its distance to the float64 run is the error an
honest fp32 evaluation of the same program makes (e_ref32 of the comparison rules, see test_gpu_prog_fp64.py).
run(..., abs_terms=True) evaluates the program on |parameters|, |inputs| and |output gradients|: every value it returns
bounds the sum of |terms| behind the corresponding value of the plain run (integer cases: must stay below 2^24).

run(..., storage='bf16') is the yardstick of the bf16 executor (forward_bf16, prog.hip; test_gpu_prog_bf16.py): forward
only, eval, still float64 arithmetic, but every value is rounded to bf16 (to nearest even, straight from float64) where
the executor stores one: convolution weights before use (EXPAND: its 27 weights, never the 64 pre-summed slices), the
output of every op except LINEAR, and an external where an op other than CONCAT_IN reads it (CONCAT_IN rounds its
result).  BatchNorm parameters, running statistics, head weights and biases stay as they are.  It never looks at the
plan: it rounds behind every op, fused or not.

`mutate` names one deliberate mistake (MUTATIONS); test_prog_ref.py shows that the comparison bars notice each of them.
"""
import numpy as np
import torch

import conv_ref

OP_SUBM, OP_DOWN, OP_UNPOOL, OP_BN, OP_ADD, OP_JOIN, OP_CONCAT_IN, OP_EXPAND, OP_LINEAR = range(9)

MUTATIONS = ('add_drops_addend', 'join_swaps_columns', 'second_reader_gradient_dropped', 'running_stats_in_training',
             'unpool_gradient_drops_a_child', 'head_data_gradient_dropped', 'batch_stats_in_eval', 'external_not_rounded')


def round_bf16(t):
    """float64 -> the nearest bf16 value (ties to even), as float64; one rounding, not float64 -> float32 -> bf16.
    (Normal range only: bf16 shares float32's exponent range, which no case comes near.)"""
    assert t.dtype == torch.float64
    u = t.detach().contiguous().clone().view(torch.int64)      # sign-magnitude: adding to the integer grows the magnitude
    u += (1 << 44) - 1 + ((u >> 45) & 1)
    u &= ~((1 << 45) - 1)
    return u.view(torch.float64)


class Geometry(object):
    """Integer tables of a pyramid, CPU int64: coords[l] (n_l, 4) [z, y, x, b] (level 0 is enough), nbr[l] (27, n_l),
    children[l] (8, n_{l+1}) and parent[l] (n_l,) for the transition l -> l + 1."""

    def __init__(self, coords0, nbr, children, parent):
        self.coords0 = torch.as_tensor(coords0).long()
        self.nbr = [torch.as_tensor(t).long() for t in nbr]
        self.children = [torch.as_tensor(t).long() for t in children]
        self.parent = [torch.as_tensor(t).long() for t in parent]
        self.n = [int(t.shape[1]) for t in self.nbr]
        self._child_nbr = None

    def child_nbr(self):
        if self._child_nbr is None and self.n[0] == 0:
            self._child_nbr = torch.zeros(27, 0, dtype=torch.long)
        if self._child_nbr is None:
            self._child_nbr = conv_ref.subm_rulebook(conv_ref.children_coords(self.coords0))
        return self._child_nbr


def oracle_geometry(coords0, nlev):
    """Geometry from coordinates alone, through the oracle's rulebooks (oracle/scn_oracle)."""
    import scn_oracle as oscn
    g = oscn.Grid(np.asarray(coords0, dtype=np.int64))
    c0 = g.coords.copy()
    nbr, children, parent = [], [], []
    for l in range(nlev):
        nbr.append(g.subm_rules(3).reshape(27, g.n))
        if l + 1 < nlev:
            coarse, par, off = oscn.down2_rules(g)
            ch, _, _ = oscn.down_tables(par, off, coarse.n)
            children.append(ch.reshape(8, coarse.n))
            parent.append(par)
            g = coarse
    return Geometry(c0, nbr, children, parent)


def _walk(x, w, table):
    """y[j] = sum_k x[table[k][j]] @ w[k] over the entries >= 0 (differentiable)."""
    y = x.new_zeros(table.shape[1], w.shape[2])
    for k in range(table.shape[0]):
        m = (table[k] >= 0).nonzero()[:, 0]
        if m.numel():
            y = y.index_add(0, m, x.index_select(0, table[k][m]) @ w[k])
    return y


class _UnpoolDroppingAChild(torch.autograd.Function):
    """UNPOOL whose gradient forgets the fine rows in child slot 7 (mutation)."""

    @staticmethod
    def forward(ctx, x, parent, children):
        ctx.save_for_backward(parent, children)
        ctx.n = x.shape[0]
        return x.index_select(0, parent)

    @staticmethod
    def backward(ctx, dy):
        parent, children = ctx.saved_tensors
        keep = torch.ones(parent.shape[0], dtype=torch.bool)
        keep[children[7][children[7] >= 0]] = False
        dx = dy.new_zeros(ctx.n, dy.shape[1]).index_add(0, parent[keep], dy[keep])
        return dx, None, None


def run(ops, bufs, opf, n_ext, rows, geom, params, ext, idx=(), training=True, gouts=None, dtype=torch.float64,
        abs_terms=False, mutate=None, storage=None):
    """ops (nops, 12), bufs (nbuf, 2), opf (nops, 4) as compiled; rows[c] the row count of rows class c; params[slot]
    tensors (None allowed); ext[b] the external tensors (None allowed); idx[i] integer arrays; gouts {buffer: gradient}.
    Returns a dict: 'bufs' (every buffer, detached), 'running' {slot: new value} (training), 'pre' {op: BatchNorm
    pre-activation t}, 'pre_mag' {op: |xhat gamma| + |beta|}, and with gouts 'gparams' [per slot, None for running
    statistics] and 'gext' [per external]; gradients nothing reaches are zeros.  storage='bf16': see the module's text."""
    assert mutate is None or mutate in MUTATIONS
    assert storage in (None, 'bf16')
    bf = storage == 'bf16'
    assert not bf or (dtype == torch.float64 and gouts is None and not training)
    rnd = round_bf16 if bf else (lambda t: t)
    ops, bufs, opf = np.asarray(ops), np.asarray(bufs), np.asarray(opf)
    prep = (lambda t: t.detach().abs()) if abs_terms else (lambda t: t.detach())
    P = [None if p is None else prep(p.cpu()).to(dtype).clone().requires_grad_(not bf) for p in params]
    E = [None if e is None else prep(e.cpu()).to(dtype).clone().requires_grad_(not bf) for e in ext]
    I = [None if i is None else torch.as_tensor(i).cpu().long() for i in idx]
    B = [None] * bufs.shape[0]
    for b in range(n_ext):
        B[b] = E[b]
    seen = set()
    out = {'running': {}, 'pre': {}, 'pre_mag': {}}

    def read(b, raw=False):
        t = B[b]
        if b < n_ext and not raw and mutate != 'external_not_rounded':
            t = rnd(t)
        if mutate == 'second_reader_gradient_dropped' and b in seen:
            t = t.detach()
        seen.add(b)
        return t

    for i in range(ops.shape[0]):
        t, in0, in1, ob, par, lev, cin, cout, in2, ia, ib, ic = (int(v) for v in ops[i])
        if t == OP_SUBM:
            y = _walk(read(in0), rnd(P[par]), geom.nbr[lev])
        elif t == OP_DOWN:
            y = _walk(read(in0), rnd(P[par]), geom.children[lev])
        elif t == OP_UNPOOL:
            if mutate == 'unpool_gradient_drops_a_child':
                y = _UnpoolDroppingAChild.apply(read(in0), geom.parent[lev], geom.children[lev])
            else:
                y = read(in0).index_select(0, geom.parent[lev])
        elif t == OP_BN:
            assert not abs_terms, 'sums of |terms| are for programs without BatchNorm'
            x = read(in0)
            gamma, beta, rm, rv = P[par], P[par + 1], P[par + 2], P[par + 3]
            eps, mom, leak = float(opf[i][0]), float(opf[i][1]), float(opf[i][2])
            n = x.shape[0]
            if (training and mutate != 'running_stats_in_training') or mutate == 'batch_stats_in_eval':
                if n:
                    mean = x.sum(0) / n
                    var = ((x - mean) ** 2).sum(0) / n
                    invstd = 1.0 / torch.sqrt(var + eps)
                    unb = var.detach() * (n / (n - 1) if n > 1 else 1.0)
                    out['running'][par + 2] = (mom * rm + (1 - mom) * mean).detach()
                    out['running'][par + 3] = (mom * rv + (1 - mom) * unb).detach()
                else:
                    mean = invstd = x.new_zeros(cin)
                    out['running'][par + 2], out['running'][par + 3] = rm.detach(), rv.detach()
            else:
                mean, invstd = rm.detach(), 1.0 / torch.sqrt(rv.detach() + eps)
            xhat = (x - mean) * invstd
            pre = xhat * gamma + beta
            out['pre'][i] = pre.detach()
            out['pre_mag'][i] = ((xhat * gamma).abs() + beta.abs()).detach()
            y = torch.where(pre > 0, pre, pre * leak)
        elif t == OP_ADD:
            a, b = read(in0), read(in1)
            y = a + 0 * b if mutate == 'add_drops_addend' else a + b
        elif t == OP_JOIN:
            a, b = read(in0), read(in1)
            y = torch.cat([b, a], 1) if mutate == 'join_swaps_columns' else torch.cat([a, b], 1)
        elif t == OP_CONCAT_IN:
            n = int(rows[lev])
            parts = []
            for src, slot in ((in0, ia), (in1, ib), (in2, ic)):
                if src < 0:
                    continue
                x = read(src, raw=True)
                if slot < 0 or I[slot] is None:
                    assert x.shape[0] == n
                    parts.append(x)
                else:
                    j = I[slot]
                    assert j.shape[0] == n
                    if x.shape[0] == 0:          # a source without rows: every index is negative
                        assert bool((j < 0).all())
                        parts.append(x.new_zeros(n, x.shape[1]) + 0 * x.sum())
                        continue
                    g = x.index_select(0, j.clamp_min(0))
                    parts.append(torch.where((j >= 0)[:, None], g, torch.zeros_like(g)))
            y = torch.cat(parts, 1)
        elif t == OP_EXPAND:
            y = _walk(read(in0).repeat_interleave(8, 0), rnd(P[par]), geom.child_nbr())
        elif t == OP_LINEAR:
            x = read(in0)
            if mutate == 'head_data_gradient_dropped':
                x = x.detach()
            cols = []
            for q in range(cout):
                yq = x @ P[par + 2 * q].reshape(-1, 1)
                if P[par + 2 * q + 1] is not None:
                    yq = yq + P[par + 2 * q + 1].reshape(1, 1)
                cols.append(yq)
            y = torch.cat(cols, 1)
        else:
            raise ValueError('unknown op %d' % t)
        assert y.shape == (int(rows[bufs[ob][0]]), int(bufs[ob][1])), (i, tuple(y.shape), bufs[ob])
        if t != OP_LINEAR:
            y = rnd(y)
        B[ob] = y
    out['bufs'] = [None if t is None else t.detach() for t in B]
    if gouts is not None:
        loss = None
        for b, g in gouts.items():
            term = (B[b] * prep(g.cpu()).to(dtype)).sum()
            loss = term if loss is None else loss + term
        leaves = [p for p in P if p is not None] + [e for e in E if e is not None]
        if loss is not None and loss.requires_grad:
            grads = list(torch.autograd.grad(loss, leaves, allow_unused=True))
        else:
            grads = [None] * len(leaves)
        grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
        it = iter(grads)
        out['gparams'] = [None if p is None else next(it) for p in P]
        out['gext'] = [None if e is None else next(it) for e in E]
    return out


def max_norm_error(y, ref):
    """max |y - ref| / max |ref| (0 / 0 = 0; NaN in y gives inf)."""
    y, ref = y.double().cpu(), ref.double().cpu()
    if ref.numel() == 0:
        return 0.0
    d = (y - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float('inf')
    e, s = float(d.max()), float(ref.abs().max())
    return 0.0 if e == 0.0 else (e / s if s > 0 else float('inf'))


# ---- the bar of a real-data comparison (rules in test_gpu_prog_fp64.py) ----

# bar = max(BAR_K x e_ref32, floor), both max-normalised.  BAR_K is the smallest power of two that covers the worst
# err_HIP / e_ref32 measured with prog_fusion = 0 (10.8, profiles/prog_fp64_ratios.txt); fused runs meet the same k.
BAR_K = 16


def floor_of(name, ops=None, slots=None):
    """The per-op bar behind a checked tensor: sums (convolution, head and AddTable outputs, every gradient) get
    conv_ref.BAR = bn_ref.SUM_BAR = 2^-18; running statistics and BatchNorm outputs the statistics bars
    bn_ref.MEAN_BAR = bn_ref.VAR_BAR = 2^-20 (they dominate the apply pass's 2^-21)."""
    import bn_ref
    if name.startswith('running'):
        return bn_ref.MEAN_BAR
    if name.startswith('buf') and ops is not None:
        b = int(name[3:])
        if any(int(o[3]) == b and int(o[0]) == OP_BN for o in ops):
            return bn_ref.VAR_BAR
    return conv_ref.BAR


def bar(e_ref32, floor=conv_ref.BAR):
    return max(BAR_K * e_ref32, floor)


# ---- the bar of the bf16 executor (rules in test_gpu_prog_bf16.py) ----

# bar = max(BAR_K_BF16 x e_bf, 2^-8), both max-normalised: e_bf is the distance of the rounding interpreter
# (storage='bf16') from the float64 one, 2^-8 one bf16 ulp of the tensor's largest value.  BAR_K_BF16 is the smallest
# power of two that covers the worst err / e_bf measured with prog_fusion = 0: 1.149 (stage_lin_add, the BatchNorm
# output behind the up-sampling convolution; profiles/prog_bf16_ratios.txt).  The fused and the keep-everything runs
# meet the same k; the worst ratio of any run is 1.301.
BAR_K_BF16 = 2
BF16_ULP = 2.0 ** -8


def bf16_externals(ext):
    """fp32 externals rounded to bf16 by torch: what the fp64 interpreter is fed for an exact case, whose executor run
    must equal it bit for bit although the externals themselves are no bf16 values (prog_cases.BF16_EXT_SCALE)."""
    return [None if e is None else e.bfloat16().float() for e in ext]


def bar_bf16(e_bf):
    return max(BAR_K_BF16 * e_bf, BF16_ULP)
