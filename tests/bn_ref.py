"""fp64 restatements of BatchNorm(+leaky ReLU) and the per-site linear heads (bn.hip, linear.hip) and the comparators
that hold the kernels to them.  Works on CPU and on device tensors.

Like conv_ref, every reference returns values together with a magnitude (the sum of |terms| behind each value), the scale
of any rounding error a summation of those terms can make.

Rules restated (include/sgnn_hip.h, the reference's scn.BatchNormalization):
  * training: mean = sum x / n, biased var = sum (x - mean)^2 / n (two passes), invstd = 1 / sqrt(var + eps); running
    stats: r <- momentum * r + (1 - momentum) * new, momentum = the weight of the OLD value, the variance unbiased by
    n / (n - 1) (1 when n = 1).  n = 0: saved stats zero, running stats untouched.  eval: the running stats.
  * apply: t = (x - mean) invstd gamma + beta, y = t if t > 0 else t * leak.
  * backward: dz = dy where t > 0 else dy * leak; dbeta = sum dz, dgamma = sum dz xhat;
    training dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)), eval dx = gamma invstd dz; + addend.
  * heads: y = W x + b, dx = dy^T W (+ addend), dW = sum dy x^T, db = sum dy.

Bars (each derived where it is used):
  * integer data, every fp32 partial sum below 2^24 (asserted): sums are exact in any order, so dbeta and every head
    output / dx / dW / db must match fp64 bit for bit, and save_mean = (float)(s / n) the fp32 rounding of the fp64 mean
    (assert_rounded).  save_invstd may be 1 fp32 ulp off (ulp_mismatch): -ffp-contract
    may fuse s2 / n - mean * mean into one fma, which moves the fp64 variance by an fp64 rounding, and that can flip the
    final rounding to fp32.  The running stats are an fp32 expression (momentum * old + (1 - momentum) * new: two products
    and a sum, fused or not), so they get 2^-22 (|momentum old| + |(1 - momentum) new|) (RUN_BAR).
  * real data: VAR_BAR, MEAN_BAR, APPLY_BAR, SUM_BAR below.
"""
import torch

from conv_ref import EXACT_LIMIT, close_mismatch, exact_mismatch  # noqa: F401  (re-exported for the tests)

# var within 2^-20 (var + mean^2).  The statistics pass rounds x^2 to fp32 (one fma) and adds BN_FLUSH = 2 rows in fp32
# before each fp64 flush: each term of sum x^2 carries at most 2 * 2^-24 of x^2, so s2 / n is within 2^-23 E[x^2]; sum x
# likewise within 2^-23 E|x|, which moves mean^2 by at most 2^-22 |mean| E|x|.  Both are relative to E[x^2] = var +
# mean^2, not to var: E[x^2] - E[x]^2 cancels when the mean is large next to the spread.  2^-20 leaves a factor 4.
VAR_BAR = 2.0 ** -20
# mean within 2^-20 E|x| (the sum x above, 2^-23 E|x|, and one fp32 rounding of the result, 2^-24 |mean|)
MEAN_BAR = 2.0 ** -20
# apply pass, in fp64 from the kernel's own saved fp32 mean / invstd: within 2^-21 (|xhat gamma| + |beta|).  The kernel
# rounds x - mean and (x - mean) invstd (2^-23 |xhat| together), the fma xhat gamma + beta once and t * leak once
# (2^-24 each, leak <= 1): 1.5 * 2^-23 + 2^-24 < 2^-21.  The same bar decides the ReLU boundary: where |t_ref| is inside
# it, either branch is accepted.
APPLY_BAR = 2.0 ** -21
# sums (dgamma, dbeta, dx, dW, db): within 2^-18 sum |terms|, the bar of conv_ref.BAR (an fp32 summation in any order and
# any split into fp32 / fp64 partials stays far inside it; bf16, tf32 or a sequential fp32 sum over 10^6 rows does not)
SUM_BAR = 2.0 ** -18
# running statistics: two fp32 products and an fp32 sum (fma or not), each rounding 2^-24 of a term
RUN_BAR = 2.0 ** -22


# ---- data ----

def int_data(shape, gen, device, lim=3):
    """fp32 tensor of integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=gen, device=device).float()


def offset_data(shape, gen, device, mu, sigma=1.0):
    """x = mu + sigma N(0, 1): a mean large next to the spread for mu / sigma >> 1."""
    return mu + sigma * torch.randn(tuple(shape), generator=gen, device=device)


def assert_int_bound(mag, what=''):
    """Every fp32 partial sum of these terms is bounded by their sum of |terms|: below 2^24, integer sums are exact."""
    if mag.numel():
        m = float(mag.max())
        assert m < EXACT_LIMIT, '%s: integer data too large for exact fp32 sums: sum |terms| %g >= 2^24' % (what, m)


# ---- BatchNorm ----

def bn_stats(x, eps, momentum=0.9, running_mean=None, running_var=None, training=True):
    """Forward statistics of x (n, c).  Returns a dict of fp64 (c,) tensors: mean, var, invstd, the magnitudes
    mean_mag = E|x| and var_mag = var + mean^2, and rm / rv (new running stats, None when not given) with their
    magnitudes rm_mag / rv_mag.  eval: mean / var are the running stats."""
    x = x.double()
    n, c = x.shape
    dev = x.device
    out = {}
    rm = None if running_mean is None else running_mean.double()
    rv = None if running_var is None else running_var.double()
    if not training:
        mean, var = rm, rv
        out.update(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), mean_mag=mean.abs(), var_mag=var.abs(),
                   rm=rm, rv=rv, rm_mag=rm.abs(), rv_mag=rv.abs())
        return out
    if n == 0:
        z = torch.zeros(c, dtype=torch.float64, device=dev)
        out.update(mean=z, var=z, invstd=z, mean_mag=z, var_mag=z, rm=rm, rv=rv,
                   rm_mag=None if rm is None else rm.abs(), rv_mag=None if rv is None else rv.abs())
        return out
    mean = x.sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    out.update(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), mean_mag=x.abs().sum(0) / n,
               var_mag=var + mean * mean)
    m = float(torch.tensor(momentum, dtype=torch.float32))    # the kernel's fp32 momentum; 1 - m is exact in fp32
    unb = var * (n / (n - 1) if n > 1 else 1.0)
    out['rm'] = None if rm is None else m * rm + (1 - m) * mean
    out['rm_mag'] = None if rm is None else (m * rm).abs() + (1 - m) * mean.abs()
    out['rv'] = None if rv is None else m * rv + (1 - m) * unb
    out['rv_mag'] = None if rv is None else (m * rv).abs() + (1 - m) * unb.abs()
    return out


def bn_pre(x, mean, invstd, gamma=None, beta=None):
    """fp64 (xhat, t, mag): xhat = (x - mean) invstd, t = xhat gamma + beta, mag = |xhat gamma| + |beta|.  mean / invstd
    are usually the kernel's own saved fp32 statistics."""
    x = x.double()
    xhat = (x - mean.double()) * invstd.double()
    g = 1.0 if gamma is None else gamma.double()
    b = 0.0 if beta is None else beta.double()
    t = xhat * g + b
    mag = (xhat * g).abs() + (beta.double().abs() if beta is not None else 0.0)
    return xhat, t, mag


def bn_apply(x, mean, invstd, gamma=None, beta=None, leak=0.0):
    """fp64 (y, t, mag) of the apply pass."""
    _, t, mag = bn_pre(x, mean, invstd, gamma, beta)
    return torch.where(t > 0, t, t * leak), t, mag


def bn_backward(x, dy, mean, invstd, gamma=None, beta=None, leak=0.0, training=True, addend=None, mask=None):
    """fp64 backward.  mask: the ReLU mask (t > 0) to use (None: the fp64 one); the tests pass the sign of the
    kernel's own forward output, after checking it against the fp64 mask away from the boundary (bn_mask_mismatch).
    Returns a dict: dz, dbeta / dbeta_mag, dgamma / dgamma_mag, dx / dx_mag (fp64)."""
    x, dy = x.double(), dy.double()
    n = x.shape[0]
    xhat, t, _ = bn_pre(x, mean, invstd, gamma, beta)
    if mask is None:
        mask = t > 0
    dz = torch.where(mask, dy, dy * leak)
    r = {'dz': dz, 'dbeta': dz.sum(0), 'dbeta_mag': dz.abs().sum(0), 'dgamma': (dz * xhat).sum(0),
         'dgamma_mag': (dz * xhat).abs().sum(0)}
    k = (1.0 if gamma is None else gamma.double()) * invstd.double()
    if training and n > 0:
        m1, m2 = r['dbeta'] / n, r['dgamma'] / n
        a1, a2 = r['dbeta_mag'] / n, r['dgamma_mag'] / n
        dx = k * (dz - m1 - xhat * m2)
        mag = k.abs() * (dz.abs() + a1 + xhat.abs() * a2)
    else:
        dx, mag = k * dz, (k * dz).abs()
    if addend is not None:
        dx, mag = dx + addend.double(), mag + addend.double().abs()
    r['dx'], r['dx_mag'] = dx, mag
    return r


# ---- linear heads ----

def linear_fwd(x, w, b=None):
    """y = x W^T + b: fp64 (y, mag), x (n, cin), w (cout, cin), b (cout,) or None."""
    x, w = x.double(), w.double()
    y, mag = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        y, mag = y + b.double(), mag + b.double().abs()
    return y, mag


def linear_bwd(x, dy, w, addend=None):
    """fp64 dict: dx / dx_mag (dy W, + addend), dw / dw_mag (dy^T x), db / db_mag (sum dy)."""
    x, dy, w = x.double(), dy.double(), w.double()
    dx, dx_mag = dy @ w, dy.abs() @ w.abs()
    if addend is not None:
        dx, dx_mag = dx + addend.double(), dx_mag + addend.double().abs()
    return {'dx': dx, 'dx_mag': dx_mag, 'dw': dy.t() @ x, 'dw_mag': dy.abs().t() @ x.abs(), 'db': dy.sum(0),
            'db_mag': dy.abs().sum(0)}


# ---- comparators (None = pass, else a message) ----

def ulp_mismatch(y, ref, ulps=1):
    """y (fp32) within `ulps` fp32 ulps of fp32(ref): the distance of their bit patterns (same sign, finite)."""
    y = y.float()
    r = ref.float()
    a, b = y.view(torch.int32).long(), r.view(torch.int32).long()
    # order the patterns monotonically through zero
    a = torch.where(a < 0, -(a & 0x7fffffff), a)
    b = torch.where(b < 0, -(b & 0x7fffffff), b)
    bad = ~((a - b).abs() <= ulps) | ~torch.isfinite(y)
    if not bad.any():
        return None
    i = int(bad.flatten().nonzero()[0])
    return '%d of %d values more than %d ulp off, first at %d: %r vs fp64 %r' % (
        int(bad.sum()), bad.numel(), ulps, i, float(y.flatten()[i]), float(ref.flatten()[i]))


def stats_mismatch(save_mean, save_invstd, st, eps):
    """Real-data bars of the saved statistics: mean within MEAN_BAR E|x|; invstd as the var bar propagates it —
    d invstd = invstd^3 / 2 d var, so |d invstd| <= invstd^3 / 2 VAR_BAR (var + mean^2), plus 1 fp32 ulp of rounding."""
    msg = close_mismatch(save_mean, st['mean'], st['mean_mag'], MEAN_BAR)
    if msg:
        return 'mean: ' + msg
    inv = st['invstd']
    lim = 0.5 * inv ** 3 * VAR_BAR * st['var_mag'] + 2.0 ** -23 * inv
    msg = close_mismatch(save_invstd, inv, lim, 1.0)
    return None if msg is None else 'invstd: ' + msg


def apply_mismatch(y, ref_t, mag, leak):
    """y of the apply pass against fp64 t (bn_apply, from the kernel's saved stats).  Away from the boundary the branch
    must be the fp64 one; where |t| <= APPLY_BAR mag either branch is accepted."""
    y = y.double()
    lim = APPLY_BAR * mag
    pos, neg = (y - ref_t).abs() <= lim, (y - ref_t * leak).abs() <= lim
    edge = ref_t.abs() <= lim
    ok = torch.where(edge, pos | neg, torch.where(ref_t > 0, pos, neg))
    if bool(ok.all()):
        return None
    i = int((~ok).flatten().nonzero()[0])
    return '%d of %d values off, first at %d: y %r, t %r (leak %g, bar %g)' % (
        int((~ok).sum()), ok.numel(), i, float(y.flatten()[i]), float(ref_t.flatten()[i]), leak, float(lim.flatten()[i]))


def mask_mismatch(mask, ref_t, mag):
    """A ReLU mask (e.g. the sign of the kernel's forward output) against fp64 t: exact wherever |t| > APPLY_BAR mag."""
    edge = ref_t.abs() <= APPLY_BAR * mag
    bad = (mask != (ref_t > 0)) & ~edge
    if not bad.any():
        return None
    i = int(bad.flatten().nonzero()[0])
    return '%d mask entries differ away from the boundary, first at %d (t %r)' % (int(bad.sum()), i,
                                                                               float(ref_t.flatten()[i]))


def _raise(msg, what):
    assert msg is None, '%s: %s' % (what, msg)


def assert_exact(y, ref, mag, what=''):
    _raise(exact_mismatch(y, ref, mag), what)


def assert_rounded(y, ref, mag, what=''):
    """y bit for bit equal to fp32(ref): an exact fp64 value (integer sums) rounded once, as save_mean = (float)(s / n)."""
    _raise(exact_mismatch(y, ref.float().double(), mag), what)


def assert_close(y, ref, mag, what='', bar=SUM_BAR):
    _raise(close_mismatch(y, ref, mag, bar), what)


def assert_ulp(y, ref, what='', ulps=1):
    _raise(ulp_mismatch(y, ref, ulps), what)
