"""fp64 restatements of the fp32 rulebook convolutions (include/sgnn_hip.h) and the comparators that hold a kernel to them.

Every reference is a plain rulebook walk in float64 that returns (value, mag): mag is the sum of |terms| of every output
element, the scale of any rounding error a summation of those terms can make.  Works on CPU and on device tensors.

Two kinds of data:
  * integer data (int_data): every input and weight is an integer of at most 3 (1 on very long sums), so every product
    and every partial sum is an integer below 2^24 and fp32 is exact in any summation order.  The kernel's output must
    equal the fp64 value bit for bit (assert_exact, which also asserts the 2^24 bound on mag).
  * real data: |y - ref| <= BAR * mag per element (assert_close).  BAR = 2^-18: an fp32 summation of these terms (MFMA
    or FMA, any order, any split into partials) stays orders of magnitude inside it, while one bf16 rounding (2^-9),
    tf32 (2^-11) or a 3-pass xf32-style split (~2^-16 .. 2^-17 on a product) does not.
"""
import torch

EXACT_LIMIT = 2 ** 24
BAR = 2.0 ** -18


# ---- data ----

def int_data(shape, gen, device, lim=3):
    """fp32 tensor of integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=gen, device=device).float()


def real_data(shape, gen, device, scale=1.0):
    return torch.randn(tuple(shape), generator=gen, device=device) * scale


# ---- rulebook walks ----

def _rows(table, ld, n_out):
    return table.reshape(-1, ld)[:, :n_out].long()


def walk(x, w, table, K, ld, n_out, kmap=None, kadd=None, in_mul=1, groups=1, in_shift=0):
    """y[row * groups + g] = sum_k x[(e >> in_shift) * in_mul + kadd[g*K + k]] @ w[g, k],  e = table[kmap[g*K + k]][row]
    over the entries e >= 0 (sgnn_conv_fwd_ex; kmap None: row k, kadd None: + 0).  x (n_in, cin), w (groups*K, cin, cout).
    Returns fp64 (y, mag), both (n_out * groups, cout)."""
    t = _rows(table, ld, n_out)
    x = x.double()
    w = w.double().reshape(groups, K, w.shape[-2], w.shape[-1])
    cout = w.shape[-1]
    y = torch.zeros(n_out, groups, cout, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    for g in range(groups):
        for k in range(K):
            e = t[int(kmap[g * K + k]) if kmap is not None else k]
            m = e >= 0
            src = (e[m] >> in_shift) * in_mul + (int(kadd[g * K + k]) if kadd is not None else 0)
            xs = x[src]
            y[m, g] += xs @ w[g, k]
            mag[m, g] += xs.abs() @ w[g, k].abs()
    return y.reshape(n_out * groups, cout), mag.reshape(n_out * groups, cout)


def walk_adjoint(dy, w, table, K, ld, n_out, n_in):
    """Data gradient of walk (plain form) by its definition: dx[table[k][j]] += dy[j] @ w[k]^T.  Scatters over the
    FORWARD table, so no flip, transpose or parent table of the library is involved.  Returns fp64 (dx, mag)."""
    t = _rows(table, ld, n_out)
    dy, w = dy.double(), w.double()
    dx = torch.zeros(n_in, w.shape[1], dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(dx)
    for k in range(K):
        m = t[k] >= 0
        dx.index_add_(0, t[k][m], dy[m] @ w[k].t())
        mag.index_add_(0, t[k][m], dy[m].abs() @ w[k].abs().t())
    return dx, mag


def walk_dw(x, dy, table, K, ld, n_out, in_shift=0):
    """Weight gradient of walk: dw[k] = sum_j x[table[k][j] >> in_shift]^T dy[j].  Returns fp64 (dw, mag), (K, cin, cout)."""
    t = _rows(table, ld, n_out)
    x, dy = x.double(), dy.double()
    dw = torch.zeros(K, x.shape[1], dy.shape[1], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(dw)
    for k in range(K):
        m = t[k] >= 0
        xs = x[t[k][m] >> in_shift]
        dw[k] = xs.t() @ dy[m]
        mag[k] = xs.abs().t() @ dy[m].abs()
    return dw, mag


# ---- rulebooks built from coordinates (for the up-sampling reference) ----

_AX = 19          # bits per spatial axis in a packed key (coordinates + 1 must stay below 2^19)


def _pack(c):
    """(n, 4) [z, y, x, b] -> int64 keys; coordinates may be -1 (a neighbour outside the volume)."""
    c = c.long()
    return (((c[:, 3] << _AX) | (c[:, 0] + 1)) << (2 * _AX)) | ((c[:, 1] + 1) << _AX) | (c[:, 2] + 1)


def subm_rulebook(coords):
    """27-offset submanifold rulebook (27, n) int64 of sites (n, 4) [z, y, x, b]: row of the site at p_j + d_k or -1,
    k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1).  Sort and binary search only."""
    c = coords.long()
    assert c.shape[0] == 0 or (int(c[:, :3].max()) + 2 < (1 << _AX) and int(c[:, 3].max()) < (1 << 6))
    keys = _pack(c)
    sk, order = torch.sort(keys)
    assert sk.numel() < 2 or bool((sk[1:] != sk[:-1]).all()), 'duplicate sites'
    out = torch.full((27, c.shape[0]), -1, dtype=torch.int64, device=c.device)
    k = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = _pack(c + torch.tensor([dz, dy, dx, 0], device=c.device))
                pos = torch.searchsorted(sk, q).clamp_max(max(sk.numel() - 1, 0))
                hit = sk[pos] == q
                out[k][hit] = order[pos[hit]]
                k += 1
    return out


def children_coords(coords):
    """The 8 children of every site at twice the resolution: row 8p + g is 2 c_p + (g>>2 & 1, g>>1 & 1, g & 1)."""
    c = coords.long()
    g = torch.arange(8, device=c.device)
    j = torch.stack([(g >> 2) & 1, (g >> 1) & 1, g & 1, torch.zeros_like(g)], 1)
    two = torch.tensor([2, 2, 2, 1], device=c.device)
    return (c[:, None, :] * two + j[None]).reshape(-1, 4)


def expand_taps():
    """A (64, 27) fp64 0/1: slot g*8 + i of the up-sampling convolution collects the 3x3x3 taps d of child parity g
    whose neighbour 2c + j + d lies in parent c + o, o = floor((j + d) / 2), slot i = o + 1 - j per axis."""
    A = torch.zeros(64, 27, dtype=torch.float64)
    for g in range(8):
        j = ((g >> 2) & 1, (g >> 1) & 1, g & 1)
        for tap in range(27):
            d = (tap // 9 - 1, (tap // 3) % 3 - 1, tap % 3 - 1)
            i = [(j[a] + d[a]) // 2 + 1 - j[a] for a in range(3)]
            assert all(v in (0, 1) for v in i)
            A[g * 8 + i[0] * 4 + i[1] * 2 + i[2], tap] = 1.0
    return A


# ---- comparators ----

def exact_mismatch(y, ref, mag):
    """None if y equals ref bit for bit, else a message.  Asserts that the data respected the exactness bound."""
    assert float(mag.max()) < EXACT_LIMIT if mag.numel() else True, \
        'integer data too large for exact fp32 sums: max sum of |terms| %g >= 2^24' % float(mag.max())
    y = y.double()
    bad = ~(y == ref)
    if not bad.any():
        return None
    i = int(bad.flatten().nonzero()[0])
    return '%d of %d values differ, first at flat index %d: %r != %r' % (
        int(bad.sum()), bad.numel(), i, float(y.flatten()[i]), float(ref.flatten()[i]))


def close_mismatch(y, ref, mag, bar=BAR):
    """None if |y - ref| <= bar * mag everywhere (NaN fails), else a message with the worst offender."""
    y = y.double()
    err = (y - ref).abs()
    lim = bar * mag
    bad = ~(err <= lim)
    if not bad.any():
        return None
    over = torch.where(bad, torch.nan_to_num(err / mag.clamp_min(1e-300), nan=float('inf')), torch.zeros_like(err))
    i = int(over.flatten().argmax())
    return '%d of %d values off, worst at flat index %d: err %g, mag %g (err/mag %g, bar %g)' % (
        int(bad.sum()), bad.numel(), i, float(err.flatten()[i]), float(mag.flatten()[i]), float(over.flatten()[i]), bar)


def assert_exact(y, ref, mag, what=''):
    msg = exact_mismatch(y, ref, mag)
    assert msg is None, '%s: %s' % (what, msg)


def assert_close(y, ref, mag, what='', bar=BAR):
    msg = close_mismatch(y, ref, mag, bar)
    assert msg is None, '%s: %s' % (what, msg)


def worst_ratio(y, ref, mag):
    """max |y - ref| / mag (diagnostics: how far inside the bar a result is)."""
    return float(((y.double() - ref).abs() / mag.clamp_min(1e-300)).max())
