"""Host references for the autograd layer (sgnn_amd/scn/functions.py), written from the Functions' docstrings and from
include/sgnn_hip.h.  Nothing here calls the library or imports sgnn_amd.

What already states an operation is reused: the rulebook walks, the coordinate-built rulebooks and the comparators of
conv_ref, the row movement of glue_ref, BatchNorm and the linear heads of bn_ref.  Added here:
  * adjoint_gap: <dy, F(a)> - <F^T dy, a> in int64, the tolerance-free test of a backward against its forward;
  * the generative up-sampling convolution as what it replaces: expand every site into 8 children that carry its
    features, then walk a 3x3x3 submanifold rulebook built from the children's coordinates (expand_*), and its
    parent-rulebook form for an arbitrary 64-slot weight (expand_slot_*);
  * nn.Conv3d(k4, s2, p1) / nn.ConvTranspose3d(k4, s2, p1) on channel-last rows in batch-major raster order as 64
    strided slices of the padded volume (k4s2_*), in fp64, with the magnitudes the comparators need;
  * the row Functions' adjoints as index arithmetic (unpool_adjoint, gather_adjoint ...).

Every reference that sums returns (value, mag) in float64, mag = the sum of |terms| (see conv_ref)."""
import numpy as np
import torch

import conv_ref as R


# ---- the adjoint identity ----

def _as_int64(t, what):
    t = torch.as_tensor(t).detach().cpu()
    assert t.dtype == torch.float32, '%s: adjoint_gap takes fp32 tensors (got %s)' % (what, t.dtype)
    i = t.to(torch.int64)
    assert bool((i.to(torch.float32) == t).all()), '%s holds a value that is no integer (or NaN / infinity)' % what
    return i.reshape(-1)


def adjoint_gap(x, gx, y, gy):
    """sum(gy * y) - sum(gx * x) as a Python int, computed on the host in int64 from integer-valued fp32 tensors.
    For y = F(x) linear in x and gx = F^T gy this is zero exactly, whatever F is; x / gx may be lists (a Function linear
    in several arguments jointly).  |values| of a few thousand and 10^7 elements stay far below 2^63."""
    xs, gxs = (x, gx) if isinstance(x, (list, tuple)) else ([x], [gx])
    assert len(xs) == len(gxs)
    lhs = int((_as_int64(gy, 'gy') * _as_int64(y, 'y')).sum())
    rhs = 0
    for k, (a, ga) in enumerate(zip(xs, gxs)):
        a, ga = _as_int64(a, 'x[%d]' % k), _as_int64(ga, 'gx[%d]' % k)
        assert a.shape == ga.shape, 'x[%d]: %d values, gradient %d' % (k, a.numel(), ga.numel())
        rhs += int((a * ga).sum())
    return lhs - rhs


# ---- generative up-sampling convolution ----

def expand_rulebook(coords):
    """(27, 8n) submanifold rulebook of the 8 children (row 8p + g) of sites (n, 4) [z, y, x, b]."""
    return R.subm_rulebook(R.children_coords(coords))


def expand_fwd(f, w, crules):
    """y (8n, cout): SubmanifoldConvolution(3x3x3, w (27, cin, cout)) on the children, each carrying its parent's row."""
    n8 = crules.shape[1]
    return R.walk(f.repeat_interleave(8, 0), w, crules, 27, n8, n8)


def expand_df(dy, w, crules):
    """Gradient of expand_fwd w.r.t. f: the children's data gradient summed over each parent's 8 children."""
    n8 = crules.shape[1]
    d, m = R.walk_adjoint(dy, w, crules, 27, n8, n8, n8)
    return d.view(n8 // 8, 8, -1).sum(1), m.view(n8 // 8, 8, -1).sum(1)


def expand_dw(f, dy, crules):
    n8 = crules.shape[1]
    return R.walk_dw(f.repeat_interleave(8, 0), dy, crules, 27, n8, n8)


def expand_slots():
    """S (64): slot g*8 + i of child parity g = 4jz + 2jy + jx reads the PARENT level's 3x3x3 neighbour row of offset
    o = i - 1 + j per axis (i = 4iz + 2iy + ix in {0, 1}^3)."""
    S = []
    for g in range(8):
        j = ((g >> 2) & 1, (g >> 1) & 1, g & 1)
        for i_ in range(8):
            i = ((i_ >> 2) & 1, (i_ >> 1) & 1, i_ & 1)
            o = [i[a] - 1 + j[a] for a in range(3)]
            S.append((o[0] + 1) * 9 + (o[1] + 1) * 3 + (o[2] + 1))
    return S


def expand_slot_fwd(f, wc, prules):
    """y[8p + g] = sum_i wc[g*8 + i]^T f[prules[S[g*8 + i]][p]] for any wc (64, cin, cout); prules (27, n) of the parents."""
    n = prules.shape[1]
    return R.walk(f, wc, prules, 8, n, n, kmap=expand_slots(), groups=8)


def expand_slot_dwc(f, dy, prules):
    """dwc[g*8 + i] = sum_p f[prules[S[g*8 + i]][p]]^T dy[8p + g]."""
    n = prules.shape[1]
    f, dy = f.double(), dy.double().view(n, 8, -1)
    dwc = torch.zeros(64, f.shape[1], dy.shape[2], dtype=torch.float64, device=f.device)
    mag = torch.zeros_like(dwc)
    for q, s in enumerate(expand_slots()):
        e = prules[s]
        m = e >= 0
        dwc[q] = f[e[m]].t() @ dy[m, q // 8]
        mag[q] = f[e[m]].abs().t() @ dy[m, q // 8].abs()
    return dwc, mag


# ---- dense k4 / s2 / p1 convolution and its transpose on channel-last raster rows ----

def k4s2_taps():
    """Tap (kz*4 + ky)*4 + kx held by slot q = g*8 + i of the (64, Cin, Cout) weight: the fine voxel 2c + j of parity g
    meets coarse voxel c + o, o = i - 1 + j, through tap k = j + 1 - 2o = 3 - 2i - j per axis."""
    P = []
    for g in range(8):
        j = ((g >> 2) & 1, (g >> 1) & 1, g & 1)
        for i_ in range(8):
            i = ((i_ >> 2) & 1, (i_ >> 1) & 1, i_ & 1)
            k = [3 - 2 * i[a] - j[a] for a in range(3)]
            P.append((k[0] * 4 + k[1]) * 4 + k[2])
    assert sorted(P) == list(range(64))
    return P


def slots_to_taps(w):
    """(64, a, b) in slot order -> tap order."""
    out = torch.empty_like(w)
    out[torch.tensor(k4s2_taps(), device=w.device)] = w
    return out


def taps_to_slots(w):
    return w[torch.tensor(k4s2_taps(), device=w.device)]


def rows_to_vol(rows, batch, dims):
    """(B * d0 * d1 * d2, C) batch-major raster rows -> (B, d0, d1, d2, C) float64."""
    return rows.double().reshape(batch, dims[0], dims[1], dims[2], rows.shape[1])


def vol_to_rows(v):
    return v.reshape(-1, v.shape[-1])


def _tap_slices(cd):
    """Per tap (kz, ky, kx): the slices of the fine volume PADDED by 1 that hold input 2o - 1 + k for every coarse o."""
    for t in range(64):
        kz, ky, kx = t // 16, (t // 4) % 4, t % 4
        yield t, (slice(None), slice(kz, kz + 2 * cd[0], 2), slice(ky, ky + 2 * cd[1], 2), slice(kx, kx + 2 * cd[2], 2))


def _pad1(v):
    out = torch.zeros(v.shape[0], v.shape[1] + 2, v.shape[2] + 2, v.shape[3] + 2, v.shape[4], dtype=v.dtype, device=v.device)
    out[:, 1:-1, 1:-1, 1:-1] = v
    return out


def k4s2_down(x, w):
    """nn.Conv3d(k4, s2, p1): y[b, o] = sum_k x[b, 2o - 1 + k] @ w[k], zeros outside.  x (B, d0, d1, d2, Cin) fp64,
    w (64, Cin, Cout) in TAP order.  Returns fp64 (y, mag), (B, d0/2, d1/2, d2/2, Cout)."""
    w = w.double()
    cd = [d // 2 for d in x.shape[1:4]]
    xp = _pad1(x)
    y = torch.zeros(x.shape[0], cd[0], cd[1], cd[2], w.shape[2], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    for t, sl in _tap_slices(cd):
        y += xp[sl] @ w[t]
        mag += xp[sl].abs() @ w[t].abs()
    return y, mag


def k4s2_up(x, w):
    """nn.ConvTranspose3d(k4, s2, p1): y[b, 2o - 1 + k] += x[b, o] @ w[k].  x (B, c0, c1, c2, Cin) coarse, w (64, Cin,
    Cout) in TAP order.  Returns fp64 (y, mag), (B, 2c0, 2c1, 2c2, Cout)."""
    w = w.double()
    cd = list(x.shape[1:4])
    yp = torch.zeros(x.shape[0], 2 * cd[0] + 2, 2 * cd[1] + 2, 2 * cd[2] + 2, w.shape[2], dtype=torch.float64,
                     device=x.device)
    mp = torch.zeros_like(yp)
    for t, sl in _tap_slices(cd):
        yp[sl] += x @ w[t]
        mp[sl] += x.abs() @ w[t].abs()
    return yp[:, 1:-1, 1:-1, 1:-1], mp[:, 1:-1, 1:-1, 1:-1]


def k4s2_pair(fine, coarse):
    """dw[k] = sum_{b, o} fine[b, 2o - 1 + k]^T coarse[b, o]: (64, Cfine, Ccoarse) in TAP order, fp64 (value, mag).  The
    weight gradient of k4s2_down as it stands (x fine, dy coarse); that of k4s2_up is its transpose per tap."""
    cd = list(coarse.shape[1:4])
    fp = _pad1(fine)
    c2 = coarse.reshape(-1, coarse.shape[-1])
    dw = torch.zeros(64, fine.shape[-1], coarse.shape[-1], dtype=torch.float64, device=fine.device)
    mag = torch.zeros_like(dw)
    for t, sl in _tap_slices(cd):
        f2 = fp[sl].reshape(-1, fine.shape[-1])
        dw[t] = f2.t() @ c2
        mag[t] = f2.abs().t() @ c2.abs()
    return dw, mag


# ---- row Functions: adjoints as index arithmetic (forwards are glue_ref's) ----

def gather_adjoint(d, idx, n):
    """Adjoint of dst[r] = src[idx[r]] (idx unique, negative = zeros): dsrc (n rows), dsrc[idx[r]] = d[r]."""
    d, idx = np.asarray(d), np.asarray(idx, np.int64)
    out = np.zeros((n,) + d.shape[1:], d.dtype)
    out[idx[idx >= 0]] = d[:len(idx)][idx >= 0]
    return out


def unpool(coarse, parent):
    """fine[i] = coarse[parent[i]]."""
    return np.asarray(coarse)[np.asarray(parent, np.int64)]


def unpool_adjoint(d, parent, nc):
    """dcoarse[p] = sum of d[i] over the children i of p (none: zeros).  Integer data: exact in any order."""
    d = np.asarray(d, np.float64)
    out = np.zeros((nc, d.shape[1]), np.float64)
    np.add.at(out, np.asarray(parent, np.int64), d)
    return out.astype(np.float32)


def children_table(parent, slot, nc, ldc):
    """(8, ldc) int32: children[slot[i]][parent[i]] = i, -1 elsewhere."""
    t = np.full((8, ldc), -1, np.int32)
    t[np.asarray(slot), np.asarray(parent)] = np.arange(len(parent), dtype=np.int32)
    return t


def repeat_adjoint(d, rep):
    """dsrc[r] = sum_t d[r * rep + t] (integer data: exact)."""
    d = np.asarray(d, np.float64)
    return d.reshape(-1, rep, d.shape[1]).sum(1).astype(np.float32)
