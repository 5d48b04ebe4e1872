"""The host half of a Gauss-Newton alignment, shared by track (projective point-to-plane ICP) and register (point to
SDF): the layout of the 32-double system that csrc/gn_system.h builds, the launch of a sgnn_*_system entry point, the
6x6 solve, the exponential of a twist and the step T <- Exp(xi) . T over B transforms (INTEGRATION.md section I rules
6 and 8, section R rule 7).  upright shares the record rows.  Private: track re-exports the public names.
"""
import math

import numpy as np
import torch

from . import _lib

# entries of one system (section I rule 6)
A_SLICE, G_SLICE, E_INDEX, N_INDEX = slice(0, 21), slice(21, 27), 27, 28
_TRIU = np.triu_indices(6)


def record_rows(rows64, ok=None):
    """fp64 rows (B, n) -> the fp32 rows of a record table.  A record that is not `ok` (B,), or has an entry that is
    not finite after rounding (which one that is not finite in fp64 never is), is NaN all over: the device leaves it
    empty."""
    with np.errstate(all='ignore'):
        rows = rows64.astype(np.float32)
    finite = np.isfinite(rows).all(axis=1)
    rows[~(finite if ok is None else finite & ok)] = np.nan
    return rows


def check_per_item(shape, residual, item, item_name):
    """The optional per-item outputs of a system call: None or contiguous device tensors of `shape`, fp32 and int32."""
    for name, t, dtype in (('residual', residual, torch.float32), (item_name, item, torch.int32)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and
                                  tuple(t.shape) == shape):
            raise ValueError('%s must be a contiguous device %s tensor of shape %s' % (name, dtype, shape))


def launch(entry, head, table, gates, items, max_blocks, per_item, dev):
    """One sgnn_*_system call -> (B, 32) fp64 on the device, zeros without a launch when there is no record or no item.
    entry(*head, table, B, *gates, out, *per_item, workspace, its bytes): head = the entry point's own leading
    arguments, table = the host record table, items = what the blocks stride over, per_item = the two optional output
    tensors."""
    nb = int(table.shape[0])
    out = torch.zeros((nb, 32), dtype=torch.float64, device=dev)
    if nb == 0 or items == 0:
        return out
    nblk = min((items + 255) // 256, max_blocks)
    ws = torch.empty(nb * nblk * 32, dtype=torch.float64, device=dev)
    dev_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    _lib.call(entry, *head, dev_table.data_ptr(), nb, *map(float, gates), out.data_ptr(), *map(_lib.ptr, per_item),
              ws.data_ptr(), ws.numel() * 8)
    return out


def unpack(system):
    """One 32-entry system (host) -> (A (6, 6) symmetric, g (6,), E, N)."""
    s = np.asarray(system, np.float64).reshape(32)
    a = np.zeros((6, 6))
    a[_TRIU] = s[A_SLICE]
    a = a + np.triu(a, 1).T
    return a, s[G_SLICE].copy(), float(s[E_INDEX]), int(s[N_INDEX])


# ---------------------------------------------------------------------------------------------------------
# the host half (section I rule 8), fp64
# ---------------------------------------------------------------------------------------------------------
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """Closed-form exponential of the twist xi = (omega, t) -> (4, 4) fp64; the series below |omega| = 1e-8."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, t = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    k = _hat(w)
    k2 = k @ k
    if th < 1e-8:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        half = math.sin(0.5 * th)                                        # 1 - cos th = 2 sin^2(th / 2): no cancellation
        a, b, c = math.sin(th) / th, 2.0 * half * half / (th * th), (th - math.sin(th)) / (th * th * th)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + a * k + b * k2
    out[:3, 3] = (np.eye(3) + b * k + c * k2) @ t
    return out


def solve_step(system, min_pairs=64):
    """One 32-entry system (host) -> (xi or None, N, E): A xi = -g by Cholesky; None when N < min_pairs or A is not
    positive definite."""
    a, g, e, n = unpack(system)
    if n < min_pairs or not (np.isfinite(a).all() and np.isfinite(g).all()):
        return None, n, e
    try:
        low = np.linalg.cholesky(a)
    except np.linalg.LinAlgError:
        return None, n, e
    return np.linalg.solve(low.T, np.linalg.solve(low, -g)), n, e


class Steps(object):
    """B transforms advancing together from their guesses (B, 4, 4) fp64: T, and as lists of B: alive, the pairs and
    rmse of a record's last step and the pairs of every step it took (history)."""

    def __init__(self, guess, min_pairs):
        self.guess, self.min_pairs = guess, min_pairs
        self.T = guess.copy()
        nb = guess.shape[0]
        self.alive, self.pairs, self.rmse = [True] * nb, [0] * nb, [float('nan')] * nb
        self.history = [[] for _ in range(nb)]

    def step(self, systems, geometric=None):
        """systems (B, 32), read back: T <- Exp(xi) . T for every live record.  One that solve_step turns down is dead
        from here on, with its guess for T and a NaN rmse.  geometric: None, or the (B, 32) systems that rmse is taken
        from when `systems` holds more than their terms (section T rule T6: entry 28 of both is the same N)."""
        for b in range(len(self.alive)):
            if not self.alive[b]:
                continue
            xi, n, e = solve_step(systems[b], self.min_pairs)
            self.history[b].append(n)
            self.pairs[b] = n
            if xi is None:
                self.alive[b], self.rmse[b] = False, float('nan')
                self.T[b] = self.guess[b]
            else:
                self.rmse[b] = math.sqrt((e if geometric is None else float(geometric[b][E_INDEX])) / n)
                self.T[b] = se3_exp(xi) @ self.T[b]


class Timer(object):
    """Seconds per stage into a dict, or nothing at all."""

    def __init__(self, sink):
        self.sink = sink
        if sink is not None:
            import time
            self.clock = time.perf_counter
            torch.cuda.synchronize()
            self.last = self.clock()

    def __call__(self, stage):
        if self.sink is None:
            return
        torch.cuda.synchronize()
        now = self.clock()
        self.sink[stage] = self.sink.get(stage, 0.0) + (now - self.last)
        self.last = now
