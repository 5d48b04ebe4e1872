"""CPU: the rules of the differentiable cast as restated in tests/raycast_grad_ref.py: rule
4's terms against central differences of the fp64 forward with k held fixed, the closed form the sixteen sdf terms of
a pixel sum to, and plain gradient descent on an image-space loss.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import raycast_ref as C  # noqa: E402
import raycast_grad_ref as G  # noqa: E402

F32 = np.float32
VS = 0.05
BAND = F32(3.0) * F32(VS)
HW = (24, 32)
# the worst relative disagreement between rule 4 and central differences measured by the test below (per pixel:
# largest |analytic - difference| over the pixel's voxels, over the largest |difference| among them); asserted at 10x
MEASURED_DEPTH = 4.229e-5
MEASURED_BOTH = 8.120e-5
MEASURED_FEATURES = 2.034e-5


@pytest.fixture(scope='module')
def room():
    sdf, w2g = C.room_sdf(VS, 4, BAND)
    _, k, poses = R.room_frames(3, HW, seed=1)
    fe = G.smooth_features(sdf.shape)
    depth, hitk, feat, ok = G.forward(sdf, w2g, VS, k, poses, HW, BAND, fe)
    return dict(sdf=sdf, w2g=w2g, k=k, poses=poses, fe=fe, depth=depth, hit=hitk, feat=feat, ok=ok)


def test_forward_is_the_cast_with_a_record(room):
    exp = C.cast(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, BAND)
    assert np.array_equal(room['depth'].view(np.int32), exp.view(np.int32))
    assert np.array_equal(room['hit'] >= 1, np.isfinite(exp)) and (room['hit'][~np.isfinite(exp)] == -1).all()
    assert np.isfinite(exp).mean() > 0.9 and room['ok'].sum() > 0.9 * np.isfinite(exp).sum()
    assert not room['ok'][~np.isfinite(exp)].any() and (room['feat'][~np.isfinite(exp)] == 0).all()
    # the record reproduces the depth: t* from k alone
    lists = G.terms(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, room['hit'])
    for f, x, t in lists:
        assert np.array_equal(t[5].view(np.int32), room['depth'][f].ravel()[x.pix].view(np.int32))


def disagreement(room, gd, gf, hold_cell, h=1e-6, hf=1e-3):
    """Rule 4's fp32 terms for the incoming gradients gd, gf against central differences of the fp64 forward with k
    held fixed -> (over the hit pixels, the values of: largest |analytic - difference| over the pixel's voxels of sdf,
    over the largest |difference| among them; the same for one direction in feature space, over
    sum |term . direction|).  hold_cell: the features come from the trilinear piece of the cell the fp32 hit lies in,
    wherever the hit moves."""
    sdf, fe, hitk = room['sdf'], room['fe'], room['hit']
    args = (sdf, room['w2g'], VS, room['k'], room['poses'], HW, hitk, fe, gd, gf)
    lists32 = G.terms(*args)
    lists64 = G.terms(*args, dtype=np.float64)
    sdf64, fe64 = sdf.astype(np.float64).reshape(-1), fe.astype(np.float64)
    direction = np.random.default_rng(6).normal(size=fe.shape)
    rel_s, rel_f = [], []
    for (f, _, t32), (_, x, _) in zip(lists32, lists64):
        idx, terms, fidx, fterms, inside, _ = t32
        assert inside.all()
        cells = np.stack(np.unravel_index(fidx[:, 0], sdf.shape)[::-1], 1) if hold_cell else None
        g_d = gd[f].ravel()[x.pix].astype(np.float64)
        g_f = gf[f].reshape(-1, 3)[x.pix].astype(np.float64)

        def loss(c0, c1, features):
            depth, feat = G.forward64(x, c0, c1, features, cells)
            return g_d * depth + (g_f * feat).sum(1)

        c0, c1 = sdf64[x.idx0], sdf64[x.idx1]
        uniq = np.sort(idx, 1)                                              # a voxel both samples share: one variable
        an, fd = np.zeros(uniq.shape), np.zeros(uniq.shape)
        for j in range(16):
            u = uniq[:, j, None]
            up = loss(c0 + h * (x.idx0 == u), c1 + h * (x.idx1 == u), fe64)
            um = loss(c0 - h * (x.idx0 == u), c1 - h * (x.idx1 == u), fe64)
            fd[:, j] = (up - um) / (2 * h)
            an[:, j] = np.where(idx == u, terms.astype(np.float64), 0).sum(1)
        rel_s.append(np.abs(an - fd).max(1) / np.abs(fd).max(1))
        fd_f = (loss(c0, c1, fe64 + hf * direction) - loss(c0, c1, fe64 - hf * direction)) / (2 * hf)   # linear
        each = fterms.astype(np.float64) * direction.reshape(-1, 3)[fidx]
        rel_f.append(np.abs(each.sum((1, 2)) - fd_f) / np.maximum(np.abs(each).sum((1, 2)), 1e-300))
    return np.concatenate(rel_s), np.concatenate(rel_f)


def test_terms_against_central_differences(room):
    """Rule 4 is the derivative of the piece the hit lies in: depth is a rational function of the sixteen voxels, and
    the features are one trilinear polynomial per cell.  The analytic room's walls lie ON cell faces, so nearly every
    hit of this scene sits on a face, where the slope of the feature field along the ray jumps: a central difference
    that lets the hit change cells averages the slopes of both sides (measured below for the record: median
    disagreement 6 %, the half jump, second differences of the field; unbounded where gd and the feature part
    cancel).  The asserted differences therefore hold the hit's cell fixed next to k, at the cell of the fp32 forward,
    and what is left is the difference error of a smooth function and the fp32 rounding of the terms."""
    rng = np.random.default_rng(5)
    gd = rng.normal(size=room['hit'].shape).astype(F32)
    gf = rng.normal(size=room['hit'].shape + (3,)).astype(F32)
    depth_only, _ = disagreement(room, gd, np.zeros_like(gf), True)
    both, features = disagreement(room, gd, gf, True)
    free, _ = disagreement(room, gd, gf, False)
    print('rule 4 against central differences, worst relative disagreement over %d hit pixels: depth only %.3e, with '
          'features %.3e, feature volume %.3e; hit free to change cells: median %.3e, worst %.3e' % (
              len(both), depth_only.max(), both.max(), features.max(), np.median(free), free.max()))
    assert depth_only.max() <= 10 * MEASURED_DEPTH and both.max() <= 10 * MEASURED_BOTH
    assert features.max() <= 10 * MEASURED_FEATURES


def test_sixteen_terms_sum_to_the_closed_form(room):
    gd = np.ones(room['hit'].shape, F32)
    lists = G.terms(room['sdf'], room['w2g'], VS, room['k'], room['poses'], HW, room['hit'], grad_depth=gd)
    flat = room['sdf'].reshape(-1)
    n = 0
    for f, x, (idx, terms, _, _, _, _) in lists:
        pv, v = G.trilinear(flat[x.idx0], x.a0), G.trilinear(flat[x.idx1], x.a1)
        assert (pv > 0).all() and (v <= 0).all()
        closed = float(x.dt) / (pv.astype(np.float64) - v.astype(np.float64))
        t64 = terms.astype(np.float64)
        assert (np.abs(t64.sum(1) - closed) <= 16 * 2.0 ** -24 * np.abs(t64).sum(1)).all()
        n += len(pv)
    assert n == (room['hit'] >= 1).sum() > 1000


def test_gradient_descent_on_a_depth_loss(room):
    sdf, w2g, k, poses = room['sdf'], room['w2g'], room['k'], room['poses']
    true = room['depth']
    cur = np.where(np.isfinite(sdf), sdf + F32(0.02), sdf).astype(F32)          # the surfaces pushed back by 2 cm
    losses = []
    for _ in range(5):
        depth, hitk, _, ok = G.forward(cur, w2g, VS, k, poses, HW, BAND)
        m = ok & np.isfinite(true)
        err = np.where(m, depth - true, F32(0)).astype(F32)
        losses.append(float((err.astype(np.float64) ** 2).sum()))
        lists = G.terms(cur, w2g, VS, k, poses, HW, hitk, grad_depth=F32(2) * err)
        grad = G.accumulate(lists, cur.shape)[0]
        cur = (cur - F32(0.1) * grad.astype(F32)).astype(F32)
    print('depth loss over plain gradient descent: %s' % ['%.4f' % v for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))
