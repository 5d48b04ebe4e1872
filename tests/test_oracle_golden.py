"""Pins the oracle's GenModel / loss restatement (oracle/model_oracle.py) against fixtures produced by
the REAL reference model.py + loss.py (tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

import model_oracle as mo
from util import param_fill
from sgnn_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ['genmodel_train_32', 'genmodel_train_rect', 'genmodel_train_empty', 'genmodel_scene_eval']


@pytest.fixture(autouse=True)
def fixture_threads():
    """The fixtures were cut with 8 intra-op threads.  The fp32 comparisons hold to 1e-5 when the oracle's reductions are
    split the same way (bit-identical on the fixtures' host); with 1 or 16 threads they move by up to 1.5e-5."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def load(name):
    return np.load(os.path.join(GOLD, name + '.npz'), allow_pickle=False)


def run_oracle(g):
    dims = tuple(int(d) for d in g['dims'])
    scene = bool(g['scene_mode'])
    m = mo.GenModel(8, (32, 32, 32) if scene else dims, 1, 16, 16, 4, True, True, 1, 1)
    param_fill(m, seed=int(g['cfg']))
    m.train(bool(g['train']))
    data = synth.make_batch(int(g['batch']), dims, cfg=int(g['cfg']), occupancy=float(g['occupancy']))
    locs, feats = data['input']
    assert np.array_equal(locs.numpy(), g['in_locs']) and np.array_equal(feats.numpy(), g['in_feats'])
    lw = np.ones(5, dtype=np.float32)
    res = {}
    if scene:
        m.update_sizes(np.array(dims), np.array(dims) // 8)   # test_scene.py:78
        with torch.no_grad():
            osdf, oocc = m([locs, feats], lw)
    else:
        sdf, known, hier = data['sdf'].clone(), data['known'], [h.clone() for h in data['hierarchy']]
        t_sdf, t_occ, t_hier = mo.compute_targets(sdf, hier, 4, 3, True, known)
        osdf, oocc = m([locs, feats], lw)
        loss, losses = mo.compute_loss(osdf, oocc, t_sdf, t_occ, t_hier, lw, 3, True, float(g['weight_missing_geo']),
                                       locs, True, known)
        loss.backward()
        res['loss'], res['losses'] = loss.item(), losses
    return m, osdf, oocc, res


@pytest.mark.parametrize('name', CASES)
def test_oracle_model_matches_reference_golden(name):
    g = load(name)
    m, osdf, oocc, res = run_oracle(g)
    for h in range(4):
        gl, gv = g['occ%d_locs' % h], g['occ%d_vals' % h]
        if gl.size == 0:
            assert len(oocc[h][0]) == 0
            continue
        assert np.array_equal(oocc[h][0].numpy(), gl), 'level %d site list differs' % h
        assert np.abs(oocc[h][1].detach().numpy() - gv).max() < 1e-5
    if g['sdf_locs'].size:
        assert np.array_equal(osdf[0].numpy(), g['sdf_locs'])
        assert np.abs(osdf[1].detach().numpy() - g['sdf_vals']).max() < 1e-5
    else:
        assert len(osdf[0]) == 0
    if 'loss' in g.files:
        assert abs(res['loss'] - float(g['loss'])) < 1e-5 * max(1.0, abs(float(g['loss'])))
        assert np.allclose(np.array(res['losses']), g['losses'], rtol=1e-5, atol=1e-6)
        params = dict(m.named_parameters())
        for n, s, a in zip(g['grad_names'], g['grad_sum'], g['grad_abssum']):
            gr = params[str(n)].grad
            gr = torch.zeros(1) if gr is None else gr
            assert abs(gr.double().abs().sum().item() - a) <= 1e-4 * max(1.0, a), n
        for k in g.files:
            if k.startswith('grad::'):
                gr = params[k[6:]].grad
                assert gr is not None, k
                assert np.abs(gr.numpy() - g[k]).max() <= 1e-5 * max(1.0, np.abs(g[k]).max()), k
            if k.startswith('buf::'):
                assert np.abs(dict(m.named_buffers())[k[5:]].numpy() - g[k]).max() < 1e-6, k


@pytest.mark.parametrize('name', ['genmodel_train_32', 'genmodel_train_rect', 'genmodel_train_empty'])
def test_oracle_fp64_gradients_match_reference_fp64(name):
    """Round 5: the fixtures carry the reference's fp64 loss and parameter gradients (grad64::, stored rounded to fp32) and,
    per tensor, how far the reference's own fp32 run is from them (grad_eref).  The oracle's fp64 evaluation of the same
    step must reproduce the exact values — only the storage rounding (6e-8) separates them."""
    g = load(name)
    dims = tuple(int(d) for d in g['dims'])
    m = mo.GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1)
    param_fill(m, seed=int(g['cfg']))
    m = m.train().double()
    data = synth.make_batch(int(g['batch']), dims, cfg=int(g['cfg']), occupancy=float(g['occupancy']))
    locs, feats = data['input']
    lw = np.ones(5, dtype=np.float32)
    t_sdf, t_occ, t_hier = mo.compute_targets(data['sdf'].clone(), [h.clone() for h in data['hierarchy']], 4, 3, True,
                                              data['known'])
    osdf, oocc = m([locs, feats.double()], lw)
    loss, _ = mo.compute_loss(osdf, oocc, t_sdf.double(), [t.double() for t in t_occ], [t.double() for t in t_hier], lw, 3,
                              True, float(g['weight_missing_geo']), locs, True, data['known'])
    loss.backward()
    assert abs(loss.item() - float(g['loss64'])) <= 1e-10 * max(1.0, abs(float(g['loss64'])))
    names = [str(n) for n in g['grad_names']]
    assert len(g['grad_eref']) == len(names)
    for n, p in m.named_parameters():
        want = g['grad64::' + n].astype(np.float64)
        got = np.zeros_like(want) if p.grad is None else p.grad.numpy()
        scale = max(float(np.abs(want).max()), 1e-300)
        assert np.abs(got - want).max() <= 2e-7 * scale + 1e-30, n
    # the reference's own fp32 run is up to a few per cent from its exact value on some tensors (ReLU / mask flips): that
    # spread, not a flat tolerance, is what the GPU paths are held to (tests/test_gpu_graphstep_parity.py)
    assert float(np.max(g['grad_eref'])) < 0.1


def test_state_dict_keys_follow_reference_layout():
    # nn.Sequential numeric child naming via .add(); 643 735 parameters
    m = mo.GenModel(8, (64, 64, 64), 1, 16, 16, 4, True, True, 1, 1)
    keys = list(m.state_dict().keys())
    assert sum(p.numel() for p in m.parameters()) == 643735
    for k in ['encoder.process_sparse.0.p2.0.1.1.weight', 'refinement.0.p2.2.1.2.0.1.1.weight',
              'refinement.2.n1.weight', 'surfacepred.linear.bias', 'encoder.sdfpred.0.weight']:
        assert k in keys
    g = load('genmodel_train_32')
    assert [str(n) for n in g['grad_names']] == [n for n, _ in m.named_parameters()]
