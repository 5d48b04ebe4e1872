"""CPU: the marching-cubes restatement (and, when built, the reference's own extension) against the stored
reference outputs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import mc_oracle  # noqa: E402
from mc_cases import CASES, make_volume  # noqa: E402

SMALL = ['snap', 'jumps', 'colors', 'dense', 'empty', 'iso1']


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(HERE, 'golden', 'mc_expected.npz'))


@pytest.mark.parametrize('name', SMALL)
def test_restatement_matches_reference(g, name):
    spec = CASES[name]
    tsdf, colors = make_volume(spec)
    v, c, f = mc_oracle.run_marching_cubes(tsdf.numpy(), None if colors is None else colors.numpy(), spec['iso'],
                                           spec['trunc'], spec['thresh'])
    assert np.array_equal(v.view(np.int32), g[name + '_v'].view(np.int32))
    assert np.array_equal(c, g[name + '_c']) and np.array_equal(f, g[name + '_f'])


def test_reference_module_reproduces_the_fixture(g):
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_ref'))
    try:
        import marching_cubes_cpp as ref
    except ImportError:
        pytest.skip('oracle/_ref not built (make -C oracle ref needs /root/reference)')
    for name, spec in CASES.items():
        tsdf, colors = make_volume(spec)
        col = colors if colors is not None else torch.ones(tuple(tsdf.shape) + (3,), dtype=torch.uint8) * 220
        v, c, f = ref.run_marching_cubes(tsdf, col, spec['iso'], spec['trunc'], spec['thresh'])
        assert np.array_equal(v.numpy(), g[name + '_v']) and np.array_equal(f.numpy(), g[name + '_f'])


@pytest.mark.parametrize('seed', range(6))
def test_restatement_matches_live_reference_on_random_volumes(seed):
    """Random small volumes (noisy, partially invalid, random iso / thresholds): the restatement against the
    reference's own extension (its meshes of these very volumes are stored in tests/golden/live_reference.npz by
    tests/golden/make_golden_live.py)."""
    import live_cases
    g = live_cases.load()
    vol, colors, iso, trunc, thresh = live_cases.mc_volume(seed)
    rv, rc, rf = g['mc%d_v' % seed], g['mc%d_c' % seed], g['mc%d_f' % seed]
    v, c_, f = mc_oracle.run_marching_cubes(vol, colors, iso, trunc, thresh)
    assert np.array_equal(v.view(np.int32), rv.view(np.int32))
    assert np.array_equal(c_, rc) and np.array_equal(f, rf)


# ---------------------------------------------------------------------------------------------------------------------
# stage cases (mc_cases.STAGE_CASES): every cube configuration, three rounds of the block scan, non-finite voxels, odd
# extents and parameters; the reference extension's meshes of them are tests/golden/mc_stage_expected.npz
# ---------------------------------------------------------------------------------------------------------------------
from mc_cases import NO_SURFACE, STAGE_CASES, cube_table, interp_branches, make_stage_volume  # noqa: E402

STORED = [name for name, spec in STAGE_CASES.items() if spec['stored']]


@pytest.fixture(scope='module')
def gs():
    return np.load(os.path.join(HERE, 'golden', 'mc_stage_expected.npz'))


@pytest.mark.parametrize('name', STORED)
def test_restatement_matches_reference_on_stage_cases(gs, name):
    """Pins the restatement, and through it every row of the triangle table it parses out of csrc/mc_table.h, to the
    reference's own extension."""
    spec = STAGE_CASES[name]
    tsdf, colors = make_stage_volume(spec)
    v, c, f = mc_oracle.run_marching_cubes(tsdf.numpy(), None if colors is None else colors.numpy(), spec['iso'],
                                           spec['trunc'], spec['thresh'])
    assert len(f) > 100
    assert v.shape == gs[name + '_v'].shape and np.array_equal(v.view(np.int32), gs[name + '_v'].view(np.int32))
    assert np.array_equal(c, gs[name + '_c']) and np.array_equal(f, gs[name + '_f'])


@pytest.mark.parametrize('name', [n for n in STAGE_CASES if STAGE_CASES[n]['kind'] == 'allcfg'])
def test_every_configuration_occurs(name):
    """The coverage the all-configurations volumes are there for, counted on the host: each of the 252 configurations
    that have a surface emits at least once, and 0, 255 and the two the reference's edgeTable == 255 rule silences,
    85 and 170, pass every test up to the table look-up."""
    spec = STAGE_CASES[name]
    ci, _ = cube_table(make_stage_volume(spec)[0].numpy(), spec['iso'], spec['trunc'], spec['thresh'])
    seen = set(np.unique(ci[ci >= 0]).tolist())
    assert seen == set(range(256)), sorted(set(range(256)) - seen)
    rows = {k for k in range(256) if mc_oracle.TRI[k]}
    assert rows == set(range(1, 255)) and len(rows) == 254
    silent = {k for k in rows if sum(1 << e for e in set(mc_oracle.TRI[k])) == 255}
    assert silent == {85, 170} and set(NO_SURFACE) == silent | {0, 255}


def test_reference_module_reproduces_the_stage_fixture(gs):
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_ref'))
    try:
        import marching_cubes_cpp as ref
    except ImportError:
        pytest.skip('oracle/_ref not built (make -C oracle ref needs /root/reference)')
    for name in STORED:
        spec = STAGE_CASES[name]
        tsdf, colors = make_stage_volume(spec)
        col = colors if colors is not None else torch.ones(tuple(tsdf.shape) + (3,), dtype=torch.uint8) * 220
        v, c, f = ref.run_marching_cubes(tsdf, col, spec['iso'], spec['trunc'], spec['thresh'])
        assert np.array_equal(v.numpy().view(np.int32), gs[name + '_v'].view(np.int32)), name
        assert np.array_equal(c.numpy(), gs[name + '_c']) and np.array_equal(f.numpy(), gs[name + '_f']), name


def test_stage_volumes_have_their_properties():
    """Conditions on the inputs, all counted on the host."""
    tables = {}
    for name, spec in STAGE_CASES.items():
        vol = make_stage_volume(spec)[0].numpy()
        tables[name] = (vol,) + cube_table(vol, spec['iso'], spec['trunc'], spec['thresh'])
    ntri = np.array([0 if k in NO_SURFACE else len(row) // 3 for k, row in enumerate(mc_oracle.TRI)])
    # carry: more than 2048 blocks of 256 voxels, a tail, and triangles in each of the three rounds of the block scan
    vol, ci, _ = tables['carry']
    per_block = np.add.reduceat(np.where(ci >= 0, ntri[np.maximum(ci, 0)], 0).reshape(-1), np.arange(0, vol.size, 256))
    assert len(per_block) > 2048 and vol.size % 256 != 0
    assert all(per_block[lo:lo + 1024].sum() > 100 for lo in (0, 1024, 2048))
    # allcfg_iso: both end-point snaps and the division occur.  The third snap of vertexInterp, |d1 - d2| < 1e-5, cannot
    # be reached on a crossed edge: with d1 < iso <= d2 the exact iso - d1 is at most d2 - d1, float subtraction rounds
    # monotonically, so |iso - d1| < 1e-5 fires first (and |iso - d2| the other way round).  It stays at zero everywhere.
    snap1, snap2, snap3, divide = interp_branches(*tables['allcfg_iso'][1:], STAGE_CASES['allcfg_iso']['iso'])
    assert min(snap1, snap2, divide) > 1000 and snap3 == 0
    assert all(interp_branches(ci, dist, STAGE_CASES[name]['iso'])[2] == 0 for name, (_, ci, dist) in tables.items())
    # params: part of the cubes fall to the jump threshold, part emit
    vol, ci, _ = tables['params']
    _, loose, _ = (vol,) + cube_table(vol, STAGE_CASES['params']['iso'], STAGE_CASES['params']['trunc'], 1e9)
    rejected = int(((loose >= 0) & (ci < 0)).sum())
    assert rejected > 30 and int((ci >= 0).sum() - np.isin(ci, NO_SURFACE).sum()) > 30, rejected
    # nonfinite: every kind of special voxel is there, and cubes survive beside them
    vol, ci, _ = tables['nonfinite']
    trunc = np.float32(STAGE_CASES['nonfinite']['trunc'])
    assert np.isnan(vol).sum() == 4 and (vol == np.inf).sum() == 4 and (vol == -np.inf).sum() == 4
    assert (np.abs(vol) == trunc).sum() == 8 and (np.abs(vol) == np.nextafter(trunc, np.float32(0))).sum() == 8
    assert (ci >= 0).sum() > 100
