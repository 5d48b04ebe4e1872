"""GPU: device marching cubes + mesh clean-up against the REFERENCE's own compiled extension — stored outputs
(tests/golden/mc_expected.npz, made with oracle/_ref/marching_cubes_cpp.so) and, at scene size, stored sizes + digests
of its meshes (tests/golden/live_reference.npz).  Everything is compared bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from mc_cases import CASES, make_volume  # noqa: E402

from sgnn_amd import marching_cubes as mc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(HERE, 'golden', 'mc_expected.npz'))


def same_mesh(got, want):
    v, c, f = (t.cpu().numpy() for t in got)
    wv, wc, wf = want
    assert v.shape == wv.shape and f.shape == wf.shape, (v.shape, wv.shape, f.shape, wf.shape)
    assert np.array_equal(v.view(np.int32), wv.view(np.int32))          # every float bit
    assert np.array_equal(c, wc) and c.dtype == np.uint8
    assert np.array_equal(f, wf) and f.dtype == np.int32


@pytest.mark.parametrize('name', list(CASES))
def test_matches_reference_output(g, name):
    spec = CASES[name]
    tsdf, colors = make_volume(spec)
    got = mc.run_marching_cubes(tsdf.cuda(), colors, spec['iso'], spec['trunc'], spec['thresh'])
    same_mesh(got, (g[name + '_v'], g[name + '_c'], g[name + '_f']))
    v, c, f = got
    if len(f):
        assert int(f.max()) < len(v) and int(f.min()) >= 0
        assert not ((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])).any()
        key = torch.sort(f.long(), 1).values
        assert len(torch.unique(key, dim=0)) == len(f)


def test_ply_file_is_byte_identical(g, tmp_path):
    tsdf, _ = make_volume(CASES['sphere32'])
    p = str(tmp_path / 'm.ply')
    mc.marching_cubes(tsdf, None, 0.0, 3.0, 10.0, p)           # host tensor in, as data_util.py:270 passes it
    assert np.array_equal(np.fromfile(p, dtype=np.uint8), g['sphere32_ply'])
    q = str(tmp_path / 'm.obj')
    mc.marching_cubes(tsdf, None, 0.0, 3.0, 10.0, q)
    lines = open(q).read().splitlines()
    assert sum(l.startswith('v ') for l in lines) == len(g['sphere32_v'])
    assert sum(l.startswith('f ') for l in lines) == len(g['sphere32_f'])


def test_host_tensor_rejected_by_the_kernel_entry():
    with pytest.raises(RuntimeError, match='GPU only'):
        mc.run_marching_cubes(torch.zeros(4, 4, 4), None, 0.0, 3.0, 10.0)


def test_scene_size_against_live_reference():
    """(96,160,192) surface volume: ~1e5 triangles, long welding chains along shared edges.  The reference extension's
    meshes of these volumes are stored as sizes + sha256 digests (tests/golden/live_reference.npz,
    tests/golden/make_golden_live.py): bit for bit, like every other comparison here."""
    import live_cases
    g = live_cases.load()
    vols, _ = live_cases.mc_scene_volumes()
    for i, tsdf in enumerate(vols):
        v, c, f = (t.cpu().numpy() for t in mc.run_marching_cubes(tsdf.cuda(), None, 0.0, 3.0, 10.0))
        assert [len(v), len(f)] == g['mcscene%d_shapes' % i].tolist(), (i, len(v), len(f))
        assert len(f) > 20000 and c.dtype == np.uint8 and f.dtype == np.int32
        assert live_cases.digest(v, c, f) == str(g['mcscene%d_sha' % i]), 'scene-size mesh %d differs from the reference' % i


def test_save_predictions_files_match_reference(g, tmp_path):
    """test_scene.py:98 -> data_util.save_predictions: the two mesh files, byte for byte."""
    from mc_cases import scene_prediction
    names, inputs, pred = scene_prediction()
    mc.save_predictions(str(tmp_path), names, inputs, None, None, pred, None, None, 3.0)
    for f, key in (('scene0_input-mesh.ply', 'pred_scene0_input_mesh_ply'), ('scene0_pred-mesh.ply', 'pred_scene0_pred_mesh_ply')):
        got = np.fromfile(str(tmp_path / f), dtype=np.uint8)
        assert got.size > 1000 and np.array_equal(got, g[key]), f
    # per-level occupancy point clouds (data_util.py:268-276): one vertex per predicted site, z,y,x -> x,y,z, voxel
    # centres scaled to the finest resolution; a level without predictions writes nothing
    locs = torch.tensor([[1, 2, 3, 0], [4, 5, 6, 0]])
    mc.save_predictions(str(tmp_path), names, inputs, None, None, pred, [None, [locs]], None, 3.0)
    assert not (tmp_path / 'scene0_pred-0.ply').exists()
    txt = (tmp_path / 'scene0_pred-1.ply').read_bytes()
    assert b'element vertex 2' in txt
