"""GPU: the chunk cutter (sgnn_amd.chunks, csrc/chunks.hip) and fusion.TSDFPyramid against the route that already
exists: the NumPy restatement of tests/chunks_ref.py writes .sdfs files, and the reference-pinned loaders
(DeviceBatchLoader chunk mode, SceneDataset + collate) read them.  Nothing is compared against the cutter's own
output, and nothing has a tolerance: every value is a copy or one or two correctly rounded fp32 divisions."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chunks_ref as C  # noqa: E402

from sgnn_amd import _lib, chunks, data, fusion, train  # noqa: E402
from sgnn_amd.model import GenModel  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

# z, y, x: on and off the stride grid; (0, 0, 0) has no input site, four overhang the volume (in z, and in x);
# (8, 16, 40) starts coarse windows at x = 10 (1/4) and x = 5 (1/8): rows that are not 16-byte aligned
ORIGINS = np.array([(0, 0, 0), (0, 8, 16), (0, 16, 32), (0, 24, 0), (16, 0, 16), (8, 16, 40), (16, 16, 16), (16, 24, 32)])


@pytest.fixture(scope='module')
def scene():
    dims, vs, w2g, depth, k, poses = C.room_scene()
    ref_in, ref_tgt = C.room_pair()
    n = C.N_INPUT
    pyr = fusion.TSDFPyramid(dims, vs, w2g).integrate(depth[:n], k[:n], poses[:n])
    vol_in = pyr[0].copy()
    pyr.integrate(depth[n:], k[n:], poses[n:])
    return dict(dims=dims, vs=vs, w2g=w2g, depth=depth, k=k, poses=poses, ref_in=ref_in, ref_tgt=ref_tgt, pyr=pyr,
                vol_in=vol_in)


def ref_files(s, out_dir, origins, prefix='room', trunc_factor=6.0):
    os.makedirs(str(out_dir), exist_ok=True)
    return C.write_all(out_dir, prefix, origins, s['ref_in'].sdf, [g.sdf for g in s['ref_tgt']],
                       s['ref_tgt'][0].known(), s['vs'], s['w2g'], crop=C.CROP, trunc_factor=trunc_factor)


def same_batch(got, exp, device=True):
    """Key by key, bit for bit.  exp: a DeviceBatchLoader batch (device) or a collate() batch (host)."""
    def eq(a, e):
        assert a.dtype == e.dtype and tuple(a.shape) == tuple(e.shape), (a.dtype, e.dtype, a.shape, e.shape)
        a, e = a.cpu(), e.cpu()
        if a.dtype == torch.float32:
            a, e = a.view(torch.int32), e.view(torch.int32)
        assert torch.equal(a, e)

    assert got['name'] == exp['name']
    eq(got['input'][0], exp['input'][0])
    eq(got['input'][1], exp['input'][1])
    eq(got['sdf'], exp['sdf'])
    eq(got['known'], exp['known'])
    assert len(got['hierarchy']) == len(exp['hierarchy']) == 3
    for k, (a, e) in enumerate(zip(got['hierarchy'], exp['hierarchy'])):
        assert tuple(a.shape[2:]) == tuple(c // (8 >> k) for c in C.CROP)       # [1/8, 1/4, 1/2]
        eq(a, e)
    eq(got['world2grid'], exp['world2grid'])
    eq(got['orig_dims'], exp['orig_dims'])
    if device:
        for t in (got['input'][0], got['input'][1], got['sdf'], got['known'], got['world2grid']) + tuple(got['hierarchy']):
            assert t.is_cuda


def loader_batch(files, nb):
    return next(iter(data.DeviceBatchLoader(files, nb, 3.0, 4)))


def test_pyramid_equals_separate_volumes_and_copy_is_a_snapshot(scene):
    s = scene
    n = C.N_INPUT
    pyr = fusion.TSDFPyramid(s['dims'], s['vs'], s['w2g']).integrate(s['depth'][:n], s['k'][:n], s['poses'][:n])
    snap = pyr.copy()
    before = [v.sdf().clone() for v in snap.volumes]
    pyr.integrate(s['depth'][n:], s['k'][n:], s['poses'][n:])
    assert len(pyr) == 4
    for k in range(4):
        f = 2 ** k
        dims_k = tuple(-(-d // f) for d in s['dims'])
        w2g_k = (fusion.level_transform(k) @ np.asarray(s['w2g'], F32).astype(np.float64)).astype(F32)
        assert np.array_equal(w2g_k, C.level_matrix(s['w2g'], k))
        one = fusion.TSDFVolume(dims_k, F32(f) * F32(s['vs']), w2g_k).integrate(s['depth'], s['k'], s['poses'])
        lvl = pyr[k]
        assert lvl.dims_xyz == dims_k and lvl.voxel_size == one.voxel_size and np.array_equal(lvl.world2grid, w2g_k)
        assert torch.equal(lvl.sdf().view(torch.int32), one.sdf().view(torch.int32))
        assert torch.equal(lvl.weight(), one.weight()) and torch.equal(lvl.free_count(), one.free_count())
        # and the fp32 restatement, level by level (what the files of the other tests are cut from)
        assert np.array_equal(lvl.sdf().cpu().numpy().view(np.int32), s['ref_tgt'][k].sdf.view(np.int32))
        assert torch.equal(snap[k].sdf(), before[k]) and not torch.equal(lvl.sdf(), before[k])
        assert torch.equal(scene['pyr'][k].sdf().view(torch.int32), lvl.sdf().view(torch.int32))
    assert np.array_equal(scene['vol_in'].sdf().cpu().numpy().view(np.int32), s['ref_in'].sdf.view(np.int32))
    # an obb travels through the levels: corner through S_k, edges / f
    obb = np.array([2.0, -4.0, -1.0, 32.0, 8.0, 0.0, -10.0, 45.0, 0.0, 0.0, 0.0, 31.0], F32)
    p = fusion.TSDFPyramid(s['dims'], s['vs'], s['w2g'], levels=3, obb=obb)
    o2 = p[2].obb.reshape(4, 3)
    assert np.array_equal(o2[0], ((obb[:3].astype(np.float64) - 1.5) / 4).astype(F32))
    assert np.array_equal(o2[1:], (obb[3:].reshape(3, 3).astype(np.float64) / 4).astype(F32))


@pytest.mark.parametrize('thresholds', [(1000, 1), (50, 50)])
def test_candidates_equal_the_restatement(scene, thresholds):
    s = scene
    table = C.window_table(s['ref_tgt'][0].sdf, s['ref_in'].sdf, s['vs'], C.CROP, C.STRIDE)
    eo, et, ei = C.candidates(table, *thresholds)
    assert len(eo) >= 8 and len(eo) < len(table[0])                   # by the restatement: a non-degenerate fixture
    cutter = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE)
    cand = cutter.candidates(min_target=thresholds[0], min_input=thresholds[1])
    assert cand.origins.dtype == np.int64 and cand.origins.shape == (len(eo), 3)
    assert np.array_equal(cand.origins, eo) and np.array_equal(cand.n_target, et) and np.array_equal(cand.n_input, ei)
    origins, counts = cutter.scores()
    assert np.array_equal(origins, table[0]) and np.array_equal(counts, table[1])


def test_scores_with_other_filters_and_strides(scene):
    s = scene
    for crop, stride, trunc, factor in (((32, 32, 64), (8, 24, 8), 1.5, 1.0), ((64, 32, 32), (32, 16, 40), 3.0, 6.0)):
        table = C.window_table(s['ref_tgt'][0].sdf, s['ref_in'].sdf, s['vs'], crop, stride, trunc, factor)
        origins, counts = chunks.ChunkCutter(s['vol_in'], s['pyr'], crop, stride, trunc, factor).scores()
        assert np.array_equal(origins, table[0]) and np.array_equal(counts, table[1])
        assert counts[:, 1].sum() > 0


@pytest.mark.parametrize('trunc_factor', [6.0, 4.0])
def test_batch_equals_the_loaders_on_the_restatements_files(scene, tmp_path, trunc_factor):
    s = scene
    files = ref_files(s, tmp_path / 'ref', ORIGINS, trunc_factor=trunc_factor)
    cutter = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE, trunc_factor=trunc_factor)
    got = cutter.batch(ORIGINS, prefix='room')
    exp = loader_batch(files, len(ORIGINS))
    same_batch(got, exp)
    ds = data.SceneDataset(files, None, 3.0, 4, 0)
    same_batch(got, data.collate([ds[i] for i in range(len(files))]), device=False)
    # the fixture exercises what it claims to
    b = got['input'][0][:, 3].cpu().numpy()
    per_crop = np.bincount(b, minlength=len(ORIGINS))
    assert per_crop[0] == 0 and (per_crop[1:] > 0).sum() >= 5 and len(b) > 3000
    dz, dy, dx = s['pyr'][0].dims_zyx
    assert (ORIGINS[:, 0] + C.CROP[0] > dz).any() and (ORIGINS[:, 2] + C.CROP[2] > dx).any()
    assert (got['known'] == 255).any() and (got['known'] == 0).any() and (got['known'] > 2).any()
    assert all(torch.isfinite(h).any().item() for h in got['hierarchy'])


def test_save_writes_the_restatements_files(scene, tmp_path):
    s = scene
    ref = ref_files(s, tmp_path / 'ref', ORIGINS)
    cutter = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE)
    os.makedirs(str(tmp_path / 'out'))
    paths = cutter.save(ORIGINS, tmp_path / 'out', 'room')
    assert [os.path.basename(p) for p in paths] == [os.path.basename(p) for p in ref]
    for p, r in zip(paths, ref):
        assert open(p, 'rb').read() == open(r, 'rb').read()
    same_batch(cutter.batch(ORIGINS, prefix='room'), loader_batch(paths, len(ORIGINS)))


def test_batch_does_not_depend_on_the_grouping(scene):
    s = scene
    cutter = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE)
    whole = cutter.batch(ORIGINS)
    a, b = cutter.batch(ORIGINS[:4]), cutter.batch(ORIGINS[4:])
    locs_b = b['input'][0].clone()
    locs_b[:, 3] += 4
    assert torch.equal(whole['input'][0], torch.cat([a['input'][0], locs_b]))
    assert torch.equal(whole['input'][1].view(torch.int32), torch.cat([a['input'][1], b['input'][1]]).view(torch.int32))
    for key in ('sdf', 'known', 'world2grid', 'orig_dims'):
        assert torch.equal(whole[key], torch.cat([a[key], b[key]])), key
    for k in range(3):
        assert torch.equal(whole['hierarchy'][k], torch.cat([a['hierarchy'][k], b['hierarchy'][k]]))
    assert whole['name'] == a['name'] + b['name']


def test_frames_to_training_steps(scene, tmp_path):
    """frames -> pyramid pair -> candidates -> batch -> train_step and GraphStep; the loss of train_step equals, to
    the bit, the loss of the same step on the batch loaded from the restatement's files."""
    s = scene
    cutter = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE)
    cand = cutter.candidates(min_target=1000, min_input=500)
    assert len(cand.origins) >= 4
    origins = cand.origins[:4]
    batch = cutter.batch(origins, prefix='room')
    from_files = loader_batch(ref_files(s, tmp_path / 'ref', origins), len(origins))
    same_batch(batch, from_files)
    lw = np.ones(5, dtype=np.float32)

    def one_step(b):
        torch.manual_seed(0)
        model = GenModel(8, C.CROP, 1, 16, 16, 4, True, True, 1, 1).cuda().train()
        opt = train.make_optimizer(model.parameters(), lr=1e-3)
        loss, _, _ = train.train_step(model, opt, b, lw)
        return loss.detach().cpu().numpy()

    l_cut, l_file = one_step(batch), one_step(from_files)
    assert np.isfinite(l_cut) and l_cut.view(np.int32) == l_file.view(np.int32)
    torch.manual_seed(0)
    gs = train.GraphStep(GenModel(8, C.CROP, 1, 16, 16, 4, True, True, 1, 1).cuda().train(), lr=1e-3, settle=False)
    vals = [float(gs(batch, lw)) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in vals)


def test_bad_arguments_raise(scene):
    s = scene
    good = chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, C.STRIDE)
    other = fusion.TSDFVolume((64, 56, 48), s['vs'], s['w2g'])
    with pytest.raises(ValueError, match='voxels'):
        chunks.ChunkCutter(other, s['pyr'], C.CROP, C.STRIDE)
    with pytest.raises(ValueError, match='voxel size'):
        chunks.ChunkCutter(fusion.TSDFVolume(s['dims'], 0.05, s['w2g']), s['pyr'], C.CROP, C.STRIDE)
    with pytest.raises(ValueError, match='world2grid'):
        chunks.ChunkCutter(fusion.TSDFVolume(s['dims'], s['vs'], np.eye(4)), s['pyr'], C.CROP, C.STRIDE)
    with pytest.raises(ValueError, match='levels'):
        chunks.ChunkCutter(s['vol_in'], fusion.TSDFPyramid(s['dims'], s['vs'], s['w2g'], levels=3), C.CROP, C.STRIDE)
    with pytest.raises(ValueError, match='multiple of 32'):
        chunks.ChunkCutter(s['vol_in'], s['pyr'], (32, 48, 32), C.STRIDE)
    with pytest.raises(ValueError, match='multiple of 8'):
        chunks.ChunkCutter(s['vol_in'], s['pyr'], C.CROP, (16, 12, 16))
    with pytest.raises(ValueError, match='multiple of 8'):
        good.batch(np.array([(0, 4, 0)]))
    with pytest.raises(ValueError, match='multiple of 8'):
        good.batch(np.array([(0, -8, 0)]))
    with pytest.raises(ValueError, match='no origins'):
        good.batch(np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match='shape'):
        good.batch(np.array([0, 8, 16]))
    # the C ABI refuses what the wrapper would never send
    t = torch.zeros(64, dtype=torch.float32, device='cuda')
    o = torch.zeros(3, dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.SgnnError, match='sgnn_chunk_crop'):
        _lib.call('sgnn_chunk_crop', t.data_ptr(), 4, 4, 4, o.data_ptr(), 1, 4, 4, 6, 0, 1.0, 1.0, t.data_ptr(), None)
    with pytest.raises(_lib.SgnnError, match='sgnn_chunk_score'):
        _lib.call('sgnn_chunk_score', t.data_ptr(), t.data_ptr(), 4, 4, 4, 1.0, 3.0, 6.0, 32, 32, 32, 8, 12, 8, 1, 1, 1,
                  o.data_ptr(), o.data_ptr())
