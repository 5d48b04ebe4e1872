"""GPU: TSDF fusion (sgnn_amd.fusion, csrc/fusion.hip) against the NumPy restatement of tests/fusion_ref.py —
raw depth and integration bit for bit, the bilateral filter against fp64 — and the fused volume through the
existing readers, loaders, model, loss and marching cubes."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402

from sgnn_amd import data, fusion, loss as L, marching_cubes as mc  # noqa: E402
from sgnn_amd.model import GenModel  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def spoil(depth, seed):
    """Invalid pixels and depths outside [0.4, 4.0] m."""
    rng = np.random.default_rng(seed)
    d = depth.copy()
    u = rng.random(d.shape)
    d[u < 0.04] = -np.inf
    d[(u >= 0.04) & (u < 0.06)] = F32(4.6)
    d[(u >= 0.06) & (u < 0.08)] = F32(0.25)
    return d


def scene(case):
    """(dims_xyz, voxel size, world2grid, obb, depth (F,h,w) unfiltered, intrinsics, cam2world)."""
    if case == 'cube48':
        depth, k, poses = R.room_frames(24, (48, 64), seed=1)
        poses[5] = R.look_at((-5.0, 1.0, 1.0), (-9.0, 1.0, 1.0))         # looks away from the grid
        return (48, 48, 48), 0.085, R.grid_transform((0.0, 0.0, 0.0), 0.085), None, spoil(depth, 1), k, poses
    depth, k, poses = R.room_frames(24, (40, 56), seed=2)
    close = R.look_at((0.6, 1.6, 1.2), (-1.0, 1.7, 1.1))                  # 0.6 m from a wall: weight saturates
    cd = R.render(k[0], close, (40, 56), R.ROOM_PLANES, R.ROOM_BOXES)
    n = 66
    depth = np.concatenate([depth[:12], np.repeat(cd[None], n, 0), depth[12:]])
    poses = np.concatenate([poses[:12], np.repeat(close[None], n, 0), poses[12:]])
    k = np.tile(k[0], (len(poses), 1))
    obb = np.array([2.0, -4.0, -1.0, 32.0, 8.0, 0.0, -10.0, 45.0, 0.0, 0.0, 0.0, 31.0], F32)   # rotated about z
    return (37, 53, 29), 0.1, R.grid_transform((-0.2, -0.3, -0.1), 0.1), obb, spoil(depth, 2), k, poses


CASES = ['cube48', 'odd37x53x29']


@pytest.fixture(scope='module')
def fused():
    out = {}
    for case in CASES:
        dims, vs, w2g, obb, depth, k, poses = scene(case)
        filt = fusion.bilateral(torch.from_numpy(depth).cuda())
        ref = R.Grid(dims, vs, w2g, obb=obb).integrate(filt.cpu().numpy(), k, poses)
        vol = fusion.TSDFVolume(dims, vs, w2g, obb=obb).integrate(filt, k, poses, chunk=len(poses))
        out[case] = dict(dims=dims, vs=vs, w2g=w2g, obb=obb, filt=filt, k=k, poses=poses, ref=ref, vol=vol)
    return out


def same_state(vol, ref):
    assert np.array_equal(vol.sdf().cpu().numpy().view(np.int32), ref.sdf.astype(F32).view(np.int32))
    assert np.array_equal(vol.weight().cpu().numpy().astype(np.int64), ref.weight)
    assert np.array_equal(vol.free_count().cpu().numpy().astype(np.int64), ref.free)


def test_raw_depth_bitwise():
    rng = np.random.default_rng(0)
    for (nf, hr, wr), (h, w) in (((3, 97, 131), (61, 83)), ((2, 480, 640), (240, 320))):
        raw = rng.integers(0, 14000, size=(nf, hr, wr)).astype(np.uint16)
        raw[rng.random(raw.shape) < 0.1] = 0
        k_raw = np.array([577.6, 578.7, 318.9, 242.7], F32)
        got, k = fusion.raw_depth_to_metric(raw, 1000.0, (h, w), intrinsics=k_raw)
        exp = R.raw_to_metric(raw, 1000.0, (h, w))
        assert got.is_cuda and got.shape == (nf, h, w)
        assert np.array_equal(got.cpu().numpy().view(np.int32), exp.view(np.int32))
        assert np.array_equal(k, R.adapt_intrinsics(k_raw, (hr, wr), (h, w)))
        assert np.isinf(exp).any() and np.isfinite(exp).any()
    one, _ = fusion.raw_depth_to_metric(raw[0], 1000.0, (h, w), min_depth=0.5, max_depth=3.0)
    assert np.array_equal(one.cpu().numpy(), R.raw_to_metric(raw[0], 1000.0, (h, w), 0.5, 3.0))


def test_bilateral_against_fp64(fused):
    depth, _, _ = R.room_frames(6, (120, 160), seed=4)
    depth = spoil(depth, 4)
    got = fusion.bilateral(depth).cpu().numpy()
    exp = R.bilateral64(depth)
    assert np.array_equal(np.isfinite(got), np.isfinite(exp))
    assert np.array_equal(got == -np.inf, exp == -np.inf)
    fin = np.isfinite(exp)
    assert fin.mean() > 0.5
    assert np.abs(got[fin] - exp[fin]).max() <= 2e-6 * np.abs(exp[fin]).max()
    assert (np.abs(got[fin] - exp[fin]) <= 2e-6 * np.abs(exp[fin])).all()


@pytest.mark.parametrize('case', CASES)
def test_integrate_bitwise(fused, case):
    c = fused[case]
    ref, vol = c['ref'], c['vol']
    same_state(vol, ref)
    assert np.isfinite(ref.sdf).sum() > 5000
    assert ref.behind_updates > 0                                         # the reference's quirk is exercised
    if case == 'odd37x53x29':
        assert ref.weight.max() == 255
        inside = fusion.obb_contains(c['obb'], np.stack(np.meshgrid(*[np.arange(d) for d in c['dims']],
                                                                    indexing='ij'), -1)).transpose(2, 1, 0)
        assert not inside.all() and (ref.weight[~inside] == 0).all()


@pytest.mark.parametrize('case', CASES)
def test_chunking_and_repeat_are_bit_identical(fused, case):
    c = fused[case]
    for chunk in (1, 7, len(c['poses']), None):
        vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'])
        vol.integrate(c['filt'], c['k'], c['poses'], chunk=chunk)
        same_state(vol, c['ref'])
    # frames handed over in two calls fold in the same order
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g'], obb=c['obb'])
    vol.integrate(c['filt'][:9], c['k'][:9], c['poses'][:9]).integrate(c['filt'][9:], c['k'][9:], c['poses'][9:])
    same_state(vol, c['ref'])


@pytest.mark.parametrize('case', CASES)
def test_sparse_and_known(fused, case):
    c = fused[case]
    locs, vals = c['vol'].sparse()
    el, ev = c['ref'].sparse(6.0)
    assert len(ev) > 1000
    assert np.array_equal(locs.cpu().numpy().astype(np.int64), el.astype(np.int64))
    assert np.array_equal(vals.cpu().numpy().view(np.int32), ev.view(np.int32))
    assert np.array_equal(c['vol'].known().cpu().numpy(), c['ref'].known())
    _, v3 = c['vol'].sparse(3.0)
    assert np.array_equal(v3.cpu().numpy(), c['ref'].sparse(3.0)[1])


def test_copy_is_a_snapshot(fused):
    c = fused['cube48']
    vol = fusion.TSDFVolume(c['dims'], c['vs'], c['w2g']).integrate(c['filt'][:10], c['k'][:10], c['poses'][:10])
    snap = vol.copy()
    before = snap.sdf().clone()
    vol.integrate(c['filt'][10:], c['k'][10:], c['poses'][10:])
    assert torch.equal(snap.sdf(), before) and not torch.equal(vol.sdf(), before)
    same_state(vol, c['ref'])


@pytest.mark.parametrize('height', [0, 16, 64])
def test_scan_sample_equals_the_loaders(fused, tmp_path, height):
    c = fused['cube48']
    ind, tgd = tmp_path / 'in', tmp_path / 'tgt'
    ind.mkdir()
    tgd.mkdir()
    c['vol'].save(str(ind / 'scan.sdf'))
    c['vol'].save(str(tgd / 'scan.sdf'))
    got = fusion.scan_sample(c['vol'], 3.0, 4, height)
    b = next(iter(data.DeviceBatchLoader([str(ind / 'scan.sdf')], 1, 3.0, 4, max_input_height=height,
                                         target_path=str(tgd))))
    for a, e in ((got['input'][0], b['input'][0]), (got['input'][1], b['input'][1]), (got['known'], b['known']),
                 (got['world2grid'], b['world2grid'])):
        assert a.is_cuda and a.dtype == e.dtype and a.shape == e.shape
        assert torch.equal(a, e)
    assert torch.equal(got['orig_dims'], b['orig_dims'])
    assert tuple(b['sdf'].shape[2:]) == got['padded_dims']
    ds = data.SceneDataset([str(ind / 'scan.sdf')], None, 3.0, 4, height, target_path=str(tgd))
    h = data.collate([ds[0]])
    assert torch.equal(got['input'][0].cpu(), h['input'][0]) and torch.equal(got['input'][1].cpu(), h['input'][1])
    assert torch.equal(got['known'].cpu(), h['known'])
    assert len(got['input'][0]) > 1000
    if height == 16:
        assert int(got['input'][0][:, 0].max()) < 16 and int(c['vol'].sparse()[0][:, 2].max()) >= 16


def test_frames_to_model_loss_and_meshes(tmp_path):
    """Fuser.cpp's pair flow on a synthetic room: frames 0..9 -> input scan (snapshot), all frames -> target +
    .knw; DeviceBatchLoader scene mode -> GenModel forward -> targets and a masked loss -> meshes."""
    vs = 0.05
    depth, k, poses = R.room_frames(30, (120, 160), seed=7)
    w2g = R.grid_transform((-0.3, -0.3, -0.3), vs)                    # walls inside the grid: both sides seen
    dims = (92, 76, 64)
    filt = fusion.bilateral(spoil(depth, 7))
    vol = fusion.TSDFVolume(dims, vs, w2g).integrate(filt[:10], k[:10], poses[:10])
    ind, tgd = tmp_path / 'in', tmp_path / 'tgt'
    ind.mkdir()
    tgd.mkdir()
    vol.copy().save(str(ind / 'room.sdf'), known=False)
    vol.integrate(filt[10:], k[10:], poses[10:]).save(str(tgd / 'room.sdf'))
    sample = next(iter(data.DeviceBatchLoader([str(ind / 'room.sdf')], 1, 3.0, 4, max_input_height=64,
                                              target_path=str(tgd))))
    assert tuple(sample['sdf'].shape[2:]) == (64, 96, 96) and len(sample['input'][0]) > 5000

    torch.manual_seed(0)
    model = GenModel(8, (64, 64, 64), 1, 16, 16, 4, True, True, 1, 1).cuda()
    input_dim = np.array(sample['sdf'].shape[2:])
    model.update_sizes(input_dim, input_dim // 8)
    lw = np.ones(5, dtype=np.float32)
    with torch.no_grad():
        model.train()                                   # random init: batch statistics, so every level has sites
        output_sdf, output_occs = model(sample['input'], lw)
        sdf = sample['sdf']
        hierarchy = [sdf[:, :, ::f, ::f, ::f].contiguous() for f in (8, 4, 2)]
        t = L.compute_targets(sdf.clone(), hierarchy, 4, 3.0, True, sample['known'])
        loss, _ = L.compute_loss(output_sdf, output_occs, t[0], t[1], t[2], lw, 3.0, True, 1.0,
                                 sample['input'][0], True, sample['known'])
    assert torch.isfinite(loss).item() and len(output_sdf[0]) > 0
    od = sample['orig_dims'][0]
    keep = (output_sdf[0][:, 0] < od[0]) & (output_sdf[0][:, 1] < od[1]) & (output_sdf[0][:, 2] < od[2])
    pred = [[output_sdf[0][keep].cpu().numpy(), output_sdf[1][keep].squeeze(1).cpu().numpy()]]
    inputs = [sample['input'][0].cpu().numpy(), sample['input'][1].cpu().numpy()]
    out = tmp_path / 'vis'
    mc.save_predictions(str(out), sample['name'], inputs, None, None, pred, None, sample['world2grid'], 3.0)
    head = open(out / 'roominput-mesh.ply', 'rb').read(200).decode('ascii', 'ignore')
    assert int(head.split('element vertex ')[1].split('\n')[0]) > 500
    assert int(head.split('element face ')[1].split('\n')[0]) > 500
