"""GPU: depth rendering (sgnn_amd.render, csrc/render.hip) against the NumPy restatement of tests/render_ref.py, bit
for bit, and a rendered mesh through fusion, the scene sample and the model."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402

from sgnn_amd import fusion, marching_cubes as mc, render  # noqa: E402
from sgnn_amd.model import GenModel  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HW = (48, 64)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == exp.shape
    g, e = bits(got), bits(exp)
    assert np.array_equal(g, e), '%d of %d pixels differ' % ((g != e).sum(), g.size)


def counted(verts, faces, k, poses, hw, **kw):
    c = torch.zeros(3, dtype=torch.int64, device='cuda')
    out = render.render_depth(verts, faces, k, poses, hw, counters=c, **kw)
    return out, [int(v) for v in c.cpu()]


@pytest.mark.parametrize('n', [2, 9])
def test_room_bitwise(n):
    _, k, poses = R.room_frames(24, HW, seed=1)
    verts, faces = RR.tessellate_room(n)
    exp = RR.render_ref(verts, faces, k, poses, HW)
    assert np.isfinite(exp).mean() > 0.9
    got, (lane, wave, pixels) = counted(verts, faces, k, poses, HW)
    same(got, exp)
    same(render.render_depth(verts, faces, k, poses, HW), exp)
    assert pixels >= np.isfinite(exp).sum() and lane + wave > 0
    if n == 2:
        assert wave > 0                                                  # 2 m triangles fill the 64 x 48 image


def test_triangle_soup_takes_both_paths():
    verts, faces = RR.triangle_soup(20000, seed=7)
    _, k, poses = R.room_frames(3, (60, 80), seed=3)
    exp = RR.render_ref(verts, faces, k, poses, (60, 80), depth_min=0.1, depth_max=50.0)
    assert np.isfinite(exp).mean() > 0.2 and len(np.unique(exp)) > 2000
    got, (lane, wave, pixels) = counted(verts, faces, k, poses, (60, 80), depth_min=0.1, depth_max=50.0)
    same(got, exp)
    assert lane > 1000 and wave > 100, (lane, wave)
    # the split between the two paths does not show in the image
    for wave_pixels in (1, 1 << 30):
        old = render.WAVE_PIXELS
        render.WAVE_PIXELS = wave_pixels
        try:
            g2, (l2, w2, p2) = counted(verts, faces, k, poses, (60, 80), depth_min=0.1, depth_max=50.0)
        finally:
            render.WAVE_PIXELS = old
        same(g2, exp)
        assert p2 == pixels and l2 + w2 == lane + wave
        assert (w2 == 0) if wave_pixels > 1 else (w2 > lane)


def test_near_plane_bitwise():
    k = np.array([0.8 * 64, 0.8 * 64, 31.5, 23.5], F32)
    poses = np.stack([R.look_at((0.05, 0.5, 1.3), (0.6, 3.0, 1.2)), R.look_at((1.85, 1.3, 0.5), (1.6, 0.0, 0.4))])
    kk = np.tile(k, (2, 1))
    for n in (1, 4):
        verts, faces = RR.tessellate_room(n)
        exp = RR.render_ref(verts, faces, kk, poses, HW)
        assert np.isfinite(exp).any() and (exp == -np.inf).any()
        same(render.render_depth(verts, faces, kk, poses, HW), exp)
        exp2 = RR.render_ref(verts, faces, kk, poses, HW, z_clip=0.3, depth_min=0.3, depth_max=2.5)
        same(render.render_depth(verts, faces, kk, poses, HW, z_clip=0.3, depth_min=0.3, depth_max=2.5), exp2)


@pytest.mark.parametrize('nf,hw', [(1, (48, 64)), (37, (37, 53)), (5, (1, 3))])
def test_frame_lists_and_odd_sizes(nf, hw):
    k = np.array([0.8 * hw[1], 0.8 * hw[1], (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0], F32)
    poses = R.room_trajectory(nf, seed=4)
    if nf > 10:
        poses[3, 1, 2] = np.nan                                          # non-finite pose: an empty frame
        poses[9, 0, 3] = np.inf
        poses[20] = R.look_at((-5.0, 1.0, 1.0), (-9.0, 1.0, 1.0))        # outside the room, looking away
    kk = np.tile(k, (nf, 1))
    verts, faces = RR.tessellate_room(5)
    exp = RR.render_ref(verts, faces, kk, poses, hw)
    if nf > 10:
        assert (exp[[3, 9, 20]] == -np.inf).all() and np.isfinite(exp[4]).any()
    same(render.render_depth(verts, faces, kk, poses, hw), exp)


def test_chunks_order_and_residence_change_no_bit():
    _, k, poses = R.room_frames(37, HW, seed=6)
    verts, faces = RR.tessellate_room(6)
    exp = RR.render_ref(verts, faces, k, poses, HW)
    for chunk in (1, 5, 37, None):
        same(render.render_depth(verts, faces, k, poses, HW, chunk=chunk), exp)
    rng = np.random.default_rng(0)
    shuffled = faces[rng.permutation(len(faces))]
    flip = rng.random(len(faces)) < 0.5
    shuffled[flip] = shuffled[flip][:, ::-1]
    same(render.render_depth(verts, shuffled, k, poses, HW), exp)
    dv, df = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    same(render.render_depth(dv, df, torch.from_numpy(k).cuda(), torch.from_numpy(poses).cuda(), HW), exp)
    same(render.render_depth(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(k),
                             torch.from_numpy(poses), HW), exp)
    same(render.render_depth(dv, df.to(torch.int64), k, poses, HW), exp)


def test_argument_errors():
    _, k, poses = R.room_frames(2, HW, seed=1)
    verts, faces = RR.tessellate_room(2)
    bad = faces.copy()
    bad[7, 1] = len(verts)
    with pytest.raises(ValueError, match='face index'):
        render.render_depth(verts, bad, k, poses, HW)
    with pytest.raises(ValueError, match='face index'):
        render.render_depth(verts, torch.from_numpy(bad).cuda(), k, poses, HW)
    bad[7, 1] = -1
    with pytest.raises(ValueError, match='face index'):
        render.render_depth(verts, bad, k, poses, HW)
    with pytest.raises(ValueError, match='face index'):
        render.render_depth(torch.from_numpy(verts).cuda(), torch.from_numpy(bad).cuda(), k, poses, HW)
    with pytest.raises(ValueError):
        render.render_depth(verts[:, :2], faces, k, poses, HW)
    with pytest.raises(ValueError):
        render.render_depth(verts, faces.reshape(-1, 6), k, poses, HW)
    with pytest.raises(ValueError):
        render.render_depth(verts, faces, k[0], poses, HW)
    with pytest.raises(ValueError):
        render.render_depth(verts, faces, k, poses[:1], HW)
    with pytest.raises(ValueError):
        render.render_depth(verts, faces, k, poses, (1 << 15, 1 << 15))
    with pytest.raises(ValueError):
        render.render_depth(verts, faces, k, poses, HW, z_clip=0.0)
    same(render.render_depth(verts, faces, k, poses, HW), RR.render_ref(verts, faces, k, poses, HW))


def test_mesh_to_frames_to_volume_to_model():
    """A fused room -> marching cubes -> the mesh rendered along new poses -> fused again -> scene sample -> one
    eval forward of a small GenModel, all on the device.

    "Occupied" is the project's own notion, the one the targets of the loss and the rows of scan_sample use
    (loss.compute_targets: |sdf / voxel| < truncation, truncation 3): every occupied voxel of the re-fused volume
    must lie within two voxels (Euclidean) of an occupied voxel of the first.  Measured: all 35 769 within one voxel
    (34 677 coincide).  A band of one voxel around zero is not a usable notion of the surface here: a projective
    TSDF falls by more than one voxel size per voxel where the surface was seen at a grazing angle, so a zero
    crossing need not have a voxel with |sdf| <= one voxel next to it, and which voxels have one depends on the
    viewpoints.  That narrower set is printed as a measurement only: 3 of its 9 690 voxels are further than two
    voxels from the first volume's, all three at the vertical edge x = 2.6, y = 0.3 of a box whose face y = 0.3 the
    first trajectory saw edge-on only (first volume there: -2.4, -2.4 and unobserved)."""
    vs = 0.05
    depth, k, poses = R.room_frames(30, (120, 160), seed=7)
    w2g = R.grid_transform((-0.3, -0.3, -0.3), vs)
    dims = (92, 76, 64)
    first = fusion.TSDFVolume(dims, vs, w2g).integrate(depth, k, poses)
    tsdf = first.sdf() / vs                                               # voxel units, -inf = no data
    verts_vox, _, faces = mc.run_marching_cubes(tsdf, None, 0.0, 3.0, 10.0)
    assert verts_vox.is_cuda and len(faces) > 5000
    g2w = torch.from_numpy(np.linalg.inv(w2g.astype(np.float64))).to(verts_vox.device)
    verts = (verts_vox.double() @ g2w[:3, :3].T + g2w[:3, 3]).float()     # voxel -> world metres
    _, k2, poses2 = R.room_frames(30, (120, 160), seed=8)
    frames = render.render_depth(verts, faces, k2, poses2, (120, 160))
    assert frames.is_cuda and torch.isfinite(frames).float().mean().item() > 0.5
    second = fusion.TSDFVolume(dims, vs, w2g).integrate(frames, k2, poses2)
    truncation = 3.0
    s1, s2 = (first.sdf() / vs).cpu().numpy(), (second.sdf() / vs).cpu().numpy()

    def squared_distance(occ_a, occ_b):
        """For the voxels of occ_b: squared distance (voxels) to the nearest voxel of occ_a, 99 beyond three."""
        oa = np.pad(occ_a, 3)
        z, y, x = occ_b.shape
        dist2 = np.full(occ_b.shape, 99, np.int64)
        for dz in range(-3, 4):
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    d2 = dz * dz + dy * dy + dx * dx
                    if d2 <= 9:
                        hit = oa[3 + dz:3 + dz + z, 3 + dy:3 + dy + y, 3 + dx:3 + dx + x]
                        dist2 = np.where(hit, np.minimum(dist2, d2), dist2)
        return dist2[occ_b]

    def histogram(d2):
        return dict(zip(*(v.tolist() for v in np.unique(d2, return_counts=True))))

    occ1, occ2 = np.abs(s1) < truncation, np.abs(s2) < truncation          # loss.compute_targets' occupancy
    assert occ2.sum() > 20000
    d2_occ = squared_distance(occ1, occ2)
    print('re-fused occupied voxels: %d; squared distance to the first volume\'s: %s' % (occ2.sum(), histogram(d2_occ)))
    print('measurement only, |sdf| <= one voxel: %s' % histogram(squared_distance(np.abs(s1) <= 1.0, np.abs(s2) <= 1.0)))
    assert (d2_occ <= 4).all(), '%d of %d re-fused occupied voxels are more than two voxels off' % (
        (d2_occ > 4).sum(), occ2.sum())
    sample = fusion.scan_sample(second, 3.0, 4, 64)
    assert len(sample['input'][0]) > 5000
    torch.manual_seed(0)
    model = GenModel(8, (64, 64, 64), 1, 16, 16, 4, True, True, 1, 1).cuda()
    input_dim = np.array(sample['padded_dims'])
    model.update_sizes(input_dim, input_dim // 8)
    lw = np.ones(5, dtype=np.float32)
    saved = []
    for mod in model.modules():                                           # running statistics := this scan's statistics,
        if isinstance(mod, torch.nn.BatchNorm3d):                         # so that the eval forward of a random
            saved.append((mod, mod.momentum))                             # initialisation keeps every level populated
            mod.momentum = 1.0
        elif hasattr(mod, 'running_mean') and hasattr(mod, 'momentum'):
            saved.append((mod, mod.momentum))                             # scn BatchNormReLU: weight of the OLD value
            mod.momentum = 0.0
    with torch.no_grad():
        model.train()
        model(sample['input'], lw)
        for mod, mom in saved:
            mod.momentum = mom
        model.eval()
        output_sdf, output_occs = model(sample['input'], lw)
    assert len(output_sdf[0]) > 0 and torch.isfinite(output_sdf[1]).all()
    assert all(torch.isfinite(o[1]).all() for o in output_occs)
