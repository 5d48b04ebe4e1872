"""sgnn_amd.regrid on the device against tests/regrid_ref.py, bit for bit (sdf bits, weight, free counter and colour
record as integers), and against fusing on the destination grid.  The cases are
tests/regrid_cases.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_scenes as PS  # noqa: E402
import regrid_cases as RC  # noqa: E402
import regrid_ref as GR  # noqa: E402
from test_regrid_ref import (E2E_FACTOR, E2E_MEASURED, MERGE_EXTRA_MEASURED, MERGE_MEASURED, MIN_FAR_VOXELS,  # noqa: E402
                             MIN_VOXELS, RESAMPLE_EXTRA_MEASURED, RESAMPLE_MEASURED, extra_limits, limits)

from sgnn_amd import fusion, marching_cubes as mc, meshdist, points, regrid, render, voxelize  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def device_state(v):
    out = [bits(v.sdf().cpu().numpy()), v.weight().cpu().numpy().astype(np.int64),
           v.free_count().cpu().numpy().astype(np.int64)]
    if v.color_state() is not None:
        out.append(v.color_state().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64))
    return out


def ref_state(v):
    return [bits(v.sdf), v.weight, v.free] + ([] if v.color is None else [v.color])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def upload(ref):
    """A regrid_ref.Vol as a fusion.TSDFVolume with the same state."""
    v = fusion.TSDFVolume(ref.dims_xyz, ref.voxel_size, ref.world2grid, color=ref.color is not None)
    v._sdf.copy_(torch.from_numpy(ref.sdf))
    v._weight.copy_(torch.from_numpy(ref.weight.astype(np.uint8)))
    v._free.copy_(torch.from_numpy(ref.free.astype(np.int32)))
    if ref.color is not None:
        v._color.copy_(torch.from_numpy(ref.color.astype(np.uint16).view(np.int16)))
    return v


@functools.lru_cache(maxsize=None)
def source(color, dims=RC.SRC_DIMS, seed=5):
    return GR.random_volume(dims, seed, color=color, world2grid=RC.SRC_W2G)


@functools.lru_cache(maxsize=None)
def target(color, dims, seed=8):
    """A destination that already holds something, for the fold."""
    return GR.random_volume(dims, seed, color=color, world2grid=RC.similarity_w2g(dims))


@pytest.mark.parametrize('color', [False, True])
@pytest.mark.parametrize('mode', ['linear', 'nearest'])
@pytest.mark.parametrize('ddims', RC.DST_DIMS)
def test_store_and_fold_bit_exact_against_the_restatement(ddims, mode, color):
    src = source(color)
    assert 0.25 < np.isneginf(src.sdf).mean() < 0.45 and ((src.weight > 0) & np.isneginf(src.sdf)).sum() > 50
    w2g = RC.similarity_w2g(ddims)
    want = GR.resample(src, ddims, w2g, mode=mode)
    dev_src = upload(src)
    got = regrid.resample(dev_src, ddims, w2g, mode=mode)
    assert got.dims_xyz == tuple(ddims) and (got.color_state() is not None) == color and got.obb is None
    assert same(device_state(got), ref_state(want))
    if ddims == RC.DST_DIMS[0]:
        g = GR.positions(GR.grid_map(src.world2grid, w2g), ddims)
        outside = (g[0] < -1) | (g[0] > src.dims_xyz[0]) | (g[2] < -1) | (g[2] > src.dims_xyz[2])
        assert outside.mean() > 0.05 and (want.weight > 0).sum() > 100 and (want.weight == 0).sum() > 100
    # the fold into a destination that holds something, with and without colour on either side
    for dst_color in (color, not color):
        dst = target(dst_color, tuple(ddims))
        dev_dst = upload(dst)
        assert regrid.merge(dev_dst, dev_src, mode=mode) is dev_dst
        assert same(device_state(dev_dst), ref_state(GR.merge(dst.copy(), src, mode)))
    for skip in (True, False):
        for shape in (0, 1, 2):
            assert same(device_state(regrid.resample(dev_src, ddims, w2g, mode=mode, skip=skip, _shape=shape)),
                        ref_state(want))


@pytest.mark.parametrize('mode', ['linear', 'nearest'])
def test_a_source_with_a_dimension_of_one(mode):
    src = GR.random_volume((20, 1, 13), 9, color=True, world2grid=RC.EXACT_W2G)
    dev_src = upload(src)
    m = np.eye(4)
    m[:3, :3] = PS.rotation((0, 1, 0), 0.4) / 0.8          # a turn about y keeps the destination in the one y plane
    m[1, 1] = 1.0                                          # and y exact: g_y = j, so a_y == 0 and one plane suffices
    m[:3, 3] = (3.0, 0.0, 2.0)
    w2g = (np.linalg.inv(m) @ RC.EXACT_W2G).astype(F32)
    assert (GR.positions(GR.grid_map(src.world2grid, w2g), (19, 1, 14))[1] == 0).all()
    for ddims in ((19, 1, 14), (11, 3, 9)):
        want = GR.resample(src, ddims, w2g, mode=mode)
        assert same(device_state(regrid.resample(dev_src, ddims, w2g, mode=mode)), ref_state(want))
    assert (want.weight > 0).sum() > 5


@pytest.mark.parametrize('dims', RC.EXACT_DIMS)
@pytest.mark.parametrize('mode', ['linear', 'nearest'])
def test_exact_maps_against_numpy_slicing(dims, mode):
    src = RC.exact_source(dims)
    norm = RC.normalised(src)
    dev_src = upload(src)
    for name, ddims, m, expect in RC.exact_maps(dims):
        got = regrid.resample(dev_src, ddims, RC.exact_dst_w2g(m), mode=mode)
        want = [expect(a) for a in RC.arrays(norm)]
        want[0] = bits(want[0])
        assert same(device_state(got), want), name
    # the last plane and half-integer positions
    ddims = (2 * dims[0], dims[1] + 1, dims[2])
    want = GR.resample(src, ddims, RC.planes_w2g(), mode=mode)
    g = GR.positions(GR.grid_map(src.world2grid, RC.planes_w2g()), ddims)
    assert (g[0] == dims[0] - 1).any() and (g[0] % 1 == 0.5).any() and (g[1] == -0.5).any()
    for skip in (True, False):
        assert same(device_state(regrid.resample(dev_src, ddims, RC.planes_w2g(), mode=mode, skip=skip)),
                    ref_state(want))


def test_whole_blocks_outside_the_source_with_and_without_skip():
    src = source(True)
    dev_src = upload(src)
    m = np.eye(4)
    m[:3, :3] = PS.rotation((0.2, 0.1, 1.0), 0.5)
    m[:3, 3] = (-30.0, -16.0, -9.0)                          # most of the 70 x 33 x 21 destination misses the source
    w2g = (np.linalg.inv(m) @ RC.SRC_W2G.astype(np.float64)).astype(F32)
    ddims = (70, 33, 21)
    for mode in ('linear', 'nearest'):
        want = GR.resample(src, ddims, w2g, mode=mode)
        assert (want.weight > 0).sum() > 100 and (want.weight[:, :, :16] == 0).all() and (want.free[:, :, :16] == 0).all()
        dst = GR.random_volume(ddims, 12, color=True, world2grid=w2g)
        folded = ref_state(GR.merge(dst.copy(), src, mode))
        for skip in (True, False):
            for shape in (0, 1, 2):
                got = regrid.resample(dev_src, ddims, w2g, mode=mode, skip=skip, _shape=shape)
                assert same(device_state(got), ref_state(want))
            assert same(device_state(regrid.merge(upload(dst), dev_src, mode=mode, skip=skip)), folded)


def test_merge_twice_is_deterministic_and_pyramids_resample_level_by_level():
    src = source(True)
    dev_src = upload(src)
    ddims = RC.DST_DIMS[0]
    runs = []
    for _ in range(2):
        dst = upload(target(True, tuple(ddims)))
        regrid.merge(dst, dev_src)
        regrid.merge(dst, dev_src)
        runs.append(device_state(dst))
    assert same(runs[0], runs[1])
    ref = GR.merge(GR.merge(target(True, tuple(ddims)).copy(), src), src)
    assert same(runs[0], ref_state(ref))
    # a pyramid whose levels hold three different random states
    pyr = fusion.TSDFPyramid(RC.SRC_DIMS, 0.05, RC.SRC_W2G, levels=3, color=True)
    for k, level in enumerate(pyr.volumes):
        state = GR.random_volume(level.dims_xyz, 20 + k, color=True, world2grid=level.world2grid)
        pyr.volumes[k] = upload(state)
        pyr.volumes[k].voxel_size = level.voxel_size
    w2g = RC.similarity_w2g(ddims)
    out = regrid.resample_pyramid(pyr, ddims, w2g)
    assert len(out) == 3
    for k, level in enumerate(out.volumes):
        lw = (fusion.level_transform(k) @ w2g.astype(np.float64)).astype(F32)
        ld = tuple(-(-d // 2 ** k) for d in ddims)
        alone = regrid.resample(pyr[k], ld, lw)
        assert level.dims_xyz == ld and np.array_equal(level.world2grid, lw) and level.voxel_size == pyr[k].voxel_size
        assert same(device_state(level), device_state(alone)) and int((level.weight() > 0).sum()) > 0


@pytest.mark.parametrize('carve', [True, False])
def test_a_cloud_fused_directly_and_a_cloud_merged_are_one_fold(carve):
    """Rules P and Q.8 claim the same fold, and csrc/tsdf.h writes it once: a cloud integrated into V, and the same
    cloud integrated into an empty volume on V's grid that is then merged into a copy of V, leave the same bits in sdf,
    weight, free counter and colour record, in both modes (equal world2grid: the identity map, every a == 0).  The
    scene and what it exercises are checked on the restatements in tests/test_regrid_ref.py; the cloud goes in twice, so
    the second call meets the colour and the saturated weights of the first."""
    sc = RC.fold_scene()

    def empty():
        return fusion.TSDFVolume(sc['dims'], PS.VS, sc['w2g'], color=True)
    direct = empty().integrate(sc['depth'], sc['k'], sc['poses'])
    via = {mode: direct.copy() for mode in regrid.MODES}
    alone = points.integrate(empty(), sc['pts'], sc['org'], sc['oid'], color=sc['rgba'], carve=carve)
    x, y, z = RC.FOLD_VOXEL
    assert int(alone.weight()[z, y, x]) == 255 and int((direct.weight() > 0).sum()) > 3000
    for _ in range(2):
        points.integrate(direct, sc['pts'], sc['org'], sc['oid'], color=sc['rgba'], carve=carve)
        for mode, v in via.items():
            regrid.merge(v, alone, mode=mode)
            assert same(device_state(v), device_state(direct)), mode
    assert int((direct.color_weight() == 255).sum()) > 0


@functools.lru_cache(maxsize=None)
def device_routes():
    """The room on the device: frames rendered once; (A all six, B all six, A frames 0-2, B frames 3-5)."""
    room = PS.room()
    depth = render.render_depth(room['verts'], room['faces'], room['k'], room['poses'], PS.ROOM_HW)
    dims_b, w2g_b = RC.grid_b()

    def fuse(dims, w2g, sel):
        return fusion.TSDFVolume(dims, PS.VS, w2g).integrate(depth[sel], room['k'][sel], room['poses'][sel])
    return (fuse(room['dims'], room['w2g'], slice(0, 6)), fuse(dims_b, w2g_b, slice(0, 6)),
            fuse(room['dims'], room['w2g'], slice(0, 3)), fuse(dims_b, w2g_b, slice(3, 6)))


def figures(got, want):
    share, diff, n = PS.cross_route_figures(got.sdf().cpu().numpy(), got.weight().cpu().numpy(),
                                            want.sdf().cpu().numpy(), want.weight().cpu().numpy(), PS.VS)
    return n, share, diff


def extra(got, want):
    return RC.cross_route_extra(got.sdf().cpu().numpy(), got.weight().cpu().numpy(), want.sdf().cpu().numpy(),
                                want.weight().cpu().numpy(), PS.VS)


def test_cross_route_resample_against_fusing_on_the_yawed_grid():
    """Limits from tests/test_regrid_ref.py, measured there on the CPU: 4 766 voxels, 16.97 % differ in sign,
    max |dsdf| / vs 1.888, mean |dsdf| / vs 0.158, 3.35 % of the 2 446 voxels beyond 0.3 vs differ in sign; the limits
    are those figures plus half again."""
    a_all, b_all, _, _ = device_routes()
    dims_b, w2g_b = RC.grid_b()
    got = regrid.resample(a_all, dims_b, w2g_b)
    n, share, diff = figures(got, b_all)
    print('cross-route resample on the device: %d voxels, sign disagreements %.7f, max |dsdf| / vs %.7f' % (n, share, diff))
    assert n >= MIN_VOXELS and share <= limits(RESAMPLE_MEASURED)[0] and diff <= limits(RESAMPLE_MEASURED)[1]
    mean, far_share, far = extra(got, b_all)
    print('  mean |dsdf| / vs %.7f, sign disagreements beyond 0.3 vs %.7f of %d' % (mean, far_share, far))
    assert far >= MIN_FAR_VOXELS
    assert mean <= extra_limits(RESAMPLE_EXTRA_MEASURED)[0] and far_share <= extra_limits(RESAMPLE_EXTRA_MEASURED)[1]


def test_cross_route_merge_against_fusing_all_frames_on_the_yawed_grid():
    """Limits from tests/test_regrid_ref.py: 5 637 voxels, 7.97 % differ in sign, max |dsdf| / vs 1.896, mean
    |dsdf| / vs 0.078, 1.84 % of the 3 211 voxels beyond 0.3 vs differ in sign, plus half again."""
    _, b_all, a_012, b_345 = device_routes()
    merged = regrid.merge(b_345.copy(), a_012)
    n, share, diff = figures(merged, b_all)
    print('cross-route merge on the device: %d voxels, sign disagreements %.7f, max |dsdf| / vs %.7f' % (n, share, diff))
    assert n >= MIN_VOXELS and share <= limits(MERGE_MEASURED)[0] and diff <= limits(MERGE_MEASURED)[1]
    mean, far_share, far = extra(merged, b_all)
    print('  mean |dsdf| / vs %.7f, sign disagreements beyond 0.3 vs %.7f of %d' % (mean, far_share, far))
    assert far >= MIN_FAR_VOXELS
    assert mean <= extra_limits(MERGE_EXTRA_MEASURED)[0] and far_share <= extra_limits(MERGE_EXTRA_MEASURED)[1]


def test_end_to_end_box_voxelized_resampled_meshed_and_measured():
    """A box mesh voxelised on grid A, resampled to A yawed by 30 degrees about the box's centre, marching cubes, the
    meshdist accuracy (mean distance of 20 000 points of the extracted surface to the box).  The restatement route
    (voxelize_ref, regrid_ref, mc_oracle, meshdist_ref; tests/test_regrid_ref.py) gives 0.004317 m on the CPU; the
    allowance is 1.5 times that."""
    verts, faces = RC.e2e_box()
    dims_b, w2g_b = RC.e2e_grid_b()
    on_a = voxelize.mesh_to_volume(verts, faces, RC.E2E_DIMS, RC.E2E_VS, RC.e2e_w2g_a(), band=RC.E2E_BAND)
    on_b = regrid.resample(on_a, dims_b, w2g_b)
    v, _, f = mc.run_marching_cubes(on_b.sdf(), None, *RC.E2E_MC_ARGS)
    assert f.shape[0] > 1000 and int((on_b.weight() > 0).sum()) > 4000
    world = torch.from_numpy(RC.e2e_world(v.cpu().numpy(), w2g_b)).to(v.device)
    acc = meshdist.compare((world, f), (verts, faces), n=RC.E2E_SAMPLES, max_dist=RC.E2E_MAX_DIST)['accuracy']
    print('end to end on the device: accuracy %.9f m against %.9f m on the CPU, %d faces' % (acc, E2E_MEASURED, f.shape[0]))
    assert acc <= E2E_FACTOR * E2E_MEASURED
