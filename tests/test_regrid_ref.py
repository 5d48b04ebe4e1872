"""tests/regrid_ref.py, the NumPy restatement of INTEGRATION.md section Q, held to facts that need no device, and the
cross-route figures of that section measured on the CPU.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_scenes as PS  # noqa: E402
import regrid_cases as RC  # noqa: E402
import regrid_ref as GR  # noqa: E402

F32 = np.float32

# Cross-route figures measured here on the CPU (fusion_ref + regrid_ref on the room of points_scenes, 6 poses, 60 x 80,
# 5 cm voxels, grid B = grid A yawed by 30 degrees about the up axis through the room's centre), over the voxels where
# both B volumes are observed and |sdf| < vs; the limits of the device tests are those figures plus half again:
#   resample A -> B against B fused directly: 4 766 voxels, 16.97 % differ in sign, max |dsdf| / vs = 1.888
#   frames 0-2 on A merged into frames 3-5 on B against all six on B: 5 637 voxels, 7.97 %, 1.896
# (voxels, sign share, max |dsdf| / vs).  The sign share is large because grid B's voxel centres lie at every distance
# from the walls (grid A keeps them 0.37 of a voxel off), and the frame route's own per-voxel noise (nearest-pixel depth
# look-up, median |dsdf| 0.08 vs between the routes) decides the sign of a voxel that close to the surface: the voxels
# that disagree have a mean |sdf| of 0.2 vs on either route.
#
# Those two limits are loose (a quarter of the signs, 2.8 voxels), so two more figures over the same selection are held
# the same way (regrid_cases.cross_route_extra): the mean |dsdf| / vs, and the sign share among the voxels more than
# 0.3 vs off the surface on both routes, where the noise above no longer decides:
#   resample: mean |dsdf| / vs = 0.158, 3.35 % of 2 446 voxels;  merge: 0.078, 1.84 % of 3 211
RESAMPLE_MEASURED = (4766, 0.1697441, 1.8882724)
MERGE_MEASURED = (5637, 0.0796523, 1.8957371)
RESAMPLE_EXTRA_MEASURED = (0.1582942, 0.0335241, 2446)
MERGE_EXTRA_MEASURED = (0.0778667, 0.0183743, 3211)
MIN_VOXELS = 2000
MIN_FAR_VOXELS = 1000

# End to end (regrid_cases.e2e_ref): a 0.66 x 0.52 x 0.37 m box voxelised on a 26 x 24 x 20 grid of 5 cm voxels (band 4),
# resampled to its 35 x 34 x 20 box under a 30 degree yaw, marching cubes, mean distance of 20 000 points of the
# extracted surface to the box.  Measured here on the CPU (voxelize_ref, regrid_ref, mc_oracle, meshdist_ref):
# 0.004317 m (0.086 vs) over 1 484 faces; the device test allows 1.5 times that.
E2E_MEASURED = 0.004317059
E2E_FACTOR = 1.5


def limits(measured):
    return 1.5 * measured[1], 1.5 * measured[2]


def extra_limits(measured):
    return 1.5 * measured[0], 1.5 * measured[1]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(xs, ys):
    return len(xs) == len(ys) and all(
        np.array_equal(bits(x), bits(y)) if x.dtype == F32 else np.array_equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize('dims', RC.EXACT_DIMS)
@pytest.mark.parametrize('mode', ['linear', 'nearest'])
def test_exact_maps_reproduce_the_source(dims, mode):
    src = RC.exact_source(dims)
    norm = RC.normalised(src)
    assert np.isneginf(src.sdf).mean() > 0.25 and ((src.weight > 0) & np.isneginf(src.sdf)).any()
    assert any(1 in d for d in RC.EXACT_DIMS)
    for name, ddims, m, expect in RC.exact_maps(dims):
        got = GR.resample(src, ddims, RC.exact_dst_w2g(m), mode=mode)
        want = [expect(a) for a in RC.arrays(norm)]
        assert same(RC.arrays(got), want), name
    # a crop and a pad on the source's own world2grid (equal matrices: the identity map), any world2grid
    odd = GR.random_volume(dims, 4, color=True, world2grid=PS.world2grid())
    pad = GR.resample(odd, [d + 2 for d in dims], PS.world2grid(), mode=mode)
    sx, sy, sz = dims
    assert same([a[:sz, :sy, :sx] for a in RC.arrays(pad)], RC.arrays(RC.normalised(odd)))
    assert pad.weight[sz:].sum() == 0 and pad.weight[:, sy:].sum() == 0 and pad.weight[:, :, sx:].sum() == 0


def test_a_linear_field_survives_a_general_rotation():
    """An sdf that is linear in position is reproduced by trilinear interpolation up to rounding.  Against the field
    evaluated in fp64 at the fp32 position g the kernel forms (a = g - floor(g) is exact), the error is: one rounding of
    every corner value (u Smax, u = 2^-24, Smax = max |field|), and per lerp level one rounding each of q - p
    (|q - p| <= 2 Smax), of the product and of the sum: at most 5 u Smax; three levels -> 16 u Smax."""
    src = GR.Vol(RC.SRC_DIMS, 0.05, RC.SRC_W2G)
    z, y, x = np.indices(src.sdf.shape).astype(np.float64)
    coef = np.array([0.013, -0.021, 0.034, -0.11])
    field = coef[0] * x + coef[1] * y + coef[2] * z + coef[3]
    src.sdf[...] = field.astype(F32)
    src.weight[...] = 7
    for ddims in RC.DST_DIMS:
        w2g = RC.similarity_w2g(ddims)
        got = GR.resample(src, ddims, w2g)
        g = [v.astype(np.float64) for v in GR.positions(GR.grid_map(src.world2grid, w2g), ddims)]
        want = coef[0] * g[0] + coef[1] * g[1] + coef[2] * g[2] + coef[3]
        ok = got.weight > 0
        assert ok.sum() > 20 and (got.weight[ok] == 7).all() and np.isneginf(got.sdf[~ok]).all()
        assert (~ok).any() or ddims != RC.DST_DIMS[0]
        err = np.abs(got.sdf[ok].astype(np.float64) - want[ok]).max()
        bound = 16 * 2.0 ** -24 * np.abs(field).max()
        print('linear field %s: max error %.3e, bound %.3e' % (ddims, err, bound))
        assert err <= bound


def test_one_bad_corner_makes_a_sample_unseen_unless_its_weight_is_zero():
    src = GR.Vol((3, 3, 3), 0.05, np.eye(4), color=True)
    src.sdf[...] = np.arange(27, dtype=F32).reshape(3, 3, 3) / 16
    src.weight[...] = 9
    src.free[...] = 2
    src.color[...] = (256, 512, 768, 5)
    src.weight[1, 1, 1] = 0                                   # the corner (1, 1, 1) of the cell (0, 0, 0)

    def at(gx, gy, gz, mode='linear'):
        a = np.array([[1, 0, 0, gx], [0, 1, 0, gy], [0, 0, 1, gz]], F32)
        s, w, f, c = GR.sample(src, (1, 1, 1), a, mode)
        return float(s[0, 0, 0]), int(w[0, 0, 0]), int(f[0, 0, 0]), c[0, 0, 0].tolist()
    assert at(0.5, 0.5, 0.5) == (-np.inf, 0, 2, [0, 0, 0, 0])                  # free is that of r = (1, 1, 1)
    s, w, f, c = at(0.5, 0.5, 0.0)                                             # a_z == 0: the z + 1 plane takes no part
    assert (s, w, f, c) == ((0 + 1 + 3 + 4) / 4 / 16, 9, 2, [256, 512, 768, 5])
    assert at(0.5, 0.5, 2.0)[1] == 9 and at(0.5, 0.5, 2.25)[1] == 0            # the last plane; past it
    assert at(1.0, 1.0, 1.0) == (-np.inf, 0, 2, [0, 0, 0, 0])                  # the bad voxel itself
    assert at(0.5, 0.5, 0.5, 'nearest')[1] == 0 and at(0.49, 0.5, 0.5, 'nearest')[1] == 9
    assert at(0.49, 0.49, 0.49, 'nearest') == (0.0, 9, 2, [256, 512, 768, 5])
    assert at(-0.5, 0.0, 0.0, 'nearest') == (-np.inf, 0, 0, [0, 0, 0, 0])      # halves go away from zero: r = -1


def test_the_merge_fold_by_hand():
    w2g = PS.world2grid()
    src = GR.random_volume(RC.SRC_DIMS, 5, color=True, world2grid=RC.SRC_W2G)
    for ddims in RC.DST_DIMS:
        for mode in ('linear', 'nearest'):
            empty = GR.Vol(ddims, 0.05, RC.similarity_w2g(ddims), color=True)
            assert same(RC.arrays(GR.merge(empty, src, mode)),
                        RC.arrays(GR.resample(src, ddims, RC.similarity_w2g(ddims), mode=mode)))
    # an empty source changes nothing at all
    dst = GR.random_volume((9, 8, 3), 6, color=True, world2grid=w2g)
    before = [a.copy() for a in RC.arrays(dst)]
    GR.merge(dst, GR.Vol(RC.SRC_DIMS, 0.05, RC.SRC_W2G, color=True))
    assert same(RC.arrays(dst), before)
    # two voxels by hand
    a, b = GR.Vol((2, 1, 1), 0.05, w2g, color=True), GR.Vol((2, 1, 1), 0.05, w2g, color=True)
    a.sdf[0, 0, 0], a.weight[0, 0, 0], a.free[0, 0, 0], a.color[0, 0, 0] = F32(0.1), 3, 1, (1000, 2000, 3000, 2)
    b.sdf[0, 0, 0], b.weight[0, 0, 0], b.free[0, 0, 0], b.color[0, 0, 0] = F32(-0.2), 5, 4, (500, 100, 65535, 7)
    a.weight[0, 0, 1], a.free[0, 0, 1] = 0, 7
    b.sdf[0, 0, 1], b.weight[0, 0, 1], b.color[0, 0, 1] = F32(0.25), 255, (1, 2, 3, 4)
    GR.merge(a, b)
    mean = (F32(0.1) * F32(3) + F32(-0.2) * F32(5)) / (F32(3) + F32(5))
    assert bits(a.sdf[0, 0, 0]) == bits(mean) and a.weight[0, 0, 0] == 8 and a.free[0, 0].tolist() == [5, 7]
    # (1000 2 + 500 7 + 4) / 9 = 611, (2000 2 + 100 7 + 4) / 9 = 522, (3000 2 + 65535 7 + 4) / 9 = 51638
    assert a.color[0, 0, 0].tolist() == [611, 522, 51638, 9]
    assert bits(a.sdf[0, 0, 1]) == bits(F32(0.25)) and a.weight[0, 0, 1] == 255
    assert a.color[0, 0, 1].tolist() == [1, 2, 3, 4]
    GR.merge(a, b)                                             # 8 + 5, and the saturated voxel stays at 255
    assert a.weight[0, 0].tolist() == [13, 255] and a.color[0, 0, :, 3].tolist() == [16, 8]
    # a source without colour leaves colours alone; a destination without colour ignores them
    c = GR.Vol((2, 1, 1), 0.05, w2g)
    c.sdf[...], c.weight[...] = F32(0.5), 1
    kept = a.color.copy()
    assert np.array_equal(GR.merge(a, c).color, kept) and a.weight[0, 0, 0] == 14
    assert GR.merge(c, b).color is None and c.weight[0, 0].tolist() == [6, 255]


@pytest.mark.parametrize('carve', [True, False])
def test_a_cloud_fused_directly_and_a_cloud_merged_are_one_fold(carve):
    """Rules P and Q.8 claim the same fold (csrc/tsdf.h writes it once): a cloud integrated into V, and the same cloud
    integrated into an empty volume on V's grid that is then merged into a copy of V, leave the same bits.  With equal
    world2grid the map is the identity and every a == 0, so both modes qualify.  The cloud goes in twice: the second
    call meets the colour and the saturated weights the first one left."""
    import fusion_ref as FR
    import points_ref as PR
    sc = RC.fold_scene()
    cloud = (sc['pts'], sc['org'], sc['oid'], sc['rgba'], carve)
    filled = FR.Grid(sc['dims'], PS.VS, sc['w2g']).integrate(sc['depth'], sc['k'], sc['poses'])
    direct = PR.Volume(sc['dims'], PS.VS, sc['w2g'], color=True)
    direct.sdf, direct.weight, direct.free = filled.sdf.copy(), filled.weight.copy(), filled.free.copy()
    via = {mode: RC.as_vol(direct) for mode in ('linear', 'nearest')}
    alone = PR.integrate(PR.Volume(sc['dims'], PS.VS, sc['w2g'], color=True), *cloud)
    x, y, z = RC.FOLD_VOXEL
    assert (filled.weight > 0).sum() > 3000 and ((filled.weight > 0) & (alone.weight > 0)).sum() > 300
    assert ((filled.weight == 0) & (alone.weight > 0)).sum() > 50 and (alone.color[..., 3] > 0).sum() > 200
    assert alone.weight[z, y, x] == 255 and alone.free.max() > RC.FOLD_AIMED // 2
    for _ in range(2):
        PR.integrate(direct, *cloud)
        for mode, v in via.items():
            GR.merge(v, RC.as_vol(alone), mode)
            assert same(RC.arrays(v), RC.arrays(RC.as_vol(direct))), mode
    assert direct.weight[z, y, x] == 255 and (direct.color[..., 3] == 255).any()


def figures(got, want):
    share, diff, n = PS.cross_route_figures(got.sdf, got.weight, want.sdf, want.weight, PS.VS)
    return n, share, diff


def extra(got, want):
    return RC.cross_route_extra(got.sdf, got.weight, want.sdf, want.weight, PS.VS)


def test_cross_route_resample_against_fusing_on_the_yawed_grid():
    """Measured here: RESAMPLE_MEASURED at the top of this file; this test holds the restatement to the device's limits."""
    resampled, direct, _, _ = RC.cross_route_ref()
    n, share, diff = figures(resampled, direct)
    print('cross-route resample on the CPU: %d voxels, sign disagreements %.7f, max |dsdf| / vs %.7f' % (n, share, diff))
    assert n >= MIN_VOXELS
    assert share <= limits(RESAMPLE_MEASURED)[0] and diff <= limits(RESAMPLE_MEASURED)[1]
    mean, far_share, far = extra(resampled, direct)
    print('  mean |dsdf| / vs %.7f, sign disagreements beyond 0.3 vs %.7f of %d' % (mean, far_share, far))
    assert far >= MIN_FAR_VOXELS
    assert mean <= extra_limits(RESAMPLE_EXTRA_MEASURED)[0] and far_share <= extra_limits(RESAMPLE_EXTRA_MEASURED)[1]


def test_cross_route_merge_against_fusing_all_frames_on_the_yawed_grid():
    _, direct, merged, _ = RC.cross_route_ref()
    n, share, diff = figures(merged, direct)
    print('cross-route merge on the CPU: %d voxels, sign disagreements %.7f, max |dsdf| / vs %.7f' % (n, share, diff))
    assert n >= MIN_VOXELS
    assert share <= limits(MERGE_MEASURED)[0] and diff <= limits(MERGE_MEASURED)[1]
    mean, far_share, far = extra(merged, direct)
    print('  mean |dsdf| / vs %.7f, sign disagreements beyond 0.3 vs %.7f of %d' % (mean, far_share, far))
    assert far >= MIN_FAR_VOXELS
    assert mean <= extra_limits(MERGE_EXTRA_MEASURED)[0] and far_share <= extra_limits(MERGE_EXTRA_MEASURED)[1]


def test_end_to_end_box_through_the_restatement_route():
    """Measured here: E2E_MEASURED at the top of this file.  The box's inside is negative on A, the resampled volume
    keeps a closed band around the surface, and the extracted surface lies within a tenth of a voxel of the box."""
    acc, faces, on_a, on_b = RC.e2e_ref()
    print('end to end on the CPU: accuracy %.9f m (%.4f vs), %d faces, %d -> %d observed voxels'
          % (acc, acc / float(RC.E2E_VS), faces, (on_a.weight > 0).sum(), (on_b.weight > 0).sum()))
    assert on_a.sdf[10, 12, 13] < 0 and on_a.sdf[10, 12, 3] > 0
    assert faces > 1000 and (on_b.weight > 0).sum() > 4000
    assert acc <= E2E_FACTOR * E2E_MEASURED and acc < 0.1 * float(RC.E2E_VS)
