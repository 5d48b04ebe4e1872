"""GPU: the upright kernels (sgnn_amd.upright, csrc/upright.hip) against the NumPy restatement of tests/upright_ref.py:
every histogram and every fixed-point sum bit for bit, find() equal to the same host steps run on the restatement's
integers, and straighten() against the share the restatement reaches on the CPU (tests/test_upright_ref.py)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import points_scenes as PS  # noqa: E402
import upright_ref as U  # noqa: E402

from sgnn_amd import fusion, upright  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SKEW = np.array([0.31, -0.52, 0.79])                                        # the gradient of small_volume's skew plane


CASE_SEED = {'rotated': 1, 'aligned': 2}


def grid(kind):
    if kind == 'rotated':
        return PS.world2grid()
    m = np.eye(4)
    m[:3, :3] /= float(PS.VS)
    m[:3, 3] = (3.25, -1.5, 7.75)
    return m.astype(F32)


@functools.lru_cache(maxsize=None)
def case(dims, kind):
    """(sdf, w2g, band, surface, records, the arguments of the height pass) of one volume: one set-up, shared."""
    if dims == 'room':
        sdf, w2g, dims = U.room_scene()[:3]
        band, surface, axis = F32(3.0) * U.VS, U.VS, U.room_hint()
    else:
        w2g = grid(kind)
        sdf, band, surface = U.small_volume(dims, w2g, seed=CASE_SEED[kind]), F32(3.0), F32(1.0)
        axis = w2g[:3, :3].astype(np.float64).T @ SKEW
    axis = axis / np.linalg.norm(axis)
    e1, e2 = upright.plane_frame(axis)
    records = upright.axis_table(np.stack([axis, axis + np.nan, axis, -axis]), np.stack([e1, e1, e1, e2]),
                                 np.stack([e2, e2, e2, e1]), [math.cos(math.radians(20.0)), 0.9, 1.5, 0.5],
                                 [math.sin(math.radians(30.0)), 0.5, 0.7, -1.0])
    assert np.isnan(records['u'][1]).all() and records['cos_cone'][2] > 1
    h0, size, nbins = upright.height_bins(dims, w2g, axis, PS.VS)
    return sdf, w2g, band, surface, records, (axis.astype(F32), F32(0.9), h0, size, nbins)


CASES = [((3, 3, 3), 'rotated'), ((3, 3, 3), 'aligned'), ((2, 9, 9), 'rotated'), ((70, 37, 19), 'rotated'),
         ((70, 37, 19), 'aligned'), ('room', 'aligned')]


@pytest.mark.parametrize('dims,kind', CASES)
def test_the_three_passes_against_the_restatement(dims, kind):
    sdf, w2g, band, surface, records, hargs = case(dims, kind)
    dev = torch.from_numpy(sdf).cuda()
    n = len(U.surface_voxels(sdf, w2g, band, surface)['v'])
    for bins in (8, 16, 32):
        got = upright.normal_histogram(dev, w2g, band, surface, bins)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (6, bins, bins)
        exp = U.histogram(sdf, w2g, band, surface, bins)
        assert np.array_equal(got.cpu().numpy(), exp) and int(exp.sum()) == n
    got = upright.axis_sums(dev, w2g, band, surface, records)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (4, 8)
    exp = U.sums(sdf, w2g, band, surface, [tuple(r)[:5] for r in records])
    assert np.array_equal(got.cpu().numpy(), exp)
    assert not exp[1].any() and not exp[2, :5].any() and not exp[3, 5:].any()     # the NaN record, the empty cone, no wall
    one = upright.axis_sums(dev, w2g, band, surface, records[:1])                   # B does not show in a record
    assert tuple(one.shape) == (1, 8) and np.array_equal(one.cpu().numpy()[0], exp[0])
    assert tuple(upright.axis_sums(dev, w2g, band, surface, records[:0]).shape) == (0, 8)
    rows = upright.height_histogram(dev, w2g, band, surface, *hargs)
    assert rows.is_cuda and rows.dtype == torch.int32 and tuple(rows.shape) == (2, hargs[4])
    exp_rows = U.heights(sdf, w2g, band, surface, *hargs)
    assert np.array_equal(rows.cpu().numpy(), exp_rows)
    print('%s %s: %d surface voxels; record 0 %s; heights %d + %d' % (dims, kind, n, exp[0].tolist(), exp_rows[0].sum(),
                                                                      exp_rows[1].sum()))
    if dims == (2, 9, 9):
        assert n == 0 and not exp.any() and not exp_rows.any()                      # nothing launched, all zeros
    elif dims == (3, 3, 3):
        assert n == 1
    else:
        assert n > 500 and exp[0, 3] + exp[0, 4] > 100 and exp[0, 7] > 100 and exp[2, 7] > 100 and exp_rows.sum() > 100
        assert exp[3, 3] > 0 and exp[3, 4] > 0                                      # the wide cone about the flipped axis


def test_gates_and_ties_are_exercised():
    """The inputs the bit-for-bit test relies on are really there: every special value next to a surface, and on the
    axis-aligned grid the two planes whose normals sit on a cell border and on a tie for the major axis."""
    sdf, w2g, band, surface = case((70, 37, 19), 'aligned')[:4]
    plain = np.where(np.isfinite(sdf), sdf, 0)
    near = len(U.surface_voxels(np.clip(plain, -2.5, 2.5), w2g, band, F32(1.01))['v'])
    assert near > len(U.surface_voxels(sdf, w2g, band, surface)['v'])               # the gates drop voxels
    for value in (-np.inf, np.inf, 3.0, -3.0, 1.0, -1.0):
        assert (sdf == F32(value)).sum() >= 1000
    assert np.isnan(sdf).sum() >= 1000
    m = U.surface_voxels(sdf, w2g, band, surface)['m']
    flat = (m[:, 0] == 0) & (m[:, 1] == 0)
    tie = (m[:, 0] == 0) & (np.abs(m[:, 1]) == np.abs(m[:, 2])) & (m[:, 1] != 0)
    assert flat.sum() > 50 and tie.sum() > 50
    hist = U.histogram(sdf, w2g, band, surface, 16)
    assert hist[4, 8, 8] + hist[5, 8, 8] == flat.sum() and hist[4, 8, 8] > 50      # a = b = 0: the upper of the two cells
    assert hist[2].sum() + hist[3].sum() >= tie.sum()                               # |my| = |mz|: a y face, not a z face
    assert hist[2, 8, 0] > 0 and hist[2, 8, 15] > 0                                 # a = -1 and a = +1: the outer cells


def test_launch_independence():
    sdf, w2g, band, surface, records, hargs = case((70, 37, 19), 'rotated')
    dev = torch.from_numpy(sdf).cuda()
    big = torch.full((sdf.shape[0] + 2, sdf.shape[1] + 3, sdf.shape[2] + 5), 0.25, device='cuda')
    view = big[1:-1, 2:-1, 3:-2]
    view.copy_(dev)
    assert not view.is_contiguous()
    host_tensor = torch.from_numpy(sdf.copy())
    first = None
    for source in (dev, dev, view, sdf, host_tensor):
        out = (upright.normal_histogram(source, w2g, band, surface, 16).cpu().numpy(),
               upright.axis_sums(source, torch.from_numpy(w2g.copy()), band, surface, records).cpu().numpy(),
               upright.height_histogram(source, w2g, band, surface, *hargs).cpu().numpy())
        first = first or out
        assert all(np.array_equal(a, b) for a, b in zip(first, out))


@pytest.fixture(scope='module')
def room_volume():
    sdf, w2g, dims, up, walls = U.room_scene()
    vol = fusion.TSDFVolume(dims, U.VS, w2g)
    vol.sdf().copy_(torch.from_numpy(sdf))
    vol.weight().copy_(torch.from_numpy(np.isfinite(sdf).astype(np.uint8)))
    return vol, sdf, w2g, dims, up, walls


def test_find_equals_the_host_steps_on_the_restatements_integers(room_volume):
    vol, sdf, w2g, dims, up, walls = room_volume
    passes = U.Passes(sdf, w2g, F32(3.0) * U.VS, U.VS)
    for kw in (dict(up_hint=U.room_hint()), dict(), dict(up_hint=U.room_hint(), bins=32, cones=(15.0, 4.0), wall_tol=5.0)):
        got = upright.find(vol, **kw)
        exp = upright.solve(passes, dims, w2g, U.VS, **kw)
        assert got.ok and got.yaw_ok and got.votes == exp.votes and got.R.dtype == np.float64
        assert np.array_equal(got.R, exp.R) and np.array_equal(got.up, exp.up)
        assert got.yaw == exp.yaw and got.yaw_confidence == exp.yaw_confidence
        assert got.floor == exp.floor and got.ceiling == exp.ceiling
        print('%s: up %.4f degrees, wall %.4f degrees off; floor %.4f ceiling %.4f; votes %s' % (
            sorted(kw), U.angle_deg(got.up, up), U.wall_error_deg(got.R[0], walls), got.floor, got.ceiling, got.votes))
        assert U.angle_deg(got.up, up) <= 0.25 and U.wall_error_deg(got.R[0], walls) <= 0.25
    triple = upright.find((vol.sdf(), w2g, U.VS), up_hint=U.room_hint())            # the volume as a triple
    assert np.array_equal(triple.R, upright.find(vol, up_hint=U.room_hint()).R)
    empty = fusion.TSDFVolume(dims, U.VS, w2g)
    res = upright.find(empty, up_hint=U.room_hint())
    assert not res.ok and np.array_equal(res.R, np.eye(3)) and res.votes == (0, 0, 0)


def test_straighten(room_volume):
    """At least 95 % of the up-facing surface voxels of the floor lie in two adjacent z layers of the straightened
    volume (the restatement alone reaches 100 % on the CPU, tests/test_upright_ref.py; in the tilted volume it is 23 %),
    and straightening the result once more finds a frame within 0.25 degrees of the identity."""
    vol, sdf, w2g, dims, up, walls = room_volume
    level, T, res = upright.straighten(vol, up_hint=U.room_hint(), pad=2, mode='linear')
    assert isinstance(level, fusion.TSDFVolume) and res.ok and np.array_equal(T, upright.transform(res, 0.0))
    box = (level.world2grid.astype(np.float64) @ np.linalg.inv(T)).astype(F32)      # the upright world -> its grid
    share, n = U.floor_layer_share(level.sdf().cpu().numpy(), box, U.VS)
    print('%.4f of %d up-facing floor voxels in two adjacent layers' % (share, n))
    assert n > 1000 and share >= 0.95
    upright_vol = fusion.TSDFVolume(level.dims_xyz, U.VS, box)
    upright_vol.sdf().copy_(level.sdf())
    upright_vol.weight().copy_(level.weight())
    again, T2, res2 = upright.straighten(upright_vol, up_hint=(0, 0, 1))
    turn = math.degrees(math.acos(min(1.0, (np.trace(res2.R) - 1.0) / 2.0)))
    print('second pass: %.4f degrees from the identity, floor %.4f m' % (turn, res2.floor))
    assert res2.ok and res2.yaw_ok and turn <= 0.25 and abs(res2.floor) <= 0.5 * float(U.VS)


def test_argument_errors():
    sdf, w2g, band, surface, records, hargs = case((70, 37, 19), 'rotated')
    dev = torch.from_numpy(sdf).cuda()
    launches = upright._lib.load().sgnn_launch_count
    before = launches()
    singular = w2g.copy()
    singular[2] = singular[1]
    bad = [dict(sdf=dev[0]), dict(sdf=dev[None]), dict(w2g=singular), dict(w2g=w2g[:3]), dict(w2g=w2g * np.nan),
           dict(band=-1.0), dict(band=0.0), dict(surface=-0.5), dict(surface=float('nan'))]
    for change in bad:
        a = dict(dict(sdf=dev, w2g=w2g, band=band, surface=surface), **change)
        with pytest.raises(ValueError):
            upright.normal_histogram(a['sdf'], a['w2g'], a['band'], a['surface'])
        with pytest.raises(ValueError):
            upright.axis_sums(a['sdf'], a['w2g'], a['band'], a['surface'], records)
        with pytest.raises(ValueError):
            upright.height_histogram(a['sdf'], a['w2g'], a['band'], a['surface'], *hargs)
    for bins in (0, 12, 64, 16.5):
        with pytest.raises(ValueError):
            upright.normal_histogram(dev, w2g, band, surface, bins)
    with pytest.raises(ValueError):
        upright.axis_sums(dev, w2g, band, surface, np.zeros((1, 12), F32))
    for change in (dict(up=(0, 0)), dict(up=(0, np.nan, 1)), dict(cos_cone=0.0), dict(bin=0.0), dict(nbins=0),
                   dict(nbins=4097), dict(h0=np.inf)):
        a = dict(dict(up=hargs[0], cos_cone=hargs[1], h0=hargs[2], bin=hargs[3], nbins=hargs[4]), **change)
        with pytest.raises(ValueError):
            upright.height_histogram(dev, w2g, band, surface, **a)
    vol = (dev, w2g, PS.VS)
    for kw in (dict(up_hint=(0, 0, 0)), dict(bins=12), dict(band=-1.0), dict(surface=-1.0), dict(cones=()),
               dict(max_tilt=-5.0, up_hint=(0, 0, 1)), dict(min_votes=0)):
        with pytest.raises(ValueError):
            upright.find(vol, **kw)
    for v in ((dev, w2g), (dev, singular, PS.VS), (dev, w2g, 0.0), (dev[0], w2g, PS.VS), 'volume'):
        with pytest.raises(ValueError):
            upright.find(v)
    with pytest.raises(ValueError):
        upright.straighten(vol)
    assert launches() == before                                                     # raised before any launch
    upright.normal_histogram(dev, w2g, band, surface)
    assert launches() > before
