"""GPU: register.search (sgnn_amd.register, csrc/register_search.hip) against the NumPy restatement of
tests/register_search_ref.py.  Every device result is an integer and is compared bit for bit: the scores of the kernel
at its edges, the field, the level-0 scores, the kept poses of every level and the guesses handed to align.  Only the
final transform, which align's fp64 summation order touches, is held to 1.5 times the error the restatement reaches on
the CPU (tests/test_register_search_ref.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import register_ref as G  # noqa: E402
import register_search_ref as S  # noqa: E402

from sgnn_amd import _lib, fusion, register, voxelize  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
EINVAL = -1
CAP2 = 9
DIMS = [(2, 3, 5), (7, 1, 9)]                                               # z, y, x; the second has an axis of 1


# ---------------------------------------------------------------------------------------------------------
# the kernel alone: a dist2 volume built by hand, records given as rows
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand(dims):
    """(dist2 with -1 entries, zeros and values above CAP2; a pool of 5000 points in grid coordinates; 257 records)."""
    dz, dy, dx = dims
    rng = np.random.default_rng(dx * 100 + dz)
    dist2 = rng.integers(-1, 14, size=dims).astype(np.int32)
    dist2.reshape(-1)[:4] = (0, -1, CAP2 + 3, CAP2)
    assert (dist2 == -1).any() and (dist2 == 0).any() and (dist2 > CAP2).any()
    special = []
    mid = [F32((d - 1) // 2) for d in (dx, dy, dz)]
    for axis, d in enumerate((dx, dy, dz)):
        def along(v):
            p = list(mid)
            p[axis] = F32(v)
            return p
        for n in range(d + 1):                                              # the rounding of rule 3: exact half-integers
            special += [along(n - 0.5), along(n + 0.5)]
        lo, hi = F32(-0.5), F32(d - 0.5)                                    # one ulp either side of each face
        special += [along(np.nextafter(lo, F32(-np.inf))), along(np.nextafter(lo, F32(np.inf))),
                    along(np.nextafter(hi, F32(-np.inf))), along(np.nextafter(hi, F32(np.inf)))]
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38):
            special.append(along(v))
    special = np.array(special, F32)
    rand = rng.uniform(-1.5, np.array([dx, dy, dz]) + 0.5, size=(5000 - len(special), 3)).astype(F32)
    pool = np.concatenate([special, rand])[rng.permutation(5000)]
    pool[0] = special[1]                                                    # P = 1 scores a half-integer
    rows = np.zeros((257, 12), F32)
    rows[:] = np.eye(4, dtype=F32)[:3].reshape(12)
    rows[1] = np.nan                                                        # a NaN record
    rows[2, 3] = 1000.0                                                     # sends every point outside
    rows[3, 0] = np.nan                                                     # the kernel tests m[0]
    for b in range(4, 257):                                                 # small turns, scales and shifts of the grid
        a = rng.uniform(-0.4, 0.4)
        m = np.eye(4)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, :3] *= rng.uniform(0.7, 1.2)
        m[:3, 3] = rng.uniform(-1.0, 1.0, size=3)
        rows[b] = m[:3].astype(F32).reshape(12)
    rows[5, 7] = np.inf                                                     # a row that makes every g_y non-finite
    return dist2, pool, rows


@functools.lru_cache(maxsize=None)
def hand_expected(dims, npts, inlier2):
    dist2, pool, rows = hand(dims)
    return S.score_rows(pool[:npts], dist2, rows, CAP2, inlier2)            # one reference per (dims, P), shared


def device_scores(dims, pts, rows, inlier2, cap2=CAP2, dist2=None):
    dist2 = hand(dims)[0] if dist2 is None else dist2
    field = register.SearchField(torch.from_numpy(dist2).cuda(), np.eye(4, dtype=F32), dims, cap2)
    table = np.zeros(len(rows), dtype=register.POSE_DTYPE)
    table['m'] = rows
    out = register._score_table(torch.from_numpy(np.ascontiguousarray(pts)).cuda(), field, table, inlier2)
    assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (len(rows), 3)
    return out.cpu().numpy()


@pytest.mark.parametrize('dims', DIMS)
@pytest.mark.parametrize('npts', [0, 1, 63, 64, 65, 257, 5000])
def test_scores_at_the_edges(dims, npts):
    """5000 points are 20 tiles of 256: with few records the launch slices them across blocks that add with atomics,
    with 257 records it has two blocks of lanes; 0 points write zeros."""
    dist2, pool, rows = hand(dims)
    exp = hand_expected(dims, npts, 4)
    for nb in (0, 1, 63, 65, 257):
        got = device_scores(dims, pool[:npts], rows[:nb], 4)
        assert np.array_equal(got, exp[:nb]), (dims, npts, nb)
    if npts:
        assert exp[0, 2] > 0 or npts == 1
        assert exp[1].tolist() == [npts * CAP2, 0, npts] and exp[2].tolist() == exp[1].tolist() == exp[3].tolist()
    else:
        assert not exp.any()


@pytest.mark.parametrize('dims', DIMS)
def test_inlier_bounds_repeats_and_splits(dims):
    dist2, pool, rows = hand(dims)
    last = None
    for inlier2 in (0, 4, CAP2):
        exp = hand_expected(dims, 257, inlier2)
        got = device_scores(dims, pool[:257], rows[:65], inlier2)
        assert np.array_equal(got, exp[:65])
        assert last is None or ((got[:, 1] >= last[:, 1]).all() and np.array_equal(got[:, [0, 2]], last[:, [0, 2]]))
        last = got
    again = device_scores(dims, pool[:257], rows[:65], CAP2)
    assert np.array_equal(again, last)                                      # the same inputs, the same bits
    halves = np.concatenate([device_scores(dims, pool[:257], rows[:31], CAP2),
                             device_scores(dims, pool[:257], rows[31:65], CAP2)])
    assert np.array_equal(halves, last)                                     # B does not show in a record's sums


def test_the_record_index_goes_past_65535():
    dims = DIMS[0]
    dist2, pool, rows = hand(dims)
    many = np.tile(rows, (273, 1))[:70000].copy()
    many[65536:, 3] += F32(1.0)                                             # the far records differ from the near ones
    pts = pool[[1, 70, 4000]]
    got = device_scores(dims, pts, many, 4)
    exp = S.score_rows(pts, dist2, many[:514], CAP2, 4)                     # the table repeats every 257 records
    exp_far = S.score_rows(pts, dist2, many[65536:65536 + 514], CAP2, 4)
    first_far = 65536 % 257
    for b0 in range(0, 65536 - 256, 257):
        assert np.array_equal(got[b0:b0 + 257], exp[:257])
    assert np.array_equal(got[65536:65536 + 514], exp_far)
    assert np.array_equal(got[65536 - first_far:65536], exp[:first_far])
    assert np.array_equal(got[-200:], S.score_rows(pts, dist2, many[-200:], CAP2, 4))
    assert not np.array_equal(exp_far[:257 - first_far], exp[first_far:257])


def test_invalid_arguments_return_einval():
    """By the return value only; every pointer handed over is a valid allocation of the size the valid call needs."""
    lib = _lib.load()
    dims = DIMS[0]
    dist2, pool, rows = hand(dims)
    d = torch.from_numpy(dist2).cuda()
    p = torch.from_numpy(pool[:8].copy()).cuda()
    t = torch.from_numpy(rows[:4].copy()).cuda()
    out = torch.full((4, 3), -7, dtype=torch.int64, device='cuda')
    ok = dict(points=p.data_ptr(), npoints=8, dist2=d.data_ptr(), dx=5, dy=3, dz=2, poses=t.data_ptr(), nposes=4, cap2=CAP2,
              inlier2=4, out=out.data_ptr())

    def call(**change):
        a = dict(ok, **change)
        return lib.sgnn_register_score(a['points'], a['npoints'], a['dist2'], a['dx'], a['dy'], a['dz'], a['poses'],
                                       a['nposes'], a['cap2'], a['inlier2'], a['out'], _lib.stream())

    for change in (dict(points=None), dict(dist2=None), dict(poses=None), dict(out=None), dict(dx=0), dict(dy=-1),
                   dict(dz=0), dict(dx=2048, dy=1024, dz=1024), dict(cap2=0), dict(cap2=-3), dict(inlier2=-1),
                   dict(npoints=-1), dict(npoints=2 ** 31 - 65536), dict(nposes=-1), dict(nposes=(1 << 24) + 1)):
        assert call(**change) == EINVAL, change
        assert b'sgnn_register_score' in lib.sgnn_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all()                                                # nothing was written
    assert call(nposes=0) == 0 and call(nposes=0, poses=None, out=None) == 0
    torch.cuda.synchronize()
    assert (out == -7).all()
    assert call(npoints=0, points=None) == 0                                # no points: zeros
    torch.cuda.synchronize()
    assert not out.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), S.score_rows(pool[:8], dist2, rows[:4], CAP2, 4))


# ---------------------------------------------------------------------------------------------------------
# the host mirror and the field
# ---------------------------------------------------------------------------------------------------------
def test_score_forms_the_records_of_rule_1():
    sdf, w2g = G.small_volume()
    dev_field = register.distance_field((torch.from_numpy(sdf).cuda(), w2g, G.SMALL_BAND), 4.0)
    field = S.distance_field(sdf, w2g, G.SMALL_BAND, 4.0)
    assert dev_field.cap2 == field.cap2 == 16 and dev_field.dims == sdf.shape
    assert np.array_equal(dev_field.dist2.cpu().numpy(), field.dist2)
    pts = G.small_points(300)
    Ts = np.stack(G.small_transforms())                                     # the first is not finite
    for inlier, inlier2 in ((None, 1), (0, 0), (2.5, 6)):
        got = register.score(pts, dev_field, Ts, inlier=inlier)
        exp = S.score(pts, field, Ts, inlier2)
        assert np.array_equal(got.cpu().numpy(), exp)
    assert exp[0].tolist() == [300 * 16, 0, 300]
    one = register.score(torch.from_numpy(pts).cuda(), dev_field, Ts[2])
    assert tuple(one.shape) == (1, 3) and np.array_equal(one.cpu().numpy()[0], S.score(pts, field, Ts[2])[0])
    assert tuple(register.score(pts, dev_field, np.zeros((0, 4, 4))).shape) == (0, 3)


@pytest.fixture(scope='module')
def room():
    sdf, w2g, band, pts, centre, true, settings = S.room_search_scene()
    vol = fusion.TSDFVolume((88, 72, 60), G.VS, w2g)
    vol.sdf().copy_(torch.from_numpy(sdf))
    return vol, S.room_search_scene()


def test_the_field_of_the_small_volume_and_of_the_room(room):
    vol, (sdf, w2g, band, pts, centre, true, settings) = room
    small_sdf, small_w2g = G.small_volume()
    for reach in (1.0, 2.5, 10.0):
        got = register.distance_field((small_sdf, small_w2g, G.SMALL_BAND), reach)
        exp = S.distance_field(small_sdf, small_w2g, G.SMALL_BAND, reach)
        assert got.dist2.is_cuda and got.dist2.dtype == torch.int32 and got.cap2 == exp.cap2
        assert np.array_equal(got.dist2.cpu().numpy() == 0, S.seeds(small_sdf, G.SMALL_BAND))
        assert np.array_equal(got.dist2.cpu().numpy(), exp.dist2)
    got = register.distance_field(vol, S.ROOM_REACH_VOX * float(vol.voxel_size))    # metres for a TSDFVolume
    exp = S.room_field()
    assert got.cap2 == exp.cap2 == 100 and np.array_equal(got.world2grid, w2g)
    assert np.array_equal(got.dist2.cpu().numpy() == 0, S.seeds(sdf, band))
    assert np.array_equal(got.dist2.cpu().numpy(), exp.dist2)
    assert register.distance_field(vol).cap2 == 99                          # 0.5 m of fp32 0.05 m voxels: just under 10


# ---------------------------------------------------------------------------------------------------------
# the ladder
# ---------------------------------------------------------------------------------------------------------
def test_the_ladder_step_by_step(room):
    """The CPU test's scene and settings.  Integers and poses exactly; the final transform within 1.5 times the error the
    restatement reaches (register_search_ref.SEARCH_ERROR), the margin of sections H, I and R: the same rules run and
    only the fp64 summation order of align differs."""
    vol, (sdf, w2g, band, pts, centre, true, settings) = room
    _, ref = S.search(pts, sdf, w2g, band, S.room_field(), finish=False, **settings)
    field = register.distance_field(vol, S.ROOM_REACH_VOX * float(vol.voxel_size))
    trace = {}
    res = register.search(pts, vol, field=field, trace=trace, **settings)
    assert np.array_equal(np.array(trace['lattice'][0]), np.array(ref.lattice[0])) and trace['lattice'][1:] == ref.lattice[1:]
    assert torch.equal(trace['level0'].cpu(), torch.from_numpy(ref.level0))
    assert len(trace['kept']) == len(ref.kept) == settings['levels'] + 1
    for level, ((poses, scores), (ref_poses, ref_scores)) in enumerate(zip(trace['kept'], ref.kept)):
        assert np.array_equal(poses, ref_poses), 'level %d' % level
        assert np.array_equal(scores, ref_scores), 'level %d' % level
    assert np.array_equal(trace['guesses'], ref.guesses)
    assert [c[1:] for c in res.candidates] == [tuple(int(v) for v in s) for s in ref.kept[-1][1]]
    assert all(np.array_equal(c[0], g) for c, g in zip(res.candidates, ref.guesses))
    assert res.ok and res.result is not None and res.field is field
    dt, dr = G.transform_error(true, res.T, centre)
    print('search: %d pairs, rmse %.3g m, %.4g m %.4g deg from the true transform' % (res.result.pairs, res.result.rmse,
                                                                                      dt, dr))
    assert dt <= 1.5 * S.SEARCH_ERROR[0] and dr <= 1.5 * S.SEARCH_ERROR[1]
    alone = register.align(pts, vol)                                        # the search is what found it
    off = G.transform_error(true, alone.T, centre)
    assert (not alone.ok) or off[0] > float(band)
    same = register.search(pts, vol, reach=S.ROOM_REACH_VOX * float(vol.voxel_size), **settings)   # builds its own field
    assert np.array_equal(same.T, res.T) and same.ok


def test_search_volumes_of_two_boxes():
    """Section R's box voxelised twice, the second time turned by 40 degrees and moved by 30 cm, with the defaults of
    search_volumes.  A cuboid maps onto itself under three half turns, so the error is taken against the nearest of the
    four equivalent transforms, as tests/test_register_search_ref.py does for the record
    register_search_ref.BOX_SEARCH_ERROR; the bound is 1.5 times that record."""
    true = S.box_search_true()
    src = voxelize.mesh_to_volume(*G.box_mesh(), G.BOX_DIMS, G.BOX_VS, G.box_w2g(), band=G.BOX_VOX_BAND)
    dst = voxelize.mesh_to_volume(*G.box_mesh(true), G.BOX_DIMS, G.BOX_VS, G.box_w2g(), band=G.BOX_VOX_BAND)
    assert np.array_equal(dst.sdf().cpu().numpy().view(np.int32), G.box_volume_ref(true).view(np.int32))
    trace = {}
    res = register.search_volumes(src, dst, stride=G.BOX_STRIDE, trace=trace)
    ref = S.box_search_ref(finish=False)[1]
    assert torch.equal(trace['level0'].cpu(), torch.from_numpy(ref.level0))
    assert np.array_equal(trace['guesses'], ref.guesses) and len(res.candidates) == 16
    centre = register.surface_points(src, stride=G.BOX_STRIDE).double().mean(0).cpu().numpy()
    dt, dr = S.nearest_twin(true, res.T, centre)
    print('search_volumes: %d pairs, rmse %.6f m, %.6f m %.5f deg from the nearest twin of the true transform' % (
        res.result.pairs, res.result.rmse, dt, dr))
    assert res.ok and dt <= 1.5 * S.BOX_SEARCH_ERROR[0] and dr <= 1.5 * S.BOX_SEARCH_ERROR[1]
    with pytest.raises(ValueError):
        register.search_volumes((dst.sdf(), dst.world2grid, 0.15), dst)
