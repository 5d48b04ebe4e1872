"""The rules of register.search on the CPU: the NumPy restatement alone finds a transform
that align alone cannot, and the scoring and selection rules have the properties the section states.  No GPU."""
import math

import numpy as np
import pytest

import register_ref as R
import register_search_ref as S

F32 = np.float32


@pytest.fixture(scope='module')
def room():
    return S.room_search_scene()


@pytest.fixture(scope='module')
def ladder(room):
    sdf, w2g, band, pts, centre, true, settings = room
    return S.search(pts, sdf, w2g, band, S.room_field(), **settings)


def basin(true, poses, centre):
    """Index and error of the pose nearest the truth: metres plus what the angle subtends at 1 m."""
    errs = [R.transform_error(true, t, centre) for t in poses]
    k = min(range(len(errs)), key=lambda i: errs[i][0] + math.radians(errs[i][1]))
    return k, errs[k]


def test_the_scene_is_out_of_aligns_reach(room):
    """70 degrees and 1.6 m: the yaw is a third of a step off the 30 degree turns, the centroid 0.35, 0.44 and 0.33
    pitches off the nearest lattice node; align from the identity does not get there."""
    sdf, w2g, band, pts, centre, true, settings = room
    assert S.ROOM_YAW >= 60 and abs(S.ROOM_YAW / settings['yaw_step'] % 1.0 - 1 / 3) < 1e-9
    assert np.linalg.norm(true[:3, 3]) >= 1.0
    origin, counts, pitch = S.lattice(sdf.shape, w2g, settings['step'], (0, 0, 1), settings['z_range'])
    sub = pts[::-(-len(pts) // settings['max_points'])].astype(np.float64)
    off = ((true[:3, :3] @ sub.mean(0) + true[:3, 3] - np.array(origin)) / pitch) % 1.0
    print('lattice %s, pitch %.3f m, centroid off a node by %s pitches' % (counts, pitch, np.round(off, 3)))
    assert (np.minimum(off, 1 - off) >= 0.33).all()
    res = R.align(pts, sdf, w2g, band)
    dt, dr = R.transform_error(true, res.T, centre)
    print('align from the identity: ok %s, %d pairs, %.3g m %.3g deg off' % (res.ok, res.pairs, dt, dr))
    assert (not res.ok) or dt > float(band)


def test_the_restatement_recovers_the_transform(room, ladder):
    """The end of the ladder is align, so the final error is the resolution of section R's rules: rounding noise.
    Section R records 1.53e-7 m and 6.29e-7 degrees (register_ref.ALIGN_ERROR) for near guesses of this room, and argues
    and asserts its bound: two ulps of a 4.4 m coordinate, 1e-6 m, and the angle that subtends at 1 m.  The source
    world here rounds every point anew, so the noise is another draw from the same resolution: it is held to that
    bound (6.5 times R's figure), and the recorded figure of this run from above at the 1.5x of R's records."""
    sdf, w2g, band, pts, centre, true, settings = room
    T, tr = ladder
    order = np.argsort(tr.level0[:, 0], kind='stable')
    print('level 0: %d poses, %d scoring points, best cost %d, worst %d' % (
        len(order), len(pts[::-(-len(pts) // settings['max_points'])]), tr.level0[order[0], 0], tr.level0[order[-1], 0]))
    for level, (poses, scores) in enumerate(tr.kept):
        k, (dt, dr) = basin(true, poses, centre)
        rank = int(np.argsort(scores[:, 0], kind='stable').tolist().index(k))
        print('level %d: true basin is kept[%d], rank %d of %d by cost, cost %d, inliers %d, %.3f m %.2f deg off' % (
            level, k, rank, len(poses), scores[k, 0], scores[k, 1], dt, dr))
        assert rank == 0                                                    # the asymmetric room: the basin leads
    costs = [s[basin(true, p, centre)[0], 0] for p, s in tr.kept]
    assert all(b <= a for a, b in zip(costs, costs[1:]))                    # a level never raises the cost: 0 offset is scored
    assert T is not None
    dt, dr = R.transform_error(true, T, centre)
    print('final error: %.4g m %.4g deg' % (dt, dr))
    assert dt <= 1e-6 and dr <= math.degrees(1e-6)
    assert dt <= 1.5 * S.SEARCH_ERROR[0] and dr <= 1.5 * S.SEARCH_ERROR[1]   # the record in section X is this run's


def test_two_volumes_of_one_box():
    """The figure tests/test_gpu_register_search.py holds search_volumes to: section R's box voxelised twice on one grid,
    the second time turned by 40 degrees and moved by 30 cm.  A cuboid maps onto itself under three half turns, so the
    error is taken against the nearest of the four equivalent transforms; the kept candidates show the twins (several
    end with the same rmse).  The two volumes sample the box on different lattices: a fraction of a millimetre, as in
    section R, not rounding."""
    T, tr, true, pts, centre = S.box_search_ref()
    assert T is not None and len(tr.level0) == 36 * 7 * 6 * 5
    dt, dr = S.nearest_twin(true, T, centre)
    plain = R.transform_error(true, T, centre)
    print('box: %d points, final error %.4g m %.4g deg against the nearest twin (%.4g m %.4g deg against the truth)' % (
        len(pts), dt, dr, plain[0], plain[1]))
    print('kept costs per level: %s' % [s[:, 0].tolist() for _, s in tr.kept])
    assert dt <= float(R.BOX_VS) / 10 and dr <= 0.5                         # far inside a voxel: the basin, not a neighbour
    assert dt <= 1.5 * S.BOX_SEARCH_ERROR[0] and dr <= 1.5 * S.BOX_SEARCH_ERROR[1]   # the record in section X is this run's


def test_a_pose_onto_seed_centres_costs_nothing():
    """Points that a pose maps exactly onto the centres of seed voxels: cost 0, all inliers, none outside."""
    sdf, w2g = R.small_volume()
    field = S.distance_field(sdf, w2g, R.SMALL_BAND, 4.0)
    idx = np.argwhere(field.dist2 == 0)[::3]                                # z, y, x
    grid = idx[:, ::-1].astype(np.float64)
    inv = np.linalg.inv(w2g.astype(np.float64))                             # exact: powers of two and quarters
    world = grid @ inv[:3, :3].T + inv[:3, 3]
    shift = np.eye(4)
    shift[:3, 3] = [0.5, -0.25, 1.0]                                        # exact in fp32 as well
    pts = (world - shift[:3, 3]).astype(F32)
    assert np.array_equal(pts.astype(np.float64), world - shift[:3, 3])
    for inlier2 in (0, 4):
        assert S.score(pts, field, shift, inlier2).tolist() == [[0, len(pts), 0]]
    assert S.score(pts, field, np.eye(4), 0)[0, 0] > 0


def test_a_nan_record_scores_everything_outside():
    sdf, w2g = R.small_volume()
    field = S.distance_field(sdf, w2g, R.SMALL_BAND, 4.0)
    pts = R.small_points(40)
    for bad in (np.nan, np.inf, 1e300):                                     # 1e300: finite in fp64, not in fp32
        T = np.eye(4)
        T[1, 3] = bad
        assert np.isnan(S.pose_rows(w2g, T)).all()
        assert S.score(pts, field, T).tolist() == [[len(pts) * field.cap2, 0, len(pts)]]
    w_bad = w2g.copy()
    w_bad[2, 2] = np.nan
    assert np.isnan(S.pose_rows(w_bad, np.eye(4))).all()
    assert np.array_equal(S.pose_rows(w2g, np.eye(4)), w2g[:3].reshape(12))
    assert np.array_equal(S.pose_rows_many(w2g, np.stack([np.eye(4), T])), np.stack([S.pose_rows(w2g, np.eye(4)),
                                                                                     S.pose_rows(w2g, T)]),
                          equal_nan=True)


def test_the_cost_is_monotone_in_the_cap():
    sdf, w2g = R.small_volume()
    pts = R.small_points(200)
    T = np.stack(R.small_transforms()[1:])
    dist2 = S.dist2_of(S.seeds(sdf, R.SMALL_BAND), 6.0)
    last = None
    for cap2 in (1, 2, 5, 9, 16, 36, 1000):
        sc = S.score_rows(pts, dist2, S.pose_rows_many(w2g, T), cap2, 1)
        assert last is None or (sc[:, 0] >= last[:, 0]).all()
        assert last is None or np.array_equal(sc[:, 1:], last[:, 1:])       # inliers and outside do not see the cap
        last = sc
    assert (sc[:, 2] > 0).all() and (sc[:, 0] >= 1000 * sc[:, 2]).all()     # the edge cases of small_points are outside


def test_selection_keeps_no_neighbours():
    rng = np.random.default_rng(5)
    nr, nz, ny, nx = 6, 3, 5, 7
    costs = rng.integers(0, 40, size=nr * nz * ny * nx)                     # many ties: the index decides

    def decode(i):
        return i // (nx * ny * nz), (i // (nx * ny)) % nz, (i // nx) % ny, i % nx

    for cyclic in (0, nr):
        kept = S.select(costs, decode, 12, cyclic)
        assert len(kept) == 12 and kept[0] == int(np.argmin(costs))
        assert [costs[i] for i in kept] == sorted(costs[i] for i in kept)
        for a in range(len(kept)):
            for b in range(a):
                (r, z, y, x), (q, qz, qy, qx) = decode(kept[a]), decode(kept[b])
                dr = min(abs(r - q), nr - abs(r - q)) if cyclic else abs(r - q)
                assert dr > 1 or max(abs(z - qz), abs(y - qy), abs(x - qx)) > 1
    assert len(S.select(costs[:8], lambda i: (0, 0, 0, i), 16)) == 4        # a row of 8: every other one at the most


def test_field_by_hand():
    """One crossing pair on a row: both voxels are seeds, distances are squared voxel counts, -1 beyond the reach."""
    sdf = np.full((1, 2, 7), 1.0, F32)
    sdf[0, 0, 3:] = -1.0                                                    # crossings: x pair (2, 3) of row 0; y pairs x >= 3
    sdf[0, 0, 6] = np.nan
    seeds = S.seeds(sdf, 3.0)
    assert seeds[0, 0].tolist() == [False, False, True, True, True, True, False]
    assert seeds[0, 1].tolist() == [False, False, False, True, True, True, False]
    d = S.dist2_of(seeds, 1.5)
    assert d[0, 0].tolist() == [-1, 1, 0, 0, 0, 0, 1] and d[0, 1].tolist() == [-1, 2, 1, 0, 0, 0, 1]
