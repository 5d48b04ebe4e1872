"""GPU: mesh distances (sgnn_amd.meshdist, csrc/meshdist.hip) against the NumPy restatement of tests/meshdist_ref.py,
bit for bit, and a fused, extracted room mesh compared with the mesh it was rendered from."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import meshdist_ref as M  # noqa: E402
import render_ref as RR  # noqa: E402

from sgnn_amd import fusion, marching_cubes as mc, meshdist, render  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x, F32).view(np.int32)


def same(got, exp):
    (gd, gf), (ed, ef) = got, exp
    assert gd.is_cuda and gd.dtype == torch.float32 and gf.dtype == torch.int32 and tuple(gd.shape) == ed.shape
    assert np.array_equal(bits(gd), bits(ed)), '%d of %d distances differ' % ((bits(gd) != bits(ed)).sum(), ed.size)
    assert np.array_equal(gf.cpu().numpy(), ef), '%d of %d faces differ' % ((gf.cpu().numpy() != ef).sum(), ef.size)


def fp_bar(*arrays):
    return 16.0 * 2.0 ** -24 * max(float(np.abs(a[np.isfinite(a)]).max()) for a in arrays)


def counted(index, pts, **kw):
    c = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = index.distance(pts, counters=c, **kw)
    return out, [int(v) for v in c.cpu()]


@functools.lru_cache(None)
def soup_case():
    """render_ref.triangle_soup(3000), 5 000 points, a third of them half a metre to a metre outside the bounding box."""
    verts, faces = RR.triangle_soup(3000)
    lo, hi = M.grid_box(verts, faces)
    rng = np.random.default_rng(11)
    # outside: next to the five outermost vertices of each side of the box, pushed 0.5 to 1 m beyond that side, so that
    # the nearest face stays a few shells away (a point many metres from every face walks the whole grid: slow)
    used = verts[np.unique(faces)]
    axis, side = rng.integers(0, 3, 1667), rng.random(1667) < 0.5
    order = np.argsort(used, axis=0)
    pick = rng.integers(0, 5, 1667)
    anchor = used[np.where(side, order[-1 - pick, axis], order[pick, axis])]
    out = anchor + rng.uniform(-0.3, 0.3, (1667, 3))
    out[np.arange(1667), axis] = np.where(side, hi[axis] + rng.uniform(0.5, 1.0, 1667), lo[axis] - rng.uniform(0.5, 1.0, 1667))
    pts = np.concatenate([M.near_surface_points(verts, faces, 1700, 11), rng.uniform(-1.0, 5.0, (1633, 3)), out]).astype(F32)
    exp = M.distance_ref(pts, verts, faces, block=512)
    for x in (verts, faces, pts) + exp:
        x.setflags(write=False)
    return verts, faces, pts, exp


def test_soup_inside_and_outside_the_grid():
    verts, faces, pts, exp = soup_case()
    a, ab, ac, _ = M.pack_ref(verts, faces)
    median = float(np.median(np.concatenate([np.linalg.norm(x, axis=1) for x in (ab, ac, ac - ab)])))
    seen = []
    for cell in (None, 1000.0, 0.8 * median):
        index = meshdist.TriangleIndex(verts, faces, cell)
        got, (cells, pairs) = counted(index, pts)
        same(got, exp)
        same(index.distance(pts, sort=True), exp)
        seen.append((index.dims, cells, pairs))
    print('dims, cells, pairs per cell value:', seen)
    assert seen[1][0] == (1, 1, 1) and seen[1][1:] == (len(pts), len(pts) * len(faces))
    assert seen[2][0][0] > seen[0][0][0] > 1
    assert abs(float(meshdist.TriangleIndex(verts, faces).cell) / float(M.default_cell_ref(verts, faces)) - 1) < 1e-5
    # the order of the points and of the faces (remapped) changes no bit
    rng = np.random.default_rng(0)
    pp, fp = rng.permutation(len(pts)), rng.permutation(len(faces))
    index = meshdist.TriangleIndex(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda())
    d, f = index.distance(torch.from_numpy(pts[pp]).cuda())
    same((d, f), (exp[0][pp], exp[1][pp]))
    d, f = meshdist.TriangleIndex(verts, faces[fp]).distance(pts)
    assert np.array_equal(bits(d), bits(exp[0]))
    orig = fp[f.cpu().numpy()]
    ties = orig != exp[1]                                         # another face at exactly the same distance
    assert np.array_equal(bits(np.sqrt(M.tri_dist2(pts[ties], a[orig[ties]], ab[orig[ties]], ac[orig[ties]]))),
                          bits(exp[0][ties]))
    assert (f.cpu().numpy()[ties] < np.argsort(fp)[exp[1][ties]]).all()      # and it wins by its lower new index


@pytest.mark.parametrize('n,cell', [(1, 0.1), (1, None), (6, None), (6, 0.07)])
def test_large_triangles_and_ties(n, cell):
    verts, faces = RR.tessellate_room(n)
    v = verts.astype(np.float64)
    mid = ((v[faces] + v[faces[:, [1, 2, 0]]]) / 2).reshape(-1, 3)        # on edges that two faces share
    pts = np.concatenate([M.near_surface_points(verts, faces, 1500, n, off=0.0), verts, mid,
                          M.near_surface_points(verts, faces, 500, n + 1, off=0.02)]).astype(F32)
    exp = M.distance_ref(pts, verts, faces)
    assert (exp[0] == 0).sum() > len(verts)
    index = meshdist.TriangleIndex(verts, faces, cell)
    if cell == 0.1:
        assert index.n_refs > 100 * len(faces)                   # every face spans hundreds of cells
    same(index.distance(pts), exp)
    twice = np.concatenate([faces, faces])
    got = meshdist.TriangleIndex(verts, twice, cell).distance(pts)
    same(got, exp)                                               # the lowest index wins: never the second copy
    same(meshdist.TriangleIndex(verts, twice[::-1].copy(), cell).distance(pts),
         (exp[0], M.distance_ref(pts, verts, twice[::-1])[1]))


WAVE_CELLS = 256            # csrc/box_lists.h: a face whose box touches more cells is listed by its whole wave


def lists_equal(verts, faces, cell):
    """The index's CSR lists against meshdist_ref.GridRef: offsets entry by entry, every cell's faces as sorted sets
    (the order inside a cell is the atomics').  Returns the number of cells each face is listed in."""
    index = meshdist.TriangleIndex(verts, faces, cell)
    grid = M.GridRef(verts, faces, index.cell)
    assert index.dims == grid.dims and index.n_refs == grid.offsets[-1] == len(grid.refs)
    assert index.offsets.dtype == torch.int32 and index.refs.dtype == torch.int32
    offsets, refs = index.offsets.cpu().numpy(), index.refs.cpu().numpy()[:index.n_refs]
    assert np.array_equal(offsets, grid.offsets)
    cells = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    assert np.array_equal(refs[np.lexsort((refs, cells))], grid.refs)
    return np.bincount(grid.refs, minlength=len(faces))


def test_the_cell_lists_of_faces_listed_by_their_wave():
    """The room at cell = 0.1: its twelve wall triangles span a thousand cells each (the smallest wall is 3.2 x 2.6 m),
    the faces of its furniture tens to hundreds; one face with a NaN vertex sits among them and is in no list."""
    verts, faces = RR.tessellate_room(1)
    verts = np.concatenate([verts, [[np.nan, 0.5, 0.5]]]).astype(F32)
    faces = np.concatenate([faces[:5], [[len(verts) - 1, 0, 1]], faces[5:]]).astype(np.int32)
    per_face = lists_equal(verts, faces, 0.1)
    assert per_face[5] == 0 and (np.delete(per_face, 5) >= 1).all()
    assert (per_face[:13] > 3 * WAVE_CELLS).sum() == 12 and per_face.sum() > 100 * len(faces)


def test_the_cell_lists_of_big_and_small_faces_in_one_wave():
    verts, faces = RR.triangle_soup(300)
    per_face = lists_equal(verts, faces, None)
    big = per_face > WAVE_CELLS
    assert per_face.min() >= 1 and 10 <= big.sum() <= len(faces) // 2
    waves = np.arange(len(faces)) // 64
    assert any(big[waves == w].any() and not big[waves == w].all() for w in np.unique(waves))


def test_ignored_faces_and_bad_points():
    verts, faces, pts, exp = soup_case()
    verts, faces, pts = verts.copy(), faces[:1200].copy(), pts[:2000].copy()
    exp = M.distance_ref(pts, verts, faces)
    rng = np.random.default_rng(2)
    nv = len(verts)
    verts2 = np.concatenate([verts, [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(F32)
    two = faces[rng.integers(0, 1200, 40)].copy()
    two[:, 2] = two[:, 0]                                         # two equal vertices
    three = np.repeat(rng.integers(0, nv, 40)[:, None], 3, 1)     # three equal vertices
    nan = faces[rng.integers(0, 1200, 40)].copy()
    nan[:, 1] = nv + rng.integers(0, 2, 40)                       # a non-finite vertex
    mixed = np.concatenate([faces, two, three, nan]).astype(np.int32)
    where = rng.permutation(len(mixed))
    back = np.full(len(mixed), -1)
    back[np.argsort(where)[:1200]] = np.arange(1200)              # position in `mixed[where]` -> face of the soup
    index = meshdist.TriangleIndex(verts2, mixed[where])
    assert index.packed.n_usable == 1200
    pts[3], pts[4, 2], pts[5, 0] = np.nan, np.inf, -np.inf
    d, f = index.distance(pts)
    e_d, e_f = M.distance_ref(pts, verts2, mixed[where])
    same((d, f), (e_d, e_f))
    assert np.isinf(e_d[[3, 4, 5]]).all() and (e_f[[3, 4, 5]] == -1).all()
    ok = np.ones(len(pts), bool)
    ok[[3, 4, 5]] = False
    assert np.array_equal(bits(d)[ok], bits(exp[0])[ok])
    mapped = back[f.cpu().numpy()[ok]]
    assert (mapped >= 0).all()
    ties = mapped != exp[1][ok]
    a, ab, ac, _ = M.pack_ref(verts, faces)
    assert np.array_equal(bits(np.sqrt(M.tri_dist2(pts[ok][ties], a[mapped[ties]], ab[mapped[ties]], ac[mapped[ties]]))),
                          bits(exp[0][ok][ties]))
    bad = faces.copy()
    bad[17, 2] = nv
    with pytest.raises(ValueError, match='face index'):
        meshdist.TriangleIndex(verts, torch.from_numpy(bad).cuda())
    with pytest.raises(ValueError, match='face index'):
        meshdist.TriangleIndex(verts, bad)
    with pytest.raises(ValueError, match='face index'):
        meshdist.sample_surface(torch.from_numpy(verts).cuda(), torch.from_numpy(-bad).cuda(), 10)
    with pytest.raises(ValueError, match='usable'):
        meshdist.TriangleIndex(verts2, np.concatenate([two, three, nan]).astype(np.int32))
    with pytest.raises(ValueError):
        meshdist.TriangleIndex(verts, faces[:0])
    with pytest.raises(ValueError):
        meshdist.TriangleIndex(verts[:, :2], faces)
    with pytest.raises(ValueError):
        meshdist.TriangleIndex(verts, faces.reshape(-1, 6))
    with pytest.raises(ValueError, match='larger cell'):
        meshdist.TriangleIndex(verts, faces, cell=1e-4)
    with pytest.raises(ValueError):
        index.distance(pts[:, :2])
    d, f = index.distance(pts[:0])
    assert d.shape == (0,) and f.shape == (0,) and f.dtype == torch.int32
    p0, f0 = meshdist.sample_surface(verts, faces, 0)
    assert p0.shape == (0, 3) and f0.shape == (0,)


def test_max_dist():
    verts, faces, pts, exp = soup_case()
    index = meshdist.TriangleIndex(verts, faces)
    _, (_, full) = counted(index, pts)
    for md in (0.0, 0.05, 1.5):
        e_d, e_f = exp[0].copy(), exp[1].copy()
        far = ~(e_d <= F32(md))
        e_d[far], e_f[far] = np.inf, -1
        got, (_, pairs) = counted(index, pts, max_dist=md)
        same(got, (e_d, e_f))
        assert pairs < full and far.any()


def test_pruning():
    """A condition, not a measurement: the counter of evaluated pairs stays at or below P T / 10 (the rule itself
    needs under P T / 20, tests/test_meshdist_ref.py)."""
    verts, faces, pts = M.pruning_case()
    index = meshdist.TriangleIndex(verts, faces)
    grid = M.GridRef(verts, faces, index.cell)
    assert grid.dims == index.dims and index.n_refs == len(grid.refs)
    exp = M.walk_ref(pts, grid)
    for sort in (False, True):
        got, (cells, pairs) = counted(index, pts, sort=sort)
        same(got, exp[:2])
        print('pairs %d = P T / %.1f, cells %d (restatement: %d, %d)' % (
            pairs, len(pts) * len(faces) / pairs, cells, exp[2], exp[3]))
        assert pairs <= len(pts) * len(faces) // 10
        assert (pairs, cells) == (exp[2], exp[3])                 # one lane per point: exactly the rule's walk


@functools.lru_cache(None)
def sampled():
    verts, faces = M.clipped_soup(2000, seed=8, big=0.1)
    faces = faces.copy()
    faces[5, 1] = faces[5, 0]
    faces[1999, 2] = faces[1999, 1]                               # the last face is ignored: the clamp target moves
    n = 50001
    pts, fid, cum = meshdist.sample_surface(verts, faces, n, seed=3, return_table=True)
    return verts, faces, n, pts, fid, cum.cpu().numpy()


def test_sample_surface():
    verts, faces, n, pts, fid, cum = sampled()
    area, ref_cum = M.areas_ref(verts, faces)
    assert np.abs(cum - ref_cum).max() <= 1e-12 * ref_cum[-1]
    e_pts, e_fid = M.sample_ref(verts, faces, n, 3, cum)
    assert pts.is_cuda and np.array_equal(bits(pts), bits(e_pts)) and np.array_equal(fid.cpu().numpy(), e_fid)
    counts = np.bincount(e_fid, minlength=len(faces))
    assert counts[5] == 0 and counts[1999] == 0 and np.abs(counts - n * area / cum[-1]).max() <= 1.0
    again = meshdist.sample_surface(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), n, seed=3)
    assert torch.equal(again[0], pts) and torch.equal(again[1], fid)
    assert (meshdist.sample_surface(verts, faces, n, seed=4)[0] != pts).any(1).float().mean().item() > 0.99
    d, f = meshdist.TriangleIndex(verts, faces).distance(pts)
    d, f = d.cpu().numpy(), f.cpu().numpy()
    other = f != e_fid                                            # then the sample's own face is exactly as near
    a, ab, ac, _ = M.pack_ref(verts, faces)
    own = np.sqrt(M.tri_dist2(e_pts[other], a[e_fid[other]], ab[e_fid[other]], ac[e_fid[other]]))
    print('%d of %d samples have another nearest face than their own' % (other.sum(), n))
    assert np.array_equal(bits(own), bits(d[other]))


def test_samples_lie_on_the_mesh_within_the_bar():
    """index.distance(samples) <= 16 * 2^-24 * max |coordinate| (4.77e-6 here), thin triangles included: the
    refinement step of rule 2 keeps the in-plane error of the interior case out of the distance."""
    verts, faces, n, pts, fid, cum = sampled()
    d = meshdist.TriangleIndex(verts, faces).distance(pts)[0].cpu().numpy()
    bar = fp_bar(verts)
    print('largest distance of a sample from the mesh %.3g, bar %.3g' % (d.max(), bar))
    assert d.max() <= bar


def test_sample_surface_counts_within_one():
    """The per-face counts of the device's samples are within +-1 of n area / A."""
    verts, faces, n, pts, fid, cum = sampled()
    area = M.areas_ref(verts, faces)[0]
    dev = np.abs(np.bincount(fid.cpu().numpy(), minlength=len(faces)) - n * area / cum[-1])
    print('largest |count - n area / A| = %.3f, %d faces above 1' % (dev.max(), (dev > 1).sum()))
    assert dev.max() <= 1.0


def test_compare():
    room = RR.tessellate_room(6)
    verts, faces = RR.tessellate_room(4)
    moved = (verts + np.array([0.06, 0.0, 0.0], F32), faces)
    rep = meshdist.compare(pred=moved, target=room, n=20000, thresholds=(0.02, 0.05), seed=1, max_dist=0.04)
    ref = M.compare_ref(rep['pred_to_target'].cpu().numpy(), rep['target_to_pred'].cpu().numpy(), (0.02, 0.05), 0.04)
    for key in ('accuracy', 'completeness', 'chamfer'):
        assert abs(rep[key] - ref[key]) <= 1e-12 * abs(ref[key]), key
    for key in ('hits_pred', 'hits_target', 'precision', 'recall'):
        assert rep[key] == ref[key], key
    assert np.allclose(rep['fscore'], ref['fscore'], rtol=1e-12, atol=0)
    assert 0 < rep['hits_pred'][0] <= rep['hits_pred'][1] < 20000 and torch.isinf(rep['pred_to_target']).any()
    pts = meshdist.sample_surface(*moved, 20000, seed=1)[0]
    same(meshdist.TriangleIndex(*room).distance(pts, max_dist=0.04),
         M.distance_ref(pts.cpu().numpy(), *room, max_dist=0.04))
    itself = meshdist.compare(pred=room, target=room, n=20000)
    bar = fp_bar(room[0])
    assert itself['fscore'] == [1.0] and itself['accuracy'] <= bar and itself['completeness'] <= bar
    assert float(itself['pred_to_target'].max()) <= bar


def test_end_to_end_room():
    """Room mesh -> rendered frames -> fusion -> marching cubes -> compare with the room mesh.  Every pred -> target
    distance is at most (3 + depth_max) voxel_size, the fusion's largest truncation band, plus one voxel diagonal."""
    vs, depth_max = 0.05, 4.0
    room = RR.tessellate_room(8)
    _, k, poses = R.room_frames(30, (120, 160), seed=7)
    depth = render.render_depth(*room, k, poses, (120, 160), depth_max=depth_max)
    w2g = R.grid_transform((-0.3, -0.3, -0.3), vs)
    vol = fusion.TSDFVolume((92, 76, 64), vs, w2g).integrate(depth, k, poses)
    verts_vox, _, faces = mc.run_marching_cubes(vol.sdf() / vs, None, 0.0, 3.0, 10.0)
    assert verts_vox.is_cuda and len(faces) > 5000
    g2w = torch.from_numpy(np.linalg.inv(w2g.astype(np.float64))).to(verts_vox.device)
    verts = (verts_vox.double() @ g2w[:3, :3].T + g2w[:3, 3]).float()
    rep = meshdist.compare(pred=(verts, faces), target=room, n=100000, thresholds=(0.05,))
    print('accuracy %.4f completeness %.4f chamfer %.4f precision %.4f recall %.4f fscore %.4f, largest pred -> target %.4f'
          % (rep['accuracy'], rep['completeness'], rep['chamfer'], rep['precision'][0], rep['recall'][0],
             rep['fscore'][0], float(rep['pred_to_target'].max())))
    assert float(rep['pred_to_target'].max()) <= (3 + depth_max) * vs + np.sqrt(3.0) * vs
    assert torch.isfinite(rep['target_to_pred']).all()
