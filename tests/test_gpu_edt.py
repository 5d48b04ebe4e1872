"""sgnn_amd.edt on the GPU against the brute-force host restatement tests/edt_ref.py: dist2
and nearest are integers and must be EQUAL, ties included; every case runs twice and the runs must be equal too."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_ref as ER  # noqa: E402

from sgnn_amd import edt, fusion, marching_cubes as mc, render  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(19, 37, 70),                              # ragged on every axis, crosses a 64-lane chunk in x
          (3, 5, 300), (300, 3, 5), (5, 300, 3),     # a long axis in each position
          (1, 1, 130), (1, 40, 1), (40, 1, 1),       # degenerate
          (16, 16, 64)]                              # exactly one chunk
DENSITIES = (0.3, 0.02, 0.001)
MAX_DISTS = (0, 1, 1.5, 2.5, 7, 1000)
IDS = ['x'.join(str(v) for v in s) for s in SHAPES]


def corners(shape):
    return [tuple((s - 1) * b for s, b in zip(shape, c)) for c in np.ndindex(2, 2, 2)]


@functools.lru_cache(maxsize=None)
def seeds_of(shape, kind):
    m = np.zeros(shape, dtype=np.uint8)
    if kind.startswith('random'):
        m = (np.random.default_rng(7).random(shape) < float(kind[6:])).astype(np.uint8)
    elif kind == 'lattice':
        m[::4, ::4, ::4] = 1
    elif kind == 'corners':
        for c in corners(shape):
            m[c] = 1
    elif kind.startswith('corner'):
        m[corners(shape)[int(kind[6:])]] = 1
    elif kind.startswith('plane'):
        axis = int(kind[5:])
        index = [slice(None)] * 3
        index[axis] = shape[axis] // 2
        m[tuple(index)] = 1
    elif kind == 'all':
        m[:] = 1
    else:
        assert kind == 'none'
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref_of(shape, kind):
    out = ER.brute(seeds_of(shape, kind))
    for a in out:
        a.setflags(write=False)
    return out


def run(seeds, max_dist=None):
    """feature_transform twice -> (dist2, nearest) as numpy."""
    a = edt.feature_transform(seeds, max_dist)
    b = edt.feature_transform(seeds, max_dist)
    shape = tuple(seeds.shape)
    for t in a:
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == shape
    assert torch.equal(a.dist2, b.dist2) and torch.equal(a.nearest, b.nearest), 'two runs differ'
    return a.dist2.cpu().numpy(), a.nearest.cpu().numpy()


def check(shape, kind):
    want = ref_of(shape, kind)
    got = run(seeds_of(shape, kind))
    assert np.array_equal(got[0], want[0]), '%d of %d dist2 differ' % ((got[0] != want[0]).sum(), want[0].size)
    assert np.array_equal(got[1], want[1]), '%d of %d nearest differ' % ((got[1] != want[1]).sum(), want[1].size)
    return got


@pytest.mark.parametrize('kind', ['random%s' % d for d in DENSITIES] + ['lattice'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_random_and_lattice(shape, kind):
    check(shape, kind)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_corners(shape):
    for k in range(8):
        check(shape, 'corner%d' % k)
    check(shape, 'corners')


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_planes(shape):
    for axis in range(3):
        d2, _ = check(shape, 'plane%d' % axis)
        far = np.abs(np.arange(shape[axis]) - shape[axis] // 2) ** 2
        assert np.array_equal(d2, np.broadcast_to(far.reshape([-1 if a == axis else 1 for a in range(3)]), shape))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_no_seeds_and_all_seeds(shape):
    d2, nr = check(shape, 'none')
    assert (d2 == -1).all() and (nr == -1).all()
    d2, nr = check(shape, 'all')
    assert (d2 == 0).all() and np.array_equal(nr.reshape(-1), np.arange(nr.size))


@pytest.mark.parametrize('kind', ['random%s' % d for d in DENSITIES] + ['lattice'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_max_dist(shape, kind):
    seeds = seeds_of(shape, kind)
    free = ref_of(shape, kind)
    for r in MAX_DISTS:
        want = ER.cap(*free, r)
        got = run(seeds, r)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
        near = (free[0] >= 0) & (free[0] <= int(np.floor(np.float64(r) * np.float64(r))))
        assert np.array_equal(got[0][near], free[0][near]) and np.array_equal(got[1][near], free[1][near]), r
        assert (got[0][~near] == -1).all() and (got[1][~near] == -1).all(), r


def test_inputs_may_live_anywhere():
    shape, kind = SHAPES[0], 'random0.02'
    m = seeds_of(shape, kind)
    want = ref_of(shape, kind)
    for seeds in (m, m.astype(bool), torch.from_numpy(m.copy()), torch.from_numpy(m.copy()).cuda(),
                  torch.from_numpy(m.astype(bool)).cuda(), torch.from_numpy(m.astype(np.float32) * -2.5).cuda(),
                  torch.from_numpy(np.repeat(m, 2, axis=2)).cuda()[:, :, ::2]):      # not contiguous
        ft = edt.feature_transform(seeds)
        assert isinstance(ft, edt.FeatureTransform)
        assert np.array_equal(ft.dist2.cpu().numpy(), want[0]) and np.array_equal(ft.nearest.cpu().numpy(), want[1])
    ft = edt.feature_transform(np.zeros((0, 4, 5), dtype=np.uint8))
    assert tuple(ft.dist2.shape) == (0, 4, 5) and tuple(ft.nearest.shape) == (0, 4, 5)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1], SHAPES[4]], ids=[IDS[0], IDS[1], IDS[4]])
def test_fill_colors(shape):
    rng = np.random.default_rng(11)
    colors = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    for kind, r in (('random0.02', None), ('random0.02', 2.5), ('random0.001', 7), ('lattice', 1), ('none', None)):
        valid = seeds_of(shape, kind)
        d2, nr = ER.cap(*ref_of(shape, kind), r)
        want = ER.fill_colors(colors, nr)
        a = edt.fill_colors(colors, valid, r)
        b = edt.fill_colors(torch.from_numpy(colors).cuda(), torch.from_numpy(valid.astype(bool)).cuda(), max_dist=r)
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == shape + (3,) and torch.equal(a, b)
        got = a.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got[valid != 0], colors[valid != 0])                   # seeds keep their own colour
        assert not got[nr < 0].any()
    ones = np.maximum(colors, 1)                                                     # no channel is 0: 0 = not filled
    got = edt.fill_colors(ones, seeds_of(shape, 'random0.001'), 7).cpu().numpy()
    _, nr = ER.cap(*ref_of(shape, 'random0.001'), 7)
    assert np.array_equal((got == 0).all(axis=-1), nr < 0) and np.array_equal((got != 0).all(axis=-1), nr >= 0)


@pytest.mark.parametrize('max_dist,voxel_size', [(None, 1.0), (7, 0.046875), (2.5, 0.02)])
def test_distance(max_dist, voxel_size):
    seeds = torch.from_numpy(seeds_of(SHAPES[0], 'random0.001').copy()).cuda()
    dist2 = edt.feature_transform(seeds, max_dist).dist2
    want = torch.sqrt(dist2.float()) * voxel_size
    want[dist2 < 0] = float('inf')
    got = edt.distance(seeds, max_dist, voxel_size)
    assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got, want)
    assert bool(torch.isinf(got).any()) == (max_dist is not None)
    assert torch.isinf(edt.distance(np.zeros((3, 4, 5), dtype=np.uint8))).all()


def test_distance_of_one_seed_is_the_norm_of_the_coordinates():
    """Independent of the module's own expression: one seed at the origin, so dist2 = z^2 + y^2 + x^2 by hand.  With
    voxel_size = 0.5 the product is exact in fp32, so only the square root rounds: where dist2 is a perfect square the
    distance is exact, and elsewhere a square root that is faithfully rounded is within one ulp (2^-23 relative) of
    NumPy's correctly rounded one."""
    shape, vs = SHAPES[0], 0.5
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing='ij')
    d2 = z * z + y * y + x * x
    want = np.sqrt(d2.astype(np.float32)) * np.float32(vs)
    got = edt.distance(seeds_of(shape, 'corner0'), voxel_size=vs).cpu().numpy()
    root = np.rint(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    square = root * root == d2
    assert int(square.sum()) > 100 and np.array_equal(got[square], (root[square] * vs).astype(np.float32))
    assert got[0, 3, 4] == np.float32(2.5) and got[12, 16, 21] == np.float32(14.5)      # 25 and 841, halved
    np.testing.assert_allclose(got, want, rtol=2.0 ** -23, atol=0.0)
    capped = edt.distance(seeds_of(shape, 'corner0'), max_dist=7, voxel_size=vs).cpu().numpy()
    assert np.array_equal(np.isinf(capped), d2 > 49) and np.array_equal(capped[d2 <= 49], got[d2 <= 49])


def test_a_half_coloured_sphere_is_meshed_in_colour():
    n, vs = 24, 0.05
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij')
    d = (np.sqrt((x - 11.5) ** 2 + (y - 11.5) ** 2 + (z - 11.5) ** 2) - 8.0) * vs       # metres, positive outside
    sdf = np.where(np.abs(d) <= 3 * vs, d, -np.inf).astype(np.float32)                  # never seen: -inf
    valid = np.broadcast_to(np.arange(n) < 12, (n, n, n)).copy()
    colors = np.random.default_rng(3).integers(1, 256, size=(n, n, n, 3), dtype=np.uint8)
    colors[~valid] = 0
    tsdf, raw = torch.from_numpy(sdf).cuda(), torch.from_numpy(colors).cuda()
    args = (0.0, 3 * vs, 10.0)
    v0, c0, f0 = mc.run_marching_cubes(tsdf, raw, *args)
    filled = edt.fill_colors(raw, torch.from_numpy(valid).cuda())
    v1, c1, f1 = mc.run_marching_cubes(tsdf, filled, *args)
    assert torch.equal(v0, v1) and torch.equal(f0, f1) and len(v0) > 1000
    black0, black1 = (c0 == 0).all(dim=1), (c1 == 0).all(dim=1)
    assert int(black0.sum()) > 100 and int(black1.sum()) == 0 and bool((c1 != 0).all())
    # a vertex lies within half a voxel of its cell, and the cell's corners within one voxel of that: at x <= 10 all
    # eight are valid
    seen = v0[:, 0] <= 10.0
    assert int(seen.sum()) > 100 and torch.equal(c0[seen], c1[seen]) and not bool(black0[seen].any())
    assert torch.equal(filled[torch.from_numpy(valid).cuda()], raw[torch.from_numpy(valid).cuda()])


@functools.lru_cache(maxsize=None)
def quad_volume():
    """A (dz, dy, dx) = (16, 20, 24) colour volume fused from two colour renderings of a coloured quad."""
    vs, dims_xyz = 0.05, (24, 20, 16)
    w2g = np.eye(4, dtype=np.float32)
    w2g[:3, :3] /= vs
    verts = np.array([[0.2, 0.2, 0.4], [0.7, 0.2, 0.4], [0.7, 0.8, 0.4], [0.2, 0.8, 0.4]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    vcol = np.array([[250, 20, 20], [20, 250, 20], [20, 20, 250], [250, 250, 20]], np.uint8)
    hw = (48, 64)
    k = np.tile(np.array([60.0, 60.0, 31.5, 23.5], np.float32), (2, 1))
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[0, :3, 3] = (0.6, 0.5, -0.4)
    poses[1, :3, 3] = (0.4, 0.5, -0.3)
    depth, rgba = render.render_color(verts, faces, vcol, k, poses, hw)
    vol = fusion.TSDFVolume(dims_xyz, vs, w2g, color=True)
    vol.integrate(depth, k, poses, color=rgba)
    return vol


@pytest.mark.parametrize('pd', [None, (19, 22, 29), (14, 20, 21), (18, 17, 24)],
                         ids=['same', 'padded', 'cropped', 'both'])
@pytest.mark.parametrize('max_dist', [None, 3.0])
def test_volume_colors(pd, max_dist):
    vol = quad_volume()
    wc = vol.color_weight()
    assert 50 < int((wc > 0).sum()) < wc.numel() // 2
    rgb = vol.colors(pd)
    valid = torch.zeros(tuple(rgb.shape[:3]), dtype=torch.bool, device=rgb.device)
    z, y, x = (min(a, b) for a, b in zip(valid.shape, wc.shape))
    valid[:z, :y, :x] = wc[:z, :y, :x] > 0
    want = edt.fill_colors(rgb, valid, max_dist)
    got = edt.volume_colors(vol, pd, max_dist)
    assert tuple(got.shape) == tuple(rgb.shape) and got.dtype == torch.uint8 and torch.equal(got, want)
    assert torch.equal(got[valid], rgb[valid])
    _, nr = ER.feature_transform(valid.cpu().numpy(), max_dist)
    assert np.array_equal(got.cpu().numpy(), ER.fill_colors(rgb.cpu().numpy(), nr))
    assert int((got != 0).any(dim=-1).sum()) > int((rgb != 0).any(dim=-1).sum())       # colour went somewhere new


def test_volume_colors_needs_a_colour_volume():
    plain = fusion.TSDFVolume((8, 8, 8), 0.05, np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError):
        edt.volume_colors(plain)
    with pytest.raises(ValueError):
        edt.volume_colors(quad_volume(), (4, 4, 1025))
