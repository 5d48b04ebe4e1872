"""Seeded TSDF volumes for the marching-cubes tests (shared by tests/golden/make_golden_mc.py and the tests)."""
import numpy as np
import torch

from sgnn_amd import synth

CASES = {
    # name: dims (z,y,x), seed, occupancy, iso, trunc, thresh, flavour
    'sphere32': dict(dims=(32, 32, 32), seed=3, occ=0.08, iso=0.0, trunc=3.0, thresh=10.0, kind='block'),
    'rect': dict(dims=(24, 40, 56), seed=4, occ=0.10, iso=0.0, trunc=3.0, thresh=10.0, kind='block'),
    'iso1': dict(dims=(32, 32, 32), seed=5, occ=0.08, iso=1.0, trunc=3.0, thresh=10.0, kind='block'),   # --vis_dfs path
    'jumps': dict(dims=(32, 32, 32), seed=6, occ=0.08, iso=0.0, trunc=3.0, thresh=1.1, kind='noisy'),   # threshold rejections
    'snap': dict(dims=(24, 24, 24), seed=7, occ=0.10, iso=0.0, trunc=3.0, thresh=10.0, kind='quantised'),  # exact hits, near-coincident vertices
    'colors': dict(dims=(24, 24, 24), seed=8, occ=0.10, iso=0.0, trunc=3.0, thresh=10.0, kind='block', colors=True),
    'dense': dict(dims=(20, 20, 20), seed=9, occ=0.3, iso=0.0, trunc=100.0, thresh=200.0, kind='full'),   # every voxel valid, border cubes
    'empty': dict(dims=(16, 16, 16), seed=1, occ=0.05, iso=0.0, trunc=3.0, thresh=10.0, kind='empty'),
    'block64': dict(dims=(64, 64, 64), seed=5, occ=0.05, iso=0.0, trunc=3.0, thresh=10.0, kind='block'),
}


def make_volume(spec):
    """-> (tsdf (z,y,x) float32 CPU tensor with -inf where nothing is stored, colors (z,y,x,3) uint8 or None)."""
    dims, rng = spec['dims'], np.random.default_rng(1000 + spec['seed'])
    sdf = synth._block_sdf(dims, np.random.default_rng(spec['seed']), spec['occ']).astype(np.float32)
    kind = spec['kind']
    if kind == 'full':
        vol = sdf
    elif kind == 'empty':
        vol = np.full(dims, -np.inf, dtype=np.float32)
    else:
        if kind == 'noisy':
            sdf = sdf + rng.normal(0, 0.6, dims).astype(np.float32)
        if kind == 'quantised':
            sdf = np.round(sdf * 2) / 2          # many corner averages land exactly on the iso value or within 1e-5
            sdf = sdf + (rng.random(dims) < 0.05) * np.float32(4e-6)
        vol = np.where(np.abs(sdf) < 4.0, sdf, -np.inf).astype(np.float32)   # band wider than the truncation
    colors = None
    if spec.get('colors'):
        colors = torch.from_numpy(rng.integers(0, 256, dims + (3,), dtype=np.uint8))
    return torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)), colors


# ---------------------------------------------------------------------------------------------------------------------
# Stage cases: hand-built volumes for tests/test_gpu_mc_stages.py and the second half of tests/test_oracle_mc.py.  The
# reference extension's meshes of those marked stored=True are in tests/golden/mc_stage_expected.npz
# (tests/golden/make_golden_mc_stages.py).  CASES above is left alone: its fixture is mc_expected.npz.
# ---------------------------------------------------------------------------------------------------------------------
F32 = np.float32
# x,y,z side of the cube corner behind cube-index bit b (marching_cubes.cpp: dist010 -> 1, dist110 -> 2, dist100 -> 4,
# dist000 -> 8, dist011 -> 16, dist111 -> 32, dist101 -> 64, dist001 -> 128)
BIT_CORNER = [(0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1), (0, 0, 1)]
# the reference's distArray order 000,100,010,001,110,011,101,111, which is also trilerp's accumulation order
DIST_ORDER = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
# cube edge -> its two corners as x,y,z sides, in the order of the reference's twelve vertexInterp calls
EDGE_CORNERS = [((0, 1, 0), (1, 1, 0)), ((1, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 1, 0)),
                ((0, 1, 1), (1, 1, 1)), ((1, 1, 1), (1, 0, 1)), ((1, 0, 1), (0, 0, 1)), ((0, 0, 1), (0, 1, 1)),
                ((0, 1, 0), (0, 1, 1)), ((1, 1, 0), (1, 1, 1)), ((1, 0, 0), (1, 0, 1)), ((0, 0, 0), (0, 0, 1))]
NO_SURFACE = (0, 85, 170, 255)      # configurations that emit nothing: 85 and 170 by the reference's edgeTable == 255 rule

STAGE_CASES = {
    # every cube configuration: one 3x3x3 neighbourhood per configuration k = 16 row + col, `pitch` voxels apart
    'allcfg': dict(kind='allcfg', pitch=4, iso=0.0, trunc=3.0, thresh=10.0, stored=True),
    'allcfg_colors': dict(kind='allcfg', pitch=3, iso=0.0, trunc=3.0, thresh=10.0, colors=True, seed=21, stored=True),
    # the same with the iso value off zero and the background of neighbourhood k cycling through 0.25, the iso value
    # itself and 4e-6 above it: vertexInterp divides in the first, snaps to an end point in the other two
    'allcfg_iso': dict(kind='allcfg', pitch=3, iso=0.125, trunc=3.0, thresh=10.0, backgrounds=True, stored=True),
    # 2470 blocks of 256 voxels with a tail of 36: three rounds of the block-sum scan, surface in every one of them
    'carry': dict(kind='bands', dims=(7, 300, 301), seed=22, iso=0.0, trunc=3.0, thresh=10.0, stored=True),
    # NaN, +inf, -inf and voxels exactly at +-trunc inside a noisy, otherwise fully valid volume
    'nonfinite': dict(kind='nonfinite', dims=(8, 10, 12), seed=23, iso=0.0, trunc=1.5, thresh=10.0, stored=True),
    # odd extents, iso off zero, a jump threshold that rejects part of the cubes
    'params': dict(kind='noise', dims=(7, 9, 11), seed=24, iso=0.1, trunc=3.0, thresh=0.5, colors=True, stored=True),
}
# no voxel has all 26 neighbours: an extent of 1 or 2 on each axis in turn, and volumes smaller than one block
NO_INTERIOR_DIMS = [(1, 1, 1), (2, 2, 2), (1, 9, 10), (9, 1, 10), (9, 10, 1), (2, 9, 10), (9, 2, 10), (9, 10, 2)]


def _allcfg_volume(pitch, iso, backgrounds):
    side = 16 * pitch + 1
    vol = np.full((5, side, side), 0.25, dtype=F32)
    for k in range(256):
        z, y, x = 2, 2 + pitch * (k // 16), 2 + pitch * (k % 16)
        if backgrounds:
            vol[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = (F32(0.25), F32(iso), F32(iso) + F32(4e-6))[k % 3]
        for bit, (sx, sy, sz) in enumerate(BIT_CORNER):
            if k >> bit & 1:
                vol[z + 2 * sz - 1, y + 2 * sy - 1, x + 2 * sx - 1] = -2.0 - 0.125 * ((7 * k + bit) % 5)
    return vol


def make_stage_volume(spec):
    """-> (tsdf (z,y,x) float32 CPU tensor, colors (z,y,x,3) uint8 CPU tensor or None) of a STAGE_CASES entry."""
    kind, rng = spec['kind'], np.random.default_rng(2000 + spec.get('seed', 0))
    if kind == 'allcfg':
        vol = _allcfg_volume(spec['pitch'], spec['iso'], spec.get('backgrounds', False))
    elif kind == 'bands':        # three bands of rows, 40 voxels long, on every z; everything else was never observed
        dims = spec['dims']
        vol = np.full(dims, -np.inf, dtype=F32)
        for y in (10, 150, 285):
            vol[:, y:y + 5, 100:140] = rng.normal(0, 0.5, (dims[0], 5, 40)).astype(F32)
    else:
        vol = rng.normal(0, 0.5, spec['dims']).astype(F32)
        if kind == 'nonfinite':
            trunc = F32(spec['trunc'])
            special = [np.nan, np.inf, -np.inf, trunc, -trunc, np.nextafter(trunc, F32(0)), -np.nextafter(trunc, F32(0))]
            where = rng.permutation(vol.size)[:4 * len(special)]
            vol.reshape(-1)[where] = np.tile(np.array(special, dtype=F32), 4)
    colors = None
    if spec.get('colors'):
        colors = torch.from_numpy(rng.integers(0, 256, vol.shape + (3,), dtype=np.uint8))
    return torch.from_numpy(np.ascontiguousarray(vol, dtype=F32)), colors


def cube_table(tsdf, iso, trunc, thresh):
    """Host classification of every voxel, vectorised: (ci (z,y,x) int16 = the cube configuration, or -1 where the
    reference returns before its table look-up: border, an invalid voxel among the 27, or a jump/size threshold;
    dist (8,z,y,x) float32 corner values in DIST_ORDER, meaningful where ci >= 0).  float32 throughout, in the
    reference's order of operations."""
    t = np.asarray(tsdf, dtype=F32)
    iso, trunc, thresh = F32(iso), F32(trunc), F32(thresh)
    d0, d1, d2 = t.shape
    ci = np.full(t.shape, -1, dtype=np.int16)
    dist = np.zeros((8,) + t.shape, dtype=F32)
    if min(t.shape) < 3:
        return ci, dist

    def win(a, oz, oy, ox):      # a[z-1+oz, y-1+oy, x-1+ox] over the interior voxels
        return a[oz:d0 - 2 + oz, oy:d1 - 2 + oy, ox:d2 - 2 + ox]

    with np.errstate(invalid='ignore', over='ignore'):
        valid = (t != -np.inf) & (np.abs(t) < trunc)
        ok = np.ones((d0 - 2, d1 - 2, d2 - 2), dtype=bool)
        for oz in range(3):
            for oy in range(3):
                for ox in range(3):
                    ok &= win(valid, oz, oy, ox)
        d = []
        for sx, sy, sz in DIST_ORDER:
            acc = np.zeros(ok.shape, dtype=F32)
            for ox, oy, oz in DIST_ORDER:
                acc = acc + F32(0.125) * win(t, sz + oz, sy + oy, sx + ox)
            d.append(acc)
        index = np.zeros(ok.shape, dtype=np.int16)
        for bit, corner in enumerate(BIT_CORNER):
            index += (d[DIST_ORDER.index(corner)] < iso).astype(np.int16) << bit
        for a in d:
            for b in d:
                ok &= ~np.where(a * b < 0, np.abs(a) + np.abs(b) > thresh, np.abs(a - b) > thresh)
            ok &= ~(np.abs(a) > thresh)
    ci[1:-1, 1:-1, 1:-1] = np.where(ok, index, -1)
    dist[:, 1:-1, 1:-1, 1:-1] = np.stack(d)
    return ci, dist


def interp_branches(ci, dist, iso):
    """How often each exit of the reference's vertexInterp is taken over the crossed edges of the emitting cubes:
    [snap to p1 (|iso-d1| < 1e-5), snap to p2 (|iso-d2| < 1e-5), snap to p1 (|d1-d2| < 1e-5), division]."""
    iso, eps = F32(iso), F32(0.00001)
    emit = (ci >= 0) & ~np.isin(ci, NO_SURFACE)
    counts = np.zeros(4, dtype=np.int64)
    for a, b in EDGE_CORNERS:
        d1, d2 = dist[DIST_ORDER.index(a)][emit], dist[DIST_ORDER.index(b)][emit]
        crossed = (d1 < iso) != (d2 < iso)
        d1, d2 = d1[crossed], d2[crossed]
        b1 = np.abs(iso - d1) < eps
        b2 = ~b1 & (np.abs(iso - d2) < eps)
        b3 = ~b1 & ~b2 & (np.abs(d1 - d2) < eps)
        counts += [b1.sum(), b2.sum(), b3.sum(), (~b1 & ~b2 & ~b3).sum()]
    return counts


def scene_prediction():
    """Inputs of a test_scene.py:96-98 style save_predictions call: one scene's input sites [z,y,x,b] + tsdf values and
    a sparse sdf prediction (coordinates + values), numpy on the host as the reference passes them."""
    a = synth.block_arrays((40, 48, 56), 33, occupancy=0.12, stored_band=2.85, voxelsize=1.0)
    il, iv = a['input']
    tl, tv = a['target']
    rng = np.random.default_rng(77)
    keep = rng.random(len(tl)) < 0.93
    inputs = [np.concatenate([il, np.zeros((len(il), 1), np.int64)], 1), iv[:, None].astype(np.float32)]
    pred = [[np.concatenate([tl[keep], np.zeros((int(keep.sum()), 1), np.int64)], 1),
             (tv[keep] + rng.normal(0, 0.05, int(keep.sum()))).astype(np.float32)]]
    return ['scene0_'], inputs, pred
