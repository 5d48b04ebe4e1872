"""Seeded random inputs that the reference's own code was run on (tests/golden/make_golden_live.py) and that the tests
rebuild to compare against its stored outputs (tests/golden/live_reference.npz).  Shared by both so that the inputs of a
test and of its fixture are one definition."""
import hashlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIVE = os.path.join(HERE, 'golden', 'live_reference.npz')


def load():
    return np.load(LIVE, allow_pickle=False)


def digest(*arrays):
    """sha256 over the shapes, dtypes and bytes of the arrays (fixtures of outputs too large to store whole)."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def file_digest(path):
    return hashlib.sha256(open(path, 'rb').read()).hexdigest()


def data_files(tmp, seed):
    """test_oracle_data: one chunk file and one scene triple (input / target / known) written by this build's writer."""
    from sgnn_amd import synth
    rng = np.random.default_rng(seed)
    dims = tuple(int(8 * v) for v in rng.integers(1, 4, 3))
    vs = float(rng.choice([0.02, 0.046875, 0.1]))
    chunk = os.path.join(tmp, 'c.sdfs')
    synth.write_chunk(chunk, dims, 40 + seed, occupancy=float(rng.uniform(0.05, 0.4)), voxelsize=vs)
    s_in, s_tgt = os.path.join(tmp, 'a.sdf'), os.path.join(tmp, 'b.sdf')
    synth.write_scene_triple(s_in, s_tgt, (int(rng.integers(9, 30)), int(rng.integers(9, 30)), int(rng.integers(9, 30))),
                             60 + seed, occupancy=0.3, voxelsize=vs)
    return chunk, s_tgt, s_tgt[:-4] + '.knw'


def train_fields(out):
    """load_train_file's result as named arrays: ((locs, vals), target, dims, world2grid, known, hierarchy[3])."""
    (locs, vals), tgt, dims, w2g, known, hier = out
    f = {'locs': locs, 'vals': vals, 'tgt': tgt, 'dims': np.asarray(list(dims), dtype=np.int64), 'w2g': w2g,
         'known': known}
    for h in range(3):
        f['hier%d' % h] = hier[h]
    return f


def scene_fields(scene, known):
    """load_scene's result ((locs, vals), dims, ...) and load_scene_known's volume as named arrays."""
    return {'locs': scene[0][0], 'vals': scene[0][1], 'dims': np.asarray(list(scene[1]), dtype=np.int64), 'known': known}


def metrics_inputs(seed):
    """test_oracle_metrics: random target occupancy / sdf / known volumes and sparse predictions (numpy)."""
    rng = np.random.default_rng(seed)
    nb, d = 2, int(rng.choice([8, 12]))
    occ = rng.choice([-1, 0, 1], size=(nb, 1, d, d, d), p=[0.15, 0.6, 0.25]).astype(np.int8)
    pred = []
    for b in range(nb):
        cells = rng.permutation(d ** 3)[:int(rng.integers(5, d ** 3 // 2))]
        cells.sort()
        pred.append(np.stack([cells // (d * d), (cells // d) % d, cells % d], 1).astype(np.int64))
    sdf = rng.normal(0, 2.5, (nb, 1, d, d, d)).astype(np.float32).clip(-3, 3)
    known = rng.integers(0, 4, (nb, 1, d, d, d)).astype(np.uint8)
    locs = np.concatenate([np.concatenate([p, np.full((len(p), 1), b)], 1) for b, p in enumerate(pred)])
    vals = rng.normal(0, 2, (len(locs), 1)).astype(np.float32)
    return occ, pred, sdf, known, locs, vals


L1_CASES = [(masking, thresh) for masking in (True, False) for thresh in (None, 1.0)]


def mc_volume(seed):
    """test_oracle_mc: a small noisy, partially invalid sphere volume with random iso / truncation / threshold."""
    rng = np.random.default_rng(100 + seed)
    dims = tuple(int(v) for v in rng.integers(7, 13, 3))
    zz, yy, xx = np.meshgrid(*[np.arange(d) for d in dims], indexing='ij')
    c = rng.uniform(0.3, 0.7, 3) * np.array(dims)
    sdf = np.sqrt((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) - rng.uniform(2.0, 4.0)
    sdf = sdf + rng.normal(0, rng.choice([0.0, 0.2, 0.8]), dims)
    if seed % 2:
        sdf = np.round(sdf * 4) / 4                                       # exact iso hits and ties
    vol = np.where(rng.random(dims) < 0.9, sdf, -np.inf).astype(np.float32)   # holes
    iso = float(rng.choice([0.0, 0.25, 1.0]))
    trunc = float(rng.choice([3.0, 2.5, 50.0]))
    thresh = float(rng.choice([10.0, 1.2]))
    colors = rng.integers(0, 256, dims + (3,), dtype=np.uint8)
    return vol, colors, iso, trunc, thresh


def mc_scene_volumes():
    """test_gpu_marching_cubes: two (96,160,192) surface volumes (~1e5 triangles) and the colour volume the reference
    is called with."""
    from mc_cases import make_volume
    spec = dict(dims=(96, 160, 192), seed=11, occ=0.12, iso=0.0, trunc=3.0, thresh=10.0, kind='block')
    out = []
    for s in (spec, dict(spec, kind='quantised', seed=12)):
        tsdf, _ = make_volume(s)
        out.append(tsdf)
    col = torch.ones(tuple(out[0].shape) + (3,), dtype=torch.uint8) * 220
    return out, col
