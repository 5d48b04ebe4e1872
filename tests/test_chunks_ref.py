"""CPU: the NumPy restatement of the training-chunk rules (tests/chunks_ref.py) against the .sdfs file contract
(written by sgnn_amd.data.write_train_file, read by the reference-pinned oracle/data_oracle.load_train_file), the
pyramid's level geometry, and the window scores against a brute-force count.  tests/test_gpu_chunks.py then holds
the device cutter to this restatement."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import chunks_ref as C  # noqa: E402
import data_oracle  # noqa: E402

F32 = np.float32
ORIGINS = [(0, 0, 0), (0, 16, 32), (16, 24, 32), (8, 16, 40), (16, 8, 16)]   # z, y, x; three overhang the volume


@pytest.fixture(scope='module')
def pair():
    return C.room_pair()


def dense_of(block, dims, vs):
    """What a reader makes of a block: values / voxel size scattered into -inf."""
    locs, vals = block
    out = np.full(dims, -np.inf, F32)
    out[locs[:, 0], locs[:, 1], locs[:, 2]] = vals / F32(vs)
    return out


@pytest.mark.parametrize('trunc_factor', [6.0, 4.0])
def test_crops_survive_the_file_contract(pair, tmp_path, trunc_factor):
    inp, tgt = pair
    vs, w2g = F32(C.VOXEL), inp.w2g
    sdfs = [g.sdf for g in tgt]
    known0 = tgt[0].known()
    overhang = zero_input = removed = 0
    for o in ORIGINS:
        c = C.cut(inp.sdf, sdfs, known0, vs, w2g, o, C.CROP, trunc_factor)
        path = C.write(str(tmp_path / (C.chunk_name('room', o) + '.sdfs')), c)
        (il, iv), target, dims, world2grid, known, hierarchy = data_oracle.load_train_file(path)
        assert dims == list(C.CROP)
        # the arrays the restatement started from, after the reader's division by the voxel size, bit for bit
        assert np.array_equal(il, c['input'][0]) and np.array_equal(iv.view(np.int32), (c['input'][1] / vs).view(np.int32))
        assert np.array_equal(target.view(np.int32), dense_of(c['target'], C.CROP, vs).view(np.int32))
        assert np.array_equal(known, c['known'])
        assert np.array_equal(world2grid, c['world2grid'])
        assert len(hierarchy) == 3
        for got, k in zip(hierarchy, (3, 2, 1)):                      # the reader returns [1/8, 1/4, 1/2]
            dims_k = tuple(d // 2 ** k for d in C.CROP)
            assert got.shape == dims_k
            assert np.array_equal(got.view(np.int32), dense_of(c['hierarchy'][k - 1], dims_k, vs).view(np.int32))
        # and against plain slicing of the volumes: inside the volume the crop is the volume
        z, y, x = o
        ez, ey, ex = (min(C.CROP[i], tgt[0].sdf.shape[i] - o[i]) for i in range(3))
        vol = tgt[0].sdf[z:z + ez, y:y + ey, x:x + ex]
        with np.errstate(all='ignore'):
            exp = np.where(np.abs(vol) <= F32(trunc_factor) * vs, vol / vs, F32(-np.inf)).astype(F32)
        assert np.array_equal(target[:ez, :ey, :ex], exp)
        removed += int((np.isfinite(vol) & ~np.isfinite(exp)).sum())
        if (ez, ey, ex) != C.CROP:
            overhang += 1
            pad = np.ones(C.CROP, bool)
            pad[:ez, :ey, :ex] = False
            assert (known[pad] == 255).all() and np.isinf(target[pad]).all()
            assert not ((il >= np.array([ez, ey, ex])).any(1)).any()
        zero_input += len(iv) == 0
    assert overhang >= 1 and zero_input >= 1
    assert (removed > 0) == (trunc_factor < 6.0)                      # the narrower band removes target voxels


def test_pyramid_geometry(pair):
    inp, tgt = pair
    w2g = np.asarray(inp.w2g, F32)
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.0, 5.0, size=(2000, 3))                      # world metres, in and around the grid
    g0 = pts @ w2g[:3, :3].astype(np.float64).T + w2g[:3, 3].astype(np.float64)
    for k in range(C.LEVELS):
        f = 2.0 ** k
        assert tgt[k].sdf.shape == tuple(-(-d // 2 ** k) for d in C.DIMS_XYZ[::-1])
        assert tgt[k].vs == F32(2 ** k) * F32(C.VOXEL)
        m = C.level_matrix(w2g, k)
        assert m.dtype == F32
        gk = pts @ m[:3, :3].astype(np.float64).T + m[:3, 3].astype(np.float64)
        # one fp32 rounding per matrix entry: relative error 2^-24 each, so |error| <= 2^-24 * (sum_j |m_ij| |p_j| +
        # |m_i3|) per coordinate, evaluated with the magnitudes at hand (points within 5 m, entries ~ 1 / (f * 0.07))
        bound = 2.0 ** -24 * (np.abs(pts) @ np.abs(m[:3, :3]).astype(np.float64).T + np.abs(m[:3, 3]).astype(np.float64))
        assert (np.abs(gk - (g0 - (f - 1.0) / 2.0) / f) <= bound).all()
        # the product's host half (no GPU needed) builds the same matrix
        from sgnn_amd import fusion
        assert np.array_equal((fusion.level_transform(k) @ w2g.astype(np.float64)).astype(F32), m)
    assert np.array_equal(C.level_matrix(w2g, 0), w2g)


def test_window_counts_equal_brute_force(pair):
    inp, tgt = pair
    origins, counts = C.window_table(tgt[0].sdf, inp.sdf, C.VOXEL, C.CROP, C.STRIDE)
    grid = C.window_grid(tgt[0].sdf.shape, C.CROP, C.STRIDE)
    assert grid == (2, 4, 3) and len(origins) == 24
    assert np.array_equal(origins, np.array([(z, y, x) for z in (0, 16) for y in (0, 8, 16, 24) for x in (0, 16, 32)]))
    for o, c in zip(origins, counts):
        assert tuple(c) == C.window_counts_brute(tgt[0].sdf, inp.sdf, C.VOXEL, o, C.CROP)
    assert (counts[:, 1] == 0).any() and (counts[:, 1] > 1000).any() and (counts[:, 0] > 0).all()
    # another truncation and band: the input count follows both filters
    o2, c2 = C.window_table(tgt[0].sdf, inp.sdf, C.VOXEL, C.CROP, C.STRIDE, truncation=1.5, trunc_factor=1.0)
    for o, c in zip(o2, c2):
        assert tuple(c) == C.window_counts_brute(tgt[0].sdf, inp.sdf, C.VOXEL, o, C.CROP, 1.5, 1.0)
    assert (c2 <= counts).all() and (c2[:, 1] < c2[:, 0]).any() and c2[:, 1].sum() > 0
