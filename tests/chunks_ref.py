"""Independent NumPy restatement of the training-chunk rules (INTEGRATION.md "Training chunks"): the pyramid's level
geometry, the window scores and the crops, cut with array slicing from host copies of the volumes.

Nothing here imports sgnn_amd.chunks or sgnn_amd.fusion.  Volumes come from the fp32 fusion restatement of
tests/fusion_ref.py; crops leave through the host-only writer sgnn_amd.data.write_train_file, so that the existing,
reference-pinned .sdfs readers and loaders are the yardstick for everything the device cutter produces.
"""
import os

import numpy as np

import fusion_ref as R

F32 = np.float32
LEVELS = 4


# ---------------------------------------------------------------------------------------------------------
# pyramid geometry
# ---------------------------------------------------------------------------------------------------------
def level_matrix(world2grid, k):
    """world2grid of level k: fine coordinate g0 -> (g0 - (f-1)/2) / f, f = 2**k; fp64 product of the fp32 matrix,
    rounded once to fp32."""
    f = 2.0 ** k
    w = np.asarray(world2grid, F32).astype(np.float64)
    out = w.copy()
    out[:3] = w[:3] / f
    out[:3, 3] -= (f - 1.0) / (2.0 * f)
    return out.astype(F32)


def level_dims(dims_xyz, k):
    return tuple((int(d) + 2 ** k - 1) // 2 ** k for d in dims_xyz)


def level_voxel_size(voxel_size, k):
    return F32(2 ** k) * F32(voxel_size)


def pyramid(dims_xyz, voxel_size, world2grid, levels=LEVELS):
    """fusion_ref.Grid per level (fp32 arithmetic)."""
    return [R.Grid(level_dims(dims_xyz, k), level_voxel_size(voxel_size, k), level_matrix(world2grid, k))
            for k in range(levels)]


# ---------------------------------------------------------------------------------------------------------
# window scores
# ---------------------------------------------------------------------------------------------------------
def flags(target_sdf, input_sdf, vs, truncation=3.0, trunc_factor=6.0):
    """(target voxels in the training band, input voxels a loader keeps), boolean (dz, dy, dx)."""
    vs = F32(vs)
    t, s = np.asarray(target_sdf, F32), np.asarray(input_sdf, F32)
    with np.errstate(all='ignore'):
        ft = np.abs(t / vs) < F32(truncation)
        fi = (np.abs(s) <= F32(trunc_factor) * vs) & (np.abs(s / vs) < F32(truncation))
    return ft, fi


def window_grid(dims_zyx, crop, stride):
    """Windows per axis: enough to cover the volume; the last may overhang."""
    return tuple(-(-max(d - c, 0) // s) + 1 for d, c, s in zip(dims_zyx, crop, stride))


def window_table(target_sdf, input_sdf, vs, crop, stride, truncation=3.0, trunc_factor=6.0):
    """(origins (W, 3) int64 z, y, x in raster order, counts (W, 2) int64) via 3-D prefix sums of the flags."""
    ft, fi = flags(target_sdf, input_sdf, vs, truncation, trunc_factor)
    grid = window_grid(ft.shape, crop, stride)
    ext = [(n - 1) * s + c for n, s, c in zip(grid, stride, crop)]
    origins, counts, sums = [], [], []
    for f in (ft, fi):
        p = np.zeros([e + 1 for e in ext], np.int64)
        p[1:f.shape[0] + 1, 1:f.shape[1] + 1, 1:f.shape[2] + 1] = f
        sums.append(p.cumsum(0).cumsum(1).cumsum(2))
    for wz in range(grid[0]):
        for wy in range(grid[1]):
            for wx in range(grid[2]):
                z0, y0, x0 = wz * stride[0], wy * stride[1], wx * stride[2]
                z1, y1, x1 = z0 + crop[0], y0 + crop[1], x0 + crop[2]
                origins.append((z0, y0, x0))
                counts.append([int(c[z1, y1, x1] - c[z0, y1, x1] - c[z1, y0, x1] - c[z1, y1, x0] + c[z0, y0, x1] +
                                   c[z0, y1, x0] + c[z1, y0, x0] - c[z0, y0, x0]) for c in sums])
    return np.array(origins, np.int64), np.array(counts, np.int64)


def window_counts_brute(target_sdf, input_sdf, vs, origin, crop, truncation=3.0, trunc_factor=6.0):
    ft, fi = flags(target_sdf, input_sdf, vs, truncation, trunc_factor)
    sl = tuple(slice(o, o + c) for o, c in zip(origin, crop))          # slicing stops at the volume's end
    return int(ft[sl].sum()), int(fi[sl].sum())


def candidates(table, min_target, min_input):
    origins, counts = table
    ok = (counts[:, 0] >= min_target) & (counts[:, 1] >= min_input)
    return origins[ok], counts[ok, 0], counts[ok, 1]


# ---------------------------------------------------------------------------------------------------------
# crops
# ---------------------------------------------------------------------------------------------------------
def _window(vol, origin, crop, fill):
    """vol[origin : origin + crop] padded with `fill` where the window leaves the volume."""
    out = np.full(crop, fill, vol.dtype)
    src = vol[tuple(slice(o, o + c) for o, c in zip(origin, crop))]
    out[:src.shape[0], :src.shape[1], :src.shape[2]] = src
    return out


def _block(vol, keep):
    z, y, x = np.nonzero(keep)                                          # raster order, x fastest
    return np.stack([z, y, x], 1).astype(np.int64), vol[z, y, x].astype(F32)


def cut(input_sdf, target_sdfs, known0, vs, world2grid, origin, crop, trunc_factor=6.0):
    """Everything one .sdfs file stores for the crop at `origin` (z, y, x): metric values.
    target_sdfs: the dense fp32 volumes of levels 0..3; known0: the level-0 known codes."""
    vs = F32(vs)
    origin = tuple(int(o) for o in origin)
    assert all(o % 8 == 0 for o in origin) and all(c % 32 == 0 for c in crop)
    inp = _window(np.asarray(input_sdf, F32), origin, crop, F32(-np.inf))
    tgt = _window(np.asarray(target_sdfs[0], F32), origin, crop, F32(-np.inf))
    keep0 = F32(trunc_factor) * vs
    hier = []
    for k in (1, 2, 3):
        f = 2 ** k
        win = _window(np.asarray(target_sdfs[k], F32), tuple(o // f for o in origin), tuple(c // f for c in crop),
                      F32(-np.inf))
        keep = F32(trunc_factor) * (F32(f) * vs)
        hier.append(_block((win / F32(f)).astype(F32), np.abs(win) <= keep))
    w2g = np.array(world2grid, F32)
    for r, o in zip(range(3), origin[::-1]):                          # rows x, y, z
        w2g[r, 3] = w2g[r, 3] - F32(o)
    return {'dims': tuple(crop), 'voxelsize': vs, 'world2grid': w2g, 'input': _block(inp, np.abs(inp) <= keep0),
            'target': _block(tgt, np.abs(tgt) <= keep0), 'known': _window(np.asarray(known0, np.uint8), origin, crop, 255),
            'hierarchy': hier}


def chunk_name(prefix, origin):
    return '%s_z%d_y%d_x%d' % ((prefix,) + tuple(int(o) for o in origin))


def write(path, c):
    from sgnn_amd import data
    data.write_train_file(path, c['dims'], c['voxelsize'], c['world2grid'], c['input'], c['target'], c['known'],
                          c['hierarchy'])
    return path


def write_all(out_dir, prefix, origins, *cut_args, **cut_kw):
    return [write(os.path.join(str(out_dir), chunk_name(prefix, o) + '.sdfs'), cut(*cut_args, origin=o, **cut_kw))
            for o in origins]


# ---------------------------------------------------------------------------------------------------------
# the fixture scene: the analytic room of fusion_ref, a subset of the frames as input, all of them as target
# ---------------------------------------------------------------------------------------------------------
DIMS_XYZ, VOXEL, ORIGIN = (64, 56, 40), 0.07, (-0.2, -0.3, -0.1)
CROP, STRIDE = (32, 32, 32), (16, 8, 16)                # z, y, x: the second z window overhangs (16 + 32 > 40)
N_FRAMES, N_INPUT = 20, 6


def room_scene():
    """(dims_xyz, voxel size, world2grid, depth (F, h, w), intrinsics, cam2world)."""
    depth, k, poses = R.room_frames(N_FRAMES, (48, 64), seed=3)
    rng = np.random.default_rng(5)
    depth = depth.copy()
    depth[rng.random(depth.shape) < 0.03] = -np.inf
    return DIMS_XYZ, VOXEL, R.grid_transform(ORIGIN, VOXEL), depth, k, poses


def room_pair():
    """(input Grid (first N_INPUT frames), target pyramid of Grids (all frames)) by the fp32 fusion restatement."""
    dims, vs, w2g, depth, k, poses = room_scene()
    inp = R.Grid(dims, vs, w2g).integrate(depth[:N_INPUT], k[:N_INPUT], poses[:N_INPUT])
    tgt = [g.integrate(depth, k, poses) for g in pyramid(dims, vs, w2g)]
    return inp, tgt
