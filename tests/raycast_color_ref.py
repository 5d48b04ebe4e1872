"""Independent NumPy restatement of the colour rules of TSDF ray casting (part B), on the
helpers of tests/raycast_ref.py.  Nothing here imports sgnn_amd.raycast.

Depth and normals are raycast_ref.cast's.  The colour of a pixel is evaluated once, at the hit, from the corners of the
hit's cell that have a colour; fp32 with one rounding per operation, corners visited x fastest, then y, then z, and a
corner without a colour is left out of both sums.  The device result must match `cast_color` bit for bit.
"""
import numpy as np

import fusion_ref as R
import raycast_ref as C

F32 = np.float32


def rgba_volume(colors):
    """(Z, Y, X, 4) uint8 from (Z, Y, X, 3 | 4): three channels mean that every voxel has a colour."""
    colors = np.asarray(colors, np.uint8)
    if colors.shape[-1] == 4:
        return colors
    return np.concatenate([colors, np.full(colors.shape[:3] + (1,), 255, np.uint8)], -1)


def hit_cells(shape_zyx, g):
    """Rule 2: (inside (P,), cell (P, 3) int64 x y z, 0 where outside) of grid positions g (P, 3) fp32."""
    dz, dy, dx = shape_zyx
    f = np.floor(g)
    inside = np.ones(len(g), bool)
    for a, d in enumerate((dx, dy, dz)):
        inside &= (f[:, a] >= 0) & (f[:, a] <= d - 2)
    return inside, np.where(inside[:, None], f, 0).astype(np.int64)


def hit_colors(colors, g):
    """Rules 2-6 at grid positions g (P, 3) fp32, x y z -> (P, 4) uint8."""
    colors = rgba_volume(colors)
    inside, cell = hit_cells(colors.shape[:3], g)
    a = (g - cell.astype(F32)).astype(F32)                                  # g - floor(g) where inside
    axis_w = [(F32(1.0) - a[:, n], a[:, n]) for n in range(3)]              # x, y, z
    s = np.zeros(len(g), F32)
    n = np.zeros((len(g), 3), F32)
    x, y, z = cell[:, 0], cell[:, 1], cell[:, 2]
    zmax, ymax, xmax = (d - 1 for d in colors.shape[:3])
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                w = (axis_w[2][k] * axis_w[1][j]) * axis_w[0][i]
                c = colors[np.minimum(z + k, zmax), np.minimum(y + j, ymax), np.minimum(x + i, xmax)]   # read where inside
                counted = inside & (c[:, 3] != 0)
                s = np.where(counted, s + w, s).astype(F32)
                for ch in range(3):
                    n[:, ch] = np.where(counted, n[:, ch] + w * c[:, ch].astype(F32), n[:, ch])
    out = np.zeros((len(g), 4), np.uint8)
    some = inside & (s != 0)
    with np.errstate(all='ignore'):
        for ch in range(3):
            r = R.round_away((n[:, ch] / s).astype(F32))
            out[:, ch] = np.where(some, np.clip(np.where(np.isnan(r), 0, r), 0, 255), 0).astype(np.uint8)
    out[:, 3] = np.where(some, 255, 0)
    return out


def cast_color(sdf, colors, world2grid, voxel_size, intrinsics, cam2world, hw, band, step=0.5, depth_min=0.4,
               depth_max=4.0, normals=False):
    """(depth, rgba) or (depth, normal, rgba): raycast_ref.cast and (F, h, w, 4) uint8 colour frames."""
    geo = C.cast(sdf, world2grid, voxel_size, intrinsics, cam2world, hw, band, step, depth_min, depth_max, normals)
    depth = geo[0] if normals else geo
    h, w = hw
    intr = np.asarray(intrinsics, F32).reshape(-1, 4)
    poses = np.asarray(cam2world, np.float64).reshape(-1, 4, 4)
    rgba = np.zeros((len(poses), h * w, 4), np.uint8)
    for f in range(len(poses)):
        g = C.frame_matrix(world2grid, poses[f])
        hit = np.isfinite(depth[f]).ravel()
        if g is None or not hit.any():
            continue
        o, d = C.rays(g, intr[f], hw)
        t = depth[f].ravel()[hit]
        rgba[f, hit] = hit_colors(colors, (o + t[:, None] * d[hit]).astype(F32))      # rule 1: at g* = o + t* d
    rgba = rgba.reshape(len(poses), h, w, 4)
    return (depth, geo[1], rgba) if normals else (depth, rgba)
