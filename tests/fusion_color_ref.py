"""Independent NumPy restatement of the colour rules of TSDF fusion, on the helpers of
tests/fusion_ref.py.  Nothing here imports sgnn_amd.fusion.

ColorGrid restates the frame loop of fusion_ref.Grid in fp32, one rounding per operation, with the colour update
behind the geometry update; the device state must match it as integers.  pack() restates the resampling of colour
frames, and the painted room gives every primitive of fusion_ref's analytic room a colour of its own.
"""
import numpy as np

import fusion_ref as R

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------
# colour frames
# ---------------------------------------------------------------------------------------------------------
def pack(raw, out_hw=None):
    """(F, hr, wr, 3|4) or (hr, wr, 3|4) uint8 -> (F, h, w, 4) uint8 R, G, B, A: nearest index round(i (wr-1)/(w-1)),
    half away from zero, in fp32; A = 255 for three channels, (a != 0) ? 255 : 0 for four."""
    raw = np.asarray(raw, dtype=np.uint8)
    raw = raw[None] if raw.ndim == 3 else raw
    nf, hr, wr, ch = raw.shape
    h, w = (hr, wr) if out_hw is None else out_hw
    xs = R.round_away(np.arange(w, dtype=F32) * (F32(wr - 1) / F32(w - 1))).astype(np.int64)
    ys = R.round_away(np.arange(h, dtype=F32) * (F32(hr - 1) / F32(h - 1))).astype(np.int64)
    src = raw[:, ys][:, :, xs]
    out = np.empty((nf, h, w, 4), np.uint8)
    out[..., :3] = src[..., :3]
    out[..., 3] = 255 if ch == 3 else np.where(src[..., 3] != 0, 255, 0)
    return out


# ---------------------------------------------------------------------------------------------------------
# integration with colour
# ---------------------------------------------------------------------------------------------------------
class ColorGrid(object):
    """sdf / weight / free as fusion_ref.Grid (fp32), q (dz, dy, dx, 3) int64 = R, G, B in 8.8 fixed point and
    wc (dz, dy, dx) int64 = the colour weight."""

    def __init__(self, dims_xyz, voxel_size, world2grid, dmin=0.4, dmax=4.0, obb=None):
        dx, dy, dz = dims_xyz
        self.dims = tuple(dims_xyz)
        self.vs, self.w2g, self.dmin, self.dmax, self.obb = F32(voxel_size), np.asarray(world2grid), dmin, dmax, obb
        self.sdf = np.full((dz, dy, dx), -np.inf, F32)
        self.weight = np.zeros((dz, dy, dx), np.int64)
        self.free = np.zeros((dz, dy, dx), np.int64)
        self.q = np.zeros((dz, dy, dx, 3), np.int64)
        self.wc = np.zeros((dz, dy, dx), np.int64)

    def integrate(self, depth, intr, c2w, rgba=None):
        depth = np.asarray(depth, F32)
        h, w = depth.shape[1:]
        for f in range(depth.shape[0]):
            box = R.frame_box(intr[f], c2w[f], (h, w), self.w2g, self.dims, self.dmin, self.dmax)
            if box is None:
                continue
            zz, yy, xx = np.meshgrid(np.arange(box[4], box[5] + 1), np.arange(box[2], box[3] + 1),
                                     np.arange(box[0], box[1] + 1), indexing='ij')
            vox = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)
            if self.obb is not None:
                vox = vox[R.in_obb(self.obb, vox)]
            m = R.voxel_to_camera(c2w[f], self.w2g)
            p = vox.astype(F32)
            pf = [((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)]
            fx, fy, cx, cy = (F32(v) for v in intr[f])
            with np.errstate(all='ignore'):
                px = R.round_away((pf[0] * fx) / pf[2] + cx)
                py = R.round_away((pf[1] * fy) / pf[2] + cy)
            on = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            vox, pz, px, py = vox[on], pf[2][on], px[on].astype(np.int64), py[on].astype(np.int64)
            d = depth[f, py, px]
            ok = np.isfinite(d) & (d >= F32(self.dmin)) & (d <= F32(self.dmax))
            vox, pz, px, py, d = vox[ok], pz[ok], px[ok], py[ok], d[ok]
            self.free[vox[:, 2], vox[:, 1], vox[:, 0]] += (pz < d)
            sd0 = d - pz
            tr = self.vs * F32(3.0) + d * self.vs
            up = sd0 > -tr
            vox, px, py, d, sd0, tr = vox[up], px[up], py[up], d[up], sd0[up], tr[up]
            iz, iy, ix = vox[:, 2], vox[:, 1], vox[:, 0]
            sd = np.where(sd0 >= 0, np.minimum(tr, sd0), np.maximum(-tr, sd0)).astype(F32)
            z01 = (d - F32(0.4)) / (F32(4.0) - F32(0.4))
            wu = np.maximum(F32(4.5) * (F32(1.0) - z01), F32(1.0)).astype(F32)
            old, ow = self.sdf[iz, iy, ix], self.weight[iz, iy, ix].astype(F32)
            with np.errstate(invalid='ignore'):
                self.sdf[iz, iy, ix] = np.where(old == -np.inf, sd, (old * ow + sd * wu) / (ow + wu)).astype(F32)
            self.weight[iz, iy, ix] = np.minimum(self.weight[iz, iy, ix] + wu.astype(np.int64), 255)
            if rgba is None:
                continue
            pix = rgba[f, py, px]
            col = (sd0 < tr) & (pix[:, 3] != 0)                     # not clamped on the free side, pixel has a colour
            iz, iy, ix, wu, pix = iz[col], iy[col], ix[col], wu[col], pix[col]
            wc = self.wc[iz, iy, ix]
            wcf = wc.astype(F32)
            for c in range(3):
                ci = (pix[:, c].astype(np.int64) * 256).astype(F32)
                q = self.q[iz, iy, ix, c].astype(F32)
                mean = R.round_away(((q * wcf + ci * wu) / (wcf + wu)).astype(F32))
                self.q[iz, iy, ix, c] = np.where(wc == 0, ci, mean).astype(np.int64)
            self.wc[iz, iy, ix] = np.minimum(wc + wu.astype(np.int64), 255)
        return self

    def state(self):
        """(dz, dy, dx, 4) uint16, the layout of TSDFVolume.color_state()."""
        return np.concatenate([self.q, self.wc[..., None]], -1).astype(np.uint16)

    def colors(self):
        """(dz, dy, dx, 3) uint8: (q + 128) >> 8 where wc > 0, else 0."""
        return np.where(self.wc[..., None] > 0, (self.q + 128) >> 8, 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------
# colour frames for the tests
# ---------------------------------------------------------------------------------------------------------
def noise_frames(shape_fhw, seed, invalid=0.05):
    """Random R, G, B with A = 255, and A = 0 on about `invalid` of the pixels."""
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, size=tuple(shape_fhw) + (4,), dtype=np.uint8)
    rgba[..., 3] = np.where(rng.random(shape_fhw) < invalid, 0, 255)
    return rgba


def uniform_frames(shape_fhw, rgb, seed, invalid=0.05):
    out = noise_frames(shape_fhw, seed, invalid)
    out[..., :3] = np.asarray(rgb, np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------
# the conditions of the mesh tests, shared by the CPU test of this reference and the GPU test of the kernels
# ---------------------------------------------------------------------------------------------------------
INVALID = 0.05        # share of A == 0 pixels in the test frames
# A mesh vertex takes the colour of its cell's centre voxel, which lies within a voxel of the zero crossing; meshing
# with a truncation of three voxels keeps only cells whose 27 voxels hold |sdf| < 3 voxels, so none of them was clamped
# on the free side (the clamp value is at least 3 voxels).  Such a voxel stays without a colour only if every pixel
# that updated it had A == 0: with one observation that happens for INVALID of the voxels, with more for fewer.
BLACK_SHARE_CAP = INVALID
KEPT_SHARE_MIN = 0.5  # painted room: vertices away from every colour boundary must be at least half of all


def mc_args(voxel_size):
    """(isovalue, truncation, thresh) for run_marching_cubes on a metric sdf(): the surface inside the band of three
    voxels, no jump test."""
    return 0.0, float(F32(3.0) * F32(voxel_size)), 10.0


def painted_margin(voxel_size, fx):
    """The colour band (3 voxels) plus one pixel footprint at 4 m, in metres."""
    return 3.0 * float(voxel_size) + 4.0 / float(fx)


def black_share(vertex_colors):
    c = np.asarray(vertex_colors)
    return float((c == 0).all(1).mean())


# ---------------------------------------------------------------------------------------------------------
# the painted room: fusion_ref's primitives, a colour per primitive
# ---------------------------------------------------------------------------------------------------------
# floor, ceiling and the four walls in the order of fusion_ref.ROOM_PLANES; the three boxes of ROOM_BOXES
PLANE_COLORS = [(200, 40, 30), (90, 90, 90), (30, 180, 60), (220, 200, 40), (160, 60, 200), (40, 200, 200)]
BOX_COLORS = [(40, 60, 220), (250, 120, 20), (120, 250, 130)]


def render_painted(k, cam2world, hw, planes=R.ROOM_PLANES, boxes=R.ROOM_BOXES, plane_colors=PLANE_COLORS,
                   box_colors=BOX_COLORS):
    """fusion_ref.render with the colour of the primitive each ray hits first: (depth (h, w) f32, rgba (h, w, 4) u8,
    A = 0 where the ray misses everything).  The depth equals fusion_ref.render's."""
    h, w = hw
    fx, fy, cx, cy = (float(v) for v in k)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c2w = np.asarray(cam2world, np.float64)
    dw = dirs @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = np.full((h, w), np.inf)
    rgba = np.zeros((h, w, 4), np.uint8)
    with np.errstate(all='ignore'):
        for (n, c), col in zip(planes, plane_colors):
            n = np.asarray(n, np.float64)
            tt = (c - n @ o) / (dw @ n)
            hit = (tt > 0) & (tt < t)
            t = np.where(hit, tt, t)
            rgba[hit] = tuple(col) + (255,)
        for (lo, hi), col in zip(boxes, box_colors):
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            t0 = (lo - o) / dw
            t1 = (hi - o) / dw
            tn = np.minimum(t0, t1).max(-1)
            tf = np.maximum(t0, t1).min(-1)
            hit = (tf >= tn) & (tn > 0) & (tn < t)
            t = np.where(hit, tn, t)
            rgba[hit] = tuple(col) + (255,)
    return np.where(np.isfinite(t), t, -np.inf).astype(F32), rgba


def painted_frames(intr, poses, hw):
    """(depth (F, h, w), rgba (F, h, w, 4)) of the painted room for the given intrinsics and poses."""
    out = [render_painted(intr[f], poses[f], hw) for f in range(len(poses))]
    return np.stack([d for d, _ in out]), np.stack([c for _, c in out])


def primitive_distances(points_world):
    """Distance of world points (n, 3) to the surface of every primitive: (n, 6 planes + 3 boxes)."""
    p = np.asarray(points_world, np.float64)
    cols = []
    for n, c in R.ROOM_PLANES:
        n = np.asarray(n, np.float64)
        cols.append(np.abs(p @ n - c))
    for lo, hi in R.ROOM_BOXES:
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        out = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)          # outside: to the box
        ins = np.minimum(p - lo, hi - p).min(1)                                            # inside: to the nearest face
        cols.append(np.where(out > 0, out, np.maximum(ins, 0.0)))
    return np.stack(cols, 1)


def painted_expectation(verts_vox, world2grid, margin):
    """For mesh vertices in voxel coordinates: (colour (n, 3) u8 of the nearest primitive, keep (n,) bool = every
    primitive of another colour is farther than `margin` metres away)."""
    g2w = np.linalg.inv(np.asarray(world2grid, np.float64))
    v = np.asarray(verts_vox, np.float64)
    pw = v @ g2w[:3, :3].T + g2w[:3, 3]
    dist = primitive_distances(pw)
    colours = np.array(PLANE_COLORS + BOX_COLORS, np.uint8)
    near = dist.argmin(1)
    own = colours[near]
    other = (colours[None, :, :] != own[:, None, :]).any(-1)
    far = np.where(other, dist, np.inf).min(1)
    return own, far > margin
