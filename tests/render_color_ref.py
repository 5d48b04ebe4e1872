"""Independent NumPy restatement of the colour rules of mesh rendering (part A), on the
helpers of tests/render_ref.py.  Nothing here imports sgnn_amd.render.

Section F's rules 1-9 are restated again with a colour carried by every vertex: fp32 values with one rounding per
operation, int64 snapped coordinates and edge functions.  The depth test is a minimum over 64-bit keys (z bit pattern
in the high word, R<<24 | G<<16 | B<<8 | 255 in the low word), so depth and rgba of the device must match
`render_color_ref` bit for bit.  `perspective=False` interpolates the colour in screen space instead (c = sum e_k c_k /
A2): not a rule, but the mistake the perspective test must catch.
"""
import numpy as np

import fusion_ref as R
import render_ref as RR

F32 = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# the affine colour of the tests: channel = AFFINE_BASE + AFFINE_GRAD . (x, y, z) in world metres; inside the room of
# fusion_ref (4.0 x 3.2 x 2.6 m) every channel stays between 20 and 222
AFFINE_BASE = np.array([20.0, 30.0, 40.0])
AFFINE_GRAD = np.diag([50.0, 60.0, 70.0])


def affine_color(points):
    """The affine colour function at world points (.., 3), fp64, not rounded."""
    return AFFINE_BASE + np.asarray(points, np.float64) @ AFFINE_GRAD.T


def affine_vertex_colors(verts):
    """(V, 3) uint8: the affine colour at every vertex, rounded to the nearest integer."""
    return np.clip(np.rint(affine_color(verts)), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------
# rules 1 and 2 of section N: colours carried through section F's rules 2-5
# ---------------------------------------------------------------------------------------------------------
def _clip(a, b, ca, cb, zc):
    """The clip point and its colour, from the kept end a towards the dropped end b, with one t for both."""
    with np.errstate(all='ignore'):
        t = (zc - a[:, 2]) / (b[:, 2] - a[:, 2])
        x = a[:, 0] + t * (b[:, 0] - a[:, 0])
        y = a[:, 1] + t * (b[:, 1] - a[:, 1])
        c = ca + t[:, None] * (cb - ca)
    return np.stack([x, y, np.full_like(x, zc)], -1), c.astype(F32)


def camera_triangles(verts, faces, vcolors, m, z_clip):
    """((n, 3, 3) fp32 camera-space triangles, (n, 3, 3) fp32 colours of their vertices) after the near-plane clip."""
    zc = F32(z_clip)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    first = np.argmin(faces, 1)                                            # smallest index first, cyclic order kept
    faces = np.take_along_axis(faces, (first[:, None] + np.arange(3)) % 3, 1)
    p = RR._transform(m, np.asarray(verts, F32))[faces]
    col = np.asarray(vcolors, np.uint8).astype(F32)[faces]
    kept = p[:, :, 2] >= zc
    nk = kept.sum(1)
    tris, cols = [p[nk == 3]], [col[nk == 3]]
    one = nk == 1
    if one.any():
        q, qc, s = p[one], col[one], np.argmax(kept[one], 1)
        a, b, c = (RR._take(q, (s + i) % 3) for i in range(3))
        ca, cb, cc = (RR._take(qc, (s + i) % 3) for i in range(3))
        pb, colb = _clip(a, b, ca, cb, zc)
        pc, colc = _clip(a, c, ca, cc, zc)
        tris.append(np.stack([a, pb, pc], 1))
        cols.append(np.stack([ca, colb, colc], 1))
    two = nk == 2
    if two.any():
        q, qc, s, idx = p[two], col[two], np.argmin(kept[two], 1), faces[two]
        ia, ib = (s + 1) % 3, (s + 2) % 3
        swap = RR._take(idx, ib) < RR._take(idx, ia)                       # apex: the kept vertex of smaller index
        ip, io = np.where(swap, ib, ia), np.where(swap, ia, ib)
        pa, po, d = RR._take(q, ip), RR._take(q, io), RR._take(q, s)
        ca, co, cd = RR._take(qc, ip), RR._take(qc, io), RR._take(qc, s)
        xo, colo = _clip(po, d, co, cd, zc)
        xp, colp = _clip(pa, d, ca, cd, zc)
        tris += [np.stack([pa, po, xo], 1), np.stack([pa, xo, xp], 1)]
        cols += [np.stack([ca, co, colo], 1), np.stack([ca, colo, colp], 1)]
    return np.concatenate(tris), np.concatenate(cols)


def screen_triangles(tri, col, k):
    """Section F's rules 4 and 5 with the colours: X, Y int64 (n, 3), z fp32 (n, 3), A2 int64 (n,), colours (n, 3, 3)."""
    fx, fy, cx, cy = (F32(v) for v in k)
    with np.errstate(all='ignore'):
        u = (tri[:, :, 0] * fx) / tri[:, :, 2] + cx
        v = (tri[:, :, 1] * fy) / tri[:, :, 2] + cy
    X, okx = RR._snap(u)
    Y, oky = RR._snap(v)
    ok = (okx & oky).all(1)
    X, Y, z, col = X[ok], Y[ok], tri[ok][:, :, 2], col[ok]
    a2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    neg = a2 < 0
    for arr in (X, Y, z, col):
        arr[neg] = arr[neg][:, [0, 2, 1]]
    a2 = np.abs(a2)
    nz = a2 != 0
    return X[nz], Y[nz], z[nz], a2[nz], col[nz]


# ---------------------------------------------------------------------------------------------------------
# rules 3 and 4 of section N: pixel colour and the depth test on keys
# ---------------------------------------------------------------------------------------------------------
def channel8(c):
    """(int)roundf(c), half away from zero, clamped to 0..255."""
    with np.errstate(invalid='ignore'):
        r = R.round_away(c.astype(F32))
        return np.where(r >= 255, 255, np.where(r >= 0, r, 0)).astype(np.uint64)


def rasterise(keys, X, Y, z, a2, col, hw, perspective=True):
    """Fold the triangles into keys (h*w,) uint64, the running minimum of (z bits, packed colour)."""
    h, w = hw
    i0 = np.maximum((X.min(1) + 255) >> 8, 0)
    i1 = np.minimum(X.max(1) >> 8, w - 1)
    j0 = np.maximum((Y.min(1) + 255) >> 8, 0)
    j1 = np.minimum(Y.max(1) >> 8, h - 1)
    for t in np.nonzero((i0 <= i1) & (j0 <= j1))[0]:                        # one triangle at a time: plain and slow
        pi, pj = np.meshgrid(np.arange(i0[t], i1[t] + 1), np.arange(j0[t], j1[t] + 1))
        px, py = pi * 256, pj * 256
        x, y = X[t], Y[t]
        e = [RR._edge(x[(k + 1) % 3], y[(k + 1) % 3], x[(k + 2) % 3], y[(k + 2) % 3], px, py) for k in range(3)]
        cov = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
        if not cov.any():
            continue
        e = [v[cov] for v in e]
        r = [F32(1.0) / z[t, k] for k in range(3)]
        with np.errstate(all='ignore'):
            wk = [e[k].astype(F32) * r[k] for k in range(3)]
            q = (wk[0] + wk[1]) + wk[2]
            depth = (F32(a2[t]) / q).astype(F32)
            packed = np.zeros(len(q), np.uint64)
            for ch in range(3):
                if perspective:
                    c = ((wk[0] * col[t, 0, ch] + wk[1] * col[t, 1, ch]) + wk[2] * col[t, 2, ch]) / q
                else:
                    c = (e[0] * float(col[t, 0, ch]) + e[1] * float(col[t, 1, ch]) + e[2] * float(col[t, 2, ch])) / float(a2[t])
                packed = (packed << np.uint64(8)) | channel8(np.asarray(c, F32))
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (packed << np.uint64(8)) | np.uint64(255)
        np.minimum.at(keys, (pj * w + pi)[cov], key)


def render_color_ref(verts, faces, vcolors, intrinsics, cam2world, hw, z_clip=0.1, depth_min=0.4, depth_max=4.0,
                     perspective=True):
    """(depth (F, h, w) fp32, rgba (F, h, w, 4) uint8) of the coloured mesh."""
    h, w = hw
    k = np.asarray(intrinsics, F32).reshape(-1, 4)
    poses = np.asarray(cam2world, np.float64).reshape(-1, 4, 4)
    depth = np.empty((len(poses), h, w), F32)
    rgba = np.zeros((len(poses), h, w, 4), np.uint8)
    for f in range(len(poses)):
        keys = np.full(h * w, NO_KEY, np.uint64)
        m = RR.camera_rows(poses[f])
        if m is not None and len(np.asarray(faces).reshape(-1, 3)):
            tri, col = camera_triangles(verts, faces, vcolors, m, z_clip)
            rasterise(keys, *screen_triangles(tri, col, k[f]), hw, perspective=perspective)
        zf = (keys >> np.uint64(32)).astype(np.uint32).view(F32)
        with np.errstate(invalid='ignore'):
            keep = (keys != NO_KEY) & np.isfinite(zf) & (zf >= F32(depth_min)) & (zf <= F32(depth_max))   # rule 5
        depth[f] = np.where(keep, zf, F32(-np.inf)).reshape(h, w)
        low = keys.astype(np.uint32)
        for ch, shift in enumerate((24, 16, 8, 0)):
            rgba[f, :, :, ch] = np.where(keep, (low >> np.uint32(shift)) & np.uint32(255), 0).reshape(h, w)
    return depth, rgba
