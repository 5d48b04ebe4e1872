"""Independent NumPy restatement of the depth-rendering rules and a tessellated
version of the analytic room of tests/fusion_ref.py.

Nothing here imports sgnn_amd.render.  Camera-space values are fp32 with one rounding per operation, snapped
coordinates, areas and edge functions are int64, so the device result must match `render_ref` bit for bit.  The
triangles of one frame are rasterised in buckets of equal (power of two) pixel-box size, vectorised over the
triangles of a bucket; the depth test is a minimum over the unsigned bit patterns (`np.minimum.at`).
"""
import numpy as np

import fusion_ref as R

F32 = np.float32
SNAP_LIMIT = float(2 ** 29)
INF_BITS = np.uint32(0x7F800000)


# ---------------------------------------------------------------------------------------------------------
# rule 1: the camera matrix
# ---------------------------------------------------------------------------------------------------------
def camera_rows(cam2world):
    """Rows 0..2 of inv(cam2world), fp64 -> fp32; None for a non-finite pose."""
    c = np.asarray(cam2world, np.float64).reshape(4, 4)
    if not np.isfinite(c).all():
        return None
    return np.linalg.inv(c)[:3].astype(F32)


# ---------------------------------------------------------------------------------------------------------
# rules 2-5: triangles of one frame -> snapped screen triangles
# ---------------------------------------------------------------------------------------------------------
def _transform(m, v):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], -1)


def _clip_point(a, b, zc):
    """From the kept end a (n, 3) towards the dropped end b."""
    with np.errstate(all='ignore'):
        t = (zc - a[:, 2]) / (b[:, 2] - a[:, 2])
        x = a[:, 0] + t * (b[:, 0] - a[:, 0])
        y = a[:, 1] + t * (b[:, 1] - a[:, 1])
    return np.stack([x, y, np.full_like(x, zc)], -1)


def _take(p, pos):
    return p[np.arange(len(p)), pos]


def camera_triangles(verts, faces, m, z_clip):
    """(n, 3, 3) fp32 camera-space triangles after the near-plane clip (rules 2 and 3)."""
    zc = F32(z_clip)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    first = np.argmin(faces, 1)                                            # smallest index first, cyclic order kept
    faces = np.take_along_axis(faces, (first[:, None] + np.arange(3)) % 3, 1)
    p = _transform(m, np.asarray(verts, F32))[faces]                       # (T, 3 vertices, 3)
    kept = p[:, :, 2] >= zc                                                # NaN: not kept
    nk = kept.sum(1)
    out = [p[nk == 3]]
    one = nk == 1
    if one.any():
        q, s = p[one], np.argmax(kept[one], 1)
        a, b, c = _take(q, s), _take(q, (s + 1) % 3), _take(q, (s + 2) % 3)
        out.append(np.stack([a, _clip_point(a, b, zc), _clip_point(a, c, zc)], 1))
    two = nk == 2
    if two.any():
        q, s, idx = p[two], np.argmin(kept[two], 1), faces[two]
        ia, ib = (s + 1) % 3, (s + 2) % 3                                  # the kept two, in cyclic order after d
        swap = _take(idx, ib) < _take(idx, ia)                             # apex: the kept vertex of smaller index
        ip, io = np.where(swap, ib, ia), np.where(swap, ia, ib)
        pa, po, d = _take(q, ip), _take(q, io), _take(q, s)
        co, cp = _clip_point(po, d, zc), _clip_point(pa, d, zc)
        out.append(np.stack([pa, po, co], 1))
        out.append(np.stack([pa, co, cp], 1))
    return np.concatenate(out)


def _snap(u):
    with np.errstate(all='ignore'):
        s = R.round_away(u * F32(256.0))
        ok = np.abs(s) <= F32(SNAP_LIMIT)                                  # NaN and inf fail
    return np.where(ok, s, 0).astype(np.int64), ok


def screen_triangles(tri, k):
    """Rules 4 and 5: (X, Y) int64 (n, 3), z fp32 (n, 3), A2 int64 (n,) > 0 of the triangles that survive."""
    fx, fy, cx, cy = (F32(v) for v in k)
    with np.errstate(all='ignore'):
        u = (tri[:, :, 0] * fx) / tri[:, :, 2] + cx
        v = (tri[:, :, 1] * fy) / tri[:, :, 2] + cy
    X, okx = _snap(u)
    Y, oky = _snap(v)
    ok = (okx & oky).all(1)
    X, Y, z = X[ok], Y[ok], tri[ok][:, :, 2]
    a2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    neg = a2 < 0
    for arr in (X, Y, z):
        arr[neg] = arr[neg][:, [0, 2, 1]]
    a2 = np.abs(a2)
    nz = a2 != 0
    return X[nz], Y[nz], z[nz], a2[nz]


# ---------------------------------------------------------------------------------------------------------
# rules 6-8: coverage, depth and the depth test
# ---------------------------------------------------------------------------------------------------------
def _edge(xa, ya, xb, yb, px, py):
    return (xb - xa) * (py - ya) - (yb - ya) * (px - xa)


def rasterise(bits, X, Y, z, a2, hw):
    """Fold the triangles into bits (h*w,) uint32, the running minimum of the depth bit patterns."""
    h, w = hw
    i0 = np.maximum((X.min(1) + 255) >> 8, 0)
    i1 = np.minimum(X.max(1) >> 8, w - 1)
    j0 = np.maximum((Y.min(1) + 255) >> 8, 0)
    j1 = np.minimum(Y.max(1) >> 8, h - 1)
    on = (i0 <= i1) & (j0 <= j1)
    X, Y, z, a2, i0, i1, j0, j1 = (a[on] for a in (X, Y, z, a2, i0, i1, j0, j1))
    if not len(a2):
        return
    side = np.maximum(i1 - i0, j1 - j0) + 1
    bucket = np.ceil(np.log2(side)).astype(np.int64)
    r = (F32(1.0) / z).astype(F32)
    af = a2.astype(F32)
    for b in np.unique(bucket):
        sel = np.nonzero(bucket == b)[0]
        n = 1 << int(b)
        step = max(1, (1 << 18) // (n * n))
        oi, oj = np.meshgrid(np.arange(n), np.arange(n))
        for s0 in range(0, len(sel), step):
            t = sel[s0:s0 + step]
            pi = i0[t, None, None] + oi
            pj = j0[t, None, None] + oj
            inside = (pi <= i1[t, None, None]) & (pj <= j1[t, None, None])
            px, py = pi * 256, pj * 256
            x, y = X[t][:, :, None, None], Y[t][:, :, None, None]
            e0 = _edge(x[:, 1], y[:, 1], x[:, 2], y[:, 2], px, py)
            e1 = _edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], px, py)
            e2 = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], px, py)
            assert ((e0 + e1 + e2) == a2[t, None, None]).all()
            cov = inside & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
            rr = r[t][:, :, None, None]
            with np.errstate(all='ignore'):
                q = (e0.astype(F32) * rr[:, 0] + e1.astype(F32) * rr[:, 1]) + e2.astype(F32) * rr[:, 2]
                depth = (af[t, None, None] / q).astype(F32)
            np.minimum.at(bits, (pj * w + pi)[cov], depth[cov].view(np.uint32))


def render_ref(verts, faces, intrinsics, cam2world, hw, z_clip=0.1, depth_min=0.4, depth_max=4.0):
    """(F, h, w) fp32 depth of the mesh, -inf where nothing is seen (rules 1-9)."""
    h, w = hw
    k = np.asarray(intrinsics, F32).reshape(-1, 4)
    poses = np.asarray(cam2world, np.float64).reshape(-1, 4, 4)
    out = np.empty((len(poses), h, w), F32)
    for f in range(len(poses)):
        bits = np.full(h * w, INF_BITS, np.uint32)
        m = camera_rows(poses[f])
        if m is not None:
            tri = camera_triangles(verts, faces, m, z_clip)
            rasterise(bits, *screen_triangles(tri, k[f]), hw)
        zf = bits.view(F32)
        keep = (bits != INF_BITS) & (zf >= F32(depth_min)) & (zf <= F32(depth_max))      # rule 9
        out[f] = np.where(keep, zf, F32(-np.inf)).reshape(h, w)
    return out


# ---------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------
def _grid_face(origin, eu, ev, n):
    """n x n quads on the rectangle origin + s*eu + t*ev -> ((n+1)^2, 3) points, (2 n^2, 3) triangles."""
    s = np.arange(n + 1, dtype=np.float64) / n
    pts = (origin[None, None] + s[:, None, None] * eu[None, None] + s[None, :, None] * ev[None, None]).reshape(-1, 3)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None]).ravel()
    tris = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)])
    return pts, tris


def box_mesh(lo, hi, n):
    """The six faces of an axis-aligned box as n x n quads each; vertices on shared edges are merged."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pts, tris, base = [], [], 0
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        eu, ev = np.zeros(3), np.zeros(3)
        eu[u], ev[v] = hi[u] - lo[u], hi[v] - lo[v]
        for c in (lo[ax], hi[ax]):
            o = lo.copy()
            o[ax] = c
            p, t = _grid_face(o, eu, ev, n)
            pts.append(p)
            tris.append(t + base)
            base += len(p)
    pts = np.concatenate(pts)
    # merge by lattice position (exact: every face places its points at integer multiples of the extent / n)
    key = np.round((pts - lo) / np.where(hi > lo, hi - lo, 1.0) * n).astype(np.int64)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return pts[first], inv.reshape(-1)[np.concatenate(tris)]


def tessellate_room(n):
    """The closed 4.0 x 3.2 x 2.6 m room of fusion_ref.ROOM_PLANES and the three ROOM_BOXES, n x n quads per face:
    (verts (V, 3) fp32, faces (T, 3) int32)."""
    ext = np.array([-R.ROOM_PLANES[3][1], -R.ROOM_PLANES[5][1], -R.ROOM_PLANES[1][1]])
    parts = [box_mesh((0.0, 0.0, 0.0), ext, n)] + [box_mesh(lo, hi, n) for lo, hi in R.ROOM_BOXES]
    verts, faces, base = [], [], 0
    for p, t in parts:
        verts.append(p)
        faces.append(t + base)
        base += len(p)
    return np.concatenate(verts).astype(F32), np.concatenate(faces).astype(np.int32)


def triangle_soup(n, seed=0, lo=(-1.0, -1.0, -0.5), hi=(5.0, 4.2, 3.1)):
    """n random triangles, most from millimetres to decimetres, one in fifty several metres, some sharing vertices."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo), np.asarray(hi)
    centre = rng.uniform(lo, hi, (n, 3))
    size = 10.0 ** np.where(rng.random((n, 1, 1)) < 0.02, rng.uniform(0.0, 0.8, (n, 1, 1)), rng.uniform(-2.5, -0.5, (n, 1, 1)))
    pts = centre[:, None] + rng.normal(size=(n, 3, 3)) * size
    verts = pts.reshape(-1, 3).astype(F32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    share = rng.random(n) < 0.3                                             # some triangles reuse earlier vertices
    faces[share, 0] = rng.integers(0, 3 * n, share.sum())
    return verts, faces
