"""Independent NumPy restatement of the mesh voxelisation rules.

Nothing here imports sgnn_amd.voxelize or touches a device.  Every fp32 value is produced by one NumPy operation per
rounding in the order sections G and L state, so the device's distance magnitudes and faces must match
`signed_distance_ref` bit for bit; signs must match wherever the reference itself is not ambiguous.  Brute force over
all (voxel, usable face) pairs: no bricks, no boxes.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
Q32 = 4294967296.0
VERT_A, VERT_B, VERT_C, EDGE_AB, EDGE_AC, EDGE_BC, INTERIOR = range(7)
AMBIGUOUS = 1e-4        # a sign is left out of comparisons when |s| <= AMBIGUOUS * |e| * |N|


# ---------------------------------------------------------------------------------------------------------
# rule 1: grid coordinates
# ---------------------------------------------------------------------------------------------------------
def grid_coords_ref(verts, world2grid):
    m = np.asarray(world2grid, F32).reshape(4, 4)
    v = np.asarray(verts, F32).reshape(-1, 3)
    with np.errstate(all='ignore'):
        return np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)], 1)


# ---------------------------------------------------------------------------------------------------------
# rule 2: usable faces (section G, rule 1)
# ---------------------------------------------------------------------------------------------------------
def pack_ref(verts, faces, dtype=F32):
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all='ignore'):
        ab, ac = b - a, c - a
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
    usable = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1) & ~(n == 0).all(1)
    if dtype is not F32:
        with np.errstate(all='ignore'):
            a, ab, ac = a.astype(dtype), b.astype(dtype) - a.astype(dtype), c.astype(dtype) - a.astype(dtype)
    return a, ab, ac, usable


# ---------------------------------------------------------------------------------------------------------
# rules 3 and 4: the residual of section G's rule 2 and the branch that produced it
# ---------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _away(u, s, v):
    return u - s[..., None] * v


def residual_ref(p, a, ab, ac):
    """e (.., 3) and feature (..) for broadcastable (.., 3) arrays of one dtype."""
    with np.errstate(all='ignore'):
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = ap - ab
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = ap - ac
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s, t = d4 - d3, d5 - d6
        den = (va + vb) + vc
        e = _away(_away(ap, vb / den, ab), vc / den, ac)
        r1, r2 = _dot(ab, e), _dot(ac, e)
        g11, g12, g22 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
        e = _away(_away(e, (r1 * g22 - r2 * g12) / den, ab), (r2 * g11 - r1 * g12) / den, ac)
        feature = np.full(np.broadcast(d1, d2).shape, INTERIOR, np.int8)
        # the first matching branch wins, so the branches are applied last to first
        for cond, val, code in (((va <= 0) & (s >= 0) & (t >= 0), _away(bp, s / (s + t), ac - ab), EDGE_BC),
                                ((vb <= 0) & (d2 >= 0) & (d6 <= 0), _away(ap, d2 / (d2 - d6), ac), EDGE_AC),
                                ((d6 >= 0) & (d5 <= d6), cp, VERT_C),
                                ((vc <= 0) & (d1 >= 0) & (d3 <= 0), _away(ap, d1 / (d1 - d3), ab), EDGE_AB),
                                ((d3 >= 0) & (d4 <= d3), bp, VERT_B),
                                ((d1 <= 0) & (d2 <= 0), ap, VERT_A)):
            e = np.where(cond[..., None], val, e)
            feature = np.where(cond, np.int8(code), feature)
        return e, feature


def _sq(e):
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def centres(dims_xyz, dtype=F32):
    """(dz * dy * dx, 3) voxel centres x, y, z in raster order, x fastest."""
    dx, dy, dz = dims_xyz
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing='ij')
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(dtype)


def nearest_ref(points, verts, faces, dtype=F32, block=2048):
    """Brute force: (best squared distance, face or -1) per point over all usable faces, lowest index among equals."""
    pts = np.asarray(points, F32).astype(dtype)
    a, ab, ac, usable = pack_ref(verts, faces, dtype)
    ids = np.nonzero(usable)[0]
    best = np.full(len(pts), np.inf, dtype)
    face = np.full(len(pts), -1, np.int64)
    if len(ids):
        for s in range(0, len(pts), block):
            e, _ = residual_ref(pts[s:s + block, None, :], a[None, ids], ab[None, ids], ac[None, ids])
            d2 = _sq(e)
            d2 = np.where(np.isnan(d2), np.inf, d2)
            k = np.argmin(d2, 1)                                                # first = lowest face index
            m = d2[np.arange(len(k)), k]
            best[s:s + block] = m
            face[s:s + block] = np.where(m < np.inf, ids[k], -1)
    return best, face


# ---------------------------------------------------------------------------------------------------------
# rule 5: pseudo-normals, fp64 contributions quantised to 2^-32 and summed as integers
# ---------------------------------------------------------------------------------------------------------
def _quant(x):
    return np.rint(x * Q32).astype(np.int64)


def pseudo_normals_ref(verts, faces):
    """(face normals n = ab x ac (T, 3) fp64, vertex sums (V, 3) int64, {(i, j) with i < j: edge sum (3,) int64})."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    _, ab, ac, usable = pack_ref(verts, faces)
    ab, ac = ab.astype(F64), ac.astype(F64)
    with np.errstate(all='ignore'):
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        length = np.sqrt(_dot(n, n))
        ok = usable & (length > 0) & np.isfinite(length)
        unit = n / length[:, None]
        g11, g12, g22 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
        angles = np.stack([np.arctan2(length, g12), np.arctan2(length, g11 - g12), np.arctan2(length, g22 - g12)], 1)
    vsum = np.zeros((len(v), 3), np.int64)
    edges = {}
    for t in np.nonzero(ok)[0]:
        for k in range(3):
            vsum[f[t, k]] += _quant(angles[t, k] * unit[t])
            i, j = int(f[t, k]), int(f[t, (k + 1) % 3])
            key = (min(i, j), max(i, j))
            edges[key] = edges.get(key, np.zeros(3, np.int64)) + _quant(unit[t])
    return n, vsum, edges


# ---------------------------------------------------------------------------------------------------------
# rules 3 to 6 for a whole volume
# ---------------------------------------------------------------------------------------------------------
class RefResult(object):
    """dist (dz, dy, dx) fp32 signed, +inf beyond the band; face int32, -1 beyond; ambiguous bool: the sign is left out
    of comparisons; naive_dist: the same distances signed by the winning face's own normal (what rules 4 to 6 replace)."""


def signed_distance_ref(verts_grid, faces, dims_xyz, band, flip=False):
    dx, dy, dz = dims_xyz
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    pts = centres(dims_xyz)
    best, face = nearest_ref(pts, verts_grid, f)
    d = np.sqrt(best.astype(F64)).astype(F32)              # correctly rounded fp32 root
    inband = (face >= 0) & (d <= F32(band))
    a, ab, ac, _ = pack_ref(verts_grid, f)
    normals, vsum, edges = pseudo_normals_ref(verts_grid, f)
    sel = np.nonzero(inband)[0]
    t = face[sel]
    e, feature = residual_ref(pts[sel], a[t], ab[t], ac[t])
    N = normals[t].copy()
    for k, code in enumerate((VERT_A, VERT_B, VERT_C)):
        m = feature == code
        N[m] = vsum[f[t[m], k]].astype(F64) * (1.0 / Q32)
    for (i, j), code in (((0, 1), EDGE_AB), ((0, 2), EDGE_AC), ((1, 2), EDGE_BC)):
        for q in np.nonzero(feature == code)[0]:
            u, w = int(f[t[q], i]), int(f[t[q], j])
            N[q] = edges[(min(u, w), max(u, w))].astype(F64) * (1.0 / Q32)
    if flip:
        N, normals = -N, -normals
    e64 = e.astype(F64)
    s = _dot(e64, N)
    s_naive = _dot(e64, normals[t])
    res = RefResult()
    dist = np.full(len(pts), np.inf, F32)
    dist[sel] = np.where(s >= 0, d[sel], -d[sel])
    naive = np.full(len(pts), np.inf, F32)
    naive[sel] = np.where(s_naive >= 0, d[sel], -d[sel])
    amb = np.zeros(len(pts), bool)
    amb[sel] = np.abs(s) <= AMBIGUOUS * np.sqrt(_dot(e64, e64)) * np.sqrt(_dot(N, N))
    res.dist, res.naive_dist = dist.reshape(dz, dy, dx), naive.reshape(dz, dy, dx)
    res.face = np.where(inband, face, -1).astype(np.int32).reshape(dz, dy, dx)
    res.ambiguous = amb.reshape(dz, dy, dx)
    return res


# ---------------------------------------------------------------------------------------------------------
# "Bricks and the hot kernel": the brick lists
# ---------------------------------------------------------------------------------------------------------
def brick_lists_ref(boxes, dims_xyz, band, brick=8):
    """CSR lists of the faces of every brick, bricks in raster order (x fastest): (offsets (bricks + 1,) int64, refs
    int64, ascending inside a brick).  boxes (T, 6) fp32 vertex boxes lo, hi, (+inf, -inf) for an ignored face.  A
    face's voxel box is its vertex box grown by band + 2^-16 m in fp32, m the largest of band, the largest dimension
    and the box's magnitudes; the face is listed in every brick that holds a voxel lo <= i <= hi of that box."""
    bx = np.asarray(boxes, F32).reshape(-1, 6)
    dims = np.array(dims_xyz, np.int64)
    nb = -(-dims // brick)
    band = F32(band)
    bricks, ids = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for t in range(len(bx)):
        if not bx[t, 0] <= bx[t, 3]:
            continue
        m = max(band, F32(dims.max()), np.abs(bx[t]).max())
        marg = band + m * F32(2.0 ** -16)
        first = np.maximum(np.ceil(bx[t, :3] - marg), F32(0))
        last = np.minimum(np.floor(bx[t, 3:] + marg), (dims - 1).astype(F32))
        if not (first <= last).all():
            continue
        r = [np.arange(int(first[k]) // brick, int(last[k]) // brick + 1) for k in range(3)]
        b = ((r[2][:, None, None] * nb[1] + r[1][None, :, None]) * nb[0] + r[0][None, None, :]).ravel()
        bricks.append(b)
        ids.append(np.full(len(b), t, np.int64))
    bricks, ids = np.concatenate(bricks), np.concatenate(ids)
    order = np.lexsort((ids, bricks))
    return np.concatenate([[0], np.cumsum(np.bincount(bricks, minlength=int(nb.prod())))]), ids[order]


# ---------------------------------------------------------------------------------------------------------
# fp64 checks of the restatement itself
# ---------------------------------------------------------------------------------------------------------
def distance64(points, verts, faces):
    """The same construction with every operation in fp64: the distance the fp32 rules approximate."""
    best, _ = nearest_ref(points, verts, faces, F64)
    return np.sqrt(best)


def _segment_distance2(p, a, d):
    """Squared fp64 distance from p (P, 1, 3) to the segments a + t d, t in [0, 1] (1, T, 3)."""
    t = np.clip(np.einsum('pti,pti->pt', p - a, np.broadcast_to(d, (p.shape[0],) + d.shape[1:])) /
                np.einsum('pti,pti->pt', d, d), 0.0, 1.0)
    r = p - a - t[..., None] * d
    return np.einsum('pti,pti->pt', r, r)


def exact_distance64(points, verts, faces):
    """Distance to the mesh by another construction than rule 2, in fp64, so that a slip in residual_ref's branches
    cannot sit on both sides of a comparison: where the foot of the perpendicular to a face's plane has barycentric
    coordinates inside the triangle the distance is the height over the plane, elsewhere the smallest distance to the
    three edges as clamped segments.  Brute force over the usable faces."""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[pack_ref(verts, faces)[3]]
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    g11, g12, g22 = (ab * ab).sum(2), (ab * ac).sum(2), (ac * ac).sum(2)
    det = g11 * g22 - g12 * g12
    out = np.empty(len(points), F64)
    for s in range(0, len(points), 4096):
        p = np.asarray(points[s:s + 4096], F64)[:, None, :]
        q = p - a
        d1, d2 = (q * ab).sum(2), (q * ac).sum(2)
        u, w = (g22 * d1 - g12 * d2) / det, (g11 * d2 - g12 * d1) / det
        height2 = (q * n).sum(2) ** 2 / (n * n).sum(2)
        edges2 = np.minimum(np.minimum(_segment_distance2(p, a, ab), _segment_distance2(p, a, ac)),
                            _segment_distance2(p, b, c - b))
        inside = (u >= 0) & (w >= 0) & (u + w <= 1)
        out[s:s + 4096] = np.sqrt(np.where(inside, height2, edges2).min(1))
    return out


def winding_number(points, verts, faces):
    """Generalised winding number (fp64, Van Oosterom-Strackee solid angles): 1 inside a closed mesh whose normals
    point outwards, 0 outside."""
    v = np.asarray(verts, F64)
    f = np.asarray(faces, np.int64)
    p = np.asarray(points, F64)[:, None, :]
    a, b, c = v[f[:, 0]][None] - p, v[f[:, 1]][None] - p, v[f[:, 2]][None] - p
    la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
    det = np.einsum('pti,pti->pt', a, np.cross(b, c))
    den = la * lb * lc + np.einsum('pti,pti->pt', a, b) * lc + np.einsum('pti,pti->pt', a, c) * lb \
        + np.einsum('pti,pti->pt', b, c) * la
    return (2.0 * np.arctan2(det, den)).sum(1) / (4.0 * np.pi)


# ---------------------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def needle_tetrahedron(offset=(9.37, 8.61, 3.29)):
    """A thin-based needle with outward normals: the two long edges at the base's 15-degree corners have dihedral
    angles of about 15 degrees.  Fits a 24 x 24 x 32 volume, no vertex on the lattice."""
    base = np.array([[0.0, 0.0, 0.0], [11.0, 0.0, 0.0], [5.5, 5.5 * np.tan(np.radians(15.0)), 0.0]])
    apex = np.array([[5.1, 0.6, 24.0]])
    v = np.concatenate([base, apex]) @ rotation((0.3, 1.0, 0.2), 0.21).T + np.asarray(offset)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v.astype(F32), f


def l_prism(offset=(6.43, 5.71, 4.87), scale=9.3, height=14.6, shear=(0.45, 0.3)):
    """An L-shaped prism extruded along a slanted direction (so some wall-cap edges are sharper than 90 degrees), with
    outward normals and one re-entrant edge.  Fits a 40 x 40 x 28 volume, no vertex on the lattice."""
    poly = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], F64) * scale
    bottom = np.concatenate([poly, np.zeros((6, 1))], 1)
    top = bottom + np.array([shear[0] * height, shear[1] * height, height])
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
    f = [(a, c, b) for a, b, c in cap] + [(a + 6, b + 6, c + 6) for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        f += [(i, j, j + 6), (i, j + 6, i + 6)]
    v = np.concatenate([bottom, top]) @ rotation((0.1, 0.2, 1.0), 0.13).T + np.asarray(offset)
    return v.astype(F32), np.array(f, np.int32)


def dihedral_angles(verts, faces):
    """{(i, j): interior dihedral angle in degrees} of a closed, consistently oriented mesh."""
    v = np.asarray(verts, F64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    owner = {}
    out = {}
    for t, tri in enumerate(f):
        for k in range(3):
            i, j = int(tri[k]), int(tri[(k + 1) % 3])
            if (j, i) in owner:                              # the neighbour runs the edge the other way
                t2 = owner[(j, i)]
                between = np.degrees(np.arccos(np.clip(np.dot(n[t], n[t2]), -1.0, 1.0)))
                convex = np.dot(n[t2], v[int(tri[(k + 2) % 3])] - v[i]) < 0      # t's third vertex lies behind t2
                out[(min(i, j), max(i, j))] = 180.0 - between if convex else 180.0 + between
            owner[(i, j)] = t
    return out


def uv_sphere(centre, radius, nlon, nlat):
    """A closed sphere of 2 * nlon * (nlat - 1) faces with outward normals."""
    c = np.asarray(centre, F64)
    v = [c + [0, 0, radius]]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2 * np.pi * j / nlon
            v.append(c + radius * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    v.append(c - [0, 0, radius])
    south = len(v) - 1
    f = []
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon       # noqa: E731
    for j in range(nlon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        for i in range(1, nlat - 1):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
        f.append((ring(nlat - 1, j), south, ring(nlat - 1, j + 1)))
    return np.array(v, F32), np.array(f, np.int32)
