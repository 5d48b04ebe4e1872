"""NumPy restatement of INTEGRATION.md section K (sgnn_amd.simplify): vertex clustering with quadric placement.

Written from the rules, not from the kernels.  Every fp32 and fp64 operation is a NumPy operation on arrays of that
type, one rounding each, in the order section K writes down; the only sums whose order matters, a cluster's sums over
its corners, are taken one corner at a time in ascending corner number.  No GPU, no torch."""
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
CELLS_AXIS = 1 << 21

Simplified = namedtuple('Simplified', 'verts faces colors vertex_map face_map')
Sums = namedtuple('Sums', 'A b s count color o clusters')


class RangeError(Exception):
    """What the device reports as SGNN_STATUS_COORD_RANGE."""


def cells(verts, cell, origin=None):
    """Rule 1: (cell indices (V, 3) int64, origin (3,) fp32)."""
    v = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    if origin is None:
        origin = v.min(0) if len(v) else np.zeros(3, F32)
    origin = np.asarray(origin, dtype=F32).reshape(3)
    with np.errstate(invalid='ignore', over='ignore'):
        c = np.floor((v - origin) / F32(cell))          # fp32 throughout
    if not np.all((c >= 0) & (c < CELLS_AXIS)):         # a NaN fails both comparisons
        raise RangeError('a vertex is not finite or its cell index lies outside [0, 2^21)')
    return c.astype(np.int64), origin


def clusters(c):
    """Rule 2: (cluster number of every vertex (V,), first member of every cluster (C,))."""
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # first occurrence = smallest index
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inverse.reshape(-1)], np.sort(first)


def check_faces(faces, nv):
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= nv):
        raise RangeError('face index out of range [0, %d)' % nv)
    return f


def kept_faces(cf):
    """Rule 6: indices of the faces (in cluster numbers) that stay: three different clusters, and the first face with
    that set of three."""
    ok = np.nonzero((cf[:, 0] != cf[:, 1]) & (cf[:, 0] != cf[:, 2]) & (cf[:, 1] != cf[:, 2]))[0]
    if len(ok) == 0:
        return ok
    _, first = np.unique(np.sort(cf[ok], axis=1), axis=0, return_index=True)
    return ok[np.sort(first)]


def cluster_sums(v, f, vcluster, first, origin, cell, colors=None):
    """Rules 3 and 4 for every cluster: fp64 sums over its corners in ascending corner number."""
    nclust = len(first)
    cd = F64(F32(cell))
    c = np.floor((v[first] - origin) / F32(cell)).astype(F64)                       # the cluster's cell, rule 1 again
    o = origin.astype(F64) + (c + 0.5) * cd                                         # (C, 3)
    corner_vertex = f.reshape(-1)
    corner_cluster = vcluster[corner_vertex]                                        # (3F,)
    oc = o[corner_cluster]                                                          # centre each corner works from
    q = [v[np.repeat(f[:, a], 3)].astype(F64) - oc for a in range(3)]               # its face's p0, p1, p2 minus o
    u, w = q[1] - q[0], q[2] - q[0]
    n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    d = (n0 * q[0][:, 0] + n1 * q[0][:, 1]) + n2 * q[0][:, 2]
    pk = v[corner_vertex].astype(F64) - oc
    terms = np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * d, n1 * d, n2 * d,
                      pk[:, 0], pk[:, 1], pk[:, 2]], 1)
    # sequential sums: step j adds the j-th corner of every cluster that has one
    order = np.argsort(corner_cluster, kind='stable')
    count = np.bincount(corner_cluster, minlength=nclust)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    by_count = np.argsort(-count, kind='stable')                                    # clusters with corners left: a prefix
    left = count[by_count]
    acc = np.zeros((nclust, 12), F64)
    for j in range(int(count.max()) if nclust else 0):
        active = by_count[:np.searchsorted(-left, -j, side='left')]                 # count > j
        acc[active] += terms[order[start[active] + j]]
    color = None
    if colors is not None:
        color = np.zeros((nclust, 3), np.int64)
        np.add.at(color, corner_cluster, np.asarray(colors, dtype=np.int64)[corner_vertex])     # integers: any order
    A = np.stack([acc[:, 0], acc[:, 1], acc[:, 2], acc[:, 1], acc[:, 3], acc[:, 4], acc[:, 2], acc[:, 4], acc[:, 5]],
                 1).reshape(-1, 3, 3)
    return Sums(A, acc[:, 6:9], acc[:, 9:12], count, color, o, np.arange(nclust))


def solve_ldl(M, r):
    """(A + delta I) y = r by L D L^T in the order of rule 5; M (.., 3, 3) symmetric, r (.., 3)."""
    d0 = M[..., 0, 0]
    l10, l20 = M[..., 0, 1] / d0, M[..., 0, 2] / d0
    d1 = M[..., 1, 1] - l10 * M[..., 0, 1]
    u12 = M[..., 1, 2] - l20 * M[..., 0, 1]
    l21 = u12 / d1
    d2 = (M[..., 2, 2] - l20 * M[..., 0, 2]) - l21 * u12
    z1 = r[..., 1] - l10 * r[..., 0]
    z2 = (r[..., 2] - l20 * r[..., 0]) - l21 * z1
    y2 = z2 / d2
    y1 = z1 / d1 - l21 * y2
    y0 = (r[..., 0] / d0 - l10 * y1) - l20 * y2
    return np.stack([y0, y1, y2], -1)


def delta_of(A):
    return (1e-5 * ((A[..., 0, 0] + A[..., 1, 1]) + A[..., 2, 2])) / 3.0


def place(sums, cell, placement):
    """Rule 5: x (C, 3) fp64 relative to the cell centre, for the clusters that have a corner."""
    A, b, s = sums.A, sums.b, sums.s
    cd = F64(F32(cell))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = s / sums.count[:, None].astype(F64)
        if placement == 'mean':
            return m
        assert placement == 'quadric'
        delta = delta_of(A)
        r = np.stack([b[:, i] - ((A[:, i, 0] * m[:, 0] + A[:, i, 1] * m[:, 1]) + A[:, i, 2] * m[:, 2]) for i in range(3)], 1)
        M = A.copy()
        for i in range(3):
            M[:, i, i] = A[:, i, i] + delta
        x = m + solve_ldl(M, r)
        inside = (np.abs(x[:, 0]) <= cd) & (np.abs(x[:, 1]) <= cd) & (np.abs(x[:, 2]) <= cd)
    return np.where(((delta != 0.0) & inside)[:, None], x, m)


def cluster(verts, faces, cell, colors=None, placement='quadric', origin=None):
    """Rules 1 to 6.  Arrays in, arrays out; RangeError where the device raises its status word."""
    v = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    f = check_faces(faces, len(v))
    c, origin = cells(v, cell, origin)
    vcluster, first = clusters(c)
    cf = vcluster[f]
    face_map = kept_faces(cf)
    used = np.zeros(len(first), bool)
    used[cf[face_map].reshape(-1)] = True
    newc = np.full(len(first), -1, np.int64)
    newc[used] = np.arange(int(used.sum()))
    out_c = None
    if used.any():
        sums = cluster_sums(v, f, vcluster, first, origin, cell, colors)
        x = place(sums, cell, placement)
        out_v = (sums.o + x).astype(F32)[used]
        if colors is not None:
            cnt = sums.count[:, None]
            out_c = ((2 * sums.color + cnt) // np.maximum(2 * cnt, 1)).astype(np.uint8)[used]
    else:
        out_v = np.zeros((0, 3), F32)
        if colors is not None:
            out_c = np.zeros((0, 3), np.uint8)
    return Simplified(out_v, newc[cf[face_map]].astype(np.int32).reshape(-1, 3), out_c,
                      newc[vcluster].astype(np.int32), face_map.astype(np.int32))


def count_faces(verts, faces, cell, origin=None):
    """Rule 7's count-only route: rules 1, 2 and 6."""
    v = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    f = check_faces(faces, len(v))
    vcluster, _ = clusters(cells(v, cell, origin)[0])
    return len(kept_faces(vcluster[f]))


def cell_for_faces(verts, faces, target_faces, lo=None, hi=None, iters=16):
    """Rule 7."""
    v = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    if lo is None or hi is None:
        ext = (v.max(0) - v.min(0)).astype(F64)
        diag = float(np.sqrt((ext * ext).sum()))
        lo = diag / 2 ** 20 if lo is None else lo
        hi = diag if hi is None else hi
    lo, hi = float(F32(lo)), float(F32(hi))
    if count_faces(v, faces, hi) >= target_faces:
        return hi
    if count_faces(v, faces, lo) < target_faces:
        raise ValueError('fewer than %d faces even at cell %g' % (target_faces, lo))
    for _ in range(iters):
        mid = float(F32(0.5 * (lo + hi)))
        if mid <= lo or mid >= hi:
            break
        if count_faces(v, faces, mid) >= target_faces:
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------------------------------------
# meshes of the tests
# ---------------------------------------------------------------------------------------------------------
def grid_faces(nu, nv, base=0):
    """Two triangles per quad of an (nu + 1) x (nv + 1) vertex grid numbered u-major."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a = (base + i * (nv + 1) + j).reshape(-1)
    b, c, d = a + 1, a + nv + 1, a + nv + 2
    return np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, d], 1)]).astype(np.int32)


def tilted_plane(n=12):
    """An n x n-quad grid on the plane through p0 spanned by two orthogonal unit-free directions; (verts, faces, p0,
    unit normal fp64)."""
    p0 = np.array([0.25, -0.125, 0.0625])
    e1, e2 = np.array([2.0, 1.0, 0.5]), np.array([-1.0, 2.0, 0.0])             # e1 . e2 = 0
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    pts = p0 + (i.reshape(-1, 1) * e1 + j.reshape(-1, 1) * e2) * (1.0 / 16)
    nrm = np.cross(e1, e2)
    return pts.astype(F32), grid_faces(n, n), p0, nrm / np.linalg.norm(nrm)


def cube_surface(q=8):
    """The surface of the unit cube, q x q quads per side, welded: (verts (V, 3) fp32 on multiples of 1/q, faces)."""
    sides = []
    t = np.arange(q + 1) / q
    a, b = (m.reshape(-1) for m in np.meshgrid(t, t, indexing='ij'))
    for axis in range(3):
        for val in (0.0, 1.0):
            p = np.zeros((len(a), 3))
            p[:, axis] = val
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a, b
            sides.append(p)
    pts = np.concatenate(sides)
    faces = np.concatenate([grid_faces(q, q, k * (q + 1) ** 2) for k in range(6)])
    ids = np.round(pts * q).astype(np.int64)
    _, first, inverse = np.unique(ids, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                                                    # keep first-seen vertex order
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    return pts[first[order]].astype(F32), rank[inverse.reshape(-1)][faces].astype(np.int32)
