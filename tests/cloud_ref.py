"""NumPy restatement of INTEGRATION.md section Z (sgnn_amd.cloud): brute-force neighbours in fp32, normals, outlier
means and voxel down-sampling in fp64, written from the text of the rules and not from the kernels.  There is no grid
here: every query is measured against every point.

fp32 expressions are NumPy float32 arrays, every operation rounded once; fp64 ones are Python floats, whose + - * /
and math.sqrt are the correctly rounded IEEE operations, taken in the order the rules write down."""
import math

import numpy as np

F32 = np.float32
EMPTY = np.uint64(2 ** 64 - 1)


def finite_rows(x):
    return np.isfinite(np.asarray(x, F32)).all(1)


def dist2(q, p):
    """(Q, N) fp32: (dx dx + dy dy) + dz dz with dx = q.x - p.x (rule C.1)."""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    with np.errstate(all='ignore'):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        return (dx * dx + dy * dy) + dz * dz


def limit2(max_dist):
    if max_dist is None:
        return F32(np.inf)
    with np.errstate(over='ignore'):
        return F32(max_dist) * F32(max_dist)


def knn(points, queries, k, max_dist=None, chunk=512):
    """(idx (Q, k) int32, d2 (Q, k) fp32).  queries None: the points themselves, each without its own row."""
    points = np.asarray(points, F32).reshape(-1, 3)
    own = queries is None
    queries = points if own else np.asarray(queries, F32).reshape(-1, 3)
    n, nq = len(points), len(queries)
    usable, lim = finite_rows(points), limit2(max_dist)
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), np.inf, F32)
    index = np.arange(n, dtype=np.uint64)
    for q0 in range(0, nq, chunk):
        q = queries[q0:q0 + chunk]
        d2 = dist2(q, points)
        with np.errstate(invalid='ignore'):
            ok = usable[None, :] & finite_rows(q)[:, None] & (d2 <= lim)
        if own:
            ok[np.arange(len(q)), np.arange(q0, q0 + len(q))] = False
        keys = np.where(ok, d2.view(np.uint32).astype(np.uint64) << np.uint64(32) | index[None, :], EMPTY)
        keys = np.sort(keys, axis=1)[:, :k]
        found = keys != EMPTY
        m = keys.shape[1]
        idx[q0:q0 + len(q), :m] = np.where(found, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        out[q0:q0 + len(q), :m] = np.where(found, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return idx, out


def root32(d2):
    """The correctly rounded fp32 root (the fp64 root rounded to fp32 is that)."""
    with np.errstate(invalid='ignore'):
        return np.sqrt(np.asarray(d2, F32).astype(np.float64)).astype(F32)


def nearest(points, queries, max_dist=None):
    idx, d2 = knn(points, queries, 1, max_dist)
    return root32(d2[:, 0]), idx[:, 0]


def radius(points, queries, r):
    """(count (Q,) int32, start (Q+1,) int64, nbr (M,) int32 ascending per query): d2 <= r r, the fp32 product."""
    points, queries = np.asarray(points, F32).reshape(-1, 3), np.asarray(queries, F32).reshape(-1, 3)
    with np.errstate(invalid='ignore'):
        ok = (dist2(queries, points) <= limit2(r)) & finite_rows(points)[None, :] & finite_rows(queries)[:, None]
    count = ok.sum(1).astype(np.int32)
    start = np.zeros(len(queries) + 1, np.int64)
    start[1:] = np.cumsum(count)
    return count, start, np.nonzero(ok)[1].astype(np.int32)


def jacobi(a):
    """Rule C.3 on a = [a00, a01, a02, a11, a12, a22]: (diagonal [3], V columns [3][3]) after five cyclic sweeps."""
    m = [[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]      # v[i][j]: row i, column j
    for _ in range(5):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = m[p][q]
            if apq == 0.0:
                continue
            theta = (m[q][q] - m[p][p]) / (2.0 * apq)
            root = math.sqrt(theta * theta + 1.0)
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + root)
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            m[p][p] = m[p][p] - t * apq
            m[q][q] = m[q][q] + t * apq
            m[p][q] = m[q][p] = 0.0
            arp, arq = m[r][p], m[r][q]
            m[r][p] = m[p][r] = c * arp - s * arq
            m[r][q] = m[q][r] = s * arp + c * arq
            for i in range(3):
                vip, viq = v[i][p], v[i][q]
                v[i][p] = c * vip - s * viq
                v[i][q] = s * vip + c * viq
    return [m[0][0], m[1][1], m[2][2]], v


def covariance(rows):
    """The six fp64 sums of products of rows - centroid, rows in the given order (rule C.3)."""
    rows = [[float(x) for x in r] for r in rows]
    s = list(rows[0])
    for r in rows[1:]:
        s = [s[0] + r[0], s[1] + r[1], s[2] + r[2]]
    m = float(len(rows))
    c = [s[0] / m, s[1] / m, s[2] / m]
    a = [0.0] * 6
    for r in rows:
        dx, dy, dz = r[0] - c[0], r[1] - c[1], r[2] - c[2]
        a = [a[0] + dx * dx, a[1] + dx * dy, a[2] + dx * dz, a[3] + dy * dy, a[4] + dy * dz, a[5] + dz * dz]
    return a


def normal_of(rows, toward=None):
    """(normal [3] fp64 or None, variation fp64, eigenvalues) of one neighbourhood, its own point first."""
    lam, v = jacobi(covariance(rows))
    trace = (lam[0] + lam[1]) + lam[2]
    if not trace > 0.0:
        return None, 0.0, lam
    col = 0
    for j in (1, 2):
        if lam[j] < lam[col]:
            col = j
    n = [v[0][col], v[1][col], v[2][col]]
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [n[0] / length, n[1] / length, n[2] / length]
    if toward is not None:
        t = [float(toward[a]) - float(rows[0][a]) for a in range(3)]
        flip = (n[0] * t[0] + n[1] * t[1]) + n[2] * t[2] < 0.0
    else:
        big = n[0]
        for a in (1, 2):
            if abs(n[a]) > abs(big):
                big = n[a]
        flip = big < 0.0
    if flip:
        n = [-n[0], -n[1], -n[2]]
    return n, max(lam[col], 0.0) / trace, lam


def normals(points, k=16, max_dist=None, toward=None):
    """(normal (N, 3) fp32, variation (N,) fp32, valid (N,) bool) by rule C.3."""
    points = np.asarray(points, F32).reshape(-1, 3)
    n = len(points)
    idx, _ = knn(points, None, k, max_dist)
    normal, variation, valid = np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, bool)
    if toward is not None:
        toward = np.asarray(toward, F32)
    for i in range(n):
        nbr = idx[i][idx[i] >= 0]
        if len(nbr) < 2:
            continue
        tw = None if toward is None else (toward if toward.ndim == 1 else toward[i])
        vec, var, _ = normal_of([points[i]] + [points[j] for j in nbr], tw)
        if vec is not None:
            normal[i], variation[i], valid[i] = np.array(vec, np.float64).astype(F32), F32(var), True
    return normal, variation, valid


def mean_dist(idx, d2):
    """(N,) fp64: the sum over rank order of the fp32 roots, as fp64, over their number; +inf for none (rule C.4)."""
    roots = root32(d2)
    out = np.full(len(idx), np.inf, np.float64)
    for i in range(len(idx)):
        kk = int((idx[i] >= 0).sum())
        if kk:
            s = 0.0
            for u in range(kk):
                s = s + float(roots[i, u])
            out[i] = s / float(kk)
    return out


def voxel_downsample(points, cell, colors=None, normals=None):
    """Rule C.5: (points (C, 3) fp32, colors or None, normals or None, count, first, cell_of), or the string 'range'."""
    points = np.asarray(points, F32).reshape(-1, 3)
    n, cell = len(points), F32(cell)
    ok = finite_rows(points)
    with np.errstate(all='ignore'):
        c = np.floor(points / cell)
    if (np.abs(c[ok]) >= F32(2 ** 20)).any():
        return 'range'
    c = np.where(ok[:, None], c, 0).astype(np.int64) + (2 ** 20 - 1)
    key = c[:, 2] << 42 | c[:, 1] << 21 | c[:, 0]
    members = np.nonzero(ok)[0]
    members = members[np.argsort(key[members], kind='stable')]
    cell_of = np.full(n, -1, np.int32)
    rows, cols, nrms, count, first = [], [], [], [], []
    j = 0
    while j < len(members):
        e = j
        while e < len(members) and key[members[e]] == key[members[j]]:
            e += 1
        run = members[j:e]
        m = len(run)
        s, t = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for i in run:
            s = [s[a] + float(points[i, a]) for a in range(3)]
            if normals is not None:
                t = [t[a] + float(normals[i][a]) for a in range(3)]
        rows.append([s[a] / float(m) for a in range(3)])
        if normals is not None:
            length = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
            nrms.append([t[a] / length for a in range(3)] if length > 0.0 else [0.0, 0.0, 0.0])
        if colors is not None:
            tot = np.asarray(colors)[run].astype(np.int64).sum(0)
            cols.append((2 * tot + m) // (2 * m))
        cell_of[run] = len(count)
        count.append(m)
        first.append(int(run[0]))
        j = e
    nc = len(count)
    return (np.array(rows, np.float64).reshape(nc, 3).astype(F32),
            None if colors is None else np.array(cols, np.int64).reshape(nc, np.shape(colors)[1]).astype(np.uint8),
            None if normals is None else np.array(nrms, np.float64).reshape(nc, 3).astype(F32),
            np.array(count, np.int32), np.array(first, np.int32), cell_of)
