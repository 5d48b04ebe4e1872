"""Host restatement of sgnn_amd.smooth, written from INTEGRATION.md section Y (rules 1 to 12), not from the kernels:
fp32 with every operation rounded on its own, plain Python loops over the lists.  The kernels must give the same bits.

Also the small meshes the tests share: a flat patch, an icosphere, a subdivided cube, a fan and one mesh of every kind.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
ISOLATED, INTERIOR, BOUNDARY, NONMANIFOLD = 0, 1, 2, 3
BOUNDARIES = ('fixed', 'curve', 'free')

Adjacency = namedtuple('Adjacency', 'start neighbor mult kind')


class RangeError(Exception):
    """What the device reports through a status word: a face index outside [0, V) or a non-finite coordinate."""


# ---------------------------------------------------------------------------------------------------------------------
# rules 1 to 3
# ---------------------------------------------------------------------------------------------------------------------
def contributing(faces, nv):
    """Rule 1: the mask of the faces that contribute.  An index outside [0, nv) raises."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise RangeError('face index out of range')
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def adjacency(faces, nv):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = contributing(f, nv)
    count = {}
    for a, b, c in f[ok].tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            count[(p, q)] = count.get((p, q), 0) + 1
            count[(q, p)] = count.get((q, p), 0) + 1
    pairs = sorted(count)
    start = np.zeros(nv + 1, dtype=np.int64)
    for p, _ in pairs:
        start[p + 1] += 1
    start = np.cumsum(start)
    neighbor = np.array([q for _, q in pairs], dtype=np.int32).reshape(-1)
    mult = np.array([min(count[k], 255) for k in pairs], dtype=np.uint8).reshape(-1)
    kind = np.zeros(nv, dtype=np.uint8)
    for i in range(nv):
        m = mult[start[i]:start[i + 1]]
        kind[i] = ISOLATED if len(m) == 0 else NONMANIFOLD if (m > 2).any() else BOUNDARY if (m == 1).any() else INTERIOR
    return Adjacency(start, neighbor, mult, kind)


def boundary_edges(adj):
    out = []
    for i in range(len(adj.kind)):
        for e in range(adj.start[i], adj.start[i + 1]):
            if adj.mult[e] == 1 and i < adj.neighbor[e]:
                out.append((i, int(adj.neighbor[e])))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# rules 4 to 8
# ---------------------------------------------------------------------------------------------------------------------
def _finite(verts):
    if not np.isfinite(verts).all():
        raise RangeError('a vertex coordinate is not finite')


def _mask(fixed, nv):
    return np.zeros(nv, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(nv)


def step(x, adj, f, boundary, fixed):
    """One umbrella step with factor f over (V, 3) fp32 x: a new array."""
    f = F32(f)
    out = x.copy()
    for i in range(len(x)):
        kind = adj.kind[i]
        if fixed[i] or kind in (ISOLATED, NONMANIFOLD) or (kind == BOUNDARY and boundary == 'fixed'):
            continue
        rim = kind == BOUNDARY and boundary == 'curve'
        s, deg = None, 0
        for e in range(adj.start[i], adj.start[i + 1]):
            if rim and adj.mult[e] != 1:
                continue
            p = x[adj.neighbor[e]]
            s = p.copy() if s is None else s + p          # three fp32 additions, in ascending neighbour order
            deg += 1
        if deg == 0:
            continue
        m = s / F32(deg)
        out[i] = x[i] + f * (m - x[i])
    return out


def _umbrella(verts, faces, iterations, factors, boundary, fixed):
    assert boundary in BOUNDARIES and iterations >= 0
    x = np.array(verts, dtype=F32).reshape(-1, 3)
    adj = faces if isinstance(faces, Adjacency) else adjacency(faces, len(x))
    if iterations > 0 and len(x):
        _finite(x)
    fixed = _mask(fixed, len(x))
    with np.errstate(all='ignore'):
        for _ in range(iterations):
            for f in factors:
                x = step(x, adj, f, boundary, fixed)
    return x


def laplacian(verts, faces, iterations=5, lam=0.5, boundary='curve', fixed=None):
    return _umbrella(verts, faces, iterations, (lam,), boundary, fixed)


def taubin(verts, faces, iterations=10, lam=0.5, mu=-0.53, boundary='curve', fixed=None):
    return _umbrella(verts, faces, iterations, (lam, mu), boundary, fixed)


# ---------------------------------------------------------------------------------------------------------------------
# rules 9 and 10
# ---------------------------------------------------------------------------------------------------------------------
def _cross(a, b, c):
    u, w = b - a, c - a
    return np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], dtype=F32)


def _unit(c, other):
    length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return c / length if length > 0 else other


ZERO = np.zeros(3, dtype=F32)


def _cross_all(x, f, ok):
    out = np.zeros((len(f), 3), dtype=F32)
    for t in np.nonzero(ok)[0]:
        out[t] = _cross(x[f[t, 0]], x[f[t, 1]], x[f[t, 2]])
    return out


def face_normals(verts, faces):
    x = np.array(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        raw = _cross_all(x, f, contributing(f, len(x)))
        return np.array([_unit(c, ZERO) for c in raw], dtype=F32).reshape(-1, 3)


def corner_lists(f, ok, nv):
    """Every vertex's contributing faces in ascending order."""
    lists = [[] for _ in range(nv)]
    for t in np.nonzero(ok)[0]:
        for k in range(3):
            lists[f[t, k]].append(int(t))
    return lists


def vertex_normals(verts, faces):
    x = np.array(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = contributing(f, len(x))
    out = np.zeros((len(x), 3), dtype=F32)
    with np.errstate(all='ignore'):
        raw = _cross_all(x, f, ok)
        for i, faces_i in enumerate(corner_lists(f, ok, len(x))):
            s = ZERO.copy()
            for t in faces_i:
                s = s + raw[t]
            out[i] = _unit(s, ZERO)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rules 11 and 12
# ---------------------------------------------------------------------------------------------------------------------
def filter_normals(n, f, ok, lists, threshold):
    threshold = F32(threshold)
    out = n.copy()
    for i in np.nonzero(ok)[0]:
        ni = n[i]
        s = ZERO.copy()
        for k in range(3):
            earlier = set(f[i, :k].tolist())
            for t in lists[f[i, k]]:
                if earlier & set(f[t].tolist()):
                    continue
                nt = n[t]
                u = ((ni[0] * nt[0] + ni[1] * nt[1]) + ni[2] * nt[2]) - threshold
                w = u * u if u > 0 else F32(0)
                s = s + w * nt
        out[i] = _unit(s, ni)
    return out


def update_vertices(x, f, n, lists, kind, fixed):
    out = x.copy()
    three = F32(3)
    for i in range(len(x)):
        if fixed[i] or kind[i] in (ISOLATED, NONMANIFOLD):
            continue
        s, cnt = ZERO.copy(), 0
        for t in lists[i]:
            nt = n[t]
            if not nt.any():
                continue
            c = ((x[f[t, 0]] + x[f[t, 1]]) + x[f[t, 2]]) / three
            d = c - x[i]
            dot = (nt[0] * d[0] + nt[1] * d[1]) + nt[2] * d[2]
            s = s + nt * dot
            cnt += 1
        if cnt:
            out[i] = x[i] + s / F32(cnt)
    return out


def denoise(verts, faces, normal_iterations=5, vertex_iterations=10, threshold=0.4, fixed=None):
    x = np.array(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = contributing(f, len(x))
    if vertex_iterations == 0 or len(x) == 0:
        return x
    _finite(x)
    kind = adjacency(f, len(x)).kind
    fixed = _mask(fixed, len(x))
    lists = corner_lists(f, ok, len(x))
    with np.errstate(all='ignore'):
        n = np.array([_unit(c, ZERO) for c in _cross_all(x, f, ok)], dtype=F32).reshape(-1, 3)
        for _ in range(normal_iterations):
            n = filter_normals(n, f, ok, lists, threshold)
        for _ in range(vertex_iterations):
            x = update_vertices(x, f, n, lists, kind, fixed)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def grid_faces(nu, nv):
    """Two triangles per cell of an (nu + 1) x (nv + 1) vertex grid numbered i * (nv + 1) + j."""
    out = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * (nv + 1) + j, (i + 1) * (nv + 1) + j, (i + 1) * (nv + 1) + j + 1, i * (nv + 1) + j + 1
            out += [(a, b, c), (a, c, d)]
    return np.array(out, dtype=np.int32)


def flat_patch(nu=6, nv=5, z=2.0, pitch=0.25):
    """(nu + 1) x (nv + 1) vertices on multiples of pitch at height z."""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    verts = np.stack([pitch * i.reshape(-1), pitch * j.reshape(-1), np.full(i.size, z)], 1).astype(F32)
    return verts, grid_faces(nu, nv)


def icosphere(levels=3):
    """The unit icosphere: 10 * 4^levels + 2 vertices, faces counter-clockwise from outside."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v).astype(F32), np.array(f, dtype=np.int32)


def cube_surface(q=8):
    """The surface of the unit cube with q x q quads per side, welded, faces counter-clockwise from outside.
    Returns (verts, faces, on_edge): on_edge marks the vertices of the twelve edges."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, q):
            for i in range(q):
                for j in range(q):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:
                        quad.reverse()
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    grid = np.array(verts)
    on_edge = ((grid == 0) | (grid == q)).sum(1) >= 2
    return (grid / float(q)).astype(F32), np.array(faces, dtype=np.int32), on_edge


def cube_edge_distance(x):
    """fp64 distances of points (N, 3) to the nearest of the twelve edge segments of the unit cube."""
    x = np.asarray(x, dtype=np.float64)
    best = np.full(len(x), np.inf)
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for cu in (0.0, 1.0):
            for cw in (0.0, 1.0):
                along = np.clip(x[:, axis], 0.0, 1.0) - x[:, axis]
                best = np.minimum(best, np.sqrt(along ** 2 + (x[:, u] - cu) ** 2 + (x[:, w] - cw) ** 2))
    return best


def fan(n=70, seed=3):
    """n triangles round vertex 0, closed: the hub has valence n."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang), 0.1 * rng.standard_normal(n)], 1)
    verts = np.concatenate([[[0.03, -0.02, 0.4]], ring]).astype(F32)
    faces = np.array([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)], dtype=np.int32)
    return verts, faces


def kinds_mesh(seed=5):
    """One mesh with every kind: a closed tetrahedron (0-3), an open quad (4-7), three faces on the edge 8-9 (with
    10, 11, 12), an unused vertex (13), two faces with a repeated index and one face given twice (14-16)."""
    verts = np.random.default_rng(seed).uniform(-1.0, 1.0, (17, 3)).astype(F32)
    faces = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3),
                      (4, 5, 6), (4, 6, 7),
                      (8, 9, 10), (8, 9, 11), (9, 8, 12),
                      (4, 4, 5), (13, 5, 13),
                      (14, 15, 16), (14, 15, 16)], dtype=np.int32)
    return verts, faces


KINDS_KIND = [INTERIOR] * 4 + [BOUNDARY] * 4 + [NONMANIFOLD] * 2 + [BOUNDARY] * 3 + [ISOLATED] + [INTERIOR] * 3
KINDS_NEIGHBOR = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2],
                  [5, 6, 7], [4, 6], [4, 5, 7], [4, 6],
                  [9, 10, 11, 12], [8, 10, 11, 12], [8, 9], [8, 9], [8, 9], [],
                  [15, 16], [14, 16], [14, 15]]
KINDS_MULT = [[2, 2, 2]] * 4 + [[1, 2, 1], [1, 1], [2, 1, 1], [1, 1],
                                [3, 1, 1, 1], [3, 1, 1, 1], [1, 1], [1, 1], [1, 1], [],
                                [2, 2], [2, 2], [2, 2]]
KINDS_BOUNDARY_EDGES = [(4, 5), (4, 7), (5, 6), (6, 7), (8, 10), (8, 11), (8, 12), (9, 10), (9, 11), (9, 12)]


def enclosed_volume(verts, faces):
    """fp64 signed volume of a closed mesh."""
    x = np.asarray(verts, dtype=np.float64)
    a, b, c = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
