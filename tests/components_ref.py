"""Host restatement of sgnn_amd.components: NumPy and plain Python only.

Volumes and meshes go through a sequential union-find, sparse rows through a breadth-first search over a set of
coordinates, so the two volume routes do not share code.  Numbering is the rule of section J: component k is the
one with the k-th smallest minimum index.  Results are integers and are compared with np.array_equal.

The hand-written cases of the tests (serpentine, contacts across a tile corner, row ends) are built here too, so
that the CPU tests of this file and the GPU tests use the same inputs.
"""
import itertools
from collections import deque

import numpy as np


def offsets(connectivity, forward=False):
    """(dz, dy, dx) of the 6, 18 or 26 neighbours; forward: only those after (0, 0, 0) in raster order."""
    maxc = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for o in itertools.product((-1, 0, 1), repeat=3):
        c = sum(abs(v) for v in o)
        if 0 < c <= maxc and (not forward or o > (0, 0, 0)):
            out.append(o)
    return out


def offset_class(o):
    """1 face, 2 edge, 3 corner."""
    return sum(abs(v) for v in o)


class _Forest:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)


def _number(forest, members, n):
    """labels (n,) int32 (-1 for non-members) and sizes: members in ascending order, a new root opens the next label."""
    labels = np.full(n, -1, np.int32)
    of_root, sizes = {}, []
    for i in members:
        r = forest.find(i)
        k = of_root.get(r)
        if k is None:
            k = of_root[r] = len(sizes)
            sizes.append(0)
        labels[i] = k
        sizes[k] += 1
    return labels, np.asarray(sizes, np.int64).reshape(-1)


def _axis(o, length):
    return slice(max(0, -o), length - max(0, o)), slice(max(0, o), length + min(0, o))


def label_volume(mask, connectivity=26):
    """mask (Z, Y, X) or (B, Z, Y, X), non-zero = foreground -> labels int32 of that shape, sizes (C,) int64."""
    mask = np.asarray(mask) != 0
    m4 = mask.reshape((-1,) + mask.shape[-3:])
    n = m4.size
    idx = np.arange(n).reshape(m4.shape)
    forest = _Forest(n)
    for oz, oy, ox in offsets(connectivity, forward=True):
        (sz, tz), (sy, ty), (sx, tx) = (_axis(o, length) for o, length in zip((oz, oy, ox), m4.shape[1:]))
        both = m4[:, sz, sy, sx] & m4[:, tz, ty, tx]
        for a, b in zip(idx[:, sz, sy, sx][both].tolist(), idx[:, tz, ty, tx][both].tolist()):
            forest.union(a, b)
    labels, sizes = _number(forest, np.flatnonzero(m4).tolist(), n)
    return labels.reshape(mask.shape), sizes


def foreground(sdf, band):
    """isfinite(sdf) & (|sdf| <= band), band rounded to the volume's precision."""
    sdf = np.asarray(sdf)
    with np.errstate(invalid='ignore'):
        return np.isfinite(sdf) & (np.abs(sdf) <= sdf.dtype.type(band))


def label_sparse(locs, dims_zyx, connectivity=26):
    """locs (N, 3) z, y, x or (N, 4) with the batch last -> labels (N,) int32 in row order, sizes (C,) int64 counting
    distinct voxels.  Breadth-first search from the voxels in (b, z, y, x) order.  A row outside dims raises."""
    locs = np.asarray(locs, np.int64)
    rows = [(int(r[3]) if len(r) == 4 else 0, int(r[0]), int(r[1]), int(r[2])) for r in locs]
    for b, z, y, x in rows:
        if b < 0 or not (0 <= z < dims_zyx[0] and 0 <= y < dims_zyx[1] and 0 <= x < dims_zyx[2]):
            raise ValueError('a row lies outside dims')
    label_of, sizes = {}, []
    cells = set(rows)
    nbrs = offsets(connectivity)
    for start in sorted(cells):
        if start in label_of:
            continue
        k = len(sizes)
        label_of[start] = k
        queue, count = deque([start]), 0
        while queue:
            b, z, y, x = queue.popleft()
            count += 1
            for oz, oy, ox in nbrs:
                c = (b, z + oz, y + oy, x + ox)
                if c in cells and c not in label_of:
                    label_of[c] = k
                    queue.append(c)
        sizes.append(count)
    return np.asarray([label_of[r] for r in rows], np.int32).reshape(-1), np.asarray(sizes, np.int64).reshape(-1)


def label_mesh(nverts, faces):
    """faces (F, 3) -> face_labels (F,) int32, vertex_labels (V,) int32 (-1 = unreferenced), face_sizes, vertex_sizes
    (C,) int64; numbered by the smallest referenced vertex.  A face index outside [0, V) raises."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= nverts):
        raise ValueError('face index out of range')
    forest = _Forest(nverts)
    for a, b, c in faces.tolist():
        forest.union(a, b)
        forest.union(a, c)
    vertex_labels, vertex_sizes = _number(forest, np.unique(faces).tolist(), nverts)
    face_labels = vertex_labels[faces[:, 0]].astype(np.int32) if len(faces) else np.zeros(0, np.int32)
    face_sizes = np.bincount(face_labels, minlength=len(vertex_sizes)).astype(np.int64)
    return face_labels, vertex_labels, face_sizes, vertex_sizes


def select(sizes, min_size=None, keep_largest=None):
    """(C,) bool: sizes >= min_size, and among the keep_largest largest (ties to the lower label); both must hold."""
    sizes = np.asarray(sizes, np.int64)
    keep = np.ones(len(sizes), bool)
    if min_size is not None:
        keep &= sizes >= min_size
    if keep_largest is not None:
        top = np.zeros(len(sizes), bool)
        for k in sorted(range(len(sizes)), key=lambda k: (-int(sizes[k]), k))[:keep_largest]:
            top[k] = True
        keep &= top
    return keep


# ---------------------------------------------------------------------------
# hand-written cases
# ---------------------------------------------------------------------------
def default_shape(tile_zyx):
    """Two full tiles and a ragged remainder on every axis."""
    tz, ty, tx = tile_zyx
    return (2 * tz + 3, 2 * ty + 1, 2 * tx + 5)


def serpentine(shape):
    """The voxels, in path order, of one voxel-wide chain through a (Z, Y, X) volume: along x, one step in y at the
    row end, every other row and every other slice, joined at the ends.  Consecutive entries are face neighbours
    and no other two entries are."""
    nz, ny, nx = shape
    path, x_dir, y_dir = [], 1, 1
    even_rows = list(range(0, ny, 2))
    for z in range(0, nz, 2):
        ys = even_rows if y_dir == 1 else even_rows[::-1]
        for j, y in enumerate(ys):
            xs = range(nx) if x_dir == 1 else range(nx - 1, -1, -1)
            path += [(z, y, x) for x in xs]
            x_end = xs[-1]
            if j + 1 < len(ys):
                path.append((z, y + y_dir, x_end))
            x_dir = -x_dir
        if z + 2 < nz:
            path.append((z + 1, ys[-1], x_end))
            y_dir = -y_dir
    return path


def mask_of(shape, voxels):
    m = np.zeros(shape, np.uint8)
    for v in voxels:
        m[tuple(v)] = 1
    return m


def corner_contacts(tile_zyx):
    """[(offset, two voxels)]: the last voxel of the first tile and that plus each of the 13 forward offsets."""
    a = tuple(t - 1 for t in tile_zyx)
    return [(o, [a, tuple(p + q for p, q in zip(a, o))]) for o in offsets(26, forward=True)]


def no_wrap_cases(shape):
    nz, ny, nx = shape
    return [[(0, 0, nx - 1), (0, 1, 0)], [(0, ny - 1, nx - 1), (1, 0, 0)]]


def strip_mesh(nfaces, seed):
    """A triangle strip, face t = (t, t + 1, t + 2), with its vertex numbering shuffled: (nverts, faces int32)."""
    perm = np.random.default_rng(seed).permutation(nfaces + 2)
    t = np.arange(nfaces)
    return nfaces + 2, perm[np.stack([t, t + 1, t + 2], 1)].astype(np.int32)


def cluster_mesh(nclusters, nloose, seed):
    """Random faces inside disjoint vertex ranges, with nloose vertices that no face uses sprinkled between them:
    (nverts, faces int32, face order shuffled)."""
    rng = np.random.default_rng(seed)
    spans = rng.integers(4, 40, nclusters)
    nverts = int(spans.sum()) + nloose
    used = np.sort(rng.permutation(nverts)[:nverts - nloose])        # the vertex ids that clusters may use
    faces, first = [], 0
    for span in spans:
        ids = used[first:first + span]
        faces.append(ids[rng.integers(0, span, (int(rng.integers(1, 3 * span)), 3))])
        first += span
    faces = np.concatenate(faces).astype(np.int32)
    return nverts, faces[rng.permutation(len(faces))]
