"""Independent NumPy restatement of INTEGRATION.md section S (the gravity-aligned room frame of a scan volume).
Nothing here imports sgnn_amd.upright: the surface test, the normals, the cube map, the fixed-point sums, the height
histograms and the host steps (peak, cone means, yaw, levels) have their own code.  All float arithmetic of rules S.1,
S.2, S.4 and S.5 is fp32 with one rounding per operation (NumPy rounds every array operation once and never fuses),
and every result is an integer, so the device must match bit for bit.
"""
import functools
import math

import numpy as np

import points_scenes as PS

F32 = np.float32
FIX = F32(2 ** 20)


# ---------------------------------------------------------------------------------------------------------
# S.1: surface voxels, normals, positions
# ---------------------------------------------------------------------------------------------------------
def surface_voxels(sdf, w2g, band, surface):
    """dict: x, y, z (int64), v, m (N, 3), n (N, 3), all fp32, of the surface voxels in row-major order."""
    sdf = np.asarray(sdf, F32)
    band, surface = F32(band), F32(surface)
    empty = dict(x=np.zeros(0, np.int64), y=np.zeros(0, np.int64), z=np.zeros(0, np.int64), v=np.zeros(0, F32),
                 m=np.zeros((0, 3), F32), n=np.zeros((0, 3), F32))
    if min(sdf.shape) < 3:
        return empty
    c = sdf[1:-1, 1:-1, 1:-1]
    xp, xm = sdf[1:-1, 1:-1, 2:], sdf[1:-1, 1:-1, :-2]
    yp, ym = sdf[1:-1, 2:, 1:-1], sdf[1:-1, :-2, 1:-1]
    zp, zm = sdf[2:, 1:-1, 1:-1], sdf[:-2, 1:-1, 1:-1]
    with np.errstate(invalid='ignore'):
        ok = (np.abs(c) < surface) & (np.abs(c) < band)                    # a NaN or an infinity compares false
        for nb in (xp, xm, yp, ym, zp, zm):
            ok &= np.abs(nb) < band
    z, y, x = np.nonzero(ok)
    g = [(xp[ok] - xm[ok]).astype(F32), (yp[ok] - ym[ok]).astype(F32), (zp[ok] - zm[ok]).astype(F32)]
    M = np.asarray(w2g, F32).reshape(4, 4)[:3, :3]
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        m = [((M[0, k] * g[0] + M[1, k] * g[1]) + M[2, k] * g[2]).astype(F32) for k in range(3)]
        len2 = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]).astype(F32)
    keep = (len2 > 0) & np.isfinite(len2)
    m = np.stack(m, 1)[keep]
    n = (m / np.sqrt(len2[keep])[:, None]).astype(F32)
    return dict(x=x[keep] + 1, y=y[keep] + 1, z=z[keep] + 1, v=c[ok][keep], m=m, n=n)


def grid2world(w2g):
    return np.linalg.inv(np.asarray(w2g, F32).reshape(4, 4).astype(np.float64)).astype(F32)


def positions(s, w2g):
    """(N, 3) fp32: inv(world2grid), rounded once, applied to the voxel indices, rows ((m0 x + m1 y) + m2 z) + m3."""
    g = grid2world(w2g)
    x, y, z = (s[k].astype(F32) for k in 'xyz')
    return np.stack([(((g[r, 0] * x + g[r, 1] * y) + g[r, 2] * z) + g[r, 3]).astype(F32) for r in range(3)], 1)


def dot(n, u):
    u = np.asarray(u, F32)
    return ((n[:, 0] * u[0] + n[:, 1] * u[1]) + n[:, 2] * u[2]).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# S.2, S.4, S.5: the integers
# ---------------------------------------------------------------------------------------------------------
def histogram(sdf, w2g, band, surface, bins):
    m = surface_voxels(sdf, w2g, band, surface)['m']
    out = np.zeros(6 * bins * bins, np.int32)
    if len(m):
        axis = np.argmax(np.abs(m), axis=1)                                # the first of equal maxima
        rows = np.arange(len(m))
        major = m[rows, axis]
        f = 2 * axis + (major < 0)
        cells = []
        for shift in (1, 2):
            a = (m[rows, (axis + shift) % 3] / np.abs(major)).astype(F32)
            i = (((a + F32(1)) * F32(0.5)).astype(F32) * F32(bins)).astype(F32).astype(np.int64)
            cells.append(np.minimum(i, bins - 1))
        np.add.at(out, (f * bins + cells[1]) * bins + cells[0], 1)
    return out.reshape(6, bins, bins)


def fixed(x):
    """llrint(x * 2^20): the fp32 product, then round half to even."""
    return np.rint((x * FIX).astype(F32)).astype(np.int64)


def sums(sdf, w2g, band, surface, records):
    """records: a sequence of (u, e1, e2, cos_cone, sin_wall) or a structured array with those fields -> (B, 8) int64."""
    n = surface_voxels(sdf, w2g, band, surface)['n']
    out = np.zeros((len(records), 8), np.int64)
    for b, rec in enumerate(records):
        u, e1, e2 = (np.asarray(rec[k], F32) for k in (0, 1, 2))
        cos_cone, sin_wall = F32(rec[3]), F32(rec[4])
        if not (np.isfinite(u).all() and np.isfinite(e1).all() and np.isfinite(e2).all() and np.isfinite(cos_cone) and
                np.isfinite(sin_wall)):
            continue
        t = dot(n, u)
        cone = np.abs(t) >= cos_cone
        sg = np.sign(t[cone]).astype(F32)
        for k in range(3):
            out[b, k] = fixed((sg * n[cone, k]).astype(F32)).sum()
        out[b, 3], out[b, 4] = (t[cone] > 0).sum(), (t[cone] < 0).sum()
        wall = np.abs(t) <= sin_wall
        a, bb = dot(n[wall], e1), dot(n[wall], e2)
        r2 = (a * a + bb * bb).astype(F32)
        a, bb, r2 = a[r2 > 0], bb[r2 > 0], r2[r2 > 0]
        r = np.sqrt(r2)
        c, d = (a / r).astype(F32), (bb / r).astype(F32)
        c2, s2 = (c * c - d * d).astype(F32), (F32(2) * (c * d)).astype(F32)
        c4, s4 = (c2 * c2 - s2 * s2).astype(F32), (F32(2) * (s2 * c2)).astype(F32)
        out[b, 5], out[b, 6], out[b, 7] = fixed(c4).sum(), fixed(s4).sum(), len(r2)
    return out


def heights(sdf, w2g, band, surface, up, cos_cone, h0, size, nbins):
    s = surface_voxels(sdf, w2g, band, surface)
    up, cos_cone, h0, size = np.asarray(up, F32), F32(cos_cone), F32(h0), F32(size)
    out = np.zeros((2, nbins), np.int32)
    n, p = s['n'], positions(s, w2g)
    t = dot(n, up)
    q = (p - (s['v'][:, None] * n).astype(F32)).astype(F32)
    with np.errstate(invalid='ignore', over='ignore'):
        k = np.floor(((dot(q, up) - h0).astype(F32) / size).astype(F32))
    inside = (k >= 0) & (k < nbins)
    for row, sel in ((0, t >= cos_cone), (1, t <= -cos_cone)):
        np.add.at(out[row], k[sel & inside].astype(np.int64), 1)
    return out


class Passes(object):
    """The three passes against one volume with the call shapes of the device's, for sgnn_amd.upright.solve."""

    def __init__(self, sdf, w2g, band, surface):
        self.args = (np.asarray(sdf, F32), np.asarray(w2g, F32).reshape(4, 4), F32(band), F32(surface))

    def histogram(self, bins):
        return histogram(*self.args, bins)

    def sums(self, table):
        return sums(*self.args, [(r['u'], r['e1'], r['e2'], r['cos_cone'], r['sin_wall']) for r in table])

    def heights(self, up, cos_cone, h0, size, nbins):
        return heights(*self.args, up, cos_cone, h0, size, nbins)


# ---------------------------------------------------------------------------------------------------------
# S.3 and the host steps of S.4 and S.5 (fp64), written out once more
# ---------------------------------------------------------------------------------------------------------
def centre(index, bins):
    f, rest = divmod(int(index), bins * bins)
    iv, iu = divmod(rest, bins)
    axis = f // 2
    c = np.zeros(3)
    c[axis] = -1.0 if f % 2 else 1.0
    c[(axis + 1) % 3] = (iu + 0.5) / bins * 2.0 - 1.0
    c[(axis + 2) % 3] = (iv + 0.5) / bins * 2.0 - 1.0
    return c / np.linalg.norm(c)


def bin_of(direction, bins):
    """The bin a direction falls in (fp64; for directions away from cell borders)."""
    d = np.asarray(direction, np.float64)
    axis = int(np.argmax(np.abs(d)))
    f = 2 * axis + int(d[axis] < 0)
    cell = [min(bins - 1, int((d[(axis + s) % 3] / abs(d[axis]) + 1.0) * 0.5 * bins)) for s in (1, 2)]
    return (f * bins + cell[1]) * bins + cell[0]


def peak(hist, hint=None, max_tilt=45.0):
    bins = hist.shape[1]
    flat = hist.ravel().astype(np.int64)
    best, best_score = None, 0
    for i in range(flat.size):
        c = centre(i, bins)
        if hint is not None:
            h = np.asarray(hint, np.float64)
            if c @ (h / np.linalg.norm(h)) < math.cos(math.radians(max_tilt)):
                continue
            score = flat[i]
        else:
            score = flat[i] + flat[bin_of(-c, bins)]
        if score > best_score:
            best, best_score = i, score
    return best


def frame(up):
    base = np.array([0.0, 1.0, 0.0]) if abs(up[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = base - (base @ up) * up
    e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(up, e1)


def find(sdf, w2g, vs, hint=None, max_tilt=45.0, cones=(20.0, 10.0, 5.0), wall_tol=10.0, bins=16, min_votes=256,
         floor_share=0.25):
    """dict: peak (the start direction), ups (the axis after every cone), up, votes, yaw, confidence, floor, ceiling; or
    None where rule S.3 finds no bin or a cone is empty."""
    vs = F32(vs)
    band, surface = F32(3.0) * vs, vs
    start = peak(histogram(sdf, w2g, band, surface, bins), hint, max_tilt)
    if start is None:
        return None
    up = centre(start, bins)
    out = dict(peak=up.copy(), ups=[])
    for c in cones:
        e1, e2 = frame(up)
        s = sums(sdf, w2g, band, surface, [(up, e1, e2, math.cos(math.radians(c)), -1.0)])[0]
        if s[3] + s[4] == 0:
            return None
        up = s[:3] / np.linalg.norm(s[:3].astype(np.float64))
        out['ups'].append(up.copy())
    e1, e2 = frame(up)
    cos_last = F32(math.cos(math.radians(cones[-1])))
    s = sums(sdf, w2g, band, surface, [(up, e1, e2, cos_last, math.sin(math.radians(wall_tol)))])[0]
    out.update(up=up, votes=(int(s[3]), int(s[4]), int(s[7])), ok=bool(s[3] + s[4] >= min_votes))
    out['confidence'] = math.hypot(s[5], s[6]) / (max(int(s[7]), 1) * float(FIX))
    out['yaw_ok'] = bool(s[7] >= min_votes and out['confidence'] >= 0.2)
    out['yaw'] = math.atan2(s[6], s[5]) / 4.0 if out['yaw_ok'] else 0.0
    out['x'] = math.cos(out['yaw']) * e1 + math.sin(out['yaw']) * e2
    # S.5: the range of the 8 grid corners along up, bins of half a voxel
    g = grid2world(w2g).astype(np.float64)
    dz, dy, dx = np.asarray(sdf).shape
    hs = [(g[:3, :3] @ np.array([i, j, k], np.float64) + g[:3, 3]) @ up
          for i in (0, dx - 1) for j in (0, dy - 1) for k in (0, dz - 1)]
    size = vs * F32(0.5)
    while math.ceil((max(hs) - min(hs)) / float(size)) + 5 > 4096:
        size = size * F32(2)
    nbins = int(math.ceil((max(hs) - min(hs)) / float(size)) + 5)
    h0 = F32(min(hs) - 2.0 * float(size))
    rows = heights(sdf, w2g, band, surface, up.astype(F32), cos_last, h0, size, nbins)

    def refine(row, k):
        ks = [j for j in (k - 1, k, k + 1) if 0 <= j < nbins]
        w = np.array([row[j] for j in ks], np.float64)
        return float(((float(h0) + (np.array(ks) + 0.5) * float(size)) * w).sum() / w.sum())

    out['floor'] = out['ceiling'] = None
    if rows[0].max() > 0:
        out['floor'] = refine(rows[0], int(np.nonzero(rows[0] >= floor_share * rows[0].max())[0][0]))
    if rows[1].max() > 0:
        out['ceiling'] = refine(rows[1], int(np.nonzero(rows[1] >= floor_share * rows[1].max())[0][-1]))
    if out['floor'] is not None and out['ceiling'] is not None and out['ceiling'] <= out['floor']:
        out['ceiling'] = None
    out['height_rows'] = rows
    return out


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = (a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


# ---------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------
VS = F32(0.05)
ROOM_TILT = PS.rotation((0.3, -0.5, 0.8), 0.45)         # room frame -> world: the true up is its third column
ROOM_PAD = 4
ROOM_HINT_OFF = 20.0                                    # degrees between the hint of the tests and the true up


def box_distance(p, lo, hi):
    """Signed distance of points p (.., 3) to the box [lo, hi], positive outside."""
    q = np.maximum(lo - p, p - hi)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def analytic_sdf(world_pts, vs=VS, tilt=ROOM_TILT, box=True):
    """The room of points_scenes (ROOM_EXT, ROOM_BOX) standing tilted in the world: the smaller of the distance to the
    walls (positive inside the room) and to the box, clamped at 3 voxels in free space, -inf (never seen) more than 3
    voxels behind a surface."""
    r = np.asarray(world_pts, np.float64) @ tilt                            # world -> room: the transpose applied
    d = -box_distance(r, np.zeros(3), np.array(PS.ROOM_EXT))
    if box:
        d = np.minimum(d, box_distance(r, np.array(PS.ROOM_BOX[0]), np.array(PS.ROOM_BOX[1])))
    t = 3.0 * float(vs)
    return np.where(d < -t, -np.inf, np.minimum(d, t)).astype(F32)


@functools.lru_cache(maxsize=None)
def room_scene():
    """(sdf (Z, Y, X) fp32, world2grid (4, 4) fp32, dims_xyz, true up, true wall axes (2, 3)): an axis-aligned grid of
    5 cm voxels around the tilted room, ROOM_PAD voxels of margin; the grid origin falls 0.37 of a voxel off the
    lattice so that no wall passes through voxel centres."""
    vs = float(VS)
    corners = np.array([[(c >> a & 1) * PS.ROOM_EXT[a] for a in range(3)] for c in range(8)]) @ ROOM_TILT.T
    lo = np.floor(corners.min(0) / vs) - ROOM_PAD + 0.37
    dims = tuple(int(v) for v in np.ceil(corners.max(0) / vs) + ROOM_PAD - np.floor(lo) + 1)
    w2g = np.eye(4)
    w2g[:3, :3] /= vs
    w2g[:3, 3] = -lo
    w2g = w2g.astype(F32)
    k, j, i = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims[::-1]), indexing='ij')
    world = (np.stack([i, j, k], -1) + lo) * vs
    return analytic_sdf(world), w2g, dims, ROOM_TILT[:, 2].copy(), ROOM_TILT[:, :2].T.copy()


def room_hint():
    """A unit vector ROOM_HINT_OFF degrees off the true up."""
    up, side = ROOM_TILT[:, 2], ROOM_TILT[:, 0]
    a = math.radians(ROOM_HINT_OFF)
    return math.cos(a) * up + math.sin(a) * side


def wall_error_deg(x_axis, walls):
    """The angle between a horizontal axis and the nearest of the four wall directions."""
    return min(angle_deg(x_axis, s * w) for w in walls for s in (1.0, -1.0))


def small_volume(dims_xyz, w2g, seed=0):
    """A volume for the bit-for-bit tests, in voxel units with band 3 and surface 1: a skew plane, a sphere, an
    axis-aligned plane (two exact zeros in g) and a 45-degree plane (a tie for the major axis), fp32 noise on top, then
    holes (-inf), +inf and NaN voxels, neighbours at exactly +-band and centres at exactly +-surface."""
    dx, dy, dz = dims_xyz
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in (dz, dy, dx)), indexing='ij')
    skew = (0.31 * x - 0.52 * y + 0.79 * z) / math.sqrt(0.31 ** 2 + 0.52 ** 2 + 0.79 ** 2) - 0.3 * dz
    ball = np.sqrt((x - 0.6 * dx) ** 2 + (y - 0.5 * dy) ** 2 + (z - 0.5 * dz) ** 2) - 0.3 * min(dims_xyz)
    d = np.minimum(skew, ball) + rng.normal(0, 0.02, x.shape)
    d = np.where(x < dx // 3, z - (dz // 2), d)                             # exact integers: g = (0, 0, 2)
    d = np.where((x >= dx // 3) & (x < dx // 2), (y - z) * 0.5, d)          # exact halves: g = (0, 1, -1)
    sdf = np.clip(d, -3.0, 3.0).astype(F32)
    flat = sdf.ravel()
    pick = rng.permutation(flat.size)
    n = max(flat.size // 40, 1)
    if flat.size >= 1000:                                                   # (3, 3, 3) keeps its one interior voxel
        for j, value in enumerate((-np.inf, np.inf, np.nan, 3.0, -3.0, 1.0, -1.0)):
            flat[pick[j * n:(j + 1) * n]] = value
    return flat.reshape(dz, dy, dx)


def floor_layer_share(sdf, w2g, vs, up=(0.0, 0.0, 1.0), below=0.2):
    """Of the up-facing surface voxels (n . up >= cos 5 degrees) of a volume whose height along up is under `below`
    (the floor, not the top of the box), the share that lies in the two adjacent z layers of the grid holding the
    most, and their number."""
    s = surface_voxels(sdf, w2g, F32(3.0) * F32(vs), F32(vs))
    sel = (dot(s['n'], up) >= F32(math.cos(math.radians(5.0)))) & (dot(positions(s, w2g), up) < F32(below))
    layers = np.bincount(s['z'][sel], minlength=int(np.asarray(sdf).shape[0]) + 1)
    pair = layers[:-1] + layers[1:]
    return float(pair.max()) / max(int(sel.sum()), 1), int(sel.sum())
