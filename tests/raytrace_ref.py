"""Independent NumPy restatement of the ray-tracing rules.

Nothing here imports sgnn_amd.raytrace or touches a device.  `closest_ref` and `any_hit` are brute force over all (ray,
face) pairs: every fp32 value is produced by one NumPy operation per rounding in the order section W states, so the
device result, whatever its grid, must match them bit for bit (t, uv) and exactly (face, hit).  The same construction
in fp64 (`dtype=F64`) is the yardstick for the error of fp32 and names the rays that sit on a decision boundary.  The
ray patterns, the rotation of a sweep and the colour mix are restated here as well.
"""
import numpy as np

import meshdist_ref as M

F32 = np.float32
F64 = np.float64


# ---------------------------------------------------------------------------------------------------------
# rule 1: the ray-face test on the record; elementwise on broadcastable (.., 3) arrays of one dtype
# ---------------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def ray_face(o, d, a, ab, ac):
    """det, u, v, t of rule 1 (no decision yet)."""
    one = o.dtype.type(1)
    with np.errstate(all='ignore'):
        p = _cross(d, ac)
        det = _dot(ab, p)
        inv = one / det
        s = o - a
        u = _dot(s, p) * inv
        q = _cross(s, ab)
        v = _dot(d, q) * inv
        t = _dot(ac, q) * inv
    return det, u, v, t


def decide(det, u, v, t, t_min, t_max, cull_back):
    with np.errstate(all='ignore'):
        facing = det > 0 if cull_back else det != 0
        return facing & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min) & (t < t_max)


# ---------------------------------------------------------------------------------------------------------
# rules 2 and 3: brute force
# ---------------------------------------------------------------------------------------------------------
def _usable_rays(o, d):
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def _trace(origins, dirs, verts, faces, t_min, t_max, cull_back, dtype, block):
    """Per ray over all usable faces: (best t, its lowest face, u, v, any hit).  t_max: a scalar or one per ray."""
    o = np.asarray(origins, F32).astype(dtype).reshape(-1, 3)
    d = np.asarray(dirs, F32).astype(dtype).reshape(-1, 3)
    a, ab, ac, usable = M.pack_ref(verts, faces, dtype)
    ids = np.nonzero(usable)[0]
    a, ab, ac = a[ids], ab[ids], ac[ids]
    n = len(o)
    t_min = dtype(F32(t_min))
    t_max = np.broadcast_to(np.asarray(t_max, F32).astype(dtype), (n,))
    best = np.full(n, np.inf, dtype)
    face = np.full(n, -1, np.int64)
    uv = np.zeros((n, 2), dtype)
    ok = _usable_rays(o, d)
    for s0 in range(0, n, block):
        sel = np.nonzero(ok[s0:s0 + block])[0] + s0
        if not len(sel) or not len(ids):
            continue
        det, u, v, t = ray_face(o[sel, None, :], d[sel, None, :], a[None], ab[None], ac[None])
        hit = decide(det, u, v, t, t_min, t_max[sel, None], cull_back)
        t = np.where(hit, t, np.inf)
        k = np.argmin(t, 1)                                                     # first = lowest face index
        row = np.arange(len(sel))
        found = hit[row, k]
        best[sel] = t[row, k]
        face[sel] = np.where(found, ids[k], -1)
        uv[sel, 0] = np.where(found, u[row, k], 0)
        uv[sel, 1] = np.where(found, v[row, k], 0)
    return best, face.astype(np.int32), uv


def closest_ref(origins, dirs, verts, faces, t_min=0.0, t_max=np.inf, cull_back=False, dtype=F32, block=256):
    """(t (R,), face (R,) int32, uv (R, 2)): the smallest t over all usable faces, lowest index among equals; a miss is
    +inf, -1, 0."""
    return _trace(origins, dirs, verts, faces, t_min, t_max, cull_back, dtype, block)


def any_hit(origins, dirs, verts, faces, t_min, t_max, cull_back=False, dtype=F32, block=256):
    """(R,) bool: some usable face is hit within (t_min, t_max[ray])."""
    return _trace(origins, dirs, verts, faces, t_min, t_max, cull_back, dtype, block)[1] >= 0


def occluded_ref(origins, targets, verts, faces, eps=1e-4):
    """scene.occluded: the segment origin -> target, fp32 difference, t in (eps, 1 - eps)."""
    o = np.asarray(origins, F32).reshape(-1, 3)
    d = np.asarray(targets, F32).reshape(-1, 3) - o
    return any_hit(o, d, verts, faces, F32(eps), F32(F32(1.0) - F32(eps)))


def points_ref(origins, dirs, t):
    with np.errstate(all='ignore'):
        p = np.asarray(origins, F32) + np.asarray(t, F32)[:, None] * np.asarray(dirs, F32)
    return np.where(np.isfinite(t)[:, None], p, F32(np.nan)).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# fp64: which rays sit on a decision boundary, and how steeply a ray meets its face
# ---------------------------------------------------------------------------------------------------------
def boundary64(origins, dirs, verts, faces, t_min=0.0, t_max=np.inf, tol=1e-5, block=256):
    """(R,) bool from the fp64 construction: the ray's first face, found with every gate loosened by tol, lies within
    tol of an edge in barycentrics, or within tol of t_min or t_max, or a second face lies within tol of it in t."""
    o = np.asarray(origins, F32).astype(F64).reshape(-1, 3)
    d = np.asarray(dirs, F32).astype(F64).reshape(-1, 3)
    a, ab, ac, usable = M.pack_ref(verts, faces, F64)
    a, ab, ac = a[usable], ab[usable], ac[usable]
    t_min = F64(F32(t_min))
    t_max = np.broadcast_to(np.asarray(t_max, F32).astype(F64), (len(o),))
    near = np.zeros(len(o), bool)
    for s0 in range(0, len(o), block):
        sl = slice(s0, s0 + block)
        det, u, v, t = ray_face(o[sl, None, :], d[sl, None, :], a[None], ab[None], ac[None])
        hi = t_max[sl, None]
        with np.errstate(all='ignore'):
            loose = (det != 0) & (u >= -tol) & (v >= -tol) & (u + v <= 1 + tol) & (t > t_min - tol) & (t < hi + tol)
            first = np.where(loose, t, np.inf).min(1)
            cand = loose & (t <= first[:, None] + tol)
            edge = (np.abs(u) < tol) | (np.abs(v) < tol) | (np.abs(1 - (u + v)) < tol)
            gate = (np.abs(t - t_min) < tol) | (np.abs(t - hi) < tol)
        near[sl] = (cand.sum(1) >= 2) | (cand & (edge | gate)).any(1)
    return near


def incidence_cos(dirs, verts, faces, face):
    """|cos| between each ray and the normal of its face (fp64); NaN where face < 0."""
    d = np.asarray(dirs, F32).astype(F64)
    _, ab, ac, _ = M.pack_ref(verts, faces, F64)
    n = np.cross(ab, ac)[np.maximum(face, 0)]
    with np.errstate(all='ignore'):
        c = np.abs((d * n).sum(1)) / (np.linalg.norm(d, axis=1) * np.linalg.norm(n, axis=1))
    return np.where(face >= 0, c, np.nan)


# ---------------------------------------------------------------------------------------------------------
# ray patterns, sweeps, colours
# ---------------------------------------------------------------------------------------------------------
def lidar_angles(channels, steps, fov_up, fov_down):
    """(elevation per channel, azimuth per step) in radians, fp64."""
    if channels > 1:
        el = np.array([fov_up + (fov_down - fov_up) * c / (channels - 1) for c in range(channels)], F64)
    else:
        el = np.array([0.5 * (fov_up + fov_down)], F64)
    return np.radians(el), np.array([2.0 * np.pi * s / steps for s in range(steps)], F64)


def lidar_dirs_ref(channels=32, steps=1024, fov_up=15.0, fov_down=-25.0):
    el, az = lidar_angles(channels, steps, fov_up, fov_down)
    e, z = np.meshgrid(el, az, indexing='ij')
    return np.stack([np.cos(e) * np.cos(z), np.cos(e) * np.sin(z), np.sin(e)], -1).reshape(-1, 3).astype(F32)


def panorama_angles(h, w):
    """(latitude per row, longitude per column) of the pixel centres, fp64."""
    return (np.pi / 2.0 - np.pi * (np.arange(h) + 0.5) / h), (np.pi - 2.0 * np.pi * (np.arange(w) + 0.5) / w)


def panorama_dirs_ref(h, w):
    lat, lon = panorama_angles(h, w)
    la, lo = np.meshgrid(lat, lon, indexing='ij')
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], -1).reshape(-1, 3).astype(F32)


def camera_dirs_ref(k, hw):
    fx, fy, cx, cy = (F32(x) for x in np.asarray(k, F32).reshape(4))
    h, w = hw
    v, u = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing='ij')
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3).astype(F32)


def sweep_rays(sensor2world, dirs):
    """(origins (S D, 3), world dirs (S D, 3)) of a sweep: pose rotation and translation rounded to fp32, then
    ((R.x dx + R.y dy) + R.z dz) per component."""
    poses = np.asarray(sensor2world, F64).reshape(-1, 4, 4)
    d = np.asarray(dirs, F32)
    rot, org = poses[:, :3, :3].astype(F32), poses[:, :3, 3].astype(F32)
    world = np.stack([(rot[:, None, k, 0] * d[None, :, 0] + rot[:, None, k, 1] * d[None, :, 1])
                      + rot[:, None, k, 2] * d[None, :, 2] for k in range(3)], -1)
    return np.repeat(org[:, None], len(d), 1).reshape(-1, 3), world.reshape(-1, 3).astype(F32)


def colors_ref(face, uv, faces, colors):
    """Rule 6: w = (1 - u) - v, c = (w c0 + u c1) + v c2 in fp32, floor(c + 0.5) clamped to [0, 255]."""
    f = np.asarray(faces, np.int64)[np.maximum(face, 0)]
    c0, c1, c2 = (np.asarray(colors)[f[:, k]].astype(F32) for k in range(3))
    u, v = np.asarray(uv, F32)[:, :1], np.asarray(uv, F32)[:, 1:]
    w = (F32(1.0) - u) - v
    c = np.floor(((w * c0 + u * c1) + v * c2) + F32(0.5))
    return np.where((face >= 0)[:, None], np.clip(c, 0, 255), 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------
def soup_rays(verts, faces, n, seed=0):
    """n rays around a soup: a third start inside its box, a third outside and aimed at it, a third aimed past it."""
    rng = np.random.default_rng(seed)
    lo, hi = M.grid_box(verts, faces)
    lo, hi = lo.astype(F64), hi.astype(F64)
    third = n // 3
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    inside = rng.uniform(lo, hi, (third, 3))
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo)
    out = centre + unit[third:] * rng.uniform(0.8, 1.5, (n - third, 1)) * radius
    at = rng.uniform(lo, hi, (n - third, 3))
    past = rng.normal(size=(n - 2 * third, 3))
    at[third:] = centre + 0.75 * radius * past / np.linalg.norm(past, axis=1, keepdims=True)   # outside the box
    o = np.concatenate([inside, out])
    d = np.concatenate([unit[:third], (at - out) / np.linalg.norm(at - out, axis=1, keepdims=True)])
    d *= rng.uniform(0.5, 2.0, (n, 1))                                # directions are not normalised
    return o.astype(F32), d.astype(F32)


def awkward_rays(grid):
    """Rays that lie in cell-boundary planes, run along grid edges, pass exactly through grid corners, have one or two
    zero components, or cannot hit anything (zero and non-finite directions)."""
    lo, c = grid.lo.astype(np.float64), float(grid.cell)
    n = np.array(grid.dims)
    corner = lambda i, j, k: lo + np.array([i, j, k]) * c  # noqa: E731
    o, d = [], []
    for i in (0, 1, min(2, n[0])):
        o += [corner(i, 0.3, 0.4) - [0, 1, 0], corner(i, 0, 0) - [0, 1, 1], corner(0.2, i, 0.7) - [1, 0, 0]]
        d += [[0, 1, 0], [0, 1, 1], [1, 0, 0.25]]                 # in the plane x = lo + i cell; a diagonal in it; y plane
        o += [corner(i, i, -2), corner(-3, i, i)]
        d += [[0, 0, 1], [2, 0, 0]]                               # along grid edges
        o += [corner(i, i, i) - np.array([1.0, 1.0, 1.0]) * c, corner(0, 0, 0) - np.array([1.0, 2.0, 3.0]) * c]
        d += [[c, c, c], [1.0 * c + i * c, 2.0 * c + i * c, 3.0 * c + i * c]]   # through corners
    o += [corner(1, 1, 1)] * 5
    d += [[1e-30, 0, -1], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 1], [0, -0.0, 0]]   # the last six cannot hit anything
    o += [[np.nan, 0, 0], [np.inf, 0, 0]]
    d += [[1, 0, 0], [-1, 0, 0]]
    return np.array(o, F32), np.array(d, F32)


def enters_ref(origins, dirs, lo, dims, cell, guard, t_min=0.0, t_max=np.inf):
    """(R,) bool: the ray passes the slab test of rule 4 against the grid's box grown by the guard."""
    o, d = np.asarray(origins, F32).reshape(-1, 3), np.asarray(dirs, F32).reshape(-1, 3)
    ok = _usable_rays(o, d)
    t0, t1 = np.full(len(o), F32(t_min)), np.full(len(o), F32(t_max))
    with np.errstate(all='ignore'):
        for k in range(3):
            low, high = F32(lo[k]) - F32(guard), (F32(lo[k]) + F32(dims[k]) * F32(cell)) + F32(guard)
            a, b = (low - o[:, k]) / d[:, k], (high - o[:, k]) / d[:, k]
            flat = d[:, k] == 0
            ok &= ~flat | ((o[:, k] >= low) & (o[:, k] <= high))
            t0 = np.where(flat, t0, np.maximum(t0, np.minimum(a, b)))
            t1 = np.where(flat, t1, np.minimum(t1, np.maximum(a, b)))
    return ok & (t0 <= t1) & np.isfinite(t0)


def room_camera_rays(n, hw, seed=7):
    """The cameras of fusion_ref.room_frames as rays: (intrinsics (n, 4), poses (n, 4, 4), origins, dirs (n h w, 3))."""
    import fusion_ref as R
    k = np.array([0.8 * hw[1], 0.8 * hw[1], (hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0], F32)
    poses = R.room_trajectory(n, seed)
    o, d = sweep_rays(poses, camera_dirs_ref(k, hw))
    return np.tile(k, (n, 1)), poses, o, d


def interior_pixels(face, n, hw):
    """(n h w,) bool: the pixel and its 8 neighbours hit the same face (frame borders are never interior)."""
    f = face.reshape(n, hw[0], hw[1])
    same = np.zeros(f.shape, bool)
    c = f[:, 1:-1, 1:-1]
    ok = c >= 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            ok &= f[:, dy:dy + hw[0] - 2, dx:dx + hw[1] - 2] == c
    same[:, 1:-1, 1:-1] = ok
    return same.reshape(-1)


# ---------------------------------------------------------------------------------------------------------
# rule 4: the grid walk, ray by ray (slow; for a few hundred rays).  Its result must equal closest_ref.
# ---------------------------------------------------------------------------------------------------------
class GuardGrid:
    """meshdist_ref.GridRef's grid with every face listed in the cells of its box grown by guard = cell / 64."""

    def __init__(self, verts, faces, cell):
        v = np.asarray(verts, F32)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        self.a, self.ab, self.ac, usable = M.pack_ref(verts, faces)
        self.lo, hi = M.grid_box(verts, faces)
        self.cell = F32(cell)
        self.guard = F32(F32(1.0 / 64.0) * self.cell)
        self.dims = tuple(int(np.floor(((h - l) / self.cell).astype(F32))) + 1 for l, h in zip(self.lo, hi))
        self.lists = {}
        for t in np.nonzero(usable)[0]:
            tri = v[f[t]]
            r = [range(int(M.cell_of(tri[:, k].min() - self.guard, self.lo[k], self.cell, self.dims[k])),
                       int(M.cell_of(tri[:, k].max() + self.guard, self.lo[k], self.cell, self.dims[k])) + 1)
                 for k in range(3)]
            for z in r[2]:
                for y in r[1]:
                    for x in r[0]:
                        self.lists.setdefault((x, y, z), []).append(t)


def walk_ref(origins, dirs, grid, t_min=0.0, t_max=np.inf, cull_back=False, first=False):
    """(t, face, uv, hit, cells visited, pairs tested) of the walk of rule 4; first=True: any-hit with early exit."""
    o_all, d_all = np.asarray(origins, F32).reshape(-1, 3), np.asarray(dirs, F32).reshape(-1, 3)
    n = len(o_all)
    g, inf = grid, F32(np.inf)
    t_min = F32(t_min)
    t_max = np.broadcast_to(np.asarray(t_max, F32), (n,))
    out_t, out_f, out_uv = np.full(n, inf, F32), np.full(n, -1, np.int32), np.zeros((n, 2), F32)
    out_hit = np.zeros(n, bool)
    cells = pairs = 0
    with np.errstate(all='ignore'):
        for r in range(n):
            o, d = o_all[r], d_all[r]
            if not (np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any() and t_min < t_max[r]):
                continue
            t0, t1, live = t_min, t_max[r], True
            for k in range(3):
                lo, hi = g.lo[k] - g.guard, (g.lo[k] + F32(g.dims[k]) * g.cell) + g.guard
                if d[k] == 0:
                    live = live and bool(o[k] >= lo and o[k] <= hi)
                else:
                    a, b = (lo - o[k]) / d[k], (hi - o[k]) / d[k]
                    t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
            if not (live and t0 <= t1 and np.isfinite(t0)):
                continue
            p = [o[k] if d[k] == 0 else o[k] + t0 * d[k] for k in range(3)]
            if not np.isfinite(p).all():
                continue
            i = [int(M.cell_of(p[k], g.lo[k], g.cell, g.dims[k])) for k in range(3)]
            step = [int(np.sign(d[k])) for k in range(3)]

            def crossing(k):
                if step[k] == 0:
                    return inf
                return ((g.lo[k] + F32(i[k] + (1 if step[k] > 0 else 0)) * g.cell) - o[k]) / d[k]

            nxt = [crossing(k) for k in range(3)]
            best, bf, buv = inf, -1, (F32(0), F32(0))
            while True:
                ids = np.array(g.lists.get(tuple(i), []), np.int64)
                cells += 1
                if len(ids):
                    det, u, v, t = ray_face(o[None], d[None], g.a[ids], g.ab[ids], g.ac[ids])
                    hit = decide(det, u, v, t, t_min, t_max[r], cull_back)
                    if first and hit.any():
                        # the device tests the list in an order of its own; up to its first hit
                        out_hit[r] = True
                        pairs += int(np.argmax(hit)) + 1
                        break
                    pairs += len(ids)
                    for j in np.nonzero(hit)[0]:
                        if t[j] < best or (t[j] == best and ids[j] < bf):
                            best, bf, buv = t[j], int(ids[j]), (u[j], v[j])
                m = 0
                if nxt[1] < nxt[m]:
                    m = 1
                if nxt[2] < nxt[m]:
                    m = 2
                tn = nxt[m]
                if not (tn < t1) or best <= tn:
                    break
                i[m] += step[m]
                if not 0 <= i[m] < g.dims[m]:
                    break
                nxt[m] = crossing(m)
            out_t[r], out_f[r], out_uv[r] = best, bf, buv
    return out_t, out_f, out_uv, out_hit, cells, pairs


# ---------------------------------------------------------------------------------------------------------
# more shared cases: a fine grid under grazing rays, and the LiDAR sweep of the room with its depth discontinuities
# ---------------------------------------------------------------------------------------------------------
def grazing_case(extent, ncell, ntri=400, nray=300, seed=1, cos_lo=0.002, cos_hi=0.1):
    """ntri triangles a few cells large anywhere in [0, extent]^3 (two of them pin the box's corners) and nray rays
    that meet one of them at an incidence cosine in [cos_lo, cos_hi] after 5 to 60 % of the extent:
    (verts, faces, origins, dirs, cell = extent / ncell)."""
    rng = np.random.default_rng(seed)
    cell = extent / ncell
    tri = rng.uniform(0, extent, (ntri, 1, 3)) + rng.normal(size=(ntri, 3, 3)) * cell * 1.5
    tri[0] = [[0, 0, 0], [cell, 0, 0], [0, cell, 0]]
    tri[1] = [[extent, extent, extent], [extent - cell, extent, extent], [extent, extent - cell, extent]]
    verts, faces = tri.reshape(-1, 3).astype(F32), np.arange(3 * ntri, dtype=np.int32).reshape(-1, 3)
    v = verts.astype(F64)[faces[rng.integers(0, ntri, nray)]]
    p = (v * rng.dirichlet([1, 1, 1], nray)[:, :, None]).sum(1)
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    along = (v[:, 1] - v[:, 0]) / np.linalg.norm(v[:, 1] - v[:, 0], axis=1, keepdims=True)
    c = rng.uniform(cos_lo, cos_hi, nray)
    d = along * np.sqrt(1 - c * c)[:, None] + normal * c[:, None]
    o = p - d * (rng.uniform(0.05, 0.6, nray) * extent)[:, None]
    return verts, faces, o.astype(F32), (d * rng.uniform(0.5, 2.0, (nray, 1))).astype(F32), cell


SWEEP_VS, SWEEP_DIMS = 0.05, (92, 76, 64)
SWEEP_BOUND = 1.0 + np.sqrt(3.0) / 2.0      # voxels: how far a band voxel fed by rays of one plane can lie from the mesh
SWEEP_REGION_VOXELS, SWEEP_FAR_VOXELS = 17, 9   # measured by tests/test_raytrace_ref.py: band voxels in the region; beyond
# rasteriser cross-check: the largest |t - depth| between render_ref and closest_ref on the interior pixels of four
# 60 x 80 room frames (13 981 pixels), measured and asserted by tests/test_raytrace_ref.py
MEASURED_RENDER_ERR = 5.3883e-5


def lidar_room_case():
    """One lidar_dirs(16, 256) sweep from the middle of tessellate_room(4), as the restatement sees it: a dict with the
    mesh, the pose, the rays, the brute-force hits, and the 5 cm grid the sweep is fused into."""
    import fusion_ref as R
    import render_ref as RR
    verts, faces = RR.tessellate_room(4)
    pose = np.eye(4)
    pose[:3, 3] = [2.0, 1.6, 1.3]
    pose[:3, :3] = [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]
    dirs = lidar_dirs_ref(16, 256)
    o, d = sweep_rays(pose[None], dirs)
    t, f, uv = closest_ref(o, d, verts, faces, t_min=0.1, t_max=12.0)
    return dict(verts=verts, faces=faces, pose=pose, dirs=dirs, o=o, d=d, t=t, face=f, uv=uv, keep=f >= 0,
                points=points_ref(o, d, t)[f >= 0], origins=pose[None, :3, 3].astype(F32),
                w2g=R.grid_transform((-0.3, -0.3, -0.3), SWEEP_VS))


def discontinuity_voxels(case):
    """(dz, dy, dx) bool: voxels of the sweep's grid that receive samples (section P, rules 5-7, carve=True) of rays
    that hit different planes of the mesh at ranges more than a voxel apart: a true depth discontinuity.  Only there
    can the running mean of section P put a voxel into the surface band away from the mesh: rays that see one plane
    keep a voxel of the band within vs (1 + sqrt(3) / 2) of it (tests/test_raytrace_ref.py)."""
    import points_ref as PR
    vol = PR.Volume(SWEEP_DIMS, SWEEP_VS, case['w2g'])
    pts, hit_face = case['points'], case['face'][case['keep']]
    a, ab, ac, _ = M.pack_ref(case['verts'], case['faces'], F64)
    normal = np.cross(ab, ac)
    axis = np.abs(normal).argmax(1)                                 # the room's faces are axis-aligned
    assert (np.abs(normal).sum(1) == np.abs(normal).max(1)).all()
    plane = axis * 100000 + np.round(a[np.arange(len(a)), axis] * 1000).astype(np.int64)
    R = PR.rays(vol, pts, case['origins'], np.zeros(len(pts), np.int64), True)
    live = np.nonzero(R['n'] > 0)[0]
    cnt = R['n'][live]
    rr = np.repeat(live, cnt)
    n = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    vox = PR.sample_voxels(R, rr, n, np.asarray(vol.w2g, F32), F32(vol.vs) * F32(0.5))
    dx, dy, dz = SWEEP_DIMS
    inside = ((vox >= 0) & (vox < [dx, dy, dz])).all(1)
    rr, vox = rr[inside], vox[inside].astype(np.int64)
    centre = PR.affine(PR.grid2world(vol.w2g), vox.astype(F32))
    pz = PR.dot3(centre - R['o'][rr], R['dir'][rr])
    counted = (R['d'][rr] - pz) > -R['trunc'][rr]                   # rule 7: the samples that enter the sums
    rr, vox = rr[counted], vox[counted]
    lin = (vox[:, 2] * dy + vox[:, 1]) * dx + vox[:, 0]
    planes = np.bincount(np.unique(np.stack([lin, plane[hit_face[rr]]], 1), axis=0)[:, 0], minlength=dx * dy * dz)
    near, far = np.full(dx * dy * dz, np.inf), np.full(dx * dy * dz, -np.inf)
    np.minimum.at(near, lin, R['d'][rr])
    np.maximum.at(far, lin, R['d'][rr])
    return ((planes > 1) & (far - near > SWEEP_VS)).reshape(dz, dy, dx)
