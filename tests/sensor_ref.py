"""Independent NumPy restatement of INTEGRATION.md section V (a depth sensor simulated on rendered frames), and the
two small scenes of its tests.  Nothing here imports sgnn_amd.sensor.  All float arithmetic is fp32 with one rounding
per operation (NumPy rounds every array operation once and never fuses), the draws are uint64 wrap-around arithmetic,
and there is no transcendental function of a random quantity: the device must match every bit.

A model is a dict with the twelve fields of struct sgnn_sensor_model (OFF, DEFAULTS, model()).
"""
import numpy as np

F32 = np.float32
U64 = np.uint64
NINF = F32(-np.inf)

FIELDS = ('lateral_sigma', 'min_depth', 'max_depth', 'baseline', 'cos_min', 'edge_drop', 'drop', 'a0', 'a1', 'a2', 'a3',
          'disparity_quantum')
DEFAULTS = dict(lateral_sigma=0.5, min_depth=0.4, max_depth=6.0, baseline=0.075, cos_min=0.173648178, edge_drop=0.5,
                drop=0.0, a0=0.0012, a1=0.0019, a2=0.4, a3=0.05, disparity_quantum=0.125)
OFF = dict(lateral_sigma=0.0, min_depth=-np.inf, max_depth=np.inf, baseline=0.0, cos_min=0.0, edge_drop=0.0, drop=0.0,
           a0=0.0, a1=0.0, a2=0.0, a3=0.0, disparity_quantum=0.0)
C8 = F32(1.86881243e-05)            # 1 / sqrt(8 (65536^2 - 1) / 12)
C4 = F32(0.00676587503)             # 1 / sqrt(4 (256^2 - 1) / 12)
KEEP_SALT = 0x6b6565705f66726d


def model(base=None, **changes):
    m = dict(DEFAULTS if base is None else base)
    assert set(changes) <= set(FIELDS)
    m.update(changes)
    return {k: F32(m[k]) for k in FIELDS}


# ---------------------------------------------------------------------------------------------------------
# V.1, V.2: draws and sums
# ---------------------------------------------------------------------------------------------------------
def hash64(k):
    """The murmur3 finaliser on a uint64 array, wrap-around."""
    k = np.array(k, dtype=U64)
    with np.errstate(over='ignore'):
        k ^= k >> U64(33)
        k *= U64(0xff51afd7ed558ccd)
        k ^= k >> U64(33)
        k *= U64(0xc4ceb9fe1a85ec53)
        k ^= k >> U64(33)
    return k


def draws(seed, frame_ids, h, w):
    """(4, F, h, w) uint64: stream j at pixel (x, y) of frame id f is hash64(hash64(seed) + ((f h + y) w + x) 4 + j)."""
    f = np.asarray(frame_ids, dtype=U64).reshape(-1, 1, 1)
    y = np.arange(h, dtype=U64).reshape(1, -1, 1)
    x = np.arange(w, dtype=U64).reshape(1, 1, -1)
    with np.errstate(over='ignore'):
        at = hash64(U64(seed)) + ((f * U64(h) + y) * U64(w) + x) * U64(4)
        return np.stack([hash64(at + U64(j)) for j in range(4)])


def sum16(a, b):
    """int64: the sum of the eight 16-bit fields of two draws."""
    s = np.zeros(np.shape(a), np.int64)
    for r in (a, b):
        for k in range(4):
            s += ((r >> U64(16 * k)) & U64(0xffff)).astype(np.int64)
    return s


def sum8(bits):
    """int64: the sum of the four 8-bit fields of the low 32 bits."""
    s = np.zeros(np.shape(bits), np.int64)
    for k in range(4):
        s += ((bits >> U64(8 * k)) & U64(0xff)).astype(np.int64)
    return s


def gauss8(a, b):
    return (sum16(a, b) - 262140).astype(F32) * C8


def gauss4(bits):
    return (sum8(bits) - 510).astype(F32) * C4


def round_away(v):
    """Round half away from zero: the integer part, stepped by one when the fraction (exact) reaches 1/2."""
    v = np.asarray(v, F32)
    with np.errstate(invalid='ignore'):
        t = np.trunc(v)
        r = (v - t).astype(F32)
        return np.where(r >= F32(0.5), t + F32(1), np.where(r <= F32(-0.5), t - F32(1), t)).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# V.5: the projector's shadow
# ---------------------------------------------------------------------------------------------------------
def columns(row, fx, baseline):
    """(valid, u) of one row: valid = finite and > 0, u = x - (fx baseline) / z in that order."""
    row = np.asarray(row, F32)
    with np.errstate(all='ignore'):
        valid = np.isfinite(row) & (row > 0)
        fb = F32(fx) * F32(baseline)
        u = (np.arange(row.size).astype(F32) - (fb / row).astype(F32)).astype(F32)
    return valid, u


def shadow_row_literal(row, fx, baseline):
    """The definition read literally, O(w^2)."""
    valid, u = columns(row, fx, baseline)
    out = np.zeros(row.size, bool)
    b = F32(baseline)
    for x in range(row.size):
        if not valid[x] or b == 0:
            continue
        for x2 in range(row.size):
            if valid[x2] and ((b > 0 and x2 > x and u[x2] <= u[x]) or (b < 0 and x2 < x and u[x2] >= u[x])):
                out[x] = True
    return out


def shadow_row_scan(row, fx, baseline):
    """The same as a suffix minimum (baseline > 0) or a prefix maximum (baseline < 0) along the row."""
    valid, u = columns(row, fx, baseline)
    b = F32(baseline)
    if b == 0 or row.size == 0:
        return np.zeros(row.size, bool)
    if b > 0:
        key = np.where(valid, u, F32(np.inf))
        later = np.concatenate([np.minimum.accumulate(key[::-1])[::-1][1:], [F32(np.inf)]])
        return valid & (later <= u)
    key = np.where(valid, u, F32(-np.inf))
    earlier = np.concatenate([[F32(-np.inf)], np.maximum.accumulate(key)[:-1]])
    return valid & (earlier >= u)


def shadow_mask(depth, K, baseline):
    depth = np.asarray(depth, F32)
    out = np.zeros(depth.shape, bool)
    for f in range(depth.shape[0]):
        for y in range(depth.shape[1]):
            out[f, y] = shadow_row_scan(depth[f, y], K[f, 0], baseline)
    return out


# ---------------------------------------------------------------------------------------------------------
# V.3 - V.9: one call
# ---------------------------------------------------------------------------------------------------------
def intrinsics(K, nf):
    K = np.asarray(K, F32)
    return np.ascontiguousarray(np.broadcast_to(K, (nf, 4)))


def incidence(depth, K, sx, sy):
    """(edge, c2) at the source pixels (sx, sy) (F, h, w) of the clean frames (rule V.6)."""
    nf, h, w = depth.shape
    fi = np.arange(nf).reshape(-1, 1, 1)
    fx, fy, cx, cy = (K[:, k].reshape(-1, 1, 1) for k in range(4))
    inner = (sx >= 1) & (sx + 1 < w) & (sy >= 1) & (sy + 1 < h)
    xs, ys = np.clip(sx, 1, max(w - 2, 1)), np.clip(sy, 1, max(h - 2, 1))
    at = lambda dx, dy: depth[fi, np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]      # noqa: E731
    z, dl, dr, du, dd = at(0, 0), at(-1, 0), at(1, 0), at(0, -1), at(0, 1)
    with np.errstate(all='ignore'):
        edge = ~(inner & np.isfinite(dl) & np.isfinite(dr) & np.isfinite(du) & np.isfinite(dd))
        col = lambda i: ((i.astype(F32) - cx) / fx).astype(F32)                                 # noqa: E731
        row = lambda j: ((j.astype(F32) - cy) / fy).astype(F32)                                 # noqa: E731
        xl, xc, xr = col(xs - 1), col(xs), col(xs + 1)
        yu, yc, yd = row(ys - 1), row(ys), row(ys + 1)
        ax, ay, az = xr * dr - xl * dl, yc * dr - yc * dl, dr - dl
        bx, by, bz = xc * dd - xc * du, yd * dd - yu * du, dd - du
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        vx, vy = xc * z, yc * z
        nn = (nx * nx + ny * ny) + nz * nz
        vv = (vx * vx + vy * vy) + z * z
        nv = (nx * vx + ny * vy) + nz * z
        den = nn * vv
        edge |= ~((den > 0) & (den < np.inf))
        c2 = np.where(edge, F32(0), (nv * nv) / den).astype(F32)
    return edge, c2


def degrade(depth, K, m, seed=0, frame_ids=None, stages=None):
    """(F, h, w) fp32: rules V.1 - V.9.  stages: None, or a dict that receives the boolean maps of the pixels each
    stage removed (in rule order; a pixel is charged to the first stage that removes it)."""
    depth = np.asarray(depth, F32)
    nf, h, w = depth.shape
    K = intrinsics(K, nf)
    m = model(m)
    ids = np.arange(nf) if frame_ids is None else np.asarray(frame_ids)
    r = draws(seed, ids, h, w)
    fi = np.arange(nf).reshape(-1, 1, 1)
    ys, xs = np.broadcast_to(np.arange(h).reshape(1, -1, 1), depth.shape), np.broadcast_to(np.arange(w), depth.shape)
    lost = {}
    alive = np.ones(depth.shape, bool)

    def remove(name, gone):
        nonlocal alive
        lost[name] = alive & gone
        alive = alive & ~gone

    with np.errstate(all='ignore'):
        # V.3
        sx, sy = xs, ys
        if m['lateral_sigma'] != 0:
            low, high = r[2] & U64(0xffffffff), r[2] >> U64(32)
            jx = np.clip(round_away(m['lateral_sigma'] * gauss4(low)), -2, 2).astype(np.int64)
            jy = np.clip(round_away(m['lateral_sigma'] * gauss4(high)), -2, 2).astype(np.int64)
            sx, sy = xs + jx, ys + jy
        outside = (sx < 0) | (sx >= w) | (sy < 0) | (sy >= h)
        remove('outside', outside)
        cx_, cy_ = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
        z = depth[fi, cy_, cx_]
        # V.4
        remove('range', ~np.isfinite(z) | (z < m['min_depth']) | (z > m['max_depth']))
        # V.5
        stereo = m['baseline'] != 0
        if stereo:
            remove('shadow', shadow_mask(depth, K, m['baseline'])[fi, cy_, cx_])
        # V.6
        noise = m['a0'] != 0 or m['a1'] != 0
        t = np.zeros(depth.shape, F32)
        if noise or m['cos_min'] > 0 or m['edge_drop'] > 0:
            edge, c2 = incidence(depth, K, cx_, cy_)
            low = r[3] & U64(0xffffffff)
            remove('edge', edge & (low < U64(int(m['edge_drop'] * F32(4294967296.0)))))
            remove('grazing', ~edge & (c2 < m['cos_min'] * m['cos_min']))
            tan2 = ((F32(1) - c2) / c2).astype(F32)
            t = np.where(~edge & (tan2 > 0), tan2, F32(0)).astype(F32)
        # V.7
        remove('dropout', (r[3] >> U64(32)) < U64(int(m['drop'] * F32(4294967296.0))))
        # V.8
        z1 = z
        if noise:
            g = gauss8(r[0], r[1])
            dz = z - m['a2']
            sigma = (m['a0'] + (m['a1'] * dz) * dz) * (F32(1) + m['a3'] * t)
            z1 = (z + sigma * g).astype(F32)
            remove('noise', ~((z1 > 0) & (z1 < np.inf)))
        # V.9
        z2 = z1
        if stereo and m['disparity_quantum'] != 0:
            q = m['disparity_quantum']
            B = (K[:, 0] * np.abs(m['baseline'])).astype(F32).reshape(-1, 1, 1)
            dq = round_away((B / z1) / q) * q
            z2 = (B / dq).astype(F32)
            remove('disparity', ~((dq > 0) & (z2 > 0) & (z2 < np.inf)))
    if stages is not None:
        stages.update(lost)
    return np.where(alive, z2, NINF).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# V.10: frames of an incomplete scan
# ---------------------------------------------------------------------------------------------------------
def frame_draws(n, seed):
    """(n,) fp64 in (0, 1): ((hash64((hash64(seed) ^ salt) + i) >> 12) + 0.5) / 2^52."""
    with np.errstate(over='ignore'):
        base = hash64(U64(seed)) ^ U64(KEEP_SALT)
        bits = hash64(base + np.arange(n, dtype=U64)) >> U64(12)
    return (bits.astype(np.float64) + 0.5) / 2.0 ** 52


def keep_frames(n, chance_drop, seed):
    return np.nonzero(frame_draws(n, seed) > chance_drop)[0].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------
# scenes, built analytically
# ---------------------------------------------------------------------------------------------------------
def camera(h, w):
    """fx, fy, cx, cy of a camera that sees about 60 degrees across w pixels; an odd principal point."""
    f = 0.87 * max(w, 2)
    return np.array([f, 1.03 * f, 0.5 * (w - 1) + 0.25, 0.5 * (h - 1) - 0.25], F32)


def per_frame_cameras(nf, h, w):
    k = np.tile(camera(h, w), (nf, 1))
    k[:, 0] *= 1 + 0.07 * np.arange(nf)
    k[:, 2] += 0.5 * np.arange(nf)
    return k.astype(F32)


def plane_scene(nf, h, w):
    """(depth (F, h, w), K (4,)): a plane tilted about both image axes, at 1.5 m and more, further per frame."""
    K = camera(h, w)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    rx, ry = (x - K[2]) / K[0], (y - K[3]) / K[1]
    frames = []
    for f in range(nf):
        # the plane n . p = d with n = (0.5, -0.3, 1): z = d / (0.5 rx - 0.3 ry + 1)
        frames.append((1.5 + 0.4 * f) / (0.5 * rx - 0.3 * ry + 1.0))
    return np.stack(frames).astype(F32), K


def box_scene(nf, h, w):
    """The plane with a fronto-parallel box at 0.8 m in front of its middle third, and -inf holes: one pixel in four
    of a diagonal band, the first pixel of the first row and the last of the last."""
    depth, K = plane_scene(nf, h, w)
    x0, x1 = w // 3, max(w // 3 + 1, (2 * w) // 3)
    y0, y1 = h // 4, max(h // 4 + 1, (3 * h) // 4)
    depth[:, y0:y1, x0:x1] = F32(0.8)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    holes = ((x + 2 * y) % 11 == 3) & ((x * 7 + y * 3) % 4 == 0)
    depth[:, holes] = NINF
    if h * w > 1:
        depth[:, 0, 0] = NINF
        depth[:, -1, -1] = NINF
    return depth, K


SCENES = {'plane': plane_scene, 'box': box_scene}

# the settings of the bit-for-bit cases: name -> (base, changes)
SETTINGS = {
    'off': (OFF, {}),
    'jitter': (OFF, dict(lateral_sigma=0.5)),
    'jitter_wide': (OFF, dict(lateral_sigma=3.0)),
    'range': (OFF, dict(min_depth=0.9, max_depth=1.9)),
    'shadow': (OFF, dict(baseline=0.075)),
    'shadow_left': (OFF, dict(baseline=-0.075)),
    'edges': (OFF, dict(edge_drop=0.5)),
    'grazing': (OFF, dict(cos_min=0.9)),
    'dropout': (OFF, dict(drop=0.3)),
    'noise': (OFF, dict(a0=0.0012, a1=0.0019, a2=0.4, a3=0.05)),
    'disparity': (OFF, dict(baseline=0.075, disparity_quantum=0.125)),
    'disparity_left': (OFF, dict(baseline=-0.075, disparity_quantum=0.125)),
    'all': (DEFAULTS, {}),
    'all_left': (DEFAULTS, dict(baseline=-0.075)),
    'all_dropout': (DEFAULTS, dict(drop=0.2, edge_drop=1.0)),
}
SHAPES = [(1, 1, 1), (3, 5, 7), (1, 2, 130), (2, 33, 70)]
