"""TEST INFRASTRUCTURE — plain host restatement of sgnn_amd/csrc/io.hip: the file parser (sgnn_io_layout) and the
three decode kernels (sgnn_io_flag_entries, sgnn_io_emit_entries, sgnn_io_scatter_dense).  numpy only: no torch
device, no call into the library.

Written from the file format in the docstring of sgnn_amd/data.py and the section table of include/sgnn_hip.h
(SGNN_IO_*), not from the kernels:

  * the parser works in Python integers, so no size computation can overflow;
  * the sample of packed entry i is np.searchsorted(seg, i, 'right') - 1, clipped to nb - 1 (not a bisection loop);
  * the value is one np.float32 / np.float32 division, the keep rule |value| < truncation and z < max_z;
  * coordinates are compared as Python-sized integers (int64), so max_z is never narrowed.

Parity status: PINNED — tests/test_io_ref.py checks every function here bit for bit against
tests/golden/data_expected.npz (the reference's own decodes of tests/golden/data) and against oracle/data_oracle.py.
"""
import numpy as np

KIND_CHUNK, KIND_SCENE, KIND_KNOWN = 0, 1, 2
HEADER_BYTES = 92             # u64 dimx, dimy, dimz; f32 voxelsize; f32[16] world2grid
MAX_DIM = 65535
MAX_COUNT = 1 << 40


def _u64(b, at):
    if at + 8 > len(b):
        raise ValueError('truncated: 8-byte count at %d of %d bytes' % (at, len(b)))
    return int.from_bytes(b[at:at + 8], 'little'), at + 8


def _section(b, at, nbytes):
    if at + nbytes > len(b):
        raise ValueError('truncated: %d-byte section at %d of %d bytes' % (nbytes, at, len(b)))
    return at, at + nbytes


def _block(b, at, t, base):
    n, at = _u64(b, at)
    if n > MAX_COUNT:
        raise ValueError('implausible block count %d' % n)
    t[base] = n
    t[base + 1], at = _section(b, at, 12 * n)
    t[base + 2], at = _section(b, at, 4 * n)
    return at


def layout(buf, kind, nbytes=None):
    """The 24-entry section table of one file image (include/sgnn_hip.h, SGNN_IO_*; -1 = section absent) as a list
    of Python integers, or ValueError.  Only the first `nbytes` bytes of `buf` are the file (default: all of it).
    Accepted: dimensions 1..65535 per axis, block counts up to 2^40, a known count equal to the volume, every
    section fully inside the buffer.  Trailing bytes are allowed; entry 21 is the number of bytes consumed."""
    if kind not in (KIND_CHUNK, KIND_SCENE, KIND_KNOWN):
        raise ValueError('unknown kind %r' % (kind,))
    b = np.asarray(buf, dtype=np.uint8).tobytes()
    if nbytes is not None:
        if nbytes < 0:
            raise ValueError('negative length')
        b = b[:nbytes]
    if len(b) < HEADER_BYTES:
        raise ValueError('shorter than the header')
    dx, dy, dz = (int.from_bytes(b[8 * k:8 * k + 8], 'little') for k in range(3))
    if not (1 <= dx <= MAX_DIM and 1 <= dy <= MAX_DIM and 1 <= dz <= MAX_DIM):
        raise ValueError('implausible dimensions %d x %d x %d' % (dx, dy, dz))
    t = [-1] * 24
    t[0], t[1], t[2] = dx, dy, dz
    t[3] = int.from_bytes(b[24:28], 'little')
    t[4] = 28
    at, vol = HEADER_BYTES, dx * dy * dz
    if kind == KIND_CHUNK:
        at = _block(b, at, t, 5)
        at = _block(b, at, t, 8)
        nk, at = _u64(b, at)
        if nk != vol:
            raise ValueError('known count %d != volume %d' % (nk, vol))
        t[11], at = _section(b, at, vol)
        for h in range(3):
            at = _block(b, at, t, 12 + 3 * h)
    elif kind == KIND_SCENE:
        at = _block(b, at, t, 5)
    else:
        t[11], at = _section(b, at, vol)
    t[21] = at
    return t


def header(buf, t):
    """(voxelsize float32, world2grid (4,4) float32) of a parsed file image."""
    b = np.asarray(buf, dtype=np.uint8).tobytes()
    return (np.array([t[3]], dtype=np.uint32).view(np.float32)[0],
            np.frombuffer(b, '<f4', 16, t[4]).reshape(4, 4).copy())


def block(buf, t, base):
    """(locs_xyz uint32 (n,3), raw values float32 (n,)) of the block whose table entries start at `base`."""
    b = np.asarray(buf, dtype=np.uint8).tobytes()
    n = t[base]
    return (np.frombuffer(b, '<u4', 3 * n, t[base + 1]).reshape(n, 3).copy(),
            np.frombuffer(b, '<f4', n, t[base + 2]).copy())


def known(buf, t):
    b = np.asarray(buf, dtype=np.uint8).tobytes()
    return np.frombuffer(b, np.uint8, t[0] * t[1] * t[2], t[11]).reshape(t[2], t[1], t[0]).copy()


def sample_of(seg, n):
    """Sample of each of the n packed entries: seg[s] .. seg[s+1] delimits sample s (empty samples own nothing)."""
    seg = np.asarray(seg, dtype=np.int64)
    nb = len(seg) - 1
    assert nb >= 1 and seg[0] == 0 and seg[-1] == n and np.all(np.diff(seg) >= 0)
    return np.clip(np.searchsorted(seg, np.arange(n, dtype=np.int64), 'right') - 1, None, nb - 1)


def _values(vals, voxelsize, s):
    vals = np.asarray(vals, dtype=np.float32)
    vs = np.asarray(voxelsize, dtype=np.float32)[s]
    with np.errstate(all='ignore'):
        q = vals / vs
    assert q.dtype == np.float32
    return q


def flag(locs_xyz, vals, voxelsize, seg, truncation, max_z):
    """uint8 mask: |vals / voxelsize[sample]| < truncation and z < max_z."""
    locs = np.asarray(locs_xyz, dtype=np.uint32).reshape(-1, 3)
    q = _values(vals, voxelsize, sample_of(seg, len(locs)))
    with np.errstate(invalid='ignore'):
        near = np.abs(q) < np.float32(truncation)
    return (near & (locs[:, 2].astype(np.int64) < int(max_z))).astype(np.uint8)


def emit(locs_xyz, vals, voxelsize, seg, mask):
    """(int64 rows [z, y, x, b], float32 features vals / voxelsize[b]) of the entries with mask != 0, in file order."""
    locs = np.asarray(locs_xyz, dtype=np.uint32).reshape(-1, 3)
    s = sample_of(seg, len(locs))
    keep = np.asarray(mask).astype(bool)
    rows = np.concatenate([locs[:, ::-1].astype(np.int64), s[:, None].astype(np.int64)], 1)
    return rows[keep], _values(vals, voxelsize, s)[keep]


def scatter(locs_xyz, vals, voxelsize, seg, dims, max_z):
    """Dense (nb, d0, d1, d2) float32, pre-filled with -inf, with vals / voxelsize[b] at [b, z, y, x].  Entries
    outside `dims` or at z >= max_z are dropped.

    Out of contract: two entries of one sample that land on the same voxel.  The kernel writes them from different
    threads without an order (a write race), real files never hold any, and this function asserts there are none."""
    locs = np.asarray(locs_xyz, dtype=np.uint32).reshape(-1, 3).astype(np.int64)
    d0, d1, d2 = (int(d) for d in dims)
    nb = len(seg) - 1
    s = sample_of(seg, len(locs))
    q = _values(vals, voxelsize, s)
    x, y, z = locs[:, 0], locs[:, 1], locs[:, 2]
    keep = (z < d0) & (y < d1) & (x < d2) & (z < int(max_z))
    lin = ((s[keep] * d0 + z[keep]) * d1 + y[keep]) * d2 + x[keep]
    assert len(np.unique(lin)) == len(lin), 'duplicate coordinates within a sample are out of contract'
    dense = np.full((nb, d0, d1, d2), -np.inf, dtype=np.float32)
    dense.reshape(-1)[lin] = q[keep]
    return dense
