"""CPU: tests/io_ref.py (the host restatement of io.hip) pinned to the reference-decoded fixtures and to the data
oracle, and the host parser sgnn_io_layout held to io_ref.layout at every truncation length and on corrupt counts
and dimensions.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

import data_oracle
import io_ref
from sgnn_amd import _lib, data

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, 'golden', 'data')
CHUNKS = [os.path.join(DATA, 'chunk_%d.sdfs' % i) for i in range(3)]
S_IN = os.path.join(DATA, 'scene_in', 'scene0.sdf')
S_TGT = os.path.join(DATA, 'scene_tgt', 'scene0.sdf')
S_KNW = os.path.join(DATA, 'scene_tgt', 'scene0.knw')
TRUNC = 3.0
NOLIMIT = 1 << 40
SGNN_OK, SGNN_EINVAL = 0, -1
KINDS = [io_ref.KIND_CHUNK, io_ref.KIND_SCENE, io_ref.KIND_KNOWN]
BLOCK_BASES = {io_ref.KIND_CHUNK: [5, 8, 12, 15, 18], io_ref.KIND_SCENE: [5], io_ref.KIND_KNOWN: []}


@pytest.fixture(scope='module')
def exp():
    return np.load(os.path.join(HERE, 'golden', 'data_expected.npz'))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=True)


def read(path):
    return np.fromfile(path, dtype=np.uint8)


def seg_of(counts):
    seg = np.zeros(len(counts) + 1, dtype=np.int64)
    seg[1:] = np.cumsum(counts)
    return seg


def decode_chunk(buf):
    """load_train_file's return values (data_util.py:63-117) through io_ref alone."""
    t = io_ref.layout(buf, io_ref.KIND_CHUNK)
    vs, w2g = io_ref.header(buf, t)
    dims = (t[2], t[1], t[0])
    il, iv = io_ref.block(buf, t, 5)
    rows, feats = io_ref.emit(il, iv, [vs], seg_of([len(il)]), np.ones(len(il), np.uint8))
    tl, tv = io_ref.block(buf, t, 8)
    target = io_ref.scatter(tl, tv, [vs], seg_of([len(tl)]), dims, NOLIMIT)[0]
    hier = []
    for h in range(3):
        hl, hv = io_ref.block(buf, t, 12 + 3 * h)
        hier.append(io_ref.scatter(hl, hv, [vs], seg_of([len(hl)]), tuple(d >> (h + 1) for d in dims), NOLIMIT)[0])
    hier.reverse()
    return [rows[:, :3].astype(np.int32), feats], target, list(dims), w2g, io_ref.known(buf, t), hier


def decode_scene(buf):
    t = io_ref.layout(buf, io_ref.KIND_SCENE)
    vs, w2g = io_ref.header(buf, t)
    sl, sv = io_ref.block(buf, t, 5)
    rows, feats = io_ref.emit(sl, sv, [vs], seg_of([len(sl)]), np.ones(len(sl), np.uint8))
    return [rows[:, :3].astype(np.int32), feats], [t[2], t[1], t[0]], w2g


def check_chunk(got, want):
    (il, iv), tgt, dims, w2g, known, hier = got
    (wl, wv), wtgt, wdims, ww2g, wknown, whier = want
    same(il, wl)
    same(iv, wv)
    same(tgt, wtgt)
    assert list(dims) == list(wdims)
    same(w2g, ww2g)
    same(known, wknown)
    assert len(hier) == len(whier) == 3
    for a, b in zip(hier, whier):
        same(a, b)


def test_file_decodes_match_reference_fixture(exp):
    for i, p in enumerate(CHUNKS):
        k = 'c%d_' % i
        check_chunk(decode_chunk(read(p)),
                    ([exp[k + 'in_locs'], exp[k + 'in_vals']], exp[k + 'target'], exp[k + 'dims'], exp[k + 'w2g'],
                     exp[k + 'known'], [exp[k + 'hier%d' % h] for h in range(3)]))
    (sl, sv), sdims, sw2g = decode_scene(read(S_IN))
    same(sl, exp['s_in_locs'])
    same(sv, exp['s_in_vals'])
    assert sdims == list(exp['s_dims'])
    same(sw2g, exp['s_w2g'])
    knw = read(S_KNW)
    same(io_ref.known(knw, io_ref.layout(knw, io_ref.KIND_KNOWN)), exp['s_known'])


@pytest.mark.parametrize('levels', [4, 3])
def test_packed_chunk_batch_matches_reference_fixture(exp, levels):
    """The three fixture chunks packed as one batch, the way the kernels see them."""
    bufs = [read(p) for p in CHUNKS]
    ts = [io_ref.layout(b, io_ref.KIND_CHUNK) for b in bufs]
    vs = np.array([io_ref.header(b, t)[0] for b, t in zip(bufs, ts)], dtype=np.float32)
    k = 'b%d_' % levels

    def packed(base):
        blocks = [io_ref.block(b, t, base) for b, t in zip(bufs, ts)]
        return (np.concatenate([l for l, _ in blocks]), np.concatenate([v for _, v in blocks]),
                seg_of([len(l) for l, _ in blocks]))

    locs, vals, seg = packed(5)
    mask = io_ref.flag(locs, vals, vs, seg, TRUNC, NOLIMIT)
    assert 0 < mask.sum() < len(mask)
    rows, feats = io_ref.emit(locs, vals, vs, seg, mask)
    same(rows, exp[k + 'locs'])
    same(feats[:, None], exp[k + 'feats'])
    locs, vals, seg = packed(8)
    same(io_ref.scatter(locs, vals, vs, seg, (16, 16, 16), NOLIMIT)[:, None], exp[k + 'sdf'])
    hier = []
    for h in range(3):
        locs, vals, seg = packed(12 + 3 * h)
        hier.append(io_ref.scatter(locs, vals, vs, seg, (16 >> (h + 1),) * 3, NOLIMIT)[:, None])
    hier = hier[::-1][4 - levels:]
    for h in range(levels - 1):
        same(hier[h], exp[k + 'hier%d' % h])
    same(np.stack([io_ref.known(b, t) for b, t in zip(bufs, ts)])[:, None], exp[k + 'known'])


@pytest.mark.parametrize('height', [16, 0, 128])
def test_scene_batch_matches_reference_fixture(exp, height):
    """scene_dataloader.py:80-96: the input is clipped at the height only if the scene is taller, the target and the
    known volume always (a height of 0 copies nothing), and every axis is padded to a multiple of 32."""
    k = 's%d_' % height
    b_in, b_tgt, b_knw = read(S_IN), read(S_TGT), read(S_KNW)
    t_in, t_tgt = io_ref.layout(b_in, io_ref.KIND_SCENE), io_ref.layout(b_tgt, io_ref.KIND_SCENE)
    dz, dy, dx = t_tgt[2], t_tgt[1], t_tgt[0]
    clipped = height > 0 and dz > height
    pd = tuple((d + 31) // 32 * 32 for d in ((height if clipped else dz), dy, dx))
    il, iv = io_ref.block(b_in, t_in, 5)
    vs_in, seg = [io_ref.header(b_in, t_in)[0]], seg_of([len(il)])
    mask = io_ref.flag(il, iv, vs_in, seg, TRUNC, height if clipped else NOLIMIT)
    rows, feats = io_ref.emit(il, iv, vs_in, seg, mask)
    same(rows, exp[k + 'locs'])
    same(feats[:, None], exp[k + 'feats'])
    tl, tv = io_ref.block(b_tgt, t_tgt, 5)
    limit = max(0, min(height, dz))
    same(io_ref.scatter(tl, tv, [io_ref.header(b_tgt, t_tgt)[0]], seg_of([len(tl)]), pd, limit)[None],
         exp[k + 'sdf'])
    kpad = np.full(pd, 255, dtype=np.uint8)
    kpad[:limit, :dy, :dx] = io_ref.known(b_knw, io_ref.layout(b_knw, io_ref.KIND_KNOWN))[:limit]
    same(kpad[None, None], exp[k + 'known'])


# ---- files written at test time ------------------------------------------------------------------------------
def _w2g(rng):
    return rng.normal(size=(4, 4)).astype(np.float32)


def _entries(rng, dims_zyx, n, scale=0.2):
    """n distinct voxels of the volume (z,y,x) and values in metres, some beyond any truncation."""
    if n == 0:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.float32)
    vol = int(np.prod(dims_zyx))
    lin = rng.permutation(vol)[:n]
    locs = np.stack(np.unravel_index(lin, dims_zyx), 1).astype(np.int64)
    return locs, (rng.uniform(-scale, scale, len(lin))).astype(np.float32)


def write_small(tmp, kind, dims_zyx=(1, 2, 3), seed=0, voxelsize=0.0199999):
    """One file of a few hundred bytes with a handful of entries per block."""
    rng = np.random.default_rng(seed)
    p = os.path.join(str(tmp), 'small%d_%d' % (kind, seed))
    vol = int(np.prod(dims_zyx))
    if kind == io_ref.KIND_CHUNK:
        hier = [_entries(rng, dims_zyx, c) for c in (2, 0, 1)]       # the hierarchy volumes are not decoded here
        data.write_train_file(p, dims_zyx, voxelsize, _w2g(rng), _entries(rng, dims_zyx, min(5, vol)),
                              _entries(rng, dims_zyx, min(4, vol)), rng.integers(0, 256, dims_zyx), hier)
    elif kind == io_ref.KIND_SCENE:
        data.write_scene(p, dims_zyx, voxelsize, _w2g(rng), _entries(rng, dims_zyx, min(6, vol)))
    else:
        data.write_known(p, dims_zyx, voxelsize, _w2g(rng), rng.integers(0, 256, dims_zyx))
    return read(p)


@pytest.mark.parametrize('seed,dims,vs', [(0, (8, 16, 24), 0.0199999), (1, (5, 3, 7), 0.03), (2, (16, 8, 8), 0.0467)])
def test_decodes_match_data_oracle_on_written_files(tmp_path, seed, dims, vs):
    rng = np.random.default_rng(seed)
    vol = int(np.prod(dims))
    c, s = str(tmp_path / 'c.sdfs'), str(tmp_path / 's.sdf')
    hier = [_entries(rng, tuple(d >> (h + 1) for d in dims), max(0, (vol >> (3 * h + 3)) // 2)) for h in range(3)]
    data.write_train_file(c, dims, vs, _w2g(rng), _entries(rng, dims, vol // 3), _entries(rng, dims, vol // 2),
                          rng.integers(0, 256, dims), hier)
    data.write_scene(s, dims, vs, _w2g(rng), _entries(rng, dims, vol // 4))
    check_chunk(decode_chunk(read(c)), data_oracle.load_train_file(c))
    (sl, sv), sdims, sw2g = decode_scene(read(s))
    (ol, ov), odims, ow2g = data_oracle.load_scene(s)
    same(sl, ol)
    same(sv, ov)
    assert sdims == list(odims)
    same(sw2g, ow2g)


# ---- the host parser against the restatement -------------------------------------------------------------------
def lib_layout(buf, kind, nbytes=None):
    """(return code, 24-entry table, last error) of sgnn_io_layout on an exactly sized array."""
    arr = np.array(buf, dtype=np.uint8)                # a fresh allocation of exactly this many bytes
    out = np.full(24, -12345, dtype=np.int64)
    rc = _lib.query('sgnn_io_layout', arr.ctypes.data, arr.size if nbytes is None else nbytes, kind, out.ctypes.data)
    return rc, [int(v) for v in out], _lib.load().sgnn_last_error().decode()


def agree(buf, kind, nbytes=None):
    """The library and io_ref.layout reach the same verdict on `buf`; returns it (True = accepted)."""
    try:
        want = io_ref.layout(buf, kind, nbytes)
    except ValueError:
        want = None
    rc, got, err = lib_layout(buf, kind, nbytes)
    if want is None:
        assert rc == SGNN_EINVAL and err != '', (kind, len(buf), nbytes, rc, got, err)
        return False
    assert rc == SGNN_OK and got == want, (kind, len(buf), nbytes, rc, got, want)
    return True


@pytest.mark.parametrize('kind', KINDS)
def test_parser_agrees_at_every_prefix_length(tmp_path, kind):
    raw = write_small(tmp_path, kind)
    assert 92 < raw.size < 1000
    full = io_ref.layout(raw, kind)
    assert full[21] == raw.size and (full[0], full[1], full[2]) == (3, 2, 1)
    if kind != io_ref.KIND_KNOWN:
        assert all(full[b] >= 0 for b in BLOCK_BASES[kind]) and full[5] > 0
    for tail in (0, 1, 7):
        junk = np.zeros(tail, dtype=np.uint8)          # zeros: a count read from them is a valid empty block
        accepted = [k for k in range(raw.size + 1) if agree(np.concatenate([raw[:k], junk]), kind)]
        assert raw.size in accepted
        if tail == 0:
            assert accepted == [raw.size], accepted    # every proper prefix is a truncated file
        else:                                          # the junk can only stand in for the last bytes of the file
            assert all(k >= raw.size - tail for k in accepted), accepted
        assert io_ref.layout(np.concatenate([raw, junk]), kind)[21] == raw.size


def _patch_u64(raw, off, value):
    out = raw.copy()
    out[off:off + 8] = np.frombuffer(int(value).to_bytes(8, 'little'), dtype=np.uint8)
    return out


@pytest.mark.parametrize('kind', [io_ref.KIND_CHUNK, io_ref.KIND_SCENE])
def test_parser_agrees_on_corrupt_counts(tmp_path, kind):
    raw = write_small(tmp_path, kind)
    t = io_ref.layout(raw, kind)
    for base in BLOCK_BASES[kind]:
        count_off = t[base + 1] - 8
        assert int.from_bytes(raw[count_off:count_off + 8].tobytes(), 'little') == t[base]
        for value in (2 ** 40, 2 ** 40 + 1, 2 ** 61, 2 ** 63, 2 ** 64 - 1):
            assert not agree(_patch_u64(raw, count_off, value), kind)
    assert agree(raw, kind)


def test_parser_agrees_on_known_count(tmp_path):
    raw = write_small(tmp_path, io_ref.KIND_CHUNK, dims_zyx=(2, 3, 4))
    t = io_ref.layout(raw, io_ref.KIND_CHUNK)
    vol = 24
    off = t[11] - 8
    assert int.from_bytes(raw[off:off + 8].tobytes(), 'little') == vol
    for value in (vol - 1, vol + 1, 2 ** 63 + vol, 2 ** 64 - 1):
        assert not agree(_patch_u64(raw, off, value), io_ref.KIND_CHUNK)
    assert agree(_patch_u64(raw, off, vol), io_ref.KIND_CHUNK)


@pytest.mark.parametrize('kind', KINDS)
def test_parser_agrees_on_dimensions(tmp_path, kind):
    raw = write_small(tmp_path, kind)
    for axis in range(3):
        for value, ok_for_scene in ((65535, True), (65536, False), (0, False), (2 ** 63, False)):
            verdict = agree(_patch_u64(raw, 8 * axis, value), kind)
            # a scene's sections do not depend on its volume; a chunk or a known mask of 6 voxels cannot hold 65535
            assert verdict == (ok_for_scene and kind == io_ref.KIND_SCENE)
    if kind == io_ref.KIND_KNOWN:                       # a known mask that really is 65535 long, on each axis
        for axis in range(3):
            dims = [1, 1, 1]
            dims[axis] = 65535
            p = str(tmp_path / ('long%d.knw' % axis))
            data.write_known(p, dims, 0.02, np.eye(4), np.arange(65535, dtype=np.uint8).reshape(dims))
            assert agree(read(p), kind)
            assert not agree(read(p)[:-1], kind)


@pytest.mark.parametrize('kind', KINDS)
def test_parser_rejects_bad_kind_and_length(tmp_path, kind):
    raw = write_small(tmp_path, kind)
    assert agree(raw, kind)
    for bad in (-1, 3):
        assert not agree(raw, bad)
    for nbytes in (-1, -raw.size, -2 ** 63):
        assert not agree(raw, kind, nbytes)
    assert not agree(raw, kind, raw.size - 1) and agree(raw, kind, raw.size)
