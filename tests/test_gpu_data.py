"""GPU: DeviceBatchLoader (packed file images decoded by the io kernels) against the reference-decoded
fixtures and, at training sizes, against the data oracle.  Bit-exact: integer coordinates, one float32 division."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import data_oracle  # noqa: E402

from sgnn_amd import data, synth  # noqa: E402

pytestmark = pytest.mark.gpu

DATA = os.path.join(HERE, 'golden', 'data')
CHUNKS = [os.path.join(DATA, 'chunk_%d.sdfs' % i) for i in range(3)]
S_IN = os.path.join(DATA, 'scene_in', 'scene0.sdf')
S_TGT_DIR = os.path.join(DATA, 'scene_tgt')
TRUNC = 3.0


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=True)


def check(b, e, hier_levels):
    assert b['input'][0].is_cuda and b['sdf'].is_cuda and b['known'].is_cuda
    same(b['input'][0], e['locs'])
    same(b['input'][1], e['feats'])
    same(b['sdf'], e['sdf'])
    same(b['known'], e['known'])
    same(b['orig_dims'], e['orig_dims'])
    if hier_levels:
        assert len(b['hierarchy']) == hier_levels
        for h in range(hier_levels):
            same(b['hierarchy'][h], e['hier%d' % h])
    else:
        assert b['hierarchy'] is None


@pytest.fixture(scope='module')
def exp():
    return np.load(os.path.join(HERE, 'golden', 'data_expected.npz'))


def sub(exp, k):
    return {n[len(k):]: exp[n] for n in exp.files if n.startswith(k)}


@pytest.mark.parametrize('levels', [4, 3])
def test_chunk_batch_matches_reference_fixture(exp, levels):
    batches = list(data.DeviceBatchLoader(CHUNKS, 3, TRUNC, num_hierarchy_levels=levels))
    assert len(batches) == 1
    e = sub(exp, 'b%d_' % levels)
    check(batches[0], e, levels - 1)
    same(batches[0]['world2grid'], e['w2g'])
    assert batches[0]['name'] == list(e['names'])


@pytest.mark.parametrize('height', [16, 0, 128])
def test_scene_batch_matches_reference_fixture(exp, height):
    batches = list(data.DeviceBatchLoader([S_IN], 1, TRUNC, max_input_height=height, target_path=S_TGT_DIR))
    assert len(batches) == 1
    check(batches[0], sub(exp, 's%d_' % height), 0)


def test_training_size_batches_match_oracle(tmp_path):
    files = []
    for i in range(10):                      # 64^3 chunks, 2 full batches of 4 + a dropped remainder
        p = str(tmp_path / ('blk%02d.sdfs' % i))
        synth.write_chunk(p, (64, 64, 64), 300 + i, occupancy=0.05, voxelsize=0.02 + 0.001 * (i % 3))
        files.append(p)
    loader = data.DeviceBatchLoader(files, 4, TRUNC)
    assert len(loader) == 2
    for bi, b in enumerate(loader):
        ob = data_oracle.collate([data_oracle.sample_chunk(p, TRUNC, 4) for p in files[4 * bi:4 * bi + 4]])
        same(b['input'][0], ob['input'][0])
        same(b['input'][1], ob['input'][1])
        same(b['sdf'], ob['sdf'])
        same(b['known'], ob['known'])
        same(b['world2grid'], ob['world2grid'])
        for h in range(3):
            same(b['hierarchy'][h], ob['hierarchy'][h])
    assert bi == 1
    # a second pass reuses the pinned staging buffers and yields the same bytes
    again = next(iter(loader))
    ob = data_oracle.collate([data_oracle.sample_chunk(p, TRUNC, 4) for p in files[:4]])
    same(again['input'][0], ob['input'][0])
    same(again['sdf'], ob['sdf'])


def test_loaded_batch_trains(tmp_path):
    """The decoded batch is what train_step consumes (same keys, dtypes, device)."""
    from sgnn_amd import model as M, train
    files = []
    for i in range(2):
        p = str(tmp_path / ('t%d.sdfs' % i))
        synth.write_chunk(p, (32, 32, 32), 900 + i, occupancy=0.08)
        files.append(p)
    batch = next(iter(data.DeviceBatchLoader(files, 2, TRUNC)))
    torch.manual_seed(0)
    net = M.GenModel(8, (32, 32, 32), 1, 16, 16, 4, True, True, 1, 1).cuda()
    opt = train.make_optimizer(net.parameters())
    loss, losses, _ = train.train_step(net, opt, batch, np.ones(5, dtype=np.float32))
    assert np.isfinite(loss.item())


def test_mixed_chunk_sizes_rejected(tmp_path):
    a, b = str(tmp_path / 'a.sdfs'), str(tmp_path / 'b.sdfs')
    synth.write_chunk(a, (16, 16, 16), 1, occupancy=0.2)
    synth.write_chunk(b, (16, 16, 32), 2, occupancy=0.2)
    with pytest.raises(ValueError, match='dimensions'):
        list(data.DeviceBatchLoader([a, b], 2, TRUNC))


# ---- files written at test time: empty blocks, every hierarchy depth, partial batches, buffer reuse, headers ------
EMPTY = (np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.float32))


def write_chunk_with(path, dims, seed, voxelsize=0.0199999, empty=()):
    """A synthetic chunk whose blocks named in `empty` ('input', 'target', 'hier') hold no entry."""
    a = synth.block_arrays(dims, seed, occupancy=0.2, voxelsize=voxelsize)
    pick = lambda key, blk: EMPTY if key in empty else blk
    data.write_train_file(path, a['dims'], a['voxelsize'], a['world2grid'], pick('input', a['input']),
                          pick('target', a['target']), a['known'], [pick('hier', h) for h in a['hierarchy']])
    return path


def host_chunk_batch(files, levels):
    ds = data.SceneDataset(files, 0, TRUNC, levels, 0)
    return data.collate([ds[i] for i in range(len(ds))])


def check_batch(b, ob, host=None):
    """A device batch against the oracle's (numpy) and, where given, the host loader's (torch) batch."""
    for e in [ob] + ([host] if host is not None else []):
        same(b['input'][0], e['input'][0])
        same(b['input'][1], e['input'][1])
        same(b['sdf'], e['sdf'])
        same(b['known'], e['known'])
        same(b['world2grid'], e['world2grid'])
        same(b['orig_dims'], e['orig_dims'])
        assert b['name'] == e['name']
        if e['hierarchy'] is None:
            assert b['hierarchy'] is None
        else:
            assert len(b['hierarchy']) == len(e['hierarchy'])
            for g, w in zip(b['hierarchy'], e['hierarchy']):
                same(g, w)


def oracle_chunk_batch(files, levels):
    return data_oracle.collate([data_oracle.sample_chunk(p, TRUNC, levels) for p in files])


def test_chunk_batch_with_empty_blocks(tmp_path):
    dims = (8, 16, 24)
    files = [write_chunk_with(str(tmp_path / 'in.sdfs'), dims, 1, 0.0199999, ('input',)),
             write_chunk_with(str(tmp_path / 'tgt.sdfs'), dims, 2, 0.03, ('target',)),
             write_chunk_with(str(tmp_path / 'hier.sdfs'), dims, 3, 0.0173, ('hier',)),
             write_chunk_with(str(tmp_path / 'full.sdfs'), dims, 4, 0.0467)]
    ob = oracle_chunk_batch(files, 4)
    col = ob['input'][0][:, 3]
    assert set(col) == {1, 2, 3}                                       # sample 0 has no input row
    assert np.all(np.isinf(ob['sdf'][1])) and all(np.isfinite(ob['sdf'][k]).any() for k in (0, 2, 3))
    assert all(np.all(np.isinf(h[2])) and np.isfinite(h[3]).any() for h in ob['hierarchy'])
    batches = list(data.DeviceBatchLoader(files, 4, TRUNC))
    assert len(batches) == 1
    check_batch(batches[0], ob, host_chunk_batch(files, 4))
    assert batches[0]['sdf'].shape == (4, 1) + dims


def test_chunk_batch_with_no_input_at_all(tmp_path):
    dims = (8, 16, 24)
    files = [write_chunk_with(str(tmp_path / ('e%d.sdfs' % i)), dims, 10 + i, 0.03, ('input',)) for i in range(2)]
    ob = oracle_chunk_batch(files, 4)
    assert ob['input'][0].shape == (0, 4) and ob['input'][1].shape == (0, 1) and np.isfinite(ob['sdf']).any()
    b = next(iter(data.DeviceBatchLoader(files, 2, TRUNC)))
    assert tuple(b['input'][0].shape) == (0, 4) and tuple(b['input'][1].shape) == (0, 1)
    check_batch(b, ob, host_chunk_batch(files, 4))


@pytest.mark.parametrize('levels', [1, 2, 3, 4])
def test_chunk_batch_at_every_hierarchy_depth(tmp_path, levels):
    files = [write_chunk_with(str(tmp_path / ('c%d.sdfs' % i)), (16, 8, 24), 20 + i, 0.02 + 0.0031 * i) for i in range(3)]
    ob = oracle_chunk_batch(files, levels)
    assert len(ob['hierarchy']) == levels - 1
    b = next(iter(data.DeviceBatchLoader(files, 3, TRUNC, num_hierarchy_levels=levels)))
    check_batch(b, ob, host_chunk_batch(files, levels))


def scene_triple(tmp_path, dims, seed, vs_in=0.0199999, vs_tgt=None, knw_dims=None):
    """An input .sdf, a target .sdf and its .knw.  vs_tgt: the target file gets its own voxel size and world2grid;
    knw_dims: the .knw gets dimensions of its own."""
    in_dir, tgt_dir = tmp_path / 'in', tmp_path / 'tgt'
    in_dir.mkdir()
    tgt_dir.mkdir()
    s_in, s_tgt = str(in_dir / 'scene.sdf'), str(tgt_dir / 'scene.sdf')
    a = synth.block_arrays(dims, seed, occupancy=0.2, voxelsize=vs_in)
    t = a if vs_tgt is None else synth.block_arrays(dims, seed, occupancy=0.2, voxelsize=vs_tgt)
    w2g_tgt = t['world2grid'].copy()
    if vs_tgt is not None:
        w2g_tgt[:3, 3] += np.float32(1.25)
    data.write_scene(s_in, dims, a['voxelsize'], a['world2grid'], a['input'])
    data.write_scene(s_tgt, dims, t['voxelsize'], w2g_tgt, t['target'])
    known = t['known'] if knw_dims is None else np.resize(t['known'], knw_dims)
    data.write_known(str(tgt_dir / 'scene.knw'), known.shape, t['voxelsize'], w2g_tgt, known)
    return s_in, s_tgt, str(tgt_dir)


def host_scene_batch(s_in, tgt_dir, levels, height):
    ds = data.SceneDataset([s_in], 0, TRUNC, levels, height, target_path=tgt_dir)
    return data.collate([ds[0]])


@pytest.mark.parametrize('height', [16, 128])
@pytest.mark.parametrize('levels', [1, 2, 3, 4])
def test_scene_batch_at_every_hierarchy_depth(tmp_path, levels, height):
    dims = (21, 18, 27)                                                # a different padded shape at every depth
    s_in, s_tgt, tgt_dir = scene_triple(tmp_path, dims, 30)
    ob = data_oracle.collate([data_oracle.sample_scene(s_in, s_tgt, TRUNC, levels, height)])
    q = 4 * 2 ** (levels - 1)
    want = tuple((d + q - 1) // q * q for d in (min(height, 21), 18, 27))
    assert ob['sdf'].shape == (1, 1) + want
    assert want == {(1, 16): (16, 20, 28), (2, 16): (16, 24, 32), (3, 16): (16, 32, 32), (4, 16): (32, 32, 32),
                    (1, 128): (24, 20, 28), (2, 128): (24, 24, 32), (3, 128): (32, 32, 32), (4, 128): (32, 32, 32)}[
                        (levels, height)]
    b = next(iter(data.DeviceBatchLoader([s_in], 1, TRUNC, num_hierarchy_levels=levels, max_input_height=height,
                                         target_path=tgt_dir)))
    check_batch(b, ob, host_scene_batch(s_in, tgt_dir, levels, height))


def test_partial_final_batch(tmp_path):
    files = [write_chunk_with(str(tmp_path / ('p%d.sdfs' % i)), (16, 16, 16), 40 + i, 0.02 + 0.001 * i) for i in range(5)]
    loader = data.DeviceBatchLoader(files, 2, TRUNC, drop_last=False)
    assert len(loader) == 3 and len(data.DeviceBatchLoader(files, 2, TRUNC)) == 2
    batches = list(loader)
    assert [b['sdf'].shape[0] for b in batches] == [2, 2, 1]
    for k, b in enumerate(batches):
        check_batch(b, oracle_chunk_batch(files[2 * k:2 * k + 2], 4))
    assert len(list(data.DeviceBatchLoader(files, 2, TRUNC))) == 2


def test_buffers_reused_across_small_large_small_batches(tmp_path):
    files = []
    for k, dims in enumerate([(8, 8, 8), (32, 32, 32), (8, 8, 8)]):
        files += [write_chunk_with(str(tmp_path / ('r%d_%d.sdfs' % (k, i))), dims, 50 + 2 * k + i, 0.02 + 0.003 * k)
                  for i in range(2)]
    want = [oracle_chunk_batch(files[2 * k:2 * k + 2], 4) for k in range(3)]
    probe = data.DeviceBatchLoader(files, 2, TRUNC)
    sizes = [probe._stage(files[2 * k:2 * k + 2])[1]['bytes'] for k in range(3)]
    assert sizes[0] < sizes[1] > sizes[2] and sizes[1] > 8 * sizes[0]
    runs = []
    for prefetch, workers in ((1, 1), (3, 3)):
        loader = data.DeviceBatchLoader(files, 2, TRUNC, prefetch=prefetch, workers=workers)
        batches = list(loader)
        assert len(batches) == 3
        for b, ob in zip(batches, want):
            check_batch(b, ob)
        for b, ob in zip(list(loader), want):                          # a second pass over the kept buffers
            check_batch(b, ob)
        runs.append(batches)
    for a, b in zip(*runs):
        for key in ('sdf', 'known', 'world2grid'):
            assert torch.equal(a[key], b[key])
        assert torch.equal(a['input'][0], b['input'][0]) and torch.equal(a['input'][1], b['input'][1])
        assert all(torch.equal(g, h) for g, h in zip(a['hierarchy'], b['hierarchy']))


def differing_headers(tmp_path):
    """A scene triple whose input and target files differ in voxel size and in world2grid."""
    s_in, s_tgt, tgt_dir = scene_triple(tmp_path, (21, 18, 27), 60, vs_in=0.0199999, vs_tgt=0.03)
    lay_in, lay_tgt = data.Layout(data._read(s_in), data.KIND_SCENE), data.Layout(data._read(s_tgt), data.KIND_SCENE)
    assert lay_in.voxelsize != lay_tgt.voxelsize and not np.array_equal(lay_in.world2grid, lay_tgt.world2grid)
    return s_in, s_tgt, tgt_dir, lay_in, lay_tgt


@pytest.mark.parametrize('height', [16, 128])
def test_scene_target_divided_by_its_own_voxel_size(tmp_path, height):
    """Each file's block is divided by that file's voxel size (data_util.py:121-139 runs once per file)."""
    s_in, s_tgt, tgt_dir, lay_in, lay_tgt = differing_headers(tmp_path)
    tv = lay_tgt.block(0)[1]
    assert len(tv) > 100 and np.mean((tv / lay_in.voxelsize).view(np.uint32) != (tv / lay_tgt.voxelsize).view(np.uint32)) > 0.99
    ob = data_oracle.collate([data_oracle.sample_scene(s_in, s_tgt, TRUNC, 4, height)])
    hb = host_scene_batch(s_in, tgt_dir, 4, height)
    assert len(ob['input'][0]) > 100 and np.isfinite(ob['sdf']).sum() > 100
    b = next(iter(data.DeviceBatchLoader([s_in], 1, TRUNC, max_input_height=height, target_path=tgt_dir)))
    for e in (ob, hb):
        same(b['sdf'], e['sdf'])
        same(b['input'][0], e['input'][0])
        same(b['input'][1], e['input'][1])
        same(b['known'], e['known'])


def test_scene_world2grid_is_the_target_files(tmp_path):
    """scene_dataloader.py:70-73: the second load_scene overwrites world2grid, so the batch carries the target's."""
    s_in, s_tgt, tgt_dir, lay_in, lay_tgt = differing_headers(tmp_path)
    hb = host_scene_batch(s_in, tgt_dir, 4, 128)
    b = next(iter(data.DeviceBatchLoader([s_in], 1, TRUNC, max_input_height=128, target_path=tgt_dir)))
    same(b['world2grid'], hb['world2grid'].numpy())
    same(b['world2grid'], data_oracle.sample_scene(s_in, s_tgt, TRUNC, 4, 128)['world2grid'][None])
    same(b['world2grid'][0], lay_tgt.world2grid)


@pytest.mark.parametrize('knw_dims', [(16, 16, 8), (16, 16, 32), (16, 8, 32)])
def test_mismatched_known_volume_rejected(tmp_path, knw_dims):
    """A .knw whose dimensions are not its target's is refused before a byte of the batch is packed ((16,8,32) even
    holds as many voxels as the target)."""
    s_in, s_tgt, tgt_dir = scene_triple(tmp_path, (16, 16, 16), 70, knw_dims=knw_dims)
    loader = data.DeviceBatchLoader([s_in], 1, TRUNC, max_input_height=128, target_path=tgt_dir)
    packed = []
    staging_buffer = loader._staging_buffer

    def recording(nbytes):
        packed.append(nbytes)
        return staging_buffer(nbytes)

    loader._staging_buffer = recording
    with pytest.raises(ValueError, match='dimensions'):
        list(loader)
    assert packed == []
