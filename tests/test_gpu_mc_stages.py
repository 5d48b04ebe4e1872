"""GPU: marching cubes stage by stage (csrc/mc.hip: k_mc_count, k_mc_scan, k_mc_emit) on the stage cases of
tests/mc_cases.py: volumes in which every cube configuration occurs, one whose block sums take three rounds of the scan,
non-finite voxels, odd extents and parameters, volumes without an interior voxel, non-contiguous inputs.

Three comparisons, all bit for bit: the per-voxel triangle counts and their total against a vectorised host
classification (mc_cases.cube_table); the triangle soup against oracle/mc_oracle.triangle_soup, which
tests/test_oracle_mc.py pins to the reference's extension on these very volumes; the final mesh against that
extension's stored output (tests/golden/mc_stage_expected.npz).  A mismatch names the voxel it comes from."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import mc_oracle  # noqa: E402
from mc_cases import NO_INTERIOR_DIMS, NO_SURFACE, STAGE_CASES, cube_table, make_stage_volume  # noqa: E402

from sgnn_amd import _lib, marching_cubes as mc  # noqa: E402

pytestmark = pytest.mark.gpu
NTRI = np.array([0 if k in NO_SURFACE else len(row) // 3 for k, row in enumerate(mc_oracle.TRI)])
_cache = {}


@pytest.fixture(scope='module')
def gs():
    return np.load(os.path.join(HERE, 'golden', 'mc_stage_expected.npz'))


def case(name):
    """(tsdf, colors, spec, host triangle count per voxel, oracle soup verts, oracle soup colours), computed once."""
    if name not in _cache:
        spec = STAGE_CASES[name]
        tsdf, colors = make_stage_volume(spec)
        ci, _ = cube_table(tsdf.numpy(), spec['iso'], spec['trunc'], spec['thresh'])
        cnt = np.where(ci >= 0, NTRI[np.maximum(ci, 0)], 0)
        sv, sc = mc_oracle.triangle_soup(tsdf.numpy(), None if colors is None else colors.numpy(), spec['iso'],
                                         spec['trunc'], spec['thresh'])
        assert len(sv) == 3 * cnt.sum()         # the two host computations agree on the count
        _cache[name] = (tsdf, colors, spec, cnt, sv, sc)
    return _cache[name]


def voxel_of_triangle(cnt, t):
    flat = int(np.searchsorted(np.cumsum(cnt.reshape(-1)), t, side='right'))
    return tuple(int(i) for i in np.unravel_index(flat, cnt.shape))


def device_counts(tsdf, spec):
    """sgnn_mc_count by hand -> (total read back from the device, per-voxel counts read out of its workspace)."""
    t = tsdf.cuda().contiguous()
    d0, d1, d2 = (int(v) for v in t.shape)
    wsb = _lib.query('sgnn_mc_ws_bytes', d0, d1, d2)
    ws = torch.zeros(wsb, dtype=torch.uint8, device='cuda')
    ntri = torch.full((1,), -1, dtype=torch.int64, device='cuda')
    _lib.call('sgnn_mc_count', _lib.ptr(t), d0, d1, d2, float(spec['iso']), float(spec['trunc']), float(spec['thresh']),
              _lib.ptr(ws), wsb, _lib.ptr(ntri))
    return int(ntri.item()), ws[:d0 * d1 * d2].cpu().numpy().reshape(d0, d1, d2)


def same_soup(got_v, got_c, want_v, want_c, cnt):
    v, c = got_v.cpu().numpy(), got_c.cpu().numpy()
    assert v.dtype == np.float32 and c.dtype == np.uint8 and v.ndim == 2 and v.shape[1:] == (3,) and c.shape == v.shape
    n = min(len(v), len(want_v))
    differs = (v[:n].view(np.int32) != want_v[:n].view(np.int32)).any(1) | (c[:n] != want_c[:n]).any(1)
    if differs.any():
        t = int(np.nonzero(differs)[0][0]) // 3
        raise AssertionError('triangle %d, emitted by voxel (z,y,x) %s: device %s colours %s, oracle %s colours %s' % (
            t, voxel_of_triangle(cnt, t), v[3 * t:3 * t + 3].tolist(), c[3 * t:3 * t + 3].tolist(),
            want_v[3 * t:3 * t + 3].tolist(), want_c[3 * t:3 * t + 3].tolist()))
    assert len(v) == len(want_v), 'device soup has %d vertices, the oracle %d' % (len(v), len(want_v))


@pytest.mark.parametrize('name', list(STAGE_CASES))
def test_count_stage(name):
    """k_mc_count + k_mc_scan: the count of every voxel and the total."""
    tsdf, _, spec, cnt, _, _ = case(name)
    total, dcnt = device_counts(tsdf, spec)
    if not np.array_equal(dcnt, cnt):
        z, y, x = (int(i[0]) for i in np.nonzero(dcnt != cnt))
        raise AssertionError('voxel (z,y,x) %s: device counts %d triangles, host %d' % ((z, y, x), dcnt[z, y, x], cnt[z, y, x]))
    assert total == cnt.sum(), 'per-voxel counts agree, the scanned total does not: device %d, host %d' % (total, cnt.sum())


@pytest.mark.parametrize('name', list(STAGE_CASES))
def test_soup_stage(name):
    """k_mc_emit through mc.triangle_soup: vertex float bits, colours, length and order."""
    tsdf, colors, spec, cnt, sv, sc = case(name)
    got_v, got_c = mc.triangle_soup(tsdf.cuda(), colors, spec['iso'], spec['trunc'], spec['thresh'])
    same_soup(got_v, got_c, sv, sc, cnt)


@pytest.mark.parametrize('name', [n for n in STAGE_CASES if STAGE_CASES[n]['stored']])
def test_final_mesh_matches_the_reference(gs, name):
    tsdf, colors, spec, _, _, _ = case(name)
    v, c, f = (t.cpu().numpy() for t in mc.run_marching_cubes(tsdf.cuda(), colors, spec['iso'], spec['trunc'], spec['thresh']))
    wv, wc, wf = gs[name + '_v'], gs[name + '_c'], gs[name + '_f']
    assert (v.dtype, c.dtype, f.dtype) == (np.float32, np.uint8, np.int32)
    assert v.shape == wv.shape and f.shape == wf.shape, (v.shape, wv.shape, f.shape, wf.shape)
    assert np.array_equal(v.view(np.int32), wv.view(np.int32))
    assert np.array_equal(c, wc) and np.array_equal(f, wf)


@pytest.mark.parametrize('dims', NO_INTERIOR_DIMS)
def test_no_interior_voxel(dims):
    """Extents of 1 or 2: no voxel has its 26 neighbours, whatever the values.  Empty soup, empty mesh, right types."""
    tsdf = torch.from_numpy(np.random.default_rng(sum(dims)).normal(0, 0.5, dims).astype(np.float32))
    spec = dict(iso=0.0, trunc=3.0, thresh=10.0)
    total, dcnt = device_counts(tsdf, spec)
    assert total == 0 and not dcnt.any()
    sv, sc = mc.triangle_soup(tsdf.cuda(), None, 0.0, 3.0, 10.0)
    assert sv.shape == (0, 3) and sc.shape == (0, 3) and sv.dtype == torch.float32 and sc.dtype == torch.uint8
    v, c, f = mc.run_marching_cubes(tsdf.cuda(), None, 0.0, 3.0, 10.0)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    assert (v.dtype, c.dtype, f.dtype) == (torch.float32, torch.uint8, torch.int32)
    ov, oc = mc_oracle.triangle_soup(tsdf.numpy(), None, 0.0, 3.0, 10.0)
    assert ov.shape == (0, 3) and oc.shape == (0, 3)


@pytest.mark.parametrize('name', ['params', 'allcfg_colors'])
def test_non_contiguous_inputs(name):
    """A permuted view and a strided slice of a larger tensor give what their contiguous copies give."""
    tsdf, colors, spec, cnt, sv, sc = case(name)
    args = (spec['iso'], spec['trunc'], spec['thresh'])
    t, col = tsdf.cuda(), colors.cuda()
    permuted = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    pcol = col.permute(2, 1, 0, 3).contiguous().permute(2, 1, 0, 3)
    big = torch.full(tuple(2 * s + 3 for s in t.shape), float('nan'), device='cuda')
    big[1:-2:2, 2:-1:2, 1:-2:2] = t
    sliced = big[1:-2:2, 2:-1:2, 1:-2:2]
    assert not permuted.is_contiguous() and not pcol.is_contiguous() and not sliced.is_contiguous()
    assert torch.equal(permuted, t) and torch.equal(sliced, t) and torch.equal(pcol, col)
    same_soup(*mc.triangle_soup(permuted, pcol, *args), sv, sc, cnt)
    same_soup(*mc.triangle_soup(sliced, col, *args), sv, sc, cnt)
    want = [a.cpu().numpy() for a in mc.run_marching_cubes(t, col, *args)]
    got = [a.cpu().numpy() for a in mc.run_marching_cubes(sliced, pcol, *args)]
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
