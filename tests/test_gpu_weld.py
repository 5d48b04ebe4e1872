"""The vertex weld of marching_cubes.clean_mesh (csrc/mc.hip: k_weld_cells, k_weld_insert, k_weld_sweep, k_weld_lookup,
and the face clean-up behind it) against the sequential restatement oracle/mc_oracle.clean_mesh, bit for bit, on the
synthetic soups of tests/weld_cases.py: dependency chains hundreds of cells deep, a dense block in random order, a
vertex beside a cell created after its own cell's first vertex, coordinates of either sign and on cell boundaries,
degenerate and duplicate faces, and the sizes either side of sgnn_weld_slots' switch at 8.

Every soup runs at pitch 1e-5, where tests/test_oracle_mc.py pins the restatement's welding to the reference's own
extension, and at pitch 0.25, where all the arithmetic is exact and the comparison rests on the restatement alone.

The tests without the gpu mark check, on the host, that each soup has the property it is there for."""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import mc_oracle  # noqa: E402
import weld_cases as W  # noqa: E402

from sgnn_amd import _lib, marching_cubes as mc  # noqa: E402

gpu = pytest.mark.gpu
BOTH = [(name, thresh) for name in W.SOUPS for thresh in W.PITCHES]
_cache = {}


def soup(name, thresh):
    """(verts, vcols, cells, the oracle's mesh) of a soup at a pitch, computed once."""
    key = (name, thresh)
    if key not in _cache:
        verts, vcols = W.make_soup(name, thresh)
        _cache[key] = (verts, vcols, W.cells_of(verts, thresh), mc_oracle.clean_mesh(verts, vcols, np.float32(thresh)))
    return _cache[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# host: the soups are what they claim to be
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,thresh', BOTH)
def test_host_restatements_agree(name, thresh):
    """The sequential merge kept with its look-up table (weld_cases.greedy) gives the oracle's vertices, and the fixed
    point of the sweep rule (weld_cases.sweeps) creates exactly the cells the sequential merge creates."""
    verts, vcols, cells, (ov, oc, of) = soup(name, thresh)
    lookup, created = W.greedy(cells)
    creators = np.nonzero(lookup == np.arange(len(cells)))[0]
    assert sorted(created.values()) == creators.tolist()
    assert np.array_equal(ov.view(np.int32), verts[creators].view(np.int32)) and np.array_equal(oc, vcols[creators])
    _, uniq, first, state = W.sweeps(cells)
    assert {tuple(c) for c in uniq[state == W.IN].tolist()} == set(created)
    assert all(created[tuple(c)] == f for c, f in zip(uniq[state == W.IN].tolist(), first[state == W.IN].tolist()))


@pytest.mark.parametrize('thresh', W.PITCHES)
@pytest.mark.parametrize('name', W.CHAINS)
def test_chains_are_deep(name, thresh):
    """A condition on the input: the sweep rule, run synchronously on the host, needs at least 256 sweeps."""
    depth = W.sweeps(soup(name, thresh)[2])[0]
    assert depth >= 256, depth


@pytest.mark.parametrize('thresh', W.PITCHES)
def test_diagonal_chains_resolve_by_scan_order(thresh):
    """Second-pass vertices of cells that were not created have two created neighbours; on three of the four chains
    the one the dx,dy,dz scan meets first is not the one created first."""
    cells = soup('chain_diagonal', thresh)[2]
    lookup, created = W.greedy(cells)
    against_creation_order = 0
    for i in range(len(cells) // 2, len(cells)):
        c = cells[i]
        near = [created[k] for k in (tuple(c + np.asarray(o)) for o in W.OFFSETS) if k in created and created[k] < i]
        if len(near) == 2 and lookup[i] != min(near):
            assert lookup[i] == near[0]
            against_creation_order += 1
    assert against_creation_order >= 100, against_creation_order


@pytest.mark.parametrize('thresh', W.PITCHES)
def test_dense_block_needs_the_earlier_cells_only_rule(thresh):
    """Many cells are not created although an earlier neighbour was not created either, and many created cells have
    later neighbours, which a sweep must not wait for."""
    _, uniq, first, state = W.sweeps(soup('dense', thresh)[2])
    index = {tuple(c): k for k, c in enumerate(uniq.tolist())}
    out_beside_earlier_out = in_with_later_neighbour = 0
    for k, c in enumerate(uniq.tolist()):
        near = [index[n] for n in ((c[0] + o[0], c[1] + o[1], c[2] + o[2]) for o in W.OFFSETS if o != (0, 0, 0)) if n in index]
        if state[k] == W.OUT and any(first[n] < first[k] and state[n] == W.OUT for n in near):
            out_beside_earlier_out += 1
        if state[k] == W.IN and any(first[n] > first[k] for n in near):
            in_with_later_neighbour += 1
    assert out_beside_earlier_out >= 100 and in_with_later_neighbour >= 100, (out_beside_earlier_out, in_with_later_neighbour)


@pytest.mark.parametrize('thresh', W.PITCHES)
def test_late_vertex_finds_the_cell_created_in_between(thresh):
    cells = soup('late', thresh)[2]
    assert cells.tolist() == [[2, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [12, 0, 0], [2, 0, 0]]
    lookup, created = W.greedy(cells)
    assert lookup.tolist() == [0, 0, 2, 2, 4, 0] and (1, 0, 0) not in created
    # vertex 3: its cell's first vertex is 1, the cell it resolves to was created by vertex 2, in between
    assert 1 < created[(0, 0, 0)] < 3 and lookup[1] != lookup[3]


def test_signs_soup_covers_both_sides_of_zero():
    verts, _, cells, _ = soup('signs', 0.25)
    assert np.signbit(verts).any() and (verts == 0).any() and (np.signbit(verts) & (verts == 0)).any()
    assert sorted(set(cells.reshape(-1).tolist())) == [-2, -1, 0, 1, 2]
    assert cells[(verts == np.float32(0.125)).nonzero()].tolist().count(1) > 0          # (0 + 0.5) * thresh: cell 1
    assert cells[(verts == np.float32(-0.125)).nonzero()].tolist().count(-1) > 0


@pytest.mark.parametrize('thresh', W.PITCHES)
def test_face_soups_drop_what_they_should(thresh):
    _, _, _, (ov, _, of) = soup('faces_orders', thresh)
    assert len(ov) == 6 and of.tolist() == [[0, 1, 2], [3, 4, 5]]      # corners (1,2,0) are numbered as they come
    _, _, _, (ov, _, of) = soup('faces_all_dropped', thresh)
    assert len(ov) == 5 and of.shape == (0, 3)


def test_sizes_sit_either_side_of_the_slot_formula():
    assert [len(soup('nv%d' % n, 0.25)[0]) for n in (0, 3, 6, 9)] == [0, 3, 6, 9]
    assert [_lib.query('sgnn_weld_slots', n) for n in (0, 3, 6, 7, 8, 9)] == [16, 16, 16, 16, 17, 19]
    assert len(soup('large', 0.25)[0]) >= 20000


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name,thresh', BOTH)
def test_clean_mesh_matches_the_sequential_oracle(name, thresh):
    """Vertices (every float bit), colours, faces, dtypes and shapes.  The runs at pitch 0.25 rest on the restatement
    alone: the reference's extension welds at 1e-5 only."""
    verts, vcols, _, (ov, oc, of) = soup(name, thresh)
    t0 = time.perf_counter()
    v, c, f = (t.cpu().numpy() for t in mc.clean_mesh(dev(verts), dev(vcols), thresh))
    print('%s at %g: %d vertices, clean_mesh %.3f s' % (name, thresh, len(verts), time.perf_counter() - t0))
    assert (v.dtype, c.dtype, f.dtype) == (np.float32, np.uint8, np.int32)
    assert v.shape == ov.shape and c.shape == oc.shape and f.shape == of.shape, (v.shape, ov.shape, f.shape, of.shape)
    assert np.array_equal(v.view(np.int32), ov.view(np.int32))
    assert np.array_equal(c, oc)
    if not np.array_equal(f, of):
        t = int(np.nonzero((f != of).any(1))[0][0])
        raise AssertionError('face %d: device %s, oracle %s' % (t, f[t].tolist(), of[t].tolist()))


@gpu
@pytest.mark.parametrize('name', ['chain_middle', 'chain_diagonal', 'dense'])
def test_sweep_loop_by_hand(name):
    """sgnn_weld_build, then one sgnn_weld_sweep at a time with the counter read after each: it reaches 0 within the
    number of sweeps the synchronous rule needs on the host (values decided earlier in the same launch can only make
    it faster), the states are then the host's fixed point, cell by cell, and one further sweep changes nothing."""
    thresh = 0.25
    verts, _, cells, _ = soup(name, thresh)
    depth, uniq, first, state = W.sweeps(cells)
    nv = len(verts)
    cap = _lib.query('sgnn_weld_slots', nv)
    d_verts = dev(verts)
    d_cells = torch.empty((nv, 3), dtype=torch.int32, device='cuda')
    d_rep, d_first = (torch.empty(cap, dtype=torch.int32, device='cuda') for _ in range(2))
    d_state = torch.empty(cap, dtype=torch.uint8, device='cuda')
    d_undecided = torch.full((1,), -1, dtype=torch.int64, device='cuda')
    _lib.call('sgnn_weld_build', _lib.ptr(d_verts), nv, thresh, _lib.ptr(d_cells), _lib.ptr(d_rep), _lib.ptr(d_first),
              _lib.ptr(d_state), cap)
    assert np.array_equal(d_cells.cpu().numpy(), cells)

    def sweep():
        _lib.call('sgnn_weld_sweep', _lib.ptr(d_cells), _lib.ptr(d_rep), _lib.ptr(d_first), _lib.ptr(d_state), cap,
                  _lib.ptr(d_undecided))
        return int(d_undecided.item())

    t0 = time.perf_counter()
    left, history = -1, []
    while left != 0 and len(history) < depth:
        left = sweep()
        history.append(left)
    print('%s: host depth %d, device sweeps %d, %.3f s' % (name, depth, len(history), time.perf_counter() - t0))
    assert left == 0, 'still %d undecided cells after %d sweeps (host depth %d)' % (left, len(history), depth)
    assert all(a >= b for a, b in zip(history, history[1:])), history
    rep, got_first, got_state = d_rep.cpu().numpy(), d_first.cpu().numpy(), d_state.cpu().numpy()
    used = np.nonzero(rep != -1)[0]
    assert len(used) == len(uniq)
    want = {tuple(c): (int(f), int(s)) for c, f, s in zip(uniq.tolist(), first.tolist(), state.tolist())}
    got = {tuple(cells[rep[h]].tolist()): (int(got_first[h]), int(got_state[h])) for h in used}
    wrong = sorted(c for c in want if got.get(c) != want[c])
    assert not wrong, 'cell %s: device (first, state) %s, host %s' % (wrong[0], got.get(wrong[0]), want[wrong[0]])
    assert not got_state[rep == -1].any()
    assert sweep() == 0 and np.array_equal(d_state.cpu().numpy(), got_state)
