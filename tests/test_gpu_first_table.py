"""GPU: the first-member hash table (csrc/first_table.h) at its smallest size, 16 slots, with keys chosen so that the
probe chain runs from slot 14 over slot 15 round to slots 0 and 1: the vertex weld of marching_cubes.clean_mesh, the
duplicate-face set of sgnn_mesh_faces and the vertex clusters of simplify.cluster.  The other mesh tests use tables so
sparse that a wrong wrap-around or a wrong step along a collision chain could pass them.

The two hash functions are restated here in uint64 arithmetic and the keys are searched for on the host: one with home
slot 14 and three with home slot 15.  A search that comes up short fails the test before anything runs on the device.
Last: _glue.compact with and without its read-back."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as SR  # noqa: E402

from sgnn_amd import _lib, marching_cubes as mc, simplify  # noqa: E402

gpu = pytest.mark.gpu

U64, F32 = np.uint64, np.float32
SLOTS = 16                  # sgnn_weld_slots(n) for n < 8
HOMES = (14, 15, 15, 15)    # the chain 14, 15 -> 0 -> 1


def weld_hash(c):
    """weld_hash of first_table.h for integer triples c (N, 3)."""
    c = (np.asarray(c, np.int64) & 0xFFFFFFFF).astype(U64)
    h = c[:, 0] * U64(0x9E3779B97F4A7C15)
    h = h ^ (c[:, 1] * U64(0xC2B2AE3D27D4EB4F) + (h << U64(6)) + (h >> U64(2)))
    h = h ^ (c[:, 2] * U64(0x165667B19E3779F9) + (h << U64(6)) + (h >> U64(2)))
    return h ^ (h >> U64(29))


def hash64(k):
    """sgnn_hash64 of common.h (the murmur3 finaliser) for uint64 keys k (N,)."""
    k = np.asarray(k, U64)
    k = (k ^ (k >> U64(33))) * U64(0xff51afd7ed558ccd)
    k = (k ^ (k >> U64(33))) * U64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> U64(33))


def test_the_restated_hashes():
    """Values of the two C functions, computed by a host compile of their text."""
    assert weld_hash([[0, 0, 0], [1, 2, 3], [-4, 6, -20], [63, 62, 61]]).tolist() == [
        0, 78803241148797652, 13528577255256335825, 17090905066254914867]
    assert hash64([0, 1, (3 << 42) | (5 << 21) | 7, (15 << 42) | (15 << 21) | 15]).tolist() == [
        0, 12994781566227106604, 15728772653306157750, 5245241193140207629]


def chain(candidates, homes):
    """The first candidates, in their order, whose home slots are HOMES; every one must be found."""
    homes = np.asarray(homes % U64(SLOTS), np.int64)
    picked = []
    for want in HOMES:
        rows = [i for i in np.nonzero(homes == want)[0].tolist() if i not in picked]
        assert rows, 'no key with home slot %d among %d candidates' % (want, len(homes))
        picked.append(rows[0])
    assert len(set(picked)) == 4 and homes[picked].tolist() == list(HOMES)
    return candidates[picked]


def occupied(homes):
    """Slots that linear probing with wrap-around fills for keys with these home slots (any insertion order)."""
    used = set()
    for h in homes:
        while h in used:
            h = 0 if h + 1 == SLOTS else h + 1
        used.add(h)
    return sorted(used)


def test_the_chain_wraps():
    assert occupied(HOMES) == [0, 1, 14, 15]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@gpu
def test_weld_chain_through_slot_15():
    """Four vertices in four cells, the last three colliding at slot 15, and exact copies of two of those: clean_mesh
    keeps the first vertex of every cell in input order and remaps the two triangles."""
    lattice = np.arange(-20, 21, 2)         # two lattice cells are at least 2 apart on some axis: no neighbour merges
    cand = np.array(list(itertools.product(lattice, repeat=3)), np.int64)
    cells = chain(cand, weld_hash(cand))
    thresh = F32(mc.WELD_THRESH)
    verts = np.concatenate([cells, cells[[1, 2]]]).astype(F32) * thresh
    assert len(verts) == 6 and _lib.query('sgnn_weld_slots', len(verts)) == SLOTS
    got_cells = np.trunc(verts / thresh + F32(0.5) * np.sign(verts)).astype(np.int64)          # mc.hip: k_weld_cells
    assert np.array_equal(got_cells, np.concatenate([cells, cells[[1, 2]]]))
    vcols = np.random.default_rng(3).integers(0, 256, (6, 3), dtype=np.uint8)
    first = {}
    for i, c in enumerate(map(tuple, got_cells)):
        first.setdefault(c, i)
    creators = sorted(first.values())
    assert creators == [0, 1, 2, 3]
    want_f = np.array([creators.index(first[tuple(c)]) for c in got_cells], np.int32).reshape(2, 3)
    out_v, out_c, out_f = mc.clean_mesh(dev(verts), dev(vcols))
    assert np.array_equal(host(out_v).view(np.int32), verts[creators].view(np.int32))
    assert np.array_equal(host(out_c), vcols[creators])
    assert np.array_equal(host(out_f), want_f) and want_f.tolist() == [[0, 1, 2], [3, 1, 2]]


@gpu
def test_faces_chain_through_slot_15():
    """sgnn_mesh_faces with identity maps: four faces, the last three colliding at slot 15, a flipped and a rotated copy
    of one of those and a degenerate face.  keep marks the first face of every unordered triple; the table holds those
    four firsts in the slots 14, 15, 0 and 1."""
    cand = np.array(list(itertools.combinations(range(64), 3)), np.int64)          # sorted triples
    tri = chain(cand, weld_hash(cand))
    f2 = tri[2][[0, 2, 1]]
    faces = np.array([tri[0][[1, 0, 2]], tri[1][[2, 1, 0]], f2, tri[3], f2[::-1], [tri[3][0], tri[3][0], tri[3][2]],
                      f2[[1, 2, 0]]], np.int32)
    ntri = len(faces)
    assert ntri == 7 and _lib.query('sgnn_weld_slots', ntri) == SLOTS
    first = {}
    for t, f in enumerate(faces):
        if len(set(f.tolist())) == 3:
            first.setdefault(tuple(sorted(f.tolist())), t)
    want_keep = np.array([first.get(tuple(sorted(f.tolist()))) == t for t, f in enumerate(faces)], np.uint8)
    assert want_keep.tolist() == [1, 1, 1, 1, 0, 0, 0]
    corner_ids, newid = dev(faces.reshape(-1)), dev(np.arange(64, dtype=np.int32))
    out = torch.empty((ntri, 3), dtype=torch.int32, device='cuda')
    frep = torch.empty(SLOTS, dtype=torch.int32, device='cuda')
    ffirst = torch.empty(SLOTS, dtype=torch.int32, device='cuda')
    keep = torch.empty(ntri, dtype=torch.uint8, device='cuda')
    _lib.call('sgnn_mesh_faces', _lib.ptr(corner_ids), _lib.ptr(newid), ntri, _lib.ptr(out), _lib.ptr(frep),
              _lib.ptr(ffirst), SLOTS, _lib.ptr(keep))
    assert np.array_equal(host(out), faces)
    assert np.array_equal(host(keep), want_keep)
    frep, ffirst = host(frep), host(ffirst)
    assert np.nonzero(frep != -1)[0].tolist() == occupied(HOMES)
    assert ffirst[14] == 0 and sorted(ffirst[[15, 0, 1]].tolist()) == [1, 2, 3]
    assert np.all(ffirst[frep == -1] == 0x7F7F7F7F)


@gpu
def test_cluster_chain_through_slot_15():
    """Seven vertices in five grid cells, three of the cells colliding at slot 15: simplify.cluster against the host
    restatement, bit for bit, both placements."""
    cand = np.array(list(itertools.product(range(16), repeat=3)), np.int64)
    keys = ((cand[:, 0] << 42) | (cand[:, 1] << 21) | cand[:, 2]).astype(U64)
    cells = chain(cand, hash64(keys))
    other = next(c for c in cand if not (c == cells).all(1).any())
    cells = np.concatenate([cells, other[None]])
    verts = np.concatenate([cells + 0.5, cells[[1]] + [0.25, 0.75, 0.5], cells[[2]] + [0.75, 0.25, 0.125]]).astype(F32)
    faces = np.array([[0, 1, 2], [3, 5, 6], [0, 4, 3], [2, 1, 4], [0, 6, 5], [1, 5, 3]], np.int32)
    colors = np.random.default_rng(5).integers(0, 256, (7, 3), dtype=np.uint8)
    assert len(verts) == 7 and _lib.query('sgnn_weld_slots', len(verts)) == SLOTS
    origin = np.zeros(3, F32)
    assert np.array_equal(SR.cells(verts, 1.0, origin)[0], np.concatenate([cells, cells[[1, 2]]]))
    for placement in simplify.PLACEMENTS:
        want = SR.cluster(verts, faces, 1.0, colors=colors, placement=placement, origin=origin)
        out = simplify.cluster(verts, faces, 1.0, colors=colors, placement=placement, origin=origin)
        assert np.array_equal(host(out.verts).view(np.int32), want.verts.view(np.int32))
        assert np.array_equal(host(out.faces), want.faces) and len(want.faces) >= 3
        assert np.array_equal(host(out.colors), want.colors)
        assert np.array_equal(host(out.face_map), want.face_map)
        vmap = host(out.vertex_map)
        assert np.array_equal(vmap, want.vertex_map)
        assert vmap[5] == vmap[1] >= 0 and vmap[6] == vmap[2] >= 0 and len(set(vmap[:5].tolist())) == 5


@gpu
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257])
def test_compact_with_and_without_the_read_back(n):
    from sgnn_amd._glue import compact
    mask = np.random.default_rng(n).integers(0, 2, max(n, 1), dtype=np.uint8)
    want = np.nonzero(mask[:n])[0]
    sel, count = compact(dev(mask), n, torch.device('cuda'))
    sel_late, count_late = compact(dev(mask), n, torch.device('cuda'), read=False)
    assert isinstance(count, int) and count == len(want)
    assert count_late.dtype == torch.int64 and count_late.is_cuda and count_late.tolist() == [count]
    assert np.array_equal(host(sel[:count]), want) and np.array_equal(host(sel_late[:count]), want)
