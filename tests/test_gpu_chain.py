"""sgnn_down2_chain (stride-2 pyramid of several levels with device-side row counts, one host read-back) must give
exactly what level-by-level sgnn_rulebook_down2 gives — same first-touch coarse order, parents, hashes, tables —
and the model must use 5 host read-backs per forward instead of 15 (scn.Convolution(2,2) rulebooks, torch/model.py:44
and the FullyConvolutionalNet bodies; mask compactions :233-247, :322-336)."""
import numpy as np
import pytest
import torch

from util import random_sites, param_fill

pytestmark = pytest.mark.gpu


def _levels(md, key, depth):
    out = []
    for _ in range(depth):
        nxt = tuple(v // 2 for v in key)
        out.append(md.down2(key, nxt))
        key = nxt
    return out


@pytest.mark.parametrize('surface', [False, True])
def test_chain_equals_level_by_level(surface):
    from sgnn_amd.scn import metadata as MD
    locs = random_sites(3, 32, 0.1, 5, surface)
    res = []
    for chain in (True, False):
        MD.CHAIN = chain
        try:
            rt = MD.runtime(torch.device('cuda'))
            g = MD.Grid(MD.coords_from_locs(locs, torch.device('cuda')))
            md = MD.Metadata()
            md.grids[(32, 32, 32)] = g
            s0 = rt.syncs
            md.prebuild((32, 32, 32), 3)
            ds = _levels(md, (32, 32, 32), 3)
            res.append((ds, rt.syncs - s0))
        finally:
            MD.CHAIN = True
    (a, sa), (b, sb) = res
    assert sa == 1 and sb == 3
    for da, db in zip(a, b):
        assert da.coarse.n == db.coarse.n and da.coarse.n > 0
        assert torch.equal(da.coarse.coords, db.coarse.coords)
        assert torch.equal(da.parent, db.parent)
        assert torch.equal(da.children.view(8, -1)[:, :da.coarse.n], db.children.view(8, -1)[:, :db.coarse.n])
        assert torch.equal(da.ptable.view(8, -1)[:, :da.fine.n], db.ptable.view(8, -1)[:, :db.fine.n])
        rows = da.coarse.lookup(db.coarse.coords)        # the chain's coarse hash resolves every coarse site
        assert torch.equal(rows.cpu(), torch.arange(db.coarse.n, dtype=torch.int32))
        # 3x3x3 rulebooks of the coarse levels agree as well (they are built from that hash)
        assert torch.equal(da.coarse.subm_table().view(27, -1)[:, :da.coarse.n],
                           db.coarse.subm_table().view(27, -1)[:, :db.coarse.n])


def test_model_forward_uses_five_readbacks_and_same_results():
    from sgnn_amd import synth
    from sgnn_amd.model import GenModel
    from sgnn_amd.scn import metadata as MD
    dims, cfg = (32, 32, 32), 23
    data = synth.make_batch(2, dims, cfg=cfg, occupancy=0.08)
    lw = np.ones(5, dtype=np.float32)
    m = param_fill(GenModel(8, dims, 1, 16, 16, 4, True, True, 1, 1), cfg).train().cuda()
    rt = MD.runtime(torch.device('cuda'))
    outs = []
    for chain in (True, False):
        MD.CHAIN = chain
        try:
            s0 = rt.syncs
            with torch.no_grad():
                sdf, occ = m([data['input'][0].cuda(), data['input'][1].cuda()], lw, batch_size=2)
            outs.append((sdf, occ, rt.syncs - s0))
        finally:
            MD.CHAIN = True
    (sa, oa, na), (sb, ob, nb) = outs
    assert na == 5 and nb == 15, (na, nb)
    for h in range(4):
        assert torch.equal(oa[h][0], ob[h][0]) and torch.equal(oa[h][1], ob[h][1])
    assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])


def test_teacher_forced_compaction_equals_boolean_indexing():
    """sgnn_compact_dense (the bench's teacher-forced masks): site i is kept iff the dense target occupancy volume is
    > 0.5 at its coordinates — stable order, sites outside the volume dropped — against torch boolean indexing; the
    plan variant (compaction + coordinates + stride-2 pyramid, one read-back) must agree with it."""
    from sgnn_amd.scn import functions as F_
    from sgnn_amd.scn.sites import info
    g = torch.Generator().manual_seed(5)
    B, d = 3, 16
    vol = (torch.rand(B, 1, d, d, d, generator=g) < 0.3).float()
    vol[vol == 0] = torch.rand(int((vol == 0).sum()), generator=g) * 0.5          # anything <= 0.5 is "empty"
    zz, yy, xx, bb = torch.meshgrid(torch.arange(d), torch.arange(d), torch.arange(d), torch.arange(B), indexing='ij')
    coords = torch.stack([zz, yy, xx, bb], -1).view(-1, 4)
    coords = coords[torch.randperm(coords.shape[0], generator=g)[:5000]]
    coords = torch.cat([coords, torch.tensor([[d, 0, 0, 0], [0, 0, 0, B], [-1, 2, 2, 1]])])   # outside: never kept
    keep = torch.zeros(coords.shape[0], dtype=torch.bool)
    inside = ((coords[:, :3] >= 0) & (coords[:, :3] < d)).all(1) & (coords[:, 3] >= 0) & (coords[:, 3] < B)
    c = coords[inside]
    keep[inside] = vol[c[:, 3], 0, c[:, 0], c[:, 1], c[:, 2]] > 0.5
    want = torch.nonzero(keep)[:, 0].to(torch.int32)
    c32 = coords.to(torch.int32).cuda()
    n = int(c32.shape[0])
    for depth in (0, 2):
        sel, cnt, locs = F_.compact_sigmoid_plan(c32, 2, n, c32, depth, vol.cuda())
        assert cnt == int(want.numel()) and 0 < cnt < n
        assert torch.equal(sel.cpu(), want)
        assert torch.equal(locs.cpu(), coords[keep].to(torch.int32))
        assert (info(locs).plan is not None) == (depth == 2)
    grid0, downs = info(locs).plan
    assert grid0.n == cnt and len(downs) == 2
    coarse = torch.unique(torch.cat([coords[keep][:, :3] // 2, coords[keep][:, 3:]], 1), dim=0)
    assert downs[0].coarse.n == coarse.shape[0]
    got = torch.unique(downs[0].coarse.coords[:downs[0].coarse.n].cpu().to(torch.int64), dim=0)
    assert torch.equal(got, coarse)
