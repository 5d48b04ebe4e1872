"""scn/sites.py: the one record that carries site metadata from stage to stage, and the three places that decide what
travels with a new tensor for the same sites (coords_from_locs, _inherit_bounds, GraphStep._detached).  No GPU."""
import pytest
import torch

from sgnn_amd.scn import sites
from sgnn_amd.scn.sites import SiteInfo, info, attach, carry

FIELDS = ('cnt', 'cnt8', 'bounds', 'plan', 'children', 'i64')


def _c32():
    return torch.arange(16, dtype=torch.int32).view(4, 4)


def _c64():
    return torch.arange(16, dtype=torch.int64).view(4, 4)


def _full(t):
    """Every field set, each to an object of its own."""
    vals = dict(cnt=torch.tensor([3]), cnt8=torch.tensor([24]), bounds=(2, 8, 8, 8), plan=('grid', []), children=_c32(),
                i64=_c64())
    return attach(t, **vals), vals


def test_fields_are_fixed():
    assert SiteInfo.__slots__ == FIELDS
    assert all(getattr(SiteInfo(), f) is None for f in FIELDS)


@pytest.mark.parametrize('make', [_c32, _c64, list])
def test_info_of_a_bare_object_is_empty_and_attaches_nothing(make):
    t = make()
    before = (dict(vars(t)), dir(t)) if torch.is_tensor(t) else None
    rec = info(t)
    assert all(getattr(rec, f) is None for f in FIELDS)
    assert rec is info(make())                              # shared
    if before is not None:
        assert (dict(vars(t)), dir(t)) == before


def test_the_shared_empty_record_is_read_only():
    for f in FIELDS:
        with pytest.raises(AttributeError):
            setattr(info(_c32()), f, 1)
    assert info([]).cnt is None


def test_attach_then_info_gives_the_same_object():
    t, cnt = _c64(), torch.tensor([3])
    assert attach(t, cnt=cnt) is t
    assert info(t).cnt is cnt
    assert info(t) is not info(_c64())
    bounds = (1, 4, 4, 4)
    attach(t, bounds=bounds)                                # a second call extends the same record
    assert info(t).cnt is cnt and info(t).bounds is bounds
    assert [k for k in vars(t) if k.startswith('_sgnn')] == [sites._ATTR]       # ONE attribute on the tensor


def test_a_misspelt_field_raises():
    t = _c32()
    with pytest.raises(AttributeError):
        attach(t, nope=1)
    with pytest.raises(AttributeError):
        info(t).nope
    with pytest.raises(AttributeError):
        info(attach(t, cnt=torch.tensor([1]))).nope
    with pytest.raises(AttributeError):
        carry(_c32(), t, 'nope')


def test_carry_copies_exactly_the_named_fields():
    src, vals = _full(_c32())
    dst = _c32()
    assert carry(dst, src, 'cnt', 'cnt8') is dst
    assert info(dst).cnt is vals['cnt'] and info(dst).cnt8 is vals['cnt8']
    assert all(getattr(info(dst), f) is None for f in ('plan', 'children', 'bounds', 'i64'))
    assert info(dst) is not info(src)


def test_carry_onto_itself_is_a_no_op():
    t, vals = _full(_c32())
    rec = info(t)
    assert carry(t, t, 'cnt', 'plan') is t
    assert info(t) is rec and all(getattr(rec, f) is vals[f] for f in FIELDS)
    bare = _c32()
    carry(bare, bare, 'cnt')
    assert sites._ATTR not in vars(bare)


def test_carry_does_not_overwrite_with_none():
    src = attach(_c32(), cnt=torch.tensor([2]))             # cnt8 is None here
    keep = torch.tensor([16])
    dst = attach(_c32(), cnt8=keep)
    carry(dst, src, 'cnt', 'cnt8')
    assert info(dst).cnt is info(src).cnt and info(dst).cnt8 is keep
    bare = _c32()
    carry(bare, _c32(), 'cnt', 'cnt8')                      # nothing to carry: no record is made
    assert sites._ATTR not in vars(bare)


@pytest.mark.parametrize('make', [_c32, _c64])
def test_which_tensor_operations_keep_the_record(make):
    """The facts the design rests on (a torch upgrade that changes one of them has to be noticed): a new tensor object has
    no record, and contiguous() / to(same device) of a contiguous tensor return the same object."""
    t, _ = _full(make())
    for u in (t.detach(), t[:2]):
        assert u is not t and info(u).cnt is None and sites._ATTR not in vars(u)
    assert t.contiguous() is t
    assert t.to(t.device) is t


def test_coords_from_locs_passes_int32_rows_through(monkeypatch):
    from sgnn_amd.scn import metadata as MD
    monkeypatch.setattr(MD, 'runtime', lambda device: None)         # the pass-through branch makes no library call
    t, vals = _full(_c32())
    rec = info(t)
    out = MD.coords_from_locs(t, t.device)
    assert out is t and info(out) is rec
    assert all(getattr(rec, f) is vals[f] for f in FIELDS)
    bare = _c32()
    assert MD.coords_from_locs(bare, bare.device) is bare and sites._ATTR not in vars(bare)


def test_coords_from_locs_carries_counts_plan_and_children_only(monkeypatch):
    """An int64 `locs` becomes a new int32 tensor (the conversion kernel is stubbed out here): the live counts, the plan
    and the children travel; the bound and the int64 rows do not (Grid.bounds decides which rulebook builder runs)."""
    from sgnn_amd.scn import metadata as MD

    class _Rt(object):
        status32 = None
    calls = []
    monkeypatch.setattr(MD, 'runtime', lambda device: _Rt())
    monkeypatch.setattr(MD, 'ptr', lambda t: t)
    monkeypatch.setattr(MD._lib, 'call', lambda *a: calls.append(a))
    t, vals = _full(_c64())
    out = MD.coords_from_locs(t, t.device)
    assert out is not t and out.dtype == torch.int32 and out.shape == (4, 4)
    assert calls[0][0] == 'sgnn_coords_from_i64' and calls[0][-1] is vals['cnt']
    assert all(getattr(info(out), f) is vals[f] for f in ('cnt', 'cnt8', 'plan', 'children'))
    assert info(out).bounds is None and info(out).i64 is None
    exact = attach(_c64(), plan=vals['plan'], cnt8=vals['cnt8'])          # no live count: nothing travels
    assert sites._ATTR not in vars(MD.coords_from_locs(exact, exact.device))


def test_inherit_bounds_scales_the_spatial_bound():
    from sgnn_amd.scn.functions import _inherit_bounds
    parent = attach(_c32(), bounds=(2, 4, 6, 8), cnt=torch.tensor([3]))
    same, twice = _c32(), _c32()
    assert _inherit_bounds(same, parent) is same and info(same).bounds == (2, 4, 6, 8)
    assert _inherit_bounds(twice, parent, 2) is twice and info(twice).bounds == (2, 8, 12, 16)
    assert info(same).cnt is None and info(twice).cnt is None            # the bound only
    assert info(parent).bounds == (2, 4, 6, 8)
    child = _c32()
    assert _inherit_bounds(child, _c32(), 2) is child
    assert info(child).bounds is None and sites._ATTR not in vars(child)


def test_detached_outputs_keep_their_live_counts():
    from sgnn_amd.train import GraphStep
    t = torch.zeros(4, 4, requires_grad=True) * 2.0
    assert t.grad_fn is not None
    _, vals = _full(t)
    u = _c64()
    out_sdf, out_occs = GraphStep._detached([t], [[u, []]])
    d = out_sdf[0]
    assert d is not t and d.grad_fn is None and not d.requires_grad
    assert d.data_ptr() == t.data_ptr() and d.shape == t.shape
    assert info(d).cnt is vals['cnt'] and info(d).cnt8 is vals['cnt8']
    assert all(getattr(info(d), f) is None for f in ('plan', 'children', 'bounds', 'i64'))
    assert info(t).plan is vals['plan']                                   # the original keeps its own
    du, empty = out_occs[0]
    assert du.data_ptr() == u.data_ptr() and sites._ATTR not in vars(du)
    assert empty == [] and isinstance(empty, list)
