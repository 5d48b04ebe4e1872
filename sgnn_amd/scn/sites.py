"""Host-side metadata of a tensor of sites: one typed record instead of loose attributes.

The stages hand device-side geometry to each other along with the coordinate tensors: the live row count of a
capacity-mode tensor, the bound its sites lie inside, a pyramid that was built together with them.  A Python attribute
does not survive a tensor operation (`t.detach()`, `t[:n]` return a new object without it), so every place that makes a
new tensor for the same sites says with `carry` which fields go along.  A misspelt field raises instead of reading as
"not there".  Imports nothing from the library and needs no GPU.
"""
import torch

_ATTR = '_sgnn_sites'       # the one attribute a tensor gets; nothing outside this module spells it
_EMPTY = None


class SiteInfo(object):
    """cnt:      live row count of a capacity-mode tensor (device int64[1]; None: the row count is exact)
    cnt8:     8 x that count (rows of the 8-child expansion)
    bounds:   (B, Z, Y, X) every site lies inside by construction
    plan:     (Grid, [Down2]) stride-2 pyramid built together with the compaction that made the sites
    children: their 8-child expansion, where it already exists
    i64:      the same rows as int64, where they were written in the same pass"""
    __slots__ = ('cnt', 'cnt8', 'bounds', 'plan', 'children', 'i64')

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)

    def __setattr__(self, name, value):
        if self is _EMPTY:
            raise AttributeError('the empty SiteInfo is shared and read-only: use attach()')
        object.__setattr__(self, name, value)


_EMPTY = SiteInfo()       # the record of everything that has none


def info(t):
    """The record of `t`; the shared, read-only empty one for a tensor without a record and for a non-tensor (`[]` is
    what the model returns as the locs of a level that did not run).  Never attaches anything."""
    return getattr(t, _ATTR, _EMPTY) if torch.is_tensor(t) else _EMPTY


def attach(t, **fields):
    """Set the named fields of t's own record (created on first use); returns t."""
    rec = info(t)
    own = rec if rec is not _EMPTY else SiteInfo()
    for name, value in fields.items():
        setattr(own, name, value)        # an unknown name raises (__slots__)
    if own is not rec:
        setattr(t, _ATTR, own)
    return t


def carry(dst, src, *fields):
    """Copy exactly the named fields that are set on `src` to `dst` (a new tensor for the same sites); returns dst.
    There is no copy-everything form: every call site says what travels."""
    if dst is not src:
        rec = info(src)
        live = dict((name, getattr(rec, name)) for name in fields if getattr(rec, name) is not None)
        if live:
            attach(dst, **live)
    return dst
