"""The module wrappers (sgnn_amd/scn/modules.py) against oracle/scn_oracle evaluated in float64, on integer data: every
module here is linear (or affine) in its input and in its parameters, all values stay far below 2^24, so forward, input
gradient and parameter gradients must equal the oracle's bit for bit.  Each module instance is applied to two different
grids in turn, so a rulebook or table kept on the wrong key would show on the second."""
import pytest
import torch

import scn_oracle as oscn
from util import random_sites

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SIZE = [16, 16, 16]
CIN = 8


def _scn():
    import sgnn_amd.scn as scn
    return scn


def _grids():
    return [random_sites(2, 16, 0.2, 3), random_sites(3, 16, 0.12, 4, surface=True)]


def _ints(shape, gen, lim):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=gen).double()


NETS = {
    'SubmanifoldConvolution': lambda s: s.Sequential().add(s.SubmanifoldConvolution(3, CIN, 12, 3, True)).add(s.OutputLayer(3)),
    'Convolution': lambda s: s.Sequential().add(s.Convolution(3, CIN, 12, 2, 2, True)).add(s.OutputLayer(3)),
    'Deconvolution': lambda s: s.Sequential().add(s.Convolution(3, CIN, 8, 2, 2, False))
                                             .add(s.Deconvolution(3, 8, 12, 2, 2, True)).add(s.OutputLayer(3)),
    'UnPooling': lambda s: s.Sequential().add(s.Convolution(3, CIN, 12, 2, 2, False)).add(s.UnPooling(3, 2, 2))
                                         .add(s.OutputLayer(3)),
    'NetworkInNetwork': lambda s: s.Sequential().add(s.NetworkInNetwork(CIN, 12, True)).add(s.OutputLayer(3)),
    'ConcatTable-JoinTable': lambda s: s.Sequential().add(
        s.ConcatTable().add(s.Identity()).add(s.SubmanifoldConvolution(3, CIN, 12, 3, False))
                       .add(s.NetworkInNetwork(CIN, 5, False))).add(s.JoinTable()).add(s.OutputLayer(3)),
    'ConcatTable-AddTable': lambda s: s.Sequential().add(
        s.ConcatTable().add(s.Identity()).add(s.SubmanifoldConvolution(3, CIN, CIN, 3, False))
                       .add(s.NetworkInNetwork(CIN, CIN, False))).add(s.AddTable()).add(s.OutputLayer(3)),
    'SparseToDense': lambda s: s.Sequential().add(s.SparseToDense(3, CIN)),
    'InputLayer-OutputLayer': lambda s: s.Sequential().add(s.OutputLayer(3)),
}


def _fill(mo, mh, gen):
    """Integer parameters in {-2..2} on the float64 oracle module, the same values on the HIP module."""
    with torch.no_grad():
        for p in mo.parameters():
            p.copy_(_ints(p.shape, gen, 2))
    missing = mh.load_state_dict({k: v.float() for k, v in mo.state_dict().items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys


@pytest.mark.parametrize('name', list(NETS))
def test_module_equals_float64_oracle_on_two_grids(name):
    scn = _scn()
    gen = torch.Generator().manual_seed(len(name))
    mo, mh = NETS[name](oscn).double(), NETS[name](scn).to(DEV)
    assert list(mo.state_dict().keys()) == list(mh.state_dict().keys())
    _fill(mo, mh, gen)
    for gi, locs in enumerate(_grids()):
        what = '%s grid %d' % (name, gi)
        feats = _ints((locs.shape[0], CIN), gen, 3)
        fo, fh = feats.clone().requires_grad_(True), feats.float().to(DEV).requires_grad_(True)
        yo = mo(oscn.InputLayer(3, SIZE, mode=0)([locs, fo]))
        yh = mh(scn.InputLayer(3, SIZE, mode=0)([locs.to(DEV), fh]))
        assert yh.dtype == torch.float32 and yh.shape == yo.shape, what
        assert float(yo.detach().abs().max()) < 2 ** 20
        assert torch.equal(yh.detach().cpu().double(), yo.detach()), what + ': forward'
        dy = _ints(yo.shape, gen, 3)
        mo.zero_grad()
        mh.zero_grad()
        yo.backward(dy)
        yh.backward(dy.float().to(DEV))
        assert torch.equal(fh.grad.cpu().double(), fo.grad), what + ': input gradient'
        for (ko, po), (kh, ph) in zip(mo.named_parameters(), mh.named_parameters()):
            assert ko == kh and float(po.grad.abs().max()) < 2 ** 22
            assert torch.equal(ph.grad.cpu().double(), po.grad), '%s: gradient of %s' % (what, ko)


@pytest.mark.parametrize('kind', ['SubmanifoldConvolution', 'Convolution'])
def test_grouped_reference_layout_state_dict_loads(kind):
    """Later upstream versions store (K, groups = 1, nIn, nOut): _accept_grouped_weight drops the group axis."""
    scn = _scn()
    gen = torch.Generator().manual_seed(7)
    make = (lambda s: s.SubmanifoldConvolution(3, CIN, 12, 3, True)) if kind == 'SubmanifoldConvolution' else \
        (lambda s: s.Convolution(3, CIN, 12, 2, 2, True))
    mo, mh = make(oscn).double(), make(scn).to(DEV)
    K = mo.weight.shape[0]
    w4, b = _ints((K, 1, CIN, 12), gen, 2), _ints((12,), gen, 2)
    mh.load_state_dict({'weight': w4.float(), 'bias': b.float()}, strict=True)
    assert mh.weight.shape == (K, CIN, 12) and torch.equal(mh.weight.detach().cpu().double(), w4[:, 0])
    with pytest.raises(RuntimeError):          # two groups are not this layer
        make(scn).load_state_dict({'weight': torch.zeros(K, 2, CIN, 12), 'bias': b.float()}, strict=True)
    mo.load_state_dict({'weight': w4[:, 0], 'bias': b})
    locs = _grids()[0]
    feats = _ints((locs.shape[0], CIN), gen, 3)
    yo = mo(oscn.InputLayer(3, SIZE, mode=0)([locs, feats])).features
    yh = mh(scn.InputLayer(3, SIZE, mode=0)([locs.to(DEV), feats.float().to(DEV)])).features
    assert torch.equal(yh.detach().cpu().double(), yo.detach())
