"""CPU: ``centertrack_amd.dla_seg.DLASeg`` without a GPU -- the state dict has exactly the keys and shapes of the reference's
own ``DLASeg`` (tests/golden/dlaseg_keys.json, written by tests/golden/make_dlaseg_keys.py), constructor and ``forward``
signatures, the reference's initialisation, the refusals, and the ordering of ``model_output_list``."""
import inspect
import json
import os
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADS = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2)])
HEAD_CONVS = {h: [256] for h in HEADS}


class Opt(object):
    pre_img, pre_hm = True, True
    dla_node, head_kernel, prior_bias = 'dcn', 3, -4.6
    model_output_list = False
    load_model = ''

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


@pytest.fixture(scope='module')
def model():
    from centertrack_amd.dla_seg import DLASeg
    return DLASeg(34, HEADS, HEAD_CONVS, Opt())


def test_keys_and_shapes_are_the_references(model):
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'dlaseg_keys.json')))
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == want
    tops = {k.split('.')[0] for k, _ in want}
    assert tops == {'base', 'dla_up', 'ida_up'} | set(HEADS)
    for h, c in HEADS.items():
        assert tuple(model.state_dict()[h + '.2.weight'].shape) == (c, 256, 1, 1)
    # a reference-format checkpoint loads as it is, and comes back as it went in
    sd = OrderedDict((k, torch.full(s, 0.5) if s else torch.tensor(3)) for k, s in want)
    from centertrack_amd.dla_seg import DLASeg
    m = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_signatures(model):
    from centertrack_amd.dla_seg import DLASeg
    assert list(inspect.signature(DLASeg.__init__).parameters)[1:] == ['num_layers', 'heads', 'head_convs', 'opt']
    f = inspect.signature(DLASeg.forward).parameters
    assert list(f)[1:] == ['x', 'pre_img', 'pre_hm'] and f['pre_img'].default is None and f['pre_hm'].default is None
    g = inspect.signature(DLASeg.imgpre2feats).parameters
    assert list(g)[1:] == ['x', 'pre_img', 'pre_hm'] and list(inspect.signature(DLASeg.img2feats).parameters)[1:] == ['x']
    assert (model.num_stacks, model.first_level, model.last_level) == (1, 2, 5)
    assert dict(model.heads) == dict(HEADS)


def test_initialisation(model):
    """base_model.py:54-57 and dla.py:454-463: the last bias of a head whose name contains ``hm`` is ``prior_bias`` (its first
    bias keeps torch's default), every other head bias is 0, every ``up_*`` holds the bilinear kernel"""
    from centertrack_amd.dla_seg import DLASeg
    sd = model.state_dict()
    assert bool((sd['hm.2.bias'] == -4.6).all()) and float(sd['hm.0.bias'].abs().max()) > 0
    for h in ('reg', 'wh', 'tracking'):
        assert float(sd[h + '.0.bias'].abs().max()) == 0.0 and float(sd[h + '.2.bias'].abs().max()) == 0.0
    other = DLASeg(34, HEADS, HEAD_CONVS, Opt(prior_bias=-2.19))
    assert bool((other.state_dict()['hm.2.bias'] == -2.19).all())
    ups = [k for k in sd if '.up_' in k]
    assert len(ups) == 8                                          # 1 + 2 + 3 in dla_up, 2 in ida_up
    for k in ups:
        w = sd[k]
        kk = w.shape[2]
        f = kk // 2
        c = (2 * f - 1 - f % 2) / (2.0 * f)
        line = torch.tensor([1 - abs(i / f - c) for i in range(kk)])
        assert w.shape[1] == 1 and torch.equal(w, (line.view(kk, 1) * line.view(1, kk)).expand_as(w)), k
    # the base is built without pretrained weights whatever load_model says: torch's defaults, nothing downloaded
    assert bool((sd['base.base_layer.1.weight'] == 1).all()) and bool((sd['base.level5.root.bn.running_var'] == 1).all())
    assert not hasattr(model.base, 'fc')


def test_refusals():
    from centertrack_amd import _lib
    from centertrack_amd.dla_seg import DLASeg
    for layers in (18, 60, 102, 169):
        with pytest.raises(_lib.CTError, match='DLA-34'):
            DLASeg(layers, HEADS, HEAD_CONVS, Opt())
    for node in ('gcn', 'conv'):
        with pytest.raises(_lib.CTError, match='dla_node'):
            DLASeg(34, HEADS, HEAD_CONVS, Opt(dla_node=node))
    with pytest.raises(_lib.CTError, match='head_kernel'):
        DLASeg(34, HEADS, HEAD_CONVS, Opt(head_kernel=1))
    with pytest.raises(_lib.CTError, match='one head-conv layer'):
        DLASeg(34, HEADS, {h: [256, 256] for h in HEADS}, Opt())
    with pytest.raises(_lib.CTError, match='one head-conv layer'):
        DLASeg(34, HEADS, {h: [] for h in HEADS}, Opt())
    m = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    with pytest.raises(_lib.CTError, match='no CPU fallback'):                     # CUDA tensors only
        m(torch.zeros(1, 3, 32, 32))
    plain = DLASeg(34, HEADS, HEAD_CONVS, Opt(pre_img=False, pre_hm=False))
    assert not any('pre_' in k for k in plain.state_dict())


def test_model_output_list_ordering(monkeypatch):
    """``[[logits in sorted(heads) order]]`` with ``opt.model_output_list``, ``[{head: logits}]`` without"""
    from centertrack_amd.dla_seg import DLASeg
    z = OrderedDict((h, torch.full((1, c, 2, 2), float(i))) for i, (h, c) in enumerate(HEADS.items()))
    monkeypatch.setattr(DLASeg, 'feats_nhwc', lambda self, x, pre_img=None, pre_hm=None: 'feat')
    monkeypatch.setattr(DLASeg, 'forward_nhwc', lambda self, feat: z)
    out = DLASeg(34, HEADS, HEAD_CONVS, Opt(model_output_list=True))(None)
    assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], list)
    assert [float(t.flatten()[0]) for t in out[0]] == [float(list(HEADS).index(h)) for h in sorted(HEADS)]
    out = DLASeg(34, HEADS, HEAD_CONVS, Opt())(None)
    assert len(out) == 1 and isinstance(out[0], dict) and list(out[0]) == list(HEADS)
    assert all(out[0][h] is z[h] for h in HEADS)
