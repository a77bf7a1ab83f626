"""CPU: what the trainable modules share (centertrack_amd/_train.py) -- the input check's messages word for word, the
re-exports under their earlier names, the direction of the imports and ``update_running_stats`` against ``nn.BatchNorm2d``."""
import ast
import os
import types

import pytest
import torch

from centertrack_amd import _train, dcn_v2, dla_base, dla_up, heads, ops
from centertrack_amd._lib import CTError

# the word each call site passes -> does that site check the rank
WORDS = {'centertrack_amd DCN': False, 'centertrack_amd neck': True, 'centertrack_amd backbone': True, 'FusedHeads': False,
         'heads_forward_train': False, 'heads_backward': False}


def on_device(dtype, shape):
    """what ``need_cuda`` reads of a CUDA tensor, built without one"""
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, device=torch.device('cuda:0'), shape=torch.Size(shape),
                                 dim=lambda: len(shape))


def message(fn, *args, **kw):
    with pytest.raises(CTError) as e:
        fn(*args, **kw)
    return str(e.value)


@pytest.mark.parametrize('what', list(WORDS), ids=lambda w: w.split()[-1])
def test_need_cuda_messages(what):
    dims = 4 if WORDS[what] else None
    assert message(_train.need_cuda, torch.zeros(1, 4, 2, 2), what, dims) == (
        '%s runs on an MI355X only (got a cpu tensor); no CPU fallback' % what)
    assert message(_train.need_cuda, on_device(torch.float64, (1, 4, 2, 2)), what, dims) == (
        '%s computes in fp32 (got torch.float64)' % what)
    three = on_device(torch.float32, (2, 3, 4))
    if WORDS[what]:
        assert message(_train.need_cuda, three, what) == '%s wants a 4-d tensor (got (2, 3, 4))' % what
    else:
        _train.need_cuda(three, what, dims=None)
    _train.need_cuda(on_device(torch.float32, (1, 4, 2, 2)), what, dims)


def test_call_sites_keep_their_messages():
    x = torch.zeros(1, 32, 2, 2)
    cpu = ' runs on an MI355X only (got a cpu tensor); no CPU fallback'
    assert message(dcn_v2.dcn_v2_conv, x, x[:, :18], x[:, :9], torch.zeros(32, 32, 3, 3), None) == 'centertrack_amd DCN' + cpu
    assert message(dcn_v2.DCN(32, 32, (3, 3), 1, 1), x) == 'centertrack_amd DCN' + cpu
    assert message(dla_up.to_nhwc, x) == 'centertrack_amd neck' + cpu
    assert message(dla_base.to_nhwc, x) == 'centertrack_amd backbone' + cpu
    assert message(dla_up.to_nhwc, on_device(torch.float32, (2, 3, 4))) == 'centertrack_amd neck wants a 4-d tensor (got (2, 3, 4))'
    assert message(dla_base.to_nhwc, on_device(torch.float64, (1, 4, 2, 2))) == 'centertrack_amd backbone computes in fp32 (got torch.float64)'
    assert message(dla_up.to_nhwc, on_device(torch.float32, (1, 6, 2, 2))) == 'centertrack_amd neck needs channels % 4 == 0 (got 6)'
    assert message(dla_base.to_nhwc, on_device(torch.float32, (1, 6, 2, 2))) == 'centertrack_amd backbone needs channels % 4 == 0 (got 6)'
    for word in ('heads_forward_train', 'heads_backward'):
        assert message(ops._head_tensor, x, word) == word + cpu
    fh = heads.FusedHeads({'hm': 1}, 16, 32)
    assert message(fh, x) == 'FusedHeads' + cpu
    assert message(fh.forward_nhwc, x.permute(0, 2, 3, 1)) == 'FusedHeads' + cpu
    assert message(fh, x[0]) == 'FusedHeads takes an NCHW tensor or an ops.View'
    assert message(fh.forward_nhwc, x[0]) == 'FusedHeads.forward_nhwc takes an [N,H,W,C] tensor'


def test_reexports_and_switch():
    for name in ('set_trainable', 'is_trainable', 'trainable'):
        assert getattr(dcn_v2, name) is getattr(_train, name)
    assert dla_up.update_running_stats is _train.update_running_stats
    assert dla_up.BN_MOMENTUM == _train.BN_MOMENTUM == 0.1
    for mod in (dla_up, dla_base):
        assert callable(mod.to_nhwc) and callable(mod.to_nchw)
    assert not hasattr(dcn_v2, '_differentiable') and not hasattr(dla_up, '_recording')
    assert _train.is_trainable() is False and _train.recording() is False
    with pytest.raises(RuntimeError, match='boom'):
        with dcn_v2.trainable():
            assert _train.is_trainable() is True and _train.recording() is True
            with torch.no_grad():
                assert _train.recording() is False
            raise RuntimeError('boom')
    assert _train.is_trainable() is False
    _train.set_trainable(True)
    try:
        with pytest.raises(RuntimeError, match='boom'):
            with dcn_v2.trainable(False):
                assert _train.is_trainable() is False
                raise RuntimeError('boom')
        assert _train.is_trainable() is True
    finally:
        _train.set_trainable(False)


def test_backbone_does_not_import_the_neck():
    with open(os.path.join(os.path.dirname(dla_base.__file__), 'dla_base.py')) as f:
        tree = ast.parse(f.read())
    froms = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert froms
    for n in froms:
        assert (n.module or '') != 'dla_up' and all(a.name != 'dla_up' for a in n.names), ast.dump(n)
    assert all(a.name.split('.')[-1] != 'dla_up' for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names)


@pytest.mark.parametrize('momentum', [0.1, None], ids=['momentum-0.1', 'cumulative'])
def test_update_running_stats_is_batchnorm_training_step(momentum):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn((2, 4, 3, 5), generator=g) * 2 + 3, torch.randn((2, 4, 3, 5), generator=g) - 2]
    want, got = torch.nn.BatchNorm2d(4, momentum=momentum).train(), torch.nn.BatchNorm2d(4, momentum=momentum)
    for x in xs:                                      # two steps: the cumulative average's factor changes with the counter
        want(x)
        x64 = x.double()
        _train.update_running_stats(got, x64.mean((0, 2, 3)).float(), x64.var((0, 2, 3), unbiased=False).float(), 2 * 3 * 5)
    torch.testing.assert_close(got.running_mean, want.running_mean, rtol=1e-6, atol=0)
    torch.testing.assert_close(got.running_var, want.running_var, rtol=1e-6, atol=0)
    assert int(got.num_batches_tracked) == int(want.num_batches_tracked) == 2
