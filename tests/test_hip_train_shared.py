"""GPU: the shared pieces of the training layer (centertrack_amd/_train.py, ``ops.conv_backward_input``, ``ops._workspace``).
``conv_backward_input`` is held bit for bit against the form its three call sites spelled out before it existed (transpose,
flip, ``pack_weight``, ``conv2d``, written out here) and against float64 torch autograd on the CPU with the project's bound
(tests/_dcn_bwd.py): ``min(1e-3, 4 max(e32, 2^-23 sqrt(K)))``, K = Cout ks^2 -- the terms of one element of the input gradient
-- and e32 the float32 CPU autograd's own error.  ``bn_statistics`` is held against ``ops.bn_stats`` and
``update_running_stats``, bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from _dcn_bwd import bound, err, randn

pytestmark = pytest.mark.gpu

#          N  H  W  Cin Cout: ragged W and two images; a one-tile map
SHAPES = [(2, 5, 7, 16, 32), (1, 3, 9, 32, 16)]


def nhwc_view(t, dev, ld=None, fill=7.0):
    """NCHW CPU tensor -> NHWC view on the device: channels 0 .. C of a buffer of pitch ``ld`` (``fill`` behind them)"""
    from centertrack_amd import ops
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, ld or C), fill, dtype=torch.float32)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(dev), 0, C)


def autograd_gx(gy, w, res, dtype, Cin):
    """the input gradient of ``F.conv2d`` on the CPU in ``dtype`` (+ res)"""
    N, _, H, W = gy.shape
    x = torch.zeros((N, Cin, H, W), dtype=dtype, requires_grad=True)
    gx, = torch.autograd.grad(F.conv2d(x, w.to(dtype), padding=w.shape[2] // 2), x, gy.to(dtype))
    return gx if res is None else gx + res.to(dtype)


def held(tag, got, gy, w, res, Cin):
    t64, t32 = autograd_gx(gy, w, res, torch.float64, Cin), autograd_gx(gy, w, res, torch.float32, Cin)
    e, e32 = err(got.to_nchw().cpu(), t64), err(t32, t64)
    b = bound(e32, w.shape[0] * w.shape[2] * w.shape[3])
    print('%s err %.2e  e32 %.2e  bound %.2e' % (tag, e, e32, b))
    assert e <= b, '%s: err %.2e > bound %.2e' % (tag, e, b)


@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('ks', [1, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_conv_backward_input(device, shape, ks, with_res):
    from centertrack_amd import ops
    N, H, W, Cin, Cout = shape
    gy, w = randn(1, N, Cout, H, W).float(), (randn(2, Cout, Cin, ks, ks) / (Cin * ks * ks) ** 0.5).float()
    res = randn(3, N, Cin, H, W).float() if with_res else None
    gyv, wd = nhwc_view(gy, device), w.to(device)
    resv = None if res is None else nhwc_view(res, device)
    got = ops.conv_backward_input(gyv, wd, res=resv)
    wt = wd.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    want = ops.conv2d(gyv, ops.pack_weight(wt), Cin, ks, 1, res=resv)
    assert (got.N, got.H, got.W, got.C) == (N, H, W, Cin) and torch.equal(got.buf, want.buf)
    held('conv_backward_input %s ks%d %s' % (shape, ks, 'res' if with_res else 'plain'), got, gy, w, res, Cin)
    # a caller-owned output with a pitch wider than Cin: the same bits in the view, nothing behind it
    obuf = torch.full((N, H, W, Cin + 8), 7.0, device=device)
    out = ops.conv_backward_input(gyv, wd, res=resv, out=ops.View(obuf, 0, Cin))
    assert out.buf is obuf and torch.equal(obuf[..., :Cin], want.buf[..., :Cin]) and bool((obuf[..., Cin:] == 7.0).all())


def test_conv_backward_input_padded(device):
    """the DeformConv's offset/mask conv: 27 channels in a 32-wide buffer whose five pad channels hold zeros"""
    from centertrack_amd import ops
    N, H, W, Cin = 2, 5, 7, 32
    gom, w = randn(4, N, 27, H, W).float(), (randn(5, 27, Cin, 3, 3) / (Cin * 9) ** 0.5).float()
    res = randn(6, N, Cin, H, W).float()
    gomv, resv, wd = nhwc_view(gom, device, ld=32, fill=0.0), nhwc_view(res, device), w.to(device)
    assert (gomv.C, gomv.ld) == (27, 32)
    got = ops.conv_backward_input(gomv, wd, res=resv, out=ops.new_view(N, H, W, Cin, device))
    wt = torch.zeros((Cin, 32, 3, 3), dtype=torch.float32, device=device)
    wt[:, :27] = wd.permute(1, 0, 2, 3).flip(2, 3)
    want = ops.conv2d(ops.View(gomv.buf, 0, 32), ops.pack_weight(wt), Cin, 3, 1, res=resv, out=ops.new_view(N, H, W, Cin, device))
    assert torch.equal(got.buf, want.buf)
    held('conv_backward_input padded', got, gom, w, res, Cin)
    # a view that does not start its buffer cannot be widened
    with pytest.raises(ops._lib.CTError, match='conv_backward_input'):
        ops.conv_backward_input(ops.View(gomv.buf, 4, 27), wd)


def bn_view(device, shape=(2, 3, 5, 16)):
    from centertrack_amd import ops
    N, H, W, C = shape
    return ops.View((randn(7, N, H, W, C) * 2 + 1).float().to(device))


def test_bn_statistics_eval_mode(device, monkeypatch):
    from centertrack_amd import _train, ops
    z = bn_view(device)
    bn = torch.nn.BatchNorm2d(16).to(device).eval()
    with torch.no_grad():
        bn.running_mean.copy_(randn(8, 16)); bn.running_var.copy_(randn(9, 16).abs() + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()

    def never(*a, **k):
        raise AssertionError('eval-mode statistics launch nothing but the rsqrt')
    monkeypatch.setattr(ops, 'bn_stats', never)
    monkeypatch.setattr(_train, 'update_running_stats', never)
    mean, invstd, batch = _train.bn_statistics(bn, z, 'backbone')
    assert mean is bn.running_mean and batch is False
    assert torch.equal(invstd, torch.rsqrt(rv + bn.eps))
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == 0
    assert _train.saved_mean(mean, batch) is not mean and torch.equal(_train.saved_mean(mean, batch), rm)


@pytest.mark.parametrize('momentum', [0.1, None], ids=['momentum-0.1', 'cumulative'])
def test_bn_statistics_training_mode(device, momentum):
    from centertrack_amd import _train, ops
    z = bn_view(device)
    bn, twin = (torch.nn.BatchNorm2d(16, momentum=momentum).to(device).train() for _ in range(2))
    for step in range(2):
        mean, invstd, batch = _train.bn_statistics(bn, z, 'backbone')
        m, var, inv = ops.bn_stats(z, twin.eps)
        _train.update_running_stats(twin, m, var, 2 * 3 * 5)
        assert batch is True and torch.equal(mean, m) and torch.equal(invstd, inv)
        assert _train.saved_mean(mean, batch) is mean
    assert torch.equal(bn.running_mean, twin.running_mean) and torch.equal(bn.running_var, twin.running_var)
    assert int(bn.num_batches_tracked) == int(twin.num_batches_tracked) == 2


def test_bn_statistics_without_running_statistics(device):
    from centertrack_amd import _train, ops
    z = bn_view(device)
    bn = torch.nn.BatchNorm2d(16, track_running_stats=False).to(device).eval()
    mean, invstd, batch = _train.bn_statistics(bn, z, 'backbone')
    m, _, inv = ops.bn_stats(z, bn.eps)
    assert batch is True and torch.equal(mean, m) and torch.equal(invstd, inv)
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None


@pytest.mark.parametrize('what', ['DeformConv', 'backbone'])
def test_bn_statistics_refuses_one_value_per_channel(device, what):
    from centertrack_amd import _train
    from centertrack_amd._lib import CTError
    bn = torch.nn.BatchNorm2d(16).to(device).train()
    with pytest.raises(CTError) as e:
        _train.bn_statistics(bn, bn_view(device, (1, 1, 1, 16)), what)
    assert str(e.value) == '%s: training-mode BatchNorm needs more than one value per channel (N*H*W == 1)' % what
    assert int(bn.num_batches_tracked) == 0
    _train.bn_statistics(bn.eval(), bn_view(device, (1, 1, 1, 16)), what)        # running statistics: nothing to refuse


def test_conv2d_without_a_workspace(device):
    """a launch that splits nothing asks for 0 bytes: with ``optional`` that is "none needed", not a rejected descriptor"""
    import ctypes
    from centertrack_amd import _lib, ops
    x = nhwc_view(randn(10, 1, 16, 4, 4).float(), device)
    wp = ops.pack_weight((randn(11, 16, 16, 1, 1) / 4).float().to(device))
    d = ops.make_conv_desc(x, wp, 16, 1, 1, out=ops.new_view(1, 4, 4, 16, device))
    lib = _lib.load()
    assert lib.ct_conv2d_workspace_bytes(ctypes.byref(d)) == 0
    assert ops._workspace(lib, 'ct_conv2d_workspace_bytes', d, device, optional=True) is None and not d.workspace
    with pytest.raises(_lib.CTError, match='ct_conv2d_workspace_bytes'):
        ops._workspace(lib, 'ct_conv2d_workspace_bytes', d, device)
    y = ops.conv2d(x, wp, 16, 1, 1)
    assert torch.equal(y.buf, ops.conv2d(x, wp, 16, 1, 1, split_k=1).buf)
