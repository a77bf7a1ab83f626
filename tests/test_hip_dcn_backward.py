"""GPU: the DCNv2 backward (ct_dcn_v2_backward) behind centertrack_amd.dcn_v2 under ``trainable()``.

Truth is ``torch.autograd.grad`` of ``oracle.dcn_v2.dcn_v2_conv`` in float64 on the CPU, fed the fp32-rounded inputs;
the yardstick for fp32 noise is the same oracle in float32.  For a gradient tensor g, e(g) = max|g - g64| / max|g64|,
and the bound is

    e(hip) <= min(1e-3, 4 * max(e(oracle32), 2^-23 * sqrt(K)))

with K the number of terms behind one element (B*H*W for g_weight / g_bias, Cin*Cout for g_offset / g_mask, 36*Cout for
g_x): the HIP sums are the oracle's fp32 sums in another order (MFMA K order, slab order, atomic arrival), a wrong corner,
tap, sign or validity rule shows at 1e-2 and above.  Every element of every gradient is compared; nothing is excluded.
The figures are printed before they are asserted (DESIGN.md section 9 holds the measured table)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W, offset scale): the four shapes of the specification, one with W off the 16-pixel tile and offsets of
# scale 8 on a 13 x 19 image (samples leave the image on all four sides), one with Cout (24) off the 16-wide MFMA tile
SHAPES = [(2, 64, 64, 16, 24, 2.0), (1, 256, 128, 8, 8, 0.0), (2, 128, 64, 9, 21, 0.5), (1, 64, 64, 64, 64, 2.0),
          (1, 64, 64, 13, 19, 8.0), (2, 64, 24, 12, 20, 2.0)]
NAMES = ('x', 'offset', 'mask', 'weight', 'bias')
_cache = {}


def _randn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _inputs(shape):
    B, Cin, Cout, H, W, scale = shape
    t = (_randn(1, B, Cin, H, W), _randn(2, B, 18, H, W) * scale, torch.sigmoid(_randn(3, B, 9, H, W)),
         _randn(4, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5, _randn(5, Cout), _randn(6, B, Cout, H, W))
    return [v.float() for v in t]


def _terms(shape):
    B, Cin, Cout, H, W, _ = shape
    return {'x': 36 * Cout, 'offset': Cin * Cout, 'mask': Cin * Cout, 'weight': B * H * W, 'bias': B * H * W}


def _err(g, g64, norm=None):
    return float((g.double() - g64).abs().max() / (g64.abs().max() if norm is None else norm))


def _bound(e32, K):
    return min(1e-3, 4.0 * max(e32, 2.0 ** -23 * math.sqrt(K)))


def _oracle(shape):
    """(inputs, float64 gradients, e(oracle32) per tensor) of a shape, computed once"""
    if shape not in _cache:
        from oracle import dcn_v2 as odcn
        inp = _inputs(shape)
        grads = {}
        for dt in (torch.float64, torch.float32):
            t = [v.clone().to(dt).requires_grad_() for v in inp[:5]]
            y = odcn.dcn_v2_conv(*t)
            grads[dt] = dict(zip(NAMES, torch.autograd.grad(y, t, inp[5].to(dt))))
        e32 = {n: _err(grads[torch.float32][n], grads[torch.float64][n]) for n in NAMES}
        _cache[shape] = (inp, grads[torch.float64], e32)
    return _cache[shape]


def _hip_grads(inp, device, needs=NAMES):
    from centertrack_amd import dcn_v2 as hip
    t = [v.detach().to(device).requires_grad_(n in needs) for n, v in zip(NAMES, inp[:5])]
    with hip.trainable():
        y = hip.dcn_v2_conv(*t)
    assert y.grad_fn is not None
    wanted = [v for n, v in zip(NAMES, t) if n in needs]
    got = torch.autograd.grad(y, wanted, inp[5].to(device))
    return y, {n: g.cpu() for n, g in zip([n for n in NAMES if n in needs], got)}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_gradients_match_the_float64_oracle_and_repeat(device, shape):
    inp, g64, e32 = _oracle(shape)
    K = _terms(shape)
    _, got = _hip_grads(inp, device)
    fails = []
    for n in NAMES:
        assert got[n].shape == g64[n].shape and bool(torch.isfinite(got[n]).all()), n
        e, b = _err(got[n], g64[n]), _bound(e32[n], K[n])
        print('dcn_bwd %s g_%-6s e(hip) %.3e  e(oracle32) %.3e  bound %.3e  max|g64| %.3e'
              % ('x'.join(str(v) for v in shape), n, e, e32[n], b, float(g64[n].abs().max())))
        if not e <= b:
            fails.append((n, e, b))
    assert not fails, fails
    if shape[5] == 0.0:          # integer sample positions: the one-sided derivative, not zero
        assert float(got['offset'].abs().max()) > 1e-3 * float(g64['offset'].abs().max()) > 0.0
    # a second run on the same inputs: everything but g_x (float atomics) is bitwise equal
    _, again = _hip_grads(inp, device)
    for n in ('offset', 'mask', 'weight', 'bias'):
        assert torch.equal(got[n], again[n]), 'g_%s differs between two runs' % n
    assert _err(again['x'], g64['x']) <= _bound(e32['x'], K['x'])


def test_needs_input_grad_selects_the_kernels(device, monkeypatch):
    from centertrack_amd import ops
    shape = SHAPES[0]
    inp, g64, e32 = _oracle(shape)
    _, full = _hip_grads(inp, device)
    calls = []
    real = ops.dcn_v2_backward

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((kw, out))
        return out

    monkeypatch.setattr(ops, 'dcn_v2_backward', spy)
    _, only_w = _hip_grads(inp, device, needs=('weight',))
    kw, (gx, gom, gw, gb) = calls.pop()
    assert kw['need_w'] and not (kw['need_x'] or kw['need_om'] or kw['need_b'])
    assert gx is None and gom is None and gb is None             # no g_x buffer exists, no data kernel ran
    assert torch.equal(only_w['weight'], full['weight'])
    _, only_x = _hip_grads(inp, device, needs=('x',))
    kw, (gx, gom, gw, gb) = calls.pop()
    assert kw['need_x'] and not (kw['need_om'] or kw['need_w'] or kw['need_b'])
    assert gom is None and gw is None and gb is None
    assert _err(only_x['x'], g64['x']) <= _bound(e32['x'], _terms(shape)['x'])
    _, only_om = _hip_grads(inp, device, needs=('offset', 'mask'))
    kw, (gx, gom, gw, gb) = calls.pop()
    assert gx is None and gw is None
    assert torch.equal(only_om['offset'], full['offset']) and torch.equal(only_om['mask'], full['mask'])


def test_forward_under_trainable_is_the_inference_forward(device):
    from centertrack_amd import dcn_v2 as hip
    from oracle import dcn_v2 as odcn
    inp, _, _ = _oracle(SHAPES[0])
    t = [v.to(device) for v in inp[:5]]
    plain = hip.dcn_v2_conv(*t)
    assert plain.grad_fn is None and not hip.is_trainable()
    y, _ = _hip_grads(inp, device)
    assert torch.equal(y.detach(), plain)
    mod = hip.DCNv2(64, 64, (3, 3), 1, 1).to(device)
    with torch.no_grad():
        mod.weight.copy_(t[3])
        mod.bias.copy_(t[4])
    plain = mod(t[0], t[1], t[2])
    assert plain.grad_fn is None
    with hip.trainable():
        y = mod(t[0], t[1], t[2])
        assert y.grad_fn is not None
        with torch.no_grad():
            assert mod(t[0], t[1], t[2]).grad_fn is None
    assert torch.equal(y.detach(), plain)
    ref = odcn.DCN(64, 64, (3, 3), 1, 1)
    ref.conv_offset_mask.weight.data = (_randn(11, 27, 64, 3, 3) * 0.03).float()
    ref.conv_offset_mask.bias.data = (_randn(12, 27) * 0.3).float()
    dcn = hip.DCN(64, 64, (3, 3), 1, 1)
    dcn.load_state_dict(ref.state_dict())
    dcn = dcn.to(device)
    with torch.no_grad():
        want = ref(inp[0])
    with hip.trainable():
        got = dcn(t[0])
    assert got.grad_fn is not None
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-4)


def test_backward_raises_while_the_switch_is_off(device):
    from centertrack_amd import dcn_v2 as hip
    dcn = hip.DCN(64, 32, (3, 3), 1, 1).to(device)
    x = _randn(1, 1, 64, 8, 8).float().to(device).requires_grad_()
    assert not hip.is_trainable()
    with pytest.raises(RuntimeError, match='does not require grad'):
        dcn(x).sum().backward()


def _deform_net(dcn_cls):
    """the reference's DeformConv block (DCN -> BatchNorm2d -> ReLU, dla.py), two of them: 64 -> 64 -> 32"""
    from torch import nn

    def block(chi, cho):
        return nn.Sequential(dcn_cls(chi, cho, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1),
                             nn.BatchNorm2d(cho, momentum=0.1), nn.ReLU(inplace=True))

    return nn.Sequential(block(64, 64), block(64, 32))


@pytest.mark.parametrize('init', ['zero', 'random'])
def test_one_training_step_through_two_deformconv_blocks(device, init):
    from centertrack_amd import dcn_v2 as hip
    from oracle import dcn_v2 as odcn
    torch.manual_seed(0)
    ref32 = _deform_net(odcn.DCN).train()
    if init == 'random':
        for blk in ref32:
            blk[0].conv_offset_mask.weight.data.normal_(0.0, 0.03)
            blk[0].conv_offset_mask.bias.data.normal_(0.0, 0.3)
    x = torch.randn(2, 64, 24, 40)
    target = torch.randn(2, 32, 24, 40)
    ref64 = _deform_net(odcn.DCN).train()
    ref64.load_state_dict(ref32.state_dict())
    ref64 = ref64.double()
    net = _deform_net(hip.DCN).train()
    net.load_state_dict(ref32.state_dict())
    net = net.to(device)

    def run(model, x, target):
        x = x.clone().requires_grad_()
        loss = torch.nn.functional.mse_loss(model(x), target)
        loss.backward()
        g = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
        g['input'] = x.grad.detach().cpu()
        return g

    g64 = run(ref64, x.double(), target.double())
    g32 = run(ref32, x, target)
    with hip.trainable():
        got = run(net, x.to(device), target.to(device))
    assert sorted(got) == sorted(g64)
    K = 2 * 24 * 40
    fails = []
    for n in sorted(g64):
        # DCN.bias in front of a training-mode BatchNorm has a zero gradient in real arithmetic (pure rounding in
        # fp32): it is measured against the size of the same module's weight gradient
        norm = g64[n.replace('.bias', '.weight')].abs().max() if n.endswith('.0.bias') else None
        e, e32 = _err(got[n], g64[n], norm), _err(g32[n], g64[n], norm)
        b = _bound(e32, K)
        print('dcn_bwd net[%s] %-30s e(hip) %.3e  e(oracle32) %.3e  bound %.3e  max|g64| %.3e'
              % (init, n, e, e32, b, float(g64[n].abs().max())))
        if not e <= b:
            fails.append((n, e, b))
    assert not fails, fails
    if init == 'zero':          # offset gradients flow from upstream's zero init
        for i in (0, 1):
            n = '%d.0.conv_offset_mask.weight' % i
            assert float(g64[n].abs().max()) > 1e-3 and float(got[n].abs().max()) > 0.5 * float(g64[n].abs().max())
    # one SGD step on both sides, then the plain inference forward: the cached packings follow the in-place update
    torch.optim.SGD(net.parameters(), lr=0.05).step()
    torch.optim.SGD(ref32.parameters(), lr=0.05).step()
    assert not hip.is_trainable()
    with torch.no_grad():
        want = ref32(x)
    out = net(x.to(device))
    np.testing.assert_allclose(out.detach().cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-4)
    from centertrack_amd import ops
    for blk in net:             # ... and so does the transposed packing the next backward will use
        wp, wT = blk[0]._packs()
        assert torch.equal(wp, ops.pack_weight(blk[0].weight.detach()))
        assert torch.equal(wT, ops.pack_weight_t(blk[0].weight.detach()))


def test_views_inside_wider_buffers_give_the_same_gradients(device):
    """the C entry point works on NHWC views (channel slices of wider concat buffers, ld > C), like the forward"""
    from centertrack_amd import ops
    shape = SHAPES[2]
    B, Cin, Cout, H, W, _ = shape
    inp, g64, e32 = _oracle(shape)
    x, off, mask, w, _, gy = [v.to(device) for v in inp]
    om = torch.zeros((B, H, W, 32), device=device)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = mask.permute(0, 2, 3, 1)
    wT = ops.pack_weight_t(w)

    def run(xv, gyv):
        gx, gom, gw, gb = ops.dcn_v2_backward(xv, ops.View(om, 0, 27), gyv, wT)
        torch.cuda.synchronize()
        return gx.to_nchw().cpu(), gom.buf[..., :27].cpu(), gw.cpu(), gb.cpu()

    tight = run(ops.View(x.permute(0, 2, 3, 1).contiguous()), ops.View(gy.permute(0, 2, 3, 1).contiguous()))
    xw = torch.full((B, H, W, Cin + 96), 7.0, device=device)
    xw[..., 32:32 + Cin] = x.permute(0, 2, 3, 1)
    gw_ = torch.full((B, H, W, Cout + 20), -3.0, device=device)
    gw_[..., 4:4 + Cout] = gy.permute(0, 2, 3, 1)
    wide = run(ops.View(xw, 32, Cin), ops.View(gw_, 4, Cout))
    for a, b in zip(tight[1:], wide[1:]):
        assert torch.equal(a, b)
    K = _terms(shape)
    assert _err(wide[0], g64['x']) <= _bound(e32['x'], K['x'])
    assert _err(wide[2], g64['weight']) <= _bound(e32['weight'], K['weight'])
    assert _err(wide[1][..., :18].permute(0, 3, 1, 2), g64['offset']) <= _bound(e32['offset'], K['offset'])
