"""GPU: the DCNv2 backward (ct_dcn_v2_backward) behind centertrack_amd.dcn_v2 under ``trainable()``.

Truth is ``torch.autograd.grad`` of ``oracle.dcn_v2.dcn_v2_conv`` in float64 on the CPU, fed the fp32-rounded inputs;
the yardstick for fp32 noise is the same oracle in float32.  For a gradient tensor g, e(g) = max|g - g64| / max|g64|,
and the bound is

    e(hip) <= min(1e-3, 4 * max(e(oracle32), 2^-23 * sqrt(K)))

with K the number of terms behind one element (B*H*W for g_weight / g_bias, Cin*Cout for g_offset / g_mask, 36*Cout for
g_x): the HIP sums are the oracle's fp32 sums in another order (MFMA K order, slab order, atomic arrival), a wrong corner,
tap, sign or validity rule shows at 1e-2 and above.  Every element of every gradient is compared; nothing is excluded.
The figures are printed before they are asserted (DESIGN.md section 9 holds the measured table).

The second half of the file (lines printed as ``dcn_bwd*``) uses a sharper truth: the float64 oracle fed
``_dcn_bwd.effective_offsets``, whose sample positions are the fp32 sums the kernel and the float32 oracle form, bit for
bit.  Same error measure, same bound, e(oracle32) measured against that truth.  It covers every regime of the launch plan
(``_dcn_bwd.PLAN_SHAPES``: the DLA-34 neck at 512x512 and small shapes for the rest), designed sample positions on and around
the image border, the fp32 position rule, caller-owned output buffers and ordinary training code through the modules."""
import math

import numpy as np
import pytest
import torch

import _dcn_bwd as D

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W, offset scale): the four shapes of the specification, one with W off the 16-pixel tile and offsets of
# scale 8 on a 13 x 19 image (samples leave the image on all four sides), one with Cout (24) off the 16-wide MFMA tile
SHAPES = [(2, 64, 64, 16, 24, 2.0), (1, 256, 128, 8, 8, 0.0), (2, 128, 64, 9, 21, 0.5), (1, 64, 64, 64, 64, 2.0),
          (1, 64, 64, 13, 19, 8.0), (2, 64, 24, 12, 20, 2.0)]
NAMES = D.NAMES
_cache = {}
_randn, _inputs, _terms, _err, _bound = D.randn, D.inputs, D.terms, D.err, D.bound     # shared with the CPU tests


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


# ---------------------------------------------------------------------------------------------------------------------
# Below: the truth is float64 autograd of the oracle AT THE KERNEL'S SAMPLE POSITIONS (tests/_dcn_bwd.py::effective_offsets:
# the fp32 sum base + offset, not the exact one), so e(oracle32) measures summation order only and no input can put the two
# oracles into different cells.  Error measure and bound are the ones above; the float32 yardstick keeps the fp32 offsets.

def _compare(label, got, g64, e32, K, names=NAMES, scale=1.0):
    """print e(hip) / e(oracle32) / bound of every tensor, then return the ones over the bound.  ``scale``: the gradient
    is ``scale`` x g64 (accumulated passes); error and bound are both taken relative to max|g64|."""
    fails = []
    for n in names:
        assert got[n].shape == g64[n].shape and bool(torch.isfinite(got[n]).all()), n
        e, b = _err(got[n], scale * g64[n], g64[n].abs().max()), scale * _bound(e32[n], K[n])
        print('dcn_bwd* %s g_%-6s e(hip) %.3e  e(oracle32) %.3e  bound %.3e  max|g64| %.3e'
              % (label, n, e, e32[n], b, float(g64[n].abs().max())))
        if not e <= b:
            fails.append((n, e, b))
    return fails


@pytest.mark.parametrize('shape', SHAPES + D.PLAN_SHAPES, ids=D.shape_id)
def test_gradients_at_the_kernels_sample_positions(device, shape):
    """the six shapes above once more, against the sharper truth, and every regime of the launch plan (D.PLAN_SHAPES:
    the DLA-34 neck at 512x512 and the small shapes that reach what the neck does not; the CPU test
    test_plan_shapes_reach_every_regime_of_the_plan proves the coverage)"""
    inp, g64, e32 = D.truth_of_shape(shape)
    K = _terms(shape)
    p = D.plan(*shape[:5])
    print('dcn_bwd* %s plan CS %d slabs %d%s stepsPerWave %d cout groups %d (last %d tiles) idle steps %d (%d whole waves)'
          % (D.shape_id(shape), p['CS'], p['slabs'], ' (capped)' if p['capped'] else '', p['stepsPerWave'], p['groups'],
             p['nco_last'], p['idle_steps'], p['idle_waves']))
    _, got = _hip_grads(inp, device)
    fails = _compare(D.shape_id(shape), got, g64, e32, K)
    assert not fails, fails
    _, again = _hip_grads(inp, device)
    for n in ('offset', 'mask', 'weight', 'bias'):
        assert torch.equal(got[n], again[n]), 'g_%s differs between two runs' % n
    assert _err(again['x'], g64['x']) <= _bound(e32['x'], K['x'])


def _designed(B, Cin, Cout, H, W):
    """inputs whose sample positions are D.designed_positions (exact in fp32), masks random in (0, 1), gy random"""
    inp = _inputs((B, Cin, Cout, H, W, 0.0))
    pos, _ = D.designed_positions(B, H, W)
    inp[1] = (pos - D.tap_bases(H, W).unsqueeze(0)).float()
    assert torch.equal(inp[1].double() + D.tap_bases(H, W).unsqueeze(0), pos)
    return inp, pos[:, 0::2], pos[:, 1::2]


def _touched_cells(py, px, H, W):
    """the cells of the image one sample at (py, px) reads with a non-zero weight, from the definition of the op"""
    if py <= -1 or px <= -1 or py >= H or px >= W:
        return set()
    y0, x0 = math.floor(py), math.floor(px)
    rows = [(y0, 1.0 - (py - y0)), (y0 + 1, py - y0)]
    cols = [(x0, 1.0 - (px - x0)), (x0 + 1, px - x0)]
    return {(y, x) for y, wy in rows for x, wx in cols if wy > 0 and wx > 0 and 0 <= y <= H - 1 and 0 <= x <= W - 1}


@pytest.mark.parametrize('dims', [(3, 32, 16, 6, 7), (2, 64, 64, 8, 10)], ids=D.shape_id)
def test_designed_sample_positions(device, dims):
    """every pair of {-1.5, -1, -0.75, -0.5, 0, 0.25, 1, L-2, L-1.5, L-1, L-0.75, L-0.5, L, L+0.5} (rows x columns) in
    every image: outside (strict at -1 and L), the half-valid first and last cell, integers (one-sided derivative), the
    four corners.  Three images, so that row H of image n IS row 0 of image n + 1."""
    B, Cin, Cout, H, W = dims
    inp, py, px = _designed(B, Cin, Cout, H, W)
    _, pair = D.designed_positions(B, H, W)
    for n in range(B):
        assert sorted(set(pair[n].flatten().tolist())) == list(range(196))
    g64, e32 = D.truth(inp)
    K = _terms(dims)
    _, got = _hip_grads(inp, device)
    fails = _compare(D.shape_id(dims) + 'xdesigned', got, g64, e32, K)
    assert not fails, fails
    # known answers, independent of the oracle.  1: a sample at or beyond -1 / L reads nothing: exactly zero gradients
    outside = (py <= -1) | (py >= H) | (px <= -1) | (px >= W)                  # [B, 9, H, W]
    assert 0.2 * outside.numel() < int(outside.sum()) < 0.8 * outside.numel()
    for src in (got, g64):
        for name, g in (('dy', src['offset'][:, 0::2]), ('dx', src['offset'][:, 1::2]), ('mask', src['mask'])):
            assert bool((g[outside] == 0.0).all()), 'g_%s is not zero at a sample outside the image' % name
    at_last_row = (py == H - 1) & ~outside
    assert int(at_last_row.sum()) > 0 and float(got['offset'][:, 0::2][at_last_row].abs().max()) > 0.0
    # 2: ... so its mask is irrelevant: with those masks at 0, no other gradient changes a bit
    cut = [v.clone() for v in inp]
    cut[2][outside] = 0.0
    _, got0 = _hip_grads(cut, device)
    for n in ('offset', 'mask', 'weight', 'bias'):
        assert torch.equal(got[n], got0[n]), 'g_%s depends on the mask of a sample outside the image' % n
    # 3: gy non-zero at ONE pixel: g_x is non-zero exactly on the cells that pixel's nine samples read, one cell for a
    # tap at an integer position inside the image.  One pixel for each of the 16 integer pairs {0, 1, L-2, L-1}^2.
    done = 0
    for iy, ty in enumerate((0.0, 1.0, H - 2.0, H - 1.0)):
        for ix, tx in enumerate((0.0, 1.0, W - 2.0, W - 1.0)):
            n = (4 * iy + ix) % B
            hit = ((py[n] == ty) & (px[n] == tx)).nonzero()
            assert len(hit) > 0
            k, h, w = hit[0].tolist()
            assert len(_touched_cells(ty, tx, H, W)) == 1
            want = set()
            for t in range(9):
                want |= _touched_cells(float(py[n, t, h, w]), float(px[n, t, h, w]), H, W)
            one = [v.clone() for v in inp]
            one[5].zero_()
            one[5][n, :, h, w] = inp[5][n, :, h, w]
            _, gx = _hip_grads(one, device, needs=('x',))
            touched = (gx['x'] != 0.0).any(1)                                  # [B, H, W]
            have = {(y, x) for y, x in touched[n].nonzero().tolist()}
            assert have == want, ('pixel', (n, h, w), 'tap', k, 'g_x touches', sorted(have), 'expected', sorted(want))
            assert int(touched.sum()) == len(want), 'g_x of another image was touched'
            done += 1
    assert done == 16


def test_sample_positions_follow_the_fp32_sum(device):
    """offsets of +-2^-30, +-2^-26, -(1 - 2^-24) ... on every base from -1 to L: fl32(base + d) is an integer where the
    exact sum is not, so the exact sum reads another cell (or is inside where the fp32 one is outside, at -1 and L).  The
    kernel must follow the fp32 sum (make_samp: "ys is formed as the oracle forms it")."""
    B, Cin, Cout, H, W = dims = (3, 32, 16, 6, 7)
    inp = _inputs(dims + (0.0,))
    deltas = torch.tensor([2.0 ** -30, -2.0 ** -30, 2.0 ** -26, -2.0 ** -26, -(1.0 - 2.0 ** -24), 1.0 - 2.0 ** -24,
                           -(2.0 - 2.0 ** -23), 2.0 ** -25, -2.0 ** -25, 0.5, -(3.0 - 2.0 ** -22)], dtype=torch.float64)
    assert torch.equal(deltas.float().double(), deltas)
    s = torch.arange(B * H * W * 9).view(B, H, W, 9).permute(0, 3, 1, 2)
    off = torch.empty(B, 18, H, W, dtype=torch.float64)
    off[:, 0::2] = deltas[s % 11]
    off[:, 1::2] = deltas[(s // 11 + s) % 11]
    inp[1] = off.float()
    base = D.tap_bases(H, W).unsqueeze(0)
    L = torch.tensor([H, W] * 9, dtype=torch.float64).view(1, 18, 1, 1)

    def cells(pos):
        inside = ((pos > -1) & (pos < L))
        inside = inside[:, 0::2] & inside[:, 1::2]
        return torch.floor(pos[:, 0::2]), torch.floor(pos[:, 1::2]), inside

    fy, fx, ins = cells(base + D.effective_offsets(inp[1], H, W))
    ny, nx, nins = cells(base + off)
    differ = (ins != nins) | (ins & ((fy != ny) | (fx != nx)))
    print('dcn_bwd* fp32 position rule: %d of %d samples read another cell under the exact sum (%d change sides at -1 / L)'
          % (int(differ.sum()), differ.numel(), int((ins != nins).sum())))
    assert int(differ.sum()) >= 50 and int((ins != nins).sum()) >= 10
    g64, e32 = D.truth(inp)
    naive = D.oracle_grads(inp, torch.float64)
    assert _err(naive['offset'], g64['offset']) > 1e-2                         # the two truths are different functions here
    _, got = _hip_grads(inp, device)
    fails = _compare(D.shape_id(dims) + 'xfp32rule', got, g64, e32, _terms(dims))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# caller-owned output buffers (the C ABI takes ldgx >= Cin and ldgom >= 27: a channel slice of a wider buffer)

SENTINEL = -1234.5
BUF_SHAPE = (2, 128, 72, 9, 21, 0.5)


def _views(shape, device):
    from centertrack_amd import ops
    B, Cin, Cout, H, W, _ = shape
    inp, g64, e32 = D.truth_of_shape(shape)
    x, off, mask, w, _, gy = [v.to(device) for v in inp]
    om = torch.zeros((B, H, W, 32), device=device)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = mask.permute(0, 2, 3, 1)
    return (ops.View(x.permute(0, 2, 3, 1).contiguous()), ops.View(om, 0, 27), ops.View(gy.permute(0, 2, 3, 1).contiguous()),
            ops.pack_weight_t(w))


def _launch(d):
    import ctypes
    from centertrack_amd import _lib
    lib = _lib.load()
    need = lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device='cuda')
    if need:
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
    _lib.check(lib.ct_dcn_v2_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_dcn_v2_backward')
    torch.cuda.synchronize()


def test_outputs_as_channel_slices_leave_the_rest_of_the_buffer_alone(device):
    from centertrack_amd import ops
    shape = BUF_SHAPE
    B, Cin, Cout, H, W, _ = shape
    _, g64, e32 = D.truth_of_shape(shape)
    K = _terms(shape)
    x, om, gy, wT = _views(shape, device)
    gx_t = ops.View(torch.full((B, H, W, Cin), SENTINEL, device=device))
    gom_t = ops.View(torch.full((B, H, W, 32), SENTINEL, device=device), 0, 27)
    _launch(ops.make_dcn_bwd_desc(x, om, gy, wT, gx=gx_t, gom=gom_t))
    gxbuf = torch.full((B, H, W, Cin + 24), SENTINEL, device=device)
    gombuf = torch.full((B, H, W, 40), SENTINEL, device=device)
    gx_w, gom_w = ops.View(gxbuf, 8, Cin), ops.View(gombuf, 3, 27)
    d = ops.make_dcn_bwd_desc(x, om, gy, wT, gx=gx_w, gom=gom_w)
    assert (d.ldgx, d.ldgom) == (Cin + 24, 40)
    _launch(d)
    assert torch.equal(gombuf[..., 3:30], gom_t.buf[..., :27])
    got = {'x': gx_w.to_nchw().cpu(), 'offset': gombuf[..., 3:21].permute(0, 3, 1, 2).cpu(),
           'mask': gombuf[..., 21:30].permute(0, 3, 1, 2).cpu()}
    fails = _compare(D.shape_id(shape) + 'xslices', got, g64, e32, K, names=('x', 'offset', 'mask'))
    fails += _compare(D.shape_id(shape) + 'xtight', {'x': gx_t.to_nchw().cpu()}, g64, e32, K, names=('x',))
    assert not fails, fails
    for name, outside in (('gx', gxbuf[..., :8]), ('gx', gxbuf[..., 8 + Cin:]), ('gom', gombuf[..., :3]),
                          ('gom', gombuf[..., 30:]), ('gom (tight, pad)', gom_t.buf[..., 27:])):
        assert torch.equal(outside, torch.full_like(outside, SENTINEL)), '%s: a column outside the slice was written' % name


def test_a_second_launch_into_the_same_gx_starts_from_zero(device):
    from centertrack_amd import ops
    shape = BUF_SHAPE
    B, Cin, Cout, H, W, _ = shape
    _, g64, e32 = D.truth_of_shape(shape)
    x, om, gy, wT = _views(shape, device)
    gxbuf = torch.full((B, H, W, Cin + 24), SENTINEL, device=device)
    gx = ops.View(gxbuf, 8, Cin)
    d = ops.make_dcn_bwd_desc(x, om, gy, wT, gx=gx)
    for launch in (1, 2):
        _launch(d)
        fails = _compare(D.shape_id(shape) + 'xlaunch%d' % launch, {'x': gx.to_nchw().cpu()}, g64, e32, _terms(shape),
                         names=('x',))
        assert not fails, fails
    assert torch.equal(gxbuf[..., :8], torch.full_like(gxbuf[..., :8], SENTINEL))


def test_weight_gradient_without_a_bias_buffer(device):
    from centertrack_amd import _lib, ops
    shape = BUF_SHAPE
    B, Cin, Cout, H, W, _ = shape
    _, g64, e32 = D.truth_of_shape(shape)
    x, om, gy, _ = _views(shape, device)
    gw = torch.full((Cout, Cin, 3, 3), SENTINEL, device=device)
    gb = torch.full((Cout,), SENTINEL, device=device)
    _launch(ops.make_dcn_bwd_desc(x, om, gy, gw=gw, gb=gb))
    gw0 = torch.full((Cout, Cin, 3, 3), SENTINEL, device=device)
    d = ops.make_dcn_bwd_desc(x, om, gy, gw=gw0)
    assert d.flags == _lib.CT_DCN_BWD_WEIGHT and not d.gb
    _launch(d)
    assert torch.equal(gw0, gw)
    fails = _compare(D.shape_id(shape) + 'xweight', {'weight': gw.cpu(), 'bias': gb.cpu()}, g64, e32, _terms(shape),
                     names=('weight', 'bias'))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# ordinary training code through the modules

MOD_SHAPE = (2, 64, 40, 9, 13, 2.0)


def _module(shape, inp, device):
    from centertrack_amd import dcn_v2 as hip
    mod = hip.DCNv2(shape[1], shape[2], (3, 3), 1, 1).to(device)
    with torch.no_grad():
        mod.weight.copy_(inp[3])
        mod.bias.copy_(inp[4])
    return mod


def _leaves(inp, device):
    return [v.to(device).requires_grad_() for v in inp[:3]]


def _module_grads(mod, leaves):
    g = dict(zip(NAMES[:3], (v.grad.detach().cpu() for v in leaves)))
    g['weight'], g['bias'] = mod.weight.grad.detach().cpu(), mod.bias.grad.detach().cpu()
    return g


@pytest.mark.parametrize('loss', ['sum', 'every_other_channel'])
def test_module_backward_of_expanded_and_strided_grad_out(device, loss):
    """``y.sum().backward()`` hands backward a stride-0 grad_out, ``y[:, ::2].sum()`` a strided one with zeros between"""
    from centertrack_amd import dcn_v2 as hip
    shape = MOD_SHAPE
    inp = _inputs(shape)
    inp[5] = torch.ones_like(inp[5])
    if loss == 'every_other_channel':
        inp[5][:, 1::2] = 0.0
    g64, e32 = D.truth(inp)
    mod, leaves = _module(shape, inp, device), _leaves(inp, device)
    with hip.trainable():
        y = mod(*leaves)
        (y.sum() if loss == 'sum' else y[:, ::2].sum()).backward()
    fails = _compare(D.shape_id(shape) + 'x' + loss, _module_grads(mod, leaves), g64, e32, _terms(shape))
    assert not fails, fails


def test_module_backward_of_channels_last_and_sliced_inputs(device):
    from centertrack_amd import dcn_v2 as hip
    shape = MOD_SHAPE
    B, Cin, Cout, H, W, _ = shape
    inp, g64, e32 = D.truth_of_shape(shape)
    gy = inp[5].to(device)
    mod, leaves = _module(shape, inp, device), _leaves(inp, device)
    with hip.trainable():
        y = mod(*[v.contiguous(memory_format=torch.channels_last) for v in leaves])
        (y * gy.contiguous(memory_format=torch.channels_last)).sum().backward()
    fails = _compare(D.shape_id(shape) + 'xchannels_last', _module_grads(mod, leaves), g64, e32, _terms(shape))
    mod.zero_grad()
    wide = torch.full((B, Cin + 16, H, W), 3.0, device=device)
    wide[:, 8:8 + Cin] = inp[0].to(device)
    wide.requires_grad_()
    leaves = _leaves(inp, device)
    with hip.trainable():
        y = mod(wide[:, 8:8 + Cin], leaves[1], leaves[2])
        (y * gy).sum().backward()
    got = _module_grads(mod, [wide] + leaves[1:])
    assert float(got['x'][:, :8].abs().max()) == 0.0 and float(got['x'][:, 8 + Cin:].abs().max()) == 0.0
    got['x'] = got['x'][:, 8:8 + Cin]
    fails += _compare(D.shape_id(shape) + 'xchannel_slice', got, g64, e32, _terms(shape))
    assert not fails, fails


def test_two_backward_passes_and_two_micro_batches_accumulate(device):
    from centertrack_amd import dcn_v2 as hip
    shape = MOD_SHAPE
    inp, g64, e32 = D.truth_of_shape(shape)
    gy = inp[5].to(device)
    # retain_graph=True, backward twice: every .grad is the sum of two passes
    mod, leaves = _module(shape, inp, device), _leaves(inp, device)
    with hip.trainable():
        loss = (mod(*leaves) * gy).sum()
        loss.backward(retain_graph=True)
        once = _module_grads(mod, leaves)
        loss.backward()
    twice = _module_grads(mod, leaves)
    fails = _compare(D.shape_id(shape) + 'xonce', once, g64, e32, _terms(shape))
    fails += _compare(D.shape_id(shape) + 'xtwice', twice, g64, e32, _terms(shape), scale=2.0)
    for n in ('offset', 'mask', 'weight', 'bias'):                            # bitwise reproducible passes: exactly double
        assert torch.equal(twice[n], 2.0 * once[n]), n
    # one image per micro-batch: the parameters' .grad is the float64 gradient of the summed loss
    mod, leaves = _module(shape, inp, device), _leaves(inp, device)
    with hip.trainable():
        for n in range(shape[0]):
            (mod(*[v[n:n + 1] for v in leaves]) * gy[n:n + 1]).sum().backward()
    fails += _compare(D.shape_id(shape) + 'xmicro_batches', _module_grads(mod, leaves), g64, e32, _terms(shape))
    assert not fails, fails


@pytest.mark.parametrize('cls', ['DCNv2', 'DCN'])
def test_weight_changed_in_place_before_backward_raises(device, cls):
    """backward contracts gy with a transposed packing made at forward time: a weight updated in between must not be
    paired with it silently -- autograd's version check on the saved weight refuses the pass"""
    from centertrack_amd import dcn_v2 as hip
    shape = MOD_SHAPE
    inp = _inputs(shape)
    leaves = _leaves(inp, device)
    with hip.trainable():
        if cls == 'DCNv2':
            mod = _module(shape, inp, device)
            y = mod(*leaves)
        else:
            mod = hip.DCN(shape[1], shape[2], (3, 3), 1, 1).to(device)
            y = mod(leaves[0])
        with torch.no_grad():
            mod.weight.mul_(2.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            y.sum().backward()
    # a fresh forward picks the new weight up, in both packings
    from centertrack_amd import ops
    with hip.trainable():
        (mod(*leaves) if cls == 'DCNv2' else mod(leaves[0])).sum().backward()
    wp, wT = mod._packs()
    assert torch.equal(wT, ops.pack_weight_t(mod.weight.detach())) and torch.equal(wp, ops.pack_weight(mod.weight.detach()))
