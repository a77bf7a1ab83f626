"""GPU parity of the drop-in op boundaries: B1 ``DCN`` / ``DCNv2`` /
``dcn_v2_conv`` with upstream's signatures and state-dict keys, and B3 ``generic_decode``.
The checker is the CPU oracle (oracle/dcn_v2.py, oracle/decode.py); tolerance for the fp32
contraction with a different summation order: 2e-4 abs (north_star allows 1e-3); decode
indices / classes / gathered values bit-exact.  The modules follow parameters that change
between two calls by any means, writes through ``.data`` (which leave ``_version`` alone)
included: forward, and under ``trainable()`` the gradients, against the oracle on the
changed parameters."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


@pytest.mark.parametrize('cin,cout,shape', [(64, 64, (1, 16, 24)), (128, 64, (2, 9, 21)), (256, 128, (1, 8, 8))])
def test_DCN_module_is_upstream_DCN(device, cin, cout, shape):
    from centertrack_amd import dcn_v2 as hip
    from oracle import dcn_v2 as odcn
    ref = odcn.DCN(cin, cout, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
    ref.conv_offset_mask.weight.data = _rand(27, cin, 3, 3, seed=1, scale=0.03)
    ref.conv_offset_mask.bias.data = _rand(27, seed=2, scale=0.3)
    ref.bias.data = _rand(cout, seed=3)
    mod = hip.DCN(cin, cout, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
    assert list(mod.state_dict().keys()) == ['weight', 'bias', 'conv_offset_mask.weight', 'conv_offset_mask.bias']
    assert float(mod.conv_offset_mask.weight.abs().max()) == 0.0          # upstream init_offset()
    mod.load_state_dict(ref.state_dict())
    mod = mod.to(device)
    x = torch.relu(_rand(shape[0], cin, shape[1], shape[2], seed=4))
    with torch.no_grad():
        want = ref(x)
    got = mod(x.to(device))
    assert got.shape == want.shape and got.is_contiguous()
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-4)
    # weights are re-packed when a parameter changes in place
    with torch.no_grad():
        mod.weight.mul_(2.0)
        mod.bias.zero_()
        ref.weight.mul_(2.0)
        ref.bias.zero_()
        want2 = ref(x)
    np.testing.assert_allclose(mod(x.to(device)).cpu().numpy(), want2.numpy(), atol=4e-4, rtol=1e-4)


def test_DCNv2_and_functional(device):
    from centertrack_amd import dcn_v2 as hip
    from oracle import dcn_v2 as odcn
    x = _rand(2, 64, 11, 13, seed=5)
    off = _rand(2, 18, 11, 13, seed=6, scale=2.0)
    mask = torch.sigmoid(_rand(2, 9, 11, 13, seed=7))
    w, b = _rand(32, 64, 3, 3, seed=8, scale=1 / 24.), _rand(32, seed=9)
    want = odcn.dcn_v2_conv(x, off, mask, w, b)
    got = hip.dcn_v2_conv(x.to(device), off.to(device), mask.to(device), w.to(device), b.to(device), 1, 1, 1, 1)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-4)
    mod = hip.DCNv2(64, 32, (3, 3), 1, 1).to(device)
    with torch.no_grad():
        mod.weight.copy_(w)
        mod.bias.copy_(b)
    got = mod(x.to(device), off.to(device), mask.to(device))
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-4, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# parameters changed behind the version counter

STALE_SHAPE = (2, 64, 40, 9, 13, 2.0)        # (B, Cin, Cout, H, W, offset scale) of tests/_dcn_bwd.py::inputs
ATOL, RTOL = 2e-4, 1e-4


def _write_behind_the_version_counter(mod):
    """four writes through ``.data``: the storage changes, ``param._version`` need not (the reference's fill_up_weights
    and many checkpoint loaders write this way)"""
    mod.weight.data.mul_(2)
    if hasattr(mod, 'conv_offset_mask'):
        mod.conv_offset_mask.weight.data.normal_(0, 0.03)
    mod.bias.data.add_(1)
    w = mod.weight.data
    w[0] = 0


def _stale_module(cls, inp, device):
    from centertrack_amd import dcn_v2 as hip
    _, Cin, Cout = STALE_SHAPE[:3]
    mod = getattr(hip, cls)(Cin, Cout, (3, 3), 1, 1)
    mod.weight.data.copy_(inp[3])
    mod.bias.data.copy_(inp[4])
    if cls == 'DCN':
        mod.conv_offset_mask.weight.data.copy_(_rand(27, Cin, 3, 3, seed=1, scale=0.03))
        mod.conv_offset_mask.bias.data.copy_(_rand(27, seed=2, scale=0.3))
    return mod.to(device)


def _oracle_on(cls, mod, inp, dtype):
    """the oracle in ``dtype`` on the module's CURRENT parameters -> (y, d sum(y * gy) / d weight, ... / d input).  In
    float64 a DCNv2 gets the offsets whose sample positions are the fp32 sums of the kernel (_dcn_bwd.effective_offsets)."""
    import _dcn_bwd as D
    from oracle import dcn_v2 as odcn
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in mod.state_dict().items()}
    x = inp[0].clone().to(dtype).requires_grad_()
    if cls == 'DCN':
        y = odcn.dcn_forward(x, p['weight'], p['bias'], p['conv_offset_mask.weight'], p['conv_offset_mask.bias'])
    else:
        off = D.effective_offsets(inp[1], *inp[1].shape[2:]) if dtype == torch.float64 else inp[1]
        y = odcn.dcn_v2_conv(x, off, inp[2].to(dtype), p['weight'], p['bias'])
    gw, gx = torch.autograd.grad(y, [p['weight'], x], inp[5].to(dtype))
    return y.detach(), gw, gx


def _stale_call(cls, mod, inp, device, x=None):
    x = inp[0].to(device) if x is None else x
    return mod(x) if cls == 'DCN' else mod(x, inp[1].to(device), inp[2].to(device))


@pytest.mark.parametrize('cls', ['DCN', 'DCNv2'])
def test_a_write_through_data_reaches_the_next_inference_forward(device, cls):
    import _dcn_bwd as D
    inp = D.inputs(STALE_SHAPE)
    mod = _stale_module(cls, inp, device)
    before = _stale_call(cls, mod, inp, device).cpu()
    np.testing.assert_allclose(before.numpy(), _oracle_on(cls, mod, inp, torch.float32)[0].numpy(), atol=ATOL, rtol=RTOL)
    versions = [p._version for p in mod.parameters()]
    _write_behind_the_version_counter(mod)
    print('dropin stale %s inference: _version before the writes %s, after %s'
          % (cls, versions, [p._version for p in mod.parameters()]))
    want = _oracle_on(cls, mod, inp, torch.float32)[0]
    after = _stale_call(cls, mod, inp, device).cpu()
    # the changed weight alone moves the output by far more than the tolerance (bias + 1 is not packed and shows anyway)
    assert float((want - (before + 1)).abs().max()) > 100 * ATOL and float((want - before).abs().max()) > 100 * ATOL
    np.testing.assert_allclose(after.numpy(), want.numpy(), atol=ATOL, rtol=RTOL)
    assert float(after[:, 0].sub(mod.bias.data[0].cpu()).abs().max()) == 0.0             # w[0] = 0: the bias alone


@pytest.mark.parametrize('cls', ['DCN', 'DCNv2'])
def test_a_write_through_data_reaches_the_next_training_step(device, cls):
    """under ``trainable()``: the forward packing feeds y, the transposed packing the input gradient (and, for DCN, the
    offset / mask gradients behind it); weight.grad is contracted from x and gy, it is here for completeness"""
    import _dcn_bwd as D
    from centertrack_amd import dcn_v2 as hip
    inp = D.inputs(STALE_SHAPE)
    B, Cin, Cout, H, W, _ = STALE_SHAPE
    mod = _stale_module(cls, inp, device)
    gy = inp[5].to(device)

    def step():
        x = inp[0].to(device).requires_grad_()
        mod.zero_grad()
        with hip.trainable():
            y = _stale_call(cls, mod, inp, device, x)
            (y * gy).sum().backward()
        return y.detach().cpu(), mod.weight.grad.detach().cpu(), x.grad.detach().cpu()

    y0, gw0, gx0 = step()
    _write_behind_the_version_counter(mod)
    y64, gw64, gx64 = _oracle_on(cls, mod, inp, torch.float64)
    y32, gw32, gx32 = _oracle_on(cls, mod, inp, torch.float32)
    y1, gw1, gx1 = step()
    assert float((y32 - y0).abs().max()) > 100 * ATOL
    np.testing.assert_allclose(y1.numpy(), y32.numpy(), atol=ATOL, rtol=RTOL)
    # K: the terms behind one element (tests/_dcn_bwd.py::terms); through DCN the input gradient has the 27 * 9 terms of
    # the offset / mask convolution's backward on top
    K = {'weight': B * H * W, 'x': 36 * Cout + (27 * 9 if cls == 'DCN' else 0)}
    fails = []
    for n, got, old, g64, g32 in (('weight', gw1, gw0, gw64, gw32), ('x', gx1, gx0, gx64, gx32)):
        e, e32, stale = D.err(got, g64), D.err(g32, g64), D.err(old, g64)
        b = D.bound(e32, K[n])
        print('dropin stale %s g_%-6s e(hip) %.3e  e(oracle32) %.3e  bound %.3e  e(gradient before the writes) %.3e'
              % (cls, n, e, e32, b, stale))
        if not e <= b:
            fails.append((n, e, b))
        if n == 'x':
            assert stale > 100 * b             # the old gradient would not pass
    assert not fails, fails


def test_DCN_rejects_what_it_does_not_implement(device):
    from centertrack_amd import _lib, dcn_v2 as hip
    with pytest.raises(_lib.CTError):
        hip.DCN(64, 64, (3, 3), 2, 1)                    # stride 2
    with pytest.raises(_lib.CTError):
        hip.DCN(48, 64, (3, 3), 1, 1)                    # Cin % 32
    mod = hip.DCN(64, 64, (3, 3), 1, 1)
    with pytest.raises(_lib.CTError):
        mod(torch.zeros(1, 64, 8, 8))                    # CPU tensor: no fallback


def test_generic_decode_dropin(device):
    from types import SimpleNamespace
    import scenarios as S
    from centertrack_amd.decode import generic_decode
    from oracle import decode as odecode
    assert generic_decode({'reg': torch.zeros(1, 2, 4, 4)}, 10, None) == {}
    for case in S.decode_cases():
        maps = S.make_head_maps(case)
        want = odecode.generic_decode({k: v.clone() for k, v in maps.items()}, K=case['K'])
        out = {k: v.to(device) for k, v in maps.items()}
        got = generic_decode(out, case['K'], SimpleNamespace(zero_tracking=False))
        assert set(got.keys()) == set(want.keys()), case['name']
        for k, v in want.items():
            assert got[k].dtype == torch.float32 and tuple(got[k].shape) == tuple(v.shape), (case['name'], k)
            if k == 'kps_score':       # (mean over joints: summation order not restated)
                np.testing.assert_allclose(got[k].cpu().numpy(), v.numpy(), rtol=1e-5, atol=1e-7)
                continue
            np.testing.assert_array_equal(got[k].cpu().numpy(), v.numpy(), err_msg='%s.%s' % (case['name'], k))
    # zero_tracking mutates the caller's dict in place (decode.py:88-89)
    case = S.decode_cases()[0]
    maps = {k: v.to(device) for k, v in S.make_head_maps(case).items()}
    got = generic_decode(maps, case['K'], SimpleNamespace(zero_tracking=True))
    assert float(maps['tracking'].abs().max()) == 0.0 and float(got['tracking'].abs().max()) == 0.0
