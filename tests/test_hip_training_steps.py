"""GPU: three optimizer steps through the drop-in ``DCN`` (under ``trainable()``) and the fused ``GenericLoss``, where the
other network tests stop after one.  What has to survive an iteration is seen three times: the weight packings after every
update, BatchNorm in training mode behind the DCN and its running statistics, ``zero_grad`` in both flavours (a fresh
``.grad`` and one accumulated into), the momentum buffers, ``trainable()`` switched off for an evaluation forward and on
again, the loss's per-call workspaces.

The network is the ``_Net`` of tests/test_hip_losses.py (DCN -> BatchNorm2d -> ReLU, one 1x1 convolution per head).  The
same trajectory -- same initial state, same inputs per step, SGD(lr=0.01, momentum=0.9) -- runs on ``oracle.dcn_v2.DCN``
with the mirror ``_loss_ref.generic_loss`` in float64 (the truth) and in float32 (the yardstick).  Error measure and bound
are those of tests/_dcn_bwd.py, applied to the accumulated update ``theta_t - theta_0`` of every parameter: largest element
error over the largest float64 update, ``<= min(1e-3, 4 * max(e32, 2^-23 * sqrt(K)))`` with e32 the float32 trajectory's
own error and K = B*H*W, the terms behind one element of a weight gradient."""
import numpy as np
import pytest
import torch

import _loss_ref as R
import test_hip_losses as T
from _dcn_bwd import bound, err

pytestmark = pytest.mark.gpu

HEADS = {'hm': 3, 'reg': 2, 'wh': 2, 'tracking': 2}
B, H, W, M = 2, 12, 20, 8
K = B * H * W
STEPS = 3
# Parameters that may differ between two runs: those downstream of the DCN's input gradient, the one result of
# ct_dcn_v2_backward that is summed with float atomics.  In this network the DCN reads the data tensor, which requires no
# gradient: that kernel does not run (tests/test_hip_dcn_backward.py::test_needs_input_grad_selects_the_kernels), the
# offset / mask gradients behind conv_offset_mask are bitwise reproducible, and the list is empty.
NOT_BITWISE = ()


def _step_inputs(t):
    """fresh inputs per step, seeds fixed"""
    _, batch = R.make_batch(310 + t, B, H, W, M, tuple(HEADS), 3)
    x = torch.randn(B, 32, H, W, generator=torch.Generator().manual_seed(320 + t))
    return x, batch


def _initial_state():
    from oracle import dcn_v2 as odcn
    torch.manual_seed(0)
    net = T._Net(odcn.DCN, HEADS)
    net.block[0].conv_offset_mask.weight.data.normal_(0.0, 0.03)
    net.block[0].conv_offset_mask.bias.data.normal_(0.0, 0.3)
    return {k: v.clone() for k, v in net.state_dict().items()}


def _state(model):
    """copies of the parameters and float buffers, float64 on the CPU"""
    return {k: v.detach().to('cpu', torch.float64, copy=True) for k, v in model.state_dict().items() if v.is_floating_point()}


def _trajectory(model, inputs, loss_of, forward=lambda model, x: model(x), after_step=None):
    """-> per step (loss, {name: state - initial state}, state); ``after_step(t, model)`` runs between two iterations"""
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    first = _state(model)
    steps = []
    for t, (x, batch) in enumerate(inputs):
        opt.zero_grad(set_to_none=t % 2 == 0)
        if t % 2:
            assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in model.parameters())
        tot = loss_of(forward(model, x), batch)
        tot.backward()
        opt.step()
        now = _state(model)
        steps.append((float(tot.detach()), {k: now[k] - first[k] for k in now}, now))
        if after_step is not None:
            after_step(t, model)
    return steps


@pytest.fixture(scope='module')
def reference():
    """the float64 and the float32 trajectory on the oracle, once"""
    from oracle import dcn_v2 as odcn
    init = _initial_state()
    weights = R.Opt(tuple(HEADS)).weights
    runs = {}
    for dt in (torch.float64, torch.float32):
        net = T._Net(odcn.DCN, HEADS)
        net.load_state_dict(init)
        net = net.to(dt)
        inputs = []
        for t in range(STEPS):
            x, batch = _step_inputs(t)
            inputs.append((x.to(dt), {k: (v.to(dt) if v.is_floating_point() else v) for k, v in batch.items()}))
        runs[dt] = _trajectory(net, inputs, lambda o, b: R.generic_loss(o, b, tuple(HEADS), weights)[0])
    return init, runs[torch.float64], runs[torch.float32]


def _hip_run(init, device, checks=True):
    from centertrack_amd import dcn_v2 as hip, losses, ops
    from oracle import dcn_v2 as odcn
    net = T._Net(hip.DCN, HEADS)
    net.load_state_dict(init)
    net = net.to(device)
    crit = losses.GenericLoss(R.Opt(tuple(HEADS)))
    inputs = [(x.to(device), T._to(batch, device)) for x, batch in (_step_inputs(t) for t in range(STEPS))]

    def evaluation_forward_and_packings(t, model):
        # 2. the evaluation forward at the current state, outside trainable(): the inference kernels, BatchNorm on its
        # running statistics, against the oracle loaded with that state
        assert not hip.is_trainable()
        model.eval()
        with torch.no_grad():
            got = model(inputs[t][0])[0]
        model.train()
        ref = T._Net(odcn.DCN, HEADS).eval()
        ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            want = ref(inputs[t][0].cpu())[0]
        for h in HEADS:
            np.testing.assert_allclose(got[h].cpu().numpy(), want[h].numpy(), atol=2e-4, rtol=1e-4, err_msg='step %d %s' % (t, h))
        # 3. the packings the next step will use are those of the updated weight
        dcn = model.block[0]
        wp, wT = dcn._packs()
        assert torch.equal(wp, ops.pack_weight(dcn.weight.detach())) and torch.equal(wT, ops.pack_weight_t(dcn.weight.detach()))

    def loss_of(outputs, batch):
        return crit(outputs, batch)[0]

    def forward(model, x):
        with hip.trainable():
            return model(x)

    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # (the torch layers around the DCN: no atomically summed weight gradients)
    try:
        steps = _trajectory(net, inputs, loss_of, forward, evaluation_forward_and_packings if checks else None)
    finally:
        torch.backends.cudnn.deterministic = det
    return steps


def test_three_sgd_steps_through_dcn_batchnorm_and_loss(device, reference):
    init, r64, r32 = reference
    steps = _hip_run(init, device)
    fails = []
    for t in range(STEPS):
        (l, d, now), (l64, d64, now64), (l32, d32, _) = steps[t], r64[t], r32[t]
        el, el32 = T._loss_err(l, l64), T._loss_err(l32, l64)
        bl = bound(el32, B * 3 * H * W)
        print('train step %d %-34s e(hip) %.3e  e(ref32) %.3e  bound %.3e' % (t, 'loss', el, el32, bl))
        if not el <= bl:
            fails.append((t, 'loss', el, bl))
        assert sorted(d) == sorted(d64)
        for n in sorted(d64):
            # (DCN.bias in front of a training-mode BatchNorm has a zero gradient in real arithmetic: its update is
            # measured against the update of the same module's weight, as in the one-step tests)
            norm = d64['block.0.weight'].abs().max() if n == 'block.0.bias' else None
            e, e32 = err(d[n], d64[n], norm), err(d32[n], d64[n], norm)
            b = bound(e32, K)
            print('train step %d %-34s e(hip) %.3e  e(ref32) %.3e  bound %.3e  max|update64| %.3e'
                  % (t, n, e, e32, b, float(d64[n].abs().max())))
            if not e <= b:
                fails.append((t, n, e, b))
            if n != 'block.0.bias':
                assert float(d64[n].abs().max()) > 0, n
    assert not fails, fails


def test_the_whole_run_repeats(device, reference):
    """losses and parameters bitwise, but for the parameters named in NOT_BITWISE, which agree within bound(0, K)"""
    init = reference[0]
    a, b = _hip_run(init, device, checks=False), _hip_run(init, device, checks=False)
    for t in range(STEPS):
        print('train repeat step %d loss %r %r' % (t, a[t][0], b[t][0]))
        for n in sorted(a[t][2]):
            diff = float((a[t][2][n] - b[t][2][n]).abs().max())
            if diff:
                print('train repeat step %d %-34s max difference %.3e' % (t, n, diff))
    for t in range(STEPS):
        assert a[t][0] == b[t][0], t
        for n in sorted(a[t][2]):
            if n in NOT_BITWISE:
                norm = a[t][1]['block.0.weight'].abs().max() if n == 'block.0.bias' else None
                assert err(a[t][1][n], b[t][1][n], norm) <= bound(0.0, K), (t, n)
            else:
                assert torch.equal(a[t][2][n], b[t][2][n]), (t, n)
