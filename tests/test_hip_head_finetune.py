"""GPU: head fine-tuning of ``DLASegHIP`` end to end (``heads.HeadFinetuner`` + ``losses.GenericLoss``) at 128x160 input
(feature map 32x40), B = 2, MOT heads, a synthetic state dict; targets from ``_loss_ref.make_batch``.

Trajectory.  Three ``SGD(lr=0.01, momentum=0.9)`` steps, compared with the same trajectory of torch heads
(``nn.Sequential(Conv2d 3x3, ReLU, Conv2d 1x1)`` per head, the mirror loss ``_loss_ref.generic_loss``) in float64 (the
truth) and float32 (the yardstick) on the CPU, fed the feature maps the HIP trunk produced.  Measure and bound are those of
tests/test_hip_training_steps.py: the accumulated update ``theta_t - theta_0`` of every parameter, largest element error
over the largest float64 update, ``<= bound(e32, K = B*H*W)`` (tests/_dcn_bwd.py).

Condition.  The features are real-valued, so a hidden unit next to 0 could sit on different sides of the ReLU in float64 and
in fp32, and the comparison would fail as a wrong gradient.  Before comparing, the test asserts that the float64
trajectory's smallest |hidden pre-activation| over all steps is at least 64x the float32 trajectory's largest
pre-activation error.  No seed gives that margin with random first layers: 3 x 3.3 million Gaussian pre-activations of
spread ~1 put hundreds of values inside +-3e-5.  So the heads' FIRST layers of the synthetic state dict are designed, the
way ``scenarios.e2e_state_dict`` designs a bias: the feature map is the output of a ReLU (>= 0), every other hidden unit
has small non-negative weights and a positive bias (always on), the others non-positive weights and a negative bias
(always off): |bias| = 1/2 for ``hm``, whose focal-loss gradient moves its first layer most (its output layer is scaled by
1/4 for the same reason), 1/16 for the regression heads, whose updates are small enough for a larger bias to drown them in
its own fp32 spacing.  Three steps of lr 0.01 move no unit across 0: the condition asserts it over all steps (rehearsed on
the CPU with the oracle's feature map: smallest |pre-activation| 4.0e-2 against an fp32 error of 5.0e-7).  The mask logic
itself, with units on both sides and exact zeros, is the business of tests/test_hip_heads_backward.py."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _loss_ref as R
from _dcn_bwd import bound, err

pytestmark = pytest.mark.gpu

B, H_IN, W_IN, M, STEPS = 2, 128, 160, 8, 3
FH, FW = H_IN // 4, W_IN // 4
K = B * FH * FW


def _heads():
    from centertrack_amd import weights
    return weights.MOT_HEADS


def _state_dict():
    from centertrack_amd import weights
    heads = _heads()
    sd = weights.make_synthetic_state_dict(heads)
    g = torch.Generator().manual_seed(41)
    for h in heads:
        w = sd[h + '.0.weight']
        sign = torch.where(torch.arange(w.shape[0]) % 2 == 0, 1.0, -1.0)
        mag = torch.rand(w.shape, generator=g) * (3.0 / (w.shape[1] * 9)) ** 0.5 / 64
        sd[h + '.0.weight'] = mag * sign.view(-1, 1, 1, 1)
        sd[h + '.0.bias'] = sign * (0.5 if h == 'hm' else 0.0625)
    sd['hm.2.weight'] = sd['hm.2.weight'] * 0.25
    return sd


def _inputs(t):
    from centertrack_amd import weights
    x, pre, hm = weights.synthetic_inputs(B, H_IN, W_IN, seed=500 + t)
    _, batch = R.make_batch(510 + t, B, FH, FW, M, tuple(_heads()), 1)
    return (x, pre, hm), batch


def _head_keys():
    return [h + s for h in _heads() for s in ('.0.weight', '.0.bias', '.2.weight', '.2.bias')]


class _TorchHeads(torch.nn.Module):
    """the reference's heads (base_model.py:24-65) on a feature map"""

    def __init__(self, heads, sd, dtype):
        super().__init__()
        nn = torch.nn
        self.names = list(heads)
        for h, c in heads.items():
            self.add_module(h, nn.Sequential(nn.Conv2d(64, 256, 3, padding=1), nn.ReLU(), nn.Conv2d(256, c, 1)))
        self.load_state_dict({k: sd[k] for k in _head_keys()})
        self.to(dtype)
        self.pre = None

    def forward(self, feat):
        out, pre = OrderedDict(), []
        for h in self.names:
            fc = getattr(self, h)
            p = fc[0](feat)
            pre.append(p.detach())
            out[h] = fc[2](fc[1](p))
        self.pre = torch.cat(pre, 1)
        return [out]


def _torch_trajectory(sd, feats, batches, dtype):
    heads = _heads()
    net = _TorchHeads(heads, sd, dtype)
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    weights = R.Opt(tuple(heads)).weights
    first = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    steps = []
    for feat, batch in zip(feats, batches):
        opt.zero_grad()
        b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
        tot = R.generic_loss(net(feat.to(dtype)), b, tuple(heads), weights)[0]
        tot.backward()
        pre = net.pre
        opt.step()
        now = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
        steps.append((float(tot.detach()), {k: now[k] - first[k] for k in now}, pre))
    return steps


@pytest.fixture(scope='module')
def run(device):
    """everything that needs the GPU, once: the HIP trajectory and what the tests around it look at"""
    from centertrack_amd import heads as HD, losses
    from centertrack_amd.model import DLASegHIP
    heads = _heads()
    sd = _state_dict()
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    model = model.to(device)
    data = [_inputs(t) for t in range(STEPS)]
    x0 = [t.to(device) for t in data[0][0]]
    r = {'sd': sd, 'model': model}
    r['old'] = model(*x0)[0]
    trunk0 = {k: v.clone() for k, v in model.state_dict().items() if k not in _head_keys()}
    ft = HD.HeadFinetuner(model)
    r['param_names'] = [n for n, _ in ft.named_parameters()]
    crit = losses.GenericLoss(R.Opt(tuple(heads)))
    opt = torch.optim.SGD(ft.parameters(), lr=0.01, momentum=0.9)
    first = {k: v.detach().double().cpu() for k, v in ft.heads.state_dict().items()}
    feats, steps = [], []
    for (inp, batch) in data:
        opt.zero_grad()
        out = ft(*[t.to(device) for t in inp])
        assert all(o.grad_fn is not None for o in out[0].values())
        feats.append(model.get_plan(B, H_IN, W_IN, True, True, trunk_only=True)['feat'].to_nchw().cpu().clone())
        tot = crit(out, {k: v.to(device) for k, v in batch.items()})[0]
        tot.backward()
        opt.step()
        now = {k: v.detach().double().cpu() for k, v in ft.heads.state_dict().items()}
        steps.append((float(tot.detach()), {k: now[k] - first[k] for k in now}))
    r['feats'], r['steps'], r['batches'] = feats, steps, [b for _, b in data]
    r['trunk_same'] = all(torch.equal(v, trunk0[k]) for k, v in model.state_dict().items() if k in trunk0)
    r['mid_training_sd'] = OrderedDict((k, v.detach().cpu().clone()) for k, v in ft.state_dict().items())
    r['before_commit'] = model(*x0)[0]
    with torch.no_grad():
        r['train_forward'] = OrderedDict((h, v.clone()) for h, v in ft(*x0)[0].items())
    ft.commit()
    r['after_commit'] = model(*x0)[0]
    r['model_sd_after'] = OrderedDict((k, v.detach().cpu().clone()) for k, v in model.state_dict().items())
    r['x0'] = x0
    return r


@pytest.fixture(scope='module')
def reference(run):
    return (_torch_trajectory(run['sd'], run['feats'], run['batches'], torch.float64),
            _torch_trajectory(run['sd'], run['feats'], run['batches'], torch.float32))


def test_parameters_are_the_head_parameters_only(run):
    assert run['param_names'] == ['heads.' + k for k in _head_keys()]


def test_three_sgd_steps_against_torch_heads(run, reference):
    r64, r32 = reference
    # the condition: no hidden unit is close enough to 0 for fp32 and float64 to disagree about its side
    smallest = min(float(s[2].abs().min()) for s in r64)
    worst = max(float((a[2].double() - b[2]).abs().max()) for a, b in zip(r32, r64))
    print('finetune condition: smallest |pre-activation| %.3e, largest fp32 pre-activation error %.3e, ratio %.1f'
          % (smallest, worst, smallest / worst))
    assert smallest >= 64 * worst, 'the fixture drifted: a hidden unit sits next to 0 (%.3e against %.3e)' % (smallest, worst)
    assert all(bool((s[2] > 0).any()) and bool((s[2] < 0).any()) for s in r64)          # units on both sides of the ReLU
    fails = []
    for t in range(STEPS):
        (l, d), (l64, d64, _), (l32, d32, _) = run['steps'][t], r64[t], r32[t]
        el, el32 = abs(l - l64) / abs(l64), abs(l32 - l64) / abs(l64)
        bl = bound(el32, B * FH * FW)
        print('finetune step %d %-24s e(hip) %.3e  e(torch32) %.3e  bound %.3e' % (t, 'loss', el, el32, bl))
        if not el <= bl:
            fails.append((t, 'loss', el, bl))
        assert sorted(d) == sorted(d64) == sorted(_head_keys())
        for n in _head_keys():
            assert float(d64[n].abs().max()) > 0, n
            e, e32 = err(d[n], d64[n]), err(d32[n], d64[n])
            b = bound(e32, K)
            print('finetune step %d %-24s e(hip) %.3e  e(torch32) %.3e  bound %.3e  max|update64| %.3e'
                  % (t, n, e, e32, b, float(d64[n].abs().max())))
            if not e <= b:
                fails.append((t, n, e, b))
    assert not fails, fails


def test_the_trunk_is_frozen(run):
    assert run['trunk_same']


def test_commit_moves_the_heads_into_the_inference_model(run):
    """before ``commit()`` the model returns the old heads' outputs, bit for bit; after it, the fused inference heads
    launch (Winograd) gives what the finetuner's training-mode forward gives, within the tolerances tests/test_hip_ops.py
    holds those kernels to"""
    for h in _heads():
        assert torch.equal(run['before_commit'][h], run['old'][h]), h
        got, want = run['after_commit'][h].cpu().numpy(), run['train_forward'][h].cpu().numpy()
        np.testing.assert_allclose(got, want, atol=5e-4, rtol=2e-4, err_msg=h)
        assert float((run['after_commit'][h] - run['old'][h]).abs().max()) > 1e-3, h      # the heads did move
    for k in _head_keys():
        assert torch.equal(run['model_sd_after'][k], run['mid_training_sd'][k]), k


def test_a_checkpoint_saved_mid_training_loads_everywhere(run, device):
    """the finetuner's ``state_dict()`` is the full reference-format dict: strict into a fresh ``DLASegHIP``, and the CPU
    oracle (which reads the reference's keys) computes the same heads from it"""
    from centertrack_amd.model import DLASegHIP
    from oracle import dla34
    sd = run['mid_training_sd']
    fresh = DLASegHIP(_heads())
    assert list(sd) == list(fresh.state_dict())
    missing, unexpected = fresh.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k in sd:
        if k not in _head_keys():
            assert torch.equal(sd[k], run['sd'][k]), k
    assert any(not torch.equal(sd[k], run['sd'][k]) for k in _head_keys())
    feat = run['feats'][0]                                   # (the first step's inputs are x0)
    want = dla34.apply_heads(feat, _heads(), sd)
    for h in _heads():
        np.testing.assert_allclose(run['train_forward'][h].cpu().numpy(), want[h].numpy(), atol=5e-4, rtol=2e-4, err_msg=h)


def test_inference_is_untouched_while_nothing_is_committed(device):
    """a ``Detector`` built on the model before the finetuner existed gives identical rows before and after a finetuner
    is constructed and trained for a step, but not committed"""
    import scenarios as S
    from centertrack_amd import heads as HD, losses
    from centertrack_amd.detector import Detector, default_opt
    from centertrack_amd.model import DLASegHIP
    cfg = S.e2e_config()
    model = DLASegHIP(cfg['heads'])
    model.load_state_dict(S.e2e_state_dict(cfg))
    det = Detector(default_opt(cfg['heads'], track_thresh=cfg['track_thresh'], pre_thresh=cfg['pre_thresh']), model=model)
    frames = [f for f, _ in zip(S.e2e_frames(cfg), range(2))]

    def rows():
        det.reset_tracking()
        return [det.run(images, dict(meta))['results'] for images, meta in frames]
    before = rows()
    assert sum(len(r) for r in before) > 0
    ft = HD.HeadFinetuner(det.model)
    opt = torch.optim.SGD(ft.parameters(), lr=0.01)
    (x, pre, hm), batch = _inputs(0)
    out = ft(x.to(device), pre.to(device), hm.to(device))
    losses.GenericLoss(R.Opt(tuple(cfg['heads'])))(out, {k: v.to(device) for k, v in batch.items()})[0].backward()
    opt.step()
    after = rows()
    assert len(before) == len(after)
    for ra, rb in zip(before, after):
        assert len(ra) == len(rb)
        for a, b in zip(ra, rb):
            assert sorted(a) == sorted(b)
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
