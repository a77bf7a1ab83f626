"""GPU: ``centertrack_amd.dla_seg.DLASeg`` at 2 x 64 x 64 with the MOT heads (hm 1, reg 2, wh 2, tracking 2), ``pre_img`` and
``pre_hm``: a whole training step ``DLASeg(...)(x, pre_img, pre_hm) -> GenericLoss -> backward()`` against the hand-assembled
NCHW chain ``dla34 -> DLAUp -> IDAUp -> FusedHeads`` on the same state dict.

The forward has no atomics, so logits and loss agree bitwise.  A gradient agrees bitwise unless a DCN input gradient (summed
with float atomics) lies on its way: the heads and the last node of ``ida_up``.  Everything behind that node's input gradient
agrees as two runs of ONE of the paths agree, to fp32 rounding -- the bar of ``test_one_whole_training_step`` of
tests/test_hip_backbone_backward.py, 1e-4 of the tensor's maximum (measured there: 2.1e-6) -- with its exemption, the
``conv.bias`` of a ``DeformConv`` behind such a gradient, whose gradient under batch statistics is 0 in exact arithmetic and
rounding noise in fp32."""
from collections import OrderedDict

import pytest
import torch

import _backbone_bwd as BB
import _loss_ref as R
from _dcn_bwd import err
from test_dlaseg_cpu import HEAD_CONVS, HEADS, Opt

pytestmark = pytest.mark.gpu

SEED = 5200
N, H, W = 2, 64, 64
UNREAD = ['base.level%d.project.%s' % (lv, k) for lv in (3, 4) for k in ('0.weight', '1.weight', '1.bias')]


def state_dict():
    from centertrack_amd import weights as Wt
    return Wt.make_synthetic_state_dict(HEADS, seed=SEED)


def build_chain(sd, device):
    """the hand-assembled chain of the trainable modules, every module boundary NCHW"""
    from centertrack_amd import dla_base, dla_up, heads as HD
    net = torch.nn.Module()
    net.base = dla_base.dla34(pretrained=False, opt=BB.Opt())
    net.dla_up = dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8])
    net.ida_up = dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4])
    net.heads = HD.FusedHeads(HEADS)
    for part in ('base', 'dla_up', 'ida_up'):
        getattr(net, part).load_state_dict({k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(part + '.')})
    net.heads.load_state_dict({k: sd[k] for k in net.heads.state_dict()})
    return net.to(device)


def chain_forward(net, x, pre, hm):
    layers = net.dla_up(net.base(x, pre, hm))
    y = [layers[i].clone() for i in range(3)]
    net.ida_up(y, 0, len(y))
    return net.heads(y[-1])


def chain_key(k):
    """DLASeg's key -> the chain's"""
    return k if k.split('.')[0] in ('base', 'dla_up', 'ida_up') else 'heads.' + k


def data(device):
    from centertrack_amd import weights as Wt
    x, pre, hm = (t.to(device) for t in Wt.synthetic_inputs(N, H, W, seed=SEED))
    _, batch = R.make_batch(SEED + 1, N, H // 4, W // 4, 8, tuple(HEADS), 1)
    return (x, pre, hm), {k: v.to(device) for k, v in batch.items()}


def build_model(sd, device):
    from centertrack_amd.dla_seg import DLASeg
    m = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    m.load_state_dict(sd)
    return m.to(device)


def test_one_training_step_against_the_hand_assembled_chain(device):
    from centertrack_amd import dcn_v2, losses
    sd = state_dict()
    model, net = build_model(sd, device).train(), build_chain(sd, device).train()
    (x, pre, hm), batch = data(device)
    crit = losses.GenericLoss(R.Opt(tuple(HEADS)))

    def step(fwd, mod):
        mod.zero_grad(set_to_none=True)
        with dcn_v2.trainable():
            out = fwd()
            tot = crit([out], batch)[0]
            tot.backward()
        torch.cuda.synchronize()
        return out, tot.detach().clone(), {k: p.grad for k, p in mod.named_parameters()}
    out, tot, grads = step(lambda: model(x, pre, hm)[0], model)
    want, tot_c, grads_c = step(lambda: chain_forward(net, x, pre, hm), net)
    assert isinstance(out, dict) and list(out) == list(HEADS)
    for h, c in HEADS.items():
        assert out[h].shape == (N, c, H // 4, W // 4) and out[h].grad_fn is not None
        assert torch.equal(out[h], want[h]), h
    assert bool(torch.isfinite(tot)) and torch.equal(tot, tot_c)
    assert sorted(chain_key(k) for k in grads) == sorted(grads_c)
    diffs = {}
    for k, g in grads.items():
        gc = grads_c[chain_key(k)]
        if k in UNREAD:                                                  # read by nobody, here and there
            assert g is None and gc is None, k
            continue
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k
        if k.split('.')[0] in HEADS or k.startswith('ida_up.node_2.'):
            assert torch.equal(g, gc), k
        elif not k.endswith('conv.bias'):
            diffs[k] = err(g.cpu(), gc.cpu().double())
    assert len(grads) - len(UNREAD) >= 200
    top = sorted(diffs.items(), key=lambda kv: -kv[1])[:5]
    print('DLASeg step: loss %.6f; largest differences from the chain behind a DCN input gradient %s' % (
        float(tot), ['%s %.2e' % kv for kv in top]))
    assert top[0][1] <= 1e-4
    # the running statistics moved alike, bit for bit (the forward has no atomics)
    bufs, bufs_c = dict(model.named_buffers()), dict(net.named_buffers())
    for k, b in bufs.items():
        assert torch.equal(b, bufs_c[chain_key(k)]), k


def test_three_sgd_steps_lower_the_loss(device):
    """a fixed batch, plain SGD on every parameter with the gradient clipped to norm 1 (a step of 0.02 in parameter space,
    small against the curvature): the loss after three steps lies below the first one"""
    from centertrack_amd import dcn_v2, losses
    model = build_model(state_dict(), device).train()
    (x, pre, hm), batch = data(device)
    crit = losses.GenericLoss(R.Opt(tuple(HEADS)))
    opt = torch.optim.SGD(model.parameters(), lr=0.02)
    seen = []
    for step in range(4):
        opt.zero_grad(set_to_none=True)
        with dcn_v2.trainable():
            tot = crit(model(x, pre, hm), batch)[0]
            seen.append(float(tot.detach()))
            if step < 3:
                tot.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
                opt.step()
    print('DLASeg sgd: losses %s' % ['%.5f' % v for v in seen])
    assert all(v == v and abs(v) != float('inf') for v in seen) and seen[3] < seen[0]


def test_eval_mode_against_the_inference_plan_and_the_checkpoint_round_trip(device):
    """eval mode on a DLASegHIP's tensors: the feature map within the existing 1e-4 of the plan's (``trunk_only``; the two paths
    fold the BatchNorm differently); nothing recorded in the trunk; ``state_dict()`` goes through the reference format into DLASegHIP and back"""
    from centertrack_amd.model import DLASegHIP
    sd = state_dict()
    hip = DLASegHIP(HEADS)
    hip.load_state_dict(sd)
    hip = hip.to(device)
    (x, pre, hm), _ = data(device)
    with torch.no_grad():
        plan = hip.get_plan(N, H, W, True, True, trunk_only=True)
        hip.forward_plan(plan, x, pre, hm)
    torch.cuda.synchronize()
    want = plan['feat'].to_nchw().clone()
    model = build_model(sd, device).eval()
    feats = model.imgpre2feats(x, pre, hm)
    assert isinstance(feats, list) and len(feats) == 1 and feats[0].shape == (N, 64, H // 4, W // 4) and feats[0].grad_fn is None
    e = err(feats[0].cpu(), want.cpu().double())
    print('DLASeg eval against the inference plan: err %.2e' % e)
    assert e <= 1e-4
    # the trunk records only under ``trainable()``; the heads, as ``FusedHeads`` always has, whenever autograd is on
    out = model(x, pre, hm)
    assert all(out[0][h].grad_fn is not None for h in HEADS)
    with torch.no_grad():
        quiet = model(x, pre, hm)
    assert all(quiet[0][h].grad_fn is None and not quiet[0][h].requires_grad and torch.equal(quiet[0][h], out[0][h]) for h in HEADS)
    # without the previous frame: the reference's img2feats branch
    alone = model.img2feats(x)
    assert len(alone) == 1 and alone[0].shape == feats[0].shape and bool(torch.isfinite(alone[0]).all())
    # the round trip
    mine = model.state_dict()
    assert list(mine) == list(sd) or sorted(mine) == sorted(sd)
    other = DLASegHIP(HEADS)
    other.load_state_dict(OrderedDict((k, v.cpu()) for k, v in mine.items()))
    back = other.state_dict()
    assert sorted(back) == sorted(mine) and all(torch.equal(back[k], mine[k].cpu()) for k in mine)
    from centertrack_amd.dla_seg import DLASeg
    again = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    res = again.load_state_dict(back)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())


def test_model_output_list(device):
    from centertrack_amd.dla_seg import DLASeg
    m = DLASeg(34, HEADS, HEAD_CONVS, Opt(model_output_list=True))
    m.load_state_dict(state_dict())
    m = m.to(device).eval()
    (x, pre, hm), _ = data(device)
    out = m(x, pre, hm)
    ref = build_model(state_dict(), device).eval()(x, pre, hm)[0]
    assert len(out) == 1 and len(out[0]) == len(HEADS)
    for t, h in zip(out[0], sorted(HEADS)):
        assert torch.equal(t, ref[h]), h
