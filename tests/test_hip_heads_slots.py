"""GPU: the heads of a training step at the object slots (centertrack_amd/csrc/heads_slots.hip, ops.slot_gather /
ops.slot_fold, heads.FusedHeads(slot_heads=True), losses.GenericLoss on slot outputs, dla_seg.DLASeg with opt.slot_heads).

The two kernels are compared bit for bit with their restatements of tests/_heads_slots.py (torch indexing; the fold in owner
order).  The module is compared with the float64 truth of the reference's DENSE heads read at the slots, which
tests/test_heads_slots_cpu.py pins to the pipeline the module runs.  Bound: tests/_dcn_bwd.py, ``min(1e-3, 4 * max(e32,
2^-23 * sqrt(K)))`` with e32 the error of fp32 torch on the same inputs and K the number of summed terms: the valid slots for
a slot head's parameters, N*H*W for a dense head's, both for the input gradient, hc for a logit."""
from collections import OrderedDict

import pytest
import torch

import _heads_slots as S
import _loss_ref as R
from _dcn_bwd import bound, err

pytestmark = pytest.mark.gpu

C = S.CIN


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels

def _views(case, device, seed):
    """feat / gx as channels 8 .. 71 of an 80-wide buffer, rows with a pitch of 9*C + 16; random everywhere"""
    from centertrack_amd import ops
    (B, H, W, M), ind = S.CASES[case]
    g = torch.Generator().manual_seed(seed)
    mapbuf = torch.randn((B, H, W, 80), generator=g)
    rowbuf = torch.randn((B, 1, M, 9 * C + 16), generator=g)
    return (ops.View(mapbuf.to(device), 8, C), ops.View(rowbuf.to(device), 0, 9 * C), ind.to(device), mapbuf, rowbuf)


@pytest.mark.parametrize('case', list(S.CASES))
def test_slot_gather_is_torch_indexing_bit_for_bit(device, case):
    from centertrack_amd import ops
    (B, H, W, M), ind = S.CASES[case]
    feat, rows, ind_d, mapbuf, rowbuf = _views(case, device, 21)
    got = ops.slot_gather(feat, ind_d, out=rows)
    assert got is rows
    want = S.gather_ref(mapbuf[..., 8:8 + C].contiguous(), ind).view(B, 1, M, 9 * C)
    assert _same_bits(rows.buf[..., :9 * C].cpu(), want)
    assert _same_bits(rows.buf[..., 9 * C:].cpu(), rowbuf[..., 9 * C:])           # the padding keeps its sentinel
    assert _same_bits(feat.buf.cpu(), mapbuf)
    fresh = ops.slot_gather(feat, ind_d)                                       # a tight view of its own
    assert (fresh.N, fresh.H, fresh.W, fresh.C, fresh.ld) == (B, 1, M, 9 * C, 9 * C) and _same_bits(fresh.buf.cpu(), want)


@pytest.mark.parametrize('case', list(S.CASES))
def test_slot_fold_is_the_owner_order_sum_bit_for_bit(device, case):
    from centertrack_amd import ops
    (B, H, W, M), ind = S.CASES[case]
    runs = []
    for _ in range(2):
        gx, rows, ind_d, mapbuf, rowbuf = _views(case, device, 22)
        assert ops.slot_fold(rows, ind_d, gx) is gx
        runs.append(gx.buf.cpu())
        assert _same_bits(rows.buf.cpu(), rowbuf)
    assert _same_bits(runs[0], runs[1])
    P = rowbuf[..., :9 * C].reshape(B, M, 9, C)
    want, owner, _ = S.fold_owner_order(P, ind, mapbuf[..., 8:8 + C].contiguous())
    got = runs[0]
    assert _same_bits(got[..., 8:8 + C], want)
    assert _same_bits(got[..., :8], mapbuf[..., :8]) and _same_bits(got[..., 8 + C:], mapbuf[..., 8 + C:])
    untouched = owner < 0
    assert _same_bits(got[untouched], mapbuf[untouched])                        # an uncovered cell keeps its bits
    if not bool(S.valid_of(ind, H, W).any()):
        assert _same_bits(got, mapbuf)                                         # every slot invalid: nothing is written


# ---------------------------------------------------------------------------------------------------------------------
# the module

def _module(fx, device, slot_heads=True):
    from centertrack_amd import heads as HD
    m = HD.FusedHeads(fx['heads'], S.HC, slot_heads=slot_heads)
    m.load_state_dict(OrderedDict(('%s.%s' % (h, k), fx[n][h]) for h in fx['heads']
                                  for k, n in (('0.weight', 'w0'), ('0.bias', 'b0'), ('2.weight', 'w2'), ('2.bias', 'b2'))))
    return m.to(device)


def _run(m, fx, device, form='nchw', grad_x=True):
    """one forward + backward -> (outputs, x gradient as NCHW or None, {parameter: gradient})"""
    from centertrack_amd import ops
    m.zero_grad(set_to_none=True)
    ind = fx['ind'].to(device)
    x = fx['x'].to(device)
    if form == 'nchw':
        leaf = x.requires_grad_(grad_x)
        out = m(leaf, ind)
    elif form == 'nhwc':
        leaf = x.permute(0, 2, 3, 1).contiguous().requires_grad_(grad_x)
        out = m.forward_nhwc(leaf, ind)
    else:
        leaf = None
        out = m(ops.view_from_nchw(x), ind)
    sum((out[h] * fx['g'][h].to(device)).sum() for h in fx['heads']).backward()
    gx = None
    if leaf is not None and grad_x:
        gx = leaf.grad if form == 'nchw' else leaf.grad.permute(0, 3, 1, 2)
    return out, gx, OrderedDict((n, p.grad) for n, p in m.named_parameters())


def _judge(fails, tag, name, got, t64, t32, K):
    got = got.detach().cpu()
    if float(t64.abs().max()) == 0.0:
        ok, e, b = float(got.abs().max()) == 0.0, float(got.abs().max()), 0.0
    else:
        e, e32 = err(got, t64), err(t32, t64)
        b = bound(e32, K)
        ok = e <= b
    print('slot heads %-26s %-24s e(hip) %.3e  bound %.3e' % (tag, name, e, b))
    if not ok:
        fails.append((tag, name, e, b))


@pytest.mark.parametrize('combo', S.COMBOS, ids=S.combo_id)
def test_fused_heads_in_slot_mode_against_the_float64_truth(device, combo):
    fx, t64, t32 = S.truth(combo)
    (B, H, W, M) = fx['shape']
    slot, dense = S.split(fx['heads'])
    K = S.terms(combo)
    m = _module(fx, device)
    out, gx, grads = _run(m, fx, device)
    tag, fails = S.combo_id(combo), []
    for h, c in fx['heads'].items():
        assert out[h].shape == ((B, M, c) if h in slot else (B, c, H, W)), h
        _judge(fails, tag, 'logits ' + h, out[h], t64['out'][h], t32['out'][h], K['logits'])
        kk = K['slot'] if h in slot else K['dense']
        for k, n in (('w0', '0.weight'), ('b0', '0.bias'), ('w2', '2.weight'), ('b2', '2.bias')):
            _judge(fails, tag, '%s.%s' % (h, n), grads['%s.%s' % (h, n)], t64[k][h], t32[k][h], kk)
    _judge(fails, tag, 'x', gx, t64['x'], t32['x'], K['x'])
    invalid = ~S.valid_of(fx['ind'], H, W)
    for h in slot:
        assert float(out[h].detach().cpu()[invalid].abs().max() if bool(invalid.any()) else 0.0) == 0.0, h   # zero rows
    if not bool((~invalid).any()):
        for h in slot:
            for n in ('0.weight', '0.bias', '2.weight', '2.bias'):
                assert float(grads['%s.%s' % (h, n)].abs().max()) == 0.0, (h, n)
    # a second run: every bit again
    out2, gx2, grads2 = _run(m, fx, device)
    assert _same_bits(gx, gx2)
    for h in fx['heads']:
        assert _same_bits(out[h], out2[h]), h
    for n in grads:
        assert _same_bits(grads[n], grads2[n]), n
    assert not fails, fails


@pytest.mark.parametrize('combo', [('hand-2x5x7x12', 'mot'), ('tiles-2x16x16x129', 'nusc'), ('random-3x8x8x17', 'pose')],
                         ids=S.combo_id)
def test_the_three_input_forms_agree_bit_for_bit(device, combo):
    fx, _, _ = S.truth(combo)
    m = _module(fx, device)
    out, gx, grads = _run(m, fx, device, 'nchw')
    for form in ('nhwc', 'view'):
        o, g, gr = _run(m, fx, device, form)
        for h in fx['heads']:
            assert _same_bits(out[h], o[h]), (form, h)
        for n in grads:
            assert _same_bits(grads[n], gr[n]), (form, n)
        if form == 'nhwc':
            assert _same_bits(gx, g)
        else:
            assert g is None


def test_without_ind_or_without_the_flag_the_call_is_the_dense_one(device):
    combo = ('hand-2x5x7x12', 'mot')
    fx, _, _ = S.truth(combo)
    x = fx['x'].to(device)
    ind = fx['ind'].to(device)
    want = _module(fx, device, slot_heads=False)(x)
    for got in (_module(fx, device)(x), _module(fx, device, slot_heads=False)(x, ind),
                _module(fx, device).forward_nhwc(x.permute(0, 2, 3, 1).contiguous())):
        assert list(got) == list(want)
        for h in want:
            assert _same_bits(got[h], want[h]), h


def _count_launches(monkeypatch):
    from centertrack_amd import _lib
    lib = _lib.load()
    calls = []

    class Spy(object):
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ('ct_conv2d', 'ct_conv2d_backward_weight', 'ct_heads_tail_backward', 'ct_slot_gather', 'ct_slot_fold'):
                def wrapped(*a, **k):
                    calls.append(name)
                    return fn(*a, **k)
                return wrapped
            return fn
    monkeypatch.setattr(_lib, 'load', lambda: Spy())
    return calls


def test_a_frozen_feature_map_launches_no_patch_conv_and_no_fold(device, monkeypatch):
    combo = ('random-3x8x8x17', 'mot')
    fx, t64, t32 = S.truth(combo)
    K = S.terms(combo)
    m = _module(fx, device)
    calls = _count_launches(monkeypatch)
    _, gx, grads = _run(m, fx, device, grad_x=False)
    # forward: the dense hidden layer + hm, the gather, the slot hidden layer + four heads; backward: per group the tail and
    # the first layer's weight gradient
    assert calls == ['ct_conv2d'] * 2 + ['ct_slot_gather'] + ['ct_conv2d'] * 5 + \
        ['ct_heads_tail_backward', 'ct_conv2d_backward_weight'] * 2, calls
    assert gx is None
    fails = []
    for h in fx['heads']:
        kk = K['dense'] if h == 'hm' else K['slot']
        for k, n in (('w0', '0.weight'), ('b0', '0.bias'), ('w2', '2.weight'), ('b2', '2.bias')):
            _judge(fails, 'frozen feature', '%s.%s' % (h, n), grads['%s.%s' % (h, n)], t64[k][h], t32[k][h], kk)
    assert not fails, fails
    del calls[:]
    _run(m, fx, device)                                                        # with a gradient: two convs more and the fold
    assert calls[-1] == 'ct_slot_fold' and calls.count('ct_slot_fold') == 1 and calls.count('ct_conv2d') == 7 + 2, calls


# ---------------------------------------------------------------------------------------------------------------------
# the loss on slot outputs

LOSS_HEADS = R.ALL_HEADS                 # hm + ten heads read at ind


def _loss_case():
    B, Cc, H, W, M = 2, 3, 7, 9, 8
    out, batch = R.make_batch(8, B, H, W, M, LOSS_HEADS, Cc, valid=[8, 6])
    bad = {k: v.clone() for k, v in batch.items()}
    bad['ind'][1, 2] = H * W
    bad['ind'][0, 5] = -1
    clean = {k: v.clone() for k, v in batch.items()}
    for b, mm in ((1, 2), (0, 5)):                                             # the same batch with those slots masked out
        clean['ind'][b, mm] = 0
        clean['cat'][b, mm] = 0
        clean['rotbin'][b, mm] = 0
        for k in clean:
            if k.endswith('mask'):
                clean[k][b, mm] = 0
    return out, batch, bad, clean, (B, Cc, H, W, M)


def _loss_err(got, want):
    got, want = float(got), float(want)
    return (0.0 if got == 0.0 else float('inf')) if want == 0.0 else abs(got - want) / abs(want)


def _slot_truth(out, batch, dtype):
    """{head: (loss, gradient)} of the formulas of tests/_loss_ref.py with the slot heads as leaves [B,M,c]: slot m of the map
    [B,c,1,M] is its own cell"""
    B, M = batch['ind'].shape
    proxy = dict(batch, ind=torch.arange(M).view(1, M).expand(B, M).contiguous())
    res = {}
    for h in LOSS_HEADS:
        if h == 'hm':
            res[h] = R.losses_and_grads(out, batch, ('hm',), dtype)['hm']
            continue
        z = S.read_at(out[h], batch['ind']).to(dtype).requires_grad_()
        b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in proxy.items()}
        loss = R.head_loss(h, z.transpose(1, 2).unsqueeze(2), b)
        g, = torch.autograd.grad(loss, z)
        res[h] = (loss.detach(), g)
    return res


@pytest.mark.parametrize('which', ['in range', 'out of range'])
def test_generic_loss_on_slot_outputs(device, which):
    from centertrack_amd import losses
    out, batch, bad, clean, (B, Cc, H, W, M) = _loss_case()
    given, ref = (batch, batch) if which == 'in range' else (bad, clean)
    w64, w32 = _slot_truth(out, ref, torch.float64), _slot_truth(out, ref, torch.float32)
    d64 = R.losses_and_grads(out, ref, LOSS_HEADS, torch.float64)
    d32 = R.losses_and_grads(out, ref, LOSS_HEADS, torch.float32)
    dev_batch = {k: v.to(device) for k, v in given.items()}
    opt = R.Opt(LOSS_HEADS)
    fails = []
    for mode, t64, t32 in (('slot', w64, w32), ('dense', d64, d32)):
        leaves = OrderedDict()
        for h in LOSS_HEADS:
            x = out[h] if (h == 'hm' or mode == 'dense') else S.read_at(out[h], given['ind'])
            leaves[h] = x.to(device).requires_grad_()
        tot, stats = losses.GenericLoss(opt)([dict(leaves)], dev_batch)
        grads = torch.autograd.grad(sum(stats[h] for h in LOSS_HEADS), list(leaves.values()))
        for h, g in zip(LOSS_HEADS, grads):
            K = R.terms(h, out[h].shape, M)
            el, eg = _loss_err(stats[h].detach(), t64[h][0]), R.err(g, t64[h][1])
            bl = R.bound(_loss_err(t32[h][0], t64[h][0]), K)
            bg = R.bound(R.err(t32[h][1], t64[h][1]), 1)
            print('slot loss %-12s %-5s %-14s loss err %.3e (bound %.3e)  grad err %.3e (bound %.3e)' % (which, mode, h, el, bl, eg, bg))
            if not (el <= bl and eg <= bg):
                fails.append((mode, h, el, bl, eg, bg))
            if mode == 'slot' and h != 'hm':
                assert g.shape == (B, M, out[h].shape[1])
                gone = ~S.valid_of(given['ind'], H, W)
                assert float(g.cpu()[gone].abs().max() if bool(gone.any()) else 0.0) == 0.0, h
    assert not fails, fails


def test_generic_loss_slot_plumbing(device):
    """a stack of slot heads without a dense hm raises; sigmoid_outputs transforms a 3-d dep like a map"""
    from centertrack_amd import _lib, losses
    out, batch, _, _, _ = _loss_case()
    dev_batch = {k: v.to(device) for k, v in batch.items()}
    heads = ('hm', 'dep', 'wh')
    outputs = {h: (out[h] if h == 'hm' else S.read_at(out[h], batch['ind'])).to(device) for h in heads}
    raw = outputs['dep'].clone()
    losses.GenericLoss(R.Opt(heads), sigmoid_outputs=True)([outputs], dev_batch)
    assert outputs['dep'].dim() == 3 and torch.equal(outputs['dep'], 1. / (raw.sigmoid() + 1e-6) - 1.)
    with pytest.raises(_lib.CTError):
        losses.GenericLoss(R.Opt(('wh',)))([{'wh': outputs['wh']}], dev_batch)


# ---------------------------------------------------------------------------------------------------------------------
# DLASeg and Trainer

SEED = 5300
N, H, W = 2, 64, 64
HEAD_CONVS = {h: [256] for h in S.MOT}
UNREAD = ['base.level%d.project.%s' % (lv, k) for lv in (3, 4) for k in ('0.weight', '1.weight', '1.bias')]


class Opt(R.Opt):
    pre_img, pre_hm = True, True
    dla_node, head_kernel, prior_bias = 'dcn', 3, -4.6
    model_output_list = False
    load_model = ''

    def __init__(self, **kw):
        super().__init__(tuple(S.MOT))
        for k, v in kw.items():
            setattr(self, k, v)


def _dlaseg(sd, device, **kw):
    from centertrack_amd.dla_seg import DLASeg
    m = DLASeg(34, S.MOT, HEAD_CONVS, Opt(**kw))
    m.load_state_dict(sd)
    return m.to(device)


def _data(device):
    from centertrack_amd import weights as Wt
    x, pre, hm = (t.to(device) for t in Wt.synthetic_inputs(N, H, W, seed=SEED))
    _, batch = R.make_batch(SEED + 1, N, H // 4, W // 4, 8, tuple(S.MOT), 1)
    return (x, pre, hm), {k: v.to(device) for k, v in batch.items()}


def test_dlaseg_with_slot_heads_against_dense_mode(device):
    from centertrack_amd import dcn_v2, losses
    from centertrack_amd import weights as Wt
    sd = Wt.make_synthetic_state_dict(S.MOT, seed=SEED)
    (x, pre, hm), batch = _data(device)
    crit = losses.GenericLoss(Opt())
    res = {}
    for mode in ('dense', 'slot'):
        model = _dlaseg(sd, device, slot_heads=(mode == 'slot')).train()
        assert model.slot_heads == (mode == 'slot')
        with dcn_v2.trainable():
            out = model(x, pre, hm, batch['ind'])[0]
            tot = crit([out], batch)[0]
            tot.backward()
        torch.cuda.synchronize()
        res[mode] = (out, tot.detach(), {k: p.grad for k, p in model.named_parameters()})
    (od, td, gd), (os_, ts, gs) = res['dense'], res['slot']
    M = batch['ind'].shape[1]
    for h, c in S.MOT.items():
        assert od[h].shape == (N, c, H // 4, W // 4)
        assert os_[h].shape == ((N, c, H // 4, W // 4) if h == 'hm' else (N, M, c)), h
    assert torch.equal(os_['hm'], od['hm'])
    e = abs(float(ts) - float(td)) / abs(float(td))
    print('DLASeg slot heads: loss %.6f against %.6f dense (%.2e)' % (float(ts), float(td), e))
    assert e <= 1e-4
    diffs = {}
    for k, g in gs.items():
        if k in UNREAD:
            assert g is None and gd[k] is None, k
            continue
        assert g is not None and bool(torch.isfinite(g).all()), k
        if not k.endswith('conv.bias'):
            diffs[k] = err(g.cpu(), gd[k].cpu().double())
    top = sorted(diffs.items(), key=lambda kv: -kv[1])[:5]
    print('DLASeg slot heads: largest gradient differences from dense mode %s' % ['%s %.2e' % kv for kv in top])
    assert len(diffs) >= 200 and top[0][1] <= 1e-4
    # without ind: the dense maps of a module without the flag, bit for bit
    a, b = _dlaseg(sd, device, slot_heads=True).train(), _dlaseg(sd, device).train()
    with dcn_v2.trainable():
        za, zb = a(x, pre, hm)[0], b(x, pre, hm)[0]
    for h, c in S.MOT.items():
        assert za[h].shape == (N, c, H // 4, W // 4) and _same_bits(za[h], zb[h]), h


class _ClippedSGD(torch.optim.SGD):
    """plain SGD on a gradient clipped to norm 1, the step of tests/test_hip_dlaseg.py"""

    def step(self):
        torch.nn.utils.clip_grad_norm_([p for g in self.param_groups for p in g['params']], 1.0)
        return super().step()


def test_three_sgd_steps_through_trainer_lower_the_loss(device):
    from centertrack_amd import weights as Wt
    from centertrack_amd.trainer import Trainer
    model = _dlaseg(Wt.make_synthetic_state_dict(S.MOT, seed=SEED), device, slot_heads=True)
    (x, pre, hm), batch = _data(device)
    batch = dict(batch, image=x, pre_img=pre, pre_hm=hm)
    opt = Opt(slot_heads=True, num_iters=-1, print_iter=0, debug=0, device=device, task='tracking', exp_id='slots')
    tr = Trainer(opt, model, _ClippedSGD(model.parameters(), lr=0.02))
    tr.set_device([0], [N], device)
    seen = [tr.train(i, [dict(batch)])[0]['tot'] for i in range(4)]            # the loss BEFORE each step
    print('DLASeg slot heads sgd: losses %s' % ['%.5f' % v for v in seen])
    assert all(v == v and abs(v) != float('inf') for v in seen) and seen[3] < seen[0]


def test_slot_mode_allocates_less_than_dense_mode(device):
    """nuScenes heads on a 32 x 40 map: the peak of a forward + backward"""
    from centertrack_amd import heads as HD
    B, Hh, Ww, M = 2, 32, 40, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B, C, Hh, Ww), generator=g).to(device)
    ind = torch.randint(0, Hh * Ww, (B, M), generator=g).to(device)
    torch.manual_seed(1)
    sd = HD.FusedHeads(S.NUSC, S.HC).state_dict()
    peak = {}
    for mode in ('dense', 'slot'):
        m = HD.FusedHeads(S.NUSC, S.HC, slot_heads=(mode == 'slot'))
        m.load_state_dict(sd)
        m = m.to(device)
        leaf = x.clone().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m(leaf, ind)
        sum(o.sum() for o in out.values()).backward()
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
        del out, leaf, m
    print('heads peak memory: dense %d bytes, slots %d bytes' % (peak['dense'], peak['slot']))
    assert peak['slot'] < peak['dense']
