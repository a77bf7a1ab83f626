"""GPU: the composed model under the checkpoint-like weights of tests/_ckpt_weights.py (BatchNorm scales of either sign and
exactly 0, variances over eight decades, means of up to 4 sigma that the shift has to cancel, all-zero filters, DCN offsets of
a few pixels at every level with taps outside the map, masks pinned at 0 and 1), judged as the per-op tests judge a kernel:

    err   = max|got - ref64| / max|ref64|                      (tests/_dcn_bwd.py::err)
    bound = min(1e-3, 10 * max(e32, 2^-23 * sqrt(4608)))       (tests/_ckpt_weights.py::bound)

with ref64 the float64 run of oracle/dla34.py and e32 the error of its float32 run, per compared tensor.  10 = the 4 of
``_dcn_bwd.bound`` x the 2.5 by which the per-op bars let a Winograd launch exceed a direct one (5e-4 against 2e-4 in
tests/test_hip_ops.py); it is not measured on the code under test.  tests/test_ckpt_weights_cpu.py holds the weights to their
conditions for every case of this file and shows what the bound catches that ``atol = rtol = 1e-3`` does not.

All cases run at 1 x 64 x 96, 2 x 64 x 64 and 1 x 128 x 160: the smallest maps a whole DLA-34 runs at, with 2 x 3, 2 x 2 and
4 x 5 level-5 maps.  Measured on an MI355X: DESIGN.md section 'Whole-model parity under checkpoint-like weights'."""
import pytest
import torch

import _ckpt_weights as C
from _dcn_bwd import err
from test_ckpt_weights_cpu import PLAN_CASES, TRAIN_CASES, case_id

pytestmark = pytest.mark.gpu

# the conv launches that write the six level outputs (tests/test_hip_model.py::test_backbone_levels_match_oracle)
LEVEL_LAUNCHES = ['level0', 'level1', 'base.level2.root', 'base.level3.tree2.root', 'base.level4.tree2.root', 'base.level5.root']


def plan_tensors(model, plan, outputs, sd):
    """every compared tensor of one run of the inference plan, under the names of ``_ckpt_weights.oracle_run``"""
    got = {}
    convs = {l.name: l.out for l in plan['launches'] if l.fn == 'conv' and hasattr(l.out, 'to_nchw')}
    for n, launch in zip(C.LEVEL_NAMES, LEVEL_LAUNCHES):
        got[n] = convs[launch].to_nchw().cpu()
    for name, ref_name in C.dcn_result_names(sd).items():
        got[ref_name] = plan['dcn_layers'][name].to_nchw().cpu()
    got['feature'] = plan['feat'].to_nchw().cpu()
    for k, v in outputs.items():
        got['head ' + k] = v.cpu()
    return got


def run_plan(sd, heads, head_conv, inputs, device, winograd=True):
    """one forward of a fresh DLASegHIP; ``winograd=False`` builds it with every 3x3 launch on a direct algorithm (the
    attribution step of a failure)"""
    from centertrack_amd import model as M
    was = M.WINOGRAD
    M.WINOGRAD = was and winograd
    try:
        model = M.DLASegHIP(heads, head_conv=head_conv)
        assert set(model.state_dict().keys()) == set(sd.keys())
        model.load_state_dict(sd)
        model = model.to(device)
        x, pre, hm = (t.to(device) for t in inputs)
        plan = model.get_plan(x.shape[0], x.shape[2], x.shape[3], True, True, False)
        with torch.no_grad():
            out = model.forward_plan(plan, x, pre, hm)
        torch.cuda.synchronize()
        return plan_tensors(model, plan, out, sd)
    finally:
        M.WINOGRAD = was


def judge(got, t64, e32, names=None):
    """[(name, e32, err, bound)] and the report that names the layer of a failure"""
    rows = [(k, e32[k], err(got[k], t64[k]), C.bound(e32[k])) for k in (names or got)]
    lines = ['  %-30s e32 %.2e  err %.2e  err / bound %6.3f%s' % (k, e, g, g / b, '   <-- over' if g > b else '') for k, e, g, b in rows]
    return rows, '\n'.join(lines)


def over(rows):
    return [r[0] for r in rows if not r[2] <= r[3]]


# ---------------------------------------------------------------------------------------------------------------------
# (a) the inference plan

@pytest.mark.parametrize('case', PLAN_CASES, ids=case_id)
def test_inference_plan_against_float64(device, case):
    name, shape, seed, hc = case
    heads = C.head_sets()[name]
    sd, inputs, t64, t32, offsets, e32 = C.truth('ckpt', name, shape, seed, hc)
    got = run_plan(sd, heads, hc, inputs, device)
    assert set(got) <= set(t64) and len(got) == 6 + 16 + 1 + len(heads)
    rows, report = judge(got, t64, e32)
    print('%s\n%s' % (case_id(case), report))
    if over(rows):
        # one attribution step: the same case with the 3x3 launches forced to the direct algorithms
        rows_d, report_d = judge(run_plan(sd, heads, hc, inputs, device, winograd=False), t64, e32)
        pytest.fail('%s: over the bound: %s\n%s\nwith every 3x3 launch on a direct algorithm: over the bound: %s\n%s' % (
            case_id(case), over(rows), report, over(rows_d), report_d))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ---------------------------------------------------------------------------------------------------------------------
# (c) the trainable modules in eval mode

def _trainable(sd, device):
    import test_hip_dlaseg as T
    return T.build_chain(sd, device).eval(), T.build_model(sd, device).eval()


@pytest.mark.parametrize('case', TRAIN_CASES, ids=case_id)
def test_trainable_modules_in_eval_mode(device, case):
    """``dla34 -> DLAUp -> IDAUp -> FusedHeads`` and ``DLASeg`` under ``eval()``: each against float64 at the bound of the
    plan, and against the inference plan at the existing 1e-4 (tests/test_hip_dlaseg.py).  The plan folds
    ``beta - mean * scale`` once in float64; the modules hand mean, invstd, gamma and beta to their kernel."""
    import test_hip_dlaseg as T
    name, shape, seed, hc = case
    heads = C.head_sets()[name]
    assert list(heads) == list(T.HEADS)
    sd, inputs, t64, t32, offsets, e32 = C.truth('ckpt', name, shape, seed, hc)
    x, pre, hm = (t.to(device) for t in inputs)
    plan = run_plan(sd, heads, hc, inputs, device)
    net, model = _trainable(sd, device)
    names = ['feature'] + ['head ' + h for h in heads]
    with torch.no_grad():
        layers = net.dla_up(net.base(x, pre, hm))
        y = [layers[i].clone() for i in range(3)]
        net.ida_up(y, 0, len(y))
        chain = {'feature': y[-1].cpu()}
        chain.update(('head ' + h, v.cpu()) for h, v in net.heads(y[-1]).items())
        seg = {'feature': model.imgpre2feats(x, pre, hm)[0].cpu()}
        seg.update(('head ' + h, v.cpu()) for h, v in model(x, pre, hm)[0].items())
    torch.cuda.synchronize()
    for title, got in (('chain', chain), ('DLASeg', seg)):
        rows, report = judge(got, t64, e32, names)
        print('%s %s\n%s' % (case_id(case), title, report))
        assert not over(rows), '%s: %s\n%s' % (title, over(rows), report)
        # against the inference plan
        for k in names:
            e = err(got[k], plan[k].double())
            e_got, e_plan = err(got[k], t64[k]), err(plan[k], t64[k])
            print('  %-8s %-16s against the plan %.2e  (against float64: %.2e, the plan %.2e)' % (title, k, e, e_got, e_plan))
            if e > 1e-4:
                assert e_got <= C.bound(e32[k]) and e_plan <= C.bound(e32[k]) and e <= 2 * C.bound(e32[k]), (title, k, e, e_got, e_plan)
    for k in names:
        assert torch.equal(chain[k], seg[k]), k                          # the same launches on the same tensors


# ---------------------------------------------------------------------------------------------------------------------
# (d) training mode, module by module, against the float64 truths of the module tests

def _zeroed_rows(sd, gpar, unread=()):
    """what the generator's zeros imply, exactly: behind a gamma of 0 the gradient of the BatchNorm's input is 0, so the
    filter of that channel gets a gradient of 0 while gamma itself gets a finite one; an all-zero filter writes a constant
    channel whose batch variance is 0 and whose gradients are finite (their values: the Report's rows) -> channels checked"""
    n = 0
    for p, (zero, dead) in C.zeroed(sd).items():
        wkey = C._conv_before(sd, p)
        if wkey in unread:
            continue
        for c in zero:
            assert float(gpar[wkey][c].abs().max()) == 0.0 and bool(torch.isfinite(gpar[p + '.weight'][c])), (wkey, c)
        for c in dead:
            assert bool(torch.isfinite(gpar[wkey][c]).all()) and bool(torch.isfinite(gpar[p + '.weight'][c])), (wkey, c)
        assert zero and dead, p
        n += len(zero) + len(dead)
    return n


@pytest.mark.parametrize('name', ['tree-2', 'dla34'])
def test_backbone_modules_in_training_mode(device, name):
    """tests/test_hip_backbone_backward.py::test_modules in training mode with the generator's filters and BatchNorm
    parameters: forward, every gradient and the moved running statistics at that harness's own bounds and ReLU-mask rule"""
    import _backbone_bwd as BB
    import test_hip_backbone_backward as TB
    sd = C.backbone_module_params(name, C.SEEDS[1])
    res = TB.check_module(device, name, True, sd, BB.SEEDS[name], '%s train, checkpoint-like' % name)
    unread = [k for k, g in res['gpar'].items() if g is None]
    n = _zeroed_rows(sd, res['gpar'], unread)
    assert n >= {'tree-2': 30, 'dla34': 150}[name]
    worst = max(res['rows'], key=lambda r: r[1] / r[3] if r[3] else 0.0)
    print('%s train, checkpoint-like: %d zeroed channels checked; largest err / bound %.3f at %s' % (name, n, worst[1] / worst[3], worst[0]))


def test_idaup_in_training_mode(device):
    """tests/test_hip_neck_backward.py::test_idaup with the generator's ``ida_up``: DeformConv + BatchNorm + up-sampling,
    offsets of a few pixels with taps outside the map, masks pinned at 0 and 1, negative and zero gamma, an all-zero DCN
    filter (the channel is the bias: batch variance 0).  The float64 truth samples where float64 puts the coordinate, so the
    case requires that no coordinate lies within 1e-5 px of an integer: ten times what float32 can move one (e32 of an
    offset map is 1e-6 of a maximum below 10 px).  That is a property of the data, computed by the float64 run alone."""
    import _neck_bwd as NB
    import test_hip_neck_backward as TN
    sd = C.idaup_module_params(C.SEEDS[1], TN.idaup_inputs())
    res = TN.check_idaup(device, sd, 'idaup, checkpoint-like', 1e-5)
    sizes = dict(zip(('proj_1.', 'node_1.', 'proj_2.', 'node_2.'), [NB.IDA['sizes'][i] for i in (1, 0, 2, 0)]))
    for k, off in res['trace'].coords.items():
        H, W = sizes[k]
        pos = _tap_positions(off)
        outside = float(((pos[:, 0::2] <= -1) | (pos[:, 1::2] <= -1) | (pos[:, 0::2] >= H) | (pos[:, 1::2] >= W)).double().mean())
        print('idaup, checkpoint-like %s offsets: std %.2f px, max %.1f px, %.2f of the samples outside the map' % (
            k, float(off.std()), float(off.abs().max()), outside))
        assert 1.0 <= float(off.std()) <= 4.0 and float(off.abs().max()) <= 12.0 and outside >= 0.01
    n = _zeroed_rows(sd, res['gpar'])
    assert n >= 16
    worst = max(res['rows'], key=lambda r: r[1] / r[3] if r[3] else 0.0)
    print('idaup, checkpoint-like: %d zeroed channels checked; largest err / bound %.3f at %s' % (n, worst[1] / worst[3], worst[0]))


def _heads_autograd(fx, dtype, mask):
    """``_heads_bwd.autograd`` with the hidden ReLU replaced by the given mask [N, 256 * heads, H, W] (the HIP forward's)"""
    import torch.nn.functional as F
    x = fx['x'].detach().clone().to(dtype).requires_grad_()
    leaves, pres, outs, tot = [], [], {}, 0
    for j, h in enumerate(fx['heads']):
        p = [fx[k][h].detach().clone().to(dtype).requires_grad_() for k in ('w0', 'b0', 'w2', 'b2')]
        pre = F.conv2d(x, p[0], p[1], padding=1)
        mid = pre * mask[:, 256 * j:256 * (j + 1)].to(dtype)
        outs[h] = F.conv2d(mid, p[2], p[3])
        tot = tot + (outs[h] * fx['gout'][h].to(dtype)).sum()
        leaves += p
        pres.append(pre)
    g = torch.autograd.grad(tot, [x] + leaves)
    return {'pre': torch.cat([q.detach() for q in pres], 1), 'out': {h: o.detach() for h, o in outs.items()}, 'x': g[0],
            'w0': torch.cat(g[1::4], 0), 'b0': torch.cat(g[2::4], 0), 'w2': dict(zip(fx['heads'], g[3::4])),
            'b2': dict(zip(fx['heads'], g[4::4]))}


def test_heads_in_training_mode(device):
    """tests/test_hip_heads_backward.py::test_gradients_against_float64_autograd on the generator's head weights and on the
    feature map its trunk writes at 2 x 64 x 64 (post-ReLU, with exact zeros and the constant channels of the zeroed gammas).
    That fixture is not exact as the dyadic one is, so the truth takes the hidden ReLU mask from the HIP forward, held to
    ``_neck_bwd.check_mask``; bounds and K are ``_heads_bwd``'s."""
    import _heads_bwd as HB
    import _neck_bwd as NB
    import test_hip_heads_backward as TH
    from centertrack_amd import ops
    name, shape, seed, hc = TRAIN_CASES[1]
    heads = C.head_sets()[name]
    sd, inputs, t64m, t32m, _, _ = C.truth('ckpt', name, shape, seed, hc)
    x = t32m['feature'].contiguous()
    case = (tuple(int(v) for v in (x.shape[0], x.shape[2], x.shape[3])), heads)
    gen = torch.Generator().manual_seed(seed)
    fx = {'x': x, 'heads': heads, 'w0': {h: sd[h + '.0.weight'] for h in heads}, 'b0': {h: sd[h + '.0.bias'] for h in heads},
          'w2': {h: sd[h + '.2.weight'] for h in heads}, 'b2': {h: sd[h + '.2.bias'] for h in heads},
          'gout': {h: torch.randn((x.shape[0], c, x.shape[2], x.shape[3]), generator=gen) for h, c in heads.items()}}
    assert float((x == 0).float().mean()) > 0.2
    w0, b0, w2s, b2s, gouts = TH._dev(fx, device)
    feat = ops.view_from_nchw(x.to(device))
    outs, mid = ops.heads_forward_train(feat, w0, b0, w2s, b2s)
    mask = (mid.to_nchw() > 0).cpu()
    free64, free32 = (HB.autograd(fx, dt) for dt in (torch.float64, torch.float32))
    e_mid = err(torch.relu(free32['pre']), torch.relu(free64['pre']))
    flipped, near = NB.check_mask(mask, free64['pre'], e_mid, 'heads, checkpoint-like')
    print('heads, checkpoint-like: %d hidden units flipped, %d within the threshold, of %d' % (flipped, near, mask.numel()))
    t64, t32 = (_heads_autograd(fx, dt, mask) for dt in (torch.float64, torch.float32))
    tag, fails, K = 'checkpoint-like ' + HB.case_id(case), [], HB.terms(case)
    for h in heads:
        TH._judge(fails, tag, 'logits ' + h, outs[h], t64['out'][h], t32['out'][h], HB.HC)
    res = ops.heads_backward(feat, mid, gouts, w0, w2s, TH.ALL)
    TH._judge(fails, tag, 'gw0', res['w0'], t64['w0'], t32['w0'], K['w0'])
    TH._judge(fails, tag, 'gb0', res['b0'], t64['b0'], t32['b0'], K['b0'])
    TH._judge(fails, tag, 'gx', res['x'].to_nchw(), t64['x'], t32['x'], K['x'])
    for h in heads:
        TH._judge(fails, tag, 'gw2 ' + h, res['w2'][h], t64['w2'][h], t32['w2'][h], K['w2'])
        TH._judge(fails, tag, 'gb2 ' + h, res['b2'][h], t64['b2'][h], t32['b2'][h], K['b2'])
    assert float(res['gmid'].to_nchw().cpu()[~mask].abs().max()) == 0.0
    assert not fails, fails


def _tap_positions(off):
    from _dcn_bwd import tap_bases
    return tap_bases(off.shape[2], off.shape[3], off.dtype).unsqueeze(0) + off


# ---------------------------------------------------------------------------------------------------------------------
# (e) one whole training step

def exempt_from_nonzero(sd, keys):
    """the parameter tensors whose gradient may be 0 as a whole: those the generator zeroed as a whole, and those read only
    through such a tensor.  The generator zeroes channels, never a whole tensor -- a zero-gamma channel and an all-zero
    filter sit beside live ones in every layer -- so a tensor enters this list only if EVERY gamma of the BatchNorm behind
    it is 0 (the conv before it, the BatchNorm's own beta excepted) or every filter of it is."""
    out = []
    for p, (zero, dead) in C.zeroed(sd).items():
        wkey = C._conv_before(sd, p)
        if len(zero) == sd[p + '.weight'].numel():
            out += [p + '.weight', wkey]
        elif len(dead) == sd[wkey].shape[0]:
            out += [wkey]
    return [k for k in out if k in keys]


def test_one_training_step_under_checkpoint_like_weights(device):
    """``DLASeg -> GenericLoss -> backward`` at 2 x 64 x 64 against the hand-assembled chain, with the assertions of
    tests/test_hip_dlaseg.py::test_one_training_step_against_the_hand_assembled_chain.  On top of them, what the zeroed
    channels imply in exact arithmetic and the kernels must deliver exactly: behind a gamma of 0 the conv's filter gets a
    gradient of 0 and gamma itself a finite one; an all-zero filter (batch variance 0) gets a finite gradient."""
    import _loss_ref as R
    import test_hip_dlaseg as T
    from centertrack_amd import dcn_v2, losses
    name, shape, seed, hc = TRAIN_CASES[1]
    assert shape == (T.N, T.H, T.W) and seed == T.SEED
    sd = C.checkpoint_like_state_dict(T.HEADS, seed, hc, training=True)
    model, net = T.build_model(sd, device).train(), T.build_chain(sd, device).train()
    (x, pre, hm), batch = T.data(device)
    crit = losses.GenericLoss(R.Opt(tuple(T.HEADS)))

    def step(fwd, mod):
        mod.zero_grad(set_to_none=True)
        with dcn_v2.trainable():
            out = fwd()
            tot = crit([out], batch)[0]
            tot.backward()
        torch.cuda.synchronize()
        return out, tot.detach().clone(), {k: p.grad for k, p in mod.named_parameters()}
    out, tot, grads = step(lambda: model(x, pre, hm)[0], model)
    want, tot_c, grads_c = step(lambda: T.chain_forward(net, x, pre, hm), net)
    for h, c in T.HEADS.items():
        assert out[h].shape == (T.N, c, T.H // 4, T.W // 4) and torch.equal(out[h], want[h]), h
    assert bool(torch.isfinite(tot)) and torch.equal(tot, tot_c)
    assert sorted(T.chain_key(k) for k in grads) == sorted(grads_c)
    read = [k for k in grads if k not in T.UNREAD]
    exempt = exempt_from_nonzero(sd, read)
    assert len(exempt) <= len(read) // 10
    diffs = {}
    for k, g in grads.items():
        gc = grads_c[T.chain_key(k)]
        if k in T.UNREAD:
            assert g is None and gc is None, k
            continue
        assert g is not None and bool(torch.isfinite(g).all()), k
        assert k in exempt or float(g.abs().max()) > 0.0, k
        if k.split('.')[0] in T.HEADS or k.startswith('ida_up.node_2.'):
            assert torch.equal(g, gc), k
        elif not k.endswith('conv.bias'):
            diffs[k] = err(g.cpu(), gc.cpu().double())
    assert len(read) >= 200
    top = sorted(diffs.items(), key=lambda kv: -kv[1])[:5]
    print('DLASeg step under checkpoint-like weights: loss %.6f; %d exempt tensors; largest differences from the chain behind a '
          'DCN input gradient %s' % (float(tot), len(exempt), ['%s %.2e' % kv for kv in top]))
    assert top[0][1] <= 1e-4
    bufs, bufs_c = dict(model.named_buffers()), dict(net.named_buffers())
    for k, b in bufs.items():
        assert torch.equal(b, bufs_c[T.chain_key(k)]) and bool(torch.isfinite(b.float()).all()), k
    # the zeroed channels
    checked = 0
    for p, (zero, dead) in C.zeroed(sd).items():
        wkey = C._conv_before(sd, p)
        if wkey in T.UNREAD:
            continue
        for c in zero:
            assert float(grads[wkey][c].abs().max()) == 0.0, (wkey, c)
            assert bool(torch.isfinite(grads[p + '.weight'][c])), (p, c)
            checked += 1
        for c in dead:
            assert bool(torch.isfinite(grads[wkey][c]).all()) and bool(torch.isfinite(grads[p + '.weight'][c])), (wkey, c)
            # the batch variance of a constant channel is 0: the running variance moved by the momentum towards 0 alone
            rv, old = float(bufs[p + '.running_var'][c]), float(sd[p + '.running_var'][c])
            assert abs(rv - 0.9 * old) <= 1e-5 * old, (p, c, rv, old)
            checked += 1
    assert checked >= 100
