"""GPU: the training kernels carry NaN and +-Inf as torch does.

Every case of tests/_nonfinite.py -- an op's own fixture with exactly one element replaced by NaN, +Inf or -Inf -- runs through the
HIP kernel and is held to ``_nonfinite.compare`` against the float64 torch reference of the same op on the same planted input: no
laundering, a spread bounded by the launch's tile geometry, the op's usual bound on the finite rest, and a finite rest of at least
75 % (7/8 for BatchNorm) of the output.  Then the statistics, the loss on the reference's own non-finite cases
(tests/golden/losses_nonfinite.npz) and the whole ``DLASeg`` step with the guarded optimizer and the ``Trainer``.

No case makes an address depend on a planted value: DCN offsets and masks, ``ind`` and ``cat`` stay finite, and the whole-step
cases plant behind the last DeformConv (or run the backbone alone), so that no DCN ever reads a non-finite offset on the GPU."""
from collections import OrderedDict

import pytest
import torch

import _backbone_bwd as BB
import _conv_fwd as CF
import _loss_ref as R
import _neck_bwd as NB
import _nonfinite as NF
import _stem_bwd as SB
from _nonfinite import INF, NAN, compare

pytestmark = pytest.mark.gpu


def V(t, device):
    """NCHW CPU tensor -> a tight NHWC view on the device"""
    from centertrack_amd import ops
    return ops.View(t.permute(0, 2, 3, 1).contiguous().to(device))


def back(v):
    return v.to_nchw().cpu().clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# one runner per family: Case -> {output: tensor on the CPU}

def _bn_setup(c, device):
    from centertrack_amd import ops
    z, gamma, beta, rm, rv, gy, res = c.inputs['t']
    zv, gyv = V(z, device), V(gy, device)
    rsv = V(res, device) if c.inputs['residual'] else None
    if c.inputs['batch']:
        mean, var, invstd = ops.bn_stats(zv, NB.EPS)
    else:
        mean, var = rm.to(device), rv.to(device)
        invstd = torch.rsqrt(var + NB.EPS)
    return zv, gyv, rsv, mean, invstd, gamma.to(device), beta.to(device)


def run_bn_act_apply(c, device):
    from centertrack_amd import ops
    zv, gyv, rsv, mean, invstd, g, b = _bn_setup(c, device)
    y = ops.bn_act_apply(zv, mean, invstd, g, b, res=rsv, relu=True)
    if rsv is None:                                       # the neck's entry point: the same bits, NaN included
        assert same_bits(ops.bn_relu_apply(zv, mean, invstd, g, b).buf, y.buf)
    return dict(y=back(y))


def run_bn_act_backward(c, device):
    from centertrack_amd import ops
    zv, gyv, rsv, mean, invstd, g, b = _bn_setup(c, device)
    batch = c.inputs['batch']
    gz, gr, gg, gb = ops.bn_act_backward(zv, gyv, mean, invstd, g, b, batch, res=rsv, relu=True, need_res=rsv is not None)
    got = dict(gz=back(gz), ggamma=gg.cpu(), gbeta=gb.cpu())
    if rsv is not None:
        got['gres'] = back(gr)
    else:
        gz0, gg0, gb0 = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, batch)
        assert same_bits(gz0.buf, gz.buf) and same_bits(gg0, gg) and same_bits(gb0, gb)
    return got


def _stem_vectors(sd, device):
    means = [sd[p + '1.running_mean'].to(device) for p in SB.PREFIX]
    invstds = [torch.rsqrt(sd[p + '1.running_var'].to(device) + NB.EPS) for p in SB.PREFIX]
    return means, invstds, [sd[p + '1.weight'].to(device) for p in SB.PREFIX], [sd[p + '1.bias'].to(device) for p in SB.PREFIX]


def run_stem_bn_relu_sum(c, device):
    from centertrack_amd import ops
    means, invstds, gammas, betas = _stem_vectors(c.inputs['sd'], device)
    return dict(y=back(ops.stem_bn_relu_sum([V(z, device) for z in c.inputs['zs']], means, invstds, gammas, betas)))


def run_stem_conv_backward(c, device):
    from centertrack_amd import ops
    sd, s = c.inputs['sd'], c.inputs['s']
    only = tuple(i == s for i in range(3))
    gw, gin = ops.stem_conv_backward([V(g, device) for g in c.inputs['gz']], [x.to(device) for x in c.inputs['xs']],
                                     [sd[p + '0.weight'].to(device) for p in SB.PREFIX], need_w=only, need_in=only)
    return dict(gin=gin[s].cpu(), gw=gw[s].cpu())


def run_maxpool2x2(c, device):
    from centertrack_amd import ops
    return dict(y=back(ops.maxpool2x2(V(c.inputs['x'], device))))


def run_maxpool2x2_backward(c, device):
    from centertrack_amd import ops
    return dict(gx=back(ops.maxpool2x2_backward(V(c.inputs['x'], device), V(c.inputs['gy'], device))))


def run_conv2d(c, device):
    from centertrack_amd import ops
    case, d = c.inputs['case'], c.inputs['d']
    assert not case.knobs and not case.nchw and not case.proj
    dev = lambda t: None if t is None else t.to(device)
    w = d['w'].to(device)
    kw = dict(scale=dev(d['scale']), shift=dev(d['shift']), relu=case.relu, split_k=case.split_k, algo=case.algo)
    if CF.plan_of(case)['family'] == 'wino':
        kw['w_wino'] = ops.pack_winograd(w)
    if case.res:
        kw['res'] = V(d['res'], device)
    pv = None
    if case.pool:
        pv = kw['pool'] = ops.new_view(case.N, case.H // 2, case.W // 2, case.Cin, device)
    y = ops.conv2d(V(d['x'], device), ops.pack_weight(w), case.Cout, case.ks, case.stride, **kw)
    got = dict(y=back(y))
    if pv is not None:
        got['pool'] = back(pv)
    return got


def run_heads_backward(c, device):
    from centertrack_amd import ops
    fx = c.inputs['fx']
    heads = fx['heads']
    mid = V(fx['mid'], device)
    w2s = OrderedDict((h, fx['w2'][h].to(device)) for h in heads)
    gouts = OrderedDict((h, fx['gout'][h].to(device)) for h in heads)
    r = ops.heads_backward(None, mid, gouts, fx['w0'].to(device), w2s, {'x': True, 'w2': True, 'b2': True})
    return dict(gmid=back(r['gmid']), x=back(r['x']), w2=torch.cat([r['w2'][h].cpu().reshape(-1) for h in heads]),
                b2=torch.cat([r['b2'][h].cpu() for h in heads]))


def run_conv_backward_weight(c, device):
    from centertrack_amd import ops
    gw, gb = ops.conv_backward_weight(V(c.inputs['x'], device), V(c.inputs['gy'], device), 3, need_bias=True)
    return dict(gw=gw.cpu(), gb=gb.cpu())


def run_conv_backward_input(c, device):
    from centertrack_amd import ops
    return dict(gx=back(ops.conv_backward_input(V(c.inputs['gy'], device), c.inputs['w'].to(device))))


def run_conv_s2_backward(c, device):
    from centertrack_amd import ops
    gx, gw = ops.conv_s2_backward(V(c.inputs['x'], device), V(c.inputs['gy'], device), c.inputs['w'].to(device))
    return dict(gx=back(gx), gw=gw.cpu())


def run_upsample_add(c, device):
    from centertrack_amd import ops
    i = c.inputs
    return dict(y=back(ops.upsample_add(V(i['x'], device), i['w'].to(device), i['f'], V(i['skip'], device))))


def run_upsample_add_backward(c, device):
    from centertrack_amd import ops
    i = c.inputs
    gx, gw, _ = ops.upsample_add_backward(V(i['x'], device), i['w'].to(device), i['f'], V(i['gy'], device))
    return dict(gx=back(gx), gw=gw.cpu())


def run_slot_gather(c, device):
    from centertrack_amd import ops
    rows = ops.slot_gather(V(c.inputs['feat'], device), c.inputs['ind'].to(device))
    return dict(rows=rows.buf.cpu()[:, 0])


def run_slot_fold(c, device):
    from centertrack_amd import ops
    p = c.inputs['patches']
    gx = V(c.inputs['gx'], device)
    ops.slot_fold(ops.View(p.view(p.shape[0], 1, p.shape[1], p.shape[2]).contiguous().to(device)), c.inputs['ind'].to(device), gx)
    return dict(gx=back(gx))


def _dcn_inputs_are_finite_where_addresses_come_from(t):
    assert bool(torch.isfinite(t[1]).all()) and bool(torch.isfinite(t[2]).all()), 'a DCN never runs on non-finite offsets or masks'


def run_dcn_v2(c, device):
    from centertrack_amd import dcn_v2 as hip
    t = c.inputs['t']
    _dcn_inputs_are_finite_where_addresses_come_from(t)
    with torch.no_grad():
        return dict(y=hip.dcn_v2_conv(*[v.to(device) for v in t[:5]]).cpu())


def run_dcn_v2_backward(c, device):
    from centertrack_amd import dcn_v2 as hip
    from _dcn_bwd import NAMES
    t = c.inputs['t']
    _dcn_inputs_are_finite_where_addresses_come_from(t)
    leaves = [v.detach().to(device).requires_grad_() for v in t[:5]]
    with hip.trainable():
        y = hip.dcn_v2_conv(*leaves)
    return {n: g.cpu() for n, g in zip(NAMES, torch.autograd.grad(y, leaves, t[5].to(device)))}


RUNNERS = dict(bn_act_apply=run_bn_act_apply, bn_act_backward=run_bn_act_backward, stem_bn_relu_sum=run_stem_bn_relu_sum,
               stem_conv_backward=run_stem_conv_backward, maxpool2x2=run_maxpool2x2, maxpool2x2_backward=run_maxpool2x2_backward,
               conv2d_relu=run_conv2d, conv2d_pool=run_conv2d, heads_backward=run_heads_backward,
               conv_backward_weight=run_conv_backward_weight, conv_backward_input=run_conv_backward_input,
               conv_s2_backward=run_conv_s2_backward, upsample_add=run_upsample_add, upsample_add_backward=run_upsample_add_backward,
               slot_gather=run_slot_gather, slot_fold=run_slot_fold, dcn_v2=run_dcn_v2, dcn_v2_backward=run_dcn_v2_backward)


@pytest.mark.parametrize('cid', NF.case_ids())
def test_planted_case(device, cid):
    c = NF.case(cid)
    got = RUNNERS[c.family](c, device)
    torch.cuda.synchronize()
    c.check(got)


# ---------------------------------------------------------------------------------------------------------------------
# the statistics

@pytest.mark.parametrize('name', [s[0] for s in NF.bn_stats_cases()])
def test_bn_stats(device, name):
    """the planted channel's mean, variance and invstd are non-finite exactly as torch's; every other channel keeps the bits of
    the run without the plant.  With the Inf AT the pivot pixel the mean is NaN where torch's is Inf: both non-finite, and the
    variance and invstd are NaN either way"""
    from centertrack_amd import ops
    _, zp, ch = next(s for s in NF.bn_stats_cases() if s[0] == name)
    clean = [t.cpu() for t in ops.bn_stats(V(NF.bn_inputs()[0], device), NB.EPS)]
    got = [t.cpu() for t in ops.bn_stats(V(zp, device), NB.EPS)]
    want = NF.bn_stats_reference(zp)
    others = [i for i in range(zp.shape[1]) if i != ch]
    for what, g, c0, w in zip(('mean', 'var', 'invstd'), got, clean, want):
        assert same_bits(g[others], c0[others]), what
        print('NONFINITE bn_stats %-18s %-6s hip %s torch %s' % (name, what, float(g[ch]), float(w[ch])))
        assert not bool(torch.isfinite(w[ch])) and not bool(torch.isfinite(g[ch])), what
        if name == 'inf-at-the-pivot' and what == 'mean':
            continue
        assert bool(NF.same_nonfinite(g[ch].double(), w[ch])), (what, float(g[ch]), float(w[ch]))


# ---------------------------------------------------------------------------------------------------------------------
# the loss

LOSS_NAMES = [p[0] for p in NF.loss_plants()]
_loss_cache = {}


def _loss_golden(golden_dir):
    if 'g' not in _loss_cache:
        _loss_cache['g'] = NF.load_loss_golden(golden_dir)[0]
    return _loss_cache['g']


def _loss_pattern(got, want, e32, K, what):
    """a loss: non-finite as the reference's, else within the project's bound"""
    got, want = float(got), float(want)
    print('NONFINITE loss %-44s hip %s reference %s' % (what, got, want))
    if want != want:
        assert got != got, what
    elif abs(want) == INF:
        assert got == want, what
    else:
        assert abs(got - want) <= R.bound(e32, K) * abs(want), (what, got, want)


@pytest.mark.parametrize('name', LOSS_NAMES)
def test_loss_on_nonfinite_logits(device, golden_dir, name):
    from centertrack_amd import losses
    want = _loss_golden(golden_dir)[name]
    out, batch, head = NF.loss_case(name)
    heads = NF.LOSS_HEADS
    m32 = R.losses_and_grads(out, batch, heads, torch.float32)
    xs = {h: out[h].to(device).requires_grad_() for h in heads}
    b = {k: v.to(device) for k, v in batch.items()}
    vec = losses.fused_losses([losses.GenericLoss._spec(h, xs, b) for h in heads])
    grads = torch.autograd.grad(vec, [xs[h] for h in heads], torch.ones_like(vec))
    for i, h in enumerate(heads):
        w = float(want['loss'][h])
        e32 = abs(float(m32[h][0]) - w) / abs(w) if w == w and abs(w) != INF and w != 0 else 0.0
        _loss_pattern(vec[i].detach(), w, e32, R.terms(h, out[h].shape, NF.LOSS_M), '%s %s' % (name, h))
        assert bool(torch.isfinite(grads[i]).all()) or h == head, h
    compare(grads[heads.index(head)], want['grad'], NF.project_bound(m32[head][1], 1), what='loss %s grad' % name)
    with torch.no_grad():
        tot, stats = losses.GenericLoss(R.Opt(heads))([{h: out[h].to(device) for h in heads}], b)
    finite = all(bool(torch.isfinite(want['loss'][h])) for h in heads)
    assert bool(torch.isfinite(tot)) == finite
    if not finite:
        bad = [float(want['loss'][h]) for h in heads if not bool(torch.isfinite(want['loss'][h]))]
        assert float(tot) != float(tot) if bad[0] != bad[0] else float(tot) == bad[0]
    for i, h in enumerate(heads):
        assert same_bits(stats[h].reshape(1), vec[i].detach().reshape(1)), h       # the same kernels whichever way they are called


# ---------------------------------------------------------------------------------------------------------------------
# the whole step: DLASeg at 2 x 64 x 64 with the MOT heads (the fixtures of tests/test_hip_dlaseg.py)

def _dlaseg():
    import test_hip_dlaseg as T
    return T


HEAD_W = 'hm.0.weight'                    # the hm head's hidden 3 x 3 convolution: behind the last DeformConv of the network
HEAD_AT = (5, 7, 1, 1)


def _poison(model, value=INF):
    w = dict(model.named_parameters())[HEAD_W]
    with torch.no_grad():
        old = w[HEAD_AT].clone()
        w[HEAD_AT] = value
    return w, old


def _opt(device, **kw):
    T = _dlaseg()
    opt = R.Opt(tuple(T.HEADS))
    opt.num_iters, opt.print_iter, opt.debug, opt.device, opt.task, opt.exp_id = -1, 0, 0, device, 'tracking', 'nonfinite'
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def test_step_with_an_infinite_head_weight_is_skipped_by_the_guard(device):
    """(i) +Inf in one element of a convolution weight, training mode.  The hidden layer's ReLU (the fused epilogue of ct_conv2d)
    meets +Inf where the feature under the weight is positive and 0 * Inf = NaN where it is 0: the loss is NaN, the gradients are
    non-finite, ``skip_nonfinite`` skips the step and nothing moves.  (With fmaxf in the epilogue the NaN became 0, the +Inf
    logits saturated the sigmoid, and the loss was a finite number.)"""
    from centertrack_amd import dcn_v2, losses, optim as O
    T = _dlaseg()
    model = T.build_model(T.state_dict(), device).train()
    (x, pre, hm), batch = T.data(device)
    crit = losses.GenericLoss(R.Opt(tuple(T.HEADS)))
    adam = O.Adam(model.parameters(), 1e-4).guard(None, True)

    def step():
        adam.zero_grad()
        with dcn_v2.trainable():
            out = model(x, pre, hm)[0]
            tot = crit([out], batch)[0]
            tot.backward()
        adam.step()
        return out, tot.detach()
    out, tot = step()                                                  # a clean step first: the Adam state exists and is finite
    assert bool(torch.isfinite(tot)) and adam.grad_stats()['skipped'] == 0
    _poison(model)
    def bits():
        out = []
        for p in model.parameters():
            out.append(p.detach().clone().view(torch.int32))
            if 'exp_avg' in adam.state.get(p, {}):
                out += [adam.state[p][k].detach().clone().view(torch.int32) for k in ('exp_avg', 'exp_avg_sq')]
        return out
    before = bits()
    out, tot = step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out['hm']).any()) and bool(torch.isfinite(out['reg']).all())
    assert not bool(torch.isfinite(tot))
    st = adam.grad_stats()
    assert st['skipped'] == 1 and st['nonfinite'] >= 1
    after = bits()
    assert len(before) == len(after) > 600 and all(torch.equal(a, b) for a, b in zip(before, after))


def _two_batches(device):
    T = _dlaseg()
    from centertrack_amd import weights as Wt
    out = []
    for i in range(2):
        x, pre, hm = Wt.synthetic_inputs(T.N, T.H, T.W, seed=T.SEED + 10 * i)
        _, batch = R.make_batch(T.SEED + 1 + i, T.N, T.H // 4, T.W // 4, 8, tuple(T.HEADS), 1)
        batch.update(image=x, pre_img=pre, pre_hm=hm)
        out.append(batch)
    return out


def _poison_first_batch_only(model):
    """the weight holds +Inf while the first batch runs and its own value again from the second batch on"""
    state = {'calls': 0, 'old': None}

    def hook(module, args):
        if state['calls'] == 0:
            state['old'] = _poison(model)[1]
        elif state['calls'] == 1:
            with torch.no_grad():
                dict(model.named_parameters())[HEAD_W][HEAD_AT] = state['old']
        state['calls'] += 1
    model.register_forward_pre_hook(hook)


def test_trainer_epoch_with_a_poisoned_first_batch(device, capsys):
    from centertrack_amd import optim as O
    from centertrack_amd.trainer import Trainer
    T = _dlaseg()
    sd = T.state_dict()
    model = T.build_model(sd, device)
    _poison_first_batch_only(model)
    tr = Trainer(_opt(device, skip_nonfinite=True), model, O.Adam(model.parameters(), 1e-4))
    tr.set_device([0], [2], device)
    ret, _ = tr.train(1, _two_batches(device))
    assert ret['skipped'] == 1 and ret['grad_norm'] == ret['grad_norm'] and 0.0 < ret['grad_norm'] < INF
    assert ret['tot'] != ret['tot']                                    # the epoch's average holds the first batch's NaN: the loss line shows it
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    # without the guard the NaN gradients reach Adam, and every later loss is NaN as well
    model2 = T.build_model(sd, device)
    _poison_first_batch_only(model2)
    tr2 = Trainer(_opt(device), model2, O.Adam(model2.parameters(), 1e-4))
    tr2.set_device([0], [2], device)
    ret2, _ = tr2.train(1, _two_batches(device))
    assert ret2['tot'] != ret2['tot'] and 'skipped' not in ret2
    assert not all(bool(torch.isfinite(p).all()) for p in model2.parameters())


def test_backbone_on_running_statistics_carries_a_nan_pixel(device):
    """(ii) eval mode, through the training modules on running statistics, one NaN input pixel: the stems' BatchNorm + ReLU, every
    fused ReLU and every pool carry it, and each of the six level maps holds a NaN (the backbone alone: it has no DeformConv)"""
    from centertrack_amd import dla_base
    T = _dlaseg()
    sd = T.state_dict()
    base = dla_base.dla34(pretrained=False, opt=BB.Opt())
    base.load_state_dict({k[len('base.'):]: v for k, v in sd.items() if k.startswith('base.')})
    base = base.to(device).eval()
    (x, pre, hm), _ = T.data(device)
    xp = x.clone()
    xp[1, 2, 30, 41] = NAN
    with torch.no_grad():
        levels, clean = base(xp, pre, hm), base(x, pre, hm)
    torch.cuda.synchronize()
    for lv, (y, y0) in enumerate(zip(levels, clean)):
        assert bool(torch.isfinite(y0).all())
        bad = torch.isnan(y)
        print('NONFINITE backbone level %d: %d of %d elements NaN' % (lv, int(bad.sum()), bad.numel()))
        assert bool(bad.any()) and not bool(bad[0].any()), lv          # image 1 alone: running statistics do not mix the images
        assert not bool(torch.isinf(y).any())
    # the first levels keep the NaN local: the 7 x 7 stem and two 3 x 3 convolutions reach 5 pixels each way
    bad0 = torch.isnan(levels[0][1]).any(0).nonzero()
    assert int(bad0[:, 0].min()) >= 30 - 5 and int(bad0[:, 0].max()) <= 30 + 5 and int(bad0[:, 1].min()) >= 41 - 5 and int(bad0[:, 1].max()) <= 41 + 5


def test_a_nan_heat_map_logit_is_a_nan_loss(device):
    """(iii) a NaN planted in one hm logit through a forward hook: the loss is NaN, as the reference prints it"""
    from centertrack_amd import dcn_v2, losses
    T = _dlaseg()
    model = T.build_model(T.state_dict(), device).train()
    (x, pre, hm), batch = T.data(device)

    def hook(module, args, output):
        out = dict(output[0])
        at = torch.zeros_like(out['hm'], dtype=torch.bool)
        at[1, 0, 3, 5] = True
        out['hm'] = torch.where(at, torch.full_like(out['hm'], NAN), out['hm'])
        return [out]
    model.register_forward_hook(hook)
    crit = losses.GenericLoss(R.Opt(tuple(T.HEADS)))
    with dcn_v2.trainable():
        out = model(x, pre, hm)
        tot, stats = crit(out, batch)
    torch.cuda.synchronize()
    assert int(torch.isnan(out[0]['hm']).sum()) == 1
    assert float(tot) != float(tot) and float(stats['hm']) != float(stats['hm'])
    assert all(bool(torch.isfinite(stats[h])) for h in T.HEADS if h != 'hm')
