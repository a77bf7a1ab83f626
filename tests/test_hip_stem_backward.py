"""GPU: the trainable 7x7 stems (centertrack_amd/csrc/stem_train.hip, ``dla_base._StemsFunction``) against float64 torch
autograd on the CPU of ``_backbone_bwd.stem`` (tests/_stem_bwd.py).  Error measure and bound are the project's
(tests/_dcn_bwd.py): ``err`` relative to the tensor's maximum, ``bound(e32, K) = min(1e-3, 4 max(e32, 2^-23 sqrt(K)))`` with e32
the float32 CPU run of the same construction; K = 49 Cin for ``z_s`` and its term (147 for the sum ``y``), N*H*W for ``gw``,
``ggamma`` and ``gbeta``, 784 for an image gradient.

Gradient truths take every ReLU mask from the HIP forward's own term ``relu(bn_s(z_s))`` (``ct_bn_relu_apply`` on the same
``z_s``: what ``dla_base.trace`` emits and, bit for bit, what ``ct_stem_bn_relu_sum`` adds), held against the free float64 run
under ``_backbone_bwd.check_mask`` (tests/test_stem_backward_cpu.py holds the float32 reference to 0 flipped units for the same
seeds).  Shapes: ``_stem_bwd.SHAPES``, which the CPU file holds against ``_stem_bwd.REGIMES``.

Measured on an MI355X: see DESIGN.md section 14."""
import pytest
import torch

import _backbone_bwd as BB
import _stem_bwd as SB
from _backbone_bwd import Report, err

pytestmark = pytest.mark.gpu

EPS = SB.EPS


def nhwc(t, dev, ld=None, c0=0):
    """NCHW CPU tensor -> NHWC view on the device, channels c0 .. c0 + 16 of a buffer of pitch ``ld`` filled with 7"""
    from centertrack_amd import ops
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, ld or C), 7.0, dtype=torch.float32)
    buf[..., c0:c0 + C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(dev), c0, C)


def back(v):
    return v.to_nchw().cpu()


def sentinel_view(N, H, W, dev, c0=4, tail=4):
    """a caller-owned 16-channel output view inside a wider buffer: NaN where the kernel has to write, 7 in the padding"""
    from centertrack_amd import ops
    buf = torch.full((N, H, W, c0 + 16 + tail), 7.0, device=dev)
    buf[..., c0:c0 + 16] = float('nan')
    return ops.View(buf, c0, 16)


def untouched(v):
    rest = torch.ones(v.ld, dtype=torch.bool)
    rest[v.c0:v.c0 + v.C] = False
    return bool((v.buf.cpu()[..., rest] == 7.0).all())


def poison(dev, *numels):
    """blocks of these sizes are filled with NaN and freed first (stream-ordered): an element a kernel skips in an output that
    the wrapper allocates from torch's caching allocator is then seen by the comparison that follows"""
    blocks = [torch.full((n,), float('nan'), device=dev) for n in numels]
    del blocks


def hip_ops(shape, stems, training, dev, hm='sparse', sd=None, caller=False):
    """the op chain of one training step of the stems in ``stems`` -> dict of CPU tensors per stem and the sum ``y``; with
    ``caller`` every output goes to a caller-owned buffer (returned under 'views')"""
    from centertrack_amd import ops
    N, H, W = shape
    sd0, xs, gy = SB.case(shape, hm)
    sd = sd or sd0
    P = N * H * W
    dx = [xs[s].to(dev) if s in stems else None for s in range(3)]
    dw = [sd[SB.PREFIX[s] + '0.weight'].to(dev) if s in stems else None for s in range(3)]
    poison(dev, P * 16, P * 16, P * 16, P * 3, 16 * 147)
    zv = [sentinel_view(N, H, W, dev) if s in stems else None for s in range(3)] if caller else None
    zs = ops.stem_conv_forward(dx, dw, out=zv)
    means, invstds, gammas, betas, var = [None] * 3, [None] * 3, [None] * 3, [None] * 3, [None] * 3
    for s in stems:
        p = SB.PREFIX[s]
        gammas[s], betas[s] = sd[p + '1.weight'].to(dev), sd[p + '1.bias'].to(dev)
        if training:
            means[s], var[s], invstds[s] = ops.bn_stats(zs[s], EPS)
        else:
            means[s] = sd[p + '1.running_mean'].to(dev)
            invstds[s] = torch.rsqrt(sd[p + '1.running_var'].to(dev) + EPS)
    terms = [ops.bn_relu_apply(zs[s], means[s], invstds[s], gammas[s], betas[s]) if s in stems else None for s in range(3)]
    yv = sentinel_view(N, H, W, dev, c0=8, tail=8) if caller else None
    y = ops.stem_bn_relu_sum(zs, means, invstds, gammas, betas, out=yv)
    gyv = nhwc(gy, dev, ld=24 if caller else None, c0=4 if caller else 0)
    gzs, gg, gb = [None] * 3, [None] * 3, [None] * 3
    for s in stems:
        gzs[s], gg[s], gb[s] = ops.bn_relu_backward(zs[s], gyv, means[s], invstds[s], gammas[s], betas[s], training)
    if caller:                                          # the gradients of z as views with a pitch, too
        gzs = [None if g is None else nhwc(back(g), dev, ld=20, c0=0) for g in gzs]
    gws = [torch.full((16, SB.CIN[s], 7, 7), float('nan'), device=dev) for s in range(3)] if caller else None
    gins = [torch.full((N, SB.CIN[s], H, W), float('nan'), device=dev) for s in range(3)] if caller else None
    need = [s in stems for s in range(3)]
    gw, gin = ops.stem_conv_backward(gzs, dx, dw, need_w=need, need_in=need, gws=gws, gins=gins)
    torch.cuda.synchronize()
    res = dict(y=back(y), stems={}, views=dict(z=zv, y=yv, gw=gws, gin=gins, gz=gzs, gy=gyv))
    for s in stems:
        res['stems'][s] = dict(z=back(zs[s]), term=back(terms[s]), gw=gw[s].cpu(), gin=gin[s].cpu(), ggamma=gg[s].cpu(),
                               gbeta=gb[s].cpu(), mean=means[s].cpu(), var=None if var[s] is None else var[s].cpu())
    return res


def compare(rep, shape, stems, training, got, hm='sparse'):
    """every tensor of ``got`` against the shared truths; -> flipped ReLU units"""
    N, H, W = shape
    P = N * H * W
    flips = 0
    y64 = y32 = None
    for s in stems:
        g = got['stems'][s]
        f64, f32, t64, t32 = SB.truth(shape, s, training, g['term'], hm)
        flips += BB.check_mask(t64['mask'], f64['pre'], err(f32['y'], f64['y']) if float(f64['y'].abs().max()) > 0 else 0.0,
                               'stem %d' % s)[0]
        tag = 'stem%d ' % s
        rep.add(tag + 'z', g['z'], t64['z'], t32['z'], SB.K_OUT[s])
        rep.add(tag + 'term', g['term'], t64['y'], t32['y'], SB.K_OUT[s])
        rep.add(tag + 'gw', g['gw'], t64['gw'], t32['gw'], P)
        rep.add(tag + 'ggamma', g['ggamma'], t64['ggamma'], t32['ggamma'], P)
        rep.add(tag + 'gbeta', g['gbeta'], t64['gbeta'], t32['gbeta'], P)
        rep.add(tag + 'gin', g['gin'], t64['gin'], t32['gin'], SB.K_IN)
        y64 = t64['y'] if y64 is None else y64 + t64['y']
        y32 = t32['y'] if y32 is None else y32 + t32['y']
    rep.add('y', got['y'], y64, y32, max(SB.K_OUT[s] for s in stems))
    return flips


def same_bits(a, b):
    assert torch.equal(a['y'], b['y'])
    for s in a['stems']:
        for k, v in a['stems'][s].items():
            assert v is None or torch.equal(v, b['stems'][s][k]), (s, k)


@pytest.mark.parametrize('training', [True, False], ids=['batch', 'running'])
@pytest.mark.parametrize('subset', list(SB.SUBSETS))
@pytest.mark.parametrize('shape', SB.SHAPES, ids=SB.shape_id)
def test_ops_against_float64(device, shape, subset, training):
    stems = SB.SUBSETS[subset]
    title = 'stems %s %s %s' % (SB.shape_id(shape), subset, 'batch' if training else 'running')
    got = hip_ops(shape, stems, training, device)
    # the sum kernel's terms are ct_bn_relu_apply's, added in the order x, pre_img, pre_hm: torch's sum of the terms, bit for bit
    want = None
    for s in stems:
        want = got['stems'][s]['term'] if want is None else want + got['stems'][s]['term']
    assert torch.equal(got['y'], want)
    rep = Report(title)
    flips = compare(rep, shape, stems, training, got)
    print('%s: %d ReLU units flipped' % (title, flips))
    same_bits(got, hip_ops(shape, stems, training, device))             # a second run: every op, every bit
    rep.check()


@pytest.mark.parametrize('shape', [(2, 20, 36), (1, 7, 33)], ids=SB.shape_id)
def test_caller_buffers(device, shape):
    """every output in a NaN-filled caller-owned buffer, the maps as 16 channels of a wider buffer with a sentinel in the
    padding: the same bits as the wrapper-allocated run, the padding untouched"""
    own = hip_ops(shape, (0, 1, 2), True, device)
    got = hip_ops(shape, (0, 1, 2), True, device, caller=True)
    same_bits(own, got)
    v = got['views']
    assert all(untouched(z) for z in v['z']) and untouched(v['y']) and untouched(v['gy']) and all(untouched(g) for g in v['gz'])
    for s in range(3):
        assert torch.equal(v['gw'][s].cpu(), got['stems'][s]['gw']) and torch.equal(v['gin'][s].cpu(), got['stems'][s]['gin'])


def test_left_out_outputs_are_left_alone(device):
    """gw / gin NULL per stem: the buffers a caller holds for them stay as they are, the others get the bits of the full call"""
    from centertrack_amd import ops
    shape = (2, 20, 36)
    N, H, W = shape
    full = hip_ops(shape, (0, 1, 2), True, device, caller=True)
    v = full['views']
    sd, xs, _ = SB.case(shape)
    dx = [x.to(device) for x in xs]
    dw = [sd[p + '0.weight'].to(device) for p in SB.PREFIX]
    gws = [torch.full((16, c, 7, 7), 7.0, device=device) for c in SB.CIN]
    gins = [torch.full((N, c, H, W), 7.0, device=device) for c in SB.CIN]
    gw, gin = ops.stem_conv_backward(v['gz'], dx, dw, need_w=(True, False, True), need_in=(False, True, False), gws=gws, gins=gins)
    torch.cuda.synchronize()
    assert gw[1] is None and gin[0] is None and gin[2] is None
    assert bool((gws[1] == 7).all()) and bool((gins[0] == 7).all()) and bool((gins[2] == 7).all())
    for s in (0, 2):
        assert gw[s] is gws[s] and torch.equal(gw[s].cpu(), full['stems'][s]['gw'])
    assert gin[1] is gins[1] and torch.equal(gin[1].cpu(), full['stems'][1]['gin'])
    # a stem whose gz is absent, and a call that asks for nothing
    gw, gin = ops.stem_conv_backward([v['gz'][0], None, None], dx, dw, need_w=(True, True, True), need_in=(False, False, False))
    assert gw[1] is None and gw[2] is None and torch.equal(gw[0].cpu(), full['stems'][0]['gw'])
    assert ops.stem_conv_backward(v['gz'], dx, dw, need_w=(False,) * 3, need_in=(False,) * 3) == ([None] * 3, [None] * 3)


# ---------------------------------------------------------------------------------------------------------------------
# the module path: dla_base._stems over nn.Sequential stems

def module_run(mods, xs, gy, device, training, record=True):
    """forward (+ backward unless ``record`` is 'no_grad' or 'not trainable') of ``dla_base._stems`` with the trace on -> (y NHWC,
    input gradients, parameter gradients, the terms the trace received as NCHW CPU tensors)"""
    from centertrack_amd import dcn_v2, dla_base
    mods.train(training)
    layers = [getattr(mods, p[:-1]) for p in SB.PREFIX]
    ins = [x.to(device).requires_grad_() for x in xs]
    mods.zero_grad(set_to_none=True)
    dla_base.trace = []
    try:
        if record is True:
            with dcn_v2.trainable():
                y = dla_base._stems(ins, layers)
                (y * gy.to(device).permute(0, 2, 3, 1)).sum().backward()
        elif record == 'no_grad':
            with dcn_v2.trainable(), torch.no_grad():
                y = dla_base._stems(ins, layers)
        else:                                                           # trainable() off
            y = dla_base._stems(ins, layers)
        torch.cuda.synchronize()
        terms = [t.permute(0, 3, 1, 2).cpu().contiguous() for t in dla_base.trace]
    finally:
        dla_base.trace = None
    return y, [x.grad for x in ins], {k: p.grad for k, p in mods.named_parameters()}, terms


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_module_against_float64(device, training):
    """the autograd node on a shape of the op tests: the same truths (the trace emits the terms the op test held), running
    statistics after two training calls as float64 moves them, nothing recorded without a graph"""
    from centertrack_amd import dla_base
    shape = (2, 20, 36)
    P = shape[0] * shape[1] * shape[2]
    sd, xs, gy = SB.case(shape)
    mods = SB.Stems()
    mods.load_state_dict(sd)
    mods = mods.to(device)
    y, gin, gpar, terms = module_run(mods, xs, gy, device, training)
    assert len(terms) == 3 and y.shape == (shape[0], shape[1], shape[2], 16)
    rep = Report('stems module %s' % ('train' if training else 'eval'))
    y64 = y32 = None
    for s in range(3):
        f64, f32, t64, t32 = SB.truth(shape, s, training, terms[s])
        p = SB.PREFIX[s]
        rep.add(p + 'input', gin[s], t64['gin'], t32['gin'], SB.K_IN)
        for k, name in (('0.weight', 'gw'), ('1.weight', 'ggamma'), ('1.bias', 'gbeta')):
            rep.add(p + k, gpar[p + k], t64[name], t32[name], P)
        y64 = t64['y'] if y64 is None else y64 + t64['y']
        y32 = t32['y'] if y32 is None else y32 + t32['y']
    rep.add('y', y.permute(0, 3, 1, 2), y64, y32, 147)
    if training:
        module_run(mods, xs, gy, device, True)                        # a second training call
        got = mods.state_dict()
        for s in range(3):
            p = SB.PREFIX[s]
            ref = {}
            for dt in (torch.float64, torch.float32):
                once = SB.stem_reference(s, sd, xs[s], None, True, dt)['sd']
                ref[dt] = SB.stem_reference(s, once, xs[s], None, True, dt)['sd']
            assert int(got[p + '1.num_batches_tracked']) == 2 == int(ref[torch.float64][p + '1.num_batches_tracked'])
            for k in ('1.running_mean', '1.running_var'):
                rep.add(p + k, got[p + k], ref[torch.float64][p + k], ref[torch.float32][p + k], P)
        mods.load_state_dict(sd)                                        # (the statistics back where the first call found them)
        mods.train(True)
    # without a graph: the same bits, nothing recorded, no per-stem map unless the trace is on
    for off in ('no_grad', 'not trainable'):
        mods.load_state_dict(sd)
        y2, _, _, terms2 = module_run(mods, xs, gy, device, training, record=off)
        assert torch.equal(y2, y) and y2.grad_fn is None and not y2.requires_grad
        assert all(torch.equal(a, b) for a, b in zip(terms, terms2))
    rep.check()


def test_eval_mode_agrees_with_the_inference_kernel(device):
    """eval mode against ``ct_stem_forward`` (the BatchNorm folded to scale and shift, as the inference plan does) on the same
    parameters, within bound(e32, 147)"""
    from centertrack_amd import dla_base, ops
    shape = (2, 64, 64)
    sd, xs, gy = SB.case(shape)
    mods = SB.Stems()
    mods.load_state_dict(sd)
    mods = mods.to(device).eval()
    layers = [getattr(mods, p[:-1]) for p in SB.PREFIX]
    dx = [x.to(device) for x in xs]
    y = dla_base._stems(dx, layers)
    scale = torch.stack([sd[p + '1.weight'].double() / torch.sqrt(sd[p + '1.running_var'].double() + EPS) for p in SB.PREFIX])
    shift = torch.stack([sd[p + '1.bias'].double() - sd[p + '1.running_mean'].double() * scale[i] for i, p in enumerate(SB.PREFIX)])
    w = [sd[p + '0.weight'].to(device) for p in SB.PREFIX]
    inf = ops.stem(dx[0], dx[1], dx[2], w[0], w[1], w[2], scale.float().to(device).contiguous(), shift.float().to(device).contiguous())
    torch.cuda.synchronize()
    y64 = y32 = None
    for s in range(3):
        r64, r32 = (SB.stem_reference(s, sd, xs[s], None, False, dt) for dt in (torch.float64, torch.float32))
        y64 = r64['y'] if y64 is None else y64 + r64['y']
        y32 = r32['y'] if y32 is None else y32 + r32['y']
    rep = Report('stems eval')
    rep.add('y', y.permute(0, 3, 1, 2), y64, y32, 147)
    rep.add('ct_stem_forward', back(inf), y64, y32, 147)
    b = BB.bound(err(y32, y64), 147)
    e = err(y.permute(0, 3, 1, 2).cpu(), back(inf).double())
    print('stems eval: the trainable path against ct_stem_forward: err %.2e, bound %.2e' % (e, b))
    assert e <= b
    rep.check()


@pytest.mark.parametrize('beta', ['zero', 'positive'])
def test_all_zero_heat_map_in_training_mode(device, beta):
    """the first frame of every video: an all-zero pre_hm under batch statistics (z = 0, mean = 0, var = 0).  Everything stays
    finite and the stem's weight gradient is exactly 0; with beta = 0 (torch's initialisation) the pre-activation is exactly 0
    and the mask follows torch's rule, gradient 0 at exactly 0"""
    shape = (2, 20, 36)
    P = shape[0] * shape[1] * shape[2]
    sd, xs, gy = SB.case(shape, 'zero')
    sd['pre_hm_layer.1.bias'] = torch.zeros(16) if beta == 'zero' else torch.full((16,), 0.25)
    mods = SB.Stems()
    mods.load_state_dict(sd)
    mods = mods.to(device)
    y, gin, gpar, terms = module_run(mods, xs, gy, device, True)
    for t in [y] + gin + list(gpar.values()) + [b for _, b in mods.named_buffers()]:
        assert bool(torch.isfinite(t).all())
    assert float(gpar['pre_hm_layer.0.weight'].abs().max()) == 0.0
    if beta == 'zero':
        assert float(terms[2].abs().max()) == 0.0
        for k in ('pre_hm_layer.1.weight', 'pre_hm_layer.1.bias'):
            assert float(gpar[k].abs().max()) == 0.0, k
        assert float(gin[2].abs().max()) == 0.0
    rep = Report('zero pre_hm, beta %s' % beta)
    y64 = y32 = None
    for s in range(3):
        p = SB.PREFIX[s]
        r = [SB.stem_reference(s, sd, xs[s], gy, True, dt, terms[s]) for dt in (torch.float64, torch.float32)]
        for k, name in (('0.weight', 'gw'), ('1.weight', 'ggamma'), ('1.bias', 'gbeta')):
            rep.add(p + k, gpar[p + k], r[0][name], r[1][name], P)
        rep.add(p + 'input', gin[s], r[0]['gin'], r[1]['gin'], SB.K_IN)
        y64 = r[0]['y'] if y64 is None else y64 + r[0]['y']
        y32 = r[1]['y'] if y32 is None else y32 + r[1]['y']
    rep.add('y', y.permute(0, 3, 1, 2), y64, y32, 147)
    rep.check()


def test_dla34_stem_gradients_are_bitwise_reproducible(device):
    """two runs of ``dla34`` forward + backward under ``trainable()``: the stems' parameter gradients and the three image
    gradients agree in every bit (with the torch stems they agreed to 1e-5 only)"""
    from centertrack_amd import dcn_v2, dla_base
    name = 'dla34'
    seed = BB.SEEDS[name]
    mod = BB.MODULES[name][0](dla_base)
    mod.load_state_dict(BB.random_params(seed, mod))
    mod = mod.to(device).train()
    inputs = BB.module_inputs(name, seed + 1)

    def run():
        xs = [x.to(device).requires_grad_() for x in inputs]
        mod.zero_grad(set_to_none=True)
        with dcn_v2.trainable():
            outs = BB.module_call(name, mod, xs)
            gys = BB.output_gradients(outs, seed + 20)
            sum((o * g.to(device)).sum() for o, g in zip(outs, gys)).backward()
        torch.cuda.synchronize()
        return [x.grad for x in xs], {k: p.grad for k, p in mod.named_parameters() if k.startswith(SB.PREFIX)}
    gin, gpar = run()
    gin2, gpar2 = run()
    assert len(gpar) == 9
    for a, b in zip(gin, gin2):
        assert a is not None and float(a.abs().max()) > 0 and torch.equal(a, b)
    for k in gpar:
        assert gpar[k] is not None and float(gpar[k].abs().max()) > 0 and torch.equal(gpar[k], gpar2[k]), k
