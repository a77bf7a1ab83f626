"""GPU: the trainable neck (centertrack_amd/csrc/bn_train.hip, centertrack_amd/csrc/neck_bwd.hip, centertrack_amd/dla_up.py) against float64 torch autograd on
the CPU of the restated reference construction (tests/_neck_bwd.py).  Error measure and bound are the project's
(tests/_dcn_bwd.py): ``err`` relative to the tensor's maximum, ``bound(e32, K) = min(1e-3, 4 max(e32, 2^-23 sqrt(K)))`` with
e32 the float32 CPU run of the same construction.  K = N*H*W for the BatchNorm gradients, the up-sampling weight gradient and
every weight and bias gradient, 4 f^2 for the up-sampling input gradient, ``_dcn_bwd.terms`` for what the DCN produces
(36 Cout for an input gradient), and 9 Cin -- the terms of one output element -- for a forward output.  Gradient truths take
the ReLU mask from the HIP forward's own output; a separate assertion holds that mask (``_neck_bwd.check_mask``).

The op tests run twice: at toy shapes (``BN_SHAPES``, ``UP_SHAPES``), where every slab count sits at its pixel limit, and at
``BN_PLAN_SHAPES`` / ``UP_PLAN_SHAPES``, the smallest shapes that reach what production training reaches -- a slab count from the
grid target, an element-wise grid capped at 2048 workgroups (``_neck_bwd.BN_REGIMES`` / ``UP_REGIMES``;
tests/test_neck_backward_cpu.py holds the lists against them)."""
import pytest
import torch
import torch.nn.functional as F

import _neck_bwd as NB
from _neck_bwd import bound, err

pytestmark = pytest.mark.gpu


class Report(object):
    """collects (name, error, bound) of one test, prints every figure and fails at the end with all of them"""

    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, name, got, t64, t32, K, norm=None):
        got, t64, t32 = got.detach().cpu().double(), t64.detach().double(), t32.detach().double()
        assert got.shape == t64.shape, (name, got.shape, t64.shape)
        if norm is None and float(t64.abs().max()) == 0.0:
            e, e32, b = float(got.abs().max()), 0.0, 0.0
        else:
            e, e32 = err(got, t64, norm), err(t32, t64, norm)
            b = bound(e32, K)
        self.rows.append((name, e, e32, b))
        print('%s %-44s err %.2e  e32 %.2e  bound %.2e%s' % (self.title, name, e, e32, b, '' if e <= b else '   <-- MISSES'))

    def check(self):
        bad = [r for r in self.rows if not r[1] <= r[3]]
        assert not bad, '%s: %s' % (self.title, ['%s err %.2e > bound %.2e' % (r[0], r[1], r[3]) for r in bad])


def nhwc_view(t, dev, ld=None, c0=0):
    """NCHW CPU tensor -> NHWC view on the device, as channels c0 .. c0 + C of a buffer of pitch ``ld``"""
    from centertrack_amd import ops
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, ld or C), 7.0, dtype=torch.float32)
    buf[..., c0:c0 + C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(dev), c0, C)


def back(v):
    return v.to_nchw().cpu()


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm ops

bn_case = NB.bn_case


def bn_reference(case, dtype, batch, mask=None):
    z, gamma, beta, rm, rv, gy = (t.to(dtype) for t in case)
    z, gamma, beta = (t.clone().requires_grad_() for t in (z, gamma, beta))
    pre = F.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, batch, NB.MOMENTUM, NB.EPS)
    y = torch.relu(pre) if mask is None else pre * mask.to(dtype)
    gz, gg, gb = torch.autograd.grad(y, (z, gamma, beta), gy)
    zd = z.detach()
    return dict(pre=pre.detach(), y=y.detach(), gz=gz, gg=gg, gb=gb, mean=zd.mean((0, 2, 3)),
                var=zd.var((0, 2, 3), unbiased=False))


@pytest.mark.parametrize('batch', [True, False], ids=['batch-stats', 'running-stats'])
@pytest.mark.parametrize('shape', NB.BN_SHAPES, ids=str)
def test_bn_ops(device, shape, batch):
    from centertrack_amd import ops
    N, H, W, C = shape
    P = N * H * W
    case = bn_case(shape)
    z, gamma, beta, rm, rv, gy = case
    sliced = C == 8                                     # the 8-channel case is a channel slice of a 16-wide buffer
    zv = nhwc_view(z, device, 16 if sliced else None, 4 if sliced else 0)
    gyv = nhwc_view(gy, device, 16 if sliced else None, 8 if sliced else 0)
    g, b = gamma.to(device), beta.to(device)
    rep = Report('bn %s %s' % (shape, 'batch' if batch else 'running'))

    def run(need_gamma=True, need_beta=True):
        if batch:
            mean, var, invstd = ops.bn_stats(zv, NB.EPS)
        else:
            mean, var = rm.to(device), rv.to(device)
            invstd = torch.rsqrt(var + NB.EPS)
        y = ops.bn_relu_apply(zv, mean, invstd, g, b)
        gz, gg, gb = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, batch, need_gamma=need_gamma, need_beta=need_beta)
        return mean, var, y, gz, gg, gb
    mean, var, y, gz, gg, gb = run()
    yh = back(y)
    mask = yh > 0
    free64, free32 = bn_reference(case, torch.float64, batch), bn_reference(case, torch.float32, batch)
    t64, t32 = bn_reference(case, torch.float64, batch, mask), bn_reference(case, torch.float32, batch, mask)
    flipped, near = NB.check_mask(mask, free64['pre'], err(free32['y'], free64['y']), rep.title)
    print('%s: %d ReLU units flipped, %d within the threshold, of %d' % (rep.title, flipped, near, mask.numel()))
    assert not bool(mask[:, 2].any()) and bool((free64['pre'][:, 2] < 0).all())          # the all-negative channel
    if batch:
        rep.add('mean', mean, t64['mean'], t32['mean'], P)
        rep.add('var', var, t64['var'], t32['var'], P)
        assert float(var[1]) == 0.0                                                      # the constant channel
    rep.add('y', yh, free64['y'], free32['y'], P)
    rep.add('gz', back(gz), t64['gz'], t32['gz'], P)
    rep.add('ggamma', gg, t64['gg'], t32['gg'], P)
    rep.add('gbeta', gb, t64['gb'], t32['gb'], P)
    # two runs are bitwise equal; with gamma / beta frozen what remains is unchanged bit for bit
    again = run()
    for u, v in zip((mean, var, y.buf, gz.buf, gg, gb), (again[0], again[1], again[2].buf, again[3].buf, again[4], again[5])):
        assert torch.equal(u, v)
    frozen = run(need_gamma=False, need_beta=False)
    assert frozen[4] is None and frozen[5] is None and torch.equal(frozen[3].buf, gz.buf) and torch.equal(frozen[2].buf, y.buf)
    only_beta = run(need_gamma=False)
    assert only_beta[4] is None and torch.equal(only_beta[5], gb)
    rep.check()


@pytest.mark.parametrize('shape', NB.BN_SHAPES, ids=str)
def test_bn_running_statistics_after_two_training_calls(device, shape):
    from centertrack_amd import dla_up, ops
    N, H, W, C = shape
    P = N * H * W
    zs = [bn_case(shape)[0], (NB.randn(41, N, C, H, W) * 2 + 1).float()]
    bn = torch.nn.BatchNorm2d(C, momentum=NB.MOMENTUM).to(device)
    ref = {}
    for dt in (torch.float64, torch.float32):
        rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
        for z in zs:
            F.batch_norm(z.to(dt), rm, rv, None, None, True, NB.MOMENTUM, NB.EPS)
        ref[dt] = (rm, rv)
    for z in zs:
        mean, var, _ = ops.bn_stats(nhwc_view(z, device), bn.eps)
        dla_up.update_running_stats(bn, mean, var, P)
    rep = Report('bn running %s' % (shape,))
    rep.add('running_mean', bn.running_mean, ref[torch.float64][0], ref[torch.float32][0], P)
    rep.add('running_var', bn.running_var, ref[torch.float64][1], ref[torch.float32][1], P)
    assert int(bn.num_batches_tracked) == 2
    rep.check()


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans production training reaches (``_neck_bwd.BN_PLAN_SHAPES`` / ``UP_PLAN_SHAPES`` name the regime of each shape)

def sentinel_view(N, H, W, C, dev, c0=4, tail=4):
    """a caller-owned output view, channels c0 .. c0 + C of a wider buffer: NaN where the kernel has to write, 7 in the padding"""
    from centertrack_amd import ops
    buf = torch.full((N, H, W, c0 + C + tail), 7.0, device=dev)
    buf[..., c0:c0 + C] = float('nan')
    return ops.View(buf, c0, C)


def untouched(v):
    """the channels of the buffer outside the view still hold the fill value"""
    rest = torch.ones(v.ld, dtype=torch.bool)
    rest[v.c0:v.c0 + v.C] = False
    return bool((v.buf[..., rest.to(v.buf.device)] == 7.0).all())


def poison(dev, *numels):
    """An output the wrapper allocates itself comes from torch's caching allocator, which may hand back the block an earlier
    run of the same case wrote.  Blocks of these sizes are filled with NaN and freed first (stream-ordered), so that an
    element the kernel skips is seen by the comparison that follows."""
    blocks = [torch.full((n,), float('nan'), device=dev) for n in numels]
    del blocks


@pytest.mark.parametrize('batch', [True, False], ids=['batch-stats', 'running-stats'])
@pytest.mark.parametrize('shape', NB.BN_PLAN_SHAPES, ids=str)
def test_bn_ops_at_plan_shapes(device, shape, batch):
    """``test_bn_ops`` where the slab count comes from the grid target and the element-wise grid is capped at 2048
    workgroups; y goes into a caller-owned view pre-filled with NaN.  Under batch statistics ``y`` at 1x66x70x512 and 1x12x20x16 sits
    at 0.97 / 0.95 of its bound (measured 3.15e-5 / 3.24e-5 and 2.46e-5 / 2.58e-5): the mean-100 channel, where a = gamma * invstd
    = 91 multiplies the rounding of the fp32 mean (3.1e-6, 1.2e-6) and nothing else is left"""
    from centertrack_amd import ops
    N, H, W, C = shape
    P = N * H * W
    case = bn_case(shape)
    z, gamma, beta, rm, rv, gy = case
    zv, gyv = nhwc_view(z, device), nhwc_view(gy, device)
    g, b = gamma.to(device), beta.to(device)
    rep = Report('bn plan %s %s' % (shape, 'batch' if batch else 'running'))

    def run(need_gamma=True, need_beta=True):
        if batch:
            mean, var, invstd = ops.bn_stats(zv, NB.EPS)
        else:
            mean, var = rm.to(device), rv.to(device)
            invstd = torch.rsqrt(var + NB.EPS)
        out = sentinel_view(N, H, W, C, device)
        y = ops.bn_relu_apply(zv, mean, invstd, g, b, out=out)
        assert y is out and untouched(out)
        poison(device, P * C)
        gz, gg, gb = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, batch, need_gamma=need_gamma, need_beta=need_beta)
        return mean, var, y, gz, gg, gb
    mean, var, y, gz, gg, gb = run()
    yh = back(y)
    mask = yh > 0
    free64, free32 = bn_reference(case, torch.float64, batch), bn_reference(case, torch.float32, batch)
    t64, t32 = bn_reference(case, torch.float64, batch, mask), bn_reference(case, torch.float32, batch, mask)
    flipped, near = NB.check_mask(mask, free64['pre'], err(free32['y'], free64['y']), rep.title)
    print('%s: %d ReLU units flipped, %d within the threshold, of %d' % (rep.title, flipped, near, mask.numel()))
    assert not bool(mask[:, 2].any()) and bool((free64['pre'][:, 2] < 0).all())          # the all-negative channel
    if batch:
        rep.add('mean', mean, t64['mean'], t32['mean'], P)
        rep.add('var', var, t64['var'], t32['var'], P)
        assert float(var[1]) == 0.0                                                      # the constant channel
    rep.add('y', yh, free64['y'], free32['y'], P)
    rep.add('gz', back(gz), t64['gz'], t32['gz'], P)
    rep.add('ggamma', gg, t64['gg'], t32['gg'], P)
    rep.add('gbeta', gb, t64['gb'], t32['gb'], P)
    again = run()
    for u, v in zip((mean, var, y.buf, gz.buf, gg, gb), (again[0], again[1], again[2].buf, again[3].buf, again[4], again[5])):
        assert torch.equal(u, v)
    frozen = run(need_gamma=False, need_beta=False)
    assert frozen[4] is None and frozen[5] is None and torch.equal(frozen[3].buf, gz.buf)
    only_beta = run(need_gamma=False)
    assert only_beta[4] is None and torch.equal(only_beta[5], gb) and torch.equal(only_beta[3].buf, gz.buf)
    rep.check()


def test_bn_ops_on_channel_slices_at_the_capped_shape(device):
    """the 512-slab, capped-grid case once dense and once as channel slices of wider buffers: the pitch changes no bit"""
    from centertrack_amd import ops
    shape = NB.BN_PLAN_SHAPES[0]
    N, H, W, C = shape
    assert NB.bn_plan(*shape)['slabs'] == 512 and NB.bn_plan(*shape)['ew_ragged']
    z, gamma, beta, rm, rv, gy = bn_case(shape)
    g, b = gamma.to(device), beta.to(device)

    def run(zv, gyv, out):
        mean, var, invstd = ops.bn_stats(zv, NB.EPS)
        y = ops.bn_relu_apply(zv, mean, invstd, g, b, out=out)
        gz, gg, gb = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, True)
        return [mean, var, back(y), back(gz), gg, gb]
    dense = run(nhwc_view(z, device), nhwc_view(gy, device), None)
    zv, gyv, out = nhwc_view(z, device, 24, 4), nhwc_view(gy, device, 20, 0), sentinel_view(N, H, W, C, device, 8, 4)
    sliced = run(zv, gyv, out)
    assert untouched(zv) and untouched(gyv) and untouched(out)
    for name, u, v in zip(('mean', 'var', 'y', 'gz', 'ggamma', 'gbeta'), dense, sliced):
        assert torch.equal(u, v), name


@pytest.mark.parametrize('case', NB.UP_PLAN_SHAPES, ids=str)
def test_upsample_add_backward_at_plan_shapes(device, case):
    """``test_upsample_add_backward`` where the slab count comes from the grid target (one kernel per f) and, at f = 2, the
    grid of the input gradient is capped at 2048 workgroups"""
    from centertrack_amd import ops
    shape, f = case
    N, H, W, C = shape
    x, w = NB.randn(51, N, C, H, W).float(), (NB.randn(52, C, 1, 2 * f, 2 * f) * 0.5 / f).float()
    skip, gy = NB.randn(53, N, C, H * f, W * f).float(), NB.randn(54, N, C, H * f, W * f).float()
    xv, gyv = nhwc_view(x, device), nhwc_view(gy, device, C + 4, 0)
    wd = w.to(device)
    ref = {}
    for dt in (torch.float64, torch.float32):
        t = [v.to(dt).clone().requires_grad_() for v in (x, w, skip)]
        ref[dt] = torch.autograd.grad(NB.upsample_add(t[0], t[1], f, t[2]), t[:2], gy.to(dt))
    rep = Report('up plan %s f=%d' % (shape, f))

    def run(**need):
        poison(device, N * H * W * C)
        return ops.upsample_add_backward(xv if need.get('need_w', True) else None, wd, f, gyv, **need)
    gx, gw, gs = run()
    assert gs is gyv
    rep.add('gx', back(gx), ref[torch.float64][0], ref[torch.float32][0], 4 * f * f)
    rep.add('gw', gw, ref[torch.float64][1], ref[torch.float32][1], N * H * W)
    gx2, gw2, _ = run()
    assert torch.equal(gx2.buf, gx.buf) and torch.equal(gw2, gw)
    gx3, none, _ = run(need_w=False)
    assert none is None and torch.equal(gx3.buf, gx.buf)
    none, gw3, _ = run(need_x=False)
    assert none is None and torch.equal(gw3, gw)
    assert untouched(gyv)
    rep.check()


# ---------------------------------------------------------------------------------------------------------------------
# up-sampling backward

@pytest.mark.parametrize('f', [2, 4, 8])
@pytest.mark.parametrize('shape', NB.UP_SHAPES, ids=str)
def test_upsample_add_backward(device, shape, f):
    from centertrack_amd import dcn_v2, dla_up, ops
    N, H, W, C = shape
    x, w = NB.randn(51, N, C, H, W).float(), (NB.randn(52, C, 1, 2 * f, 2 * f) * 0.5 / f).float()
    skip, gy = NB.randn(53, N, C, H * f, W * f).float(), NB.randn(54, N, C, H * f, W * f).float()
    xv, sv, gyv = nhwc_view(x, device), nhwc_view(skip, device, C + 8, 4), nhwc_view(gy, device, C + 4, 0)
    wd = w.to(device)
    ref = {}
    for dt in (torch.float64, torch.float32):
        t = [v.to(dt).requires_grad_() for v in (x, w, skip)]
        y = NB.upsample_add(t[0], t[1], f, t[2])
        ref[dt] = (y.detach(),) + torch.autograd.grad(y, t, gy.to(dt))
    rep = Report('up %s f=%d' % (shape, f))
    out = ops.upsample_add(xv, wd, f, sv, out=ops.View(torch.zeros((N, H * f, W * f, C + 12), device=device), 8, C))
    rep.add('y', back(out), ref[torch.float64][0], ref[torch.float32][0], 4)
    gx, gw, gs = ops.upsample_add_backward(xv, wd, f, gyv)
    assert gs is gyv                                                                      # the skip gradient: no kernel, no copy
    rep.add('gx', back(gx), ref[torch.float64][1], ref[torch.float32][1], 4 * f * f)
    rep.add('gw', gw, ref[torch.float64][2], ref[torch.float32][2], N * H * W)
    gx2, gw2, _ = ops.upsample_add_backward(xv, wd, f, gyv)
    assert torch.equal(gx2.buf, gx.buf) and torch.equal(gw2, gw)
    gx3, none, _ = ops.upsample_add_backward(None, wd, f, gyv, need_w=False)
    assert none is None and torch.equal(gx3.buf, gx.buf)
    none, gw3, _ = ops.upsample_add_backward(xv, wd, f, gyv, need_x=False)
    assert none is None and torch.equal(gw3, gw)
    # through autograd: the same numbers, and the skip gradient is the incoming tensor
    xt, st = xv.buf.clone().requires_grad_(), sv.buf[..., 4:4 + C].contiguous().requires_grad_()
    wt = wd.clone().requires_grad_()
    gyt = gyv.buf[..., :C].contiguous()
    with dcn_v2.trainable():
        o = dla_up._UpsampleAddFunction.apply(xt, st, wt, f)
    assert torch.equal(o, out.buf[..., 8:8 + C])
    agx, ags, agw = torch.autograd.grad(o, (xt, st, wt), gyt)
    assert torch.equal(agx, gx.buf) and torch.equal(agw, gw) and ags.data_ptr() == gyt.data_ptr()
    rep.check()


# ---------------------------------------------------------------------------------------------------------------------
# modules

def record_masks(mod):
    """{state-dict prefix of a DeformConv: ReLU mask of its latest HIP output (NCHW, CPU)}, filled at every forward"""
    from centertrack_amd import dla_up
    masks = {}
    for name, m in mod.named_modules():
        if isinstance(m, dla_up.DeformConv):
            def wrap(x, _f=m.forward_nhwc, _k=(name + '.' if name else '')):
                y = _f(x)
                masks[_k] = (y.detach() > 0).permute(0, 3, 1, 2).cpu()
                return y
            m.forward_nhwc = wrap
    return masks


def reference(fn, sd, inputs, gys, training, dtype, masks=None):
    """one forward (and, with ``gys``, backward) of the construction ``fn(layers, sd, trace, training) -> outputs`` in
    ``dtype`` -> dict(outs, gin, gpar, trace, sd)"""
    sd = NB.cast(sd, dtype, grad=gys is not None)
    xs = [x.to(dtype).clone().requires_grad_(gys is not None) for x in inputs]
    tr = NB.Trace(masks)
    outs = fn(xs, sd, tr, training)
    res = dict(outs=[o.detach() for o in outs], trace=tr, sd=sd)
    if gys is not None:
        names = [k for k in sd if not NB.is_buffer(k)]
        gs = NB.grads(outs, gys, xs + [sd[k] for k in names])
        res['gin'], res['gpar'] = gs[:len(xs)], dict(zip(names, gs[len(xs):]))
    return res


def hip_run(mod, inputs, call, gys, device):
    """forward + backward of the module under ``trainable()`` -> (outputs, input gradients, {name: parameter gradient})"""
    from centertrack_amd import dcn_v2
    xs = [x.to(device).requires_grad_() for x in inputs]
    mod.zero_grad(set_to_none=True)
    with dcn_v2.trainable():
        outs = call(mod, xs)
        sum((o * g.to(device)).sum() for o, g in zip(outs, gys)).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], [x.grad for x in xs], {k: p.grad for k, p in mod.named_parameters()}


def compare(rep, hip, t64, t32, inputs, Ks, training):
    """outputs, input gradients and parameter gradients of one run against the two reference runs.  Under batch statistics a
    ``conv.bias`` gradient is 0 in exact arithmetic and is measured against ``_neck_bwd.bias_norm`` (8 P 2^-24 max|gz| in
    all; a kernel that returned 0 would pass that).  The eval-mode cases, where it is not 0, hold ``conv.bias`` to the
    tensor's maximum like every other gradient: they are what tests this path."""
    outs, gin, gpar = hip
    for i, o in enumerate(outs):
        rep.add('out[%d]' % i, o, t64['outs'][i], t32['outs'][i], Ks['out'])
    for i, g in enumerate(gin):
        assert g is not None, 'input %d got no gradient' % i
        rep.add('grad input[%d]' % i, g, t64['gin'][i], t32['gin'][i], Ks['in'][i])
    assert sorted(gpar) == sorted(t64['gpar'])
    for k in t64['gpar']:
        assert gpar[k] is not None, k + ' got no gradient'
        norm = NB.bias_norm(t64['trace'], k) if training and k.endswith('conv.bias') else None
        rep.add('grad ' + k, gpar[k], t64['gpar'][k], t32['gpar'][k], Ks['par'](k), norm)


def check_masks(title, masks, inputs, fn, sd, training):
    """the free float64 / float32 runs hold every node's HIP mask; designed coordinates stay away from the integers"""
    free64, free32 = (reference(fn, sd, inputs, None, training, dt) for dt in (torch.float64, torch.float32))
    for k, m in masks.items():
        e = err(free32['trace'].y[k], free64['trace'].y[k])
        flipped, near = NB.check_mask(m, free64['trace'].pre[k], e, title + ' ' + k)
        print('%s %s: %d ReLU units flipped, %d within the threshold, of %d' % (title, k, flipped, near, m.numel()))
    return free64, free32


def deform_fn(L, sd, tr, training):
    return [NB.deform(L[0], sd, '', training, tr)]


@pytest.mark.parametrize('offsets', ['designed', 'zero'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape', NB.DEFORM_SHAPES, ids=str)
def test_deform_conv(device, shape, training, offsets):
    from centertrack_amd import dcn_v2, dla_up
    N, H, W, cin, cout = shape
    sd = NB.deform_params(61, cin, cout, offsets=offsets)
    mod = dla_up.DeformConv(cin, cout)
    mod.load_state_dict(sd)
    mod = mod.to(device).train(training)
    masks = record_masks(mod)
    inputs, gys = [NB.randn(62, N, cin, H, W).float()], [NB.randn(63, N, cout, H, W).float()]
    hip = hip_run(mod, inputs, lambda m, xs: [m(xs[0])], gys, device)
    title = 'deform %s %s %s' % (shape, 'train' if training else 'eval', offsets)
    free64, _ = check_masks(title, masks, inputs, deform_fn, sd, training)
    if offsets == 'designed':
        d = NB.min_integer_distance(free64['trace'])
        print('%s: smallest distance of a sample coordinate from an integer %.3f' % (title, d))
        assert d >= 0.1
    t64, t32 = (reference(deform_fn, sd, inputs, gys, training, dt, masks) for dt in (torch.float64, torch.float32))
    rep = Report(title)
    P = N * H * W
    compare(rep, hip, t64, t32, inputs, dict(out=9 * cin, **{'in': [36 * cout]}, par=lambda k: P), training)
    assert len(hip[2]) == 6 and all(g is not None for g in hip[2].values())
    if training:                                                    # one training call: the running statistics moved as torch's
        for k in ('running_mean', 'running_var'):
            rep.add(k, getattr(mod.actf[0], k), t64['sd']['actf.0.' + k], t32['sd']['actf.0.' + k], P)
        assert int(mod.actf[0].num_batches_tracked) == 1
    # without a graph: the same bits, nothing recorded
    x = inputs[0].to(device).requires_grad_()
    with dcn_v2.trainable(), torch.no_grad():
        y1 = mod(x)
    y2 = mod(x)                                                      # trainable() off
    for y in (y1, y2):
        assert torch.equal(y, hip[0][0]) and y.grad_fn is None and not y.requires_grad
    rep.check()


def test_deform_conv_refuses_what_torch_refuses(device):
    from centertrack_amd import dla_up
    from centertrack_amd._lib import CTError
    mod = dla_up.DeformConv(64, 64).to(device).train()
    with pytest.raises(CTError, match='more than one value'):
        mod(torch.zeros(1, 64, 1, 1, device=device))
    mod.eval()
    assert tuple(mod(torch.zeros(1, 64, 1, 1, device=device)).shape) == (1, 64, 1, 1)
    with pytest.raises(CTError, match='fp32'):
        mod(torch.zeros(1, 64, 4, 4, device=device, dtype=torch.float64))


def ida_fn(L, sd, tr, training):
    L = list(L)
    NB.ida(L, sd, '', 0, len(L), training, tr)
    return L[1:]


def ida_call(m, xs):
    layers = list(xs)
    first = layers[0]
    m(layers, 0, len(layers))
    assert layers[0] is first and all(l.shape[2:] == first.shape[2:] and l.shape[1] == 64 for l in layers[1:])   # in place
    return layers[1:]


def ida_Ks(c):
    P = {}
    for i in range(1, len(c['channels'])):
        (h, w), f = c['sizes'][i], c['up_f'][i]
        P['proj_%d' % i], P['up_%d' % i], P['node_%d' % i] = c['N'] * h * w, c['N'] * h * w, c['N'] * h * f * w * f
    return dict(out=9 * c['o'], **{'in': [36 * c['o']] * len(c['channels'])}, par=lambda k: P[k.split('.')[0]])


def test_idaup(device):
    c = NB.IDA
    check_idaup(device, NB.ida_params(71, c['o'], c['channels'], c['up_f']), 'idaup', 0.1)


def idaup_inputs():
    c = NB.IDA
    return [NB.randn(72 + i, c['N'], ch, h, w).float() for i, (ch, (h, w)) in enumerate(zip(c['channels'], c['sizes']))]


def check_idaup(device, sd, title, min_distance):
    """one training call of the IDAUp of ``_neck_bwd.IDA`` under the state dict ``sd`` (tests/test_hip_ckpt_weights.py brings
    its own), no sample coordinate of the float64 run closer than ``min_distance`` to an integer -> the Report's rows"""
    from centertrack_amd import dla_up
    c = NB.IDA
    mod = dla_up.IDAUp(c['o'], c['channels'], c['up_f'])
    mod.load_state_dict(sd)
    mod = mod.to(device).train()
    masks = record_masks(mod)
    inputs = idaup_inputs()
    H0, W0 = c['sizes'][0]
    gys = [(NB.randn(76 + i, c['N'], c['o'], H0, W0) / (c['N'] * H0 * W0) ** 0.5).float() for i in range(2)]
    hip = hip_run(mod, inputs, ida_call, gys, device)
    free64, _ = check_masks(title, masks, inputs, ida_fn, sd, True)
    assert NB.min_integer_distance(free64['trace']) >= min_distance
    t64, t32 = (reference(ida_fn, sd, inputs, gys, True, dt, masks) for dt in (torch.float64, torch.float32))
    rep = Report(title)
    compare(rep, hip, t64, t32, inputs, ida_Ks(c), True)
    for k in sd:                                                     # one training call: the running statistics moved as torch's
        if k.endswith(('running_mean', 'running_var')):
            rep.add(k, mod.state_dict()[k], t64['sd'][k], t32['sd'][k], ida_Ks(c)['par'](k))
    rep.check()
    return dict(rows=rep.rows, gpar=hip[2], t64=t64, trace=free64['trace'])


def test_idaup_three_sgd_steps(device):
    """three SGD steps of the HIP module, the float64 and the float32 construction from one start; each reference step uses
    the ReLU masks of the HIP forward of that step.  Two parameter groups: the offset weights (values of order 0.002,
    gradients of order 10) at lr 5e-5 so that the designed sample coordinates stay 0.1 away from the integers, every other
    parameter at lr 5e-3; every tensor but ``conv.bias`` (whose gradient batch statistics cancel) then moves by more than
    5e-4 of its maximum, a hundred times the bound"""
    from centertrack_amd import dla_up
    c = NB.IDA

    def lr(k):
        return 5e-5 if k.endswith('conv_offset_mask.weight') else 5e-3
    sd0 = NB.ida_params(81, c['o'], c['channels'], c['up_f'])
    mod = dla_up.IDAUp(c['o'], c['channels'], c['up_f'])
    mod.load_state_dict(sd0)
    mod = mod.to(device).train()
    masks = record_masks(mod)
    opt = torch.optim.SGD([dict(params=[p], lr=lr(k)) for k, p in mod.named_parameters()], lr=5e-3)
    H0, W0 = c['sizes'][0]
    sds = {torch.float64: NB.cast(sd0, torch.float64), torch.float32: NB.cast(sd0, torch.float32)}
    for step in range(3):
        inputs = [NB.randn(90 + 10 * step + i, c['N'], ch, h, w).float()
                  for i, (ch, (h, w)) in enumerate(zip(c['channels'], c['sizes']))]
        gys = [(NB.randn(95 + 10 * step + i, c['N'], c['o'], H0, W0) / (c['N'] * H0 * W0) ** 0.5).float() for i in range(2)]
        hip_run(mod, inputs, ida_call, gys, device)
        opt.step()
        for dt in sds:
            r = reference(ida_fn, sds[dt], inputs, gys, True, dt, dict(masks))
            if dt == torch.float64:
                assert NB.min_integer_distance(r['trace']) >= 0.1
            nxt = r['sd']
            for k, g in r['gpar'].items():
                nxt[k] = (nxt[k].detach() - lr(k) * g)
            sds[dt] = nxt
    rep = Report('idaup sgd')
    Ks = ida_Ks(c)
    got = mod.state_dict()
    moved = {}
    for k in sd0:
        if k.endswith('num_batches_tracked'):
            assert int(got[k]) == 3 == int(sds[torch.float64][k])
            continue
        rep.add(k, got[k], sds[torch.float64][k], sds[torch.float32][k], Ks['par'](k))
        moved[k] = err(sd0[k], sds[torch.float64][k])
    print('idaup sgd: moved by (of the maximum) %s' % {k: '%.1e' % v for k, v in moved.items()})
    assert all(v > 5e-4 for k, v in moved.items() if not k.endswith('conv.bias'))
    rep.check()


def test_idaup_agrees_with_the_inference_plan(device):
    """the ``ida_up.*`` tensors of a DLASegHIP in the new IDAUp, eval mode, fed the three ``dla_up`` outputs of a 1 x 128 x 160
    plan: the plan's feature map to 1e-4 of its maximum (the two paths fold the BatchNorm differently)"""
    from centertrack_amd import dla_up, weights as W
    from centertrack_amd.model import DLASegHIP
    heads = W.MOT_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=23)
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    model = model.to(device)
    x, pre, hm = W.synthetic_inputs(1, 128, 160, seed=23)
    model(x.to(device), pre.to(device), hm.to(device))
    torch.cuda.synchronize()
    plan = model.get_plan(1, 128, 160, True, True, False)
    layers = [plan['dcn_layers'][n].to_nchw().contiguous() for n in
              ('dla_up.ida_2.node_3', 'dla_up.ida_1.node_2', 'dla_up.ida_0.node_1')]
    want = plan['feat'].to_nchw().clone()
    ida = dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4])
    ida.load_state_dict({k[len('ida_up.'):]: v for k, v in sd.items() if k.startswith('ida_up.')})
    ida = ida.to(device).eval()
    ida(layers, 0, 3)
    e = err(layers[2].cpu(), want.cpu().double())
    print('idaup against the inference plan: err %.2e' % e)
    assert e <= 1e-4


def dlaup_fn(L, sd, tr, training):
    return NB.dlaup([None, None] + list(L), sd, '', NB.DLAUP['startp'], training, tr)[:3]


def dlaup_call(m, xs):
    outs = m([None, None] + list(xs))
    assert isinstance(outs, list) and len(outs) == 4 and outs[3].shape == xs[3].shape
    return outs[:3]


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_dlaup(device, training):
    from centertrack_amd import dla_up
    c = NB.DLAUP
    sd = NB.dlaup_params(101, c['channels'], c['scales'])
    mod = dla_up.DLAUp(c['startp'], c['channels'], c['scales'])
    mod.load_state_dict(sd)
    mod = mod.to(device).train(training)
    masks = record_masks(mod)
    inputs = [NB.randn(102 + i, c['N'], ch, h, w).float() for i, (ch, (h, w)) in enumerate(zip(c['channels'], c['sizes']))]
    chans = [64, 128, 256]
    gys = [(NB.randn(110 + i, c['N'], chans[i], *c['sizes'][i]) / (c['sizes'][i][0] * c['sizes'][i][1]) ** 0.5).float() for i in range(3)]
    hip = hip_run(mod, inputs, dlaup_call, gys, device)
    title = 'dlaup %s' % ('train' if training else 'eval')
    free64, _ = check_masks(title, masks, inputs, dlaup_fn, sd, training)
    assert NB.min_integer_distance(free64['trace']) >= 0.1
    t64, t32 = (reference(dlaup_fn, sd, inputs, gys, training, dt, masks) for dt in (torch.float64, torch.float32))
    # K per parameter: the pixels of the map its node runs on
    P = {}
    for i, o, inc, up_f in NB.dlaup_structure(c['channels'], c['scales']):
        sizes = c['sizes'][-len(inc):]
        for k in range(1, len(inc)):
            (h, w), f = (sizes[0][0] // up_f[k], sizes[0][1] // up_f[k]), up_f[k]
            P['ida_%d.proj_%d' % (i, k)] = P['ida_%d.up_%d' % (i, k)] = c['N'] * h * w
            P['ida_%d.node_%d' % (i, k)] = c['N'] * h * f * w * f

    def par(k):
        return P['.'.join(k.split('.')[:2])]
    rep = Report(title)
    compare(rep, hip, t64, t32, inputs, dict(out=9 * 64, **{'in': [36 * 64] * 4}, par=par), training)
    rep.check()
