"""GPU: the trainable backbone (centertrack_amd/csrc/backbone_bwd.hip, centertrack_amd/csrc/bn_train.hip, centertrack_amd/dla_base.py) against float64 torch
autograd on the CPU of the restated reference construction (tests/_backbone_bwd.py).  Error measure and bound are the project's
(tests/_dcn_bwd.py): ``err`` relative to the tensor's maximum, ``bound(e32, K) = min(1e-3, 4 max(e32, 2^-23 sqrt(K)))`` with e32
the float32 CPU run of the same construction.  K = 4 Cout for the stride-2 input gradient (the terms of one element: at most
four taps of Cout products), N*Ho*Wo for its weight gradient, N*H*W for the BatchNorm gradients and for every parameter
gradient of a module (the pixels of the map its unit writes); for a forward map the fan-in of the unit that writes it, 9 Cin
for a 3x3 unit and Cin for the 1x1 conv of a ``Root`` (``_backbone_bwd.output_K``); for an input gradient the terms of one
element in the unit that reads the input: 9 Cout, 4 Cout behind a stride-2 unit, Cout behind a 1x1 unit, 49 * 16 behind a stem, 1
for a block's residual input (``_backbone_bwd.input_K``, which says why).

Gradient truths take every ReLU mask and every pool selection from the HIP forward's own fp32 maps
(``centertrack_amd.dla_base.trace``); ``_backbone_bwd.check_tape`` holds those masks and selections against the free float64
run: they may differ only where the deciding values lie within 64 e32 of each other (of 0 for a mask), on at most 0.1 % of a
map (tests/test_backbone_backward_cpu.py holds the float32 reference itself to that cap for the same seeds).  The backbone's
convolutions have no bias, so under batch statistics no parameter gradient is 0 in exact arithmetic; a parameter nothing
reads (the ``project`` of a two-level ``Tree``, whose result the reference drops) gets no gradient at all, here and there.

The op tests run twice: at toy shapes (``S2_SHAPES``, ``BN_SHAPES``, ``POOL_SHAPES``), where every slab count sits at its pixel
limit, and at ``S2_PLAN_SHAPES`` / ``BN_PLAN_SHAPES`` / ``POOL_PLAN_SHAPES``, the smallest shapes that reach what production training
and the API reach beyond that (``_backbone_bwd.S2_REGIMES`` / ``POOL_REGIMES``, ``_neck_bwd.BN_REGIMES``;
tests/test_backbone_backward_cpu.py holds the lists against them).

Measured on an MI355X (largest error / its bound per group): see DESIGN.md section 13."""
import pytest
import torch
import torch.nn.functional as F

import _backbone_bwd as BB
from _backbone_bwd import Report, err

pytestmark = pytest.mark.gpu


def nhwc_view(t, dev, ld=None, c0=0):
    """NCHW CPU tensor -> NHWC view on the device, as channels c0 .. c0 + C of a buffer of pitch ``ld`` filled with 7"""
    from centertrack_amd import ops
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, ld or C), 7.0, dtype=torch.float32)
    buf[..., c0:c0 + C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(dev), c0, C)


def back(v):
    return v.to_nchw().cpu()


def untouched(v):
    """the channels of the buffer outside the view still hold the fill value"""
    rest = torch.ones(v.ld, dtype=torch.bool)
    rest[v.c0:v.c0 + v.C] = False
    return bool((v.buf.cpu()[..., rest] == 7.0).all())


def sentinel_view(N, H, W, C, dev, c0=4, tail=4):
    """a caller-owned output view, channels c0 .. c0 + C of a wider buffer: NaN where the kernel has to write, 7 in the padding"""
    from centertrack_amd import ops
    buf = torch.full((N, H, W, c0 + C + tail), 7.0, device=dev)
    buf[..., c0:c0 + C] = float('nan')
    return ops.View(buf, c0, C)


def poison(dev, *numels):
    """An output the wrapper allocates itself comes from torch's caching allocator, which may hand back the block an earlier
    run of the same case wrote.  Blocks of these sizes are filled with NaN and freed first (stream-ordered), so that an
    element the kernel skips is seen by the comparison that follows."""
    blocks = [torch.full((n,), float('nan'), device=dev) for n in numels]
    del blocks


# ---------------------------------------------------------------------------------------------------------------------
# the stride-2 convolution

s2_case = BB.s2_case


@pytest.mark.parametrize('shape', BB.S2_SHAPES, ids=str)
def test_conv_s2_backward(device, shape):
    from centertrack_amd import ops
    N, H, W, Cin, Cout = shape
    x, w, gy, ref = s2_case(shape)
    xv, gyv, wd = nhwc_view(x, device), nhwc_view(gy, device), w.to(device)
    gx, gw = ops.conv_s2_backward(xv, gyv, wd)
    rep = Report('conv s2 %s' % (shape,))
    rep.add('gx', back(gx), ref[torch.float64][0], ref[torch.float32][0], 4 * Cout)
    rep.add('gw', gw, ref[torch.float64][1], ref[torch.float32][1], N * (H // 2) * (W // 2))
    # each output alone, and a second run: the same bits
    gx1, none = ops.conv_s2_backward(xv, gyv, wd, need_w=False)
    assert none is None and torch.equal(gx1.buf, gx.buf)
    none, gw1 = ops.conv_s2_backward(xv, gyv, need_x=False)
    assert none is None and torch.equal(gw1, gw)
    gx2, gw2 = ops.conv_s2_backward(xv, gyv, wd)
    assert torch.equal(gx2.buf, gx.buf) and torch.equal(gw2, gw)
    assert ops.conv_s2_backward(xv, gyv, wd, need_x=False, need_w=False) == (None, None)
    rep.check()


def test_conv_s2_backward_on_channel_slices(device):
    """x, gy and gx as channel slices of wider buffers; the neighbouring channels stay untouched"""
    from centertrack_amd import ops
    shape = (2, 6, 10, 16, 32)
    N, H, W, Cin, Cout = shape
    x, w, gy, ref = s2_case(shape)
    xv, gyv, wd = nhwc_view(x, device, 48, 16), nhwc_view(gy, device, 40, 4), w.to(device)
    gxv = ops.View(torch.full((N, H, W, 36), 7.0, device=device), 8, Cin)
    gx, gw = ops.conv_s2_backward(xv, gyv, wd, gx=gxv)
    assert gx is gxv and untouched(gxv) and untouched(xv) and untouched(gyv)
    dense = ops.conv_s2_backward(nhwc_view(x, device), nhwc_view(gy, device), wd)
    assert torch.equal(back(gx), back(dense[0])) and torch.equal(gw, dense[1])                     # the pitch changes no bit
    rep = Report('conv s2 slices')
    rep.add('gx', back(gx), ref[torch.float64][0], ref[torch.float32][0], 4 * Cout)
    rep.add('gw', gw, ref[torch.float64][1], ref[torch.float32][1], N * (H // 2) * (W // 2))
    rep.check()


@pytest.mark.parametrize('shape', BB.S2_PLAN_SHAPES, ids=str)
def test_conv_s2_backward_at_plan_shapes(device, shape):
    """``test_conv_s2_backward`` at the plans and channel edges ``_backbone_bwd.S2_PLAN_SHAPES`` names: a slab count from the
    grid target with idle waves and an idle slab, 36 steps per wave, Cin 48 / Cout 80, one tile with its halo outside the map;
    gx goes into a caller-owned view pre-filled with NaN"""
    from centertrack_amd import ops
    N, H, W, Cin, Cout = shape
    x, w, gy, ref = s2_case(shape)
    xv, gyv, wd = nhwc_view(x, device), nhwc_view(gy, device), w.to(device)
    nw = Cout * Cin * 9

    def run(**kw):
        gxv = sentinel_view(N, H, W, Cin, device) if kw.get('need_x', True) else None
        poison(device, nw, nw)                                            # the packed weight and gw
        gx, gw = ops.conv_s2_backward(xv, gyv, wd, gx=gxv, **kw)
        assert gx is gxv and (gxv is None or untouched(gxv))
        return gx, gw
    gx, gw = run()
    rep = Report('conv s2 plan %s' % (shape,))
    rep.add('gx', back(gx), ref[torch.float64][0], ref[torch.float32][0], 4 * Cout)
    rep.add('gw', gw, ref[torch.float64][1], ref[torch.float32][1], N * (H // 2) * (W // 2))
    gx1, none = run(need_w=False)
    assert none is None and torch.equal(gx1.buf, gx.buf)
    none, gw1 = run(need_x=False)
    assert none is None and torch.equal(gw1, gw)
    gx2, gw2 = run()
    assert torch.equal(gx2.buf, gx.buf) and torch.equal(gw2, gw)
    rep.check()


def test_conv_s2_backward_on_channel_slices_at_a_plan_shape(device):
    """the 29-slab case once dense and once with x, gy and gx as channel slices of wider buffers: the pitch changes no bit"""
    from centertrack_amd import ops
    shape = BB.S2_PLAN_SHAPES[0]
    N, H, W, Cin, Cout = shape
    assert BB.s2_plan(*shape)['idle_slabs'] == 1
    x, w, gy, ref = s2_case(shape)
    wd = w.to(device)
    dense = ops.conv_s2_backward(nhwc_view(x, device), nhwc_view(gy, device), wd)
    xv, gyv, gxv = nhwc_view(x, device, Cin + 32, 16), nhwc_view(gy, device, Cout + 8, 4), sentinel_view(N, H, W, Cin, device, 8, 12)
    gx, gw = ops.conv_s2_backward(xv, gyv, wd, gx=gxv)
    assert gx is gxv and untouched(gxv) and untouched(xv) and untouched(gyv)
    assert torch.equal(back(gx), back(dense[0])) and torch.equal(gw, dense[1])


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm (+ residual) (+ ReLU)

bn_case = BB.bn_case


def bn_reference(case, dtype, batch, relu, residual, mask=None):
    z, gamma, beta, rm, rv, gy, res = (t.to(dtype) for t in case)
    z, gamma, beta, res = (t.clone().requires_grad_() for t in (z, gamma, beta, res))
    pre = F.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, batch, BB.MOMENTUM, BB.EPS)
    if residual:
        pre = pre + res
    y = pre if not relu else torch.relu(pre) if mask is None else pre * mask.to(dtype)
    gz, gg, gb, gr = torch.autograd.grad(y, (z, gamma, beta, res), gy, allow_unused=True)
    return dict(pre=pre.detach(), y=y.detach(), gz=gz, gg=gg, gb=gb, gr=gr)


@pytest.mark.parametrize('batch', [True, False], ids=['batch-stats', 'running-stats'])
@pytest.mark.parametrize('residual', [True, False], ids=['residual', 'no-residual'])
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'no-relu'])
@pytest.mark.parametrize('shape', BB.BN_SHAPES, ids=str)
def test_bn_act_ops(device, shape, relu, residual, batch):
    from centertrack_amd import ops
    N, H, W, C = shape
    P = N * H * W
    case = bn_case(shape)
    z, gamma, beta, rm, rv, gy, res = case
    sliced = C == 8                                     # the 8-channel case is a channel slice of a 16-wide buffer
    zv = nhwc_view(z, device, 16 if sliced else None, 4 if sliced else 0)
    gyv = nhwc_view(gy, device, 16 if sliced else None, 8 if sliced else 0)
    rv_ = nhwc_view(res, device, 24 if sliced else None, 12 if sliced else 0) if residual else None
    g, b = gamma.to(device), beta.to(device)
    rep = Report('bn-act %s %s %s %s' % (shape, 'relu' if relu else 'linear', 'res' if residual else 'nores', 'batch' if batch else 'running'))
    if batch:
        mean, var, invstd = ops.bn_stats(zv, BB.EPS)
    else:
        mean, var = rm.to(device), rv.to(device)
        invstd = torch.rsqrt(var + BB.EPS)

    def run(**need):
        y = ops.bn_act_apply(zv, mean, invstd, g, b, res=rv_, relu=relu)
        return (y,) + ops.bn_act_backward(zv, gyv, mean, invstd, g, b, batch, res=rv_, relu=relu, need_res=residual, **need)
    y, gz, gr, gg, gb = run()
    yh = back(y)
    mask = yh > 0
    free64, free32 = (bn_reference(case, dt, batch, relu, residual) for dt in (torch.float64, torch.float32))
    t64, t32 = (bn_reference(case, dt, batch, relu, residual, mask) for dt in (torch.float64, torch.float32))
    if relu:
        flipped, near = BB.check_mask(mask, free64['pre'], err(free32['y'], free64['y']), rep.title)
        print('%s: %d ReLU units flipped, %d within the threshold, of %d' % (rep.title, flipped, near, mask.numel()))
        assert not bool(mask[:, 2].any()) and bool((free64['pre'][:, 2] < 0).all())          # the all-negative channel
    rep.add('y', yh, free64['y'], free32['y'], P)
    rep.add('gz', back(gz), t64['gz'], t32['gz'], P)
    rep.add('ggamma', gg, t64['gg'], t32['gg'], P)
    rep.add('gbeta', gb, t64['gb'], t32['gb'], P)
    if residual:
        rep.add('gres', back(gr), t64['gr'], t32['gr'], P)
        assert torch.equal(back(gr), torch.where(mask, gy, torch.zeros_like(gy)) if relu else gy)   # a pure selection
    else:
        assert gr is None
    # two runs are bitwise equal; with outputs left out what remains is unchanged bit for bit
    again = run()
    for u, v in zip((y, gz, gr, gg, gb), again):
        assert u is None and v is None or torch.equal(getattr(u, 'buf', u), getattr(v, 'buf', v))
    frozen = run(need_gamma=False, need_beta=False)
    assert frozen[3] is None and frozen[4] is None and torch.equal(frozen[1].buf, gz.buf)
    only = run(need_z=False, need_gamma=False)
    assert only[1] is None and only[3] is None and torch.equal(only[4], gb)
    if relu and not residual:                           # the neck's kernels, bit for bit
        y0 = ops.bn_relu_apply(zv, mean, invstd, g, b)
        gz0, gg0, gb0 = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, batch)
        assert torch.equal(y0.buf, y.buf) and torch.equal(gz0.buf, gz.buf) and torch.equal(gg0, gg) and torch.equal(gb0, gb)
    if sliced:
        assert untouched(zv) and untouched(gyv)
    rep.check()


PLAN_MODES = {'relu-res': (True, True, True), 'relu': (True, False, True), 'linear-res': (False, True, True),
              'relu-res-running': (True, True, False)}                    # (relu, residual, batch statistics)


@pytest.mark.parametrize('mode', list(PLAN_MODES))
@pytest.mark.parametrize('shape', BB.BN_PLAN_SHAPES, ids=str)
def test_bn_act_ops_at_plan_shapes(device, shape, mode):
    """``test_bn_act_ops`` where the slab count comes from the grid target and the element-wise grids are capped at 2048
    workgroups (``_neck_bwd.BN_PLAN_SHAPES``); y goes into a caller-owned view pre-filled with NaN"""
    from centertrack_amd import ops
    relu, residual, batch = PLAN_MODES[mode]
    N, H, W, C = shape
    P = N * H * W
    case = bn_case(shape)
    z, gamma, beta, rm, rv, gy, res = case
    zv, gyv = nhwc_view(z, device), nhwc_view(gy, device)
    rv_ = nhwc_view(res, device) if residual else None
    g, b = gamma.to(device), beta.to(device)
    rep = Report('bn-act plan %s %s' % (shape, mode))
    if batch:
        mean, var, invstd = ops.bn_stats(zv, BB.EPS)
    else:
        mean, var = rm.to(device), rv.to(device)
        invstd = torch.rsqrt(var + BB.EPS)

    def run(**need):
        out = sentinel_view(N, H, W, C, device)
        y = ops.bn_act_apply(zv, mean, invstd, g, b, res=rv_, relu=relu, out=out)
        assert y is out and untouched(out)
        poison(device, P * C, P * C)                                      # gz and gres
        return (y,) + ops.bn_act_backward(zv, gyv, mean, invstd, g, b, batch, res=rv_, relu=relu, need_res=residual, **need)
    y, gz, gr, gg, gb = run()
    yh = back(y)
    mask = yh > 0
    free64, free32 = (bn_reference(case, dt, batch, relu, residual) for dt in (torch.float64, torch.float32))
    t64, t32 = (bn_reference(case, dt, batch, relu, residual, mask) for dt in (torch.float64, torch.float32))
    if relu:
        flipped, near = BB.check_mask(mask, free64['pre'], err(free32['y'], free64['y']), rep.title)
        print('%s: %d ReLU units flipped, %d within the threshold, of %d' % (rep.title, flipped, near, mask.numel()))
    rep.add('y', yh, free64['y'], free32['y'], P)
    rep.add('gz', back(gz), t64['gz'], t32['gz'], P)
    rep.add('ggamma', gg, t64['gg'], t32['gg'], P)
    rep.add('gbeta', gb, t64['gb'], t32['gb'], P)
    if residual:
        rep.add('gres', back(gr), t64['gr'], t32['gr'], P)
        assert torch.equal(back(gr), torch.where(mask, gy, torch.zeros_like(gy)) if relu else gy)   # a pure selection
    else:
        assert gr is None
    again = run()
    for u, v in zip((y, gz, gr, gg, gb), again):
        assert u is None and v is None or torch.equal(getattr(u, 'buf', u), getattr(v, 'buf', v))
    frozen = run(need_gamma=False, need_beta=False)
    assert frozen[3] is None and frozen[4] is None and torch.equal(frozen[1].buf, gz.buf)
    assert gr is None or torch.equal(frozen[2].buf, gr.buf)
    only = run(need_z=False, need_gamma=False)
    assert only[1] is None and only[3] is None and torch.equal(only[4], gb) and (gr is None or torch.equal(only[2].buf, gr.buf))
    if relu and not residual:                           # the neck's kernels, bit for bit
        y0 = ops.bn_relu_apply(zv, mean, invstd, g, b)
        gz0, gg0, gb0 = ops.bn_relu_backward(zv, gyv, mean, invstd, g, b, batch)
        assert torch.equal(y0.buf, y.buf[..., y.c0:y.c0 + C]) and torch.equal(gz0.buf, gz.buf)
        assert torch.equal(gg0, gg) and torch.equal(gb0, gb)
    rep.check()


def test_bn_act_ops_on_channel_slices_at_the_capped_shape(device):
    """the 512-slab, capped-grid case with a residual once dense and once as channel slices of wider buffers: the pitch
    changes no bit"""
    from centertrack_amd import ops
    shape = BB.BN_PLAN_SHAPES[0]
    N, H, W, C = shape
    assert BB.bn_plan(*shape)['slabs'] == 512 and BB.bn_plan(*shape)['ew_ragged']
    z, gamma, beta, rm, rv, gy, res = bn_case(shape)
    g, b = gamma.to(device), beta.to(device)

    def run(zv, gyv, rsv, out):
        mean, var, invstd = ops.bn_stats(zv, BB.EPS)
        y = ops.bn_act_apply(zv, mean, invstd, g, b, res=rsv, relu=True, out=out)
        gz, gr, gg, gb = ops.bn_act_backward(zv, gyv, mean, invstd, g, b, True, res=rsv, relu=True, need_res=True)
        return [back(y), back(gz), back(gr), gg, gb]
    dense = run(nhwc_view(z, device), nhwc_view(gy, device), nhwc_view(res, device), None)
    views = nhwc_view(z, device, 24, 4), nhwc_view(gy, device, 20, 0), nhwc_view(res, device, 32, 12)
    out = sentinel_view(N, H, W, C, device, 8, 4)
    sliced = run(*views, out)
    assert untouched(out) and all(untouched(v) for v in views)
    for name, u, v in zip(('y', 'gz', 'gres', 'ggamma', 'gbeta'), dense, sliced):
        assert torch.equal(u, v), name


# ---------------------------------------------------------------------------------------------------------------------
# max-pool backward

tie_input = BB.tie_input


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'add'])
@pytest.mark.parametrize('shape', BB.POOL_SHAPES, ids=str)
def test_maxpool_backward(device, shape, with_add):
    from centertrack_amd import ops
    N, H, W, C = shape
    x = tie_input(41, N, C, H, W)
    assert BB.tie_fraction(x) >= 0.3
    gy, add = BB.randn(42, N, C, H // 2, W // 2).float(), BB.randn(43, N, C, H, W).float()
    xt = x.clone().requires_grad_()
    plain, = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, gy)
    want = plain + add if with_add else plain                            # one fp32 addition per element, here and there
    sliced = C == 8
    xv = nhwc_view(x, device, 16 if sliced else None, 4 if sliced else 0)
    gyv = nhwc_view(gy, device, 24 if sliced else None, 8 if sliced else 0)
    addv = nhwc_view(add, device, C + 4, 4) if with_add else None
    out = ops.View(torch.full((N, H, W, C + 8), 7.0, device=device), 4, C)
    gx = ops.maxpool2x2_backward(xv, gyv, add=addv, out=out)
    assert gx is out and untouched(out)
    assert torch.equal(back(gx), want)                                   # bitwise: a pure selection
    assert torch.equal(ops.maxpool2x2_backward(xv, gyv, add=addv).buf, out.buf[..., 4:4 + C])
    assert torch.equal(back(ops.maxpool2x2(xv)), F.max_pool2d(x, 2, 2))
    # through autograd
    from centertrack_amd import dcn_v2, dla_base
    xd = xv.buf[..., xv.c0:xv.c0 + C].contiguous().requires_grad_()
    with dcn_v2.trainable():
        y = dla_base._MaxPoolFunction.apply(xd)
    g, = torch.autograd.grad(y, xd, gyv.buf[..., gyv.c0:gyv.c0 + C].contiguous())
    assert torch.equal(g.permute(0, 3, 1, 2).cpu(), plain)


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'add'])
@pytest.mark.parametrize('shape', BB.POOL_PLAN_SHAPES, ids=str)
def test_maxpool_backward_with_a_capped_grid(device, shape, with_add):
    """549 120 windows x channel quads on 2048 workgroups: the grid-stride loop runs a second, ragged round.  torch's result
    bit for bit, into a caller-owned view pre-filled with NaN"""
    from centertrack_amd import ops
    N, H, W, C = shape
    assert BB.pool_plan(*shape)['ew_ragged']
    x = tie_input(41, N, C, H, W)
    assert BB.tie_fraction(x) >= 0.3
    gy, add = BB.randn(42, N, C, H // 2, W // 2).float(), BB.randn(43, N, C, H, W).float()
    xt = x.clone().requires_grad_()
    plain, = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, gy)
    want = plain + add if with_add else plain                            # one fp32 addition per element, here and there
    xv, gyv = nhwc_view(x, device), nhwc_view(gy, device, C + 4, 4)
    addv = nhwc_view(add, device, C + 4, 0) if with_add else None
    out = sentinel_view(N, H, W, C, device)
    gx = ops.maxpool2x2_backward(xv, gyv, add=addv, out=out)
    assert gx is out and untouched(out) and untouched(gyv)
    assert torch.equal(back(gx), want)                                   # bitwise: a pure selection
    out2 = sentinel_view(N, H, W, C, device, 0, 0)
    assert torch.equal(ops.maxpool2x2_backward(xv, gyv, add=addv, out=out2).buf, out.buf[..., 4:4 + C])


# ---------------------------------------------------------------------------------------------------------------------
# modules

STEMS = ('base_layer.', 'pre_img_layer.', 'pre_hm_layer.')

def hip_run(name, mod, inputs, device, gy_seed):
    """forward + backward of the module under ``trainable()`` with the trace on -> (outputs, input gradients, {name: parameter
    gradient}, the forward's maps in call order (NCHW, CPU), the output gradients)"""
    from centertrack_amd import dcn_v2, dla_base
    xs = [x.to(device).requires_grad_() for x in inputs]
    mod.zero_grad(set_to_none=True)
    dla_base.trace = []
    try:
        with dcn_v2.trainable():
            outs = BB.module_call(name, mod, xs)
            gys = BB.output_gradients(outs, gy_seed)
            sum((o * g.to(device)).sum() for o, g in zip(outs, gys)).backward()
        torch.cuda.synchronize()
        maps = [t.permute(0, 3, 1, 2).cpu().contiguous() for t in dla_base.trace]
    finally:
        dla_base.trace = None
    return [o.detach() for o in outs], [x.grad for x in xs], {k: p.grad for k, p in mod.named_parameters()}, maps, gys


def compare(rep, name, hip, t64, t32, inputs):
    outs, gin, gpar = hip[:3]
    for i, o in enumerate(outs):
        rep.add('out[%d]' % i, o, t64['outs'][i], t32['outs'][i], BB.output_K(name)[i])
    for i, g in enumerate(gin):
        assert g is not None, 'input %d got no gradient' % i
        rep.add('grad input[%d]' % i, g, t64['gin'][i], t32['gin'][i], BB.input_K(name)[i])
    assert sorted(gpar) == sorted(t64['gpar'])
    unread = []
    for k in t64['gpar']:
        if gpar[k] is None:                                              # a parameter nothing reads: no gradient in autograd either
            assert float(t64['gpar'][k].abs().max()) == 0.0, k + ' got no gradient'
            unread.append(k)
            continue
        rep.add('grad ' + k, gpar[k], t64['gpar'][k], t32['gpar'][k], BB.pixels_of(name, k, inputs))
    return unread


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('name', list(BB.MODULES))
def test_modules(device, name, training):
    from centertrack_amd import dla_base
    seed = BB.SEEDS[name]
    sd = BB.random_params(seed, BB.MODULES[name][0](dla_base))
    check_module(device, name, training, sd, seed, '%s %s' % (name, 'train' if training else 'eval'))


def check_module(device, name, training, sd, seed, title):
    """forward, every gradient, the moved running statistics and the bitwise repeat of the module ``name`` of
    ``_backbone_bwd.MODULES`` under the state dict ``sd`` (tests/test_hip_ckpt_weights.py brings its own) -> the Report's rows"""
    from centertrack_amd import dcn_v2, dla_base
    mod = BB.MODULES[name][0](dla_base)
    mod.load_state_dict(sd)
    mod = mod.to(device).train(training)
    inputs = BB.module_inputs(name, seed + 1)
    hip = hip_run(name, mod, inputs, device, seed + 20)
    maps, gys = hip[3], hip[4]
    free64, free32 = (BB.reference(name, sd, inputs, None, training, dt) for dt in (torch.float64, torch.float32))
    t64, t32 = (BB.reference(name, sd, inputs, gys, training, dt, maps) for dt in (torch.float64, torch.float32))
    flips, wins = BB.check_tape(title, t64['tape'], free64['tape'], free32['tape'])
    print('%s: %d maps, %d ReLU units flipped, %d pool windows differ' % (title, len(maps), flips, wins))
    rep = Report(title)
    unread = compare(rep, name, hip, t64, t32, inputs)
    assert unread == {'tree-2': ['project.0.weight', 'project.1.weight', 'project.1.bias'],
                      'dla34': ['level%d.project.%s' % (lv, k) for lv in (3, 4) for k in ('0.weight', '1.weight', '1.bias')]}.get(name, [])
    # a second run: every output and every gradient of this package's kernels bit for bit.  The three stems are torch modules
    # (out of scope): the vendor library's 7x7 weight gradient is not reproducible from run to run
    # (measured: ``base_layer.0.weight`` differs in the last bits), so the stems' own parameters and the gradients of the
    # images are held to fp32 rounding, 1e-5 of the tensor's maximum, instead
    again = hip_run(name, mod, inputs, device, seed + 20)
    for u, v in zip(hip[0], again[0]):
        assert torch.equal(u, v)
    for k, g in list(hip[2].items()) + [('input[%d]' % i, g) for i, g in enumerate(hip[1])]:
        g2 = again[2][k] if k in again[2] else again[1][int(k[6:-1])]
        if name == 'dla34' and (k.startswith(STEMS) or k.startswith('input')):
            assert err(g2.cpu(), g.cpu().double()) <= 1e-5, k
        else:
            assert g is None and g2 is None or torch.equal(g, g2), k
    if training:                                                        # two training calls: the running statistics moved as torch's
        ref = {}
        for dt in (torch.float64, torch.float32):
            once = BB.reference(name, sd, inputs, None, True, dt)['sd']
            ref[dt] = BB.reference(name, once, inputs, None, True, dt)['sd']
        got = mod.state_dict()
        for k in sd:
            if k.endswith('num_batches_tracked'):
                assert int(got[k]) == 2 == int(ref[torch.float64][k]), k
            elif BB.is_buffer(k):
                rep.add(k, got[k], ref[torch.float64][k], ref[torch.float32][k], BB.pixels_of(name, k, inputs))
    # without a graph: the same bits, nothing recorded
    xs = [x.to(device).requires_grad_() for x in inputs]
    with dcn_v2.trainable(), torch.no_grad():
        y1 = BB.module_call(name, mod, xs)
    y2 = BB.module_call(name, mod, xs)                                  # trainable() off
    for ys in (y1, y2):
        for y, want in zip(ys, hip[0]):
            assert torch.equal(y, want) and y.grad_fn is None and not y.requires_grad
    rep.check()
    return dict(rows=rep.rows, gpar=hip[2], t64=t64, buffers=mod.state_dict())


def test_forward_nhwc_returns_the_same_maps(device):
    from centertrack_amd import dla_base
    mod = dla_base.dla34(pretrained=False, opt=BB.Opt())
    mod.load_state_dict(BB.random_params(BB.SEEDS['dla34'], mod))
    mod = mod.to(device).eval()
    xs = [x.to(device) for x in BB.module_inputs('dla34', BB.SEEDS['dla34'] + 1)]
    nchw, nhwc = mod(*xs), mod.forward_nhwc(*xs)
    assert len(nchw) == 6 and [t.shape[1] for t in nchw] == BB.DLA34['channels']
    for a, b in zip(nchw, nhwc):
        assert torch.equal(a, b.permute(0, 3, 1, 2))


def test_tree_three_sgd_steps(device):
    """three SGD steps of the level-3 ``Tree`` (the 'tree-2' case), the float64 and the float32 construction from one start;
    each reference step uses the ReLU masks and pool selections of the HIP forward of that step.  Two parameter groups
    (``_backbone_bwd.sgd_lr``); every tensor a gradient reaches moves by more than 5e-4 of its maximum, a hundred times the
    bound (tests/test_backbone_backward_cpu.py holds that on the CPU)."""
    from centertrack_amd import dla_base
    name = 'tree-2'
    sd0 = BB.sgd_start()
    mod = BB.MODULES[name][0](dla_base)
    mod.load_state_dict(sd0)
    mod = mod.to(device).train()
    opt = torch.optim.SGD([dict(params=[p], lr=BB.sgd_lr(k, p)) for k, p in mod.named_parameters()], lr=1.0)
    maps = []
    for step in range(BB.SGD_STEPS):
        inputs, gys = BB.sgd_data(step)
        xs = [x.to(device) for x in inputs]
        from centertrack_amd import dcn_v2
        opt.zero_grad(set_to_none=True)
        dla_base.trace = []
        try:
            with dcn_v2.trainable():
                (mod(xs[0]) * gys[0].to(device)).sum().backward()
            maps.append([t.permute(0, 3, 1, 2).cpu().contiguous() for t in dla_base.trace])
        finally:
            dla_base.trace = None
        opt.step()
    (s64, moved), (s32, _) = BB.sgd_trajectory(torch.float64, maps), BB.sgd_trajectory(torch.float32, maps)
    rep = Report('tree sgd')
    got = mod.state_dict()
    P = 2 * 8 * 8
    for k in sd0:
        if k.endswith('num_batches_tracked'):
            assert int(got[k]) == BB.SGD_STEPS == int(s64[k])
            continue
        if k.startswith('project.') and not BB.is_buffer(k):              # read by nobody: it does not move, bit for bit
            assert torch.equal(got[k].cpu(), sd0[k])
            continue
        rep.add(k, got[k], s64[k], s32[k], P)
    print('tree sgd: moved by (of the maximum) %s' % {k: '%.1e' % v for k, v in moved.items()})
    assert all(v > 5e-4 for k, v in moved.items() if not k.startswith('project.'))
    rep.check()


# ---------------------------------------------------------------------------------------------------------------------
# the whole network

def build_chain(sd, device):
    """the reference's DLASeg (dla.py:592-640) from the trainable modules: base -> dla_up -> ida_up -> heads"""
    from centertrack_amd import dla_base, dla_up, heads as HD, weights as W
    net = torch.nn.Module()
    net.base = dla_base.dla34(pretrained=False, opt=BB.Opt())
    net.dla_up = dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8])
    net.ida_up = dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4])
    net.heads = HD.FusedHeads(W.MOT_HEADS)
    for part in ('base', 'dla_up', 'ida_up'):
        getattr(net, part).load_state_dict({k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(part + '.')})
    net.heads.load_state_dict({k: sd[k] for k in net.heads.state_dict()})
    return net.to(device)


def chain_features(net, x, pre_img, pre_hm):
    layers = net.dla_up(net.base(x, pre_img, pre_hm))
    y = [layers[i].clone() for i in range(3)]
    net.ida_up(y, 0, len(y))
    return y[-1]


def test_one_whole_training_step(device):
    """new DLA -> DLAUp -> IDAUp -> FusedHeads -> GenericLoss -> backward() at 2 x 64 x 64: every parameter something reads
    has a finite, non-zero gradient.  Two runs agree bitwise wherever no DCN input gradient (summed with float atomics) lies
    on the way: the loss, the heads and the last node of ``ida_up``; everything behind that node's input gradient agrees to
    fp32 rounding (1e-4 of the tensor's maximum).  Not compared there: the ``conv.bias`` of a ``DeformConv`` behind such a
    gradient -- under batch statistics its gradient is 0 in exact arithmetic, what fp32 leaves of it is
    rounding noise, and two orders of the atomic additions leave two different noises (measured: 1.8 of the tensor's
    maximum)."""
    import _loss_ref as R
    from centertrack_amd import dcn_v2, losses, weights as W
    heads = W.MOT_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=BB.SEEDS['step'])
    net = build_chain(sd, device).train()
    x, pre, hm = (t.to(device) for t in W.synthetic_inputs(2, 64, 64, seed=BB.SEEDS['step']))
    _, batch = R.make_batch(BB.SEEDS['step'] + 1, 2, 16, 16, 8, tuple(heads), 1)
    batch = {k: v.to(device) for k, v in batch.items()}
    crit = losses.GenericLoss(R.Opt(tuple(heads)))

    def step():
        net.zero_grad(set_to_none=True)
        with dcn_v2.trainable():
            tot = crit([net.heads(chain_features(net, x, pre, hm))], batch)[0]
            tot.backward()
        torch.cuda.synchronize()
        return tot.detach().clone(), {k: p.grad for k, p in net.named_parameters()}
    tot, grads = step()
    assert bool(torch.isfinite(tot))
    unread = ['base.level%d.project.%s' % (lv, k) for lv in (3, 4) for k in ('0.weight', '1.weight', '1.bias')]
    for k, g in grads.items():
        if k in unread:
            assert g is None, k
            continue
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k
    assert len(grads) - len(unread) >= 200
    tot2, grads2 = step()
    assert torch.equal(tot, tot2)
    diffs = {}
    for k, g in grads.items():
        if g is None:
            continue
        if k.startswith('heads.') or k.startswith('ida_up.node_2.'):
            assert torch.equal(g, grads2[k]), k
        elif not k.endswith('conv.bias'):
            diffs[k] = err(grads2[k].cpu(), g.cpu().double())
    top = sorted(diffs.items(), key=lambda kv: -kv[1])[:5]
    print('whole step: loss %.6f, largest run-to-run differences behind a DCN input gradient %s' % (
        float(tot), ['%s %.2e' % kv for kv in top]))
    assert top[0][1] <= 1e-4


def test_eval_mode_agrees_with_the_inference_plan(device):
    """the chain holding a DLASegHIP's tensors, eval mode: the plan's feature map (``trunk_only``) to 1e-4 of its maximum
    (the two paths fold the BatchNorm differently), the bar of tests/test_hip_neck_backward.py"""
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    heads = W.MOT_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=23)
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    model = model.to(device)
    x, pre, hm = (t.to(device) for t in W.synthetic_inputs(1, 128, 160, seed=23))
    with torch.no_grad():
        plan = model.get_plan(1, 128, 160, True, True, trunk_only=True)
        model.forward_plan(plan, x, pre, hm)
    torch.cuda.synchronize()
    want = plan['feat'].to_nchw().clone()
    net = build_chain(sd, device).eval()
    got = chain_features(net, x, pre, hm)
    assert got.grad_fn is None
    e = err(got.cpu(), want.cpu().double())
    print('the trainable chain against the inference plan: err %.2e' % e)
    assert e <= 1e-4
