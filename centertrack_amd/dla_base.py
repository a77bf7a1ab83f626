"""The DLA-34 backbone base as trainable drop-in modules: ``BasicBlock``, ``Root``, ``Tree``, ``DLA`` and ``dla34`` of the
reference's ``model/networks/dla.py`` (lines 38-66, 154-316, 333-342), with its constructor signatures, state-dict keys,
buffer names, default initialisation and calling conventions, on the kernels of libcentertrack_hip.so (DESIGN.md section 13,
INTEGRATION.md section A).

Behind the stems every tensor is an NHWC ``[N,H,W,C]`` fp32 tensor; NCHW <-> NHWC conversion happens once per input and once
per returned tensor of the outermost module that is called, and every module also has ``forward_nhwc``.  The unit of the
backbone and of autograd is ``conv (ks 1 | 3, stride 1 | 2, no bias) -> BatchNorm (-> + residual) (-> ReLU)``: ``ct_conv2d``
(the raw ``z``), ``ct_bn_stats`` (training mode only) and ``ct_bn_act_apply``; its backward is ``ct_bn_act_backward``, then
the weight gradient (``ct_conv2d_backward_weight`` / ``ct_conv2d_s2_backward``) and the input gradient (``ct_conv2d`` with the
transposed, flipped weight / ``ct_conv2d_s2_backward``).  ``Tree.downsample`` is ``ct_maxpool2x2``; where a ``Tree`` feeds one
tensor to a stride-2 block and to the pool, the block's first unit returns the pooled map as a second output and its backward
hands the conv's input gradient to ``ct_maxpool2x2_backward`` as ``add``.

The parameters live in real ``nn.Conv2d`` / ``nn.BatchNorm2d`` objects (``load_state_dict``, optimizers and torch's default
initialisation work unchanged) and are packed at every call: no packing is cached.  Statistics follow torch: batch statistics
when, and only when, the BatchNorm is in training mode, and then the running statistics are updated as torch does.  A graph is
recorded only under ``dcn_v2.trainable()`` with autograd enabled; otherwise the same forward runs with nothing saved and
returns the same bits.  CUDA fp32 tensors only: there is no CPU fallback.

The three 7x7 stems (``base_layer``, ``pre_img_layer``, ``pre_hm_layer``) stay ``nn.Sequential(Conv2d, BatchNorm2d, ReLU)``
parameter holders and run as one autograd node on the kernels of DESIGN.md section 14: ``ct_stem_conv_forward`` (the raw
``z`` of every stem present, NCHW planes in, NHWC out), ``ct_bn_stats`` per stem (training mode only) and
``ct_stem_bn_relu_sum`` (BatchNorm, ReLU and the sum in one pass); the backward is ``ct_bn_relu_backward`` per stem on the
incoming gradient itself, then ``ct_stem_conv_backward``.  The images never leave NCHW and nothing behind them is NCHW.

Not covered: a first width other than 16 (such a ``DLA`` keeps the torch stems; NCHW, their sum is converted once);
``Bottleneck`` / ``BottleneckX``; dilation; nothing is ever downloaded."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train, ops
from ._train import BN_MOMENTUM, bn_statistics, need_cuda, recording, saved_mean, to_nchw
from .ops import View

# None = off; a list receives, in call order, the NHWC output of every conv-BN-act unit, of every pool and of every stem
# (ahead of their sum): what a float64 truth needs to take the ReLU masks and pool selections of this forward
trace = None


def _emit(t):
    if trace is not None:
        trace.append(t.detach())


def to_nhwc(x):
    return _train.to_nhwc(x, 'backbone')


def _check_channels(*cs):
    for c in cs:
        if c <= 0 or c % 16:
            raise _lib.CTError('centertrack_amd backbone needs channel counts that are multiples of 16 (got %d)' % c)


# ---------------------------------------------------------------------------------------------------------------------
# conv -> BatchNorm (-> + residual) (-> ReLU)

def _unit_forward(x, conv, bn, res, relu, pool):
    """The unit on the NHWC view ``x`` -> (output view, pooled view of ``x`` or None, what a backward needs)"""
    ks, stride = conv.kernel_size[0], conv.stride[0]
    if x.C != conv.in_channels:
        raise _lib.CTError('Conv2d(%d, %d) of the backbone got %d channels' % (conv.in_channels, conv.out_channels, x.C))
    if stride == 2 and (x.H % 2 or x.W % 2):
        raise _lib.CTError('centertrack_amd backbone: a stride-2 level needs even H and W (got %d x %d)' % (x.H, x.W))
    z = ops.conv2d(x, ops.pack_weight(conv.weight.detach()), conv.out_channels, ks, stride)
    pooled = ops.maxpool2x2(x) if pool else None
    mean, invstd, batch = bn_statistics(bn, z, 'backbone')
    y = ops.bn_act_apply(z, mean, invstd, bn.weight.detach(), _train.bn_beta(batch, bn.bias.detach()), res=res, relu=relu)
    return y, pooled, (z, mean, invstd, batch)


class _ConvBnActFunction(torch.autograd.Function):
    """One unit over ``[N,H,W,C]`` tensors -> ``y`` or, with ``pool``, ``(y, max_pool2d(x, 2, 2))``.  Saved: the input, the raw
    convolution output ``z``, the statistics and the residual; the ReLU mask is recomputed from them with the forward's own
    arithmetic, the pool selection from the input."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, res, conv, bn, relu, pool):
        y, pooled, (z, mean, invstd, batch) = _unit_forward(View(x), conv, bn, None if res is None else View(res), relu, pool)
        # z, mean and invstd are kept on ctx, not through save_for_backward: they are private to this call (z and the batch
        # statistics are allocated here, running statistics are cloned), nobody else holds them, so there is no in-place write
        # for autograd's version check to catch
        ctx.z, ctx.mean, ctx.invstd, ctx.batch = z, saved_mean(mean, batch), invstd, batch
        ctx.relu, ctx.pool, ctx.ks, ctx.stride = relu, pool, conv.kernel_size[0], conv.stride[0]
        ctx.save_for_backward(x, weight, gamma, beta, res)
        ctx.set_materialize_grads(False)
        return (y.buf, pooled.buf) if pool else y.buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gpool=None):
        x, weight, gamma, beta, res = ctx.saved_tensors
        need_x, need_w, need_gamma, need_beta, need_res = ctx.needs_input_grad[:5]
        need_res = need_res and res is not None
        xv = View(x)
        gx = gw = gg = gb = gres = None
        if gy is not None:
            gy = gy.contiguous()
            need_z = need_x or need_w
            # without the ReLU the residual's gradient is the incoming tensor itself: no kernel, no copy
            if isinstance(ctx.batch, _train.SyncedBatch):  # statistics over all ranks: sums -> all-reduce -> apply
                gz, gr, gg, gb = _train.synced_bn_backward([dict(
                    z=ctx.z, gy=View(gy), mean=ctx.mean, invstd=ctx.invstd, gamma=gamma.detach(), beta=beta.detach(),
                    sync=ctx.batch, res=None if res is None else View(res), relu=ctx.relu, need_z=need_z,
                    need_res=need_res and ctx.relu, need_gamma=need_gamma, need_beta=need_beta)])[0]
            else:
                gz, gr, gg, gb = ops.bn_act_backward(ctx.z, View(gy), ctx.mean, ctx.invstd, gamma.detach(), beta.detach(),
                                                     ctx.batch, res=None if res is None else View(res), relu=ctx.relu,
                                                     need_z=need_z, need_res=need_res and ctx.relu, need_gamma=need_gamma,
                                                     need_beta=need_beta)
            if need_res:
                gres = gr.buf if ctx.relu else gy
            if ctx.stride == 2:
                gx, gw = ops.conv_s2_backward(xv, gz, weight.detach(), need_x=need_x, need_w=need_w) if need_z else (None, None)
            else:
                if need_w:
                    gw, _ = ops.conv_backward_weight(xv, gz, ctx.ks, need_bias=False)
                if need_x:
                    gx = ops.conv_backward_input(gz, weight.detach())
        if ctx.pool and gpool is not None and need_x:
            gx = ops.maxpool2x2_backward(xv, View(gpool.contiguous()), add=gx)
        return (gx.buf if gx is not None else None, gw, gg, gb, gres, None, None, None, None)


class _MaxPoolFunction(torch.autograd.Function):
    """``max_pool2d(x, 2, 2)`` over ``[N,H,W,C]`` tensors on its own (a ``Tree`` whose first child is a ``Tree``)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.maxpool2x2(View(x)).buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        return ops.maxpool2x2_backward(View(x), View(gy.contiguous())).buf


def _conv_bn_act(x, conv, bn, res=None, relu=True, pool=False):
    """The unit on ``[N,H,W,C]`` tensors; with ``pool`` -> (y, the 2x2 max-pool of ``x``)"""
    x = x.contiguous()
    res = None if res is None else res.contiguous()
    if recording():
        out = _ConvBnActFunction.apply(x, conv.weight, bn.weight, bn.bias, res, conv, bn, relu, pool)
    else:
        with torch.no_grad():
            y, pooled, _ = _unit_forward(View(x), conv, bn, None if res is None else View(res), relu, pool)
            out = (y.buf, pooled.buf) if pool else y.buf
    for t in (out if pool else (out,)):
        _emit(t)
    return out


def _maxpool(x):
    x = x.contiguous()
    if x.shape[1] % 2 or x.shape[2] % 2:
        raise _lib.CTError('centertrack_amd backbone: the 2x2 max-pool needs even H and W (got %d x %d)' % (x.shape[1], x.shape[2]))
    if recording():
        y = _MaxPoolFunction.apply(x)
    else:
        with torch.no_grad():
            y = ops.maxpool2x2(View(x)).buf
    _emit(y)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the 7x7 stems: sum_s relu(bn_s(conv7x7_s(in_s)))

def _stems_forward(inputs, layers):
    """``inputs`` = (x, pre_img, pre_hm) as contiguous NCHW tensors (None = absent), ``layers`` = their ``nn.Sequential`` ->
    (the NHWC view of the sum, what a backward needs).  With the trace on, every term is emitted ahead of the sum."""
    live = [s for s in range(3) if inputs[s] is not None]
    zs = ops.stem_conv_forward(inputs, [None if layers[s] is None else layers[s][0].weight.detach() for s in range(3)])
    means, invstds, batches = [None] * 3, [None] * 3, [False] * 3
    # (on the synchronised path the stems share one all-gather)
    stats = _train.bn_statistics_many([layers[s][1] if s in live else None for s in range(3)], zs, 'backbone')
    for s in live:
        means[s], invstds[s], batches[s] = stats[s]
    gammas = [layers[s][1].weight.detach() if s in live else None for s in range(3)]
    betas = [_train.bn_beta(batches[s], layers[s][1].bias.detach()) if s in live else None for s in range(3)]
    if trace is not None:
        for s in live:
            _emit(ops.bn_relu_apply(zs[s], means[s], invstds[s], gammas[s], betas[s]).buf)
    y = ops.stem_bn_relu_sum(zs, means, invstds, gammas, betas)
    return y, (zs, means, invstds, batches)


class _StemsFunction(torch.autograd.Function):
    """The three stems and their sum as one node: NCHW images -> the NHWC ``[N,H,W,16]`` sum.  Saved: the inputs, every raw
    convolution output ``z_s`` and the statistics (private to the call, kept on ctx as ``_ConvBnActFunction`` does); the ReLU
    masks are recomputed from them with the forward's own arithmetic.  Since the output is a plain sum, every stem's output
    gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, pre_img, pre_hm, w0, w1, w2, g0, g1, g2, b0, b1, b2, layers):
        inputs = (x, pre_img, pre_hm)
        y, (zs, means, invstds, batches) = _stems_forward(inputs, layers)
        ctx.zs, ctx.invstds, ctx.batches = zs, invstds, batches
        ctx.means = [None if m is None else saved_mean(m, b) for m, b in zip(means, batches)]
        ctx.save_for_backward(x, pre_img, pre_hm, w0, w1, w2, g0, g1, g2, b0, b1, b2)
        return y.buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        inputs, ws, gammas, betas = saved[0:3], saved[3:6], saved[6:9], saved[9:12]
        need = ctx.needs_input_grad
        gyv = View(gy.contiguous())
        gzs, gg, gb = [None] * 3, [None] * 3, [None] * 3
        need_in = [inputs[s] is not None and need[s] for s in range(3)]
        need_w = [inputs[s] is not None and need[3 + s] for s in range(3)]
        synced = [s for s in range(3) if inputs[s] is not None and isinstance(ctx.batches[s], _train.SyncedBatch)]
        if synced:                                     # statistics over all ranks: the stems share one all-reduce
            got = _train.synced_bn_backward([dict(
                z=ctx.zs[s], gy=gyv, mean=ctx.means[s], invstd=ctx.invstds[s], gamma=gammas[s].detach(), beta=betas[s].detach(),
                sync=ctx.batches[s], neck=True, need_z=need_in[s] or need_w[s], need_gamma=need[6 + s], need_beta=need[9 + s])
                for s in synced])
            for s, (gz, _, g, b) in zip(synced, got):
                gzs[s], gg[s], gb[s] = gz, g, b
        for s in range(3):
            if inputs[s] is None or s in synced:
                continue
            gzs[s], gg[s], gb[s] = ops.bn_relu_backward(ctx.zs[s], gyv, ctx.means[s], ctx.invstds[s], gammas[s].detach(),
                                                        betas[s].detach(), ctx.batches[s], need_z=need_in[s] or need_w[s],
                                                        need_gamma=need[6 + s], need_beta=need[9 + s])
        gw, gin = ops.stem_conv_backward(gzs, inputs, [None if w is None else w.detach() for w in ws], need_w=need_w,
                                         need_in=need_in)
        return tuple(gin) + tuple(gw) + tuple(gg) + tuple(gb) + (None,)


def _stems(inputs, layers):
    """The stems on NCHW tensors -> the NHWC ``[N,H,W,16]`` tensor of their sum"""
    inputs = tuple(None if t is None else t.contiguous() for t in inputs)
    if recording():
        # the parameters are read from the modules at every call: three weights, three gammas, three betas
        par = [None if m is None else p(m) for p in (lambda m: m[0].weight, lambda m: m[1].weight, lambda m: m[1].bias)
               for m in layers]
        return _StemsFunction.apply(*(inputs + tuple(par) + (layers,)))
    with torch.no_grad():
        return _stems_forward(inputs, layers)[0].buf


# ---------------------------------------------------------------------------------------------------------------------
# the modules

def _no_dilation(dilation):
    if dilation != 1:
        raise _lib.CTError('centertrack_amd backbone supports dilation 1 only (got %s)' % (dilation,))


class BasicBlock(nn.Module):
    """Reference ``BasicBlock(inplanes, planes, stride=1, dilation=1)``"""

    def __init__(self, inplanes, planes, stride=1, dilation=1):
        super().__init__()
        _no_dilation(dilation)
        if stride not in (1, 2):
            raise _lib.CTError('centertrack_amd BasicBlock supports stride 1 and 2 (got %s)' % (stride,))
        _check_channels(inplanes, planes)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=dilation, bias=False, dilation=dilation)
        self.bn1 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=dilation, bias=False, dilation=dilation)
        self.bn2 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        self.stride = stride

    def first_half(self, x, pool=False):
        return _conv_bn_act(x, self.conv1, self.bn1, relu=True, pool=pool)

    def second_half(self, h, residual):
        return _conv_bn_act(h, self.conv2, self.bn2, res=residual, relu=True)

    def forward_nhwc(self, x, residual=None):
        return self.second_half(self.first_half(x), x if residual is None else residual)

    def forward(self, x, residual=None):
        return to_nchw(self.forward_nhwc(to_nhwc(x), None if residual is None else to_nhwc(residual)))


class Root(nn.Module):
    """Reference ``Root(in_channels, out_channels, kernel_size, residual)``; ``forward(*x)`` concatenates its arguments"""

    def __init__(self, in_channels, out_channels, kernel_size, residual):
        super().__init__()
        if kernel_size != 1:
            raise _lib.CTError('centertrack_amd Root supports root_kernel_size 1 only (got %s)' % (kernel_size,))
        _check_channels(in_channels, out_channels)
        self.conv = nn.Conv2d(in_channels, out_channels, 1, stride=1, bias=False, padding=(kernel_size - 1) // 2)
        self.bn = nn.BatchNorm2d(out_channels, momentum=BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)
        self.residual = residual

    def forward_nhwc(self, *x):
        return _conv_bn_act(torch.cat(x, 3), self.conv, self.bn, res=x[0] if self.residual else None, relu=True)

    def forward(self, *x):
        return to_nchw(self.forward_nhwc(*[to_nhwc(t) for t in x]))


class Tree(nn.Module):
    """Reference ``Tree(levels, block, in_channels, out_channels, stride=1, level_root=False, root_dim=0, root_kernel_size=1,
    dilation=1, root_residual=False)``.  As in the reference, the ``residual`` argument of ``forward`` is overwritten by the
    tree's own (``project(downsample(x))``), and a ``project`` whose result no block reads still runs."""

    def __init__(self, levels, block, in_channels, out_channels, stride=1, level_root=False, root_dim=0, root_kernel_size=1,
                 dilation=1, root_residual=False):
        super().__init__()
        if block is not BasicBlock:
            raise _lib.CTError('centertrack_amd Tree builds its blocks from centertrack_amd.dla_base.BasicBlock only')
        _no_dilation(dilation)
        if stride not in (1, 2):
            raise _lib.CTError('centertrack_amd Tree supports stride 1 and 2 (got %s)' % (stride,))
        if root_dim == 0:
            root_dim = 2 * out_channels
        if level_root:
            root_dim += in_channels
        if levels == 1:
            self.tree1 = block(in_channels, out_channels, stride, dilation=dilation)
            self.tree2 = block(out_channels, out_channels, 1, dilation=dilation)
        else:
            self.tree1 = Tree(levels - 1, block, in_channels, out_channels, stride, root_dim=0,
                              root_kernel_size=root_kernel_size, dilation=dilation, root_residual=root_residual)
            self.tree2 = Tree(levels - 1, block, out_channels, out_channels, root_dim=root_dim + out_channels,
                              root_kernel_size=root_kernel_size, dilation=dilation, root_residual=root_residual)
        if levels == 1:
            self.root = Root(root_dim, out_channels, root_kernel_size, root_residual)
        self.level_root = level_root
        self.root_dim = root_dim
        self.downsample = None
        self.project = None
        self.levels = levels
        if stride > 1:
            self.downsample = nn.MaxPool2d(stride, stride=stride)
        if in_channels != out_channels:
            self.project = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, bias=False),
                                         nn.BatchNorm2d(out_channels, momentum=BN_MOMENTUM))

    def _project(self, bottom):
        return _conv_bn_act(bottom, self.project[0], self.project[1], relu=False) if self.project else bottom

    def forward_nhwc(self, x, residual=None, children=None):
        children = [] if children is None else children
        if self.levels == 1:
            # the block's first unit and the pool read the same tensor: one autograd node, one input-gradient pass
            if self.downsample:
                h, bottom = self.tree1.first_half(x, pool=True)
            else:
                h, bottom = self.tree1.first_half(x), x
            residual = self._project(bottom)
            if self.level_root:
                children.append(bottom)
            x1 = self.tree1.second_half(h, residual)
            x2 = self.tree2.forward_nhwc(x1)
            return self.root.forward_nhwc(x2, x1, *children)
        bottom = _maxpool(x) if self.downsample else x
        self._project(bottom)                       # the reference computes it (and moves its running statistics); nobody reads it
        if self.level_root:
            children.append(bottom)
        x1 = self.tree1.forward_nhwc(x)
        children.append(x1)
        return self.tree2.forward_nhwc(x1, children=children)

    def forward(self, x, residual=None, children=None):
        children = None if children is None else [to_nhwc(c) for c in children]
        return to_nchw(self.forward_nhwc(to_nhwc(x), children=children))


class DLA(nn.Module):
    """Reference ``DLA(levels, channels, num_classes=1000, block=BasicBlock, residual_root=False, linear_root=False,
    opt=None)``.  ``forward(x, pre_img=None, pre_hm=None)`` returns the six level outputs (NCHW), ``forward_nhwc`` the same as
    ``[N,H,W,C]`` tensors.  With ``channels[0] == 16`` the stems run on this package's kernels (``_StemsFunction``), else on torch."""

    def __init__(self, levels, channels, num_classes=1000, block=BasicBlock, residual_root=False, linear_root=False, opt=None):
        super().__init__()
        if block is not BasicBlock:
            raise _lib.CTError('centertrack_amd DLA builds its levels from centertrack_amd.dla_base.BasicBlock only '
                               '(Bottleneck / BottleneckX are not covered)')
        _check_channels(*channels)
        self.channels = channels
        self.num_classes = num_classes

        def stem(cin):
            return nn.Sequential(nn.Conv2d(cin, channels[0], kernel_size=7, stride=1, padding=3, bias=False),
                                 nn.BatchNorm2d(channels[0], momentum=BN_MOMENTUM), nn.ReLU(inplace=True))
        self.base_layer = stem(3)
        self.level0 = self._make_conv_level(channels[0], channels[0], levels[0])
        self.level1 = self._make_conv_level(channels[0], channels[1], levels[1], stride=2)
        self.level2 = Tree(levels[2], block, channels[1], channels[2], 2, level_root=False, root_residual=residual_root)
        self.level3 = Tree(levels[3], block, channels[2], channels[3], 2, level_root=True, root_residual=residual_root)
        self.level4 = Tree(levels[4], block, channels[3], channels[4], 2, level_root=True, root_residual=residual_root)
        self.level5 = Tree(levels[5], block, channels[4], channels[5], 2, level_root=True, root_residual=residual_root)
        if getattr(opt, 'pre_img', False):
            self.pre_img_layer = stem(3)
        if getattr(opt, 'pre_hm', False):
            self.pre_hm_layer = stem(1)

    def _make_conv_level(self, inplanes, planes, convs, stride=1, dilation=1):
        _no_dilation(dilation)
        modules = []
        for i in range(convs):
            modules.extend([nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride if i == 0 else 1, padding=dilation, bias=False,
                                      dilation=dilation),
                            nn.BatchNorm2d(planes, momentum=BN_MOMENTUM), nn.ReLU(inplace=True)])
            inplanes = planes
        return nn.Sequential(*modules)

    def _stem_parts(self, x, pre_img, pre_hm):
        """[(stem, its input)] for x, pre_img, pre_hm; (None, None) where the input is absent"""
        parts = [(self.base_layer, x)]
        for name, t in (('pre_img_layer', pre_img), ('pre_hm_layer', pre_hm)):
            if t is not None and not hasattr(self, name):
                raise _lib.CTError('DLA: built without %s (opt.%s)' % (name, name[:-len('_layer')]))
            parts.append((getattr(self, name), t) if t is not None else (None, None))
        for _, t in parts:
            if t is not None:
                need_cuda(t, 'centertrack_amd backbone')
        return parts

    def _stems(self, x, pre_img, pre_hm):
        """the torch stems of a first width other than 16 -> the NCHW sum"""
        y = None
        for layer, t in self._stem_parts(x, pre_img, pre_hm):
            if t is None:
                continue
            s = layer(t)
            _emit(s.permute(0, 2, 3, 1))
            y = s if y is None else y + s
        return y

    def forward_nhwc(self, x, pre_img=None, pre_hm=None):
        """NCHW images -> the six level outputs as ``[N,H,W,C]`` tensors"""
        if self.channels[0] == 16:
            parts = self._stem_parts(x, pre_img, pre_hm)
            y = _stems([t for _, t in parts], [m for m, _ in parts])
        else:
            with torch.set_grad_enabled(recording()):
                y = self._stems(x, pre_img, pre_hm)
            y = to_nhwc(y)
        return self._levels_nhwc(y)

    def _levels_nhwc(self, y):
        """the six levels on the NHWC sum of the stems"""
        out = []
        for i in range(6):
            level = getattr(self, 'level{}'.format(i))
            if isinstance(level, Tree):
                y = level.forward_nhwc(y)
            else:
                for j in range(0, len(level), 3):
                    y = _conv_bn_act(y, level[j], level[j + 1], relu=True)
            out.append(y)
        return out

    def forward(self, x, pre_img=None, pre_hm=None):
        return [to_nchw(t) for t in self.forward_nhwc(x, pre_img, pre_hm)]

    def load_pretrained_model(self, data='imagenet', name='dla34', hash='ba72cf86'):
        """The reference's loader for a LOCAL ``.pth`` (``data + name`` is its path); nothing is downloaded"""
        if not name.endswith('.pth'):
            raise _lib.CTError('centertrack_amd DLA.load_pretrained_model reads a local .pth only (got name=%r): nothing is '
                               'downloaded' % (name,))
        model_weights = torch.load(data + name)
        num_classes = len(model_weights[list(model_weights.keys())[-1]])
        self.fc = nn.Conv2d(self.channels[-1], num_classes, kernel_size=1, stride=1, padding=0, bias=True)
        self.load_state_dict(model_weights, strict=False)


def dla34(pretrained=True, **kwargs):
    """Reference ``dla34``; ``pretrained=True`` would download the ImageNet weights and is refused: build with
    ``pretrained=False`` and call ``load_pretrained_model`` with a local file"""
    if pretrained:
        raise _lib.CTError('centertrack_amd dla34(pretrained=True) is refused: nothing is downloaded; use pretrained=False and '
                           'DLA.load_pretrained_model(data=<directory>, name=<file>.pth)')
    return DLA([1, 1, 1, 2, 2, 1], [16, 32, 64, 128, 256, 512], block=BasicBlock, **kwargs)
