"""The neck of DLA-34 as trainable drop-in modules: ``DeformConv``, ``IDAUp`` and ``DLAUp`` of the reference's
``model/networks/dla.py`` (lines 506-574), with its constructor signatures, state-dict keys, initialisation and calling
conventions, on the kernels of libcentertrack_hip.so.

Between the first node's input and the last node's output every tensor is an NHWC ``[N,H,W,C]`` fp32 tensor; NCHW <-> NHWC
conversion happens once per input and once per returned tensor of the outermost module that is called.  A ``DeformConv`` is
the offset/mask conv (``ct_conv2d``, sigmoid fused), ``ct_dcn_v2``, BatchNorm statistics (``ct_bn_stats``, training mode
only) and BatchNorm + ReLU (``ct_bn_relu_apply``); an ``IDAUp`` step is ``proj`` -> ``ct_upsample_add`` -> ``node``.

The parameters live in real ``nn.BatchNorm2d`` / ``nn.ConvTranspose2d`` / ``nn.Conv2d`` objects and in the ``DCN`` drop-in
(``load_state_dict``, optimizers and the reference's ``fill_up_weights`` work unchanged) and are packed at every call: no
packing is cached.  Statistics follow torch: batch statistics when, and only when, the BatchNorm is in training mode, and
then the running statistics are updated as torch does.  A graph is recorded only under ``dcn_v2.trainable()`` with autograd
enabled; otherwise the same forward runs with nothing saved.  CUDA fp32 tensors only: there is no CPU fallback.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train, dcn_v2, ops
from ._train import BN_MOMENTUM, bn_statistics, recording, saved_mean, to_nchw, update_running_stats  # noqa: F401
from .ops import View


def to_nhwc(x):
    return _train.to_nhwc(x, 'neck')


def fill_up_weights(up):
    """The bilinear kernel the reference gives every ``up_i`` (dla.py:454-463), same for every channel"""
    w = up.weight.data
    k = w.size(2)
    f = math.ceil(k / 2)
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    line = torch.tensor([1 - abs(i / f - c) for i in range(k)], dtype=w.dtype)
    w.copy_((line.view(k, 1) * line.view(1, k)).expand_as(w))


# ---------------------------------------------------------------------------------------------------------------------
# DeformConv

def _deform_forward(x, mod):
    """``DeformConv.forward`` on the NHWC view ``x`` -> (output view, what a backward needs)"""
    dcn, bn = mod.conv, mod.actf[0]
    if x.C != dcn.in_channels:
        raise _lib.CTError('DeformConv(%d, %d) got %d channels' % (dcn.in_channels, dcn.out_channels, x.C))
    dev = x.buf.device
    off = dcn.conv_offset_mask
    # ``o1, o2, mask = chunk(out, 3, 1); offset = cat(o1, o2)`` is out[:, :18]; the sigmoid of channels 18..26 is fused
    om = ops.conv2d(x, ops.pack_weight(off.weight.detach()), 27, 3, 1, shift=off.bias.detach(), sig=(18, 27),
                    out=ops.new_view(x.N, x.H, x.W, 32, dev))
    om = View(om.buf, 0, 27)
    z = ops.dcn_v2(x, om, ops.pack_weight(dcn.weight.detach()), dcn.out_channels, shift=dcn.bias.detach())
    mean, invstd, batch = bn_statistics(bn, z, 'DeformConv')
    y = ops.bn_relu_apply(z, mean, invstd, bn.weight.detach(), _train.bn_beta(batch, bn.bias.detach()))
    return y, (om, z, mean, invstd, batch)


class _DeformConvFunction(torch.autograd.Function):
    """One DeformConv node over ``[N,H,W,C]`` tensors.  Saved: the input, the offset/mask map, the DCN output ``z`` and
    the statistics; the ReLU mask is recomputed from ``z`` with the forward's own fma."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_off, b_off, gamma, beta, mod):
        y, (om, z, mean, invstd, batch) = _deform_forward(View(x), mod)
        ctx.om, ctx.z, ctx.mean, ctx.invstd, ctx.batch = om, z, saved_mean(mean, batch), invstd, batch
        ctx.save_for_backward(x, weight, w_off, gamma, beta)
        return y.buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, w_off, gamma, beta = ctx.saved_tensors
        need_x, need_w, need_b, need_woff, need_boff, need_gamma, need_beta = ctx.needs_input_grad[:7]
        need_off = need_woff or need_boff
        need_om = need_off or need_x                   # the input reaches the output through the offsets as well
        need_z = need_om or need_w or need_b
        xv, om = View(x), ctx.om
        if isinstance(ctx.batch, _train.SyncedBatch):  # statistics over all ranks: sums -> all-reduce -> apply
            gz, _, ggamma, gbeta = _train.synced_bn_backward([dict(
                z=ctx.z, gy=View(gy.contiguous()), mean=ctx.mean, invstd=ctx.invstd, gamma=gamma.detach(), beta=beta.detach(),
                sync=ctx.batch, neck=True, need_z=need_z, need_gamma=need_gamma, need_beta=need_beta)])[0]
        else:
            gz, ggamma, gbeta = ops.bn_relu_backward(ctx.z, View(gy.contiguous()), ctx.mean, ctx.invstd, gamma.detach(),
                                                     beta.detach(), ctx.batch, need_z=need_z, need_gamma=need_gamma,
                                                     need_beta=need_beta)
        gx = gw = gb = gwoff = gboff = None
        if need_z:
            wT = ops.pack_weight_t(weight.detach()) if need_om else None
            # zeroed: the five pad channels of the 32-wide buffer are inputs of the convolution below
            gom = View(torch.zeros((xv.N, xv.H, xv.W, 32), dtype=torch.float32, device=x.device), 0, 27) if need_om else None
            gx, gom, gw, gb = ops.dcn_v2_backward(xv, om, gz, wT, need_x=need_x, need_om=need_om, need_w=need_w,
                                                  need_b=need_b, gom=gom)
        if need_om:
            ops.mask_sigmoid_backward(gom, om)
        if need_off:
            gwoff, gboff = ops.conv_backward_weight(xv, gom, 3, need_bias=need_boff)
        if need_x:
            # gx += conv3x3(gom, w_off^T) over the 32-wide buffer
            gx = ops.conv_backward_input(gom, w_off.detach(), res=gx, out=ops.new_view(xv.N, xv.H, xv.W, xv.C, x.device))
        return (gx.buf if need_x else None, gw if need_w else None, gb if need_b else None,
                gwoff if need_woff else None, gboff if need_boff else None, ggamma, gbeta, None)


class DeformConv(nn.Module):
    """Reference ``DeformConv(chi, cho)``: ``conv`` = the ``DCN`` drop-in as parameter holder, ``actf`` = BatchNorm2d + ReLU"""

    def __init__(self, chi, cho):
        super().__init__()
        if cho % 4:
            raise _lib.CTError('centertrack_amd DeformConv needs out channels %% 4 == 0 (got %d)' % cho)
        self.actf = nn.Sequential(nn.BatchNorm2d(cho, momentum=BN_MOMENTUM), nn.ReLU(inplace=True))
        self.conv = dcn_v2.DCN(chi, cho, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)

    def forward_nhwc(self, x):
        """``x``: contiguous ``[N,H,W,chi]`` fp32 CUDA tensor -> ``[N,H,W,cho]``"""
        if recording():
            c, bn = self.conv, self.actf[0]
            return _DeformConvFunction.apply(x, c.weight, c.bias, c.conv_offset_mask.weight, c.conv_offset_mask.bias,
                                             bn.weight, bn.bias, self)
        with torch.no_grad():
            return _deform_forward(View(x), self)[0].buf

    def forward(self, x):
        return to_nchw(self.forward_nhwc(to_nhwc(x)))


# ---------------------------------------------------------------------------------------------------------------------
# IDAUp / DLAUp

class _UpsampleAddFunction(torch.autograd.Function):
    """``up(x) + skip`` over ``[N,H,W,C]`` tensors: ct_upsample_add and its backward; the skip gradient is the incoming one"""

    @staticmethod
    def forward(ctx, x, skip, w, f):
        ctx.f = f
        ctx.save_for_backward(x, w)
        return ops.upsample_add(View(x), w.detach(), f, View(skip)).buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        need_x, need_skip, need_w = ctx.needs_input_grad[:3]
        gy = gy.contiguous()
        gx, gw, _ = ops.upsample_add_backward(View(x), w.detach(), ctx.f, View(gy), need_x=need_x, need_w=need_w)
        return (gx.buf if need_x else None, gy if need_skip else None, gw, None)


def _upsample_add(x, skip, up):
    f = up.stride[0]
    if tuple(skip.shape) != (x.shape[0], x.shape[1] * f, x.shape[2] * f, x.shape[3]):
        raise _lib.CTError('IDAUp: up x%d of %s does not fit the skip %s (NHWC)' % (f, tuple(x.shape), tuple(skip.shape)))
    if recording():
        return _UpsampleAddFunction.apply(x, skip, up.weight, f)
    with torch.no_grad():
        return ops.upsample_add(View(x), up.weight.detach(), f, View(skip)).buf


def _node_types(node_type):
    """``node_type`` as the reference passes it: one class (both nodes) or a (proj, node) pair, e.g. ``DLA_NODE['dcn']``"""
    types = (node_type, node_type) if isinstance(node_type, type) else tuple(node_type)
    if len(types) != 2 or any(t is not DeformConv for t in types):
        raise _lib.CTError('centertrack_amd IDAUp / DLAUp build their nodes from centertrack_amd.dla_up.DeformConv only')
    return types


class IDAUp(nn.Module):
    """Reference ``IDAUp(o, channels, up_f)``: per level i >= 1 ``proj_i`` (DeformConv c_i -> o), ``up_i`` (depth-wise
    ConvTranspose2d, kernel 2f, stride f, padding f/2, bilinear init) and ``node_i`` (DeformConv o -> o)"""

    def __init__(self, o, channels, up_f, node_type=(DeformConv, DeformConv)):
        super().__init__()
        proj_t, node_t = _node_types(node_type)
        for i in range(1, len(channels)):
            c, f = channels[i], int(up_f[i])
            if f not in (2, 4, 8):
                raise _lib.CTError('centertrack_amd IDAUp supports up factors 2, 4 and 8 (got %d)' % f)
            proj, node = proj_t(c, o), node_t(o, o)
            up = nn.ConvTranspose2d(o, o, f * 2, stride=f, padding=f // 2, output_padding=0, groups=o, bias=False)
            fill_up_weights(up)
            setattr(self, 'proj_' + str(i), proj)
            setattr(self, 'up_' + str(i), up)
            setattr(self, 'node_' + str(i), node)

    def forward_nhwc(self, layers, startp, endp):
        """The reference's loop on a list of ``[N,H,W,C]`` tensors, rewritten in place"""
        for i in range(startp + 1, endp):
            k = str(i - startp)
            x = getattr(self, 'proj_' + k).forward_nhwc(layers[i])
            x = _upsample_add(x, layers[i - 1], getattr(self, 'up_' + k))
            layers[i] = getattr(self, 'node_' + k).forward_nhwc(x)

    def forward(self, layers, startp, endp):
        """``layers``: NCHW tensors; entries startp + 1 .. endp - 1 are rewritten in place, as the reference does"""
        nhwc = list(layers)
        for i in range(startp, endp):
            nhwc[i] = to_nhwc(layers[i])
        self.forward_nhwc(nhwc, startp, endp)
        for i in range(startp + 1, endp):
            layers[i] = to_nchw(nhwc[i])


class DLAUp(nn.Module):
    """Reference ``DLAUp(startp, channels, scales, in_channels=None)``: ``ida_i`` for i = 0 .. len(channels) - 2, each built
    with the ``node_type`` given (a class or a (proj, node) pair, as the reference's ``DLASeg`` passes it).
    ``forward(layers)`` returns the list of outputs, finest first, and rewrites ``layers[startp + 1:]`` in place as the
    reference does; the levels stay NHWC across all ``ida_i``, each tensor that leaves is converted once, and the coarsest
    output is ``layers[-1]`` itself."""

    def __init__(self, startp, channels, scales, in_channels=None, node_type=DeformConv):
        super().__init__()
        self.startp = startp
        node_type = _node_types(node_type)
        if in_channels is None:
            in_channels = channels
        self.channels = channels
        channels = list(channels)
        in_channels = list(in_channels)
        scales = np.array(scales, dtype=int)
        for i in range(len(channels) - 1):
            j = -i - 2
            setattr(self, 'ida_{}'.format(i), IDAUp(channels[j], in_channels[j:], scales[j:] // scales[j], node_type=node_type))
            scales[j + 1:] = scales[j]
            in_channels[j + 1:] = [channels[j] for _ in channels[j + 1:]]

    def forward_nhwc(self, layers):
        """``forward`` on a list of ``[N,H,W,C]`` tensors, with its in-place semantics (``layers[startp + 1:]`` are rewritten)
        and no conversion: every returned tensor is an entry of ``layers``"""
        n = len(layers)
        out = [layers[-1]]
        for i in range(n - self.startp - 1):
            getattr(self, 'ida_{}'.format(i)).forward_nhwc(layers, n - i - 2, n)
            out.insert(0, layers[-1])
        return out

    def forward(self, layers):
        n = len(layers)
        out = [layers[-1]]
        steps = n - self.startp - 1
        if steps < 1:
            return out
        nhwc = list(layers)
        for i in range(self.startp, n):
            nhwc[i] = to_nhwc(layers[i])
        for i in range(steps):
            getattr(self, 'ida_{}'.format(i)).forward_nhwc(nhwc, n - i - 2, n)
            out.insert(0, to_nchw(nhwc[-1]))
        for i in range(self.startp + 1, n - 1):
            layers[i] = to_nchw(nhwc[i])
        layers[-1] = out[0]
        return out
