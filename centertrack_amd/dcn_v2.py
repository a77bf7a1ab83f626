"""Drop-in for the un-vendored ``DCNv2`` extension (SURVEY.md boundary B1).

The reference does ``from .DCNv2.dcn_v2 import DCN`` (src/lib/model/networks/dla.py:19,
necks/dlaup.py:17, resdcn.py:20, necks/msraup.py:20) and builds
``DCN(chi, cho, kernel_size=(3,3), stride=1, padding=1, dilation=1, deformable_groups=1)``
(dla.py:513), called as ``self.conv(x)`` on an NCHW fp32 tensor.  This module exports the
upstream names -- ``DCN``, ``DCNv2``, ``dcn_v2_conv`` -- with upstream's constructor
signatures and state-dict keys (``weight, bias, conv_offset_mask.weight,
conv_offset_mask.bias``), backed by ``ct_conv2d`` (offset/mask conv, sigmoid fused) and
``ct_dcn_v2`` (fused bilinear gather + fp32 MFMA contraction) of libcentertrack_hip.so.
Placing / aliasing this file as ``model/networks/DCNv2/dcn_v2.py`` makes the reference's
``dla.py`` run on the HIP kernel unchanged.

CUDA tensors only: there is no CPU fallback.  Supported geometry is what the hot path uses:
3x3, stride 1, padding 1, dilation 1, one deformable group, Cin a multiple of 32.

Training is opt-in: by default the three ``forward``s run under ``no_grad`` exactly as an
inference build does.  After ``set_trainable(True)`` (or inside ``with trainable():``) and with
autograd enabled they return tensors with a ``grad_fn`` whose backward is ``ct_dcn_v2_backward``
(gradients for input, offset, mask, weight and bias).  The input gradient is
accumulated with float atomics and is equal from run to run only to fp32 rounding; the other
four are bitwise reproducible.

The modules keep no packed copy of their parameters: ``weight`` (and ``conv_offset_mask.weight``) are packed into the
MFMA fragment layouts at every call, from the values the storage holds at that moment.  A parameter may therefore be
changed by any means between two calls -- an optimizer step, ``load_state_dict``, ``nn.init``, or a write through
``.data`` (``m.weight.data.mul_(2)``, ``w = m.weight.data; w[...] = ...``, as the reference's ``fill_up_weights`` and
many checkpoint loaders do), which does not advance the parameter's version counter -- and the next call uses it.
"""
import math

import torch
from torch import nn

from . import _lib, ops
from ._train import is_trainable, need_cuda, recording, set_trainable, trainable  # noqa: F401  (the switch is public API here)


def _check_geometry(kernel_size, stride, padding, dilation, deformable_groups, cin):
    ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    st = stride if isinstance(stride, int) else stride[0]
    pd = padding if isinstance(padding, int) else padding[0]
    dl = dilation if isinstance(dilation, int) else dilation[0]
    if ks != (3, 3) or st != 1 or pd != 1 or dl != 1 or deformable_groups != 1:
        raise _lib.CTError('centertrack_amd DCN supports kernel 3x3, stride 1, padding 1, dilation 1, '
                           'deformable_groups 1 (the DLA-34 hot path, dla.py:513); got k=%s s=%s p=%s d=%s dg=%s'
                           % (ks, st, pd, dl, deformable_groups))
    if cin % 32:
        raise _lib.CTError('centertrack_amd DCN needs in_channels %% 32 == 0 (got %d)' % cin)


def _om_view(offset, mask):
    """NCHW offset [B,18,H,W] + mask [B,9,H,W] -> the kernel's NHWC offset/mask map [B,H,W,32]"""
    B, _, H, W = offset.shape
    om = ops.new_view(B, H, W, 32, offset.device)
    lib = _lib.load()
    st = _lib.stream_ptr()
    cat = torch.cat((offset, mask), 1).contiguous()
    _lib.check(lib.ct_nchw_to_nhwc(cat.data_ptr(), B, 27, H, W, om.ptr, om.ld, st), 'ct_nchw_to_nhwc')
    return ops.View(om.buf, 0, 27)


def _forward(input, offset, mask, weight, bias, wp):
    """The drop-in's forward on NCHW tensors -> (out view, x view, om view).  ``wp``: the fragment packing of ``weight``, or
    None to make it here"""
    x = ops.view_from_nchw(input)
    om = _om_view(offset.float(), mask.float())
    if wp is None:
        wp = ops.pack_weight(weight.detach())
    out = ops.dcn_v2(x, om, wp, weight.shape[0], shift=None if bias is None else bias.detach().contiguous())
    return out, x, om


class _DCNv2Function(torch.autograd.Function):
    """``ct_dcn_v2`` forward (the inference kernel, unchanged) + ``ct_dcn_v2_backward``.  ``packs`` = the (forward,
    transposed) fragment packings of ``weight`` when the caller has made them (the modules, at every call), else None:
    the transposed one is then made in backward."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, packs):
        wp, wT = packs if packs is not None else (None, None)
        out, ctx.x, ctx.om = _forward(input, offset, mask, weight, bias, wp)
        ctx.wT = wT
        ctx.has_bias = bias is not None
        ctx.save_for_backward(weight)
        return ops.view_to_nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        weight, = ctx.saved_tensors
        need_x, need_off, need_mask, need_w, need_b = ctx.needs_input_grad[:5]
        need_om = need_off or need_mask
        wT = ctx.wT
        if (need_x or need_om) and wT is None:
            wT = ops.pack_weight_t(weight.detach())
        gy = ops.view_from_nchw(grad_out)
        gx, gom, gw, gb = ops.dcn_v2_backward(ctx.x, ctx.om, gy, wT, need_x=need_x, need_om=need_om, need_w=need_w,
                                              need_b=need_b and ctx.has_bias)
        return (ops.view_to_nchw(gx) if need_x else None,
                ops.view_to_nchw(gom.slice(0, 18)) if need_off else None,
                ops.view_to_nchw(gom.slice(18, 9)) if need_mask else None,
                gw if need_w else None, gb if need_b and ctx.has_bias else None, None)


def dcn_v2_conv(input, offset, mask, weight, bias, stride=1, padding=1, dilation=1, deformable_groups=1):
    """Upstream ``dcn_v2_conv = _DCNv2.apply``.  offset [B,18,H,W] with (dy,dx) interleaved per tap, mask [B,9,H,W]
    (already sigmoid-ed), weight [Co,Ci,3,3], bias [Co].  Differentiable under ``trainable()``."""
    need_cuda(input, 'centertrack_amd DCN', dims=None)
    _check_geometry(tuple(weight.shape[2:]), stride, padding, dilation, deformable_groups, input.shape[1])
    if recording():
        return _DCNv2Function.apply(input, offset, mask, weight, bias, None)
    return _dcn_v2_conv_inference(input, offset, mask, weight, bias)


@torch.no_grad()
def _dcn_v2_conv_inference(input, offset, mask, weight, bias):
    return ops.view_to_nchw(_forward(input, offset, mask, weight, bias, None)[0])


class DCNv2(nn.Module):
    """Upstream ``DCNv2``: ``forward(input, offset, mask)`` with caller-provided offsets."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        _check_geometry(kernel_size, stride, padding, dilation, deformable_groups, in_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        stdv = 1.0 / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        self.bias.data.zero_()

    def _packs(self):
        """(forward, transposed) MFMA-fragment packings of ``weight``, made from its current values at every call: one
        small launch each on the caller's stream.  Nothing is cached: a write through ``weight.data`` changes the storage
        without advancing the parameter's version counter, so no key built from ``data_ptr`` and ``_version`` sees it."""
        w = self.weight.detach()
        return ops.pack_weight(w), ops.pack_weight_t(w)

    def forward(self, input, offset, mask):
        need_cuda(input, 'centertrack_amd DCN', dims=None)
        if recording():
            return _DCNv2Function.apply(input, offset, mask, self.weight, self.bias, self._packs())
        return self._forward_inference(input, offset, mask)

    @torch.no_grad()
    def _forward_inference(self, input, offset, mask):
        return ops.view_to_nchw(_forward(input, offset, mask, self.weight, self.bias, None)[0])


class DCN(DCNv2):
    """Upstream ``DCN``: owns ``conv_offset_mask`` (Conv2d Cin -> 27, zero-initialised);
    ``forward(x)`` = offset/mask conv -> chunk(o1,o2,mask) -> sigmoid(mask) -> deformable conv."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        channels_ = self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset_mask = nn.Conv2d(self.in_channels, channels_, kernel_size=self.kernel_size,
                                          stride=self.stride, padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def forward(self, input):
        need_cuda(input, 'centertrack_amd DCN', dims=None)
        if recording():
            # as upstream: the offset/mask conv, chunk / cat / sigmoid in torch (their backward is torch's), the
            # deformable conv through the Function
            out = self.conv_offset_mask(input)
            o1, o2, mask = torch.chunk(out, 3, dim=1)
            offset = torch.cat((o1, o2), dim=1)
            return _DCNv2Function.apply(input, offset, torch.sigmoid(mask), self.weight, self.bias, self._packs())
        return self._forward_inference(input)

    @torch.no_grad()
    def _forward_inference(self, input):
        x = ops.view_from_nchw(input)
        B, H, W = x.N, x.H, x.W
        # ``o1, o2, mask = chunk(out, 3, 1); offset = cat(o1, o2)`` is out[:, :18]; the sigmoid of
        # channels 18..26 is fused into the conv epilogue
        om = ops.conv2d(x, ops.pack_weight(self.conv_offset_mask.weight.detach()), 27, 3, 1,
                        shift=self.conv_offset_mask.bias.detach(), sig=(18, 27),
                        out=ops.new_view(B, H, W, 32, input.device))
        out = ops.dcn_v2(x, ops.View(om.buf, 0, 27), ops.pack_weight(self.weight.detach()), self.out_channels,
                         shift=self.bias.detach())
        return ops.view_to_nchw(out)
