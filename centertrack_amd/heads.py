"""Trainable heads (reference ``BaseModel.__init__`` / ``forward``, src/lib/model/networks/base_model.py:24-65,86-90) on the
HIP kernels: ``FusedHeads`` is the differentiable module, ``HeadFinetuner`` puts it on a frozen ``DLASegHIP`` trunk.

Forward is the un-fused heads plan of ``model.DLASegHIP`` (one ``ct_conv2d`` 64 -> hc * nheads with bias and ReLU into an
NHWC hidden map, one 1x1 ``ct_conv2d`` per head into NCHW logits); backward is ``ct_heads_tail_backward``,
``ct_conv2d_backward_weight`` and, for the input gradient, a ``ct_conv2d`` with the transposed weight (csrc/heads_bwd.hip,
DESIGN.md section 11).  No atomics: every gradient is bitwise equal from run to run.

Like ``dcn_v2.DCN`` the module keeps no packed copy of a parameter: the weights are packed into the MFMA fragment layout
at every call from what their storage holds at that moment, so an optimizer step, ``load_state_dict`` or a write through
``.data`` is seen by the next call.  CUDA tensors only: a CPU tensor raises ``CTError``.

Slot heads (``FusedHeads(..., slot_heads=True)`` and a call with ``ind``): a head of ``SLOT_HEADS`` -- one
the training loss reads at ``batch['ind']`` only -- is evaluated at those M cells per image.  ``ct_slot_gather`` builds the
im2col rows of the 3x3 layer at the slots, on which the heads are 1x1 convolutions over a map [N,1,M,9*C]: the same
``ct_conv2d`` / ``ct_heads_tail_backward`` / ``ct_conv2d_backward_weight`` calls with kernel size 1, and ``ct_slot_fold`` adds
the input gradient's patches onto the dense heads' input gradient.  Still no atomics, still bitwise reproducible.
"""
from collections import OrderedDict

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._train import need_cuda


# the heads GenericLoss reads at batch['ind'] only (losses.py; hm and hm_hp are dense, hp_offset is read at hp_ind)
SLOT_HEADS = ('reg', 'wh', 'tracking', 'ltrb', 'ltrb_amodal', 'hps', 'dep', 'dim', 'amodel_offset', 'velocity', 'rot',
              'nuscenes_att')


def _one_head_conv(head_conv, heads):
    """the single hidden width of all heads, from an int or the reference's {head: [256]}"""
    if isinstance(head_conv, dict):
        vals = {tuple(v) if isinstance(v, (list, tuple)) else (v,) for h, v in head_conv.items() if h in heads}
    else:
        vals = {tuple(head_conv) if isinstance(head_conv, (list, tuple)) else (head_conv,)}
    if len(vals) != 1 or len(next(iter(vals))) != 1:
        raise _lib.CTError('FusedHeads supports one head-conv layer of one width for all heads (got %r)' % (head_conv,))
    hc = int(next(iter(vals))[0])
    if hc <= 0 or hc % 16:
        raise _lib.CTError('FusedHeads needs head_conv %% 16 == 0 (got %d)' % hc)
    return hc


def _split(names, params):
    """``params`` = (w0, b0, w2, b2) per head in the order of ``names``, detached -> ([w0], [b0], {head: w2}, {head: b2})"""
    p = [t.detach() for t in params]
    return p[0::4], p[1::4], OrderedDict(zip(names, p[2::4])), OrderedDict(zip(names, p[3::4]))


class _HeadsFunction(torch.autograd.Function):
    """(head names, feat, *(w0, b0, w2, b2 per head)) -> the heads' raw logits.  ``feat``: NCHW tensor or ``ops.View``."""

    @staticmethod
    def forward(ctx, names, feat, *params):
        nh = len(names)
        w0s, b0s, w2s, b2s = _split(names, params)
        grad = any(ctx.needs_input_grad)
        if isinstance(feat, ops.View):
            # what backward reads lives in storage private to this call: the caller's view is usually a buffer of a launch
            # plan, rewritten by the next forward
            need_feat = any(ctx.needs_input_grad[2 + 4 * j] or ctx.needs_input_grad[3 + 4 * j] for j in range(nh))
            x = ops.View(feat.buf[..., feat.c0:feat.c0 + feat.C].clone(memory_format=torch.contiguous_format)) if need_feat else feat
        else:
            x = ops.view_from_nchw(feat.detach())
        outs, mid = ops.heads_forward_train(x, torch.cat(w0s, 0), torch.cat(b0s, 0), w2s, b2s)
        if grad:
            ctx.names, ctx.x, ctx.mid = names, x, mid
            ctx.save_for_backward(*params)
        return tuple(outs.values())

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        res, grads = _heads_gradients(ctx.names, ctx.x, ctx.mid, ctx.saved_tensors, ctx.needs_input_grad, gouts)
        return (None, ops.view_to_nchw(res['x']) if ctx.needs_input_grad[1] else None) + grads


def _heads_gradients(names, x, mid, params, need, gouts):
    """what both heads functions compute in backward -> (``ops.heads_backward``'s result, the parameter gradients in the order
    of ``params``); ``need`` = the function's ``needs_input_grad`` (names, feat, *params)"""
    nh = len(names)
    w0s, _, w2s, _ = _split(names, params)
    hc = w0s[0].shape[0]
    needs = {'x': need[1], 'w0': any(need[2 + 4 * j] for j in range(nh)), 'b0': any(need[3 + 4 * j] for j in range(nh)),
             'w2': {h: need[4 + 4 * j] for j, h in enumerate(names)}, 'b2': {h: need[5 + 4 * j] for j, h in enumerate(names)}}
    w0 = torch.cat(w0s, 0) if needs['x'] else None
    res = ops.heads_backward(x, mid, dict(zip(names, gouts)), w0, w2s, needs)
    grads = []
    for j, h in enumerate(names):
        grads += [res['w0'][hc * j:hc * (j + 1)] if need[2 + 4 * j] else None,
                  res['b0'][hc * j:hc * (j + 1)] if need[3 + 4 * j] else None,
                  res['w2'][h] if need[4 + 4 * j] else None, res['b2'][h] if need[5 + 4 * j] else None]
    return res, tuple(grads)


class _HeadsNHWCFunction(torch.autograd.Function):
    """``_HeadsFunction`` over a contiguous ``[N,H,W,C]`` tensor that takes part in autograd: nothing is converted on the way
    in, and the input gradient leaves as the NHWC tensor ``ops.heads_backward`` produces."""

    @staticmethod
    def forward(ctx, names, feat, *params):
        w0s, b0s, w2s, b2s = _split(names, params)
        outs, mid = ops.heads_forward_train(ops.View(feat.detach()), torch.cat(w0s, 0), torch.cat(b0s, 0), w2s, b2s)
        if any(ctx.needs_input_grad):
            ctx.names, ctx.mid = names, mid
            ctx.save_for_backward(feat, *params)
        return tuple(outs.values())

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        feat, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        res, grads = _heads_gradients(ctx.names, ops.View(feat.detach()), ctx.mid, params, ctx.needs_input_grad, gouts)
        return (None, res['x'].buf if ctx.needs_input_grad[1] else None) + grads


def _w0_cols(w0):
    """first-layer weights [O,C,3,3] in the column order of ``ops.slot_gather``: [O, 9*C, 1, 1], column (ky*3+kx)*C + c"""
    return w0.permute(0, 2, 3, 1).reshape(w0.shape[0], -1, 1, 1)


class _SlotHeadsFunction(torch.autograd.Function):
    """(head names, names of the slot heads, nhwc, feat, ind, *(w0, b0, w2, b2 per head)) -> per head, in the order of the
    names, the dense logits [N,c,H,W] or, for a slot head, its logits at the slots [N,M,c] (a zero row for an ``ind`` outside
    [0, H*W)).  ``feat``: an NCHW tensor or an ``ops.View`` (input gradient NCHW), with ``nhwc`` a contiguous [N,H,W,C] tensor
    (input gradient NHWC).  The dense heads are ``_HeadsFunction``'s launches over the heads that are left."""
    FIRST = 5                                                            # position of the first parameter

    @staticmethod
    def forward(ctx, names, slot, nhwc, feat, ind, *params):
        F = _SlotHeadsFunction.FIRST
        w0s, b0s, w2s, b2s = _split(names, params)
        grad = any(ctx.needs_input_grad)
        if nhwc:
            x = ops.View(feat.detach())
        elif isinstance(feat, ops.View):
            need_feat = any(ctx.needs_input_grad[F + 4 * j] or ctx.needs_input_grad[F + 1 + 4 * j] for j in range(len(names)))
            x = ops.View(feat.buf[..., feat.c0:feat.c0 + feat.C].clone(memory_format=torch.contiguous_format)) if need_feat else feat
        else:
            x = ops.view_from_nchw(feat.detach())
        ind = ind.detach().long().contiguous()
        if ind.dim() != 2 or ind.shape[0] != x.N:
            raise _lib.CTError('FusedHeads: ind must be [%d, M] (got %s)' % (x.N, tuple(ind.shape)))
        N, M = ind.shape
        dense = [h for h in names if h not in slot]
        pos = {h: j for j, h in enumerate(names)}
        outs, mid_d = {}, None
        if dense:
            od, mid_d = ops.heads_forward_train(x, torch.cat([w0s[pos[h]] for h in dense], 0), torch.cat([b0s[pos[h]] for h in dense], 0),
                                                OrderedDict((h, w2s[h]) for h in dense), OrderedDict((h, b2s[h]) for h in dense))
            outs.update(od)
        cols = ops.slot_gather(x, ind)
        w0c = _w0_cols(torch.cat([w0s[pos[h]] for h in slot], 0))
        os_, mid_s = ops.heads_forward_train(cols, w0c, torch.cat([b0s[pos[h]] for h in slot], 0),
                                             OrderedDict((h, w2s[h]) for h in slot), OrderedDict((h, b2s[h]) for h in slot), ks=1)
        invalid = ((ind < 0) | (ind >= x.H * x.W)).view(N, 1, 1, M)
        for h in slot:
            outs[h] = os_[h].masked_fill_(invalid, 0.0).view(N, -1, M).transpose(1, 2)
        if grad:
            ctx.names, ctx.slot, ctx.dense, ctx.nhwc = names, slot, dense, nhwc
            ctx.x, ctx.cols, ctx.mid_d, ctx.mid_s, ctx.ind, ctx.invalid = x, cols, mid_d, mid_s, ind, invalid
            ctx.w0c = w0c if ctx.needs_input_grad[3] else None           # (a copy made in this call: the patch conv's weight)
            ctx.save_for_backward(*params)
        return tuple(outs[h] for h in names)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        F = _SlotHeadsFunction.FIRST
        names, slot, dense, need = ctx.names, ctx.slot, ctx.dense, ctx.needs_input_grad
        params = ctx.saved_tensors
        w0s, _, w2s, _ = _split(names, params)
        pos = {h: j for j, h in enumerate(names)}
        hc = w0s[0].shape[0]
        N, M = ctx.ind.shape
        need_x = need[3]

        def needs_of(group):
            return {'x': need_x, 'w0': any(need[F + 4 * pos[h]] for h in group), 'b0': any(need[F + 1 + 4 * pos[h]] for h in group),
                    'w2': {h: need[F + 2 + 4 * pos[h]] for h in group}, 'b2': {h: need[F + 3 + 4 * pos[h]] for h in group}}
        gx, res = None, {}
        # the dense heads first: their input gradient is the map the slot patches are folded into
        if dense:
            w0 = torch.cat([w0s[pos[h]] for h in dense], 0) if need_x else None
            res['dense'] = ops.heads_backward(ctx.x, ctx.mid_d, {h: gouts[pos[h]] for h in dense}, w0,
                                              OrderedDict((h, w2s[h]) for h in dense), needs_of(dense))
            gx = res['dense']['x']
        # a slot head's gradient arrives as [N,M,c]: back to the map [N,c,1,M] the logits were written as (no copy when it comes
        # from GenericLoss), rows of invalid slots dropped
        gs = {h: gouts[pos[h]].transpose(1, 2).unsqueeze(2).masked_fill(ctx.invalid, 0.0).contiguous() for h in slot}
        rs = ops.heads_backward(ctx.cols, ctx.mid_s, gs, ctx.w0c, OrderedDict((h, w2s[h]) for h in slot), needs_of(slot), ks=1)
        if rs['w0'] is not None:                                        # [O, 9*C, 1, 1] -> OIHW
            rs['w0'] = rs['w0'].view(rs['w0'].shape[0], 3, 3, -1).permute(0, 3, 1, 2).contiguous()
        res['slot'] = rs
        if need_x:
            if gx is None:
                gx = ops.View(torch.zeros((ctx.x.N, ctx.x.H, ctx.x.W, ctx.x.C), dtype=torch.float32, device=ctx.ind.device))
            ops.slot_fold(rs['x'], ctx.ind, gx)
        grads = []
        for h in names:
            j = pos[h]
            group = slot if h in slot else dense
            r, k = res['slot' if h in slot else 'dense'], group.index(h)
            grads += [r['w0'][hc * k:hc * (k + 1)] if need[F + 4 * j] else None,
                      r['b0'][hc * k:hc * (k + 1)] if need[F + 1 + 4 * j] else None,
                      r['w2'][h] if need[F + 2 + 4 * j] else None, r['b2'][h] if need[F + 3 + 4 * j] else None]
        gfeat = None
        if need_x:
            gfeat = gx.buf if ctx.nhwc else ops.view_to_nchw(gx)
        return (None, None, None, gfeat, None) + tuple(grads)


class FusedHeads(nn.Module):
    """The heads of the reference's ``BaseModel`` as one differentiable module: per head ``conv3x3 in_channels -> head_conv
    + bias, ReLU, conv1x1 head_conv -> c + bias``, parameters under the reference's names (``<head>.0.weight``,
    ``<head>.0.bias``, ``<head>.2.weight``, ``<head>.2.bias``) and with its initialisation (base_model.py:54-57: torch's
    Conv2d default for the weights; biases 0; in a head whose name contains ``hm`` the last bias = ``prior_bias`` and, as
    there, the first layer's bias keeps torch's default).

    ``forward(feat)``: NCHW fp32 CUDA tensor [B,in_channels,H,W] or an ``ops.View`` -> ``OrderedDict{head: raw logits
    [B,c,H,W]}`` through ONE autograd function for all heads.  What is computed in backward follows ``requires_grad``: a
    feature map that needs no gradient launches no input-gradient conv, frozen ``.0`` parameters launch no weight-gradient
    kernel.

    ``slot_heads=True`` and ``forward(feat, ind)`` with ``ind`` = ``batch['ind']`` (int64 [B,M], y * W + x): the heads of
    ``SLOT_HEADS`` are evaluated at those cells only and return ``[B, M, c]`` -- the reference's
    ``_tranpose_and_gather_feat(output, ind)`` -- with a zero row for an ``ind`` outside ``[0, H*W)``, whose incoming gradient
    is ignored; slots are evaluated whatever their mask.  Every other head is a dense map as before, from a launch that holds
    only those heads.  Without ``ind`` the call is the dense one, bit for bit; parameters and ``state_dict`` do not depend on
    the flag."""

    def __init__(self, heads, head_conv=256, in_channels=64, prior_bias=-4.6, slot_heads=False):
        super().__init__()
        self.slot_heads = bool(slot_heads)
        self.heads = OrderedDict(heads)
        self.head_conv = _one_head_conv(head_conv, self.heads)
        self.in_channels = in_channels
        if not self.heads or len(self.heads) > _lib.CT_LOSS_MAX_HEADS:
            raise _lib.CTError('FusedHeads takes 1 .. %d heads (got %d)' % (_lib.CT_LOSS_MAX_HEADS, len(self.heads)))
        if in_channels % 16:
            raise _lib.CTError('FusedHeads needs in_channels %% 16 == 0 (got %d)' % in_channels)
        for h, c in self.heads.items():
            # containers of the parameters only (never called): the reference's module tree, so names and default
            # initialisation are torch's own
            fc = nn.Sequential(nn.Conv2d(in_channels, self.head_conv, 3, padding=1, bias=True), nn.ReLU(inplace=True),
                               nn.Conv2d(self.head_conv, c, 1, bias=True))
            if 'hm' in h:
                fc[-1].bias.data.fill_(prior_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d) and m.bias is not None:
                        nn.init.constant_(m.bias, 0)
            self.add_module(h, fc)

    def head_parameters(self, h):
        fc = getattr(self, h)
        return fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias

    def _check_input(self, t, cin):
        """``t``: the 4-d tensor behind the input, ``cin``: the input's channel count"""
        need_cuda(t, 'FusedHeads', dims=None)
        if cin != self.in_channels:
            raise _lib.CTError('FusedHeads was built for %d input channels (got %d)' % (self.in_channels, cin))

    def slot_head_names(self):
        """the heads that are evaluated at the slots when the module is called with ``ind``"""
        return tuple(h for h in self.heads if h in SLOT_HEADS) if self.slot_heads else ()

    def _slot_call(self, nhwc, feat, ind, params):
        if not torch.is_tensor(ind) or not ind.is_cuda:
            raise _lib.CTError('FusedHeads runs on an MI355X only (ind is not a CUDA tensor); no CPU fallback')
        outs = _SlotHeadsFunction.apply(tuple(self.heads), self.slot_head_names(), nhwc, feat, ind, *params)
        return OrderedDict(zip(self.heads, outs))

    def forward(self, feat, ind=None):
        if isinstance(feat, ops.View):
            self._check_input(feat.buf, feat.C)
        elif torch.is_tensor(feat) and feat.dim() == 4:
            self._check_input(feat, feat.shape[1])
        else:
            raise _lib.CTError('FusedHeads takes an NCHW tensor or an ops.View')
        params = [t for h in self.heads for t in self.head_parameters(h)]
        if ind is not None and self.slot_head_names():
            return self._slot_call(False, feat, ind, params)
        outs = _HeadsFunction.apply(tuple(self.heads), feat, *params)
        return OrderedDict(zip(self.heads, outs))

    def forward_nhwc(self, feat, ind=None):
        """``feat``: an ``[N,H,W,in_channels]`` fp32 CUDA tensor (the layout of every trainable module's ``forward_nhwc``),
        part of the autograd graph -> the same ``OrderedDict`` of NCHW logits, the same bits as ``forward`` on the NCHW
        form of ``feat``; the input gradient is NHWC.  ``ind``: as in ``forward``."""
        if not torch.is_tensor(feat) or feat.dim() != 4:
            raise _lib.CTError('FusedHeads.forward_nhwc takes an [N,H,W,C] tensor')
        self._check_input(feat, feat.shape[3])
        params = [t for h in self.heads for t in self.head_parameters(h)]
        if ind is not None and self.slot_head_names():
            return self._slot_call(True, feat.contiguous(), ind, params)
        outs = _HeadsNHWCFunction.apply(tuple(self.heads), feat.contiguous(), *params)
        return OrderedDict(zip(self.heads, outs))


class HeadFinetuner(nn.Module):
    """Fine-tuning of the heads of a ``DLASegHIP`` on its frozen trunk -- the workflow of the reference's ``load_model``
    with ``reset_hm`` / ``reuse_hm`` or a new class count (model.py:49-63).  The trunk runs under ``no_grad`` on the
    inference kernels up to the 64-channel feature map; the heads are a ``FusedHeads`` initialised from the model's current
    head tensors.  ``parameters()`` yields the head parameters only; the model's own inference path does not change until
    ``commit()`` writes them back."""

    def __init__(self, model, slot_heads=False):
        super().__init__()
        self.model = model
        dev = next(model.buffers()).device
        self.heads = FusedHeads(model.heads, model.head_conv, slot_heads=slot_heads).to(dev)
        sd = model.state_dict()
        self.heads.load_state_dict(OrderedDict((k, sd[k]) for k in self.heads.state_dict()))

    slot_heads = property(lambda self: self.heads.slot_heads)

    def forward(self, x, pre_img=None, pre_hm=None, ind=None):
        """the reference's signature (base_model.py:73): ``[{head: raw logits with a grad_fn}]``; ``ind``: ``batch['ind']`` for
        a fine-tuner built with ``slot_heads=True`` (``FusedHeads.forward``)"""
        m = self.model
        if pre_img is not None and not m.pre_img:
            raise _lib.CTError('model was built with pre_img=False')
        if pre_hm is not None and not m.pre_hm:
            raise _lib.CTError('model was built with pre_hm=False')
        N, _, H, W = x.shape
        with torch.no_grad():
            plan = m.get_plan(N, H, W, pre_img is not None, pre_hm is not None, trunk_only=True)
            m.forward_plan(plan, x, pre_img, pre_hm)
        z = self.heads(plan['feat'], ind)
        if m.model_output_list:
            return [[z[h] for h in sorted(m.heads)]]
        return [z]

    @torch.no_grad()
    def commit(self):
        """write the head parameters back into the model's buffers: the next inference forward, a ``Detector`` built
        afterwards and the model's ``state_dict()`` see them"""
        for k, v in self.heads.state_dict().items():
            getattr(self.model, k.replace('.', '__')).copy_(v)
        self.model._prepared = None
        self.model._plans = {}

    def state_dict(self, *a, **k):
        """the full reference-format dict: trunk buffers + the current head parameters"""
        sd = self.model.state_dict()
        own = self.heads.state_dict()
        return OrderedDict((n, own[n].detach() if n in own else v) for n, v in sd.items())

    def load_state_dict(self, sd, strict=True):
        own = self.heads.state_dict()
        res = self.model.load_state_dict(sd, strict=strict)
        self.heads.load_state_dict(OrderedDict((n, sd[n]) for n in own if n in sd), strict=strict)
        return res
