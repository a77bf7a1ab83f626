"""Drop-in for the reference's training loss (``trainer.GenericLoss``, src/lib/trainer.py:20-86, and the classes of
src/lib/model/losses.py) on the fused HIP kernels of csrc/loss.hip.

``GenericLoss(opt)(outputs, batch) -> (tot, loss_stats)`` as the reference's.  All heads of a stack go through ONE
autograd function: two launches forward, three backward, whatever the number of heads, no host synchronisation, no
atomics; losses and gradients are bitwise equal from run to run.

Differences from the reference, all deliberate:

* The kernels read the RAW head outputs.  The reference first overwrites ``output['hm']``, ``['hm_hp']`` and ``['dep']``
  with their sigmoid-ed / inverted values (``_sigmoid_output``); here ``outputs`` is left alone unless
  ``sigmoid_outputs=True`` asks for those (detached) values afterwards, as ``Trainer.debug`` expects them.
* ``FastFocalLoss``, ``RegWeightedL1Loss``, ``WeightedBCELoss`` and ``BinRotLoss`` have the reference's call signatures
  but take the raw logits where the reference takes the already transformed map: ``FastFocalLoss`` applies
  ``clamp(sigmoid(x), 1e-4, 1 - 1e-4)`` itself, and ``RegWeightedL1Loss(depth=True)`` applies ``1 / (sigmoid(x) + 1e-6) - 1``.
* A slot whose ``ind`` is outside ``[0, H*W)`` or whose ``cat`` is outside ``[0, C)`` makes the reference raise (an index
  error, i.e. a host synchronisation).  Here it counts as a slot with mask 0 (``rot``: mask 0 and rotbin 0): it reads and
  writes nothing.
* A 3-d entry ``[B,M,c]`` of ``outputs[s]`` is a slot head (``heads.FusedHeads`` with ``slot_heads``: the head evaluated at
  ``batch['ind']`` only).  The slot heads of a stack are a second group of the same kernels, presented as maps ``[B,c,1,M]``
  in which slot m reads cell m; an ``ind`` outside ``[0, H*W)`` of the stack's dense ``hm`` becomes the index -1, so the rule
  above holds in both modes.  A stack with slot heads and no dense ``hm`` raises ``CTError``.

CUDA tensors only: a CPU tensor raises ``CTError``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import CT_LOSS_BCE, CT_LOSS_FOCAL, CT_LOSS_L1, CT_LOSS_L1_DEPTH, CT_LOSS_ROT

L1_HEADS = ('reg', 'wh', 'tracking', 'ltrb', 'ltrb_amodal', 'hps', 'dim', 'amodel_offset', 'velocity', 'hp_offset')
KNOWN_HEADS = ('hm', 'hm_hp', 'dep', 'rot', 'nuscenes_att') + L1_HEADS


def _cuda(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.CTError('centertrack_amd.losses runs on an MI355X only (%s is a %s tensor); no CPU fallback'
                           % (what, t.device if torch.is_tensor(t) else type(t).__name__))
    return t


def _f32(t, what):
    return _cuda(t, what).detach().float().contiguous()


def _i64(t, what):
    return _cuda(t, what).detach().long().contiguous()


def head_spec(kind, x, target, mask, ind, cat=None, name='head'):
    """One entry of ``ops.make_loss_desc``: everything made contiguous fp32 / int64, the mask broadcast to the shape the
    kernel reads ([B,M] for focal and rot heads, [B,M,C] for the others).  ``x`` keeps its autograd history."""
    _cuda(x, name)
    if x.dim() != 4:
        raise _lib.CTError('%s: a head output is [B,C,H,W], got %s' % (name, tuple(x.shape)))
    x = x.float().contiguous()
    B, C = x.shape[:2]
    ind = _i64(ind, name + ' ind').view(B, -1)
    M = ind.shape[1]
    mask = _f32(mask, name + ' mask')
    if kind in (CT_LOSS_FOCAL, CT_LOSS_ROT):
        mask = mask.reshape(B, M)
        cat = _i64(cat, name + ' cat')
        target = _f32(target, name + ' target')
    else:
        target = _f32(target, name + ' target').reshape(B, M, C)
        mask = mask.reshape(B, M, -1).expand(B, M, C).contiguous()
    return (kind, x, target, mask, ind, cat)


class _GenericLossFunction(torch.autograd.Function):
    """(heads without their logits, *logits) -> the per-head loss vector"""

    @staticmethod
    def forward(ctx, rest, *xs):
        heads = [(r[0], x.detach()) + tuple(r[1:]) for r, x in zip(rest, xs)]
        loss = ops.generic_loss_forward(heads)
        if any(ctx.needs_input_grad[1:]):
            ctx.rest = rest
            ctx.save_for_backward(*xs)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        heads = [(r[0], x) + tuple(r[1:]) for r, x in zip(ctx.rest, ctx.saved_tensors)]
        grads = ops.generic_loss_backward(heads, grad_loss, ctx.needs_input_grad[1:])
        return (None,) + tuple(grads)


def fused_losses(specs):
    """the per-head loss vector of ``head_spec`` entries, differentiable in their logits"""
    return _GenericLossFunction.apply([(s[0],) + tuple(s[2:]) for s in specs], *[s[1] for s in specs])


class GenericLoss(nn.Module):
    """``trainer.GenericLoss``: reads ``opt.heads``, ``opt.weights`` and ``opt.num_stacks``."""

    def __init__(self, opt, sigmoid_outputs=False):
        super().__init__()
        self.opt = opt
        self.sigmoid_outputs = sigmoid_outputs

    @staticmethod
    def _spec(head, output, batch):
        x = output[head]
        if head == 'hm':
            return head_spec(CT_LOSS_FOCAL, x, batch['hm'], batch['mask'], batch['ind'], batch['cat'], head)
        if head == 'hm_hp':
            return head_spec(CT_LOSS_FOCAL, x, batch['hm_hp'], batch['hm_hp_mask'], batch['hp_ind'], batch['joint'], head)
        if head == 'rot':
            return head_spec(CT_LOSS_ROT, x, batch['rotres'], batch['rot_mask'], batch['ind'], batch['rotbin'], head)
        ind = batch['hp_ind'] if head == 'hp_offset' else batch['ind']
        kind = CT_LOSS_L1_DEPTH if head == 'dep' else CT_LOSS_BCE if head == 'nuscenes_att' else CT_LOSS_L1
        return head_spec(kind, x, batch[head], batch[head + '_mask'], ind, None, head)

    @staticmethod
    def _slot_view(group, output, batch):
        """The slot heads ``group`` of a stack as the kernels read them -> (outputs, batch): each ``[B,M,c]`` output is the map
        ``[B,c,1,M]`` (the layout ``FusedHeads`` wrote it in: no copy) and slot m reads cell m of it.  A slot whose ``ind`` is
        outside ``[0, H*W)`` of the stack's dense ``hm`` gets the index -1, which the kernels count as mask 0 (``rot``: and
        rotbin 0): it reads and writes nothing, as in dense mode."""
        dense_only = [h for h in group if h in ('hm', 'hm_hp', 'hp_offset')]
        if dense_only:
            raise _lib.CTError('GenericLoss: %s cannot be slot heads: they are not read at batch[\'ind\']' % (dense_only,))
        hm = output.get('hm')
        if not torch.is_tensor(hm) or hm.dim() != 4:
            raise _lib.CTError('GenericLoss: slot heads %s without a dense hm map in the stack: the range of ind is unknown'
                               % (group,))
        ind = _i64(batch['ind'], 'ind').view(hm.shape[0], -1)
        M = ind.shape[1]
        valid = (ind >= 0) & (ind < hm.shape[2] * hm.shape[3])
        proxy = torch.where(valid, torch.arange(M, device=ind.device).expand_as(ind), torch.full_like(ind, -1))
        maps = {}
        for h in group:
            x = _cuda(output[h], h)
            if x.shape[:2] != ind.shape:
                raise _lib.CTError('GenericLoss: slot head %s is %s for ind %s' % (h, tuple(x.shape), tuple(ind.shape)))
            maps[h] = x.transpose(1, 2).unsqueeze(2)
        return maps, dict(batch, ind=proxy)

    def forward(self, outputs, batch):
        opt = self.opt
        losses = {head: 0 for head in opt.heads}
        for s in range(opt.num_stacks):
            output = outputs[s]
            # (as the reference: hp_offset is computed only next to hm_hp, trainer.py:63-70,
            # and a head of opt.heads it has no loss for stays 0 in loss_stats and in tot)
            names = [h for h in opt.heads
                     if h in KNOWN_HEADS and h in output and (h != 'hp_offset' or 'hm_hp' in output)]
            # a 3-d entry [B,M,c] is a slot head (heads.FusedHeads with slot_heads): the stack's second group
            for group in ([h for h in names if output[h].dim() != 3], [h for h in names if output[h].dim() == 3]):
                if not group:
                    continue
                src = (output, batch) if output[group[0]].dim() != 3 else self._slot_view(group, output, batch)
                vec = fused_losses([self._spec(h, *src) for h in group])
                for i, h in enumerate(group):
                    losses[h] = losses[h] + vec[i] / opt.num_stacks
            if self.sigmoid_outputs:
                with torch.no_grad():
                    for h in ('hm', 'hm_hp'):
                        if h in output:
                            output[h] = torch.clamp(output[h].detach().sigmoid(), min=1e-4, max=1 - 1e-4)
                    if 'dep' in output:
                        output['dep'] = 1. / (output['dep'].detach().sigmoid() + 1e-6) - 1.
        losses['tot'] = 0
        for head in opt.heads:
            losses['tot'] = losses['tot'] + opt.weights[head] * losses[head]
        return losses['tot'], losses


class FastFocalLoss(nn.Module):
    """``forward(out, target, ind, mask, cat)`` with ``out`` the RAW heat-map logits [B,C,H,W] (the reference takes
    ``clamp(sigmoid(out), 1e-4, 1 - 1e-4)``)."""

    def __init__(self, opt=None):
        super().__init__()

    def forward(self, out, target, ind, mask, cat):
        return fused_losses([head_spec(CT_LOSS_FOCAL, out, target, mask, ind, cat, 'FastFocalLoss')])[0]


class RegWeightedL1Loss(nn.Module):
    """``forward(output, mask, ind, target)`` on the raw head output.  ``depth=True``: the loss of the ``dep`` head, which
    applies ``1 / (sigmoid(x) + 1e-6) - 1`` itself (the reference takes the transformed map)."""

    def __init__(self, depth=False):
        super().__init__()
        self.kind = CT_LOSS_L1_DEPTH if depth else CT_LOSS_L1

    def forward(self, output, mask, ind, target):
        return fused_losses([head_spec(self.kind, output, target, mask, ind, None, 'RegWeightedL1Loss')])[0]


class WeightedBCELoss(nn.Module):
    """``forward(output, mask, ind, target)``: logits in, as the reference's (BCE-with-logits)."""

    def forward(self, output, mask, ind, target):
        return fused_losses([head_spec(CT_LOSS_BCE, output, target, mask, ind, None, 'WeightedBCELoss')])[0]


class BinRotLoss(nn.Module):
    """``forward(output, mask, ind, rotbin, rotres)`` on the raw [B,8,H,W] head output, as the reference's."""

    def forward(self, output, mask, ind, rotbin, rotres):
        return fused_losses([head_spec(CT_LOSS_ROT, output, rotres, mask, ind, rotbin, 'BinRotLoss')])[0]
