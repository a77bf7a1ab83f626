"""``DLASeg``: the reference's user-visible training module (``model/networks/dla.py:594-640`` on ``BaseModel``,
``base_model.py:14-91``) on the kernels of libcentertrack_hip.so -- ``DLASeg(num_layers, heads, head_convs, opt)`` with the
reference's constructor, calling convention (``forward(x, pre_img=None, pre_hm=None)`` -> ``[{head: NCHW logits}]``, or
``[[logits in sorted(heads) order]]`` with ``opt.model_output_list``), state-dict keys and shapes (``base.*``, ``dla_up.*``,
``ida_up.*`` and ``<head>.0.*`` / ``<head>.2.*`` at top level: a reference checkpoint's ``state_dict`` loads as it is) and
initialisation.  The inference counterpart is ``model.DLASegHIP``.

Inside, everything is NHWC: NCHW images -> the stems -> ``DLA.forward_nhwc`` -> ``DLAUp.forward_nhwc`` -> ``IDAUp.forward_nhwc``
-> ``FusedHeads.forward_nhwc``; the only layout conversions of a step are the ones the NCHW logits already have (the 1x1 head
convs write NCHW).  The trunk records a graph under ``dcn_v2.trainable()`` with autograd enabled, as every trainable module
does; the heads record, as ``FusedHeads`` always has, whenever autograd is enabled.

Covered: ``num_layers == 34``, ``opt.dla_node == 'dcn'``, ``opt.head_kernel == 3``, one head-conv layer of one width; anything
else raises ``CTError``.  Nothing is downloaded: the base is always built with ``pretrained=False``, whatever
``opt.load_model`` says (the reference downloads the ImageNet weights when it is ``''``); load them from a local file with
``model.base.load_pretrained_model`` or ``load_state_dict``.  CUDA fp32 tensors only: there is no CPU fallback.

Slot heads (``opt.slot_heads``, ``heads.FusedHeads``): the CALL takes ``batch['ind']`` as a fourth argument, ``model(x, pre_img,
pre_hm, ind)``, and then returns the heads of ``heads.SLOT_HEADS`` at the slots, ``[B, M, c]``.  ``forward`` itself keeps the
reference's three parameters.
"""
import numpy as np

from . import _lib, dla_base
from .dla_up import DeformConv, DLAUp, IDAUp
from .heads import FusedHeads

DLA_NODE = {'dcn': (DeformConv, DeformConv)}


class DLASeg(FusedHeads):
    """Reference ``DLASeg(num_layers, heads, head_convs, opt)``.  ``opt`` is read for ``dla_node``, ``head_kernel``,
    ``prior_bias``, ``model_output_list``, ``pre_img``, ``pre_hm`` and ``slot_heads`` (default False: with it, ``model(x, pre_img,
    pre_hm, ind)`` with ``ind`` = ``batch['ind']`` returns the heads of ``heads.SLOT_HEADS`` at the slots, ``[B, M, c]``;
    ``FusedHeads``)."""

    def __init__(self, num_layers, heads, head_convs, opt):
        if num_layers != 34:
            raise _lib.CTError('centertrack_amd DLASeg covers DLA-34 only (got num_layers=%r)' % (num_layers,))
        node = getattr(opt, 'dla_node', 'dcn')
        if node not in DLA_NODE:
            raise _lib.CTError('centertrack_amd DLASeg supports dla_node dcn only (got %r)' % (node,))
        if getattr(opt, 'head_kernel', 3) != 3:
            raise _lib.CTError('centertrack_amd DLASeg supports head_kernel 3 only (got %r)' % (opt.head_kernel,))
        super().__init__(heads, head_convs, 64, prior_bias=getattr(opt, 'prior_bias', -4.6),
                         slot_heads=bool(getattr(opt, 'slot_heads', False)))
        self.num_stacks = 1
        self._slot_ind = None
        self.opt = opt
        self.node_type = DLA_NODE[node]
        down_ratio = 4
        self.first_level = int(np.log2(down_ratio))
        self.last_level = 5
        self.base = dla_base.dla34(pretrained=False, opt=opt)
        channels = self.base.channels
        scales = [2 ** i for i in range(len(channels[self.first_level:]))]
        self.dla_up = DLAUp(self.first_level, channels[self.first_level:], scales, node_type=self.node_type)
        out_channel = channels[self.first_level]
        self.ida_up = IDAUp(out_channel, channels[self.first_level:self.last_level],
                            [2 ** i for i in range(self.last_level - self.first_level)], node_type=self.node_type)

    def feats_nhwc(self, x, pre_img=None, pre_hm=None):
        """the 64-channel feature map as an ``[N,H/4,W/4,64]`` tensor"""
        layers = self.dla_up.forward_nhwc(self.base.forward_nhwc(x, pre_img, pre_hm))
        # the reference clones the levels it hands to ida_up, which rewrites its list: here the list is rewritten, the tensors
        # (autograd values) are not, so a new list is enough
        y = [layers[i] for i in range(self.last_level - self.first_level)]
        self.ida_up.forward_nhwc(y, 0, len(y))
        return y[-1]

    def img2feats(self, x):
        return [dla_base.to_nchw(self.feats_nhwc(x))]

    def imgpre2feats(self, x, pre_img=None, pre_hm=None):
        return [dla_base.to_nchw(self.feats_nhwc(x, pre_img, pre_hm))]

    def __call__(self, x, pre_img=None, pre_hm=None, ind=None):
        """the reference's call with ``batch['ind']`` as an optional fourth argument (slot heads).  ``forward`` has the
        reference's signature, so ``ind`` reaches it through the instance, for the length of this call; hooks run as usual."""
        self._slot_ind = ind
        try:
            return super().__call__(x, pre_img, pre_hm)
        finally:
            self._slot_ind = None

    def forward(self, x, pre_img=None, pre_hm=None):
        feat = self.feats_nhwc(x, pre_img, pre_hm)
        z = self.forward_nhwc(feat) if self._slot_ind is None else self.forward_nhwc(feat, self._slot_ind)
        if getattr(self.opt, 'model_output_list', False):
            return [[z[head] for head in sorted(self.heads)]]
        return [dict(z)]
