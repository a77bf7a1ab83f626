"""Tensor-level wrappers over the C ABI (torch is only the allocator / stream owner).

``View`` = an NHWC fp32 activation living in (a channel slice of) a contiguous
``[N,H,W,ld]`` buffer; every op reads / writes views so concatenations
(reference ``Root.forward``, dla.py:164-166) never copy."""
import ctypes

import numpy as np
import torch

from . import _lib, _train          # (_train imports this module in turn: each reads the other at call time only)
from ._lib import CT_OUT_NCHW, CT_RELU, ConvDesc, DcnBwdDesc, DcnDesc, DecodeDesc


class View(object):
    __slots__ = ('buf', 'c0', 'C')

    def __init__(self, buf, c0=0, C=None):
        assert buf.dim() == 4 and buf.is_contiguous() and buf.dtype == torch.float32
        self.buf = buf
        self.c0 = c0
        self.C = buf.shape[3] - c0 if C is None else C
        assert 0 <= c0 and c0 + self.C <= buf.shape[3]

    N = property(lambda s: s.buf.shape[0])
    H = property(lambda s: s.buf.shape[1])
    W = property(lambda s: s.buf.shape[2])
    ld = property(lambda s: s.buf.shape[3])
    ptr = property(lambda s: s.buf.data_ptr() + 4 * s.c0)

    def slice(self, c0, C):
        return View(self.buf, self.c0 + c0, C)

    def to_nchw(self):
        """torch view (no copy) of the slice as [N,C,H,W] -- for tests / debugging."""
        return self.buf[..., self.c0:self.c0 + self.C].permute(0, 3, 1, 2)


def new_view(N, H, W, C, device, ld=None):
    return View(torch.empty((N, H, W, ld or C), dtype=torch.float32, device=device), 0, C)


def view_from_nchw(x):
    """NCHW torch tensor -> fresh NHWC view via the HIP converter."""
    N, C, H, W = x.shape
    x = x.contiguous().float()
    ld = (C + 3) // 4 * 4
    v = View(torch.zeros((N, H, W, ld), dtype=torch.float32, device=x.device), 0, C)
    _lib.check(_lib.load().ct_nchw_to_nhwc(x.data_ptr(), N, C, H, W, v.ptr, v.ld, _lib.stream_ptr()),
               'ct_nchw_to_nhwc')
    return v


def view_to_nchw(v):
    out = torch.empty((v.N, v.C, v.H, v.W), dtype=torch.float32, device=v.buf.device)
    _lib.check(_lib.load().ct_nhwc_to_nchw(v.ptr, v.N, v.C, v.H, v.W, v.ld, out.data_ptr(), _lib.stream_ptr()),
               'ct_nhwc_to_nchw')
    return out


def _pack(entry, elems, w, *dims, what=None):
    """The OIHW weight ``w`` in the layout ``entry`` (a ``ct_pack_*``) writes: ``elems`` (its ``ct_packed_*_elems``) and
    ``entry`` both take ``dims``.  ``what``: the refusal of a shape for which ``elems`` answers 0."""
    lib = _lib.load()
    w = w.contiguous().float()
    n = getattr(lib, elems)(*dims)
    if what is not None and not n:
        raise _lib.CTError(what)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    _lib.check(getattr(lib, entry)(w.data_ptr(), out.data_ptr(), *dims, _lib.stream_ptr()), entry)
    return out


def pack_weight(w):
    """OIHW conv weight (cuda, fp32) -> MFMA fragment layout (see centertrack_hip.h)."""
    Cout, Cin, ks, ks2 = w.shape
    assert ks == ks2 and Cin % 16 == 0, 'Cin must be a multiple of 16'
    return _pack('ct_pack_conv_weight', 'ct_packed_weight_elems', w, Cout, Cin, ks)


def pack_winograd(w):
    """OIHW 3x3 conv weight -> Winograd F(2x2,3x3) fragments (ct_conv2d algo 201 / 202)"""
    Cout, Cin, ks, ks2 = w.shape
    assert ks == 3 and ks2 == 3 and Cin % 16 == 0
    return _pack('ct_pack_winograd_weight', 'ct_packed_winograd_elems', w, Cout, Cin)


def _p(t):
    return None if t is None else t.data_ptr()


def make_conv_desc(x, wp, Cout, ks, stride=1, scale=None, shift=None, res=None, relu=False, out=None,
                   out_nchw=None, sig=(0, 0), dep=(0, 0), depth_scale=1.0, workspace=None, split_k=0, algo=0,
                   w_wino=None, pool=None, proj=None):
    """``pool``: NHWC view [N, H/2, W/2, Cin] that receives the 2x2 max-pool of ``x`` as a side output (3x3 stride-2);
    ``proj`` = (packed [Cout, Cin, 1, 1] weight, scale, shift, NHWC output view): Tree.project of the pooled input
    (conv1x1 + BN, no ReLU) as a second output of the same launch"""
    d = ConvDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = x.ptr, x.N, x.H, x.W, x.C, x.ld
    d.w_packed, d.Cout, d.ks, d.stride = wp.data_ptr(), Cout, ks, stride
    d.scale, d.shift = _p(scale), _p(shift)
    if res is not None:
        d.res, d.ldr = res.ptr, res.ld
    flags = CT_RELU if relu else 0
    if out_nchw is not None:
        assert out is None and out_nchw.is_contiguous()
        d.y, d.ldy = out_nchw.data_ptr(), 0
        flags |= CT_OUT_NCHW
    else:
        d.y, d.ldy = out.ptr, out.ld
    d.flags = flags
    d.sig_lo, d.sig_hi = sig
    d.dep_lo, d.dep_hi = dep
    d.depth_scale = depth_scale
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.split_k = split_k
    d.algo = algo
    if w_wino is not None:
        d.w_winograd = w_wino.data_ptr()
    if pool is not None:
        assert ks == 3 and stride == 2 and (pool.N, pool.H, pool.W, pool.C) == (x.N, x.H // 2, x.W // 2, x.C)
        d.pool_y, d.pool_ld = pool.ptr, pool.ld
    if proj is not None:
        pw, psc, psh, py = proj
        assert ks == 3 and stride == 2 and (py.N, py.H, py.W, py.C) == (x.N, x.H // 2, x.W // 2, Cout)
        d.proj_w_packed, d.proj_scale, d.proj_shift = pw.data_ptr(), _p(psc), _p(psh)
        d.proj_y, d.proj_ldy = py.ptr, py.ld
    return d


def conv2d(x, wp, Cout, ks, stride=1, out=None, **kw):
    """y = act(conv(x) * scale + shift + res); allocates the output view if not given."""
    lib = _lib.load()
    pad = ks // 2
    Ho = (x.H + 2 * pad - ks) // stride + 1
    Wo = (x.W + 2 * pad - ks) // stride + 1
    if out is None and kw.get('out_nchw') is None:
        out = new_view(x.N, Ho, Wo, Cout, x.buf.device, ld=(Cout + 3) // 4 * 4)
    d = make_conv_desc(x, wp, Cout, ks, stride, out=out, **kw)
    if d.workspace is None and kw.get('split_k', 0) != 1:
        _ws = _workspace(lib, 'ct_conv2d_workspace_bytes', d, x.buf.device, optional=True)
    _lib.check(lib.ct_conv2d(ctypes.byref(d), _lib.stream_ptr()), 'ct_conv2d')
    return out if out is not None else kw['out_nchw']


def make_dcn_desc(x, om, wp, Cout, scale, shift, relu, out, workspace=None, split_k=0, algo=0, w_off=None,
                  b_off=None, up=None, om_partial=None, raw_offsets=False, w_off_wino=None):
    """``w_off`` (packed conv_offset_mask weight) + ``b_off`` given: the offset/mask conv runs inside the DCN
    launch (``om`` may be None) -- or, with ``om_partial`` (a float buffer of ct_dcn_v2_offsets_bytes), K-split by
    the CT_DCN_OFFSETS launch; otherwise ``om`` is the precomputed NHWC offset/mask map."""
    d = DcnDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = x.ptr, x.N, x.H, x.W, x.C, x.ld
    if om is not None:
        d.om, d.ldom = om.ptr, om.ld
    if w_off is not None or raw_offsets:             # (raw sums from another launch need b_off only)
        d.fuse_offset, d.b_off = 1, b_off.data_ptr()
        if w_off is not None:
            d.w_off_packed = w_off.data_ptr()
        if om_partial is not None:
            d.fuse_offset = 3 if raw_offsets else 2          # (3: another launch writes the raw sums into om_partial)
            d.om_partial, d.om_partial_bytes = om_partial.data_ptr(), om_partial.numel() * om_partial.element_size()
            if w_off_wino is not None and not raw_offsets:    # (the OFFSETS launch runs this layer's chunks as Winograd tiles)
                d.w_off_winograd = w_off_wino.data_ptr()
    if up is not None:                 # (upsample_weight [4f^2,C], f, skip view, output view): fused IDAUp step
        w_up, f, skip, up_out = up
        d.up_w, d.up_f, d.up_skip, d.up_lds = w_up.data_ptr(), f, skip.ptr, skip.ld
        d.up_y, d.up_ldy = up_out.ptr, up_out.ld
    d.w_packed, d.Cout = wp.data_ptr(), Cout
    d.scale, d.shift = _p(scale), _p(shift)
    d.y, d.ldy = out.ptr, out.ld
    d.flags = CT_RELU if relu else 0
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.split_k = split_k
    d.algo = algo
    return d


def dcn_v2(x, om, wp, Cout, scale=None, shift=None, relu=False, out=None, split_k=0, algo=0, w_off=None, b_off=None,
           up=None, split_offsets=False, w_off_wino=None):
    lib = _lib.load()
    if out is None:
        out = new_view(x.N, x.H, x.W, Cout, x.buf.device)
    part = None
    if split_offsets:
        part = torch.empty((x.C // 64) * x.N * x.H * x.W * 32, dtype=torch.float32, device=x.buf.device)
    d = make_dcn_desc(x, om, wp, Cout, scale, shift, relu, out, split_k=split_k, algo=algo, w_off=w_off, b_off=b_off,
                      up=up, om_partial=part, w_off_wino=w_off_wino if split_offsets else None)
    if split_k != 1:
        _ws = _workspace(lib, 'ct_dcn_v2_workspace_bytes', d, x.buf.device, optional=True)
    _lib.check(lib.ct_dcn_v2(ctypes.byref(d), _lib.stream_ptr()), 'ct_dcn_v2')
    return out


def pack_weight_t(w):
    """OIHW 3x3 DCN weight -> the transposed fragment layout ct_dcn_v2_backward contracts gy with (centertrack_hip.h)."""
    Cout, Cin, ks, ks2 = w.shape
    assert ks == 3 and ks2 == 3 and Cin % 16 == 0
    return _pack('ct_pack_dcn_weight_t', 'ct_packed_dcn_weight_t_elems', w, Cout, Cin)


def make_dcn_bwd_desc(x, om, gy, wT=None, gx=None, gom=None, gw=None, gb=None, workspace=None):
    """ct_dcn_bwd_desc over caller-owned buffers; the gradients to compute are the output buffers given (``gb`` rides
    with ``gw``)."""
    d = DcnBwdDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = x.ptr, x.N, x.H, x.W, x.C, x.ld
    d.om, d.ldom = om.ptr, om.ld
    d.gy, d.Cout, d.ldgy = gy.ptr, gy.C, gy.ld
    d.wT_packed = _p(wT)
    flags = 0
    if gx is not None:
        d.gx, d.ldgx = gx.ptr, gx.ld
        flags |= _lib.CT_DCN_BWD_INPUT
    if gom is not None:
        d.gom, d.ldgom = gom.ptr, gom.ld
        flags |= _lib.CT_DCN_BWD_OFFSET_MASK
    if gw is not None:
        d.gw, d.gb = gw.data_ptr(), _p(gb)
        flags |= _lib.CT_DCN_BWD_WEIGHT
    d.flags = flags
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return d


def dcn_v2_backward(x, om, gy, wT=None, need_x=True, need_om=True, need_w=True, need_b=True, gom=None):
    """Gradients of ``dcn_v2(x, om, w) + bias`` for the incoming gradient ``gy`` (NHWC views; ``om`` = the forward's
    offset/mask map, mask after the sigmoid; ``wT`` = pack_weight_t(w), needed for ``need_x`` / ``need_om``).
    Returns ``(gx view, gom view [N,H,W,27 of 32], gw OIHW, gb)``, None for what was not asked for -- no buffer is
    allocated and no kernel runs for those.  ``gx`` is summed with float atomics (equal from run to run only to fp32
    rounding); the other three are bitwise reproducible.  ``gom``: a caller-owned 27-of-32 view for the offset/mask gradient
    (the trainable DeformConv passes a zeroed buffer: its five pad channels feed a 32-channel convolution)."""
    lib = _lib.load()
    dev = x.buf.device
    if not (need_x or need_om or need_w or need_b):
        return None, None, None, None
    if (need_x or need_om) and wT is None:
        raise _lib.CTError('dcn_v2_backward: the input / offset / mask gradients need the transposed weight packing')
    gx = new_view(x.N, x.H, x.W, x.C, dev) if need_x else None
    if not need_om:
        gom = None
    elif gom is None:
        gom = View(torch.empty((x.N, x.H, x.W, 32), dtype=torch.float32, device=dev), 0, 27)
    gw = torch.empty((gy.C, x.C, 3, 3), dtype=torch.float32, device=dev) if need_w or need_b else None
    gb = torch.empty(gy.C, dtype=torch.float32, device=dev) if need_b else None
    d = make_dcn_bwd_desc(x, om, gy, wT, gx, gom, gw, gb)
    _ws = _workspace(lib, 'ct_dcn_v2_backward_workspace_bytes', d, dev, optional=True)
    _lib.check(lib.ct_dcn_v2_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_dcn_v2_backward')
    return gx, gom, (gw if need_w else None), gb


def make_loss_desc(heads, grads=None):
    """``ct_loss_desc`` of ``heads`` = [(kind, logits [B,C,H,W], target, mask, ind, cat or None)], every tensor cuda,
    contiguous, fp32 (ind / cat int64).  Returns (descriptor, keep-alive list)."""
    if not heads:
        raise _lib.CTError('generic_loss: no heads')
    B, _, H, W = heads[0][1].shape
    arr = (_lib.LossHead * len(heads))()
    for i, (kind, x, target, mask, ind, cat) in enumerate(heads):
        for t, dt in ((x, torch.float32), (target, torch.float32), (mask, torch.float32), (ind, torch.int64),
                      (cat, torch.int64)):
            if t is None:
                continue
            if not t.is_cuda:
                raise _lib.CTError('generic_loss runs on an MI355X only (got a %s tensor); no CPU fallback' % t.device)
            if t.dtype != dt or not t.is_contiguous():
                raise _lib.CTError('generic_loss: head %d wants contiguous %s tensors (centertrack_amd.losses prepares them)'
                                   % (i, dt))
        if x.dim() != 4 or x.shape[0] != B or tuple(x.shape[2:]) != (H, W):
            raise _lib.CTError('generic_loss: head %d is %s, the first head [%d, C, %d, %d]' % (i, tuple(x.shape), B, H, W))
        C, M = x.shape[1], ind.numel() // B
        want = {_lib.CT_LOSS_FOCAL: (x.numel(), B * M, B * M), _lib.CT_LOSS_ROT: (B * M * 2, B * M, B * M * 2)}.get(
            kind, (B * M * C, B * M * C, 0))
        if ind.numel() != B * M or (target.numel(), mask.numel(), 0 if cat is None else cat.numel()) != want:
            raise _lib.CTError('generic_loss: head %d (kind %d): target / mask / ind / cat sizes do not fit B=%d M=%d C=%d'
                               % (i, kind, B, M, C))
        h = arr[i]
        h.kind, h.logits, h.C, h.target, h.mask, h.ind, h.cat, h.M = (kind, x.data_ptr(), C, target.data_ptr(), mask.data_ptr(),
                                                                    ind.data_ptr(), _p(cat), M)
        h.grad = _p(grads[i]) if grads is not None else None
    d = _lib.LossDesc()
    d.B, d.H, d.W, d.heads, d.nheads = B, H, W, arr, len(heads)
    return d, arr


def _workspace(lib, query_name, d, dev, optional=False):
    """Allocate what ``query_name`` (a ``ct_*_workspace_bytes``) asks for the descriptor ``d`` and hand it to ``d``; 0 bytes is
    a rejected descriptor or, with ``optional``, "none needed" (-> None).  The caller keeps the returned tensor alive over its
    launch."""
    need = getattr(lib, query_name)(ctypes.byref(d))
    if not need:
        if optional:
            return None
        raise _lib.CTError('%s: %s' % (query_name, lib.ct_last_error().decode()))
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    return ws


def generic_loss_forward(heads):
    """The per-head losses [len(heads)] of one stack (``make_loss_desc`` for ``heads``): two launches, no host sync."""
    lib = _lib.load()
    d, _keep = make_loss_desc(heads)
    dev = heads[0][1].device
    loss = torch.empty(len(heads), dtype=torch.float32, device=dev)
    _ws = _workspace(lib, 'ct_generic_loss_workspace_bytes', d, dev)
    d.loss = loss.data_ptr()
    _lib.check(lib.ct_generic_loss_forward(ctypes.byref(d), _lib.stream_ptr()), 'ct_generic_loss_forward')
    return loss


def generic_loss_backward(heads, grad_loss, needs=None):
    """d(sum_i grad_loss[i] * loss[i]) / d(logits) per head of ``heads``: a list of [B,C,H,W] tensors, None where
    ``needs[i]`` is false (no buffer is allocated for those).  Three launches, bitwise reproducible."""
    lib = _lib.load()
    needs = [True] * len(heads) if needs is None else list(needs)
    if not any(needs):
        return [None] * len(heads)
    grads = [torch.empty_like(h[1]) if n else None for h, n in zip(heads, needs)]
    d, _keep = make_loss_desc(heads, grads)
    dev = heads[0][1].device
    grad_loss = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
    if grad_loss.numel() != len(heads):
        raise _lib.CTError('generic_loss_backward: grad_loss has %d elements for %d heads' % (grad_loss.numel(), len(heads)))
    _ws = _workspace(lib, 'ct_generic_loss_workspace_bytes', d, dev)
    d.grad_loss = grad_loss.data_ptr()
    _lib.check(lib.ct_generic_loss_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_generic_loss_backward')
    return grads


def conv_backward_weight(x, gy, ks, need_bias=True):
    """Weight (and bias) gradient of ``conv(x, w) + b`` (``ks`` 1 or 3, stride 1, pad ks // 2) for the output gradient ``gy``
    (NHWC views) -> ``(gw OIHW [gy.C, x.C, ks, ks], gb [gy.C] or None)``.  Two launches, bitwise reproducible."""
    lib = _lib.load()
    dev = x.buf.device
    if (x.N, x.H, x.W) != (gy.N, gy.H, gy.W):
        raise _lib.CTError('conv_backward_weight: x is %s pixels, gy %s' % ((x.N, x.H, x.W), (gy.N, gy.H, gy.W)))
    d = _lib.ConvBwdWeightDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = x.ptr, x.N, x.H, x.W, x.C, x.ld
    d.gy, d.Cout, d.ldgy = gy.ptr, gy.C, gy.ld
    d.ks, d.stride = ks, 1
    _ws = _workspace(lib, 'ct_conv2d_backward_weight_workspace_bytes', d, dev)
    gw = torch.empty((gy.C, x.C, ks, ks), dtype=torch.float32, device=dev)
    gb = torch.empty(gy.C, dtype=torch.float32, device=dev) if need_bias else None
    d.gw, d.gb = gw.data_ptr(), _p(gb)
    _lib.check(lib.ct_conv2d_backward_weight(ctypes.byref(d), _lib.stream_ptr()), 'ct_conv2d_backward_weight')
    return gw, gb


def conv_backward_input(gy, w, res=None, out=None, ks=None):
    """Input gradient of ``conv(x, w)`` (OIHW ``w``, ``ks`` 1 or 3, stride 1, pad ks // 2) for the output gradient view ``gy``
    (+ ``res``, into ``out`` if given), on the forward conv kernels: ``conv(gy, wt)`` with ``wt[ci, co, ky, kx] =
    w[co, ci, ks - 1 - ky, ks - 1 - kx]``.  ``ks``: what the caller expects ``w`` to be (None: whatever it is).  Those kernels contract multiples of 16 channels: where ``w.shape[0]`` is none (the
    DeformConv's 27 offset/mask channels in a 32-wide buffer), ``gy`` must start its buffer, ``wt`` is zero-padded to ``gy.ld``
    channels and the full width of ``gy.buf`` is contracted -- its pad channels must hold zeros."""
    if ks is not None and tuple(w.shape[2:]) != (ks, ks):
        raise _lib.CTError('conv_backward_input: a %dx%d weight where ks=%d was asked for' % (w.shape[2], w.shape[3], ks))
    Cout, Cin, ks, _ = w.shape
    wt = w.permute(1, 0, 2, 3).flip(2, 3)
    if Cout % 16:
        if gy.c0 or gy.ld % 16:
            raise _lib.CTError('conv_backward_input: %d output channels need a view at the start of a buffer whose width is a '
                               'multiple of 16 (got c0=%d, ld=%d)' % (Cout, gy.c0, gy.ld))
        padded = torch.zeros((Cin, gy.ld, ks, ks), dtype=torch.float32, device=w.device)
        padded[:, :Cout] = wt
        wt, gy = padded, View(gy.buf, 0, gy.ld)
    else:
        wt = wt.contiguous()
    return conv2d(gy, pack_weight(wt), Cin, ks, 1, res=res, out=out)


def _head_tensor(t, what):
    _train.need_cuda(t, what, dims=None)
    return t.detach().contiguous()


def heads_forward_train(feat, w0, b0, w2s, b2s, ks=3):
    """The heads (base_model.py:24-65) with the hidden map kept for a backward: ``feat`` NHWC view [N,H,W,Cin]; ``w0``
    [nheads*hc, Cin, 3, 3] / ``b0`` [nheads*hc] = the heads' first layers concatenated in the order of ``w2s``; ``w2s`` /
    ``b2s`` = {head: [c, hc(, 1, 1)]} / {head: [c]}.  -> (OrderedDict {head: raw logits NCHW [N,c,H,W]}, ``mid`` = the NHWC
    view [N,H,W,nheads*hc] after the ReLU).  The un-fused heads plan of the model: one ct_conv2d into ``mid``, one per
    head into its logits; the weights are packed here, from what their storage holds now.
    ``ks`` = 1: the first layer is a 1x1 convolution, ``w0`` [nheads*hc, Cin, 1, 1] -- the heads at the slots, where ``feat``
    is the gathered map [N,1,M,9*Cin'] of ``slot_gather``."""
    from collections import OrderedDict
    nh = len(w2s)
    w0, b0 = _head_tensor(w0, 'heads_forward_train'), _head_tensor(b0, 'heads_forward_train')
    if nh == 0 or w0.shape[0] % nh or w0.shape[1] != feat.C or tuple(w0.shape[2:]) != (ks, ks) or b0.numel() != w0.shape[0]:
        raise _lib.CTError('heads_forward_train: w0 %s / b0 %s do not fit %d heads on %d channels'
                           % (tuple(w0.shape), tuple(b0.shape), nh, feat.C))
    hc = w0.shape[0] // nh
    dev = feat.buf.device
    mid = new_view(feat.N, feat.H, feat.W, hc * nh, dev)
    conv2d(feat, pack_weight(w0), hc * nh, ks, 1, shift=b0, relu=True, out=mid)
    out = OrderedDict()
    for j, (h, w2) in enumerate(w2s.items()):
        w2, b2 = _head_tensor(w2, 'heads_forward_train'), _head_tensor(b2s[h], 'heads_forward_train')
        c = w2.shape[0]
        if w2.numel() != c * hc or b2.numel() != c:
            raise _lib.CTError('heads_forward_train: head %s: w2 %s / b2 %s with %d hidden channels'
                               % (h, tuple(w2.shape), tuple(b2.shape), hc))
        o = torch.empty((feat.N, c, feat.H, feat.W), dtype=torch.float32, device=dev)
        conv2d(mid.slice(hc * j, hc), pack_weight(w2.reshape(c, hc, 1, 1)), c, 1, 1, shift=b2, out_nchw=o)
        out[h] = o
    return out, mid


def make_heads_tail_desc(mid, gouts, w2s=None, gmid=None, gw2s=None, gb2s=None):
    """``ct_heads_tail_bwd_desc`` over caller-owned buffers: ``gouts`` = [logit gradient NCHW] per head, ``w2s`` = [[c, hc]],
    ``gw2s`` / ``gb2s`` = [buffer or None]; what is computed follows from the output buffers given.  Returns (descriptor,
    keep-alive)."""
    nh = len(gouts)
    arr = (_lib.HeadsTailHead * max(nh, 1))()
    for i, g in enumerate(gouts):
        h = arr[i]
        h.gout, h.c = g.data_ptr(), g.shape[1]
        h.w2 = _p(w2s[i]) if w2s is not None else None
        h.gw2 = _p(gw2s[i]) if gw2s is not None else None
        h.gb2 = _p(gb2s[i]) if gb2s is not None else None
    d = _lib.HeadsTailBwdDesc()
    d.N, d.H, d.W, d.hc = mid.N, mid.H, mid.W, (mid.C // nh if nh else 0)
    d.heads, d.nheads = arr, nh
    d.mid, d.ldmid = mid.ptr, mid.ld
    flags = 0
    if gmid is not None:
        d.gmid, d.ldgmid = gmid.ptr, gmid.ld
        flags |= _lib.CT_HEADS_BWD_HIDDEN
    if (gw2s is not None and any(t is not None for t in gw2s)) or (gb2s is not None and any(t is not None for t in gb2s)):
        flags |= _lib.CT_HEADS_BWD_WEIGHT
    d.flags = flags
    return d, arr


def heads_backward(feat, mid, gouts, w0, w2s, needs, gmid=None, ks=3):
    """Gradients of ``heads_forward_train`` for the logit gradients ``gouts`` = {head: [N,c,H,W]} (every head, in the order
    of ``w2s``).  ``needs`` = {'x', 'w0', 'b0': bool, 'w2', 'b2': bool or {head: bool}}; missing keys are False.  Returns
    {'x': view or None, 'w0': [nheads*hc,Cin,3,3] or None, 'b0', 'w2': {head: [c,hc,1,1] or None}, 'b2': {head: ...},
    'gmid': the hidden gradient's view or None}: no buffer is allocated and no kernel runs for what was not asked for.
    ``gmid``: a caller-owned view for the hidden gradient (any pitch).  ``feat`` may be None when neither 'w0' nor 'b0' is
    needed.  Every result is bitwise reproducible.  ``ks``: the first layer's kernel size (``heads_forward_train``); 'w0' is
    [nheads*hc,Cin,ks,ks]."""
    lib = _lib.load()
    heads = list(w2s)
    nh = len(heads)
    dev = mid.buf.device
    hc = mid.C // nh
    if mid.C != hc * nh or sorted(gouts) != sorted(heads):
        raise _lib.CTError('heads_backward: %d hidden channels / gradients %s for heads %s' % (mid.C, sorted(gouts), heads))

    def per_head(v):
        return {h: bool(v.get(h, False)) for h in heads} if isinstance(v, dict) else {h: bool(v) for h in heads}
    need_x, need_w0, need_b0 = (bool(needs.get(k, False)) for k in ('x', 'w0', 'b0'))
    need_w2, need_b2 = per_head(needs.get('w2', False)), per_head(needs.get('b2', False))
    need_mid = need_x or need_w0 or need_b0
    res = {'x': None, 'w0': None, 'b0': None, 'w2': {h: None for h in heads}, 'b2': {h: None for h in heads}, 'gmid': None}
    g, w2 = [], []
    for h in heads:
        t = _head_tensor(gouts[h], 'heads_backward')
        if t.dim() != 4 or (t.shape[0], t.shape[2], t.shape[3]) != (mid.N, mid.H, mid.W):
            raise _lib.CTError('heads_backward: gradient of %s is %s on a %s map' % (h, tuple(t.shape), (mid.N, mid.H, mid.W)))
        g.append(t)
        w = _head_tensor(w2s[h], 'heads_backward')
        if w.numel() != t.shape[1] * hc:
            raise _lib.CTError('heads_backward: head %s: w2 %s for %d logit and %d hidden channels' % (h, tuple(w.shape), t.shape[1], hc))
        w2.append(w)
    gw2 = [torch.empty((t.shape[1], hc, 1, 1), dtype=torch.float32, device=dev) if need_w2[h] else None for h, t in zip(heads, g)]
    gb2 = [torch.empty(t.shape[1], dtype=torch.float32, device=dev) if need_b2[h] else None for h, t in zip(heads, g)]
    if need_mid:
        if gmid is None:
            gmid = new_view(mid.N, mid.H, mid.W, mid.C, dev)
        elif (gmid.N, gmid.H, gmid.W, gmid.C) != (mid.N, mid.H, mid.W, mid.C):
            raise _lib.CTError('heads_backward: the gmid view does not have the shape of mid')
    else:
        gmid = None
    d, _keep = make_heads_tail_desc(mid, g, w2, gmid, gw2, gb2)
    if d.flags:
        if d.flags & _lib.CT_HEADS_BWD_WEIGHT:
            _ws = _workspace(lib, 'ct_heads_tail_backward_workspace_bytes', d, dev)
        _lib.check(lib.ct_heads_tail_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_heads_tail_backward')
    res['w2'], res['b2'], res['gmid'] = dict(zip(heads, gw2)), dict(zip(heads, gb2)), gmid
    if need_w0 or need_b0:
        gw0, gb0 = conv_backward_weight(feat, gmid, ks, need_bias=need_b0)
        res['w0'], res['b0'] = (gw0 if need_w0 else None), gb0
    if need_x:
        res['x'] = conv_backward_input(gmid, _head_tensor(w0, 'heads_backward'), ks=ks)
    return res


def _slot_desc(what, view, ind, rows):
    """``ct_slot_desc`` of the NHWC view ``view``, ``ind`` int64 [N,M] and the view ``rows`` [N,1,M,9*C]"""
    if not torch.is_tensor(ind) or not ind.is_cuda:
        raise _lib.CTError('%s runs on an MI355X only (ind is not a CUDA tensor); no CPU fallback' % what)
    if ind.dtype != torch.int64 or ind.dim() != 2 or ind.shape[0] != view.N or not ind.is_contiguous():
        raise _lib.CTError('%s: ind must be a contiguous int64 [%d, M] tensor (got %s %s)' % (what, view.N, ind.dtype, tuple(ind.shape)))
    M = ind.shape[1]
    if (rows.N, rows.H, rows.W, rows.C) != (view.N, 1, M, 9 * view.C):
        raise _lib.CTError('%s: the rows are %s for %d slots of %d channels' % (what, (rows.N, rows.H, rows.W, rows.C), M, view.C))
    d = _lib.SlotDesc()
    d.map, d.N, d.H, d.W, d.C, d.ld = view.ptr, view.N, view.H, view.W, view.C, view.ld
    d.ind, d.M = ind.data_ptr(), M
    d.rows, d.ldr = rows.ptr, rows.ld
    return d


def slot_gather(feat, ind, out=None):
    """The im2col rows of a 3x3, pad 1 convolution over the NHWC view ``feat`` at the cells ``ind`` (int64 [N,M], y * W + x) ->
    the view [N,1,M,9*C], ``[n,0,m,(ky*3+kx)*C + c] = feat[n, y+ky-1, x+kx-1, c]``; 0 outside the map, a row of zeros for an
    ``ind`` outside [0, H*W).  One launch, exact."""
    if out is None and torch.is_tensor(ind) and ind.dim() == 2:
        out = new_view(feat.N, 1, ind.shape[1], 9 * feat.C, feat.buf.device)
    d = _slot_desc('slot_gather', feat, ind, out)
    _lib.check(_lib.load().ct_slot_gather(ctypes.byref(d), _lib.stream_ptr()), 'ct_slot_gather')
    return out


def slot_fold(patches, ind, gx):
    """The transpose of ``slot_gather``: adds the view ``patches`` [N,1,M,9*C] into the NHWC view ``gx`` in place (and returns
    it).  No atomics: a cell is written once, by its lowest valid covering slot, as gx + (the covering slots' values added in
    ascending slot order) -- bitwise reproducible; cells no slot covers are not written."""
    d = _slot_desc('slot_fold', gx, ind, patches)
    _lib.check(_lib.load().ct_slot_fold(ctypes.byref(d), _lib.stream_ptr()), 'ct_slot_fold')
    return gx


def stem(x, pre_img, pre_hm, w_x, w_img, w_hm, scale3, shift3, out=None):
    N, _, H, W = x.shape
    if out is None:
        out = new_view(N, H, W, 16, x.device)
    _lib.check(_lib.load().ct_stem_forward(
        x.data_ptr(), _p(pre_img), _p(pre_hm), N, H, W, w_x.data_ptr(), _p(w_img), _p(w_hm),
        scale3.data_ptr(), shift3.data_ptr(), out.ptr, out.ld, _lib.stream_ptr()), 'ct_stem_forward')
    return out


def maxpool2x2(x, out=None):
    if out is None:
        out = new_view(x.N, x.H // 2, x.W // 2, x.C, x.buf.device)
    _lib.check(_lib.load().ct_maxpool2x2(x.ptr, x.N, x.H, x.W, x.C, x.ld, out.ptr, out.ld, _lib.stream_ptr()),
               'ct_maxpool2x2')
    return out


def upsample_weight(w):
    """ConvTranspose2d depth-wise weight [C,1,2f,2f] -> the kernel's [2f,2f,C] layout"""
    return w.reshape(w.shape[0], -1).t().contiguous()


def upsample_add(x, w, f, skip, out=None):
    """w: the module weight [C,1,2f,2f] (transposed here) or an ``upsample_weight`` result [4f^2,C]"""
    if w.dim() == 4:
        w = upsample_weight(w)
    if out is None:
        out = new_view(x.N, x.H * f, x.W * f, x.C, x.buf.device)
    _lib.check(_lib.load().ct_upsample_add(x.ptr, x.N, x.H, x.W, x.C, x.ld, w.data_ptr(), f, skip.ptr, skip.ld,
                                           out.ptr, out.ld, _lib.stream_ptr()), 'ct_upsample_add')
    return out


def _bn_vec(t, C, what):
    if t.numel() != C or t.dtype != torch.float32 or not t.is_contiguous() or t.device != what.buf.device:
        raise _lib.CTError('batch norm: a per-channel vector must be contiguous fp32 [%d] on %s' % (C, what.buf.device))
    return t


def _bn_desc(cls, z, mean, invstd, gamma=None, beta=None, flags=0):
    """a ``ct_bn_desc`` (``_lib.BnDesc``) or ``ct_bn_act_desc`` (``_lib.BnActDesc``) over the map ``z``: the fields the two share"""
    d = cls()
    d.z, d.N, d.H, d.W, d.C, d.ldz = z.ptr, z.N, z.H, z.W, z.C, z.ld
    d.mean, d.invstd, d.gamma, d.beta = (None if t is None else _bn_vec(t, z.C, z).data_ptr() for t in (mean, invstd, gamma, beta))
    d.flags = flags
    return d


def _bn_apply(entry, d, z, out):
    if out is None:
        out = new_view(z.N, z.H, z.W, z.C, z.buf.device)
    d.y, d.ldy = out.ptr, out.ld
    _lib.check(getattr(_lib.load(), entry)(ctypes.byref(d), _lib.stream_ptr()), entry)
    return out


def _bn_backward(entry, query_name, d, z, gy, need_z, need_gamma, need_beta):
    """``gy``, the outputs asked for and, where the call sums, the workspace into ``d``; the call -> (gz, ggamma, gbeta)"""
    lib = _lib.load()
    dev = z.buf.device
    if (gy.N, gy.H, gy.W, gy.C) != (z.N, z.H, z.W, z.C):
        raise _lib.CTError('%s: gy does not have the shape of z' % entry[3:])
    d.gy, d.ldgy = gy.ptr, gy.ld
    gz = new_view(z.N, z.H, z.W, z.C, dev) if need_z else None
    gg = torch.empty(z.C, dtype=torch.float32, device=dev) if need_gamma else None
    gb = torch.empty(z.C, dtype=torch.float32, device=dev) if need_beta else None
    if gz is not None:
        d.gz, d.ldgz = gz.ptr, gz.ld
    d.ggamma, d.gbeta = _p(gg), _p(gb)
    if need_gamma or need_beta or (need_z and d.flags & _lib.CT_BN_BATCH_STATS):
        _ws = _workspace(lib, query_name, d, dev)
    _lib.check(getattr(lib, entry)(ctypes.byref(d), _lib.stream_ptr()), entry)
    return gz, gg, gb


def bn_stats(z, eps=1e-5):
    """Per-channel (mean, biased variance, 1 / sqrt(var + eps)) of the NHWC view ``z`` over N*H*W: two passes (sum, then squared
    deviations), four launches, bitwise reproducible."""
    lib = _lib.load()
    dev = z.buf.device
    mean, var, invstd = (torch.empty(z.C, dtype=torch.float32, device=dev) for _ in range(3))
    d = _bn_desc(_lib.BnDesc, z, mean, invstd)
    d.var, d.eps = var.data_ptr(), eps
    _ws = _workspace(lib, 'ct_bn_workspace_bytes', d, dev)
    _lib.check(lib.ct_bn_stats(ctypes.byref(d), _lib.stream_ptr()), 'ct_bn_stats')
    return mean, var, invstd


def bn_relu_apply(z, mean, invstd, gamma, beta, out=None):
    """y = max(0, fma(z - mean, a, beta)), a = gamma * invstd on NHWC views; allocates ``out`` if not given."""
    return _bn_apply('ct_bn_relu_apply', _bn_desc(_lib.BnDesc, z, mean, invstd, gamma, beta), z, out)


def bn_relu_backward(z, gy, mean, invstd, gamma, beta, batch_stats, need_z=True, need_gamma=True, need_beta=True):
    """Gradients of ``bn_relu_apply`` (with ``batch_stats``: through the batch statistics as well) for the output gradient
    ``gy`` -> ``(gz view, ggamma, gbeta)``, None for what was not asked for.  Bitwise reproducible."""
    if not (need_z or need_gamma or need_beta):
        return None, None, None
    d = _bn_desc(_lib.BnDesc, z, mean, invstd, gamma, beta, _lib.CT_BN_BATCH_STATS if batch_stats else 0)
    return _bn_backward('ct_bn_relu_backward', 'ct_bn_workspace_bytes', d, z, gy, need_z, need_gamma, need_beta)


# ---- synchronised BatchNorm: the statistics as a row to gather, the merge of the gathered rows, and the
# backward in two halves with the all-reduce of the sums between them

def bn_row_floats(C):
    """floats of one rank's row ``[mean[C] | var[C] | resid[C] | pixel count]``: ``mean + resid`` is the mean before its
    rounding to float, the count is a 64-bit integer, stored twice so that the row is a multiple of 16 bytes with every byte
    defined"""
    return 3 * C + 4


def bn_stats_row(z, eps, row):
    """``bn_stats`` written as the row a merge takes: ``row`` is a contiguous fp32 ``[bn_row_floats(C)]``, 16-byte aligned;
    mean and biased variance (the bits of ``bn_stats``) go straight into it, the mean's rounding residual and the pixel count
    N*H*W behind them -> invstd of the local statistics.  Four launches, as ``bn_stats``."""
    lib = _lib.load()
    _bn_vec(row, bn_row_floats(z.C), z)
    invstd = torch.empty(z.C, dtype=torch.float32, device=z.buf.device)
    d = _bn_desc(_lib.BnDesc, z, None, invstd)
    d.eps = eps
    _ws = _workspace(lib, 'ct_bn_workspace_bytes', d, z.buf.device)
    _lib.check(lib.ct_bn_stats_row(ctypes.byref(d), row.data_ptr(), _lib.stream_ptr()), 'ct_bn_stats_row')
    return invstd


class MergedStats(object):
    """what ``bn_merge_stats`` leaves on the device: ``mean``, biased ``var``, ``invstd``, ``unbiased`` variance ([C] each),
    ``inv_count`` ([1] fp32, 1 / the pixels of all rows), ``count`` ([1] int64) and, when gamma and beta were given, ``beta``
    ([C]): beta shifted by what the rounding of the merged mean to float dropped, times gamma * invstd -- the vector to hand the
    apply and backward calls in the place of beta (None otherwise)"""
    __slots__ = ('mean', 'var', 'invstd', 'unbiased', 'inv_count', 'count', 'beta')


def bn_merge_stats(rows, C, eps=1e-5, gamma=None, beta=None):
    """The statistics of the union of ``world`` shards from their rows: ``rows`` is a 2-D fp32 device tensor, one row per rank
    in rank order, each ``[mean[C] | var[C] | resid[C] | count]`` as ``bn_stats_row`` writes it (a column slice of a wider gathered block
    is fine: the row pitch is its stride).  Pooled moments in double, the rows added in row order, one rounding to float; one
    launch, bitwise reproducible -> ``MergedStats``.  ``gamma`` and ``beta`` (both or neither): the affine pair of the BatchNorm,
    for ``MergedStats.beta``."""
    lib = _lib.load()
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_cuda or rows.shape[1] < bn_row_floats(C) or \
            (rows.shape[1] > 1 and rows.stride(1) != 1):
        raise _lib.CTError('bn_merge_stats: rows must be a 2-d fp32 device tensor of at least %d floats per row' % bn_row_floats(C))
    world = rows.shape[0]
    dev = rows.device
    if (gamma is None) != (beta is None):
        raise _lib.CTError('bn_merge_stats: gamma and beta go together')
    out = torch.empty(5 * C + 4, dtype=torch.float32, device=dev)
    m = MergedStats()
    m.mean, m.var, m.invstd, m.unbiased, m.inv_count = out[:C], out[C:2 * C], out[2 * C:3 * C], out[3 * C:4 * C], out[5 * C:5 * C + 1]
    m.beta = None if beta is None else out[4 * C:5 * C]
    m.count = torch.empty(1, dtype=torch.int64, device=dev)
    d = _lib.BnMergeDesc()
    d.rows, d.world, d.C, d.ld, d.eps = rows.data_ptr(), world, C, rows.stride(0) if world > 1 else rows.shape[1], eps
    d.mean, d.var, d.invstd, d.unbiased = (t.data_ptr() for t in (m.mean, m.var, m.invstd, m.unbiased))
    d.inv_count, d.count = m.inv_count.data_ptr(), m.count.data_ptr()
    if beta is not None:
        for t in (gamma, beta):
            if t.numel() != C or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise _lib.CTError('bn_merge_stats: gamma and beta must be contiguous fp32 [%d] on %s' % (C, dev))
        d.gamma, d.beta, d.beta_shifted = gamma.data_ptr(), beta.data_ptr(), m.beta.data_ptr()
    _lib.check(lib.ct_bn_merge_stats(ctypes.byref(d), _lib.stream_ptr()), 'ct_bn_merge_stats')
    return m


def _bn_backward_sums(entry, query_name, d, z, gy, out):
    """the first half of a batch-statistics backward: the call with gz = gres = NULL -> ``[sum g | sum g * xhat]`` as one [2C]"""
    lib = _lib.load()
    if (gy.N, gy.H, gy.W, gy.C) != (z.N, z.H, z.W, z.C):
        raise _lib.CTError('%s: gy does not have the shape of z' % entry[3:])
    sums = torch.empty(2 * z.C, dtype=torch.float32, device=z.buf.device) if out is None else _bn_vec(out, 2 * z.C, z)
    d.gy, d.ldgy = gy.ptr, gy.ld
    d.gbeta, d.ggamma = sums.data_ptr(), sums.data_ptr() + 4 * z.C
    _ws = _workspace(lib, query_name, d, z.buf.device)
    _lib.check(getattr(lib, entry)(ctypes.byref(d), _lib.stream_ptr()), entry)
    return sums


def _bn_backward_apply(entry, d, z, gy, sums, inv_count, need_z):
    """the second half: ``sums`` ([2C]) and ``inv_count`` ([1]) are the caller's device tensors -> gz (a view, or None)"""
    if (gy.N, gy.H, gy.W, gy.C) != (z.N, z.H, z.W, z.C):
        raise _lib.CTError('%s: gy does not have the shape of z' % entry[3:])
    _bn_vec(sums, 2 * z.C, z)
    _bn_vec(inv_count, 1, z)
    d.gy, d.ldgy = gy.ptr, gy.ld
    gz = new_view(z.N, z.H, z.W, z.C, z.buf.device) if need_z else None
    if gz is not None:
        d.gz, d.ldgz = gz.ptr, gz.ld
    _lib.check(getattr(_lib.load(), entry)(ctypes.byref(d), sums.data_ptr(), inv_count.data_ptr(), _lib.stream_ptr()), entry)
    return gz


def bn_relu_backward_sums(z, gy, mean, invstd, gamma, beta, out=None):
    """``[sum g | sum g * xhat]`` of ``bn_relu_backward`` under batch statistics (this shard's; ``out``: a [2C] to fill)"""
    d = _bn_desc(_lib.BnDesc, z, mean, invstd, gamma, beta, _lib.CT_BN_BATCH_STATS)
    return _bn_backward_sums('ct_bn_relu_backward', 'ct_bn_workspace_bytes', d, z, gy, out)


def bn_relu_backward_apply(z, gy, mean, invstd, gamma, beta, sums, inv_count):
    """gz of ``bn_relu_backward`` under batch statistics from ``sums`` (over every shard) and ``inv_count`` (1 / their pixels)"""
    d = _bn_desc(_lib.BnDesc, z, mean, invstd, gamma, beta, _lib.CT_BN_BATCH_STATS)
    return _bn_backward_apply('ct_bn_relu_backward_apply', d, z, gy, sums, inv_count, True)


def upsample_add_backward(x, w, f, gy, need_x=True, need_w=True):
    """Gradients of ``upsample_add(x, w, f, skip)`` for the output gradient ``gy`` (NHWC views; ``w``: the module weight
    [C,1,2f,2f] or an ``upsample_weight`` result; ``x`` may be None without ``need_w``) -> ``(gx view, gw [C,1,2f,2f], gskip)``,
    None for what was not asked for.  ``gskip`` is ``gy`` itself: no kernel and no copy.  Bitwise reproducible."""
    lib = _lib.load()
    dev = gy.buf.device
    H, W = gy.H // f, gy.W // f
    if f not in (2, 4, 8) or (H * f, W * f) != (gy.H, gy.W) or (need_w and (x.N, x.H, x.W, x.C) != (gy.N, H, W, gy.C)):
        raise _lib.CTError('upsample_add_backward: f=%s, gy %s, x %s do not fit' % (
            f, (gy.N, gy.H, gy.W, gy.C), None if x is None else (x.N, x.H, x.W, x.C)))
    if not (need_x or need_w):
        return None, None, gy
    d = _lib.UpsampleBwdDesc()
    d.gy, d.N, d.H, d.W, d.C, d.ldgy, d.f = gy.ptr, gy.N, H, W, gy.C, gy.ld, f
    gx = gw = None
    if need_x:
        if w.dim() == 4:
            w = upsample_weight(w)
        gx = new_view(gy.N, H, W, gy.C, dev)
        d.w, d.gx, d.ldgx = w.data_ptr(), gx.ptr, gx.ld
    if need_w:
        gw = torch.empty((gy.C, 1, 2 * f, 2 * f), dtype=torch.float32, device=dev)
        d.x, d.ldx, d.gw = x.ptr, x.ld, gw.data_ptr()
        _ws = _workspace(lib, 'ct_upsample_add_backward_workspace_bytes', d, dev)
    _lib.check(lib.ct_upsample_add_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_upsample_add_backward')
    return gx, gw, gy


def mask_sigmoid_backward(gom, om):
    """g <- g * m * (1 - m) on the nine mask channels (18..26) of the offset/mask gradient ``gom``, in place; ``om`` = the
    forward's offset/mask map (mask after the sigmoid)."""
    if (gom.N, gom.H, gom.W) != (om.N, om.H, om.W) or gom.C < 27 or om.C < 27:
        raise _lib.CTError('mask_sigmoid_backward: two 27-channel views of one shape expected')
    _lib.check(_lib.load().ct_dcn_mask_sigmoid_backward(gom.ptr, gom.ld, om.ptr, om.ld, om.N, om.H, om.W, _lib.stream_ptr()),
               'ct_dcn_mask_sigmoid_backward')
    return gom


def pack_weight_s2t(w):
    """OIHW 3x3 conv weight -> the fragment layout the stride-2 input gradient contracts gy with (centertrack_hip.h)."""
    Cout, Cin, ks, ks2 = w.shape
    what = ('pack_weight_s2t: a [Cout,Cin,3,3] weight with Cout %% 16 == 0 and Cin %% 16 == 0 expected (got %s)'
            % (tuple(w.shape),))
    if ks != 3 or ks2 != 3:
        raise _lib.CTError(what)
    return _pack('ct_pack_conv_weight_s2t', 'ct_packed_conv_weight_s2t_elems', w, Cout, Cin, what=what)


def conv_s2_backward(x, gy, w=None, need_x=True, need_w=True, gx=None):
    """Gradients of ``conv3x3(x, w, stride 2, pad 1)`` for the output gradient ``gy`` (NHWC views; ``w``: the OIHW weight,
    packed here, needed for ``need_x``; ``x`` is read for ``need_w`` only but gives the shape) -> ``(gx view, gw OIHW)``, None
    for what was not asked for: no buffer is allocated and no kernel runs for those.  ``gx``: a caller-owned view for the input
    gradient.  Bitwise reproducible."""
    lib = _lib.load()
    dev = gy.buf.device
    if (gy.N, gy.H * 2, gy.W * 2) != (x.N, x.H, x.W):
        raise _lib.CTError('conv_s2_backward: x is %s pixels, gy %s' % ((x.N, x.H, x.W), (gy.N, gy.H, gy.W)))
    if not (need_x or need_w):
        return None, None
    d = _lib.ConvS2BwdDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = x.ptr, x.N, x.H, x.W, x.C, x.ld
    d.gy, d.Cout, d.ldgy = gy.ptr, gy.C, gy.ld
    gw = wp = None
    if need_x:
        if w is None:
            raise _lib.CTError('conv_s2_backward: the input gradient needs the weight')
        wp = pack_weight_s2t(w)
        if gx is None:
            gx = new_view(x.N, x.H, x.W, x.C, dev)
        d.w_s2t, d.gx, d.ldgx = wp.data_ptr(), gx.ptr, gx.ld
    else:
        gx = None
    if need_w:
        _ws = _workspace(lib, 'ct_conv2d_s2_backward_workspace_bytes', d, dev)
        gw = torch.empty((gy.C, x.C, 3, 3), dtype=torch.float32, device=dev)
        d.gw = gw.data_ptr()
    _lib.check(lib.ct_conv2d_s2_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_conv2d_s2_backward')
    return gx, gw


def _bn_act_desc(z, mean, invstd, gamma, beta, res, relu, batch_stats=False):
    d = _bn_desc(_lib.BnActDesc, z, mean, invstd, gamma, beta,
                 (_lib.CT_BN_ACT_RELU if relu else 0) | (_lib.CT_BN_BATCH_STATS if batch_stats else 0))
    if res is not None:
        if (res.N, res.H, res.W, res.C) != (z.N, z.H, z.W, z.C):
            raise _lib.CTError('batch norm: the residual does not have the shape of z')
        d.res, d.ldr = res.ptr, res.ld
    return d


def bn_act_apply(z, mean, invstd, gamma, beta, res=None, relu=True, out=None):
    """y = fma(z - mean, a, beta) (+ res) (max 0), a = gamma * invstd on NHWC views; allocates ``out`` if not
    given."""
    return _bn_apply('ct_bn_act_apply', _bn_act_desc(z, mean, invstd, gamma, beta, res, relu), z, out)


def bn_act_backward(z, gy, mean, invstd, gamma, beta, batch_stats, res=None, relu=True, need_z=True, need_res=False,
                    need_gamma=True, need_beta=True):
    """Gradients of ``bn_act_apply`` (with ``batch_stats``: through the batch statistics as well) for the output gradient
    ``gy`` -> ``(gz view, gres view, ggamma, gbeta)``, None for what was not asked for.  ``res``: the forward's residual (it
    decides the ReLU mask).  Bitwise reproducible."""
    if not (need_z or need_res or need_gamma or need_beta):
        return None, None, None, None
    d = _bn_act_desc(z, mean, invstd, gamma, beta, res, relu, batch_stats)
    gr = new_view(z.N, z.H, z.W, z.C, z.buf.device) if need_res else None
    if gr is not None:
        d.gres, d.ldgres = gr.ptr, gr.ld
    gz, gg, gb = _bn_backward('ct_bn_act_backward', 'ct_bn_act_workspace_bytes', d, z, gy, need_z, need_gamma, need_beta)
    return gz, gr, gg, gb


def bn_act_backward_sums(z, gy, mean, invstd, gamma, beta, res=None, relu=True, out=None):
    """``[sum g | sum g * xhat]`` of ``bn_act_backward`` under batch statistics (this shard's; ``out``: a [2C] to fill)"""
    d = _bn_act_desc(z, mean, invstd, gamma, beta, res, relu, True)
    return _bn_backward_sums('ct_bn_act_backward', 'ct_bn_act_workspace_bytes', d, z, gy, out)


def bn_act_backward_apply(z, gy, mean, invstd, gamma, beta, sums, inv_count, res=None, relu=True, need_z=True, need_res=False):
    """``(gz view, gres view)`` of ``bn_act_backward`` under batch statistics from ``sums`` (over every shard) and ``inv_count``
    (1 / their pixels); None for what was not asked for"""
    if not (need_z or need_res):
        return None, None
    d = _bn_act_desc(z, mean, invstd, gamma, beta, res, relu, True)
    gr = new_view(z.N, z.H, z.W, z.C, z.buf.device) if need_res else None
    if gr is not None:
        d.gres, d.ldgres = gr.ptr, gr.ld
    return _bn_backward_apply('ct_bn_act_backward_apply', d, z, gy, sums, inv_count, need_z), gr


def maxpool2x2_backward(x, gy, add=None, out=None):
    """Backward of ``maxpool2x2``: ``x`` the pool's input, ``gy`` the gradient of its output (NHWC views) -> the view ``gx``;
    each window's gradient goes to its first maximum in row-major order; ``add`` (a view of the shape of ``x``) is summed in."""
    if (gy.N, gy.H * 2, gy.W * 2, gy.C) != (x.N, x.H, x.W, x.C) or (add is not None and (add.N, add.H, add.W, add.C) != (x.N, x.H, x.W, x.C)):
        raise _lib.CTError('maxpool2x2_backward: x %s, gy %s do not fit' % ((x.N, x.H, x.W, x.C), (gy.N, gy.H, gy.W, gy.C)))
    if out is None:
        out = new_view(x.N, x.H, x.W, x.C, x.buf.device)
    _lib.check(_lib.load().ct_maxpool2x2_backward(x.ptr, x.N, x.H, x.W, x.C, x.ld, gy.ptr, gy.ld, None if add is None else add.ptr,
                                                  0 if add is None else add.ld, out.ptr, out.ld, _lib.stream_ptr()),
               'ct_maxpool2x2_backward')
    return out


STEM_CIN = (3, 3, 1)


def _stem_planes(t, s, N, H, W, dev, what):
    """a contiguous fp32 NCHW input (or image gradient) of stem ``s``"""
    if (t.dim() != 4 or tuple(t.shape) != (N, STEM_CIN[s], H, W) or t.dtype != torch.float32 or not t.is_contiguous()
            or t.device != dev):
        raise _lib.CTError('%s: stem %d wants a contiguous fp32 [%d,%d,%d,%d] tensor on %s (got %s)' % (
            what, s, N, STEM_CIN[s], H, W, dev, tuple(t.shape)))
    return t


def _stem_weight(t, s, dev, what):
    if tuple(t.shape) != (16, STEM_CIN[s], 7, 7) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
        raise _lib.CTError('%s: stem %d wants a contiguous fp32 [16,%d,7,7] weight on %s (got %s)' % (
            what, s, STEM_CIN[s], dev, tuple(t.shape)))
    return t


def stem_conv_forward(inputs, weights, out=None):
    """``z_s = conv7x7(inputs[s], weights[s])`` (pad 3, no bias) for every stem present: ``inputs`` = (x, pre_img, pre_hm) as
    contiguous NCHW tensors, ``None`` = stem absent (x must be given); ``weights``: the OIHW [16,Cin,7,7] weights; ``out``:
    optional caller-owned 16-channel views.  -> a list of three NHWC views (None for an absent stem).  One launch."""
    lib = _lib.load()
    if inputs[0] is None:
        raise _lib.CTError('stem_conv_forward: the image stem is part of every call')
    N, _, H, W = inputs[0].shape
    dev = inputs[0].device
    d = _lib.StemConvDesc()
    d.N, d.H, d.W = N, H, W
    zs = [None, None, None]
    for s in range(3):
        if inputs[s] is None:
            continue
        d.inp[s] = _stem_planes(inputs[s], s, N, H, W, dev, 'stem_conv_forward').data_ptr()
        d.w[s] = _stem_weight(weights[s], s, dev, 'stem_conv_forward').data_ptr()
        zs[s] = out[s] if out is not None and out[s] is not None else new_view(N, H, W, 16, dev)
        if (zs[s].N, zs[s].H, zs[s].W, zs[s].C) != (N, H, W, 16):
            raise _lib.CTError('stem_conv_forward: out[%d] is not a [%d,%d,%d,16] view' % (s, N, H, W))
        d.z[s], d.ldz[s] = zs[s].ptr, zs[s].ld
    _lib.check(lib.ct_stem_conv_forward(ctypes.byref(d), _lib.stream_ptr()), 'ct_stem_conv_forward')
    return zs


def stem_bn_relu_sum(zs, means, invstds, gammas, betas, out=None):
    """``y = sum_s max(0, fma(z_s - mean_s, gamma_s * invstd_s, beta_s))`` over the stems present (``zs[s]`` a 16-channel NHWC
    view or None; ``zs[0]`` must be given), added in the order x, pre_img, pre_hm; each term has the bits of
    ``bn_relu_apply``.  One pass; allocates ``out`` if not given."""
    lib = _lib.load()
    if zs[0] is None:
        raise _lib.CTError('stem_bn_relu_sum: the image stem is part of every call')
    z0 = zs[0]
    if out is None:
        out = new_view(z0.N, z0.H, z0.W, 16, z0.buf.device)
    d = _lib.StemSumDesc()
    d.N, d.H, d.W = z0.N, z0.H, z0.W
    for s in range(3):
        z = zs[s]
        if z is None:
            continue
        if (z.N, z.H, z.W, z.C) != (z0.N, z0.H, z0.W, 16):
            raise _lib.CTError('stem_bn_relu_sum: z[%d] does not have the shape of z[0] with 16 channels' % s)
        d.z[s], d.ldz[s] = z.ptr, z.ld
        d.mean[s], d.invstd[s], d.gamma[s], d.beta[s] = (_bn_vec(t[s], 16, z).data_ptr() for t in (means, invstds, gammas, betas))
    if (out.N, out.H, out.W, out.C) != (z0.N, z0.H, z0.W, 16):
        raise _lib.CTError('stem_bn_relu_sum: out does not have the shape of z[0]')
    d.y, d.ldy = out.ptr, out.ld
    _lib.check(lib.ct_stem_bn_relu_sum(ctypes.byref(d), _lib.stream_ptr()), 'ct_stem_bn_relu_sum')
    return out


def stem_conv_backward(gzs, inputs=(None, None, None), weights=(None, None, None), need_w=(True, True, True),
                       need_in=(False, False, False), gws=None, gins=None):
    """Gradients of ``stem_conv_forward`` for the gradients ``gzs[s]`` of ``z_s`` (16-channel NHWC views, None = stem absent)
    -> ``(gw list, gin list)``: ``gw[s]`` OIHW (needs ``inputs[s]``) where ``need_w[s]``, ``gin[s]`` NCHW (needs
    ``weights[s]``) where ``need_in[s]``, None for what was not asked for: no buffer is allocated and no kernel runs for
    those.  ``gws`` / ``gins``: optional caller-owned outputs.  Bitwise reproducible."""
    lib = _lib.load()
    what = 'stem_conv_backward'
    live = [s for s in range(3) if gzs[s] is not None and (need_w[s] or need_in[s])]
    gw, gin = [None, None, None], [None, None, None]
    if not live:
        return gw, gin
    g0 = gzs[live[0]]
    N, H, W, dev = g0.N, g0.H, g0.W, g0.buf.device
    d = _lib.StemConvDesc()
    d.N, d.H, d.W = N, H, W
    for s in live:
        g = gzs[s]
        if (g.N, g.H, g.W, g.C) != (N, H, W, 16):
            raise _lib.CTError('%s: gz[%d] is not a [%d,%d,%d,16] view' % (what, s, N, H, W))
        d.gz[s], d.ldgz[s] = g.ptr, g.ld
        if need_w[s]:
            if inputs[s] is None:
                raise _lib.CTError('%s: the weight gradient of stem %d needs its input' % (what, s))
            d.inp[s] = _stem_planes(inputs[s], s, N, H, W, dev, what).data_ptr()
            gw[s] = (_stem_weight(gws[s], s, dev, what) if gws is not None and gws[s] is not None
                     else torch.empty((16, STEM_CIN[s], 7, 7), dtype=torch.float32, device=dev))
            d.gw[s] = gw[s].data_ptr()
        if need_in[s]:
            if weights[s] is None:
                raise _lib.CTError('%s: the image gradient of stem %d needs its weight' % (what, s))
            d.w[s] = _stem_weight(weights[s], s, dev, what).data_ptr()
            gin[s] = (_stem_planes(gins[s], s, N, H, W, dev, what) if gins is not None and gins[s] is not None
                      else torch.empty((N, STEM_CIN[s], H, W), dtype=torch.float32, device=dev))
            d.gin[s] = gin[s].data_ptr()
    if any(g is not None for g in gw):
        _ws = _workspace(lib, 'ct_stem_conv_backward_workspace_bytes', d, dev)
    _lib.check(lib.ct_stem_conv_backward(ctypes.byref(d), _lib.stream_ptr()), 'ct_stem_conv_backward')
    return gw, gin


# field order of a packed decode row after (score, cls, xs0, ys0)
_DECODE_REST = ['tracking', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity']


def decode_layout(head_names):
    """[(field, start, width)] of one packed row, mirroring ct_decode_row_floats."""
    names = set(head_names)
    lay = [('scores', 0, 1), ('clses', 1, 1), ('xs', 2, 1), ('ys', 3, 1)]
    f = 4
    if names & {'wh', 'ltrb', 'ltrb_amodal'}:
        lay.append(('bboxes', f, 4)); f += 4
    if 'ltrb_amodal' in names:
        lay.append(('bboxes_amodal', f, 4)); f += 4
    for n in _DECODE_REST:
        if n in names:
            lay.append((n, f, _lib.HEAD_CH[n])); f += _lib.HEAD_CH[n]
    return lay, f


def _planes_ok(t, h, w):      # every image's [c,h,w] block contiguous; images may be strided (channel slices)
    return t.stride(3) == 1 and t.stride(2) == w and (t.shape[1] == 1 or t.stride(1) == h * w)


def _sparse_feat(spec, B, h, w):      # -> (pointer, pitch, flip_B) of the sparse heads' feature view; flip_test: 2 * B images
    feat, flip = spec['feat'], bool(spec.get('flip'))
    assert feat.C == 64 and (feat.N, feat.H, feat.W) == ((2 * B if flip else B), h, w)
    return feat.ptr, feat.ld, B if flip else 0


def _head_ptrs(w1, b1, w2, b2, c):      # a sparse head of c channels: packed conv3x3 weight, hidden bias [256], w2 [c,256], b2 [c]
    assert tuple(w2.shape) == (c, 256) and w2.is_contiguous() and b1.numel() == 256 and b2.numel() == c
    return w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()


class Decoder(object):
    """Pre-built ct_decode call (+ ct_decode_pose when the pose heads ``hps`` / ``hm_hp`` are given) for fixed
    shapes (graph-capture friendly).  One packed buffer ``out`` [B,K,F]: the rows of ct_decode followed, for the
    pose task, by the refined key points [2J] and ``kps_score`` [1]."""

    @staticmethod
    def row_floats(heads, sparse=None, sparse_pose=None):
        """floats per packed row for this set of heads (the pose fields included; ``sparse``: names of sparse heads;
        ``sparse_pose``: the argument of that name of the constructor -- the same rows as with an ``hps`` map)"""
        _, F = decode_layout([n for n in heads if n in _lib.HEAD_INDEX] + list(sparse or ()))
        if 'hps' in heads and 'hm_hp' in heads:
            F += heads['hps'].shape[1] + 1
        elif sparse_pose is not None and 'hm_hp' in heads:
            F += 2 * heads['hm_hp'].shape[1] + 1
        return F

    def __init__(self, hm, heads, K, host_out=None, done_flag=None, sparse=None, sparse_pose=None):
        """``host_out`` (pinned host float32 [B,K,F]) / ``done_flag`` (pinned host int32): the decode also stores the
        rows straight into host memory and raises the flag when they are complete (no pose heads).
        ``sparse`` (round 5, opt-in): ``{'feat': NHWC view of the 64-channel feature map, 'heads': [(name, w1_packed, b1,
        w2 [c,256], b2)], 'depth_scale', 'zero_tracking'}`` -- these regression heads have no map in ``heads``; they are
        evaluated at the K winners only (ct_sparse_heads_desc).
        ``sparse_pose`` (opt-in, independent of ``sparse``): ``{'feat': that NHWC view, 'hps': (w1_packed, b1, w2 [2J,256],
        b2), 'off': the same of the hp_offset head (else the reg head) with w2 [2,256], or None for +0.5, 'flip': bool,
        'flip_pairs': int pairs}`` -- ``heads`` holds ``hm_hp`` but neither ``hps`` nor ``hp_offset``; ``hps`` is evaluated
        at the K winners and the offset head at the K peaks of every joint map (ct_decode_pose_sparse).  Same row layout
        as with the two maps.  A ``reg`` map in ``heads`` only serves the gate box then.  With ``sparse`` the match needs
        its gate box in the rows: no ``ltrb_amodal`` head."""
        lib = _lib.load()
        self.K = K
        B, C, h, w = hm.shape
        self.hm, self.heads = hm, dict(heads)
        sparse_names = [n for n, *_ in sparse['heads']] if sparse is not None else []
        d = self._dense_desc(hm, heads, K)
        self.sparse = None
        if sparse is not None:
            assert 'hps' not in heads and all(n not in heads for n in sparse_names)
            self.sparse = (self._sparse_heads_desc(sparse, B, h, w), sparse)      # (keeps the tensors alive)
            d.sparse = ctypes.pointer(self.sparse[0])
        self.layout, F0 = decode_layout([n for n in heads if n in _lib.HEAD_INDEX] + sparse_names)
        assert lib.ct_decode_row_floats(ctypes.byref(d)) == F0
        J = self._pose_joints(heads, sparse_names, sparse_pose)
        self.F = F0
        if J is not None:
            self.layout = self.layout + [('hps', F0, 2 * J), ('kps_score', F0 + 2 * J, 1)]
            self.F = F0 + 2 * J + 1
        self.out = torch.empty((B, K, self.F), dtype=torch.float32, device=hm.device)
        self.inds = torch.empty((B, K), dtype=torch.int64, device=hm.device)
        nbytes = lib.ct_decode_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            _lib.check(1, 'ct_decode_workspace_bytes')
        # (zeroed for tidiness only: ct_decode writes every byte it reads -- candidates, winner keys, partials -- and the one
        #  extra word past ``nbytes`` is never handed to it)
        self.ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=hm.device)
        d.out, d.inds = self.out.data_ptr(), self.inds.data_ptr()
        d.out_stride = self.F
        d.workspace, d.workspace_bytes = self.ws.data_ptr(), nbytes
        self.direct = False
        if host_out is not None and done_flag is not None and J is None:
            assert tuple(host_out.shape) == (B, K, self.F) and host_out.is_pinned() and done_flag.is_pinned()
            self.done_counter = torch.zeros((4,), dtype=torch.int32, device=hm.device)
            d.host_out, d.done_flag = host_out.data_ptr(), done_flag.data_ptr()
            d.done_counter = self.done_counter.data_ptr()
            self.direct = True
        self.desc = d
        self.pose = self.pose_sparse = None
        if J is not None and sparse_pose is None:
            pd = _lib.PoseDesc()
            self._fill_pose_desc(pd, heads, sparse_names, J, F0, heads['hps'], heads.get('hp_offset', heads.get('reg')))
            pbytes = lib.ct_decode_pose_workspace_bytes(ctypes.byref(pd))
            if pbytes == 0:
                _lib.check(1, 'ct_decode_pose_workspace_bytes')
            self.pose_ws = torch.empty(pbytes // 8 + 1, dtype=torch.int64, device=hm.device)
            pd.workspace, pd.workspace_bytes = self.pose_ws.data_ptr(), self.pose_ws.numel() * 8
            self.pose = pd
        elif J is not None:
            spd = _lib.PoseSparseDesc()
            self._fill_pose_desc(spd.base, heads, sparse_names, J, F0)
            pairs = self._fill_pose_sparse_desc(spd, sparse_pose, J)
            need = ctypes.c_size_t(0)
            _lib.check(lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(spd), ctypes.byref(need)),
                       'ct_decode_pose_sparse_workspace_bytes')
            # (zeroed only so that the offsets area reads as 0 without an offset head: the call neither writes nor reads it
            #  then, and of everything else it reads nothing it has not written)
            self.pose_ws = torch.zeros(need.value // 8 + 1, dtype=torch.int64, device=hm.device)
            spd.base.workspace, spd.base.workspace_bytes = self.pose_ws.data_ptr(), self.pose_ws.numel() * 8
            self.pose_sparse = (spd, sparse_pose, pairs)                # (keeps the tensors and the pairs alive)

    @staticmethod
    def _dense_desc(hm, heads, K):
        """the ct_decode descriptor of the heat map and the dense head maps (outputs and workspace are set by the caller)"""
        B, C, h, w = hm.shape
        d = DecodeDesc()
        assert _planes_ok(hm, h, w)
        d.hm, d.B, d.C, d.h, d.w, d.K = hm.data_ptr(), B, C, h, w, K
        d.hm_batch_stride = hm.stride(0)
        for name, t in heads.items():
            if name in _lib.HEAD_INDEX:
                assert _planes_ok(t, h, w) and t.shape[1] == _lib.HEAD_CH[name], name
                d.heads[_lib.HEAD_INDEX[name]] = t.data_ptr()
                d.head_batch_stride[_lib.HEAD_INDEX[name]] = t.stride(0)
        return d

    @staticmethod
    def _sparse_heads_desc(sparse, B, h, w):
        sp = _lib.SparseHeadsDesc()
        sp.feat, sp.ldf, sp.flip_B = _sparse_feat(sparse, B, h, w)
        sp.nheads = len(sparse['heads'])
        for i, (name, *wts) in enumerate(sparse['heads']):
            sp.head[i] = _lib.HEAD_INDEX[name]
            sp.flip_mode[i] = (1 if name in ('wh', 'dep', 'dim') else 2 if name == 'amodel_offset' else 0) if sp.flip_B else 0
            sp.w1[i], sp.b1[i], sp.w2[i], sp.b2[i] = _head_ptrs(*wts, _lib.HEAD_CH[name])
        sp.depth_scale = float(sparse.get('depth_scale', 1.0))
        sp.zero_tracking = int(bool(sparse.get('zero_tracking', False)))
        return sp

    @staticmethod
    def _pose_joints(heads, sparse_names, sparse_pose):
        """the number of joints of the pose task (decode.py:161-171), None without one"""
        if sparse_pose is not None:
            if 'hps' in heads or 'hp_offset' in heads or 'hm_hp' not in heads:
                raise _lib.CTError('sparse pose heads: `heads` holds hm_hp and neither hps nor hp_offset')
            if 'ltrb_amodal' in sparse_names:
                raise _lib.CTError('sparse pose heads beside a sparse ltrb_amodal head: the rows do not hold the gate box')
            return heads['hm_hp'].shape[1]
        if 'hps' not in heads:
            return None
        if 'hm_hp' not in heads:                           # decode.py:80-81: no refinement, kps_score = kps
            raise _lib.CTError('the pose branch without an hm_hp head is not implemented')
        return heads['hps'].shape[1] // 2

    def _fill_pose_desc(self, pd, heads, sparse_names, J, F0, hps=None, off=None):
        """what ct_decode_pose and ct_decode_pose_sparse share: the rows, the gate box, the joint heat maps and the output
        columns; ``hps`` / ``off``: the two maps of the dense form"""
        (B, _, h, w), K = self.hm.shape, self.K
        hm_hp = heads['hm_hp']
        assert hm_hp.is_contiguous() and hm_hp.shape[1] == J and all(t is None or _planes_ok(t, h, w) for t in (hps, off))
        pd.rows, pd.row_floats, pd.inds = self.out.data_ptr(), self.F, self.inds.data_ptr()
        # the gate box of _update_kps_with_hm is generic_decode's local `bboxes`: wh, overridden by ltrb -- never the
        # ltrb_amodal box that replaces ret['bboxes'] in the packed row (decode.py:123,137 vs 159)
        # (sparse main heads: the rows are the only place the box is -- column 4, or the box-less variant)
        in_rows = set(heads) | set(sparse_names)
        if 'ltrb_amodal' in in_rows or not ({'wh', 'ltrb'} & in_rows):
            pd.box_col = -1
            for name, fld in (('wh', 'box_wh'), ('ltrb', 'box_ltrb')):
                if name in heads:
                    assert _planes_ok(heads[name], h, w)
                    setattr(pd, fld, heads[name].data_ptr())
                    setattr(pd, fld + '_batch_stride', heads[name].stride(0))
            if 'wh' in heads and 'reg' in heads:
                pd.box_reg, pd.box_reg_batch_stride = heads['reg'].data_ptr(), heads['reg'].stride(0)
        else:
            pd.box_col = 4
        pd.B, pd.h, pd.w, pd.K, pd.num_joints = B, h, w, K, J
        pd.hps, pd.hm_hp, pd.hp_offset = _p(hps), hm_hp.data_ptr(), _p(off)
        pd.hps_batch_stride = hps.stride(0) if hps is not None else 0
        pd.hp_offset_batch_stride = off.stride(0) if off is not None else 0
        pd.out, pd.out_stride = self.out.data_ptr() + 4 * F0, self.F

    @staticmethod
    def _fill_pose_sparse_desc(spd, sparse_pose, J):
        """the feature view, the two heads' weights and the flip pairs behind ``spd.base``; returns the pairs array"""
        spd.feat, spd.ldf, spd.flip_B = _sparse_feat(sparse_pose, spd.base.B, spd.base.h, spd.base.w)
        for pre, c, wts in (('hps', 2 * J, sparse_pose['hps']), ('off', 2, sparse_pose.get('off'))):
            if wts is not None:
                for fld, ptr in zip(('w1', 'b1', 'w2', 'b2'), _head_ptrs(*wts, c)):
                    setattr(spd, '%s_%s' % (pre, fld), ptr)
        pairs = np.ascontiguousarray(sparse_pose.get('flip_pairs', ()), np.int32).reshape(-1, 2)
        spd.flip_pairs, spd.num_pairs = pairs.ctypes.data, len(pairs)
        return pairs

    def run(self):
        _lib.check(_lib.load().ct_decode(ctypes.byref(self.desc), _lib.stream_ptr()), 'ct_decode')
        if self.pose is not None:
            _lib.check(_lib.load().ct_decode_pose(ctypes.byref(self.pose), _lib.stream_ptr()), 'ct_decode_pose')
        if self.pose_sparse is not None:
            _lib.check(_lib.load().ct_decode_pose_sparse(ctypes.byref(self.pose_sparse[0]), _lib.stream_ptr()),
                       'ct_decode_pose_sparse')
        return self.out

    def pose_values(self):
        """what the match of the last ``run`` read instead of maps (``sparse_pose``): the merged raw ``hps`` values [B,K,2J] at
        the winners, before the centre is added, and the offset values [B*J,K,2] at the joint peaks (None without an offset
        head) -- views of the workspace"""
        spd = self.pose_sparse[0]
        B, K, J = spd.base.B, spd.base.K, spd.base.num_joints
        f = self.pose_ws.view(torch.float32)
        n = B * K * 2 * J
        at = ((n * 4 + 255) // 256) * 64
        return f[:n].view(B, K, 2 * J), (f[at:at + B * J * K * 2].view(B * J, K, 2) if spd.off_w1 else None)

    def unpack(self, packed):
        """packed [B,K,F] (torch or numpy) -> the reference's ``dets`` dict (decode.py:99-180)."""
        ret = {}
        for name, s, wd in self.layout:
            v = packed[..., s:s + wd]
            ret[name] = v[..., 0] if name in ('scores', 'clses', 'xs', 'ys', 'kps_score') else v
        ret['cts'] = packed[..., 2:4]
        return ret


def _fill_targets_desc(t, staging_host, staging_dev, words, B, max_objs, slot_words, nout, pre_hm):
    """the fields of a ``ct_targets_desc`` that ``build_targets`` and ``build_pose_targets`` fill alike"""
    t.staging_host, t.staging_dev, t.words = staging_host.data_ptr(), staging_dev.data_ptr(), words
    t.B, t.max_objs, t.slot_words, t.nout = B, max_objs, slot_words, nout
    if pre_hm is not None:
        t.pre_hm = pre_hm.data_ptr()
        t.H, t.W = pre_hm.shape[2:]


def build_targets(staging_host, staging_dev, words, B, max_objs, slot_words, nout, hm=None, pre_hm=None):
    """ct_build_targets (csrc/targets.hip) on the current stream: upload ``words`` int32 words of the packed batch from the
    pinned ``staging_host`` to ``staging_dev`` and write hm [B,C,h,w], pre_hm [B,1,H,W] (either may be None) and the slot
    tensors the buffer's output table names, in one launch.  ``centertrack_amd.targets.TargetBuilder.render`` packs the
    buffer; bad contents raise ``CTError`` before anything is enqueued."""
    d = _lib.TargetsDesc()
    _fill_targets_desc(d, staging_host, staging_dev, words, B, max_objs, slot_words, nout, pre_hm)
    if hm is not None:
        d.hm = hm.data_ptr()
        _, d.C, d.h, d.w = hm.shape
    _lib.check(_lib.load().ct_build_targets(ctypes.byref(d), _lib.stream_ptr()), 'ct_build_targets')


def build_pose_targets(staging_host, staging_dev, words, B, max_objs, slot_words, nout, C, J, hw, hm=None, pre_hm=None,
                       hm_hp=None):
    """ct_build_pose_targets (csrc/targets.hip) on the current stream: ``build_targets`` plus hm_hp [B,J,h,w] in the same
    launch.  ``C`` class planes and ``J`` joint planes of ``hw`` = (h, w) number the planes of the lists whichever maps
    are asked for (each of hm, pre_hm, hm_hp may be None).  ``centertrack_amd.targets.PoseTargetBuilder.render`` packs
    the buffer; bad contents raise ``CTError`` before anything is enqueued."""
    d = _lib.PoseTargetsDesc()
    t = d.base
    _fill_targets_desc(t, staging_host, staging_dev, words, B, max_objs, slot_words, nout, pre_hm)
    t.C, (t.h, t.w), d.J = C, hw, J
    if hm is not None:
        t.hm = hm.data_ptr()
    if hm_hp is not None:
        d.hm_hp = hm_hp.data_ptr()
    _lib.check(_lib.load().ct_build_pose_targets(ctypes.byref(d), _lib.stream_ptr()), 'ct_build_pose_targets')


def build_inputs(staging_host, staging_dev, nbytes, B, N, H, W, mean, std, image, pre_img, warped, partials,
                 gs_mean=None):
    """ct_build_inputs (csrc/inputs.hip) on the current stream: upload ``nbytes`` bytes of descriptors and u8 source rows
    from the pinned ``staging_host`` to ``staging_dev`` and write image [B,3,H,W] (and pre_img, with N = 2 B) in two
    launches.  ``warped`` int32 [N,H,W] and ``partials`` float64 [N * ct_build_inputs_partials(H, W)] are scratch,
    ``gs_mean`` float32 [N] is optional.  ``centertrack_amd.inputs.InputBuilder.render`` packs the buffer; bad contents
    raise ``CTError`` before anything is enqueued."""
    d = _lib.InputsDesc()
    d.staging_host, d.staging_dev, d.bytes = staging_host.data_ptr(), staging_dev.data_ptr(), nbytes
    d.B, d.N, d.H, d.W = B, N, H, W
    for c in range(3):
        d.mean[c], d.stdv[c] = float(mean[c]), float(std[c])
    d.image = image.data_ptr()
    d.pre_img = pre_img.data_ptr() if pre_img is not None else None
    d.warped, d.partials = warped.data_ptr(), partials.data_ptr()
    d.gs_mean = gs_mean.data_ptr() if gs_mean is not None else None
    _lib.check(_lib.load().ct_build_inputs(ctypes.byref(d), _lib.stream_ptr()), 'ct_build_inputs')


def optim_step(table, n, chunks, kind):
    """ct_optim_step (csrc/optim.hip) on the current stream: one launch over the ``n`` records and the chunk prefix of the
    DEVICE int32 tensor ``table`` (``centertrack_amd.optim.pack`` lays it out, the caller has uploaded it)."""
    _lib.check(_lib.load().ct_optim_step(table.data_ptr(), n, chunks, kind, _lib.stream_ptr()), 'ct_optim_step')


def optim_pack_grads(table, n, chunks, scale):
    """ct_optim_pack_grads (csrc/optim.hip) on the current stream: one launch that gathers
    ``src[i] * scale`` of every record of the uploaded ``table`` into the flat buffer its ``g`` points into, the tail of every
    tensor's last chunk written as +0.0."""
    _lib.check(_lib.load().ct_optim_pack_grads(table.data_ptr(), n, chunks, float(scale), _lib.stream_ptr()),
               'ct_optim_pack_grads')


def optim_norms_workspace_bytes(n, chunks):
    """bytes of workspace ``optim_norms`` needs for ``n`` tensors in ``chunks`` chunks (0: sizes it refuses)"""
    return int(_lib.load().ct_optim_norms_workspace_bytes(n, chunks))


def optim_norms(table, n, chunks, max_norm, skip_nonfinite, per_tensor, guard, workspace):
    """ct_optim_norms (csrc/optim.hip) on the current stream: two launches over the uploaded ``table``
    that leave the sum of squares of every gradient in the DEVICE float64 tensor ``per_tensor`` (or ``None``) and norm, clip
    coefficient, skip decision and running counters in the ``ct_optim_guard`` at the start of the DEVICE tensor
    ``guard``.  ``workspace``: a DEVICE byte tensor of at least ``optim_norms_workspace_bytes(n, chunks)`` bytes."""
    _lib.check(_lib.load().ct_optim_norms(table.data_ptr(), n, chunks, float(max_norm), int(bool(skip_nonfinite)),
                                          per_tensor.data_ptr() if per_tensor is not None else None, guard.data_ptr(),
                                          workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                          _lib.stream_ptr()), 'ct_optim_norms')


def optim_step_guarded(table, n, chunks, kind, guard):
    """ct_optim_step_guarded on the current stream: ``optim_step`` scaled by the guard's clip coefficient, or skipped"""
    _lib.check(_lib.load().ct_optim_step_guarded(table.data_ptr(), n, chunks, kind, guard.data_ptr(), _lib.stream_ptr()),
               'ct_optim_step_guarded')
