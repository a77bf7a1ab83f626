"""What the trainable modules (``dcn_v2``, ``dla_up``, ``dla_base``, ``heads``) share: the trainable switch, the one input
check, the NCHW <-> NHWC boundary and the BatchNorm statistics step.  Nothing here launches a kernel of
its own; it depends on ``ops`` and on no module."""
import contextlib

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops

BN_MOMENTUM = 0.1

_trainable = False


def set_trainable(flag):
    """Switch the differentiable path of ``dcn_v2_conv`` / ``DCNv2`` / ``DCN`` on or off (default: off).  Returns the
    previous setting.  Off, every call is today's inference call whatever ``requires_grad`` or ``module.training`` say."""
    global _trainable
    was = _trainable
    _trainable = bool(flag)
    return was


def is_trainable():
    return _trainable


@contextlib.contextmanager
def trainable(flag=True):
    was = set_trainable(flag)
    try:
        yield
    finally:
        set_trainable(was)


def recording():
    """is a graph being recorded: the switch is on and autograd is enabled"""
    return _trainable and torch.is_grad_enabled()


def need_cuda(x, what, dims=4):
    """The input check: ``x`` is a CUDA fp32 tensor of ``dims`` dimensions (``None``: any rank); ``what`` opens the message"""
    if not x.is_cuda:
        raise _lib.CTError('%s runs on an MI355X only (got a %s tensor); no CPU fallback' % (what, x.device))
    if x.dtype != torch.float32:
        raise _lib.CTError('%s computes in fp32 (got %s)' % (what, x.dtype))
    if dims is not None and x.dim() != dims:
        raise _lib.CTError('%s wants a %d-d tensor (got %s)' % (what, dims, tuple(x.shape)))


# ---------------------------------------------------------------------------------------------------------------------
# layout at the public boundary

class ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.view_from_nchw(x).buf

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.view_to_nchw(ops.View(g.contiguous()))


class ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.view_to_nchw(ops.View(x))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.view_from_nchw(g).buf


def to_nhwc(x, what):
    """NCHW fp32 CUDA tensor -> contiguous ``[N,H,W,C]`` tensor (differentiable while a graph is recorded); ``what`` names
    the caller (``neck``, ``backbone``) in the messages"""
    need_cuda(x, 'centertrack_amd ' + what)
    if x.shape[1] % 4:
        raise _lib.CTError('centertrack_amd %s needs channels %% 4 == 0 (got %d)' % (what, x.shape[1]))
    if recording():
        return ToNHWC.apply(x)
    with torch.no_grad():
        return ops.view_from_nchw(x).buf


def to_nchw(x):
    if recording():
        return ToNCHW.apply(x)
    with torch.no_grad():
        return ops.view_to_nchw(ops.View(x))


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics

@torch.no_grad()
def update_running_stats(bn, mean, var, P):
    """What a training-mode ``nn.BatchNorm2d`` does with the batch statistics of ``P`` values per channel: the counter, the
    momentum (``None`` = cumulative average) and the unbiased variance"""
    bn.num_batches_tracked += 1
    m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    bn.running_mean.mul_(1 - m).add_(mean, alpha=m)
    bn.running_var.mul_(1 - m).add_(var, alpha=m * P / (P - 1))


def bn_statistics(bn, z, what):
    """The statistics ``bn`` normalises the NHWC view ``z`` with -> ``(mean, invstd, batch)``.  As torch: batch statistics
    (``ops.bn_stats``) in training mode or without running statistics, and a training-mode module then moves its running
    statistics; otherwise the running statistics themselves.  ``what`` opens the refusal of one value per channel."""
    batch = bn.training or bn.running_mean is None
    if not batch:
        return bn.running_mean, torch.rsqrt(bn.running_var + bn.eps), False
    P = z.N * z.H * z.W
    if P == 1:
        raise _lib.CTError('%s: training-mode BatchNorm needs more than one value per channel (N*H*W == 1)' % what)
    mean, var, invstd = ops.bn_stats(z, bn.eps)
    if bn.training and bn.running_mean is not None:
        update_running_stats(bn, mean, var, P)
    return mean, invstd, True


def saved_mean(mean, batch):
    """what an ``autograd.Function`` keeps of ``bn_statistics``' mean: a batch mean is private to the call, the running mean
    is the module's buffer and is cloned"""
    return mean if batch else mean.clone()
