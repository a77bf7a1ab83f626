"""What the trainable modules (``dcn_v2``, ``dla_up``, ``dla_base``, ``heads``) share: the trainable switch, the one input
check, the NCHW <-> NHWC boundary and the BatchNorm statistics step, with its synchronised form and
the backward that goes with it (section 32).  Nothing here launches a kernel of its own; it depends on ``ops`` and ``parallel``
and on no module."""
import contextlib

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops, parallel

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


@torch.no_grad()
def update_running_stats_merged(bn, mean, unbiased):
    """``update_running_stats`` with the statistics of ``ops.bn_merge_stats``: the unbiased variance comes from the device, where
    the count over all ranks lives"""
    bn.num_batches_tracked += 1
    m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    bn.running_mean.mul_(1 - m).add_(mean, alpha=m)
    bn.running_var.mul_(1 - m).add_(unbiased, alpha=m)


class SyncedBatch(object):
    """The ``batch`` of ``bn_statistics`` on the synchronised path: true like ``True``, and it carries
    what the backward needs -- ``inv_count``, the device scalar 1 / (pixels of all ranks), and the process ``group`` -- and
    ``beta``: the module's beta shifted by what the rounding of the merged mean to float dropped (``ops.MergedStats.beta``; None
    for a BatchNorm without affine parameters), which apply and backward take in the place of beta"""
    __slots__ = ('inv_count', 'group', 'beta')

    def __init__(self, inv_count, group, beta=None):
        self.inv_count, self.group, self.beta = inv_count, group, beta

    def __bool__(self):
        return True


def bn_statistics(bn, z, what):
    """The statistics ``bn`` normalises the NHWC view ``z`` with -> ``(mean, invstd, batch)``.  As torch: batch statistics
    (``ops.bn_stats``) in training mode or without running statistics, and a training-mode module then moves its running
    statistics; otherwise the running statistics themselves.  ``what`` opens the refusal of one value per channel.

    The one place that decides the path: a BatchNorm marked by ``parallel.sync_batchnorm`` that uses batch statistics while a
    process group of more than one rank is active takes them over the batches of all ranks -- local ``ct_bn_stats`` into a
    row, one all-gather, ``ct_bn_merge_stats`` -- moves its running statistics with the merged mean and the merged unbiased
    variance, and ``batch`` is a ``SyncedBatch``.  In every other case the path is the unsynchronised one, bit for bit."""
    return bn_statistics_many([bn], [z], what)[0]


def bn_statistics_many(bns, zs, what):
    """``bn_statistics`` of several BatchNorms at once (``None`` entries stay ``None``): those on the synchronised path share
    ONE all-gather, their rows concatenated (the three stems)"""
    out = [None] * len(bns)
    synced = {}
    for i, (bn, z) in enumerate(zip(bns, zs)):
        if bn is None:
            continue
        batch = bn.training or bn.running_mean is None
        mark = parallel.sync_batchnorm_of(bn) if batch else None
        if mark is not None:
            synced.setdefault(id(mark.group), []).append((i, bn, z, mark))
            continue
        if not batch:
            out[i] = (bn.running_mean, torch.rsqrt(bn.running_var + bn.eps), False)
            continue
        P = z.N * z.H * z.W
        if P == 1:
            raise _lib.CTError('%s: training-mode BatchNorm needs more than one value per channel (N*H*W == 1)' % what)
        mean, var, invstd = ops.bn_stats(z, bn.eps)
        if bn.training and bn.running_mean is not None:
            update_running_stats(bn, mean, var, P)
        out[i] = (mean, invstd, True)
    for members in synced.values():
        group = members[0][3].group
        if parallel.world_size(group) == 1 and any(z.N * z.H * z.W == 1 for _, _, z, _ in members):
            # (with more ranks every rank adds at least one value: nothing to refuse)
            raise _lib.CTError('%s: training-mode BatchNorm needs more than one value per channel (N*H*W == 1)' % what)
        sizes = [ops.bn_row_floats(z.C) for _, _, z, _ in members]
        row = torch.empty(sum(sizes), dtype=torch.float32, device=members[0][2].buf.device)
        at = 0
        for (_, bn, z, _), n in zip(members, sizes):
            ops.bn_stats_row(z, bn.eps, row[at:at + n])
            at += n
        rows = parallel.all_gather_rows(row, group)
        at = 0
        for (i, bn, z, _), n in zip(members, sizes):
            affine = bn.weight is not None and bn.bias is not None
            m = ops.bn_merge_stats(rows[:, at:at + n], z.C, bn.eps, gamma=bn.weight.detach() if affine else None,
                                   beta=bn.bias.detach() if affine else None)
            at += n
            if bn.training and bn.running_mean is not None:
                update_running_stats_merged(bn, m.mean, m.unbiased)
            out[i] = (m.mean, m.invstd, SyncedBatch(m.inv_count, group, m.beta))
    return out


def synced_bn_backward(items):
    """The backward of BatchNorm (+ residual) (+ ReLU) on the synchronised path, for several BatchNorms that share ONE
    all-reduce (the three stems; a list of one elsewhere).  Each item is a dict: ``z``, ``gy`` (views), ``mean``, ``invstd``,
    ``gamma``, ``beta``, ``sync`` (the forward's ``SyncedBatch``), and optionally ``res``, ``relu`` (True), ``neck`` (False: the
    ``ct_bn_act_*`` entry points; True: their ``ct_bn_relu_*`` twins), ``need_z`` (True), ``need_res`` (False), ``need_gamma``,
    ``need_beta`` (True).  Per item: the local sums, [all-reduce of every item's sums at once,] the apply half against the
    sums and the count of all ranks -> ``(gz, gres, ggamma, gbeta)``, None for what was not asked for.  ``ggamma`` and
    ``gbeta`` stay the LOCAL sums: the distributed step averages them with every other gradient."""
    def get(it, k, default):
        return it[k] if k in it else default
    if not items:
        return []
    # one [2C] slot per item; an item that asks for gres alone never reads its slot (it stays zero)
    offsets, total = [], 0
    for it in items:
        offsets.append(total)
        total += 2 * it['z'].C
    flat = torch.zeros(total, dtype=torch.float32, device=items[0]['z'].buf.device)
    local = []
    for it, at in zip(items, offsets):
        C = it['z'].C
        need_gamma, need_beta = get(it, 'need_gamma', True), get(it, 'need_beta', True)
        if not (get(it, 'need_z', True) or need_gamma or need_beta):
            local.append((None, None))
            continue
        args = (it['z'], it['gy'], it['mean'], it['invstd'], it['gamma'], bn_beta(it['sync'], it['beta']))
        if get(it, 'neck', False):
            ops.bn_relu_backward_sums(*args, out=flat[at:at + 2 * C])
        else:
            ops.bn_act_backward_sums(*args, res=get(it, 'res', None), relu=get(it, 'relu', True), out=flat[at:at + 2 * C])
        local.append((flat[at + C:at + 2 * C].clone() if need_gamma else None, flat[at:at + C].clone() if need_beta else None))
    if any(get(it, 'need_z', True) for it in items):
        parallel.all_reduce_flat(flat, items[0]['sync'].group)
    results = []
    for it, at, (gg, gb) in zip(items, offsets, local):
        need_z, need_res = get(it, 'need_z', True), get(it, 'need_res', False)
        gz = gr = None
        if need_z or need_res:
            args = (it['z'], it['gy'], it['mean'], it['invstd'], it['gamma'], bn_beta(it['sync'], it['beta']), flat[at:at + 2 * it['z'].C],
                    it['sync'].inv_count)
            if get(it, 'neck', False):
                gz = ops.bn_relu_backward_apply(*args)
            else:
                gz, gr = ops.bn_act_backward_apply(*args, res=get(it, 'res', None), relu=get(it, 'relu', True),
                                                   need_z=need_z, need_res=need_res)
        results.append((gz, gr, gg, gb))
    return results


def bn_beta(batch, beta):
    """the beta the apply and backward calls take for the ``batch`` of ``bn_statistics``: the module's, or on the synchronised
    path the shifted one that goes with the merged mean"""
    return batch.beta if isinstance(batch, SyncedBatch) and batch.beta is not None else beta


def saved_mean(mean, batch):
    """what an ``autograd.Function`` keeps of ``bn_statistics``' mean: a batch mean is private to the call, the running mean
    is the module's buffer and is cloned"""
    return mean if batch else mean.clone()
