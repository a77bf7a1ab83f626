"""Shared pieces of the synchronised-BatchNorm tests (tests/test_sync_bn_cpu.py, tests/test_hip_sync_bn.py,
tests/_sync_bn_worker.py): the shard lists, the data, the merge of per-shard statistics in numpy
float64 with its mutations, the float64 / float32 torch reference on the whole batch, and the two ways the ops are driven on a
device -- every shard in one process (``emulate``) and one shard per rank through a process group (``through_group``)."""
import numpy as np
import torch
import torch.nn.functional as F

import _neck_bwd as NB

EPS = NB.EPS
SHIFT, SHIFT_CHANNEL = 50.0, 3

# (global shape (N, H, W, C), shards of N).  The shapes are the smallest of their regimes in ``_neck_bwd``: cw 33 leaves dead
# threads; 8 channels are channels 4..11 of a 16-wide buffer; (3,254,258,16) takes its slab count from the grid target and
# caps the element-wise grid (on the shard of two samples).
SHARD_LISTS = [((2, 5, 7, 64), (1, 1)), ((3, 9, 11, 132), (2, 1)), ((3, 9, 11, 132), (1, 1, 1)), ((2, 33, 65, 8), (1, 1)),
               ((3, 254, 258, 16), (2, 1))]
TWO_RANK_LISTS = [sl for sl in SHARD_LISTS if len(sl[1]) == 2]
FORMS = ('neck', 'backbone')         # <ReLU, no residual> on ct_bn_relu_*, <ReLU, residual> on ct_bn_act_*


def list_id(sl):
    return '%s-%s' % ('x'.join(str(v) for v in sl[0]), '|'.join(str(n) for n in sl[1]))


def sync_case(shape, shards, residual=False):
    """``_neck_bwd.bn_case`` -- a channel of mean 100 / std 0.01 (0), a constant channel (1), an all-negative channel (2) --
    with channel 3 of the LAST shard shifted by +50: i.i.d. shards have nearly equal means, and a merge that drops the
    between-shard term, one that ignores the counts or a backward that keeps its sums local would all pass without it"""
    assert sum(shards) == shape[0]
    case = NB.bn_case(shape, residual)
    case[0][shape[0] - shards[-1]:, SHIFT_CHANNEL] += SHIFT
    return case


def split(t, shards):
    return list(torch.split(t, list(shards), 0))


# ---------------------------------------------------------------------------------------------------------------------
# the merge, in numpy float64

def shard_rows(z, shards):
    """[(mean[C], biased var[C], pixels)] of every shard of the NCHW tensor ``z``, in float64"""
    rows = []
    for zs in split(z.double(), shards):
        rows.append((zs.mean((0, 2, 3)).numpy(), zs.var((0, 2, 3), unbiased=False).numpy(), zs.shape[0] * zs.shape[2] * zs.shape[3]))
    return rows


def reference_merge(rows, between=True, counts=True):
    """Pooled moments of ``rows`` = [(mean, var, count)] -> (mean, biased var, N): N = sum P_r, mean = sum P_r mean_r / N,
    var = (sum P_r var_r + sum P_r (mean_r - mean)^2) / N, the rows added in order.  The two switches are the MUTATIONS the
    data must catch: ``between=False`` drops the second sum, ``counts=False`` weighs every row alike."""
    N = sum(int(r[2]) for r in rows)
    w = [float(r[2]) if counts else float(N) / len(rows) for r in rows]
    mean = sum(wr * np.asarray(r[0], np.float64) for wr, r in zip(w, rows)) / N
    var = sum(wr * np.asarray(r[1], np.float64) for wr, r in zip(w, rows))
    if between:
        var = var + sum(wr * (np.asarray(r[0], np.float64) - mean) ** 2 for wr, r in zip(w, rows))
    return mean, var / N, N


def backward_formula(z, gy, gamma, mean, var, shards, local_sums=False):
    """gz of plain BatchNorm (no ReLU) in float64 from the explicit formula gz = a (g - sum g / N - xhat sum g xhat / N), a =
    gamma invstd, with the statistics and N of the WHOLE batch; ``local_sums`` is the mutation: every shard uses its own
    two sums (the all-reduce forgotten)"""
    z, gy, gamma = z.double(), gy.double(), gamma.double().view(1, -1, 1, 1)
    mean, invstd = torch.as_tensor(mean).view(1, -1, 1, 1), torch.rsqrt(torch.as_tensor(var) + EPS).view(1, -1, 1, 1)
    N = z.shape[0] * z.shape[2] * z.shape[3]
    xh = (z - mean) * invstd
    out = []
    for g, x in zip(split(gy, shards) if local_sums else [gy], split(xh, shards) if local_sums else [xh]):
        sg, sgx = g.sum((0, 2, 3), keepdim=True), (g * x).sum((0, 2, 3), keepdim=True)
        out.append(gamma * invstd * (g - sg / N - x * sgx / N))
    return torch.cat(out, 0)


def fp32_rows(z, shards):
    """What ``ct_bn_stats_row`` leaves per shard, restated in numpy float32 (the summation order is sequential here, slab-wise
    on the device: the last bits differ, the sizes do not): [(mean, var about the rounded mean, resid, pixels)] with the
    kernel's arithmetic -- pivot = pixel 0, mean = pivot + sum(z - pivot) / P, resid by the two-sum, var = sum (z - mean)^2 / P"""
    f = np.float32
    rows = []
    for zs in split(z, shards):
        a = zs.permute(1, 0, 2, 3).reshape(zs.shape[1], -1).numpy().astype(f)          # [C, P], pixel 0 first
        P, pivot = a.shape[1], a[:, 0].copy()
        s0 = np.zeros(len(pivot), f)
        for j in range(P):
            s0 = (s0 + (a[:, j] - pivot)).astype(f)
        q = (s0 / f(P)).astype(f)
        m = (pivot + q).astype(f)
        bb = (m - pivot).astype(f)
        resid = ((pivot - (m - bb).astype(f)).astype(f) + (q - bb).astype(f)).astype(f)
        s1 = np.zeros(len(pivot), f)
        for j in range(P):
            d = (a[:, j] - m).astype(f)
            s1 = (s1 + (d * d).astype(f)).astype(f)
        rows.append((m, (s1 / f(P)).astype(f), resid, P))
    return rows


def merge_fp32_rows(rows, refine):
    """``bn_merge_kernel`` in numpy float64 over ``fp32_rows`` -> (mean, var); ``refine=False`` ignores the resid column (the
    first version of the row, [mean | var | count])"""
    N = sum(r[3] for r in rows)
    mr = [r[0].astype(np.float64) + (r[2].astype(np.float64) if refine else 0.0) for r in rows]
    vr = [r[1].astype(np.float64) - (r[2].astype(np.float64) ** 2 if refine else 0.0) for r in rows]
    mean = sum(r[3] * x for r, x in zip(rows, mr)) / N
    var = (sum(r[3] * x for r, x in zip(rows, vr)) + sum(r[3] * (x - mean) ** 2 for r, x in zip(rows, mr))) / N
    return mean, np.where(var < 0, 0.0, var)


# ---------------------------------------------------------------------------------------------------------------------
# the truth on the whole batch

def reference(case, dtype, form, mask=None):
    """F.batch_norm (+ res) + ReLU on the concatenated batch in ``dtype`` with autograd; ``mask`` (NCHW 0/1) replaces the ReLU"""
    z, gamma, beta, rm, rv, gy = (t.to(dtype) for t in case[:6])
    res = case[6].to(dtype) if form == 'backbone' else None
    leaves = [t.clone().requires_grad_() for t in ((z, gamma, beta) if res is None else (z, gamma, beta, res))]
    pre = F.batch_norm(leaves[0], rm.clone(), rv.clone(), leaves[1], leaves[2], True, NB.MOMENTUM, EPS)
    if res is not None:
        pre = pre + leaves[3]
    y = torch.relu(pre) if mask is None else pre * mask.to(dtype)
    gs = torch.autograd.grad(y, leaves, gy)
    zd = z.detach()
    out = dict(pre=pre.detach(), y=y.detach(), gz=gs[0], gg=gs[1], gb=gs[2], mean=zd.mean((0, 2, 3)),
               var=zd.var((0, 2, 3), unbiased=False))
    if res is not None:
        out['gres'] = gs[3]
    return out


def running_reference(zs, dtype):
    """running (mean, var) after training calls on the whole batches ``zs``, from (0, 1)"""
    C = zs[0].shape[1]
    rm, rv = torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    for z in zs:
        F.batch_norm(z.to(dtype), rm, rv, None, None, True, NB.MOMENTUM, EPS)
    return rm, rv


# ---------------------------------------------------------------------------------------------------------------------
# the ops on a device

def nhwc_view(t, dev, sliced):
    """NCHW CPU tensor -> NHWC view on the device; ``sliced``: channels 4 .. 4 + C of a buffer 8 channels wider"""
    from centertrack_amd import ops
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, C + 8 if sliced else C), 7.0, dtype=torch.float32)
    c0 = 4 if sliced else 0
    buf[..., c0:c0 + C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(dev), c0, C)


class Shard(object):
    """one shard's views on the device"""

    def __init__(self, case, shards, r, form, dev):
        C = case[0].shape[1]
        sliced = C == 8
        self.z = nhwc_view(split(case[0], shards)[r], dev, sliced)
        self.gy = nhwc_view(split(case[5], shards)[r], dev, sliced)
        self.res = nhwc_view(split(case[6], shards)[r], dev, sliced) if form == 'backbone' else None
        self.gamma, self.beta = case[1].to(dev), case[2].to(dev)


def forward_ops(sh, form, m):
    from centertrack_amd import ops
    if form == 'neck':
        return ops.bn_relu_apply(sh.z, m.mean, m.invstd, sh.gamma, m.beta)
    return ops.bn_act_apply(sh.z, m.mean, m.invstd, sh.gamma, m.beta, res=sh.res, relu=True)


def sums_ops(sh, form, m):
    from centertrack_amd import ops
    if form == 'neck':
        return ops.bn_relu_backward_sums(sh.z, sh.gy, m.mean, m.invstd, sh.gamma, m.beta)
    return ops.bn_act_backward_sums(sh.z, sh.gy, m.mean, m.invstd, sh.gamma, m.beta, res=sh.res, relu=True)


def apply_ops(sh, form, m, sums):
    """-> (gz, gres) as NHWC views (gres None on the neck form)"""
    from centertrack_amd import ops
    if form == 'neck':
        return ops.bn_relu_backward_apply(sh.z, sh.gy, m.mean, m.invstd, sh.gamma, m.beta, sums, m.inv_count), None
    return ops.bn_act_backward_apply(sh.z, sh.gy, m.mean, m.invstd, sh.gamma, m.beta, sums, m.inv_count, res=sh.res,
                                     relu=True, need_z=True, need_res=True)


def merged_vectors(m):
    return [m.mean, m.var, m.invstd, m.unbiased, m.inv_count, m.count] + ([m.beta] if m.beta is not None else [])


def emulate(case, shards, form, dev):
    """Every rank in one process: ``ct_bn_stats`` per shard into its row, ``ct_bn_merge_stats``, apply per shard, sums per shard
    added in rank order, the apply half per shard -> dict(rows, m, local_invstd, y, sums (per shard), total, gz, gres)"""
    from centertrack_amd import ops
    C = case[0].shape[1]
    world = len(shards)
    sh = [Shard(case, shards, r, form, dev) for r in range(world)]
    rows = torch.empty((world, ops.bn_row_floats(C)), dtype=torch.float32, device=dev)
    local_invstd = [ops.bn_stats_row(sh[r].z, EPS, rows[r]) for r in range(world)]
    m = ops.bn_merge_stats(rows, C, EPS, gamma=sh[0].gamma, beta=sh[0].beta)      # (m.beta takes beta's place from here on)
    y = [forward_ops(s, form, m) for s in sh]
    sums = [sums_ops(s, form, m) for s in sh]
    total = sums[0].clone()
    for s in sums[1:]:
        total += s
    back = [apply_ops(s, form, m, total) for s in sh]
    return dict(rows=rows, m=m, local_invstd=local_invstd, y=y, sums=sums, total=total, gz=[b[0] for b in back],
                gres=[b[1] for b in back])


def through_group(case, shards, form, rank, dev, group=None):
    """This rank's shard through a real process group: the row, ``all_gather_rows``, the merge, apply, the local sums,
    ``all_reduce_flat``, the apply half -> dict(rows, m, y, sums (local), total, gz, gres)"""
    from centertrack_amd import ops, parallel
    C = case[0].shape[1]
    s = Shard(case, shards, rank, form, dev)
    row = torch.empty(ops.bn_row_floats(C), dtype=torch.float32, device=dev)
    ops.bn_stats_row(s.z, EPS, row)
    rows = parallel.all_gather_rows(row, group)
    m = ops.bn_merge_stats(rows, C, EPS, gamma=s.gamma, beta=s.beta)
    y = forward_ops(s, form, m)
    sums = sums_ops(s, form, m)
    total = parallel.all_reduce_flat(sums.clone(), group)
    gz, gres = apply_ops(s, form, m, total)
    return dict(rows=rows, m=m, y=y, sums=sums, total=total, gz=gz, gres=gres)


def nchw(v):
    return v.to_nchw().cpu()


def cat_nchw(views):
    return torch.cat([nchw(v) for v in views], 0)
