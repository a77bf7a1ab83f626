"""The training loss as plain torch formulas on RAW head outputs, in whatever dtype the inputs have (float64 for the
truth of the tests, float32 as the composed-from-torch-ops baseline of tools/loss_bench.py).  Written from the formulas
the kernels implement (include/centertrack_hip.h); tests/test_losses_cpu.py pins it to the
reference's own numbers (tests/golden/losses.npz).  No GPU code, no ctypes.

A batch is a dict with the reference's keys (hm, ind, mask, cat, reg, reg_mask, ..., hp_ind, hm_hp_mask, joint, rotbin,
rotres, rot_mask); ``outputs`` maps head -> logits [B,C,H,W]."""
import math
import os

import numpy as np
import torch

L1_HEADS = ('reg', 'wh', 'tracking', 'ltrb', 'ltrb_amodal', 'hps', 'dim', 'amodel_offset', 'velocity', 'hp_offset')
ALL_HEADS = ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity')
HEAD_CH = {'hm': None, 'hm_hp': 17, 'reg': 2, 'wh': 2, 'tracking': 2, 'ltrb': 4, 'ltrb_amodal': 4, 'hps': 34, 'dep': 1,
           'rot': 8, 'dim': 3, 'amodel_offset': 2, 'nuscenes_att': 8, 'velocity': 3, 'hp_offset': 2}


def gather(x, ind):
    """x [B,C,H,W], ind [B,M] -> x[b, :, ind[b, m]] as [B,M,C]"""
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).permute(0, 2, 1).gather(1, ind.unsqueeze(2).expand(B, ind.shape[1], C))


def focal(x, gt, ind, mask, cat):
    p = torch.sigmoid(x).clamp(min=1e-4, max=1 - 1e-4)
    neg = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4).sum()
    pp = gather(p, ind).gather(2, cat.unsqueeze(2)).squeeze(2)
    mask = mask.to(x.dtype)
    pos = (torch.log(pp) * (1 - pp) ** 2 * mask).sum()
    num_pos = mask.sum()
    return -neg if float(num_pos) == 0 else -(pos + neg) / num_pos


def weighted_l1(x, mask, ind, target, depth=False):
    if depth:
        x = 1. / (torch.sigmoid(x) + 1e-6) - 1.
    mask = mask.to(x.dtype)
    pred = gather(x, ind)
    return (pred * mask - target * mask).abs().sum() / (mask.sum() + 1e-4)


def weighted_bce(x, mask, ind, target):
    z = gather(x, ind)
    mask = mask.to(x.dtype)
    bce = z.clamp(min=0) - z * target + torch.log1p(torch.exp(-z.abs()))
    return (mask * bce).sum() / (mask.sum() + 1e-4)


def _smooth_l1(d):
    # (torch's own op, as the reference calls it: a torch.where of the two branches would differentiate the branch not taken as
    # well, 0 * Inf = NaN at an infinite d; tests/test_nonfinite_cpu.py)
    return torch.nn.functional.smooth_l1_loss(d, torch.zeros_like(d), reduction='none')


def bin_rot(x, mask, ind, rotbin, rotres):
    """bin logits times the mask, cross-entropy mean over ALL rows; sin / cos smooth-L1 means over the rows with a non-zero
    target bin, NOT masked; a residual term without such a row is 0"""
    pred = gather(x, ind).reshape(-1, 8)
    tb, tr, m = rotbin.reshape(-1, 2), rotres.reshape(-1, 2).to(x.dtype), mask.reshape(-1, 1).to(x.dtype)
    loss = 0
    for k in (0, 1):
        z = pred[:, 4 * k:4 * k + 2] * m
        # log_softmax, as the reference's cross_entropy: z - max - log(sum(exp(z - max))) meets Inf - Inf at an infinite logit
        # and is NaN there, where torch.logsumexp would answer Inf
        loss = loss - torch.log_softmax(z, 1).gather(1, tb[:, k:k + 1]).squeeze(1).mean()
        rows = tb[:, k] != 0
        if bool(rows.any()):
            loss = loss + _smooth_l1(pred[rows, 4 * k + 2] - torch.sin(tr[rows, k])).mean()
            loss = loss + _smooth_l1(pred[rows, 4 * k + 3] - torch.cos(tr[rows, k])).mean()
    return loss


def head_loss(head, x, batch):
    if head == 'hm':
        return focal(x, batch['hm'].to(x.dtype), batch['ind'], batch['mask'], batch['cat'])
    if head == 'hm_hp':
        return focal(x, batch['hm_hp'].to(x.dtype), batch['hp_ind'], batch['hm_hp_mask'], batch['joint'])
    if head == 'rot':
        return bin_rot(x, batch['rot_mask'], batch['ind'], batch['rotbin'], batch['rotres'])
    ind = batch['hp_ind'] if head == 'hp_offset' else batch['ind']
    if head == 'nuscenes_att':
        return weighted_bce(x, batch[head + '_mask'], ind, batch[head].to(x.dtype))
    return weighted_l1(x, batch[head + '_mask'], ind, batch[head].to(x.dtype), depth=head == 'dep')


def generic_loss(outputs, batch, heads, weights, num_stacks=1):
    """(tot, {head: loss}) of ``outputs`` = a list of num_stacks dicts"""
    losses = {h: 0 for h in heads}
    for s in range(num_stacks):
        for h in heads:
            if h in outputs[s]:
                losses[h] = losses[h] + head_loss(h, outputs[s][h], batch) / num_stacks
    tot = 0
    for h in heads:
        tot = tot + weights[h] * losses[h]
    return tot, losses


def losses_and_grads(outputs, batch, heads, dtype=torch.float64, device=None):
    """per head (loss, d loss / d logits) in ``dtype`` from fp32 inputs"""
    res = {}
    for h in heads:
        x = outputs[h].detach().to(device=device or outputs[h].device, dtype=dtype).requires_grad_()
        b = {k: (v.to(device=x.device, dtype=dtype) if v.is_floating_point() else v.to(x.device)) for k, v in batch.items()}
        loss = head_loss(h, x, b)
        g, = torch.autograd.grad(loss, x)
        res[h] = (loss.detach(), g)
    return res


def terms(head, x_shape, M):
    """K, the number of summed terms behind a loss: B*C*H*W for a focal head, B*M*C for a slot head"""
    B, C, H, W = x_shape
    return B * C * H * W if head in ('hm', 'hm_hp') else B * M * C


def err(a, ref, norm=None):
    """the measure of tests/_dcn_bwd.py: max error over the largest reference magnitude"""
    ref = ref.double()
    n = float(ref.abs().max()) if norm is None else norm
    return float((a.double().cpu() - ref.cpu()).abs().max()) / (n if n > 0 else 1.0)


def bound(e32, K):
    return min(1e-3, 4.0 * max(e32, 2.0 ** -23 * math.sqrt(K)))


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def away_from_clamp(x, margin=1e-3, edge=9.2102):
    """push logits that lie within ``margin`` of +-edge (where clamp(sigmoid(x), 1e-4, 1 - 1e-4) starts to act) out of
    that band, so that float32 and float64 agree on which side they fall"""
    for e in (edge, -edge):
        near = (x - e).abs() < 2 * margin
        x = torch.where(near, torch.full_like(x, e + 4 * margin), x)
    return x


def make_batch(seed, B, H, W, M, heads, num_classes, valid=None, scale=3.0, joints=17):
    """(outputs {head: fp32 logits}, batch) with the reference's keys; ``valid[b]`` = objects of image b (default M // 2 + b)"""
    g = _gen(seed)
    HW = H * W
    valid = [min(M, M // 2 + b) for b in range(B)] if valid is None else valid
    mask = torch.zeros(B, M)
    ind = torch.zeros(B, M, dtype=torch.int64)
    cat = torch.zeros(B, M, dtype=torch.int64)
    for b in range(B):
        n = valid[b]
        mask[b, :n] = 1
        ind[b, :n] = torch.randint(0, HW, (n,), generator=g)
        cat[b, :n] = torch.randint(0, num_classes, (n,), generator=g)
    batch = {'ind': ind, 'mask': mask, 'cat': cat}
    outputs = {}
    for h in heads:
        C = num_classes if h == 'hm' else joints if h == 'hm_hp' else HEAD_CH[h]
        outputs[h] = away_from_clamp(torch.randn(B, C, H, W, generator=g) * scale)
        if h == 'hm':
            hm = torch.rand(B, C, H, W, generator=g) ** 4
            for b in range(B):
                for m in range(valid[b]):
                    hm[b, cat[b, m], ind[b, m] // W, ind[b, m] % W] = 1
            batch['hm'] = hm
        elif h == 'hm_hp':
            hp_mask = (torch.rand(B, M, joints, generator=g) < 0.7).float() * mask.unsqueeze(2)
            hp_ind = torch.randint(0, HW, (B, M, joints), generator=g) * hp_mask.long()
            batch['hp_ind'] = hp_ind.reshape(B, M * joints)
            batch['hm_hp_mask'] = hp_mask.reshape(B, M * joints)
            batch['joint'] = torch.arange(joints).repeat(B, M).reshape(B, M * joints)
            hm = torch.rand(B, joints, H, W, generator=g) ** 4
            bi = torch.arange(B).view(B, 1).expand(B, M * joints)
            sel = batch['hm_hp_mask'] > 0
            hm[bi[sel], batch['joint'][sel], batch['hp_ind'][sel] // W, batch['hp_ind'][sel] % W] = 1
            batch['hm_hp'] = hm
        elif h == 'hp_offset':
            if 'hm_hp_mask' not in batch:
                raise ValueError('list hm_hp before hp_offset')
            batch['hp_offset'] = torch.rand(B, M * joints, 2, generator=g)
            batch['hp_offset_mask'] = batch['hm_hp_mask'].unsqueeze(2).expand(B, M * joints, 2).contiguous()
        elif h == 'rot':
            batch['rotbin'] = torch.randint(0, 2, (B, M, 2), generator=g)     # (not masked: the residual terms are not either)
            batch['rotres'] = (torch.rand(B, M, 2, generator=g) - 0.5) * 3
            batch['rot_mask'] = mask.clone()
        elif h == 'nuscenes_att':
            batch[h] = (torch.rand(B, M, 8, generator=g) < 0.3).float()
            batch[h + '_mask'] = (torch.rand(B, M, 8, generator=g) < 0.5).float() * mask.unsqueeze(2)
        else:
            C = HEAD_CH[h]
            batch[h] = torch.randn(B, M, C, generator=g) * 2
            if h == 'dep':
                batch[h] = batch[h].abs() * 10 + 1
            batch[h + '_mask'] = mask.unsqueeze(2).expand(B, M, C).contiguous()
    return outputs, batch


class Opt(object):
    def __init__(self, heads, weights=None, num_stacks=1):
        self.heads = {h: 0 for h in heads}
        self.weights = {h: (0.1 if h == 'wh' else 1.0) for h in heads}
        if weights:
            self.weights.update(weights)
        self.num_stacks = num_stacks


# ---------------------------------------------------------------------------------------------------------------------
# training scale: the inputs of tests/test_hip_losses_scale.py, shared with the CPU checks of tests/test_losses_cpu.py

DENSE_THREADS = 256                      # LOSS_DENSE_THREADS of csrc/loss.hip
MAX_PARTIALS = 1024                      # LOSS_MAX_PARTIALS
TRIP = 4 * DENSE_THREADS * MAX_PARTIALS  # elements one trip of the capped grid covers on the float4 path (1,048,576)
CAP = 4 * TRIP                           # loss_plan gives a workgroup 4 trips; above 4,194,304 elements the grid stays 1024
MAX_SLOTS = 8192                         # CT_LOSS_MAX_SLOTS of include/centertrack_hip.h
SCALE = (2, 80, 128, 208, 16)            # B, C, H, W, M: 4,259,840 elements, the smallest COCO-like map above CAP
SHARE_TOL = 1.0 / (8 * MAX_PARTIALS)     # the loss bound that sees one lost or doubled partial
FIFTEEN = ('hm', 'reg', 'wh', 'tracking', 'ltrb', 'ltrb_amodal', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att',
           'velocity', 'hm_hp', 'hps', 'hp_offset')

_scale_cache = {}


def _once(key, make):
    if key not in _scale_cache:
        _scale_cache[key] = make()
    return _scale_cache[key]


def loss_err(got, want):
    """relative; a zero truth wants a zero"""
    got, want = float(got), float(want)
    if want == 0.0:
        return 0.0 if got == 0.0 else float('inf')
    return abs(got - want) / abs(want)


def truth_and_e32(key, out, batch, heads):
    """({head: (loss, grad)} in float64, {head: (loss error, gradient error)} of the float32 mirror), once per process"""
    def make():
        w64 = losses_and_grads(out, batch, heads, torch.float64)
        w32 = losses_and_grads(out, batch, heads, torch.float32)
        return w64, {h: (loss_err(w32[h][0], w64[h][0]), err(w32[h][1], w64[h][1])) for h in heads}
    return _once(('truth', key), make)


def scale_batch():
    """A1: random logits and targets above the partial cap"""
    B, C, H, W, M = SCALE
    return _once('scale', lambda: make_batch(41, B, H, W, M, ('hm',), C))


def positive_elements(batch, shape):
    """flat element indices of the positives (b, cat, ind) of a focal head of ``shape`` = [B,C,H,W]"""
    B, C, H, W = shape
    b = torch.arange(B).view(B, 1).expand_as(batch['ind'])
    sel = batch['mask'] > 0
    return ((b[sel] * C + batch['cat'][sel]) * (H * W) + batch['ind'][sel]).tolist()


def partial_shares(x, batch, vec):
    """float64 [MAX_PARTIALS]: the part of the loss that each workgroup's partial of loss_dense_fwd_kernel carries, i.e.
    partial / (pos + neg).  Element i belongs to workgroup (i // 4 // 256) % 1024 on the float4 path and to
    (i // 256) % 1024 on the scalar path (more than CAP elements, so the grid is capped at 1024)."""
    n = x.numel()
    assert n % 4 == 0 and n > CAP
    xd, gt = x.double(), batch['hm'].double()
    p = torch.sigmoid(xd).clamp(min=1e-4, max=1 - 1e-4)
    t = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4).reshape(-1)
    i = torch.arange(n)
    wg = ((i // 4 if vec else i) // DENSE_THREADS) % MAX_PARTIALS
    part = torch.zeros(MAX_PARTIALS, dtype=torch.float64).index_add_(0, wg, t)
    pp = gather(p, batch['ind']).gather(2, batch['cat'].unsqueeze(2)).squeeze(2)
    pos = (torch.log(pp) * (1 - pp) ** 2 * batch['mask'].double()).sum()
    assert abs(float(part.sum() - t.sum())) <= 1e-9 * abs(float(t.sum()))
    return part / (pos + t.sum())


def scale_shares(vec):
    out, batch = scale_batch()
    return _once(('shares', vec), lambda: partial_shares(out['hm'], batch, vec))


def probe_indices(n):
    """A2: both ends, the elements beside the first and the last float4, both sides of every trip boundary, the middle"""
    S = TRIP
    return [0, 3, 4, n - 1, n - 4, n - 5, S - 1, S, S + 1, 3 * S - 1, 3 * S, n // 2]


def probe_batch():
    """A2: the inputs of A1 with a target of 1 everywhere but at the 12 probes (target 0): every other negative term is
    exactly 0, so the loss is the 12 probe terms and the positives.  Probe k has the logit 0.5 + k / 4: twelve different
    terms between 0.37 and 4.5, each a visible part of the loss, so that a lost probe is not made up for by a doubled one"""
    def make():
        out, batch = scale_batch()
        probes = probe_indices(out['hm'].numel())
        x = out['hm'].clone()
        x.view(-1)[probes] = 0.5 + 0.25 * torch.arange(len(probes))
        hm = torch.ones_like(batch['hm'])
        hm.view(-1)[probes] = 0
        return {'hm': x}, dict(batch, hm=hm), probes
    return _once('probes', make)


def slot_limit_batch():
    """A3: hp_ind with M = 512 * 16 = MAX_SLOTS slots over 16 * 24 = 384 positions, (nearly) every object valid: a position
    is named by about 15 live slots spread over the 32 scatter workgroups of its image, and position 0 by the masked ones"""
    heads = ('hm', 'reg', 'hm_hp', 'hp_offset')
    return _once('slots', lambda: make_batch(43, 2, 16, 24, 512, heads, 3, valid=[512, 509], joints=16) + (heads,))


def fifteen_batch():
    """A4: every head of losses.KNOWN_HEADS"""
    return _once('fifteen', lambda: make_batch(44, 2, 8, 12, 8, FIFTEEN, 3))


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/losses.npz

CASES = ('A', 'B', 'C')


def load_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, 'losses.npz'))
    heads = str(z['%s/heads' % name].reshape(-1)[0]).split(',')
    pick = lambda prefix: {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}
    return dict(heads=heads, out=pick('%s/out/' % name), batch=pick('%s/batch/' % name), loss=pick('%s/loss/' % name),
                grad=pick('%s/grad/' % name), e32_loss=pick('%s/e32_loss/' % name), e32_grad=pick('%s/e32_grad/' % name))
