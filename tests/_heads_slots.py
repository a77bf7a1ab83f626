"""Shared pieces of the slot-heads tests (tests/test_heads_slots_cpu.py, tests/test_hip_heads_slots.py): the cases, the
fixture, the float64 / float32 truth and the restatements of the two kernels of centertrack_amd/csrc/heads_slots.hip.  No GPU,
no ctypes.  Error measure and bound: tests/_dcn_bwd.py.

The truth is the reference's DENSE construction (conv3x3 -> ReLU -> conv1x1 per head, torch autograd on the CPU) read at the
slots: the loss is ``sum(gout * out)`` over the maps of the dense heads plus ``sum_{b,m valid} g[b,m] . out[b,:,ind[b,m]]`` over
the slot heads.  As in tests/_heads_bwd.py ``x``, ``w0`` and ``b0`` are dyadic, so the hidden pre-activation is exact in fp32
and no unit of the ReLU mask can differ between a float64 truth and an fp32 kernel; ``w2`` and the incoming gradients are
Gaussian."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from _dcn_bwd import bound, err  # noqa: F401  (re-exported)
from _heads_bwd import CIN, HC, NUSC, dyadic

SLOT_HEADS = ('reg', 'wh', 'tracking', 'ltrb', 'ltrb_amodal', 'hps', 'dep', 'dim', 'amodel_offset', 'velocity', 'rot',
              'nuscenes_att')
MOT = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2), ('ltrb_amodal', 4)])
POSE = OrderedDict([('hm', 80), ('hps', 34), ('hm_hp', 17), ('hp_offset', 2)])
HEAD_SETS = OrderedDict([('mot', MOT), ('nusc', NUSC), ('pose', POSE)])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _hand_placed():
    """(2,5,7,12): the four corners, an edge cell, the centre, a duplicate pair, two adjacent cells, -1 and H*W"""
    H, W = 5, 7
    a = [0, W - 1, (H - 1) * W, H * W - 1, 3, 2 * W + 3, 3 * W + 5, 3 * W + 5, W + 1, W + 2, -1, H * W]
    return torch.tensor([a, a[::-1]], dtype=torch.int64)


# name -> (B, H, W, M), ind [B,M]
CASES = OrderedDict([
    ('hand-2x5x7x12', ((2, 5, 7, 12), _hand_placed())),
    ('one-cell-1x1x1x3', ((1, 1, 1, 3), torch.tensor([[0, 1, 0]], dtype=torch.int64))),
    ('row-1x1x6x4', ((1, 1, 6, 4), torch.tensor([[0, 5, 2, 3]], dtype=torch.int64))),
    ('random-3x8x8x17', ((3, 8, 8, 17), torch.randint(0, 64, (3, 17), generator=_gen(11)))),
    ('tiles-2x16x16x129', ((2, 16, 16, 129), torch.randint(0, 256, (2, 129), generator=_gen(12)))),
    ('stack-1x6x6x40', ((1, 6, 6, 40), torch.full((1, 40), 2 * 6 + 2, dtype=torch.int64))),
    ('invalid-2x4x4x5', ((2, 4, 4, 5), torch.tensor([[-1, 16, 100, -7, 2 ** 40], [16, -1, 17, 2 ** 31, -2 ** 33]], dtype=torch.int64))),
])
COMBOS = [(c, s) for c in CASES for s in HEAD_SETS]


def combo_id(combo):
    return '%s-%s' % combo


def valid_of(ind, H, W):
    return (ind >= 0) & (ind < H * W)


def split(heads):
    """(slot heads, dense heads) of a head dict, each in the dict's order"""
    return [h for h in heads if h in SLOT_HEADS], [h for h in heads if h not in SLOT_HEADS]


def fixture(combo, seed=0):
    """fp32 CPU tensors: x [B,64,H,W], ind, per head w0, b0 (dyadic), w2, b2 and the incoming gradient ``g``: [B,c,H,W] for a
    dense head, [B,M,c] for a slot head (Gaussian)"""
    case, hs = combo
    (B, H, W, M), ind = CASES[case]
    heads = HEAD_SETS[hs]
    fx = {'x': dyadic(seed + 1, (B, CIN, H, W), 8.0), 'ind': ind, 'heads': heads, 'shape': (B, H, W, M)}
    for k in ('w0', 'b0', 'w2', 'b2', 'g'):
        fx[k] = OrderedDict()
    for j, (h, c) in enumerate(heads.items()):
        s = seed + 100 * (j + 1)
        fx['w0'][h] = dyadic(s + 1, (HC, CIN, 3, 3), 64.0)
        fx['b0'][h] = dyadic(s + 2, (HC,), 8.0)
        fx['w2'][h] = torch.randn((c, HC, 1, 1), generator=_gen(s + 3)) * HC ** -0.5
        fx['b2'][h] = torch.randn((c,), generator=_gen(s + 4))
        fx['g'][h] = torch.randn((B, M, c) if h in SLOT_HEADS else (B, c, H, W), generator=_gen(s + 5))
    return fx


def read_at(out, ind):
    """out [B,c,H,W], ind [B,M] -> [B,M,c] = out[b, :, ind[b,m]], a zero row where ind is out of range"""
    B, c, H, W = out.shape
    v = valid_of(ind, H, W)
    k = ind.clamp(0, H * W - 1)
    rows = out.reshape(B, c, H * W).permute(0, 2, 1).gather(1, k.unsqueeze(2).expand(B, k.shape[1], c))
    return torch.where(v.unsqueeze(2), rows, torch.zeros_like(rows))


def autograd(fx, dtype, heads=None):
    """torch autograd of the dense construction in ``dtype`` over ``heads`` (default: all) -> {'out': {h: [B,c,H,W] or, for a
    slot head, [B,M,c]}, 'pre': {h}, 'x', 'w0': {h}, 'b0': {h}, 'w2': {h}, 'b2': {h}}"""
    heads = list(fx['heads']) if heads is None else list(heads)
    x = fx['x'].detach().clone().to(dtype).requires_grad_()
    leaves, outs, pres = [], OrderedDict(), OrderedDict()
    tot = 0
    for h in heads:
        p = [fx[k][h].detach().clone().to(dtype).requires_grad_() for k in ('w0', 'b0', 'w2', 'b2')]
        pres[h] = F.conv2d(x, p[0], p[1], padding=1)
        o = F.conv2d(F.relu(pres[h]), p[2], p[3])
        outs[h] = read_at(o, fx['ind']) if h in SLOT_HEADS else o
        tot = tot + (outs[h] * fx['g'][h].to(dtype)).sum()
        leaves += p
    g = torch.autograd.grad(tot, [x] + leaves, allow_unused=True)
    g = [torch.zeros_like(t) if v is None else v for v, t in zip(g, [x] + leaves)]
    res = {'out': OrderedDict((h, o.detach()) for h, o in outs.items()), 'pre': OrderedDict((h, p.detach()) for h, p in pres.items()),
           'x': g[0]}
    for i, k in enumerate(('w0', 'b0', 'w2', 'b2')):
        res[k] = OrderedDict(zip(heads, g[1 + i::4]))
    return res


_cache = {}


def truth(combo):
    """(fixture, float64 autograd, float32 autograd), once per process"""
    if combo not in _cache:
        fx = fixture(combo)
        _cache[combo] = (fx, autograd(fx, torch.float64), autograd(fx, torch.float32))
    return _cache[combo]


def terms(combo):
    """K, the number of summed terms: the valid slots for a slot head's parameters, N*H*W for a dense head's, both for x"""
    (B, H, W, M), ind = CASES[combo[0]]
    nv = int(valid_of(ind, H, W).sum())
    return {'slot': nv, 'dense': B * H * W, 'x': nv + B * H * W, 'logits': HC}


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels, restated

def gather_ref(x, ind):
    """x [B,H,W,C] (NHWC), ind [B,M] -> cols [B,M,9,C] by torch indexing; what ct_slot_gather writes, bit for bit"""
    B, H, W, C = x.shape
    v = valid_of(ind, H, W)
    k = ind.clamp(0, H * W - 1)
    y, xx = k // W, k % W
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    bi = torch.arange(B).view(B, 1).expand_as(k)
    cols = torch.stack([xp[bi, y + ky, xx + kx] for ky in range(3) for kx in range(3)], 2)
    return torch.where(v.view(B, -1, 1, 1), cols, torch.zeros_like(cols))


def fold_index_add(P, ind, gx):
    """gx [B,H,W,C] + the patches P [B,M,9,C] by index_add, in the dtype of the arguments (the float64 truth of the fold)"""
    B, H, W, C = gx.shape
    out = gx.clone().view(B * H * W, C)
    v = valid_of(ind, H, W)
    k = ind.clamp(0, H * W - 1)
    y, xx = k // W, k % W
    base = torch.arange(B).view(B, 1) * (H * W)
    for ky in range(3):
        for kx in range(3):
            yc, xc = y + ky - 1, xx + kx - 1
            ok = v & (yc >= 0) & (yc < H) & (xc >= 0) & (xc < W)
            out.index_add_(0, (base + yc * W + xc)[ok], P[:, :, ky * 3 + kx][ok])
    return out.view(B, H, W, C)


def fold_owner_order(P, ind, gx):
    """ct_slot_fold restated in the dtype of the arguments: per touched cell the covering (slot, tap) pairs in ascending slot
    order, acc = the first one's value, + the others in order, cell = gx + acc.  -> (result, owner [B,H,W]: the slot that
    writes the cell or -1, count [B,H,W]: the covering slots)"""
    B, H, W, C = gx.shape
    out = gx.clone()
    owner = torch.full((B, H, W), -1, dtype=torch.int64)
    count = torch.zeros((B, H, W), dtype=torch.int64)
    for b in range(B):
        cover = OrderedDict()
        for m, k in enumerate(ind[b].tolist()):
            if not 0 <= k < H * W:
                continue
            y, x = divmod(k, W)
            for ky in range(3):
                for kx in range(3):
                    yc, xc = y + ky - 1, x + kx - 1
                    if 0 <= yc < H and 0 <= xc < W:
                        cover.setdefault((yc, xc), []).append((m, ky * 3 + kx))
        for (yc, xc), lst in cover.items():
            acc = P[b, lst[0][0], lst[0][1]].clone()
            for m, tap in lst[1:]:
                acc = acc + P[b, m, tap]
            out[b, yc, xc] = gx[b, yc, xc] + acc
            owner[b, yc, xc] = lst[0][0]
            count[b, yc, xc] = len(lst)
    return out, owner, count


def lowest_covering_slot(ind, H, W):
    """[B,H,W]: the lowest valid slot whose 3x3 neighbourhood covers the cell, -1 for none -- by comparison of all pairs, not
    by the walk of ``fold_owner_order``"""
    B, M = ind.shape
    v = valid_of(ind, H, W)
    k = ind.clamp(0, H * W - 1)
    y, x = (k // W).view(B, M, 1, 1), (k % W).view(B, M, 1, 1)
    yc, xc = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    cov = v.view(B, M, 1, 1) & ((y - yc).abs() <= 1) & ((x - xc).abs() <= 1)
    first = torch.where(cov, torch.arange(M).view(1, M, 1, 1).expand_as(cov), torch.full(cov.shape, M)).min(1).values
    return torch.where(first == M, torch.full_like(first, -1), first)


def slot_pipeline(fx, dtype):
    """The slot heads of ``fx`` as the module computes them, in ``dtype``, every step written out: gather, matmul, ReLU,
    matmul forward; the transposed matmuls and ``index_add`` as the fold backward -> the layout of ``autograd`` over the
    slot heads"""
    (B, H, W, M), ind = fx['shape'], fx['ind']
    slot, _ = split(fx['heads'])
    v = valid_of(ind, H, W).view(B * M, 1).to(dtype)
    cols = gather_ref(fx['x'].to(dtype).permute(0, 2, 3, 1).contiguous(), ind).view(B * M, 9 * CIN)
    res = {k: OrderedDict() for k in ('out', 'w0', 'b0', 'w2', 'b2')}
    P = torch.zeros((B * M, 9 * CIN), dtype=dtype)
    for h in slot:
        w0 = fx['w0'][h].to(dtype).permute(0, 2, 3, 1).reshape(HC, 9 * CIN)
        w2 = fx['w2'][h].to(dtype).view(-1, HC)
        hid = torch.relu(cols @ w0.t() + fx['b0'][h].to(dtype))
        res['out'][h] = ((hid @ w2.t() + fx['b2'][h].to(dtype)) * v).view(B, M, -1)
        g = fx['g'][h].to(dtype).view(B * M, -1) * v
        ghid = (g @ w2) * (hid > 0).to(dtype)
        res['w2'][h] = (g.t() @ hid).view(fx['w2'][h].shape)
        res['b2'][h] = g.sum(0)
        res['w0'][h] = (ghid.t() @ cols).view(HC, 3, 3, CIN).permute(0, 3, 1, 2)
        res['b0'][h] = ghid.sum(0)
        P = P + ghid @ w0
    gx = fold_index_add(P.view(B, M, 9, CIN), ind, torch.zeros((B, H, W, CIN), dtype=dtype))
    res['x'] = gx.permute(0, 3, 1, 2)
    return res
