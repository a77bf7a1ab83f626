"""Shared pieces of the DCNv2 backward tests (tests/test_dcn_backward_cpu.py, tests/test_hip_dcn_backward.py): the inputs
and the error measure, a float64 truth whose sample positions are the kernel's, a pure-Python mirror of ``make_plan``
(centertrack_amd/csrc/dcn_bwd.hip) and the list of shapes that reaches every regime of it.  No GPU, no ctypes."""
import math

import torch

NAMES = ('x', 'offset', 'mask', 'weight', 'bias')


def randn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def inputs(shape):
    """fp32 (x, offset, mask, weight, bias, gy) of a (B, Cin, Cout, H, W, offset scale)"""
    B, Cin, Cout, H, W, scale = shape
    t = (randn(1, B, Cin, H, W), randn(2, B, 18, H, W) * scale, torch.sigmoid(randn(3, B, 9, H, W)),
         randn(4, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5, randn(5, Cout), randn(6, B, Cout, H, W))
    return [v.float() for v in t]


def terms(shape):
    """K, the number of terms behind one element of each gradient"""
    B, Cin, Cout, H, W = shape[:5]
    return {'x': 36 * Cout, 'offset': Cin * Cout, 'mask': Cin * Cout, 'weight': B * H * W, 'bias': B * H * W}


def err(g, g64, norm=None):
    return float((g.double() - g64).abs().max() / (g64.abs().max() if norm is None else norm))


def bound(e32, K):
    return min(1e-3, 4.0 * max(e32, 2.0 ** -23 * math.sqrt(K)))


def shape_id(shape):
    return 'x'.join(str(v) for v in shape)


# ---------------------------------------------------------------------------------------------------------------------
# a float64 truth at the kernel's sample positions

def tap_bases(H, W, dtype=torch.float64):
    """[18, H, W]: channel 2k = h - 1 + k // 3, channel 2k + 1 = w - 1 + k % 3 (the integer part of a sample position)"""
    h = torch.arange(H, dtype=dtype).view(H, 1).expand(H, W)
    w = torch.arange(W, dtype=dtype).view(1, W).expand(H, W)
    rows = []
    for k in range(9):
        rows += [h - 1 + k // 3, w - 1 + k % 3]
    return torch.stack(rows)


def effective_offsets(offset_fp32, H, W):
    """float64(fl32(fl32(base) + d)) - base per tap and axis.  The kernel and the float32 oracle form a sample
    coordinate as one fp32 add of the offset to a small integer; the float64 oracle fed the same fp32 offset forms the
    exact sum, up to 7.6e-6 px away and on the other side of an integer where the fp32 sum rounds onto it.  Fed THESE
    offsets, base + offset is exact in float64 and equals the fp32 coordinate bit for bit, so floor, the validity
    rules and the bilinear weights are those of the kernel for every input; d(position) / d(offset) = 1 either way, so
    the gradients are those of the same function."""
    assert offset_fp32.dtype == torch.float32 and tuple(offset_fp32.shape[1:]) == (18, H, W)
    pos32 = tap_bases(H, W, torch.float32).unsqueeze(0) + offset_fp32           # the one fp32 add
    return pos32.double() - tap_bases(H, W).unsqueeze(0)


def oracle_grads(inp, dtype, effective=False):
    """autograd of the oracle in ``dtype`` on the fp32 inputs (x, offset, mask, weight, bias, gy) -> {name: gradient}"""
    from oracle import dcn_v2 as odcn
    t = [v.clone().to(dtype) for v in inp[:5]]
    if effective:
        assert dtype == torch.float64
        t[1] = effective_offsets(inp[1], inp[1].shape[2], inp[1].shape[3])
    t = [v.requires_grad_() for v in t]
    y = odcn.dcn_v2_conv(*t)
    return dict(zip(NAMES, torch.autograd.grad(y, t, inp[5].to(dtype))))


def truth(inp):
    """(float64 gradients at the kernel's positions, e(oracle32) per tensor against them); the float32 yardstick keeps
    the original offsets"""
    g64 = oracle_grads(inp, torch.float64, effective=True)
    g32 = oracle_grads(inp, torch.float32)
    return g64, {n: err(g32[n], g64[n]) for n in NAMES}


_truth_cache = {}


def truth_of_shape(shape):
    """(inputs, g64, e(oracle32)) of ``inputs(shape)``, computed once per process"""
    if shape not in _truth_cache:
        inp = inputs(shape)
        _truth_cache[shape] = (inp,) + truth(inp)
    return _truth_cache[shape]


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan, restated

def cdiv(a, b):
    return -(-a // b)


def plan(B, Cin, Cout, H, W):
    """make_plan of dcn_bwd.hip in Python, plus what follows from it inside dcn_bwd_weight_kernel.  ``slabs`` is checked
    against the library through ct_dcn_v2_backward_workspace_bytes (tests/test_dcn_backward_cpu.py); CS is not
    observable through the ABI and is mirrored by reading."""
    NT = cdiv(Cout, 16)
    tilesPerImg = cdiv(H * W, 16)
    tiles = B * tilesPerImg
    if tiles >= 1024 or Cin < 64:
        CS = 1
    elif tiles >= 512 or Cin < 128:
        CS = 2
    else:
        CS = 4
    groups = cdiv(NT, 4)
    units = 9 * (Cin // 32) * groups
    nsteps = cdiv(B * H * W, 4)
    wanted, maxSlabs = cdiv(1024, units), cdiv(nsteps, 32)
    slabs = max(1, min(wanted, maxSlabs))
    spw = cdiv(nsteps, slabs * 4)
    waves = slabs * 4
    return dict(NT=NT, tilesPerImg=tilesPerImg, tiles=tiles, CS=CS, units=units, nsteps=nsteps, slabs=slabs,
                capped=wanted > maxSlabs, stepsPerWave=spw, groups=groups, nco_last=NT - (groups - 1) * 4,
                idle_steps=waves * spw - nsteps, idle_waves=waves - cdiv(nsteps, spw))


def neck_shapes(S=512):
    """(Cin, Cout, H = W) of the seven distinct DeformConv shapes of the DLA-34 neck (tools/dcn_bwd_bench.py::shapes)"""
    return [(512, 256, S // 32), (256, 256, S // 16), (256, 128, S // 16), (128, 128, S // 8), (128, 64, S // 8),
            (256, 64, S // 16), (64, 64, S // 4)]


# (B, Cin, Cout, H, W, offset scale).  The neck at 512x512: all seven at batch 1, at batch 4 the four whose regime changes
# (CS 4 -> 1, stepsPerWave 18 -> 69 and 9 -> 36, a capped slab count -> an uncapped one); offsets of scale 2 px, 0.5 px on the 16x16 map.
PLAN_SHAPES = [(1, ci, co, s, s, 0.5 if s == 16 else 2.0) for ci, co, s in neck_shapes()] + [
    (4, 128, 128, 64, 64, 2.0), (4, 128, 64, 64, 64, 2.0), (4, 256, 64, 32, 32, 2.0), (4, 64, 64, 128, 128, 2.0),
    # small shapes for what the neck does not reach:
    (1, 32, 16, 6, 7, 2.0),        # Cin 32 (CS 1 by Cin), one slab, stepsPerWave 3, H*W % 16 and N*H*W % 4 non-zero
    (3, 32, 72, 11, 13, 2.0),      # three images, Cout 72: a second cout group of ONE ragged tile, stepsPerWave 7
    (1, 64, 200, 9, 9, 2.0),       # four cout groups, the last one tile wide and ragged (200 = 12 * 16 + 8)
    (1, 64, 512, 8, 8, 2.0),       # the largest Cout: 33 KB gy tile in LDS, eight cout groups
    (1, 256, 128, 29, 47, 2.0),    # eight uncapped slabs, stepsPerWave 11, ragged pixel tile, N*H*W % 4 == 3
]


def _regimes():
    """name -> predicate over (shape, plan): everything make_plan and the kernels branch on"""
    r = {}
    for cs in (1, 2, 4):
        r['CS == %d' % cs] = lambda s, p, cs=cs: p['CS'] == cs
    r['CS == 1 because tiles >= 1024'] = lambda s, p: p['tiles'] >= 1024 and s[1] >= 64
    r['CS == 1 because Cin < 64'] = lambda s, p: p['tiles'] < 1024 and s[1] < 64
    r['slabs from cdiv(1024, units)'] = lambda s, p: not p['capped']
    r['slabs cut by maxSlabs'] = lambda s, p: p['capped']
    r['slabs == 1'] = lambda s, p: p['slabs'] == 1
    for m in (0, 1, 2, 3):
        r['stepsPerWave %% 4 == %d' % m] = lambda s, p, m=m: p['stepsPerWave'] % 4 == m
    r['a whole idle wave'] = lambda s, p: p['idle_waves'] >= 1
    r['cout groups == 1'] = lambda s, p: p['groups'] == 1
    r['cout groups == 2'] = lambda s, p: p['groups'] == 2
    r['cout groups >= 4'] = lambda s, p: p['groups'] >= 4
    r['a last cout group with nco == 1'] = lambda s, p: p['groups'] > 1 and p['nco_last'] == 1
    r['Cout % 16 != 0 with more than one group'] = lambda s, p: s[2] % 16 != 0 and p['groups'] > 1
    r['Cin == 32'] = lambda s, p: s[1] == 32
    r['Cout == 512'] = lambda s, p: s[2] == 512
    r['H*W % 16 != 0'] = lambda s, p: (s[3] * s[4]) % 16 != 0
    r['N*H*W % 4 != 0'] = lambda s, p: (s[0] * s[3] * s[4]) % 4 != 0
    r['N >= 3'] = lambda s, p: s[0] >= 3
    return r


REGIMES = _regimes()


def missing_regimes(shapes):
    """names of the regimes no shape of the list reaches"""
    plans = [(s, plan(*s[:5])) for s in shapes]
    return [name for name, pred in REGIMES.items() if not any(pred(s, p) for s, p in plans)]


# ---------------------------------------------------------------------------------------------------------------------
# designed sample positions

def axis_targets(L):
    """where the validity rules live: outside (strict at -1 and L), the half-valid first and last cell, integers"""
    return [-1.5, -1.0, -0.75, -0.5, 0.0, 0.25, 1.0, L - 2.0, L - 1.5, L - 1.0, L - 0.75, L - 0.5, float(L), L + 0.5]


def designed_positions(B, H, W):
    """float64 [B, 18, H, W] sample POSITIONS (channel 2k = row, 2k + 1 = column): sample number s = ((n*H + h)*W + w)*9 + k
    gets pair s % 196 of axis_targets(H) x axis_targets(W).  Every value is a multiple of 0.25."""
    ty, tx = torch.tensor(axis_targets(H), dtype=torch.float64), torch.tensor(axis_targets(W), dtype=torch.float64)
    s = torch.arange(B * H * W * 9).view(B, H, W, 9) % 196
    pos = torch.empty(B, 18, H, W, dtype=torch.float64)
    pos[:, 0::2] = ty[s // 14].permute(0, 3, 1, 2)
    pos[:, 1::2] = tx[s % 14].permute(0, 3, 1, 2)
    return pos, s.permute(0, 3, 1, 2)
