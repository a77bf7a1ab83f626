"""Shared pieces of the trainable-stem tests (tests/test_stem_backward_cpu.py, tests/test_hip_stem_backward.py) and of the
``DLASeg`` tests: the launch plans of centertrack_amd/csrc/stem_train.hip restated, the table of what they branch on, the
inputs (random images, the sparse prior heat-map of production, the all-zero one of a video's first frame), the parameters
and the float64 / float32 truth of one stem, which is ``_backbone_bwd.stem`` over a ``Tape``.  No GPU, no ctypes.

The three stems of a call share nothing but the output gradient: ``y`` is a plain sum, so ``z_s``, the term ``relu(bn_s(z_s))``
and every gradient of stem s are the same whichever other stems the call holds.  A truth is therefore computed once per (shape,
statistics mode, stem) and shared by the subsets of stems that the tests call."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

import _backbone_bwd as BB
from _backbone_bwd import EPS, MOMENTUM, Tape, cast, cdiv, grads, randn  # noqa: F401
from _neck_bwd import bn_plan, ew_plan

CIN = (3, 3, 1)
PREFIX = ('base_layer.', 'pre_img_layer.', 'pre_hm_layer.')
SUBSETS = OrderedDict([('x', (0,)), ('x+pre_img', (0, 1)), ('x+pre_hm', (0, 2)), ('all', (0, 1, 2))])     # what the reference calls
K_OUT = [49 * c for c in CIN]                  # z_s and its term: the fan-in
K_IN = 49 * 16                                 # an image gradient

# (N, H, W) of the GPU op tests; tests/test_stem_backward_cpu.py holds the list against REGIMES
#   (1,8,8)       a map smaller than one tile (8 x 32 MFMA, 16 x 16 image gradient); 60 of 64 7x7 windows leave the image
#   (1,7,33)      one pixel into a second tile column; odd sizes
#   (2,20,36)     ragged tiles on both axes, two images
#   (3,5,70)      H below the halo height; three tile columns
#   (2,64,64)     aligned tiles; the size of the ``dla34`` module test
#   (2,256,260)   576 tiles: the weight gradient's grid is capped at 512 slabs and 64 workgroups run a second tile (a ragged
#                 second round); 532 480 quads of the sum kernel: its grid is capped with a ragged second round too
SHAPES = [(1, 8, 8), (1, 7, 33), (2, 20, 36), (3, 5, 70), (2, 64, 64), (2, 256, 260)]
TW, TH, GW_SLAB_CAP, GT = 32, 8, 512, 16       # stem_train.hip


def bench_shapes():
    """(batch, H, W) of tools/stem_bwd_bench.py"""
    return [(1, 512, 512), (4, 512, 512)]


def shape_id(s):
    return 'x'.join(str(v) for v in s)


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated

def stem_plan(N, H, W, gw_stems=(0, 1, 2)):
    """tile_plan / make_bwd_plan of stem_train.hip: forward and weight gradient tile the image in 8 x 32 pixels; the weight
    gradient runs min(tiles, 512) workgroups per stem, workgroup b walks the tiles b, b + slabs, ... and writes slab b:
    16 x (49 Cin padded to 16) floats; the image gradient tiles in 16 x 16; the sum kernel is element-wise over P * 4 quads."""
    tilesX, tilesY = cdiv(W, TW), cdiv(H, TH)
    tiles = N * tilesX * tilesY
    slabs = min(tiles, GW_SLAB_CAP)
    ncp = [cdiv(49 * c, 16) * 16 for c in CIN]
    return dict(tilesX=tilesX, tilesY=tilesY, tiles=tiles, slabs=slabs, capped=tiles > GW_SLAB_CAP,
                rounds=cdiv(tiles, slabs), ragged_round=tiles % slabs != 0,
                bytes=sum(slabs * 16 * ncp[s] * 4 for s in gw_stems), gin_tiles=N * cdiv(H, GT) * cdiv(W, GT),
                bn=bn_plan(N, H, W, 16), **ew_plan(N * H * W * 4))


def _regimes():
    """name -> predicate over ((N, H, W), plan): what the host plans and the kernels of stem_train.hip branch on"""
    r = OrderedDict()
    r['a map inside one MFMA tile (H <= 8, W <= 32)'] = lambda s, p: p['tiles'] == s[0] and s[1] <= TH and s[2] <= TW
    r['H, W <= 8: no pixel further than 3 from a border, all but the central 7x7 windows leave the image'] = lambda s, p: s[1] <= 8 and s[2] <= 8
    r['H below the halo height (H < 7)'] = lambda s, p: s[1] < 7
    r['ragged MFMA tiles in x only'] = lambda s, p: s[2] % TW != 0 and s[1] % TH == 0
    r['ragged MFMA tiles on both axes'] = lambda s, p: s[2] % TW != 0 and s[1] % TH != 0
    r['aligned MFMA tiles'] = lambda s, p: s[2] % TW == 0 and s[1] % TH == 0
    r['a last tile column of one pixel'] = lambda s, p: s[2] % TW == 1
    r['three or more tile columns'] = lambda s, p: p['tilesX'] >= 3
    r['two or more tile rows'] = lambda s, p: p['tilesY'] >= 2
    r['W % 4 != 0: a 4-pixel MFMA step crosses the right border'] = lambda s, p: s[2] % 4 != 0
    r['more than one image'] = lambda s, p: s[0] >= 2
    r['gw: one tile per workgroup (slabs == tiles)'] = lambda s, p: not p['capped']
    r['gw: a single slab'] = lambda s, p: p['slabs'] == 1
    r['gw: grid capped, a ragged second round'] = lambda s, p: p['capped'] and p['ragged_round']
    r['gin: a map inside one 16 x 16 tile'] = lambda s, p: p['gin_tiles'] == s[0]
    r['gin: ragged tiles on both axes'] = lambda s, p: s[1] % GT != 0 and s[2] % GT != 0 and p['gin_tiles'] > s[0]
    r['gin: aligned tiles'] = lambda s, p: s[1] % GT == 0 and s[2] % GT == 0
    r['sum: grid uncapped'] = lambda s, p: not p['ew_capped']
    r['sum: grid capped, a ragged second round'] = lambda s, p: p['ew_ragged']
    r['sum: fewer quads than one workgroup'] = lambda s, p: p['quads'] <= 256
    return r


REGIMES = _regimes()


def missing_regimes(shapes):
    """names of the regimes no (N, H, W) of the list reaches"""
    got = BB.reached(REGIMES, [(s, stem_plan(*s)) for s in shapes])
    return [name for name in REGIMES if name not in got]


# ---------------------------------------------------------------------------------------------------------------------
# inputs and parameters

def sparse_hm(seed, N, H, W, blobs=3):
    """zeros with ``blobs`` Gaussian blobs per image, values in [0, 1]: the prior heat-map of production"""
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(H, dtype=torch.float64).view(H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, W)
    hm = torch.zeros(N, 1, H, W, dtype=torch.float64)
    for n in range(N):
        for _ in range(blobs):
            cy, cx = float(torch.rand(1, generator=g)) * (H - 1), float(torch.rand(1, generator=g)) * (W - 1)
            r = 1.0 + 2.0 * float(torch.rand(1, generator=g))
            d = (ys - round(cy)) ** 2 + (xs - round(cx)) ** 2
            blob = torch.exp(-d / (2 * ((2 * r + 1) / 6) ** 2)) * (d <= 2 * r * r + 1)
            hm[n, 0] = torch.maximum(hm[n, 0], blob)
    return hm.float()


def inputs(seed, N, H, W, hm='sparse'):
    """fp32 [x, pre_img, pre_hm]: random images; ``hm``: 'sparse' | 'zero' | 'random'"""
    x, pre = randn(seed, N, 3, H, W).float(), randn(seed + 1, N, 3, H, W).float()
    if hm == 'sparse':
        h = sparse_hm(seed + 2, N, H, W)
    elif hm == 'zero':
        h = torch.zeros(N, 1, H, W)
    else:
        h = randn(seed + 2, N, 1, H, W).abs().clamp(max=1.0).float()
    return [x, pre, h]


def output_gradient(seed, N, H, W):
    """the gradient of the sum (NCHW), scaled by (pixels)^-1/2 so that sums over the map stay of order 1"""
    return (randn(seed, N, 16, H, W) / math.sqrt(N * H * W)).float()


class Stems(nn.Module):
    """the three stems as the reference's ``DLA`` holds them: the keys of ``base_layer.*``, ``pre_img_layer.*``, ``pre_hm_layer.*``"""

    def __init__(self):
        super().__init__()
        for p, c in zip(PREFIX, CIN):
            setattr(self, p[:-1], nn.Sequential(nn.Conv2d(c, 16, 7, 1, 3, bias=False), nn.BatchNorm2d(16, momentum=MOMENTUM),
                                                nn.ReLU(inplace=True)))


def params(seed):
    """``_backbone_bwd.random_params`` for the three stems: gamma of both signs, beta ~ 0.3 randn, random running statistics"""
    return BB.random_params(seed, Stems())


SEED = 4100


def case(shape, hm='sparse'):
    """(state dict, [x, pre_img, pre_hm], gy) of a shape"""
    N, H, W = shape
    return params(SEED), inputs(SEED + 11, N, H, W, hm), output_gradient(SEED + 17, N, H, W)


# ---------------------------------------------------------------------------------------------------------------------
# the truth of one stem

def stem_reference(s, sd, x, gy, training, dtype, term=None):
    """stem ``s`` in ``dtype`` -> dict(z, pre, y, mask, sd[, gin, gw, ggamma, gbeta]); ``term``: the HIP forward's
    relu(bn(z_s)) (NCHW, CPU) whose mask replaces the ReLU, or None for a free run"""
    p = PREFIX[s]
    own = OrderedDict((k, v) for k, v in sd.items() if k.startswith(p))
    sdc = cast(own, dtype, grad=gy is not None)
    xt = x.to(dtype).clone().requires_grad_(gy is not None)
    tape = Tape(None if term is None else [term])
    y = BB.stem(xt, sdc, p, training, tape)
    tape.done()
    _, pre, yd, _, mask = tape.units[0]
    res = dict(z=F.conv2d(xt.detach(), sdc[p + '0.weight'].detach(), None, 1, 3), pre=pre, y=yd, mask=mask, sd=sdc)
    if gy is not None:
        gs = grads([y], [gy], [xt, sdc[p + '0.weight'], sdc[p + '1.weight'], sdc[p + '1.bias']])
        res.update(gin=gs[0], gw=gs[1], ggamma=gs[2], gbeta=gs[3])
    return res


_truths = {}


def truth(shape, s, training, term, hm='sparse'):
    """(free64, free32, t64, t32) of stem ``s`` at ``shape``, the masked runs with the mask of ``term``; once per process.  A
    second caller's ``term`` must be the first one's bit for bit: a stem's term does not depend on the other stems."""
    key = (shape, s, training, hm)
    if key not in _truths:
        sd, xs, gy = case(shape, hm)
        free = [stem_reference(s, sd, xs[s], None, training, dt) for dt in (torch.float64, torch.float32)]
        given = [stem_reference(s, sd, xs[s], gy, training, dt, term) for dt in (torch.float64, torch.float32)]
        _truths[key] = (term.clone(), free + given)
    first, res = _truths[key]
    assert torch.equal(first, term), 'stem %d: the term differs between two calls that hold it' % s
    return res
