"""Shared pieces of the heads-backward tests (tests/test_heads_backward_cpu.py, tests/test_hip_heads_backward.py): the
fixture whose hidden pre-activation is exact in fp32, the float64 / float32 truth (torch autograd on the CPU of the
reference's construction, conv3x3 -> ReLU -> conv1x1 per head), a pure-Python restatement of the two host plans of
centertrack_amd/csrc/heads_bwd.hip and the list of shapes.  No GPU, no ctypes.  Error measure and bound: tests/_dcn_bwd.py.

The ReLU mask.  A float64 truth and an fp32 kernel can disagree about the sign of a hidden value next to 0, and one flipped
unit changes a weight gradient by a whole term.  So ``x``, ``w0`` and ``b0`` are dyadic -- integers in [-8, 8] over 8, 64 and
8: every product and every partial sum in any order (and every Winograd-domain intermediate) is a small multiple of 2^-11,
far below 2^24 units, and fp32 equals float64 bit for bit, exact zeros included.  ``w2`` and the incoming logit gradients
are ordinary Gaussians, so every gradient is a genuine fp32 sum."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from _dcn_bwd import bound, cdiv, err  # noqa: F401  (re-exported)

HC = 256
CIN = 64
MOT = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('ltrb_amodal', 4)])
POSE = OrderedDict([('hm', 80), ('hps', 34), ('hm_hp', 17)])
NUSC = OrderedDict([('hm', 10), ('reg', 2), ('wh', 2), ('tracking', 2), ('dep', 1), ('rot', 8), ('dim', 3),
                    ('amodel_offset', 2), ('nuscenes_att', 8), ('velocity', 3)])

# ((N, H, W), heads) and, per shape, the branches of the two host plans it reaches (``cw_plan`` of the first layer's weight
# gradient, Cin 64 -> Cout 256 * nheads, ks 3; ``tail_plan``), asserted by tests/test_heads_backward_cpu.py:
#   (2,11,13) MOT        ragged pixel tile, N*H*W % 4 == 2 (the last 4-pixel step is half empty); cw: 288 units, slab count cut
#                        by maxSlabs (4 -> 3), stepsPerWave 6; tail: 5 slabs of 64 pixels, the last one 30 pixels
#   (3,8,8) one head c=1 cw: 72 units, slabs cut 15 -> 2, stepsPerWave 6; tail: one head, 3 slabs of 64
#   (1,9,10) POSE        c > 16: 5 / 3 / 2 passes of 16 logit channels per head, a grid sized for the widest head whose other
#                        workgroups leave at once, c % 16 != 0; cw: 216 units, slabs cut 5 -> 1 (the reduce adds one slab)
#   (1,32,40) NUSC       ten heads (more than the 8 of the fused inference launch); cw: 720 units, 2 uncapped slabs,
#                        stepsPerWave 40, every wave full; tail: 20 slabs of 64 pixels (capped by the pixels)
#   (1,31,40) NUSC       cw: 2 uncapped slabs with a ragged last slab: stepsPerWave 39, the last wave runs 37 steps
#   (4,16,16) two heads  cw: 144 units, the slab count 8 lands exactly on maxSlabs, stepsPerWave 8 = two full rounds of four
#                        steps, no ragged wave; tail: 16 slabs of 64
SHAPES = [((2, 11, 13), MOT), ((3, 8, 8), OrderedDict([('hm', 1)])), ((1, 9, 10), POSE), ((1, 32, 40), NUSC),
          ((1, 31, 40), NUSC), ((4, 16, 16), OrderedDict([('hm', 2), ('wh', 2)]))]


def case_id(case):
    (N, H, W), heads = case
    return '%dx%dx%d-%s' % (N, H, W, '+'.join('%s%d' % (h, c) for h, c in heads.items()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic(seed, shape, den):
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float() / den


def fixture(case, seed=0):
    """fp32 CPU tensors: x [N,64,H,W], per head w0 [hc,64,3,3], b0 [hc], w2 [c,hc,1,1], b2 [c], gout [N,c,H,W]"""
    (N, H, W), heads = case
    fx = {'x': dyadic(seed + 1, (N, CIN, H, W), 8.0), 'heads': heads, 'w0': OrderedDict(), 'b0': OrderedDict(),
          'w2': OrderedDict(), 'b2': OrderedDict(), 'gout': OrderedDict()}
    for j, (h, c) in enumerate(heads.items()):
        s = seed + 100 * (j + 1)
        fx['w0'][h] = dyadic(s + 1, (HC, CIN, 3, 3), 64.0)
        fx['b0'][h] = dyadic(s + 2, (HC,), 8.0)
        fx['w2'][h] = torch.randn((c, HC, 1, 1), generator=_gen(s + 3)) * HC ** -0.5
        fx['b2'][h] = torch.randn((c,), generator=_gen(s + 4))
        fx['gout'][h] = torch.randn((N, c, H, W), generator=_gen(s + 5))
    return fx


def autograd(fx, dtype):
    """torch autograd of the heads in ``dtype`` -> {'pre' (hidden pre-activation), 'mid', 'out': {h}, 'x', 'gmid', 'w0',
    'b0' (concatenated over the heads), 'w2': {h}, 'b2': {h}}"""
    # (copies: ``.to`` of an fp32 tensor to fp32 is the tensor itself, and the fixture is shared and stays without a grad flag)
    x = fx['x'].detach().clone().to(dtype).requires_grad_()
    leaves, pres, mids, outs = [], [], [], OrderedDict()
    tot = 0
    for h in fx['heads']:
        p = [fx[k][h].detach().clone().to(dtype).requires_grad_() for k in ('w0', 'b0', 'w2', 'b2')]
        pre = F.conv2d(x, p[0], p[1], padding=1)
        mid = F.relu(pre)
        outs[h] = F.conv2d(mid, p[2], p[3])
        tot = tot + (outs[h] * fx['gout'][h].to(dtype)).sum()
        leaves += p
        pres.append(pre)
        mids.append(mid)
    g = torch.autograd.grad(tot, [x] + leaves + pres)
    nh = len(fx['heads'])
    gl = g[1:1 + 4 * nh]
    return {'pre': torch.cat([p.detach() for p in pres], 1), 'mid': torch.cat([m.detach() for m in mids], 1),
            'out': OrderedDict((h, o.detach()) for h, o in outs.items()), 'x': g[0], 'gmid': torch.cat(g[1 + 4 * nh:], 1),
            'w0': torch.cat(gl[0::4], 0), 'b0': torch.cat(gl[1::4], 0),
            'w2': OrderedDict(zip(fx['heads'], gl[2::4])), 'b2': OrderedDict(zip(fx['heads'], gl[3::4]))}


_cache = {}


def truth(case):
    """(fixture, float64 autograd, float32 autograd), once per process"""
    key = case_id(case)
    if key not in _cache:
        fx = fixture(case)
        _cache[key] = (fx, autograd(fx, torch.float64), autograd(fx, torch.float32))
    return _cache[key]


def terms(case):
    """K, the number of terms behind one element of each gradient"""
    (N, H, W), heads = case
    return {'w0': N * H * W, 'b0': N * H * W, 'w2': N * H * W, 'b2': N * H * W, 'x': 9 * HC * len(heads), 'gmid': None}


# ---------------------------------------------------------------------------------------------------------------------
# the host plans, restated

def cw_plan(N, H, W, Cin, Cout, ks):
    """make_cw_plan / ct_conv_weight_plan of heads_bwd.hip (with the bias tail); ``slabs`` is observable through ct_conv2d_backward_weight_workspace_bytes"""
    taps = ks * ks
    NT = cdiv(Cout, 16)
    units = taps * cdiv(Cin, 32) * cdiv(NT, 4)
    nsteps = cdiv(N * H * W, 4)
    wanted, maxSlabs = cdiv(1024, units), cdiv(nsteps, 32)
    slabs = max(1, min(wanted, maxSlabs))
    spw = cdiv(nsteps, slabs * 4)
    stride = Cout * Cin * taps + Cout
    return dict(units=units, nsteps=nsteps, slabs=slabs, capped=wanted > maxSlabs, stepsPerWave=spw,
                last_wave_steps=nsteps - (slabs * 4 - 1) * spw, slabStride=stride, bytes=slabs * stride * 4)


def tail_plan(N, H, W, hc, cs):
    """make_tail_plan of heads_bwd.hip for heads of widths ``cs``"""
    total = N * H * W
    kblocks = cdiv(hc, 256)
    wgs = sum(cdiv(c, 16) * kblocks for c in cs)
    slabs = max(1, min(cdiv(2048, wgs), cdiv(total, 64)))
    pps = cdiv(cdiv(total, slabs), 64) * 64
    slabs = cdiv(total, pps)
    stride = sum(c * (hc + 1) for c in cs)
    return dict(kblocks=kblocks, passes=[cdiv(c, 16) for c in cs], slabs=slabs, pixPerSlab=pps,
                last_slab_pixels=total - (slabs - 1) * pps, slabStride=stride, bytes=slabs * stride * 4,
                wanted=cdiv(2048, wgs), maxSlabs=cdiv(total, 64), capped=cdiv(2048, wgs) > cdiv(total, 64))


# The tail at two tiles per slab.  In ``SHAPES`` the pixel limit always wins and ``pixPerSlab`` is 64, one tile: the tile loop
# of heads_tail_weight_kernel runs once.  Sixteen heads of width 20 on (2, 41, 51): 32 workgroups per slab, 64 slabs wanted
# of 66 possible, ``pixPerSlab`` 128 -- two tiles, ``g`` re-staged between them and ``bsum`` carried across -- 33 slabs, the
# last one 86 pixels = a full tile and a ragged one of 22; images of 2091 pixels, so tile 32 of the 66 crosses the image
# border.  (Training at batch 4 on 512 x 512 runs ``pixPerSlab`` 128 as well.)  The hidden map is built directly, see
# ``tail_fixture``.
TAIL_CASE = ((2, 41, 51), OrderedDict(('h%02d' % i, 20) for i in range(16)))


def tail_cases():
    """every ((N, H, W), heads) the GPU tests run through ct_heads_tail_backward"""
    return list(SHAPES) + [TAIL_CASE]


def _tail_regimes():
    """name -> predicate over (((N, H, W), heads), tail plan): what make_tail_plan and the two tail kernels branch on"""
    r = OrderedDict()
    r['slabs cut by the pixels'] = lambda s, p: p['capped']
    r['slabs from the grid target'] = lambda s, p: not p['capped']
    r['pixPerSlab == 64'] = lambda s, p: p['pixPerSlab'] == 64
    r['pixPerSlab >= 128'] = lambda s, p: p['pixPerSlab'] >= 128
    r['a last slab of more than one tile whose last tile is ragged'] = \
        lambda s, p: p['last_slab_pixels'] > 64 and p['last_slab_pixels'] % 64 != 0
    r['a last slab of one ragged tile'] = lambda s, p: p['last_slab_pixels'] < 64
    r['a tile that crosses an image border'] = lambda s, p: s[0][0] >= 2 and (s[0][1] * s[0][2]) % 64 != 0
    r['a head wider than 16 next to a narrower one'] = lambda s, p: max(p['passes']) > 1 and min(p['passes']) < max(p['passes'])
    r['every head wider than 16'] = lambda s, p: min(p['passes']) > 1
    r['kblocks == 1'] = lambda s, p: p['kblocks'] == 1
    return r


TAIL_REGIMES = _tail_regimes()


def reached_tail_regimes(cases, hc=HC):
    plans = [(c, tail_plan(*c[0], hc, tuple(c[1].values()))) for c in cases]
    return [name for name, pred in TAIL_REGIMES.items() if any(pred(c, p) for c, p in plans)]


def missing_tail_regimes(cases, hc=HC):
    """names of the tail regimes no case of the list reaches"""
    got = reached_tail_regimes(cases, hc)
    return [name for name in TAIL_REGIMES if name not in got]


def tail_fixture(case, seed=0):
    """fp32 CPU tensors for the tail alone: the hidden map ``mid`` [N, nheads*hc, H, W] = relu of a Gaussian, built directly
    (half of it exact zeros: the ReLU mask is taken from ``mid`` itself, as by the kernel), per head w2 [c,hc,1,1] and gout
    [N,c,H,W], and the first layers' weight w0 [nheads*hc, 64, 3, 3] for the input gradient"""
    (N, H, W), heads = case
    nh = len(heads)
    fx = {'heads': heads, 'mid': torch.relu(torch.randn((N, nh * HC, H, W), generator=_gen(seed + 1))), 'w2': OrderedDict(),
          'gout': OrderedDict(), 'w0': torch.randn((nh * HC, CIN, 3, 3), generator=_gen(seed + 2)) * (9 * CIN) ** -0.5}
    for j, (h, c) in enumerate(heads.items()):
        s = seed + 100 * (j + 1)
        fx['w2'][h] = torch.randn((c, HC, 1, 1), generator=_gen(s + 3)) * HC ** -0.5
        fx['gout'][h] = torch.randn((N, c, H, W), generator=_gen(s + 5))
    return fx


def tail_truth(fx, dtype):
    """the tail's gradients in ``dtype`` as explicit sums: gw2[h] = sum_{n,p} gout[h] x mid[h], gb2[h] = sum gout[h],
    gmid[h] = (w2[h]^T gout[h]) where mid > 0, and gx = conv3x3 of gmid with w0 transposed -> dict"""
    mid = fx['mid'].to(dtype)
    res = {'w2': OrderedDict(), 'b2': OrderedDict()}
    gm = []
    for j, h in enumerate(fx['heads']):
        m = mid[:, HC * j:HC * (j + 1)]
        g, w2 = fx['gout'][h].to(dtype), fx['w2'][h].to(dtype)
        res['w2'][h] = torch.einsum('nchw,nkhw->ck', g, m).view(w2.shape)
        res['b2'][h] = g.sum((0, 2, 3))
        gm.append(torch.einsum('nchw,ck->nkhw', g, w2[:, :, 0, 0]) * (m > 0).to(dtype))
    res['gmid'] = torch.cat(gm, 1)
    res['x'] = F.conv_transpose2d(res['gmid'], fx['w0'].to(dtype), padding=1)
    return res
