"""Shared pieces of the trainable-neck tests (tests/test_neck_backward_cpu.py, tests/test_hip_neck_backward.py): the
reference construction of DeformConv / IDAUp / DLAUp restated on torch functions (``oracle.dcn_v2.dcn_forward``,
``F.batch_norm``, ``F.conv_transpose2d(groups = C)``) for any dtype, the up-sampling backward as the explicit sums, the
designed offset parameters, and the slab / workspace formulas of centertrack_amd/csrc/bn_train.hip (BatchNorm) and
centertrack_amd/csrc/neck_bwd.hip (up-sampling).  No GPU, no ctypes."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from _dcn_bwd import bound, cdiv, err, randn  # noqa: F401  (the project's error measure and bound)

EPS, MOMENTUM = 1e-5, 0.1
BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked')


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated

# ``ew_grid`` of ct_train.h launches cdiv(total, 256) workgroups of 256 threads below this many channel
# quads and 2048 from there on, where the grid-stride loop of the element-wise kernels runs a second time.  The constant is
# not observable through the ABI: it is mirrored by reading.
EW_CAP = 2048 * 256


def ew_plan(quads):
    """``ew_grid(quads)`` and what follows from it inside a grid-stride kernel"""
    capped = quads >= EW_CAP
    return dict(quads=quads, ew_capped=capped, ew_grid=2048 if capped else cdiv(quads, 256),
                ew_ragged=capped and quads % EW_CAP != 0)


def bn_plan(N, H, W, C):
    """make_bn_plan of bn_train.hip (the one plan of ct_bn_* and ct_bn_act_*): slabs of pixels x chunks of up to 64 channel
    quads; workspace = (slabs + 1) * 2 * C floats.  ``wanted`` = the grid target, ``maxSlabs`` = the pixel limit;
    the element-wise kernels (apply, backward) run over P * C / 4 quads (``ew_plan``)."""
    P, C4 = N * H * W, C // 4
    cw = min(C4, 64)
    rows = 256 // cw
    chunks = cdiv(C4, cw)
    wanted, maxSlabs = cdiv(512, chunks), cdiv(P, rows * 4)
    slabs = max(1, min(wanted, maxSlabs))
    pix = cdiv(cdiv(P, slabs), rows) * rows
    slabs = cdiv(P, pix)
    return dict(cw=cw, rows=rows, chunks=chunks, slabs=slabs, pixPerSlab=pix, bytes=(slabs + 1) * 2 * C * 4,
                wanted=wanted, maxSlabs=maxSlabs, capped=wanted > maxSlabs, last_slab_pixels=P - (slabs - 1) * pix,
                dead_threads=256 - rows * cw, **ew_plan(P * C4))


def up_plan(N, H, W, C, f):
    """make_up_plan (H, W = the input grid): slabs of input pixels x chunks of 16 channel quads; workspace = slabs * 4f^2 * C;
    ``up_gx_kernel`` runs over Pin * C / 4 quads (``ew_plan``)"""
    Pin = N * H * W
    chunks = cdiv(C // 4, 16)
    wanted, maxSlabs = cdiv(512, chunks), cdiv(Pin, 8)
    slabs = max(1, min(wanted, maxSlabs))
    pix = cdiv(Pin, slabs)
    slabs = cdiv(Pin, pix)
    return dict(chunks=chunks, slabs=slabs, pixPerSlab=pix, bytes=slabs * 4 * f * f * C * 4, wanted=wanted, maxSlabs=maxSlabs,
                capped=wanted > maxSlabs, last_slab_pixels=Pin - (slabs - 1) * pix, f=f, **ew_plan(Pin * (C // 4)))


BN_SHAPES = [(2, 5, 7, 64), (3, 9, 11, 132), (1, 33, 65, 8)]
UP_SHAPES = [(2, 5, 7, 8), (2, 5, 7, 64), (1, 3, 2, 132)]                 # (N, H, W, C) of the input grid, f in {2, 4, 8}

# The shapes above keep every slab count at the pixel limit and every element-wise grid below its cap.  What production
# training reaches beyond that (tests/test_neck_backward_cpu.py holds the lists against ``missing_*_regimes``), each the
# smallest shape of its kind:
#   (3,254,258,16)   512 slabs from the grid target, the last one 372 of 384 pixels; 786 384 quads: the element-wise grid is
#                    capped and the second round of its loop is ragged
#   (1,66,70,512)    two chunks, 231 slabs from the target (256), 591 360 quads
#   (2,90,94,132)    cw 33: 25 dead threads per workgroup, 484 slabs from the target, 558 360 quads
#   (1,12,20,16)     one slab, and that one partial (240 of 256 pixels)
BN_PLAN_SHAPES = [(3, 254, 258, 16), (1, 66, 70, 512), (2, 90, 94, 132), (1, 12, 20, 16)]
#   (2,48,50,8) f 8       480 slabs from the grid target (512), one chunk
#   (1,40,44,132) f 4     three chunks (the last one a single quad), 160 slabs from the target (171)
#   (2,128,132,64) f 2    540 672 quads: the grid of up_gx_kernel is capped
UP_PLAN_SHAPES = [((2, 48, 50, 8), 8), ((1, 40, 44, 132), 4), ((2, 128, 132, 64), 2)]                # ((N, H, W, C), f)


def _bn_regimes():
    """name -> predicate over (shape, plan): what make_bn_plan, the reduce kernels and the element-wise kernels branch on"""
    r = OrderedDict()
    r['slabs cut by the pixels'] = lambda s, p: p['capped']
    r['slabs from the grid target'] = lambda s, p: not p['capped']
    r['slabs == 1'] = lambda s, p: p['slabs'] == 1
    r['slabs == 512'] = lambda s, p: p['slabs'] == 512
    r['a partial last slab'] = lambda s, p: p['last_slab_pixels'] < p['pixPerSlab']
    r['chunks == 1'] = lambda s, p: p['chunks'] == 1
    r['chunks == 2'] = lambda s, p: p['chunks'] == 2
    r['dead threads (256 % cw != 0)'] = lambda s, p: p['dead_threads'] > 0
    r['dead threads, slabs from the grid target'] = lambda s, p: p['dead_threads'] > 0 and not p['capped']
    r['element-wise grid uncapped'] = lambda s, p: not p['ew_capped']
    r['element-wise grid capped'] = lambda s, p: p['ew_capped']
    r['element-wise grid capped, total not a multiple of 2048 * 256'] = lambda s, p: p['ew_ragged']
    return r


def _up_regimes():
    """name -> predicate over ((N, H, W, C, f), plan)"""
    r = OrderedDict()
    r['slabs cut by the pixels'] = lambda s, p: p['capped']
    r['slabs from the grid target'] = lambda s, p: not p['capped']
    r['chunks == 1'] = lambda s, p: p['chunks'] == 1
    r['chunks > 1'] = lambda s, p: p['chunks'] > 1
    r['up_gx grid uncapped'] = lambda s, p: not p['ew_capped']
    r['up_gx grid capped'] = lambda s, p: p['ew_capped']
    for f in (2, 4, 8):
        r['f == %d' % f] = lambda s, p, f=f: p['f'] == f
        r['f == %d, slabs from the grid target' % f] = lambda s, p, f=f: p['f'] == f and not p['capped']   # one kernel per f
    return r


BN_REGIMES, UP_REGIMES = _bn_regimes(), _up_regimes()


def reached(regimes, plans):
    """names of the regimes some (shape, plan) of the list reaches"""
    return [name for name, pred in regimes.items() if any(pred(s, p) for s, p in plans)]


def reached_bn_regimes(shapes):
    return reached(BN_REGIMES, [(s, bn_plan(*s)) for s in shapes])


def reached_up_regimes(shapes):
    """``shapes``: (N, H, W, C, f)"""
    return reached(UP_REGIMES, [(s, up_plan(*s)) for s in shapes])


def missing_bn_regimes(shapes):
    """names of the BatchNorm regimes no (N, H, W, C) of the list reaches"""
    got = reached_bn_regimes(shapes)
    return [name for name in BN_REGIMES if name not in got]


def missing_up_regimes(shapes):
    """names of the up-sampling regimes no (N, H, W, C, f) of the list reaches"""
    got = reached_up_regimes(shapes)
    return [name for name in UP_REGIMES if name not in got]


def gpu_bn_shapes():
    """every (N, H, W, C) the BatchNorm op tests of tests/test_hip_neck_backward.py run"""
    return list(BN_SHAPES) + list(BN_PLAN_SHAPES)


def gpu_up_shapes():
    """every (N, H, W, C, f) the up-sampling op tests of tests/test_hip_neck_backward.py run"""
    return [s + (f,) for s in UP_SHAPES for f in (2, 4, 8)] + [s + (f,) for s, f in UP_PLAN_SHAPES]


DEFORM_SHAPES = [(2, 5, 7, 128, 64), (3, 5, 6, 64, 64)]                   # (N, H, W, Cin, Cout)
IDA = dict(o=64, channels=[64, 128, 256], up_f=[1, 2, 4], N=2, sizes=[(16, 24), (8, 12), (4, 6)])
DLAUP = dict(startp=2, channels=[64, 128, 256, 512], scales=[1, 2, 4, 8], N=1, sizes=[(16, 16), (8, 8), (4, 4), (2, 2)])


def bench_shapes():
    """(name, batch, o, channels, up_f, sizes) of tools/neck_bwd_bench.py"""
    out = []
    for b in (1, 4):
        out.append(('ida_up', b, 64, [64, 128, 256], [1, 2, 4], [(128, 128), (64, 64), (32, 32)]))
        out.append(('dla_up.ida_0', b, 256, [256, 512], [1, 2], [(32, 32), (16, 16)]))
    return out


def ida_nodes(o, channels, up_f, N, sizes):
    """[(kind, N, H, W, C[, f])] of every BatchNorm and up-sampling call of one IDAUp forward"""
    calls = []
    for i in range(1, len(channels)):
        (h, w), f = sizes[i], up_f[i]
        calls += [('bn', N, h, w, o), ('up', N, h, w, o, f), ('bn', N, h * f, w * f, o)]
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# the BatchNorm case of the op tests

def bn_case(shape, residual=False):
    """fp32 [z, gamma, beta, running_mean, running_var, gy(, res)] (NCHW): z with a channel of mean 100 / std 0.01 (0), a
    constant channel (1) and a channel whose pre-activations are all negative (2: beta = -30); gamma of both signs"""
    N, H, W, C = shape
    z = randn(31, N, C, H, W)
    z[:, 0] = 100 + 0.01 * z[:, 0]
    z[:, 1] = 3.0
    gamma = randn(32, C) * 0.5 + 1.0
    gamma[3::2] *= -1
    beta = randn(33, C) * 0.3
    beta[2] = -30.0
    rm, rv = randn(34, C) * 0.2, torch.rand(C, generator=torch.Generator().manual_seed(35), dtype=torch.float64) + 0.5
    rm[0] = 100.0
    t = [z, gamma, beta, rm, rv, randn(36, N, C, H, W)]
    if residual:
        t.append(randn(37, N, C, H, W))
    return [v.float() for v in t]


def bn_free_run(case, dtype, batch, residual=False):
    """(pre-activation, relu of it) of BatchNorm (+ res) in ``dtype`` with its own mask"""
    z, gamma, beta, rm, rv = (t.to(dtype) for t in case[:5])
    pre = F.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, batch, MOMENTUM, EPS)
    if residual:
        pre = pre + case[6].to(dtype)
    return pre, torch.relu(pre)


# ---------------------------------------------------------------------------------------------------------------------
# the up-sampling and its backward as the explicit sums

def upsample_add(x, w, f, skip):
    return F.conv_transpose2d(x, w, stride=f, padding=f // 2, groups=x.shape[1]) + skip


def upsample_backward_formula(x, w, f, gy):
    """gx[n,c,iy,ix] = sum_{ky,kx<2f} gy[n,c,iy*f - f/2 + ky, ix*f - f/2 + kx] * w[c,0,ky,kx] and
    gw[c,0,ky,kx] = sum_{n,iy,ix} x[n,c,iy,ix] * gy[same index] (NCHW tensors of one dtype)"""
    N, C, H, W = x.shape
    p = f // 2
    gp = F.pad(gy, (p, f, p, f))                      # index o + p: every shifted window stays inside
    gx, gw = torch.zeros_like(x), torch.zeros_like(w)
    for ky in range(2 * f):
        for kx in range(2 * f):
            win = gp[:, :, ky:ky + H * f:f, kx:kx + W * f:f]           # gy[iy*f - p + ky, ix*f - p + kx]
            gx += win * w[:, 0, ky, kx].view(1, C, 1, 1)
            gw[:, 0, ky, kx] = (x * win).sum((0, 2, 3))
    return gx, gw


# ---------------------------------------------------------------------------------------------------------------------
# parameters

def deform_keys(prefix):
    return [prefix + k for k in ('actf.0.weight', 'actf.0.bias', 'actf.0.running_mean', 'actf.0.running_var',
                                 'actf.0.num_batches_tracked', 'conv.weight', 'conv.bias', 'conv.conv_offset_mask.weight',
                                 'conv.conv_offset_mask.bias')]


def deform_params(seed, cin, cout, prefix='', offsets='designed'):
    """fp32 state dict of one DeformConv: gamma of both signs, random beta / running statistics; ``offsets`` = 'designed'
    (bias[:18] = 0.5, weight 0.05 * randn * (9 Cin)^-1/2, mask bias randn: every sample far from an integer) or 'zero'"""
    sd = OrderedDict()
    g = randn(seed, cout) * 0.5 + 1.0
    g[1::3] *= -1
    sd['actf.0.weight'] = g
    sd['actf.0.bias'] = randn(seed + 1, cout) * 0.3
    sd['actf.0.running_mean'] = randn(seed + 2, cout) * 0.2
    sd['actf.0.running_var'] = torch.rand(cout, generator=torch.Generator().manual_seed(seed + 3), dtype=torch.float64) + 0.5
    sd['actf.0.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)
    sd['conv.weight'] = randn(seed + 4, cout, cin, 3, 3) * (9 * cin) ** -0.5 * 2
    sd['conv.bias'] = randn(seed + 5, cout) * 0.1
    wo, bo = torch.zeros(27, cin, 3, 3, dtype=torch.float64), torch.zeros(27, dtype=torch.float64)
    if offsets == 'designed':
        wo = 0.05 * randn(seed + 6, 27, cin, 3, 3) * (9 * cin) ** -0.5
        bo[:18] = 0.5
        bo[18:] = randn(seed + 7, 9)
    sd['conv.conv_offset_mask.weight'], sd['conv.conv_offset_mask.bias'] = wo, bo
    return OrderedDict((prefix + k, v if v.dtype == torch.long else v.float()) for k, v in sd.items())


def ida_params(seed, o, channels, up_f, prefix='', offsets='designed'):
    """fp32 state dict of one IDAUp with random (not bilinear) up-sampling weights"""
    sd = OrderedDict()
    for i in range(1, len(channels)):
        f = int(up_f[i])
        sd.update(deform_params(seed + 100 * i, channels[i], o, '%sproj_%d.' % (prefix, i), offsets))
        sd['%sup_%d.weight' % (prefix, i)] = (randn(seed + 100 * i + 50, o, 1, 2 * f, 2 * f) * 0.5 / f).float()
        sd.update(deform_params(seed + 100 * i + 60, o, o, '%snode_%d.' % (prefix, i), offsets))
    return sd


def dlaup_structure(channels, scales):
    """[(i, o, in_channels, up_f)] of the ``ida_i`` of DLAUp(startp, channels, scales)"""
    channels, inc, scales = list(channels), list(channels), list(scales)
    out = []
    for i in range(len(channels) - 1):
        j = -i - 2
        out.append((i, channels[j], list(inc[j:]), [s // scales[j] for s in scales[j:]]))
        scales[j + 1:] = [scales[j]] * len(scales[j + 1:])
        inc[j + 1:] = [channels[j]] * len(inc[j + 1:])
    return out


def dlaup_params(seed, channels, scales, prefix='', offsets='designed'):
    sd = OrderedDict()
    for i, o, inc, up_f in dlaup_structure(channels, scales):
        sd.update(ida_params(seed + 1000 * i, o, inc, up_f, '%sida_%d.' % (prefix, i), offsets))
    return sd


def is_buffer(key):
    return key.rsplit('.', 1)[1] in BUFFERS


def cast(sd, dtype, grad=False):
    """a copy of the state dict in ``dtype``; with ``grad`` the parameters are leaves that require a gradient"""
    out = OrderedDict()
    for k, v in sd.items():
        if v.dtype == torch.long:
            out[k] = v.clone()
        else:
            out[k] = v.detach().cpu().to(dtype).clone()
            if grad and not is_buffer(k):
                out[k].requires_grad_()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference construction

class Trace(object):
    """what a run leaves behind per DeformConv prefix: the pre-activation ``pre``, the output ``y``, the raw offsets ``coords``
    and, after a backward, the gradient ``gz`` of the DCN output; ``masks`` = {prefix:
    ReLU mask (NCHW, 0 / 1)} replaces the ReLU by a multiplication with the given mask"""

    def __init__(self, masks=None):
        self.masks, self.pre, self.y, self.coords, self.gz = masks, OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()


def deform(x, sd, prefix, training, trace):
    """DeformConv.forward (dla.py:515-518) on NCHW ``x``; running statistics of ``sd`` are updated in place when training"""
    from oracle import dcn_v2 as odcn
    wo, bo = sd[prefix + 'conv.conv_offset_mask.weight'], sd[prefix + 'conv.conv_offset_mask.bias']
    z = odcn.dcn_forward(x, sd[prefix + 'conv.weight'], sd[prefix + 'conv.bias'], wo, bo)
    if z.requires_grad:
        z.register_hook(lambda g: trace.gz.__setitem__(prefix, g.detach()))
    pre = F.batch_norm(z, sd[prefix + 'actf.0.running_mean'], sd[prefix + 'actf.0.running_var'], sd[prefix + 'actf.0.weight'],
                       sd[prefix + 'actf.0.bias'], training, MOMENTUM, EPS)
    if training:
        sd[prefix + 'actf.0.num_batches_tracked'] += 1
    y = torch.relu(pre) if trace.masks is None else pre * trace.masks[prefix].to(pre.dtype)
    trace.pre[prefix], trace.y[prefix] = pre.detach(), y.detach()
    trace.coords[prefix] = F.conv2d(x.detach(), wo.detach(), bo.detach(), padding=1)[:, :18]
    return y


def ida(layers, sd, prefix, startp, endp, training, trace):
    """IDAUp.forward (dla.py:539-545) on a list of NCHW tensors, rewritten in place"""
    for i in range(startp + 1, endp):
        k = i - startp
        w = sd['%sup_%d.weight' % (prefix, k)]
        x = deform(layers[i], sd, '%sproj_%d.' % (prefix, k), training, trace)
        x = upsample_add(x, w, w.shape[2] // 2, layers[i - 1])
        layers[i] = deform(x, sd, '%snode_%d.' % (prefix, k), training, trace)


def dlaup(layers, sd, prefix, startp, training, trace):
    """DLAUp.forward (dla.py:568-574)"""
    layers = list(layers)
    out = [layers[-1]]
    for i in range(len(layers) - startp - 1):
        ida(layers, sd, '%sida_%d.' % (prefix, i), len(layers) - i - 2, len(layers), training, trace)
        out.insert(0, layers[-1])
    return out


def min_integer_distance(trace):
    """the smallest distance of a sample coordinate (integer tap base + offset) from an integer over all nodes of a run"""
    d = 1.0
    for off in trace.coords.values():
        fr = off.double() - off.double().floor()
        d = min(d, float(torch.minimum(fr, 1 - fr).min()))
    return d


def grads(outs, gys, leaves):
    """d(sum_i <outs[i], gys[i]>) / d(leaves) -> list (zeros where a leaf is unused)"""
    total = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, gys))
    gs = torch.autograd.grad(total, leaves, allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, gs)]


def check_mask(mask_hip, pre64, e32_y, what=''):
    """the HIP forward's ReLU mask may differ from the float64 one only where |pre64| <= 64 * e32(y) * max|y64|, at no more
    than 0.1 % of the map -> (flipped units, units that close to 0)"""
    m64 = pre64 > 0
    thr = 64.0 * e32_y * float(torch.relu(pre64).max())
    near = pre64.abs() <= thr
    flipped = mask_hip.bool() != m64
    assert not bool((flipped & ~near).any()), '%s: a ReLU unit flipped away from 0 (threshold %.3g)' % (what, thr)
    assert int(flipped.sum()) <= 1e-3 * pre64.numel(), '%s: %d of %d units flipped' % (what, int(flipped.sum()), pre64.numel())
    return int(flipped.sum()), int(near.sum())


def bias_norm(trace, key):
    """The yardstick of a ``conv.bias`` gradient under batch statistics.  BatchNorm subtracts the batch mean, so this gradient
    -- the sum of ``gz`` over the P pixels -- is 0 in exact arithmetic and what float64 leaves of it (1e-16) is no scale to
    measure against.  What fp32 leaves: every ``gz`` carries a few roundings of terms no larger than max|gz|, and the error of
    the fp32 batch mean of the gradient is the same in all P of them, so the errors add linearly: P * 2^-24 * max|gz| times
    a small factor.  With the norm sqrt(P) * max|gz| the project's bound at K = P is 4 * 2^-23 * sqrt(P) * norm
    = 8 * P * 2^-24 * max|gz|.  An implementation that returns 0 passes this by construction; the eval-mode cases, where the
    gradient is not 0, hold ``conv.bias`` to the tensor's maximum like every other gradient."""
    gz = trace.gz[key[:-len('conv.bias')]]
    P = gz.shape[0] * gz.shape[2] * gz.shape[3]
    return float(gz.abs().max()) * math.sqrt(P)
