"""Shared pieces of the trainable-backbone tests (tests/test_backbone_backward_cpu.py, tests/test_hip_backbone_backward.py):
the reference construction of BasicBlock / Root / Tree / DLA (dla.py:38-66,154-316) restated on torch functions (``F.conv2d``,
``F.batch_norm``, ``F.max_pool2d``) for any dtype over a state dict, the stride-2 input gradient and the pool's tie rule as
explicit sums, and the slab / workspace formulas of centertrack_amd/csrc/backbone_bwd.hip (the BatchNorm plan, bn_train.hip's,
comes from tests/_neck_bwd.py).  No GPU, no ctypes.

A construction run takes a ``Tape``.  Empty, the run is free: every ReLU and every pool decides by its own values.  Filled
with the maps ``centertrack_amd.dla_base.trace`` received from a HIP forward (moved to the CPU, NCHW), every ReLU becomes a
multiplication with the mask of the HIP output and every pool a gather at the indices torch's max_pool2d picks on the HIP
input map, so that the float64 truth differentiates the function the HIP forward computed.  The construction therefore calls
its units in the order dla_base emits them: in a one-level ``Tree`` the first block's first unit, then the pool, then
``project`` (the reference computes pool and project first; the values do not depend on the order)."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

import _neck_bwd
from _dcn_bwd import bound, cdiv, err, randn  # noqa: F401  (the project's error measure and bound)
from _neck_bwd import (BN_PLAN_SHAPES, BN_REGIMES, BN_SHAPES, EPS, EW_CAP, MOMENTUM, bn_plan, cast, ew_plan, grads,  # noqa: F401
                       is_buffer, missing_bn_regimes, reached, reached_bn_regimes)

S2_SHAPES = [(2, 6, 10, 16, 32), (1, 4, 4, 64, 128), (3, 2, 2, 256, 512), (1, 34, 66, 32, 64)]     # (N, H, W, Cin, Cout)
POOL_SHAPES = [(2, 6, 10, 16), (1, 2, 2, 132), (1, 34, 66, 8)]                                  # (N, H, W, C)
DLA34 = dict(levels=[1, 1, 1, 2, 2, 1], channels=[16, 32, 64, 128, 256, 512])

# The shapes above keep the slab count of the weight gradient at ``maxSlabs`` and every element-wise grid below its cap.
# What production training and the API reach beyond that (tests/test_backbone_backward_cpu.py holds the lists against
# ``missing_*_regimes``), each the smallest shape of its kind:
#   (2,96,100,64,128)   29 slabs from cdiv(1024, 36 units); stepsPerWave 11 (% 4 == 3); 1200 steps over 116 waves: six waves
#                       and one whole slab idle (the slab must still write zeros); two images of 2400 output pixels: no
#                       4-pixel step crosses the image border; Wo 50, Ho 48: ragged in x only
#   (1,64,72,256,512)   2 slabs from the target (576 units), stepsPerWave 36; eight cout groups, eight LDS chunks in gx
#   (1,6,10,48,80)      Cin % 32 == 16 with two channel groups (``has1`` false with cig > 0); Cout 80: a partial second LDS
#                       chunk of 16 couts in gx, a second cout group of ONE tile in gw (nco 1 with cog > 0)
#   (1,8,32,16,16)      Wo 16, Ho 4: one tile whose halo row and column lie wholly outside the map
S2_PLAN_SHAPES = [(2, 96, 100, 64, 128), (1, 64, 72, 256, 512), (1, 6, 10, 48, 80), (1, 8, 32, 16, 16)]
#   (3,256,260,44)      3 * 128 * 130 windows * 11 quads = 549 120 >= 2048 * 256 and no multiple of it: the grid is capped;
#                       11 quads per pixel: the split of the index is a real division
POOL_PLAN_SHAPES = [(3, 256, 260, 44)]


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated

def s2_plan(N, H, W, Cin, Cout):
    """make_s2_plan (its weight half is ct_conv_weight_plan of heads_bwd.hip): the input gradient runs one workgroup per (image, 4 x 16 cells, 32 input channels); the weight gradient
    one per (tap, 32 input channels, 64 couts) and K slab of output pixels; workspace = slabs * Cout * Cin * 9 floats.
    ``wanted`` = the grid target, ``maxSlabs`` = the pixel limit; then what follows inside conv_bwd_weight_kernel<2> (wave j of the
    slabs * 4 runs steps j * stepsPerWave .. of ``nsteps``: the waves and slabs past the end are idle) and conv_s2_gx_kernel."""
    Ho, Wo = H // 2, W // 2
    cgroups = cdiv(Cin, 32)
    gx_units = N * cdiv(Wo, 16) * cdiv(Ho, 4) * cgroups
    NT = Cout // 16
    cogroups = cdiv(NT, 4)
    gw_units = 9 * cgroups * cogroups
    nsteps = cdiv(N * Ho * Wo, 4)
    wanted, maxSlabs = cdiv(1024, gw_units), cdiv(nsteps, 32)
    slabs = max(1, min(wanted, maxSlabs))
    spw = cdiv(nsteps, slabs * 4)
    return dict(gx_units=gx_units, gw_units=gw_units, slabs=slabs, stepsPerWave=spw, bytes=slabs * Cout * Cin * 9 * 4,
                Ho=Ho, Wo=Wo, cgroups=cgroups, cogroups=cogroups, nco_last=NT - (cogroups - 1) * 4, nsteps=nsteps,
                wanted=wanted, maxSlabs=maxSlabs, capped=wanted > maxSlabs, idle_waves=slabs * 4 - cdiv(nsteps, spw),
                idle_slabs=slabs - cdiv(nsteps, spw * 4))


def pool_plan(N, H, W, C):
    """the grid of maxpool_bwd_kernel: one thread per 2x2 window and channel quad"""
    return ew_plan(N * (H // 2) * (W // 2) * (C // 4))


def _s2_regimes():
    """name -> predicate over ((N, H, W, Cin, Cout), plan): what make_s2_plan and the two kernels branch on"""
    r = OrderedDict()
    r['slabs cut by maxSlabs'] = lambda s, p: p['capped']
    r['slabs from cdiv(1024, units)'] = lambda s, p: not p['capped']
    r['slabs == 1'] = lambda s, p: p['slabs'] == 1
    for m in (0, 1, 2, 3):
        r['stepsPerWave %% 4 == %d' % m] = lambda s, p, m=m: p['stepsPerWave'] % 4 == m
    r['a whole idle wave'] = lambda s, p: p['idle_waves'] >= 1
    r['a whole idle slab'] = lambda s, p: p['idle_slabs'] >= 1
    r['stepsPerWave >= 32 with slabs from the target'] = lambda s, p: not p['capped'] and p['stepsPerWave'] >= 32
    r['nco < 4 in a cout group other than the first'] = lambda s, p: p['cogroups'] > 1 and p['nco_last'] < 4
    r['Cin % 32 == 16 with more than one channel group'] = lambda s, p: s[3] % 32 == 16 and p['cgroups'] > 1
    r['Cout % 64 != 0 with Cout > 64'] = lambda s, p: s[4] > 64 and s[4] % 64 != 0
    r['Wo % 16 == 0 and Ho % 4 == 0'] = lambda s, p: p['Wo'] % 16 == 0 and p['Ho'] % 4 == 0
    r['Wo == 16 and Ho == 4: the halo lies wholly outside the map'] = lambda s, p: p['Wo'] == 16 and p['Ho'] == 4
    r['ragged tiles on both axes'] = lambda s, p: p['Wo'] % 16 != 0 and p['Ho'] % 4 != 0
    r['N >= 2, a 4-pixel step crosses an image border'] = lambda s, p: s[0] >= 2 and (p['Ho'] * p['Wo']) % 4 != 0
    r['N >= 2, no 4-pixel step crosses an image border'] = lambda s, p: s[0] >= 2 and (p['Ho'] * p['Wo']) % 4 == 0
    return r


def _pool_regimes():
    r = OrderedDict()
    r['grid uncapped'] = lambda s, p: not p['ew_capped']
    r['grid capped'] = lambda s, p: p['ew_capped']
    r['grid capped, total not a multiple of 2048 * 256'] = lambda s, p: p['ew_ragged']
    return r


S2_REGIMES, POOL_REGIMES = _s2_regimes(), _pool_regimes()


def reached_s2_regimes(shapes):
    return reached(S2_REGIMES, [(s, s2_plan(*s)) for s in shapes])


def reached_pool_regimes(shapes):
    return reached(POOL_REGIMES, [(s, pool_plan(*s)) for s in shapes])


def missing_s2_regimes(shapes):
    """names of the stride-2 regimes no (N, H, W, Cin, Cout) of the list reaches"""
    got = reached_s2_regimes(shapes)
    return [name for name in S2_REGIMES if name not in got]


def missing_pool_regimes(shapes):
    """names of the max-pool regimes no (N, H, W, C) of the list reaches"""
    got = reached_pool_regimes(shapes)
    return [name for name in POOL_REGIMES if name not in got]


def gpu_bn_shapes():
    """every (N, H, W, C) the BatchNorm-act op tests of tests/test_hip_backbone_backward.py run"""
    return list(BN_SHAPES) + list(BN_PLAN_SHAPES)


def dla_units(N, H, W, levels=None, channels=None):
    """[('s2', N, H, W, Cin, Cout) | ('bn', N, H, W, C)] of every stride-2 conv backward and every BatchNorm of one DLA-34
    training step on an N x H x W input (H, W = the input grid of the call)"""
    levels, channels = levels or DLA34['levels'], channels or DLA34['channels']
    calls = [('bn', N, H, W, channels[0]), ('s2', N, H, W, channels[0], channels[1]), ('bn', N, H // 2, W // 2, channels[1])]
    h, w = H // 2, W // 2
    for lv in range(2, 6):
        cin, cout = channels[lv - 1], channels[lv]
        calls.append(('s2', N, h, w, cin, cout))
        h, w = h // 2, w // 2
        calls.append(('bn', N, h, w, cout))
    return calls


def bench_shapes():
    """(batch, H, W) of tools/backbone_bwd_bench.py"""
    return [(1, 512, 512), (4, 512, 512)]


# ---------------------------------------------------------------------------------------------------------------------
# explicit sums

def conv_s2_gx_formula(gy, w, H, W):
    """The parity decomposition of the stride-2 input gradient (NCHW, one dtype): cell (cy, cx) of the output grid owns the
    input pixels (2cy + a, 2cx + b); along one axis a = 0 meets tap 1 at cy, a = 1 meets tap 2 at cy and tap 0 at cy + 1; gy
    outside the map counts as zero.  Nine products in all, each tap once."""
    N, Cout, Ho, Wo = gy.shape
    Cin = w.shape[1]
    gp = F.pad(gy, (0, 1, 0, 1))                                     # the halo row and column
    gx = torch.zeros(N, Cin, H, W, dtype=gy.dtype)
    axis = {0: [(1, 0)], 1: [(2, 0), (0, 1)]}                         # parity -> [(tap, cell shift)]
    for a in (0, 1):
        for b in (0, 1):
            acc = torch.zeros(N, Cin, Ho, Wo, dtype=gy.dtype)
            for ky, dy in axis[a]:
                for kx, dx in axis[b]:
                    acc += torch.einsum('nohw,oi->nihw', gp[:, :, dy:dy + Ho, dx:dx + Wo], w[:, :, ky, kx])
            gx[:, :, a::2, b::2] = acc
    return gx


def conv_s2_gw_formula(x, gy):
    """gw[co,ci,ky,kx] = sum_{n,oy,ox} gy[n,co,oy,ox] * x[n,ci,2oy-1+ky,2ox-1+kx], zero outside the image"""
    N, Cout, Ho, Wo = gy.shape
    xp = F.pad(x, (1, 1, 1, 1))
    gw = torch.zeros(Cout, x.shape[1], 3, 3, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            gw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', gy, xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    return gw


def pool_selection(x):
    """[N,C,H/2,W/2] position 0..3 (row-major in the window) of the FIRST maximum: a later value wins only if it is greater"""
    v = [x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]]
    best, sel = v[0].clone(), torch.zeros_like(v[0], dtype=torch.long)
    for j in (1, 2, 3):
        win = v[j] > best
        best = torch.where(win, v[j], best)
        sel = torch.where(win, torch.full_like(sel, j), sel)
    return sel


def pool_backward_formula(x, gy, add=None):
    """each window's gradient to its first maximum, 0 to the other three, plus ``add``"""
    sel = pool_selection(x)
    gx = torch.zeros_like(x) if add is None else add.clone()
    for j in range(4):
        gx[:, :, j // 2::2, j % 2::2] += torch.where(sel == j, gy, torch.zeros_like(gy))
    return gx


def tie_fraction(x):
    """share of the 2x2 windows whose maximum is reached more than once"""
    v = torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]])
    return float(((v == v.max(0).values).sum(0) > 1).double().mean())


def tie_input(seed, N, C, H, W):
    """a post-ReLU map (fp32): most windows all zero, one of equal positive values, -0.0 in front of and behind a 0"""
    x = torch.relu(randn(seed, N, C, H, W) - 1.0)
    x[:, :, 0:2, 0:2] = 0.75
    x[:, 0::2, -2, -2] = -0.0
    x[:, 1::2, -1, -1] = -0.0
    return x.float()


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the op tests

def bn_case(shape):
    """``_neck_bwd.bn_case`` plus a residual"""
    return _neck_bwd.bn_case(shape, residual=True)


_s2_cache = {}


def s2_case(shape):
    """fp32 (x, w, gy) of a (N, H, W, Cin, Cout) and {dtype: (gx, gw)} of torch autograd on the CPU, once per process"""
    if shape not in _s2_cache:
        N, H, W, Cin, Cout = shape
        x, w = randn(11, N, Cin, H, W).float(), (randn(12, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5).float()
        gy = randn(13, N, Cout, H // 2, W // 2).float()
        ref = {}
        for dt in (torch.float64, torch.float32):
            xt, wt = x.to(dt).clone().requires_grad_(), w.to(dt).clone().requires_grad_()     # (the fp32 ``.to`` is x itself)
            ref[dt] = torch.autograd.grad(F.conv2d(xt, wt, None, 2, 1), (xt, wt), gy.to(dt))
        _s2_cache[shape] = (x, w, gy, ref)
    return _s2_cache[shape]


# ---------------------------------------------------------------------------------------------------------------------
# parameters

def random_params(seed, module):
    """fp32 state dict for ``module`` (keys and shapes from its own state dict): conv weights randn * fan_in^-1/2, gamma of
    both signs, random beta and running statistics"""
    sd = OrderedDict()
    for i, (k, v) in enumerate(module.state_dict().items()):
        s, leaf = seed + 7 * i, k.rsplit('.', 1)[1]
        if leaf == 'num_batches_tracked':
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif leaf == 'running_var':
            sd[k] = (torch.rand(v.shape, generator=torch.Generator().manual_seed(s), dtype=torch.float64) + 0.5).float()
        elif leaf == 'running_mean':
            sd[k] = (randn(s, *v.shape) * 0.2).float()
        elif v.dim() == 4:
            sd[k] = (randn(s, *v.shape) * (v.shape[1] * v.shape[2] * v.shape[3]) ** -0.5).float()
        elif leaf == 'weight':
            g = randn(s, *v.shape) * 0.25 + 1.0
            g[1::3] *= -1
            sd[k] = g.float()
        else:
            sd[k] = (randn(s, *v.shape) * 0.3).float()
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# the reference construction

class Tape(object):
    """``maps``: the HIP forward's maps in call order (NCHW, CPU, fp32) or None for a free run.  ``units`` / ``pools`` collect
    what the run did: (key, pre-activation, output, had a ReLU, the mask used) and (input, indices used, output); ``out``:
    every unit and pool output in call order, the form of ``maps``.  A pool needs the HIP map of its input: the caller binds
    the module inputs (``bind_inputs``), the construction binds every output."""

    def __init__(self, maps=None):
        self.maps, self.i = maps, 0
        self.units, self.pools, self.hip, self.out = [], [], {}, []

    def next(self):
        if self.maps is None:
            return None
        m = self.maps[self.i]
        self.i += 1
        return m

    def bind(self, t, hip):
        """``t`` of the construction corresponds to the HIP map ``hip``"""
        if hip is not None:
            self.hip[id(t)] = (t, hip)
        return t

    def bind_inputs(self, xs):
        if self.maps is not None:
            for x in xs:
                self.bind(x, x.detach().float())

    def hip_of(self, t):
        return self.hip[id(t)][1]

    def done(self):
        assert self.maps is None or self.i == len(self.maps), 'the construction used %d of %d maps' % (self.i, len(self.maps))


def unit(x, sd, conv, bn, stride, res, relu, training, tape):
    """conv (no bias) -> BatchNorm (-> + res) (-> ReLU); running statistics of ``sd`` are updated in place when training"""
    w = sd[conv + '.weight']
    z = F.conv2d(x, w, None, stride, w.shape[2] // 2)
    pre = F.batch_norm(z, sd[bn + '.running_mean'], sd[bn + '.running_var'], sd[bn + '.weight'], sd[bn + '.bias'], training,
                       MOMENTUM, EPS)
    if training:
        sd[bn + '.num_batches_tracked'] += 1
    if res is not None:
        pre = pre + res
    hip = tape.next()
    assert hip is None or hip.shape == pre.shape, (conv, hip.shape, pre.shape)
    mask = (pre.detach() > 0) if hip is None else (hip > 0)
    y = pre * mask.to(pre.dtype) if relu else pre
    tape.units.append((conv, pre.detach(), y.detach(), relu, mask))
    tape.out.append(y.detach())
    return tape.bind(y, hip)


def pool(x, tape):
    hip = tape.next()
    if hip is None:
        y, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    else:
        hx = tape.hip_of(x)
        hy, idx = F.max_pool2d(hx, 2, 2, return_indices=True)
        assert torch.equal(hy, hip), 'the HIP pool output is not the maximum of its input'
        y = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    tape.pools.append((x.detach(), idx, y.detach()))
    tape.out.append(y.detach())
    return tape.bind(y, hip)


def basic_block(x, sd, p, stride, residual, training, tape):
    h = unit(x, sd, p + 'conv1', p + 'bn1', stride, None, True, training, tape)
    return unit(h, sd, p + 'conv2', p + 'bn2', 1, x if residual is None else residual, True, training, tape)


def root(xs, sd, p, residual, training, tape):
    return unit(torch.cat(xs, 1), sd, p + 'conv', p + 'bn', 1, xs[0] if residual else None, True, training, tape)


def tree(x, sd, p, levels, cin, cout, stride, level_root, root_residual, training, tape, children=None):
    """Tree.forward (dla.py:215-228)"""
    children = [] if children is None else children
    if levels == 1:
        h = unit(x, sd, p + 'tree1.conv1', p + 'tree1.bn1', stride, None, True, training, tape)
        bottom = pool(x, tape) if stride == 2 else x
        residual = unit(bottom, sd, p + 'project.0', p + 'project.1', 1, None, False, training, tape) if cin != cout else bottom
        if level_root:
            children.append(bottom)
        x1 = unit(h, sd, p + 'tree1.conv2', p + 'tree1.bn2', 1, residual, True, training, tape)
        x2 = basic_block(x1, sd, p + 'tree2.', 1, None, training, tape)
        return root([x2, x1] + children, sd, p + 'root.', root_residual, training, tape)
    bottom = pool(x, tape) if stride == 2 else x
    if cin != cout:
        unit(bottom, sd, p + 'project.0', p + 'project.1', 1, None, False, training, tape)       # read by nobody, as in the reference
    if level_root:
        children.append(bottom)
    x1 = tree(x, sd, p + 'tree1.', levels - 1, cin, cout, stride, False, root_residual, training, tape)
    children.append(x1)
    return tree(x1, sd, p + 'tree2.', levels - 1, cout, cout, 1, False, root_residual, training, tape, children=children)


def stem(x, sd, p, training, tape):
    return unit(x, sd, p + '0', p + '1', 1, None, True, training, tape)


def dla(x, pre_img, pre_hm, sd, training, tape, levels=None, channels=None):
    """DLA.forward (dla.py:305-316) -> the six level outputs"""
    levels, channels = levels or DLA34['levels'], channels or DLA34['channels']
    y = stem(x, sd, 'base_layer.', training, tape)
    if pre_img is not None:
        y = y + stem(pre_img, sd, 'pre_img_layer.', training, tape)
    if pre_hm is not None:
        y = y + stem(pre_hm, sd, 'pre_hm_layer.', training, tape)
    out = []
    for lv in (0, 1):
        assert levels[lv] == 1
        y = unit(y, sd, 'level%d.0' % lv, 'level%d.1' % lv, lv + 1, None, True, training, tape)
        out.append(y)
    for lv in range(2, 6):
        y = tree(y, sd, 'level%d.' % lv, levels[lv], channels[lv - 1], channels[lv], 2, lv > 2, False, training, tape)
        out.append(y)
    return out


class Opt(object):
    pre_img, pre_hm = True, True


def _block_s2(xs, sd, tape, training):
    return [basic_block(xs[0], sd, '', 2, xs[1], training, tape)]


def _block_id(xs, sd, tape, training):
    return [basic_block(xs[0], sd, '', 1, None, training, tape)]


def _root(residual):
    return lambda xs, sd, tape, training: [root(list(xs), sd, '', residual, training, tape)]


def _tree1(xs, sd, tape, training):
    return [tree(xs[0], sd, '', 1, 32, 64, 2, False, False, training, tape)]


def _tree2(xs, sd, tape, training):
    return [tree(xs[0], sd, '', 2, 64, 128, 2, True, False, training, tape)]


def _dla(xs, sd, tape, training):
    return dla(xs[0], xs[1], xs[2], sd, training, tape)


# name -> (module factory on centertrack_amd.dla_base, N, input shapes (C, H, W), the construction, pixels of the finest map)
MODULES = OrderedDict([
    ('block-s2', (lambda db: db.BasicBlock(32, 64, 2), 2, [(32, 8, 12), (64, 4, 6)], _block_s2)),
    ('block-identity', (lambda db: db.BasicBlock(64, 64), 2, [(64, 8, 12)], _block_id)),
    ('root', (lambda db: db.Root(160, 64, 1, False), 2, [(64, 8, 12), (64, 8, 12), (32, 8, 12)], _root(False))),
    ('root-residual', (lambda db: db.Root(160, 64, 1, True), 2, [(64, 8, 12), (64, 8, 12), (32, 8, 12)], _root(True))),
    ('tree-1', (lambda db: db.Tree(1, db.BasicBlock, 32, 64, 2), 2, [(32, 16, 24)], _tree1)),
    ('tree-2', (lambda db: db.Tree(2, db.BasicBlock, 64, 128, 2, level_root=True), 2, [(64, 16, 16)], _tree2)),
    ('dla34', (lambda db: db.dla34(pretrained=False, opt=Opt()), 2, [(3, 64, 64), (3, 64, 64), (1, 64, 64)], _dla)),
])


SEEDS = dict((n, 1000 + 100 * i) for i, n in enumerate(list(MODULES) + ['sgd', 'step']))
SGD_STEPS = 3


def sgd_lr(key, tensor):
    """two parameter groups: the convolution weights (gradients of order 10 on values of order 0.05) at 2e-4, gamma and beta at
    2e-3; every tensor a gradient reaches then moves by 1e-3 .. 3e-2 of its maximum in three steps"""
    return 2e-4 if tensor.dim() == 4 else 2e-3


def sgd_data(step):
    """(inputs, output gradients) of one step of the level-3 ``Tree`` trajectory (the 'tree-2' case)"""
    inputs = module_inputs('tree-2', SEEDS['sgd'] + 10 * step + 1)
    gys = [(randn(SEEDS['sgd'] + 10 * step + 5, 2, 128, 8, 8) / 128 ** 0.5).float()]
    return inputs, gys


def sgd_start():
    from centertrack_amd import dla_base
    return random_params(SEEDS['sgd'], MODULES['tree-2'][0](dla_base))


def sgd_trajectory(dtype, maps_per_step):
    """SGD_STEPS plain SGD steps (``sgd_lr``) of the construction in ``dtype`` from ``sgd_start()``; step t takes its ReLU masks
    and pool selections from ``maps_per_step[t]`` (None: a free run) -> (final state dict, {key: movement of the tensor
    relative to its maximum})"""
    sd0 = sgd_start()
    sd = cast(sd0, dtype)
    for step in range(SGD_STEPS):
        inputs, gys = sgd_data(step)
        r = reference('tree-2', sd, inputs, gys, True, dtype, None if maps_per_step is None else maps_per_step[step])
        sd = r['sd']
        for k, g in r['gpar'].items():
            sd[k] = sd[k].detach() - sgd_lr(k, g) * g
    moved = OrderedDict((k, err(sd0[k], sd[k].detach().double())) for k in sd0 if sd0[k].dtype != torch.long)
    return sd, moved


def module_call(name, m, xs):
    """the module's own calling convention -> list of outputs"""
    if name == 'block-s2':
        return [m(xs[0], xs[1])]
    if name.startswith('root'):
        return [m(*xs)]
    if name == 'dla34':
        return list(m(xs[0], xs[1], xs[2]))
    return [m(xs[0])]


def module_inputs(name, seed):
    _, N, shapes, _ = MODULES[name]
    xs = [randn(seed + i, N, *s).float() for i, s in enumerate(shapes)]
    if name == 'dla34':
        xs[2] = xs[2].abs().clamp(max=1.0)                           # a prior heat-map lies in [0, 1]
    if name.startswith('tree'):
        xs = [torch.relu(x) for x in xs]                             # a Tree reads a post-ReLU map: its pool meets exact ties
    return xs


def output_gradients(outs, seed):
    """one incoming gradient per output, scaled by (pixels)^-1/2 so that sums over a map stay of order 1"""
    return [(randn(seed + i, *o.shape) / (o.shape[0] * o.shape[2] * o.shape[3]) ** 0.5).float() for i, o in enumerate(outs)]


def reference(name, sd, inputs, gys, training, dtype, maps=None):
    """one forward (and, with ``gys``, backward) of the construction in ``dtype`` -> dict(outs, gin, gpar, tape, sd); ``maps``:
    the HIP forward's maps (NCHW, CPU) or None for a free run"""
    fn = MODULES[name][3]
    sd = cast(sd, dtype, grad=gys is not None)
    xs = [x.to(dtype).clone().requires_grad_(gys is not None) for x in inputs]
    tape = Tape(maps)
    tape.bind_inputs(xs)
    outs = fn(xs, sd, tape, training)
    tape.done()
    res = dict(outs=[o.detach() for o in outs], tape=tape, sd=sd)
    if gys is not None:
        names = [k for k in sd if not is_buffer(k)]
        gs = grads(outs, gys, xs + [sd[k] for k in names])
        res['gin'], res['gpar'] = gs[:len(xs)], dict(zip(names, gs[len(xs):]))
    return res


def output_K(name):
    """K of each forward map: the fan-in of the unit that writes it, 9 Cin for a 3x3 unit, Cin for the 1x1 conv of a ``Root``
    (whose Cin is the width of the concatenation: 2 Cout, + Cin of the tree with ``level_root``, + Cout per outer level)"""
    c = DLA34['channels']
    return {'block-s2': [9 * 64], 'block-identity': [9 * 64], 'root': [160], 'root-residual': [160],
            'tree-1': [2 * 64], 'tree-2': [2 * 128 + 64 + 128],
            'dla34': [9 * c[0], 9 * c[0], 2 * c[2], 2 * c[3] + c[2] + c[3], 2 * c[4] + c[3] + c[4], 2 * c[5] + c[4]]}[name]


def input_K(name):
    """K of each input gradient: the terms of one element in the unit that reads the input -- 9 Cout behind a 3x3 stride-1
    unit, 4 Cout behind a 3x3 stride-2 unit (at most four taps reach one input pixel), Cout behind a 1x1 unit, 49 * 16 behind a
    7x7 stem, 1 for the residual input of a block (its gradient is a selection of the incoming one).  The further paths of an
    input (a residual, the pool) add single terms.  An input gradient of ``dla34`` crosses the whole network, so its error is
    set by e32, not by this floor; K only names the last sum."""
    return {'block-s2': [4 * 64, 1], 'block-identity': [9 * 64], 'root': [64, 64, 64], 'root-residual': [64, 64, 64],
            'tree-1': [4 * 64], 'tree-2': [4 * 128], 'dla34': [49 * 16] * 3}[name]


def pixels_of(name, key, inputs):
    """K of a parameter's gradient: the pixels N*H*W of the map its unit writes"""
    N, _, H, W = inputs[0].shape
    if name == 'dla34':
        lv = key.split('.')[0]
        s = {'level%d' % i: 4 ** i for i in range(6)}.get(lv, 1)
        return N * H * W // s
    if name in ('block-s2', 'tree-1', 'tree-2'):
        return N * H * W // 4
    return N * H * W


# ---------------------------------------------------------------------------------------------------------------------
# what holds the masks and selections a truth was given

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


def check_selection(idx_hip, x64, e32_x, what=''):
    """the indices the HIP forward's pool selected may differ from the float64 run's own only where the value float64 finds
    there lies within 64 * e32(x) * max|x64| of float64's maximum, at no more than 0.1 % of the windows -> windows that differ"""
    y64, idx64 = F.max_pool2d(x64, 2, 2, return_indices=True)
    got = x64.flatten(2).gather(2, idx_hip.flatten(2)).view(idx_hip.shape)
    thr = 64.0 * e32_x * float(x64.abs().max())
    differ = idx_hip != idx64
    assert not bool((differ & ((y64 - got) > thr)).any()), '%s: a pool selected a value away from the maximum (threshold %.3g)' % (what, thr)
    assert int(differ.sum()) <= 1e-3 * idx64.numel(), '%s: %d of %d windows differ' % (what, int(differ.sum()), idx64.numel())
    return int(differ.sum())


def check_tape(title, given, free64, free32):
    """``given``: the Tape of a run that was handed HIP maps; ``free64`` / ``free32``: the Tapes of the free runs.  Every ReLU
    mask and pool selection of ``given`` is held against the free float64 run.  -> (flipped units, differing windows)"""
    assert len(given.units) == len(free64.units) and len(given.pools) == len(free64.pools)
    flips = wins = 0
    for (k, _, _, relu, mask), (_, pre64, y64, _, _), (_, _, y32, _, _) in zip(given.units, free64.units, free32.units):
        if relu:
            flips += check_mask(mask, pre64, err(y32, y64), '%s %s' % (title, k))[0]
    for i, ((_, idx, _), (x64, _, _), (x32, _, _)) in enumerate(zip(given.pools, free64.pools, free32.pools)):
        e = err(x32, x64) if float(x64.abs().max()) > 0 else 0.0
        wins += check_selection(idx, x64, e, '%s pool %d' % (title, i))
    return flips, wins


class Report(object):
    """collects (name, error, bound) of one test, prints every figure and fails at the end with all of them"""

    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, name, got, t64, t32, K, norm=None):
        got, t64, t32 = got.detach().cpu().double(), t64.detach().double(), t32.detach().double()
        assert got.shape == t64.shape, (name, got.shape, t64.shape)
        if norm is None and float(t64.abs().max()) == 0.0:
            e, e32, b = float(got.abs().max()), 0.0, 0.0
        else:
            e, e32 = err(got, t64, norm), err(t32, t64, norm)
            b = bound(e32, K)
        self.rows.append((name, e, e32, b))
        print('%s %-44s err %.2e  e32 %.2e  bound %.2e%s' % (self.title, name, e, e32, b, '' if e <= b else '   <-- MISSES'))

    def check(self):
        bad = [r for r in self.rows if not r[1] <= r[3]]
        assert not bad, '%s: %s' % (self.title, ['%s err %.2e > bound %.2e' % (r[0], r[1], r[3]) for r in bad])
