"""Shared pieces of the non-finite tests (tests/test_nonfinite_cpu.py, tests/test_hip_nonfinite.py): the rule a training kernel is
held to when one element of its input is NaN, +Inf or -Inf, and the planted inputs.  No GPU, no ctypes.

The rule (``compare``), for a kernel output ``hip`` and the float64 torch reference ``ref64`` of the same op on the same planted input:

  (a) no laundering   where ref64 is NaN hip is NaN, where ref64 is +-Inf hip is the same infinity;
  (b) bounded spread  where hip is non-finite and ref64 is finite the element lies inside ``spread``, a mask derived from the
                      launch's tile geometry and never from the output (element-wise, pooling, BatchNorm and loss ops: empty);
  (c) the rest        on the elements finite on both sides the op's usual measure and bound hold: ``err`` and ``bound(e32, K)`` of
                      tests/_dcn_bwd.py with e32 taken on the same finite set, or bit equality where the op is bit-equal today;
  (d) no hiding       the finite set holds at least ``floor`` of the output (0.75; 7/8 for a BatchNorm over 8 channels with one
                      planted channel).  Every case is placed so that the float64 reference ALONE satisfies this
                      (tests/test_nonfinite_cpu.py asserts it for every case of ``cases()``).

A case (``Case``) is built on the fixtures of the op's own tests (_neck_bwd, _backbone_bwd, _conv_fwd, _heads_bwd, _stem_bwd,
_loss_ref) with exactly one element replaced.  ``Case.reference(dtype, launder)`` runs the op in torch on the CPU; ``launder`` emulates
the kernels before this rule held (``nan_to_num`` behind every ReLU, pool and clamp) so that the CPU tests can show that ``compare``
rejects them."""
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import _backbone_bwd as BB
import _conv_fwd as CF
import _dcn_bwd as DB
import _heads_bwd as HB
import _loss_ref as R
import _neck_bwd as NB
import _stem_bwd as SB
from _dcn_bwd import bound, randn

NAN, INF = float('nan'), float('inf')
VALUES = OrderedDict([('nan', NAN), ('+inf', INF), ('-inf', -INF)])
FLOOR = 0.75


class Rejected(AssertionError):
    """``compare`` refused a result; ``rule`` = 'a' | 'b' | 'c' | 'd'"""

    def __init__(self, rule, text):
        AssertionError.__init__(self, '(%s) %s' % (rule, text))
        self.rule = rule


def same_nonfinite(hip, ref):
    """the elements at which ``hip`` carries the non-finite value of ``ref``: NaN for NaN, the same infinity for an infinity"""
    return (torch.isnan(ref) & torch.isnan(hip)) | (torch.isinf(ref) & (hip == ref))


def project_bound(ref32, K):
    """the project's bound as ``compare`` wants it: ``finite -> bound(e32, K)`` with e32 = the error of the float32 reference
    ``ref32`` against float64 on that finite set"""
    def of(finite, ref64):
        r32 = ref32.detach().double().cpu()
        ok = finite & torch.isfinite(r32)
        norm = float(ref64[finite].abs().max()) if bool(finite.any()) else 0.0
        e32 = float((r32[ok] - ref64[ok]).abs().max()) / norm if norm > 0 and bool(ok.any()) else 0.0
        return bound(e32, K), e32
    return of


def compare(hip, ref64, bound, spread=None, floor=FLOOR, what=''):
    """The four rules of the module docstring.  ``bound``: 'equal' (bit equality on the finite set) or ``project_bound(ref32, K)``.
    Raises ``Rejected``; returns dict(err, bound, e32, ratio, finite) of rule (c)."""
    hip, ref64 = hip.detach().cpu().double(), ref64.detach().cpu().double()
    if hip.shape != ref64.shape:
        raise Rejected('c', '%s: shape %s against %s' % (what, tuple(hip.shape), tuple(ref64.shape)))
    spread = torch.zeros_like(ref64, dtype=torch.bool) if spread is None else spread.expand_as(ref64)
    rf, hf = torch.isfinite(ref64), torch.isfinite(hip)
    laundered = ~rf & ~same_nonfinite(hip, ref64)
    if bool(laundered.any()):
        i = tuple(int(v) for v in laundered.nonzero()[0])
        raise Rejected('a', '%s: %d of %d non-finite reference elements laundered, first at %s: reference %s, got %s'
                       % (what, int(laundered.sum()), int((~rf).sum()), i, float(ref64[i]), float(hip[i])))
    extra = ~hf & rf & ~spread
    if bool(extra.any()):
        i = tuple(int(v) for v in extra.nonzero()[0])
        raise Rejected('b', '%s: %d non-finite elements outside the spread, first at %s: %s where the reference has %s'
                       % (what, int(extra.sum()), i, float(hip[i]), float(ref64[i])))
    finite = rf & hf
    share = float(finite.double().mean()) if finite.numel() else 1.0
    if share < floor:
        raise Rejected('d', '%s: only %.3f of the output is finite on both sides (floor %.3f)' % (what, share, floor))
    if isinstance(bound, str):
        assert bound == 'equal'
        differ = finite & (hip != ref64)
        if bool(differ.any()):
            i = tuple(int(v) for v in differ.nonzero()[0])
            raise Rejected('c', '%s: %d finite elements differ, first at %s: %r against %r'
                           % (what, int(differ.sum()), i, float(hip[i]), float(ref64[i])))
        return dict(err=0.0, bound=0.0, e32=0.0, ratio=0.0, finite=share)
    b, e32 = bound(finite, ref64)
    norm = float(ref64[finite].abs().max()) if bool(finite.any()) else 0.0
    worst = float((hip[finite] - ref64[finite]).abs().max()) if bool(finite.any()) else 0.0
    e = worst / norm if norm > 0 else worst
    print('NONFINITE %-58s err %.3e e32 %.3e bound %.3e ratio %.3f finite %.3f' % (what, e, e32, b, e / b if b > 0 else 0.0, share))
    if not e <= b:
        raise Rejected('c', '%s: err %.3e > bound %.3e on the finite set' % (what, e, b))
    return dict(err=e, bound=b, e32=e32, ratio=e / b if b > 0 else 0.0, finite=share)


def finite_share(ref64):
    """the share of finite elements: rule (d) from the reference alone"""
    return float(torch.isfinite(ref64).double().mean())


def launder(t):
    """what fmaxf / fminf made of a non-finite value behind a ReLU, a pool or a clamp: a finite number"""
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


def plant(t, index, value):
    """a copy of ``t`` with ``value`` at ``index`` (a tuple)"""
    t = t.clone()
    t[index] = value
    return t


class Case(object):
    """One planted input of one op.  ``run(dtype, launder) -> {output: tensor}`` is the torch reference; ``outputs`` =
    {output: dict(K=..., equal=..., spread=..., floor=...)}; ``inputs`` = what the GPU test hands the kernel (fp32, CPU);
    ``launders``: whether the op holds a ReLU, a pool or a clamp that the emulation can turn finite."""

    def __init__(self, family, name, inputs, run, outputs, launders=False, meta=None):
        self.family, self.name, self.inputs, self.run, self.outputs = family, name, inputs, run, outputs
        self.launders, self.meta = launders, meta or {}
        self._ref = {}

    @property
    def id(self):
        return '%s-%s' % (self.family, self.name)

    def reference(self, dtype=torch.float64, laundered=False):
        key = (dtype, laundered)
        if key not in self._ref:
            with torch.no_grad() if self.meta.get('no_grad') else torch.enable_grad():
                self._ref[key] = OrderedDict((k, v.detach()) for k, v in self.run(dtype, laundered).items())
        return self._ref[key]

    def check(self, got, only=None):
        """``compare`` of every output of ``got`` = {output: tensor}; -> {output: figures}"""
        r64, r32 = self.reference(torch.float64), self.reference(torch.float32)
        res = OrderedDict()
        for k, spec in self.outputs.items():
            if only is not None and k not in only:
                continue
            b = 'equal' if spec.get('equal') else project_bound(r32[k], spec['K'])
            res[k] = compare(got[k], r64[k], b, spec.get('spread'), spec.get('floor', FLOOR), '%s %s' % (self.id, k))
        return res


def _out(K=None, equal=False, spread=None, floor=FLOOR):
    return dict(K=K, equal=equal, spread=spread, floor=floor)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm (+ residual) + ReLU, forward and backward; the statistics

BN_SHAPE = (2, 9, 11, 8)                  # N, H, W, C: odd map, 198 pixels, two channel quads
BN_FLOOR = 7.0 / 8.0                      # one planted channel of eight
BN_CHANNEL, BN_PIXEL = 5, (0, 4, 5)       # the planted channel (gamma < 0 there) and (n, y, x): a positive pre-activation in all four modes
BN_MARGIN = (0.02, 1e-4)                 # channel 0 (mean 100, std 0.01: fp32 loses 1e-3 of a pre-activation there), the others


def bn_inputs():
    """``_neck_bwd.bn_case`` at BN_SHAPE with a residual, z nudged so that no pre-activation of the four modes (batch / running
    statistics, with / without the residual) lies within BN_MARGIN of 0 (the constant channel 1, whose batch-statistics
    pre-activation is beta + res whatever z holds, is left alone: nothing is lost there in fp32): float32 and float64 then agree
    on every ReLU mask, and the float64 reference can run torch.relu itself"""
    if 'bn' not in _cache:
        z, gamma, beta, rm, rv, gy, res = NB.bn_case(BN_SHAPE, residual=True)
        z = z.double()
        margin = torch.full((1, BN_SHAPE[3], 1, 1), BN_MARGIN[1], dtype=torch.float64)
        margin[0, 0] = BN_MARGIN[0]
        for it in range(32):
            moved = False
            for batch in (True, False):
                for residual in (True, False):
                    pre = F.batch_norm(z, rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), batch, NB.MOMENTUM, NB.EPS)
                    if residual:
                        pre = pre + res.double()
                    near = pre.abs() < 2 * margin
                    near[:, 1] = False                                # (the constant channel stays constant: pre = beta there)
                    if bool(near.any()):
                        std = z.var((0, 2, 3), unbiased=False, keepdim=True).sqrt() if batch else rv.double().view(1, -1, 1, 1).sqrt()
                        step = 0.25 * std / gamma.double().abs().view(1, -1, 1, 1).clamp(min=0.1)
                        z = torch.where(near, z + step * (1.0 + 0.37 * it), z)
                        moved = True
            if not moved:
                break
        z = z.float()
        for batch in (True, False):
            for residual in (True, False):
                pre = F.batch_norm(z.double(), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), batch, NB.MOMENTUM, NB.EPS)
                pre = pre + res.double() if residual else pre
                assert bool((pre.abs() >= margin).all()), (batch, residual, float(pre.abs().min()))
        _cache['bn'] = [z, gamma, beta, rm, rv, gy, res]
    return _cache['bn']


_cache = {}


def _bn_run(t, batch, residual, relu, backward):
    def run(dtype, laundered):
        z, gamma, beta, rm, rv, gy, res = (v.to(dtype).clone() for v in t)
        z, gamma, beta, res = (v.requires_grad_() for v in (z, gamma, beta, res))
        pre = F.batch_norm(z, rm, rv, gamma, beta, batch, NB.MOMENTUM, NB.EPS)
        if residual:
            pre = pre + res
        y = pre
        if relu:
            y = torch.relu(launder(pre)) if laundered else torch.relu(pre)
        out = OrderedDict(y=y.detach())
        if backward:
            gz, gg, gb, gr = torch.autograd.grad(y, (z, gamma, beta, res), gy, allow_unused=True)
            out.update(gz=gz, ggamma=gg, gbeta=gb)
            if residual:
                out['gres'] = gr
        return out
    return run


def bn_cases():
    L = []
    base = bn_inputs()
    n, y, x = BN_PIXEL
    idx = (n, BN_CHANNEL, y, x)
    P = BN_SHAPE[0] * BN_SHAPE[1] * BN_SHAPE[2]
    for batch in (True, False):
        for residual in (True, False):
            mode = '%s-%s' % ('batch' if batch else 'running', 'res' if residual else 'nores')
            floor = BN_FLOOR
            for where in ('z', 'res', 'gy'):
                if where == 'res' and not residual:
                    continue
                for vname, v in VALUES.items():
                    t = list(base)
                    k = {'z': 0, 'res': 6, 'gy': 5}[where]
                    t[k] = plant(t[k], idx, v)
                    if where != 'gy':
                        L.append(Case('bn_act_apply', '%s-%s-%s' % (mode, where, vname), dict(t=t, batch=batch, residual=residual, relu=True),
                                      _bn_run(t, batch, residual, True, False), OrderedDict(y=_out(K=P, floor=floor)), launders=True))
                    if vname == 'nan' or where == 'gy':
                        outs = OrderedDict(gz=_out(K=P, floor=floor), ggamma=_out(K=P, floor=floor), gbeta=_out(K=P, floor=floor))
                        if residual:
                            outs['gres'] = _out(K=P, floor=floor)
                        # (the emulation cannot launder a backward: torch's relu backward reads the laundered input and the
                        # planted gy stays what it is, so only the z / res plants are rejected through y)
                        L.append(Case('bn_act_backward', '%s-%s-%s' % (mode, where, vname), dict(t=t, batch=batch, residual=residual, relu=True),
                                      _bn_run(t, batch, residual, True, True), outs, launders=where != 'gy'))
    return L


def bn_stats_reference(z, dtype=torch.float64):
    """(mean, biased variance, 1 / sqrt(var + eps)) per channel of an NCHW map as torch computes them"""
    z = z.to(dtype)
    mean = z.mean((0, 2, 3))
    var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    return mean, var, 1.0 / torch.sqrt(var + NB.EPS)


def bn_stats_cases():
    """[(name, planted z, channel)]: one Inf, then one NaN, in one channel away from the pivot pixel; and the Inf AT the pivot
    (pixel 0 of the view), where ``sum(z - pivot)`` meets Inf - Inf: the mean is NaN where torch's is Inf"""
    z = bn_inputs()[0]
    n, y, x = BN_PIXEL
    return [('inf', plant(z, (n, BN_CHANNEL, y, x), INF), BN_CHANNEL), ('-inf', plant(z, (n, BN_CHANNEL, y, x), -INF), BN_CHANNEL),
            ('nan', plant(z, (n, BN_CHANNEL, y, x), NAN), BN_CHANNEL), ('inf-at-the-pivot', plant(z, (0, BN_CHANNEL, 0, 0), INF), BN_CHANNEL)]


# ---------------------------------------------------------------------------------------------------------------------
# the stems' BatchNorm + ReLU + sum

STEM_SHAPE = (2, 9, 11)


def stem_inputs():
    """(state dict, [z_s] = the three stems' conv outputs in fp32 (NCHW), gz = the gradient of the sum)"""
    if 'stem' not in _cache:
        sd, xs, gy = SB.case(STEM_SHAPE)
        zs = [F.conv2d(xs[s], sd[SB.PREFIX[s] + '0.weight'], None, 1, 3) for s in range(3)]
        _cache['stem'] = (sd, xs, zs, gy)
    return _cache['stem']


def _stem_sum_run(sd, zs):
    def run(dtype, laundered):
        y = 0
        for s in range(3):
            p = SB.PREFIX[s]
            pre = F.batch_norm(zs[s].to(dtype), sd[p + '1.running_mean'].to(dtype), sd[p + '1.running_var'].to(dtype),
                               sd[p + '1.weight'].to(dtype), sd[p + '1.bias'].to(dtype), False, NB.MOMENTUM, NB.EPS)
            y = y + torch.relu(launder(pre) if laundered else pre)
        return OrderedDict(y=y)
    return run


def stem_cases():
    sd, xs, zs, gy = stem_inputs()
    L = []
    for s in range(3):
        for vname, v in VALUES.items():
            t = list(zs)
            t[s] = plant(t[s], (1, 3 + s, 4, 7), v)
            L.append(Case('stem_bn_relu_sum', 'stem%d-%s' % (s, vname), dict(sd=sd, zs=t), _stem_sum_run(sd, t),
                          OrderedDict(y=_out(K=3)), launders=True, meta=dict(no_grad=True)))
    # the convolution's backward with one NaN in the gradient of z_s, away from the border (no tap of the planted pixel meets
    # the zero padding): the 7 x 7 footprint of the image gradient is 49 of 198 pixels, the weight gradient loses the planted
    # output channel
    for s in (0, 2):
        gz = [randn(5200 + i, STEM_SHAPE[0], 16, STEM_SHAPE[1], STEM_SHAPE[2]).float() / math.sqrt(198.0) for i in range(3)]
        co = 5
        gz[s] = plant(gz[s], (0, co, 4, 5), NAN)

        def run(dtype, laundered, s=s, gz=gz):
            x = xs[s].to(dtype).clone().requires_grad_()
            w = sd[SB.PREFIX[s] + '0.weight'].to(dtype).clone().requires_grad_()
            gin, gw = torch.autograd.grad(F.conv2d(x, w, None, 1, 3), (x, w), gz[s].to(dtype))
            return OrderedDict(gin=gin, gw=gw)
        rowmask = torch.zeros(16, 1, 1, 1, dtype=torch.bool)
        rowmask[co] = True
        L.append(Case('stem_conv_backward', 'stem%d-gz-nan' % s, dict(sd=sd, xs=xs, gz=gz, s=s), run,
                      OrderedDict(gin=_out(K=SB.K_IN), gw=_out(K=2 * 9 * 11, spread=rowmask))))
    return L


# ---------------------------------------------------------------------------------------------------------------------
# max-pool, forward and backward

POOL_SHAPE = (2, 9, 11, 8)                # odd H and W: the last row and column are dropped


def pool_inputs():
    N, H, W, Cc = POOL_SHAPE
    return torch.relu(randn(61, N, Cc, H, W)).float(), randn(62, N, Cc, H // 2, W // 2).float()


def pool_cases():
    x, gy = pool_inputs()
    N, H, W, Cc = POOL_SHAPE
    L = []
    for pos in range(4):
        for vname, v in VALUES.items():
            xp = plant(x, (1, 3, 2 * 1 + pos // 2, 2 * 3 + pos % 2), v)

            def fwd(dtype, laundered, xp=xp):
                return OrderedDict(y=F.max_pool2d(launder(xp.to(dtype)) if laundered else xp.to(dtype), 2, 2))
            L.append(Case('maxpool2x2', 'pos%d-%s' % (pos, vname), dict(x=xp), fwd, OrderedDict(y=_out(equal=True)), launders=vname != '-inf',
                          meta=dict(no_grad=True)))
            if vname == 'nan':
                xe = xp[:, :, :2 * (H // 2), :2 * (W // 2)].contiguous()           # (the backward takes even maps only)

                def bwd(dtype, laundered, xe=xe):
                    xt = xe.to(dtype).clone().requires_grad_()
                    gx, = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, gy.to(dtype))
                    return OrderedDict(gx=gx)
                L.append(Case('maxpool2x2_backward', 'pos%d-%s' % (pos, vname), dict(x=xe, gy=gy), bwd, OrderedDict(gx=_out(equal=True))))
    return L


# ---------------------------------------------------------------------------------------------------------------------
# ct_conv2d: ReLU epilogues on the four launch families, the pool side output of the two stride-2 families

# the smallest case of _conv_fwd.GPU_CASES of each family (Winograd: the smallest with more than one tile each way, so that the
# spread of a pixel is a proper part of the map), with the ReLU switched on where it is not; scale and shift are present in all
CONV_BASES = OrderedDict([('row', 'chunks1_k1s1_nkk1'), ('ksplit', 'ksplit1_k1_chunks1'), ('splitk', 'split_auto_half'),
                          ('wino', 'wino202_cin64')])
CONV_POOL_BASES = OrderedDict([('row', 'rowpool_cfg7_pool'), ('ksplit', 'ksplitpool0_pool')])


def conv_case_of(family):
    base = CF.CASE[CONV_BASES[family]]
    return base._replace(name='nonfinite_' + base.name, relu=True)


def wino_spread(case, n, y, x):
    """[N,1,H,W] outputs a non-finite input pixel (n, y, x) can reach in a Winograd F(2x2, 3x3) launch: every 2 x 2 output tile
    whose 4 x 4 input tile (rows 2i - 1 .. 2i + 2) holds the pixel -- the direct 3 x 3 footprint dilated by the tile overlap"""
    m = torch.zeros(case.N, 1, case.H, case.W, dtype=torch.bool)
    for i in range(CF.cdiv(case.H, 2)):
        for j in range(CF.cdiv(case.W, 2)):
            if 2 * i - 1 <= y <= 2 * i + 2 and 2 * j - 1 <= x <= 2 * j + 2:
                m[n, 0, 2 * i:2 * i + 2, 2 * j:2 * j + 2] = True
    return m


def direct_footprint(case, n, y, x):
    """[N,1,Ho,Wo] outputs whose window holds input pixel (n, y, x)"""
    p = CF.plan_of(case)
    pad = case.ks // 2
    m = torch.zeros(case.N, 1, p['Ho'], p['Wo'], dtype=torch.bool)
    for oy in range(p['Ho']):
        for ox in range(p['Wo']):
            if 0 <= y - (oy * case.stride - pad) < case.ks and 0 <= x - (ox * case.stride - pad) < case.ks:
                m[n, 0, oy, ox] = True
    return m


def _conv_run(case, d):
    def run(dtype, laundered, conv=None):
        x, w = d['x'].to(dtype), d['w'].to(dtype)
        if conv is None and dtype == torch.float32 and 201 <= case.algo <= 211:
            conv = CF.winograd32                                       # the yardstick of a Winograd launch (_conv_fwd.yardstick32)
        z = F.conv2d(x, w, None, case.stride, case.ks // 2) if conv is None else conv(x, w)
        if laundered:
            lin = case._replace(relu=False)
            y = torch.relu(launder(CF.epilogue(lin, z, d, dtype)))
        else:
            y = CF.epilogue(case, z, d, dtype)
        out = OrderedDict(y=y)
        if case.pool:
            out['pool'] = F.max_pool2d(launder(d['x']) if laundered else d['x'], 2, 2).to(dtype)
        return out
    return run


def conv_cases():
    L = []
    for fam in CONV_BASES:
        case = conv_case_of(fam)
        base = CF.conv_inputs(case)
        wino = fam == 'wino'
        n, y, x = case.N - 1, min(2, case.H - 1), min(5, case.W - 1)
        co, ci = 3, 7
        chan = torch.zeros(1, case.Cout, 1, 1, dtype=torch.bool)
        chan[0, co] = True
        # Winograd transforms d -> B^T d B and g -> G g G^T with differences: an infinity meets its own negative there, so the
        # algorithm keeps a NaN a NaN but cannot keep an infinity an infinity; x and w take the NaN only
        plants = [('x', (n, ci, y, x), ('nan',) if wino else tuple(VALUES)), ('w', (co, ci, case.ks // 2, case.ks // 2), ('nan',) if wino else tuple(VALUES)),
                  ('shift', (co,), tuple(VALUES))]
        for where, idx, values in plants:
            for vname in values:
                d = dict(base)
                d[where] = plant(d[where], idx, VALUES[vname])
                if where == 'x':
                    spread = wino_spread(case, n, y, x) if wino else None
                else:
                    spread = chan if wino else None                          # (a planted weight or shift owns its whole channel)
                L.append(Case('conv2d_relu', '%s-%s-%s' % (fam, where, vname), dict(case=case, d=d), _conv_run(case, d),
                              OrderedDict(y=_out(K=case.Cin * case.ks ** 2, spread=spread)), launders=True,
                              meta=dict(no_grad=True, wino=wino, pixel=(n, y, x), where=where)))
    for fam, name in CONV_POOL_BASES.items():
        case = CF.CASE[name]
        base = CF.conv_inputs(case)
        for pos in (0, 3):
            for vname in ('nan', '+inf'):
                d = dict(base)
                d['x'] = plant(d['x'], (1, 5, 2 * 2 + pos // 2, 2 * 7 + pos % 2), VALUES[vname])
                L.append(Case('conv2d_pool', '%s-pos%d-%s' % (fam, pos, vname), dict(case=case, d=d), _conv_run(case, d),
                              OrderedDict(y=_out(K=case.Cin * 9), pool=_out(equal=True)), launders=True, meta=dict(no_grad=True)))
    return L


# ---------------------------------------------------------------------------------------------------------------------
# the heads' tail backward

HEADS_CASE = HB.SHAPES[0]                 # (2, 11, 13) with the MOT heads


def _heads_run(fx):
    def run(dtype, laundered):
        pre = fx['mid'].to(dtype).clone().requires_grad_()        # mid >= 0: relu(mid) = mid, and relu'(0) = 0 as in the kernel
        mid = torch.relu(pre)
        w2 = [fx['w2'][h].to(dtype).clone().requires_grad_() for h in fx['heads']]
        b2 = [torch.zeros(w.shape[0], dtype=dtype, requires_grad=True) for w in w2]
        tot = 0
        for j, h in enumerate(fx['heads']):
            tot = tot + (F.conv2d(mid[:, HB.HC * j:HB.HC * (j + 1)], w2[j], b2[j]) * fx['gout'][h].to(dtype)).sum()
        g = torch.autograd.grad(tot, [pre] + w2 + b2)
        nh = len(w2)
        return OrderedDict(gmid=g[0], x=F.conv_transpose2d(g[0], fx['w0'].to(dtype), padding=1),
                           w2=torch.cat([t.reshape(-1) for t in g[1:1 + nh]]), b2=torch.cat(g[1 + nh:]))
    return run


def heads_cases():
    (N, H, W), heads = HEADS_CASE
    base = HB.tail_fixture(HEADS_CASE)
    P = N * H * W
    L = []
    for where in ('mid', 'gout'):
        fx = dict(base)
        if where == 'mid':
            fx['mid'] = plant(base['mid'], (1, HB.HC + 17, 4, 6), NAN)           # head 1 ('reg'), hidden unit 17
        else:
            fx['gout'] = OrderedDict(base['gout'])
            fx['gout']['wh'] = plant(base['gout']['wh'], (1, 1, 4, 6), NAN)
        # (w2 / b2: the heads' gradients side by side, [sum c * hc] and [sum c])
        outs = OrderedDict(gmid=_out(K=max(heads.values())), x=_out(K=9 * HB.HC * len(heads)), w2=_out(K=P), b2=_out(K=P))
        L.append(Case('heads_backward', where + '-nan', dict(fx=fx), _heads_run(fx), outs))
    return L


# ---------------------------------------------------------------------------------------------------------------------
# linear kernels: no laundering, bounded spread

LIN = dict(N=2, H=9, W=11, Cin=32, Cout=16)


def _lin_tensors():
    N, H, W, Cin, Cout = (LIN[k] for k in ('N', 'H', 'W', 'Cin', 'Cout'))
    return (randn(71, N, Cin, H, W).float(), (randn(72, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5).float(), randn(73, N, Cout, H, W).float())


def linear_cases():
    L = []
    N, H, W, Cin, Cout = (LIN[k] for k in ('N', 'H', 'W', 'Cin', 'Cout'))
    x, w, gy = _lin_tensors()
    pix = (1, 5, 4, 6)
    # ---- conv_backward_weight (3x3 stride 1): gw = sum over the pixels of gy x patches of x
    for where, t, idx in (('x', 0, pix), ('gy', 2, (1, 3, 4, 6))):
        for vname in ('nan', '+inf'):
            ts = [x, w, gy]
            ts[t] = plant(ts[t], idx, VALUES[vname])

            def run(dtype, laundered, ts=ts):
                wt = ts[1].to(dtype).clone().requires_grad_()
                bt = torch.zeros(Cout, dtype=dtype, requires_grad=True)
                gw, gb = torch.autograd.grad(F.conv2d(ts[0].to(dtype), wt, bt, 1, 1), (wt, bt), ts[2].to(dtype))
                return OrderedDict(gw=gw, gb=gb)
            L.append(Case('conv_backward_weight', '%s-%s' % (where, vname), dict(x=ts[0], gy=ts[2]), run,
                          OrderedDict(gw=_out(K=N * H * W), gb=_out(K=N * H * W)), meta=dict(no_grad=False)))
    # ---- conv_backward_input (3x3 stride 1): gx = conv(gy, w transposed and flipped)
    for where, t, idx in (('gy', 2, (1, 3, 4, 6)), ('w', 1, (3, 5, 1, 1))):
        for vname in ('nan', '+inf'):
            ts = [x, w, gy]
            ts[t] = plant(ts[t], idx, VALUES[vname])

            def run(dtype, laundered, ts=ts):
                return OrderedDict(gx=F.conv_transpose2d(ts[2].to(dtype), ts[1].to(dtype), padding=1))
            L.append(Case('conv_backward_input', '%s-%s' % (where, vname), dict(w=ts[1], gy=ts[2]), run,
                          OrderedDict(gx=_out(K=9 * Cout)), meta=dict(no_grad=True)))
    # ---- conv_s2_backward on the smallest shape of its own tests
    shape = BB.S2_SHAPES[0]
    sx, sw, sgy, _ = BB.s2_case(shape)
    for where, t, idx in (('x', 0, (1, 5, 2, 4)), ('w', 1, (3, 5, 1, 1)), ('gy', 2, (1, 3, 1, 2))):
        ts = [sx, sw, sgy]
        ts[t] = plant(ts[t], idx, NAN)

        def run(dtype, laundered, ts=ts):
            xt, wt = ts[0].to(dtype).clone().requires_grad_(), ts[1].to(dtype).clone().requires_grad_()
            gx, gw = torch.autograd.grad(F.conv2d(xt, wt, None, 2, 1), (xt, wt), ts[2].to(dtype))
            return OrderedDict(gx=gx, gw=gw)
        sN, sH, sW, sCin, sCout = shape
        L.append(Case('conv_s2_backward', where + '-nan', dict(x=ts[0], w=ts[1], gy=ts[2]), run,
                      OrderedDict(gx=_out(K=4 * sCout), gw=_out(K=sN * (sH // 2) * (sW // 2)))))
    # ---- upsample_add and its backward (f = 2, the pitched shape of _conv_fwd.UP_SHAPES is too small for rule (d): 9 x 11 here)
    C, f = 8, 2
    ux, uw, usk = randn(81, 2, C, 9, 11).float(), (randn(82, C, 1, 2 * f, 2 * f) * 0.5).float(), randn(83, 2, C, 9 * f, 11 * f).float()
    ugy = randn(84, 2, C, 9 * f, 11 * f).float()
    for where, t, idx in (('x', 0, (1, 5, 4, 6)), ('w', 1, (5, 0, 1, 2)), ('skip', 2, (1, 5, 8, 12))):
        for vname in ('nan', '+inf'):
            ts = [ux, uw, usk]
            ts[t] = plant(ts[t], idx, VALUES[vname])

            def run(dtype, laundered, ts=ts):
                return OrderedDict(y=NB.upsample_add(ts[0].to(dtype), ts[1].to(dtype), f, ts[2].to(dtype)))
            # a planted weight owns its channel: 1 / 8 of the map
            L.append(Case('upsample_add', '%s-%s' % (where, vname), dict(x=ts[0], w=ts[1], skip=ts[2], f=f), run,
                          OrderedDict(y=_out(K=4)), meta=dict(no_grad=True)))
    for where, t, idx in (('x', 0, (1, 5, 4, 6)), ('w', 1, (5, 0, 1, 2)), ('gy', 2, (1, 5, 8, 12))):
        ts = [ux, uw, ugy]
        ts[t] = plant(ts[t], idx, NAN)

        def run(dtype, laundered, ts=ts):
            gx, gw = NB.upsample_backward_formula(ts[0].to(dtype), ts[1].to(dtype), f, ts[2].to(dtype))
            return OrderedDict(gx=gx, gw=gw)
        L.append(Case('upsample_add_backward', where + '-nan', dict(x=ts[0], w=ts[1], gy=ts[2], f=f), run,
                      OrderedDict(gx=_out(K=4 * f * f), gw=_out(K=2 * 9 * 11)), meta=dict(no_grad=True)))
    # ---- slot_gather / slot_fold: exact copies and ordered sums; ind stays finite and in range
    feat = randn(91, 2, 16, 9, 11).float()
    ind = torch.tensor([[0, 50, 51, 98, 37, 37], [10, 98, 0, 62, 12, 13]], dtype=torch.int64)
    fp = plant(feat, (1, 5, 1, 1), NAN)                                # pixel 12 of image 1: slots 10, 12, 13 and 0 see it

    def gather_run(dtype, laundered):
        cols = F.unfold(fp.to(dtype), 3, padding=1).view(2, 16, 9, 99)           # [N, C, tap, pixel]
        rows = cols.permute(0, 3, 2, 1).reshape(2, 99, 9 * 16)                  # [N, pixel, tap * C + c]
        return OrderedDict(rows=rows.gather(1, ind.view(2, -1, 1).expand(2, ind.shape[1], 144)))
    L.append(Case('slot_gather', 'feat-nan', dict(feat=fp, ind=ind), gather_run, OrderedDict(rows=_out(equal=True)), meta=dict(no_grad=True)))
    patches = randn(92, 2, ind.shape[1], 144).float()
    pp = plant(patches, (1, 4, 4 * 16 + 5), NAN)                       # slot 4 of image 1, centre tap, channel 5 -> pixel 12
    gx0 = randn(93, 2, 16, 9, 11).float()

    def fold_run(dtype, laundered):
        out = []
        for n in range(2):
            c = torch.zeros(99, 144, dtype=dtype).index_add_(0, ind[n], pp[n].to(dtype))
            c = c.view(99, 9, 16).permute(2, 1, 0).reshape(1, 16 * 9, 99)
            out.append(F.fold(c, (9, 11), 3, padding=1))
        return OrderedDict(gx=gx0.to(dtype) + torch.cat(out, 0))
    L.append(Case('slot_fold', 'patches-nan', dict(patches=pp, ind=ind, gx=gx0), fold_run, OrderedDict(gx=_out(K=9 * 2)), meta=dict(no_grad=True)))
    # ---- dcn_v2 and its backward: x, weight and gy only.  Offsets and masks stay finite: a sample ADDRESS must never depend
    # on a planted value (DESIGN section 31 settles by reading what a non-finite offset would do)
    # Offsets stay below one pixel.  The oracle gathers a corner outside the map at a clamped index with weight 0, and 0 * NaN
    # = NaN then lands on a border pixel that the operation itself never touches (the kernels, like the reference's
    # col2im, skip such a corner).  With |offset| < 1 every sample of the planted interior pixel stays inside the map, and the
    # centre tap (the planted weight's) keeps a valid corner of positive weight at the very pixel a clamped corner would name.
    dshape = (2, 32, 16, 9, 11, 0.5)
    dx, doff, dmask, dw, dbias, dgy = DB.inputs(dshape)
    doff = doff.clamp(-0.9, 0.9)
    for where, t, idx in (('x', 0, (1, 5, 4, 6)), ('w', 3, (3, 5, 1, 1))):
        ts = [dx, doff, dmask, dw, dbias, dgy]
        ts[t] = plant(ts[t], idx, NAN)

        def run(dtype, laundered, ts=ts):
            from oracle import dcn_v2 as odcn
            v = [u.to(dtype) for u in ts[:5]]
            if dtype == torch.float64:
                v[1] = DB.effective_offsets(ts[1], 9, 11)
            return OrderedDict(y=odcn.dcn_v2_conv(*v))
        L.append(Case('dcn_v2', where + '-nan', dict(t=ts), run, OrderedDict(y=_out(K=9 * 32)), meta=dict(no_grad=True)))
    for where, t, idx in (('x', 0, (1, 5, 4, 6)), ('w', 3, (3, 5, 1, 1)), ('gy', 5, (1, 3, 4, 6))):
        ts = [dx, doff, dmask, dw, dbias, dgy]
        ts[t] = plant(ts[t], idx, NAN)

        def run(dtype, laundered, ts=ts):
            g = DB.oracle_grads(ts, dtype, effective=dtype == torch.float64)
            return OrderedDict((n, g[n]) for n in DB.NAMES)
        K = DB.terms(dshape)
        L.append(Case('dcn_v2_backward', where + '-nan', dict(t=ts), run,
                      OrderedDict((n, _out(K=K[n])) for n in DB.NAMES)))
    return L


# ---------------------------------------------------------------------------------------------------------------------
# the loss: tests/golden/losses_nonfinite.npz (tests/golden/make_loss_nonfinite_golden.py, from the reference's GenericLoss)

LOSS_B, LOSS_H, LOSS_W, LOSS_M, LOSS_CLASSES = 2, 8, 12, 8, 3
LOSS_HEADS = R.ALL_HEADS
P_OUT, P_NONE = 77, 90                    # the pixel only a masked-out slot names, and a pixel no slot names (image 0)


def loss_base():
    """(outputs, batch) of ``_loss_ref.make_batch`` with 5 and 3 objects; the last slot of image 0 (masked out) names pixel
    P_OUT alone, and no slot names P_NONE"""
    if 'loss' not in _cache:
        out, batch = R.make_batch(51, LOSS_B, LOSS_H, LOSS_W, LOSS_M, LOSS_HEADS, LOSS_CLASSES, valid=[5, 3])
        ind = batch['ind']
        for b in range(LOSS_B):
            for m in range(LOSS_M):
                while int(ind[b, m]) in (P_OUT, P_NONE) or (float(batch['mask'][b, m]) > 0 and int(ind[b, m]) == 0):
                    ind[b, m] = (int(ind[b, m]) + 7) % (LOSS_H * LOSS_W)
        ind[0, LOSS_M - 1] = P_OUT
        hm = batch['hm']
        for b, n in ((0, 5), (1, 3)):
            for m in range(n):
                hm[b, batch['cat'][b, m], ind[b, m] // LOSS_W, ind[b, m] % LOSS_W] = 1
        assert float(batch['mask'][0, LOSS_M - 1]) == 0
        _cache['loss'] = (out, batch)
    return _cache['loss']


def loss_plants():
    """[(name, head, flat index into the head's [B,C,H,W] logits, value name)]"""
    out, batch = loss_base()
    HW = LOSS_H * LOSS_W
    ind, cat = batch['ind'], batch['cat']
    pos = (0 * LOSS_CLASSES + int(cat[0, 1])) * HW + int(ind[0, 1])                 # the positive of slot 1, image 0
    taken = set(int(cat[0, m]) * HW + int(ind[0, m]) for m in range(5))
    neg = next(i for i in range(HW + 5, 3 * HW) if i not in taken)                  # a negative location of image 0
    slot_in = lambda C, c, m=2: (0 * C + c) * HW + int(ind[0, m])                   # a masked-in slot of image 0
    L = []
    for v in VALUES:
        L.append(('hm-negative-' + v, 'hm', neg, v))
        L.append(('hm-positive-' + v, 'hm', pos, v))
        L.append(('dep-' + v, 'dep', slot_in(1, 0), v))
    for v in ('nan', '+inf'):
        L.append(('reg-masked-in-' + v, 'reg', slot_in(2, 1), v))
        L.append(('reg-masked-out-' + v, 'reg', (0 * 2 + 1) * HW + P_OUT, v))
        L.append(('reg-unread-' + v, 'reg', (0 * 2 + 1) * HW + P_NONE, v))
        L.append(('rot-bin-' + v, 'rot', slot_in(8, 1), v))
        L.append(('nuscenes_att-' + v, 'nuscenes_att', slot_in(8, 3), v))
    # beyond the list of the issue: the sin residual of a slot whose first target bin is set (smooth-L1: its gradient is a sign)
    m = next(m for m in range(5) if int(batch['rotbin'][0, m, 0]) != 0)
    L.append(('rot-residual-nan', 'rot', slot_in(8, 2, m), 'nan'))
    return L


def loss_case(name):
    """(outputs with the plant, batch, head) of a plant of ``loss_plants``"""
    out, batch = loss_base()
    _, head, flat, v = next(p for p in loss_plants() if p[0] == name)
    out = dict(out)
    x = out[head].clone()
    x.view(-1)[flat] = VALUES[v]
    out[head] = x
    return out, batch, head


def load_loss_golden(golden_dir):
    """{case: dict(loss={head: float64 scalar}, grad=the planted head's logit gradient)} plus the inputs the file was made from"""
    z = np.load(os.path.join(golden_dir, 'losses_nonfinite.npz'))
    cases = OrderedDict()
    for name in str(z['cases'].reshape(-1)[0]).split(','):
        cases[name] = dict(loss={h: torch.from_numpy(z['%s/loss/%s' % (name, h)]) for h in LOSS_HEADS},
                           grad=torch.from_numpy(z['%s/grad' % name]))
    inputs = dict(out={h: torch.from_numpy(z['base/out/%s' % h]) for h in LOSS_HEADS},
                  batch={k[len('base/batch/'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('base/batch/')})
    return cases, inputs


# ---------------------------------------------------------------------------------------------------------------------

def _all_cases():
    return bn_cases() + stem_cases() + pool_cases() + conv_cases() + heads_cases() + linear_cases()


_cases = []


def cases():
    """every ``Case`` of the op tests, built once per process"""
    if not _cases:
        _cases.extend(_all_cases())
        assert len(set(c.id for c in _cases)) == len(_cases)
    return _cases


def case_ids(family=None):
    return [c.id for c in cases() if family is None or c.family == family]


def case(cid):
    return next(c for c in cases() if c.id == cid)
