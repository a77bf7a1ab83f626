"""Checkpoint-like DLA-34 weights for the whole-model tests (tests/test_ckpt_weights_cpu.py, tests/test_hip_ckpt_weights.py):
the generator, a run of the oracle that keeps every compared tensor, the conditions the weights have to meet, the error
measure and bound, and CPU mutants of the float32 oracle.  No GPU, no ctypes.

``weights.make_synthetic_state_dict`` draws one benign family (BatchNorm gamma and variance in [0.5, 1.5], means ~ 0.1,
offsets below a pixel).  ``checkpoint_like_state_dict`` starts from it and redraws, seeded and on the CPU:

  BN variance    running_var log-uniform over 1e-6 .. 1e2
  BN scale       gamma = s * sqrt(var + eps): the folded scale s has |s| in [0.5, 1.5] * GAIN; per layer 5 % of the channels
                 (at least one) have s = 0 exactly, 15 % (at least one) s < 0
  BN mean        running_mean = m * sqrt(var), m ~ N(0, MEAN_SIGMAS) cut at +-4: up to 40 against activations of O(1).  beta
                 takes back COMPENSATE of mean * s, as the beta of a trained layer does whose input really has that mean: the
                 shift beta - mean * scale is a difference of two large terms (up to ~50 each) and stays O(1)
  dead channels  max(1, C // 32) all-zero filters in every trunk conv and every DeformConv's main conv, their running_var
                 1e-8 .. 1e-6 (invstd ~ 1 / sqrt(eps): eps decides their output), mean and gamma drawn like the others': a
                 constant channel, batch variance 0 in training mode
  DCN offsets    offset weights ~ N(0, .) and biases rescaled layer by layer, on one float64 pass of the oracle over a fixed
                 1 x 64 x 96 input, to a standard deviation of OFFSET_PX pixels at every DeformConv; mask biases of tap 2 and
                 tap 6 at +10 and -10 (masks pinned at 1 and 0)
  heads          hm / hm_hp output layers centred over their (positive) inputs, x HM_GAIN, bias HM_BIAS: scores spread over
                 (0, 1) instead of sitting at 0.01

The trunk does not depend on the head set (the synthetic generator draws the heads last), so the calibration pass runs once
per seed and process."""
import contextlib
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from _dcn_bwd import err

BN_EPS = 1e-5
GAIN = 1.0
MEAN_SIGMAS = 1.5
COMPENSATE = 0.9
OFFSET_PX = 2.0
OFFSET_BIAS_SHARE = 0.3            # of the offset variance, the share the bias carries
HM_GAIN, HM_BIAS = 4.0, -0.5
ZERO_SHARE, NEG_SHARE = 0.05, 0.15
K_LONGEST = 4608                   # 512 input channels x 9 taps: the longest contraction of the model
M = 10.0                           # 4 (_dcn_bwd.bound) x 2.5 (Winograd 5e-4 against direct 2e-4 in tests/test_hip_ops.py)

SHAPES = [(1, 64, 96), (2, 64, 64), (1, 128, 160)]
SEEDS = (317, 5200)                # every seed the GPU file uses
FAMILIES = ('base', 'dla_up', 'ida_up')
LEVEL_NAMES = ['level%d' % i for i in range(6)]


def bound(e32):
    """the whole-model bar: M x what float32 torch does on the same data, never below M x 2^-23 sqrt(K), never above 1e-3"""
    return min(1e-3, M * max(e32, 2.0 ** -23 * math.sqrt(K_LONGEST)))


def head_sets():
    """'mot4' is the head set of tests/test_hip_dlaseg.py"""
    from centertrack_amd import weights as W
    return {'mot': W.MOT_HEADS, 'nusc': W.NUSC_HEADS, 'pose': W.POSE_HEADS, 'coco': W.COCO_HEADS, 'kitti': W.KITTI_HEADS,
            'mot4': OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2)])}


# ---------------------------------------------------------------------------------------------------------------------
# the generator

def _bn_prefixes(sd):
    return [k[:-len('.running_var')] for k in sd if k.endswith('.running_var')]


def _conv_before(sd, p):
    """the key of the conv whose output BatchNorm ``p`` normalises"""
    if p.endswith('.actf.0'):
        return p[:-len('.actf.0')] + '.conv.weight'
    for a, b in (('.bn1', '.conv1.weight'), ('.bn2', '.conv2.weight'), ('.root.bn', '.root.conv.weight'), ('.1', '.0.weight')):
        if p.endswith(a):
            return p[:-len(a)] + b
    raise KeyError(p)


def dcn_prefixes(sd):
    return [k[:-len('.conv.conv_offset_mask.weight')] for k in sd if k.endswith('.conv.conv_offset_mask.weight')]


_trunk_cache = {}


def _redraw_trunk(sd, seed, training):
    g = torch.Generator().manual_seed(1000003 * seed + 17)

    def rand(*shape):
        return torch.rand(shape, generator=g, dtype=torch.float64)

    def randn(*shape):
        return torch.randn(shape, generator=g, dtype=torch.float64)

    for p in _bn_prefixes(sd):
        C = sd[p + '.running_var'].numel()
        var = 10.0 ** (rand(C) * 8.0 - 6.0)
        s = (rand(C) + 0.5) * GAIN
        order = torch.randperm(C, generator=g)
        nz, nn, nd = max(1, round(ZERO_SHARE * C)), max(1, round(NEG_SHARE * C)), max(1, C // 32)
        zero, neg, dead = order[:nz], order[nz:nz + nn], order[nz + nn:nz + nn + nd]
        s[neg] = -s[neg]
        s[zero] = 0.0
        mean = randn(C).mul(MEAN_SIGMAS).clamp(-4.0, 4.0) * var.sqrt()
        # the dead channels: an all-zero filter, the statistics of a channel that never moved
        var[dead] = 10.0 ** (rand(nd) * 2.0 - 8.0)
        mean[dead] = randn(nd).mul(MEAN_SIGMAS).clamp(-4.0, 4.0) * var[dead].sqrt()
        wkey = _conv_before(sd, p)
        w = sd[wkey].clone()
        w[dead] = 0.0
        sd[wkey] = w
        gamma = s * (var + BN_EPS).sqrt()
        beta = COMPENSATE * mean * s + randn(C) * 0.2
        sd[p + '.weight'] = gamma.float()
        sd[p + '.bias'] = beta.float()
        sd[p + '.running_mean'] = mean.float()
        sd[p + '.running_var'] = var.float()
    for p in dcn_prefixes(sd):
        b = sd[p + '.conv.conv_offset_mask.bias'].clone()
        b[18 + 2], b[18 + 6] = 10.0, -10.0
        sd[p + '.conv.conv_offset_mask.bias'] = b
    _calibrate_offsets(sd, seed, training)


def _calibrate_offsets(sd, seed, training):
    """one float64 pass over a fixed input: each DeformConv's 18 offset rows are rescaled, before the layer runs, so that its
    offsets have a standard deviation of OFFSET_PX pixels, OFFSET_BIAS_SHARE of the variance from the bias.  ``training``: the
    pass normalises with batch statistics (a 2 x 64 x 64 input), as a training step does -- there the activations have the
    scale of gamma, four decades wide, not that of the folded scale, and offsets calibrated on the running statistics would
    throw every tap of the small maps out of the image"""
    from centertrack_amd import weights as W
    from oracle import dla34
    g = torch.Generator().manual_seed(1000003 * seed + 29)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    real = dla34._deform_conv

    def deform(x, sdd, p):
        wk, bk = p + '.conv.conv_offset_mask.weight', p + '.conv.conv_offset_mask.bias'
        raw = F.conv2d(x, sdd[wk][:18], None, padding=1)
        k = OFFSET_PX * math.sqrt(1.0 - OFFSET_BIAS_SHARE) / max(float(raw.std()), 1e-12)
        w = sdd[wk].clone()
        w[:18] *= k
        b = sdd[bk].clone()
        b[:18] = torch.randn(18, generator=g, dtype=torch.float64) * (OFFSET_PX * math.sqrt(OFFSET_BIAS_SHARE))
        sd[wk], sd[bk] = w.float(), b.float()
        sdd[wk], sdd[bk] = sd[wk].double(), sd[bk].double()
        return real(x, sdd, p)
    real_bn = dla34._bn

    def batch_bn(x, sdd, p):
        return F.batch_norm(x, None, None, sdd[p + '.weight'], sdd[p + '.bias'], True, 0.1, BN_EPS)
    x, pre, hm = W.synthetic_inputs(*((2, 64, 64) if training else (1, 64, 96)), seed=seed + 7, dtype=torch.float64)
    dla34._deform_conv = deform
    if training:
        dla34._bn = batch_bn
    try:
        with torch.no_grad():
            dla34.dla_seg_features(x, pre, hm, sd64)
    finally:
        dla34._deform_conv, dla34._bn = real, real_bn


def checkpoint_like_state_dict(heads, seed, head_conv=256, training=False):
    """a state dict with the keys and shapes of ``make_synthetic_state_dict(heads, seed, head_conv=head_conv)`` and the
    distribution of this module's docstring; CPU float32, finite, a function of its arguments alone.  ``training``: the
    same draw with the offsets calibrated under batch statistics, for the tests that run the modules in training mode"""
    from centertrack_amd import weights as W
    sd = W.make_synthetic_state_dict(heads, seed=seed, head_conv=head_conv)
    trunk = [k for k in sd if k.split('.')[0] in FAMILIES]
    if (seed, training) not in _trunk_cache:
        t = OrderedDict((k, sd[k].clone()) for k in trunk)
        _redraw_trunk(t, seed, training)
        _trunk_cache[seed, training] = t
    for k in trunk:
        sd[k] = _trunk_cache[seed, training][k].clone()
    for h in heads:
        if h in ('hm', 'hm_hp'):
            w = sd[h + '.2.weight'].double()
            sd[h + '.2.weight'] = ((w - w.mean(1, keepdim=True)) * HM_GAIN).float()
            sd[h + '.2.bias'] = torch.full_like(sd[h + '.2.bias'], HM_BIAS)
    return sd


def backbone_module_params(name, seed):
    """the generator's parameters under the keys of a module of ``_backbone_bwd.MODULES``: 'dla34' is ``base.*``, 'tree-2'
    (a two-level Tree 64 -> 128 with ``level_root``) is ``base.level3.*``"""
    sd = checkpoint_like_state_dict(head_sets()['mot4'], seed, training=True)
    prefix = {'dla34': 'base.', 'tree-2': 'base.level3.'}[name]
    return OrderedDict((k[len(prefix):], v.clone()) for k, v in sd.items() if k.startswith(prefix))


def idaup_module_params(seed, inputs):
    """``ida_up.*`` of the generator under the keys of the IDAUp of ``_neck_bwd.IDA`` (64 <- [64, 128, 256], factors 1, 2, 4).
    The module test feeds it N(0, 1) maps, not the trunk's, so the 18 offset rows of each DeformConv are rescaled once more,
    node by node in call order, to OFFSET_PX on those inputs: free float64 training-mode runs of ``_neck_bwd.ida``"""
    import _neck_bwd as NB
    full = checkpoint_like_state_dict(head_sets()['mot4'], seed, training=True)
    sd = OrderedDict((k[len('ida_up.'):], v.clone()) for k, v in full.items() if k.startswith('ida_up.'))
    for prefix in ('proj_1.', 'node_1.', 'proj_2.', 'node_2.'):
        tr = NB.Trace()
        with torch.no_grad():
            NB.ida([x.double() for x in inputs], NB.cast(sd, torch.float64), '', 0, len(inputs), True, tr)
        k = OFFSET_PX / float(tr.coords[prefix].std())
        for key in (prefix + 'conv.conv_offset_mask.weight', prefix + 'conv.conv_offset_mask.bias'):
            v = sd[key].double()
            v[:18] *= k
            sd[key] = v.float()
    return sd


def zeroed(sd):
    """what the generator set to zero: {BN prefix: (indices of gamma == 0, indices of all-zero filters)}"""
    out = OrderedDict()
    for p in _bn_prefixes(sd):
        w = sd[_conv_before(sd, p)]
        out[p] = ((sd[p + '.weight'] == 0).nonzero().flatten().tolist(),
                  (w.flatten(1).abs().amax(1) == 0).nonzero().flatten().tolist())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a run of the oracle that keeps every compared tensor

class Mutant(object):
    """a wrong float32 oracle: ``kind`` applied at the one layer ``p`` (channel / tap ``idx``)"""

    def __init__(self, kind, p, idx=None):
        self.kind, self.p, self.idx = kind, p, idx

    def __repr__(self):
        return '%s @ %s%s' % (self.kind, self.p, '' if self.idx is None else '[%d]' % self.idx)


@contextlib.contextmanager
def _patched(record, mutant):
    from oracle import dcn_v2 as odcn, dla34
    real_bn, real_deform = dla34._bn, dla34._deform_conv

    def bn(x, sd, p):
        if mutant is not None and mutant.p == p and mutant.kind == 'abs_gamma':
            sd = dict(sd)
            sd[p + '.weight'] = sd[p + '.weight'].abs()
        if mutant is not None and mutant.p == p and mutant.kind == 'zero_gamma_1e-3':
            sd = dict(sd)
            sd[p + '.weight'] = sd[p + '.weight'].clone()
            assert float(sd[p + '.weight'][mutant.idx]) == 0.0
            sd[p + '.weight'][mutant.idx] = 1e-3
        y = real_bn(x, sd, p)
        if mutant is not None and mutant.p == p and mutant.kind == 'epilogue_1e-4':
            y = y * (1.0 + 1e-4)
        if mutant is not None and mutant.p == p and mutant.kind == 'no_eps':
            c = mutant.idx
            y = y.clone()
            y[:, c] = (x[:, c] - sd[p + '.running_mean'][c]) / sd[p + '.running_var'][c].sqrt() * sd[p + '.weight'][c] \
                + sd[p + '.bias'][c]
        return y

    def deform(x, sd, p):
        w_off, b_off = sd[p + '.conv.conv_offset_mask.weight'], sd[p + '.conv.conv_offset_mask.bias']
        om = F.conv2d(x, w_off, b_off, padding=1)
        offset, mask = om[:, :18], torch.sigmoid(om[:, 18:])
        H, Wd = x.shape[2], x.shape[3]
        from _dcn_bwd import tap_bases
        pos = tap_bases(H, Wd, x.dtype).unsqueeze(0) + offset
        if record is not None:
            py, px = pos[:, 0::2], pos[:, 1::2]
            outside = (py <= -1) | (px <= -1) | (py >= H) | (px >= Wd)
            record['offsets'][p] = dict(std=float(offset.double().std()), max=float(offset.abs().max()),
                                        outside=float(outside.double().mean()),
                                        pinned=float(((mask < 1e-3) | (mask > 1 - 1e-3)).double().mean()))
            record['tensors'][p + '.in'] = x
        if mutant is not None and mutant.p == p and mutant.kind == 'clamp_taps':
            lim = torch.tensor([H - 1.0, Wd - 1.0] * 9, dtype=x.dtype).view(1, 18, 1, 1)
            offset = torch.minimum(pos.clamp(min=0.0), lim) - tap_bases(H, Wd, x.dtype).unsqueeze(0)
        if mutant is not None and mutant.p == p and mutant.kind == 'no_sigmoid':
            mask = mask.clone()
            mask[:, mutant.idx] = om[:, 18 + mutant.idx]
        y = odcn.dcn_v2_conv(x, offset, mask, sd[p + '.conv.weight'], sd[p + '.conv.bias'], 1, 1, 1, 1)
        y = F.relu(bn(y, sd, p + '.actf.0'))
        if record is not None:
            record['tensors'][p + '.out'] = y
        return y
    dla34._bn, dla34._deform_conv = bn, deform
    try:
        yield
    finally:
        dla34._bn, dla34._deform_conv = real_bn, real_deform


def dcn_result_names(sd):
    """{name of DLASegHIP's plan['dcn_layers']: the oracle tensor that view holds}: a ``node`` holds its own output, a
    ``proj`` the up-sampled sum that is the input of its node"""
    out = OrderedDict()
    for p in dcn_prefixes(sd):
        out[p] = p + '.out' if '.node_' in p else p.replace('.proj_', '.node_') + '.in'
    return out


def trunk_run(sd, inputs, dtype, mutant=None):
    """the oracle's trunk in ``dtype`` -> (tensors, offsets): tensors = {level0 .. level5, every DeformConv's '<prefix>.in' /
    '.out', 'feature'}; offsets = {DeformConv prefix: std, max, share outside the map, share of pinned masks}"""
    from oracle import dla34
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.split('.')[0] in FAMILIES}
    x, pre, hm = (t.to(dtype) for t in inputs)
    record = {'tensors': OrderedDict(), 'offsets': OrderedDict()}
    with torch.no_grad(), _patched(record, mutant):
        base = dla34.dla_base(x, pre, hm, sdd)
        for n, t in zip(LEVEL_NAMES, base):
            record['tensors'][n] = t
        ups = dla34.dla_up(base, sdd)
        z = [ups[0].clone(), ups[1].clone(), ups[2].clone()]
        dla34._ida_up(z, 0, 3, sdd, 'ida_up', [1, 2, 4])
        record['tensors']['feature'] = z[-1]
    return record['tensors'], record['offsets']


def heads_run(feat, sd, heads, dtype):
    from oracle import dla34
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.split('.')[0] in heads}
    with torch.no_grad():
        return OrderedDict(('head ' + k, v) for k, v in dla34.apply_heads(feat.to(dtype), heads, sdd).items())


def training_offsets(sd, inputs):
    """the offsets of a float64 pass that normalises with batch statistics, as the first training step does"""
    from oracle import dla34
    real = dla34._bn
    dla34._bn = lambda x, sdd, p: F.batch_norm(x, None, None, sdd[p + '.weight'], sdd[p + '.bias'], True, 0.1, BN_EPS)
    try:
        return trunk_run(sd, inputs, torch.float64)[1]
    finally:
        dla34._bn = real


def oracle_run(sd, inputs, heads, dtype, mutant=None):
    """trunk and heads: (tensors with 'head <name>' added, offsets)"""
    tensors, offsets = trunk_run(sd, inputs, dtype, mutant)
    tensors.update(heads_run(tensors['feature'], sd, heads, dtype))
    return tensors, offsets


_trunk_truth, _truth_cache = {}, {}


def make_state_dict(family, heads, seed, head_conv=256):
    """``family`` is 'ckpt' or 'benign:<off_std>'"""
    from centertrack_amd import weights as W
    if family == 'ckpt':
        return checkpoint_like_state_dict(heads, seed, head_conv)
    return W.make_synthetic_state_dict(heads, seed=seed, off_std=float(family.split(':')[1]), head_conv=head_conv)


def truth(family, heads_name, shape, seed, head_conv=256):
    """(sd, inputs, float64 tensors, float32 tensors, offsets of the float64 run, e32 per tensor) of one case.  The trunk does
    not depend on the head set: it runs once per (family, shape, seed) and process, the heads once per case."""
    from centertrack_amd import weights as W
    key = (family, heads_name, shape, seed, head_conv)
    if key not in _truth_cache:
        heads = head_sets()[heads_name]
        sd = make_state_dict(family, heads, seed, head_conv)
        inputs = W.synthetic_inputs(*shape, seed=seed)
        tk = (family, shape, seed)
        if tk not in _trunk_truth:
            _trunk_truth[tk] = trunk_run(sd, inputs, torch.float64) + trunk_run(sd, inputs, torch.float32)[:1]
        t64, offsets, t32 = _trunk_truth[tk]
        t64, t32 = OrderedDict(t64), OrderedDict(t32)
        t64.update(heads_run(t64['feature'], sd, heads, torch.float64))
        t32.update(heads_run(t32['feature'], sd, heads, torch.float32))
        e32 = OrderedDict((k, err(t32[k], t64[k])) for k in t64)
        _truth_cache[key] = (sd, inputs, t64, t32, offsets, e32)
    return _truth_cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# the conditions

E32_CAP = 1e-4


def conditions(sd, t64, offsets, e32):
    """every condition as (name, value, lower, upper); ``failed`` picks those out of range"""
    rows = [('finite', float(all(bool(torch.isfinite(t).all()) for t in t64.values())
                             and all(bool(torch.isfinite(v).all()) for v in sd.values())), 1.0, 1.0)]
    for n in LEVEL_NAMES:
        rows.append(('positive share ' + n, float((t64[n] > 0).double().mean()), 0.2, 0.8))
        rows.append(('max ' + n, float(t64[n].abs().max()), 0.0, 50.0))
    for p, o in offsets.items():
        rows.append(('positive share ' + p, float((t64[p + '.out'] > 0).double().mean()), 0.2, 0.8))
        rows.append(('max ' + p, float(t64[p + '.out'].abs().max()), 0.0, 50.0))
        rows.append(('offset std ' + p, o['std'], 1.0, 4.0))
        rows.append(('offset max ' + p, o['max'], 0.0, 12.0))
        rows.append(('outside share ' + p, o['outside'], 0.01, 1.0))
    z = zeroed(sd)
    for fam in FAMILIES:
        ps = [p for p in z if p.startswith(fam + '.')]
        rows.append(('negative gamma in every layer of ' + fam, float(all(bool((sd[p + '.weight'] < 0).any()) for p in ps)), 1.0, 1.0))
        rows.append(('zero gamma in every layer of ' + fam, float(all(len(z[p][0]) > 0 for p in ps)), 1.0, 1.0))
        rows.append(('dead filter in every layer of ' + fam, float(all(len(z[p][1]) > 0 for p in ps)), 1.0, 1.0))
        rows.append(('variance below 1e-5 in ' + fam, float(min(float(sd[p + '.running_var'].min()) for p in ps)), 0.0, 1e-5))
        rows.append(('variance decades in ' + fam, min(float(torch.log10(sd[p + '.running_var'].max() / sd[p + '.running_var'].min()))
                                                       for p in ps), 4.0, 20.0))
        rows.append(('largest |mean| / std in ' + fam, max(float((sd[p + '.running_mean'].abs() / sd[p + '.running_var'].sqrt()).max())
                                                           for p in ps), 2.0, 4.001))
    for fam in FAMILIES[1:]:
        ps = [p for p in offsets if p.startswith(fam + '.')]
        rows.append(('pinned masks in ' + fam, min(offsets[p]['pinned'] for p in ps), 0.1, 1.0))
    rows.append(('e32 feature', e32['feature'], 0.0, E32_CAP))
    return rows


def failed(rows):
    return ['%s = %.4g not in [%g, %g]' % r for r in rows if not r[2] <= r[1] <= r[3]]


def summary(rows):
    """the measured values of one case in one line (DESIGN.md's table)"""
    def rng(prefix):
        v = [r[1] for r in rows if r[0].startswith(prefix)]
        return '%.3g .. %.3g' % (min(v), max(v))
    return 'positive share %s; max %s; offset std %s px; offset max %s px; outside %s; e32 %.2e' % (
        rng('positive share'), rng('max '), rng('offset std'), rng('offset max'), rng('outside share'),
        [r[1] for r in rows if r[0] == 'e32 feature'][0])


# ---------------------------------------------------------------------------------------------------------------------
# the mutants

def mutants(sd):
    """the wrong oracles of tests/test_ckpt_weights_cpu.py, each at one layer, chosen from the state dict alone (the sixth is
    the error the whole-model bar was blind to by construction: 1e-4 of the value in the epilogue of the last layer): the BN
    mutants at ``base.level2.tree1.bn1`` (64 channels at stride 4, early enough that nothing after it is spared), the
    zero-gamma mutant at that layer's zero channel of the smallest variance (gamma 1e-3 is a scale of 1e-3 / sqrt(var + eps)),
    the eps mutant at its dead channel, the DCN mutants at the last node, whose output is the feature map"""
    p = 'base.level2.tree1.bn1'
    z, dead = zeroed(sd)[p]
    zc = min(z, key=lambda c: float(sd[p + '.running_var'][c])) if z else None
    return [Mutant('abs_gamma', p), Mutant('zero_gamma_1e-3', p, zc), Mutant('no_eps', p, dead[0] if dead else None),
            Mutant('clamp_taps', 'ida_up.node_2'), Mutant('no_sigmoid', 'ida_up.node_2', 4),
            Mutant('epilogue_1e-4', 'ida_up.node_2.actf.0')]


def old_bar_passes(got, want):
    """the bar of test_forward_matches_oracle: atol = rtol = 1e-3 against the float32 oracle"""
    return bool(((got - want).abs() <= 1e-3 + 1e-3 * want.abs()).all())
