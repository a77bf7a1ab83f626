"""CPU: what the non-finite GPU tests (tests/test_hip_nonfinite.py) rely on, checked without a GPU.

  * torch's own treatment of NaN and +-Inf in float64 -- the truth table the kernels are held to;
  * the reference's ``GenericLoss`` on non-finite logits (tests/golden/losses_nonfinite.npz, from
    tests/golden/make_loss_nonfinite_golden.py) and the float64 mirror tests/_loss_ref.py, which must reproduce every case before
    it may serve as the GPU tests' reference;
  * ``_nonfinite.compare`` notices laundering: fed the float64 reference with ``nan_to_num`` behind its ReLU, pool or clamp
    (what fmaxf / fminf did in the kernels) it rejects every case, and it rejects one extra NaN outside the spread;
  * the spread mask of a Winograd launch against the fp32 restatement ``_conv_fwd.winograd32`` fed the same NaN;
  * rule (d): every case leaves at least its floor of the output finite in the float64 reference alone."""
import os

import pytest
import torch
import torch.nn.functional as F

import _conv_fwd as CF
import _loss_ref as R
import _nonfinite as NF
from _nonfinite import INF, NAN, Rejected, compare

t64 = lambda *v: torch.tensor(v, dtype=torch.float64)


def _same(a, b):
    """equal, NaN matching NaN"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------------------------
# the truth table

def test_torch_relu_and_its_backward():
    assert _same(torch.relu(t64(NAN, INF, -INF, -1.0, 2.0)), t64(NAN, INF, 0.0, 0.0, 2.0))
    x = t64(NAN, 1.0, -1.0, 0.0).requires_grad_()
    torch.relu(x).backward(t64(2.0, 3.0, 4.0, 5.0))
    assert _same(x.grad, t64(2.0, 3.0, 0.0, 0.0))                      # threshold_backward passes gy where the input is NaN


def test_torch_max_pool_and_its_backward():
    for pos in range(4):
        x = torch.arange(16, dtype=torch.float64).view(1, 1, 4, 4).clone()
        x[0, 0, pos // 2, pos % 2] = NAN
        xt = x.clone().requires_grad_()
        y = F.max_pool2d(xt, 2, 2)
        assert torch.isnan(y[0, 0, 0, 0]) and int(torch.isnan(y).sum()) == 1
        y.backward(torch.ones_like(y))
        assert float(xt.grad[0, 0, pos // 2, pos % 2]) == 1.0 and float(xt.grad[0, 0, :2, :2].sum()) == 1.0   # the NaN takes the gradient
    x = t64(1.0, INF, -INF, 3.0).view(1, 1, 2, 2)
    assert float(F.max_pool2d(x, 2, 2)) == INF


def test_torch_clamp():
    assert _same(t64(NAN, INF, -INF).clamp(1e-4, 1 - 1e-4), t64(NAN, 1 - 1e-4, 1e-4))
    x = t64(NAN).requires_grad_()
    x.clamp(1e-4, 1 - 1e-4).backward(t64(1.0))
    assert float(x.grad) == 0.0                                         # clamp's backward masks a NaN out


@pytest.mark.parametrize('training', [True, False])
def test_torch_batch_norm(training):
    z = NF.bn_inputs()[0].double()
    C = z.shape[1]
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for v in (NAN, INF, -INF):
        zp = NF.plant(z, (1, 5, 4, 6), v)
        y = F.batch_norm(zp, rm.clone(), rv.clone(), None, None, training, 0.1, 1e-5)
        bad = ~torch.isfinite(y)
        if training:                                                    # the whole channel: mean and variance are non-finite
            assert bool(torch.isnan(y[:, 5]).all()) and int(bad.sum()) == y[:, 5].numel()
        else:                                                           # the element alone
            assert int(bad.sum()) == 1 and _same(y[1, 5, 4, 6], t64(v)[0])
    mean, var, invstd = NF.bn_stats_reference(NF.plant(z, (1, 5, 4, 6), INF))
    assert float(mean[5]) == INF and torch.isnan(var[5]) and torch.isnan(invstd[5]) and bool(torch.isfinite(mean[:5]).all())


def test_torch_conv2d():
    x, w = NF.randn(1, 2, 4, 9, 11), NF.randn(2, 6, 4, 3, 3)
    y = F.conv2d(NF.plant(x, (1, 2, 4, 6), NAN), w, None, 1, 1)
    want = torch.zeros(2, 6, 9, 11, dtype=torch.bool)
    want[1, :, 3:6, 5:8] = True                                         # the 3 x 3 footprint, every output channel
    assert torch.equal(torch.isnan(y), want)
    y = F.conv2d(x, NF.plant(w, (3, 2, 1, 1), NAN), None, 1, 1)
    want = torch.zeros(2, 6, 9, 11, dtype=torch.bool)
    want[:, 3] = True                                                   # the output channel, every pixel
    assert torch.equal(torch.isnan(y), want)
    y = F.conv2d(x, NF.plant(w, (3, 2, 1, 1), INF), None, 1, 1)
    assert torch.equal(y[:, 3], torch.where(x[:, 2] > 0, t64(INF), t64(-INF)).expand_as(y[:, 3]))


# ---------------------------------------------------------------------------------------------------------------------
# the loss

LOSS_NAMES = [p[0] for p in NF.loss_plants()]


def test_nonfinite_loss_golden_holds_the_cases(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, 'losses_nonfinite.npz')) < 256 * 1024
    cases, inputs = NF.load_loss_golden(golden_dir)
    assert list(cases) == LOSS_NAMES and len(LOSS_NAMES) == 20
    out, batch = NF.loss_base()
    for h in NF.LOSS_HEADS:
        assert torch.equal(inputs['out'][h], out[h])
    for k, v in batch.items():
        assert torch.equal(inputs['batch'][k], v), k
    # the slots the plants rely on
    ind, mask = batch['ind'], batch['mask']
    assert float(mask[0, NF.LOSS_M - 1]) == 0 and int(ind[0, NF.LOSS_M - 1]) == NF.P_OUT
    assert int((ind == NF.P_OUT).sum()) == 1 and int((ind == NF.P_NONE).sum()) == 0
    assert not bool(((ind == 0) & (mask > 0)).any())                    # (the masked-out slots name pixel 0)
    # what the reference does: a NaN logit on a focal head is a NaN loss, an infinite one a finite loss (the sigmoid saturates)
    for v in ('nan', '+inf', '-inf'):
        for where in ('hm-negative-', 'hm-positive-'):
            assert bool(torch.isnan(cases[where + v]['loss']['hm'])) == (v == 'nan')
            assert bool(torch.isfinite(cases[where + v]['grad']).all()) == (v != 'nan')
    assert torch.isnan(cases['reg-masked-out-nan']['loss']['reg']) and torch.isfinite(cases['reg-unread-nan']['loss']['reg'])
    assert float(cases['reg-masked-in-+inf']['loss']['reg']) == INF
    head_of = {p[0]: p[1] for p in NF.loss_plants()}
    for name, c in cases.items():                                       # the other heads never notice
        for h in NF.LOSS_HEADS:
            if h != head_of[name]:
                other = next(n for n in LOSS_NAMES if head_of[n] not in (h, head_of[name]))
                assert bool(torch.isfinite(c['loss'][h])) and float(c['loss'][h]) == float(cases[other]['loss'][h]), (name, h)


@pytest.mark.parametrize('name', LOSS_NAMES)
def test_mirror_reproduces_the_reference_on_nonfinite_logits(golden_dir, name):
    """non-finite positions match; finite values to 1e-12, as in tests/test_losses_cpu.py"""
    cases, _ = NF.load_loss_golden(golden_dir)
    out, batch, head = NF.loss_case(name)
    got = R.losses_and_grads(out, batch, NF.LOSS_HEADS, torch.float64)
    want = cases[name]
    for h in NF.LOSS_HEADS:
        a, b = got[h][0].double(), want['loss'][h].double()
        assert _same(a, b) or (bool(torch.isfinite(a)) and bool(torch.isfinite(b)) and abs(float(a) - float(b)) <= 1e-12 * abs(float(b))), (h, float(a), float(b))
    g, w = got[head][1], want['grad']
    assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(torch.isinf(g), torch.isinf(w)), (int(torch.isnan(g).sum()), int(torch.isnan(w).sum()))
    fin = torch.isfinite(w)
    assert float((g[fin] - w[fin]).abs().max()) <= 1e-12 * float(w[fin].abs().max())
    assert NF.finite_share(w) >= NF.FLOOR                               # rule (d) from the reference alone
    tot, _ = R.generic_loss([{h: out[h].double() for h in NF.LOSS_HEADS}],
                            {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}, NF.LOSS_HEADS,
                            R.Opt(NF.LOSS_HEADS).weights)
    assert bool(torch.isfinite(tot)) == all(bool(torch.isfinite(want['loss'][h])) for h in NF.LOSS_HEADS)


def test_compare_rejects_a_laundered_focal_clamp(golden_dir):
    """p = fmin(fmax(sigmoid(x), 1e-4), 1 - 1e-4) turned a NaN logit into p = 1e-4: a finite loss and a zero gradient"""
    cases, _ = NF.load_loss_golden(golden_dir)
    for name in ('hm-negative-nan', 'hm-positive-nan'):
        out, batch, head = NF.loss_case(name)
        x = out['hm'].double().requires_grad_()
        p = torch.where(torch.isnan(x), torch.full_like(x, 1e-4), torch.sigmoid(torch.nan_to_num(x)).clamp(1e-4, 1 - 1e-4))
        gt = batch['hm'].double()
        neg = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4).sum()
        pp = R.gather(p, batch['ind']).gather(2, batch['cat'].unsqueeze(2)).squeeze(2)
        loss = -((torch.log(pp) * (1 - pp) ** 2 * batch['mask'].double()).sum() + neg) / batch['mask'].sum()
        g, = torch.autograd.grad(loss, x)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
        with pytest.raises(Rejected) as e:
            compare(loss.reshape(1), cases[name]['loss']['hm'].reshape(1), 'equal', floor=0.0)
        assert e.value.rule == 'a'
        with pytest.raises(Rejected) as e:
            compare(g, cases[name]['grad'], 'equal')
        assert e.value.rule == 'a'


# ---------------------------------------------------------------------------------------------------------------------
# compare

def test_compare_rules():
    ref = NF.randn(7, 4, 50)
    ok = NF.project_bound(ref.float(), 1)
    assert compare(ref.float(), ref, ok)['finite'] == 1.0
    r = NF.plant(ref, (1, 3), NAN)
    compare(r.float(), r, ok)
    with pytest.raises(Rejected) as e:                                  # (a) a NaN turned finite
        compare(ref.float(), r, ok)
    assert e.value.rule == 'a'
    for v, w in ((INF, -INF), (INF, NAN), (-INF, 3.0)):                  # (a) the same infinity, nothing else
        with pytest.raises(Rejected) as e:
            compare(NF.plant(ref, (1, 3), w).float(), NF.plant(ref, (1, 3), v), ok)
        assert e.value.rule == 'a'
    compare(NF.plant(ref, (1, 3), INF).float(), NF.plant(ref, (1, 3), INF), ok)
    with pytest.raises(Rejected) as e:                                  # (b) one extra NaN outside the spread
        compare(NF.plant(r, (2, 9), NAN).float(), r, ok)
    assert e.value.rule == 'b'
    spread = torch.zeros(4, 50, dtype=torch.bool)
    spread[2, 9] = True
    compare(NF.plant(r, (2, 9), NAN).float(), r, ok, spread)            # ... inside it: allowed
    with pytest.raises(Rejected) as e:
        compare(NF.plant(r, (2, 10), NAN).float(), r, ok, spread)
    assert e.value.rule == 'b'
    with pytest.raises(Rejected) as e:                                  # (c) the finite rest is held to the bound
        compare(NF.plant(r, (0, 0), float(r[0, 0]) + 1e-2).float(), r, ok)
    assert e.value.rule == 'c'
    with pytest.raises(Rejected) as e:
        compare(NF.plant(r, (0, 0), float(r[0, 0]) + 1e-6).float(), r, 'equal')
    assert e.value.rule == 'c'
    wide = r.clone()
    wide[:, :13] = NAN                                                  # (d) 26 % non-finite: the test would hide failures
    with pytest.raises(Rejected) as e:
        compare(wide.float(), wide, ok)
    assert e.value.rule == 'd'
    compare(wide.float(), wide, ok, floor=0.7)


CASE_IDS = NF.case_ids()


@pytest.mark.parametrize('cid', CASE_IDS)
def test_every_case_keeps_its_floor_in_the_reference_alone(cid):
    """rule (d), and that the plant is where the test says: the reference of every case holds a non-finite element somewhere
    or routes a finite value differently than without the plant"""
    c = NF.case(cid)
    r64 = c.reference()
    for k, spec in c.outputs.items():
        assert NF.finite_share(r64[k]) >= spec['floor'], (cid, k, NF.finite_share(r64[k]))
        if spec.get('spread') is not None:
            assert NF.finite_share(r64[k]) - float(spec['spread'].expand_as(r64[k]).double().mean()) >= spec['floor'] - 1e-12, (cid, k)
    c.check(r64)                                                        # the float64 reference passes its own check


@pytest.mark.parametrize('cid', [c.id for c in NF.cases() if c.launders])
def test_compare_rejects_the_laundering_emulation(cid):
    c = NF.case(cid)
    r64, old = c.reference(), c.reference(torch.float64, laundered=True)
    if all(bool(torch.isfinite(v).all()) for v in r64.values()):
        # -Inf behind a ReLU is 0 in torch as well: nothing reaches the output, and the emulation is right about it
        assert c.name.endswith('inf') and all(torch.equal(old[k], r64[k]) for k in c.outputs)
        return
    with pytest.raises(Rejected) as e:
        c.check(old)
    assert e.value.rule in ('a', 'c'), e.value
    print('%s: %s' % (cid, e.value))


def test_the_cases_cover_the_issue():
    fams = set(c.family for c in NF.cases())
    assert fams == {'bn_act_apply', 'bn_act_backward', 'stem_bn_relu_sum', 'stem_conv_backward', 'maxpool2x2', 'maxpool2x2_backward',
                    'conv2d_relu', 'conv2d_pool', 'heads_backward', 'conv_backward_weight', 'conv_backward_input', 'conv_s2_backward',
                    'upsample_add', 'upsample_add_backward', 'slot_gather', 'slot_fold', 'dcn_v2', 'dcn_v2_backward'}
    ids = set(CASE_IDS)
    for fam in NF.CONV_BASES:
        for where in ('x', 'w', 'shift'):
            assert 'conv2d_relu-%s-%s-nan' % (fam, where) in ids
    for pos in range(4):
        assert 'maxpool2x2-pos%d-nan' % pos in ids
    plans = {f: CF.plan_of(NF.conv_case_of(f)) for f in NF.CONV_BASES}
    assert [plans[f]['family'] for f in ('row', 'ksplit', 'wino')] == ['row', 'ksplit', 'wino'] and plans['splitk']['splits'] > 1
    assert all(p['splits'] == 1 for f, p in plans.items() if f != 'splitk')
    for f, name in NF.CONV_POOL_BASES.items():
        assert CF.plan_of(CF.CASE[name])['family'] == f and CF.CASE[name].pool
    # no case plants an offset, a mask or an index: an address never depends on a planted value
    for c in NF.cases():
        if c.family.startswith('dcn'):
            t = c.inputs['t']
            assert bool(torch.isfinite(t[1]).all()) and bool(torch.isfinite(t[2]).all())
        if c.family.startswith('slot'):
            assert c.inputs['ind'].dtype == torch.int64


# ---------------------------------------------------------------------------------------------------------------------
# the Winograd spread

@pytest.mark.parametrize('cid', [c.id for c in NF.cases() if c.meta.get('wino')])
def test_winograd_spread_holds_the_fp32_restatement(cid):
    """``winograd32`` fed the same plant: its non-finite set lies inside reference u spread; for a planted pixel the spread is
    the direct 3 x 3 footprint dilated by the overlap of the 4 x 4 input tiles, and the restatement fills it"""
    c = NF.case(cid)
    case, d = c.inputs['case'], c.inputs['d']
    r64 = c.reference()['y']
    y32 = c.run(torch.float32, False, conv=CF.winograd32)['y']
    spread = c.outputs['y']['spread'].expand_as(r64)
    bad32, bad64 = ~torch.isfinite(y32), ~torch.isfinite(r64)
    assert not bool((bad32 & ~(bad64 | spread)).any())
    c.check(dict(y=y32))
    if c.meta['where'] == 'x':
        n, y, x = c.meta['pixel']
        direct = NF.direct_footprint(case, n, y, x).expand_as(r64)
        assert torch.equal(bad64, direct) and bool((direct & spread).eq(direct).all())
        # dilated: rows 2 * ((y - 1) // 2) .. the end of the tile that starts at y + 1 rounded down to even, columns likewise
        ys, xs = spread[n, 0].any(1).nonzero().view(-1), spread[n, 0].any(0).nonzero().view(-1)
        assert int(ys.min()) == max(0, 2 * ((y - 1) // 2)) and int(ys.max()) == min(case.H - 1, 2 * ((y + 1) // 2) + 1)
        assert int(xs.min()) == max(0, 2 * ((x - 1) // 2)) and int(xs.max()) == min(case.W - 1, 2 * ((x + 1) // 2) + 1)
        assert torch.equal(bad32 & ~bad64, spread & ~bad64)              # the restatement fills the spread, no more and no less
