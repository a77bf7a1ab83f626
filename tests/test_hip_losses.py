"""GPU: the fused training loss (centertrack_amd.losses on csrc/loss.hip) against the reference's own float64 numbers
(tests/golden/losses.npz) and against the float64 mirror tests/_loss_ref.py, which tests/test_losses_cpu.py pins to them.

The error measure and the bound are those of the DCNv2 backward tests (tests/_dcn_bwd.py):
``err <= min(1e-3, 4 * max(e32, 2^-23 * sqrt(K)))`` with e32 the float32 reference's own error against float64 and K the
number of summed terms: B*C*H*W for a focal loss, B*M*C for a slot loss, 1 for a gradient element.  A loss error is
relative, a gradient error is the largest element error over the largest float64 magnitude."""
import ctypes

import pytest
import torch

import _loss_ref as R
from _loss_ref import CASES, load_case

pytestmark = pytest.mark.gpu

POSE = ('hm', 'hm_hp', 'hps', 'hp_offset', 'reg', 'wh')
EDGE = 9.2102            # |logit| at which clamp(sigmoid(x), 1e-4, 1 - 1e-4) starts to act


def _assert_away_from_the_clamp(out):
    """float32 and float64 must agree on which side of the clamp a random logit falls"""
    for h in ('hm', 'hm_hp'):
        if h in out:
            assert float((out[h].abs() - EDGE).abs().min()) >= 1e-3, h


def _to(d, device):
    return {k: v.to(device) for k, v in d.items()}


def _slots(head, batch):
    return (batch['hp_ind'] if head in ('hm_hp', 'hp_offset') else batch['ind']).shape[1]


def hip_losses_and_grads(out, batch, heads, device):
    """{head: (loss, d loss / d logits)} through ONE fused forward and ONE fused backward"""
    from centertrack_amd import losses
    xs = {h: out[h].to(device).requires_grad_() for h in heads}
    b = _to(batch, device)
    vec = losses.fused_losses([losses.GenericLoss._spec(h, xs, b) for h in heads])
    grads = torch.autograd.grad(vec, [xs[h] for h in heads], torch.ones_like(vec))
    return {h: (vec[i].detach(), g) for i, (h, g) in enumerate(zip(heads, grads))}


def hip_tot(out, batch, heads, device, **kw):
    from centertrack_amd import losses
    opt = R.Opt(heads, **kw)
    with torch.no_grad():
        tot, stats = losses.GenericLoss(opt)([_to(out, device)], _to(batch, device))
    return tot, stats


def _loss_err(got, want):
    got, want = float(got), float(want)
    if want == 0.0:
        return 0.0 if got == 0.0 else float('inf')
    return abs(got - want) / abs(want)


def compare(label, got, want, e32, heads, out, batch, terms=None):
    """``want`` / ``e32``: {head: (loss, grad)} in float64 and the float32 reference's errors {head: (loss, grad)};
    ``terms``: {head: K of the loss} where fewer terms than R.terms counts are non-zero by construction"""
    fails, bounds = [], {}
    for h in heads:
        K = terms[h] if terms else R.terms(h, out[h].shape, _slots(h, batch))
        el, eg = _loss_err(got[h][0], want[h][0]), R.err(got[h][1], want[h][1])
        bl, bg = R.bound(e32[h][0], K), R.bound(e32[h][1], 1)
        bounds[h] = bl
        print('loss %s %-14s loss err %.3e (e32 %.3e bound %.3e)  grad err %.3e (e32 %.3e bound %.3e)  max|g64| %.3e'
              % (label, h, el, e32[h][0], bl, eg, e32[h][1], bg, float(want[h][1].abs().max())))
        if not el <= bl:
            fails.append((h, 'loss', el, bl))
        if not eg <= bg:
            fails.append((h, 'grad', eg, bg))
        if float(want[h][1].abs().max()) == 0.0:
            assert float(got[h][1].abs().max()) == 0.0, h
    assert not fails, fails
    return bounds


_mirror_cache = {}


def mirror(key, out, batch, heads):
    """(float64 truth, e32) of the mirror, once per process"""
    if key not in _mirror_cache:
        w64 = R.losses_and_grads(out, batch, heads, torch.float64)
        w32 = R.losses_and_grads(out, batch, heads, torch.float32)
        e32 = {h: (_loss_err(w32[h][0], w64[h][0]) if float(w64[h][0]) != 0 else 0.0, R.err(w32[h][1], w64[h][1]))
               for h in heads}
        _mirror_cache[key] = (w64, e32)
    return _mirror_cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# goldens

@pytest.mark.parametrize('name', CASES)
def test_golden_losses_and_gradients(device, golden_dir, name):
    g = load_case(golden_dir, name)
    heads = g['heads']
    _assert_away_from_the_clamp(g['out'])
    got = hip_losses_and_grads(g['out'], g['batch'], heads, device)
    want = {h: (g['loss'][h], g['grad'][h]) for h in heads}
    e32 = {h: (float(g['e32_loss'][h]), float(g['e32_grad'][h])) for h in heads}
    bounds = compare('golden ' + name, got, want, e32, heads, g['out'], g['batch'])
    # tot with wh weighted 0.1: a positive combination of the head losses, so its relative error stays below the
    # largest relative bound of a head
    tot, stats = hip_tot(g['out'], g['batch'], heads, device)
    want_tot = sum((0.1 if h == 'wh' else 1.0) * float(g['loss'][h]) for h in heads)
    assert _loss_err(tot, want_tot) <= max(bounds.values())
    assert sorted(stats) == sorted(list(heads) + ['tot'])
    for h in heads:
        assert float(stats[h]) == float(got[h][0])       # the same kernels whichever way they are called


# ---------------------------------------------------------------------------------------------------------------------
# extra shapes against the float64 mirror

#        id                     B  C   H   W   M    valid        heads
SHAPES = [('1x3x5x7', 1, 3, 5, 7, 4, [3], R.ALL_HEADS + ('hm_hp', 'hps', 'hp_offset')),   # odd everywhere, below one vector
          ('2x80x32x40', 2, 80, 32, 40, 32, [20, 32], R.ALL_HEADS),       # many workgroups, ragged tail, many partials
          ('C1', 2, 1, 8, 12, 8, [5, 3], ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal', 'dep')),
          ('M1', 2, 4, 8, 12, 1, [1, 0], R.ALL_HEADS),
          ('M256', 2, 5, 16, 24, 256, [200, 200], R.ALL_HEADS + ('hm_hp', 'hp_offset'))]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: s[0])
def test_extra_shapes_against_the_float64_mirror(device, shape):
    name, B, C, H, W, M, valid, heads = shape
    out, batch = R.make_batch(100 + len(name), B, H, W, M, heads, C, valid=valid)
    _assert_away_from_the_clamp(out)
    want, e32 = mirror(name, out, batch, heads)
    got = hip_losses_and_grads(out, batch, heads, device)
    compare(name, got, want, e32, heads, out, batch)


# ---------------------------------------------------------------------------------------------------------------------
# designed values

def test_saturated_logits_have_a_zero_gradient(device):
    """|x| = 12: the clamp is active on every element, the positives included: the gradient is exactly 0, as torch's"""
    heads = ('hm',)
    out, batch = R.make_batch(5, 2, 8, 12, 8, heads, 3)
    sign = torch.where(out['hm'] > 0, 1.0, -1.0)
    out['hm'] = 12.0 * sign
    got = hip_losses_and_grads(out, batch, heads, device)
    assert float(got['hm'][1].abs().max()) == 0.0
    want, e32 = mirror('saturated', out, batch, heads)
    assert float(want['hm'][1].abs().max()) == 0.0
    compare('saturated', got, want, e32, heads, out, batch)


def test_a_target_of_one_everywhere_leaves_only_the_positive_term(device):
    heads = ('hm',)
    out, batch = R.make_batch(6, 2, 8, 12, 8, heads, 3)
    _assert_away_from_the_clamp(out)
    batch['hm'] = torch.ones_like(batch['hm'])
    want, e32 = mirror('ones', out, batch, heads)
    got = hip_losses_and_grads(out, batch, heads, device)
    compare('gt=1', got, want, e32, heads, out, batch)
    touched = torch.zeros(2, 3, 96, dtype=torch.bool)
    for b in range(2):
        touched[b, batch['cat'][b], batch['ind'][b]] = True
    assert float(got['hm'][1].cpu().reshape(2, 3, 96)[~touched].abs().max()) == 0.0      # a zero negative term


def test_four_slots_on_one_element_sum_in_a_fixed_order(device):
    heads = ('hm', 'reg', 'dep', 'rot', 'nuscenes_att')
    out, batch = R.make_batch(7, 2, 8, 12, 8, heads, 3, valid=[8, 6])
    _assert_away_from_the_clamp(out)
    batch['ind'][0, [1, 3, 4, 7]] = 50
    batch['cat'][0, [1, 3, 4, 7]] = 2
    batch['hm'][0, 2, 50 // 12, 50 % 12] = 1
    want, e32 = mirror('four', out, batch, heads)
    got = hip_losses_and_grads(out, batch, heads, device)
    compare('four slots', got, want, e32, heads, out, batch)
    again = hip_losses_and_grads(out, batch, heads, device)
    for h in heads:
        assert torch.equal(got[h][0], again[h][0]) and torch.equal(got[h][1], again[h][1]), h
    # (the four slots really add up: the element's gradient is not that of one slot alone)
    single = dict(batch, mask=batch['mask'].clone())
    single['mask'][0, [3, 4, 7]] = 0
    one = R.losses_and_grads(out, single, ('hm',))['hm'][1]
    assert abs(float(want['hm'][1][0, 2, 4, 2]) - float(one[0, 2, 4, 2])) > 1e-3 * float(want['hm'][1].abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# slots out of range

def _mask_out(batch, b, m):
    """the same batch with slot (b, m) masked out"""
    r = {k: v.clone() for k, v in batch.items()}
    r['ind'][b, m] = 0
    r['cat'][b, m] = 0
    r['rotbin'][b, m] = 0
    for k in r:
        if k.endswith('mask'):
            r[k][b, m] = 0
    return r


def test_out_of_range_slots_touch_nothing(device):
    """ind = H*W and cat = C.  Every head map and every gradient buffer is a slice of a larger allocation filled with a
    sentinel, so an unguarded access shows as a wrong number or a changed sentinel, not as a fault."""
    from centertrack_amd import _lib, losses, ops
    heads = R.ALL_HEADS
    B, C, H, W, M = 2, 3, 7, 9, 8            # C*H*W*4 is no multiple of 16 for C in (1, 2, 3): those slices are unaligned
    out, batch = R.make_batch(8, B, H, W, M, heads, C, valid=[8, 6])
    _assert_away_from_the_clamp(out)
    bad = {k: v.clone() for k, v in batch.items()}
    bad['ind'][1, 2] = H * W                  # the LAST image: channel C - 1 of this slot lies behind the slice
    bad['ind'][0, 5] = H * W
    bad['cat'][1, 4] = C
    # the focal head skips (1, 2) and (1, 4) and (0, 5); the other heads skip (1, 2) and (0, 5) only
    clean_hm = _mask_out(_mask_out(_mask_out(batch, 1, 2), 0, 5), 1, 4)
    clean = _mask_out(_mask_out(batch, 1, 2), 0, 5)
    want = R.losses_and_grads(out, clean, heads, torch.float64)
    want['hm'] = R.losses_and_grads(out, clean_hm, ('hm',), torch.float64)['hm']
    w32 = R.losses_and_grads(out, clean, heads, torch.float32)
    w32['hm'] = R.losses_and_grads(out, clean_hm, ('hm',), torch.float32)['hm']
    e32 = {h: (_loss_err(w32[h][0], want[h][0]), R.err(w32[h][1], want[h][1])) for h in heads}

    SENT = 777.0
    b = _to(bad, device)
    xs, grads, bigs = {}, {}, []
    for h in heads:
        for store, fill in ((xs, out[h]), (grads, None)):
            big = torch.full((B + 2,) + tuple(out[h].shape[1:]), SENT, device=device)
            store[h] = big[1:1 + B]
            if fill is not None:
                store[h].copy_(fill)
            bigs.append(big)
    specs = [losses.GenericLoss._spec(h, xs, b) for h in heads]
    for s, h in zip(specs, heads):
        assert s[1].data_ptr() == xs[h].data_ptr()            # no copy was made: the kernels see the slices
    lib = _lib.load()
    loss = torch.full((len(heads) + 2,), SENT, device=device)
    up = torch.ones(len(heads), device=device)
    d, _keep = ops.make_loss_desc(specs, [grads[h] for h in heads])
    need = lib.ct_generic_loss_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(need // 4, device=device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    d.loss, d.grad_loss = loss[1:].data_ptr(), up.data_ptr()
    _lib.check(lib.ct_generic_loss_forward(ctypes.byref(d), _lib.stream_ptr()))
    _lib.check(lib.ct_generic_loss_backward(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = {h: (loss[1 + i], grads[h]) for i, h in enumerate(heads)}
    compare('out of range', got, want, e32, heads, out, batch)
    assert float(loss[0]) == SENT and float(loss[-1]) == SENT
    for big in bigs:
        assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# plumbing

def _generic(out, batch, heads, device, opt=None, **kw):
    """(tot, stats, leaves, outputs) of GenericLoss on fresh leaves"""
    from centertrack_amd import losses
    opt = opt or R.Opt(heads)
    stacks = out if isinstance(out, list) else [out]
    leaves = [{h: o[h].to(device).requires_grad_() for h in heads} for o in stacks]
    outputs = [dict(l) for l in leaves]
    tot, stats = losses.GenericLoss(opt, **kw)(outputs, _to(batch, device))
    return tot, stats, leaves, outputs


def _plain(device):
    heads = R.ALL_HEADS
    out, batch = R.make_batch(9, 2, 8, 12, 8, heads, 3, valid=[8, 5])
    tot, stats, leaves, _ = _generic(out, batch, heads, device)
    tot.backward()
    return heads, out, batch, tot.detach(), {h: leaves[0][h].grad for h in heads}


def test_two_runs_are_bitwise_equal(device):
    heads, out, batch, tot, grads = _plain(device)
    _, _, _, tot2, grads2 = _plain(device)
    assert torch.equal(tot, tot2)
    for h in heads:
        assert torch.equal(grads[h], grads2[h]), h


def test_channels_last_sliced_and_integer_inputs(device):
    from centertrack_amd import losses
    heads, out, batch, tot, grads = _plain(device)
    leaves = {}
    for i, h in enumerate(heads):
        x = out[h].to(device)
        if i % 2 == 0:
            wide = torch.zeros(2, x.shape[1] + 3, 8, 12, device=device)
            wide[:, 1:1 + x.shape[1]] = x
            leaves[h] = wide.requires_grad_()
        else:
            leaves[h] = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    outputs = {h: (leaves[h][:, 1:1 + out[h].shape[1]] if i % 2 == 0 else leaves[h]) for i, h in enumerate(heads)}
    b = _to(batch, device)
    b['mask'] = b['mask'].to(torch.uint8)
    b['rot_mask'] = b['rot_mask'].to(torch.int32)
    b['reg_mask'] = b['reg_mask'].bool()
    b['ind'] = b['ind'].to(torch.int32)
    tot2, _ = losses.GenericLoss(R.Opt(heads))([outputs], b)
    tot2.backward()
    assert torch.equal(tot2.detach(), tot)
    for i, h in enumerate(heads):
        g = leaves[h].grad
        if i % 2 == 0:
            assert float(g[:, :1].abs().max()) == 0 and float(g[:, 1 + out[h].shape[1]:].abs().max()) == 0
            g = g[:, 1:1 + out[h].shape[1]]
        assert torch.equal(g, grads[h]), h


def test_heads_without_requires_grad_get_no_gradient(device, monkeypatch):
    from centertrack_amd import losses, ops
    heads, out, batch, tot, grads = _plain(device)
    frozen = ('hm', 'wh', 'rot')
    leaves = {h: out[h].to(device).requires_grad_(h not in frozen) for h in heads}
    seen = []
    real = ops.generic_loss_backward
    monkeypatch.setattr(ops, 'generic_loss_backward', lambda hs, gl, needs=None: seen.append(list(needs)) or real(hs, gl, needs))
    tot2, _ = losses.GenericLoss(R.Opt(heads))([dict(leaves)], _to(batch, device))
    tot2.backward()
    assert seen == [[h not in frozen for h in heads]]
    for h in heads:
        if h in frozen:
            assert leaves[h].grad is None
        else:
            assert torch.equal(leaves[h].grad, grads[h]), h


def test_no_grad_keeps_no_backward_state(device, monkeypatch):
    from centertrack_amd import losses, ops
    heads, out, batch, tot, _ = _plain(device)
    monkeypatch.setattr(ops, 'generic_loss_backward', lambda *a, **k: pytest.fail('backward under no_grad'))
    leaves = {h: out[h].to(device).requires_grad_() for h in heads}
    with torch.no_grad():
        tot2, stats = losses.GenericLoss(R.Opt(heads))([dict(leaves)], _to(batch, device))
    assert tot2.grad_fn is None and not tot2.requires_grad and torch.equal(tot2, tot)
    assert all(stats[h].grad_fn is None for h in heads)


def test_two_stacks_and_an_upstream_gradient(device):
    heads = ('hm', 'reg', 'wh', 'dep')
    o1, batch = R.make_batch(21, 2, 8, 12, 8, heads, 3)
    o2, _ = R.make_batch(22, 2, 8, 12, 8, heads, 3)
    for o in (o1, o2):
        _assert_away_from_the_clamp(o)
    opt = R.Opt(heads, num_stacks=2)
    tot, stats, leaves, _ = _generic([o1, o2], batch, heads, device, opt=opt)
    (2.5 * tot).backward()
    l64 = [{h: o[h].double().requires_grad_() for h in heads} for o in (o1, o2)]
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    tot64, st64 = R.generic_loss(l64, b64, heads, opt.weights, 2)
    (2.5 * tot64).backward()
    l32 = [{h: o[h].clone().requires_grad_() for h in heads} for o in (o1, o2)]
    tot32, st32 = R.generic_loss(l32, batch, heads, opt.weights, 2)
    (2.5 * tot32).backward()
    K = max(R.terms(h, o1[h].shape, 8) for h in heads)
    assert _loss_err(tot, tot64) <= R.bound(_loss_err(tot32, tot64), K)
    for h in heads:
        assert _loss_err(stats[h], st64[h]) <= R.bound(_loss_err(st32[h], st64[h]), R.terms(h, o1[h].shape, 8)), h
        for s in (0, 1):
            e32 = R.err(l32[s][h].grad, l64[s][h].grad)
            assert R.err(leaves[s][h].grad, l64[s][h].grad) <= R.bound(e32, 1), (h, s)


def test_sigmoid_outputs_replaces_the_three_maps_afterwards(device):
    heads = ('hm', 'reg', 'dep')
    out, batch = R.make_batch(23, 2, 8, 12, 8, heads, 3)
    tot, _, leaves, outputs = _generic(out, batch, heads, device)
    assert all(outputs[0][h] is leaves[0][h] for h in heads)            # the default does not touch ``outputs``
    tot2, _, leaves2, outputs2 = _generic(out, batch, heads, device, sigmoid_outputs=True)
    assert torch.equal(tot.detach(), tot2.detach())
    x = leaves2[0]
    assert outputs2[0]['reg'] is x['reg']
    for h in ('hm', 'dep'):
        assert not outputs2[0][h].requires_grad
    torch.testing.assert_close(outputs2[0]['hm'], x['hm'].detach().sigmoid().clamp(1e-4, 1 - 1e-4), rtol=1e-6, atol=0)
    torch.testing.assert_close(outputs2[0]['dep'], 1. / (x['dep'].detach().sigmoid() + 1e-6) - 1., rtol=1e-6, atol=1e-6)
    tot2.backward()
    assert x['hm'].grad is not None and x['dep'].grad is not None


def test_a_head_without_a_loss_stays_zero_as_in_the_reference(device):
    """trainer.py:42,82-84: every head of opt.heads is in loss_stats; one that no loss is defined for stays 0"""
    from centertrack_amd import losses
    heads = ('hm', 'reg')
    out, batch = R.make_batch(24, 2, 8, 12, 8, heads, 3)
    opt = R.Opt(heads + ('embedding',))
    o = _to(out, device)
    o['embedding'] = torch.zeros(2, 4, 8, 12, device=device)
    tot, stats = losses.GenericLoss(opt)([o], _to(batch, device))
    want, _ = losses.GenericLoss(R.Opt(heads))([_to(out, device)], _to(batch, device))
    assert stats['embedding'] == 0 and torch.equal(tot, want)


def test_the_single_loss_classes_run_on_the_same_kernels(device):
    from centertrack_amd import losses
    heads, out, batch, _, grads = _plain(device)
    _, stats, _, _ = _generic(out, batch, heads, device)
    b, o = _to(batch, device), _to(out, device)
    assert float(losses.FastFocalLoss()(o['hm'], b['hm'], b['ind'], b['mask'], b['cat'])) == float(stats['hm'])
    assert float(losses.RegWeightedL1Loss()(o['wh'], b['wh_mask'], b['ind'], b['wh'])) == float(stats['wh'])
    assert float(losses.RegWeightedL1Loss(depth=True)(o['dep'], b['dep_mask'], b['ind'], b['dep'])) == float(stats['dep'])
    assert float(losses.WeightedBCELoss()(o['nuscenes_att'], b['nuscenes_att_mask'], b['ind'], b['nuscenes_att'])) \
        == float(stats['nuscenes_att'])
    x = o['rot'].clone().requires_grad_()
    l = losses.BinRotLoss()(x, b['rot_mask'], b['ind'], b['rotbin'], b['rotres'])
    assert float(l) == float(stats['rot'])
    l.backward()
    assert torch.equal(x.grad, grads['rot'])


# ---------------------------------------------------------------------------------------------------------------------
# one step through the network

class _Net(torch.nn.Module):
    """a DLASeg-style stack in small: the reference's DeformConv block (DCN -> BatchNorm2d -> ReLU) and one 1x1
    convolution per head"""

    def __init__(self, dcn_cls, heads):
        super().__init__()
        nn = torch.nn
        self.block = nn.Sequential(dcn_cls(32, 32, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1),
                                   nn.BatchNorm2d(32, momentum=0.1), nn.ReLU(inplace=True))
        self.heads = nn.ModuleDict({h: nn.Conv2d(32, c, 1) for h, c in heads.items()})

    def forward(self, x):
        f = self.block(x)
        return [{h: conv(f) for h, conv in self.heads.items()}]


def test_one_training_step_through_dcn_and_loss(device):
    from centertrack_amd import dcn_v2 as hip, losses
    from oracle import dcn_v2 as odcn
    from _dcn_bwd import bound, err
    torch.manual_seed(0)
    heads = {'hm': 3, 'reg': 2, 'wh': 2, 'tracking': 2}
    B, H, W, M = 2, 12, 20, 8
    _, batch = R.make_batch(31, B, H, W, M, tuple(heads), 3)
    x = torch.randn(B, 32, H, W)
    ref32 = _Net(odcn.DCN, heads).train()
    ref32.block[0].conv_offset_mask.weight.data.normal_(0.0, 0.03)
    ref32.block[0].conv_offset_mask.bias.data.normal_(0.0, 0.3)
    ref64 = _Net(odcn.DCN, heads).train()
    ref64.load_state_dict(ref32.state_dict())
    ref64 = ref64.double()
    net = _Net(hip.DCN, heads).train()
    net.load_state_dict(ref32.state_dict())
    net = net.to(device)
    opt = R.Opt(tuple(heads))

    def run(model, x, loss_fn):
        tot = loss_fn(model(x))
        tot.backward()
        return float(tot), {n: p.grad.detach().cpu() for n, p in model.named_parameters()}

    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    t64, g64 = run(ref64, x.double(), lambda o: R.generic_loss(o, b64, tuple(heads), opt.weights)[0])
    t32, g32 = run(ref32, x, lambda o: R.generic_loss(o, batch, tuple(heads), opt.weights)[0])
    crit = losses.GenericLoss(opt)
    bdev = _to(batch, device)
    with hip.trainable():
        t, got = run(net, x.to(device), lambda o: crit(o, bdev)[0])
    K = B * H * W
    assert _loss_err(t, t64) <= bound(_loss_err(t32, t64), B * 3 * H * W)
    fails = []
    for n in sorted(g64):
        # (DCN.bias in front of a training-mode BatchNorm has a zero gradient in real arithmetic: measured against the
        # same module's weight gradient, as tests/test_hip_dcn_backward.py does)
        norm = g64[n.replace('.bias', '.weight')].abs().max() if n == 'block.0.bias' else None
        e, e32 = err(got[n], g64[n], norm), err(g32[n], g64[n], norm)
        print('loss net %-34s e(hip) %.3e  e(ref32) %.3e  bound %.3e' % (n, e, e32, bound(e32, K)))
        if not e <= bound(e32, K):
            fails.append((n, e, bound(e32, K)))
    assert not fails, fails
