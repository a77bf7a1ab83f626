"""GPU: the backward of the heads (ct_heads_tail_backward, ct_conv2d_backward_weight and the input-gradient conv;
centertrack_amd/csrc/heads_bwd.hip, ops.heads_backward, heads.FusedHeads) against float64 torch autograd on the CPU of the
reference's construction, conv3x3 -> ReLU -> conv1x1 per head.

Bound: tests/_dcn_bwd.py -- largest element error over the largest float64 element, ``<= min(1e-3, 4 * max(e32, 2^-23 *
sqrt(K)))`` with e32 the error of fp32 torch on the same inputs; K = N*H*W for gw0, gb0, gw2, gb2, K = 9*hc*nheads for gx,
K = c for gmid.  The fixture's hidden pre-activation is exact in fp32 (tests/_heads_bwd.py), so the ReLU mask of the kernel
and of the truth are the same set: the HIP hidden map must equal torch's bit for bit.

Shapes: ``_heads_bwd.SHAPES``; its comment names the branch of the two host plans each one reaches, and
tests/test_heads_backward_cpu.py asserts that; ``_heads_bwd.TAIL_CASE`` runs the tail alone at two tiles per slab, the plan of
training at batch 4, on a hidden map that is built directly (``_heads_bwd.TAIL_REGIMES`` names what the cases reach)."""
from collections import OrderedDict

import pytest
import torch

import _heads_bwd as HB
from _dcn_bwd import bound, err

pytestmark = pytest.mark.gpu


def _dev(fx, device):
    heads = fx['heads']
    w0 = torch.cat([fx['w0'][h] for h in heads], 0).to(device)
    b0 = torch.cat([fx['b0'][h] for h in heads], 0).to(device)
    w2s = OrderedDict((h, fx['w2'][h].to(device)) for h in heads)
    b2s = OrderedDict((h, fx['b2'][h].to(device)) for h in heads)
    gouts = OrderedDict((h, fx['gout'][h].to(device)) for h in heads)
    return w0, b0, w2s, b2s, gouts


ALL = {'x': True, 'w0': True, 'b0': True, 'w2': True, 'b2': True}


def _judge(fails, tag, name, got, t64, t32, K):
    e, e32 = err(got.cpu(), t64), err(t32, t64)
    b = bound(e32, K)
    print('heads bwd %-28s %-12s e(hip) %.3e  e(torch32) %.3e  bound %.3e' % (tag, name, e, e32, b))
    if not e <= b:
        fails.append((tag, name, e, b))


@pytest.mark.parametrize('case', HB.SHAPES, ids=HB.case_id)
def test_gradients_against_float64_autograd(device, case):
    from centertrack_amd import ops
    (N, H, W), heads = case
    fx, t64, t32 = HB.truth(case)
    assert torch.equal(t32['mid'].double(), t64['mid'])                      # the fixture is exact
    w0, b0, w2s, b2s, gouts = _dev(fx, device)
    feat = ops.view_from_nchw(fx['x'].to(device))
    outs, mid = ops.heads_forward_train(feat, w0, b0, w2s, b2s)
    assert torch.equal(mid.to_nchw().cpu(), t32['mid']), 'the HIP hidden map differs from the exact one'
    tag = HB.case_id(case)
    fails = []
    for h in heads:
        _judge(fails, tag, 'logits ' + h, outs[h], t64['out'][h], t32['out'][h], HB.HC)
    res = ops.heads_backward(feat, mid, gouts, w0, w2s, ALL)
    K = HB.terms(case)
    _judge(fails, tag, 'gw0', res['w0'], t64['w0'], t32['w0'], K['w0'])
    _judge(fails, tag, 'gb0', res['b0'], t64['b0'], t32['b0'], K['b0'])
    _judge(fails, tag, 'gx', res['x'].to_nchw(), t64['x'], t32['x'], K['x'])
    c0 = 0
    for j, (h, c) in enumerate(heads.items()):
        _judge(fails, tag, 'gw2 ' + h, res['w2'][h], t64['w2'][h], t32['w2'][h], K['w2'])
        _judge(fails, tag, 'gb2 ' + h, res['b2'][h], t64['b2'][h], t32['b2'][h], K['b2'])
        sl = slice(HB.HC * j, HB.HC * (j + 1))
        _judge(fails, tag, 'gmid ' + h, res['gmid'].to_nchw()[:, sl], t64['gmid'][:, sl], t32['gmid'][:, sl], c)
    # torch's ReLU convention: no gradient where the hidden value is exactly 0 (the fixture has such units)
    dead = t64['mid'] == 0
    assert bool((t64['pre'] == 0).any()) and float(res['gmid'].to_nchw().cpu()[dead].abs().max()) == 0.0
    assert not fails, fails


def test_the_tail_at_two_tiles_per_slab(device):
    """``_heads_bwd.TAIL_CASE``: ``pixPerSlab`` 128, so the tile loop of heads_tail_weight_kernel runs twice -- ``g`` re-staged,
    ``bsum`` carried -- with a last slab of a full and a ragged tile and a tile across the image border.  Once with only
    ``w2`` / ``b2`` needed (the weight part alone), once with ``x`` needed as well (the hidden gradient into a caller-owned view
    pre-filled with NaN, 7 in its pitch padding), against the float64 sums over the hidden map itself; K = N*H*W for gw2 and
    gb2, c for gmid, 9 * hc * nheads for gx.  Two runs are bitwise equal, and leaving ``x`` out changes no bit of gw2 / gb2."""
    from centertrack_amd import ops
    case = HB.TAIL_CASE
    (N, H, W), heads = case
    plan = HB.tail_plan(N, H, W, HB.HC, tuple(heads.values()))
    assert (plan['pixPerSlab'], plan['slabs'], plan['last_slab_pixels']) == (128, 33, 86) and (H * W) % 64 != 0
    fx = HB.tail_fixture(case)
    t64, t32 = HB.tail_truth(fx, torch.float64), HB.tail_truth(fx, torch.float32)
    C = HB.HC * len(heads)
    mid = ops.View(fx['mid'].permute(0, 2, 3, 1).contiguous().to(device))
    w0 = fx['w0'].to(device)
    w2s = OrderedDict((h, fx['w2'][h].to(device)) for h in heads)
    gouts = OrderedDict((h, fx['gout'][h].to(device)) for h in heads)
    tag = '%dx%dx%d-%d heads of 20' % (N, H, W, len(heads))
    fails = []

    def flat(r):
        return [r['w2'][h] for h in heads] + [r['b2'][h] for h in heads]

    def poison():
        """gw2 / gb2 come from torch's caching allocator, which may hand back what an earlier run wrote: blocks of their sizes
        are filled with NaN and freed first, so that an element the reduce kernel skips is seen"""
        blocks = [torch.full((n,), float('nan'), device=device) for c in heads.values() for n in (c * HB.HC, c)]
        del blocks
    poison()
    tail = ops.heads_backward(None, mid, gouts, w0, w2s, {'w2': True, 'b2': True})
    assert tail['gmid'] is None and tail['x'] is None and tail['w0'] is None
    for h in heads:
        _judge(fails, tag, 'gw2 ' + h, tail['w2'][h], t64['w2'][h], t32['w2'][h], N * H * W)
        _judge(fails, tag, 'gb2 ' + h, tail['b2'][h], t64['b2'][h], t32['b2'][h], N * H * W)

    def full():
        gbuf = torch.full((N, H, W, C + 16), 7.0, device=device)
        gbuf[..., :C] = float('nan')
        poison()
        r = ops.heads_backward(None, mid, gouts, w0, w2s, {'x': True, 'w2': True, 'b2': True}, gmid=ops.View(gbuf, 0, C))
        assert r['gmid'].buf is gbuf and bool((gbuf[..., C:] == 7.0).all())
        return r
    res = full()
    for a, b in zip(flat(res), flat(tail)):
        assert torch.equal(a, b)                                         # the hidden gradient changes no bit of the weight part
    gm = res['gmid'].to_nchw().cpu()
    for j, (h, c) in enumerate(heads.items()):
        sl = slice(HB.HC * j, HB.HC * (j + 1))
        _judge(fails, tag, 'gmid ' + h, gm[:, sl], t64['gmid'][:, sl], t32['gmid'][:, sl], c)
    dead = fx['mid'] == 0
    assert 0.4 < float(dead.double().mean()) < 0.6 and float(gm[dead].abs().max()) == 0.0
    _judge(fails, tag, 'gx', res['x'].to_nchw(), t64['x'], t32['x'], 9 * HB.HC * len(heads))
    again = full()
    for a, b in zip(flat(res) + [res['gmid'].buf, res['x'].buf], flat(again) + [again['gmid'].buf, again['x'].buf]):
        assert torch.equal(a, b)
    assert not fails, fails


def _module(case, device, freeze=()):
    from centertrack_amd import heads as HD
    fx, _, _ = HB.truth(case)
    m = HD.FusedHeads(fx['heads'], HB.HC)
    m.load_state_dict(OrderedDict(('%s.%s' % (h, k), fx[n][h]) for h in fx['heads']
                                  for k, n in (('0.weight', 'w0'), ('0.bias', 'b0'), ('2.weight', 'w2'), ('2.bias', 'b2'))))
    m = m.to(device)
    for n, p in m.named_parameters():
        if any(n.startswith(f) or n.endswith(f) for f in freeze):
            p.requires_grad_(False)
    return m, fx


def _backward(m, fx, x, device):
    out = m(x)
    tot = sum((out[h] * fx['gout'][h].to(device)).sum() for h in fx['heads'])
    tot.backward()
    return out


def _count_launches(monkeypatch):
    """names of the C entry points ops.* calls during a backward"""
    from centertrack_amd import _lib
    lib = _lib.load()
    calls = []

    class Spy(object):
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ('ct_conv2d', 'ct_conv2d_backward_weight', 'ct_heads_tail_backward'):
                def wrapped(*a, **k):
                    calls.append((name, a[0]._obj.flags if name == 'ct_heads_tail_backward' else None))
                    return fn(*a, **k)
                return wrapped
            return fn
    monkeypatch.setattr(_lib, 'load', lambda: Spy())
    return calls


def test_needs_input_grad_selects_the_launches(device, monkeypatch):
    """frozen feature, frozen ``.0.*``, frozen everything but one head's ``.2.*``: the right gradients for what is asked,
    None for the rest, and no launch for what nobody needs"""
    from centertrack_amd import _lib
    case = HB.SHAPES[0]
    _, t64, t32 = HB.truth(case)
    K = HB.terms(case)
    heads = list(case[1])
    names64 = {}
    for j, h in enumerate(heads):
        sl = slice(HB.HC * j, HB.HC * (j + 1))
        names64.update({h + '.0.weight': ('w0', sl), h + '.0.bias': ('b0', sl), h + '.2.weight': ('w2', h), h + '.2.bias': ('b2', h)})

    def check(m, fails, tag):
        for n, p in m.named_parameters():
            if not p.requires_grad:
                assert p.grad is None, (tag, n)
                continue
            key, idx = names64[n]
            _judge(fails, tag, n, p.grad, t64[key][idx], t32[key][idx], K[key])

    fails = []
    # 1. frozen feature: no input-gradient conv
    m, fx = _module(case, device)
    x = fx['x'].to(device)
    assert not x.requires_grad
    calls = _count_launches(monkeypatch)
    out = m(x)
    fwd = len(calls)
    assert [c[0] for c in calls] == ['ct_conv2d'] * (1 + len(heads))
    sum((out[h] * fx['gout'][h].to(device)).sum() for h in heads).backward()
    assert calls[fwd:] == [('ct_heads_tail_backward', 3), ('ct_conv2d_backward_weight', None)], calls[fwd:]
    assert x.grad is None
    check(m, fails, 'frozen feature')
    # 2. feature with a gradient, frozen first layers: the hidden gradient and the conv, no weight-gradient kernel
    m, fx = _module(case, device, freeze=('.0.weight', '.0.bias'))
    x = fx['x'].to(device).requires_grad_()
    del calls[:]
    out = m(x)
    fwd = len(calls)
    sum((out[h] * fx['gout'][h].to(device)).sum() for h in heads).backward()
    assert calls[fwd:] == [('ct_heads_tail_backward', 3), ('ct_conv2d', None)], calls[fwd:]
    _judge(fails, 'frozen .0', 'x', x.grad, t64['x'], t32['x'], K['x'])
    check(m, fails, 'frozen .0')
    # 3. everything frozen but one head's last layer: the tail's weight part alone, for that head alone
    m, fx = _module(case, device, freeze=['%s.%s' % (h, k) for h in heads for k in ('0.weight', '0.bias', '2.weight', '2.bias')
                                          if not (h == 'wh' and k[0] == '2')])
    x = fx['x'].to(device)
    del calls[:]
    out = m(x)
    fwd = len(calls)
    sum((out[h] * fx['gout'][h].to(device)).sum() for h in heads).backward()
    assert calls[fwd:] == [('ct_heads_tail_backward', _lib.CT_HEADS_BWD_WEIGHT)], calls[fwd:]
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == ['wh.2.bias', 'wh.2.weight']
    check(m, fails, 'one head .2')
    assert not fails, fails


def test_two_backward_runs_are_bitwise_equal(device):
    from centertrack_amd import ops
    for case in (HB.SHAPES[0], HB.SHAPES[4]):
        fx, _, _ = HB.truth(case)
        w0, b0, w2s, b2s, gouts = _dev(fx, device)
        feat = ops.view_from_nchw(fx['x'].to(device))
        _, mid = ops.heads_forward_train(feat, w0, b0, w2s, b2s)
        runs = []
        for _ in range(2):
            r = ops.heads_backward(feat, mid, gouts, w0, w2s, ALL)
            flat = [r['x'].buf, r['gmid'].buf, r['w0'], r['b0']] + [r['w2'][h] for h in w2s] + [r['b2'][h] for h in w2s]
            runs.append([t.clone() for t in flat])
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_a_second_forward_does_not_disturb_the_first_backward(device):
    """what backward needs is private to its call: two forwards (the second on other data, through the same caller-owned
    view, as a launch plan's feature buffer is reused), then the backward of the first"""
    from centertrack_amd import ops
    case = HB.SHAPES[0]
    m, fx = _module(case, device)
    view = ops.view_from_nchw(fx['x'].to(device))
    _backward(m, fx, view, device)
    alone = OrderedDict((n, p.grad.clone()) for n, p in m.named_parameters())
    m.zero_grad(set_to_none=True)
    out1 = m(view)
    view.buf.copy_(torch.randn_like(view.buf))                 # the plan's buffer moves on to the next frame
    out2 = m(view)
    sum((out1[h] * fx['gout'][h].to(device)).sum() for h in fx['heads']).backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, alone[n]), n
    del out2


def test_padding_of_caller_views_is_neither_read_nor_written(device):
    """``feat`` with a pitch of 80 > 64 and a ``gmid`` view with a pitch of nheads*hc + 16: NaN in the padding of the inputs
    does not reach a result, and the padding of the output keeps its sentinel"""
    from centertrack_amd import ops
    case = HB.SHAPES[0]
    (N, H, W), heads = case
    fx, _, _ = HB.truth(case)
    w0, b0, w2s, b2s, gouts = _dev(fx, device)
    tight = ops.view_from_nchw(fx['x'].to(device))
    _, mid = ops.heads_forward_train(tight, w0, b0, w2s, b2s)
    want = ops.heads_backward(tight, mid, gouts, w0, w2s, ALL)
    wide = ops.View(torch.full((N, H, W, 80), float('nan'), device=device), 8, 64)      # channels 8 .. 71 of 80
    wide.buf[..., 8:72] = tight.buf
    _, mid_w = ops.heads_forward_train(wide, w0, b0, w2s, b2s)
    assert torch.equal(mid_w.buf, mid.buf)
    C = HB.HC * len(heads)
    mid_p = ops.View(torch.full((N, H, W, C + 16), float('nan'), device=device), 0, C)   # the hidden map itself with a pitch
    mid_p.buf[..., :C] = mid.buf
    gbuf = torch.full((N, H, W, C + 16), -7.0, device=device)
    got = ops.heads_backward(wide, mid_p, gouts, w0, w2s, ALL, gmid=ops.View(gbuf, 0, C))
    assert torch.equal(gbuf[..., C:], torch.full_like(gbuf[..., C:], -7.0))
    assert torch.equal(gbuf[..., :C], want['gmid'].buf)
    assert torch.equal(got['w0'], want['w0']) and torch.equal(got['b0'], want['b0']) and torch.equal(got['x'].buf, want['x'].buf)
    for h in heads:
        assert torch.equal(got['w2'][h], want['w2'][h]) and torch.equal(got['b2'][h], want['b2'][h])
    assert torch.equal(torch.isnan(wide.buf), torch.isnan(torch.full_like(wide.buf, float('nan')).index_fill_(
        3, torch.arange(8, 72, device=device), 0.0)))


_generic = {}


def _generic_truth(ks, cin, cout):
    key = (ks, cin, cout)
    if key not in _generic:
        N, H, W = 2, 9, 11
        g = torch.Generator().manual_seed(1000 * ks + cin + cout)
        x = torch.randn((N, cin, H, W), generator=g)
        gy = torch.randn((N, cout, H, W), generator=g)
        w = [torch.nn.grad.conv2d_weight(x.to(dt), (cout, cin, ks, ks), gy.to(dt), padding=ks // 2) for dt in (torch.float64, torch.float32)]
        b = [gy.to(dt).sum((0, 2, 3)) for dt in (torch.float64, torch.float32)]
        _generic[key] = (x, gy, w, b)
    return _generic[key]


@pytest.mark.parametrize('cout', [8, 72, 256])
@pytest.mark.parametrize('cin', [16, 64, 256])
@pytest.mark.parametrize('ks', [1, 3])
def test_generic_conv_weight_gradient(device, ks, cin, cout):
    """ct_conv2d_backward_weight on its own against torch.nn.grad.conv2d_weight in float64: Cin 16 (half a channel group),
    Cout 8 / 72 (ragged cout tiles, a second cout group of one tile), (2, 9, 11): N*H*W % 4 == 2"""
    from centertrack_amd import ops
    x, gy, w, b = _generic_truth(ks, cin, cout)
    K = x.shape[0] * x.shape[2] * x.shape[3]
    gw, gb = ops.conv_backward_weight(ops.view_from_nchw(x.to(device)), ops.view_from_nchw(gy.to(device)), ks, need_bias=True)
    fails = []
    tag = 'ks%d %d->%d' % (ks, cin, cout)
    _judge(fails, tag, 'gw', gw, w[0], w[1], K)
    _judge(fails, tag, 'gb', gb, b[0], b[1], K)
    gw2, none = ops.conv_backward_weight(ops.view_from_nchw(x.to(device)), ops.view_from_nchw(gy.to(device)), ks, need_bias=False)
    assert none is None and torch.equal(gw2, gw)
    assert not fails, fails
