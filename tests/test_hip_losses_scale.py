"""GPU: the fused training loss (csrc/loss.hip) in the launch regimes of a real training batch, which the shapes of
tests/test_hip_losses.py do not reach: a focal map above the cap of 1024 workgroups (more than four trips through the grid-stride
loop, a finishing step over exactly 1024 partials) on the float4 and on the scalar path, CT_LOSS_MAX_SLOTS slots and the
first rejected value, all fifteen heads of ``losses.KNOWN_HEADS`` in one launch, and logits that are not float32.

Truth, error measure and bound are those of tests/test_hip_losses.py (the float64 mirror tests/_loss_ref.py,
``min(1e-3, 4 * max(e32, 2^-23 * sqrt(K)))``).  Above the cap that bound is 9.8e-4 for the loss, which is what one lost or
doubled partial changes it by (1 / 1024): there the loss is held to ``min(bound, 1 / 8192)`` as well, and the test first
shows, from the float64 share of every workgroup, that this is below half of what the smallest partial carries.  The inputs
are made once in tests/_loss_ref.py; tests/test_losses_cpu.py checks them (shares, probes, the float32 mirror) without a GPU."""
import ctypes

import pytest
import torch

import _loss_ref as R
import test_hip_losses as T

pytestmark = pytest.mark.gpu

SENT = 777.0


def _offset_slice(t, device, guard=8):
    """``t`` in a slice that starts 4 bytes into a sentinel-filled allocation (so it is not 16-byte aligned) with
    ``guard - 1`` sentinels behind it -> (slice, allocation); ``t`` = a shape: the slice keeps the sentinel"""
    shape = tuple(t.shape) if torch.is_tensor(t) else tuple(t)
    n = 1
    for v in shape:
        n *= v
    big = torch.full((n + guard,), SENT, device=device)
    view = big[1:1 + n].view(shape)
    if torch.is_tensor(t):
        view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view, big


def _guards_intact(big, n):
    return float(big[0]) == SENT and bool((big[1 + n:] == SENT).all())


def _c_entry_points(specs, grads, device):
    """forward and backward through the C entry points on caller-owned buffers -> the loss vector; its two neighbours
    in the allocation keep their sentinel"""
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    loss = torch.full((len(specs) + 2,), SENT, device=device)
    up = torch.ones(len(specs), device=device)
    d, _keep = ops.make_loss_desc(specs, grads)
    need = lib.ct_generic_loss_workspace_bytes(ctypes.byref(d))
    assert need > 0
    ws = torch.empty(need // 4, device=device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    d.loss, d.grad_loss = loss[1:].data_ptr(), up.data_ptr()
    _lib.check(lib.ct_generic_loss_forward(ctypes.byref(d), _lib.stream_ptr()))
    _lib.check(lib.ct_generic_loss_backward(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert float(loss[0]) == SENT and float(loss[-1]) == SENT
    return loss[1:-1]


# ---------------------------------------------------------------------------------------------------------------------
# A1: above the partial cap, random data

def _share_tolerance(label, e32_loss, K, vec):
    """min(project bound, 1 / 8192), shown to be below half of the smallest workgroup's share of the loss"""
    shares = R.scale_shares(vec)
    tol = min(R.bound(e32_loss, K), R.SHARE_TOL)
    print('loss %s shares of the 1024 partials (%s path): min %.3e max %.3e  project bound %.3e  tolerance %.3e'
          % (label, 'float4' if vec else 'scalar', float(shares.min()), float(shares.max()), R.bound(e32_loss, K), tol))
    assert tol < 0.5 * float(shares.min())
    return tol


@pytest.mark.parametrize('path', ['float4', 'scalar'])
def test_above_the_partial_cap_every_partial_counts_once(device, path):
    from centertrack_amd import losses
    heads = ('hm',)
    out, batch = R.scale_batch()
    n = out['hm'].numel()
    assert n > R.CAP and n % R.TRIP != 0                   # a capped grid: a fifth trip, and a ragged one
    T._assert_away_from_the_clamp(out)
    want, e32 = R.truth_and_e32('scale', out, batch, heads)
    tol = _share_tolerance('scale', e32['hm'][0], n, path == 'float4')
    if path == 'float4':
        got = T.hip_losses_and_grads(out, batch, heads, device)
    else:
        x, big_x = _offset_slice(out['hm'], device)
        gt, big_gt = _offset_slice(batch['hm'], device)
        grad, big_g = _offset_slice(out['hm'].shape, device)
        b = dict(T._to(batch, device), hm=gt)
        spec = losses.GenericLoss._spec('hm', {'hm': x}, b)
        assert spec[1].data_ptr() == x.data_ptr() and spec[2].data_ptr() == gt.data_ptr()     # the kernels see the slices
        loss = _c_entry_points([spec], [grad], device)
        got = {'hm': (loss[0], grad)}
        for big in (big_x, big_gt, big_g):
            assert _guards_intact(big, n)
        assert torch.equal(x.cpu(), out['hm']) and torch.equal(gt.cpu(), batch['hm'])
    T.compare('scale ' + path, got, want, e32, heads, out, batch)
    el = T._loss_err(got['hm'][0], want['hm'][0])
    print('loss scale %s hm loss err %.3e  tolerance %.3e' % (path, el, tol))
    assert el <= tol


# ---------------------------------------------------------------------------------------------------------------------
# A2: above the cap, probes

def test_above_the_partial_cap_probes_at_trip_boundaries_and_ends(device):
    heads = ('hm',)
    out, batch, probes = R.probe_batch()
    B, C, H, W, M = R.SCALE
    want, e32 = R.truth_and_e32('probes', out, batch, heads)
    got = T.hip_losses_and_grads(out, batch, heads, device)
    T.compare('probes', got, want, e32, heads, out, batch, terms={'hm': len(probes) + B * M})
    live = torch.zeros(out['hm'].numel(), dtype=torch.bool)
    live[probes] = True
    live[R.positive_elements(batch, out['hm'].shape)] = True
    g = got['hm'][1].cpu().reshape(-1)
    assert float(g[~live].abs().max()) == 0.0
    assert bool((g[probes] != 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# A3: the slot limit

def test_the_largest_slot_count(device):
    out, batch, heads = R.slot_limit_batch()
    assert batch['hp_ind'].shape[1] == R.MAX_SLOTS and batch['ind'].shape[1] == 512
    T._assert_away_from_the_clamp(out)
    want, e32 = R.truth_and_e32('slots', out, batch, heads)
    got = T.hip_losses_and_grads(out, batch, heads, device)
    T.compare('M8192', got, want, e32, heads, out, batch)
    again = T.hip_losses_and_grads(out, batch, heads, device)
    for h in heads:
        assert torch.equal(got[h][0], again[h][0]) and torch.equal(got[h][1], again[h][1]), h


def test_one_slot_more_is_rejected_and_nothing_is_written(device):
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    B, C, H, W, M = 2, 2, 16, 24, R.MAX_SLOTS + 1
    assert _lib.CT_LOSS_MAX_SLOTS == R.MAX_SLOTS
    x = torch.zeros(B, C, H, W, device=device)
    spec = (_lib.CT_LOSS_L1, x, torch.zeros(B, M, C, device=device), torch.ones(B, M, C, device=device),
            torch.zeros(B, M, dtype=torch.int64, device=device), None)
    grad = torch.full_like(x, SENT)
    loss = torch.full((3,), SENT, device=device)
    up = torch.ones(1, device=device)
    ws = torch.empty(4096, device=device)
    d, _keep = ops.make_loss_desc([spec], [grad])
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.loss, d.grad_loss = loss[1:].data_ptr(), up.data_ptr()
    for fn in (lib.ct_generic_loss_forward, lib.ct_generic_loss_backward):
        assert fn(ctypes.byref(d), _lib.stream_ptr()) == _lib.CT_ERR_ARG
        assert b'CT_LOSS_MAX_SLOTS' in lib.ct_last_error(), lib.ct_last_error()
    assert lib.ct_generic_loss_workspace_bytes(ctypes.byref(d)) == 0
    assert b'CT_LOSS_MAX_SLOTS' in lib.ct_last_error()
    torch.cuda.synchronize()
    assert bool((loss == SENT).all()) and bool((grad == SENT).all())
    # (the same descriptor with one slot fewer is accepted)
    _keep[0].M = R.MAX_SLOTS
    assert lib.ct_generic_loss_workspace_bytes(ctypes.byref(d)) > 0


# ---------------------------------------------------------------------------------------------------------------------
# A4: fifteen heads in one launch

def _fused(out, batch, heads, device, needs=None):
    """{head: (loss, gradient or None)} of ONE fused call; ``needs``: the heads whose logits require a gradient"""
    from centertrack_amd import losses
    xs = {h: out[h].to(device).requires_grad_(needs is None or h in needs) for h in heads}
    b = T._to(batch, device)
    vec = losses.fused_losses([losses.GenericLoss._spec(h, xs, b) for h in heads])
    wanted = [h for h in heads if xs[h].requires_grad]
    grads = dict(zip(wanted, torch.autograd.grad(vec, [xs[h] for h in wanted], torch.ones_like(vec))))
    return {h: (vec[i].detach(), grads.get(h)) for i, h in enumerate(heads)}


@pytest.fixture(scope='module')
def alone(device):
    """every head of A4 run alone"""
    out, batch = R.fifteen_batch()
    return {h: _fused(out, batch, (h,), device)[h] for h in R.FIFTEEN}


@pytest.mark.parametrize('case', ['in order', 'reversed', 'only the last needs a gradient', 'all but the last need a gradient',
                                  'reversed, only the last needs a gradient', 'reversed, all but the last need a gradient'])
def test_fifteen_heads_in_one_launch_equal_each_head_alone(device, alone, case):
    from centertrack_amd import _lib, losses
    assert sorted(R.FIFTEEN) == sorted(losses.KNOWN_HEADS) and len(R.FIFTEEN) <= _lib.CT_LOSS_MAX_HEADS
    out, batch = R.fifteen_batch()
    T._assert_away_from_the_clamp(out)
    heads = R.FIFTEEN[::-1] if case.startswith('reversed') else R.FIFTEEN
    needs = None
    if 'only the last' in case:
        needs = heads[-1:]
    elif 'all but the last' in case:
        needs = heads[:-1]
    got = _fused(out, batch, heads, device, needs)
    for h in heads:
        assert torch.equal(got[h][0], alone[h][0]), (h, float(got[h][0]), float(alone[h][0]))
        if needs is None or h in needs:
            assert torch.equal(got[h][1], alone[h][1]), h
        else:
            assert got[h][1] is None


def test_fifteen_heads_against_the_float64_mirror(device, alone):
    """(what the fused launches are equal to is right)"""
    out, batch = R.fifteen_batch()
    want, e32 = R.truth_and_e32('fifteen', out, batch, R.FIFTEEN)
    T.compare('fifteen', alone, want, e32, R.FIFTEEN, out, batch)


# ---------------------------------------------------------------------------------------------------------------------
# A5: input types

@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float64], ids=lambda d: str(d).split('.')[1])
def test_logits_of_other_types_give_the_float32_loss_and_a_gradient_of_their_type(device, dtype):
    from centertrack_amd import losses
    heads = ('hm', 'reg', 'dep')
    out, batch = R.make_batch(45, 2, 8, 12, 8, heads, 3)
    b = T._to(batch, device)
    b['hm'] = b['hm'].half()
    leaves = {h: out[h].to(device).to(dtype).requires_grad_() for h in heads}
    as32 = {h: leaves[h].detach().float().requires_grad_() for h in heads}          # the same values as float32
    b32 = dict(b, hm=b['hm'].float())
    res = {}
    for key, xs, bb in (('typed', leaves, b), ('f32', as32, b32)):
        vec = losses.fused_losses([losses.GenericLoss._spec(h, xs, bb) for h in heads])
        vec.backward(torch.ones_like(vec))
        res[key] = vec.detach()
    assert res['typed'].dtype == torch.float32 and torch.equal(res['typed'], res['f32'])
    for h in heads:
        g, g32 = leaves[h].grad, as32[h].grad
        assert g.dtype == dtype and g32.dtype == torch.float32 and float(g32.abs().max()) > 0
        assert torch.equal(g, g32.to(dtype)), h
