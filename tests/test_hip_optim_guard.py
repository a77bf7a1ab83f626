"""GPU: the guarded optimizer step (csrc/optim.hip: ``ct_optim_norms``, ``ct_optim_step_guarded``).

The norms against numpy's float64 sums with the textbook bound for two orders of N non-negative terms, bit-equal from run
to run and from one table to one table per tensor; the guarded step bit-equal to ``ct_optim_step`` when the norm is far
below ``max_norm``; clipping against torch's float64 ``clip_grad_norm_`` + optimizer with the bound of section 20; a NaN
and an Inf at four places leaving every bit of p, m, v alone; no host wait and no allocation in a guarded ``step()``;
``Trainer`` with the options against a hand-written loop.

Measured on an MI355X, largest error over bound: norms 0.0001; clipping: Adam 0.250 (weight decay 0) and 0.288 (1e-4), SGD
0.306 and 0.350; the step after two skipped steps: Adam 0.250, SGD 0.186."""
import functools

import numpy as np
import pytest
import torch

import _optim as T
import _optim_guard as G
from test_hip_optim import (BATCH_SIZES, SENTINEL, Arena, DeviceReads, lines, make_params, optim_class, residues, set_grads,
                            snapshot, tr_batches, tr_model, tr_opt)

pytestmark = pytest.mark.gpu

ALL_SIZES = T.SIZES + T.VIEW_SIZES + [G.BIG]


def bits(t):
    return t.detach().view(torch.int32)


def same_bits(a, b):
    return (a is None) == (b is None) and (a is None or torch.equal(bits(a), bits(b)))


def packed(garena_tensors, kind='sgd', others=None):
    """(device table, n, chunks) over the gradient tensors; p (never read by the norms) points at the gradient unless
    ``others`` gives [(p, m, v)] tensors"""
    from centertrack_amd import optim as O
    items = []
    for i, g in enumerate(garena_tensors):
        p, m, v = others[i] if others else (g, None, None)
        items.append((p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0,
                      g.numel(), (0.0, 0.0, 0.0) if kind == 'sgd' else (0.1, 0.999, 0.001, 0.01, 0.5, 1e-8, 0.0), 0))
    words, n, chunks = O.pack(O.KINDS[kind], items)
    return torch.from_numpy(words).to(garena_tensors[0].device), n, chunks


def guard_of(state):
    from centertrack_amd import optim as O
    return state[:O.GUARD.itemsize].cpu().numpy().view(O.GUARD)[0]


class NormBuffers(object):
    """guard + per-tensor sums and the workspace of one table, each between sentinels"""

    def __init__(self, device, n, chunks):
        from centertrack_amd import optim as O
        self.n = n
        self.arena = Arena(device, [O.GUARD.itemsize // 4, 2 * n, O.norms_workspace_bytes(n, chunks) // 4])
        self.guard, self.per, self.work = (t.view(torch.uint8) for t in self.arena.tensors)
        self.guard.zero_()
        assert self.guard.data_ptr() % 16 == 0 and self.per.data_ptr() % 8 == 0 and self.work.data_ptr() % 16 == 0

    def run(self, table, n, chunks, max_norm=0.0, skip=False):
        from centertrack_amd import ops
        ops.optim_norms(table, n, chunks, max_norm, skip, self.per, self.guard, self.work)
        return guard_of(self.guard), self.per.view(torch.float64).cpu().numpy().copy()


# ------------------------------------------------------------------ 1. norms
def test_norms_against_float64(device):
    """|S - S64| <= 2 N 2^-53 S64 per tensor and in total: both are sums of the same N non-negative doubles (every square
    of a float32 is exact in double) in two orders, each within (N - 1) 2^-53 of the exact sum"""
    from centertrack_amd import ops
    grads = G.norm_grads()
    sizes = ALL_SIZES
    garena = Arena(device, sizes, residues() + [0])
    garena.fill(grads)
    # p, m, v of an Adam table: never read, never written
    others = [Arena(device, sizes) for _ in range(3)]
    for a in others:
        a.fill([np.full(n, 0.5, np.float32) for n in sizes])
    table, n, chunks = packed(garena.tensors, 'adam', list(zip(*(a.tensors for a in others))))
    assert n == 13 and chunks > 2048 + 20
    before = [a.words.clone() for a in [garena] + others]
    buf = NormBuffers(device, n, chunks)
    g1, per1 = buf.run(table, n, chunks, max_norm=1.0)
    g2, per2 = buf.run(table, n, chunks, max_norm=1.0)
    torch.cuda.synchronize()
    assert buf.arena.untouched() and garena.untouched() and all(a.untouched() for a in others)
    assert all(torch.equal(b, a.words) for b, a in zip(before, [garena] + others))          # p, g, m, v: every bit
    want = [G.sumsq64(g) for g in grads]
    worst = 0.0
    for i, (got, w, g) in enumerate(zip(per1, want, grads)):
        tol = 2 * g.size * G.U53 * w
        assert abs(got - w) <= tol, (i, got, w)
        if tol:
            worst = max(worst, abs(got - w) / tol)
    assert per1[2] == 0.0 and want[2] == 0.0
    total = sum(want)                                                    # (dominated by the 1e30 tensors)
    N = sum(sizes)
    assert abs(g1['sumsq'] - total) <= 2 * N * G.U53 * total
    worst = max(worst, abs(g1['sumsq'] - total) / (2 * N * G.U53 * total))
    print('optim guard norms: largest error / bound %.4f' % worst)
    # the total is the per-tensor sums added in tensor order, exactly
    s = 0.0
    for x in per1:
        s += float(x)
    assert s == g1['sumsq']
    assert abs(g1['norm'] - np.sqrt(g1['sumsq'])) <= np.spacing(np.sqrt(g1['sumsq']))
    print('optim guard norms: norm == sqrt(sumsq) to the bit: %s' % (g1['norm'] == np.sqrt(g1['sumsq'])))
    assert g1['nonfinite'] == 0 and g1['skip'] == 0 and g1['steps'] == 1 and g2['steps'] == 2
    c = 1.0 / (g1['norm'] + 1e-6)
    assert g1['coef'] == np.float32(c) and g2['clipped'] == 2 and g2['skipped'] == 0
    assert g2['norm_sum'] == g1['norm'] + g1['norm'] and g2['norm_max'] == g1['norm']
    # two runs: every bit
    assert np.array_equal(per1.view(np.int64), per2.view(np.int64)) and g1['sumsq'].tobytes() == g2['sumsq'].tobytes()
    # one table per tensor (other grids, other chunk numbers): the same per-tensor bits
    for i, g in enumerate(garena.tensors):
        t1, n1, c1 = packed([g])
        b1 = NormBuffers(device, n1, c1)
        gi, pi = b1.run(t1, n1, c1)
        assert pi.view(np.int64)[0] == per1.view(np.int64)[i] and gi['sumsq'] == pi[0], i
        assert gi['coef'] == 1.0 and gi['clipped'] == 0                                       # max_norm = 0: no clipping
        assert b1.arena.untouched()
    # alignment does not change the bits either: the views' gradients at residue 0
    aligned = Arena(device, T.VIEW_SIZES)
    aligned.fill(grads[10:12])
    t2, n2, c2 = packed(aligned.tensors)
    _, p2 = NormBuffers(device, n2, c2).run(t2, n2, c2)
    assert np.array_equal(p2.view(np.int64), per1.view(np.int64)[10:12])
    # per_tensor is optional
    buf3 = NormBuffers(device, n, chunks)
    ops.optim_norms(table, n, chunks, 0.0, False, None, buf3.guard, buf3.work)
    assert guard_of(buf3.guard)['sumsq'].tobytes() == g1['sumsq'].tobytes()
    assert bool((buf3.per.view(torch.int32) == SENTINEL).all())


def test_grad_norms_without_an_optimizer(device):
    from centertrack_amd import optim as O
    grads = G.norm_grads()[:12]
    garena = Arena(device, T.SIZES + T.VIEW_SIZES, residues())
    garena.fill(grads)
    params = [torch.zeros(g.numel(), device=device).requires_grad_() for g in garena.tensors]
    for p, g in zip(params, garena.tensors):
        p.grad = g
    params[3].grad = None
    total, per = O.grad_norms(params)
    assert total.dtype == torch.float64 and total.is_cuda and per.shape == (11,)
    want = [np.sqrt(G.sumsq64(g)) for i, g in enumerate(grads) if i != 3]
    assert np.allclose(per.cpu().numpy(), want, rtol=1e-12, atol=0.0)
    assert np.isclose(float(total), np.sqrt(sum(w * w for w in want)), rtol=1e-12)
    total2, per2 = O.grad_norms([g for i, g in enumerate(garena.tensors) if i != 3])         # the gradients themselves
    assert torch.equal(per, per2) and torch.equal(total, total2) and garena.untouched()


# ------------------------------------------------------------------ 2. guard off in effect
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_a_large_max_norm_changes_no_bit(device, kind):
    _, grads = T.data()
    runs = []
    for guarded in (False, True):
        arena, tensors = make_params(device)
        garena = Arena(device, T.SIZES + T.VIEW_SIZES)
        opt = optim_class(kind)(T.groups(tensors, kind, 1e-4))
        if guarded:
            assert opt.guard(max_norm=1e9, skip_nonfinite=True) is opt           # the norm is about 6e5
        snaps = []
        for row in grads:
            set_grads(tensors, garena, row)
            opt.step()
            snaps.append(snapshot([opt], tensors, kind))
        assert arena.untouched() and garena.untouched()
        runs.append(snaps)
        if guarded:
            st = opt.grad_stats()
            assert st['steps'] == 5 and st['clipped'] == 0 and st['skipped'] == 0 and st['coef'] == 1.0 and not st['skip']
            assert 1e5 < st['norm'] < 1e7 and st['norm_max'] >= st['norm_mean'] > 0 and len(st['per_tensor']) == 12
    for step, (a, b) in enumerate(zip(*runs)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert all(same_bits(u, v) for u, v in zip(x, y)), (step, i)
    # guard() with both off: the unguarded step again
    assert opt.guard()._guard is None


# ------------------------------------------------------------------ 3. clipping
@pytest.mark.parametrize('wd', [0, 1e-4])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_clipped_steps_against_torchs_float64_trajectory(device, kind, wd):
    """T.data()'s gradients times 4 (norm about 2.4e6) against max_norm = 1e6 -- every step at least twice max_norm:
    asserted -- over five steps, with the bound of section 20: 4 max(e32, 2^-23) max|ref|, e32 torch's own float32 CPU
    trajectory with clip_grad_norm_.  The norm itself: torch's float64 norm and the device's add the same N exact
    squares in two orders, (N + 4) 2^-53 apart at most (tests/test_optim_guard_cpu.py derives it)."""
    ref64, norms64 = G.torch_clipped_trajectory(kind, wd, torch.float64)
    ref32, _ = G.torch_clipped_trajectory(kind, wd, torch.float32)
    assert all(nrm >= 2 * G.CLIP_MAX_NORM for nrm in norms64)
    _, grads = T.data()
    N = sum(T.SIZES + T.VIEW_SIZES)
    arena, tensors = make_params(device)
    garena = Arena(device, T.SIZES + T.VIEW_SIZES)
    opt = optim_class(kind)(T.groups(tensors, kind, wd)).guard(max_norm=G.CLIP_MAX_NORM)
    names = ('p',) + T.STATE_KEYS[kind]
    worst = [0.0]
    for step, row in enumerate(grads):
        set_grads(tensors, garena, [None if g is None else g * np.float32(G.CLIP_SCALE) for g in row])
        before = [g.clone() for g in garena.tensors]
        opt.step()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, garena.tensors))     # gradients are not scaled in place
        st = opt.grad_stats()
        assert abs(st['norm'] - norms64[step]) <= (N + 4) * G.U53 * norms64[step] and st['clipped'] == step + 1
        assert st['coef'] == np.float32(G.CLIP_MAX_NORM / (st['norm'] + 1e-6)) < 0.5
        snap = snapshot([opt], tensors, kind)
        for i, (got, want64, want32) in enumerate(zip(snap, ref64[step], ref32[step])):
            for name, g, w64, w32 in zip(names, got, want64, want32):
                assert (g is None) == (w64 is None), (step, i, name)
                if g is not None:
                    T.check_against(g.double().cpu().numpy(), w64, w32, '%s wd %g step %d tensor %d %s'
                                    % (kind, wd, step + 1, i, name), worst)
    assert arena.untouched() and garena.untouched()
    print('optim guard clipping: %s weight_decay %g: largest error / bound %.3f' % (kind, wd, worst[0]))
    assert worst[0] > 0.0


# ------------------------------------------------------------------ 4. skip
SKIP_SIZES = T.SIZES + T.VIEW_SIZES + [G.BIG]
# (tensor, element): the first element of all; the last of a tensor whose size is no multiple of 4; inside a misaligned
# view; in a chunk past the 2048th workgroup (the big tensor's chunk 2048 is chunk 2048 + 33 of the table)
PLACES = {'first': (0, 0), 'last_ragged': (9, 70000), 'misaligned_view': (10, 517), 'past_the_grid': (12, 2048 * T.CHUNK + 1)}


SKIP_HYPER = {kind: dict(T.HYPER[kind], weight_decay=1e-4, lr=1e-2) for kind in ('adam', 'sgd')}


@functools.lru_cache(maxsize=None)
def skip_data():
    rs = np.random.RandomState(41)
    params = [rs.standard_normal(n).astype(np.float32) for n in SKIP_SIZES]
    grads = [[rs.standard_normal(n).astype(np.float32) for n in SKIP_SIZES] for _ in range(2)]
    return params, grads


@functools.lru_cache(maxsize=None)
def skip_reference(kind):
    """the emulation of warm-up step, two skipped steps, one step -- the host's step counts run on through the skips --
    in float64 and float32, unfused as the device computes: {dtype: [[p, state...] per tensor]}"""
    from centertrack_amd import optim as O
    params, grads = skip_data()
    skip, go = dict(skip=True, coef=1.0), dict(skip=False, coef=1.0)
    ref = {}
    for dt in (np.float64, np.float32):
        ref[dt] = []
        for i in range(len(SKIP_SIZES)):
            p, s = params[i].astype(dt), {}
            O.reference_step(kind, p, grads[0][i], s, SKIP_HYPER[kind], fused=False)
            O.reference_step(kind, p, grads[1][i], s, SKIP_HYPER[kind], fused=False, guard=skip)
            O.reference_step(kind, p, grads[1][i], s, SKIP_HYPER[kind], fused=False, guard=skip)
            O.reference_step(kind, p, grads[1][i], s, SKIP_HYPER[kind], fused=False, guard=go)
            ref[dt].append([p] + [s[k] for k in T.STATE_KEYS[kind]])
    return ref


@pytest.mark.parametrize('place', sorted(PLACES))
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_a_nonfinite_gradient_skips_the_step(device, kind, place):
    """one warm-up step, then a NaN step and an Inf step that must leave every bit of p, m, v alone, then a finite step
    that matches the float32 emulation of the same sequence (warm-up, two skips, step) within section 20's bound against
    the float64 emulation"""
    params, grads = skip_data()
    res = residues() + [0]
    arena = Arena(device, SKIP_SIZES, res)
    arena.fill(params)
    tensors = [t.requires_grad_() for t in arena.tensors]
    garena = Arena(device, SKIP_SIZES, res)
    opt = optim_class(kind)(tensors, **SKIP_HYPER[kind]).guard(max_norm=1e9, skip_nonfinite=True)
    ti, ei = PLACES[place]
    assert place != 'last_ragged' or (SKIP_SIZES[ti] % 4 != 0 and ei == SKIP_SIZES[ti] - 1)
    assert place != 'misaligned_view' or tensors[ti].data_ptr() % 16 != 0

    def step(row):
        set_grads(tensors, garena, row)
        opt.step()
    step(grads[0])
    keep = arena.words.clone()
    state = snapshot([opt], tensors, kind)
    for k, bad in enumerate((np.nan, np.inf)):
        row = [g.copy() for g in grads[1]]
        row[ti][ei] = bad
        step(row)
        st = opt.grad_stats()
        assert st['nonfinite'] == 1 and st['skip'] and st['skipped'] == k + 1 and st['coef'] == 1.0, (place, bad)
        assert st['steps'] == k + 2 and st['nonfinite_steps'] == k + 1 and st['clipped'] == 0
        assert torch.equal(keep, arena.words)                                           # p and the sentinels: every bit
        now = snapshot([opt], tensors, kind)
        assert all(same_bits(u, v) for a, b in zip(state, now) for u, v in zip(a, b))   # m, v
    step(grads[1])
    st = opt.grad_stats()
    assert st['nonfinite'] == 0 and not st['skip'] and st['skipped'] == 2 and st['steps'] == 4
    assert arena.untouched() and garena.untouched()
    if kind == 'adam':
        assert all(int(opt.state[p]['step']) == 4 for p in tensors)                     # the host counts every call
    names = ('p',) + T.STATE_KEYS[kind]
    worst = [0.0]
    ref = skip_reference(kind)
    got = snapshot([opt], tensors, kind)
    for i in range(len(SKIP_SIZES)):
        for name, g, w64, w32 in zip(names, got[i], ref[np.float64][i], ref[np.float32][i]):
            T.check_against(g.double().cpu().numpy(), w64, w32.astype(np.float64), '%s %s tensor %d %s' % (kind, place, i, name),
                            worst)
    print('optim guard skip: %s %s: largest error / bound %.3f' % (kind, place, worst[0]))


def test_sgd_skipped_on_its_very_first_step(device):
    """the momentum buffers, created by a step the device skips, are zeros (whatever the allocation held), and the step
    after it is torch's first step: m = g"""
    rs = np.random.RandomState(43)
    sizes = T.SIZES + T.VIEW_SIZES
    params = [rs.randn(n).astype(np.float32) for n in sizes]
    grads = [rs.randn(n).astype(np.float32) for n in sizes]
    arena, garena, marena = (Arena(device, sizes, residues()) for _ in range(3))
    arena.fill(params)
    marena.fill([np.full(n, 7.0, np.float32) for n in sizes])                   # what an uninitialised buffer may hold
    tensors = [t.requires_grad_() for t in arena.tensors]
    hyper = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt = optim_class('sgd')(tensors, **hyper).guard(skip_nonfinite=True)
    made = []
    real_empty_like = torch.empty_like

    def empty_like(t, **kw):                                                     # hand out the prepared buffers
        for p, m in zip(tensors, marena.tensors):
            if t is p or t.data_ptr() == p.data_ptr():
                made.append(m)
                return m
        return real_empty_like(t, **kw)
    torch.empty_like = empty_like
    try:
        bad = [g.copy() for g in grads]
        bad[5][100] = np.nan
        set_grads(tensors, garena, bad)
        keep = arena.words.clone()
        opt.step()
    finally:
        torch.empty_like = real_empty_like
    assert len(made) == len(sizes)
    st = opt.grad_stats()
    assert st['skip'] and st['skipped'] == 1 and st['nonfinite'] == 1
    assert torch.equal(keep, arena.words) and marena.untouched()
    assert all(bool((bits(opt.state[p]['momentum_buffer']) == 0).all()) for p in tensors)     # +0.0, every element
    set_grads(tensors, garena, grads)
    opt.step()
    assert not opt.grad_stats()['skip']
    # the float32 restatement of torch's first step, unfused as the device computes: the same values everywhere
    from centertrack_amd import optim as O
    for i, p in enumerate(tensors):
        q, s = params[i].copy(), {}
        O.reference_step('sgd', q, grads[i], s, hyper, fused=False)
        assert np.array_equal(p.detach().cpu().numpy(), q), i
        assert np.array_equal(opt.state[p]['momentum_buffer'].cpu().numpy(), s['momentum_buffer']), i
    # and torch's own first step, float32 on the CPU, whose vectorised kernels fuse g + wd p and p + (-lr) m: the exact
    # values differ by half an ulp of the product that the device rounds, then both sides round once
    cpu = [torch.tensor(p).requires_grad_() for p in params]
    theirs = torch.optim.SGD(cpu, foreach=False, **hyper)
    for t, g in zip(cpu, grads):
        t.grad = torch.tensor(g)
    theirs.step()
    for i, (p, t) in enumerate(zip(tensors, cpu)):
        m, tm = opt.state[p]['momentum_buffer'].cpu().numpy(), theirs.state[t]['momentum_buffer'].numpy()
        assert (np.abs(m - tm) <= np.spacing(np.abs(tm)) + np.spacing(np.float32(1e-4) * np.abs(params[i]))).all(), i
        got, want = p.detach().cpu().numpy(), t.detach().numpy()
        top = np.maximum(np.maximum(np.abs(want), np.abs(params[i])), np.float32(1e-2) * np.abs(tm))
        assert (np.abs(got - want) <= 2 * np.spacing(top)).all(), i
    assert arena.untouched() and marena.untouched() and garena.untouched()


# ------------------------------------------------------------------ 5. no waits, no allocations
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_a_guarded_step_neither_waits_nor_allocates(device, kind, monkeypatch):
    _, grads = T.data()
    arena, tensors = make_params(device)
    garena = Arena(device, T.SIZES + T.VIEW_SIZES)
    opt = optim_class(kind)(T.groups(tensors, kind, 1e-4)).guard(max_norm=1e5, skip_nonfinite=True)     # a norm of 6e5
    set_grads(tensors, garena, grads[0])
    torch.cuda.synchronize()
    reads = DeviceReads(monkeypatch)
    allocated = []
    for step in range(10):
        opt.step()
        allocated.append(torch.cuda.memory_stats(device)['allocation.all.allocated'])
    assert reads.n == 0
    assert len(set(allocated[2:])) == 1, allocated                       # from the third guarded step on: none
    st = opt.grad_stats()
    assert reads.n == 1
    assert st['steps'] == 10 and st['clipped'] == 10 and st['skipped'] == 0 and len(st['per_tensor']) == 12
    want = [np.sqrt(G.sumsq64(g)) for g in grads[0]]
    assert np.allclose(st['per_tensor'], want, rtol=1e-12, atol=0.0)
    # guard() with both off: the two enqueues of before, and still no wait
    opt.guard()
    reads.n = 0
    opt.step()
    assert reads.n == 0
    torch.cuda.synchronize()
    assert arena.untouched() and garena.untouched()


# ------------------------------------------------------------------ 6. Trainer
def run_trainer(device, monkeypatch, capsys, sd, nan_batch=None, **options):
    """Trainer.train over the four batches; ``nan_batch``: the batch in whose backward pass a hook plants a NaN"""
    from centertrack_amd import optim as O
    from centertrack_amd.trainer import Trainer
    opt = tr_opt(device, **options)
    model = tr_model(sd)
    adam = O.Adam(model.parameters(), 1e-3)
    tr = Trainer(opt, model, adam)
    tr.set_device([0], [2], device)
    plant(model, nan_batch)
    reads = DeviceReads(monkeypatch)
    ret, results = tr.train(1, tr_batches())
    n_reads = reads.n
    monkeypatch.undo()
    return ret, model, adam, n_reads, lines(capsys)


def plant(model, nan_batch):
    """a hook on the first parameter's gradient: element 0 becomes NaN in backward pass number ``nan_batch``"""
    if nan_batch is None:
        return
    first = next(model.parameters())
    calls = [0]

    def hook(grad):
        calls[0] += 1
        if calls[0] - 1 == nan_batch:
            grad = grad.clone()
            grad.view(-1)[0] = float('nan')
            return grad
        return None
    first.register_hook(hook)


def state_bits(model):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v).clone() for k, v in model.state_dict().items()}


def test_trainer_with_the_guard_options(device, monkeypatch, capsys):
    from centertrack_amd import optim as O
    from centertrack_amd.losses import GenericLoss
    from centertrack_amd.trainer import ModelWithLoss
    sd = {k: v.clone() for k, v in tr_model().state_dict().items()}
    MAX = 1e-2
    # the hand-written loop with the same guarded optimizer; the norms read after every step (this loop may wait)
    model = tr_model(sd).to(device)
    mwl = ModelWithLoss(model, GenericLoss(tr_opt(device))).train()
    adam = O.Adam(model.parameters(), 1e-3).guard(MAX, True)
    plant(model, 2)
    norms, skipped = [], 0
    for batch in tr_batches():
        for k in batch:
            if k != 'meta':
                batch[k] = batch[k].to(device=device, non_blocking=True)
        _, loss, stats = mwl(batch)
        adam.zero_grad()
        loss.mean().backward()
        adam.step()
        st = adam.grad_stats()
        if st['nonfinite']:
            skipped += 1
        else:
            norms.append(st['norm'])
    assert skipped == 1 and len(norms) == 3 and st['skipped'] == 1 and st['steps'] == 4
    with capsys.disabled():
        print('trainer guard: norms %s, clipped %d of 3' % (norms, st['clipped']))
    assert st['clipped'] >= 1
    hand = state_bits(model)
    capsys.readouterr()
    # Trainer with the options
    ret, model2, adam2, n_reads, out = run_trainer(device, monkeypatch, capsys, sd, nan_batch=2, max_grad_norm=MAX,
                                                   skip_nonfinite=True)
    assert n_reads == 1                                                          # one wait for the epoch
    assert ret['skipped'] == 1
    total = 0.0
    for x in norms:
        total += x
    assert ret['grad_norm'] == total / 3
    assert list(ret) == ['tot', 'hm', 'wh', 'reg', 'grad_norm', 'skipped', 'time']
    got = state_bits(model2)
    assert all(torch.equal(got[k], hand[k]) for k in hand)
    assert all(int(adam2.state[p]['step']) == len(BATCH_SIZES) for p in model2.parameters())
    assert len(out) == 1 and '|grad_norm %.4f ' % ret['grad_norm'] in out[0] and '|skipped 1 ' in out[0]
    # print_iter = 1: one read per iteration and one at the end, the mean norm on every line
    ret1, _, _, n_reads1, out1 = run_trainer(device, monkeypatch, capsys, sd, nan_batch=2, max_grad_norm=MAX,
                                             skip_nonfinite=True, print_iter=1)
    assert n_reads1 == len(BATCH_SIZES) + 1 and len(out1) == len(BATCH_SIZES) + 1
    assert all('|grad_norm ' in l for l in out1) and '|skipped' not in out1[0] and '|skipped 1 ' in out1[-1]
    assert ret1['grad_norm'] == ret['grad_norm'] and ret1['skipped'] == 1
    # without the options: today's Trainer, to the bit -- against a hand loop with an unguarded optimizer
    model3 = tr_model(sd).to(device)
    mwl3 = ModelWithLoss(model3, GenericLoss(tr_opt(device))).train()
    adam3 = O.Adam(model3.parameters(), 1e-3)
    for batch in tr_batches():
        for k in batch:
            if k != 'meta':
                batch[k] = batch[k].to(device=device, non_blocking=True)
        _, loss, _ = mwl3(batch)
        adam3.zero_grad()
        loss.mean().backward()
        adam3.step()
    plain = state_bits(model3)
    ret4, model4, adam4, n_reads4, out4 = run_trainer(device, monkeypatch, capsys, sd)
    assert n_reads4 == 1 and list(ret4) == ['tot', 'hm', 'wh', 'reg', 'time'] and len(out4) == 1 and 'grad_norm' not in out4[0]
    got4 = state_bits(model4)
    assert all(torch.equal(got4[k], plain[k]) for k in plain)
    assert adam4.__dict__.get('_guard') is None and adam4.guard_counters() is None
    assert any(not torch.equal(got4[k], got[k]) for k in got)                   # the guard did change the run
