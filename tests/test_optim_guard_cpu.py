"""CPU: the guarded optimizer step without a GPU -- ``optim.reference_guard`` and the guarded
``reference_step`` against ``torch.nn.utils.clip_grad_norm_`` followed by torch's own optimizers, the coefficient and skip
rules on known answers, three mutations of the rule that those answers catch, ``ct_optim_guard`` against the header, the
argument refusals of ``ct_optim_norms`` / ``ct_optim_step_guarded`` on fake pointers, the workspace size, and the host side
of ``optimizer.guard`` / ``get_optimizer`` / ``Trainer``."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import _optim as T
import _optim_guard as G


# ------------------------------------------------------------------ reference_guard + reference_step against torch
@pytest.mark.parametrize('wd', [0, 1e-4])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_reference_guard_is_torchs_clip_then_step(kind, wd):
    """Five steps on float64 CPU tensors, two groups, tensor 3 without a gradient on steps 2 and 4; max_norm = 5 against
    norms of about 40, and step 3 with gradients 100 times smaller so that the clamp at 1 is taken too.

    torch forms ``max_norm / (total_norm + 1e-6)`` as ``(total_norm + 1e-6).reciprocal() * max_norm``: two roundings where
    the rule divides once.  With u = 2^-53: reciprocal (1 + d1), product (1 + d2), division (1 + d3), |d| <= u, so the two
    coefficients differ by at most 3 u relative (plus O(u^2): 3.5 u asserted).  And the total norm: torch takes the norm
    of the per-tensor norms, numpy adds the N squares pairwise.  Any order of N non-negative terms is within (N - 1) u of
    the exact sum, two orders within 2 (N - 1) u of each other, halved by the square root, plus torch's per-tensor roots
    and squares (3 u) and the two last roots (u): (N + 4) u asserted.  That is the whole difference: fed torch's own
    coefficient, ``reference_step`` reproduces torch's parameters and state bit for bit over the five steps."""
    from centertrack_amd import optim as O
    sizes = [1, 2, 27, 64, 512, 1000]
    N = sum(sizes)
    max_norm = 5.0
    rs = np.random.RandomState(9)
    tensors = [torch.tensor(rs.randn(n)).requires_grad_() for n in sizes]
    mine = [t.detach().numpy().copy() for t in tensors]
    states = [{} for _ in sizes]
    kw = dict(T.HYPER[kind], weight_decay=wd)
    lrs = [1e-2] * 3 + [3e-3] * 3
    opt = T.torch_class(kind)([dict(params=tensors[:3], lr=1e-2, **kw), dict(params=tensors[3:], lr=3e-3, **kw)],
                              foreach=False)
    clipped = 0
    for step in range(5):
        grads = [None if (i == 3 and step in (1, 3)) else rs.randn(n) * (0.01 if step == 2 else 1.0)
                 for i, n in enumerate(sizes)]
        for t, g in zip(tensors, grads):
            t.grad = None if g is None else torch.tensor(g)
        total = G.clip_(tensors, max_norm)
        theirs = torch.clamp(max_norm / (total + 1e-6), max=1.0)              # clip_grad_norm_'s own lines
        own = O.reference_guard(grads, max_norm)
        assert abs(own['norm'] - float(total)) <= (N + 4) * G.U53 * float(total), step
        fed = O.reference_guard(grads, max_norm, norm=float(total))
        assert fed['coef'].dtype == np.float64 and own['nonfinite'] == 0 and not own['skip']
        assert abs(float(fed['coef']) - float(theirs)) <= 3.5 * G.U53 * float(theirs), step
        assert abs(float(own['coef']) - float(theirs)) <= (N + 8) * G.U53 * float(theirs), step
        assert (float(theirs) == 1.0) == (step == 2) == (float(own['coef']) == 1.0)
        clipped += float(own['coef']) < 1.0
        fed['coef'] = np.float64(float(theirs))
        for i, g in enumerate(grads):
            if g is not None:
                O.reference_step(kind, mine[i], g, states[i], dict(kw, lr=lrs[i]), guard=fed)
        opt.step()
        for i, t in enumerate(tensors):
            assert np.array_equal(t.detach().numpy(), mine[i]), (step, i)
            for k in T.STATE_KEYS[kind]:
                assert np.array_equal(opt.state[t][k].numpy(), states[i][k]), (step, i, k)
    assert clipped == 4


# ------------------------------------------------------------------ the coefficient rule
def test_the_coefficient_rule_on_known_answers():
    from centertrack_amd import optim as O
    zero = O.reference_guard([np.zeros(5, np.float32), np.zeros(1, np.float32)], 1.0)
    assert zero['norm'] == 0.0 and zero['sumsq'] == 0.0 and zero['coef'] == 1.0 and not zero['skip']     # 1 / 1e-6, clamped
    below = O.reference_guard([np.array([3.0, 0.0], np.float32), np.array([4.0], np.float32)], 10.0)
    assert below['norm'] == 5.0 and below['sumsq'] == 25.0 and below['per_tensor'] == [9.0, 16.0] and below['coef'] == 1.0
    four = O.reference_guard([np.array([3.0, 0.0], np.float32), None, np.array([4.0], np.float32)], 1.25)
    assert four['norm'] == 5.0 and float(four['coef']) == 1.25 / 5.000001 == 0.24999995000001 and four['coef'] != 0.25
    four32 = O.reference_guard([np.array([3.0, 4.0], np.float32)], 1.25, dtype=np.float32)
    assert four32['coef'].dtype == np.float32 and four32['coef'] == np.float32(0.24999995000001)
    assert four32['coef'] == np.float32(0.24999995) != np.float32(0.25)
    for off in (None, 0, 0.0, -1.0):
        r = O.reference_guard([np.array([3.0, 4.0], np.float32)], off)
        assert r['coef'] == 1.0 and r['norm'] == 5.0 and not r['skip']
    # values of 1e30 do not overflow the double sum; 1e-30 does not vanish in it
    big = O.reference_guard([np.full(4, 1e30, np.float32), np.full(3, 1e-30, np.float32)], 1.0)
    assert np.isfinite(big['norm']) and big['per_tensor'][1] > 0.0 and 0.0 < big['coef'] < 1e-29


def test_the_skip_rule_and_the_first_sgd_buffer():
    from centertrack_amd import optim as O
    good = [np.array([1.0, -2.0, 0.5], np.float32), np.array([0.25], np.float32)]
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = [good[0].copy(), good[1].copy()]
        bad[0][1] = bad_value
        r = O.reference_guard(bad, 1.0, skip_nonfinite=True)
        assert r['nonfinite'] == 1 and r['skip'] and r['coef'] == 1.0 and not np.isfinite(r['norm'])
        r = O.reference_guard(bad, 1.0, skip_nonfinite=False)                  # counted, not skipped, not clipped either
        assert r['nonfinite'] == 1 and not r['skip'] and r['coef'] == 1.0
    skip = O.reference_guard([np.array([np.nan, np.inf], np.float32)], None, skip_nonfinite=True)
    assert skip['nonfinite'] == 2 and skip['skip']
    # Adam: nothing moves, the host's step count advances
    p, st = np.array([1.0, 2.0]), {}
    O.reference_step('adam', p, np.array([np.nan, 1.0]), st, dict(lr=0.1), guard=skip)
    assert p.tolist() == [1.0, 2.0] and st['step'] == 1 and not st['exp_avg'].any() and not st['exp_avg_sq'].any()
    # SGD: the skipped first step leaves a buffer of zeros, and the step after it is torch's first step
    hyper = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    p, st = np.array([1.0, 2.0, -3.0]), {}
    O.reference_step('sgd', p, np.array([np.nan, 1.0, 1.0]), st, hyper, guard=skip)
    assert p.tolist() == [1.0, 2.0, -3.0] and st['momentum_buffer'].tolist() == [0.0, 0.0, 0.0]
    g = np.array([0.5, -0.25, 2.0])
    O.reference_step('sgd', p, g, st, hyper, guard=O.reference_guard([g], 100.0, skip_nonfinite=True))
    t = torch.tensor([1.0, 2.0, -3.0], dtype=torch.float64, requires_grad=True)
    theirs = torch.optim.SGD([t], foreach=False, **hyper)
    t.grad = torch.tensor(g)
    theirs.step()
    assert np.array_equal(p, t.detach().numpy()) and np.array_equal(st['momentum_buffer'], theirs.state[t]['momentum_buffer'].numpy())
    # without momentum a skipped step creates nothing
    p, st = np.array([1.0]), {}
    O.reference_step('sgd', p, np.array([np.inf]), st, dict(lr=0.1), guard=skip)
    assert p.tolist() == [1.0] and st == {}
    with pytest.raises(O.CTError):
        O.reference_step('rmsprop', p, p, {}, dict(lr=1.0), guard=skip)


def test_three_mutations_of_the_rule_fail_the_known_answers():
    """the known answers above have teeth: the rule without its 1e-6, without its clamp, and with the skipped first SGD step
    leaving no buffer each miss one of them"""
    from centertrack_amd import optim as O
    g = [np.array([3.0, 4.0], np.float32)]
    assert float(O.reference_guard(g, 1.25)['coef']) == 0.24999995000001
    assert float(O.reference_guard(g, 1.25, eps=0.0)['coef']) == 0.25                        # 1e-6 dropped
    assert O.reference_guard(g, 10.0)['coef'] == 1.0
    assert float(O.reference_guard(g, 10.0, clamp=False)['coef']) == 10.0 / 5.000001 > 1.9    # clamp dropped: gradients grow
    zeros = [np.zeros(3, np.float32)]
    assert O.reference_guard(zeros, 1.0)['coef'] == 1.0
    with np.errstate(divide='ignore'):
        assert not np.isfinite(O.reference_guard(zeros, 1.0, eps=0.0, clamp=False)['coef'])
    hyper = dict(lr=0.1, momentum=0.9)
    skip = O.reference_guard([np.array([np.nan], np.float32)], None, skip_nonfinite=True)
    for zero_first in (True, False):
        p, st = np.array([1.0]), {}
        O.reference_step('sgd', p, np.array([np.nan]), st, hyper, guard=skip, zero_first=zero_first)
        assert ('momentum_buffer' in st) == zero_first
        if not zero_first:
            st['momentum_buffer'] = np.array([7.0])              # what an uninitialised buffer may hold
        O.reference_step('sgd', p, np.array([0.5]), st, hyper)
        assert (p[0] == 1.0 - 0.1 * 0.5) == zero_first          # torch's first step: m = g


# ------------------------------------------------------------------ the C side
def test_guard_struct_matches_the_header_layout(tmp_path):
    import shutil
    import subprocess
    from centertrack_amd import _lib, optim as O
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = G.GUARD_FIELDS
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "centertrack_hip.h"\nint main(void) {'
                   'printf("%zu' + ' %zu' * len(fields) + '\\n", sizeof(ct_optim_guard), '
                   + ', '.join('offsetof(ct_optim_guard, %s)' % f for f in fields) + '); return 0; }\n')
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(T.ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    D = _lib.OptimGuard
    assert [f for f, _ in D._fields_] == list(fields) == list(O.GUARD.names)
    assert got[0] == ctypes.sizeof(D) == O.GUARD.itemsize == 80 <= O.GUARD_SLOT and O.GUARD_SLOT % 16 == 0
    assert got[1:] == [getattr(D, f).offset for f in fields] == [O.GUARD.fields[f][1] for f in fields]
    # what guard_counters slices: norm_sum, then steps .. nonfinite_steps
    assert O.GUARD.fields['norm_sum'][1] == 16 and O.GUARD.fields['steps'][1] == 40 and O.GUARD.fields['coef'][1] == 72
    assert O.GUARD.fields['norm'][1] == 8


def test_argument_checks_without_gpu():
    """ct_optim_norms and ct_optim_step_guarded refuse before they enqueue anything"""
    from centertrack_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.int32)
    ptr = buf.ctypes.data
    ptr += (-ptr) % 16
    A, S = _lib.CT_OPTIM_ADAM, _lib.CT_OPTIM_SGD

    def norms(table=ptr, n=4, chunks=4, max_norm=1.0, skip=1, per=None, guard=ptr, ws=ptr, ws_bytes=1 << 12):
        return lib.ct_optim_norms(table, n, chunks, max_norm, skip, per, guard, ws, ws_bytes, None)

    def rejected(rc, what, who):
        assert rc == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error() and who in lib.ct_last_error(), lib.ct_last_error()

    who = b'ct_optim_norms:'
    rejected(norms(table=None), b'null table', who)
    rejected(norms(n=0), b'tensors outside', who)
    rejected(norms(n=-3), b'tensors outside', who)
    rejected(norms(n=_lib.CT_OPTIM_MAX_TENSORS + 1, chunks=1 << 21), b'tensors outside', who)
    rejected(norms(chunks=3), b'chunks', who)
    rejected(norms(chunks=1 << 31), b'chunks', who)
    rejected(norms(guard=None), b'null guard', who)
    rejected(norms(ws=None), b'null workspace', who)
    rejected(norms(ws_bytes=16 * 8 - 1), b'127 bytes, 128 needed', who)
    rejected(norms(ws_bytes=0), b'needed', who)
    rejected(norms(max_norm=float('nan')), b'NaN', who)
    rejected(norms(ws=ptr + 4), b'16-byte aligned', who)
    who = b'ct_optim_step_guarded:'
    step = lib.ct_optim_step_guarded
    rejected(step(None, 1, 1, A, ptr, None), b'null table', who)
    rejected(step(ptr, 0, 1, A, ptr, None), b'tensors outside', who)
    rejected(step(ptr, _lib.CT_OPTIM_MAX_TENSORS + 1, 1 << 21, S, ptr, None), b'tensors outside', who)
    rejected(step(ptr, 4, 3, A, ptr, None), b'chunks', who)
    rejected(step(ptr, 4, 1 << 31, A, ptr, None), b'chunks', who)
    rejected(step(ptr, 4, 4, 2, ptr, None), b'kind 2', who)
    rejected(step(ptr, 4, 4, -1, ptr, None), b'kind -1', who)
    rejected(step(ptr, 4, 4, A, None, None), b'null guard', who)
    rejected(step(ptr, 4, 4, S, None, None), b'null guard', who)


@pytest.mark.parametrize('which', ['list', 'dlaseg'])
def test_workspace_bytes(which):
    """16 bytes per chunk and per tensor, from the library and from its restatement: for every size alone, for every
    prefix of the list and for the whole list; 0 for what the calls refuse"""
    from centertrack_amd import _lib, optim as O
    lib = _lib.load()
    sizes = T.SIZES if which == 'list' else T.dlaseg_sizes()
    assert len(sizes) == (10 if which == 'list' else 243)
    chunks_of = [(s + O.CHUNK - 1) // O.CHUNK for s in sizes]
    for c in chunks_of:
        assert lib.ct_optim_norms_workspace_bytes(1, c) == O.norms_workspace_bytes(1, c) == 16 * (c + 1)
    for n in range(1, len(sizes) + 1):
        c = sum(chunks_of[:n])
        assert lib.ct_optim_norms_workspace_bytes(n, c) == O.norms_workspace_bytes(n, c) == 16 * (c + n)
    if which == 'dlaseg':
        assert sum(chunks_of) == 5003 and O.norms_workspace_bytes(243, 5003) == 83936
    for n, c in ((0, 1), (-1, 5), (3, 2), (1, 1 << 31), (_lib.CT_OPTIM_MAX_TENSORS + 1, 1 << 21)):
        assert lib.ct_optim_norms_workspace_bytes(n, c) == O.norms_workspace_bytes(n, c) == 0
    assert lib.ct_optim_norms_workspace_bytes(1, (1 << 31) - 1) == 16 * (1 << 31)          # does not wrap at 32 bits


# ------------------------------------------------------------------ the host side of the classes
def cpu_params():
    torch.manual_seed(3)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def test_guard_switches_on_and_off():
    from centertrack_amd import optim as O
    for cls in (O.Adam, O.SGD):
        opt = cls(cpu_params(), lr=1e-3)
        assert opt.guard(max_norm=2.5) is opt and opt._guard == (2.5, False)
        assert opt.guard(skip_nonfinite=True)._guard == (0.0, True)
        assert opt.guard(1, True)._guard == (1.0, True)
        assert opt.guard()._guard is None and opt.guard(None, False)._guard is None
        assert opt.guard(0)._guard is None and opt.guard(-3.0)._guard is None        # max_norm <= 0: no clipping
        assert opt.guard(-3.0, True)._guard == (0.0, True)
        with pytest.raises(O.CTError, match='NaN'):
            opt.guard(float('nan'))
        assert opt.guard_counters() is None
        with pytest.raises(O.CTError, match='no guarded step'):
            opt.grad_stats()
        # the state dict knows nothing of the guard
        assert set(opt.state_dict()) == {'state', 'param_groups'}
        assert 'max_norm' not in opt.defaults and all('max_norm' not in g for g in opt.param_groups)
    with pytest.raises(O.CTError, match='CUDA float32'):
        O.grad_norms([torch.ones(3)])
    with pytest.raises(O.CTError, match='no gradient'):
        O.grad_norms([torch.nn.Parameter(torch.ones(3))])


def test_get_optimizer_and_trainer_read_the_options():
    from centertrack_amd import optim as O, trainer as TR
    from centertrack_amd._lib import CTError
    ns = types.SimpleNamespace
    assert O.guard_options(ns()) == (None, False)
    assert O.guard_options(ns(max_grad_norm=35.0)) == (35.0, False)
    assert O.guard_options(ns(max_grad_norm=0, skip_nonfinite=1)) == (None, True)
    assert O.guard_options(ns(max_grad_norm=-1.0)) == (None, False)
    model = torch.nn.Linear(3, 2)
    assert O.get_optimizer(ns(optim='adam', lr=1e-4), model).__dict__.get('_guard') is None
    a = O.get_optimizer(ns(optim='adam', lr=1e-4, max_grad_norm=35.0), model)
    assert type(a) is O.Adam and a._guard == (35.0, False)
    s = O.get_optimizer(ns(optim='sgd', lr=1e-2, skip_nonfinite=True), model)
    assert type(s) is O.SGD and s._guard == (0.0, True)
    # the options are not among the package's defaults
    from centertrack_amd.detector import default_opt
    d = default_opt({'hm': 1})
    assert not hasattr(d, 'max_grad_norm') and not hasattr(d, 'skip_nonfinite')
    # Trainer switches the guard of the optimizer it is given; torch's optimizers have none
    heads = {'hm': 1, 'reg': 2, 'wh': 2}
    opt = ns(heads=heads, weights={h: 1 for h in heads}, num_stacks=1, debug=0, num_iters=-1, print_iter=0, device='cpu')
    plain = O.Adam(model.parameters(), 1e-3)
    TR.Trainer(opt, model, plain)
    assert plain.__dict__.get('_guard') is None
    opt.max_grad_norm, opt.skip_nonfinite = 10.0, True
    TR.Trainer(opt, model, plain)
    assert plain._guard == (10.0, True)
    with pytest.raises(CTError, match='centertrack_amd.optim'):
        TR.Trainer(opt, model, torch.optim.SGD(model.parameters(), lr=0.1))
    TR.Trainer(opt, model, None)
