"""GPU: synchronised BatchNorm (centertrack_amd/csrc/bn_train.hip: ``ct_bn_merge_stats``, ``ct_bn_*_backward_apply``;
``parallel.all_gather_rows`` / ``sync_batchnorm``) against float64 ``F.batch_norm`` (+ res) + ReLU
autograd on the CONCATENATED batch.  Error measure and bound are the project's (tests/_dcn_bwd.py): ``err`` relative to the
tensor's maximum, ``bound(e32, K) = min(1e-3, 4 max(e32, 2^-23 sqrt(K)))`` with e32 torch's own float32 error on the same data
and K the pixels of all shards.  The shifted channel (tests/_sync_bn.py) is held a second time against its own maximum: in
``gz`` the whole tensor's maximum belongs to the std-0.01 channel and hides everything else
(tests/test_sync_bn_cpu.py::test_local_backward_sums_miss_on_the_shifted_channel).

1. Emulated ranks: every shard in one process, the sums added in rank order.
2. A world of one row gives ``ct_bn_stats``' bits back.
3. The one-call backward equals its two halves fed its own sums and ``1.0f / P``, bit for bit.
4.-6. Two ranks over gloo on one GPU, ONE torchrun job (tests/_sync_bn_worker.py): the ops through a real group, the three
   BatchNorm sites, ``Trainer`` on ``DLASeg`` with ``opt.sync_bn``.
7. RCCL: world 1 with ``force=True``; world 2 where the box has two GPUs."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _neck_bwd as NB
import _sync_bn as SB
from _neck_bwd import bound, err

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
WORKER = os.path.join(ROOT, 'tests', '_sync_bn_worker.py')
C3 = SB.SHIFT_CHANNEL


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


_cases, _truths = {}, {}


def case_of(sl, form):
    key = (sl, form)
    if key not in _cases:
        _cases[key] = SB.sync_case(sl[0], sl[1], residual=form == 'backbone')
    return _cases[key]


def free_truth(sl, form):
    """(free64, free32): the references with their own ReLU masks, once per (shard list, form)"""
    key = (sl, form)
    if key not in _truths:
        _truths[key] = [SB.reference(case_of(sl, form), dt, form) for dt in (torch.float64, torch.float32)]
    return _truths[key]


# ------------------------------------------------------------------ 1. emulated ranks
@pytest.mark.parametrize('form', SB.FORMS)
@pytest.mark.parametrize('sl', SB.SHARD_LISTS, ids=SB.list_id)
def test_emulated_ranks(device, sl, form):
    """``y`` of the mean-100 / std-0.01 channel is what ``MergedStats.beta`` is for.  With the module's own beta, 2x33x65x8 1|1
    in the neck form measured err 3.59e-05 against a bound of 3.12e-05 on an MI355X, mean, var and invstd of the case being at
    1.4e-08, 3.7e-08, 5.4e-08: the merged mean is the float nearest to the true mean, 1.43e-06 away, and a = gamma * invstd =
    136.9 times that over max|y| is 3.59e-05 to three digits.  The merge knows the dropped part in double and folds it into
    beta; the kernels are the same."""
    shape, shards = sl
    N, H, W, C = shape
    P = N * H * W
    case = case_of(sl, form)
    rep = Report('sync bn %s %s' % (SB.list_id(sl), form))
    run = SB.emulate(case, shards, form, device)
    m = run['m']
    yh = SB.cat_nchw(run['y'])
    mask = yh > 0
    free64, free32 = free_truth(sl, form)
    t64, t32 = (SB.reference(case, dt, form, mask) for dt in (torch.float64, torch.float32))
    flipped, near = NB.check_mask(mask, free64['pre'], err(free32['y'], free64['y']), rep.title)
    print('%s: %d ReLU units flipped, %d within the threshold, of %d' % (rep.title, flipped, near, mask.numel()))
    if form == 'neck':
        assert not bool(mask[:, 2].any()) and bool((free64['pre'][:, 2] < 0).all())      # the all-negative channel
    rep.add('mean', m.mean, t64['mean'], t32['mean'], P)
    rep.add('var', m.var, t64['var'], t32['var'], P)
    assert float(m.var[1]) == 0.0 and float(m.mean[1]) == 3.0                             # the constant channel
    assert int(m.count) == P and float(m.inv_count) == float(np.float32(1.0 / P))
    unbiased64 = t64['var'] * P / (P - 1)
    rep.add('unbiased var', m.unbiased, unbiased64, t32['var'] * P / (P - 1), P)
    rep.add('invstd', m.invstd, torch.rsqrt(t64['var'] + SB.EPS), torch.rsqrt(t32['var'] + SB.EPS), P)
    rep.add('y', yh, free64['y'], free32['y'], P)
    rep.add('y, shifted channel', yh[:, C3], free64['y'][:, C3], free32['y'][:, C3], P)
    gz = SB.cat_nchw(run['gz'])
    rep.add('gz', gz, t64['gz'], t32['gz'], P)
    rep.add('gz, shifted channel', gz[:, C3], t64['gz'][:, C3], t32['gz'][:, C3], P)
    if form == 'backbone':
        rep.add('gres', SB.cat_nchw(run['gres']), t64['gres'], t32['gres'], P)
    # ggamma and gbeta stay per shard; their sum over the shards is the whole batch's
    total = run['total'].cpu()
    rep.add('sum of the shards\' ggamma', total[C:], t64['gg'], t32['gg'], P)
    rep.add('sum of the shards\' gbeta', total[:C], t64['gb'], t32['gb'], P)
    again = SB.emulate(case, shards, form, device)
    def everything(r):
        views = r['y'] + r['gz'] + (r['gres'] if form == 'backbone' else [])
        return [r['rows']] + SB.merged_vectors(r['m']) + r['sums'] + [r['total']] + [t.buf for t in views]
    first, second = everything(run), everything(again)
    assert len(first) == len(second) == 1 + 7 + len(shards) + 1 + (3 if form == 'backbone' else 2) * len(shards)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    rep.check()


@pytest.mark.parametrize('sl', SB.SHARD_LISTS, ids=SB.list_id)
def test_running_statistics_after_two_training_calls(device, sl):
    """the merged mean and the merged unbiased variance (total N) move the running statistics as one process on the whole batch
    would; ``num_batches_tracked`` counts the calls"""
    from centertrack_amd import _train, ops
    shape, shards = sl
    N, H, W, C = shape
    P = N * H * W
    zs = [case_of(sl, 'neck')[0], (NB.randn(41, N, C, H, W) * 2 + 1).float()]
    bn = torch.nn.BatchNorm2d(C, momentum=NB.MOMENTUM).to(device)
    for z in zs:
        rows = torch.empty((len(shards), ops.bn_row_floats(C)), dtype=torch.float32, device=device)
        for r, part in enumerate(SB.split(z, shards)):
            ops.bn_stats_row(SB.nhwc_view(part, device, C == 8), bn.eps, rows[r])
        m = ops.bn_merge_stats(rows, C, bn.eps)
        _train.update_running_stats_merged(bn, m.mean, m.unbiased)
    r64, r32 = SB.running_reference(zs, torch.float64), SB.running_reference(zs, torch.float32)
    rep = Report('sync bn running %s' % SB.list_id(sl))
    rep.add('running_mean', bn.running_mean, r64[0], r32[0], P)
    rep.add('running_var', bn.running_var, r64[1], r32[1], P)
    rep.add('running_var, shifted channel', bn.running_var[C3:C3 + 1], r64[1][C3:C3 + 1], r32[1][C3:C3 + 1], P)
    assert int(bn.num_batches_tracked) == 2
    rep.check()


def test_merge_is_reproducible_and_what_a_permutation_changes(device):
    """1|1|1: the same rows give the same bits; permuted rows may differ where the float64 sums round differently -- the
    observation is printed, only its size is held (one rounding to float: at most one unit in the last place)"""
    from centertrack_amd import ops
    sl = SB.SHARD_LISTS[2]
    assert sl[1] == (1, 1, 1)
    C = sl[0][3]
    run = SB.emulate(case_of(sl, 'neck'), sl[1], 'neck', device)
    rows = run['rows']
    a, b = ops.bn_merge_stats(rows, C, SB.EPS), ops.bn_merge_stats(rows.clone(), C, SB.EPS)
    for u, v in zip(SB.merged_vectors(a), SB.merged_vectors(b)):
        assert torch.equal(u, v)
    p = ops.bn_merge_stats(rows[[2, 0, 1]].contiguous(), C, SB.EPS)
    for name, u, v in zip(('mean', 'var', 'invstd', 'unbiased'), SB.merged_vectors(a), SB.merged_vectors(p)):
        differ = int((u.view(torch.int32) != v.view(torch.int32)).sum())
        print('merge of permuted rows, %-8s: %d of %d bit patterns differ' % (name, differ, C))
        ulp = torch.maximum(u.abs(), v.abs()) * 2.0 ** -22
        assert bool(((u - v).abs() <= ulp).all()), name
    assert torch.equal(a.count, p.count) and torch.equal(a.inv_count, p.inv_count)


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')], ids=['+inf', '-inf', 'nan'])
def test_merge_carries_non_finite_statistics(device, bad):
    """One non-finite value in one shard: that channel's merged variance, invstd, unbiased variance and shifted beta are NaN
    and its mean is not finite -- what ``ct_bn_stats`` on the whole batch and torch give -- and no other channel moves a bit.
    (A maximum against 0 that drops the NaN would leave var 0 and the finite invstd 1 / sqrt(eps).)"""
    from centertrack_amd import ops
    shape, shards = SB.SHARD_LISTS[1]
    N, H, W, C = shape
    case = SB.sync_case(shape, shards)
    gamma, beta = case[1].to(device), case[2].to(device)
    CH = 5

    def merged(z):
        rows = torch.empty((len(shards), ops.bn_row_floats(C)), dtype=torch.float32, device=device)
        for r, part in enumerate(SB.split(z, shards)):
            ops.bn_stats_row(SB.nhwc_view(part, device, False), SB.EPS, rows[r])
        return ops.bn_merge_stats(rows, C, SB.EPS, gamma=gamma, beta=beta)
    clean = merged(case[0])
    z = case[0].clone()
    z[N - 1, CH, 2, 3] = bad                                                  # in the last shard
    m = merged(z)
    whole = ops.bn_stats(SB.nhwc_view(z, device, False), SB.EPS)              # (mean, var, invstd) of one process
    for name, v in (('var', m.var), ('invstd', m.invstd), ('unbiased', m.unbiased), ('beta', m.beta)):
        assert bool(torch.isnan(v[CH])), (name, float(v[CH]))
    assert not bool(torch.isfinite(m.mean[CH]))
    assert bool(torch.isnan(whole[1][CH])) and bool(torch.isnan(whole[2][CH])) and not bool(torch.isfinite(whole[0][CH]))
    keep = torch.arange(C, device=device) != CH
    for u, v in zip(SB.merged_vectors(m), SB.merged_vectors(clean)):
        if u.numel() == C:
            assert torch.equal(u[keep].view(torch.int32), v[keep].view(torch.int32))
        else:
            assert torch.equal(u, v)                                          # the count and its reciprocal


# ------------------------------------------------------------------ 2. a world of one row
@pytest.mark.parametrize('shape', [s for s, _ in SB.SHARD_LISTS[:2]] + [SB.SHARD_LISTS[3][0], SB.SHARD_LISTS[4][0]], ids=str)
def test_one_row_gives_the_row_back(device, shape):
    from centertrack_amd import ops
    N, H, W, C = shape
    zv = SB.nhwc_view(SB.sync_case(shape, (N,))[0], device, C == 8)
    mean, var, invstd = ops.bn_stats(zv, SB.EPS)
    row = torch.empty(ops.bn_row_floats(C), dtype=torch.float32, device=device)
    invstd_row = ops.bn_stats_row(zv, SB.EPS, row)
    assert torch.equal(row[:C], mean) and torch.equal(row[C:2 * C], var) and torch.equal(invstd_row, invstd)
    assert row[3 * C:].view(torch.int64).tolist() == [N * H * W] * 2
    gamma, beta = (t.to(device) for t in SB.sync_case(shape, (N,))[1:3])
    m = ops.bn_merge_stats(row.view(1, -1), C, SB.EPS, gamma=gamma, beta=beta)
    assert torch.equal(m.beta.view(torch.int32), beta.view(torch.int32))          # one row: nothing dropped, beta as it is
    for name, u, v in (('mean', m.mean, mean), ('var', m.var, var), ('invstd', m.invstd, invstd)):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), name
    assert int(m.count) == N * H * W


# ------------------------------------------------------------------ 3. the paths that did not change
@pytest.mark.parametrize('shape', [SB.SHARD_LISTS[0][0], SB.SHARD_LISTS[1][0], SB.SHARD_LISTS[3][0]], ids=str)
def test_one_call_backward_equals_its_two_halves(device, shape):
    """``ct_bn_act_backward`` / ``ct_bn_relu_backward`` with every output against sums followed by the apply half fed the
    call's own sums and ``1.0f / P``: the split moved no bit of the existing entry points"""
    from centertrack_amd import ops
    N, H, W, C = shape
    P = N * H * W
    inv = torch.tensor([np.float32(1.0) / np.float32(P)], dtype=torch.float32, device=device)
    for form in SB.FORMS:
        sh = SB.Shard(SB.sync_case(shape, (N,), residual=form == 'backbone'), (N,), 0, form, device)
        mean, var, invstd = ops.bn_stats(sh.z, SB.EPS)
        if form == 'neck':
            gz, gg, gb = ops.bn_relu_backward(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta, True)
            sums = ops.bn_relu_backward_sums(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta)
            gz2, gr, gr2 = ops.bn_relu_backward_apply(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta, sums, inv), None, None
        else:
            gz, gr, gg, gb = ops.bn_act_backward(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta, True, res=sh.res, relu=True,
                                                 need_res=True)
            sums = ops.bn_act_backward_sums(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta, res=sh.res, relu=True)
            gz2, gr2 = ops.bn_act_backward_apply(sh.z, sh.gy, mean, invstd, sh.gamma, sh.beta, sums, inv, res=sh.res, relu=True,
                                                 need_z=True, need_res=True)
        assert torch.equal(sums[:C].view(torch.int32), gb.view(torch.int32)), form
        assert torch.equal(sums[C:].view(torch.int32), gg.view(torch.int32)), form
        assert torch.equal(SB.nchw(gz2).view(torch.int32), SB.nchw(gz).view(torch.int32)), form
        if gr is not None:
            assert torch.equal(SB.nchw(gr2).view(torch.int32), SB.nchw(gr).view(torch.int32)), form


# ------------------------------------------------------------------ the jobs
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def run_job(tmp, name, ranks, job, backend):
    out = os.path.join(str(tmp), name)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), WORKER, '--job', job, '--backend', backend, '--out', out]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    found = []
    for r in range(ranks):
        f = json.load(open('%s.%d.json' % (out, r)))
        f['tensors'] = torch.load('%s.%d.pt' % (out, r))
        found.append(f)
    assert [f['rank'] for f in found] == list(range(ranks)) and all(f['world'] == ranks for f in found)
    return found


@pytest.fixture(scope='module')
def world2(device, tmp_path_factory):
    return run_job(tmp_path_factory.mktemp('sync_bn'), 'world2', 2, 'world2', 'gloo')


@pytest.fixture(scope='module')
def world1(device, tmp_path_factory):
    return run_job(tmp_path_factory.mktemp('sync_bn'), 'world1', 1, 'world1', 'nccl')[0]


# ------------------------------------------------------------------ 4. the ops through a real group
def check_ops(found, backend):
    a, b = found
    assert a['backend'] == b['backend'] == backend
    assert len(a['ops']) == len(SB.TWO_RANK_LISTS) * len(SB.FORMS)
    for key in a['ops']:
        fa, fb = a['ops'][key], b['ops'][key]
        assert fa['merged'] == fb['merged'], key                              # the merged vectors: the same bits on both ranks
        assert fa['total'] == fb['total'], key                                # and the all-reduced sums
        for f in (fa, fb):
            assert f['merged'] == f['emulated_merged'] and f['total'] == f['emulated_total'], key
            assert f['mine'] == f['emulated_mine'], key                       # y, gz, gres of this rank's shard
        assert fa['mine'] != fb['mine'], key                                  # (the ranks hold different shards)


def test_ops_through_a_group_are_the_emulation(world2):
    check_ops(world2, 'gloo')


# ------------------------------------------------------------------ 5. the three sites
SITES = ('deform', 'block', 'stems')


def site_reference(site, sd, xs, G, dtype):
    """the torch-ops construction of the existing neck, backbone and stem tests on the CONCATENATED batch, training mode,
    loss = 0.5 * sum(out * G) -> dict(out, gin (list), grads {key: tensor}, buffers {key: tensor})"""
    import _backbone_bwd as BB
    import _stem_bwd as ST
    sdc = NB.cast(sd, dtype, grad=True)
    xt = [x.to(dtype).clone().requires_grad_() for x in xs]
    trace = NB.Trace()
    if site == 'deform':
        out = NB.deform(xt[0], sdc, '', True, trace)
    elif site == 'block':
        out = BB.basic_block(xt[0], sdc, '', 1, None, True, BB.Tape())
    else:
        tape = BB.Tape()
        out = sum(BB.stem(xt[s], sdc, ST.PREFIX[s], True, tape) for s in range(3))
    keys = [k for k in sdc if not NB.is_buffer(k)]
    gs = torch.autograd.grad(0.5 * (out * G.to(dtype)).sum(), xt + [sdc[k] for k in keys], allow_unused=True)
    return dict(out=out.detach(), gin=[g for g in gs[:len(xt)]], grads=dict(zip(keys, gs[len(xt):])),
                buffers={k: sdc[k].detach() for k in sdc if NB.is_buffer(k)}, trace=trace)


def check_site(found, site):
    """Marked, one sample per rank, against the same module unmarked in one process on the batch of two at weight 1/2; both
    sides are this package's kernels, e32 and the scale of every tensor come from the torch-ops references.

    The running means must NOT be those of the unsynchronised two-rank run.  The op tests shift one channel of one shard; here a
    convolution sits in front of every BatchNorm and mixes the channels, so the worker puts the whole of sample 1 of the first
    input at another scale and offset (``site_inputs``) and the assertion -- more than 1e-3 apart somewhere in every running
    mean -- stands in for "on the shifted channel".  For the ``pre_img`` and ``pre_hm`` stems, whose inputs are not rescaled,
    it rests on the two samples being different draws."""
    a, b = (f['tensors'][site] for f in found)
    sd, xs, G = a['sd'], a['inputs'], a['G']
    t64, t32 = (site_reference(site, sd, xs, G, dt) for dt in (torch.float64, torch.float32))
    K = int(xs[0].shape[0] * xs[0].shape[2] * xs[0].shape[3])
    rep = Report('sync bn site %s' % site)
    single = a['single']

    def hold(name, got, want, r64, r32, norm=None):
        norm = float(r64.abs().max()) if norm is None else norm
        e, e32 = err(got, want.double(), norm), err(r32, r64, norm)
        b_ = bound(e32, K)
        rep.rows.append((name, e, e32, b_))
        print('%s %-44s two ranks vs one process %.2e  (vs float64 %.2e)  e32 %.2e  bound %.2e%s'
              % (rep.title, name, e, err(got, r64, norm), e32, b_, '' if e <= b_ else '   <-- MISSES'))
    hold('out', torch.cat([a['out'], b['out']], 0), single['out'], t64['out'], t32['out'])
    for s in range(len(xs)):
        # the two-rank loss is sum(out_r * G_r) per rank, the one-process loss weighs the batch of two by 1/2
        hold('gin[%d]' % s, 0.5 * torch.cat([a['gin'][s], b['gin'][s]], 0), single['gin'][s], t64['gin'][s], t32['gin'][s])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k                   # averaged: the same on both ranks
        # (a conv bias ahead of batch statistics has the gradient 0: ``_neck_bwd.bias_norm`` is its yardstick)
        norm = NB.bias_norm(t64['trace'], k) if k == 'conv.bias' else None
        hold('grad ' + k, a['grads'][k], single['grads'][k], t64['grads'][k], t32['grads'][k], norm)
    moved = 0
    for k in a['buffers']:
        assert torch.equal(a['buffers'][k], b['buffers'][k]), k               # no broadcast, the same bits
        if k.endswith('num_batches_tracked'):
            assert int(a['buffers'][k]) == int(single['buffers'][k]) == 1
            continue
        hold('buffer ' + k, a['buffers'][k], single['buffers'][k], t64['buffers'][k], t32['buffers'][k])
        if k.endswith('running_mean'):
            # the unsynchronised two-rank run keeps per-rank statistics: rank 0's running mean is another one
            assert not torch.equal(a['buffers'][k], a['unsynced_buffers'][k]), k
            assert float((a['buffers'][k] - a['unsynced_buffers'][k]).abs().max()) > 1e-3, k
            moved += 1
    assert moved >= 1
    rep.check()


@pytest.mark.parametrize('site', SITES)
def test_site_on_two_ranks_is_one_process_on_the_whole_batch(world2, site):
    check_site(world2, site)


# ------------------------------------------------------------------ 6. Trainer on DLASeg
def check_trainer(found):
    a, b = (f['trainer'] for f in found)
    for f in (a, b):
        assert f['marked'] == f['n_bn'] > 40                                  # set_device marked every BatchNorm
        assert f['buffer_broadcasts'] == 0                                    # the epoch did not broadcast the buffers
        assert f['in_sync'] == 'ok', f['in_sync']
        assert all(np.isfinite(v) for v in f['ret'].values())
    assert a['after'] == b['after'] and a['after'] != a['before']             # parameters: bitwise equal across ranks
    assert a['buffers_after'] == b['buffers_after'] != a['buffers_before']    # and the buffers, without a broadcast
    assert a['ret'] == b['ret'] and list(a['ret'])[0] == 'tot'
    assert a['plain_buffers_after'] == b['plain_buffers_after']               # (sync_bn off: rank 0's, broadcast)
    assert a['plain_buffer_broadcasts'] == 1
    assert a['buffers_after'] != a['plain_buffers_after']
    # a NaN in rank 1's input: the guarded step skips on BOTH ranks, the parameters stay, the ranks stay equal
    assert a['nan_skipped'] == b['nan_skipped'] == 1
    assert a['nan_after'] == b['nan_after'] == a['after']
    for f in found:
        assert 'rank(s) [1] differ' in f['trainer']['buffers_out_of_sync'], f['trainer']['buffers_out_of_sync']


def test_trainer_with_sync_bn_on_two_ranks(world2):
    check_trainer(world2)


# ------------------------------------------------------------------ 7. RCCL
def test_world_1_forced_goes_through_rccl(world1):
    f = world1
    assert f['backend'] == 'nccl' and f['world'] == 1
    assert f['gathers'] > 0 and f['reduces'] > 0 and f['unforced_gathers'] == 0
    t = f['tensors']['world1']
    sd, xs, G = t['sd'], t['inputs'], t['G']
    t64, t32 = (site_reference('block', sd, xs, G, dt) for dt in (torch.float64, torch.float32))
    K = int(xs[0].shape[0] * xs[0].shape[2] * xs[0].shape[3])
    rep = Report('sync bn world 1 forced')

    def hold(name, got, want, r64, r32):
        e, e32 = err(got, want.double(), float(r64.abs().max())), err(r32, r64)
        rep.rows.append((name, e, e32, bound(e32, K)))
        print('%s %-40s forced vs unforced %.2e  e32 %.2e  bound %.2e' % (rep.title, name, e, e32, bound(e32, K)))
    hold('out', t['forced']['out'], t['plain']['out'], t64['out'], t32['out'])
    hold('gin', t['forced']['gin'][0], t['plain']['gin'][0], t64['gin'][0], t32['gin'][0])
    for k in t['forced']['grads']:
        hold('grad ' + k, t['forced']['grads'][k], t['plain']['grads'][k], t64['grads'][k], t32['grads'][k])
    for k in t['forced']['buffers']:
        if not k.endswith('num_batches_tracked'):
            hold('buffer ' + k, t['forced']['buffers'][k], t['plain']['buffers'][k], t64['buffers'][k], t32['buffers'][k])
    rep.check()


def test_world_2_on_rccl(device, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('one GPU: RCCL between two ranks needs two')
    found = run_job(tmp_path, 'world2_rccl', 2, 'world2', 'nccl')
    check_ops(found, 'nccl')
    for site in SITES:
        check_site(found, site)
    check_trainer(found)
