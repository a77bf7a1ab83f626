"""CPU: synchronised BatchNorm without a device -- the merge formula in numpy float64 against float64
statistics of the whole batch, the strength of the data (every mutation of the merge and of the backward must miss by more
than the GPU tests could forgive), the marking of modules, and the refusals of the new C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import _neck_bwd as NB
import _sync_bn as SB

# the GPU tests' bound is min(1e-3, ...): a mutation that misses by more than the cap misses every bound they can compute
GPU_BOUND_CAP = 1e-3


def whole(z):
    z = z.double()
    return z.mean((0, 2, 3)).numpy(), z.var((0, 2, 3), unbiased=False).numpy()


def rel(got, want):
    """per channel, relative to the channel's own truth (absolute where that is 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))


def on_shifted(got, want):
    """the project's error measure (relative to the tensor's maximum) on the shifted channel"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return abs(got[SB.SHIFT_CHANNEL] - want[SB.SHIFT_CHANNEL]) / np.abs(want).max()


@pytest.mark.parametrize('sl', SB.SHARD_LISTS, ids=SB.list_id)
def test_reference_merge_is_the_statistics_of_the_whole_batch(sl):
    shape, shards = sl
    z = SB.sync_case(shape, shards)[0]
    mean, var, N = SB.reference_merge(SB.shard_rows(z, shards))
    m64, v64 = whole(z)
    assert N == shape[0] * shape[1] * shape[2]
    assert rel(mean, m64).max() <= 1e-12 and rel(var, v64).max() <= 1e-12, (rel(mean, m64).max(), rel(var, v64).max())
    assert var[1] == 0.0 and mean[1] == 3.0                                   # the constant channel
    assert abs(m64[0] - 100) < 0.01 and abs(np.sqrt(v64[0]) - 0.01) < 2e-3   # mean 100, std 0.01: held to the same bound above
    assert abs(m64[SB.SHIFT_CHANNEL]) > 10 and v64[SB.SHIFT_CHANNEL] > 100    # the shift is in the data


@pytest.mark.parametrize('sl', SB.SHARD_LISTS, ids=SB.list_id)
def test_mutations_of_the_merge_miss_on_the_shifted_channel(sl):
    shape, shards = sl
    z = SB.sync_case(shape, shards)[0]
    rows = SB.shard_rows(z, shards)
    m64, v64 = whole(z)
    _, var, _ = SB.reference_merge(rows, between=False)
    assert on_shifted(var, v64) > GPU_BOUND_CAP, on_shifted(var, v64)
    mean, var, _ = SB.reference_merge(rows, counts=False)
    if len(set(shards)) == 1:
        # equal shards: a plain average IS the weighted one -- nothing to catch, by arithmetic
        assert rel(mean, m64).max() <= 1e-12 and rel(var, v64).max() <= 1e-12
    else:
        assert on_shifted(mean, m64) > GPU_BOUND_CAP and on_shifted(var, v64) > GPU_BOUND_CAP, (on_shifted(mean, m64),
                                                                                                on_shifted(var, v64))


def test_the_unequal_lists_are_there():
    """the counts-ignored mutation is only caught where the shards differ in size"""
    assert sum(1 for _, shards in SB.SHARD_LISTS if len(set(shards)) > 1) >= 2


@pytest.mark.parametrize('sl', SB.SHARD_LISTS, ids=SB.list_id)
def test_local_backward_sums_miss_on_the_shifted_channel(sl):
    """The four small lists catch a forgotten all-reduce.  3x254x258x16 2|1 cannot, and is held to that statement: what the
    mutation changes is sum g / N and sum g xhat / N, which for a random gy shrink as 1 / sqrt(N); at N = 196 596 the miss is
    7.1e-05, under that list's own GPU bound of 4 * 2^-23 * sqrt(N) = 2.1e-04.  That list is there for the launch plan (slab
    count from the grid target, capped element-wise grid), not for this mutation."""
    shape, shards = sl
    z, gamma, _, _, _, gy = SB.sync_case(shape, shards)
    m64, v64 = whole(z)
    want = SB.backward_formula(z, gy, gamma, m64, v64, shards)
    # the formula is autograd's
    zz, gg = z.double().requires_grad_(), gamma.double()
    pre = torch.nn.functional.batch_norm(zz, None, None, gg, None, True, 0.1, SB.EPS)
    auto, = torch.autograd.grad(pre, zz, gy.double())
    assert float((want - auto).abs().max() / auto.abs().max()) <= 1e-10
    got = SB.backward_formula(z, gy, gamma, m64, v64, shards, local_sums=True)
    # Relative to the maximum of the WHOLE tensor this mutation is invisible: channel 0 (std 0.01) has a = gamma * invstd of
    # order 100 and owns that maximum, the shifted channel (std 25) has a of order 0.04 (measured: a miss of 9e-7 at 2x5x7x64).
    # So the GPU tests hold the shifted channel of gz a second time against its OWN maximum, and this is that measure.
    c = SB.SHIFT_CHANNEL
    miss = float((got[:, c] - want[:, c]).abs().max() / want[:, c].abs().max())
    if sl == SB.SHARD_LISTS[4]:
        assert 0.0 < miss < NB.bound(0.0, shape[0] * shape[1] * shape[2]), miss
        return
    assert miss > GPU_BOUND_CAP, miss


@pytest.mark.parametrize('sl', SB.SHARD_LISTS[:4], ids=SB.list_id)
def test_why_the_row_carries_the_residual_of_the_mean(sl):
    """The figures of DESIGN.md section 32, reproducible: the float rows of ``ct_bn_stats_row`` restated in numpy, merged with
    and without the resid column.  Without it the invstd of the mean-100 / std-0.01 channel is off by parts in 1e6 of the
    largest invstd (measured on an MI355X: 1.19e-6, 9.9e-7, 3.98e-6 at the first three lists; this emulation: 1.20e-6, 9.6e-7,
    3.93e-6, 4.9e-7) -- at 1|1|1 half the GPU bound of 8.22e-6 before anything is computed with it; with it, the rounding of
    the variance to float is what remains.  (The largest list is left out: the emulation walks the pixels in Python.)  The
    second figure is ``beta_shifted``'s: y of that channel is off by a * |float(mean) - mean| with the module's beta."""
    shape, shards = sl
    case = SB.sync_case(shape, shards)
    z = case[0]
    rows = SB.fp32_rows(z, shards)
    m64, v64 = whole(z)
    inv64 = 1.0 / np.sqrt(v64 + SB.EPS)

    def invstd_err(var):
        inv = 1.0 / np.sqrt(var.astype(np.float32).astype(np.float64) + SB.EPS)
        return np.abs(inv - inv64).max() / inv64.max()
    plain, refined = invstd_err(SB.merge_fp32_rows(rows, False)[1]), invstd_err(SB.merge_fp32_rows(rows, True)[1])
    mean = SB.merge_fp32_rows(rows, True)[0]
    y64 = SB.reference(case, torch.float64, 'neck')['y']
    a0 = float(case[1][0]) * inv64[0]
    y_err = abs(a0) * abs(float(np.float32(mean[0])) - m64[0]) / float(y64.abs().max())
    print('%s: invstd off by %.2e without resid, %.2e with it; y off by %.2e from the rounding of the merged mean alone'
          % (SB.list_id(sl), plain, refined, y_err))
    assert refined <= 3e-7 and refined < plain                                # (2^-24 of the variance, and a little)
    if sl == SB.SHARD_LISTS[2]:
        assert plain > 3e-6                                                   # 1|1|1: what sent gz over its bound
    if sl == SB.SHARD_LISTS[3]:
        assert 3.4e-5 < y_err < 3.8e-5 and y_err > NB.bound(0.0, shape[0] * shape[1] * shape[2])     # measured: 3.59e-05


# ---------------------------------------------------------------------------------------------------------------------
# the modules

def test_sync_batchnorm_marks_and_unmarks():
    from centertrack_amd import parallel
    from centertrack_amd.dla_base import BasicBlock
    m = BasicBlock(16, 16)
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(bns) == 2 and not any(parallel.SYNC_BN_MARK in b.__dict__ for b in bns)
    assert parallel.sync_batchnorm(m) is m
    assert all(b.__dict__[parallel.SYNC_BN_MARK].group is None and not b.__dict__[parallel.SYNC_BN_MARK].force for b in bns)
    assert all(type(b) is torch.nn.BatchNorm2d for b in bns)                  # marked, not replaced
    parallel.sync_batchnorm(m, force=True)
    assert all(b.__dict__[parallel.SYNC_BN_MARK].force for b in bns)
    assert parallel.sync_batchnorm(m, False) is m
    assert not any(parallel.SYNC_BN_MARK in b.__dict__ for b in bns)
    one = torch.nn.BatchNorm2d(8)
    parallel.sync_batchnorm(one)                                              # the module itself counts
    assert parallel.SYNC_BN_MARK in one.__dict__


def test_state_dict_keys_of_dlaseg_are_unchanged():
    from test_dlaseg_cpu import HEAD_CONVS, HEADS, Opt
    from centertrack_amd import parallel
    from centertrack_amd.dla_seg import DLASeg
    model = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    keys = list(model.state_dict().keys())
    buffers = [k for k, _ in model.named_buffers()]
    parallel.sync_batchnorm(model)
    assert list(model.state_dict().keys()) == keys and [k for k, _ in model.named_buffers()] == buffers
    n = sum(1 for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d))
    assert n > 40 and sum(1 for b in model.modules() if parallel.SYNC_BN_MARK in b.__dict__) == n
    again = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    again.load_state_dict(model.state_dict())                                 # checkpoints go both ways
    model.load_state_dict(again.state_dict())


def test_a_marked_model_without_a_group_takes_the_unsynchronised_path(monkeypatch):
    from centertrack_amd import _train, ops, parallel
    assert not parallel.group_active()
    bn = torch.nn.BatchNorm2d(16)
    parallel.sync_batchnorm(bn, force=True)
    assert parallel.sync_batchnorm_of(bn) is None                             # marked, forced even: no group, no collective
    calls = []

    def fake_stats(z, eps):
        calls.append('bn_stats')
        return torch.zeros(16), torch.ones(16), torch.ones(16)

    def never(*a, **k):
        raise AssertionError('the synchronised path ran')
    monkeypatch.setattr(ops, 'bn_stats', fake_stats)
    monkeypatch.setattr(ops, 'bn_stats_row', never)
    monkeypatch.setattr(ops, 'bn_merge_stats', never)
    monkeypatch.setattr(parallel, 'all_gather_rows', never)
    z = ops.View(torch.zeros(2, 3, 5, 16))
    mean, invstd, batch = _train.bn_statistics(bn, z, 'backbone')
    assert batch is True and calls == ['bn_stats'] and int(bn.num_batches_tracked) == 1
    mean, invstd, batch = _train.bn_statistics(bn.eval(), z, 'backbone')
    assert batch is False and mean is bn.running_mean and calls == ['bn_stats']


def test_all_gather_rows_without_a_group_is_the_row():
    from centertrack_amd import parallel
    row = torch.arange(12, dtype=torch.float32)
    out = parallel.all_gather_rows(row)
    assert out.shape == (1, 12) and out.data_ptr() == row.data_ptr()


def test_trainer_documents_the_mode():
    from centertrack_amd import trainer
    not_covered = trainer.__doc__.split('Not covered:')[1]
    assert 'synchronised BatchNorm' not in not_covered and 'opt.sync_bn' in trainer.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI

@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib
    return _lib.load()


def aligned(n, dtype=np.float32):
    """zeros whose first element sits on a 16-byte boundary"""
    a = np.zeros(n + 4, dtype)
    off = (-a.ctypes.data % 16) // a.itemsize
    return a[off:off + n]


def merge_desc(C=16, world=2, ld=None, eps=1e-5):
    """a descriptor whose pointers are host memory: a refused call never reads them"""
    from centertrack_amd import _lib
    keep = [aligned(max(world, 1) * (3 * C + 4) + 8)] + [aligned(C + 4) for _ in range(5)] + [aligned(2, np.int64)]
    d = _lib.BnMergeDesc()
    d.rows, d.world, d.C, d.ld, d.eps = keep[0].ctypes.data, world, C, 3 * C + 4 if ld is None else ld, eps
    d.mean, d.var, d.invstd, d.unbiased, d.inv_count = (k.ctypes.data for k in keep[1:6])
    d.count = keep[6].ctypes.data
    return d, keep


def test_merge_refusals(lib):
    from centertrack_amd import _lib

    def refused(d, what):
        assert lib.ct_bn_merge_stats(ctypes.byref(d) if d is not None else None, None) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error(), lib.ct_last_error()
    refused(None, b'null descriptor')
    for field in ('rows', 'mean', 'var', 'invstd', 'unbiased', 'inv_count'):
        d, keep = merge_desc()
        setattr(d, field, None)
        refused(d, b'null pointer')
    refused(merge_desc(C=18)[0], b'multiple of 4')
    refused(merge_desc(C=0)[0], b'multiple of 4')
    refused(merge_desc(world=0)[0], b'world=0')
    refused(merge_desc(world=-3)[0], b'world=-3')
    refused(merge_desc(eps=-1e-5)[0], b'eps=')
    refused(merge_desc(eps=float('nan'))[0], b'eps=')
    refused(merge_desc(ld=3 * 16)[0], b'row pitch')                           # no room for the count
    refused(merge_desc(ld=3 * 16 + 3)[0], b'row pitch')                       # the 64-bit count would be misaligned
    for field in ('gamma', 'beta', 'beta_shifted'):                           # all three or none
        d, keep = merge_desc()
        setattr(d, field, keep[1].ctypes.data)
        refused(d, b'go together')
    d, keep = merge_desc()
    d.rows = keep[0].ctypes.data + 4
    refused(d, b'8-byte aligned')
    assert lib.ct_version() == 103


def test_stats_row_refusals(lib):
    from centertrack_amd import _lib
    d, keep, _, _ = bn_desc(_lib.BnDesc)
    row = aligned(3 * 16 + 4)

    def refused(d, row, what, code=_lib.CT_ERR_ARG):
        assert lib.ct_bn_stats_row(ctypes.byref(d) if d is not None else None, row, None) == code
        msg = lib.ct_last_error()
        assert what in msg and b'ct_bn_stats_row' in msg, msg
    refused(d, None, b'null pointer (row)')
    refused(d, row.ctypes.data + 4, b'row must be 16-byte aligned')
    refused(None, row.ctypes.data, b'null descriptor')
    refused(d, row.ctypes.data, b'workspace', _lib.CT_ERR_WORKSPACE)           # (mean and var of the descriptor are not read)
    d.invstd = None
    refused(d, row.ctypes.data, b'null pointer (invstd)')
    d, keep, _, _ = bn_desc(_lib.BnDesc, C=18)
    refused(d, row.ctypes.data, b'multiple of 4')


def bn_desc(cls, C=16, flags=None):
    from centertrack_amd import _lib
    keep = [aligned(2 * 3 * 5 * C + 8) for _ in range(5)] + [aligned(2 * C + 8) for _ in range(6)]
    for k in keep:
        assert k.ctypes.data % 16 == 0
    d = cls()
    d.z, d.N, d.H, d.W, d.C, d.ldz = keep[0].ctypes.data, 2, 3, 5, C, C
    d.gy, d.ldgy, d.gz, d.ldgz = keep[1].ctypes.data, C, keep[2].ctypes.data, C
    d.mean, d.invstd, d.gamma, d.beta = (k.ctypes.data for k in keep[5:9])
    d.flags = _lib.CT_BN_BATCH_STATS if flags is None else flags
    return d, keep, keep[9].ctypes.data, keep[10].ctypes.data


@pytest.mark.parametrize('entry', ['ct_bn_act_backward_apply', 'ct_bn_relu_backward_apply'])
def test_backward_apply_refusals(lib, entry):
    from centertrack_amd import _lib
    cls = _lib.BnActDesc if entry == 'ct_bn_act_backward_apply' else _lib.BnDesc
    fn = getattr(lib, entry)

    def refused(d, sums, inv, what):
        assert fn(ctypes.byref(d) if d is not None else None, sums, inv, None) == _lib.CT_ERR_ARG
        msg = lib.ct_last_error()
        assert what in msg and entry.encode() in msg, msg
    d, keep, sums, inv = bn_desc(cls)
    refused(None, sums, inv, b'null descriptor')
    refused(d, None, inv, b'null pointer (sums)')
    refused(d, sums, None, b'null pointer (inv_count)')
    refused(d, sums + 4, inv, b'sums must be 16-byte aligned')
    refused(d, sums, inv + 2, b'inv_count must be 4-byte aligned')
    d.gz = None
    refused(d, sums, inv, b'no output asked for')
    d, keep, sums, inv = bn_desc(cls, flags=0)
    refused(d, sums, inv, b'without CT_BN_BATCH_STATS')
    d, keep, sums, inv = bn_desc(cls, C=18)
    refused(d, sums, inv, b'multiple of 4')
    d, keep, sums, inv = bn_desc(cls)
    d.gy = None
    refused(d, sums, inv, b'null pointer (gy)')
    d, keep, sums, inv = bn_desc(cls)
    d.mean = None
    refused(d, sums, inv, b'null pointer (mean)')
    if cls is _lib.BnActDesc:
        d, keep, sums, inv = bn_desc(cls)
        d.gres, d.ldgres = keep[3].ctypes.data, 12
        refused(d, sums, inv, b'channel pitch of gres')
