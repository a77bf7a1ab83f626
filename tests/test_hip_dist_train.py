"""GPU: data-parallel training.

1. ``ct_optim_pack_grads`` in process, bit for bit against ``optim.reference_pack``.
2. World 1 on RCCL (torchrun, one rank, ``nccl``): the distributed ``Adam`` / ``SGD`` step, unguarded and guarded, against the
   same optimizer without ``distribute`` -- the scale is 1 and the sum over one rank is the identity, so every bit agrees.
3. World 2 over gloo, both ranks on ``cuda:0``, the ranks on different data: both ranks end with the same bits, those of a
   one-process emulation that puts ``g0 * 0.5 + g1 * 0.5`` into ``p.grad`` (a sum of two halves has no order to disagree
   about); the guard decides alike on both; an Inf on one rank makes both skip; ``check_in_sync``.
4. ``Trainer`` on ``DLASeg(34)`` in the same two-rank job.  The parameters that "have moved" are those that receive a
   gradient: the six ``project`` tensors of ``base.level3`` / ``base.level4`` are read by nobody (tests/test_hip_dlaseg.py's
   ``UNREAD``), have no gradient on any rank and stay where the broadcast put them.
5. World 2 on RCCL, one GPU per rank: skipped on a box with one GPU.

Each multi-process job is ONE fresh child (``python -m torch.distributed.run``) started once per module; the ranks write
their findings as JSON (tests/_dist_train_worker.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
WORKER = os.path.join(ROOT, 'tests', '_dist_train_worker.py')
CHUNK = 4096
NUMELS = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5]
BIG = (2048 + 3) * 4096 + 7                      # more chunks than OPT_MAX_BLOCKS = 2048: the strided loop runs
UNALIGNED = [1030, 4096 + 9]                     # gradients at buf[1:]: 4-byte but not 16-byte aligned
SCALES = [1.0, 0.5, float(np.float32(1.0) / np.float32(3.0))]
UNREAD = ['base.level%d.project.%s' % (lv, k) for lv in (3, 4) for k in ('0.weight', '1.weight', '1.bias')]
KEYS = ['adam', 'adam_guard', 'sgd', 'sgd_guard']


# ------------------------------------------------------------------ 1. the kernel
@pytest.fixture(scope='module')
def host_grads():
    rs = np.random.RandomState(77)
    grads = [rs.randn(n).astype(np.float32) for n in NUMELS + [BIG] + UNALIGNED]
    grads[2][5], grads[3][0], grads[4][-1] = np.inf, -np.inf, np.nan
    grads[6][CHUNK * 2049 + 3], grads[6][-1], grads[7][2], grads[8][-2] = np.nan, -np.inf, np.inf, np.nan
    grads[5][17] = np.float32(1e-41)                                         # a denormal passes as it is
    return grads


def upload(host_grads, device):
    """the gradients on the device, the last len(UNALIGNED) of them as views one element into their buffers"""
    out, keep = [], []
    for i, g in enumerate(host_grads):
        if i < len(host_grads) - len(UNALIGNED):
            t = torch.from_numpy(g).to(device)
            assert t.data_ptr() % 16 == 0
        else:
            buf = torch.zeros(g.size + 1, dtype=torch.float32, device=device)
            t = buf[1:]
            t.copy_(torch.from_numpy(g))
            assert t.data_ptr() % 16 == 4
        keep.append(t)
        out.append(t)
    return out


def pack_on_device(grads, flat_base, scale, device):
    from centertrack_amd import _lib, ops, optim as O
    offsets, total = O.flat_layout([g.numel() for g in grads])
    items = [(flat_base.data_ptr() + 4 * off, flat_base.data_ptr() + 4 * off, 0, 0, g.numel(), (0.0, 0.0, 0.0), 0)
             for g, off in zip(grads, offsets)]
    words, n, chunks = O.pack(_lib.CT_OPTIM_SGD, items, src=[g.data_ptr() for g in grads])
    assert chunks * CHUNK == total
    table = torch.from_numpy(words).to(device)
    ops.optim_pack_grads(table, n, chunks, scale)
    torch.cuda.synchronize()
    return total


def compare(got, want):
    """bitwise, except that a NaN need only stay a NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


@pytest.mark.parametrize('scale', SCALES)
def test_pack_grads_bit_for_bit(device, host_grads, scale):
    from centertrack_amd import optim as O
    want = O.reference_pack(host_grads, scale)
    grads = upload(host_grads, device)
    CANARY = 64
    flat = torch.full((want.size + CANARY,), float('nan'), dtype=torch.float32, device=device)
    flat[want.size:] = 12345.0
    assert flat.data_ptr() % 16 == 0
    total = pack_on_device(grads, flat, scale, device)
    assert total == want.size and total // CHUNK > 2048 + len(host_grads)
    got = flat.cpu().numpy()
    compare(got[:total], want)
    assert (got[total:] == 12345.0).all()                                    # nothing behind chunks * CHUNK
    offsets, _ = O.flat_layout([g.size for g in host_grads])
    covered = np.zeros(total, bool)
    for g, off in zip(host_grads, offsets):
        covered[off:off + g.size] = True
        inf = np.isinf(g)
        assert np.array_equal(got[off:off + g.size][inf], g[inf])            # +-Inf comes through
    assert (got[:total][~covered].view(np.int32) == 0).all()                 # the padding is +0.0
    if scale == 1.0:
        assert got[offsets[5] + 17] == np.float32(1e-41)
    for t, g in zip(grads, host_grads):                                      # the sources are unchanged
        assert np.array_equal(t.cpu().numpy().view(np.int32), g.view(np.int32))


def test_pack_grads_into_a_buffer_that_is_not_16_byte_aligned(device, host_grads):
    """the stores fall back to single elements: what a caller with its own buffer may hand in"""
    from centertrack_amd import optim as O
    small = [g for i, g in enumerate(host_grads) if i != len(NUMELS)]         # (without the large one)
    want = O.reference_pack(small, 0.5)
    base = torch.full((want.size + 1 + 64,), float('nan'), dtype=torch.float32, device=device)
    base[want.size + 1:] = 12345.0
    base[0] = 54321.0
    flat = base[1:]
    assert flat.data_ptr() % 16 == 4
    pack_on_device(upload(small, device), flat, 0.5, device)
    got = base.cpu().numpy()
    compare(got[1:want.size + 1], want)
    assert got[0] == 54321.0 and (got[want.size + 1:] == 12345.0).all()


def test_pack_grads_refusals(device):
    from centertrack_amd import _lib
    lib = _lib.load()
    table = torch.zeros(64, dtype=torch.int32, device=device)
    for args, what in (((None, 1, 1, 1.0, None), b'null table'),
                       ((table.data_ptr(), 1, 1, float('nan'), None), b'not finite'),
                       ((table.data_ptr(), 1, 1, float('inf'), None), b'not finite'),
                       ((table.data_ptr(), 0, 1, 1.0, None), b'tensors outside'),
                       ((table.data_ptr(), 3, 2, 1.0, None), b'chunks')):
        assert lib.ct_optim_pack_grads(*args) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error(), lib.ct_last_error()


# ------------------------------------------------------------------ the jobs
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def run_job(tmp, name, ranks, job, backend, trainer=False):
    out = os.path.join(str(tmp), name + '.json')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), WORKER, '--job', job, '--backend', backend, '--out', out]
    if trainer:
        cmd.append('--trainer')
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    found = [json.load(open('%s.%d' % (out, r))) for r in range(ranks)]
    assert [f['rank'] for f in found] == list(range(ranks)) and all(f['world'] == ranks for f in found)
    return found


@pytest.fixture(scope='module')
def world1(device, tmp_path_factory):
    return run_job(tmp_path_factory.mktemp('dist'), 'world1', 1, 'world1', 'nccl')[0]


@pytest.fixture(scope='module')
def world2(device, tmp_path_factory):
    return run_job(tmp_path_factory.mktemp('dist'), 'world2', 2, 'world2', 'gloo', trainer=True)


# ------------------------------------------------------------------ 2. world 1 on RCCL
def test_world_1_goes_through_rccl(world1):
    assert world1['backend'] == 'nccl' and world1['world'] == 1


@pytest.mark.parametrize('key', KEYS)
def test_world_1_distributed_step_equals_the_plain_step(world1, key):
    f = world1[key]
    assert len(f['dist']) == 3 and f['dist'] == f['plain']                   # parameters and state, after every step
    assert len({d[1] for d in f['dist']}) == 3                               # (and they moved)
    assert f['reduced_equal']                                                # reduced_grads() is p.grad: the scale is 1
    if key.endswith('_guard'):
        assert f['stats'] == f['stats_plain'] and [s[4] for s in f['stats']] == [1, 2, 3]     # clipped at every step


def test_a_changed_layout_is_refused(world1):
    assert 'changed after the first distributed step' in world1['layout_change'] and not world1['layout_change_moved']


# ------------------------------------------------------------------ 3. world 2 over gloo
def check_two_ranks(found, backend):
    a, b = found
    assert a['backend'] == b['backend'] == backend
    for key in KEYS:
        fa, fb = a[key], b[key]
        assert len(fa['dist']) == 3 and fa['dist'] == fb['dist'], key        # bitwise equal on both ranks
        assert fa['dist'] == fa['emulated'] == fb['emulated'], key           # and equal to the one-process emulation
        assert fa['dist'][0] != fa['rank0_alone'][0] and fa['dist'][-1][1] != fa['rank0_alone'][-1][1], key
        if key.endswith('_guard'):
            assert fa['stats'] == fb['stats'] == fa['stats_emulated'] and len(fa['stats']) == 3, key
            assert [s[4] for s in fa['stats']] == [1, 2, 3] and all(0.0 < s[1] < 1.0 for s in fa['stats']), key
    for kind in ('adam', 'sgd'):
        fa, fb = a[kind + '_inf'], b[kind + '_inf']
        assert fa['dist'] == fb['dist'] == fa['emulated'], kind
        assert fa['stats'] == fb['stats'], kind
        # the Inf sits in rank 1's gradient only, at step 2: both ranks skip it, and the parameters do not move
        assert [s[2] for s in fa['stats']] == [0, 1, 0] and [s[3] for s in fa['stats']] == [0, 1, 1], kind
        assert fa['stats'][1][5] == 1, kind
        assert fa['dist'][1][1] == fa['dist'][0][1] and fa['dist'][2][1] != fa['dist'][1][1], kind
    assert a['in_sync'] == b['in_sync'] == 'ok'
    for f in found:
        assert 'rank(s) [1] differ' in f['out_of_sync'], f['out_of_sync']


def check_trainer(found):
    a, b = found
    assert a['constructed'] != b['constructed']                              # another seed on rank 1 ...
    assert a['before'] == b['before'] == a['constructed']                    # ... and the broadcast gave it rank 0's
    assert a['buffers_before'] == b['buffers_before']
    assert a['after'] == b['after'] and a['after'] != a['before']            # bitwise equal across ranks
    for f in found:
        assert f['n_params'] == 243 and sorted(f['unmoved']) == sorted(UNREAD), f['unmoved']     # every other one moved
        assert f['in_sync'] == 'ok'
    assert a['ret'] == b['ret'] and list(a['ret'])[0] == 'tot'
    assert all(np.isfinite(v) for v in a['ret'].values())
    assert a['buffers_after'] == b['buffers_after'] != a['buffers_before']   # rank 0's running statistics


def test_world_2_over_gloo(world2):
    check_two_ranks(world2, 'gloo')


def test_trainer_on_two_ranks(world2):
    check_trainer(world2)


# ------------------------------------------------------------------ 5. world 2 on RCCL
def test_world_2_on_rccl(device, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('one GPU: RCCL between two ranks needs two')
    found = run_job(tmp_path, 'world2_rccl', 2, 'world2', 'nccl', trainer=True)
    check_two_ranks(found, 'nccl')
    check_trainer(found)
