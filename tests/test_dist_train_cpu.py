"""CPU: the host side of data-parallel training -- the ``src`` column of ``optim.pack`` and its place
in ``ct_optim_rec``, the layout of the flat gradient buffer and the host restatement of ``ct_optim_pack_grads``, the three
collectives of ``centertrack_amd.parallel`` over a two-rank gloo group, and the refusals."""
import ctypes
import os
import shutil
import socket
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CHUNK = 4096
NUMELS = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5]


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def fake_items(sizes):
    """Adam records over made-up, 16-byte aligned addresses"""
    items, addr = [], 1 << 20
    for n in sizes:
        ptrs = []
        for _ in range(4):
            ptrs.append(addr)
            addr += (4 * n + 65535) // 65536 * 65536
        items.append(tuple(ptrs) + (n, (0.1, 0.999, 0.001, 0.01, 0.5, 1e-8, 0.0), 0))
    return items


# ------------------------------------------------------------------ pack
def test_pack_with_src_differs_in_the_src_words_only():
    from centertrack_amd import _lib, optim as O
    items = fake_items(NUMELS)
    src = [(7 << 32) + 4 * (3 * i + 1) for i in range(len(items))]           # 4-byte aligned, above 2^32
    plain, n, chunks = O.pack(_lib.CT_OPTIM_ADAM, items)
    again, _, _ = O.pack(_lib.CT_OPTIM_ADAM, items, src=None)
    with_src, n2, chunks2 = O.pack(_lib.CT_OPTIM_ADAM, items, src=src)
    assert np.array_equal(plain, again) and (n, chunks) == (n2, chunks2) and plain.shape == with_src.shape
    off = O.REC.fields['src'][1]
    assert off % 4 == 0 and O.REC.fields['src'][0] == np.dtype('<u8')
    src_words = np.zeros(plain.size, bool)
    for t in range(n):
        src_words[t * O.REC_WORDS + off // 4:t * O.REC_WORDS + off // 4 + 2] = True
    assert np.array_equal(plain[~src_words], with_src[~src_words]) and not plain[src_words].any()
    rec = np.frombuffer(with_src[:n * O.REC_WORDS].tobytes(), O.REC)
    assert [int(v) for v in rec['src']] == src and not rec['reserved'].any()
    # out=: filled in place, the same words
    out = np.full(O.table_words(n) + 3, -1, np.int32)
    got, _, _ = O.pack(_lib.CT_OPTIM_ADAM, items, out=out, src=src)
    assert got is out and np.array_equal(out[:-3], with_src) and (out[-3:] == -1).all()


def test_pack_refuses_a_null_or_misaligned_src():
    from centertrack_amd import _lib, optim as O
    items = fake_items([5, 9])
    with pytest.raises(O.CTError, match='null source'):
        O.pack(_lib.CT_OPTIM_ADAM, items, src=[4096, 0])
    with pytest.raises(O.CTError, match='4-byte'):
        O.pack(_lib.CT_OPTIM_ADAM, items, src=[4096, 4098])
    with pytest.raises(O.CTError, match='source addresses'):
        O.pack(_lib.CT_OPTIM_ADAM, items, src=[4096])


def test_src_sits_where_the_header_puts_it(tmp_path):
    from centertrack_amd import _lib, optim as O
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "centertrack_hip.h"\nint main(void) {'
                   'printf("%zu %zu %zu %zu\\n", sizeof(ct_optim_rec), offsetof(ct_optim_rec, src), '
                   'offsetof(ct_optim_rec, reserved), sizeof(((ct_optim_rec *)0)->src)); return 0; }\n')
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    size, off, reserved, width = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == 128 == O.REC.itemsize == ctypes.sizeof(_lib.OptimRec) == _lib.CT_OPTIM_REC_BYTES
    assert off == O.REC.fields['src'][1] == _lib.OptimRec.src.offset and width == 8
    assert reserved == O.REC.fields['reserved'][1] == _lib.OptimRec.reserved.offset


# ------------------------------------------------------------------ flat_layout, reference_pack
def test_flat_layout_is_the_chunk_prefix():
    from centertrack_amd import _lib, optim as O
    assert O.CHUNK == CHUNK
    offsets, total = O.flat_layout(NUMELS)
    words, n, chunks = O.pack(_lib.CT_OPTIM_ADAM, fake_items(NUMELS))
    prefix = words[n * O.REC_WORDS:n * O.REC_WORDS + n + 1]
    assert offsets == [int(c) * CHUNK for c in prefix[:-1]] == [0, 4096, 8192, 12288, 16384, 24576]
    assert total == chunks * CHUNK == 9 * CHUNK
    assert all(o % 4 == 0 for o in offsets)                                   # 16-byte aligned when the buffer is
    for numel in NUMELS:
        assert O.flat_layout([numel]) == ([0], (numel + CHUNK - 1) // CHUNK * CHUNK)
    with pytest.raises(O.CTError):
        O.flat_layout([])
    with pytest.raises(O.CTError):
        O.flat_layout([4, 0])


@pytest.mark.parametrize('scale', [1.0, 0.5, float(np.float32(1.0) / np.float32(3.0))])
def test_reference_pack_values_and_padding(scale):
    from centertrack_amd import optim as O
    rs = np.random.RandomState(31)
    grads = [rs.randn(n).astype(np.float32) for n in NUMELS]
    grads[2][5], grads[3][0], grads[4][-1] = np.inf, -np.inf, np.nan
    flat = O.reference_pack(grads, scale)
    offsets, total = O.flat_layout(NUMELS)
    assert flat.dtype == np.float32 and flat.shape == (total,)
    covered = np.zeros(total, bool)
    for g, off in zip(grads, offsets):
        with np.errstate(invalid='ignore'):
            want = g * np.float32(scale)
        assert np.array_equal(flat[off:off + g.size].view(np.int32), want.view(np.int32))
        covered[off:off + g.size] = True
    pad = flat[~covered]
    assert pad.size == total - sum(NUMELS) and (pad.view(np.int32) == 0).all()      # +0.0: sign bit clear
    assert not np.signbit(pad).any()
    assert np.isposinf(flat[offsets[2] + 5]) and np.isneginf(flat[offsets[3]]) and np.isnan(flat[offsets[4] + 4096])
    # float64 gradients are rounded to float32 first: float32(g) * float32(scale)
    g64 = rs.randn(7)
    assert np.array_equal(O.reference_pack([g64], scale)[:7], g64.astype(np.float32) * np.float32(scale))


# ------------------------------------------------------------------ the symbol
def test_pack_grads_is_exported_and_refuses_without_a_gpu():
    from centertrack_amd import _lib
    assert 'ct_optim_pack_grads' in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'ct_optim_pack_grads')
    buf = np.zeros(1024, np.int32)

    def rejected(args, what):
        assert lib.ct_optim_pack_grads(*args) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error() and b'ct_optim_pack_grads' in lib.ct_last_error(), lib.ct_last_error()
    rejected((None, 1, 1, 1.0, None), b'null table')
    rejected((buf.ctypes.data, 0, 1, 1.0, None), b'tensors outside')
    rejected((buf.ctypes.data, _lib.CT_OPTIM_MAX_TENSORS + 1, 1 << 21, 1.0, None), b'tensors outside')
    rejected((buf.ctypes.data, 2, 1, 1.0, None), b'chunks')
    rejected((buf.ctypes.data, 1, 1 << 31, 1.0, None), b'chunks')
    for bad in (float('nan'), float('inf'), -float('inf')):
        rejected((buf.ctypes.data, 1, 1, bad, None), b'not finite')
    from centertrack_amd import ops
    assert callable(ops.optim_pack_grads)


# ------------------------------------------------------------------ gloo, world 2
def _bn_model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Linear(5, 2))
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
        m[1].num_batches_tracked.fill_(seed)
    return m


def _flat_of(rank, n=3 * CHUNK + 5):
    g = torch.Generator().manual_seed(500 + rank)
    return torch.randn(n, generator=g)


def _collectives_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    from centertrack_amd import optim as O, parallel, trainer as TR
    from centertrack_amd._lib import CTError
    parallel.init_from_env(backend='gloo')
    flat = _flat_of(rank)
    back = parallel.all_reduce_flat(flat)
    sums = parallel.reduce_sums(torch.tensor([1.5 + rank, 10.0 * (rank + 1), 4.0], dtype=torch.float64))
    model = _bn_model(10 + rank)
    parallel.broadcast_module(model, src=0)
    state = {k: v.numpy().copy() for k, v in model.state_dict().items()}    # (numpy: the queue pickles it whole)
    bad = parallel.ranks_that_differ(torch.tensor([7, 9 + rank]))
    try:
        parallel.check_same_digest('numels %d' % rank, 'the list')
        digest = 'ok'
    except RuntimeError as e:
        digest = str(e)
    # a torch optimizer cannot exchange gradients
    heads = {'hm': 1, 'reg': 2, 'wh': 2}
    opt = types.SimpleNamespace(heads=heads, weights={h: 1 for h in heads}, num_stacks=1, debug=0, num_iters=-1,
                                print_iter=0, device='cpu')
    lin = torch.nn.Linear(2, 2)
    tr = TR.Trainer(opt, lin, torch.optim.SGD(lin.parameters(), lr=0.1))
    try:
        tr.set_device([0, 1], [1, 1], 'cpu')
        refused = ''
    except CTError as e:
        refused = str(e)
    # with a group distribute() is accepted, and switched off again
    adam = O.Adam(lin.parameters(), 1e-3)
    on = adam.distribute() is adam and adam._dist is not None and adam.distribute(False) is adam and adam._dist is None
    parallel.barrier()
    q.put((rank, back is flat, flat.numpy(), sums.numpy(), state, bad, digest, refused, on, parallel.world_size()))
    parallel.shutdown()


@pytest.fixture(scope='module')
def two_ranks():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_collectives_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=180) for _ in range(world)), key=lambda g: g[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def test_all_reduce_flat_is_the_sum_bit_for_bit_on_both_ranks(two_ranks):
    want = (_flat_of(0) + _flat_of(1)).numpy()
    for rank, same_object, flat, *_ in two_ranks:
        assert same_object and np.array_equal(flat.view(np.int32), want.view(np.int32)), rank


def test_reduce_sums_gives_the_sum_on_both_ranks(two_ranks):
    for got in two_ranks:
        assert got[3].dtype == np.float64 and got[3].tolist() == [1.5 + 2.5, 10.0 + 20.0, 8.0]
        assert got[9] == 2


def test_broadcast_module_gives_rank_1_the_parameters_and_buffers_of_rank_0(two_ranks):
    want = _bn_model(10).state_dict()
    other = _bn_model(11).state_dict()
    assert any(not torch.equal(want[k], other[k]) for k in want if 'running' in k)
    assert int(want['1.num_batches_tracked']) == 10 != int(other['1.num_batches_tracked'])
    for got in two_ranks:
        assert list(got[4]) == list(want)
        for k, v in want.items():
            assert got[4][k].dtype == v.numpy().dtype and np.array_equal(got[4][k], v.numpy()), (got[0], k)


def test_ranks_learn_who_differs_from_rank_0(two_ranks):
    for got in two_ranks:
        assert got[5] == [1]
        assert 'the list differs between ranks' in got[6] and 'rank(s) [1]' in got[6]


def test_a_torch_optimizer_on_two_ranks_is_refused(two_ranks):
    for got in two_ranks:
        assert 'needs an optimizer of centertrack_amd.optim' in got[7] and 'SGD' in got[7]
        assert got[8]


# ------------------------------------------------------------------ refusals and no-ops without a group
def test_without_a_group_the_collectives_are_no_ops_and_distribute_is_refused():
    from centertrack_amd import optim as O, parallel, trainer as TR
    assert not parallel.group_active() and parallel.world_size() == 1
    flat = _flat_of(0, 10)
    keep = flat.clone()
    assert parallel.all_reduce_flat(flat) is flat and torch.equal(flat, keep)
    t = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert parallel.reduce_sums(t) is t
    m = _bn_model(3)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    assert parallel.broadcast_module(m) is m and all(torch.equal(v, want[k]) for k, v in m.state_dict().items())
    assert parallel.ranks_that_differ(torch.tensor([1, 2])) == [] and len(parallel.check_same_digest('x', 'y')) == 16
    lin = torch.nn.Linear(2, 2)
    for cls, kw in ((O.Adam, {}), (O.SGD, dict(momentum=0.9))):
        optimizer = cls(lin.parameters(), 1e-3, **kw)
        with pytest.raises(O.CTError, match='process group'):
            optimizer.distribute()
        assert optimizer.distribute(False) is optimizer                  # off is always accepted
        with pytest.raises(O.CTError, match='no distributed step'):
            optimizer.reduced_grads()
        with pytest.raises(O.CTError, match='distribute'):
            optimizer.check_in_sync()
    heads = {'hm': 1, 'reg': 2, 'wh': 2}
    opt = types.SimpleNamespace(heads=heads, weights={h: 1 for h in heads}, num_stacks=1, debug=0, num_iters=-1,
                                print_iter=0, device='cpu')
    tr = TR.Trainer(opt, lin, O.Adam(lin.parameters(), 1e-3))
    with pytest.raises(O.CTError, match='torchrun'):
        tr.set_device([0, 1], [4, 4], 'cpu')
