"""CPU: ``centertrack_amd.optim`` without a GPU -- ``reference_step`` against torch's own CPU
optimizers, the packing of the record table against a brute-force walk and against the header, ``ct_optim_step``'s
argument refusals on fake pointers, the constructors and refusals of ``Adam`` / ``SGD``, the resume branch of
``load_model`` against the reference's own (tests/golden/resume.json, written by tests/golden/make_resume_golden.py),
``save_model``, and the refusals of ``Trainer``."""
import ctypes
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

import _optim as T

GOLD = os.path.join(T.ROOT, 'tests', 'golden', 'resume.json')


# ------------------------------------------------------------------ reference_step
@pytest.mark.parametrize('wd', [0, 1e-4])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_reference_step_is_torchs_float64_step(kind, wd):
    """five steps on float64 CPU tensors, two groups with different lr, tensor 3 without a gradient on steps 2 and 4:
    parameters and state equal torch's (foreach=False) bit for bit after every step"""
    from centertrack_amd import optim as O
    sizes = [1, 2, 27, 64, 512, 1000]
    rs = np.random.RandomState(7)
    tensors = [torch.tensor(rs.randn(n)).requires_grad_() for n in sizes]
    mine = [t.detach().numpy().copy() for t in tensors]
    states = [{} for _ in sizes]
    kw = dict(T.HYPER[kind], weight_decay=wd)
    lrs = [1e-2] * 3 + [3e-3] * 3
    opt = T.torch_class(kind)([dict(params=tensors[:3], lr=1e-2, **kw), dict(params=tensors[3:], lr=3e-3, **kw)],
                              foreach=False)
    for step in range(5):
        for i, t in enumerate(tensors):
            g = rs.randn(sizes[i])
            if i == 3 and step in (1, 3):
                t.grad = None
                continue
            t.grad = torch.tensor(g)
            O.reference_step(kind, mine[i], g, states[i], dict(kw, lr=lrs[i]))
        opt.step()
        for i, t in enumerate(tensors):
            assert np.array_equal(t.detach().numpy(), mine[i]), (step, i)
            for k in T.STATE_KEYS[kind]:
                assert np.array_equal(opt.state[t][k].numpy(), states[i][k]), (step, i, k)
    assert states[3]['step'] == 3 if kind == 'adam' else True
    if kind == 'adam':
        assert [int(opt.state[t]['step']) for t in tensors] == [5, 5, 5, 3, 5, 5]
    # float32: same functions, every array stays float32
    p32, st32 = np.ones(5, np.float32), {}
    O.reference_step(kind, p32, np.full(5, 0.5, np.float32), st32, dict(kw, lr=1e-2))
    assert p32.dtype == np.float32 and all(v.dtype == np.float32 for v in st32.values() if isinstance(v, np.ndarray))
    with pytest.raises(O.CTError):
        O.reference_step('rmsprop', p32, p32, {}, dict(lr=1.0))


# ------------------------------------------------------------------ pack
def fake_items(sizes, kind):
    """records over made-up addresses: 64 KiB-spaced, 16-byte aligned"""
    items, addr = [], 1 << 20
    for n in sizes:
        ptrs = []
        for _ in range(4):
            ptrs.append(addr)
            addr += (4 * n + 65535) // 65536 * 65536
        if kind == 'sgd':
            ptrs[3] = 0
        items.append(tuple(ptrs) + (n, (0.1, 0.999, 0.001, 0.01, 0.5, 1e-8, 0.0)[:7 if kind == 'adam' else 3], 0))
    return items


def unpack(words, n):
    from centertrack_amd import optim as O
    rec = np.frombuffer(words[:n * O.REC_WORDS].tobytes(), O.REC)
    return rec, words[n * O.REC_WORDS:n * O.REC_WORDS + n + 1]


@pytest.mark.parametrize('which', ['list', 'dlaseg'])
def test_pack_covers_every_element_once(which):
    from centertrack_amd import _lib, optim as O
    assert O.CHUNK == T.CHUNK == _lib.CT_OPTIM_CHUNK
    sizes = T.SIZES if which == 'list' else T.dlaseg_sizes()
    if which == 'dlaseg':                                        # what DESIGN.md section 20 says of this list
        assert len(sizes) == 243 and sum(sizes) == 19807015
        assert sum(n <= 512 for n in sizes) == 158 and sum(n > 65536 for n in sizes) == 40 and sum(n % 4 != 0 for n in sizes) == 20
    items = fake_items(sizes, 'adam')
    words, n, chunks = O.pack(_lib.CT_OPTIM_ADAM, items)
    assert n == len(sizes) and words.dtype == np.int32 and words.size == O.table_words(n) == n * 32 + n + 1
    rec, prefix = unpack(words, n)
    assert prefix[0] == 0 and prefix[-1] == chunks and (np.diff(prefix) >= 1).all()          # monotone, no empty tensor
    assert rec['numel'].tolist() == sizes and [int(v) for v in rec['p']] == [it[0] for it in items]
    assert np.array_equal(rec['s'][0, :7], np.array(items[0][5], np.float32)) and not rec['reserved'].any()
    # brute force: walk every chunk as the kernel does and mark its elements
    seen = [np.zeros(s, np.uint8) for s in sizes]
    owner = np.repeat(np.arange(n), np.diff(prefix))
    for c in range(chunks):
        t = O.find_tensor(prefix, c)
        assert t == owner[c], c
        base = (c - int(prefix[t])) * O.CHUNK
        cnt = min(O.CHUNK, sizes[t] - base)
        assert cnt >= 1
        seen[t][base:base + cnt] += 1
    assert all((s == 1).all() for s in seen)
    # out=: the pinned block of the ring, filled in place
    out = np.full(O.table_words(n) + 5, -1, np.int32)
    got, _, _ = O.pack(_lib.CT_OPTIM_ADAM, items, out=out)
    assert got is out and np.array_equal(out[:-5], words) and (out[-5:] == -1).all()


def test_pack_refusals():
    from centertrack_amd import _lib, optim as O
    ok = fake_items([5, 9], 'adam')
    with pytest.raises(O.CTError, match='kind'):
        O.pack(7, ok)
    with pytest.raises(O.CTError, match='tensors outside'):
        O.pack(_lib.CT_OPTIM_ADAM, [])
    for col, val, what in ((0, 0, 'null'), (3, 0, 'null'), (1, ok[0][1] + 2, '4-byte'), (4, 0, 'without elements')):
        bad = [tuple(val if j == col else x for j, x in enumerate(ok[0])), ok[1]]
        with pytest.raises(O.CTError, match=what):
            O.pack(_lib.CT_OPTIM_ADAM, bad)
    sgd = fake_items([5], 'sgd')
    O.pack(_lib.CT_OPTIM_SGD, [tuple(0 if j == 2 else x for j, x in enumerate(sgd[0]))])    # no momentum buffer: fine
    with pytest.raises(O.CTError, match='out must be'):
        O.pack(_lib.CT_OPTIM_ADAM, ok, out=np.zeros(3, np.int32))
    with pytest.raises(O.CTError, match='chunks'):
        O.pack(_lib.CT_OPTIM_ADAM, [ok[0][:4] + (O.CHUNK << 31,) + ok[0][5:]])


def test_record_matches_the_header_layout(tmp_path):
    import shutil
    import subprocess
    from centertrack_amd import _lib, optim as O
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = ('p', 'g', 'm', 'v', 'numel', 's', 'first', 'reserved')
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "centertrack_hip.h"\nint main(void) {'
                   'printf("%zu %d %d %d %d %d %d' + ' %zu' * len(fields) + '\\n", sizeof(ct_optim_rec), CT_OPTIM_REC_BYTES, '
                   'CT_OPTIM_CHUNK, CT_OPTIM_SCALARS, CT_OPTIM_MAX_TENSORS, CT_OPTIM_ADAM, CT_OPTIM_SGD, '
                   + ', '.join('offsetof(ct_optim_rec, %s)' % f for f in fields) + '); return 0; }\n')
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(T.ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    D = _lib.OptimRec
    assert got[:7] == [ctypes.sizeof(D), _lib.CT_OPTIM_REC_BYTES, _lib.CT_OPTIM_CHUNK, _lib.CT_OPTIM_SCALARS,
                       _lib.CT_OPTIM_MAX_TENSORS, _lib.CT_OPTIM_ADAM, _lib.CT_OPTIM_SGD]
    assert got[7:] == [getattr(D, f).offset for f in fields] == [O.REC.fields[f][1] for f in fields]
    assert O.REC.itemsize == got[0] == 128 and got[0] & (got[0] - 1) == 0


def test_argument_checks_without_gpu():
    """ct_optim_step refuses before it enqueues anything"""
    from centertrack_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1024, np.int32)
    ptr = buf.ctypes.data

    def rejected(args, what):
        assert lib.ct_optim_step(*args) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error() and b'ct_optim_step' in lib.ct_last_error(), lib.ct_last_error()

    rejected((None, 1, 1, _lib.CT_OPTIM_ADAM, None), b'null table')
    rejected((ptr, 0, 1, _lib.CT_OPTIM_ADAM, None), b'tensors outside')
    rejected((ptr, -3, 1, _lib.CT_OPTIM_SGD, None), b'tensors outside')
    rejected((ptr, _lib.CT_OPTIM_MAX_TENSORS + 1, 1 << 21, _lib.CT_OPTIM_ADAM, None), b'tensors outside')
    rejected((ptr, 4, 3, _lib.CT_OPTIM_ADAM, None), b'chunks')
    rejected((ptr, 4, 1 << 31, _lib.CT_OPTIM_ADAM, None), b'chunks')
    rejected((ptr, 4, 4, 2, None), b'kind 2')
    rejected((ptr, 4, 4, -1, None), b'kind -1')


# ------------------------------------------------------------------ constructors
def cpu_params():
    torch.manual_seed(3)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def test_constructors_are_torchs():
    from centertrack_amd import optim as O
    for mine, theirs in ((O.Adam, torch.optim.Adam), (O.SGD, torch.optim.SGD)):
        assert issubclass(mine, theirs)
        a, b = inspect.signature(mine.__init__).parameters, inspect.signature(theirs.__init__).parameters
        assert list(a) == list(b) and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
        ps = cpu_params()
        for kw in (dict(lr=1.25e-4), dict(lr=3e-3, weight_decay=1e-4)):
            if mine is O.SGD:
                kw = dict(kw, momentum=0.9)
            groups = lambda: [{'params': ps[:1]}, {'params': ps[1:], 'lr': 0.5}]   # noqa: E731
            x, y = mine(groups(), **kw), theirs(groups(), **kw)
            assert x.defaults == y.defaults and x.param_groups == y.param_groups
            assert x.state_dict() == y.state_dict()
    assert O.Adam(cpu_params(), 1.25e-4).defaults == torch.optim.Adam(cpu_params(), 1.25e-4).defaults   # main.py's call


def test_state_dict_of_torch_adam_loads_bit_for_bit():
    from centertrack_amd import optim as O
    ps = cpu_params()
    theirs = torch.optim.Adam(ps, lr=1e-2)
    for s in range(2):
        for p in ps:
            p.grad = torch.full_like(p, 0.25 * (s + 1))
        theirs.step()
    sd = theirs.state_dict()
    mine = O.Adam(cpu_params(), lr=5.0)
    mine.load_state_dict(sd)
    assert mine.param_groups[0]['lr'] == 1e-2
    for (i, st), p in zip(sorted(sd['state'].items()), mine.param_groups[0]['params']):
        got = mine.state[p]
        assert set(got) == set(st) == {'step', 'exp_avg', 'exp_avg_sq'}
        for k in st:
            assert got[k].dtype == st[k].dtype and got[k].device == st[k].device and torch.equal(got[k], st[k]), (i, k)
        assert float(got['step']) == 2.0
    back = mine.state_dict()
    assert back['param_groups'] == sd['param_groups']
    assert all(torch.equal(back['state'][i][k], sd['state'][i][k]) for i in sd['state'] for k in sd['state'][i])


def test_refusals():
    from centertrack_amd import optim as O
    ps = cpu_params()
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
               dict(decoupled_weight_decay=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(O.CTError):
            O.Adam(ps, **kw)
    for kw in (dict(momentum=0.9, nesterov=True), dict(momentum=0.9, dampening=0.1), dict(maximize=True),
               dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(O.CTError):
            O.SGD(ps, **kw)
    # a flag switched on behind the constructor's back is caught by step()
    for opt, key in ((O.Adam(ps), 'amsgrad'), (O.SGD(ps, momentum=0.9), 'nesterov')):
        opt.param_groups[0][key] = True
        with pytest.raises(O.CTError, match=key):
            opt.step()
    # tensors that are not CUDA float32 contiguous dense: no CPU fallback
    for cls in (O.Adam, O.SGD):
        ps = cpu_params()
        for p in ps:
            p.grad = torch.ones_like(p)
        with pytest.raises(O.CTError, match='no CPU fallback'):
            cls(ps, lr=1e-3).step()
        assert all(len(s) == 0 for s in cls(ps, lr=1e-3).state.values())
    # nothing to do: no launch, no error, the closure is evaluated as torch does
    ps = cpu_params()
    calls = []

    def closure():
        assert torch.is_grad_enabled()
        calls.append(1)
        return torch.tensor(2.5)
    assert float(O.Adam(ps).step(closure)) == 2.5 and float(O.SGD(ps).step(closure)) == 2.5 and len(calls) == 2


def test_get_optimizer_restates_main():
    from centertrack_amd import optim as O
    model = torch.nn.Linear(3, 2)
    a = O.get_optimizer(types.SimpleNamespace(optim='adam', lr=1.25e-4), model)
    assert type(a) is O.Adam and a.defaults == torch.optim.Adam(model.parameters(), 1.25e-4).defaults
    s = O.get_optimizer(types.SimpleNamespace(optim='sgd', lr=0.01), model)
    assert type(s) is O.SGD
    assert s.defaults == torch.optim.SGD(model.parameters(), 0.01, momentum=0.9, weight_decay=0.0001).defaults
    with pytest.raises(AssertionError):
        O.get_optimizer(types.SimpleNamespace(optim='rmsprop', lr=0.01), model)


# ------------------------------------------------------------------ load_model resume, save_model
def tiny(group_lrs):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    optimizer = torch.optim.Adam([{'params': model[0].parameters(), 'lr': group_lrs[0]},
                                  {'params': model[1].parameters(), 'lr': group_lrs[1]}])
    model(torch.ones(4, 3)).sum().backward()
    optimizer.step()
    return model, optimizer


def state_bits(optimizer):
    return [[k, v.tolist()] for st in optimizer.state_dict()['state'].values() for k, v in sorted(st.items())]


def test_load_model_resume_against_the_reference(tmp_path, capsys):
    from centertrack_amd.model import load_model, save_model
    gold = json.load(open(GOLD))
    cases = gold['cases']
    assert sorted({c['epoch'] for c in cases}) == [0, 59, 60, 61, 120] and len(cases) == 40
    assert {tuple(c['lr_step']) for c in cases} == {(60,), (60, 120)}
    assert any(c['lr'] != [float(x).hex() for x in gold['group_lrs']] for c in cases)
    path = str(tmp_path / 'ckpt.pth')
    for c in cases:
        model, optimizer = tiny(gold['group_lrs'])
        save_model(path, c['epoch'], model, optimizer if c['optimizer_in_checkpoint'] else None)
        ckpt = torch.load(path, map_location='cpu')
        assert set(ckpt) == {'epoch', 'state_dict'} | ({'optimizer'} if c['optimizer_in_checkpoint'] else set())
        before = state_bits(optimizer)
        opt = types.SimpleNamespace(resume=c['resume'], lr=gold['lr'], lr_step=c['lr_step'], reset_hm=False, reuse_hm=False)
        m, o, start = load_model(model, path, opt, optimizer)
        assert m is model and o is optimizer
        assert start == c['start_epoch'], c
        assert [float(g['lr']).hex() for g in optimizer.param_groups] == c['lr'], c              # bitwise
        assert (state_bits(optimizer) == before) == c['state_untouched'] and c['state_untouched'], c
    # the reference's iterated product, not main.py's power
    two = [c for c in cases if c['epoch'] == 120 and c['lr_step'] == [60, 120] and c['resume'] and c['optimizer_in_checkpoint']]
    assert two and float.fromhex(two[0]['lr'][0]) == gold['lr'] * 0.1 * 0.1 != gold['lr'] * 0.1 ** 2
    capsys.readouterr()
    # optimizer=None: the bare model and the prints of before
    model, optimizer = tiny(gold['group_lrs'])
    save_model(path, 7, model, optimizer)
    assert load_model(model, path, types.SimpleNamespace(resume=True, lr=1.0, lr_step=[1])) is model
    assert capsys.readouterr().out == 'loaded {}, epoch 7\n'.format(path)
    assert load_model(model, path) is model


def test_save_model_round_trip(tmp_path):
    from centertrack_amd import optim as O
    from centertrack_amd.model import load_model, save_model
    model, _ = tiny((1e-3, 1e-3))
    optimizer = O.Adam(model.parameters(), 1.25e-4)
    path = str(tmp_path / 'model_last.pth')
    save_model(path, 3, model, optimizer)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    other, _ = tiny((1e-3, 1e-3))
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    opt = types.SimpleNamespace(resume=True, lr=1.25e-4, lr_step=[2, 5])
    m, o, start = load_model(other, path, opt, O.Adam(other.parameters(), 1.0))
    assert start == 3 and o.param_groups[0]['lr'] == 1.25e-4 * 0.1
    assert all(torch.equal(v, want[k]) for k, v in m.state_dict().items())
    ckpt = torch.load(path, map_location='cpu')
    assert ckpt['epoch'] == 3 and ckpt['optimizer']['param_groups'] == optimizer.state_dict()['param_groups']
    # DataParallel's wrapper is looked through, as in the reference
    save_model(path, 4, torch.nn.DataParallel(model))
    assert list(torch.load(path, map_location='cpu')['state_dict']) == list(want)


# ------------------------------------------------------------------ Trainer without a GPU
def test_trainer_refusals_and_loss_order():
    from centertrack_amd import trainer as TR
    from centertrack_amd._lib import CTError
    heads = {'hm': 1, 'tracking': 2, 'reg': 2, 'wh': 2}
    opt = types.SimpleNamespace(heads=heads, weights={h: 1 for h in heads}, num_stacks=1, debug=0, num_iters=-1,
                                print_iter=0, device='cpu')
    model = torch.nn.Linear(2, 2)
    tr = TR.Trainer(opt, model, torch.optim.SGD(model.parameters(), lr=0.1))
    assert tr.loss_stats == ['tot', 'hm', 'wh', 'reg', 'tracking']                # the reference's order
    assert isinstance(tr.model_with_loss, TR.ModelWithLoss) and tr.model_with_loss.model is model
    with pytest.raises(CTError, match='one GPU'):
        tr.set_device([0, 1], [4, 4], 'cpu')
    with pytest.raises(CTError, match='debug'):
        TR.Trainer(types.SimpleNamespace(**dict(vars(opt), debug=1)), model)
    opt.debug = 2
    with pytest.raises(CTError, match='debug'):
        tr.run_epoch('train', 1, [])
    opt.debug = 0
    with pytest.raises(CTError, match='optimizer'):
        TR.Trainer(opt, model).run_epoch('train', 1, [])
    assert list(inspect.signature(TR.Trainer.__init__).parameters)[1:] == ['opt', 'model', 'optimizer']
    assert list(inspect.signature(TR.Trainer.set_device).parameters)[1:] == ['gpus', 'chunk_sizes', 'device']
    assert list(inspect.signature(TR.Trainer.run_epoch).parameters)[1:] == ['phase', 'epoch', 'data_loader']
