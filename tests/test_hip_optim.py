"""GPU: ``centertrack_amd.optim.Adam`` / ``SGD`` (csrc/optim.hip) and ``centertrack_amd.trainer``.

Accuracy against torch's own float64 CPU trajectory with the project's bound (``_optim.bound``); independence of how the
tensors are split over optimizers and launches, bit for bit; sentinels around every tensor; the first Adam step of the
whole ``DLASeg`` (every element moves by lr against the sign of its gradient); state dicts crossing to and from
``torch.optim.Adam``; ``Trainer`` against a hand-written loop, without a host wait before the end of the epoch.

Measured on an MI355X, largest error over bound: Adam 0.333 (weight decay 0) and 0.390 (1e-4), SGD 0.250 and 0.336."""
import io
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _loss_ref as R
import _optim as T

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                          # a NaN payload no arithmetic produces
GUARD = 67                                     # sentinel words between two tensors (odd: the next start is re-aligned)


class Arena(object):
    """float32 tensors inside one buffer filled with the sentinel.  ``offsets_mod4[i]``: the residue of tensor i's first
    element (0: 16-byte aligned, the buffer's base being 256-byte aligned; 1..3: only 4-byte aligned)."""

    def __init__(self, device, sizes, offsets_mod4=None):
        offsets_mod4 = offsets_mod4 or [0] * len(sizes)
        self.spans, cur = [], GUARD
        for n, r in zip(sizes, offsets_mod4):
            off = (cur + 3) // 4 * 4 + r
            self.spans.append((off, n))
            cur = off + n + GUARD
        self.words = torch.full((cur + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        assert self.words.data_ptr() % 16 == 0
        self.buf = self.words.view(torch.float32)
        self.tensors = [self.buf[o:o + n] for o, n in self.spans]
        for t, r in zip(self.tensors, offsets_mod4):
            assert t.data_ptr() % 16 == 4 * r and t.is_contiguous()

    def fill(self, arrays):
        for t, a in zip(self.tensors, arrays):
            if a is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))

    def untouched(self):
        keep = torch.ones(self.words.numel(), dtype=torch.bool, device=self.words.device)
        for o, n in self.spans:
            keep[o:o + n] = False
        return bool((self.words[keep] == SENTINEL).all())


def residues():
    return [0] * len(T.SIZES) + [1, 3]


def make_params(device):
    params, _ = T.data()
    arena = Arena(device, T.SIZES + T.VIEW_SIZES, residues())
    arena.fill(params)
    return arena, [t.requires_grad_() for t in arena.tensors]


def lr_of(i):
    return T.LRS[0] if i < 5 else T.LRS[1]


def optim_class(kind):
    from centertrack_amd import optim as O
    return O.Adam if kind == 'adam' else O.SGD


def set_grads(tensors, garena, row):
    """fresh gradients of one step: views into the gradient arena, None where the step has none"""
    garena.fill(row)
    for t, g, a in zip(tensors, garena.tensors, row):
        t.grad = None if a is None else g


def state_of(opts, p):
    for o in opts:
        if p in o.state:
            return o.state[p]
    return {}


def snapshot(opts, tensors, kind):
    out = []
    for p in tensors:
        st = state_of(opts, p)
        out.append([p.detach().clone()] + [st[k].detach().clone() if st.get(k) is not None else None
                                           for k in T.STATE_KEYS[kind]])
    return out


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize('wd', [0, 1e-4])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_five_steps_against_torchs_float64_trajectory(device, kind, wd):
    ref64 = T.torch_trajectory(kind, wd, torch.float64)
    ref32 = T.torch_trajectory(kind, wd, torch.float32)
    _, grads = T.data()
    arena, tensors = make_params(device)
    garena = Arena(device, T.SIZES + T.VIEW_SIZES)           # gradients 16-byte aligned: the views mix alignments
    opt = optim_class(kind)(T.groups(tensors, kind, wd))
    names = ('p',) + T.STATE_KEYS[kind]
    worst = [0.0]
    for step, row in enumerate(grads):
        set_grads(tensors, garena, row)
        opt.step()
        snap = snapshot([opt], tensors, kind)
        for i, (got, want64, want32) in enumerate(zip(snap, ref64[step], ref32[step])):
            for name, g, w64, w32 in zip(names, got, want64, want32):
                assert (g is None) == (w64 is None), (step, i, name)
                if g is not None:
                    T.check_against(g.double().cpu().numpy(), w64, w32, '%s wd %g step %d tensor %d %s'
                                    % (kind, wd, step + 1, i, name), worst)
        if kind == 'adam':
            steps = [int(opt.state[p]['step']) if p in opt.state else 0 for p in tensors]
            assert steps == [int(ref_step) for ref_step in expected_steps(step)], step
            assert all(opt.state[p]['step'].device.type == 'cpu' and opt.state[p]['step'].dtype == torch.float32
                       for p in tensors if p in opt.state)
    assert arena.untouched() and garena.untouched()
    print('optim accuracy: %s weight_decay %g: largest error / bound %.3f' % (kind, wd, worst[0]))
    assert worst[0] > 0.0


def expected_steps(step):
    """the step counts after ``step + 1`` calls: a tensor without a gradient does not advance"""
    return [step + 1 - sum(1 for s in T.SKIP.get(i, ()) if s <= step) for i in range(len(T.SIZES + T.VIEW_SIZES))]


# ------------------------------------------------------------------ partition independence
def run_partition(device, kind, wd, how):
    _, grads = T.data()
    arena, tensors = make_params(device)
    garena = Arena(device, T.SIZES + T.VIEW_SIZES)
    cls = optim_class(kind)
    kw = dict(T.HYPER[kind], weight_decay=wd)
    idx = list(range(len(tensors)))
    if how == 'one':
        opts = [cls(T.groups(tensors, kind, wd))]
    elif how == 'each':
        opts = [cls([tensors[i]], lr=lr_of(i), **kw) for i in idx]
    else:                                                    # one optimizer, tensors and groups in reversed order
        opts = [cls([dict(params=[tensors[i] for i in reversed(idx) if i >= 5], lr=T.LRS[1], **kw),
                     dict(params=[tensors[i] for i in reversed(idx) if i < 5], lr=T.LRS[0], **kw)])]
    for row in grads[:3]:
        set_grads(tensors, garena, row)
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    return snapshot(opts, tensors, kind)


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_results_do_not_depend_on_the_partition(device, kind):
    base = run_partition(device, kind, 1e-4, 'one')
    for how in ('one', 'each', 'reversed'):
        other = run_partition(device, kind, 1e-4, how)
        for i, (a, b) in enumerate(zip(base, other)):
            for x, y in zip(a, b):
                assert (x is None) == (y is None) and (x is None or torch.equal(x.view(torch.int32), y.view(torch.int32))), (how, i)


# ------------------------------------------------------------------ extents
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_nothing_outside_the_tensors_is_written(device, kind):
    """p, g and (Adam) the pre-seeded exp_avg / exp_avg_sq all sit between sentinels, at every alignment; tensor 3 never has
    a gradient"""
    params, grads = T.data()
    sizes = T.SIZES + T.VIEW_SIZES
    arena, tensors = make_params(device)
    garena = Arena(device, sizes, [0] * len(T.SIZES) + [2, 3])
    opt = optim_class(kind)(T.groups(tensors, kind, 1e-4))
    state_arenas = []
    if kind == 'adam':
        for r in ([0] * len(T.SIZES) + [1, 0], [0] * len(T.SIZES) + [3, 1]):
            a = Arena(device, sizes, r)
            a.fill([np.zeros(n, np.float32) for n in sizes])
            state_arenas.append(a)
        for i, p in enumerate(tensors):
            if i != 3:
                opt.state[p] = {'step': torch.tensor(0.0), 'exp_avg': state_arenas[0].tensors[i],
                                'exp_avg_sq': state_arenas[1].tensors[i]}
    start = [p.detach().clone() for p in tensors]
    for step in range(3):
        set_grads(tensors, garena, [None if i == 3 else (g if g is not None else grads[0][i])
                                    for i, g in enumerate(grads[step])])
        before = [g.clone() for g in garena.tensors]
        opt.step()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, garena.tensors))
    torch.cuda.synchronize()
    for a in [arena, garena] + state_arenas:
        assert a.untouched()
    assert torch.equal(start[3].view(torch.int32), tensors[3].detach().view(torch.int32)) and tensors[3] not in opt.state
    moved = [i for i, p in enumerate(tensors) if not torch.equal(start[i], p.detach())]
    assert moved == [i for i in range(len(tensors)) if i != 3]
    for i, p in enumerate(tensors):
        if i != 3:
            st = opt.state[p]
            if kind == 'adam':
                assert int(st['step']) == 3 and st['exp_avg'].data_ptr() == state_arenas[0].tensors[i].data_ptr()
            assert all(bool(torch.isfinite(st[k]).all()) for k in T.STATE_KEYS[kind])


# ------------------------------------------------------------------ the whole model
def test_first_adam_steps_of_the_whole_model(device):
    from centertrack_amd import dcn_v2, losses, optim as O
    from test_hip_dlaseg import HEADS, UNREAD, build_model, data as dla_data, state_dict
    lr = 1.25e-4
    model = build_model(state_dict(), device).train()
    (x, pre, hm), batch = dla_data(device)
    crit = losses.GenericLoss(R.Opt(tuple(HEADS)))
    opt = O.Adam(model.parameters(), lr)
    named = dict(model.named_parameters())
    start = {k: p.detach().clone() for k, p in named.items()}

    def step():
        opt.zero_grad()
        with dcn_v2.trainable():
            crit(model(x, pre, hm), batch)[0].backward()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items()}
        opt.step()
        return grads
    grads = step()
    f32 = np.float32
    checked = 0
    for k, p in named.items():
        if k in UNREAD:
            assert grads[k] is None and p not in opt.state and torch.equal(p.detach(), start[k]), k
            continue
        old, new, g = (t.cpu().numpy() for t in (start[k], p.detach(), grads[k]))
        assert np.isfinite(new).all(), k
        ulp = np.spacing(np.maximum(np.abs(old), np.abs(new)).astype(f32)).astype(np.float64)
        delta = new.astype(np.float64) - old.astype(np.float64)
        assert (np.abs(delta) <= lr * (1 + 1e-3) + ulp).all(), k
        big = np.abs(g) >= 1e-4
        want = -lr * np.sign(g[big]).astype(np.float64)
        assert (np.abs(delta[big] - want) <= 1e-3 * lr + ulp[big]).all(), k
        checked += int(big.sum())
        assert int(opt.state[p]['step']) == 1
    assert checked > 1000
    for _ in range(2):
        step()
    for k, p in named.items():
        if k in UNREAD:
            assert torch.equal(p.detach(), start[k]), k
            continue
        moved = (p.detach().double() - start[k].double()).abs().max().item()
        assert moved <= 3 * 3.2 * lr, (k, moved)
        assert int(opt.state[p]['step']) == 3


# ------------------------------------------------------------------ checkpoints cross to torch.optim.Adam and back
def through_a_file(state_dict):
    """a checkpoint's trip (load_state_dict itself shares the tensors it is given)"""
    f = io.BytesIO()
    torch.save(state_dict, f)
    f.seek(0)
    return torch.load(f, map_location='cpu')


def test_state_dicts_cross_both_ways(device):
    from centertrack_amd import optim as O
    wd = 1e-4
    ref64 = T.torch_trajectory('adam', wd, torch.float64)
    ref32 = T.torch_trajectory('adam', wd, torch.float32)
    params, grads = T.data()

    def fresh():
        return [torch.tensor(p, device=device).requires_grad_() for p in params]

    def run(opt, tensors, rows):
        for row in rows:
            for t, g in zip(tensors, row):
                t.grad = None if g is None else torch.tensor(g, device=device)
            opt.step()

    def check(opt, tensors, what):
        worst = [0.0]
        for i, (p, want64, want32) in enumerate(zip(tensors, ref64[2], ref32[2])):
            got = [p.detach()] + [opt.state[p][k] for k in T.STATE_KEYS['adam']]
            for g, w64, w32 in zip(got, want64, want32):
                T.check_against(g.double().cpu().numpy(), w64, w32, '%s tensor %d' % (what, i), worst)
        assert [int(opt.state[p]['step']) for p in tensors] == expected_steps(2)
        return worst[0]
    # two steps here, the third by torch
    a = fresh()
    mine = O.Adam(T.groups(a, 'adam', wd))
    run(mine, a, grads[:2])
    b = [t.detach().clone().requires_grad_() for t in a]
    theirs = torch.optim.Adam(T.groups(b, 'adam', wd))
    theirs.load_state_dict(through_a_file(mine.state_dict()))
    run(theirs, b, grads[2:3])
    run(mine, a, grads[2:3])
    r1, r2 = check(theirs, b, 'torch after ours'), check(mine, a, 'ours throughout')
    # two steps by torch, the third here
    c = fresh()
    theirs = torch.optim.Adam(T.groups(c, 'adam', wd))
    run(theirs, c, grads[:2])
    d = [t.detach().clone().requires_grad_() for t in c]
    mine = O.Adam(T.groups(d, 'adam', wd))
    mine.load_state_dict(through_a_file(theirs.state_dict()))
    assert all(mine.state[p]['exp_avg'].is_cuda for p in d)
    run(mine, d, grads[2:3])
    r3 = check(mine, d, 'ours after torch')
    print('optim crossing: largest error / bound %.3f (torch after ours), %.3f (ours), %.3f (ours after torch)' % (r1, r2, r3))


# ------------------------------------------------------------------ Trainer
TR_HEADS = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2)])
BATCH_SIZES = (2, 2, 1, 2)


class HeadsOnFeatures(torch.nn.Module):
    """the fused heads on the batch's feature map, in the ``model(image, pre_img, pre_hm)`` convention: no atomics anywhere
    in its step, so two runs agree bit for bit"""

    def __init__(self):
        super().__init__()
        from centertrack_amd.heads import FusedHeads
        self.heads = FusedHeads(TR_HEADS, head_conv=32, in_channels=64)

    def forward(self, image, pre_img=None, pre_hm=None):
        return [self.heads(image)]


def tr_batches():
    out = []
    for i, B in enumerate(BATCH_SIZES):
        _, batch = R.make_batch(900 + i, B, 8, 12, 8, tuple(TR_HEADS), 1)
        g = torch.Generator().manual_seed(950 + i)
        batch['image'] = torch.randn(B, 64, 8, 12, generator=g)
        batch['meta'] = {'note': 'stays on the host'}
        out.append(batch)
    return out


def tr_opt(device, **kw):
    opt = R.Opt(tuple(TR_HEADS))
    opt.num_iters, opt.print_iter, opt.debug, opt.device, opt.task, opt.exp_id = -1, 0, 0, device, 'tracking', 'test'
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def tr_model(sd=None):
    torch.manual_seed(77)
    m = HeadsOnFeatures()
    if sd is not None:
        m.load_state_dict(sd)
    return m


class DeviceReads(object):
    """counts what makes the host wait for the device: reads of CUDA tensors and synchronize calls"""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
            monkeypatch.setattr(torch.Tensor, name, self._tensor(getattr(torch.Tensor, name)))
        for owner in (torch.cuda, torch.cuda.Stream, torch.cuda.Event):
            monkeypatch.setattr(owner, 'synchronize', self._always(getattr(owner, 'synchronize')))

    def _tensor(self, fn):
        def wrapped(t, *a, **k):
            if t.is_cuda:
                self.n += 1
            return fn(t, *a, **k)
        return wrapped

    def _always(self, fn):
        def wrapped(*a, **k):
            self.n += 1
            return fn(*a, **k)
        return wrapped


def lines(capsys):
    return [l for l in capsys.readouterr().out.splitlines() if l.startswith('tracking/test|')]


def test_trainer_against_a_hand_written_loop(device, monkeypatch, capsys):
    from centertrack_amd import optim as O
    from centertrack_amd.losses import GenericLoss
    from centertrack_amd.trainer import ModelWithLoss, Trainer
    sd = {k: v.clone() for k, v in tr_model().state_dict().items()}
    names = ['tot', 'hm', 'wh', 'reg']
    # the hand-written loop: zero_grad, backward, step; the statistics read afterwards
    opt = tr_opt(device)
    model = tr_model(sd).to(device)
    mwl = ModelWithLoss(model, GenericLoss(opt)).train()
    adam = O.Adam(model.parameters(), 1e-3)
    kept = []
    reads = DeviceReads(monkeypatch)
    for batch in tr_batches():
        for k in batch:
            if k != 'meta':
                batch[k] = batch[k].to(device=device, non_blocking=True)
        _, loss, stats = mwl(batch)
        adam.zero_grad()
        loss.mean().backward()
        adam.step()
        kept.append(([stats[l].detach().mean() for l in names], batch['image'].size(0)))
    hand_reads = reads.n
    sums, count = [0.0] * len(names), 0
    for vals, n in kept:
        for j, v in enumerate(vals):
            sums[j] += v.item() * n                              # AverageMeter.update(val, n)
        count += n
    want = {l: s / count for l, s in zip(names, sums)}
    hand = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert hand_reads == 0 and any(not torch.equal(hand[k], sd[k].to(device)) for k in hand)
    # Trainer.train
    model2 = tr_model(sd)
    adam2 = O.Adam(model2.parameters(), 1e-3)
    tr = Trainer(opt, model2, adam2)
    tr.set_device([0], [2], device)
    reads.n = 0
    ret, results = tr.train(1, tr_batches())
    assert reads.n == 1                                          # the one read at the end of the epoch
    assert results == {} and list(ret) == names + ['time'] and ret['time'] >= 0.0
    assert {l: ret[l] for l in names} == want
    got = model2.state_dict()
    assert all(torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                           hand[k].view(torch.int32) if hand[k].dtype == torch.float32 else hand[k]) for k in hand)
    assert all(int(adam2.state[p]['step']) == len(BATCH_SIZES) for p in model2.parameters())
    assert len(lines(capsys)) == 1                               # print_iter = 0: the closing line only
    # val: nothing moves; print_iter = 1 prints (and reads) every iteration
    opt.print_iter = 1
    reads.n = 0
    ret_val, _ = tr.val(1, tr_batches())
    assert reads.n == len(BATCH_SIZES) + 1
    assert len(lines(capsys)) == len(BATCH_SIZES) + 1
    assert list(ret_val) == names + ['time'] and all(np.isfinite(ret_val[l]) for l in names)
    assert all(torch.equal(v, got[k]) for k, v in model2.state_dict().items())
    assert all(int(adam2.state[p]['step']) == len(BATCH_SIZES) for p in model2.parameters())
    # num_iters
    opt.print_iter, opt.num_iters = 0, 2
    model3 = tr_model(sd)
    adam3 = O.Adam(model3.parameters(), 1e-3)
    tr3 = Trainer(opt, model3, adam3)
    tr3.set_device([0], [2], device)
    tr3.train(2, tr_batches())
    assert all(int(adam3.state[p]['step']) == 2 for p in model3.parameters())
    # set_device moves an optimizer state that was loaded on the host, as the reference's does; the next step takes it
    model4 = tr_model(sd)
    adam4 = O.Adam(model4.parameters(), 1e-3)
    adam4.load_state_dict(adam3.state_dict())                    # (cast to where the parameters are: the host)
    assert not any(st['exp_avg'].is_cuda for st in adam4.state.values())
    opt.num_iters = 1
    tr4 = Trainer(opt, model4, adam4)
    tr4.set_device([0], [2], device)
    assert all(st['exp_avg'].is_cuda and st['step'].is_cuda for st in adam4.state.values())
    tr4.train(3, tr_batches())
    assert all(int(st['step']) == 3 and st['step'].device.type == 'cpu' for st in adam4.state.values())
