"""One rank of the multi-process jobs of tests/test_hip_dist_train.py, started under ``python -m torch.distributed.run``:
``--job world1`` (one rank, RCCL), ``--job world2`` (two ranks; ``--backend gloo`` with both on ``cuda:0``, or ``nccl`` with
one GPU each; ``--trainer`` adds the ``Trainer`` epoch on ``DLASeg``).  Every rank writes what it found as JSON to
``<out>.<rank>``; tensors go in as SHA-256 digests of their bits, so that the test compares ranks by comparing strings."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (HERE, ROOT):
    if path not in sys.path:
        sys.path.insert(0, path)

CHUNK = 4096
NUMELS = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5]
STEPS = 3
MAX_NORM = 1.0                                   # far below the norms of this data (about 1e2): every step is clipped
STATE_KEYS = {'adam': ('exp_avg', 'exp_avg_sq'), 'sgd': ('momentum_buffer',)}


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def initial(device):
    g = torch.Generator().manual_seed(4100)
    return [torch.randn(n, generator=g).to(device).requires_grad_() for n in NUMELS]


def data_of(rank, device):
    """a_r: what rank r multiplies the parameters by"""
    g = torch.Generator().manual_seed(4200 + rank)
    return [(torch.randn(n, generator=g) * 2.0).to(device) for n in NUMELS]


def gradients(params, a):
    """d/dp of sum_t sum(sin(p_t a_t)): elementwise, so two runs give the same bits"""
    loss = sum((p * x).sin().sum() for p, x in zip(params, a))
    return list(torch.autograd.grad(loss, params))


def make(kind, params, guard):
    from centertrack_amd import optim as O
    opt = O.Adam(params, 1e-2, weight_decay=1e-4) if kind == 'adam' else O.SGD(params, 1e-2, momentum=0.9, weight_decay=1e-4)
    if guard:
        opt.guard(MAX_NORM, skip_nonfinite=True)
    return opt


def state_of(opt, params, kind):
    out = list(params)
    for p in params:
        out += [opt.state[p][k] for k in STATE_KEYS[kind]]
        if kind == 'adam':
            out.append(opt.state[p]['step'])
    return out


def run(kind, guard, device, grads_fn, distribute, inf_rank=None, rank=0):
    """STEPS steps from the common start; ``grads_fn(params) -> gradients``.  Returns (optimizer, params, digests after
    every step, extras)."""
    params = initial(device)
    opt = make(kind, params, guard)
    if distribute:
        opt.distribute()
    after, stats, reduced_equal = [], [], True
    for step in range(STEPS):
        grads = grads_fn(params)
        if inf_rank is not None and step == 1 and inf_rank == rank:
            grads[2][7] = float('inf')
        for p, g in zip(params, grads):
            p.grad = g
        kept = [g.clone() for g in grads]
        opt.step()
        if distribute:
            red = opt.reduced_grads()
            reduced_equal = reduced_equal and all(torch.equal(r.view(torch.int32), g.view(torch.int32))
                                                  for r, g in zip(red, kept))
        assert all(torch.equal(p.grad.view(torch.int32), k.view(torch.int32)) for p, k in zip(params, kept))   # never written
        after.append([digest(state_of(opt, params, kind)), digest(params)])      # (everything, the parameters alone)
        if guard:
            st = opt.grad_stats()
            stats.append([st['norm'], st['coef'], int(st['skip']), st['skipped'], st['clipped'], st['nonfinite']])
    return opt, params, after, dict(stats=stats, reduced_equal=reduced_equal)


def job_world1(rank, world, device, out):
    """distributed against plain, the same data: the scale is 1 and the sum over one rank is the identity"""
    import torch.distributed as dist
    from centertrack_amd._lib import CTError
    out['backend'] = dist.get_backend()
    a = data_of(0, device)
    for kind in ('adam', 'sgd'):
        for guard in (False, True):
            key = '%s%s' % (kind, '_guard' if guard else '')
            opt, params, got, extra = run(kind, guard, device, lambda ps: gradients(ps, a), True)
            _, _, want, extra0 = run(kind, guard, device, lambda ps: gradients(ps, a), False)
            out[key] = dict(dist=got, plain=want, reduced_equal=extra['reduced_equal'], stats=extra['stats'],
                            stats_plain=extra0['stats'])
            opt.check_in_sync()
    # the layout is fixed by the first distributed step: a tensor that loses its gradient is refused, before any collective
    for p, g in zip(params, gradients(params, a)):
        p.grad = g
    params[1].grad = None
    before = digest(params)
    try:
        opt.step()
        out['layout_change'] = 'accepted'
    except CTError as e:
        out['layout_change'] = str(e)
    out['layout_change_moved'] = digest(params) != before


def job_world2(rank, world, device, out):
    import torch.distributed as dist
    from centertrack_amd._lib import CTError
    out['backend'] = dist.get_backend()
    a = [data_of(r, device) for r in range(world)]

    def emulated(ps, inf=False):
        g0, g1 = gradients(ps, a[0]), gradients(ps, a[1])
        if inf:
            g1[2][7] = float('inf')
        return [x * 0.5 + y * 0.5 for x, y in zip(g0, g1)]
    for kind in ('adam', 'sgd'):
        for guard in (False, True):
            key = '%s%s' % (kind, '_guard' if guard else '')
            opt, params, got, extra = run(kind, guard, device, lambda ps: gradients(ps, a[rank]), True)
            _, _, emul, extra_e = run(kind, guard, device, emulated, False)
            _, _, alone, _ = run(kind, guard, device, lambda ps: gradients(ps, a[0]), False)
            out[key] = dict(dist=got, emulated=emul, rank0_alone=alone, stats=extra['stats'], stats_emulated=extra_e['stats'])
        # an Inf in rank 1's gradient only, at step 2: every rank skips that step
        calls = [0]

        def emulated_inf(ps):
            calls[0] += 1
            return emulated(ps, inf=calls[0] == 2)
        opt, params, got, extra = run(kind, True, device, lambda ps: gradients(ps, a[rank]), True, inf_rank=1, rank=rank)
        _, _, emul, _ = run(kind, True, device, emulated_inf, False)
        out[kind + '_inf'] = dict(dist=got, emulated=emul, stats=extra['stats'])
    # check_in_sync: passes, then raises on both ranks after rank 1 moved one element
    try:
        opt.check_in_sync()
        out['in_sync'] = 'ok'
    except CTError as e:
        out['in_sync'] = str(e)
    if rank == 1:
        with torch.no_grad():
            params[4][100] += 1e-3
    try:
        opt.check_in_sync()
        out['out_of_sync'] = 'ok'
    except CTError as e:
        out['out_of_sync'] = str(e)


def job_trainer(rank, world, device, out):
    """Trainer on DLASeg(34) at 2 x 64 x 64 per rank, Adam, one epoch of two iterations, the ranks on different data"""
    import _loss_ref as R
    from test_dlaseg_cpu import HEAD_CONVS, HEADS, Opt
    from centertrack_amd import optim as O, weights as Wt
    from centertrack_amd.dla_seg import DLASeg
    from centertrack_amd.trainer import Trainer
    N, H, W = 2, 64, 64
    model = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    model.load_state_dict(Wt.make_synthetic_state_dict(HEADS, seed=5200 + rank))     # another start on every rank
    opt = R.Opt(tuple(HEADS))
    opt.num_iters, opt.print_iter, opt.debug, opt.device, opt.task, opt.exp_id = -1, 0, 0, device, 'tracking', 'dist'
    opt.optim, opt.lr = 'adam', 1.25e-4
    out['constructed'] = digest(list(model.parameters()))
    tr = Trainer(opt, model, O.get_optimizer(opt, model))
    tr.set_device(list(range(world)), [N] * world, device)
    names = [k for k, _ in model.named_parameters()]
    start = [p.detach().clone() for p in model.parameters()]
    out['before'] = digest(start)
    out['buffers_before'] = digest(list(model.buffers()))
    batches = []
    for i in range(2):
        seed = 6000 + 10 * rank + i
        _, batch = R.make_batch(seed, N, H // 4, W // 4, 8, tuple(HEADS), 1)
        batch['image'], batch['pre_img'], batch['pre_hm'] = Wt.synthetic_inputs(N, H, W, seed=seed)
        batches.append(batch)
    ret, _ = tr.train(1, batches)
    torch.cuda.synchronize()
    out['ret'] = {k: v for k, v in ret.items() if k != 'time'}
    out['after'] = digest(list(model.parameters()))
    out['buffers_after'] = digest(list(model.buffers()))
    out['unmoved'] = [k for k, p, s in zip(names, model.parameters(), start) if torch.equal(p, s)]
    out['n_params'] = len(names)
    try:
        tr.optimizer.check_in_sync()
        out['in_sync'] = 'ok'
    except Exception as e:
        out['in_sync'] = str(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--job', required=True, choices=['world1', 'world2'])
    ap.add_argument('--backend', required=True, choices=['nccl', 'gloo'])
    ap.add_argument('--trainer', action='store_true')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    from centertrack_amd import parallel
    rank, world, local = parallel.init_from_env(backend=args.backend)
    device = torch.device('cuda', local if args.backend == 'nccl' else 0)
    torch.cuda.set_device(device)
    out = dict(rank=rank, world=world, device=str(device))
    if args.job == 'world1':
        job_world1(rank, world, device, out)
    else:
        job_world2(rank, world, device, out)
        if args.trainer:
            job_trainer(rank, world, device, out)
    parallel.barrier()
    with open('%s.%d' % (args.out, rank), 'w') as f:
        json.dump(out, f)
    parallel.shutdown()


if __name__ == '__main__':
    main()
