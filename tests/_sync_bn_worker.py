"""One rank of the multi-process jobs of tests/test_hip_sync_bn.py, started under ``python -m torch.distributed.run``:
``--job world2`` (two ranks; ``--backend gloo`` with both on ``cuda:0``, or ``nccl`` with one GPU each): the ops through a
real group, the three BatchNorm sites, ``Trainer`` on ``DLASeg`` with ``opt.sync_bn``; ``--job world1`` (one rank, RCCL): the
synchronised path forced in a group of one.  Every rank writes what it found to ``<out>.<rank>.json`` -- tensors compared
bit for bit go in as SHA-256 digests -- and the tensors the test holds against references to ``<out>.<rank>.pt``."""
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

SITES = ('deform', 'block', 'stems')
STEPS = 3


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ the ops
def job_ops(rank, world, device, out):
    import _sync_bn as SB
    found = {}
    for sl in SB.TWO_RANK_LISTS:
        for form in SB.FORMS:
            case = SB.sync_case(sl[0], sl[1], residual=form == 'backbone')
            got = SB.through_group(case, sl[1], form, rank, device)
            emu = SB.emulate(case, sl[1], form, device)
            mine = [got['y'].buf, got['gz'].buf] + ([got['gres'].buf] if got['gres'] is not None else [])
            emu_mine = [emu['y'][rank].buf, emu['gz'][rank].buf] + ([emu['gres'][rank].buf] if form == 'backbone' else [])
            found['%s %s' % (SB.list_id(sl), form)] = dict(
                merged=digest(SB.merged_vectors(got['m'])), emulated_merged=digest(SB.merged_vectors(emu['m'])),
                total=digest([got['total']]), emulated_total=digest([emu['total']]),
                mine=digest(mine), emulated_mine=digest(emu_mine))
    out['ops'] = found


# ------------------------------------------------------------------ the three sites
def build_site(site, device):
    """(module in training mode on the device, its fp32 state dict)"""
    import _backbone_bwd as BB
    import _neck_bwd as NB
    import _stem_bwd as ST
    from centertrack_amd.dla_base import BasicBlock
    from centertrack_amd.dla_up import DeformConv
    if site == 'deform':
        m = DeformConv(64, 64)
        sd = NB.deform_params(7100, 64, 64)
    elif site == 'block':
        m = BasicBlock(64, 64)
        sd = BB.random_params(7200, m)
    else:
        m = ST.Stems()
        sd = ST.params(7300)
    m.load_state_dict(sd)
    return m.to(device).train(), sd


def site_inputs(site):
    """(inputs, G) for a batch of two, NCHW fp32 on the CPU; sample 1 lives at another scale and offset than sample 0, so
    that the statistics of the two ranks differ by far more than any bound"""
    import _neck_bwd as NB
    import _stem_bwd as ST
    if site == 'stems':
        xs = ST.inputs(7500, 2, 8, 8)
        G = ST.output_gradient(7501, 2, 8, 8)
    else:
        xs = [NB.randn(7400, 2, 64, 5, 7).float()]
        G = NB.randn(7401, 2, 64, 5, 7).float()
    xs[0][1] = xs[0][1] * 2.0 + 1.5
    return xs, G


def call_site(site, m, ins):
    from centertrack_amd import dla_base
    import _stem_bwd as ST
    if site == 'stems':
        return dla_base._stems(ins, [getattr(m, p[:-1]) for p in ST.PREFIX]).permute(0, 3, 1, 2)
    return m(ins[0])


def run_site(site, m, xs, G, device, weight, backward=True):
    """forward (+ backward of ``weight * sum(out * G)``) -> dict(out, gin, grads, buffers), the gradients still on the device"""
    from centertrack_amd import dcn_v2
    m.zero_grad(set_to_none=True)
    ins = [x.to(device).requires_grad_(backward) for x in xs]
    with dcn_v2.trainable(), torch.set_grad_enabled(backward):
        y = call_site(site, m, ins)
        if backward:
            (weight * (y * G.to(device)).sum()).backward()
    torch.cuda.synchronize()
    return dict(out=y.detach().cpu().contiguous(), gin=[x.grad for x in ins] if backward else [],
                grads={k: p.grad for k, p in m.named_parameters()} if backward else {},
                buffers={k: b.detach().cpu().clone() for k, b in m.named_buffers()})


def to_cpu(run):
    return dict(out=run['out'], gin=[g.cpu() for g in run['gin']], grads={k: g.cpu() for k, g in run['grads'].items()},
                buffers=run['buffers'])


def job_sites(rank, world, device, out, tensors):
    from centertrack_amd import parallel
    for site in SITES:
        xs, G = site_inputs(site)
        mine, G_mine = [x[rank:rank + 1].contiguous() for x in xs], G[rank:rank + 1].contiguous()
        # marked, one sample per rank; the parameter gradients are averaged over the ranks as the distributed step does
        m, sd = build_site(site, device)
        parallel.sync_batchnorm(m)
        got = run_site(site, m, mine, G_mine, device, 1.0)
        keys = list(got['grads'])
        flat = torch.cat([got['grads'][k].reshape(-1) for k in keys])
        parallel.all_reduce_flat(flat)
        flat *= 1.0 / world
        at = 0
        for k in keys:
            n = got['grads'][k].numel()
            got['grads'][k] = flat[at:at + n].view(got['grads'][k].shape).clone()
            at += n
        res = to_cpu(got)
        # the same module unmarked, in one process, on the batch of two at weight 1 / world
        m, _ = build_site(site, device)
        res['single'] = to_cpu(run_site(site, m, xs, G, device, 1.0 / world))
        # unmarked on two ranks: per-rank statistics
        m, _ = build_site(site, device)
        res['unsynced_buffers'] = run_site(site, m, mine, G_mine, device, 1.0, backward=False)['buffers']
        res.update(sd=sd, inputs=xs, G=G)
        tensors[site] = res


# ------------------------------------------------------------------ Trainer on DLASeg
def trainer_batches(rank, device, n, nan=False):
    """the data of the world-2 trainer job of tests/_dist_train_worker.py: 2 x 64 x 64 per rank, other seeds on every rank"""
    import _loss_ref as R
    from test_dlaseg_cpu import HEADS
    from centertrack_amd import weights as Wt
    N, H, W = 2, 64, 64
    batches = []
    for i in range(n):
        seed = 6000 + 10 * rank + i
        _, batch = R.make_batch(seed, N, H // 4, W // 4, 8, tuple(HEADS), 1)
        batch['image'], batch['pre_img'], batch['pre_hm'] = Wt.synthetic_inputs(N, H, W, seed=seed)
        if nan:
            batch['image'] = batch['image'].clone()
            batch['image'][1, 2, 5, 7] = float('nan')
        batches.append(batch)
    return batches


def make_trainer(rank, world, device, sync_bn):
    import _loss_ref as R
    from test_dlaseg_cpu import HEAD_CONVS, HEADS, Opt
    from centertrack_amd import optim as O, weights as Wt
    from centertrack_amd.dla_seg import DLASeg
    from centertrack_amd.trainer import Trainer
    model = DLASeg(34, HEADS, HEAD_CONVS, Opt())
    model.load_state_dict(Wt.make_synthetic_state_dict(HEADS, seed=5200 + rank))     # another start on every rank
    opt = R.Opt(tuple(HEADS))
    opt.num_iters, opt.print_iter, opt.debug, opt.device, opt.task, opt.exp_id = -1, 0, 0, device, 'tracking', 'sync_bn'
    opt.optim, opt.lr = 'adam', 1.25e-4
    opt.skip_nonfinite = True
    opt.sync_bn = sync_bn
    tr = Trainer(opt, model, O.get_optimizer(opt, model))
    tr.set_device(list(range(world)), [2] * world, device)
    return tr, model


def job_trainer(rank, world, device, out):
    from centertrack_amd import parallel
    found = {}
    calls = {'buffers': 0}
    real = parallel.broadcast_module

    def spy(module, src=0, group=None, parameters=True, buffers=True):
        if not parameters and buffers:
            calls['buffers'] += 1
        return real(module, src=src, group=group, parameters=parameters, buffers=buffers)
    parallel.broadcast_module = spy
    try:
        tr, model = make_trainer(rank, world, device, True)
        bns = [b for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d)]
        found['n_bn'], found['marked'] = len(bns), sum(1 for b in bns if parallel.sync_batchnorm_of(b) is not None)
        found['before'] = digest(list(model.parameters()))
        found['buffers_before'] = digest(list(model.buffers()))
        ret, _ = tr.train(1, trainer_batches(rank, device, STEPS))
        torch.cuda.synchronize()
        found['buffer_broadcasts'] = calls['buffers']
        found['ret'] = {k: v for k, v in ret.items() if k != 'time'}
        found['after'] = digest(list(model.parameters()))
        found['buffers_after'] = digest(list(model.buffers()))
        try:
            tr.check_in_sync()
            found['in_sync'] = 'ok'
        except Exception as e:
            found['in_sync'] = str(e)
        # check_in_sync sees a buffer that rank 1 moved (and the element goes back)
        buf = bns[3].running_mean
        kept = buf.clone()
        if rank == 1:
            with torch.no_grad():
                buf[0] += 1e-3
        try:
            tr.check_in_sync()
            found['buffers_out_of_sync'] = 'ok'
        except Exception as e:
            found['buffers_out_of_sync'] = str(e)
        with torch.no_grad():
            buf.copy_(kept)
        # a NaN in rank 1's input only: the guarded step skips on both ranks
        ret, _ = tr.train(2, trainer_batches(rank, device, 1, nan=rank == 1))
        torch.cuda.synchronize()
        found['nan_skipped'] = int(ret['skipped'])
        found['nan_after'] = digest(list(model.parameters()))
        # the same job with sync_bn off: rank 0's running statistics, broadcast after the epoch
        calls['buffers'] = 0
        tr, model = make_trainer(rank, world, device, False)
        tr.train(1, trainer_batches(rank, device, STEPS))
        torch.cuda.synchronize()
        found['plain_buffer_broadcasts'] = calls['buffers']
        found['plain_buffers_after'] = digest(list(model.buffers()))
    finally:
        parallel.broadcast_module = real
    out['trainer'] = found


# ------------------------------------------------------------------ world 1 on RCCL
def job_world1(rank, world, device, out, tensors):
    """a BasicBlock on a batch of two, the synchronised path forced in a group of one rank against the unforced step"""
    import torch.distributed as dist
    from centertrack_amd import parallel
    out['backend'] = dist.get_backend()
    xs, G = site_inputs('block')
    m, sd = build_site('block', device)
    parallel.sync_batchnorm(m)                               # marked, world 1, not forced: today's path, no collective
    parallel.reset_collective_counts()
    plain = to_cpu(run_site('block', m, xs, G, device, 0.5))
    out['unforced_gathers'] = parallel.COLLECTIVES['all_gather_rows'] + parallel.COLLECTIVES['all_reduce_flat']
    m, _ = build_site('block', device)
    parallel.sync_batchnorm(m, force=True)
    parallel.reset_collective_counts()
    forced = to_cpu(run_site('block', m, xs, G, device, 0.5))
    out['gathers'], out['reduces'] = parallel.COLLECTIVES['all_gather_rows'], parallel.COLLECTIVES['all_reduce_flat']
    tensors['world1'] = dict(plain=plain, forced=forced, sd=sd, inputs=xs, G=G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--job', required=True, choices=['world1', 'world2'])
    ap.add_argument('--backend', required=True, choices=['nccl', 'gloo'])
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    from centertrack_amd import parallel
    rank, world, local = parallel.init_from_env(backend=args.backend)
    device = torch.device('cuda', local if args.backend == 'nccl' else 0)
    torch.cuda.set_device(device)
    out, tensors = dict(rank=rank, world=world, device=str(device)), {}
    if args.job == 'world1':
        job_world1(rank, world, device, out, tensors)
    else:
        import torch.distributed as dist
        out['backend'] = dist.get_backend()
        job_ops(rank, world, device, out)
        job_sites(rank, world, device, out, tensors)
        job_trainer(rank, world, device, out)
    parallel.barrier()
    torch.save(tensors, '%s.%d.pt' % (args.out, rank))
    with open('%s.%d.json' % (args.out, rank), 'w') as f:
        json.dump(out, f)
    parallel.shutdown()


if __name__ == '__main__':
    main()
