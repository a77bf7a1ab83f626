"""One ``DLASeg`` training step with and without synchronised BatchNorm, on ONE GPU.

``DLASeg(34, MOT heads)`` in training mode at 512x512, batch 1 and 4, under ``dcn_v2.trainable()``: forward, a loss that is
linear in the outputs (``sum_h <out_h, G_h>`` with fixed random ``G``: the targets are none of this measurement's business),
backward, the distributed ``centertrack_amd.optim.Adam`` step.  A process group of ONE rank on RCCL is created, so every
collective is a real one -- and costs what a collective among one rank costs: a launch and a copy.  Two contestants on the
same model, alternating in one process:

  unmarked   ``parallel.sync_batchnorm(model, False)``: per-replica BatchNorm, the gradient all-reduce of the step only
  forced     ``parallel.sync_batchnorm(model, force=True)``: every BatchNorm site through ``ct_bn_stats_row`` -> all-gather ->
             ``ct_bn_merge_stats`` forward and sums -> all-reduce -> apply backward

Per contestant and batch: ``ms_device`` -- device events around ``steps`` steps, per step, the minimum over the rounds;
``ms_wall`` -- the host clock around the same steps ending in a device synchronise; ``launches`` -- kernels and copies of one
step from the torch profiler (null when it is not available); ``collectives`` -- calls and payload bytes of
``all_gather_rows`` and ``all_reduce_flat`` in one step, counted by ``parallel.COLLECTIVES`` in a run of one step (the
gradient all-reduce of the optimizer is one of the ``all_reduce_flat`` calls in both contestants).

What this cannot show: the cost at world >= 2.  One GPU measures the added launches, the merge and the host work; a
collective between two GPUs waits for the slowest rank and crosses the fabric, and nothing here times that.

    python tools/sync_bn_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--batches 1,4] [--size 512]

appends one line per batch to profiles/sync_bn_bench.jsonl."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.dist_step_bench import one_rank_group  # noqa: E402
from tools.optim_bench import HEADS, Opt, count_launches  # noqa: E402


def measure(batch, size, steps, warmup, rounds, dev):
    import torch
    from centertrack_amd import dcn_v2, optim as O, parallel
    from centertrack_amd.dla_seg import DLASeg
    g = torch.Generator().manual_seed(3200 + batch)
    model = DLASeg(34, HEADS, {h: [256] for h in HEADS}, Opt()).to(dev).train()
    opt = O.Adam(model.parameters(), lr=1.25e-4).distribute()
    image, pre_img = (torch.randn((batch, 3, size, size), generator=g).to(dev) for _ in range(2))
    pre_hm = torch.rand((batch, 1, size, size), generator=g).to(dev)
    G = {h: (torch.randn((batch, c, size // 4, size // 4), generator=g) / (batch * size * size / 16) ** 0.5).to(dev)
         for h, c in HEADS.items()}

    def step():
        opt.zero_grad()
        with dcn_v2.trainable():
            out = model(image, pre_img, pre_hm)[-1]
            sum((out[h] * G[h]).sum() for h in HEADS).backward()
        opt.step()
    contestants = {'unmarked': lambda: parallel.sync_batchnorm(model, False),
                   'forced': lambda: parallel.sync_batchnorm(model, force=True)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    wall, device = {k: [] for k in contestants}, {k: [] for k in contestants}
    collectives, launches = {}, {}
    for name, mark in contestants.items():
        mark()
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        parallel.reset_collective_counts()
        step()
        torch.cuda.synchronize()
        collectives[name] = dict(parallel.COLLECTIVES)
        launches[name] = count_launches(types.SimpleNamespace(step=step))
    for _ in range(rounds):
        for name, mark in contestants.items():
            mark()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for _ in range(steps):
                step()
            ev[1].record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            device[name].append(ev[0].elapsed_time(ev[1]) / steps)
    n_bn = sum(1 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    rec = {'tool': 'sync_bn_bench', 'batch': batch, 'size': size, 'world': 1, 'backend': torch.distributed.get_backend(),
           'batchnorms': n_bn, 'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per training step; min over rounds (each the mean of `steps` steps); *_all: every round; one GPU: '
                   'the cost of the collectives at world >= 2 is NOT measured',
           'collectives_per_step': collectives, 'launches_per_step': launches}
    for k in contestants:
        rec['ms_device_' + k] = round(min(device[k]), 3)
        rec['ms_wall_' + k] = round(min(wall[k]), 3)
        rec['ms_device_%s_all' % k] = [round(v, 3) for v in device[k]]
    rec['forced_over_unmarked_device'] = round(rec['ms_device_forced'] / rec['ms_device_unmarked'], 3)
    rec['forced_over_unmarked_wall'] = round(rec['ms_wall_forced'] / rec['ms_wall_unmarked'], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sync_bn_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('sync_bn_bench.py measures on a GPU: none found')
    from centertrack_amd import parallel
    one_rank_group()
    rank, world, local = parallel.init_from_env(backend='nccl')
    dev = torch.device('cuda', local % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for batch in (int(b) for b in args.batches.split(',')):
        rec = measure(batch, args.size, args.steps, args.warmup, args.rounds, dev)
        print(json.dumps(rec), flush=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
    parallel.shutdown()


if __name__ == '__main__':
    main()
