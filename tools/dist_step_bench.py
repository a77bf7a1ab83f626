"""The data-parallel optimizer step beside the plain one, per step, and its parts alone.

On the parameter list of ``DLASeg(34, MOT heads)`` -- 243 tensors -- with random gradients, alternating in one process
(the method of tools/optim_bench.py):

  plain          ``centertrack_amd.optim.Adam`` / ``SGD``: one copy and one ``ct_optim_step`` launch
  distributed    the same after ``.distribute()``: one copy, the ``ct_optim_pack_grads`` launch, one all-reduce of the flat
                 buffer, one ``ct_optim_step`` launch
  pack           ``ct_optim_pack_grads`` alone, on a table packed once
  all_reduce     ``parallel.all_reduce_flat`` of the flat buffer alone
  torch_gather   the same gather done with torch: ``_flatten_dense_tensors(grads)`` followed by a multiply

Per contestant: ``ms_device`` -- device events around ``steps`` calls, per call, the minimum over the rounds; ``ms_wall`` --
the host clock around the same calls ending in a device synchronise; ``launches`` -- kernels, copies and the kernels' summed
duration of one call from the torch profiler (null when the profiler is not available).

Run it as it is (a process group of one rank is created, so the all-reduce is a real collective on RCCL) or under torchrun
at any world size (``--backend gloo`` takes the path through the host); rank 0 appends one line per optimizer to
profiles/dist_step_bench.jsonl.

    python tools/dist_step_bench.py [--steps 50] [--warmup 5] [--rounds 3] [--optimizers adam,sgd] [--backend nccl]
    python -m torch.distributed.run --nproc-per-node 8 tools/dist_step_bench.py
"""
import argparse
import json
import os
import socket
import sys
import time
import types
from collections import OrderedDict

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import count_launches, parameter_shapes  # noqa: E402


def one_rank_group():
    """without a launcher: the rendezvous variables of a group of one rank"""
    if 'RANK' in os.environ:
        return
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))


def measure(kind, shapes, steps, warmup, rounds, dev, world):
    import torch
    from torch._utils import _flatten_dense_tensors
    from centertrack_amd import ops, optim as O, parallel
    import numpy as np
    g = torch.Generator(device=dev).manual_seed(11)
    init = [torch.randn(s, device=dev, generator=g) for s in shapes]
    grads = [torch.randn(s, device=dev, generator=g) * 0.1 for s in shapes]
    numel = sum(t.numel() for t in init)
    kw = dict(lr=1.25e-4) if kind == 'adam' else dict(lr=1.25e-4, momentum=0.9, weight_decay=1e-4)
    cls = O.Adam if kind == 'adam' else O.SGD
    made = OrderedDict()
    for name in ('plain', 'distributed'):
        ps = [t.clone().requires_grad_() for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt = cls(ps, **kw)
        made[name] = opt.distribute() if name == 'distributed' else opt
    # the parts alone: a table packed once over a flat buffer of their own
    offsets, total = O.flat_layout([t.numel() for t in grads])
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    items = [(flat.data_ptr() + 4 * off, flat.data_ptr() + 4 * off, 0, 0, t.numel(), (0.0, 0.0, 0.0), 0)
             for t, off in zip(grads, offsets)]
    words, n, chunks = O.pack(O.KINDS['sgd'], items, src=[t.data_ptr() for t in grads])
    table = torch.from_numpy(words).to(dev)
    scale = float(np.float32(1.0 / world))
    made['pack'] = types.SimpleNamespace(step=lambda: ops.optim_pack_grads(table, n, chunks, scale))
    made['all_reduce'] = types.SimpleNamespace(step=lambda: parallel.all_reduce_flat(flat))
    made['torch_gather'] = types.SimpleNamespace(step=lambda: _flatten_dense_tensors(grads).mul_(scale))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    wall = {k: [] for k in made}
    device = {k: [] for k in made}
    for opt in made.values():
        for _ in range(warmup):
            opt.step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, opt in made.items():
            flat.zero_()                                     # (a sum of sums of .. would overflow at a large world)
            parallel.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for _ in range(steps):
                opt.step()
            ev[1].record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            device[name].append(ev[0].elapsed_time(ev[1]) / steps)
    rec = {'tool': 'dist_step_bench', 'optimizer': kind, 'world': world, 'backend': torch.distributed.get_backend(),
           'tensors': len(shapes), 'elements': numel, 'chunks': chunks, 'flat_bytes': total * 4,
           'bytes_pack': numel * 4 + total * 4, 'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per call; min over rounds (each the mean of `steps` calls); *_all: every round',
           'launches_per_call': {k: count_launches(opt) for k, opt in made.items()}}
    for k in made:
        rec['ms_device_' + k] = round(min(device[k]), 4)
        rec['ms_wall_' + k] = round(min(wall[k]), 4)
        rec['ms_device_%s_all' % k] = [round(v, 4) for v in device[k]]
    rec['gbps_pack'] = round(rec['bytes_pack'] / (rec['ms_device_pack'] * 1e-3) / 1e9, 1)
    rec['distributed_over_plain_device'] = round(rec['ms_device_distributed'] / rec['ms_device_plain'], 3)
    rec['pack_over_torch_gather_device'] = round(rec['ms_device_pack'] / rec['ms_device_torch_gather'], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--optimizers', default='adam,sgd')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dist_step_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('dist_step_bench.py measures on a GPU: none found')
    from centertrack_amd import parallel
    one_rank_group()
    rank, world, local = parallel.init_from_env(backend=args.backend)
    dev = torch.device('cuda', local % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    shapes = parameter_shapes()
    recs = []
    for kind in args.optimizers.split(','):
        rec = measure(kind, shapes, args.steps, args.warmup, args.rounds, dev, world)
        recs.append(rec)
        if rank == 0:
            print(json.dumps(rec), flush=True)
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for rec in recs:
                f.write(json.dumps(rec) + '\n')
    parallel.shutdown()


if __name__ == '__main__':
    main()
