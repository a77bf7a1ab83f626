"""The optimizer step: centertrack_amd.optim against torch.optim, per step.

On the parameter list of ``DLASeg(34, MOT heads)`` with random gradients, alternating in one process:

  ours           ``centertrack_amd.optim.Adam`` / ``SGD``: one pinned-to-device copy and one ``ct_optim_step`` launch
  torch          ``torch.optim.Adam`` / ``SGD`` as constructed by default (the ``_foreach`` implementation on a GPU)
  torch_fused    the same with ``fused=True``

Adam is ``Adam(params, 1.25e-4)``, SGD is ``SGD(params, 1.25e-4, momentum=0.9, weight_decay=1e-4)``: the reference's two
calls (src/main.py:17-26).  Per contestant: ``ms_wall`` -- host clock around ``steps`` calls of ``step()`` ending in a
device synchronise, per step, which is what a training loop waits for when nothing else is enqueued; ``ms_device`` --
device events around the same calls (where the host is the slower side this is the host's time too); ``launches`` --
kernels, copies and the kernels' summed duration of one step as the torch profiler lists them (null when the profiler is
not available); ``ms_kernel_ours`` -- ``ct_optim_step`` alone, launched back to back on a table packed once.  ``gbps`` is the bytes the arithmetic needs (Adam: read p, g, m, v and write p, m,
v; SGD: read p, g, buf and write p, buf) over ``ms_device``.  Every contestant has its own copy of the parameters; after
the timed steps the copies are compared (largest difference relative to the largest parameter).

Appends one line per optimizer to profiles/optim_bench.jsonl.

    python tools/optim_bench.py [--steps 50] [--warmup 5] [--rounds 3] [--out profiles/optim_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADS = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2)])


class Opt(object):
    pre_img, pre_hm = True, True
    dla_node, head_kernel, prior_bias = 'dcn', 3, -4.6
    model_output_list = False
    load_model = ''


def parameter_shapes():
    from centertrack_amd.dla_seg import DLASeg
    return [tuple(p.shape) for p in DLASeg(34, HEADS, {h: [256] for h in HEADS}, Opt()).parameters()]


def contestants(kind):
    import torch
    from centertrack_amd import optim as O
    if kind == 'adam':
        mine, theirs, kw = O.Adam, torch.optim.Adam, dict(lr=1.25e-4)
    else:
        mine, theirs, kw = O.SGD, torch.optim.SGD, dict(lr=1.25e-4, momentum=0.9, weight_decay=1e-4)
    return OrderedDict([('ours', lambda ps: mine(ps, **kw)), ('torch', lambda ps: theirs(ps, **kw)),
                        ('torch_fused', lambda ps: theirs(ps, fused=True, **kw))])


def count_launches(opt):
    """kernels and copies of one step, from the torch profiler; None when it cannot be had"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(e.device_type).endswith('CUDA')]
        copies = [e for e in evs if 'memcpy' in e.name.lower()]
        busy = sum(e.time_range.elapsed_us() for e in evs if e not in copies)
        return {'kernels': len(evs) - len(copies), 'copies': len(copies), 'kernel_ms': round(busy / 1e3, 4)} if evs else None
    except Exception:
        return None


def kernel_only(kind, opt, ps, steps):
    """ms per launch of ct_optim_step alone over the optimizer's tensors: a table packed once, device events around
    ``steps`` launches (the host enqueues faster than the kernel runs)"""
    import torch
    from centertrack_amd import ops, optim as O
    items = []
    for p in ps:
        st = opt.state[p]
        if kind == 'adam':
            items.append((p.data_ptr(), p.grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel(),
                          O.adam_scalars(int(st['step']) + 1, 1.25e-4, 0.9, 0.999, 1e-8, 0), 0))
        else:
            items.append((p.data_ptr(), p.grad.data_ptr(), st['momentum_buffer'].data_ptr(), 0, p.numel(),
                          (1.25e-4, 0.9, 1e-4), 0))
    words, n, chunks = O.pack(O.KINDS[kind], items)
    table = torch.from_numpy(words).to(ps[0].device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for r in range(3):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(steps):
            ops.optim_step(table, n, chunks, O.KINDS[kind])
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) / steps)
    return min(out[1:]), chunks


def measure(kind, shapes, steps, warmup, rounds):
    import numpy as np
    import torch
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(11)
    init = [torch.randn(s, device=dev, generator=g) for s in shapes]
    grads = [torch.randn(s, device=dev, generator=g) * 0.1 for s in shapes]
    numel = sum(t.numel() for t in init)
    made = OrderedDict()
    for name, make in contestants(kind).items():
        ps = [t.clone().requires_grad_() for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        made[name] = (make(ps), ps)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    wall = {k: [] for k in made}
    device = {k: [] for k in made}
    for name, (opt, _) in made.items():
        for _ in range(warmup):
            opt.step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, (opt, _) in made.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for _ in range(steps):
                opt.step()
            ev[1].record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            device[name].append(ev[0].elapsed_time(ev[1]) / steps)
    # every contestant has taken the same number of steps on the same data
    top = max(float(t.abs().max()) for t in made['ours'][1])
    diff = {k: max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(made['ours'][1], ps)) / top
            for k, (_, ps) in made.items() if k != 'ours'}
    launches = {k: count_launches(opt) for k, (opt, _) in made.items()}
    nbytes = numel * 4 * (7 if kind == 'adam' else 5)
    kernel_ms, chunks = kernel_only(kind, made['ours'][0], made['ours'][1], steps)
    rec = {'tool': 'optim_bench', 'optimizer': kind, 'tensors': len(shapes), 'elements': numel,
           'tensors_up_to_512': sum(1 for t in init if t.numel() <= 512), 'bytes_per_step': nbytes,
           'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per step; min over rounds (each the mean of `steps` steps); *_all: every round',
           'largest_difference_from_ours_over_largest_parameter': diff, 'launches_per_step': launches,
           'chunks': chunks, 'ms_kernel_ours': round(kernel_ms, 4), 'gbps_kernel_ours': round(nbytes / (kernel_ms * 1e-3) / 1e9, 1)}
    for k in made:
        rec['ms_wall_' + k] = round(min(wall[k]), 4)
        rec['ms_device_' + k] = round(min(device[k]), 4)
        rec['ms_wall_%s_all' % k] = [round(v, 4) for v in wall[k]]
        rec['ms_device_%s_all' % k] = [round(v, 4) for v in device[k]]
        rec['gbps_' + k] = round(nbytes / (min(device[k]) * 1e-3) / 1e9, 1)
    for k in ('torch', 'torch_fused'):
        rec['wall_%s_over_ours' % k] = round(rec['ms_wall_' + k] / rec['ms_wall_ours'], 2)
    assert all(np.isfinite(v) for v in diff.values())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--optimizers', default='adam,sgd')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('optim_bench.py measures on a GPU: none found')
    shapes = parameter_shapes()
    recs = []
    for kind in args.optimizers.split(','):
        rec = measure(kind, shapes, args.steps, args.warmup, args.rounds)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
