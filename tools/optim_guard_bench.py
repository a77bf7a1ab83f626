"""The guarded optimizer step against the unguarded one and against torch's clipping, per step.

On the parameter list of ``DLASeg(34, MOT heads)`` with random gradients, alternating in one process (the method of
tools/optim_bench.py):

  unguarded          ``centertrack_amd.optim.Adam`` / ``SGD``: one copy and one ``ct_optim_step`` launch
  guarded            the same after ``.guard(max_norm, skip_nonfinite=True)``: one copy, the two launches of
                     ``ct_optim_norms`` and one ``ct_optim_step_guarded`` launch
  torch_clip_fused   ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` then ``torch.optim.Adam(fused=True).step()``
  torch_clip         the same with torch's default forms of both

``max_norm`` is a tenth of the gradients' norm, so every contestant clips on every step.  torch's clipping scales ``.grad``
in place, so its gradients shrink from step to step (the second step no longer clips); the work per step does not depend
on that.  Per contestant: ``ms_wall`` -- host clock around ``steps`` steps ending in a device synchronise, per step;
``ms_device`` -- device events around the same calls; ``launches`` -- kernels, copies and the kernels' summed duration of
one step from the torch profiler (null when the profiler is not available).  ``ms_kernel_*``: ``ct_optim_step``,
``ct_optim_norms`` and ``ct_optim_step_guarded`` alone, each launched back to back on a table packed once, and
``guarded_over_unguarded_kernel`` = (norms + guarded step) / step.

Appends one line per optimizer to profiles/optim_guard_bench.jsonl.

    python tools/optim_guard_bench.py [--steps 50] [--warmup 5] [--rounds 3] [--optimizers adam,sgd]
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

from tools.optim_bench import count_launches, parameter_shapes  # noqa: E402


class Clipped(object):
    """clip_grad_norm_ + step, as a training loop calls them"""

    def __init__(self, opt, params, max_norm, foreach):
        self.opt, self.params, self.max_norm, self.foreach = opt, params, max_norm, foreach

    def step(self):
        import torch
        torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, foreach=self.foreach)
        self.opt.step()


def contestants(kind, max_norm):
    import torch
    from centertrack_amd import optim as O
    if kind == 'adam':
        mine, theirs, kw = O.Adam, torch.optim.Adam, dict(lr=1.25e-4)
    else:
        mine, theirs, kw = O.SGD, torch.optim.SGD, dict(lr=1.25e-4, momentum=0.9, weight_decay=1e-4)
    return OrderedDict([
        ('unguarded', lambda ps: mine(ps, **kw)),
        ('guarded', lambda ps: mine(ps, **kw).guard(max_norm, skip_nonfinite=True)),
        ('torch_clip_fused', lambda ps: Clipped(theirs(ps, fused=True, **kw), ps, max_norm, None)),
        ('torch_clip', lambda ps: Clipped(theirs(ps, **kw), ps, max_norm, None))])


def kernels_only(kind, opt, ps, steps, max_norm):
    """ms per call of ct_optim_step, ct_optim_norms and ct_optim_step_guarded alone over the optimizer's tensors: a table
    packed once, device events around ``steps`` calls (the host enqueues faster than the kernels run)"""
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
    dev = ps[0].device
    table = torch.from_numpy(words).to(dev)
    state = torch.zeros(O.GUARD_SLOT + 8 * n, dtype=torch.uint8, device=dev)
    work = torch.empty(O.norms_workspace_bytes(n, chunks), dtype=torch.uint8, device=dev)
    calls = OrderedDict([
        ('step', lambda: ops.optim_step(table, n, chunks, O.KINDS[kind])),
        ('norms', lambda: ops.optim_norms(table, n, chunks, max_norm, True, state[O.GUARD_SLOT:], state, work)),
        ('step_guarded', lambda: ops.optim_step_guarded(table, n, chunks, O.KINDS[kind], state)),
        ('norms_and_step_guarded', lambda: (ops.optim_norms(table, n, chunks, max_norm, True, state[O.GUARD_SLOT:], state, work),
                                            ops.optim_step_guarded(table, n, chunks, O.KINDS[kind], state)))])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in calls}
    for r in range(4):                                       # alternating; the first round warms up
        for name, call in calls.items():
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(steps):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                out[name].append(ev[0].elapsed_time(ev[1]) / steps)
    return out, chunks


def measure(kind, shapes, steps, warmup, rounds):
    import torch
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(11)
    init = [torch.randn(s, device=dev, generator=g) for s in shapes]
    grads = [torch.randn(s, device=dev, generator=g) * 0.1 for s in shapes]
    numel = sum(t.numel() for t in init)
    norm = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads)))
    max_norm = norm / 10
    made = OrderedDict()
    for name, make in contestants(kind, max_norm).items():
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
    launches = {k: count_launches(opt) for k, (opt, _) in made.items()}
    stats = made['guarded'][0].grad_stats()
    kernel_ms, chunks = kernels_only(kind, made['unguarded'][0], made['unguarded'][1], steps, max_norm)
    nbytes = numel * 4 * (7 if kind == 'adam' else 5)
    rec = {'tool': 'optim_guard_bench', 'optimizer': kind, 'tensors': len(shapes), 'elements': numel, 'chunks': chunks,
           'bytes_per_step': nbytes, 'bytes_norms': numel * 4, 'max_norm': max_norm, 'gradient_norm': norm,
           'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per step; min over rounds (each the mean of `steps` steps); *_all: every round',
           'guard_stats': {k: stats[k] for k in ('norm', 'coef', 'steps', 'clipped', 'skipped', 'nonfinite')},
           'launches_per_step': launches}
    for k, v in kernel_ms.items():
        rec['ms_kernel_' + k] = round(min(v), 4)
        rec['ms_kernel_%s_all' % k] = [round(x, 4) for x in v]
    rec['guarded_over_unguarded_kernel'] = round(rec['ms_kernel_norms_and_step_guarded'] / rec['ms_kernel_step'], 3)
    rec['gbps_kernel_norms'] = round(numel * 4 / (rec['ms_kernel_norms'] * 1e-3) / 1e9, 1)
    for k in made:
        rec['ms_wall_' + k] = round(min(wall[k]), 4)
        rec['ms_device_' + k] = round(min(device[k]), 4)
        rec['ms_wall_%s_all' % k] = [round(v, 4) for v in wall[k]]
        rec['ms_device_%s_all' % k] = [round(v, 4) for v in device[k]]
    rec['guarded_over_unguarded_wall'] = round(rec['ms_wall_guarded'] / rec['ms_wall_unguarded'], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--optimizers', default='adam,sgd')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_guard_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('optim_guard_bench.py measures on a GPU: none found')
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
