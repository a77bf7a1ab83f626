#!/usr/bin/env python
"""Forward + backward of the fused training loss (centertrack_amd.losses.GenericLoss) against the same loss composed
from torch ops (tests/_loss_ref.py in float32), on one GPU, at the reference's training shapes.

Per shape one JSON line in profiles/loss_bench.jsonl: milliseconds per step of both (device events, the two alternating
in one process), ``torch.cuda.max_memory_allocated`` over one step above what the inputs hold, and kernel launches per
step, counted from a ``rocprofv3 --kernel-trace`` run of its own (a fresh child process per shape; tracing and timing
never share a run).

    python tools/loss_bench.py                  # everything
    python tools/loss_bench.py --no-trace       # timing and memory only
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MOT = ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal')
COCO = ('hm', 'reg', 'wh', 'tracking')
NUSC = ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity')
POSE = ('hm', 'reg', 'wh', 'hm_hp', 'hps', 'hp_offset')
#         name               B   C   H    W    M   heads
SHAPES = {'coco': (16, 80, 128, 128, 128, COCO),
          'coco_pose': (16, 1, 128, 128, 32, POSE),
          'nuscenes': (8, 10, 112, 200, 128, NUSC),
          'mot': (4, 1, 136, 240, 256, MOT),
          'nuscenes_heads_at_mot': (4, 10, 136, 240, 256, NUSC)}


def make(name, device):
    import torch
    import _loss_ref as R
    B, C, H, W, M, heads = SHAPES[name]
    out, batch = R.make_batch(7, B, H, W, M, heads, C, valid=[min(M, 20 + 3 * b) for b in range(B)], scale=2.0)
    out = {h: v.to(device) for h, v in out.items()}
    batch = {k: v.to(device) for k, v in batch.items()}
    return out, batch, heads, R.Opt(heads)


def steppers(name, device):
    """{'fused': step, 'torch': step}; a step is forward + backward and returns (tot, gradients)"""
    import torch
    import _loss_ref as R
    from centertrack_amd import losses
    out, batch, heads, opt = make(name, device)
    leaves = {h: out[h].requires_grad_() for h in heads}
    crit = losses.GenericLoss(opt)

    def fused():
        tot, _ = crit([dict(leaves)], batch)
        return tot, torch.autograd.grad(tot, [leaves[h] for h in heads])

    def composed():
        tot, _ = R.generic_loss([leaves], batch, heads, opt.weights)
        return tot, torch.autograd.grad(tot, [leaves[h] for h in heads])

    return {'fused': fused, 'torch': composed}, heads


def time_ms(step, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def measure(name, steps, warmup, rounds):
    import torch
    device = torch.device('cuda:0')
    fns, heads = steppers(name, device)
    rec = {'shape': name, 'B_C_H_W_M': list(SHAPES[name][:5]), 'heads': list(heads), 'steps': steps, 'rounds': rounds}
    for k, f in fns.items():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    tf, tt = fns['fused']()[0], fns['torch']()[0]
    rec['tot_fused'], rec['tot_torch'] = float(tf), float(tt)
    ms = {'fused': [], 'torch': []}
    for _ in range(rounds):                       # the two alternate, so that a drift of the machine hits both
        for k in ('fused', 'torch'):
            ms[k].append(time_ms(fns[k], steps))
    for k in ms:
        rec['ms_' + k] = round(min(ms[k]), 4)
        rec['ms_%s_all' % k] = [round(v, 4) for v in ms[k]]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = fns[k]()
        torch.cuda.synchronize()
        rec['peak_mb_' + k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        del r
    rec['speedup'] = round(rec['ms_torch'] / rec['ms_fused'], 2)
    return rec


def traced_child(name, steps):
    """run under rocprofv3: ``steps`` fused steps, then ``steps`` composed steps, nothing else on the device"""
    import torch
    fns, _ = steppers(name, torch.device('cuda:0'))
    for k in ('fused', 'torch'):
        for _ in range(steps):
            fns[k]()
        torch.cuda.synchronize()


class ChildFailed(Exception):
    """the traced child ended badly (non-zero exit, a signal, the time limit): nothing more is started on the GPU"""


def count_launches(name, steps, timeout):
    """kernel launches per step of both, from a kernel trace: the fused phase ends with its last slot-scatter kernel.
    Returns (counts, None) or (None, why) when there is no profiler or no trace; raises ChildFailed when the child did
    not end well."""
    if shutil.which('rocprofv3') is None:
        return None, 'rocprofv3 not found'
    tmp = tempfile.mkdtemp(prefix='loss_trace_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'loss', '--',
               sys.executable, os.path.abspath(__file__), '--traced-child', name, '--steps', str(steps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            raise ChildFailed('traced child of %s ran into its time limit of %d s' % (name, timeout))
        if r.returncode != 0:
            raise ChildFailed('traced child of %s: exit %d: %s' % (name, r.returncode, (r.stderr or r.stdout)[-300:]))
        files = glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True)
        if not files:
            return None, 'no kernel trace written'
        rows = []
        for fn in files:
            with open(fn) as f:
                rows += list(csv.DictReader(f))
        if not rows or 'Kernel_Name' not in rows[0] or 'Start_Timestamp' not in rows[0]:
            return None, 'kernel trace without Kernel_Name / Start_Timestamp columns: %s' % sorted(rows[0] if rows else [])
        rows.sort(key=lambda x: int(x['Start_Timestamp']))
        names = [x['Kernel_Name'] for x in rows]
        ours = [i for i, n in enumerate(names) if 'loss_slot_scatter_kernel' in n]
        if len(ours) != steps:
            return None, 'expected %d scatter kernels in the trace, found %d' % (steps, len(ours))
        nf, nt = ours[-1] + 1, len(names) - ours[-1] - 1
        hip = sum(1 for n in names[:nf] if 'loss_' in n and '_kernel' in n)
        return {'launches_fused': nf / steps, 'launches_fused_hip': hip / steps, 'launches_torch': nt / steps}, None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write(path, recs):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace-steps', type=int, default=4)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_bench.jsonl'))
    ap.add_argument('--traced-child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        traced_child(args.traced_child, args.steps)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit('loss_bench.py measures on a GPU: none found')
    recs = []
    for name in args.shapes.split(','):
        rec = measure(name, args.steps, args.warmup, args.rounds)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    write(args.out, recs)                         # the timings are on disk before any traced child starts
    failed = None
    if not args.no_trace:
        for rec in recs:
            try:
                got, why = count_launches(rec['shape'], args.trace_steps, args.timeout)
            except ChildFailed as e:
                # a child that ended badly may have faulted the card: nothing more is started on it
                failed = str(e)
                for r in recs:
                    r.setdefault('launches', 'not measured: ' + (failed if r is rec else 'not started after a failed child'))
                break
            if got is None:
                rec['launches'] = 'not measured: ' + why
            else:
                rec.update(got)
            print(json.dumps({k: v for k, v in rec.items() if k.startswith('launches') or k == 'shape'}), flush=True)
        write(args.out, recs)
    if failed:
        sys.exit('loss_bench.py: %s; nothing more was started' % failed)


if __name__ == '__main__':
    main()
