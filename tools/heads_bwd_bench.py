#!/usr/bin/env python
"""Forward and backward of the trainable heads (centertrack_amd.heads.FusedHeads) against the same heads as torch modules
(``nn.Sequential(Conv2d 3x3, ReLU, Conv2d 1x1)`` per head on an NCHW feature map, MIOpen behind them), on one GPU, with
the feature map frozen -- the fine-tuning case -- unless ``--feat-grad``.

Per configuration one JSON line in profiles/heads_bwd_bench.jsonl: milliseconds of the forward and of the backward of both
(device events around each part, the two implementations alternating in one process), ``torch.cuda.max_memory_allocated``
over one forward + backward above what inputs and parameters hold, and kernel launches per forward + backward, counted
from a ``rocprofv3 --kernel-trace`` run of its own (a fresh child process per configuration; tracing and timing never
share a run).  The method is tools/loss_bench.py's.

    python tools/heads_bwd_bench.py                  # everything
    python tools/heads_bwd_bench.py --no-trace       # timing and memory only
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
from collections import OrderedDict

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

MOT = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2), ('ltrb_amodal', 4)])
NUSC = OrderedDict([('hm', 10), ('reg', 2), ('wh', 2), ('tracking', 2), ('dep', 1), ('rot', 8), ('dim', 3),
                    ('amodel_offset', 2), ('nuscenes_att', 8), ('velocity', 3)])
COCO = OrderedDict([('hm', 80), ('reg', 2), ('wh', 2)])
#           name           B   H    W    heads
CONFIGS = {'mot_b1': (1, 128, 128, MOT),
           'mot_b4': (4, 128, 128, MOT),
           'nuscenes_b4': (4, 112, 200, NUSC),
           'coco80_b4': (4, 128, 128, COCO)}


def steppers(name, device, feat_grad=False):
    """{'hip': (forward, backward), 'torch': (forward, backward)}: ``forward()`` -> outputs, ``backward(outputs)``"""
    import torch
    from torch import nn
    from centertrack_amd import heads as HD
    B, H, W, heads = CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    feat = torch.randn((B, 64, H, W), generator=g).clamp_(min=0).to(device).requires_grad_(feat_grad)
    gouts = OrderedDict((h, torch.randn((B, c, H, W), generator=g).to(device)) for h, c in heads.items())
    hip = HD.FusedHeads(heads).to(device)
    ref = nn.ModuleDict(OrderedDict((h, nn.Sequential(nn.Conv2d(64, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, c, 1)))
                                    for h, c in heads.items())).to(device)
    ref.load_state_dict(hip.state_dict())

    def make(forward, params):
        leaves = list(params) + ([feat] if feat_grad else [])

        def backward(out):
            return torch.autograd.grad([out[h] for h in heads], leaves, [gouts[h] for h in heads])
        return forward, backward

    return {'hip': make(lambda: hip(feat), hip.parameters()),
            'torch': make(lambda: OrderedDict((h, ref[h](feat)) for h in heads), ref.parameters())}


def time_parts(fwd, bwd, steps):
    """(forward ms, backward ms) per step, each between its own pair of device events"""
    import torch
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    for a, b, c in ev:
        a.record()
        out = fwd()
        b.record()
        bwd(out)
        c.record()
    torch.cuda.synchronize()
    return (sum(a.elapsed_time(b) for a, b, c in ev) / steps, sum(b.elapsed_time(c) for a, b, c in ev) / steps)


def measure(name, steps, warmup, rounds, feat_grad):
    import torch
    device = torch.device('cuda:0')
    fns = steppers(name, device, feat_grad)
    B, H, W, heads = CONFIGS[name]
    rec = {'config': name, 'B_H_W': [B, H, W], 'heads': dict(heads), 'feat_grad': feat_grad, 'steps': steps, 'rounds': rounds}
    for k, (f, b) in fns.items():
        for _ in range(warmup):
            b(f())
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):                       # the two alternate, so that a drift of the machine hits both
        for k, (f, b) in fns.items():
            ms[k].append(time_parts(f, b, steps))
    for k, (f, b) in fns.items():
        best = min(ms[k], key=lambda v: v[0] + v[1])
        rec['fwd_ms_' + k], rec['bwd_ms_' + k] = round(best[0], 4), round(best[1], 4)
        rec['ms_%s_all' % k] = [[round(v, 4) for v in r] for r in ms[k]]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = b(f())
        torch.cuda.synchronize()
        rec['peak_mb_' + k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        del r
    rec['fwd_torch_over_hip'] = round(rec['fwd_ms_torch'] / rec['fwd_ms_hip'], 2)
    rec['bwd_torch_over_hip'] = round(rec['bwd_ms_torch'] / rec['bwd_ms_hip'], 2)
    return rec


def traced_child(name, steps, feat_grad):
    """run under rocprofv3: a marker kernel, ``steps`` HIP forward + backward, a marker, ``steps`` torch ones, a marker"""
    import torch
    from centertrack_amd import ops
    fns = steppers(name, torch.device('cuda:0'), feat_grad)
    tiny = ops.new_view(1, 2, 2, 16, torch.device('cuda:0'))

    def marker():                                  # (a kernel neither implementation launches)
        torch.cuda.synchronize()
        ops.maxpool2x2(tiny)
        torch.cuda.synchronize()
    marker()
    for k in ('hip', 'torch'):
        f, b = fns[k]
        for _ in range(steps):
            b(f())
        marker()


class ChildFailed(Exception):
    """the traced child ended badly (non-zero exit, a signal, the time limit): nothing more is started on the GPU"""


def count_launches(name, steps, timeout, feat_grad):
    """kernel launches per forward + backward of both, from a kernel trace: the two phases lie between three marker kernels.
    Returns (counts, None) or (None, why); raises ChildFailed when the child did not end well."""
    if shutil.which('rocprofv3') is None:
        return None, 'rocprofv3 not found'
    tmp = tempfile.mkdtemp(prefix='heads_trace_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'heads', '--',
               sys.executable, os.path.abspath(__file__), '--traced-child', name, '--steps', str(steps)] + (
                   ['--feat-grad'] if feat_grad else [])
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
        marks = [i for i, n in enumerate(names) if 'maxpool2x2_kernel' in n]
        if len(marks) != 3:
            return None, 'expected 3 marker kernels in the trace, found %d' % len(marks)
        hip, ref = names[marks[0] + 1:marks[1]], names[marks[1] + 1:marks[2]]
        ours = sum(1 for n in hip if 'heads_tail_' in n or 'conv_bwd_weight_kernel' in n or 'slab_reduce_kernel' in n)
        return {'launches_hip': len(hip) / steps, 'launches_hip_new_kernels': ours / steps, 'launches_torch': len(ref) / steps}, None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write(path, recs):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace-steps', type=int, default=3)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--feat-grad', action='store_true', help='the feature map requires a gradient too (a trainable neck)')
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'heads_bwd_bench.jsonl'))
    ap.add_argument('--traced-child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        traced_child(args.traced_child, args.steps, args.feat_grad)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit('heads_bwd_bench.py measures on a GPU: none found')
    recs = []
    for name in args.configs.split(','):
        rec = measure(name, args.steps, args.warmup, args.rounds, args.feat_grad)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    write(args.out, recs)                         # the timings are on disk before any traced child starts
    failed = None
    if not args.no_trace:
        for rec in recs:
            try:
                got, why = count_launches(rec['config'], args.trace_steps, args.timeout, args.feat_grad)
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
            print(json.dumps({k: v for k, v in rec.items() if k.startswith('launches') or k == 'config'}), flush=True)
        write(args.out, recs)
    if failed:
        sys.exit('heads_bwd_bench.py: %s; nothing more was started' % failed)


if __name__ == '__main__':
    main()
