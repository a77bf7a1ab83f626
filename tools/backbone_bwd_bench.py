#!/usr/bin/env python
"""Forward and forward + backward of the trainable DLA-34 backbone (centertrack_amd.dla_base.DLA, stems included) against
the same network built from torch modules: the same ``nn.Conv2d`` / ``nn.BatchNorm2d`` objects called by torch, NCHW, vendor
convolutions, ``F.relu`` / ``F.max_pool2d`` / ``torch.cat`` as the reference composes them (dla.py:38-66,154-316).  One GPU,
training mode, 512 x 512 input with ``pre_img`` and ``pre_hm``, batch 1 and 4; every parameter something reads asks for a
gradient, the images do not.

Per configuration one JSON line in profiles/backbone_bwd_bench.jsonl: milliseconds of the forward and of the backward of both
(device events around each part, the two implementations alternating in one process, the best round of each and every
round), ``torch.cuda.max_memory_allocated`` over one forward + backward above what inputs and parameters hold, the largest
difference of the six outputs and of the parameter gradients between the two (relative to the tensor's maximum), and kernel
launches per forward + backward counted from a ``rocprofv3 --kernel-trace`` run of its own (a fresh child process per
configuration; tracing and timing never share a process).  The first line carries ``box_calibration`` (tools/box_calib.py):
the state of the machine the figures were taken on.  The method is tools/heads_bwd_bench.py's.

    python tools/backbone_bwd_bench.py
    python tools/backbone_bwd_bench.py --configs b1 --steps 10 --no-trace
"""
import argparse
import copy
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

#           name  B  H    W
CONFIGS = {'b1': (1, 512, 512), 'b4': (4, 512, 512)}


class Opt(object):
    pre_img, pre_hm = True, True


def torch_forward(m, x, pre_img, pre_hm):
    """the baseline: the modules of ``m`` (a dla_base.DLA) called by torch, as the reference's forward composes them"""
    import torch
    import torch.nn.functional as F
    from centertrack_amd import dla_base

    def unit(x, conv, bn, res=None, relu=True):
        y = bn(conv(x))
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def block(b, x, residual=None):
        return unit(unit(x, b.conv1, b.bn1), b.conv2, b.bn2, res=x if residual is None else residual)

    def root(r, *xs):
        return unit(torch.cat(xs, 1), r.conv, r.bn, res=xs[0] if r.residual else None)

    def tree(t, x, children=None):
        children = [] if children is None else children
        bottom = F.max_pool2d(x, 2, 2) if t.downsample else x
        residual = unit(bottom, t.project[0], t.project[1], relu=False) if t.project else bottom
        if t.level_root:
            children.append(bottom)
        if t.levels == 1:
            x1 = block(t.tree1, x, residual)
            return root(t.root, block(t.tree2, x1), x1, *children)
        x1 = tree(t.tree1, x)
        children.append(x1)
        return tree(t.tree2, x1, children=children)
    y = m.base_layer(x) + m.pre_img_layer(pre_img) + m.pre_hm_layer(pre_hm)
    out = []
    for i in range(6):
        level = getattr(m, 'level%d' % i)
        if isinstance(level, dla_base.Tree):
            y = tree(level, y)
        else:
            y = level(y)
        out.append(y)
    return out


def steppers(name, device):
    """{'hip': (forward, backward, module), 'torch': ...}: ``forward()`` -> the six outputs, ``backward(outputs)``"""
    import torch
    from centertrack_amd import dcn_v2, dla_base
    B, H, W = CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    x, pre = (torch.randn((B, 3, H, W), generator=g).to(device) for _ in range(2))
    hm = torch.rand((B, 1, H, W), generator=g).to(device)
    torch.manual_seed(5)
    hip = dla_base.dla34(pretrained=False, opt=Opt()).to(device).train()
    ref = copy.deepcopy(hip)
    chans = [16, 32, 64, 128, 256, 512]
    gouts = [torch.randn((B, c, H >> i, W >> i), generator=g).to(device) / (B * (H >> i) * (W >> i)) ** 0.5 for i, c in enumerate(chans)]
    unread = ('level3.project.', 'level4.project.')

    def make(mod, fwd):
        leaves = [p for k, p in mod.named_parameters() if not k.startswith(unread)]

        def forward():
            with dcn_v2.trainable():
                return fwd(mod)

        def backward(outs):
            return torch.autograd.grad(outs, leaves, gouts)
        return forward, backward, mod
    return {'hip': make(hip, lambda m: m(x, pre, hm)), 'torch': make(ref, lambda m: torch_forward(m, x, pre, hm))}


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


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def measure(name, steps, warmup, rounds):
    import torch
    device = torch.device('cuda:0')
    fns = steppers(name, device)
    B, H, W = CONFIGS[name]
    rec = {'config': name, 'B': B, 'H': H, 'W': W, 'steps': steps, 'rounds': rounds}
    res = {}
    for k, (f, b, _) in fns.items():
        for i in range(warmup):
            outs = f()
            res[k] = ([o.detach() for o in outs], b(outs))
    torch.cuda.synchronize()
    # the two compute the same network: sums in another order differ in the last bits, anything larger wants an explanation
    rec['outputs_max_rel_diff'] = max(rel(a, b) for a, b in zip(res['hip'][0], res['torch'][0]))
    rec['grads_max_rel_diff'] = max(rel(a, b) for a, b in zip(res['hip'][1], res['torch'][1]))
    del res
    ms = {k: [] for k in fns}
    for _ in range(rounds):                       # the two alternate, so that a drift of the machine hits both
        for k, (f, b, _) in fns.items():
            ms[k].append(time_parts(f, b, steps))
    for k, (f, b, _) in fns.items():
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
    rec['step_torch_over_hip'] = round((rec['fwd_ms_torch'] + rec['bwd_ms_torch']) / (rec['fwd_ms_hip'] + rec['bwd_ms_hip']), 2)
    return rec


def traced_child(name, steps):
    """run under rocprofv3: a marker kernel, ``steps`` HIP forward + backward, a marker, ``steps`` torch ones, a marker"""
    import torch
    from centertrack_amd import ops
    fns = steppers(name, torch.device('cuda:0'))
    tiny = ops.new_view(1, 2, 2, 16, torch.device('cuda:0'))
    g = ops.new_view(1, 1, 1, 16, torch.device('cuda:0'))

    def marker():                                  # (a kernel neither implementation launches)
        torch.cuda.synchronize()
        ops.upsample_add(g, torch.zeros(16, 16, device='cuda:0'), 2, tiny)
        torch.cuda.synchronize()
    marker()
    for k in ('hip', 'torch'):
        f, b, _ = fns[k]
        for _ in range(steps):
            b(f())
        marker()


class ChildFailed(Exception):
    """the traced child ended badly (non-zero exit, a signal, the time limit): nothing more is started on the GPU"""


NEW_KERNELS = ('conv_s2_gx_kernel', 'conv_bwd_weight_kernel<2>', 'pack_s2t_kernel', 'bn_act_', 'maxpool_bwd_kernel')


def count_launches(name, steps, timeout):
    """kernel launches per forward + backward of both, from a kernel trace: the two phases lie between three marker kernels.
    Returns (counts, None) or (None, why); raises ChildFailed when the child did not end well."""
    if shutil.which('rocprofv3') is None:
        return None, 'rocprofv3 not found'
    tmp = tempfile.mkdtemp(prefix='backbone_trace_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'backbone', '--',
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
        marks = [i for i, n in enumerate(names) if 'upsample_add_kernel' in n]
        if len(marks) != 3:
            return None, 'expected 3 marker kernels in the trace, found %d' % len(marks)
        hip, ref = names[marks[0] + 1:marks[1]], names[marks[1] + 1:marks[2]]
        ours = sum(1 for n in hip if any(s in n for s in NEW_KERNELS))
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
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace-steps', type=int, default=2)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--no-box-probes', action='store_true', help='box_calibration without the latency / clock probes')
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backbone_bwd_bench.jsonl'))
    ap.add_argument('--traced-child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        traced_child(args.traced_child, args.steps)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit('backbone_bwd_bench.py measures on a GPU: none found')
    recs = []
    for name in args.configs.split(','):
        rec = measure(name, args.steps, args.warmup, args.rounds)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    try:
        from tools import box_calib
        recs[0]['box_calibration'] = box_calib.box_calibration(torch.device('cuda:0'), probes=not args.no_box_probes)
    except Exception as e:                          # a probe must never cost the bench lines
        recs[0]['box_calibration'] = {'error': repr(e)}
    torch.cuda.synchronize()
    write(args.out, recs)                         # the timings are on disk before any traced child starts
    failed = None
    if not args.no_trace:
        for rec in recs:
            try:
                got, why = count_launches(rec['config'], args.trace_steps, args.timeout)
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
        sys.exit('backbone_bwd_bench.py: %s; nothing more was started' % failed)


if __name__ == '__main__':
    main()
