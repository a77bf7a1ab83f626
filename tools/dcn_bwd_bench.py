#!/usr/bin/env python
"""Forward and backward times of the DeformConv shapes of the DLA-34 neck (the seven distinct shapes among its sixteen
nodes at 512x512), batch 1 and 4, in one process per batch: ct_dcn_v2 (the yardstick), the data launches of
ct_dcn_v2_backward (zero-fill of g_x + dcn_bwd_data_kernel; also without the g_x half, which prices the scatter) and its
weight launches (dcn_bwd_weight_kernel + reduce).  Timing as tools/kbench.py: HIP events around replays of a graph of
back-to-back launches.  Prints one JSON line per shape and a table.

    python tools/dcn_bwd_bench.py [--batches 1,4] [--size 512] [--reps 20] [--off-scale 1.0] [--json out.jsonl]

Every batch runs in a child process under its own time limit; a child that fails ends the run."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12        # chip-wide float-atomic rate (added bytes / s) the scatter is budgeted against


def shapes(S):
    # (name, nodes per frame, H = W, Cin, Cout)
    return [('dcn 512-256 @%d' % (S // 32), 1, S // 32, 512, 256), ('dcn 256-256 @%d' % (S // 16), 1, S // 16, 256, 256),
            ('dcn 256-128 @%d' % (S // 16), 2, S // 16, 256, 128), ('dcn 128-128 @%d' % (S // 8), 2, S // 8, 128, 128),
            ('dcn 128-64 @%d' % (S // 8), 4, S // 8, 128, 64), ('dcn 256-64 @%d' % (S // 16), 1, S // 16, 256, 64),
            ('dcn 64-64 @%d' % (S // 4), 5, S // 4, 64, 64)]


def child(args):
    import torch
    from centertrack_amd import _lib, ops
    from tools.kbench import time_call
    lib = _lib.load()
    dev = torch.device('cuda:0')
    N = args.batch
    g = torch.Generator().manual_seed(0)
    for name, cnt, H, Cin, Cout in shapes(args.size):
        def view(C, ld=None, scale=1.0):
            t = torch.randn((N, H, H, ld or C), generator=g) * scale
            return ops.View(t.to(dev), 0, C)
        x, gy = view(Cin), view(Cout)
        om = view(27, 32)
        om.buf[..., :18] *= args.off_scale
        om.buf[..., 18:] = torch.sigmoid(om.buf[..., 18:])
        w = (torch.randn((Cout, Cin, 3, 3), generator=g) * (9 * Cin) ** -0.5).to(dev)
        wp, wT = ops.pack_weight(w), ops.pack_weight_t(w)
        out = ops.new_view(N, H, H, Cout, dev)
        gx, gom = ops.new_view(N, H, H, Cin, dev), ops.View(torch.zeros((N, H, H, 32), device=dev), 0, 27)
        gw, gb = torch.empty_like(w), torch.empty(Cout, device=dev)
        fd = ops.make_dcn_desc(x, om, wp, Cout, None, None, False, out)
        need = lib.ct_dcn_v2_workspace_bytes(ctypes.byref(fd))
        fws = torch.empty(max(need, 4) // 4, device=dev)
        fd.workspace, fd.workspace_bytes = fws.data_ptr(), need
        descs = {'data': ops.make_dcn_bwd_desc(x, om, gy, wT, gx=gx, gom=gom),
                 'data_no_gx': ops.make_dcn_bwd_desc(x, om, gy, wT, gom=gom),
                 'weight': ops.make_dcn_bwd_desc(x, om, gy, gw=gw, gb=gb)}
        need = lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(descs['weight']))
        bws = torch.empty(need // 4, device=dev)
        descs['weight'].workspace, descs['weight'].workspace_bytes = bws.data_ptr(), need
        st = _lib.stream_ptr
        t = {'forward': time_call(lambda: _lib.check(lib.ct_dcn_v2(ctypes.byref(fd), st()), 'ct_dcn_v2'), args.reps)}
        for key, d in descs.items():
            t[key] = time_call(lambda d=d: _lib.check(lib.ct_dcn_v2_backward(ctypes.byref(d), st()), 'ct_dcn_v2_backward'),
                               args.reps)
        # bytes the scatter adds: four corners per (pixel, tap, channel), less what falls outside the image or has a zero weight
        # (upper bound printed; the synthetic offsets are not integers)
        atomic_bytes = 36.0 * Cin * 4 * N * H * H
        rec = {'shape': name, 'nodes': cnt, 'batch': N, 'H': H, 'Cin': Cin, 'Cout': Cout,
               'us': {k: round(v, 1) for k, v in t.items()},
               'backward_over_forward': round((t['data'] + t['weight']) / t['forward'], 2),
               'atomic_MB': round(atomic_bytes / 1e6, 1),
               'atomic_floor_us': round(atomic_bytes / ATOMIC_RATE * 1e6, 1),
               'atomic_TBps_of_data_kernel': round(atomic_bytes / (t['data'] * 1e-6) / 1e12, 3),
               'weight_workspace_MB': round(need / 1e6, 1)}
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--off-scale', type=float, default=1.0, help='std (pixels) of the synthetic offsets')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child process')
    ap.add_argument('--json', default='', help='append the JSON lines to this file')
    ap.add_argument('--batch', type=int, default=0, help=argparse.SUPPRESS)       # (child mode)
    args = ap.parse_args()
    if args.batch:
        return child(args)
    rows = []
    for b in [int(v) for v in args.batches.split(',')]:
        cmd = [sys.executable, os.path.abspath(__file__), '--batch', str(b), '--size', str(args.size), '--reps', str(args.reps),
               '--off-scale', str(args.off_scale)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('batch %d failed with exit status %d: nothing more is started' % (b, r.returncode))
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    if args.json:
        with open(args.json, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')
    print('%-18s %2s %9s %9s %9s %9s %7s %9s %9s' % ('shape', 'B', 'fwd us', 'data us', 'no-gx us', 'weight us', 'bwd/fwd',
                                                  'floor us', 'atom TB/s'))
    for r in rows:
        u = r['us']
        print('%-18s %2d %9.1f %9.1f %9.1f %9.1f %7.2f %9.1f %9.3f' % (r['shape'], r['batch'], u['forward'], u['data'], u['data_no_gx'],
                                                                     u['weight'], r['backward_over_forward'], r['atomic_floor_us'],
                                                                     r['atomic_TBps_of_data_kernel']))
    for r in rows:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
