"""Raw video frames into StreamDetector.step: today's list of ndarrays against VideoFrames.

MOT17 heads (weights.MOT_HEADS), DLA-34, 512 x 512 network input, 1920 x 1080 sources, a rotating pool of eight seeded frames (stream s shows
frame (i + s) % 8 at step i), one and eight streams.  Routes:

  a  ndarray         a list of uint8 BGR arrays: per stream one host copy into pinned staging, one H2D, one ct_preprocess_device
                     (the path that was there before VideoFrame; it is the YARDSTICK of every other route)
  b  bgr_pinned      VideoFrame BGR in pinned host memory, with prefetch: bytes staged ahead, one ct_preprocess_frames launch
  c  nv12_pinned     VideoFrame NV12 in pinned host memory, with prefetch
  d  nv12_device     VideoFrame NV12 already on the device (a hardware decoder's surface): nothing is uploaded
  e  float_tensor    the normalised float32 tensor with prefetch: the ceiling (no pre-processing in the step at all)

Every (route, streams) measurement runs in a process of its own; the routes alternate inside a repetition, three repetitions.
Per measurement: frames/s over --steps steps behind --warmup, bytes uploaded per frame (a count), the device time of the
pre-process launch(es) of one step from events (median of 20; route a: the B ct_preprocess_device launches without their
copies), and the step's host-side timers.  The summary line per (route, streams) gives the three figures, their median and
whether the route is slower than route a by more than a's own spread (max - min of its repetitions).

Appends to profiles/video_frames_bench.jsonl.  Fails without a GPU.

    python tools/video_frames_bench.py [--streams 1,8] [--reps 3] [--steps 200] [--warmup 20] [--routes a,b,c,d,e]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROUTES = {'a': 'ndarray', 'b': 'bgr_pinned', 'c': 'nv12_pinned', 'd': 'nv12_device', 'e': 'float_tensor'}
SRC_H, SRC_W, INP = 1080, 1920, 512
POOL = 8


def child(route, B, steps, warmup):
    import torch
    if not torch.cuda.is_available():
        sys.exit('video_frames_bench.py measures on a GPU: none found')
    from centertrack_amd import _lib, frames as F, weights as W
    from centertrack_amd.detector import Detector, StreamDetector, default_opt
    from centertrack_amd.model import DLASegHIP
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    heads = W.MOT_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=317, hm_gain=14.0)
    sd['ltrb_amodal.2.bias'] = torch.tensor([-3.0, -3.0, 3.0, 3.0])
    opt = default_opt(heads, track_thresh=0.4, pre_thresh=0.5, input_h=INP, input_w=INP)
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    det = StreamDetector(opt, model=model, num_streams=B)
    helper = Detector(opt, model=model)
    rs = np.random.RandomState(317)
    yuv = [rs.randint(0, 256, (SRC_H * 3 // 2, SRC_W)).astype(np.uint8) for _ in range(POOL)]
    bgr = [F.nv12_to_bgr(y) for y in yuv]                                   # every route sees the same pictures
    meta = helper.frame_meta(bgr[0])
    metas = [meta] * B

    def pinned(arr, fmt):
        buf = F.pinned_frame(fmt, SRC_H, SRC_W)
        buf[...] = arr
        return F.VideoFrame(buf, fmt)

    # stream s shows frame (i + s) % POOL at step i: eight frames in all, the streams of a step see different ones
    upload = 0
    if route == 'a':
        one, upload = bgr, SRC_H * SRC_W * 3
    elif route == 'b':
        one, upload = [pinned(x, 'bgr24') for x in bgr], SRC_H * SRC_W * 3
    elif route == 'c':
        one, upload = [pinned(x, 'nv12') for x in yuv], SRC_H * SRC_W * 3 // 2
    elif route == 'd':
        one = [F.VideoFrame(torch.from_numpy(x).to(dev), 'nv12') for x in yuv]
    else:
        one, upload = [helper.pre_process(x, 1.0)[0][0:1] for x in bgr], 3 * INP * INP * 4
    pool = [[one[(i + s) % POOL] for s in range(B)] for i in range(POOL)]
    if route == 'e':
        pool = [torch.cat(row, 0).pin_memory() for row in pool]
    prefetch = route in ('b', 'c', 'e')
    timers, acc = {}, {'pre': 0.0, 'net': 0.0, 'track': 0.0}

    def run(n, first):
        for i in range(first, first + n):
            nxt = pool[(i + 1) % POOL] if prefetch else None
            det.step(pool[i % POOL], metas, timers, prefetch=nxt,
                     prefetch_metas=metas if route == 'e' else None)
            for k in acc:
                acc[k] += timers.get(k, 0.0)

    run(warmup, 0)
    torch.cuda.synchronize()
    for k in acc:
        acc[k] = 0.0
    t0 = time.perf_counter()
    run(steps, warmup)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    # the device time of one step's pre-process launch(es), from events
    pre_us = None
    if route != 'e':
        lib, ctx = _lib.load(), det._ctx
        det.reset_tracking()
        scratch = torch.empty_like(ctx.frames[0])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        devs = [torch.from_numpy(np.ascontiguousarray((bgr if route in ('a', 'b') else yuv)[s % POOL])).to(dev) for s in range(B)]
        vf = [F.VideoFrame(d, 'bgr24' if route == 'b' else 'nv12') for d in devs] if route != 'a' else None
        launcher = F.FrameLauncher(dev, B)
        plane, trans, ms = 3 * INP * INP * 4, np.ascontiguousarray(meta['trans_input'], np.float64), []
        for _ in range(25):
            ev[0].record()
            if route == 'a':
                for s in range(B):
                    _lib.check(lib.ct_preprocess_device(devs[s].data_ptr(), SRC_H, SRC_W, SRC_W * 3, 3, trans.ctypes.data, INP, INP,
                                                        det._lut.data_ptr(), scratch[s].data_ptr(), None, _lib.stream_ptr()), 'pre')
            else:
                launcher.launch(vf, [d.data_ptr() for d in devs], [trans] * B,
                                [scratch.data_ptr() + s * plane for s in range(B)], [None] * B, INP, INP, det._lut.data_ptr())
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        pre_us = round(float(np.median(ms[5:])) * 1e3, 2)
    rec = {'tool': 'video_frames_bench', 'kind': 'run', 'route': route, 'name': ROUTES[route], 'streams': B, 'steps': steps,
           'warmup': warmup, 'frames_per_s': round(steps * B / wall, 2), 'ms_per_step': round(wall / steps * 1e3, 4),
           'bytes_uploaded_per_frame': int(upload), 'preprocess_device_us_per_step': pre_us,
           'native_loop': det._ctx.loop is not None,
           'host_ms_per_step': {k: round(v / steps * 1e3, 4) for k, v in acc.items()}}
    print('RESULT ' + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,8')
    ap.add_argument('--routes', default='a,b,c,d,e')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--child', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'video_frames_bench.jsonl'))
    args = ap.parse_args()
    if args.child:
        child(args.child, int(args.streams), args.steps, args.warmup)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit('video_frames_bench.py measures on a GPU: none found')
    if args.steps < 200:
        print('note: fewer than 200 steps per route: a smoke run, not the measurement of DESIGN.md section 27', file=sys.stderr)
    routes, streams = args.routes.split(','), [int(s) for s in args.streams.split(',')]
    runs = []
    for rep in range(args.reps):
        for B in streams:
            for r in routes:                                 # (alternated: every repetition visits every route once)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', r, '--streams', str(B),
                                    '--steps', str(args.steps), '--warmup', str(args.warmup)],
                                   capture_output=True, text=True, timeout=600)
                line = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
                if p.returncode != 0 or not line:
                    sys.exit('route %s, %d stream(s) failed (%d):\n%s' % (r, B, p.returncode, p.stderr[-3000:]))
                rec = json.loads(line[-1][7:])
                rec['rep'] = rep
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    out = list(runs)
    for B in streams:
        base = [x['frames_per_s'] for x in runs if x['route'] == 'a' and x['streams'] == B]
        spread = (max(base) - min(base)) if base else None
        for r in routes:
            mine = [x for x in runs if x['route'] == r and x['streams'] == B]
            fps = [x['frames_per_s'] for x in mine]
            s = {'tool': 'video_frames_bench', 'kind': 'summary', 'route': r, 'name': ROUTES[r], 'streams': B,
                 'frames_per_s_all': fps, 'frames_per_s_median': round(float(np.median(fps)), 2),
                 'bytes_uploaded_per_frame': mine[0]['bytes_uploaded_per_frame'],
                 'preprocess_device_us_per_step': [x['preprocess_device_us_per_step'] for x in mine],
                 'host_ms_per_step': mine[len(mine) // 2]['host_ms_per_step']}
            if base:
                s['route_a_median'], s['route_a_spread'] = round(float(np.median(base)), 2), round(spread, 2)
                s['slower_than_a_by_more_than_its_spread'] = bool(np.median(fps) < np.median(base) - spread)
            out.append(s)
            print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in out:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
