"""The pose task, dense heads against ``opt.sparse_pose_heads``: one ``StreamDetector`` step.

``weights.POSE_HEADS`` (hm, reg, wh, tracking, hps, hm_hp, hp_offset) on synthetic weights at 512 x 512, 1 and 4 streams,
``flip_test`` off and on, alternating in one process:

  dense    every head a map (two wide heads, five in the fused launch), ct_decode + ct_decode_pose
  sparse   hm and hm_hp as maps; reg / wh / tracking at the K winners (ct_sparse_heads_desc), hps at the winners and hp_offset
           at the K peaks of every joint map (ct_decode_pose_sparse)

Per contestant: ``ms_step`` -- host clock around ``steps`` calls of ``step()`` (frames resident on the device; each call ends
with the rows on the host and the tracker updated), per step; ``ms_device`` -- device events around ``steps`` replays of the
captured frame graph; ``ms_heads`` -- the same around a captured graph of the part that differs: head launches, flip merge,
decode, pose decode; each the minimum over ``rounds`` (every round is listed).  ``heads_share`` = ms_heads / ms_device.
``launches`` -- kernels and copies of one eager frame as the torch profiler lists them (null when the profiler is not
available); ``plan_launches`` -- entries of the launch plan.

Appends one line per configuration to profiles/sparse_pose_bench.jsonl; the first line of a run carries ``box_calibration``.

    python tools/sparse_pose_bench.py [--steps 50] [--warmup 5] [--rounds 3] [--out profiles/sparse_pose_bench.jsonl]
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

H = W = 512


def count_launches(step):
    """kernels and copies of one step, from the torch profiler; None when it cannot be had"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(e.device_type).endswith('CUDA')]
        copies = [e for e in evs if 'memcpy' in e.name.lower()]
        return {'kernels': len(evs) - len(copies), 'copies': len(copies)} if evs else None
    except Exception:
        return None


def heads_part(det, ctx):
    """the launches of a frame behind the feature map: heads, flip merge, decode (``_FrameContext.device_frame`` from there on)"""
    from centertrack_amd import _lib
    lib = _lib.load()
    launches = [l for l in ctx.plan['launches'] if l.fn == 'heads' or l.name.startswith('heads.')]

    def run():
        det.model._run_plan(ctx.plan, launches=launches)
        if det.flip:
            arr, n, pairs, h, w = ctx.flip_call
            _lib.check(lib.ct_flip_merge(arr, n, pairs.ctypes.data, len(pairs), det.B, h, w, _lib.stream_ptr()), 'ct_flip_merge')
        ctx.decoder.run()
    return run


def measure(model, streams, flip, steps, warmup, rounds):
    import torch
    from centertrack_amd import weights as Wt
    from centertrack_amd.detector import StreamDetector, _HipGraph, default_opt
    from centertrack_amd.image import make_meta
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(11)
    frames = [torch.randn((streams, 3, H, W), generator=g).to(dev) for _ in range(4)]
    metas = [make_meta(H, W, 2 * H, 2 * W) for _ in range(streams)]
    dets = OrderedDict()
    for name, on in (('dense', False), ('sparse', True)):
        opt = default_opt(Wt.POSE_HEADS, track_thresh=0.3, flip_test=flip, input_h=H, input_w=W, sparse_pose_heads=on)
        dets[name] = StreamDetector(opt, model=model, num_streams=streams)
    t = [0]

    def step(name):
        t[0] += 1
        return dets[name].step(frames[t[0] % len(frames)], [dict(m) for m in metas])
    for name in dets:
        for _ in range(max(warmup, 2)):
            step(name)
    torch.cuda.synchronize()
    assert dets['sparse'].sparse_pose and not dets['dense'].sparse_pose
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def replay_ms(graph):
        for _ in range(warmup):
            graph.replay()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(steps):
            graph.replay()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps
    ms = {k: {'step': [], 'device': [], 'heads': []} for k in dets}
    for _ in range(rounds):
        for name in dets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(name)
            torch.cuda.synchronize()
            ms[name]['step'].append((time.perf_counter() - t0) * 1e3 / steps)
    parts = {}
    for name, det in dets.items():
        ctx = det._ctx
        run = heads_part(det, ctx)
        run()
        torch.cuda.synchronize()
        parts[name] = (ctx.graphs[0], _HipGraph(run, collect=False))
    for _ in range(rounds):                       # (replays behind the last step: the frame loops are idle from here on)
        for name in dets:
            ms[name]['device'].append(replay_ms(parts[name][0]))
            ms[name]['heads'].append(replay_ms(parts[name][1]))
    rec = {'tool': 'sparse_pose_bench', 'heads': 'pose', 'input': [H, W], 'streams': streams, 'flip_test': flip, 'K': 100,
           'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per step / per replay of the frame graph / per replay of heads + flip merge + decode; min over rounds '
                   '(each the mean of `steps`); *_all: every round'}
    for name, det in dets.items():
        ctx = det._ctx
        for k in ('step', 'device', 'heads'):
            rec['ms_%s_%s' % (k, name)] = round(min(ms[name][k]), 4)
            rec['ms_%s_%s_all' % (k, name)] = [round(v, 4) for v in ms[name][k]]
        rec['heads_share_' + name] = round(rec['ms_heads_' + name] / rec['ms_device_' + name], 3)
        rec['plan_launches_' + name] = len(ctx.plan['launches'])
        rec['launches_' + name] = count_launches(lambda: ctx.device_frame(0))
    for k in ('step', 'device', 'heads'):
        rec['dense_over_sparse_' + k] = round(rec['ms_%s_dense' % k] / rec['ms_%s_sparse' % k], 3)
    for det in dets.values():
        det._ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,4')
    ap.add_argument('--flips', default='0,1')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-box-probes', action='store_true', help='box_calibration without the latency / clock probes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_pose_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('sparse_pose_bench.py measures on a GPU: none found')
    from centertrack_amd import weights as Wt
    from centertrack_amd.model import DLASegHIP
    model = DLASegHIP(Wt.POSE_HEADS)
    model.load_state_dict(Wt.make_synthetic_state_dict(Wt.POSE_HEADS, seed=21, hm_gain=14.0))
    recs = []
    for streams in (int(v) for v in args.streams.split(',')):
        for flip in (bool(int(v)) for v in args.flips.split(',')):
            rec = measure(model, streams, flip, args.steps, args.warmup, args.rounds)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    try:
        from tools import box_calib
        recs[0]['box_calibration'] = box_calib.box_calibration(torch.device('cuda:0'), probes=not args.no_box_probes)
    except Exception as e:                          # a probe must never cost the bench lines
        recs[0]['box_calibration'] = {'error': repr(e)}
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
