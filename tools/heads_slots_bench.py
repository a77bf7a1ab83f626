"""The training heads, dense against slots: forward + backward of ``heads.FusedHeads`` per step.

On a random 64-channel feature map that requires a gradient, alternating in one process:

  dense   ``FusedHeads(heads)``: every head a full map, today's path and the yardstick
  slots   ``FusedHeads(heads, slot_heads=True)`` called with ``ind``: the heads of ``heads.SLOT_HEADS`` at M cells per image

Head sets: MOT (hm, reg, wh, tracking, ltrb_amodal) and nuScenes (ten heads); map 128 x 128; batch 1 and 4; M 128 and 256.
``ind`` is random without regard to duplicates, every slot valid.  Both modules hold the same parameters; the incoming
gradients are random tensors made once.  Per contestant: ``ms`` -- device events around ``steps`` forward + backward steps,
per step, the minimum over ``rounds`` (every round is listed); ``launches`` -- kernels and copies of one step as the torch
profiler lists them (null when the profiler is not available); ``peak_bytes`` -- ``max_memory_allocated`` of one step above
what was allocated before it.

Appends one line per configuration to profiles/heads_slots_bench.jsonl; the first line of a run carries ``box_calibration``.

    python tools/heads_slots_bench.py [--steps 10] [--warmup 2] [--rounds 3] [--out profiles/heads_slots_bench.jsonl]
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEAD_SETS = OrderedDict([
    ('mot', OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2), ('ltrb_amodal', 4)])),
    ('nusc', OrderedDict([('hm', 10), ('reg', 2), ('wh', 2), ('tracking', 2), ('dep', 1), ('rot', 8), ('dim', 3),
                          ('amodel_offset', 2), ('nuscenes_att', 8), ('velocity', 3)]))])
H = W = 128


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


def measure(hs, B, M, steps, warmup, rounds):
    import torch
    from centertrack_amd import heads as HD
    dev = torch.device('cuda:0')
    heads = HEAD_SETS[hs]
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn((B, H, W, 64), device=dev, generator=g).requires_grad_()
    ind = torch.randint(0, H * W, (B, M), device=dev, generator=g)
    torch.manual_seed(3)
    mods = OrderedDict([('dense', HD.FusedHeads(heads).to(dev)), ('slots', HD.FusedHeads(heads, slot_heads=True).to(dev))])
    mods['slots'].load_state_dict(mods['dense'].state_dict())
    gouts = {}
    for name, m in mods.items():
        out = m.forward_nhwc(x.detach(), ind)
        gouts[name] = [torch.randn(o.shape, device=dev, generator=g) for o in out.values()]

    def step(name):
        m = mods[name]
        m.zero_grad(set_to_none=True)
        x.grad = None
        out = m.forward_nhwc(x, ind)
        torch.autograd.backward(list(out.values()), gouts[name])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in mods}
    for name in mods:
        for _ in range(warmup):
            step(name)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name in mods:
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(steps):
                step(name)
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]) / steps)
    peak = {}
    for name in mods:
        mods[name].zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(name)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    launches = {name: count_launches(lambda: step(name)) for name in mods}
    rec = {'tool': 'heads_slots_bench', 'heads': hs, 'nheads': len(heads), 'slot_heads': list(mods['slots'].slot_head_names()),
           'batch': B, 'map': [H, W], 'M': M, 'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'note': 'ms per forward + backward step; min over rounds (each the mean of `steps` steps); *_all: every round'}
    for k in mods:
        rec['ms_' + k] = round(min(ms[k]), 4)
        rec['ms_%s_all' % k] = [round(v, 4) for v in ms[k]]
        rec['launches_' + k] = launches[k]
        rec['peak_bytes_' + k] = peak[k]
    rec['dense_over_slots'] = round(rec['ms_dense'] / rec['ms_slots'], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', default=','.join(HEAD_SETS))
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--slots', default='128,256')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-box-probes', action='store_true', help='box_calibration without the latency / clock probes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'heads_slots_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('heads_slots_bench.py measures on a GPU: none found')
    recs = []
    for hs in args.heads.split(','):
        for B in (int(v) for v in args.batches.split(',')):
            for M in (int(v) for v in args.slots.split(',')):
                rec = measure(hs, B, M, args.steps, args.warmup, args.rounds)
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
