"""Training targets: the reference's way against TargetBuilder.render, per batch.

Two ways to get the targets of one training batch onto the device, alternating in one process:

  cpu     ``encode`` + ``tb.reference`` for every sample (the dense maps drawn with numpy, as a DataLoader worker of the
          reference does), ``default_collate``, ``.to(device)`` of every tensor;
  device  ``encode`` for every sample, ``tb.render`` of the records.

Both are timed with wall time around the whole thing (one thread, synchronised at the end) and with device events around
what they enqueue (the uploads / the copy and the launch); the host parts are also given one by one.  A DataLoader
spreads the per-sample host work over its workers; the figures here are per batch on ONE core, so divide the per-sample
parts by the number of workers to compare.  Configurations: ``mot`` (1 class, 512 x 512, B = 32, about 30 objects,
tracking with pre_hm and the disturbances of the MOT experiments), ``coco`` (80 classes, 512 x 512, B = 32, about 20
objects, no pre_hm) and ``pose`` (1 class, 512 x 512, B = 32, about 8 persons with 17 key points
each, the heads of ``tracking,multi_pose``, through ``PoseTargetBuilder``).  Annotations are synthetic: nothing outside
the repository is read.

Appends one line per configuration to profiles/targets_bench.jsonl; the first line of a run carries ``box_calibration``
(tools/box_calib.py).

    python tools/targets_bench.py [--configs mot,coco,pose] [--steps 10] [--warmup 2] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {'mot': dict(C=1, hw=(512, 512), B=32, objs=30, tracking=True, max_objs=256,
                       heads=('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal'), disturb=(0.05, 0.4, 0.1)),
           'coco': dict(C=80, hw=(512, 512), B=32, objs=20, tracking=False, max_objs=128,
                        heads=('hm', 'reg', 'wh'), disturb=(0.0, 0.0, 0.0)),
           'pose': dict(C=1, hw=(512, 512), B=32, objs=8, tracking=True, max_objs=32, joints=17,
                        heads=('hm', 'reg', 'wh', 'tracking', 'hps', 'hm_hp', 'hp_offset'), disturb=(0.05, 0.4, 0.1))}


def make_builder(cfg):
    from centertrack_amd.targets import PoseTargetBuilder, TargetBuilder
    o = types.SimpleNamespace()
    o.heads = {h: 1 for h in cfg['heads']}
    o.num_classes = cfg['C']
    o.input_h, o.input_w = cfg['hw']
    o.down_ratio = 4
    o.output_h, o.output_w = cfg['hw'][0] // 4, cfg['hw'][1] // 4
    o.tracking = o.pre_hm = cfg['tracking']
    o.hm_disturb, o.lost_disturb, o.fp_disturb = cfg['disturb']
    o.dense_reg = 1
    cat_ids = {i: i for i in range(1, cfg['C'] + 1)}
    if cfg.get('joints'):
        return PoseTargetBuilder(o, cfg['C'], cfg['max_objs'], cat_ids, num_joints=cfg['joints'])
    return TargetBuilder(o, cfg['C'], cfg['max_objs'], cat_ids)


def make_samples(cfg, seed):
    rs = np.random.RandomState(seed)
    H, W = cfg['hw']
    samples = []
    for _ in range(cfg['B']):
        anns = []
        for i in range(max(1, int(rs.poisson(cfg['objs'])))):
            w, h = rs.uniform(8, W * 0.3), rs.uniform(8, H * 0.4)
            anns.append({'bbox': [float(rs.uniform(-w / 4, W - w * 0.75)), float(rs.uniform(-h / 4, H - h * 0.75)),
                                  float(w), float(h)], 'category_id': int(rs.randint(1, cfg['C'] + 1)), 'track_id': i})
            if cfg.get('joints'):              # key points over the box widened by 10 %; visibility 2 / 1 / 0 as 6 : 3 : 1
                x, y = anns[-1]['bbox'][:2]
                kp = []
                for _ in range(cfg['joints']):
                    kp += [float(rs.uniform(x - 0.1 * w, x + 1.1 * w)), float(rs.uniform(y - 0.1 * h, y + 1.1 * h)),
                           int(rs.choice([2, 2, 2, 2, 2, 2, 1, 1, 1, 0]))]
                anns[-1]['keypoints'] = kp
        samples.append(anns)
    return samples


T_OUT = np.array([[0.25, 0, 0], [0, 0.25, 0]], np.float64)
T_IN = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)


def encode_all(tb, cfg, samples, rng):
    H, W = cfg['hw']
    if cfg['tracking']:
        return [tb.encode(a, T_OUT, H, W, pre_anns=a, trans_input_pre=T_IN, trans_output_pre=T_OUT, rng=rng)
                for a in samples]
    return [tb.encode(a, T_OUT, H, W) for a in samples]


def measure(name, steps, warmup, rounds):
    import torch
    from torch.utils.data import default_collate
    cfg = CONFIGS[name]
    dev = torch.device('cuda:0')
    tb = make_builder(cfg)
    samples = make_samples(cfg, 7)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    keys = ('encode', 'reference', 'collate', 'upload_host', 'cpu_wall', 'cpu_device', 'render_host', 'device_wall',
            'device_device')
    ms = {k: [] for k in keys}

    def cpu_way(rng):
        t0 = time.perf_counter()
        recs = encode_all(tb, cfg, samples, rng)
        t1 = time.perf_counter()
        rets = [tb.reference(r) for r in recs]
        t2 = time.perf_counter()
        batch = default_collate(rets)
        t3 = time.perf_counter()
        ev[0].record()
        batch = {k: v.to(dev, non_blocking=True) for k, v in batch.items()}
        ev[1].record()
        t4 = time.perf_counter()
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        return batch, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t0, ev[0].elapsed_time(ev[1]) / 1e3)

    def device_way(rng):
        t0 = time.perf_counter()
        recs = encode_all(tb, cfg, samples, rng)
        t1 = time.perf_counter()
        ev[0].record()
        batch = tb.render(recs, device=dev)
        ev[1].record()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return batch, recs, (t1 - t0, t2 - t1, t3 - t0, ev[0].elapsed_time(ev[1]) / 1e3)

    upload_bytes = record_bytes = 0
    for r in range(rounds):
        acc = {k: [] for k in keys}
        for s in range(warmup + steps):
            a, ta = cpu_way(np.random.RandomState(100 + s))
            b, recs, tbm = device_way(np.random.RandomState(100 + s))
            if r == 0 and s == 0:             # same stream of noise: the two ways must agree
                for k in a:
                    assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
                    assert float((a[k].double() - b[k].double()).abs().max()) <= 1e-6, k
                upload_bytes = sum(v.numel() * v.element_size() for v in a.values())
                record_bytes = sum(v.nbytes for rec in recs for v in rec.values())
            if s < warmup:
                continue
            for k, v in zip(('encode', 'reference', 'collate', 'upload_host', 'cpu_wall', 'cpu_device'), ta):
                acc[k].append(v * 1e3)
            for k, v in zip(('encode', 'render_host', 'device_wall', 'device_device'), tbm):
                acc[k].append(v * 1e3)
        for k in keys:
            ms[k].append(float(np.median(acc[k])))
    rec = {'tool': 'targets_bench', 'config': name, 'B': cfg['B'], 'C': cfg['C'], 'input_hw': list(cfg['hw']),
           'pre_hm': cfg['tracking'], 'objects_per_sample': float(np.mean([len(a) for a in samples])),
           'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'bytes_uploaded_cpu_way': int(upload_bytes), 'bytes_of_records': int(record_bytes),
           'note': 'ms per batch, one host thread; median over steps, then min over rounds; *_all: every round'}
    for k in keys:
        rec['ms_' + k] = round(min(ms[k]), 4)
        rec['ms_%s_all' % k] = [round(v, 4) for v in ms[k]]
    rec['wall_cpu_over_device'] = round(rec['ms_cpu_wall'] / rec['ms_device_wall'], 2)
    # a model, not a measurement: the per-sample host work spread over 16 DataLoader workers, the rest as timed
    per_sample_cpu = rec['ms_encode'] + rec['ms_reference']
    rec['model_16_workers_cpu_over_device'] = round(
        (per_sample_cpu / 16 + rec['ms_cpu_wall'] - per_sample_cpu)
        / (rec['ms_encode'] / 16 + rec['ms_device_wall'] - rec['ms_encode']), 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-box-probes', action='store_true', help='box_calibration without the latency / clock probes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'targets_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('targets_bench.py measures on a GPU: none found')
    torch.set_num_threads(1)
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
