#!/usr/bin/env python
"""Forward and backward of the trainable ``IDAUp`` (centertrack_amd.dla_up) against the same IDAUp composed as the package
allowed before it: the reference's structure (dla.py:506-545) from ``nn.BatchNorm2d``, ``nn.ReLU``, ``nn.ConvTranspose2d`` and
the trainable ``DCN`` drop-in (centertrack_amd.dcn_v2), NCHW between the modules.  One GPU, training mode, every input and
every parameter asks for a gradient.

Per configuration one JSON line in profiles/neck_bwd_bench.jsonl: milliseconds of the forward and of the backward of both
(device events around each part, the two implementations alternating in one process, the best round of each) and
``torch.cuda.max_memory_allocated`` over one forward + backward above what inputs and parameters hold.  The method is
tools/heads_bwd_bench.py's, without its kernel-trace child.

    python tools/neck_bwd_bench.py
    python tools/neck_bwd_bench.py --configs ida_up_b1 --steps 10
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

#           name                 B  o    channels         up_f       level sizes
CONFIGS = {'ida_up_b1': (1, 64, [64, 128, 256], [1, 2, 4], [(128, 128), (64, 64), (32, 32)]),
           'ida_up_b4': (4, 64, [64, 128, 256], [1, 2, 4], [(128, 128), (64, 64), (32, 32)]),
           'dla_up.ida_0_b1': (1, 256, [256, 512], [1, 2], [(32, 32), (16, 16)]),
           'dla_up.ida_0_b4': (4, 256, [256, 512], [1, 2], [(32, 32), (16, 16)])}


def torch_idaup(o, channels, up_f):
    """the baseline: the reference's IDAUp from torch modules and the DCN drop-in"""
    from torch import nn
    from centertrack_amd import dcn_v2, dla_up

    class DeformConv(nn.Module):
        def __init__(self, chi, cho):
            super().__init__()
            self.actf = nn.Sequential(nn.BatchNorm2d(cho, momentum=0.1), nn.ReLU(inplace=True))
            self.conv = dcn_v2.DCN(chi, cho, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)

        def forward(self, x):
            return self.actf(self.conv(x))

    class IDAUp(nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(1, len(channels)):
                f = int(up_f[i])
                up = nn.ConvTranspose2d(o, o, f * 2, stride=f, padding=f // 2, output_padding=0, groups=o, bias=False)
                dla_up.fill_up_weights(up)
                setattr(self, 'proj_%d' % i, DeformConv(channels[i], o))
                setattr(self, 'up_%d' % i, up)
                setattr(self, 'node_%d' % i, DeformConv(o, o))

        def forward(self, layers, startp, endp):
            for i in range(startp + 1, endp):
                k = str(i - startp)
                layers[i] = getattr(self, 'up_' + k)(getattr(self, 'proj_' + k)(layers[i]))
                layers[i] = getattr(self, 'node_' + k)(layers[i] + layers[i - 1])
    return IDAUp()


def steppers(name, device):
    """{'hip': (forward, backward), 'torch': (forward, backward)}: ``forward()`` -> outputs, ``backward(outputs)``"""
    import torch
    from centertrack_amd import dcn_v2, dla_up
    B, o, channels, up_f, sizes = CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn((B, c, h, w), generator=g).to(device).requires_grad_() for c, (h, w) in zip(channels, sizes)]
    gouts = [torch.randn((B, o) + tuple(sizes[0]), generator=g).to(device) for _ in channels[1:]]
    hip = dla_up.IDAUp(o, channels, up_f).to(device).train()
    with torch.no_grad():                          # offsets off the integers, as in a trained network
        for m in hip.modules():
            if isinstance(m, dcn_v2.DCN):
                m.conv_offset_mask.weight.normal_(0, 0.01, generator=None)
                m.conv_offset_mask.bias.normal_(0, 0.1)
    ref = torch_idaup(o, channels, up_f).to(device).train()
    ref.load_state_dict(hip.state_dict())

    def make(mod):
        leaves = list(mod.parameters()) + xs

        def forward():
            layers = list(xs)
            with dcn_v2.trainable():
                mod(layers, 0, len(layers))
            return layers[1:]

        def backward(outs):
            return torch.autograd.grad(outs, leaves, gouts, allow_unused=True)
        return forward, backward
    return {'hip': make(hip), 'torch': make(ref)}


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


def measure(name, steps, warmup, rounds):
    import torch
    device = torch.device('cuda:0')
    fns = steppers(name, device)
    B, o, channels, up_f, sizes = CONFIGS[name]
    rec = {'config': name, 'B': B, 'o': o, 'channels': channels, 'up_f': up_f, 'sizes': sizes, 'steps': steps, 'rounds': rounds}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neck_bwd_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('neck_bwd_bench.py measures on a GPU: none found')
    recs = []
    for name in args.configs.split(','):
        rec = measure(name, args.steps, args.warmup, args.rounds)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for rec in recs:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
