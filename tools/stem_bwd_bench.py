#!/usr/bin/env python
"""Forward and forward + backward of the three trainable 7x7 stems (centertrack_amd.dla_base._stems: ct_stem_conv_forward,
ct_bn_stats, ct_stem_bn_relu_sum, ct_bn_relu_backward, ct_stem_conv_backward) against the torch stems they replace -- the same
``nn.Sequential(Conv2d, BatchNorm2d, ReLU)`` objects called by torch on NCHW tensors, vendor convolutions, two adds, and one
conversion of the sum to NHWC -- and one training step of ``dla_seg.DLASeg`` (all NHWC, HIP stems) against the hand-assembled
chain ``dla34 -> DLAUp -> IDAUp -> FusedHeads`` with NCHW module boundaries and the torch stems.  One GPU, training mode,
512 x 512 input with ``pre_img`` and ``pre_hm``, batch 1 and 4; every parameter something reads asks for a gradient, the images
do not.

Per configuration one JSON line in profiles/stem_bwd_bench.jsonl: milliseconds of the forward and of the backward of each
(device events around each part, the implementations alternating in one process, the best round of each and every round) and
the largest difference of the outputs and of the parameter gradients between the two of a pair (relative to the tensor's
maximum).  The first line carries ``box_calibration`` (tools/box_calib.py): the state of the machine the figures were taken
on.  The method is tools/backbone_bwd_bench.py's.

    python tools/stem_bwd_bench.py
    python tools/stem_bwd_bench.py --configs b1 --steps 10
"""
import argparse
import copy
import json
import os
import sys
from collections import OrderedDict

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

#           name  B  H    W
CONFIGS = {'b1': (1, 512, 512), 'b4': (4, 512, 512)}
HEADS = OrderedDict([('hm', 1), ('reg', 2), ('wh', 2), ('tracking', 2)])
STEMS = ('base_layer', 'pre_img_layer', 'pre_hm_layer')
UNREAD = ('base.level3.project.', 'base.level4.project.')


class Opt(object):
    pre_img, pre_hm = True, True
    dla_node, head_kernel, prior_bias, model_output_list, load_model = 'dcn', 3, -4.6, False, ''


def torch_base_nhwc(base, x, pre, hm):
    """``DLA.forward_nhwc`` with the torch stems: NCHW modules, their sum converted once"""
    from centertrack_amd import dla_base
    return base._levels_nhwc(dla_base.to_nhwc(base._stems(x, pre, hm)))


def steppers(name, device):
    """{'stems_hip' | 'stems_torch' | 'step_dlaseg' | 'step_chain': (forward, backward)}: ``forward()`` -> outputs,
    ``backward(outputs)`` -> the parameter gradients"""
    import torch
    from centertrack_amd import dcn_v2, dla_base, dla_up, heads as HD
    from centertrack_amd.dla_seg import DLASeg
    B, H, W = CONFIGS[name]
    g = torch.Generator().manual_seed(5)
    x, pre = (torch.randn((B, 3, H, W), generator=g).to(device) for _ in range(2))
    hm = torch.rand((B, 1, H, W), generator=g).to(device)
    torch.manual_seed(5)
    model = DLASeg(34, HEADS, {h: [256] for h in HEADS}, Opt()).to(device).train()
    chain = copy.deepcopy(model)                   # the same tensors, called module by module
    chain_heads = HD.FusedHeads(HEADS).to(device)
    chain_heads.load_state_dict({k: v for k, v in model.state_dict().items() if k.split('.')[0] in HEADS})
    gy = torch.randn((B, H, W, 16), generator=g).to(device) / (B * H * W) ** 0.5
    glog = [torch.randn((B, c, H // 4, W // 4), generator=g).to(device) / (B * H * W / 16) ** 0.5 for c in HEADS.values()]

    def stem_leaves(base):
        return [p for s in STEMS for p in getattr(base, s).parameters()]

    def stems_hip():
        with dcn_v2.trainable():
            return [dla_base._stems([x, pre, hm], [getattr(model.base, s) for s in STEMS])]

    def stems_torch():
        with dcn_v2.trainable():
            return [dla_base.to_nhwc(chain.base._stems(x, pre, hm))]

    def step_dlaseg():
        with dcn_v2.trainable():
            return list(model(x, pre, hm)[0].values())

    def step_chain():
        with dcn_v2.trainable():
            levels = [dla_base.to_nchw(t) for t in torch_base_nhwc(chain.base, x, pre, hm)]
            layers = chain.dla_up(levels)
            y = [layers[i].clone() for i in range(3)]
            chain.ida_up(y, 0, len(y))
            return list(chain_heads(y[-1]).values())
    leaves_m = [p for k, p in model.named_parameters() if not k.startswith(UNREAD)]
    leaves_c = [p for k, p in chain.named_parameters() if not k.startswith(UNREAD) and k.split('.')[0] not in HEADS]
    leaves_c += list(chain_heads.parameters())
    return OrderedDict([
        ('stems_hip', (stems_hip, lambda o: torch.autograd.grad(o, stem_leaves(model.base), [gy]))),
        ('stems_torch', (stems_torch, lambda o: torch.autograd.grad(o, stem_leaves(chain.base), [gy]))),
        ('step_dlaseg', (step_dlaseg, lambda o: torch.autograd.grad(o, leaves_m, glog))),
        ('step_chain', (step_chain, lambda o: torch.autograd.grad(o, leaves_c, glog)))])


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
    for k, (f, b) in fns.items():
        for i in range(warmup):
            outs = f()
            res[k] = ([o.detach() for o in outs], b(outs))
    torch.cuda.synchronize()
    # a pair computes the same function: sums in another order differ in the last bits, anything larger wants an explanation.
    # (The parameter lists of the step pair are in two orders -- the chain's heads come last -- so only its outputs are held.)
    rec['stems_outputs_max_rel_diff'] = max(rel(a, b) for a, b in zip(res['stems_hip'][0], res['stems_torch'][0]))
    rec['stems_grads_max_rel_diff'] = max(rel(a, b) for a, b in zip(res['stems_hip'][1], res['stems_torch'][1]))
    rec['step_outputs_max_rel_diff'] = max(rel(a, b) for a, b in zip(res['step_dlaseg'][0], res['step_chain'][0]))
    del res
    ms = {k: [] for k in fns}
    for _ in range(rounds):                       # they alternate, so that a drift of the machine hits all of them
        for k, (f, b) in fns.items():
            ms[k].append(time_parts(f, b, steps))
    for k in fns:
        best = min(ms[k], key=lambda v: v[0] + v[1])
        rec['fwd_ms_' + k], rec['bwd_ms_' + k] = round(best[0], 4), round(best[1], 4)
        rec['ms_%s_all' % k] = [[round(v, 4) for v in r] for r in ms[k]]
    rec['stems_fwd_torch_over_hip'] = round(rec['fwd_ms_stems_torch'] / rec['fwd_ms_stems_hip'], 2)
    rec['stems_step_torch_over_hip'] = round((rec['fwd_ms_stems_torch'] + rec['bwd_ms_stems_torch'])
                                             / (rec['fwd_ms_stems_hip'] + rec['bwd_ms_stems_hip']), 2)
    rec['step_chain_over_dlaseg'] = round((rec['fwd_ms_step_chain'] + rec['bwd_ms_step_chain'])
                                          / (rec['fwd_ms_step_dlaseg'] + rec['bwd_ms_step_dlaseg']), 2)
    return rec


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
    ap.add_argument('--no-box-probes', action='store_true', help='box_calibration without the latency / clock probes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stem_bwd_bench.jsonl'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('stem_bwd_bench.py measures on a GPU: none found')
    recs = []
    for name in args.configs.split(','):
        rec = measure(name, args.steps, args.warmup, args.rounds)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        write(args.out, recs)
    torch.cuda.synchronize()
    try:
        from tools import box_calib
        recs[0]['box_calibration'] = box_calib.box_calibration(torch.device('cuda:0'), probes=not args.no_box_probes)
    except Exception as e:                          # a probe must never cost the bench lines
        recs[0]['box_calibration'] = {'error': repr(e)}
    torch.cuda.synchronize()
    write(args.out, recs)


if __name__ == '__main__':
    main()
