"""GPU parity of the whole HIP forward (stems -> DLA-34 -> DCN neck -> heads) against the
CPU oracle (oracle/dla34.py, itself pinned to the reference by tests/golden) and against
the reference golden vectors directly."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _report(name, got, want):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    err = (got - want).abs()
    return '%-28s max_abs_err %.3e  (ref absmax %.3f)' % (name, float(err.max()), float(want.abs().max()))


_FORWARD_CASES = [('mot', (1, 64, 96), 0.01), ('nusc', (2, 64, 64), 0.01), ('mot', (1, 128, 160), 0.1),
                  ('coco', (2, 64, 64), 0.01), ('kitti', (1, 96, 128), 0.05), ('pose', (1, 64, 96), 0.01)]
# head_conv 64: the dense head forms without a fused launch -- the block-diagonal `heads.2` (MOT, 11 output channels) and
# conv3x3 + per-head tails (COCO: 86 channels; pose: hm_hp keeps its own sigmoid range)
_FORWARD_CASES_64 = [('mot', (1, 64, 96), 0.01), ('coco', (2, 64, 64), 0.01), ('pose', (1, 64, 96), 0.01)]


# (the cases at 256 keep the ids they had before head_conv was a parameter)
@pytest.mark.parametrize('name,shape,off_std,head_conv', [
    pytest.param(n, s, o, 256, id='%s-shape%d-%s' % (n, i, o)) for i, (n, s, o) in enumerate(_FORWARD_CASES)] + [
    pytest.param(n, s, o, 64, id='%s-head_conv64' % n) for n, s, o in _FORWARD_CASES_64])
def test_forward_matches_oracle(device, golden_dir, name, shape, off_std, head_conv):
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    from oracle import dla34
    heads = {'mot': W.MOT_HEADS, 'nusc': W.NUSC_HEADS, 'coco': W.COCO_HEADS, 'kitti': W.KITTI_HEADS,
             'pose': W.POSE_HEADS}[name]
    sd = W.make_synthetic_state_dict(heads, seed=317, off_std=off_std, head_conv=head_conv)
    x, pre, hm = W.synthetic_inputs(*shape, seed=317)
    model = DLASegHIP(heads, head_conv=head_conv)
    assert set(model.state_dict().keys()) == set(sd.keys())
    model.load_state_dict(sd)
    model = model.to(device)
    got = model(x.to(device), pre.to(device), hm.to(device))[-1]
    torch.cuda.synchronize()
    with torch.no_grad():
        feat = dla34.dla_seg_features(x, pre, hm, sd)
        want = dla34.apply_heads(feat, heads, sd)
    # intermediate report first (so a failure localises itself)
    plan = model.get_plan(shape[0], shape[1], shape[2], True, True, False)
    lines = [_report('feature', plan['feat'].to_nchw(), feat)]
    for k in heads:
        lines.append(_report('head ' + k, got[k], want[k]))
    print('\n'.join(lines))
    np.testing.assert_allclose(plan['feat'].to_nchw().cpu().numpy(), feat.numpy(), atol=1e-3, rtol=1e-3)
    for k in heads:
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].numpy(), atol=1e-3, rtol=1e-3, err_msg=k)
    # the bar of tests/test_hip_ckpt_weights.py beside the one above: err against the float64 oracle, relative to the tensor's
    # maximum, within 10 x what the float32 oracle does on the same data (never below 10 x 2^-23 sqrt(4608))
    import _ckpt_weights as C
    with torch.no_grad():
        t64, _ = C.oracle_run(sd, (x, pre, hm), heads, torch.float64)
    rows = [('feature', plan['feat'].to_nchw().cpu(), feat)] + [('head ' + k, got[k].cpu(), want[k]) for k in heads]
    rows = [(k, C.err(w32, t64[k]), C.err(g, t64[k])) for k, g, w32 in rows]
    print('\n'.join('%-28s e32 %.2e  err %.2e  err / bound %.3f' % (k, e32, e, e / C.bound(e32)) for k, e32, e in rows))
    for k, e32, e in rows:
        assert e <= C.bound(e32), (k, e32, e, C.bound(e32))
    if off_std == 0.01 and shape[1] == 64 and name in ('mot', 'nusc') and head_conv == 256:      # (recorded at 256)
        g = np.load(os.path.join(golden_dir, 'model_forward.npz'))
        for k in heads:
            np.testing.assert_allclose(got[k].cpu().numpy(), g['%s.%s' % (name, k)], atol=1e-3, rtol=1e-3,
                                       err_msg='golden ' + k)
        got2 = model(x.to(device), pre.to(device), None)[-1]
        np.testing.assert_allclose(got2['hm'].cpu().numpy(), g[name + '_nohm.hm'], atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize('name,h,w', [('mot_512', 512, 512), ('mot_544x960', 544, 960)])
def test_forward_full_size_matches_reference_golden(device, golden_dir, name, h, w):
    """the HIP forward against the REFERENCE's DLASeg at the benchmarked sizes (tests/golden/model_forward_full.npz: the
    full hm map, the regression heads at stride 2): 512 x 512 = BASELINE configs[1], 544 x 960 = the reference's own MOT
    input with its ragged 17 x 30 / 34 x 60 deep maps; 1e-3 like north_star asks"""
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    g = np.load(os.path.join(golden_dir, 'model_forward_full.npz'))
    heads = W.MOT_HEADS
    model = DLASegHIP(heads)
    model.load_state_dict(W.make_synthetic_state_dict(heads, seed=317))
    model = model.to(device)
    x, pre, hm = W.synthetic_inputs(1, h, w, seed=317)
    got = model(x.to(device), pre.to(device), hm.to(device))[-1]
    torch.cuda.synchronize()
    for k in heads:
        v = got[k].cpu().numpy()
        v = v if k == 'hm' else v[:, :, ::2, ::2]
        print(_report('%s %s' % (name, k), torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(g['%s.%s' % (name, k)])))
        np.testing.assert_allclose(v, g['%s.%s' % (name, k)], atol=1e-3, rtol=1e-3, err_msg=k)


def test_backbone_levels_match_oracle(device):
    """level-by-level check of the DLA backbone outputs (localises a bad layer)."""
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    from oracle import dla34
    heads = W.MOT_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=11)
    x, pre, hm = W.synthetic_inputs(1, 64, 96, seed=11)
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    model = model.to(device)
    model(x.to(device), pre.to(device), hm.to(device))
    torch.cuda.synchronize()
    plan = model.get_plan(1, 64, 96, True, True, False)
    with torch.no_grad():
        base = dla34.dla_base(x, pre, hm, sd)
        ups = dla34.dla_up(base, sd)
    outs = {}
    for l in plan['launches']:
        if l.fn == 'conv' and hasattr(l.out, 'to_nchw'):
            outs[l.name] = l.out
    outs.update({k + '.dcn': v for k, v in plan['dcn_layers'].items()})
    names = ['level0', 'level1', 'base.level2.root', 'base.level3.tree2.root', 'base.level4.tree2.root',
             'base.level5.root']
    refs = list(base) + [ups[2], ups[1], ups[0]]
    names += ['dla_up.ida_0.node_1.dcn', 'dla_up.ida_1.node_2.dcn', 'dla_up.ida_2.node_3.dcn']
    msgs = []
    worst = 0.0
    for n, ref in zip(names, refs):
        e = float((outs[n].to_nchw().cpu() - ref).abs().max())
        worst = max(worst, e / max(1.0, float(ref.abs().max())))
        msgs.append('%-26s err %.3e (absmax %.2f)' % (n, e, float(ref.abs().max())))
    print('\n'.join(msgs))
    assert worst < 2e-4, '\n'.join(msgs)


@pytest.mark.parametrize('head_conv', [256, 64])
def test_fused_sigmoid_and_batch_consistency(device, head_conv):
    """fuse_sigmoid == sigmoid(raw); a batch of 3 equals three batch-1 runs (streams do not mix).  At head_conv 64 the
    nuScenes heads are the block-diagonal `heads.2` launch, with a `sig` and a `dep` range at non-zero channel offsets."""
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    heads = W.NUSC_HEADS
    sd = W.make_synthetic_state_dict(heads, seed=5, hm_gain=8.0, head_conv=head_conv)
    model = DLASegHIP(heads, head_conv=head_conv, depth_scale=2.0)
    model.load_state_dict(sd)
    model = model.to(device)
    x, pre, hm = W.synthetic_inputs(3, 64, 64, seed=5)
    x, pre, hm = x.to(device), pre.to(device), hm.to(device)
    raw = model(x, pre, hm)[-1]
    fused = model(x, pre, hm, fuse_sigmoid=True)[-1]
    np.testing.assert_allclose(fused['hm'].cpu().numpy(), torch.sigmoid(raw['hm']).cpu().numpy(), atol=2e-6)
    dep = (1. / (torch.sigmoid(raw['dep']) + 1e-6) - 1.) * 2.0
    np.testing.assert_allclose(fused['dep'].cpu().numpy(), dep.cpu().numpy(), rtol=1e-4, atol=1e-4)
    for b in range(3):
        one = model(x[b:b + 1], pre[b:b + 1], hm[b:b + 1])[-1]
        for k in heads:
            np.testing.assert_allclose(one[k].cpu().numpy(), raw[k][b:b + 1].cpu().numpy(), atol=1e-4, err_msg=k)


def test_split_stem_is_bit_identical(device):
    """round 3: the x / pre_img terms of the stem computed ahead into a partial map (run_stem_partial) + the pre_hm term
    on top of it (stem_partial=) give the bits of the single three-term launch -- for the stem output and for every
    head map of the forward"""
    from centertrack_amd import ops, weights as W
    from centertrack_amd.model import DLASegHIP
    heads = W.MOT_HEADS
    model = DLASegHIP(heads)
    model.load_state_dict(W.make_synthetic_state_dict(heads, seed=5))
    model = model.to(device)
    N, H, Wd = 2, 96, 160
    x, pre, hm = W.synthetic_inputs(N, H, Wd, seed=11)
    x, pre, hm = x.to(device), pre.to(device), hm.to(device)
    plan = model.get_plan(N, H, Wd, True, True, True)
    model._run_plan(plan, inputs=(x, pre, hm))
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in plan['outputs'].items()}
    partial = ops.new_view(N, H, Wd, 16, device)
    model.run_stem_partial(x, pre, partial)
    model._run_plan(plan, inputs=(x, pre, hm), stem_partial=partial)
    torch.cuda.synchronize()
    for k, v in plan['outputs'].items():
        assert torch.equal(v, want[k]), k
    assert float(want['hm'].abs().sum()) > 0
