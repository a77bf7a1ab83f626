"""GPU: what the plan builder emits, launch by launch, against tests/golden/plan_launches.json (recorded by
tests/golden/make_plan_golden.py before the builder was rewritten as stages).

tests/test_hip_dcn_forward.py holds the 16 DCN entries of a plan against dcn_schedule; this fixture pins the rest: the
trunk and every head form -- fused, conv3x3 + per-head tails, the block-diagonal `heads.2`, the sparse plans and the
trunk-only plan -- by name, order, descriptor and channel range.  Plans are built with CENTERTRACK_AUTOTUNE=0 (read at
every plan build): fixed DCN knobs and algo 0 everywhere, so nothing here depends on a timing."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_FILE = 'plan_launches.json'
N, H, W = 1, 64, 96


def _cfg(name, heads, head_conv=256, fuse_sigmoid=True, with_inputs=True, fuse_proj=True, **plan_kw):
    return dict(name=name, heads=heads, head_conv=head_conv, fuse_sigmoid=fuse_sigmoid, with_inputs=with_inputs,
                fuse_proj=fuse_proj, plan_kw=plan_kw)


CONFIGS = [_cfg('mot', 'MOT'), _cfg('nusc', 'NUSC'), _cfg('coco', 'COCO'), _cfg('kitti', 'KITTI'), _cfg('pose', 'POSE'),
           _cfg('mot_raw', 'MOT', fuse_sigmoid=False),
           _cfg('mot_no_pre_inputs', 'MOT', with_inputs=False),
           _cfg('mot_sparse', 'MOT', sparse_heads=True), _cfg('kitti_sparse', 'KITTI', sparse_heads=True),
           _cfg('pose_sparse_pose', 'POSE', sparse_pose=True),
           _cfg('mot_trunk_only', 'MOT', trunk_only=True),
           _cfg('mot_hc64', 'MOT', head_conv=64), _cfg('coco_hc64', 'COCO', head_conv=64),
           _cfg('pose_hc64', 'POSE', head_conv=64), _cfg('nusc_hc64', 'NUSC', head_conv=64),
           _cfg('mot_no_fuse_proj', 'MOT', fuse_proj=False)]


def build_plan(cfg, device):
    """One small model and one plan of ``cfg``.  The caller has set CENTERTRACK_AUTOTUNE=0 and ``model.FUSE_PROJ``."""
    from centertrack_amd import weights as Wt
    from centertrack_amd.model import DLASegHIP
    model = DLASegHIP(getattr(Wt, cfg['heads'] + '_HEADS'), head_conv=cfg['head_conv']).to(device)
    wi = cfg['with_inputs']
    return model, model.get_plan(N, H, W, wi, wi, cfg['fuse_sigmoid'], **cfg['plan_kw'])


def summarize(model, plan):
    """The structure of a plan as JSON-ready data"""
    convs, fused = [], []
    for l in plan['launches']:
        d = l.args
        if l.fn == 'conv':
            convs.append([l.name, [d.Cin, d.Cout, d.ks, d.stride, d.flags, d.sig_lo, d.sig_hi, d.dep_lo, d.dep_hi,
                                   bool(d.res), bool(d.pool_y), bool(d.proj_y), d.ldy]])
        elif l.fn == 'heads':
            n = d.nheads
            fused.append([l.name, {'nheads': n, 'ctot': d.ctot, 'cout': list(d.cout[:n]), 'coff': list(d.coff[:n]),
                                   'sig': [d.sig_lo, d.sig_hi], 'dep': [d.dep_lo, d.dep_hi]}])
    sparse = plan['sparse']
    return {'launches': [l.name for l in plan['launches']],
            'signature': model.plan_signature(plan),
            'outputs': sorted(plan['outputs']),
            'sparse': None if sparse is None else [h[0] for h in sparse['heads']],
            'sparse_pose': plan['sparse_pose'] is not None,
            'convs': convs, 'fused': fused}


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        return json.load(f)


@pytest.mark.parametrize('cfg', CONFIGS, ids=[c['name'] for c in CONFIGS])
def test_plan_matches_recorded_structure(device, golden, monkeypatch, cfg):
    from centertrack_amd import model as M
    monkeypatch.setenv('CENTERTRACK_AUTOTUNE', '0')
    monkeypatch.setattr(M, 'FUSE_PROJ', cfg['fuse_proj'])
    model, plan = build_plan(cfg, device)
    got = json.loads(json.dumps(summarize(model, plan)))
    want = golden[cfg['name']]
    # head packings are made when a plan asks for them, under (kind, head names): a trunk-only plan asks for none
    assert any(isinstance(k, tuple) for k in model._prepared) != bool(cfg['plan_kw'].get('trunk_only'))
    assert sorted(got) == sorted(want)
    for key in ('launches', 'outputs', 'sparse', 'sparse_pose', 'fused', 'convs', 'signature'):
        assert got[key] == want[key], '%s: %s differs from the recorded plan' % (cfg['name'], key)
