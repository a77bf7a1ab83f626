"""GPU: ``PoseTargetBuilder.render`` / ct_build_pose_targets (csrc/targets.hip) against the
reference's own ``ret`` with the pose heads (tests/golden/pose_targets.npz) and, beyond the goldens, against
``PoseTargetBuilder.reference`` -- which test_pose_targets_cpu.py holds to the goldens exactly.

The bounds are those of test_hip_targets.py (section 16): slot tensors, the joint tensors included, equal bit for bit;
for hm, hm_hp and pre_hm the sets {map > 0} and {map == 1} identical, max |diff| <= 1e-6 and fewer than 1e-4 of the
pooled map elements unequal."""
import numpy as np
import pytest
import torch

import _pose_targets as P
import _targets as T

pytestmark = pytest.mark.gpu


def to_numpy(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope='module')
def gold():
    return P.golden()


@pytest.fixture(scope='module')
def gold_runs(device, gold):
    """every golden case rendered once: all samples as one batch (P1: the empty sample in the middle) and each alone"""
    runs = {}
    for c in P.CASES:
        case = gold.cases[c]
        tb, opt = P.builder(case['cfg'])
        recs = [gold.encode(tb, s) for s in case['samples']]
        batch = to_numpy(tb.render(recs, device=device))
        singles = [to_numpy(tb.render([r], device=device)) for r in recs]
        runs[c] = {'tb': tb, 'opt': opt, 'recs': recs, 'batch': batch, 'singles': singles,
                   'want': T.stack([s['ret'] for s in case['samples']])}
    return runs


def _case_stats(r, what):
    stats = P.check_batch(r['batch'], r['want'], what + ' batch')
    for i, one in enumerate(r['singles']):
        stats += P.check_batch(one, {k: v[i:i + 1] for k, v in r['want'].items()}, '%s sample %d' % (what, i))
    return stats


@pytest.mark.parametrize('case', P.CASES)
def test_golden_case_slots_bitwise_and_map_geometry(gold, gold_runs, case):
    r = gold_runs[case]
    if case == 'P1':
        e = gold.cases['P1']['empty']
        assert 0 < e < len(r['recs']) - 1 and r['recs'][e]['counts'].tolist() == [0, 0, 0, 0]
        assert not r['batch']['hm_hp'][e].any() and not r['batch']['hp_ind'][e].any()
    stats = _case_stats(r, case)
    assert max(s[0] for s in stats) <= P.MAX_DIFF
    B, M, J = len(r['recs']), r['tb'].max_objs, P.J
    assert r['batch']['hm_hp'].shape == (B, J, 24, 40) and r['batch']['hps'].shape == (B, M, 2 * J)
    assert r['batch']['hp_ind'].dtype == np.int64 and r['batch']['hp_ind'].shape == (B, M * J)
    assert r['batch']['joint'].dtype == np.int64 and r['batch']['hp_offset'].shape == (B, M * J, 2)
    if case == 'P2':
        assert not [k for k in r['batch'] if k.startswith('pre_')] and r['batch']['hm'].shape[1] == 2


def test_golden_maps_within_the_device_exp_bound_all_cases_together(gold_runs):
    stats = []
    for c, r in gold_runs.items():
        stats += _case_stats(r, c)
    P.pooled(stats, 'golden pose cases')


@pytest.fixture(scope='module')
def synth_runs(device):
    runs = {}
    for name, make in P.SYNTH.items():
        tb, recs = make()
        runs[name] = {'tb': tb, 'recs': recs, 'got': to_numpy(tb.render(recs, device=device)),
                      'want': T.stack([tb.reference(r) for r in recs])}
    return runs


@pytest.mark.parametrize('name', sorted(P.SYNTH))
def test_beyond_the_goldens_against_the_cpu_reference(synth_runs, name):
    """PE: 128 x 128 / 512 x 512, B = 2, 32 persons with 17 visible joints, 576 blobs per image; PF: CULL_CAP + 40 persons
    piled over one tile of one hm_hp plane, next to an empty image; PG: 7 x 33, two class planes; PH: one radius-0 joint"""
    r = synth_runs[name]
    stats = P.check_batch(r['got'], r['want'], name)
    assert max(s[0] for s in stats) <= P.MAX_DIFF
    got = r['got']
    if name == 'PH':
        assert got['hm_hp'].sum() == 1.0 and got['hm_hp'][0, 4, 1, 5] == 1.0 and got['hm'][0, 0, 2, 3] == 1.0
        assert got['hp_ind'][0, 4] == 1 * 8 + 5 and got['hm_hp_mask'].sum() == 1.0
    if name == 'PF':
        assert not got['hm_hp'][1].any() and not got['hm'][1].any() and not got['pre_hm'][1].any()
        assert got['hm_hp'][0, 0].max() == 1.0
    if name == 'PE':
        assert (got['hm_hp_mask'] == 1).all() and (got['hm_hp'].reshape(2, P.J, -1).max(2) == 1).all()


def test_beyond_the_goldens_unequal_elements_pooled(synth_runs):
    stats = []
    for name, r in synth_runs.items():
        stats += P.check_batch(r['got'], r['want'], name)
    P.pooled(stats, 'cases PE-PH')


def _nan_arena(tb, B, device):
    """every output of a batch carved out of ONE NaN-filled block, 16 guard words between neighbours"""
    specs = tb.output_specs(B)
    words = 16
    place = {}
    for k, (shape, dt) in specs.items():
        n = int(np.prod(shape)) * (2 if dt == torch.int64 else 1)
        place[k] = (words, n)
        words += (n + 16 + 3) // 4 * 4
    arena = torch.full((words,), float('nan'), device=device)
    views = {}
    for k, (shape, dt) in specs.items():
        o, n = place[k]
        v = arena[o:o + n]
        views[k] = (v.view(torch.int64) if dt == torch.int64 else v).view(shape)
    return arena, views, place


def _others_still_nan(arena, place, asked):
    keep = torch.ones(arena.numel(), dtype=torch.bool)
    for k in asked:
        o, n = place[k]
        keep[o:o + n] = False
    assert int(keep.sum()) > 16
    return bool(torch.isnan(arena.cpu()[keep]).all())


@pytest.mark.parametrize('subset', sorted(P.OUT_SUBSETS) + ['all but a few'])
def test_caller_owned_outputs_are_overwritten_and_others_untouched(device, gold_runs, subset):
    r = gold_runs['P1']
    tb, recs = r['tb'], r['recs']
    arena, views, place = _nan_arena(tb, len(recs), device)
    if subset in P.OUT_SUBSETS:
        asked = {k: views[k] for k in P.OUT_SUBSETS[subset]}
    else:
        asked = {k: v for k, v in views.items() if k not in ('hm', 'hp_offset', 'joint', 'hps_mask')}
        assert 'hm_hp' in asked and 'pre_hm' in asked
    ret = tb.render(recs, out=asked)
    assert sorted(ret) == sorted(asked) and all(ret[k] is asked[k] for k in asked)
    torch.cuda.synchronize()
    for k in asked:
        assert views[k].cpu().numpy().tobytes() == r['batch'][k].tobytes(), k          # every element overwritten
    assert _others_still_nan(arena, place, asked)             # guards and the tensors not asked for


def test_bad_out_tensors_are_refused(device, gold_runs):
    from centertrack_amd._lib import CTError
    r = gold_runs['P1']
    tb, recs = r['tb'], r['recs']
    good = {k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in tb.output_specs(len(recs)).items()}
    with pytest.raises(CTError, match='out'):
        tb.render(recs, out={'hm_hp': good['hm_hp'][:1]})
    with pytest.raises(CTError, match='out'):
        tb.render(recs, out={'hp_ind': good['hp_ind'].view(len(recs), tb.max_objs, P.J)})       # the reference's shape only
    with pytest.raises(CTError, match='no output named'):
        tb.render(recs, out={'rotbin': good['hm']})
    with pytest.raises(CTError, match='names no tensor'):
        tb.render(recs, out={})


@pytest.mark.parametrize('name', ('P2', 'PE'))
def test_two_runs_on_garbage_are_bitwise_equal(device, gold_runs, synth_runs, name):
    r = gold_runs[name] if name in gold_runs else synth_runs[name]
    first = r['batch'] if name in gold_runs else r['got']
    garbage = {k: torch.full(shape, 7, dtype=dt, device=device) for k, (shape, dt) in
               r['tb'].output_specs(len(r['recs'])).items()}
    again = to_numpy(r['tb'].render(r['recs'], out=garbage))
    for k in first:
        assert again[k].tobytes() == first[k].tobytes(), k


def test_back_to_back_calls_without_synchronisation(device, gold_runs, synth_runs):
    """the staging ring: the second call packs while the first one's copy may still be in flight"""
    a, e = gold_runs['P1'], synth_runs['PE']
    tb_a, _ = P.builder(P.golden().cases['P1']['cfg'])        # a builder with a fresh ring
    half = len(a['recs']) // 2
    torch.cuda.synchronize()
    first = tb_a.render(a['recs'][:half], device=device)
    second = tb_a.render(a['recs'][half:], device=device)
    third = tb_a.render(a['recs'][:half], device=device)
    first, second, third = to_numpy(first), to_numpy(second), to_numpy(third)
    for k in a['batch']:
        assert first[k].tobytes() == a['batch'][k][:half].tobytes(), k
        assert second[k].tobytes() == a['batch'][k][half:].tobytes(), k
        assert third[k].tobytes() == first[k].tobytes(), k
    assert all(x['event'].query() for x in tb_a._ring)
    tb = e['tb']                                               # a large batch right behind a small one
    small = tb.render(e['recs'][:1], device=device)
    large = tb.render(e['recs'], device=device)
    small, large = to_numpy(small), to_numpy(large)
    for k in e['got']:
        assert small[k].tobytes() == e['got'][k][:1].tobytes() and large[k].tobytes() == e['got'][k].tobytes(), k


def test_inconsistent_records_are_rejected_before_any_launch(device, gold_runs):
    from centertrack_amd._lib import CTError
    r = gold_runs['P1']
    tb, recs = r['tb'], r['recs']
    out = {k: torch.full(shape, 3, dtype=dt, device=device) for k, (shape, dt) in tb.output_specs(len(recs)).items()}
    before = to_numpy(out)
    bad = [dict(x) for x in recs]
    bad[1]['counts'] = bad[1]['counts'] + np.array([0, 1, 0, 0], np.int32)
    with pytest.raises(CTError, match='record 1.*disagree'):
        tb.render(bad, out=out)
    i = next(j for j, x in enumerate(recs) if len(x['hm_blobs']) and len(x['rects']))
    bad = [dict(x) for x in recs]
    bad[i]['hm_blobs'] = bad[i]['hm_blobs'].copy()
    bad[i]['hm_blobs'][0, 0] = tb.num_classes + tb.num_joints          # a plane behind the last hm_hp plane
    with pytest.raises(CTError, match='plane 18 outside'):
        tb.render(bad, out=out)
    bad = [dict(x) for x in recs]
    bad[i]['rects'] = bad[i]['rects'].copy()
    bad[i]['rects'][0, 0] = -3
    with pytest.raises(CTError, match='rectangle 0: plane -3'):
        tb.render(bad, out=out)
    bad = [dict(x) for x in recs]
    bad[i]['slot_k'] = np.full_like(bad[i]['slot_k'], tb.max_objs)
    with pytest.raises(CTError, match='slot indices'):
        tb.render(bad, out=out)
    with pytest.raises(CTError, match='empty batch'):
        tb.render([], device=device)
    after = to_numpy(out)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)      # nothing was written


def test_rendered_batch_plugs_into_generic_loss(device, gold_runs):
    """GenericLoss(opt)(outputs, tb.render(...)) on random logits for P1 (hm, hm_hp, hps, hp_offset, reg, wh, tracking):
    the same losses, bit for bit, as with the reference's batch uploaded with .to(device) wherever the targets are
    bitwise equal (the slot tensors always are; a heat map when the device exp rounded every element like libm)"""
    from centertrack_amd.losses import GenericLoss
    r = gold_runs['P1']
    tb, opt, recs = r['tb'], r['opt'], r['recs']
    assert sorted(opt.heads) == sorted(('hm', 'hm_hp', 'hps', 'hp_offset', 'reg', 'wh', 'tracking'))
    B = len(recs)
    g = torch.Generator().manual_seed(5)
    ch = {'hm': tb.num_classes, 'hm_hp': P.J, 'hps': 2 * P.J, 'hp_offset': 2, 'reg': 2, 'wh': 2, 'tracking': 2}
    outputs = {h: torch.randn(B, ch[h], opt.output_h, opt.output_w, generator=g).to(device) for h in opt.heads}
    batch = tb.render(recs, device=device)
    want = {k: torch.from_numpy(v).to(device) for k, v in r['want'].items()}
    crit = GenericLoss(opt)
    tot, stats = crit([outputs], batch)
    tot_ref, stats_ref = crit([outputs], want)
    torch.cuda.synchronize()
    assert np.isfinite(float(tot)) and float(tot) > 0
    equal = {h: torch.equal(batch[h], want[h]) for h in ('hm', 'hm_hp')}
    print('P1: rendered hm %s, hm_hp %s the golden bit for bit' % tuple(
        'equals' if equal[h] else 'differs from' for h in ('hm', 'hm_hp')))
    for h in opt.heads:
        assert np.isfinite(float(stats[h])), h
        if equal.get(h, True):
            assert float(stats[h]) == float(stats_ref[h]), h
    if all(equal.values()):
        assert float(tot) == float(tot_ref)
