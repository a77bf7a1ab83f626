"""GPU: ``TargetBuilder.render`` / ct_build_targets (csrc/targets.hip) against the reference's own
``ret`` (tests/golden/targets.npz) and, beyond the goldens, against ``TargetBuilder.reference`` -- which
test_targets_cpu.py holds to the goldens exactly.

Slot tensors must be equal bit for bit.  The maps are held to the bound ct_render_pre_hm's test uses for float64 ``exp``
on the device against libm (test_hip_ops.py): max |diff| <= 1e-6 and fewer than 1e-4 of all map elements of all cases
taken together unequal.  The smallest value a Gaussian takes on its support is e^-9 = 1.2e-4, so any geometric error
exceeds 1e-6 by two orders; the sets {map > 0} and {map == 1} must be identical."""
import numpy as np
import pytest
import torch

import _targets as T

pytestmark = pytest.mark.gpu

MAP_KEYS = ('hm', 'pre_hm')
MAX_DIFF, MAX_UNEQUAL = 1e-6, 1e-4


def to_numpy(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_batch(got, want, what):
    """keys, dtypes, shapes; slot tensors bitwise; per map (max |diff|, unequal, elements) after the set checks"""
    assert sorted(got) == sorted(want), what
    stats = []
    for k in want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if k in MAP_KEYS:
            assert np.isfinite(g).all(), (what, k)
            assert ((g > 0) == (w > 0)).all(), (what, k, 'support differs')
            assert ((g == 1) == (w == 1)).all(), (what, k, 'peaks / ignore regions differ')
            stats.append((float(np.abs(g - w).max()), int((g != w).sum()), g.size))
        else:
            assert g.tobytes() == w.tobytes(), (what, k)
    return stats


def pooled(stats, what):
    worst = max(s[0] for s in stats)
    unequal, total = sum(s[1] for s in stats), sum(s[2] for s in stats)
    print('%s: largest map difference %.3g, %d unequal of %d map elements' % (what, worst, unequal, total))
    assert total > 100000, total              # the cap below is never vacuous
    assert worst <= MAX_DIFF
    assert unequal < MAX_UNEQUAL * total
    return worst, unequal, total


@pytest.fixture(scope='module')
def gold():
    return T.golden()


@pytest.fixture(scope='module')
def gold_runs(device, gold):
    """every golden case rendered once: all samples as one batch (case A: the empty sample in the middle) and each
    sample alone"""
    runs = {}
    for c in T.CASES:
        case = gold.cases[c]
        tb, opt = T.builder(case['cfg'])
        recs = [gold.encode(tb, s) for s in case['samples']]
        batch = to_numpy(tb.render(recs, device=device))
        singles = [to_numpy(tb.render([r], device=device)) for r in recs]
        runs[c] = {'tb': tb, 'opt': opt, 'recs': recs, 'batch': batch, 'singles': singles,
                   'want': T.stack([s['ret'] for s in case['samples']])}
    return runs


@pytest.mark.parametrize('case', T.CASES)
def test_golden_case_slots_bitwise_and_map_geometry(gold, gold_runs, case):
    r = gold_runs[case]
    if case == 'A':
        e = gold.cases['A']['empty']
        assert 0 < e < len(r['recs']) - 1 and r['recs'][e]['counts'].tolist() == [0, 0, 0, 0]
    stats = check_batch(r['batch'], r['want'], case + ' batch')
    for i, one in enumerate(r['singles']):
        stats += check_batch(one, {k: v[i:i + 1] for k, v in r['want'].items()}, '%s sample %d' % (case, i))
    assert max(s[0] for s in stats) <= MAX_DIFF
    assert r['batch']['ind'].dtype == np.int64 and r['batch']['cat'].dtype == np.int64
    if case == 'B':
        assert r['batch']['rotbin'].dtype == np.int64 and r['batch']['rotbin'].shape[2] == 2
    if case == 'C':
        assert not [k for k in r['batch'] if k.startswith('pre_')]


def test_golden_maps_within_the_device_exp_bound_all_cases_together(gold_runs):
    stats = []
    for c, r in gold_runs.items():
        stats += check_batch(r['batch'], r['want'], c)
        for i, one in enumerate(r['singles']):
            stats += check_batch(one, {k: v[i:i + 1] for k, v in r['want'].items()}, c)
    pooled(stats, 'golden cases')


@pytest.fixture(scope='module')
def synth_runs(device):
    runs = {}
    for name, make in T.SYNTH.items():
        tb, recs = make()
        runs[name] = {'tb': tb, 'recs': recs, 'got': to_numpy(tb.render(recs, device=device)),
                      'want': T.stack([tb.reference(r) for r in recs])}
    return runs


@pytest.mark.parametrize('name', sorted(T.SYNTH))
def test_beyond_the_goldens_against_the_cpu_reference(synth_runs, name):
    """E: 128 x 128 / 512 x 512, B = 2, C = 80, 128 objects each; F: more than 2 CULL_CAP pre_hm blobs, CULL_CAP + 1 over one
    tile, next to an empty image; G: 7 x 33 / 28 x 132; H: B = 1, C = 1, one radius-0 object"""
    r = synth_runs[name]
    stats = check_batch(r['got'], r['want'], name)
    assert max(s[0] for s in stats) <= MAX_DIFF
    if name == 'H':
        hm = r['got']['hm']
        assert hm.sum() == 1.0 and hm[0, 0, 2, 3] == 1.0
    if name == 'F':
        assert not r['got']['pre_hm'][1].any() and not r['got']['hm'][1].any()
        assert r['got']['pre_hm'][0].max() == 1.0


def test_beyond_the_goldens_unequal_elements_pooled(synth_runs):
    stats = []
    for name, r in synth_runs.items():
        stats += check_batch(r['got'], r['want'], name)
    pooled(stats, 'cases E-H')


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


def test_caller_owned_outputs_are_overwritten_and_others_untouched(device, gold_runs):
    r = gold_runs['B']
    tb, recs = r['tb'], r['recs']
    arena, views, place = _nan_arena(tb, len(recs), device)
    skipped = ('wh', 'pre_hm', 'rotbin', 'dep_mask')
    asked = {k: v for k, v in views.items() if k not in skipped}
    ret = tb.render(recs, out=asked)
    assert sorted(ret) == sorted(asked) and all(ret[k] is asked[k] for k in asked)
    torch.cuda.synchronize()
    for k in asked:
        assert views[k].cpu().numpy().tobytes() == r['batch'][k].tobytes(), k          # every element overwritten
    keep = torch.ones(arena.numel(), dtype=torch.bool)
    for k in asked:
        o, n = place[k]
        keep[o:o + n] = False
    assert torch.isnan(arena.cpu()[keep]).all()               # guards and the tensors not asked for
    assert int(keep.sum()) > sum(place[k][1] for k in skipped)
    # maps alone / slots alone
    only = tb.render(recs, out={'pre_hm': views['pre_hm']})
    assert list(only) == ['pre_hm']
    torch.cuda.synchronize()
    assert views['pre_hm'].cpu().numpy().tobytes() == r['batch']['pre_hm'].tobytes()
    assert torch.isnan(views['wh']).all()
    from centertrack_amd._lib import CTError
    with pytest.raises(CTError, match='out'):
        tb.render(recs, out={'hm': views['hm'][:1]})
    with pytest.raises(CTError, match='no output named'):
        tb.render(recs, out={'hps': views['hm']})


def test_back_to_back_calls_without_synchronisation(device, gold_runs, synth_runs):
    """the staging ring: the second call packs while the first one's copy may still be in flight"""
    a, e = gold_runs['A'], synth_runs['E']
    tb_a, _ = T.builder(T.golden().cases['A']['cfg'])         # a builder with a fresh ring
    half = len(a['recs']) // 2
    torch.cuda.synchronize()
    first = tb_a.render(a['recs'][:half], device=device)
    second = tb_a.render(a['recs'][half:], device=device)     # whether it reuses the block depends on how fast the copy was
    third = tb_a.render(a['recs'][:half], device=device)
    first, second, third = to_numpy(first), to_numpy(second), to_numpy(third)
    for k in a['batch']:
        assert first[k].tobytes() == a['batch'][k][:half].tobytes(), k
        assert second[k].tobytes() == a['batch'][k][half:].tobytes(), k
        assert third[k].tobytes() == first[k].tobytes(), k
    assert all(x['event'].query() for x in tb_a._ring)
    # a large batch right behind a small one on the same builder
    tb = e['tb']
    small = tb.render(e['recs'][:1], device=device)
    large = tb.render(e['recs'], device=device)
    small, large = to_numpy(small), to_numpy(large)
    for k in e['got']:
        assert small[k].tobytes() == e['got'][k][:1].tobytes() and large[k].tobytes() == e['got'][k].tobytes(), k


def test_staging_of_a_call_in_flight_is_not_reused(device, gold_runs):
    """the ring, without a race: the first call's event is made to answer "not finished", so the second call must take a
    new pinned block and leave the first one's contents alone; once it answers "finished" the block is taken again"""
    a = gold_runs['A']
    tb, _ = T.builder(T.golden().cases['A']['cfg'])
    tb.render(a['recs'][:2], device=device)
    assert len(tb._ring) == 1
    entry = tb._ring[0]
    torch.cuda.synchronize()

    class Pending(object):
        def __init__(self, event):
            self.event, self.pending = event, True

        def query(self):
            return not self.pending and self.event.query()

        def record(self):
            self.event.record()

    entry['event'] = fake = Pending(entry['event'])
    snap = entry['host'].clone()
    got = to_numpy(tb.render(a['recs'][2:5], device=device))
    assert len(tb._ring) == 2 and tb._ring[0] is entry and torch.equal(entry['host'], snap)
    for k in a['batch']:
        assert got[k].tobytes() == a['batch'][k][2:5].tobytes(), k
    fake.pending = False
    got = to_numpy(tb.render(a['recs'][5:], device=device))
    assert len(tb._ring) == 2 and not torch.equal(entry['host'], snap)       # the idle block was taken again
    for k in a['batch']:
        assert got[k].tobytes() == a['batch'][k][5:].tobytes(), k


@pytest.mark.parametrize('name', ('B', 'E'))
def test_two_runs_are_bitwise_equal(device, gold_runs, synth_runs, name):
    r = gold_runs[name] if name in gold_runs else synth_runs[name]
    first = r['batch'] if name in gold_runs else r['got']
    garbage = {k: torch.full(shape, 7, dtype=dt, device=device) for k, (shape, dt) in
               r['tb'].output_specs(len(r['recs'])).items()}
    again = to_numpy(r['tb'].render(r['recs'], out=garbage))
    for k in first:
        assert again[k].tobytes() == first[k].tobytes(), k


def test_inconsistent_records_are_rejected_before_any_launch(device, gold_runs):
    from centertrack_amd._lib import CTError
    r = gold_runs['A']
    tb, recs = r['tb'], r['recs']
    out = {k: torch.full(shape, 3, dtype=dt, device=device) for k, (shape, dt) in tb.output_specs(len(recs)).items()}
    before = to_numpy(out)
    bad = [dict(x) for x in recs]
    bad[1]['counts'] = bad[1]['counts'] + np.array([0, 1, 0, 0], np.int32)
    with pytest.raises(CTError, match='record 1.*disagree'):
        tb.render(bad, out=out)
    i = next(j for j, x in enumerate(recs) if len(x['hm_blobs']))
    bad = [dict(x) for x in recs]
    bad[i]['hm_blobs'] = bad[i]['hm_blobs'].copy()
    bad[i]['hm_blobs'][0, 0] = tb.num_classes                 # a plane outside [0, C): refused by ct_build_targets itself
    with pytest.raises(CTError, match='plane'):
        tb.render(bad, out=out)
    bad = [dict(x) for x in recs]
    bad[i]['slot_k'] = np.full_like(bad[i]['slot_k'], tb.max_objs)
    with pytest.raises(CTError, match='slot indices'):
        tb.render(bad, out=out)
    with pytest.raises(CTError, match='empty batch'):
        tb.render([], device=device)
    after = to_numpy(out)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)      # nothing was written


@pytest.mark.parametrize('case', ('A', 'B'))
def test_rendered_batch_plugs_into_generic_loss(device, gold_runs, case):
    """GenericLoss(opt)(outputs, tb.render(...)) on random logits, no conversion in between; the same losses, bit for
    bit, as with the reference's batch uploaded with .to(device) wherever the targets are bitwise equal (the slot tensors
    always are; the heat map when the device exp rounded every element like libm)"""
    from centertrack_amd import _lib
    from centertrack_amd.losses import GenericLoss
    r = gold_runs[case]
    tb, opt, recs = r['tb'], r['opt'], r['recs']
    B = len(recs)
    g = torch.Generator().manual_seed(5)
    ch = dict(_lib.HEAD_CH, hm=tb.num_classes)
    outputs = {h: torch.randn(B, ch[h], opt.output_h, opt.output_w, generator=g).to(device) for h in opt.heads}
    batch = tb.render(recs, device=device)
    want = {k: torch.from_numpy(v).to(device) for k, v in r['want'].items()}
    crit = GenericLoss(opt)
    tot, stats = crit([outputs], batch)
    tot_ref, stats_ref = crit([outputs], want)
    torch.cuda.synchronize()
    assert np.isfinite(float(tot)) and float(tot) > 0
    hm_equal = torch.equal(batch['hm'], want['hm'])
    print('case %s: rendered hm %s the golden bit for bit' % (case, 'equals' if hm_equal else 'differs from'))
    for h in opt.heads:
        if h != 'hm' or hm_equal:
            assert float(stats[h]) == float(stats_ref[h]), h
    if hm_equal:
        assert float(tot) == float(tot_ref)
