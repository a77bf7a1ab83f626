"""GPU: ``InputBuilder.render`` / ct_build_inputs (csrc/inputs.hip) against the reference's own images
(tests/golden/inputs.npz) and, beyond the goldens, against ``InputBuilder.reference`` -- which test_inputs_cpu.py holds to
the goldens bit for bit.

* ``warped`` (the u8 image after the warp) equals ``oracle.image.warp_affine_u8`` of the flipped frame exactly.
* Outputs without colour augmentation are bit-identical to ``reference``.
* ``gs_mean`` lies within 2^-23 |mean| of the float64 mean of the float32 grey image.
* Outputs with colour augmentation: |diff| <= 4 max(e32, 2^-23) max|reference| per image, e32 being ``reference``'s own
  relative error against a float64 evaluation of the same chain on that image (computed here, on the CPU).  Only the
  order in which gs_mean is summed may differ from the host."""
import numpy as np
import pytest
import torch

import _inputs as I
from oracle.image import warp_affine_u8

pytestmark = pytest.mark.gpu


def to_numpy(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_render(ib, samples, frames, got, what):
    """every image of a rendered batch (``debug=True``) against the CPU; -> [(what, e32, largest difference, bound)]"""
    B = len(samples)
    has_pre = any(p is not None for _, p in samples)
    assert sorted(got) == sorted(['image', 'warped', 'gs_mean'] + (['pre_img'] if has_pre else [])), what
    N = B * (2 if has_pre else 1)
    assert got['image'].shape == (B, 3, ib.H, ib.W) and got['image'].dtype == np.float32
    assert got['warped'].shape == (N, ib.H, ib.W, 3) and got['warped'].dtype == np.uint8
    assert got['gs_mean'].shape == (N,) and got['gs_mean'].dtype == np.float32
    stats = []
    for n in range(N):
        b, slot = n % B, n // B
        rec, frame = samples[b][slot], frames[b][slot]
        out = got['pre_img' if slot else 'image'][b]
        tag = '%s sample %d %s' % (what, b, 'pre_img' if slot else 'image')
        assert np.isfinite(out).all(), tag
        if rec is None:                                        # a sample without pre_img in a batch that has some: zeros
            assert not out.any() and not got['warped'][n].any() and got['gs_mean'][n] == 0, tag
            continue
        want_u8 = warp_affine_u8(frame[:, ::-1] if rec['flipped'] else frame, rec['trans'], ib.W, ib.H)
        assert got['warped'][n].tobytes() == want_u8.tobytes(), tag + ': warp'
        mean64 = I.grey_mean64(want_u8)
        assert abs(float(got['gs_mean'][n]) - mean64) <= 2.0 ** -23 * abs(mean64), (tag, float(got['gs_mean'][n]), mean64)
        ref = ib.reference(rec)
        if rec['color'] is None:
            assert out.tobytes() == ref.tobytes(), tag + ': not bit-identical without colour augmentation'
            continue
        e32, bound = I.colour_bound(ib, rec)
        diff = float(np.abs(out.astype(np.float64) - ref.astype(np.float64)).max())
        print('%s: e32 %.3g, largest difference %.3g, bound %.3g' % (tag, e32, diff, bound))
        stats.append((tag, e32, diff, bound))
        assert diff <= bound, (tag, e32, diff, bound)
    return stats


@pytest.fixture(scope='module')
def gold():
    return I.golden()


@pytest.fixture(scope='module')
def gold_runs(device, gold):
    """every golden case rendered once as one batch and each sample alone"""
    runs = {}
    for c in I.CASES:
        case = gold.cases[c]
        ib = gold.builder(case['cfg'])
        samples = [gold.encode(ib, s) for s in case['samples']]
        frames = [(I.source(s['seed'], s['h'], s['w']),
                   I.source(s['pre_seed'], s['h'], s['w']) if s['pre_img'] is not None else None) for s in case['samples']]
        batch = to_numpy(ib.render(samples, debug=True, device=device))
        singles = [to_numpy(ib.render([s], debug=True, device=device)) for s in samples]
        runs[c] = {'ib': ib, 'samples': samples, 'frames': frames, 'batch': batch, 'singles': singles}
    return runs


@pytest.fixture(scope='module')
def synth_runs(device):
    runs = {}
    for name, make in I.SYNTH.items():
        ib, samples, frames = make()
        runs[name] = {'ib': ib, 'samples': samples, 'frames': frames,
                      'batch': to_numpy(ib.render(samples, debug=True, device=device))}
    return runs


def test_the_cases_reach_every_regime_of_the_kernels(gold_runs, synth_runs):
    K = I.kernel_constants()
    runs = dict(gold_runs, **synth_runs)
    for name, pred in I.regimes(K).items():
        assert [c for c, r in runs.items() if pred(r['ib'], r['samples'])], 'no case reaches: ' + name


@pytest.mark.parametrize('case', I.CASES)
def test_golden_case_as_one_batch_and_sample_by_sample(gold, gold_runs, case):
    r = gold_runs[case]
    check_render(r['ib'], r['samples'], r['frames'], r['batch'], case + ' batch')
    for i, one in enumerate(r['singles']):
        check_render(r['ib'], r['samples'][i:i + 1], r['frames'][i:i + 1], one, '%s alone %d' % (case, i))
        # an image does not depend on what else is in the batch
        assert one['image'].tobytes() == r['batch']['image'][i:i + 1].tobytes(), (case, i)
        if 'pre_img' in one:
            assert one['pre_img'].tobytes() == r['batch']['pre_img'][i:i + 1].tobytes(), (case, i)
    # and against the reference's own arrays: colour off bit for bit, colour on within the same bound
    for i, s in enumerate(gold.cases[case]['samples']):
        for key, slot in (('image', 0), ('pre_img', 1)):
            if s[key] is None:
                continue
            rec, got = r['samples'][i][slot], r['batch'][key][i]
            if rec['color'] is None:
                assert got.tobytes() == s[key].tobytes(), (case, i, key)
            else:
                assert float(np.abs(got - s[key]).max()) <= I.colour_bound(r['ib'], rec)[1], (case, i, key)


@pytest.mark.parametrize('name', sorted(I.SYNTH))
def test_beyond_the_goldens_against_the_cpu_reference(synth_runs, name):
    """E: 270 x 480 -> 128 x 192, B = 2 with pre_img; F: B = 3, three source sizes, a padded source, a missing pre_img, a
    record without colour; G: output 7 x 33; H: 1 x 1 and 2 x 2 sources; I: a tall source, most rows not uploaded; K: more
    than 64 partials"""
    r = synth_runs[name]
    check_render(r['ib'], r['samples'], r['frames'], r['batch'], name)
    if name == 'F':
        assert not r['batch']['pre_img'][1].any() and r['batch']['pre_img'][0].any()
    if name == 'I':
        rec = r['samples'][0][0]
        assert rec['rows'].shape[0] < rec['h'] // 2


def test_a_device_resident_source_is_used_in_place(device, synth_runs):
    """case J: the frames of case F's first sample already on the device -- one dense, one with a row pitch above 3 w --
    give the bits of the uploaded records"""
    r = synth_runs['F']
    ib = r['ib']
    (img, pre), (frame, pre_frame) = r['samples'][0], r['frames'][0]
    dev_frame = torch.from_numpy(frame).to(device)
    padded = torch.full((pre_frame.shape[0], pre_frame.shape[1] + 5, 3), 255, dtype=torch.uint8, device=device)
    padded[:, :pre_frame.shape[1]] = torch.from_numpy(pre_frame).to(device)
    dev_img = ib.encode(dev_frame, img['trans'], img['flipped'], img['color'])
    dev_pre = ib.encode(padded[:, :pre_frame.shape[1]], pre['trans'], pre['flipped'], pre['color'])
    assert dev_img['rows'].is_cuda and dev_img['rows'].data_ptr() == dev_frame[dev_img['row0']:].data_ptr()
    assert dev_pre['rows'].stride(0) == 3 * (pre_frame.shape[1] + 5)
    ring = len(ib._ring)
    got = to_numpy(ib.render([(dev_img, dev_pre)], debug=True))
    assert len(ib._ring) == ring                       # descriptors only: the idle block was enough
    for k in ('image', 'pre_img'):
        assert got[k].tobytes() == r['batch'][k][:1].tobytes(), k
    assert got['warped'][0].tobytes() == r['batch']['warped'][0].tobytes()
    assert got['warped'][1].tobytes() == r['batch']['warped'][3].tobytes()
    mixed = to_numpy(ib.render([(dev_img, pre), r['samples'][2]]))
    assert mixed['image'][0].tobytes() == r['batch']['image'][0].tobytes()
    assert mixed['pre_img'].tobytes() == r['batch']['pre_img'][[0, 2]].tobytes()


def _nan_arena(ib, B, device, keys):
    """the outputs of a batch carved out of ONE NaN-filled block, 16 guard words between neighbours"""
    n = B * 3 * ib.H * ib.W
    arena = torch.full((16 + len(keys) * (n + 16 + 3) // 4 * 4 + 16,), float('nan'), device=device)
    views, place, o = {}, {}, 16
    for k in keys:
        views[k], place[k] = arena[o:o + n].view(B, 3, ib.H, ib.W), (o, n)
        o += (n + 16 + 3) // 4 * 4
    return arena, views, place


def test_caller_owned_outputs_are_overwritten_and_nothing_else(device, synth_runs):
    for name in ('E', 'G', 'F'):                       # exact tiles; partial tiles both ways; a zero pre_img
        r = synth_runs[name]
        ib, samples = r['ib'], r['samples']
        arena, views, place = _nan_arena(ib, len(samples), device, ('image', 'pre_img'))
        ret = ib.render(samples, out=views)
        assert sorted(ret) == ['image', 'pre_img'] and all(ret[k] is views[k] for k in views)
        torch.cuda.synchronize()
        keep = torch.ones(arena.numel(), dtype=torch.bool)
        for k in views:
            assert views[k].cpu().numpy().tobytes() == r['batch'][k].tobytes(), (name, k)      # every element overwritten
            o, n = place[k]
            keep[o:o + n] = False
        assert int(keep.sum()) >= 48 and torch.isnan(arena.cpu()[keep]).all(), name           # the guards
    from centertrack_amd._lib import CTError
    r = synth_runs['E']
    _, views, _ = _nan_arena(r['ib'], 2, device, ('image', 'pre_img'))
    with pytest.raises(CTError, match='out must name exactly'):
        r['ib'].render(r['samples'], out={'image': views['image']})
    with pytest.raises(CTError, match=r"out\['pre_img'\]"):
        r['ib'].render(r['samples'], out={'image': views['image'], 'pre_img': views['pre_img'][:1]})
    with pytest.raises(CTError, match=r"out\['image'\]"):
        r['ib'].render(r['samples'], out={'image': views['image'].double(), 'pre_img': views['pre_img']})
    assert torch.isnan(views['image']).all() and torch.isnan(views['pre_img']).all()


def test_back_to_back_calls_without_synchronisation(device, gold_runs, synth_runs):
    """the staging ring: the second call packs while the first one's copy may still be in flight"""
    a, e = gold_runs['A'], synth_runs['E']
    ib = I.golden().builder(I.golden().cases['A']['cfg'])       # a builder with a fresh ring
    torch.cuda.synchronize()
    first = ib.render(a['samples'][:3], device=device)
    second = ib.render(a['samples'][3:], device=device)
    third = ib.render(a['samples'][:3], device=device)
    first, second, third = to_numpy(first), to_numpy(second), to_numpy(third)
    for k in ('image', 'pre_img'):
        assert first[k].tobytes() == a['batch'][k][:3].tobytes(), k
        assert second[k].tobytes() == a['batch'][k][3:].tobytes(), k
        assert third[k].tobytes() == first[k].tobytes(), k
    assert all(x['event'].query() for x in ib._ring)
    small = e['ib'].render(e['samples'][:1], device=device)     # a large batch right behind a small one
    large = e['ib'].render(e['samples'], device=device)
    small, large = to_numpy(small), to_numpy(large)
    for k in ('image', 'pre_img'):
        assert small[k].tobytes() == e['batch'][k][:1].tobytes() and large[k].tobytes() == e['batch'][k].tobytes(), k


def test_staging_of_a_call_in_flight_is_not_reused(device, gold_runs):
    """the ring, without a race: the first call's event is made to answer "not finished", so the second call must take a
    new pinned block and leave the first one's contents alone; once it answers "finished" the block is taken again"""
    a = gold_runs['A']
    ib = I.golden().builder(I.golden().cases['A']['cfg'])
    ib.render(a['samples'][:2], device=device)
    assert len(ib._ring) == 1
    entry = ib._ring[0]
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
    got = to_numpy(ib.render(a['samples'][2:4], device=device))
    assert len(ib._ring) == 2 and ib._ring[0] is entry and torch.equal(entry['host'], snap)
    for k in ('image', 'pre_img'):
        assert got[k].tobytes() == a['batch'][k][2:4].tobytes(), k
    fake.pending = False
    got = to_numpy(ib.render(a['samples'][4:], device=device))
    assert len(ib._ring) == 2 and not torch.equal(entry['host'], snap)       # the idle block was taken again
    for k in ('image', 'pre_img'):
        assert got[k].tobytes() == a['batch'][k][4:].tobytes(), k


@pytest.mark.parametrize('name', ('A', 'E', 'K'))
def test_two_runs_are_bitwise_equal(device, gold_runs, synth_runs, name):
    r = gold_runs[name] if name in gold_runs else synth_runs[name]
    ib = r['ib']
    garbage = {k: torch.full(shape, 7.0, device=device) for k, shape in
               ib.output_specs(len(r['samples']), 'pre_img' in r['batch']).items()}
    again = to_numpy(ib.render(r['samples'], out=garbage, debug=True))
    for k in r['batch']:
        assert again[k].tobytes() == r['batch'][k].tobytes(), k


def test_rejected_records_leave_the_outputs_untouched(device, synth_runs):
    from centertrack_amd import _lib, ops
    from centertrack_amd._lib import CTError
    r = synth_runs['G']
    ib, samples = r['ib'], r['samples']
    out = {k: torch.full(shape, 3.0, device=device) for k, shape in ib.output_specs(len(samples)).items()}
    good = samples[0][0]
    bad = [(dict(good, rows=good['rows'][1:]), samples[0][1]), samples[1]]        # one row short at the old origin
    with pytest.raises(CTError, match='sample 0 image.*disagrees with its matrix'):
        ib.render(bad, out=out)
    bad = [samples[0], (samples[1][0], dict(samples[1][1], w=samples[1][1]['w'] + 1))]
    with pytest.raises(CTError, match='sample 1 pre_img.*disagree with the frame'):
        ib.render(bad, out=out)
    bad = [(dict(good, color=dict(good['color'], order=np.array([1, 1, 2]))), samples[0][1]), samples[1]]
    with pytest.raises(CTError, match='permutation'):
        ib.render(bad, out=out)
    # a buffer ct_build_inputs itself refuses: real tensors, a descriptor of an unknown kind
    N, words = 4, 4 * _lib.CT_INPUTS_DESC_WORDS
    host = torch.zeros(words, dtype=torch.int32).pin_memory()
    host[0] = 7
    dev = torch.empty(words, dtype=torch.int32, device=device)
    warped = torch.empty((N, ib.H, ib.W), dtype=torch.int32, device=device)
    partials = torch.empty(N, dtype=torch.float64, device=device)
    with pytest.raises(CTError, match='kind 7'):
        ops.build_inputs(host, dev, words * 4, 2, N, ib.H, ib.W, ib.mean, ib.std, out['image'], out['pre_img'], warped,
                         partials)
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in out.values())                      # nothing was written


def test_rendered_images_and_targets_feed_a_training_forward(device):
    """``InputBuilder.render`` + ``TargetBuilder.render`` of golden case A of the targets (96 x 160 input, 24 x 40 output,
    tracking with pre_hm) -> ``DLASeg`` -> ``GenericLoss``, no conversion in between: a finite loss"""
    from collections import OrderedDict
    import _targets as T
    from centertrack_amd import _lib, dcn_v2
    from centertrack_amd.dla_seg import DLASeg
    from centertrack_amd.losses import GenericLoss
    from test_dlaseg_cpu import Opt
    tgold = T.golden()
    case = tgold.cases['A']
    tb, opt = T.builder(case['cfg'])
    picked = [s for i, s in enumerate(case['samples']) if i != case['empty']][:2]
    ib = I.builder((opt.input_h, opt.input_w))
    samples = []
    for i, s in enumerate(picked):
        frame, pre_frame = I.source(900 + i, s['height'], s['width']), I.source(950 + i, s['height'], s['width'])
        samples.append((ib.encode(frame, s['trans'][0], bool(i % 2), I.draw(ib, 900 + i)),
                        ib.encode(pre_frame, s['trans'][2], bool(i % 2), I.draw(ib, 950 + i))))
    images = ib.render(samples, device=device)
    batch = tb.render([tgold.encode(tb, s) for s in picked], device=device)
    assert images['image'].shape == (2, 3, opt.input_h, opt.input_w) and batch['pre_hm'].shape == (2, 1, opt.input_h, opt.input_w)
    heads = OrderedDict((h, dict(_lib.HEAD_CH, hm=tb.num_classes)[h]) for h in opt.heads)
    torch.manual_seed(3)
    model = DLASeg(34, heads, {h: [256] for h in heads}, Opt()).to(device).train()
    with dcn_v2.trainable():
        outputs = model(images['image'], images['pre_img'], batch['pre_hm'])
        tot, stats = GenericLoss(opt)(outputs, batch)
    torch.cuda.synchronize()
    tot = float(tot.detach())
    assert np.isfinite(tot) and tot > 0
    assert all(np.isfinite(float(v.detach())) for v in stats.values())
