"""CPU: ``centertrack_amd.targets.TargetBuilder`` on the host.  ``reference(encode(...))`` on the
inputs the golden generator recorded from the reference's own ``GenericDataset.__getitem__`` equals the ``ret`` it
returned EXACTLY -- both sides are numpy, so the bound is 0 -- and the GPU shapes of test_hip_targets.py are held against
the constants of csrc/targets.hip.  Nothing here touches a device."""
import pickle

import numpy as np
import pytest

import _targets as T


@pytest.fixture(scope='module')
def gold():
    return T.golden()


@pytest.mark.parametrize('case', T.CASES)
def test_reference_of_encode_equals_the_golden_ret_exactly(gold, case):
    c = gold.cases[case]
    tb, _ = T.builder(c['cfg'])
    assert len(c['samples']) >= 2
    for i, s in enumerate(c['samples']):
        got = tb.reference(gold.encode(tb, s))
        want = s['ret']
        assert sorted(got) == sorted(want), (case, i)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case, i, k)
            assert got[k].tobytes() == want[k].tobytes(), (case, i, k, np.abs(got[k] - want[k]).max())


def test_golden_holds_the_situations_the_cases_are_there_for(gold):
    a = gold.cases['A']
    tb, opt = T.builder(a['cfg'])
    recs = [gold.encode(tb, s) for s in a['samples']]
    blobs = np.concatenate([r['pre_blobs'] for r in recs])
    assert blobs[:, 0].min() < 0 and blobs[:, 0].max() >= opt.input_w        # left, right
    assert blobs[:, 1].min() < 0 and blobs[:, 1].max() >= opt.input_h        # top, bottom
    assert (blobs[:, 3] == 0).any() and (blobs[:, 3] == 1).any()
    e = recs[a['empty']]
    assert e['counts'].tolist() == [0, 0, 0, 0] and 0 < a['empty'] < len(recs) - 1
    assert any(len(r['slot_k']) and r['slot_k'].max() + 1 > len(r['slot_k']) for r in recs)      # holes
    rects = np.concatenate([r['rects'] for r in recs])
    assert (rects[:, 0] == -1).any() and (rects[:, 0] >= 0).any()
    assert not [k for k in gold.cases['C']['samples'][0]['ret'] if k.startswith('pre_')]
    d = gold.cases['D']
    tbd, optd = T.builder(d['cfg'])
    recd = [gold.encode(tbd, s) for s in d['samples']]
    hb = np.concatenate([r['hm_blobs'] for r in recd])
    assert (hb[:, 3] == 0).any()
    assert [0, 0] in hb[:, 1:3].tolist() and [optd.output_w - 1, optd.output_h - 1] in hb[:, 1:3].tolist()
    b = gold.cases['B']
    assert all(abs(s['aug_s'] - 1) > 1e-6 for s in b['samples'])
    rb = T.stack([s['ret'] for s in b['samples']])
    for k in ('dep_mask', 'rot_mask', 'amodel_offset_mask', 'velocity_mask', 'nuscenes_att_mask'):
        on = rb[k].reshape(rb[k].shape[0], rb[k].shape[1], -1)[..., 0][rb['mask'] > 0]
        assert (on == 0).any() and ((on == 1).any() or k == 'nuscenes_att_mask'), k


@pytest.mark.parametrize('case', ('A', 'B'))
def test_encode_consumes_a_random_stream_in_the_recorded_order(gold, case):
    c = gold.cases[case]
    tb, _ = T.builder(c['cfg'])
    drew = 0
    for s in c['samples']:
        key, pos, gauss, nxt = s['rng']
        rs = np.random.RandomState()
        rs.set_state(('MT19937', key, pos, int(gauss[0]), float(gauss[1])))
        a, b = gold.encode(tb, s, rng=rs), gold.encode(tb, s)
        for k in b:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert rs.random_sample() == nxt                     # exactly as many numbers taken as the reference took
        n = s['noise']
        drew += int((~np.isnan(n)).sum())
        # the last two numbers are drawn only where fp fired
        fired = n[:, 3] < c['cfg']['disturb'][2]
        assert (np.isnan(n[:, 4]) == ~fired).all()
    assert drew > 0


def test_without_noise_nothing_is_disturbed(gold):
    s = gold.cases['A']['samples'][0]
    tb, _ = T.builder(gold.cases['A']['cfg'])
    t = s['trans']
    rec = tb.encode(s['anns'], t[1], s['height'], s['width'], pre_anns=s['pre_anns'], trans_input_pre=t[2])
    assert (rec['pre_blobs'][:, 3] == 1).all()
    assert len(rec['pre_blobs']) == int((~np.isnan(s['noise'][:, 0])).sum())       # no false positives


def test_records_survive_pickle_and_plain_list_batching(gold):
    c = gold.cases['B']
    tb, _ = T.builder(c['cfg'])
    recs = [gold.encode(tb, s) for s in c['samples']]
    back = pickle.loads(pickle.dumps(recs, protocol=pickle.HIGHEST_PROTOCOL))
    assert len(pickle.dumps(recs[0])) < 16384                 # a record is small: a few hundred bytes per object
    for a, b in zip(recs, back):
        assert sorted(a) == sorted(b) == ['counts', 'hm_blobs', 'pre_blobs', 'rects', 'slot_k', 'slot_v']
        for k in a:
            assert isinstance(b[k], np.ndarray) and b[k].dtype == np.int32 and a[k].tobytes() == b[k].tobytes()
        ra, rb = tb.reference(a), tb.reference(b)
        assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra)
    want = T.stack([s['ret'] for s in c['samples']])
    got = T.stack([tb.reference(r) for r in back])
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_refusals():
    from centertrack_amd._lib import CTError
    from centertrack_amd.targets import TargetBuilder
    cat = {1: 1}
    for h in ('hps', 'hm_hp', 'hp_offset'):
        with pytest.raises(CTError, match='pose'):
            TargetBuilder(T.make_opt(('hm', 'reg', 'wh', h), 1, (8, 8), False, False), 1, 4, cat)
    opt = T.make_opt(('hm', 'reg', 'wh'), 1, (8, 8), False, False)
    opt.dense_reg = 2
    with pytest.raises(CTError, match='dense_reg'):
        TargetBuilder(opt, 1, 4, cat)
    tb, opt = T.synth_builder(1, (8, 8), 4)
    with pytest.raises(CTError, match='pre_anns'):
        tb.encode([], T.IDENT_OUT, 32, 32)
    with pytest.raises(CTError, match='noise'):
        T.synth_record(tb, opt, [], [{'bbox': [1, 1, 4, 4], 'category_id': 1}], noise=np.zeros((2, 6)))
    rec = T.synth_record(tb, opt, [{'bbox': [1, 1, 9, 9], 'category_id': 1, 'track_id': 1}], [])
    bad = dict(rec, counts=np.array([2, 1, 0, 0], np.int32))
    with pytest.raises(CTError, match='disagree'):
        tb.reference(bad)
    with pytest.raises(CTError, match='CPU fallback'):
        tb.render([rec], device='cpu')


def test_binding_mirrors_the_kernel_constants():
    from centertrack_amd import _lib, targets
    K = T.kernel_constants()
    assert (targets.TILE_W, targets.TILE_H, targets.CULL_CAP) == (K['TW'], K['TH'], K['CAP'])
    assert targets.CULL_CAP == _lib.CT_TARGETS_CULL_CAP and _lib.CT_TARGETS_MAX_OUT == K['MAX_OUT'] == targets.MAX_OUT
    assert targets.MAX_RADIUS == K['MAX_RADIUS']
    assert K['TW'] * K['TH'] == 256                           # one thread per pixel of a tile
    lib = _lib.load()
    assert lib.ct_build_targets_header_words(3, 8, 15, 11) == 8 * 3 + 3 * 8 + 15 + 4 * 11
    assert lib.ct_build_targets_header_words(0, 8, 15, 11) == 0
    # every head at once stays inside the output table
    heads = ('hm',) + tuple(h for h, _ in targets.HEAD_DIMS) + ('rot',)
    tb = targets.TargetBuilder(T.make_opt(heads, 10, (8, 8), True, True), 10, 4, {1: 1})
    assert len(tb.outputs) == 26 <= K['MAX_OUT'] and tb.slot_words == 3 + 2 * 31 + 5


def test_argument_checks_without_gpu():
    """ct_build_targets validates the host copy of the buffer before it enqueues anything"""
    import ctypes
    from centertrack_amd import _lib
    lib = _lib.load()
    assert lib.ct_build_targets(None, None) == _lib.CT_ERR_ARG and b'null' in lib.ct_last_error()
    B, M, S, nout = 1, 2, 3, 3
    payload = 8 * B + B * M + S + 4 * nout
    buf = np.zeros(payload + 16, np.int32)
    out = np.zeros(64, np.int64)
    d = _lib.TargetsDesc()
    d.staging_host = d.staging_dev = buf.ctypes.data
    d.words, d.B, d.max_objs, d.slot_words, d.nout = buf.size, B, M, S, nout
    d.C, d.h, d.w = 2, 8, 8
    d.hm = out.ctypes.data

    def fill():
        buf[:] = 0
        buf[0:8] = [payload, 1, payload + 3, 1, payload + 7, 1, payload + 12, 1]
        buf[8:10] = [0, -1]
        buf[10:13] = [0, 1, 2]
        for t in range(3):
            buf[13 + 4 * t:17 + 4 * t] = [1, 0, t | (1 << 16), 1 if t < 2 else 0]
        buf[payload + 3:payload + 7] = [1, 3, 3, 2]           # hm blob: plane 1
        buf[payload + 7:payload + 12] = [-1, 0, 0, 3, 3]
        buf[payload + 12:payload + 16] = [5, 5, 1, 1]

    def rejected(what):
        assert lib.ct_build_targets(ctypes.byref(d), None) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error(), lib.ct_last_error()

    fill(); buf[payload + 3] = 2; rejected(b'plane 2 outside')
    fill(); buf[payload + 7] = -2; rejected(b'rectangle')
    fill(); buf[3] = 2; buf[2] = payload + 12; rejected(b'counts beyond the buffer')
    fill(); buf[1] = -1; rejected(b'counts beyond the buffer')
    fill(); buf[6] = 3; rejected(b'counts beyond the buffer')            # an offset inside the header
    fill(); buf[9] = 1; rejected(b'row 1 of 1')
    fill(); buf[payload + 6] = -1; rejected(b'radius')
    fill(); buf[11] = 0; rejected(b'column 1')
    fill(); d.B = 0; rejected(b'bad sizes'); d.B = B
    fill(); d.h = 0; rejected(b'bad hm shape'); d.h = 8
    fill(); d.staging_dev = None; rejected(b'null staging'); d.staging_dev = buf.ctypes.data
    fill(); d.words = payload - 1; rejected(b'header alone'); d.words = buf.size


def test_regimes_are_reached_by_the_gpu_shapes(gold):
    """every regime of build_targets_kernel is run by a golden case or by one of the cases E-H of test_hip_targets.py"""
    K = T.kernel_constants()
    runs = []
    for c in T.CASES:
        tb, _ = T.builder(gold.cases[c]['cfg'])
        runs.append((tb, [gold.encode(tb, s) for s in gold.cases[c]['samples']]))
    runs += [make() for make in T.SYNTH.values()]
    R = T.regimes(K)
    missing = [name for name, pred in R.items() if not any(pred(tb, recs) for tb, recs in runs)]
    assert not missing, missing
    # what the issue asks of E-H
    tb, recs = T.SYNTH['E']()
    assert (tb.opt.output_h, tb.opt.input_h, len(recs), tb.num_classes) == (128, 512, 2, 80)
    assert all(r['counts'][0] >= 100 and r['counts'][3] >= 100 for r in recs)
    tb, recs = T.SYNTH['F']()
    assert recs[0]['counts'][3] > 2 * K['CAP'] and recs[1]['counts'][3] == 0
    assert T.tile_load(recs[:1], 'pre_blobs', (0, 1, 2), (tb.opt.input_h, tb.opt.input_w), K) >= K['CAP'] + 1
    tb, recs = T.SYNTH['G']()
    assert (tb.opt.output_h, tb.opt.output_w, tb.opt.input_h, tb.opt.input_w) == (7, 33, 28, 132)
    tb, recs = T.SYNTH['H']()
    assert len(recs) == 1 and tb.num_classes == 1 and recs[0]['hm_blobs'][0, 3] == 0
