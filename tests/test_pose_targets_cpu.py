"""CPU: ``centertrack_amd.targets.PoseTargetBuilder`` on the host.  ``reference(encode(...))`` on
the inputs the golden generator recorded from the reference's own ``GenericDataset.__getitem__`` with the pose heads
equals the ``ret`` it returned EXACTLY -- both sides are numpy, so the bound is 0 --, ct_build_pose_targets checks its
arguments on fake pointers, and the GPU shapes of test_hip_pose_targets.py are held against the constants of
csrc/targets.hip.  Nothing here touches a device."""
import ctypes
import pickle

import numpy as np
import pytest

import _pose_targets as P
import _targets as T


@pytest.fixture(scope='module')
def gold():
    return P.golden()


@pytest.mark.parametrize('case', P.CASES)
def test_reference_of_encode_equals_the_golden_ret_exactly(gold, case):
    c = gold.cases[case]
    tb, _ = P.builder(c['cfg'])
    assert len(c['samples']) >= 2
    for i, s in enumerate(c['samples']):
        got = tb.reference(gold.encode(tb, s))
        want = s['ret']
        assert sorted(got) == sorted(want), (case, i)
        assert set(P.JOINT_KEYS + ('hps', 'hps_mask', 'hm_hp')) <= set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case, i, k)
            assert got[k].tobytes() == want[k].tobytes(), (case, i, k, np.abs(got[k] - want[k]).max())


def test_golden_holds_the_situations_the_cases_are_there_for(gold):
    J = P.J
    p1 = gold.cases['P1']
    tb, opt = P.builder(p1['cfg'])
    recs = [gold.encode(tb, s) for s in p1['samples']]
    e = p1['empty']
    assert recs[e]['counts'].tolist() == [0, 0, 0, 0] and 0 < e < len(recs) - 1
    assert all(len(s['anns']) > tb.max_objs for i, s in enumerate(p1['samples']) if i != e)
    ret = T.stack([s['ret'] for s in p1['samples']])
    assert ret['hps'].shape[1:] == (8, 2 * J) and ret['hm_hp'].shape[1:] == (J, 24, 40)
    assert ret['hp_ind'].shape[1:] == (8 * J,) and ret['hp_ind'].dtype == np.int64 and ret['joint'].dtype == np.int64
    assert ret['hp_offset'].shape[1:] == (8 * J, 2) and ret['hp_offset_mask'].shape[1:] == (8 * J, 2)
    seen = ret['hps_mask'].reshape(-1, 8, J, 2)[..., 0] > 0
    learnt = ret['hm_hp_mask'].reshape(-1, 8, J) > 0
    assert (seen & learnt).any() and (seen & ~learnt).any() and not (learnt & ~seen).any()    # visibility 2 and 1
    assert (ret['joint'].reshape(-1, 8, J)[seen] == np.broadcast_to(np.arange(J), seen.shape)[seen]).all()
    assert (ret['hp_ind'].reshape(-1, 8, J)[~seen] == 0).all()
    rects = np.concatenate([r['rects'] for r in recs])
    assert (rects[:, 0] == -2).any() and (rects[:, 0] >= 1).any()          # all hm_hp planes; one of them
    between = 0
    for c in P.CASES:
        for s in gold.cases[c]['samples']:
            between += int(((s['ret']['hm_hp'] > 0) & (s['ret']['hm_hp'] < 1)).sum())
    assert between >= 1000                                                   # Gaussians, not only rectangles
    # P2: two class planes in front, hp_offset not a head but its targets are there; ignore regions with / without hm_hp
    p2 = gold.cases['P2']
    tb2, _ = P.builder(p2['cfg'])
    assert tb2.num_classes == 2 and 'hp_offset' not in p2['cfg']['heads'] and not p2['cfg']['tracking']
    recs2 = [gold.encode(tb2, s) for s in p2['samples']]
    r2 = np.concatenate([r['rects'] for r in recs2])
    assert (r2[:, 0] == -1).any() and (r2[:, 0] == 0).any() and (r2[:, 0] == 1).any() and (r2[:, 0] == -2).any()
    # class ids 0, -1, -2 mask hm_hp too (cls_id <= 1); the iscrowd annotations of class 2 mask their hm plane alone
    assert 0 < (r2[:, 0] == -2).sum() == (r2[:, 0] < 2).sum() - (r2[:, 0] == -2).sum() - len(recs2)
    assert all('hp_offset' in s['ret'] and not [k for k in s['ret'] if k.startswith('pre_')] for s in p2['samples'])
    assert np.concatenate([r['hm_blobs'] for r in recs2])[:, 0].max() == 2 + J - 1
    # P3: the edge samples
    p3 = gold.cases['P3']
    tb3, opt3 = P.builder(p3['cfg'])
    recs3 = [gold.encode(tb3, s) for s in p3['samples']]
    b0 = recs3[0]['hm_blobs']
    hp = b0[b0[:, 0] >= 1]
    assert [1, 0, 0] in hp[:, :3].tolist()                                   # joint 0 at exactly (0, 0)
    assert (hp[:, 1] == opt3.output_w - 1).any() and (hp[:, 2] == opt3.output_h - 1).any()
    assert len(np.unique(hp[:, :3], axis=0)) < len(hp)                      # two persons, one joint, one pixel
    assert any('keypoints' not in a for a in p3['samples'][0]['anns'])
    b1 = recs3[1]['hm_blobs']
    assert ((b1[:, 0] >= 1) & (b1[:, 3] == 0)).any()                        # a radius-0 person's joint
    assert recs3[1]['slot_k'].tolist() == [0, 2]                             # the person with the empty box left nothing


@pytest.mark.parametrize('case', ('P1', 'P3'))
def test_encode_consumes_a_random_stream_in_the_recorded_order(gold, case):
    c = gold.cases[case]
    tb, _ = P.builder(c['cfg'])
    for s in c['samples']:
        key, pos, gauss, nxt = s['rng']
        rs = np.random.RandomState()
        rs.set_state(('MT19937', key, pos, int(gauss[0]), float(gauss[1])))
        a, b = gold.encode(tb, s, rng=rs), gold.encode(tb, s)
        for k in b:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert rs.random_sample() == nxt


def test_records_survive_pickle(gold):
    c = gold.cases['P1']
    tb, _ = P.builder(c['cfg'])
    recs = [gold.encode(tb, s) for s in c['samples']]
    back = pickle.loads(pickle.dumps(recs, protocol=pickle.HIGHEST_PROTOCOL))
    for a, b in zip(recs, back):
        assert sorted(a) == sorted(b) == ['counts', 'hm_blobs', 'pre_blobs', 'rects', 'slot_k', 'slot_v']
        for k in a:
            assert isinstance(b[k], np.ndarray) and b[k].dtype == np.int32 and a[k].tobytes() == b[k].tobytes()
    want = T.stack([s['ret'] for s in c['samples']])
    got = T.stack([tb.reference(r) for r in back])
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_refusals():
    from centertrack_amd._lib import CTError
    from centertrack_amd.targets import PoseTargetBuilder, TargetBuilder
    cat = {1: 1}

    def opt(heads):
        return T.make_opt(heads, 1, (8, 8), False, False)

    with pytest.raises(CTError, match='hps and hm_hp'):
        PoseTargetBuilder(opt(('hm', 'reg', 'wh', 'hps')), 1, 4, cat)
    with pytest.raises(CTError, match='hps and hm_hp'):
        PoseTargetBuilder(opt(('hm', 'reg', 'wh', 'hm_hp', 'hp_offset')), 1, 4, cat)
    with pytest.raises(CTError, match='hps and hm_hp'):
        PoseTargetBuilder(opt(('hm', 'reg', 'wh')), 1, 4, cat)
    o = opt(('hm', 'reg', 'wh', 'hps', 'hm_hp'))
    o.simple_radius = 0.5
    with pytest.raises(CTError, match='simple_radius'):
        PoseTargetBuilder(o, 1, 4, cat)
    o = opt(('hm', 'reg', 'wh', 'hps', 'hm_hp'))
    o.dense_reg = 2
    with pytest.raises(CTError, match='dense_reg'):
        PoseTargetBuilder(o, 1, 4, cat)
    with pytest.raises(CTError, match='num_joints'):
        PoseTargetBuilder(opt(('hm', 'reg', 'wh', 'hps', 'hm_hp')), 1, 4, cat, num_joints=0)
    for h in ('hps', 'hm_hp', 'hp_offset'):                   # TargetBuilder itself still refuses every pose head
        with pytest.raises(CTError, match='pose'):
            TargetBuilder(opt(('hm', 'reg', 'wh', h)), 1, 4, cat)
    with pytest.raises(CTError, match='pose'):
        TargetBuilder(opt(('hm', 'reg', 'wh', 'hps', 'hm_hp', 'hp_offset')), 1, 4, cat)
    tb, o = P.synth_builder(1, (8, 8), 4, pre_hm=False)
    rec = T.synth_record(tb, o, [{'bbox': [1, 1, 9, 9], 'category_id': 1}])          # no keypoints: 17 rectangles
    assert rec['counts'].tolist() == [1, 1, P.J, 0] and sorted(rec['rects'][:, 0].tolist()) == list(range(1, 1 + P.J))
    with pytest.raises(CTError, match='disagree'):
        tb.reference(dict(rec, counts=np.array([1, 1, 0, 0], np.int32)))
    with pytest.raises(CTError, match='CPU fallback'):
        tb.render([rec], device='cpu')
    # the layout: hps behind velocity's place, the joint tensors behind the heads, as _init_ret creates them
    names = [n for n, _, _, _ in tb.outputs]
    assert names == ['ind', 'cat', 'mask', 'reg', 'reg_mask', 'wh', 'wh_mask', 'hps', 'hps_mask'] + list(P.JOINT_KEYS)
    assert tb.slot_words == 3 + 2 * (2 + 2 + 2 * P.J) + 7 * P.J
    specs = {n: (4, wd) for n, wd, _, _ in tb.outputs}
    assert specs['hp_offset'] == (4, 2 * P.J) and specs['hp_ind'] == (4, P.J)


def test_argument_checks_without_gpu():
    """ct_build_pose_targets validates the host copy of the buffer before it enqueues anything"""
    from centertrack_amd import _lib
    lib = _lib.load()
    assert lib.ct_build_pose_targets(None, None) == _lib.CT_ERR_ARG and b'null' in lib.ct_last_error()
    B, M, S, nout = 1, 2, 3, 3
    C, J = 2, 3
    payload = 8 * B + B * M + S + 4 * nout
    assert payload == lib.ct_build_targets_header_words(B, M, S, nout)
    buf = np.zeros(payload + 16, np.int32)
    out = np.zeros(64, np.int64)
    d = _lib.PoseTargetsDesc()
    t = d.base
    t.staging_host = t.staging_dev = buf.ctypes.data
    t.words, t.B, t.max_objs, t.slot_words, t.nout = buf.size, B, M, S, nout
    t.C, t.h, t.w = C, 8, 8
    t.hm = d.hm_hp = out.ctypes.data
    d.J = J

    def fill():
        buf[:] = 0
        buf[0:8] = [payload, 1, payload + 3, 1, payload + 7, 1, payload + 12, 1]
        buf[8:10] = [0, -1]
        buf[10:13] = [0, 1, 2]
        for o in range(3):
            buf[13 + 4 * o:17 + 4 * o] = [1, 0, o | (1 << 16), 1 if o < 2 else 0]
        buf[payload + 3:payload + 7] = [C + J - 1, 3, 3, 2]  # a blob on the last hm_hp plane
        buf[payload + 7:payload + 12] = [-2, 0, 0, 3, 3]     # a rectangle over all hm_hp planes
        buf[payload + 12:payload + 16] = [5, 5, 1, 1]

    def rejected(what):
        assert lib.ct_build_pose_targets(ctypes.byref(d), None) == _lib.CT_ERR_ARG
        assert what in lib.ct_last_error() and b'ct_build_pose_targets' in lib.ct_last_error(), lib.ct_last_error()

    fill(); buf[payload + 3] = C + J; rejected(b'plane 5 outside [0, 5)')
    fill(); buf[payload + 3] = -1; rejected(b'plane -1 outside')
    fill(); buf[payload + 7] = -3; rejected(b'rectangle 0: plane -3 outside [-2, 5)')
    fill(); buf[payload + 7] = C + J; rejected(b'rectangle 0: plane 5')
    # no pose planes declared: the lists may not name any, whether through a blob or through the "all" code
    fill(); d.hm_hp, d.J = None, 0; rejected(b'blob 0: plane 4 outside [0, 2)')
    fill(); buf[payload + 3] = 1; rejected(b'rectangle 0: plane -2 outside [-1, 2)')
    d.hm_hp, d.J = out.ctypes.data, J
    fill(); d.J = 0; rejected(b'hm_hp given with J 0')
    fill(); d.J = -1; rejected(b'bad J')
    d.hm_hp = None; fill(); rejected(b'bad J')                # a negative J is refused with or without the map
    d.hm_hp, d.J = out.ctypes.data, J
    fill(); t.h = 0; rejected(b'bad hm'); t.h = 8
    fill(); t.hm = None; t.C = 0; rejected(b'bad hm_hp shape'); t.hm, t.C = out.ctypes.data, C
    fill(); buf[payload + 6] = -1; rejected(b'radius')
    fill(); buf[3] = 2; buf[2] = payload + 12; rejected(b'counts beyond the buffer')
    fill(); t.staging_dev = None; rejected(b'null staging'); t.staging_dev = buf.ctypes.data
    # the layout the binding mirrors
    assert ctypes.sizeof(_lib.PoseTargetsDesc) == ctypes.sizeof(_lib.TargetsDesc) + 16
    assert _lib.PoseTargetsDesc.hm_hp.offset == ctypes.sizeof(_lib.TargetsDesc)


def test_descriptor_matches_the_header_layout(tmp_path):
    import os
    import shutil
    import subprocess
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "centertrack_hip.h"\nint main(void) {'
                   'printf("%zu %zu %zu %zu\\n", sizeof(ct_pose_targets_desc), offsetof(ct_pose_targets_desc, hm_hp),'
                   'offsetof(ct_pose_targets_desc, J), sizeof(ct_targets_desc)); return 0; }\n')
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(T.ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    D = _lib.PoseTargetsDesc
    assert got == [ctypes.sizeof(D), D.hm_hp.offset, D.J.offset, ctypes.sizeof(_lib.TargetsDesc)]


def test_regimes_are_reached_by_the_gpu_shapes(gold):
    """every regime of the pose side of build_targets_kernel is run by a golden case or by one of the cases PE-PH of
    test_hip_pose_targets.py"""
    K = T.kernel_constants()
    src = open(T.os.path.join(T.ROOT, 'centertrack_amd', 'csrc', 'targets.hip')).read()
    assert 'template <bool POSE>' in src and 'build_targets_kernel<true>' in src and 'build_targets_kernel<false>' in src
    runs = []
    for c in P.CASES:
        tb, _ = P.builder(gold.cases[c]['cfg'])
        runs.append((tb, [gold.encode(tb, s) for s in gold.cases[c]['samples']]))
    synth = {name: make() for name, make in P.SYNTH.items()}
    runs += list(synth.values())
    R = P.regimes(K)
    missing = [name for name, pred in R.items() if not any(pred(tb, recs) for tb, recs in runs)]
    assert not missing, missing
    # hm_hp asked for and not asked for (out=)
    assert any('hm_hp' in v for v in P.OUT_SUBSETS.values()) and any('hm_hp' not in v for v in P.OUT_SUBSETS.values())
    # what the issue asks of PE-PH
    tb, recs = synth['PE']
    assert (tb.opt.output_h, tb.opt.input_h, len(recs), tb.num_classes, tb.max_objs) == (128, 512, 2, 1, 32)
    assert all(r['counts'][1] == 32 * (P.J + 1) > 2 * K['CAP'] and r['counts'][2] == 0 for r in recs)
    tb, recs = synth['PF']
    assert (tb.opt.output_h, tb.opt.output_w) == (16, 24) and tb.max_objs >= K['CAP'] + 40
    assert recs[1]['counts'].tolist() == [0, 0, 0, 0] and P.hp_tile_load(tb, recs[:1], K) >= K['CAP'] + 1
    assert set(recs[0]['hm_blobs'][:, 0].tolist()) == {0, 1}                 # one joint type visible
    tb, recs = synth['PG']
    assert (tb.opt.output_h, tb.opt.output_w) == (7, 33)
    tb, recs = synth['PH']
    assert len(recs) == 1 and recs[0]['counts'].tolist() == [1, 2, 0, 0] and recs[0]['hm_blobs'][1, 3] == 0
