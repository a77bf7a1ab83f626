"""CPU: the heat-map decode's selection paths (centertrack_amd/csrc/decode.hip) -- the label table of tests/_decode_paths.py
against the cases the GPU tests run, the order rule for the threshold path, the restated schedule against
``ct_decode_workspace_bytes`` over a generated sweep, the kernel's constants against the model's, the reference against
``oracle.decode.generic_decode``, six mutations of the reference against the cases named for them, the designed conditions of
the seam and pose cases, and the argument errors ``ct_decode`` returns before any launch.  Nothing here launches a kernel: the
library calls run in a child process that sees no device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _decode_paths as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HUGE = 1 << 62


# ---------------------------------------------------------------------------------------------------------------------
# the table and the list

def test_every_label_is_reached_and_every_case_owns_one(capsys):
    own = P.owners()
    assert sorted(own) == sorted(P.LABELS), sorted(set(own) ^ set(P.LABELS))
    assert [k for k, v in own.items() if not v] == []
    assert not set(P.UNREACHABLE) & set(own)
    with capsys.disabled():
        print()
        for label, names in own.items():
            c = P.CASE[names[0]]
            info = P.case_labels(c.name)[1][0]
            print('%-20s %-13s %-5s %2d,%2d,%4d,%4d,%3d  total %6s  n %s' % (label, c.name, '' if len(names) == 1 else '(+%d)' % (len(names) - 1),
                                                                              c.B, c.C, c.h, c.w, c.K, info.get('total'),
                                                                              max(info['ns']) if 'ns' in info else '-'))
    for c in P.CASES:
        assert [k for k, v in own.items() if v == [c.name]], c.name
        assert c.why and c.B * c.C * c.h * c.w <= 1700000, c.name


def test_the_cases_end_where_they_were_built_to_end():
    ends = {c.name: {i['end'] for i in P.case_labels(c.name)[1].values()} for c in P.CASES}
    for name, end in (('regs_rank', 'regs:rank'), ('regs_radix', 'regs:radix'), ('mem_rank', 'mem:rank'), ('mem_radix', 'mem:radix'),
                      ('mem_bitonic', 'mem:bitonic'), ('mem_slow', 'mem:slow'), ('const_160', 'regs:rank'), ('const_small', 'regs:hist'),
                      ('cluster_mot', 'regs:bitonic')):
        assert ends[name] == {end}, (name, ends[name])
    L = {c.name: P.case_labels(c.name)[0] for c in P.CASES}
    assert {'tie:2a:radix', 'tie:mem:radix'} <= L['const_mem'] and 'tie:regs:radix' in L['const_radix']
    assert '2a:radix' in L['cluster_coco'] and '2a:few' in L['mem_rank'] and 's1:seg512' in L['seg_512']
    assert {'tie:s1:rank', 'tie:regs:rank'} <= L['const_160'] and 's1:all' not in L['const_160']      # rank counting in all 100 segments
    assert {'s1:midrow', 's1:ragged'} <= L['seam_17x30']
    info = P.case_labels('regs_rank')[1][0]
    assert (info['seg'], info['M2'], info['G'], info['total']) == (256, 8000, 0, 6400)
    info = P.case_labels('regs_radix')[1][3]
    assert (info['seg'], info['M2'], info['G'], info['total']) == (1024, 8100, 0, 6912)
    assert [P.case_labels(n)[1][0]['G'] for n in ('mem_rank', 'mem_radix')] == [42, 20]
    assert P.case_labels('mem_radix')[1][0]['slots2'] == 10240 and P.case_labels('mem_rank')[1][0]['slots2'] == 8400


def test_rank_and_radix_hold_under_every_slot_order():
    n = 0
    for c in P.CASES:
        for b, info in P.case_labels(c.name)[1].items():
            kind = info['end'].split(':')[-1]
            if 'ns' not in info:
                assert kind not in ('rank', 'radix', 'rank-or-radix')
                continue
            assert len(info['ns']) == 1 + len(P.ORDER_SEEDS) == 17
            if kind == 'rank':
                assert c.K <= max(info['ns']) <= P.FCAP // 2, (c.name, b, info['ns'])
            else:
                assert kind == 'radix' and c.K > 256 and info['total'] > P.FCAP and set(info['ns']) == {info['total']}, (c.name, b, info)
            n += 1
    assert n >= 25                                          # regs_rank, mem_rank, mem_radix, const_160, const_mem, 2 x 10 images of *_radix


def test_the_reuse_maps_end_where_the_reuse_tests_say():
    for where, (shape_of, maps) in P.REUSE.items():
        case = P.CASE[shape_of]
        for make, want in maps:
            hm = make(case)
            thr, first = P.classify_threshold(hm, case.K)
            for b, (labels, info) in enumerate(first):
                assert (thr[b][0] if b in thr else info['end']) == want, (where, want, b, info)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's constants and the schedule, through the source and through the ABI

def test_the_models_constants_are_the_kernels():
    src = open(os.path.join(ROOT, 'centertrack_amd', 'csrc', 'decode.hip')).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r'^constexpr int (\w+) = (\d+);', src, re.M)}
    for name in ('SEG_MAX', 'MAXK', 'FCAP', 'SLICE', 'SEL_U', 'SEL_BINS', 'TIECAP'):
        assert got[name] == getattr(P, name), (name, got[name])
    assert P.SLICE == P.SEL_U * P.NT and re.search(r'decode_stage2_kernel, dim3\(\(unsigned\)d->B\), dim3\(1024\)', src)


def _sweep():
    shapes = [(3, 3), (17, 30), (1, 600), (600, 1), (64, 64), (90, 100), (96, 320), (128, 128), (144, 192), (160, 160), (2, 4096), (300, 500)]
    i = 0
    for B in (1, 2, 4, 10):
        for C in (1, 2, 3, 10, 16, 80):
            for h, w in shapes:
                for K in (1, 9, 40, 100, 200, 300, 512):
                    i += 1
                    if h * w >= K and i % 5 == 0:
                        yield B, C, h, w, K
    # B*C*nseg == 255 / 256 at 1024 pixels (seg 512 / 1024) and at 512 pixels (seg 256 / 512)
    for B, C, h, w in ((1, 255, 32, 32), (1, 256, 32, 32), (3, 85, 32, 32), (4, 64, 32, 32), (1, 51, 40, 64), (1, 64, 32, 64), (5, 51, 16, 32)):
        yield B, C, h, w, 7
    # M2 == 8192 / 8193 and their neighbours
    for case in ((1, 1, 64, 64, 512), (1, 2731, 16, 16, 3), (1, 1, 64, 64, 511), (2, 1, 64, 65, 482), (1, 4, 32, 32, 512), (1, 4097, 16, 16, 2),
                 (1, 2, 100, 100, 103), (1, 2, 100, 100, 102)):
        yield case


def _ptr():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def _desc(p, B, C, h, w, K, **kw):
    from centertrack_amd import _lib
    d = _lib.DecodeDesc()
    d.hm = d.out = d.workspace = p
    d.B, d.C, d.h, d.w, d.K, d.workspace_bytes = B, C, h, w, K, HUGE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _child_main():
    """runs in the child: no device is visible, every call is host code up to (at most) a refused launch"""
    from centertrack_amd import _lib
    lib = _lib.load()
    keep, p = _ptr()
    out = {'devices': torch.cuda.device_count(), 'sweep': [], 'n': 0, 'errors': {}}
    for B, C, h, w, K in _sweep():
        got = lib.ct_decode_workspace_bytes(ctypes.byref(_desc(p, B, C, h, w, K)))
        out['n'] += 1
        if got != P.schedule(B, C, h, w, K)['bytes']:
            out['sweep'].append([B, C, h, w, K, got])

    def call(name, d):
        rc = lib.ct_decode(ctypes.byref(d), None)
        out['errors'][name] = [rc, lib.ct_last_error().decode()]
    need = P.schedule(1, 2, 16, 16, 10)['bytes']
    call('K=0', _desc(p, 1, 2, 16, 16, 0))
    call('K=513', _desc(p, 1, 2, 32, 32, 513))
    call('h*w<K', _desc(p, 1, 2, 3, 3, 10))
    call('workspace', _desc(p, 1, 2, 16, 16, 10, workspace_bytes=need - 1))
    call('w=4097', _desc(p, 1, 1, 1, 4097, 4))
    call('out_stride', _desc(p, 1, 2, 16, 16, 10, out_stride=3))
    call('done_flag', _desc(p, 1, 2, 16, 16, 10, host_out=p, done_flag=p))
    if out['devices'] == 0:                                  # the accepted side: validation passes, the launch has no device
        call('accepted', _desc(p, 1, 1, 2, 4096, 16, workspace_bytes=P.schedule(1, 1, 2, 4096, 16)['bytes'], out_stride=4))
    print(json.dumps(out))


@pytest.fixture(scope='module')
def child():
    from centertrack_amd import _lib, build
    build.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.dirname(__file__)] + sys.path))
    code = 'import test_decode_paths_cpu as T\nT._child_main()\n'
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_restated_schedule_gives_the_librarys_workspace_size(child):
    """(B*M2 + B*G*K) * 8 with M2 = C*nseg*K and G monotone in M2: the byte count pins nseg, hence seg, and G"""
    assert child['n'] > 300 and child['sweep'] == [], child['sweep'][:10]
    segs = {P.schedule(*c)['seg'] for c in _sweep()}
    gs = {P.schedule(*c)['G'] for c in _sweep()}
    assert segs == {256, 512, 1024} and {0, 2} <= gs and max(gs) >= 100
    for c, want in (((1, 255, 32, 32, 7), 512), ((1, 256, 32, 32, 7), 1024), ((1, 51, 40, 64, 7), 256), ((1, 64, 32, 64, 7), 512)):
        assert P.schedule(*c)['seg'] == want
    assert P.schedule(1, 1, 64, 64, 512)['M2'] == 8192 and P.schedule(1, 1, 64, 64, 512)['G'] == 0
    assert P.schedule(1, 2731, 16, 16, 3)['M2'] == 8193 and P.schedule(1, 2731, 16, 16, 3)['G'] == 2


def test_argument_errors_return_before_any_launch(child):
    from centertrack_amd import _lib
    e = child['errors']
    for name, rc, word in (('K=0', _lib.CT_ERR_ARG, 'K=0 out of range'), ('K=513', _lib.CT_ERR_ARG, 'K=513 out of range'),
                           ('h*w<K', _lib.CT_ERR_ARG, 'h*w=9 < K=10'), ('workspace', _lib.CT_ERR_WORKSPACE, 'workspace bytes'),
                           ('w=4097', _lib.CT_ERR_ARG, 'w=4097'), ('out_stride', _lib.CT_ERR_ARG, 'out_stride 3'),
                           ('done_flag', _lib.CT_ERR_ARG, 'done_flag needs')):
        assert e[name][0] == rc and word in e[name][1], (name, e[name])
    if child['devices'] == 0:
        assert e['accepted'][0] in (_lib.CT_OK, _lib.CT_ERR_LAUNCH), e['accepted']


# ---------------------------------------------------------------------------------------------------------------------
# the reference

@pytest.mark.parametrize('name', [c.name for c in P.CASES if c.distinct])
def test_the_reference_is_the_oracle_where_scores_are_distinct(name):
    from oracle import decode as odecode
    case = P.CASE[name]
    maps = {'hm': torch.from_numpy(P.heat_map(name).copy())}
    maps.update((k, torch.from_numpy(v.copy())) for k, v in P.head_maps(name).items())
    ref = P.reference(name)
    want = odecode.generic_decode(maps, K=case.K, return_inds=True)
    nms = P.nms(P.heat_map(name))
    for b in range(case.B):
        # distinct where it matters: among the positive survivors; a map with fewer than K of them is compared on that prefix
        pos = nms[b][nms[b] > 0]
        assert np.unique(pos).size == pos.size
        npos = min(case.K, pos.size)
        for k, v in ref.items():
            np.testing.assert_array_equal(v[b, :npos], want[k][b, :npos].numpy(), err_msg='%s.%s' % (name, k))
    assert {'bboxes', 'tracking'} <= set(ref) and set(ref) <= set(want)


def test_the_reference_is_the_oracle_under_the_documented_tie_order():
    from oracle import decode as odecode
    for case in P.CASES:
        if case.distinct:
            continue
        maps = {'hm': torch.from_numpy(P.heat_map(case.name).copy())}
        maps.update((k, torch.from_numpy(v.copy())) for k, v in P.head_maps(case.name).items())
        with P.documented_tie_order():
            want = odecode.generic_decode(maps, K=case.K, return_inds=True)
        for k, v in P.reference(case.name).items():
            np.testing.assert_array_equal(v, want[k].numpy(), err_msg='%s.%s' % (case.name, k))
    assert torch.topk(torch.tensor([1.0, 3.0, 2.0]), 2)[1].tolist() == [1, 2]          # (the real top-K is back)


def test_every_mutation_is_caught_by_its_case():
    assert sorted(P.MUTATION_CASE) == sorted(P.MUTATIONS) == list('abcdef')
    for m, name in P.MUTATION_CASE.items():
        ref, mut = P.reference(name), P.mutated(name, m)
        assert not P.same(ref, mut), (m, name)
        assert not np.array_equal(ref['inds'], mut['inds']) or not np.array_equal(ref['clses'], mut['clses']), (m, name)
    # and the unmutated decode is the reference
    assert P.same(P.reference('seam_17x30'), P.mutated('seam_17x30', None))


def test_the_seam_case_holds_what_it_was_built_for():
    case = P.CASE['seam_17x30']
    assert P.schedule(case.B, case.C, case.h, case.w, case.K)['seg'] == 256 and 256 // case.w == 8 and 256 % case.w == 16
    ref = P.reference('seam_17x30')
    got = list(zip(ref['ys'][0].astype(int).tolist(), ref['xs'][0].astype(int).tolist()))
    assert got[:6] == [(8, 15), (8, 16), (8, 10), (9, 10), (9, 6), (7, 23)]         # equal neighbours both survive, lower pixel first
    assert (8, 5) not in got and (8, 22) not in got                                    # suppressed from across the seam
    bad = P.mutated('seam_17x30', 'd')
    assert (8, 5) in list(zip(bad['ys'][0].astype(int).tolist(), bad['xs'][0].astype(int).tolist()))
    assert ref['scores'][0, 0] == ref['scores'][0, 1] == np.float32(0.9)


def test_the_saturated_and_over_range_cases_fill_bin_1023():
    nms = P.nms(P.heat_map('saturated'))[0]
    assert (nms == 1.0).sum() > P.TIECAP and (P.reference('saturated')['scores'] == 1.0).all()
    over = P.reference('over_range')['scores']
    assert over.max() > 2.9 and over.min() >= 1.0


def test_the_pose_case_holds_what_it_was_built_for():
    maps, ref = P.pose_maps(), P.pose_reference()
    assert maps['hm_hp'][0, 0, 10, 12] == np.float32(0.2) and not (np.float32(0.2) > np.float32(0.2))
    assert ref['inds'][0, :2].tolist() == [10 * 40 + 10, 2 * 40 + 20]
    np.testing.assert_array_equal(ref['bboxes'][0, :2], np.array([[4.5, 4.5, 16.5, 16.5], [15.5, -0.5, 25.5, 5.5]], np.float32))
    for (det, j), (xy, why) in P.POSE_WANT.items():
        assert why.startswith('pose:')
        np.testing.assert_array_equal(ref['hps'][0, det, 2 * j:2 * j + 2], np.array(xy, np.float32), err_msg=why)
    # the opposite decision of each designed test gives another key point: with >= the 0.2 peak would be taken, ...
    assert (ref['hps'][0, 0, 0:2] != np.array([12.5, 10.5], np.float32)).all()
    # joint 3's map has 5 positive peaks: its decode (one of B*J single-class images) ends in the slow path
    hm_hp = maps['hm_hp'].reshape(-1, 1, 24, 40)
    ends = [P.image_paths(hm_hp[i], hm_hp.shape[0], P.POSE['K'], kernels_only=True)[1]['end'] for i in (3, 4)]
    assert ends == ['regs:slow', 'regs:hist']
    assert (ref['kps_score'] > 0).all() and ref['hps'].shape == (2, 40, 34)
