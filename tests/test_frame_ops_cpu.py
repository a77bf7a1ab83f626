"""CPU: the frame's other kernels (stem, fused heads, flip, prior heat map, pose match) -- the regime tables of tests/_frame_ops.py
against the cases the GPU tests run, the constants and the padding rule of stem_kernel's tab[] against the sources, the restated
plans at their edges, the references against the oracle where it has the operation, the designed conditions of the cases, and every
mutation of a reference against the case named for it.  Nothing here launches a kernel or loads the library."""
import os
import re

import numpy as np
import pytest
import torch

import _frame_ops as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _src(name):
    return open(os.path.join(ROOT, 'centertrack_amd', 'csrc', name)).read()


FAMILIES = [
    ('stem', P.STEM_REGIMES, P.missing_stem_regimes, P.stem_keys, P.STEM_CASES),
    ('heads', P.HEADS_REGIMES, P.missing_heads_regimes, P.heads_keys, P.HEADS_CASES),
    ('flip', P.FLIP_REGIMES, P.missing_flip_regimes, P.flip_keys, P.FLIP_CASES + P.IMG_CASES),
    ('pre_hm', P.PHM_REGIMES, P.missing_phm_regimes, P.phm_keys, P.PHM_CASES),
    ('pose', P.POSE_REGIMES, P.missing_pose_regimes, P.pose_keys, P.POSE_CASES),
]


# ---------------------------------------------------------------------------------------------------------------------
# the tables and the lists

@pytest.mark.parametrize('family', [f[0] for f in FAMILIES])
def test_every_regime_is_reached_and_every_case_owns_one(family, capsys):
    _, regimes, missing, keys_of, cases = next(f for f in FAMILIES if f[0] == family)
    assert missing(cases) == []
    assert all(isinstance(line, str) and line for line in regimes.values())
    own = P.owned(keys_of, cases)
    with capsys.disabled():
        print()
        for c in cases:
            print('%-7s %-16s owns %s' % (family, c.name, ', '.join(map(str, own[c.name]))))
    assert [n for n, keys in own.items() if not keys] == []
    assert len({c.name for c in cases}) == len(cases) and all(c.why for c in cases)
    for c in cases:                                         # (the completeness is the list's: a shorter list misses a regime)
        assert missing([d for d in cases if d is not c]) != [], c.name


# ---------------------------------------------------------------------------------------------------------------------
# constants, read back from the sources

def _constexpr(src):
    out = {}
    for m in re.finditer(r'constexpr int ([^;]+);', src):
        for part in m.group(1).split(','):
            mm = re.match(r'\s*(\w+) = (\d+)\s*$', part)
            if mm:
                out[mm.group(1)] = int(mm.group(2))
    return out


def test_the_constants_are_the_sources():
    stem, flip, elem, pose = _src('stem.hip'), _src('flip.hip'), _src('elementwise.hip'), _src('pose.hip')
    c = _constexpr(stem)
    assert (c['ST_TW'], c['ST_PW'], c['ST_KTOT']) == (P.ST_TW, P.ST_PW, P.ST_KTOT)
    assert 'return s == 2 ? 52 : 148;' in stem and 'return s * 148;' in stem
    assert P.st_koff(2) + P.st_k4(2) == P.ST_KTOT
    m = re.search(r'rows16 = want == 16 \|\| \(want == 0 && blocks8 > (\d+) && blocks8 <= (\d+)\);', stem)
    assert (int(m.group(1)), int(m.group(2))) == (P.ST_ROWS16_ABOVE, P.ST_ROWS16_UPTO)
    assert 'const long blocks8 = (long)N * a.tilesX * ct_cdiv(H, 8);' in stem and 'a.tilesX = ct_cdiv(W, ST_TW);' in stem
    c = _constexpr(elem)
    assert (c['PHM_TW'], c['PHM_TH'], c['PHM_CAP']) == (P.PHM_TW, P.PHM_TH, P.PHM_CAP)
    c = _constexpr(flip)
    assert (c['FLIP_MAX_HEADS'], c['FLIP_MAX_JOINTS']) == (P.FLIP_MAX_HEADS, P.FLIP_MAX_JOINTS)
    m = re.search(r'unsigned blocks_for\(size_t threads\)\s*\{\s*size_t b = \(threads \+ 255\) / 256;\s*if \(b > (\d+)\) b = (\d+);', flip)
    assert int(m.group(1)) == int(m.group(2)) == P.FLIP_BLOCK_CAP
    hdr = open(os.path.join(ROOT, 'include', 'centertrack_hip.h')).read()
    assert int(re.search(r'#define CT_MAX_FUSED_HEADS (\d+)', hdr).group(1)) == P.CT_MAX_FUSED_HEADS
    assert np.float32(re.search(r'constexpr float POSE_THRESH = ([0-9.]+)f;', pose).group(1)) == P.POSE_THRESH
    assert re.search(r'__launch_bounds__\((\d+)\) void pose_match_kernel', pose).group(1) == str(P.POSE_BLOCK)
    assert 'hipLaunchKernelGGL(pose_match_kernel, dim3((unsigned)(d->B * d->num_joints)), dim3(%d),' % P.POSE_BLOCK in pose
    wino = _src('wino_mfma.hip')
    assert 'const unsigned per = nblocks >> 3;' in wino and 'ubid < per * 8u ? (ubid & 7u) * per + (ubid >> 3) : ubid' in wino
    assert 'a.tilesX = ct_cdiv(d->W, 16); a.tilesY = ct_cdiv(d->H, 4); a.coutBlocks = d->nheads;' in wino


# ---------------------------------------------------------------------------------------------------------------------
# the stem's tab[] and tile choice

def test_every_k_an_active_stem_visits_reads_a_plane_the_launch_staged():
    """the defect this pins: a padding k (zero weight) read plane 0, which only a launch with x stages -- in the {pre_hm} launch
    of every frame that was LDS left by the previous kernel, and NaN * 0 = NaN"""
    for mask in range(1, 8):
        staged = P.stem_staged_planes(mask)
        for k in P.stem_visited(mask):
            plane, row, col = P.stem_tab(k)
            assert plane in staged, (mask, k, plane)
            assert 0 <= row < 7 and 0 <= col < 7
    assert len(P.stem_visited(7)) == P.ST_KTOT
    padding = [k for k in range(P.ST_KTOT) if k - P.st_koff(k // 148) >= P.STEM_K[k // 148]]
    assert padding == [147, 295, 345, 346, 347] and [P.stem_tab(k)[0] for k in padding] == [0, 3, 6, 6, 6]
    taps = [P.stem_tab(k) for k in range(P.ST_KTOT) if k not in padding]      # ... and every other k its own (plane, ky, kx)
    assert taps == [(p, ky, kx) for p in range(7) for ky in range(7) for kx in range(7)]


def test_the_padding_rule_of_tab_is_the_kernels():
    """fails when the block is rewritten: restate it in tests/_frame_ops.py::stem_tab then"""
    block = re.search(r'for \(int k = tid; k < ST_KTOT; k \+= 256\) \{(.*?)tab\[k\] = off;', _src('stem.hip'), re.S).group(1)
    code = re.sub(r'//[^\n]*', '', block)
    m = re.search(r'int off = ([^;]+);\s*if \(kk < cin \* 49\) \{\s*const int c = kk / 49, r = kk - c \* 49;\s*'
                  r'off = \(3 \* s \+ c\) \* ST_PS \+ \(r / 7\) \* ST_PW \+ \(r % 7\);\s*\}', code)
    assert m, code
    assert m.group(1).strip() == P.STEM_TAB_PADDING
    assert 'const int s = (k >= 296) ? 2 : ((k >= 148) ? 1 : 0);' in code and 'const int cin = (s == 2) ? 1 : 3;' in code


def test_the_stem_plan_at_its_edges():
    for h, b8 in P.STEM_AUTO:
        p = P.stem_plan(1, h, 5)
        assert p['blocks8'] == b8 and p['rows16'] == (b8 in (769, 1536)), (h, p)
        assert p['grid'] == (P.cdiv(h, 16) if p['rows16'] else b8)
    # (W = 768 has 24 tile columns and reaches multiples of 24 only: 768 and 1536 but neither 769 nor 1537; one tile column reaches all four)
    assert [P.stem_plan(1, h, 768)['blocks8'] for h in (256, 257, 512, 513)] == [768, 792, 1536, 1560]
    assert P.stem_plan(1, 512, 512)['rows16'] and not P.stem_plan(1, 544, 960)['rows16']                   # 1024 and 2040 workgroups
    for c in P.STEM_CASES:
        p = P.stem_plan(c.N, c.H, c.W, c.knob)
        assert p['rows16'] == (c.knob == 16 or c.name in ('auto_769', 'auto_1536')), c.name
        assert c.N * c.H * c.W <= 70000, c.name
    assert P.stem_plan(1, 17, 40, 8)['grid'] == 6 and P.stem_plan(1, 17, 40, 16)['grid'] == 4


# ---------------------------------------------------------------------------------------------------------------------
# the heads' order and designed inputs

def test_the_xcd_affine_order_visits_every_workgroup_once():
    for c in P.HEADS_CASES:
        nh = len(c.cout)
        p = P.heads_plan(c.N, c.H, c.W, nh)
        seen = sorted(P.heads_order2(b, p['nblocks'], nh) for b in range(p['nblocks']))
        assert seen == [(h, t) for h in range(nh) for t in range(p['per_head'])], c.name
    p = P.heads_plan(1, 12, 40, 5)
    assert (p['nblocks'], p['per'], p['per_head'], p['straddles']) == (45, 5, 9, True)
    assert [P.heads_order2(b, 45, 5) for b in (40, 44)] == [(4, 4), (4, 8)]            # the last five keep their place
    assert P.heads_plan(2, 5, 17, 8)['nblocks'] == 64 and not P.heads_plan(2, 5, 17, 8)['straddles']


def test_the_heads_cases_are_what_they_were_built_to_be():
    widths = set()
    for c in P.HEADS_CASES:
        assert len(c.cout) == len(c.coff) <= P.CT_MAX_FUSED_HEADS
        spans = sorted(zip(c.coff, c.cout))
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= c.ctot, c.name
        widths |= set(c.cout)
        d = P.heads_inputs(c.name)
        for i in range(len(c.cout)):
            hid = torch.nn.functional.conv2d(d['x'].double(), d['w0'][i].double(), padding=1) + d['b0'][i].double().view(1, 256, 1, 1)
            assert bool((hid[:, P.HIDDEN_DEAD] < 0).all()) and bool((hid[:, P.HIDDEN_LIVE] > 0).all()), (c.name, i)
            assert bool((hid[:, 64:] < 0).any()) and bool((hid[:, 64:] > 0).any())
    assert widths == set(range(1, 9))
    e = P.HEADS_CASE['eight']
    assert P.heads_unowned(e).nonzero()[0].tolist() == [18, 19, 38, 39] and e.sig not in (None, 0) and e.dep not in (None, e.sig)
    r64 = P.heads_refs('eight')[0]
    gap = torch.from_numpy(P.heads_unowned(e))
    assert bool(torch.isnan(r64[:, gap]).all()) and not bool(torch.isnan(r64[:, ~gap]).any())


# ---------------------------------------------------------------------------------------------------------------------
# the references against the oracle

def test_the_flip_reference_is_the_oracles_on_disjoint_pairs():
    from oracle import detector as odet
    assert tuple(map(tuple, odet.COCO_FLIP_IDX)) == P.COCO_PAIRS
    c = P.FLIP_CASE['eight']
    for src, (C, mode), want in zip(P.flip_inputs('eight'), c.heads, P.flip_reference('eight')):
        t = torch.from_numpy(np.array(src))
        a, f = t[:c.B], t[c.B:]
        if mode == P.FLIP_NEG_EVEN:
            ft = torch.flip(f, [3]).clone()
            ft[:, 0::2] *= -1
        elif mode in (P.FLIP_JOINTS, P.FLIP_JOINT_OFFSETS):
            ft = odet.mirror_joints(f, odet.COCO_FLIP_IDX, mode == P.FLIP_JOINT_OFFSETS)
        else:
            ft = torch.flip(f, [3])
        np.testing.assert_array_equal(((a + ft) / 2).numpy(), want)
    chained = P.FLIP_CASE['chained']                           # successive swaps of (0,1), (1,2), (0,3): a 4-cycle, not an involution
    idx = list(range(4))
    for u, v in chained.pairs:
        idx[u], idx[v] = idx[v], idx[u]
    assert idx == [3, 2, 0, 1]
    src = P.flip_inputs('chained')[0]
    np.testing.assert_array_equal(P.flip_reference('chained')[0], (src[:1] + src[1:, idx, :, ::-1]) / np.float32(2))


def test_the_flip_plans():
    plans = {c.name: P.flip_plan(c) for c in P.FLIP_CASES}
    assert [n for n, p in plans.items() if p['vec']] == ['eight', 'chained', 'cap_vec']
    assert plans['eight']['grid_x'] == 5 and plans['cap_vec']['grid_x'] == plans['cap_scalar']['grid_x'] == 4096
    for name, c in (('cap_vec', 4), ('cap_scalar', 1)):
        k = P.FLIP_CASE[name]
        assert k.B * k.h * k.w == c * (2 ** 20 + 1)            # the smallest total past the cap
    assert P.img_plan(P.IMG_CASE['img_cap_vec'])['capped'] and P.img_plan(P.IMG_CASE['img_cap_scalar'])['capped']
    assert not P.img_plan(P.IMG_CASE['img_vec'])['capped']


def test_the_pre_hm_reference_on_known_values():
    r = P.phm_reference('p_1x1')
    assert r.shape == (1, 1, 1, 1) and r[0, 0, 0, 0] == 1.0                             # r = 0 on the pixel; the r = 3 row is past counts
    c = P.PHM_CASE['p_8x32']
    r = P.phm_reference('p_8x32')
    assert r.shape == (6, 1, 8, 32) and not r[0].any() and not r[3].any() and r[1].any()
    np.testing.assert_array_equal(r[3:], r[:3, :, :, ::-1])
    cx, cy, rad = P.phm_live(c, 1)[0]
    assert r[1, 0, cy, cx] == 1.0
    if rad > 0 and cx + 1 < c.W:
        assert r[1, 0, cy, cx + 1] == np.float32(np.exp(-1.0 / (2 * ((2 * rad + 1) / 6.0) ** 2)))
    assert [P.phm_plan(P.PHM_CASE['p_40x72'], b)['rounds'] for b in (0, 1)] == [1, 3] and P.phm_plan(P.PHM_CASE['p_9x33'], 0) == dict(n=257, rounds=2, grid=4)
    assert P.phm_reference('p_40x72')[1, 0, 35, 60] == 1.0                               # the last row of the third round shows


def test_the_pose_reference_restated_is_the_oracles_and_the_designs_hold():
    for c in P.POSE_CASES:
        want, again = P.pose_want(c.name), P.pose_reference(c.name, 'restated')
        assert sorted(want) == sorted(again)
        for k in want:
            np.testing.assert_array_equal(want[k], again[k], err_msg='%s.%s' % (c.name, k))
        hm = torch.from_numpy(np.array(P.pose_maps(c.name)['hm']))
        from oracle import decode as od
        assert int((od.nms(hm) > 0.25).flatten(1).sum(1).min()) >= c.K, c.name                     # K NMS survivors exist
        kps = od.transpose_and_gather_feat(torch.from_numpy(np.array(P.pose_maps(c.name)['hps'])), torch.from_numpy(want['inds'])).view(c.B, c.K, -1).clone()
        kps[..., 0::2] += torch.from_numpy(want['xs']).view(c.B, c.K, 1)
        kps[..., 1::2] += torch.from_numpy(want['ys']).view(c.B, c.K, 1)
        snapped = (kps.numpy() != want['hps'])[..., 0::2]
        if c.designed:
            assert not snapped[..., 3].any()
            snapped = np.delete(snapped, 3, axis=-1)
        assert 0.05 < snapped.mean() < 0.98, (c.name, snapped.mean())                               # the gate decides both ways
    want = P.pose_want('k128_designed')
    assert (want['xs'][0, 0], want['ys'][0, 0], want['scores'][0, 0]) == (10.0, 10.0, np.float32(0.99))
    np.testing.assert_array_equal(want['bboxes'][0, 0], np.array([4.5, 4.5, 16.5, 16.5], np.float32))
    for j, (xy, why) in P.POSE_WANT.items():
        np.testing.assert_array_equal(want['hps'][0, 0, 2 * j:2 * j + 2], np.array(xy, np.float32), err_msg=why)


# ---------------------------------------------------------------------------------------------------------------------
# the mutations

def test_every_mutation_the_issue_names_is_there():
    assert {f: len(m) for f, m in P.MUTATIONS.items()} == dict(stem=4, heads=4, flip=3, pre_hm=3, pose=3)
    assert sorted(P.MUTATION_CASE) == sorted((f, l) for f, m in P.MUTATIONS.items() for l in m)


@pytest.mark.parametrize('letter', list(P.STEM_MUTATIONS))
def test_stem_mutation_leaves_the_bound(letter):
    c = P.STEM_CASE[P.MUTATION_CASE[('stem', letter)]]
    r64, e32, b = P.stem_refs(c.N, c.H, c.W, c.mask, bool(c.add))
    e = P.err(P.mutated('stem', letter), r64)
    print('stem %s on %s: err %.3e e32 %.3e bound %.3e' % (letter, c.name, e, e32, b))
    assert e32 <= b < e, (letter, e, e32, b)


@pytest.mark.parametrize('letter', list(P.HEADS_MUTATIONS))
def test_heads_mutation_leaves_the_bound(letter):
    name = P.MUTATION_CASE[('heads', letter)]
    rows = P.heads_errors(name, P.mutated('heads', letter))
    print('heads %s on %s: %s' % (letter, name, ['%.2e/%.2e' % (e, b) for _, e, _, b in rows]))
    assert all(e32 <= b for _, _, e32, b in rows)
    assert any(e > b for _, e, _, b in rows), rows


@pytest.mark.parametrize('family,letter', [(f, l) for f in ('flip', 'pre_hm', 'pose') for l in P.MUTATIONS[f]])
def test_exact_mutation_differs_on_its_case(family, letter):
    name, wrong = P.MUTATION_CASE[(family, letter)], P.mutated(family, letter)
    if family == 'flip':
        assert any(not np.array_equal(a, b) for a, b in zip(wrong, P.flip_reference(name)))
    elif family == 'pre_hm':
        d = P.ulps(np.nan_to_num(wrong), P.phm_reference(name))
        assert d.max() > 1                                      # (past the one ulp the GPU test grants)
    else:
        want = P.pose_want(name)
        assert not np.array_equal(wrong['hps'], want['hps'])
        assert all(np.array_equal(wrong[k], want[k]) for k in want if k not in ('hps', 'kps_score'))
        if name == 'k128_designed':
            j = {'a': 2, 'b': 0}[letter]
            assert not np.array_equal(wrong['hps'][0, 0, 2 * j:2 * j + 2], np.array(P.POSE_WANT[j][0], np.float32))
