"""CPU: the sparse heads of both tasks as far as they go without a GPU -- the case tables of tests/_sparse_heads.py and
tests/_sparse_pose.py reach every regime of the launch arithmetic, the seeded inputs really hold the edges they were built for
(judged with the oracle's own NMS / top-K), the references agree with the oracle, and the two workspace queries equal the tables'
own formulas (host code only: no call here launches a kernel)."""
import ctypes

import numpy as np
import pytest
import torch

import _sparse_heads as SH
import _sparse_pose as SP


def test_the_cases_reach_every_regime_of_the_kernels():
    got = set()
    for c in SH.CASES:
        got |= SH.regimes(c)
    assert sorted(got) == SH.MAIN_REGIMES
    got = set()
    for c in SP.CASES:
        got |= SH.pose_regimes(c)
    assert sorted(got) == SH.POSE_REGIMES
    assert len(set(c.name for c in SH.CASES)) == len(SH.CASES) and len(set(c.name for c in SP.CASES)) == len(SP.CASES)
    assert max(SH.ldf(c) for c in SH.CASES) == 256 and all(SH.ldf(c) % 4 == 0 and c.c0 % 4 == 0 for c in SH.CASES)


def test_the_pose_jobs_start_where_the_table_says():
    """tile0 of every job and the grid, case by case (ct_decode_pose_sparse: tile0 = tiles so far, 4 workgroups per tile)"""
    want = {'b1_hp_offset_wh': ([(20, 34, 0), (340, 2, 2)], 24), 'b2_reg_wh_flip': ([(74, 34, 0), (74, 34, 5), (1258, 2, 10)], 89),
            'b3_boxless_k100': ([(300, 34, 0)], 19), 'k1_three_jobs': ([(3, 8, 0), (3, 8, 1), (12, 2, 2)], 3),
            'j32_full_tiles_pitch256': ([(16, 64, 0), (512, 2, 1)], 33)}
    for c in SP.CASES:
        if c.name in want:
            assert SH.pose_jobs(c) == want[c.name], c.name
        assert all(ch <= 64 for _, ch, _ in SH.pose_jobs(c)[0])


def test_the_head_table_is_the_librarys():
    from centertrack_amd import _lib
    assert SH.HEAD_CH == _lib.HEAD_CH and [_lib.HEAD_INDEX[n] for n in SH.ALL_HEADS] == list(range(len(SH.ALL_HEADS)))


@pytest.mark.parametrize('c', SH.CASES, ids=[c.name for c in SH.CASES])
def test_main_inputs_hold_the_edges_they_were_built_for(c):
    """winners (the oracle's _nms / _topk restatement, documented tie order) on row 0, on column 0 and on column w-1, and for
    C >= 2 pixels that win in two classes of one image; the float64 and the float32 reference select the same winners"""
    cls, ys, xs = SH.winners(c)
    r64 = SH.reference(c, torch.float64)
    for k in ('scores', 'clses', 'xs', 'ys', 'inds'):
        assert torch.equal(r64[k].double(), SH.reference(c, torch.float32)[k].double()), k
    if c.K >= 16:
        assert (ys == 0).any() and (xs == 0).any() and (xs == c.w - 1).any()
    else:
        assert c.h == 1 and bool((ys == 0).all())
    if c.C >= 2:
        for b in range(c.B):
            pix = (ys[b] * c.w + xs[b]).tolist()
            twice = set(p for p in pix if pix.count(p) > 1)
            assert twice >= set(y * c.w + x for y, x in SH.spots(c)) and len(SH.spots(c)) >= 2, (c.name, b)
    # the rows show every head of the case: a field of its own, or the box it is the last to write (reg only moves the wh box)
    shown = set(k for k in r64 if k not in SH.INTEGER_FIELDS + ('inds',) and float(r64[k].abs().max()) > 0)
    for n in c.heads:
        if n in ('wh', 'ltrb', 'ltrb_amodal', 'reg'):
            hidden = {'wh': ('ltrb', 'ltrb_amodal'), 'ltrb': ('ltrb_amodal',), 'ltrb_amodal': (), 'reg': ('ltrb', 'ltrb_amodal')}[n]
            assert 'bboxes' in shown and (n != 'reg' or 'wh' in c.heads)
            assert any(h in c.heads for h in hidden) or float((r64['bboxes'][..., 2:] - r64['bboxes'][..., :2]).abs().max()) > 0
        else:
            assert n in shown or (n == 'tracking' and c.zero_tracking), n
    # the scores above zero are distinct: the order of the winners owes nothing to a tie rule except among suppressed zeros
    for b in range(c.B):
        s = r64['scores'][b]
        s = s[s > 0]
        assert len(torch.unique(s)) == len(s)


def test_every_head_is_the_one_the_rows_show_in_some_case():
    """ltrb overwrites the wh box and ltrb_amodal both (decode.py:131-159), reg only moves the wh box: each of the four must be
    what the box columns hold in some case, with and without flip for wh; every other head is a field wherever it is listed"""
    box = lambda c: 'ltrb_amodal' if 'ltrb_amodal' in c.heads else 'ltrb' if 'ltrb' in c.heads else 'wh' if 'wh' in c.heads else None
    assert set(box(c) for c in SH.CASES) >= {'wh', 'ltrb', 'ltrb_amodal'}
    assert any(box(c) == 'wh' and c.flip for c in SH.CASES) and any(box(c) == 'wh' and 'reg' in c.heads for c in SH.CASES)
    assert any(box(c) == 'wh' and 'reg' in c.heads and c.flip for c in SH.CASES)
    for flip in (False, True):
        assert set(n for c in SH.CASES if c.flip == flip for n in c.heads) == set(SH.ALL_HEADS) - ({'ltrb_amodal'} if flip else set())


def test_main_inputs_edges_over_the_table():
    """every border is reached by a winner in some case of every flip setting"""
    for flip in (False, True):
        seen = set()
        for c in SH.CASES:
            if c.flip == flip:
                _, ys, xs = SH.winners(c)
                seen |= {k for k, v in (('row 0', ys == 0), ('column 0', xs == 0), ('column w-1', xs == c.w - 1)) if bool(v.any())}
        assert seen == {'row 0', 'column 0', 'column w-1'}, (flip, seen)


def test_the_main_reference_is_the_gather_of_its_maps():
    """generic_decode of the float64 maps == the maps gathered at the winners, field by field through ops.decode_layout (the rows
    the GPU test unpacks have this layout): bboxes from reg / wh, tracking as it is"""
    from centertrack_amd import ops
    c = SH.CASE['flip_test']
    r = SH.reference(c, torch.float64)
    maps = SH.head_maps(c, torch.float64)
    lay, F = ops.decode_layout(c.heads)
    assert [n for n, _, _ in lay] == ['scores', 'clses', 'xs', 'ys', 'bboxes', 'tracking', 'dep', 'dim', 'amodel_offset'] and F == 16
    b = torch.arange(c.B).view(-1, 1)
    at = lambda n: maps[n][b, :, r['ys'].long(), r['xs'].long()]
    assert torch.equal(r['tracking'], at('tracking')) and torch.equal(r['dim'], at('dim')) and torch.equal(r['dep'], at('dep'))
    xs, ys, wh = r['xs'] + at('reg')[..., 0], r['ys'] + at('reg')[..., 1], at('wh').clamp(min=0)
    box = torch.stack((xs - wh[..., 0] / 2, ys - wh[..., 1] / 2, xs + wh[..., 0] / 2, ys + wh[..., 1] / 2), -1)
    assert torch.equal(r['bboxes'], box)
    # the flip merge: mode 1 and mode 2 against their definitions at one winner on column 0 (its mirror is column w-1)
    d = SH.make_case(c)
    k = int((r['xs'][0] == 0).nonzero()[0])
    y = int(r['ys'][0, k])
    for n, *wts in d['heads']:
        if n in ('dim', 'amodel_offset'):
            m = SH.head_map(d['feat'], wts, torch.float64)
            other = m[c.B, :, y, c.w - 1].clone()
            if n == 'amodel_offset':
                other[0::2] *= -1
            assert torch.equal(r[n][0, k], (m[0, :, y, 0] + other) / 2), n


@pytest.mark.parametrize('c', SP.CASES, ids=[c.name for c in SP.CASES])
def test_pose_inputs_hold_the_edges_they_were_built_for(c):
    """winners on row 0 and joint peaks on the first and on the last column; from K = 20 on (the lifted pixels saturate at
    0.999 and equal scores rank lower pixel first: row 0 takes the first places) winners on both columns as well"""
    from oracle import decode as odecode
    from _decode_paths import documented_tie_order
    d = SP.make_case(c)
    with documented_tie_order():
        _, inds, _, ys, xs = odecode.topk(odecode.nms(d['hm']), K=c.K)
        _, jinds, _, jxs = odecode.topk_channel(odecode.nms(d['hm_hp']), K=c.K)
    assert (ys == 0).any()
    assert (jxs == 0).any() and (jxs == c.w - 1).any()
    if c.K >= 20:
        assert (xs == 0).any() and (xs == c.w - 1).any()
    if SP.weak_joint(c) is not None:
        assert float(d['hm_hp'][:, SP.weak_joint(c)].max()) <= 0.2
    else:
        assert c.J <= SP.WEAK_JOINT


@pytest.mark.parametrize('c', SH.CASES, ids=[c.name for c in SH.CASES])
def test_decode_workspace_with_a_sparse_descriptor_equals_the_table(c):
    """ct_decode_workspace_bytes: the selection's bytes, then keys B*K*8, then partials B*ceil(K/16)*nheads*2*4*16*8*4"""
    from centertrack_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert p % 16 == 0
    d = _lib.DecodeDesc()
    d.hm = d.out = p
    d.B, d.C, d.h, d.w, d.K = c.B, c.C, c.h, c.w, c.K
    dense = lib.ct_decode_workspace_bytes(ctypes.byref(d))
    sp = _lib.SparseHeadsDesc()
    sp.feat, sp.ldf, sp.nheads, sp.flip_B = p + 4 * c.c0, SH.ldf(c), len(c.heads), c.B if c.flip else 0
    for i, n in enumerate(c.heads):
        sp.head[i] = _lib.HEAD_INDEX[n]
        sp.w1[i] = sp.b1[i] = sp.w2[i] = sp.b2[i] = p
    d.sparse = ctypes.pointer(sp)
    sel, keys, partials = SH.workspace_bytes(c)
    assert dense == sel
    assert keys == c.B * c.K * 8 and partials == c.B * -(-c.K // 16) * len(c.heads) * 2 * 4 * 16 * 8 * 4
    assert lib.ct_decode_workspace_bytes(ctypes.byref(d)) == sel + keys + partials
    assert lib.ct_decode_row_floats(ctypes.byref(d)) == 4 + sum(wd for _, _, wd in _layout(c)[4:])


def _layout(c):
    from centertrack_amd import ops
    return ops.decode_layout(c.heads)[0]


@pytest.mark.parametrize('c', SP.CASES, ids=[c.name for c in SP.CASES])
def test_pose_workspace_carve_equals_the_table(c):
    from centertrack_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    pairs = np.ascontiguousarray(c.pairs, np.int32).reshape(-1, 2)
    d = _lib.PoseSparseDesc()
    b = d.base
    b.rows = b.inds = b.hm_hp = b.out = p
    b.row_floats, b.box_col = 8 + 2 * c.J + 1, 4
    b.B, b.h, b.w, b.K, b.num_joints = c.B, c.h, c.w, c.K, c.J
    d.feat, d.ldf, d.flip_B = p + 4 * c.c0, c.c0 + 64 + c.pad, c.B if c.flip else 0
    d.hps_w1 = d.hps_b1 = d.hps_w2 = d.hps_b2 = p
    if c.offset:
        d.off_w1 = d.off_b1 = d.off_w2 = d.off_b2 = p
    d.flip_pairs, d.num_pairs = pairs.ctypes.data, len(pairs)
    need = ctypes.c_size_t(0)
    assert lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == _lib.CT_OK, lib.ct_last_error()
    assert need.value == SH.pose_workspace_bytes(c)
