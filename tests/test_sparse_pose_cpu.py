"""CPU: sparse pose heads (opt.sparse_pose_heads, ct_decode_pose_sparse) as far as they go without a GPU -- the test reference's own
flip merge against the oracle's, the row layout, the ctypes mirror of ct_pose_sparse_desc, and every argument error of the
two entry points (they all return before the first launch)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _sparse_pose as SP

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.mark.parametrize('J,pairs', [(17, SP.COCO_PAIRS), (4, [(0, 1), (2, 3)]), (4, SP.OVERLAPPING_PAIRS), (1, [])])
def test_point_merge_equals_the_oracles_merged_map_at_the_points(J, pairs):
    """the reference the GPU tests trust: merging hps point by point == gathering the map the oracle merges
    (flip_output -> mirror_joints(offsets=True)), exactly, in float64 -- also for pairs that share a joint, where both follow
    the reference's successive in-place swaps (utils.py:47-49) and a swap from a snapshot gives another map"""
    from oracle import detector as odet
    g = torch.Generator().manual_seed(J)
    B, h, w, K = 2, 7, 10, 30
    m = torch.randn((2 * B, 2 * J, h, w), generator=g, dtype=torch.float64)
    inds = torch.stack([torch.randperm(h * w, generator=g)[:K] for _ in range(B)])
    inds[:, 0], inds[:, 1] = 0, w - 1                                   # both ends of a row: the mirrored border
    imgs = torch.arange(B).view(B, 1).expand(B, K).reshape(-1)
    got = SP.merge_points(SP.gather_points(m, imgs, inds.reshape(-1)), SP.gather_points(m, imgs + B, inds.reshape(-1), mirror=True), pairs)
    for b in range(B):
        merged = odet.flip_output({'hps': torch.stack((m[b], m[B + b]))}, [list(p) for p in pairs])['hps']
        want = SP.gather_points(merged, torch.zeros(K, dtype=torch.long), inds[b])
        assert torch.equal(got[b * K:(b + 1) * K], want)


def test_pairs_that_share_a_joint_are_swapped_one_after_the_other():
    """[(0, 1), (1, 2), (0, 3)] worked by hand: [0,1,2,3] -> [1,0,2,3] -> [1,2,0,3] -> [3,2,0,1], so the merged joint j reads the
    mirrored joint (3, 2, 0, 1)[j]; swapping from a snapshot would give (3, 2, 1, 0)"""
    from oracle import detector as odet
    b = torch.arange(1.0, 9.0, dtype=torch.float64).view(1, 8)
    got = SP.merge_points(torch.zeros((1, 8), dtype=torch.float64), b, SP.OVERLAPPING_PAIRS) * 2
    want = torch.tensor([[-7.0, 8.0, -5.0, 6.0, -1.0, 2.0, -3.0, 4.0]], dtype=torch.float64)
    assert torch.equal(got, want)
    m = odet.mirror_joints(b.view(1, 8, 1, 1), [list(p) for p in SP.OVERLAPPING_PAIRS], True)
    assert torch.equal(m.view(1, 8), want)


def test_row_layout_equals_the_dense_pose_layout():
    from centertrack_amd import ops
    J, h, w = 17, 8, 8
    hm_hp, hps = torch.zeros((1, J, h, w)), torch.zeros((1, 2 * J, h, w))
    box = {'wh': torch.zeros((1, 2, h, w)), 'reg': torch.zeros((1, 2, h, w)), 'tracking': torch.zeros((1, 2, h, w))}
    dense = dict(box, hps=hps, hm_hp=hm_hp, hp_offset=torch.zeros((1, 2, h, w)))
    want = ops.Decoder.row_floats(dense)
    assert want == 4 + 4 + 2 + 2 * J + 1
    # the main heads as maps, hps / offset sparse; and all of them sparse
    assert ops.Decoder.row_floats(dict(box, hm_hp=hm_hp), None, {}) == want
    assert ops.Decoder.row_floats({'hm_hp': hm_hp}, ['reg', 'wh', 'tracking'], {}) == want
    assert ops.Decoder.row_floats({'hm_hp': hm_hp}, None, {}) == 4 + 2 * J + 1                      # the box-less head set
    lay, F0 = ops.decode_layout(['reg', 'wh', 'tracking'])
    assert F0 == 10 and [n for n, _, _ in lay] == ['scores', 'clses', 'xs', 'ys', 'bboxes', 'tracking']


def test_default_opt_has_the_flag_and_it_is_off():
    from centertrack_amd import weights as W
    from centertrack_amd.detector import default_opt
    assert default_opt(W.POSE_HEADS).sparse_pose_heads is False
    assert default_opt(W.POSE_HEADS, sparse_pose_heads=True).sparse_pose_heads is True


def test_ctypes_mirror_of_the_descriptor_matches_the_header(tmp_path):
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [n for n, _ in _lib.PoseSparseDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ct_pose_sparse_desc));']
    lines += ['printf("%s %%zu\\n", offsetof(ct_pose_sparse_desc, %s));' % (f, f) for f in fields]
    lines += ['return 0; }']
    src = tmp_path / 'lay.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.PoseSparseDesc)
    for f in fields:
        assert int(got[f]) == getattr(_lib.PoseSparseDesc, f).offset, f
    assert _lib.PoseSparseDesc.base.offset == 0 and _lib.PoseSparseDesc.base.size == ctypes.sizeof(_lib.PoseDesc)


def _valid_desc(keep):
    """a descriptor both entry points accept as far as the host checks go (host memory stands in for every pointer)"""
    from centertrack_amd import _lib
    buf = np.zeros(4096, np.float32)
    keep.append(buf)
    p = buf.ctypes.data
    assert p % 16 == 0
    d = _lib.PoseSparseDesc()
    b = d.base
    b.rows = b.inds = b.hm_hp = b.out = p
    b.row_floats, b.box_col = 8 + 35, 4
    b.B, b.h, b.w, b.K, b.num_joints = 2, 16, 24, 20, 17
    d.feat, d.ldf, d.flip_B = p, 64, 0
    d.hps_w1 = d.hps_b1 = d.hps_w2 = d.hps_b2 = p
    d.off_w1 = d.off_b1 = d.off_w2 = d.off_b2 = p
    pairs = np.asarray(SP.COCO_PAIRS, np.int32)
    keep.append(pairs)
    d.flip_pairs, d.num_pairs = pairs.ctypes.data, len(pairs)
    return d, p


BAD = {
    'null feat': lambda d, p: setattr(d, 'feat', None),
    'misaligned feat': lambda d, p: setattr(d, 'feat', p + 4),
    'ldf below 64': lambda d, p: setattr(d, 'ldf', 60),
    'no joints': lambda d, p: setattr(d.base, 'num_joints', 0),
    '33 joints': lambda d, p: setattr(d.base, 'num_joints', 33),
    'hps map beside the weights': lambda d, p: setattr(d.base, 'hps', p),
    'offset map beside the weights': lambda d, p: setattr(d.base, 'hp_offset', p),
    'flip_B neither 0 nor B': lambda d, p: setattr(d, 'flip_B', 1),
    'flip_B without pairs': lambda d, p: (setattr(d, 'flip_B', 2), setattr(d, 'flip_pairs', None)),
    'half an offset head': lambda d, p: setattr(d, 'off_w2', None),
    'no hps weights': lambda d, p: setattr(d, 'hps_w1', None),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_argument_errors_return_before_any_launch(what):
    from centertrack_amd import _lib
    lib = _lib.load()
    keep = []
    d, p = _valid_desc(keep)
    need = ctypes.c_size_t(123)
    assert lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == _lib.CT_OK and need.value > 0
    ok = need.value
    d.flip_B = 2                                                         # (the flip pass adds its partial buffer)
    assert lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == _lib.CT_OK and need.value > ok
    d.flip_B = 0
    BAD[what](d, p)
    assert lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == _lib.CT_ERR_ARG, what
    assert need.value == 0 and lib.ct_last_error()
    assert lib.ct_decode_pose_sparse(ctypes.byref(d), None) == _lib.CT_ERR_ARG, what


def test_a_small_workspace_is_refused_before_any_launch():
    from centertrack_amd import _lib
    lib = _lib.load()
    keep = []
    d, p = _valid_desc(keep)
    d.base.workspace, d.base.workspace_bytes = p, 256
    assert lib.ct_decode_pose_sparse(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    assert lib.ct_decode_pose_sparse_workspace_bytes(ctypes.byref(d), None) == _lib.CT_ERR_ARG
