"""Sparse pose heads (ct_decode_pose_sparse, centertrack_amd/csrc/sparse_pose.hip): the case table of tests/test_hip_sparse_pose.py and
its CPU references -- a head evaluated densely on the small map with ``F.conv2d`` (float64 or float32) and gathered at a point
list, and the point-wise flip merge of ``hps``.  No GPU and no product code in here.  tests/_sparse_heads.py holds the
main task's table and the launch arithmetic of both (``pose_regimes``)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

# B, h, w, K, J, offset head ('hp_offset' / 'reg' / None), gate box ('wh' / 'ltrb' / None), flip, joint pairs; the feature map is
# the channel slice [c0, c0 + 64) of a buffer of pitch c0 + 64 + pad whose other channels are NaN
Case = namedtuple('Case', 'name B h w K J offset box flip pairs c0 pad', defaults=(0, 0))
COCO_PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
OVERLAPPING_PAIRS = [(0, 1), (1, 2), (0, 3)]       # pairs that share a joint: successive swaps != swaps from a snapshot
CASES = [Case('b1_hp_offset_wh', 1, 16, 24, 20, 17, 'hp_offset', 'wh', False, COCO_PAIRS),
         Case('b2_reg_wh_flip', 2, 17, 30, 37, 17, 'reg', 'wh', True, COCO_PAIRS),
         Case('b3_boxless_k100', 3, 24, 40, 100, 17, None, None, False, COCO_PAIRS),
         Case('b2_j4_ltrb_flip', 2, 16, 24, 20, 4, 'hp_offset', 'ltrb', True, [(0, 1), (2, 3)]),
         # one joint = 2 output channels; flip_B > 0 with no pair at all
         Case('j1_flip_no_pairs', 2, 16, 24, 20, 1, 'hp_offset', 'wh', True, []),
         # 32 joints = 64 channels, the whole W2 staging and 1024 tail items; B*K = 16 and B*J*K = 512: no ragged tile;
         # a sliced feature map at a wide pitch
         Case('j32_full_tiles_pitch256', 1, 17, 30, 16, 32, 'hp_offset', 'wh', False, COCO_PAIRS, 8, 184),
         # one point per image: B*K = 3 and B*J*K = 12, three jobs of one ragged tile each
         Case('k1_three_jobs', 3, 16, 24, 1, 4, 'reg', 'ltrb', True, OVERLAPPING_PAIRS),
         # pairs that share a joint; B*K = 74 and B*J*K = 296, neither a multiple of 16; a slice at pitch 64 + 8 + 4
         Case('j4_overlapping_pairs_slice', 2, 17, 30, 37, 4, 'hp_offset', 'wh', True, OVERLAPPING_PAIRS, 8, 4)]
CASE = {c.name: c for c in CASES}
WEAK_JOINT = 3            # its peaks are all <= 0.2: the match keeps the regressed joint (cases with J > 3: ``weak_joint``)
K_TERMS = 576 + 256       # terms behind one head value: conv3x3 over 64 channels, then conv1x1 over 256


def weak_joint(c):
    """the joint of the case whose peaks are all <= 0.2, or None where the case has too few joints for one"""
    return WEAK_JOINT if c.J > WEAK_JOINT else None


def head_weights(g, c, gain=1.0):
    """conv3x3 64 -> 256, bias, conv1x1 256 -> c, bias of one head (CPU float32)"""
    return (torch.randn((256, 64, 3, 3), generator=g) * 0.05, torch.randn((256,), generator=g) * 0.1,
            torch.randn((c, 256), generator=g) * 0.05 * gain, torch.randn((c,), generator=g) * 0.1)


def make_case(c):
    """seeded inputs of a case: feature maps of the B (2 B with flip) images, post-sigmoid hm [B,1,h,w] lifted on row 0 and on
    the first and last column, hm_hp [B,J,h,w] lifted on the first and last column (winners and peaks on borders, and with
    flip on the mirrored border), one joint weak; head weights of hps and of the offset head; dense maps of the box heads"""
    g = torch.Generator().manual_seed(1000 + 7 * c.K + c.J)
    NB = 2 * c.B if c.flip else c.B
    d = {'feat': torch.randn((NB, 64, c.h, c.w), generator=g)}
    hm = torch.rand((c.B, 1, c.h, c.w), generator=g)
    hm[:, :, 0, :] += 0.5
    hm[:, :, 1:, 0] += 0.5
    hm[:, :, 1:, -1] += 0.5
    d['hm'] = hm.clamp(0, 0.999)
    hm_hp = torch.rand((c.B, c.J, c.h, c.w), generator=g)
    hm_hp[:, :, :, -1] += 0.5
    hm_hp[:, :, :, 0] += 0.5
    hm_hp = hm_hp.clamp(0, 0.999)
    if weak_joint(c) is not None:
        hm_hp[:, weak_joint(c)] *= 0.15
    d['hm_hp'] = hm_hp
    d['hps'] = head_weights(g, 2 * c.J, gain=1.0 if c.box is None else 4.0)
    d['off'] = head_weights(g, 2) if c.offset else None
    d['maps'] = {}
    if c.box == 'wh':
        d['maps']['wh'] = torch.rand((c.B, 2, c.h, c.w), generator=g) * 10 + 2
        if c.offset == 'reg':                   # (the reg MAP only moves the box; the offsets come from the head's weights)
            d['maps']['reg'] = torch.rand((c.B, 2, c.h, c.w), generator=g)
    elif c.box == 'ltrb':
        d['maps']['ltrb'] = torch.randn((c.B, 4, c.h, c.w), generator=g).abs() * torch.tensor([-3.0, -3.0, 3.0, 3.0]).view(1, 4, 1, 1)
    return d


def head_map(feat, wts, dtype):
    """the head as a dense map [N,c,h,w] in ``dtype``: conv3x3 (zero padding) + bias + ReLU + conv1x1 + bias"""
    w1, b1, w2, b2 = (t.to(dtype) for t in wts)
    return F.conv2d(F.relu(F.conv2d(feat.to(dtype), w1, b1, padding=1)), w2.view(w2.shape[0], 256, 1, 1), b2)


def gather_points(m, imgs, pix, mirror=False):
    """rows [P,c] of the dense map ``m`` at points (image, flat pixel); ``mirror``: at the pixel mirrored left-right"""
    w = m.shape[3]
    y, x = pix // w, pix % w
    if mirror:
        x = w - 1 - x
    return m[imgs, :, y, x]


def merge_points(a, b, pairs):
    """the flip merge of hps at a point: ``a`` [P,2J] from image b at the pixel, ``b`` [P,2J] from the mirrored image at the
    mirrored pixel -> (a + s * b') / 2, b' = the partner joint's pair with x negated (flip_lr_off, utils.py:40-50).  The swaps
    are successive, each on the result of the one before, like the reference's in-place loop over flip_idx (utils.py:47-49)"""
    P = a.shape[0]
    m = b.view(P, -1, 2).clone()
    m[:, :, 0] *= -1
    for u, v in pairs:
        m[:, u], m[:, v] = m[:, v].clone(), m[:, u].clone()
    return (a + m.view(P, -1)) / 2


def hps_at_winners(feat, wts, B, inds, flip, pairs, dtype):
    """reference of the compact hps values [B*K, 2J] at the winners ``inds`` [B,K] (merged under ``flip``)"""
    m = head_map(feat, wts, dtype)
    K = inds.shape[1]
    imgs = torch.arange(B).view(B, 1).expand(B, K).reshape(-1)
    pix = inds.reshape(-1)
    a = gather_points(m, imgs, pix)
    if not flip:
        return a
    return merge_points(a, gather_points(m, imgs + B, pix, mirror=True), pairs)


def offsets_at_peaks(feat, wts, B, J, jinds, dtype):
    """reference of the compact offset values [B*J*K, 2] at the joint peaks ``jinds`` [B*J,K] (image b alone)"""
    m = head_map(feat[:B], wts, dtype)
    K = jinds.shape[1]
    imgs = (torch.arange(B * J) // J).view(-1, 1).expand(B * J, K).reshape(-1)
    return gather_points(m, imgs, jinds.reshape(-1))
