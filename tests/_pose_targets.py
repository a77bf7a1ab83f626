"""Shared by test_pose_targets_cpu.py and test_hip_pose_targets.py: the golden samples of tests/golden/pose_targets.npz
(written by tests/golden/make_pose_targets_golden.py from the reference's own ``GenericDataset.__getitem__`` with the
pose heads), the builders they need, synthetic cases beyond the goldens, the regime table of the pose side of
csrc/targets.hip and the comparison of a rendered batch with the reference's (the bounds of test_hip_targets.py)."""
import json
import os

import numpy as np

import _targets as T

GOLDEN = os.path.join(T.ROOT, 'tests', 'golden', 'pose_targets.npz')
CASES = ('P1', 'P2', 'P3')
J = 17
JOINT_KEYS = ('hm_hp_mask', 'hp_offset', 'hp_ind', 'hp_offset_mask', 'joint')
MAP_KEYS = ('hm', 'hm_hp', 'pre_hm')
MAX_DIFF, MAX_UNEQUAL = 1e-6, 1e-4           # test_hip_targets.py: float64 exp on the device against libm
# the out= subsets test_hip_pose_targets.py asks for
OUT_SUBSETS = {'hm_hp alone': ('hm_hp',), 'joint tensors without hm_hp': JOINT_KEYS + ('hps', 'hps_mask')}


def builder(cfg):
    from centertrack_amd.targets import PoseTargetBuilder
    opt = T.make_opt(cfg['heads'], cfg['num_classes'], tuple(cfg['out_hw']), cfg['tracking'], cfg['pre_hm'],
                     tuple(cfg['disturb']))
    cat_ids = {int(k): v for k, v in cfg['cat_ids'].items()}
    return PoseTargetBuilder(opt, cfg['num_classes'], cfg['max_objs'], cat_ids, num_joints=cfg['num_joints']), opt


class Golden(object):
    """the file, parsed once (the layout of targets.npz)"""

    def __init__(self):
        g = np.load(GOLDEN)

        def one(k):
            return g[k].reshape(-1)[0]

        self.cases = {}
        for c in CASES:
            cfg = json.loads(str(one(c + '/cfg')))
            samples = []
            for i in range(int(one(c + '/n'))):
                pre = '%s/%d/' % (c, i)
                s = json.loads(str(one(pre + 'in')))
                s['trans'], s['noise'] = g[pre + 'trans'], g[pre + 'noise']
                if cfg['tracking']:
                    s['rng'] = (g[pre + 'rng_key'], int(one(pre + 'rng_pos')), g[pre + 'rng_gauss'],
                                float(one(pre + 'rng_next')))
                s['ret'] = {k[len(pre) + 4:]: g[k] for k in g.files if k.startswith(pre + 'ret/')}
                samples.append(s)
            self.cases[c] = {'cfg': cfg, 'samples': samples, 'empty': int(one(c + '/empty')) if c == 'P1' else None}

    encode = T.Golden.encode


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = Golden()
    return _GOLDEN


# ---- cases beyond the goldens ------------------------------------------------------------------------------------
def synth_builder(C, out_hw, max_objs, pre_hm=True):
    from centertrack_amd.targets import PoseTargetBuilder
    heads = ('hm', 'reg', 'wh', 'hps', 'hm_hp', 'hp_offset') + (('tracking',) if pre_hm else ())
    opt = T.make_opt(heads, C, out_hw, pre_hm, pre_hm)
    return PoseTargetBuilder(opt, C, max_objs, {i: i for i in range(1, C + 1)}), opt


def with_joints(rs, anns, inp_hw, vis=(2,), spread=0.0):
    """key points uniform over each box (widened by `spread`), clipped into the image when spread is 0"""
    H, W = inp_hw
    for a in anns:
        x, y, w, h = a['bbox']
        kp = []
        for _ in range(J):
            px, py = rs.uniform(x - spread * w, x + (1 + spread) * w), rs.uniform(y - spread * h, y + (1 + spread) * h)
            if spread == 0:
                px, py = min(max(px, 0.0), W - 0.5), min(max(py, 0.0), H - 0.5)
            kp += [float(px), float(py), int(vis[rs.randint(len(vis))])]
        a['keypoints'] = kp
    return anns


def case_pe():
    """128 x 128 / 512 x 512, B = 2, 1 class, 32 persons with all 17 joints visible and inside: 576 blobs per image"""
    tb, opt = synth_builder(1, (128, 128), 32)
    rs = np.random.RandomState(151)
    recs = []
    for _ in range(2):
        anns = T.synth_anns(rs, 32, 1, (512, 512), 0.3)
        for a in anns:                           # boxes inside the image: no person is dropped
            a['bbox'][0], a['bbox'][1] = max(a['bbox'][0], 0.0), max(a['bbox'][1], 0.0)
        anns = with_joints(rs, anns, (512, 512))
        recs.append(T.synth_record(tb, opt, anns, anns))
    return tb, recs


def case_pf():
    """16 x 24 / 64 x 96: CULL_CAP + 40 persons whose one visible joint lies around pixel (10, 5) of plane C + 0 -- more
    than CULL_CAP blobs over one tile of one hm_hp plane -- next to an empty image"""
    from centertrack_amd import targets
    n = targets.CULL_CAP + 40
    tb, opt = synth_builder(1, (16, 24), n)
    rs = np.random.RandomState(161)
    anns = []
    for i in range(n):
        w, h = rs.uniform(12, 30), rs.uniform(12, 30)
        x, y = 40 - w / 2 + rs.uniform(-1, 1), 20 - h / 2 + rs.uniform(-1, 1)
        kp = [float(40 + rs.uniform(-3, 3)), float(20 + rs.uniform(-3, 3)), 2 - i % 2]
        for j in range(1, J):                    # visible but outside the map: nothing; every eighth person: unlabelled
            kp += [-50.0, 10.0, 2] if i % 8 else [0.0, 0.0, 0]
        anns.append({'bbox': [float(x), float(y), float(w), float(h)], 'category_id': 1, 'track_id': i, 'keypoints': kp})
    return tb, [T.synth_record(tb, opt, anns, anns[:4]), T.synth_record(tb, opt, [], [])]


def case_pg():
    """7 x 33 / 28 x 132, 2 classes: smaller than a tile in y, ragged in x, W mod 4 != 0; joints of every visibility,
    inside and outside"""
    tb, opt = synth_builder(2, (7, 33), 8)
    rs = np.random.RandomState(171)
    recs = []
    for _ in range(2):
        anns = with_joints(rs, T.synth_anns(rs, 6, 2, (28, 132)), (28, 132), vis=(0, 1, 2), spread=0.2)
        recs.append(T.synth_record(tb, opt, anns, anns))
    return tb, recs


def case_ph():
    """B = 1, one radius-0 person with one visible joint"""
    tb, opt = synth_builder(1, (8, 8), 2, pre_hm=False)
    kp = [-9.0, -9.0, 2] * J
    kp[12:15] = [21.0, 6.5, 2]
    rec = T.synth_record(tb, opt, [{'bbox': [13.0, 9.0, 1.0, 1.0], 'category_id': 1, 'keypoints': kp}])
    assert rec['hm_blobs'].tolist() == [[0, 3, 2, 0], [1 + 4, 5, 1, 0]] and len(rec['rects']) == 0
    return tb, [rec]


SYNTH = {'PE': case_pe, 'PF': case_pf, 'PG': case_pg, 'PH': case_ph}


# ---- the regimes of the pose side of build_targets_kernel ----------------------------------------------------------
def hp_tile_load(tb, recs, K):
    """the largest number of blobs of one hm_hp plane of one image whose support touches one tile"""
    best = 0
    for rec in recs:
        b = rec['hm_blobs']
        for plane in range(tb.num_classes, tb.num_classes + tb.num_joints):
            sub = {'hm_blobs': b[b[:, 0] == plane]}
            best = max(best, T.tile_load([sub], 'hm_blobs', (1, 2, 3), (tb.opt.output_h, tb.opt.output_w), K))
    return best


def regimes(K):
    """name -> predicate(tb, records): what the pose side of the kernel and of the host code branches on"""
    def hp_blobs(tb, rec):
        return rec['hm_blobs'][rec['hm_blobs'][:, 0] >= tb.num_classes]

    def hp_rects(tb, rec):
        r = rec['rects']
        return r[(r[:, 0] >= tb.num_classes) | (r[:, 0] == -2)]

    return {
        'hm_hp behind one class plane': lambda tb, r: tb.num_classes == 1,
        'hm_hp behind several class planes': lambda tb, r: tb.num_classes > 1,
        'more than two culling rounds of hm + hm_hp blobs': lambda tb, r: max(int(x['counts'][1]) for x in r) > 2 * K['CAP'],
        'a round that fills the list (CULL_CAP + 1 blobs over one tile of one hm_hp plane)':
            lambda tb, r: hp_tile_load(tb, r, K) >= K['CAP'] + 1,
        'more than one culling round of rectangles': lambda tb, r: max(int(x['counts'][2]) for x in r) > K['CAP'],
        'hm_hp rectangles: one plane and all planes': lambda tb, r: any(
            (x['rects'][:, 0] >= tb.num_classes).any() and (x['rects'][:, 0] == -2).any() for x in r),
        'an ignore region that leaves hm_hp alone': lambda tb, r: any(
            (x['rects'][:, 0] == -1).sum() > (x['rects'][:, 0] == -2).sum() or
            ((x['rects'][:, 0] >= 0) & (x['rects'][:, 0] < tb.num_classes)).any() for x in r),
        'an image without joints': lambda tb, r: any(not len(hp_blobs(tb, x)) and not len(hp_rects(tb, x)) for x in r),
        'hm_hp radius 0': lambda tb, r: any(len(hp_blobs(tb, x)) and hp_blobs(tb, x)[:, 3].min() == 0 for x in r),
        'two joints on one pixel of one plane': lambda tb, r: any(
            len(np.unique(hp_blobs(tb, x)[:, :3], axis=0)) < len(hp_blobs(tb, x)) for x in r),
        'joint rows (max_objs * J) over more than one workgroup': lambda tb, r: tb.max_objs * tb.num_joints > 256,
        'slots: a row that straddles two workgroups': lambda tb, r: tb.slot_words % 256 != 0
            and len(r) * tb.max_objs * tb.slot_words > 256,
        'slots: an image without objects': lambda tb, r: min(int(x['counts'][0]) for x in r) == 0,
        'hm_hp: ragged last tile, row length no multiple of 4': lambda tb, r: tb.opt.output_w % K['TW'] != 0
            and tb.opt.output_w % 4 != 0 and tb.opt.output_h < K['TH'],
        'hm_hp: several tiles on both axes': lambda tb, r: tb.opt.output_h > K['TH'] and tb.opt.output_w > K['TW'],
    }


# ---- a rendered batch against the reference's ----------------------------------------------------------------------
def stack(rets):
    return T.stack(rets)


def check_batch(got, want, what):
    """keys, dtypes, shapes; slot tensors (the joint tensors included) bitwise; per map (name, max |diff|, unequal,
    elements) after the set checks"""
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
