"""Golden vectors of the pose training targets from the reference's own ``GenericDataset.__getitem__`` (build container
only, like make_targets_golden.py, whose ``DS`` / ``Opt`` / ``record`` scaffolding and key layout this generator uses):
tests/golden/pose_targets.npz.

The heads hold ``hps``, ``hm_hp`` and (P1, P3) ``hp_offset``; the annotations carry COCO ``keypoints`` (17 x (x, y, v));
``flip_idx`` is the class default of the reference's ``GenericDataset``.  The annotation lists are recorded as the object
loop saw them: after ``_flip_anns`` mirrored the boxes and mirrored and swapped the key points in place.

Cases (``<case>/cfg`` as JSON, samples as in targets.npz):
  P1  tracking,multi_pose: 1 class, pre_hm, the three disturbances, max_objs 8 of 9-12 annotations, flipped and
      unflipped samples, one empty sample in the middle
  P2  2 classes, detection only, heads without hp_offset; ignore annotations of class id 0, -1, -2 and an iscrowd
      annotation of class 2: rectangles on all / one hm plane with and without the rectangle on all hm_hp planes
  P3  no augmentation (image = network input): a joint at exactly (0, 0), joints whose pixel is on the last column / the
      last row, a radius-0 person, two persons whose same joint falls on one pixel, an annotation without keypoints, a
      person whose clipped box is empty while its key points lie inside the map

Fixed zip timestamps: a second run reproduces the file byte for byte.

    python tests/golden/make_pose_targets_golden.py
"""
import copy
import io
import json
import os
import zipfile

import numpy as np

import make_targets_golden as M
from make_targets_golden import DS, G, HERE, IMG_H, IMG_W, Opt, box_anns, record

J = 17
OUT_HW = (24, 40)
POSE_HEADS = ('hm', 'reg', 'wh', 'tracking', 'hps', 'hm_hp', 'hp_offset')
NEED = {'v2', 'v1', 'v0', 'left', 'right', 'top', 'bottom', 'swapped', 'all_hm_hp', 'hm_only'}


def add_keypoints(rs, anns, spread=0.2):
    """joints uniform over the box widened by `spread` on every side, visibility uniform over 0 / 1 / 2"""
    for a in anns:
        x, y, w, h = a['bbox']
        kp = []
        for _ in range(J):
            kp += [float(rs.uniform(x - spread * w, x + (1 + spread) * w)),
                   float(rs.uniform(y - spread * h, y + (1 + spread) * h)), int(rs.randint(0, 3))]
        a['keypoints'] = kp
    return anns


def flags_of(ds, opt, ret, before, flipped):
    """which of the required situations the sample holds; the key-point arithmetic is redone with the reference's own
    helper on the annotations the object loop saw, and held against the ret it returned"""
    got = set()
    t_out = ds.log['trans'][1]
    hps_mask = np.asarray(ret['hps_mask'])
    hm_hp_mask = np.asarray(ret['hm_hp_mask']).reshape(ds.max_objs, J)
    for k, a in enumerate(ds.anns[:ds.max_objs]):
        cls_id = int(ds.cat_ids[a['category_id']])
        if cls_id > opt.num_classes or cls_id <= -999:
            continue
        if cls_id <= 0 or a.get('iscrowd', 0) > 0:
            got.add('all_hm_hp' if cls_id <= 1 else 'hm_only')
            continue
        if ret['mask'][k] == 0:                              # empty clipped box: returned before _add_hps
            assert not hps_mask[k].any()
            continue
        pts = (np.array(a['keypoints'], np.float32).reshape(J, 3) if 'keypoints' in a
               else np.zeros((J, 3), np.float32))
        for j in range(J):
            pts[j, :2] = G.affine_transform(pts[j, :2], t_out)
            px, py, v = pts[j]
            inside = 0 <= px < opt.output_w and 0 <= py < opt.output_h
            if v == 0:
                got.add('v0')
                assert hps_mask[k, 2 * j] == 0
            elif inside:
                got.add('v2' if v == 2 else 'v1')
                assert hps_mask[k, 2 * j] == 1 and hm_hp_mask[k, j] == (1 if v == 2 else 0)
            else:
                assert hps_mask[k, 2 * j] == 0
                for hit, name in ((px < 0, 'left'), (px >= opt.output_w, 'right'), (py < 0, 'top'),
                                  (py >= opt.output_h, 'bottom')):
                    if hit:
                        got.add(name)
    if flipped:
        for a, b in zip(ds.anns, before):
            if 'keypoints' not in b:
                continue
            new, old = np.array(a['keypoints']).reshape(J, 3), np.array(b['keypoints'], np.float32).reshape(J, 3)
            mirrored = ds.img_hw[1] - old[:, 0] - 1
            for l, r in ds.flip_idx:
                assert new[l, 2] == old[r, 2] and new[l, 1] == old[r, 1] and new[l, 0] == mirrored[r]
                if (old[l] != old[r]).any():
                    got.add('swapped')
    return got


def between(ret):
    hp = np.asarray(ret['hm_hp'])
    return int(((hp > 0) & (hp < 1)).sum())


def renumber(arrays, tmps, name):
    for i, tmp in enumerate(tmps):
        for k, v in tmp.items():
            arrays['%s/%d/%s' % (name, i, k.split('/', 2)[2])] = v
    arrays[name + '/n'] = np.int64(len(tmps))


def case_p1(arrays, seen):
    cat_ids = {1: 1, 2: 0, 3: -1000}
    disturb = (0.3, 0.4, 0.3)
    cfg = {'heads': POSE_HEADS, 'num_classes': 1, 'max_objs': 8, 'cat_ids': cat_ids, 'out_hw': OUT_HW, 'tracking': True,
           'pre_hm': True, 'disturb': disturb, 'num_joints': J}
    tmps, flips, count = [], [], 0
    for seed in range(6):
        rs = np.random.RandomState(5000 + seed)
        n = int(rs.randint(9, 13))
        anns = add_keypoints(rs, box_anns(rs, n, list(rs.permutation([1, 1, 1, 1, 2, 1, 1, 3, 1, 1, 1, 1]))))
        anns[int(rs.randint(0, 8))]['iscrowd'] = 1
        pre = copy.deepcopy(anns[1:])
        flip = float(seed % 2)
        opt = Opt(POSE_HEADS, 1, OUT_HW, True, True, disturb, flip=flip)
        ds = DS(opt, 8, cat_ids, (IMG_H, IMG_W))
        ret = ds.run(seed, anns, pre)
        if flip:
            assert ds.anns[0]['bbox'] != anns[0]['bbox']
        assert ret['hps'].shape == (8, 2 * J) and ret['hm_hp'].shape == (J,) + OUT_HW
        assert ret['hp_ind'].shape == (8 * J,) and ret['hp_ind'].dtype == np.int64 and ret['hp_offset'].shape == (8 * J, 2)
        tmp = {}
        record(tmp, 'P1', 0, ds, opt, ret)
        seen |= flags_of(ds, opt, ret, anns, flip)
        count += between(ret)
        tmps.append(tmp)
        flips.append(flip)
    assert 0.0 in flips and 1.0 in flips
    opt = Opt(POSE_HEADS, 1, OUT_HW, True, True, disturb)
    ds = DS(opt, 8, cat_ids, (IMG_H, IMG_W))
    ret = ds.run(7, [], [])
    tmp = {}
    record(tmp, 'P1', 0, ds, opt, ret)
    mid = len(tmps) // 2
    tmps.insert(mid, tmp)
    renumber(arrays, tmps, 'P1')
    arrays['P1/cfg'], arrays['P1/empty'] = np.array(json.dumps(cfg)), np.int64(mid)
    print('P1: %d samples, %d hm_hp elements strictly between 0 and 1' % (len(tmps), count))
    return count


def case_p2(arrays, seen):
    heads = ('hm', 'reg', 'wh', 'hps', 'hm_hp')
    cat_ids = {1: 1, 2: 2, 3: 0, 4: -1, 5: -2, 6: 3}
    cfg = {'heads': heads, 'num_classes': 2, 'max_objs': 12, 'cat_ids': cat_ids, 'out_hw': OUT_HW, 'tracking': False,
           'pre_hm': False, 'disturb': (0.0, 0.0, 0.0), 'num_joints': J}
    tmps, count = [], 0
    for seed in range(3):
        rs = np.random.RandomState(6000 + seed)
        anns = add_keypoints(rs, box_anns(rs, 12, list(rs.permutation([1, 2, 3, 4, 5, 6, 1, 2, 1, 2, 1, 2]))))
        crowd = [i for i, a in enumerate(anns) if a['category_id'] == 2]
        anns[crowd[0]]['iscrowd'] = 1                         # class 2: one hm plane, hm_hp untouched
        for a in anns:
            if a['category_id'] in (3, 4, 5):                 # small ignore regions: the Gaussians stay visible
                a['bbox'][2], a['bbox'][3] = a['bbox'][2] * 0.4, a['bbox'][3] * 0.4
        opt = Opt(heads, 2, OUT_HW, False, False, flip=float(seed == 1))
        ds = DS(opt, 12, cat_ids, (IMG_H, IMG_W))
        ret = ds.run(seed, anns, [])
        assert not [k for k in ret if k.startswith('pre_')] and 'hp_offset' in ret and 'hp_offset_mask' in ret
        ids = [int(cat_ids[a['category_id']]) for a in ds.anns]
        assert {0, -1, -2} <= set(ids)
        tmp = {}
        record(tmp, 'P2', 0, ds, opt, ret)
        seen |= flags_of(ds, opt, ret, anns, seed == 1)
        count += between(ret)
        tmps.append(tmp)
    renumber(arrays, tmps, 'P2')
    arrays['P2/cfg'] = np.array(json.dumps(cfg))
    print('P2: %d samples, %d hm_hp elements strictly between 0 and 1' % (len(tmps), count))
    return count


def person(bbox, joints, track_id, cat=1):
    """`joints`: {j: (x, y, v)}; every other joint is (0, 0, 0)"""
    kp = [0.0, 0.0, 0] * J
    for j, (x, y, v) in joints.items():
        kp[3 * j:3 * j + 3] = [float(x), float(y), int(v)]
    return {'bbox': [float(v) for v in bbox], 'category_id': cat, 'track_id': track_id, 'keypoints': kp}


def case_p3(arrays, seen):
    cat_ids = {1: 1}
    cfg = {'heads': POSE_HEADS, 'num_classes': 1, 'max_objs': 8, 'cat_ids': cat_ids, 'out_hw': OUT_HW, 'tracking': True,
           'pre_hm': True, 'disturb': (0.0, 0.0, 0.0), 'num_joints': J}
    w, h = OUT_HW[1], OUT_HW[0]
    every = {j: (40.0 + 3 * j, 30.0 + 2 * j, 2 - j % 2) for j in range(J)}
    sets = [
        # (0, 0) exactly; the last column / the last row; the same joint of two persons on pixel (12, 9)
        [person([0, 0, 60, 50], {0: (0.0, 0.0, 2), 1: (4 * w - 2.0, 20.0, 2), 2: (30.0, 4 * h - 1.5, 1),
                                 5: (50.0, 38.0, 2)}, 1),
         person([30, 20, 50, 40], {5: (49.0, 37.0, 2), 6: (4 * w - 0.5, 4 * h - 0.5, 2)}, 2),
         {'bbox': [90.0, 10.0, 40.0, 60.0], 'category_id': 1, 'track_id': 3}],            # no keypoints at all
        # a radius-0 person; a person whose clipped box is empty while its key points lie inside the map
        [person([80.3, 50.2, 1.0, 1.0], {3: (80.5, 50.5, 2), 4: (20.0, 20.0, 1)}, 1),
         person([-900, 10, 30, 30], every, 2),
         person([20, 10, 100, 70], every, 3)]]
    tmps, count = [], 0
    for n, anns in enumerate(sets):
        opt = Opt(POSE_HEADS, 1, OUT_HW, True, True)
        ds = DS(opt, 8, cat_ids, (4 * h, 4 * w), fixed_aug=True)
        ret = ds.run(n, anns, copy.deepcopy(anns))
        ind = ret['hp_ind'].reshape(8, J)
        on = ret['hps_mask'].reshape(8, J, 2)[..., 0] > 0
        if n == 0:
            assert on[0, 0] and ind[0, 0] == 0 and (ret['hp_offset'].reshape(8, J, 2)[0, 0] < 1e-12).all()
            assert on[0, 1] and ind[0, 1] % w == w - 1 and on[0, 2] and ind[0, 2] // w == h - 1
            assert on[1, 6] and ind[1, 6] == h * w - 1
            assert on[0, 5] and on[1, 5] and ind[0, 5] == ind[1, 5] == 9 * w + 12
            assert ret['mask'][2] == 1 and not on[2].any()
        else:
            assert ret['mask'].tolist()[:3] == [1, 0, 1] and not on[1].any() and on[2].all()
            assert on[0, 3] and ret['hm_hp'][3, 12, 20] == 1.0
        tmp = {}
        record(tmp, 'P3', 0, ds, opt, ret)
        seen |= flags_of(ds, opt, ret, anns, False)
        count += between(ret)
        tmps.append(tmp)
    renumber(arrays, tmps, 'P3')
    arrays['P3/cfg'] = np.array(json.dumps(cfg))
    print('P3: %d samples, %d hm_hp elements strictly between 0 and 1' % (len(tmps), count))
    return count


def main():
    assert DS.num_joints == J and len(DS.flip_idx) == 8
    arrays, seen = {}, set()
    count = case_p1(arrays, seen) + case_p2(arrays, seen) + case_p3(arrays, seen)
    assert seen >= NEED, NEED - seen
    assert count >= 1000, count                               # the Gaussians are not buried under the rectangles
    print('situations %s; %d hm_hp elements strictly between 0 and 1' % (sorted(seen), count))
    path = os.path.join(HERE, 'pose_targets.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    assert M.IMG_H == IMG_H
    main()
