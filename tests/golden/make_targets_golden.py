"""Golden vectors of the training targets from the reference's own ``GenericDataset.__getitem__`` (build container
only, like make_loss_golden.py): tests/golden/targets.npz.

A bare ``GenericDataset`` subclass runs the reference's ``__getitem__`` on the CPU over synthetic annotation lists
(``_load_data`` / ``_load_pre_data`` return them, ``_get_input`` returns zeros).  Per sample the generator records, by
wrapping names in its own process, what ``centertrack_amd.targets.TargetBuilder.encode`` takes as input -- the
annotation lists as the object loop saw them (after the in-place flip), the affine matrices in call order, ``aug_s``,
the six noise numbers of every previous object, the state of numpy's global stream before ``_get_pre_dets`` and the
first number after it -- and the ``ret`` the reference returned (images dropped).

Keys: ``<case>/n`` samples, ``<case>/cfg`` (JSON), ``<case>/<i>/in`` (JSON), ``<case>/<i>/trans`` [4,2,3],
``<case>/<i>/noise`` [n_pre,6] (NaN = not drawn), ``<case>/<i>/rng_key|rng_pos|rng_gauss|rng_next``,
``<case>/<i>/ret/<key>``.  Fixed zip timestamps: a second run reproduces the file byte for byte.

    python tests/golden/make_targets_golden.py
"""
import copy
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_import  # noqa: E402

ref_import.install()
_coco = types.ModuleType('pycocotools.coco')          # imported by the reference's dataset module, never called here
sys.modules.setdefault('pycocotools', types.ModuleType('pycocotools')).coco = _coco
sys.modules['pycocotools.coco'] = _coco

from dataset import generic_dataset as G  # noqa: E402  (the reference's)

IMG_H, IMG_W = 120, 200


class Opt(object):
    def __init__(self, heads, num_classes, out_hw, tracking, pre_hm, disturb=(0.0, 0.0, 0.0), flip=0.0):
        self.heads = {h: 1 for h in heads}
        self.num_classes = num_classes
        self.output_h, self.output_w = out_hw
        self.down_ratio = 4
        self.input_h, self.input_w = out_hw[0] * 4, out_hw[1] * 4
        self.tracking, self.pre_hm = tracking, pre_hm
        self.hm_disturb, self.lost_disturb, self.fp_disturb = disturb
        self.not_rand_crop = False
        self.not_max_crop = False
        self.scale, self.shift, self.aug_rot, self.rotate = 0, 0, 0, 0
        self.flip = flip
        self.same_aug_pre = False
        self.max_frame_dist = 3
        self.dense_reg = 1
        self.debug = 0
        self.velocity = 'velocity' in heads
        self.simple_radius = 0
        self.no_color_aug = True


class DS(G.GenericDataset):
    """the reference's __getitem__ over one synthetic sample, with recorders around the names it calls"""

    def __init__(self, opt, max_objs, cat_ids, img_hw, fixed_aug=False):
        super(DS, self).__init__(opt, 'train')
        self.max_objs, self.cat_ids, self.img_hw, self.fixed_aug = max_objs, cat_ids, img_hw, fixed_aug
        self.num_categories = opt.num_classes

    def run(self, seed, anns, pre_anns):
        self.anns, self.pre_anns = copy.deepcopy(anns), copy.deepcopy(pre_anns)
        self.log = {'trans': [], 'aug_s': [], 'draws': [], 'centres': []}
        keep = G.get_affine_transform

        def affine(*a, **k):
            t = keep(*a, **k)
            self.log['trans'].append(np.array(t, np.float64))
            return t

        G.get_affine_transform = affine
        np.random.seed(seed)
        try:
            ret = self[0]
        finally:
            G.get_affine_transform = keep
        return ret

    def __len__(self):
        return 1

    def _load_data(self, index):
        img = np.zeros(self.img_hw + (3,), np.uint8)
        return img, self.anns, {'id': 1, 'video_id': 1, 'frame_id': 2}, ''

    def _load_pre_data(self, video_id, frame_id, sensor_id=1):
        return np.zeros(self.img_hw + (3,), np.uint8), self.pre_anns, 1

    def _get_input(self, img, trans_input):
        return np.zeros((3, self.opt.input_h, self.opt.input_w), np.float32)

    def _get_aug_param(self, c, s, width, height, disturb=False):
        # (fixed_aug: the augmentation parameters are the caller's; centre crop at scale 1)
        r = (c, 1, 0) if self.fixed_aug else super(DS, self)._get_aug_param(c, s, width, height, disturb)
        self.log['aug_s'].append(r[1])
        return r

    def _get_pre_dets(self, anns, trans_input, trans_output):
        log = self.log
        log['state'] = np.random.get_state()
        keep = (np.random.randn, np.random.random, G.draw_umich_gaussian, self._coco_box_to_bbox)

        def randn():
            v = keep[0]()
            log['draws'].append(('n', v))
            return v

        def random():
            v = keep[1]()
            log['draws'].append(('u', v))
            return v

        def draw(hm, ct, radius, k=1):
            log['centres'].append((int(ct[0]), int(ct[1]), int(radius), int(k)))
            return keep[2](hm, ct, radius, k=k)

        def box(b):
            log['draws'].append(('box', None))
            return keep[3](b)

        np.random.randn, np.random.random, G.draw_umich_gaussian, self._coco_box_to_bbox = randn, random, draw, box
        try:
            r = super(DS, self)._get_pre_dets(anns, trans_input, trans_output)
        finally:
            np.random.randn, np.random.random, G.draw_umich_gaussian = keep[:3]
            del self._coco_box_to_bbox
        after = np.random.RandomState()
        after.set_state(np.random.get_state())
        log['next'] = after.random_sample()
        return r


def noise_rows(ds, opt):
    """[n_pre, 6] from the draw log: every previous annotation that passes the class filter opens a group (its box is
    converted first); a group holds nothing, or normal, normal, uniform, uniform and two more normals if fp fired"""
    pre = ds.pre_anns
    passing = [j for j, a in enumerate(pre)
               if not (int(ds.cat_ids[a['category_id']]) > opt.num_classes or int(ds.cat_ids[a['category_id']]) <= -99
                       or a.get('iscrowd', 0) > 0)]
    rows = np.full((len(pre), 6), np.nan)
    groups = []
    for kind, v in ds.log['draws']:
        if kind == 'box':
            groups.append([])
        else:
            groups[-1].append((kind, v))
    assert len(groups) == len(passing)
    for j, g in zip(passing, groups):
        kinds = ''.join(k for k, _ in g)
        assert kinds in ('', 'nnuu', 'nnuunn'), kinds
        rows[j, :len(g)] = [v for _, v in g]
    return rows


def flags_of(ds, opt, noise, trans_input_pre):
    """which of the required situations the sample's previous objects produce (the centre arithmetic is redone here
    with the reference's own helpers, and checked against the centres it drew)"""
    got, drawn = set(), list(ds.log['centres'])
    H, W = opt.input_h, opt.input_w
    for j, a in enumerate(ds.pre_anns):
        if np.isnan(noise[j, 0]):
            continue
        b = ds._coco_box_to_bbox(a['bbox'])
        b[:2] = G.affine_transform(b[:2], trans_input_pre)
        b[2:] = G.affine_transform(b[2:], trans_input_pre)
        b[[0, 2]] = np.clip(b[[0, 2]], 0, W - 1)
        b[[1, 3]] = np.clip(b[[1, 3]], 0, H - 1)
        h, w = b[3] - b[1], b[2] - b[0]
        ct = np.array([(b[0] + b[2]) / 2, (b[1] + b[3]) / 2], dtype=np.float32)
        ct[0] = ct[0] + float(noise[j, 0]) * opt.hm_disturb * w
        ct[1] = ct[1] + float(noise[j, 1]) * opt.hm_disturb * h
        ci = ct.astype(np.int32)
        first = drawn.pop(0)
        assert first[:2] == (int(ci[0]), int(ci[1])), (first, ci)
        if first[3] == 0:
            got.add('conf0')
        if not np.isnan(noise[j, 4]):
            got.add('fp')
            drawn.pop(0)
        for v, lim, lo, hi in ((ct[0], W, 'left', 'right'), (ct[1], H, 'top', 'bottom')):
            if v <= -1:
                got.add(lo)
            if v >= lim:
                got.add(hi)
            if -1 < v < 0 and v != int(v):
                got.add('negfrac')
    assert not drawn
    return got


def record(arrays, name, i, ds, opt, ret):
    log = ds.log
    trans = log['trans']
    assert len(trans) in (2, 4)
    if len(trans) == 2:
        trans = trans + trans
    noise = noise_rows(ds, opt) if opt.tracking else np.zeros((0, 6))
    pre = '%s/%d/' % (name, i)
    arrays[pre + 'in'] = np.array(json.dumps({'anns': ds.anns, 'pre_anns': ds.pre_anns if opt.tracking else None,
                                              'aug_s': float(log['aug_s'][0]), 'height': ds.img_hw[0],
                                              'width': ds.img_hw[1]}))
    arrays[pre + 'trans'] = np.stack(trans)
    arrays[pre + 'noise'] = noise
    if opt.tracking:
        st = log['state']
        assert st[0] == 'MT19937'
        arrays[pre + 'rng_key'] = np.asarray(st[1], np.uint32)
        arrays[pre + 'rng_pos'] = np.int64(st[2])
        arrays[pre + 'rng_gauss'] = np.array([st[3], st[4]], np.float64)
        arrays[pre + 'rng_next'] = np.float64(log['next'])
    for k, v in ret.items():
        if k not in ('image', 'pre_img'):
            arrays[pre + 'ret/' + k] = np.asarray(v)
    return noise, trans


def box_anns(rs, n, cats, track0=1, ddd=False):
    """n random boxes over (and beyond) the IMG_H x IMG_W image; every fourth one straddles a border"""
    anns = []
    for i in range(n):
        w, h = rs.uniform(6, 90), rs.uniform(6, 70)
        x, y = rs.uniform(0, IMG_W - w), rs.uniform(0, IMG_H - h)
        side = i % 8
        if side == 1:
            x = -w / 2
        elif side == 3:
            x = IMG_W - w / 3
        elif side == 5:
            y = -h / 3
        elif side == 7:
            y = IMG_H - h / 2
        a = {'bbox': [float(x), float(y), float(w), float(h)], 'category_id': int(cats[i % len(cats)]),
             'track_id': track0 + i}
        if ddd:
            if i % 5 != 4:
                a['depth'] = float(rs.uniform(3, 60))
            if i % 4 != 3:
                a['alpha'] = float(rs.uniform(-np.pi, np.pi))
            if i % 3 != 2:
                a['amodel_center'] = [float(x + w / 2 + rs.uniform(-20, 20)), float(y + h / 2 + rs.uniform(-9, 9))]
            a['dim'] = [float(v) for v in rs.uniform(0.5, 5, 3)]
            a['attributes'] = int(i % 9)                      # 0 = none
            a['velocity'] = [-2000.0, 0.0, 1.0] if i % 6 == 5 else [float(v) for v in rs.uniform(-5, 5, 3)]
        anns.append(a)
    return anns


def case_a(arrays):
    """MOT heads + tracking + pre_hm, 3 classes, max_objs 8 of 10-12 annotations, all three disturbances"""
    heads = ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal')
    cat_ids = {1: 1, 2: 2, 3: 3, 4: 0, 5: -2, 6: 4, 7: -1000}
    cfg = {'heads': heads, 'num_classes': 3, 'max_objs': 8, 'cat_ids': cat_ids, 'out_hw': (24, 40), 'tracking': True,
           'pre_hm': True, 'disturb': (0.3, 0.4, 0.3)}
    need = {'left', 'right', 'top', 'bottom', 'negfrac', 'conf0', 'fp'}
    kept, seen = [], set()
    for seed in range(400):
        rs = np.random.RandomState(1000 + seed)
        n = int(rs.randint(10, 13))
        cats = list(rs.permutation([1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5]))
        anns = box_anns(rs, n, cats)
        anns[int(rs.randint(0, 8))]['iscrowd'] = 1
        out = {'bbox': [-900.0, 10.0, 30.0, 30.0], 'category_id': 1 if seed % 2 else 4, 'track_id': 90}
        anns[int(rs.randint(0, 8))] = out                       # entirely outside: no object; still a rectangle if ignored
        pre = copy.deepcopy(anns[2:]) + box_anns(rs, 2, [1, 2], track0=50)   # [0], [1] have no past, two have no present
        for a in pre:
            a['bbox'] = [float(v + d) for v, d in zip(a['bbox'], rs.uniform(-4, 4, 4))]
            a['bbox'][2], a['bbox'][3] = max(a['bbox'][2], 2.0), max(a['bbox'][3], 2.0)
        opt = Opt(heads, 3, (24, 40), True, True, cfg['disturb'])
        ds = DS(opt, 8, cat_ids, (IMG_H, IMG_W))
        ret = ds.run(seed, anns, pre)
        tmp = {}
        noise, trans = record(tmp, 'A', len(kept), ds, opt, ret)
        got = flags_of(ds, opt, noise, trans[2])
        if (got - seen) or (seen >= need and len(kept) < 7):
            seen |= got
            kept.append(tmp)
            arrays.update(tmp)
        if seen >= need and len(kept) >= 7:
            break
    assert seen >= need, need - seen
    # the empty sample goes into the middle
    opt = Opt(heads, 3, (24, 40), True, True, cfg['disturb'])
    ds = DS(opt, 8, cat_ids, (IMG_H, IMG_W))
    ret = ds.run(7, [], [])
    mid = len(kept) // 2
    for i in range(len(kept) - 1, mid - 1, -1):                 # shift samples mid.. up by one
        for k in [k for k in arrays if k.startswith('A/%d/' % i)]:
            arrays['A/%d/%s' % (i + 1, k.split('/', 2)[2])] = arrays.pop(k)
    record(arrays, 'A', mid, ds, opt, ret)
    arrays['A/n'], arrays['A/cfg'] = np.int64(len(kept) + 1), np.array(json.dumps(cfg))
    arrays['A/empty'] = np.int64(mid)
    print('A: %d samples, situations %s' % (len(kept) + 1, sorted(seen)))


def case_b(arrays):
    """the nuScenes ddd heads, 10 classes, flipped and unflipped, aug_s != 1"""
    heads = ('hm', 'reg', 'wh', 'tracking', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity',
             'ltrb_amodal')
    cat_ids = {i: i for i in range(1, 11)}
    cat_ids[11] = -3
    cfg = {'heads': heads, 'num_classes': 10, 'max_objs': 16, 'cat_ids': cat_ids, 'out_hw': (24, 40), 'tracking': True,
           'pre_hm': True, 'disturb': (0.3, 0.4, 0.3)}
    n = 0
    for seed in range(40):
        rs = np.random.RandomState(2000 + seed)
        anns = box_anns(rs, 12, list(rs.permutation(11) + 1), ddd=True)
        pre = copy.deepcopy(anns[1:])
        opt = Opt(heads, 10, (24, 40), True, True, cfg['disturb'], flip=float(n % 2))
        ds = DS(opt, 16, cat_ids, (IMG_H, IMG_W))
        ret = ds.run(seed, anns, pre)
        if abs(float(ds.log['aug_s'][0]) - 1) < 1e-6:
            continue
        if n % 2:                                                # the flip rewrote the annotations in place
            assert ds.anns[0]['bbox'] != anns[0]['bbox'] and ds.anns[0]['velocity'][0] == -10000
        record(arrays, 'B', n, ds, opt, ret)
        n += 1
        if n == 4:
            break
    assert n == 4
    arrays['B/n'], arrays['B/cfg'] = np.int64(n), np.array(json.dumps(cfg))
    print('B: %d samples' % n)


def case_c(arrays):
    """detection only, 80 classes, 16 x 20: no pre_* keys at all"""
    heads = ('hm', 'reg', 'wh')
    cat_ids = {i: i for i in range(1, 81)}
    cfg = {'heads': heads, 'num_classes': 80, 'max_objs': 16, 'cat_ids': cat_ids, 'out_hw': (16, 20), 'tracking': False,
           'pre_hm': False, 'disturb': (0.0, 0.0, 0.0)}
    for n, seed in enumerate((5, 6, 7)):
        rs = np.random.RandomState(3000 + seed)
        anns = box_anns(rs, 14, list(rs.randint(1, 81, 14)))
        anns[3]['iscrowd'] = 1
        opt = Opt(heads, 80, (16, 20), False, False)
        ds = DS(opt, 16, cat_ids, (IMG_H, IMG_W))
        ret = ds.run(seed, anns, [])
        assert not [k for k in ret if k.startswith('pre_')]
        record(arrays, 'C', n, ds, opt, ret)
    arrays['C/n'], arrays['C/cfg'] = np.int64(3), np.array(json.dumps(cfg))
    print('C: 3 samples')


def case_d(arrays):
    """no augmentation (the image is the network input, the output grid a quarter of it): 1 x 1 and sub-pixel boxes
    (radius 0), centres at (0, 0) and (w - 1, h - 1)"""
    heads = ('hm', 'reg', 'wh', 'tracking')
    cat_ids = {1: 1, 2: 2}
    cfg = {'heads': heads, 'num_classes': 2, 'max_objs': 8, 'cat_ids': cat_ids, 'out_hw': (24, 40), 'tracking': True,
           'pre_hm': True, 'disturb': (0.0, 0.0, 0.0)}
    # left edges one float32 step below 39 and 23 on the output grid: the clipped box keeps a positive size and its centre
    # rounds (to even) onto the last pixel
    x0, y0 = 4 * (39 - 2.0 ** -18), 4 * (23 - 2.0 ** -19)
    sets = [[{'bbox': [40.0, 40.0, 4.0, 4.0], 'category_id': 1, 'track_id': 1},
             {'bbox': [80.3, 50.2, 1.0, 1.0], 'category_id': 2, 'track_id': 2},
             {'bbox': [-2.0, -2.0, 4.0, 4.0], 'category_id': 1, 'track_id': 3},
             {'bbox': [x0, y0, 30.0, 30.0], 'category_id': 2, 'track_id': 4}],
            [{'bbox': [x0, y0, 30.0, 30.0], 'category_id': 1, 'track_id': 1},
             {'bbox': [-3.0, -1.0, 4.0, 2.0], 'category_id': 1, 'track_id': 2},
             {'bbox': [100.0, 60.0, 0.5, 0.25], 'category_id': 2, 'track_id': 3}]]
    for n, anns in enumerate(sets):
        opt = Opt(heads, 2, (24, 40), True, True)
        ds = DS(opt, 8, cat_ids, (96, 160), fixed_aug=True)
        ret = ds.run(n, anns, copy.deepcopy(anns))
        ind = [int(v) for v, m in zip(ret['ind'], ret['mask']) if m > 0]
        assert 0 in ind and 24 * 40 - 1 in ind, ind
        assert len(ind) == len(anns)
        record(arrays, 'D', n, ds, opt, ret)
    arrays['D/n'], arrays['D/cfg'] = np.int64(2), np.array(json.dumps(cfg))
    print('D: 2 samples')


def main():
    arrays = {}
    case_a(arrays)
    case_b(arrays)
    case_c(arrays)
    case_d(arrays)
    path = os.path.join(HERE, 'targets.npz')
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
    main()
