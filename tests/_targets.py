"""Shared by test_targets_cpu.py and test_hip_targets.py: the golden samples of tests/golden/targets.npz (written by
tests/golden/make_targets_golden.py from the reference's own ``GenericDataset.__getitem__``), the builders they need,
synthetic cases beyond the goldens, and the regime table of csrc/targets.hip."""
import json
import os
import re
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'targets.npz')
CASES = ('A', 'B', 'C', 'D')


def make_opt(heads, num_classes, out_hw, tracking, pre_hm, disturb=(0.0, 0.0, 0.0), inp_hw=None):
    o = types.SimpleNamespace()
    o.heads = {h: 1 for h in heads}
    o.num_classes = num_classes
    o.output_h, o.output_w = out_hw
    o.down_ratio = 4
    o.input_h, o.input_w = inp_hw if inp_hw is not None else (out_hw[0] * 4, out_hw[1] * 4)
    o.tracking, o.pre_hm = tracking, pre_hm
    o.hm_disturb, o.lost_disturb, o.fp_disturb = disturb
    o.dense_reg = 1
    o.num_stacks = 1
    o.weights = {h: 1.0 for h in heads}
    return o


def builder(cfg):
    from centertrack_amd.targets import TargetBuilder
    opt = make_opt(cfg['heads'], cfg['num_classes'], tuple(cfg['out_hw']), cfg['tracking'], cfg['pre_hm'],
                   tuple(cfg['disturb']))
    cat_ids = {int(k): v for k, v in cfg['cat_ids'].items()}
    return TargetBuilder(opt, cfg['num_classes'], cfg['max_objs'], cat_ids), opt


class Golden(object):
    """the file, parsed once: per case the config, and per sample the inputs of ``encode`` and the reference's ret"""

    def __init__(self):
        g = np.load(GOLDEN)

        def one(k):              # (scalars and strings are stored as one-element arrays)
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
            self.cases[c] = {'cfg': cfg, 'samples': samples, 'empty': int(one(c + '/empty')) if c == 'A' else None}

    def encode(self, tb, s, rng=None):
        t = s['trans']
        return tb.encode(s['anns'], t[1], s['height'], s['width'], aug_s=s['aug_s'], pre_anns=s['pre_anns'],
                         trans_input_pre=t[2], trans_output_pre=t[3],
                         noise=None if rng is not None or s['pre_anns'] is None else s['noise'], rng=rng)


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = Golden()
    return _GOLDEN


def stack(rets):
    """what default_collate makes of the reference's samples, as numpy"""
    return {k: np.stack([r[k] for r in rets]) for k in rets[0]}


# ---- cases beyond the goldens ------------------------------------------------------------------------------------
IDENT_OUT = np.array([[0.25, 0, 0], [0, 0.25, 0]], np.float64)     # image = network input, output grid a quarter of it
IDENT_IN = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)


def synth_builder(C, out_hw, max_objs, pre_hm=True, disturb=(0.0, 0.0, 0.0), inp_hw=None):
    from centertrack_amd.targets import TargetBuilder
    heads = ('hm', 'reg', 'wh') + (('tracking',) if pre_hm else ())
    opt = make_opt(heads, C, out_hw, pre_hm, pre_hm, disturb, inp_hw)
    return TargetBuilder(opt, C, max_objs, {i: i for i in range(1, C + 1)}), opt


def synth_anns(rs, n, C, inp_hw, wmax=0.5):
    H, W = inp_hw
    anns = []
    for i in range(n):
        w, h = rs.uniform(2, W * wmax), rs.uniform(2, H * wmax)
        anns.append({'bbox': [float(rs.uniform(-w / 2, W - w / 2)), float(rs.uniform(-h / 2, H - h / 2)), float(w), float(h)],
                     'category_id': int(rs.randint(1, C + 1)), 'track_id': i + 1})
    return anns


def synth_record(tb, opt, anns, pre_anns=None, noise=None):
    return tb.encode(anns, IDENT_OUT, opt.input_h, opt.input_w, pre_anns=pre_anns, trans_input_pre=IDENT_IN,
                     trans_output_pre=IDENT_OUT, noise=noise)


def case_e():
    """128 x 128 / 512 x 512, B = 2, C = 80, 128 objects each"""
    tb, opt = synth_builder(80, (128, 128), 128)
    rs = np.random.RandomState(51)
    recs = []
    for _ in range(2):
        anns = synth_anns(rs, 128, 80, (512, 512), 0.3)
        recs.append(synth_record(tb, opt, anns, anns))
    return tb, recs


def case_f():
    """one image with more than 2 * CULL_CAP pre_hm blobs, at least CULL_CAP + 1 of them over a single tile, next to an
    image with none (an empty sample)"""
    from centertrack_amd import targets as T
    tb, opt = synth_builder(1, (16, 24), 8, disturb=(0.02, 0.2, 1.1))       # fp always fires: two blobs per object
    rs = np.random.RandomState(61)
    n = T.CULL_CAP + 40
    pre = []
    for i in range(n):
        if i < T.CULL_CAP // 2 + 8:          # boxes around pixel (40, 20): every blob covers the tile of that pixel
            w, h = rs.uniform(12, 30), rs.uniform(12, 30)
            x, y = 40 - w / 2 + rs.uniform(-1, 1), 20 - h / 2 + rs.uniform(-1, 1)
        else:
            w, h = rs.uniform(3, 20), rs.uniform(3, 20)
            x, y = rs.uniform(0, 96 - w), rs.uniform(0, 64 - h)
        pre.append({'bbox': [float(x), float(y), float(w), float(h)], 'category_id': 1, 'track_id': i})
    noise = np.stack([rs.randn(n), rs.randn(n), rs.uniform(0.3, 1, n), np.zeros(n), rs.randn(n), rs.randn(n)], 1)
    rec = synth_record(tb, opt, pre[:3], pre, noise)
    return tb, [rec, synth_record(tb, opt, [], [])]


def case_g():
    """7 x 33 / 28 x 132: smaller than a tile in one axis, ragged in the other, W mod 4 != 0"""
    tb, opt = synth_builder(3, (7, 33), 8)
    rs = np.random.RandomState(71)
    recs = []
    for _ in range(2):
        anns = synth_anns(rs, 6, 3, (28, 132))
        recs.append(synth_record(tb, opt, anns, anns))
    return tb, recs


def case_h():
    """B = 1, C = 1, a single radius-0 object"""
    tb, opt = synth_builder(1, (8, 8), 4, pre_hm=False)
    rec = synth_record(tb, opt, [{'bbox': [13.0, 9.0, 1.0, 1.0], 'category_id': 1}])
    assert rec['hm_blobs'].tolist() == [[0, 3, 2, 0]]
    return tb, [rec]


SYNTH = {'E': case_e, 'F': case_f, 'G': case_g, 'H': case_h}


# ---- the regimes of build_targets_kernel -------------------------------------------------------------------------
def kernel_constants():
    """TGT_TW, TGT_TH of csrc/targets.hip and CT_TARGETS_CULL_CAP / CT_TARGETS_MAX_OUT of the header"""
    src = open(os.path.join(ROOT, 'centertrack_amd', 'csrc', 'targets.hip')).read()
    hdr = open(os.path.join(ROOT, 'include', 'centertrack_hip.h')).read()
    m = re.search(r'constexpr int TGT_TW = (\d+), TGT_TH = (\d+), TGT_CAP = CT_TARGETS_CULL_CAP;', src)
    return {'TW': int(m.group(1)), 'TH': int(m.group(2)),
            'CAP': int(re.search(r'#define CT_TARGETS_CULL_CAP (\d+)', hdr).group(1)),
            'MAX_OUT': int(re.search(r'#define CT_TARGETS_MAX_OUT (\d+)', hdr).group(1)),
            'MAX_RADIUS': int(re.search(r'constexpr int TGT_MAX_RADIUS = (\d+);', src).group(1))}


def tile_load(rec_list, key, cols, hw, K):
    """the largest number of blobs of one image whose support touches one tile (what a workgroup keeps after culling)"""
    best = 0
    for rec in rec_list:
        b = rec[key]
        if not len(b):
            continue
        cx, cy, r = (b[:, c].astype(np.int64) for c in cols)
        for y0 in range(0, hw[0], K['TH']):
            for x0 in range(0, hw[1], K['TW']):
                hit = (cx + r >= x0) & (cx - r < x0 + K['TW']) & (cy + r >= y0) & (cy - r < y0 + K['TH'])
                best = max(best, int(hit.sum()))
    return best


def regimes(K):
    """name -> predicate(tb, records): what the kernel branches on (csrc/targets.hip): the tile grid of each map, the
    culling rounds of CULL_CAP blobs, the survivors of a round, rectangles, the slot part"""
    def hm_hw(tb):
        return tb.opt.output_h, tb.opt.output_w

    def pre_hw(tb):
        return tb.opt.input_h, tb.opt.input_w

    def nmax(recs, i):
        return max(int(r['counts'][i]) for r in recs)

    return {
        'hm: several tiles on both axes': lambda tb, r: hm_hw(tb)[0] > K['TH'] and hm_hw(tb)[1] > K['TW'],
        'hm: map smaller than a tile in y': lambda tb, r: hm_hw(tb)[0] < K['TH'],
        'hm: ragged last tile in x': lambda tb, r: hm_hw(tb)[1] % K['TW'] != 0,
        'hm: ragged last tile in y': lambda tb, r: hm_hw(tb)[0] % K['TH'] != 0,
        'hm: row length no multiple of 4': lambda tb, r: hm_hw(tb)[1] % 4 != 0,
        'hm: one plane': lambda tb, r: tb.num_classes == 1,
        'hm: many planes': lambda tb, r: tb.num_classes >= 80,
        'hm: an image without blobs (no culling round)': lambda tb, r: min(int(x['counts'][1]) for x in r) == 0,
        'hm: ignore rectangles, one plane and all planes': lambda tb, r: any(
            len(x['rects']) and x['rects'][:, 0].min() < 0 and x['rects'][:, 0].max() >= 0 for x in r),
        'hm: radius 0': lambda tb, r: any(len(x['hm_blobs']) and x['hm_blobs'][:, 3].min() == 0 for x in r),
        'pre_hm: absent': lambda tb, r: not tb.pre_hm,
        'pre_hm: several tiles on both axes': lambda tb, r: tb.pre_hm and pre_hw(tb)[0] > K['TH'] and pre_hw(tb)[1] > K['TW'],
        'pre_hm: ragged last tile in x': lambda tb, r: tb.pre_hm and pre_hw(tb)[1] % K['TW'] != 0,
        'pre_hm: more than two culling rounds': lambda tb, r: tb.pre_hm and nmax(r, 3) > 2 * K['CAP'],
        'pre_hm: a round that fills the list (CULL_CAP + 1 blobs over one tile)': lambda tb, r: tb.pre_hm and tile_load(
            r, 'pre_blobs', (0, 1, 2), pre_hw(tb), K) >= K['CAP'] + 1,
        'pre_hm: an image without blobs': lambda tb, r: tb.pre_hm and min(int(x['counts'][3]) for x in r) == 0,
        'pre_hm: conf 0 blobs': lambda tb, r: any(len(x['pre_blobs']) and x['pre_blobs'][:, 3].min() == 0 for x in r),
        'pre_hm: centres outside the map': lambda tb, r: any(
            len(x['pre_blobs']) and (x['pre_blobs'][:, 0].min() < 0 or x['pre_blobs'][:, 0].max() >= pre_hw(tb)[1])
            for x in r),
        'slots: holes': lambda tb, r: any(len(x['slot_k']) and int(x['slot_k'].max()) + 1 > len(x['slot_k']) for x in r),
        'slots: an image without objects': lambda tb, r: min(int(x['counts'][0]) for x in r) == 0,
        'slots: int64 pairs (rotbin)': lambda tb, r: 'rot' in tb.heads,
        'slots: more than one workgroup': lambda tb, r: len(r) * tb.max_objs * tb.slot_words > 256,
        'slots: a single partly filled workgroup': lambda tb, r: len(r) * tb.max_objs * tb.slot_words < 256,
    }
