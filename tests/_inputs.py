"""Shared by test_inputs_cpu.py and test_hip_inputs.py: the golden samples of tests/golden/inputs.npz (written by
tests/golden/make_inputs_golden.py from the reference's own ``GenericDataset.__getitem__``), the builders they need, the
synthetic cases beyond the goldens, the float64 evaluation behind the colour bound, and the regime table of
csrc/inputs.hip."""
import json
import os
import random
import re
import types

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'inputs.npz')
CASES = ('A', 'B', 'C', 'D')
MEAN = np.array([0.40789654, 0.44719302, 0.47026115], np.float32)
STD = np.array([0.28863828, 0.27408164, 0.27809835], np.float32)


def source(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def make_opt(inp_hw, no_color_aug=False):
    o = types.SimpleNamespace()
    o.input_h, o.input_w = inp_hw
    o.no_color_aug = no_color_aug
    return o


def builder(inp_hw, mean=MEAN, std=STD, no_color_aug=False):
    from centertrack_amd.inputs import InputBuilder
    return InputBuilder(make_opt(tuple(inp_hw), no_color_aug), mean, std)


class Golden(object):
    """the file, parsed once: per case the config and per sample the sources, matrices, draws and the reference's images"""

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
                s['trans'] = g[pre + 'trans']
                s['image'] = g[pre + 'image']
                s['pre_img'] = g[pre + 'pre_img'] if pre + 'pre_img' in g.files else None
                s['calls'] = []
                for j in range(2 if s['pre_img'] is not None else 1):
                    cp = '%scall%d/' % (pre, j)
                    s['calls'].append({k[len(cp):]: g[k] for k in g.files if k.startswith(cp)})
                samples.append(s)
            self.cases[c] = {'cfg': cfg, 'samples': samples}

    @staticmethod
    def builder(cfg):
        return builder(cfg['input_hw'], np.array(cfg['mean'], np.float32), np.array(cfg['std'], np.float32))

    @staticmethod
    def color(call):
        if 'order' not in call:
            return None
        return {'order': call['order'], 'alpha': call['alpha'], 'light': call['light']}

    def encode(self, ib, s):
        """(img_record, pre_img_record or None) of a golden sample, from the frames as loaded"""
        t = s['trans']
        img = ib.encode(source(s['seed'], s['h'], s['w']), t[0], bool(s['flipped']), self.color(s['calls'][0]))
        if s['pre_img'] is None:
            return img, None
        pre = ib.encode(source(s['pre_seed'], s['h'], s['w']), t[2], bool(s['flipped']), self.color(s['calls'][1]))
        return img, pre

    @staticmethod
    def streams(s):
        """the two streams as the generator left them before the sample's first ``_get_input``"""
        rng = np.random.RandomState(s['seed'])
        rng.random_sample()
        return rng, random.Random(s['seed'])


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = Golden()
    return _GOLDEN


def next_of(rng):
    c = np.random.RandomState()
    c.set_state(rng.get_state())
    return c.random_sample()


def py_next_of(py):
    c = random.Random()
    c.setstate(py.getstate())
    return c.random()


# ---- the float64 evaluation of the chain: the yardstick of the colour bound ------------------------------------------
def chain64(ib, warped, color):
    """``_get_input`` behind the warp in float64 throughout (exact inputs: the u8 image, float32 mean / std, the draws):
    float64 [3, H, W]"""
    x = warped.astype(np.float64) / 255.0
    if color is not None:
        gs = 0.114 * x[:, :, 0] + 0.587 * x[:, :, 1] + 0.299 * x[:, :, 2]
        gs_mean = gs.mean()
        for f, alpha in zip(color['order'].tolist(), color['alpha'].tolist()):
            x = x * alpha
            if f == 1:
                x = x + gs_mean * (1 - alpha)
            elif f == 2:
                x = x + (gs * (1 - alpha))[:, :, None]
        x = x + color['light']
    x = (x - ib.mean.astype(np.float64)) / ib.std.astype(np.float64)
    return x.transpose(2, 0, 1)


def grey_mean64(warped):
    """float64 mean of the float32 grey image (the grey values as the kernel and the reference form them)"""
    x = warped.astype(np.float32) / np.float32(255.)
    gs = (np.float32(0.114) * x[:, :, 0] + np.float32(0.587) * x[:, :, 1]) + np.float32(0.299) * x[:, :, 2]
    return float(gs.astype(np.float64).mean())


def colour_bound(ib, rec):
    """(e32, bound) of one record: e32 = the relative error of ``reference`` against the float64 chain on this image,
    bound = 4 max(e32, 2^-23) max|reference|"""
    ref = ib.reference(rec)
    hi = float(np.abs(ref).max())
    e32 = float(np.abs(ref.astype(np.float64) - chain64(ib, ib.warped_reference(rec), rec['color'])).max()) / hi
    return e32, 4.0 * max(e32, 2.0 ** -23) * hi


# ---- cases beyond the goldens --------------------------------------------------------------------------------------------
def get_affine(c, s, rot, out_wh):
    from centertrack_amd.image import get_affine_transform
    return get_affine_transform(np.array(c, np.float32), s, rot, list(out_wh))


def draw(ib, seed):
    return ib.draw_color(np.random.RandomState(seed), random.Random(seed))


def _pair(ib, seed, hw, out_wh, aug_s=1.0, rot=0, flipped=False, color=True, pre=True, c=None):
    """((img_record, pre_img_record or None), (frame, pre_frame or None)): the frames as loaded, never flipped"""
    h, w = hw
    c = (w / 2., h / 2.) if c is None else c
    s = max(h, w) * aug_s
    frame = source(seed, h, w)
    img = ib.encode(frame, get_affine(c, s, rot, out_wh), flipped, draw(ib, seed) if color else None)
    if not pre:
        return (img, None), (frame, None)
    pre_frame = source(seed + 500, h, w)
    pre_rec = ib.encode(pre_frame, get_affine((c[0] + 3, c[1] - 2), s * 1.04, rot, out_wh), flipped,
                        draw(ib, seed + 500) if color else None)
    return (img, pre_rec), (frame, pre_frame)


def _case(ib, pairs):
    return ib, [p[0] for p in pairs], [p[1] for p in pairs]


def case_e():
    """270 x 480 sources -> 128 x 192, B = 2 with pre_img: 3 x 8 tiles = 24 partials per image, four images"""
    ib = builder((128, 192))
    return _case(ib, [_pair(ib, 51, (270, 480), (192, 128), 0.8, flipped=True),
                      _pair(ib, 52, (270, 480), (192, 128), 1.1, rot=7)])


def case_f():
    """B = 3, three source sizes; sample 0's source has a row pitch above 3 w, sample 1 has no pre_img, sample 2's image
    has no colour record"""
    ib = builder((40, 72))
    a = _pair(ib, 61, (50, 70), (72, 40), 0.9)
    rec = a[0][0]
    padded = np.zeros((rec['rows'].shape[0], 70 + 9, 3), np.uint8)
    padded[:, :70] = rec['rows']
    padded[:, 70:] = 255                                   # the padding must never be read
    rec['rows'] = padded[:, :70]
    assert rec['rows'].strides[0] == 3 * 79
    b = _pair(ib, 62, (33, 90), (72, 40), 1.2, pre=False)
    c = _pair(ib, 63, (64, 48), (72, 40), 0.7, flipped=True)
    c = ((dict(c[0][0], color=None), c[0][1]), c[1])
    return _case(ib, [a, b, c])


def case_g():
    """output 7 x 33: below one wave per row, a partial tile both ways"""
    ib = builder((7, 33))
    return _case(ib, [_pair(ib, 71, (40, 56), (33, 7), 1.0, flipped=True), _pair(ib, 72, (40, 56), (33, 7), 0.6)])


def case_h():
    """1 x 1 and 2 x 2 sources"""
    ib = builder((16, 24))
    return _case(ib, [_pair(ib, 81, (1, 1), (24, 16), 1.0, pre=False),
                      _pair(ib, 82, (2, 2), (24, 16), 1.0, flipped=True, pre=False)])


def case_i():
    """a tall source at aug_s 0.6, flipped: most rows are not uploaded"""
    ib = builder((32, 48))
    pair = _pair(ib, 91, (400, 60), (48, 32), 0.6, flipped=True, c=(30., 250.))
    assert pair[0][0]['rows'].shape[0] < 400 // 2 and pair[0][0]['row0'] > 0
    return _case(ib, [pair])


def case_k():
    """output 264 x 320 from one 60 x 80 source: 17 x 5 = 85 partials, more than the 64 lanes that add them in pass 2 (a
    lane takes a second partial), ragged in y.  Larger than case E: no smaller output has more than 64 tiles of 64 x 16"""
    ib = builder((264, 320))
    return _case(ib, [_pair(ib, 95, (60, 80), (320, 264), 0.9, pre=False)])


SYNTH = {'E': case_e, 'F': case_f, 'G': case_g, 'H': case_h, 'I': case_i, 'K': case_k}


# ---- the regimes of the two kernels ----------------------------------------------------------------------------------
def kernel_constants():
    """CT_INPUTS_TILE_W / _H / DESC_WORDS of the header, as csrc/inputs.hip uses them"""
    hdr = open(os.path.join(ROOT, 'include', 'centertrack_hip.h')).read()
    src = open(os.path.join(ROOT, 'centertrack_amd', 'csrc', 'inputs.hip')).read()
    assert 'constexpr int IN_TW = CT_INPUTS_TILE_W, IN_TH = CT_INPUTS_TILE_H, IN_DESC = CT_INPUTS_DESC_WORDS;' in src
    return {'TW': int(re.search(r'#define CT_INPUTS_TILE_W (\d+)', hdr).group(1)),
            'TH': int(re.search(r'#define CT_INPUTS_TILE_H (\d+)', hdr).group(1)),
            'DESC': int(re.search(r'#define CT_INPUTS_DESC_WORDS (\d+)', hdr).group(1))}


def partials(K, ib):
    return -(-ib.W // K['TW']) * -(-ib.H // K['TH'])


def regimes(K):
    """name -> predicate(ib, samples): what the kernels branch on (csrc/inputs.hip)"""
    def recs(samples):
        return [r for s in samples for r in s if r is not None]

    return {
        'several tiles on both axes': lambda ib, s: ib.W > K['TW'] and ib.H > K['TH'],
        'output narrower than a wave': lambda ib, s: ib.W < 64,
        'output lower than a tile': lambda ib, s: ib.H < K['TH'],
        'ragged last tile in x': lambda ib, s: ib.W % K['TW'] != 0,
        'ragged last tile in y': lambda ib, s: ib.H % K['TH'] != 0,
        'exact tiles in y': lambda ib, s: ib.H % K['TH'] == 0,
        'one partial per image': lambda ib, s: partials(K, ib) == 1,
        'partials, fewer than a wave': lambda ib, s: 1 < partials(K, ib) < 64,
        'more partials than a wave': lambda ib, s: partials(K, ib) > 64,
        'image and pre_img': lambda ib, s: all(p is not None for _, p in s),
        'image only': lambda ib, s: all(p is None for _, p in s),
        'a batch with a missing pre_img': lambda ib, s: len({p is None for _, p in s}) == 2,
        'flipped and not': lambda ib, s: len({r['flipped'] for r in recs(s)}) == 2,
        'colour on and off in one batch': lambda ib, s: len({r['color'] is None for r in recs(s)}) == 2,
        'a row pitch above 3 w': lambda ib, s: any(r['rows'].shape[0] and r['rows'].strides[0] > 3 * r['w'] for r in recs(s)),
        'cropped rows (row0 > 0 and fewer than h)': lambda ib, s: any(r['row0'] > 0 and r['rows'].shape[0] < r['h'] for r in recs(s)),
        'whole frame uploaded': lambda ib, s: any(r['rows'].shape[0] == r['h'] for r in recs(s)),
        'a 1 x 1 source': lambda ib, s: any(r['h'] == 1 and r['w'] == 1 for r in recs(s)),
        'rotation': lambda ib, s: any(r['trans'][0, 1] != 0 for r in recs(s)),
        'sources of different sizes': lambda ib, s: len({(r['h'], r['w']) for r in recs(s)}) > 1,
    }
