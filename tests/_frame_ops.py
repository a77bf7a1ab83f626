"""The kernels an inference frame runs besides the convolutions, the DCN and the heat-map decode, restated for the tests:
the fused 7x7 stems (csrc/stem.hip), the fused heads (the HEADS instance of wino_body, csrc/wino_mfma.hip), the flip_test merge and
mirror (csrc/flip.hip), the prior heat map (render_pre_hm_kernel, csrc/elementwise.hip) and the pose match (csrc/pose.hip).  Per
family: the host's launch plan in Python, a regime table (a hashable key -> the source line it restates), the case list
tests/test_frame_ops_cpu.py proves complete and tests/test_hip_frame_ops.py runs on the GPU, the float64 reference with its float32
yardstick, and the mutations of the reference that the named cases must tell from it.  No GPU, no ctypes.

THE ERROR MEASURE.  Float results (stem, heads): e = err(got, ref64), e32 = err(ref32, ref64), e <= bound(e32, K) with the
project's bound = min(1e-3, 4 max(e32, 2^-23 sqrt(K))); K = 147 per image stem + 49 for pre_hm over the stems of the launch,
K = 576 + 256 for a head; ref32 is the torch fp32 composition (stem) and ``winograd32`` followed by the fp32 epilogue (heads).
Selections and exact arithmetic (flip, key points) compare bit for bit.  ``ct_render_pre_hm`` compares with the float64 max-splat
of its own formula cast to float32: 1 float32 ulp per value, fewer than 1e-3 of the touched pixels not bit-equal.

NOT OBSERVABLE THROUGH THE ABI, mirrored by reading: the stem's tile height (``stem_plan``: rows16), the k -> patch-offset table of
stem_kernel (``stem_tab``), the workgroup order of the fused heads (``heads_plan``), which of the two flip kernels runs
(``flip_plan``).  tests/test_frame_ops_cpu.py reads the constants and the padding rule of ``tab[]`` back from the source."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from _conv_fwd import winograd32
from _dcn_bwd import bound, cdiv, err, randn

# constants of the sources (tests/test_frame_ops_cpu.py reads them back)
ST_TW, ST_PW, ST_KTOT = 32, 40, 348
ST_ROWS16_ABOVE, ST_ROWS16_UPTO = 768, 1536          # rows16 = blocks8 > 768 && blocks8 <= 1536
PHM_TW, PHM_TH, PHM_CAP = 32, 8, 256
FLIP_MAX_HEADS, FLIP_MAX_JOINTS, FLIP_BLOCK_CAP = 8, 64, 4096
CT_MAX_FUSED_HEADS = 8
POSE_THRESH, POSE_BLOCK = np.float32(0.2), 128
KNOBS = {'stem_rows': 0, 'heads_order': 2}           # the defaults every test restores
FLIP_AVG, FLIP_NEG_EVEN, FLIP_JOINTS, FLIP_JOINT_OFFSETS = range(4)
COCO_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
DEPTH_SCALE = 2.0


def _missing(regimes, keys_of, cases):
    reached = set()
    for c in cases:
        reached |= keys_of(c)
    assert reached <= set(regimes), sorted(map(str, reached - set(regimes)))
    return [k for k in regimes if k not in reached]


def owned(keys_of, cases):
    """{case name: the keys only this case reaches}"""
    count = collections.Counter(k for c in cases for k in keys_of(c))
    return {c.name: sorted((k for k in keys_of(c) if count[k] == 1), key=str) for c in cases}


def _rand01(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the stem

STEM_K = (147, 147, 49)
STEM_TAB_PADDING = '(3 * s) * ST_PS'                 # stem_kernel: what ``int off`` holds for a padding k


def st_k4(s):
    return 52 if s == 2 else 148


def st_koff(s):
    return 148 * s


def stem_tab(k):
    """stem_kernel's tab[k] as (plane, row, column) of the patch: k = (ci, ky, kx) of stem s -> plane 3 s + ci; a padding k
    (147 of stems 0 and 1, 49..51 of stem 2, zero weight) -> the stem's own first plane"""
    s = 2 if k >= 296 else 1 if k >= 148 else 0
    kk, cin = k - st_koff(s), 1 if s == 2 else 3
    if kk < cin * 49:
        c, r = divmod(kk, 49)
        return 3 * s + c, r // 7, r % 7
    return 3 * s, 0, 0


def stem_staged_planes(mask):
    """the LDS planes a launch of the stems in ``mask`` stages (stage_store: planes[(3 s + c) * ST_PS ...])"""
    return {3 * s + c for s in range(3) if mask >> s & 1 for c in range(1 if s == 2 else 3)}


def stem_visited(mask):
    """every k the MFMA loop of an active stem visits: k = st_koff(s) + 4 st + lg, st < st_k4(s) / 4, lg < 4"""
    return [st_koff(s) + k for s in range(3) if mask >> s & 1 for k in range(st_k4(s))]


def stem_plan(N, H, W, knob=0):
    """ct_stem_forward_parts: tilesX, blocks8, rows16, tilesY, the grid.  rows16 is not observable through the ABI (both tile
    heights give the same bits): mirrored by reading"""
    tilesX = cdiv(W, ST_TW)
    blocks8 = N * tilesX * cdiv(H, 8)
    rows16 = knob == 16 or (knob == 0 and ST_ROWS16_ABOVE < blocks8 <= ST_ROWS16_UPTO)
    tilesY = cdiv(H, 16 if rows16 else 8)
    return dict(tilesX=tilesX, tilesY=tilesY, blocks8=blocks8, rows16=rows16, grid=N * tilesX * tilesY)


StemCase = collections.namedtuple('StemCase', 'name N H W mask add ldadd ldy knob why')
SUBSET_SHAPE = (3, 9, 33)                            # three images, 2 x 2 tiles, both ragged
STEM_GEO = [(1, 1), (1, 33), (7, 31), (8, 32)]       # (9 x 33 is the subset shape)
STEM_ROWS_H = [17, 24, 25, 31]                       # H % 16 = 1, 8, 9, 15
STEM_AUTO = [(6144, 768), (6145, 769), (12288, 1536), (12289, 1537)]     # H at W = 5, N = 1 -> blocks8


def _stem_cases():
    out = []
    N, H, W = SUBSET_SHAPE
    for mask in range(1, 8):
        for add in (0, 1):
            parts = '+'.join(n for s, n in enumerate(('x', 'pre_img', 'pre_hm')) if mask >> s & 1)
            out.append(StemCase('m%d%s' % (mask, '_add' if add else ''), N, H, W, mask, add, (24 if mask & 1 else 16) if add else 0,
                                24 if (mask + add) & 1 else 16, 0, '{%s}%s at three images and 2 x 2 ragged tiles' % (parts, ' on a partial map' if add else '')))
    for h, w in STEM_GEO:
        out.append(StemCase('geo_%dx%d' % (h, w), 1, h, w, 7, 0, 0, 16, 0, 'the tile edges at %d x %d' % (h, w)))
    for h in STEM_ROWS_H:
        out.append(StemCase('rows16_h%d' % h, 1, h, 40, 7, 1, 16, 16, 16, 'H %% 16 = %d on 16-row tiles (the second slab %s)'
                            % (h % 16, 'empty' if 0 < h % 16 <= 8 else 'ragged')))
    for h, b8 in STEM_AUTO:
        out.append(StemCase('auto_%d' % b8, 1, h, 5, 7, 0, 0, 16, 0, 'blocks8 = %d: the knob at 0 picks %d-row tiles'
                            % (b8, 16 if ST_ROWS16_ABOVE < b8 <= ST_ROWS16_UPTO else 8)))
    return out


STEM_CASES = _stem_cases()
STEM_CASE = collections.OrderedDict((c.name, c) for c in STEM_CASES)


def _stem_regimes():
    r = collections.OrderedDict()
    for mask in range(1, 8):
        for add in (False, True):
            r[('subset', mask, add)] = ('stem_kernel: a.in[] = %s, a.add %s; first / nxt / have_next, src = a.in[s] + n * cin * HW, at N > 1 and '
                                        'more than one tile each way' % (format(mask, '03b')[::-1], 'given' if add else 'null'))
    for ld in (16, 24):
        r[('ldadd', ld)] = 'stem_kernel: a.add[(...) * a.ldadd + li]'
        r[('ldy', ld)] = 'stem_kernel: a.y[(...) * a.ldy + li]'
    for n in (1, 3):
        r[('N', n)] = 'stem_kernel: n = bid / (tilesX * tilesY)'
    for h, w in STEM_GEO + [SUBSET_SHAPE[1:]]:
        r[('geo', h, w)] = 'stem_kernel: ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W; oy < a.H && ox < a.W'
    for h in STEM_ROWS_H:
        r[('H%16', h % 16)] = 'stem_kernel<16>: oy = oy0 + 8 * h + 2 * wave + (mt >> 1); if (oy >= a.H) continue'
    r['rows8'] = 'ct_stem_forward_parts: stem_kernel<8>'
    r['rows16'] = 'ct_stem_forward_parts: stem_kernel<16>'
    for b8 in (768, 769, 1536, 1537):
        r[('auto', b8)] = 'ct_stem_forward_parts: rows16 = want == 16 || (want == 0 && blocks8 > 768 && blocks8 <= 1536)'
    return r


STEM_REGIMES = _stem_regimes()


def stem_keys(c):
    p = stem_plan(c.N, c.H, c.W, c.knob)
    k = {('ldy', c.ldy), ('N', c.N), 'rows16' if p['rows16'] else 'rows8'}
    if c.N > 1 and p['tilesX'] > 1 and p['tilesY'] > 1:
        k.add(('subset', c.mask, bool(c.add)))
    if c.add:
        k.add(('ldadd', c.ldadd))
    if ('geo', c.H, c.W) in STEM_REGIMES:
        k.add(('geo', c.H, c.W))
    if c.knob == 16 and c.H in STEM_ROWS_H:
        k.add(('H%16', c.H % 16))
    if c.knob == 0 and ('auto', p['blocks8']) in STEM_REGIMES:
        k.add(('auto', p['blocks8']))
    return k


def missing_stem_regimes(cases):
    return _missing(STEM_REGIMES, stem_keys, cases)


@functools.lru_cache(maxsize=None)
def stem_inputs(N, H, W):
    """fp32: the three inputs (pre_hm in [0, 1)), the three weights, scale in [0.5, 1.5), shift, and a partial map"""
    s = 1000 + 131 * N + 17 * H + W
    d = dict(inp=[randn(s, N, 3, H, W).float(), randn(s + 1, N, 3, H, W).float(), _rand01(s + 2, N, 1, H, W).float()],
             w=[(randn(s + 3, 16, 3, 7, 7) * 0.1).float(), (randn(s + 4, 16, 3, 7, 7) * 0.1).float(), (randn(s + 5, 16, 1, 7, 7) * 0.2).float()],
             scale=(_rand01(s + 6, 3, 16) + 0.5).float(), shift=(randn(s + 7, 3, 16) * 0.3).float(), add=randn(s + 8, N, 16, H, W).float())
    return d


STEM_MUTATIONS = collections.OrderedDict([
    ('a', 'a halo of 2 instead of 3: the outer ring of the 7 x 7 window reads zero'),
    ('b', 'ReLU after the sum instead of per stem'),
    ('c', 'pre_hm read with the image stride 3 HW (image n from plane 3 n, zero past the tensor)'),
    ('d', 'the add term dropped'),
])


def stem_compose(d, mask, add, dt, mutation=None):
    """add + relu(bn0(conv(x))) + relu(bn1(conv(pre_img))) + relu(bn2(conv(pre_hm))) over the stems of ``mask``, in ``dt``, in the
    kernel's order of terms"""
    N, _, H, W = d['inp'][0].shape
    y = d['add'].to(dt).clone() if add and mutation != 'd' else torch.zeros((N, 16, H, W), dtype=dt)
    for s in range(3):
        if not mask >> s & 1:
            continue
        x, w = d['inp'][s].to(dt), d['w'][s].to(dt)
        if mutation == 'a':
            w = w.clone()
            w[:, :, 0], w[:, :, 6], w[:, :, :, 0], w[:, :, :, 6] = 0, 0, 0, 0
        if mutation == 'c' and s == 2:
            flat, x = x.reshape(-1), torch.zeros_like(x)
            for n in range(N):
                if (3 * n + 1) * H * W <= flat.numel():
                    x[n, 0] = flat[3 * n * H * W:(3 * n + 1) * H * W].view(H, W)
        z = F.conv2d(x, w, padding=3) * d['scale'][s].to(dt).view(1, 16, 1, 1) + d['shift'][s].to(dt).view(1, 16, 1, 1)
        y = y + (z if mutation == 'b' else torch.relu(z))
    return torch.relu(y) if mutation == 'b' else y


def stem_K(mask):
    return sum(k for s, k in enumerate(STEM_K) if mask >> s & 1)


@functools.lru_cache(maxsize=None)
def stem_refs(N, H, W, mask, add):
    """(ref64, e32, bound) of a launch, once per process"""
    d = stem_inputs(N, H, W)
    r64 = stem_compose(d, mask, add, torch.float64)
    e32 = err(stem_compose(d, mask, add, torch.float32), r64)
    return r64, e32, bound(e32, stem_K(mask))


def stem_errors(case, got):
    r64, e32, b = stem_refs(case.N, case.H, case.W, case.mask, bool(case.add))
    return err(got, r64), e32, b


# ---------------------------------------------------------------------------------------------------------------------
# the fused heads

HeadsCase = collections.namedtuple('HeadsCase', 'name N H W cout coff ctot sig dep ldx why')


def heads_plan(N, H, W, nheads):
    """ct_heads_fused and the head-major orders of wino_body<HEADS>: one workgroup per (64-pixel tile, head).  The order is a
    speed knob, not observable through the ABI: mirrored by reading"""
    tilesX, tilesY = cdiv(W, 16), cdiv(H, 4)
    nblocks = N * tilesX * tilesY * nheads
    per, per_head = nblocks >> 3, nblocks // nheads
    straddles = per > 0 and any((x * per) // per_head != ((x + 1) * per - 1) // per_head for x in range(8))
    return dict(tilesX=tilesX, tilesY=tilesY, nblocks=nblocks, per=per, per_head=per_head, straddles=straddles)


def heads_order2(bid, nblocks, nheads):
    """(head, tile) of workgroup ``bid`` under heads_order 2"""
    per, per_head = nblocks >> 3, nblocks // nheads
    lin = (bid & 7) * per + (bid >> 3) if bid < per * 8 else bid
    return lin // per_head, lin % per_head


HEADS_CASES = [
    HeadsCase('one', 1, 4, 16, (2,), (0,), 2, None, None, 64, 'one head, one full tile, one workgroup, no sigmoid and no depth range'),
    HeadsCase('tiny', 1, 1, 1, (3, 1), (0, 3), 4, 1, None, 64, 'one pixel: every other lane of the tile is outside the map'),
    HeadsCase('slice', 2, 3, 15, (1, 2, 2, 2, 4), (0, 1, 3, 5, 7), 11, 0, None, 96, 'five heads on a channel slice of a 96-wide buffer, ragged both ways'),
    HeadsCase('eight', 2, 5, 17, (1, 2, 3, 4, 5, 6, 7, 8), (8, 27, 15, 29, 33, 9, 20, 0), 40, 3, 5, 64,
              'eight heads of every width, coff permuted with gaps at [18, 20) and [38, 40), sigmoid on head 3, depth on head 5, 64 workgroups'),
    HeadsCase('mot45', 1, 12, 40, (1, 2, 2, 2, 4), (0, 1, 3, 5, 7), 11, 0, None, 64, '45 workgroups: five keep their place, an eighth of five straddles a head of nine'),
]
HEADS_CASE = collections.OrderedDict((c.name, c) for c in HEADS_CASES)


def _heads_regimes():
    r = collections.OrderedDict()
    for n in (1, 5, 8):
        r[('nheads', n)] = 'ct_heads_fused: a.coutBlocks = d->nheads'
    for c in range(1, 9):
        r[('width', c)] = 'wino_body<HEADS>: if (j >= hc) break'
    r['coff:permuted'] = 'wino_body<HEADS>: gc = g0 + j with g0 = a.hcoff[cb] not ascending in cb'
    r['coff:gap'] = 'ct_heads_fused: coff[i] + cout[i] <= ctot is all that is asked: channels no head owns are not written'
    r['sig:not-head-0'] = 'ct_epilogue_value: co >= e.sig_lo && co < e.sig_hi'
    r['dep'] = 'ct_epilogue_value: co >= e.dep_lo && co < e.dep_hi'
    r['sig,dep:empty'] = 'ct_epilogue_value: sig_lo == sig_hi, dep_lo == dep_hi'
    for ld in (64, 96):
        r[('ldx', ld)] = 'wino_body: xin = a.x + n * a.H * a.W * a.ldx'
    for h in (1, 3, 4, 5):
        r[('H', h)] = 'wino_body<HEADS>: if (oy >= a.epi.Ho || ox >= a.epi.Wo) continue'
    for w in (1, 15, 16, 17):
        r[('W', w)] = 'wino_body<HEADS>: if (oy >= a.epi.Ho || ox >= a.epi.Wo) continue'
    for n in (1, 2):
        r[('N', n)] = 'wino_body: n = bid / (tilesX * tilesY)'
    r['order2:per=0'] = 'wino_body<HEADS>: per = nblocks >> 3 == 0, lin = ubid'
    r['order2:nblocks%8=0'] = 'wino_body<HEADS>: lin = (ubid & 7) * per + (ubid >> 3) for every workgroup'
    r['order2:nblocks%8=5'] = 'wino_body<HEADS>: the last nblocks % 8 keep their place'
    r['order2:straddle'] = 'wino_body<HEADS>: cb = lin / per_head changes inside [x * per, (x + 1) * per)'
    r['hidden:dead+live'] = 'wino_body<HEADS>: fmaxf(v + b0, 0) with hidden channels negative everywhere and positive everywhere'
    return r


HEADS_REGIMES = _heads_regimes()


def heads_keys(c):
    p = heads_plan(c.N, c.H, c.W, len(c.cout))
    k = {('ldx', c.ldx), ('N', c.N), 'hidden:dead+live'} | {('width', w) for w in c.cout}
    for key in (('nheads', len(c.cout)), ('H', c.H), ('W', c.W)):
        if key in HEADS_REGIMES:
            k.add(key)
    if list(c.coff) != sorted(c.coff):
        k.add('coff:permuted')
    if sum(c.cout) < c.ctot:
        k.add('coff:gap')
    if c.sig is not None and c.sig != 0:
        k.add('sig:not-head-0')
    if c.dep is not None:
        k.add('dep')
    if c.sig is None and c.dep is None:
        k.add('sig,dep:empty')
    if p['per'] == 0:
        k.add('order2:per=0')
    elif p['nblocks'] % 8 in (0, 5):
        k.add('order2:nblocks%%8=%d' % (p['nblocks'] % 8))
    if p['straddles']:
        k.add('order2:straddle')
    return k


def missing_heads_regimes(cases):
    return _missing(HEADS_REGIMES, heads_keys, cases)


HIDDEN_DEAD, HIDDEN_LIVE, HIDDEN_BIAS = slice(0, 32), slice(32, 64), 5.0


@functools.lru_cache(maxsize=None)
def heads_inputs(name):
    """fp32: a post-ReLU feature map, per head w0 [256,64,3,3], b0 [256] (hidden channels 0..31 at -5: negative everywhere, 32..63
    at +5: positive everywhere), w2 [c,256], b2 [c] (the depth head's at -6: a sigmoid near 0, where the 1e-6 counts)"""
    c = HEADS_CASE[name]
    s = 2000 + sum(map(ord, name))
    d = dict(x=torch.relu(randn(s, c.N, 64, c.H, c.W)).float(), w0=[], b0=[], w2=[], b2=[])
    for i, co in enumerate(c.cout):
        d['w0'].append((randn(s + 10 + i, 256, 64, 3, 3) * 576 ** -0.5).float())
        b0 = randn(s + 20 + i, 256) * 0.2
        b0[HIDDEN_DEAD], b0[HIDDEN_LIVE] = -HIDDEN_BIAS, HIDDEN_BIAS
        d['b0'].append(b0.float())
        d['w2'].append((randn(s + 30 + i, co, 256) * 256 ** -0.5).float())
        d['b2'].append((randn(s + 40 + i, co) - (6.0 if i == c.dep else 0.0)).float())
    return d


def heads_ranges(c, mutation=None):
    """(sig_lo, sig_hi, dep_lo, dep_hi) in output channels"""
    sig = (c.coff[c.sig], c.coff[c.sig] + c.cout[c.sig]) if c.sig is not None else (0, 0)
    dep = (c.coff[c.dep], c.coff[c.dep] + c.cout[c.dep]) if c.dep is not None else (0, 0)
    if mutation == 'b':
        sig = (sig[0] + 1, sig[1] + 1)
    return sig + dep


HEADS_MUTATIONS = collections.OrderedDict([
    ('a', 'no ReLU on the hidden layer'),
    ('b', 'the sigmoid range shifted by one channel'),
    ('c', 'the depth transform without its + 1e-6'),
    ('d', "a head's 1x1 rows taken from its neighbour"),
])


def heads_compose(name, dt, conv=None, mutation=None):
    """[N, ctot, H, W] in ``dt`` (NaN where no head writes): conv3x3 + b0, ReLU, the 1x1 layer + b2 per head, then sigmoid and the
    depth transform by output channel range, as ct_epilogue_value applies them"""
    c, d = HEADS_CASE[name], heads_inputs(name)
    x = d['x'].to(dt)
    out = torch.full((c.N, c.ctot, c.H, c.W), float('nan'), dtype=dt)
    nh = len(c.cout)
    for i in range(nh):
        w0 = d['w0'][i].to(dt)
        hid = (F.conv2d(x, w0, padding=1) if conv is None else conv(x, w0)) + d['b0'][i].to(dt).view(1, 256, 1, 1)
        if mutation != 'a':
            hid = torch.relu(hid)
        w2 = d['w2'][i]
        if mutation == 'd':
            nb = d['w2'][(i + 1) % nh]
            w2 = torch.stack([nb[j % nb.shape[0]] for j in range(c.cout[i])])
        y = torch.einsum('oc,nchw->nohw', w2.to(dt), hid) + d['b2'][i].to(dt).view(1, -1, 1, 1)
        out[:, c.coff[i]:c.coff[i] + c.cout[i]] = y
    slo, shi, dlo, dhi = heads_ranges(c, mutation)
    out[:, slo:shi] = torch.sigmoid(out[:, slo:shi])
    out[:, dlo:dhi] = (1.0 / (torch.sigmoid(out[:, dlo:dhi]) + (0.0 if mutation == 'c' else 1e-6)) - 1.0) * DEPTH_SCALE
    return out


HEADS_K = 576 + 256


@functools.lru_cache(maxsize=None)
def heads_refs(name):
    """(ref64, [e32 per head]) once per process; ref32 = winograd32, then bias, ReLU, the 1x1 layer, bias, transforms in fp32"""
    c = HEADS_CASE[name]
    r64, r32 = heads_compose(name, torch.float64), heads_compose(name, torch.float32, winograd32)
    return r64, [err(_head(c, r32, i), _head(c, r64, i)) for i in range(len(c.cout))]


def _head(c, t, i):
    return t[:, c.coff[i]:c.coff[i] + c.cout[i]]


def heads_errors(name, got):
    """[(head, err, e32, bound)]: every head by its own norm, so that the depth head's range does not hide the others"""
    c = HEADS_CASE[name]
    r64, e32 = heads_refs(name)
    return [(i, err(_head(c, got, i), _head(c, r64, i)), e32[i], bound(e32[i], HEADS_K)) for i in range(len(c.cout))]


def heads_unowned(c):
    own = np.zeros(c.ctot, bool)
    for co, off in zip(c.cout, c.coff):
        own[off:off + co] = True
    return ~own


# ---------------------------------------------------------------------------------------------------------------------
# flip_test: the merge and the mirror

FlipCase = collections.namedtuple('FlipCase', 'name B h w heads pairs src why')       # heads: ((C, mode), ..); src: how the source lies
ImgCase = collections.namedtuple('ImgCase', 'name rows W src why')
_CAP_H = 61681                                                                        # 2^20 + 1 = 17 * 61681


FLIP_CASES = [
    FlipCase('eight', 2, 6, 12, ((1, FLIP_AVG), (2, FLIP_AVG), (2, FLIP_NEG_EVEN), (17, FLIP_JOINTS), (34, FLIP_JOINT_OFFSETS), (3, FLIP_AVG),
                                 (8, FLIP_AVG), (4, FLIP_NEG_EVEN)), COCO_PAIRS, 'slices',
             'the four modes in one 8-head call, 1 to 34 channels: the grid is sized by hps, hm relies on its loop guard; channel slices of one tensor'),
    FlipCase('w13', 1, 5, 13, ((17, FLIP_JOINTS), (34, FLIP_JOINT_OFFSETS), (2, FLIP_NEG_EVEN)), COCO_PAIRS, 'dense', 'w % 4 != 0: the scalar kernel'),
    FlipCase('src_plus4', 1, 3, 8, ((2, FLIP_NEG_EVEN), (3, FLIP_AVG)), (), 'offset', 'w % 4 == 0 but src starts 4 bytes past a 16-byte boundary'),
    FlipCase('stride_odd', 2, 3, 8, ((2, FLIP_AVG), (4, FLIP_NEG_EVEN)), (), 'stride+1', 'src_batch_stride = C h w + 1: images 1.. are not 16-byte aligned'),
    FlipCase('chained', 1, 4, 8, ((4, FLIP_JOINTS), (8, FLIP_JOINT_OFFSETS)), ((0, 1), (1, 2), (0, 3)), 'dense',
             "pairs that share joints: the reference's successive swaps, not an involution"),
    FlipCase('cap_vec', 1, _CAP_H, 68, ((1, FLIP_AVG),), (), 'dense', 'total / 4 = 2^20 + 1: 4097 workgroups wanted, 4096 launched, the grid-stride loop runs twice'),
    FlipCase('cap_scalar', 1, _CAP_H, 17, ((1, FLIP_NEG_EVEN),), (), 'dense', 'total = 2^20 + 1 in the scalar kernel'),
]
FLIP_CASE = collections.OrderedDict((c.name, c) for c in FLIP_CASES)
IMG_CASES = [
    ImgCase('img_vec', 7, 12, 'dense', 'the 16-byte form'),
    ImgCase('img_w13', 7, 13, 'dense', 'W % 4 != 0'),
    ImgCase('img_src_plus4', 5, 8, 'offset', 'src 4 bytes past a 16-byte boundary'),
    ImgCase('img_cap_vec', _CAP_H, 68, 'dense', 'rows * W / 4 = 2^20 + 1'),
    ImgCase('img_cap_scalar', _CAP_H, 17, 'dense', 'rows * W = 2^20 + 1'),
]
IMG_CASE = collections.OrderedDict((c.name, c) for c in IMG_CASES)


def flip_blocks(threads):
    return max(1, min(FLIP_BLOCK_CAP, cdiv(threads, 256)))


def flip_plan(c):
    """ct_flip_merge: which kernel, the grid (x by the largest head), whether the cap cuts it.  Mirrored by reading"""
    aligned = c.src in ('dense', 'slices')
    vec = c.w % 4 == 0 and aligned
    most = max(c.B * C * c.h * c.w for C, _ in c.heads)
    threads = most // 4 if vec else most
    return dict(vec=vec, grid_x=flip_blocks(threads), capped=cdiv(threads, 256) > FLIP_BLOCK_CAP,
                why_scalar=None if vec else 'w%4' if c.w % 4 else {'offset': 'src-misaligned', 'stride+1': 'stride%4'}[c.src])


def img_plan(c):
    vec = c.W % 4 == 0 and c.src == 'dense'
    threads = c.rows * (c.W // 4 if vec else c.W)
    return dict(vec=vec, grid_x=flip_blocks(threads), capped=cdiv(threads, 256) > FLIP_BLOCK_CAP)


FLIP_REGIMES = collections.OrderedDict([
    ('merge:vec', 'ct_flip_merge: flip_merge_kernel<true>'),
    ('merge:scalar:w%4', 'ct_flip_merge: bool vec = (w & 3) == 0'),
    ('merge:scalar:src-misaligned', 'ct_flip_merge: (((uintptr_t)hd.src | (uintptr_t)hd.dst) & 15) == 0'),
    ('merge:scalar:stride%4', 'ct_flip_merge: (hd.src_batch_stride & 3) == 0'),
] + [
    (('mode', m, form), 'flip_merge_kernel<%s>: %s' % ('true' if form == 'vec' else 'false', line))
    for form in ('vec', 'scalar') for m, line in ((FLIP_AVG, 'cs = c, sgn = 1'), (FLIP_NEG_EVEN, 'sgn = (c & 1) ? 1.0f : -1.0f'), (FLIP_JOINTS, 'cs = a.partner[c]'),
                                                   (FLIP_JOINT_OFFSETS, 'cs = 2 * a.partner[c >> 1] + (c & 1)'))
] + [
    ('merge:8-heads', 'ct_flip_merge: nheads <= FLIP_MAX_HEADS, grid.y = nheads'),
    ('merge:unequal-heads', 'flip_merge_kernel: idx < total with total of the head, the grid sized by the largest'),
    ('merge:stride>image', 'flip_merge_kernel: s0 = hd.src + b * hd.src_batch_stride'),
    ('merge:pairs-chained', 'ct_flip_merge: successive swaps of a.partner[u], a.partner[v]'),
    ('merge:cap:vec', 'blocks_for: if (b > 4096) b = 4096, flip_merge_kernel<true>'),
    ('merge:cap:scalar', 'blocks_for: if (b > 4096) b = 4096, flip_merge_kernel<false>'),
    ('img:vec', 'ct_flip_images: flip_rows_kernel<true>'),
    ('img:scalar:W%4', 'ct_flip_images: vec = (W & 3) == 0'),
    ('img:scalar:src-misaligned', 'ct_flip_images: (((uintptr_t)src | (uintptr_t)dst) & 15) == 0'),
    ('img:cap:vec', 'blocks_for: if (b > 4096) b = 4096, flip_rows_kernel<true>'),
    ('img:cap:scalar', 'blocks_for: if (b > 4096) b = 4096, flip_rows_kernel<false>'),
])


def flip_keys(c):
    if isinstance(c, ImgCase):
        p = img_plan(c)
        if p['capped']:
            return {'img:cap:vec' if p['vec'] else 'img:cap:scalar'}
        return {'img:vec' if p['vec'] else 'img:scalar:W%4' if c.W % 4 else 'img:scalar:src-misaligned'}
    p = flip_plan(c)
    k = {'merge:vec' if p['vec'] else 'merge:scalar:' + p['why_scalar']} | {('mode', m, 'vec' if p['vec'] else 'scalar') for _, m in c.heads}
    if p['capped']:
        k.add('merge:cap:vec' if p['vec'] else 'merge:cap:scalar')
    if len(c.heads) == FLIP_MAX_HEADS:
        k.add('merge:8-heads')
    if len({C for C, _ in c.heads}) > 1 and p['grid_x'] > flip_blocks(min(c.B * C * c.h * c.w for C, _ in c.heads) // (4 if p['vec'] else 1)):
        k.add('merge:unequal-heads')
    if c.src in ('slices', 'stride+1'):
        k.add('merge:stride>image')
    joints = [j for pr in c.pairs for j in pr]
    if len(joints) != len(set(joints)):
        k.add('merge:pairs-chained')
    return k


def missing_flip_regimes(cases):
    return _missing(FLIP_REGIMES, flip_keys, cases)


@functools.lru_cache(maxsize=None)
def flip_inputs(name):
    """per head a float32 [2B, C, h, w]"""
    c = FLIP_CASE[name]
    rng = np.random.default_rng(3000 + sum(map(ord, name)))
    out = [rng.standard_normal((2 * c.B, C, c.h, c.w), dtype=np.float32) for C, _ in c.heads]
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def img_inputs(name):
    c = IMG_CASE[name]
    v = np.random.default_rng(3500 + sum(map(ord, name))).standard_normal((c.rows, c.W), dtype=np.float32)
    v.setflags(write=False)
    return v


FLIP_MUTATIONS = collections.OrderedDict([
    ('a', 'the sign on the odd instead of the even channels'),
    ('b', "hps: the partner of the channel instead of the partner of the joint"),
    ('c', 'no mirror inside a 4-pixel group'),
])


def _mirror(f, mutation=None):
    if mutation == 'c' and f.shape[-1] % 4 == 0:
        g = f.reshape(f.shape[:-1] + (f.shape[-1] // 4, 4))
        return g[..., ::-1, :].reshape(f.shape)
    return f[..., ::-1]


def flip_reference(name, mutation=None):
    """Detector._flip_output per stream in float32: (a + flipped(b)) / 2 with flip_tensor / flip_lr / flip_lr_off -- the mirror,
    then the reference's successive channel swaps over ``pairs``, the x offsets negated"""
    c = FLIP_CASE[name]
    out = []
    for src, (C, mode) in zip(flip_inputs(name), c.heads):
        a, f = src[:c.B], _mirror(src[c.B:], mutation).copy()
        if mode == FLIP_NEG_EVEN:
            f[:, (1 if mutation == 'a' else 0)::2] *= -1
        elif mode == FLIP_JOINTS or (mode == FLIP_JOINT_OFFSETS and mutation == 'b'):
            if mode == FLIP_JOINT_OFFSETS:
                f[:, 0::2] *= -1
            for u, v in c.pairs:
                f[:, [u, v]] = f[:, [v, u]]
        elif mode == FLIP_JOINT_OFFSETS:
            g = f.reshape(c.B, C // 2, 2, c.h, c.w)
            g[:, :, (1 if mutation == 'a' else 0)] *= -1
            for u, v in c.pairs:
                g[:, [u, v]] = g[:, [v, u]]
            f = g.reshape(c.B, C, c.h, c.w)
        out.append((a + f) / np.float32(2))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the prior heat map

PhmCase = collections.namedtuple('PhmCase', 'name B H W cap counts flipped why')
PHM_CASES = [
    PhmCase('p_1x1', 1, 1, 1, 4, (3,), 0, 'one pixel: a blob of r = 0 on it, an entry of r < 0, a blob wholly off the map'),
    PhmCase('p_8x32', 3, 8, 32, 8, (0, 1, 5), 1, 'three streams of 0, 1 and 5 blobs on one tile each, with the flipped copy'),
    PhmCase('p_9x33', 1, 9, 33, 257, (300,), 0, 'counts > cap: 257 blobs count, the last 43 rows of the 300 written are not there to read; a second cull round of one blob'),
    PhmCase('p_40x72', 2, 40, 72, 600, (256, 600), 1, '256 blobs (one full cull round) and 600 (three rounds); partly and wholly off every side; overlaps'),
]
PHM_CASE = collections.OrderedDict((c.name, c) for c in PHM_CASES)


def phm_plan(c, b):
    n = min(c.counts[b], c.cap)
    return dict(n=n, rounds=max(1, cdiv(n, PHM_CAP)), grid=c.B * cdiv(c.H, PHM_TH) * cdiv(c.W, PHM_TW))


@functools.lru_cache(maxsize=None)
def phm_params(name):
    """int32 [B, cap, 3] rows (cx, cy, r); rows past counts[b] (and past cap in the caller's mind) hold a blob that would show"""
    c = PHM_CASE[name]
    rng = np.random.default_rng(4000 + sum(map(ord, name)))
    p = np.zeros((c.B, c.cap, 3), np.int32)
    p[:, :, 0], p[:, :, 1] = rng.integers(0, c.W, (c.B, c.cap)), rng.integers(0, c.H, (c.B, c.cap))
    p[:, :, 2] = rng.integers(0, 6, (c.B, c.cap))
    if name == 'p_1x1':
        p[0, :4] = [(0, 0, 0), (0, 0, -1), (5, 5, 2), (0, 0, 3)]                   # (the fourth is past counts)
    if name == 'p_9x33':
        p[0, 256] = (16, 4, 2)                                                       # the one blob of the second round
    if name == 'p_40x72':
        W, H = c.W, c.H
        p[1, :12] = [(-2, 20, 4), (W + 1, 20, 4), (30, -2, 4), (30, H + 1, 4),       # partly off: left, right, top, bottom
                     (-10, 20, 4), (W + 10, 20, 4), (30, -10, 4), (30, H + 10, 4),   # wholly off
                     (50, 10, 0), (51, 10, -3), (20, 30, 7), (22, 31, 5)]            # r = 0, r < 0, two that overlap
        p[1, 599] = (60, 35, 3)                                                      # the last row of the third round
    p.setflags(write=False)
    return p


def phm_live(c, b):
    p = phm_params(c.name)[b, :phm_plan(c, b)['n']]
    return p[p[:, 2] >= 0]


PHM_REGIMES = collections.OrderedDict(
    [(('n', n), 'render_pre_hm_kernel: n = min(counts[b], cap); for (c0 = 0; c0 == 0 || c0 < n; c0 += PHM_CAP)') for n in (0, 1, 256, 257, 600)] +
    [('counts>cap', 'render_pre_hm_kernel: n = min(counts[b], cap)'),
     ('r=0', 'render_pre_hm_kernel: sigma = (2 r + 1) / 6 = 1 / 6, one pixel'),
     ('r<0', 'render_pre_hm_kernel: hit = i < c1 && r >= 0 && ...')] +
    [('partly-off:' + s, 'render_pre_hm_kernel: the cull keeps the blob, if (x >= W || y >= H) return') for s in ('left', 'right', 'top', 'bottom')] +
    [('wholly-off:' + s, 'render_pre_hm_kernel: cx + r >= x0 && cx - r < x0 + PHM_TW && cy + r >= y0 && cy - r < y0 + PHM_TH fails for every tile')
     for s in ('left', 'right', 'top', 'bottom')] +
    [('B=3', 'render_pre_hm_kernel: b = bid / tilesY, p = params + b * cap * 3')] +
    [(('geo', h, w), 'render_pre_hm_kernel: tilesX, tilesY; if (x >= W || y >= H) return') for h, w in ((1, 1), (8, 32), (9, 33), (40, 72))] +
    [(('flipped', f), 'render_pre_hm_kernel: if (also_flipped) out[(B + b) ...][W - 1 - x] = v') for f in (0, 1)] +
    [('overlap', 'render_pre_hm_kernel: v = fmaxf(v, (float)g)')])


def phm_keys(c):
    k = {('geo', c.H, c.W), ('flipped', c.flipped)}
    if c.B == 3:
        k.add('B=3')
    for b in range(c.B):
        n = phm_plan(c, b)['n']
        if ('n', n) in PHM_REGIMES:
            k.add(('n', n))
        if c.counts[b] > c.cap:
            k.add('counts>cap')
        rows = phm_params(c.name)[b, :n]
        if (rows[:, 2] == 0).any():
            k.add('r=0')
        if (rows[:, 2] < 0).any():
            k.add('r<0')
        cover = np.zeros((c.H, c.W), int)
        for cx, cy, r in phm_live(c, b):
            x0, x1, y0, y1 = cx - r, cx + r, cy - r, cy + r
            inside = x1 >= 0 and x0 < c.W and y1 >= 0 and y0 < c.H
            for side, partly, wholly in (('left', x0 < 0, x1 < 0), ('right', x1 >= c.W, x0 >= c.W), ('top', y0 < 0, y1 < 0), ('bottom', y1 >= c.H, y0 >= c.H)):
                if wholly:
                    k.add('wholly-off:' + side)
                elif partly and inside:
                    k.add('partly-off:' + side)
            if inside:
                cover[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] += 1
        if (cover > 1).any():
            k.add('overlap')
    return k


def missing_phm_regimes(cases):
    return _missing(PHM_REGIMES, phm_keys, cases)


PHM_MUTATIONS = collections.OrderedDict([('a', 'sum instead of max'), ('b', 'sigma = r / 3'), ('c', 'the flipped copy not mirrored')])


def phm_reference(name, mutation=None):
    """float32 [B or 2B, 1, H, W]: the float64 max-splat of the kernel's formula, every Gaussian value cast to float32"""
    c = PHM_CASE[name]
    out = np.zeros((c.B * (2 if c.flipped else 1), 1, c.H, c.W), np.float32)
    ys, xs = np.mgrid[0:c.H, 0:c.W]
    for b in range(c.B):
        v = np.zeros((c.H, c.W), np.float32)
        for cx, cy, r in phm_live(c, b):
            dx, dy = xs - int(cx), ys - int(cy)
            sigma = (r / 3.0 if mutation == 'b' else (2 * r + 1) / 6.0)
            with np.errstate(divide='ignore', invalid='ignore'):
                g = np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2.0 * sigma * sigma)).astype(np.float32)
            g = np.where((np.abs(dx) <= r) & (np.abs(dy) <= r), np.nan_to_num(g), np.float32(0))
            v = v + g if mutation == 'a' else np.maximum(v, g)
        out[b, 0] = v
        if c.flipped:
            out[c.B + b, 0] = v if mutation == 'c' else v[:, ::-1]
    return out


def ulps(a, b):
    """distance in float32 steps between two non-negative float32 arrays"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def phm_compare(name, got):
    """(largest distance in ulps, pixels not bit-equal, touched pixels) against the reference"""
    ref = phm_reference(name)
    d = ulps(np.ascontiguousarray(got, np.float32), ref)
    return int(d.max()), int((d != 0).sum()), int((ref > 0).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the pose match

PoseCase = collections.namedtuple('PoseCase', 'name B K J offset box sliced designed hps_std why')
POSE_HW = (40, 48)
POSE_CASES = [
    PoseCase('k20_j1', 1, 20, 1, None, 'wh', False, False, 3.0, 'one joint, K < 128 threads, peaks at + 0.5, the gate box from the packed row'),
    PoseCase('k128_designed', 2, 128, 17, None, 'wh', False, True, 3.0, 'K = 128: every thread one detection; the designed joints of POSE_WANT'),
    PoseCase('k129_slices', 2, 129, 17, 'hp_offset', 'wh+reg+amodal', True, False, 3.0,
             'K = 129: one thread takes a second detection; hps, hp_offset, box_wh and box_reg are channel slices of wider tensors'),
    PoseCase('k200_ltrb', 1, 200, 17, 'reg', 'ltrb+amodal', True, False, 3.0, 'K = 200: 72 threads take a second detection; box_ltrb a channel slice'),
    PoseCase('k20_boxless', 2, 20, 17, None, 'none', False, False, 1.0, 'no box head: the extent of the regressed joints, widened from the widened left / top'),
]
POSE_CASE = collections.OrderedDict((c.name, c) for c in POSE_CASES)
# image 0 of k128_designed: detection 0 at (x 10, y 10), wh (12, 12): gate box 4.5 .. 16.5 both ways
POSE_WANT = collections.OrderedDict([        # joint -> (the key point of detection 0, what decides it)
    (0, ((12.0, 10.0), 'thresh: the only peak near scores exactly 0.2f, not strong (s > 0.2): the regressed joint is kept')),
    (1, ((4.5, 10.5), "edge: a strong peak exactly on the box's left edge (hx < bl is false): snapped")),
    (2, ((12.5, 10.5), 'equidistant: two strong peaks at distance 2, the earlier one (the higher score) wins like torch.min')),
    (3, ((13.0, 13.0), 'weak: every peak of the joint is <= 0.2: the regressed joint is kept')),
])

POSE_REGIMES = collections.OrderedDict([
    ('K<128', 'pose_match_kernel: for (k = threadIdx.x; k < a.K; k += blockDim.x), idle threads'),
    ('K=128', 'pose_match_kernel: dim3(128), one pass, no idle thread'),
    ('K=129', 'pose_match_kernel: k += blockDim.x, a second pass of one thread'),
    ('K=200', 'pose_match_kernel: a second pass of 72 threads'),
    (('J', 1), 'ct_decode_pose: dim3(B * num_joints); pose_score_kernel: sum / (float)a.J'),
    (('J', 17), 'ct_decode_pose: dim3(B * num_joints)'),
    ('off:none', 'pose_match_kernel: x = x + 0.5f'),
    ('off:hp_offset', 'pose_match_kernel: x = x + a.off[b * a.off_bs + ind]'),
    ('off:reg', 'Decoder: heads.get("hp_offset", heads.get("reg"))'),
    ('box:row', 'pose_match_kernel: a.box_col >= 0'),
    ('box:wh+reg', 'pose_match_kernel: else if (a.bwh), if (a.breg)'),
    ('box:ltrb', 'pose_match_kernel: else if (a.bltrb)'),
    ('box:none', 'pose_match_kernel: the extent of the regressed joints; br = br + (br - bl) * margin from the widened bl'),
    ('stride:hps', 'ct_decode_pose: a.hps_bs = d->hps_batch_stride'),
    ('stride:hp_offset', 'ct_decode_pose: a.off_bs = d->hp_offset_batch_stride'),
    ('stride:box_wh', 'ct_decode_pose: a.bwh_bs = d->box_wh_batch_stride'),
    ('stride:box_reg', 'ct_decode_pose: a.breg_bs = d->box_reg_batch_stride'),
    ('stride:box_ltrb', 'ct_decode_pose: a.bltrb_bs = d->box_ltrb_batch_stride'),
    ('design:thresh', 'pose_match_kernel: strong = s > POSE_THRESH'),
    ('design:edge', 'pose_match_kernel: hx < bl'),
    ('design:equidistant', 'pose_match_kernel: if (d < best)'),
    ('design:weak', 'pose_match_kernel: keep_reg = hs < POSE_THRESH'),
])


def pose_heads(c):
    """OrderedDict head -> channels of a case"""
    heads = collections.OrderedDict([('hm', 1), ('hps', 2 * c.J), ('hm_hp', c.J)])
    for name in c.box.split('+'):
        if name != 'none':
            heads['ltrb_amodal' if name == 'amodal' else name] = {'wh': 2, 'reg': 2, 'ltrb': 4, 'amodal': 4}[name]
    if c.offset:
        heads['reg'] = 2
        if c.offset == 'hp_offset':
            heads['hp_offset'] = 2
    return heads


def pose_keys(c):
    heads = pose_heads(c)
    k = {('J', c.J), 'off:' + (c.offset or 'none'), 'K<128' if c.K < POSE_BLOCK else 'K=%d' % c.K}
    from_heads = 'ltrb_amodal' in heads or not ({'wh', 'ltrb'} & set(heads))              # Decoder: box_col = -1
    box = 'box:row' if not from_heads else 'box:ltrb' if 'ltrb' in heads else 'box:wh+reg' if 'wh' in heads and 'reg' in heads else 'box:none'
    k.add(box)
    if c.sliced:
        k.add('stride:hps')
        if c.offset == 'hp_offset':
            k.add('stride:hp_offset')
        if box == 'box:wh+reg':
            k |= {'stride:box_wh', 'stride:box_reg'}
        if box == 'box:ltrb':
            k.add('stride:box_ltrb')
    if c.designed:
        k |= {'design:thresh', 'design:edge', 'design:equidistant', 'design:weak'}
    return k


def missing_pose_regimes(cases):
    return _missing(POSE_REGIMES, pose_keys, cases)


def _peaks(rng, c, lo, hi):
    """[c, h, w]: distinct peaks in (lo, hi) on every other pixel both ways over a distinct background below 0.04: the 3x3 NMS keeps
    exactly the 20 x 24 = 480 peaks"""
    h, w = POSE_HW
    n = c * h * w
    m = ((rng.permutation(n).astype(np.float64) + 1) / (n + 1) * 0.04).reshape(c, h, w)
    npk = c * (h // 2) * (w // 2)
    m[:, 0::2, 0::2] = (lo + (hi - lo) * (rng.permutation(npk).astype(np.float64) + 1) / (npk + 1)).reshape(c, h // 2, w // 2)
    return m.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pose_maps(name):
    c = POSE_CASE[name]
    h, w = POSE_HW
    rng = np.random.default_rng(5000 + sum(map(ord, name)))
    m = collections.OrderedDict()
    for head, ch in pose_heads(c).items():
        shape = (c.B, ch, h, w)
        if head == 'hm':
            v = np.stack([_peaks(rng, 1, 0.3, 0.9) for _ in range(c.B)])
        elif head == 'hm_hp':
            v = np.stack([_peaks(rng, c.J, 0.05, 0.95) for _ in range(c.B)])
        elif head in ('reg', 'hp_offset'):
            v = rng.random(shape)
        elif head == 'wh':
            v = rng.standard_normal(shape) * 4 + 11
        elif head == 'ltrb':
            v = np.abs(rng.standard_normal(shape) * 2) * np.array([-3.0, -3.0, 3.0, 3.0]).reshape(1, 4, 1, 1)
        elif head == 'hps':
            v = rng.standard_normal(shape) * c.hps_std
        else:
            v = rng.standard_normal(shape) * 2
        m[head] = np.ascontiguousarray(v, np.float32)
    if c.designed:
        hm, wh, hps, hm_hp = m['hm'], m['wh'], m['hps'], m['hm_hp']
        hm[0, 0, 10, 10] = 0.99                                                      # detection 0 of image 0
        wh[0, :, 10, 10] = (12.0, 12.0)
        weak = lambda: (rng.permutation(h * w).astype(np.float64).reshape(h, w) / (h * w) * 0.15).astype(np.float32)
        hm_hp[0, 0] = weak()
        hm_hp[0, 0, 10, 12] = POSE_THRESH
        hps[0, 0:2, 10, 10] = (2.0, 0.0)
        hm_hp[0, 1] = weak()
        hm_hp[0, 1, 10, 4] = 0.8
        hps[0, 2:4, 10, 10] = (-5.0, 1.0)
        hm_hp[0, 2] = weak()
        hm_hp[0, 2, 10, 12], hm_hp[0, 2, 10, 8] = 0.7, 0.6
        hps[0, 4:6, 10, 10] = (0.5, 0.5)
        hm_hp[:, 3] *= np.float32(0.15)
        hps[0, 6:8, 10, 10] = (3.0, 3.0)
    for v in m.values():
        v.setflags(write=False)
    return m


POSE_MUTATIONS = collections.OrderedDict([
    ('a', 'the last minimum instead of the first'),
    ('b', '>= instead of > at POSE_THRESH'),
    ('c', 'br (bb) widened from the un-widened bl (bt)'),
])


def pose_refine(kps, output, K, bboxes, scores, mutation=None):
    """oracle.decode.refine_keypoints restated with the three switches of POSE_MUTATIONS (None: the same fp32 operations)"""
    from oracle import decode as od
    batch, J = kps.shape[0], kps.shape[2] // 2
    p_score, p_inds, p_ys, p_xs = od.topk_channel(od.nms(output['hm_hp']), K=K)
    off = output.get('hp_offset', output.get('reg'))
    if off is not None:
        o = od.transpose_and_gather_feat(off, p_inds.view(batch, -1)).view(batch, J, K, 2)
        p_xs, p_ys = p_xs + o[..., 0], p_ys + o[..., 1]
    else:
        p_xs, p_ys = p_xs + 0.5, p_ys + 0.5
    strong = p_score >= float(POSE_THRESH) if mutation == 'b' else p_score > float(POSE_THRESH)
    p_score = torch.where(strong, p_score, torch.full_like(p_score, -1.0))
    p_xs = torch.where(strong, p_xs, torch.full_like(p_xs, -10000.0))
    p_ys = torch.where(strong, p_ys, torch.full_like(p_ys, -10000.0))
    new_kps, joint_score = kps.clone(), torch.empty((batch, J, K), dtype=kps.dtype)
    for b in range(batch):
        if bboxes is not None:
            l, t, r, bt = bboxes[b, :, 0], bboxes[b, :, 1], bboxes[b, :, 2], bboxes[b, :, 3]
        else:
            xs_, ys_ = kps[b, :, 0::2], kps[b, :, 1::2]
            l0, r, t0, bt = xs_.min(dim=1)[0], xs_.max(dim=1)[0], ys_.min(dim=1)[0], ys_.max(dim=1)[0]
            l, t = l0 - (r - l0) * 0.25, t0 - (bt - t0) * 0.25
            r = r + (r - (l0 if mutation == 'c' else l)) * 0.25
            bt = bt + (bt - (t0 if mutation == 'c' else t)) * 0.25
        for j in range(J):
            rx, ry = kps[b, :, 2 * j], kps[b, :, 2 * j + 1]
            dist = ((rx[:, None] - p_xs[b, j][None, :]) ** 2 + (ry[:, None] - p_ys[b, j][None, :]) ** 2) ** 0.5
            at_min = (dist == dist.min(dim=1, keepdim=True)[0]).float()
            first, last = at_min.argmax(dim=1), K - 1 - at_min.flip(1).argmax(dim=1)
            assert bool((first == dist.argmin(dim=1)).all())                         # (torch.min takes the first minimum)
            near = last if mutation == 'a' else first
            hs, hx, hy = p_score[b, j][near], p_xs[b, j][near], p_ys[b, j][near]
            keep = (hs < float(POSE_THRESH)) | (hx < l) | (hx > r) | (hy < t) | (hy > bt)
            new_kps[b, :, 2 * j] = torch.where(keep, rx, hx)
            new_kps[b, :, 2 * j + 1] = torch.where(keep, ry, hy)
            joint_score[b, j] = torch.where(keep, scores[b], hs)
    return new_kps, scores * joint_score.mean(dim=1)


def pose_reference(name, mutation=None):
    """oracle.decode.generic_decode on the case's maps -> dict of numpy arrays; with a mutation, its refine_keypoints replaced by
    ``pose_refine`` (with None as well when ``mutation`` is 'restated': the CPU test compares that with the oracle's own)"""
    from oracle import decode as od
    c = POSE_CASE[name]
    maps = {k: torch.from_numpy(np.array(v)) for k, v in pose_maps(name).items()}
    real = od.refine_keypoints
    if mutation is not None:
        od.refine_keypoints = lambda kps, output, K, bboxes, scores: pose_refine(kps, output, K, bboxes, scores, None if mutation == 'restated' else mutation)
    try:
        want = od.generic_decode(maps, K=c.K, return_inds=True)
    finally:
        od.refine_keypoints = real
    return {k: v.numpy() for k, v in want.items()}


@functools.lru_cache(maxsize=None)
def pose_want(name):
    return pose_reference(name)


# ---------------------------------------------------------------------------------------------------------------------
# the mutations, by family

MUTATIONS = dict(stem=STEM_MUTATIONS, heads=HEADS_MUTATIONS, flip=FLIP_MUTATIONS, pre_hm=PHM_MUTATIONS, pose=POSE_MUTATIONS)
MUTATION_CASE = {
    ('stem', 'a'): 'geo_7x31', ('stem', 'b'): 'm7', ('stem', 'c'): 'm4', ('stem', 'd'): 'm4_add',
    ('heads', 'a'): 'one', ('heads', 'b'): 'eight', ('heads', 'c'): 'eight', ('heads', 'd'): 'slice',
    ('flip', 'a'): 'src_plus4', ('flip', 'b'): 'w13', ('flip', 'c'): 'eight',
    ('pre_hm', 'a'): 'p_40x72', ('pre_hm', 'b'): 'p_8x32', ('pre_hm', 'c'): 'p_8x32',
    ('pose', 'a'): 'k128_designed', ('pose', 'b'): 'k128_designed', ('pose', 'c'): 'k20_boxless',
}


def mutated(family, letter):
    """the wrong reference ``letter`` of ``family`` on the case MUTATION_CASE names for it, in the form of the family's reference"""
    name = MUTATION_CASE[(family, letter)]
    if family == 'stem':
        c = STEM_CASE[name]
        return stem_compose(stem_inputs(c.N, c.H, c.W), c.mask, c.add, torch.float64, letter)
    if family == 'heads':
        return heads_compose(name, torch.float64, mutation=letter)
    if family == 'flip':
        return flip_reference(name, letter)
    if family == 'pre_hm':
        return phm_reference(name, letter)
    return pose_reference(name, letter)
