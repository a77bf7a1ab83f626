"""The near-limit cases (tests/test_limits_cpu.py, tests/test_hip_limits.py): for every entry point whose host check bounds a
view or a pixel count, a launch of a few hundred pixels at the largest pitch the check accepts -- so that the last pixel's byte
offset lies within one pitch of the limit -- or, where the limit is on the pixel index, the smallest map that reaches it.  No GPU,
no ctypes.  In order: ``ct_conv2d`` and ``ct_dcn_v2`` / ``ct_dcn_v2_group`` (LIMITS, DCN_GROUP), the many-pixel cases with their exact
inputs and band references (MANY_PIXELS), then the training entry points, whose limit bounds the whole batch (DCN_BWD_*, BN_*,
TRAIN_*, STEM_*).

A pitch is derived from the check's own formula (``widest_pitch``), never written down; ``offsets_formed`` lists, per case, the
largest values the kernels form from it (read from the sources named there) beside what the type that holds them can hold."""
from collections import OrderedDict, namedtuple

import _conv_fwd as C
import _dcn_fwd as D

GIB2 = 2 ** 31                                  # ct_common.h: VIEW_LIMIT
INT_MAX = 2 ** 31 - 1
DCN_LDX_LIMIT, DCN_LDY_LIMIT, DCN_PIXELS = 2 ** 21, 2 ** 23, 2 ** 23       # dcn_mfma.hip make_plan: ldx < 2^21, ldy < 2^23, H*W <= 2^23
PITCH_STEP = 4                                  # every entry point wants 16-byte aligned pixels


def extent_bytes(px, ld, Cc):
    """bytes from the first channel of the first pixel to the end of the last: what the 2 GiB checks bound"""
    return ((px - 1) * ld + Cc) * 4


def widest_pitch(px, Cc, limit=GIB2):
    """the largest pitch (a multiple of 4) at which ``px`` pixels of ``Cc`` channels stay below ``limit`` bytes: the check's own
    formula, ((px - 1) * ld + Cc) * 4 < limit, one step below the first pitch it refuses"""
    ld = ((limit // 4 - 1 - Cc) // (px - 1)) // PITCH_STEP * PITCH_STEP
    assert extent_bytes(px, ld, Cc) < limit <= extent_bytes(px, ld + PITCH_STEP, Cc) and ld >= Cc
    return ld


# kind: 'conv' (case: _conv_fwd.Case) or 'dcn' (case: _dcn_fwd.Case); wide: the views that lie at the widest pitch (every other view
# at the pitch the ordinary tests use)
Limit = namedtuple('Limit', 'name entry kind case wide why')


def _conv_limits():
    L = []

    def add(name, wide, why, **kw):
        L.append(Limit(name, 'ct_conv2d', 'conv', C.mk('limit_' + name, why=why, **kw), tuple(wide), why))
    add('conv_row_k1', ('x', 'y'), 'row kernel, 1x1, N = 2: image 1 starts above 2 GiB, the batch view lies between 2 and 4 GiB',
        N=2, H=12, W=20, Cin=64, Cout=59, ks=1, stride=1, algo=5, relu=True)
    add('conv_row_k3', ('x', 'y', 'res'), 'row kernel, 3x3, with a residual at the wide pitch',
        N=1, H=12, W=20, Cin=64, Cout=59, ks=3, stride=1, algo=3, res=True, relu=True)
    add('conv_ksplit', ('x', 'y'), 'K-split kernel (algo 102), 3x3',
        N=1, H=12, W=20, Cin=64, Cout=59, ks=3, stride=1, algo=102)
    add('conv_wino', ('x', 'y', 'res'), 'Winograd (algo 202) with residual and ReLU',
        N=1, H=12, W=20, Cin=64, Cout=59, ks=3, stride=1, algo=202, res=True, relu=True)
    add('conv_s2_sides', ('y', 'pool', 'proj'), '3x3 stride 2 with the pool and projection side outputs, all three outputs wide',
        N=1, H=24, W=40, Cin=64, Cout=59, ks=3, stride=2, algo=5, pool=True, proj=True)
    add('conv_s2_x', ('x',), '3x3 stride 2 with both side outputs, the input wide (960 pixels)',
        N=1, H=24, W=40, Cin=64, Cout=59, ks=3, stride=2, algo=5, pool=True, proj=True)
    add('conv_ksplit_s2_sides', ('y', 'pool', 'proj'), 'K-split kernel (algo 102), 3x3 stride 2 with both side outputs',
        N=1, H=24, W=40, Cin=64, Cout=59, ks=3, stride=2, algo=102, pool=True, proj=True)
    add('conv_nchw', ('x',), 'NCHW output (no pitch of its own): the input wide',
        N=1, H=12, W=20, Cin=64, Cout=59, ks=1, stride=1, algo=5, nchw=True)
    return L


def conv_view_dims(case):
    """name -> (pixels per image, channels) of every NHWC view the case's launch takes"""
    p = C.plan_of(case)
    out = p['Ho'] * p['Wo']
    v = OrderedDict(x=(case.H * case.W, case.Cin))
    if not case.nchw:
        v['y'] = (out, case.Cout)
    if case.res:
        v['res'] = (out, case.Cout)
    if case.pool:
        v['pool'] = ((case.H // 2) * (case.W // 2), case.Cin)
    if case.proj:
        v['proj'] = (out, case.Cout)
    return v


CONV_FIELD = dict(x='ldx', y='ldy', res='ldr', pool='pool_ld', proj='proj_ldy')          # the descriptor's pitch field of a view
CONV_WORD = dict(x='x', y='y', res='res', pool='pool_y', proj='proj_y')                  # ... and its name in the refusal


def _dcn_limits():
    L = []

    def add(name, wide, why, entry='ct_dcn_v2', **kw):
        L.append(Limit(name, entry, 'dcn', D.mk('limit_' + name, why=why, **kw), tuple(wide), why))
    add('dcn_map_ldx', ('x',), 'given map, direct store: ldx = 2^21 - 4 at 16 x 16 pixels (the 24-bit multiply of dcn_tab_entry)',
        N=2, H=16, W=16, Cin=32, Cout=20, algo=3264, split_k=1, src='map')
    add('dcn_map_ldy', ('y',), 'given map, direct store: ldy = 2^23 - 4 at 8 x 8 pixels (the 24-bit multiply of dcn_store_acc)',
        N=2, H=8, W=8, Cin=32, Cout=20, algo=3264, split_k=1, src='map')
    add('dcn_map_ldy64', ('y',), 'the same on the 64-pixel tile (algo 64)',
        N=1, H=8, W=8, Cin=32, Cout=20, algo=64, split_k=1, src='map')
    add('dcn_split_ldy', ('y',), 'split layer: a small partial map, y at the wide pitch through the finishing launch (64-bit offsets)',
        N=2, H=12, W=20, Cin=128, Cout=20, algo=3264, split_k=2, src='map')
    for src in ('fused', 'parts', 'wino'):
        add('dcn_%s_ldx' % src, ('x',), 'own offset conv (%s) reading x at ldx = 2^21 - 4' % src,
            N=1, H=16, W=16, Cin=128 if src != 'fused' else 64, Cout=20, algo=3264, split_k=1, src=src)
    add('dcn_persist', ('x', 'om'), 'persistent form: x of the N = 2 batch just below 4 GiB, the offset/mask map of the batch just below 2 GiB',
        N=2, H=16, W=17, Cin=128, Cout=20, algo=53264, split_k=1, src='map')
    add('dcn_up_wide', ('up', 'skip'), 'fused IDAUp finish: up_y and skip at the wide pitch',
        N=1, H=6, W=10, Cin=128, Cout=20, algo=3264, split_k=2, src='map', up_f=2)
    return L


def dcn_view_dims(case):
    """name -> (pixels per image, channels); ``om``: the pixels of the whole batch, which the persistent form puts behind one descriptor"""
    v = OrderedDict(x=(case.H * case.W, case.Cin), y=(case.H * case.W, case.Cout), om=(case.N * case.H * case.W, 27))
    if case.up_f:
        f2 = case.up_f ** 2
        v['up'] = v['skip'] = (case.H * case.W * f2, case.Cout)
    return v


def dcn_limit_of(case, view):
    """(the largest pitch the host check accepts, the words of the refusal one step up) of a DCN view: the smallest of the 2 GiB
    extent per image, the 24-bit limit of the kernel that addresses it and, in the persistent form, the 4 GiB of x and the 2 GiB of
    the offset/mask map of the whole batch.  A split layer's y and the IDAUp views go through the finishing launch, which forms 64-bit
    element offsets: no host check bounds their extent below 2^32 elements (out of reach here), so they lie at the 2 GiB pitch and
    nothing is refused one step up -- the arena alone guards them."""
    px, Cc = dcn_view_dims(case)[view]
    ld = widest_pitch(px, Cc)
    p = D.plan_of(case)
    if view == 'x':
        best = (ld, '2 GiB')
        if DCN_LDX_LIMIT - PITCH_STEP < best[0]:
            best = (DCN_LDX_LIMIT - PITCH_STEP, 'ldx < 2^21')
        if p['family'] == 'persist':
            batch = ((2 ** 30 - 1) // (case.N * px)) // PITCH_STEP * PITCH_STEP          # N * H * W * ldx * 4 < 2^32
            if batch < best[0]:
                best = (batch, 'input view of 4 GiB')
        return best
    if view == 'y' and not p['use_ws']:
        if ld >= DCN_LDY_LIMIT:
            return DCN_LDY_LIMIT - PITCH_STEP, 'ldy < 2^23'
        return ld, '2 GiB'
    if view == 'om':
        return ld, ('offset/mask map of 2 GiB' if p['family'] == 'persist' else None)
    return ld, None


# ct_dcn_v2_group: two layers of one tile shape; the wide pitches (x and y) on the second only
DCN_GROUP = [D.mk('limit_dcn_group_0', 2, 6, 10, 64, 20, 3264, split_k=1, src='map', entry='group', why='the ordinary layer of the group'),
             D.mk('limit_dcn_group_1', 1, 16, 16, 64, 20, 3264, split_k=1, src='map', entry='group', why='x at 2^21 - 4 and y at the 2 GiB pitch inside a group')]
LIMITS = _conv_limits() + _dcn_limits()
LIMIT = OrderedDict((l.name, l) for l in LIMITS)
assert len(LIMIT) == len(LIMITS)


def pitches(lim):
    """view -> pitch of the wide views of a case"""
    out = OrderedDict()
    for v in lim.wide:
        if lim.kind == 'conv':
            out[v] = widest_pitch(*conv_view_dims(lim.case)[v])
        else:
            out[v] = dcn_limit_of(lim.case, v)[0]
    return out


def view_dims(lim):
    return conv_view_dims(lim.case) if lim.kind == 'conv' else dcn_view_dims(lim.case)


def offsets_formed(lim):
    """[(what, largest value formed, what its type holds, where)] for the wide views of a case, by reading the sources"""
    rows, case = [], lim.case
    dims = view_dims(lim)
    for v, ld in pitches(lim).items():
        px, Cc = dims[v]
        ext = extent_bytes(px, ld, Cc)
        rows.append(('%s: descriptor size cast to int' % v, ext, INT_MAX, 'make_buffer_rsrc(.., (int)(((img - 1u) * ld + C) * 4u), ..)'))
        rows.append(('%s: int byte offset of the last element' % v, ext - 4, INT_MAX, '(lpix * ld + co) * 4 / (iy * W + ix) * ldx * 4'))
        rows.append(('%s: base of the last image in bytes (64-bit)' % v, (case.N - 1) * px * ld * 4, 2 ** 63 - 1, '(size_t)n * img * ld'))
        if lim.kind == 'dcn' and v == 'x':
            rows.append(('x: __mul24 operand ldx * 4', ld * 4, 2 ** 23 - 1, 'dcn_mfma.hip dcn_tab_entry: __mul24(__mul24(y0, W) + x0, ldx4)'))
            rows.append(('x: __mul24 operand pixel index', px - 1, 2 ** 23 - 1, 'dcn_mfma.hip dcn_tab_entry'))
            rows.append(('x: __mul24 product (low 32 bits, int)', (px - 1) * ld * 4, INT_MAX, 'dcn_mfma.hip dcn_tab_entry'))
        if lim.kind == 'dcn' and v == 'y' and not D.plan_of(case)['use_ws']:
            top = (D.cdiv(case.H, 2) * 2 + 1) * case.W          # (rows of a ragged last tile are formed and skipped, never stored)
            rows.append(('y: __mul24 operand ldy', ld, 2 ** 23 - 1, 'dcn_mfma.hip dcn_store_acc: __mul24(__mul24(oyb, W) + px0, ldy)'))
            rows.append(('y: __mul24 operand pixel index', top, 2 ** 23 - 1, 'dcn_mfma.hip dcn_store_acc'))
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the many-pixel cases: the limit is on the pixel index, a float64 CPU reference of 8 to 16 million pixels is too slow.  The inputs
# are chosen so that fp32 is exact in ANY order (small integers, offsets and masks that are multiples of 1/4: every product and
# every partial sum is a multiple of 1/64 far below 2^24 / 64), and the whole map is compared bit for bit with plain torch ops in
# float64 on the device, in row bands.  tests/test_limits_cpu.py holds these references against F.conv2d / oracle.dcn_v2 in
# float64 at a small shape on the same kind of inputs.

Pixels = namedtuple('Pixels', 'name entry N H W Cin Cout ldx ldy algo split_k why')
MANY_PIXELS = OrderedDict((p.name, p) for p in (
    Pixels('conv_pixels', 'ct_conv2d', 1, 4096, 4096, 16, 16, 32, 32, 1, 1,
           '1x1 row kernel at 2^24 pixels, pitch 32: extent 2^31 - 64 bytes (BELOW[1] of tests/test_conv_forward_cpu.py)'),
    Pixels('dcn_pixels', 'ct_dcn_v2', 1, 2048, 4096, 32, 16, 32, 32, 3264, 1,
           'H*W = 2^23, the largest pixel index the 24-bit multiplies of dcn_tab_entry / dcn_store_acc take'),
    Pixels('dcn_partials', 'ct_dcn_v2', 1, 2048, 2048, 64, 112, 64, 112, 3264, 2,
           'a split layer whose partial map is the largest the finishing launch takes: 2^22 pixels x 112 couts = 7/8 of 2^29 floats per '
           'split (128 couts, the next width of the map, are refused); dropped lanes carry the byte offset 0x80000000')))
BAND = 128                                    # rows per band of the device reference


def exact_inputs(p, device, seed=7, H=None, W=None):
    """tensors of a many-pixel case on ``device`` (NHWC x; OIHW w): integers in [-4, 4] / [-2, 2], scales that are powers of two,
    integer shifts; for the DCN an [H, W, 27] map of offsets in [-2, 2] and masks in [0, 1], all multiples of 1/4"""
    import torch
    H, W = H or p.H, W or p.W
    g = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).float()
    ks = 1 if p.entry == 'ct_conv2d' else 3
    d = dict(x=ri(-4, 4, p.N, H, W, p.Cin), w=ri(-2, 2, p.Cout, p.Cin, ks, ks), scale=2.0 ** ri(-1, 1, p.Cout), shift=ri(-3, 3, p.Cout))
    if p.entry == 'ct_dcn_v2':
        d['om'] = torch.cat([ri(-8, 8, p.N, H, W, 18), ri(0, 4, p.N, H, W, 9)], 3) * 0.25
    return d


def exact_conv_band(d, n, r0, r1):
    """relu((1x1 conv) * scale + shift) of rows [r0, r1) of image n in float64 -> [r1 - r0, W, Cout]"""
    import torch
    dt = torch.float64
    z = d['x'][n, r0:r1].to(dt) @ d['w'][:, :, 0, 0].to(dt).t()
    return torch.relu(z * d['scale'].to(dt) + d['shift'].to(dt))


def exact_dcn_band(d, n, r0, r1):
    """relu(DCNv2 * scale + shift) of rows [r0, r1) of image n in float64 -> [r1 - r0, W, Cout]; the sampling rules of
    oracle/dcn_v2.py: a sample at or beyond -1 or H / W contributes nothing, a corner outside the map contributes nothing"""
    import torch
    dt = torch.float64
    x, om, w = d['x'][n], d['om'][n, r0:r1].to(dt), d['w'].to(dt)
    H, W, Cin = x.shape
    xf = x.reshape(H * W, Cin)
    ho = torch.arange(r0, r1, device=x.device, dtype=dt).view(-1, 1)
    wo = torch.arange(W, device=x.device, dtype=dt).view(1, -1)
    out = torch.zeros(((r1 - r0) * W, w.shape[0]), dtype=dt, device=x.device)
    for k in range(9):
        ys, xs = ho - 1 + k // 3 + om[..., 2 * k], wo - 1 + k % 3 + om[..., 2 * k + 1]
        inside = (ys > -1) & (xs > -1) & (ys < H) & (xs < W)
        y0, x0 = torch.floor(ys), torch.floor(xs)
        ly, lx = ys - y0, xs - x0
        val = torch.zeros(((r1 - r0) * W, Cin), dtype=dt, device=x.device)
        for yy, xx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1) & inside
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(-1)
            val += xf[idx].to(dt) * (wgt * ok.to(dt)).view(-1, 1)
        out += (val * om[..., 18 + k].reshape(-1, 1)) @ w[:, :, k // 3, k % 3].t()
    return torch.relu(out * d['scale'].to(dt) + d['shift'].to(dt)).view(r1 - r0, W, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the training entry points: VIEW_LIMIT bounds N*H*W * pitch * 4 bytes of the WHOLE batch

def widest_batch_pitch(px):
    """the largest pitch (a multiple of 4) at which a view of ``px`` pixels stays below 2 GiB by the training files' formula,
    px * ld * 4 < VIEW_LIMIT"""
    ld = ((GIB2 // 4 - 1) // px) // PITCH_STEP * PITCH_STEP
    assert px * ld * 4 < GIB2 <= px * (ld + PITCH_STEP) * 4
    return ld


# ct_dcn_v2_backward: (B, Cin, Cout, H, W, offset scale) of tests/test_hip_dcn_backward.py's SHAPES -- Cout off the 16-wide tile,
# 2 x 12 x 20 pixels: pitch 1 118 480, 2^31 - 2048 bytes -- with the wide pitch on one view at a time
DCN_BWD_SHAPE = (2, 64, 24, 12, 20, 2.0)
DCN_BWD_VIEWS = OrderedDict([('x', 'ldx'), ('om', 'ldom'), ('gy', 'ldgy'), ('gx', 'ldgx'), ('gom', 'ldgom')])      # view -> pitch field

# ct_bn_stats, ct_bn_act_apply, ct_bn_act_backward: (N, H, W, C) with ReLU, residual and batch statistics; make_bn_plan takes the
# largest pitch of z, y, gy, gz, res, gres, so each of them lies at the wide pitch in turn.  view -> (pitch field, the entry points
# that take the view)
BN_SHAPE = (2, 12, 20, 24)
BN_VIEWS = OrderedDict([('z', ('ldz', ('ct_bn_stats', 'ct_bn_act_apply', 'ct_bn_act_backward'))), ('y', ('ldy', ('ct_bn_act_apply',))),
                        ('res', ('ldr', ('ct_bn_act_apply', 'ct_bn_act_backward'))), ('gy', ('ldgy', ('ct_bn_act_backward',))),
                        ('gz', ('ldgz', ('ct_bn_act_backward',))), ('gres', ('ldgres', ('ct_bn_act_backward',)))])

# the other training entry points whose views VIEW_LIMIT bounds over the whole batch: op -> (entry point, {view: pixels (or
# slots) of the batch}); each view lies at ITS widest pitch in turn.  Shapes: tests/test_hip_limits.py (TRAIN_SHAPES there)
TRAIN_SHAPES = dict(pool_bwd=(2, 12, 20, 16), s2_bwd=(2, 12, 20, 32, 16), up_bwd=(2, 6, 10, 16, 2), mask_sigmoid=(2, 12, 20),
                    slots=(3, 8, 8, 17), cw_bwd=(2, 12, 20, 32, 24, 3))              # s2: (N, H, W, Cin, Cout); up: (N, H, W, C, f) of the input grid; slots: (N, H, W, M); cw: (N, H, W, Cin, Cout, ks)
TRAIN_OPS = OrderedDict([
    ('pool_bwd', ('ct_maxpool2x2_backward', OrderedDict([('x', 480), ('gy', 120), ('gx', 480), ('add', 480)]))),
    ('s2_bwd', ('ct_conv2d_s2_backward', OrderedDict([('x', 480), ('gy', 120), ('gx', 480)]))),
    ('up_bwd', ('ct_upsample_add_backward', OrderedDict([('gy', 480), ('gx', 120), ('x', 120)]))),
    ('cw_bwd', ('ct_conv2d_backward_weight', OrderedDict([('x', 480), ('gy', 480)]))),       # (stride 2: the gw of ct_conv2d_s2_backward above)
    ('mask_sigmoid', ('ct_dcn_mask_sigmoid_backward', OrderedDict([('g', 480), ('om', 480)]))),
    ('slot_gather', ('ct_slot_gather', OrderedDict([('map', 192), ('rows', 51)]))),
    ('slot_fold', ('ct_slot_fold', OrderedDict([('map', 192), ('rows', 51)]))),
])
TRAIN_CASES = [(op, v) for op, (_, views) in TRAIN_OPS.items() for v in views]

# ct_stem_conv_forward, ct_stem_bn_relu_sum, ct_stem_conv_backward: a shape of tests/_stem_bwd.py (N, H, W), all three stems, batch
# statistics.  wide view -> the entry points that take it: z1 is written by the forward and read by the sum, y is the sum's
# output, gz2 is read by the backward (its image and weight gradients)
STEM_SHAPE = (2, 20, 36)
STEM_VIEWS = OrderedDict([('z1', ('ct_stem_conv_forward', 'ct_stem_bn_relu_sum')), ('y', ('ct_stem_bn_relu_sum',)), ('gz2', ('ct_stem_conv_backward',))])
