"""CPU: the table of near-limit cases (tests/_limits.py) against the host checks.  Each validator's limit is read from its source
line; every case of the table is accepted and its next pitch step refused, as the refusal tests of the entry points do it: a fake
pointer, refused before any launch, and the accepted calls only in a child process that sees no device.  Every CT_FAIL_ARG line
that states a view or pixel limit is accounted for; the largest offsets each case makes the kernels form fit the types that hold
them; the exact references of the many-pixel cases equal float64 on their kind of inputs.  Nothing here launches a kernel on a GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _limits as L
import test_conv_forward_cpu as TC
import test_dcn_forward_cpu as TD

ROOT = TC.ROOT
CSRC = os.path.join(ROOT, 'centertrack_amd', 'csrc')


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ---------------------------------------------------------------------------------------------------------------------
# the limits, from the sources

def test_the_tables_limits_are_the_sources():
    common = _src('ct_common.h')
    assert float(re.search(r'VIEW_LIMIT = ([0-9.]+);', common).group(1)) == L.GIB2
    assert '(((double)H * W - 1.0) * ld + C) * 4.0 >= VIEW_LIMIT' in common                  # extent_bytes / widest_pitch
    dcn = _src('dcn_mfma.hip')
    m = re.search(r'\(double\)d->H \* d->W > ([0-9.]+) \|\| d->ldx >= \(1 << (\d+)\)', dcn)
    assert float(m.group(1)) == L.DCN_PIXELS and 1 << int(m.group(2)) == L.DCN_LDX_LIMIT
    assert 1 << int(re.search(r'd->ldy >= \(1 << (\d+)\)', dcn).group(1)) == L.DCN_LDY_LIMIT
    assert '(double)d->N * d->H * d->W * d->ldx * 4.0 >= 4294967296.0' in dcn                # dcn_limit_of: the persistent x
    assert '((px - 1.0) * d->ldom + 27.0) * 4.0 >= VIEW_LIMIT' in dcn                        # ... and its offset/mask map
    assert 'px * (maxld > maxldo ? maxld : maxldo) * 4.0 >= VIEW_LIMIT' in _src('dcn_bwd.hip')   # widest_batch_pitch


# CT_FAIL_ARG lines that state a view or pixel limit (the words GiB, 2^21, 2^23, 2^29) -> the cases of the table that sit under
# them, or why there is none ('element count': no pitch reaches the limit cheaply).  ct_heads_tail_backward states no view limit: its kernels index mid and gmid with size_t throughout
# (heads_bwd.hip), the host bounds N*H*W alone.
COVERED = {
    ('ct_common.h', 'a view of 2 GiB or more per image'): [l.name for l in L.LIMITS if l.kind == 'conv'] + ['conv_pixels', 'dcn_group'],
    ('dcn_mfma.hip', 'the kernels multiply pixel index and pitch in 24 bits (H*W <= 2^23, ldx < 2^21)'):
        ['dcn_map_ldx', 'dcn_fused_ldx', 'dcn_parts_ldx', 'dcn_wino_ldx', 'dcn_group', 'dcn_pixels'],
    ('dcn_mfma.hip', 'the kernels multiply pixel index and pitch in 24 bits (ldy < 2^23)'): ['dcn_map_ldy', 'dcn_map_ldy64'],
    ('dcn_mfma.hip', 'a partial map of 2 GiB or more'): ['dcn_partials'],
    ('dcn_mfma.hip', 'persistent shape: input view of 4 GiB or more'): ['dcn_persist'],
    ('dcn_mfma.hip', 'persistent shape: offset/mask map of 2 GiB or more'): ['dcn_persist'],
    ('dcn_bwd.hip', 'a view of 2 GiB or more'): ['dcn_bwd_' + v for v in L.DCN_BWD_VIEWS],
    ('bn_train.hip', 'a view of 2 GiB or more'): ['bn_' + v for v in L.BN_VIEWS],
    ('backbone_bwd.hip', 'a view of 2 GiB or more'): ['%s_%s' % c for c in L.TRAIN_CASES if c[0] in ('s2_bwd', 'pool_bwd')],
    ('heads_bwd.hip', 'a view of 2 GiB or more'): ['%s_%s' % c for c in L.TRAIN_CASES if c[0] == 'cw_bwd'],
    ('neck_bwd.hip', 'a view of 2 GiB or more'): ['%s_%s' % c for c in L.TRAIN_CASES if c[0] in ('up_bwd', 'mask_sigmoid')],
    ('heads_slots.hip', 'a view of 2 GiB or more'): ['%s_%s' % c for c in L.TRAIN_CASES if c[0] in ('slot_gather', 'slot_fold')],
    ('stem_train.hip', 'a view of 2 GiB or more'): ['stem_' + v for v in L.STEM_VIEWS],
}
# cases whose wide views no host check bounds below 2^32 elements (the finishing launch forms 64-bit offsets): the arena alone guards them
UNBOUNDED = ['dcn_split_ldy', 'dcn_up_wide']
OUT_OF_SCOPE = {
    ('dcn_mfma.hip', 'a packed weight of 2 GiB or more'): 'element count',
    ('inputs.hip', 'a multiple of 4 below 2 GiB'): 'element count',
}

def case_names():
    return (set(L.LIMIT) | set(L.MANY_PIXELS) | {'dcn_group'} | {'dcn_bwd_' + v for v in L.DCN_BWD_VIEWS} | {'bn_' + v for v in L.BN_VIEWS}
            | {'%s_%s' % c for c in L.TRAIN_CASES} | {'stem_' + v for v in L.STEM_VIEWS})


def _limit_lines():
    """[(file, message)] of every CT_FAIL_ARG whose message speaks of GiB, 2^21, 2^23 or 2^29"""
    out = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(('.hip', '.h', '.cpp')):
            continue
        for m in re.finditer(r'CT_FAIL_ARG\(\s*"((?:[^"\\]|\\.)*)"', _src(name)):
            if re.search(r'GiB|2\^21|2\^23|2\^29', m.group(1)):
                out.append((name, m.group(1)))
    return out


def test_every_limit_stating_line_is_accounted_for():
    lines = _limit_lines()
    assert len(lines) >= 15
    known = dict(COVERED)
    known.update(OUT_OF_SCOPE)
    names = case_names()
    used = set()
    for fname, msg in lines:
        keys = [k for k in known if k[0] == fname and k[1] in msg]
        assert len(keys) == 1, 'a limit-stating refusal with no entry here: %s: %s' % (fname, msg)
        used.add(keys[0])
    assert used == set(known), sorted(set(known) - used)
    for key, cases in COVERED.items():
        assert cases and set(cases) <= names, (key, sorted(set(cases) - names))
    assert set(c for cases in COVERED.values() for c in cases) | set(UNBOUNDED) == names       # ... and every case is accounted for
    for name in UNBOUNDED:
        assert all(L.dcn_limit_of(L.LIMIT[name].case, v)[1] is None for v in L.LIMIT[name].wide), name


# ---------------------------------------------------------------------------------------------------------------------
# accepted, and refused one step up

def conv_desc(p, lim, bump=None):
    case = lim.case
    d = TC._desc(p, case.N, case.H, case.W, case.Cin, case.Cout, case.ks, case.stride, algo=case.algo, split_k=case.split_k, proj=case.proj)
    if case.res:
        d.res = p
    if case.pool:
        d.pool_y = p
    if case.nchw:
        from centertrack_amd import _lib
        d.flags, d.ldy = _lib.CT_OUT_NCHW, 0
    for v, ld in L.pitches(lim).items():
        setattr(d, L.CONV_FIELD[v], ld + (L.PITCH_STEP if v == bump else 0))
    return d


DCN_FIELD = dict(x='ldx', y='ldy', om='ldom', up='up_ldy', skip='up_lds')


def dcn_desc(p, case, wide, bump=None):
    import _dcn_fwd as D
    d = TD._desc(p, case.N, case.H, case.W, case.Cin, case.Cout, algo=case.algo, split_k=case.split_k, fuse_offset=D.FUSE_OFFSET[case.src], up_f=case.up_f)
    if case.src == 'wino':
        d.w_off_winograd = p
    for v, ld in wide.items():
        setattr(d, DCN_FIELD[v], ld + (L.PITCH_STEP if v == bump else 0))
    return d


def dcn_bwd_desc(p, wide, bump=None):
    from centertrack_amd import _lib
    B, Cin, Cout, H, W, _ = L.DCN_BWD_SHAPE
    d = _lib.DcnBwdDesc()
    d.x = d.om = d.gy = d.wT_packed = d.gx = d.gom = d.gw = d.gb = d.workspace = p
    d.N, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, Cout
    d.ldx, d.ldom, d.ldgy, d.ldgx, d.ldgom = Cin, 32, Cout, Cin, 32
    d.flags, d.workspace_bytes = _lib.CT_DCN_BWD_INPUT | _lib.CT_DCN_BWD_OFFSET_MASK | _lib.CT_DCN_BWD_WEIGHT, TD.HUGE
    for v, ld in wide.items():
        setattr(d, L.DCN_BWD_VIEWS[v], ld + (L.PITCH_STEP if v == bump else 0))
    return d


def bn_descs(p, wide, bump=None):
    """[(entry point, descriptor)] of the three BatchNorm calls on L.BN_SHAPE: statistics, BN + residual + ReLU, its backward"""
    from centertrack_amd import _lib
    N, H, W, Cc = L.BN_SHAPE
    out = []
    for entry, cls in (('ct_bn_stats', _lib.BnDesc), ('ct_bn_act_apply', _lib.BnActDesc), ('ct_bn_act_backward', _lib.BnActDesc)):
        d = cls()
        d.z = d.mean = d.var = d.invstd = d.gamma = d.beta = d.workspace = p
        d.N, d.H, d.W, d.C, d.ldz, d.eps, d.workspace_bytes = N, H, W, Cc, Cc, 1e-5, TD.HUGE
        if entry == 'ct_bn_act_apply':
            d.y, d.ldy, d.res, d.ldr, d.flags = p, Cc, p, Cc, _lib.CT_BN_ACT_RELU
        if entry == 'ct_bn_act_backward':
            d.gy = d.gz = d.gres = d.res = d.ggamma = d.gbeta = p
            d.ldgy = d.ldgz = d.ldgres = d.ldr = Cc
            d.flags = _lib.CT_BN_ACT_RELU | _lib.CT_BN_BATCH_STATS
        for v, ld in wide.items():
            field, entries = L.BN_VIEWS[v]
            if entry in entries:
                setattr(d, field, ld + (L.PITCH_STEP if v == bump else 0))
        out.append((entry, d))
    return out


def train_rc(lib, p, op, wide, bump=None):
    """the return code of the entry point of ``op`` (L.TRAIN_OPS) on fake pointers, the views of ``wide`` at their pitch (``bump``: one step up)"""
    from centertrack_amd import _lib
    ld = lambda v, tight: wide.get(v, tight) + (L.PITCH_STEP if v == bump else 0)
    if op == 'pool_bwd':
        N, H, W, Cc = L.TRAIN_SHAPES[op]
        return lib.ct_maxpool2x2_backward(p, N, H, W, Cc, ld('x', Cc), p, ld('gy', Cc), p, ld('add', Cc), p, ld('gx', Cc), None)
    if op == 'mask_sigmoid':
        N, H, W = L.TRAIN_SHAPES[op]
        return lib.ct_dcn_mask_sigmoid_backward(p, ld('g', 32), p, ld('om', 32), N, H, W, None)
    if op == 's2_bwd':
        N, H, W, Cin, Cout = L.TRAIN_SHAPES[op]
        d = _lib.ConvS2BwdDesc()
        d.x = d.gy = d.w_s2t = d.gx = d.gw = d.workspace = p
        d.N, d.H, d.W, d.Cin, d.Cout, d.workspace_bytes = N, H, W, Cin, Cout, TD.HUGE
        d.ldx, d.ldgy, d.ldgx = ld('x', Cin), ld('gy', Cout), ld('gx', Cin)
        return lib.ct_conv2d_s2_backward(ctypes.byref(d), None)
    if op == 'up_bwd':
        N, H, W, Cc, f = L.TRAIN_SHAPES[op]
        d = _lib.UpsampleBwdDesc()
        d.gy = d.w = d.gx = d.x = d.gw = d.workspace = p
        d.N, d.H, d.W, d.C, d.f, d.workspace_bytes = N, H, W, Cc, f, TD.HUGE
        d.ldgy, d.ldgx, d.ldx = ld('gy', Cc), ld('gx', Cc), ld('x', Cc)
        return lib.ct_upsample_add_backward(ctypes.byref(d), None)
    if op == 'cw_bwd':
        N, H, W, Cin, Cout, ks = L.TRAIN_SHAPES[op]
        d = _lib.ConvBwdWeightDesc()
        d.x = d.gy = d.gw = d.gb = d.workspace = p
        d.N, d.H, d.W, d.Cin, d.Cout, d.ks, d.stride, d.workspace_bytes = N, H, W, Cin, Cout, ks, 1, TD.HUGE
        d.ldx, d.ldgy = ld('x', Cin), ld('gy', Cout)
        return lib.ct_conv2d_backward_weight(ctypes.byref(d), None)
    import _heads_slots as S
    N, H, W, M = L.TRAIN_SHAPES['slots']
    d = _lib.SlotDesc()
    d.map = d.ind = d.rows = p
    d.N, d.H, d.W, d.C, d.M, d.ld, d.ldr = N, H, W, S.CIN, M, ld('map', S.CIN), ld('rows', 9 * S.CIN)
    return (lib.ct_slot_fold if op == 'slot_fold' else lib.ct_slot_gather)(ctypes.byref(d), None)


def stem_rcs(lib, p, view, ld):
    """{entry point: (return code, message)} of the stem calls that take ``view`` (L.STEM_VIEWS) at pitch ``ld``, all three stems, fake pointers"""
    from centertrack_amd import _lib
    N, H, W = L.STEM_SHAPE
    pitch = lambda name: ld if name == view else 16
    c = _lib.StemConvDesc()
    c.N, c.H, c.W, c.workspace, c.workspace_bytes = N, H, W, p, TD.HUGE
    u = _lib.StemSumDesc()
    u.N, u.H, u.W, u.y, u.ldy = N, H, W, p, pitch('y')
    for s in range(3):
        c.inp[s] = c.w[s] = c.z[s] = c.gz[s] = c.gw[s] = c.gin[s] = p
        c.ldz[s], c.ldgz[s] = pitch('z%d' % s), pitch('gz%d' % s)
        u.z[s] = u.mean[s] = u.invstd[s] = u.gamma[s] = u.beta[s] = p
        u.ldz[s] = pitch('z%d' % s)
    calls = dict(ct_stem_conv_forward=c, ct_stem_bn_relu_sum=u, ct_stem_conv_backward=c)
    out = {}
    for entry in L.STEM_VIEWS[view]:
        rc = getattr(lib, entry)(ctypes.byref(calls[entry]), None)
        out[entry] = (rc, lib.ct_last_error().decode())
    return out


def pixels_desc(p, px, **kw):
    f = dict(W=px.W, ldx=px.ldx, ldy=px.ldy)
    f.update(kw)
    W = f.pop('W')
    if px.entry == 'ct_conv2d':
        return TC._desc(p, px.N, px.H, W, px.Cin, px.Cout, 1, 1, algo=px.algo, split_k=px.split_k, **f)
    Cout = f.pop('Cout', px.Cout)
    return TD._desc(p, px.N, px.H, W, px.Cin, Cout, algo=px.algo, split_k=px.split_k, **dict(f, ldy=max(f['ldy'], Cout)))


def accepted_calls(lib, p):
    """{name: rc} of every case of the table, called as it stands (the child process without a device runs this)"""
    import _dcn_fwd as D
    from centertrack_amd import _lib
    out = {}
    for lim in L.LIMITS:
        if lim.kind == 'conv':
            out[lim.name] = lib.ct_conv2d(ctypes.byref(conv_desc(p, lim)), None)
        else:
            out[lim.name] = lib.ct_dcn_v2(ctypes.byref(dcn_desc(p, lim.case, L.pitches(lim))), None)
    g = L.Limit('dcn_group', 'ct_dcn_v2_group', 'dcn', L.DCN_GROUP[1], ('x', 'y'), '')
    arr = (_lib.DcnDesc * 2)(dcn_desc(p, L.DCN_GROUP[0], {}), dcn_desc(p, L.DCN_GROUP[1], L.pitches(g)))
    out['dcn_group'] = lib.ct_dcn_v2_group(arr, 2, 7, None)
    for name, px in L.MANY_PIXELS.items():
        out[name] = (lib.ct_conv2d if px.entry == 'ct_conv2d' else lib.ct_dcn_v2)(ctypes.byref(pixels_desc(p, px)), None)
    ld = L.widest_batch_pitch(L.DCN_BWD_SHAPE[0] * L.DCN_BWD_SHAPE[3] * L.DCN_BWD_SHAPE[4])
    for v in L.DCN_BWD_VIEWS:
        out['dcn_bwd_' + v] = lib.ct_dcn_v2_backward(ctypes.byref(dcn_bwd_desc(p, {v: ld})), None)
    ld = L.widest_batch_pitch(L.BN_SHAPE[0] * L.BN_SHAPE[1] * L.BN_SHAPE[2])
    for v in L.BN_VIEWS:
        rcs = [getattr(lib, entry)(ctypes.byref(d), None) for entry, d in bn_descs(p, {v: ld})]
        out['bn_' + v] = max(rcs, key=lambda rc: rc not in (_lib.CT_OK, _lib.CT_ERR_LAUNCH))
    for op, v in L.TRAIN_CASES:
        out['%s_%s' % (op, v)] = train_rc(lib, p, op, {v: L.widest_batch_pitch(L.TRAIN_OPS[op][1][v])})
    ld = L.widest_batch_pitch(L.STEM_SHAPE[0] * L.STEM_SHAPE[1] * L.STEM_SHAPE[2])
    for v in L.STEM_VIEWS:
        out['stem_' + v] = max((rc for rc, _ in stem_rcs(lib, p, v, ld).values()), key=lambda rc: rc not in (_lib.CT_OK, _lib.CT_ERR_LAUNCH))
    return out


def test_every_case_is_refused_one_step_up(lib):
    from centertrack_amd import _lib
    keep, p = TC._ptr()
    n = 0

    def refused(rc, words, what):
        msg = lib.ct_last_error().decode()
        assert rc == _lib.CT_ERR_ARG and all(w in msg for w in words), (what, rc, msg)
        return 1
    for lim in L.LIMITS:
        for v in lim.wide:
            if lim.kind == 'conv':
                n += refused(lib.ct_conv2d(ctypes.byref(conv_desc(p, lim, bump=v)), None), ('2 GiB', '(%s:' % L.CONV_WORD[v]), (lim.name, v))
            else:
                words = L.dcn_limit_of(lim.case, v)[1]
                if words is not None:
                    n += refused(lib.ct_dcn_v2(ctypes.byref(dcn_desc(p, lim.case, L.pitches(lim), bump=v)), None), (words,), (lim.name, v))
    g = L.Limit('dcn_group', 'ct_dcn_v2_group', 'dcn', L.DCN_GROUP[1], ('x', 'y'), '')
    for v in g.wide:
        arr = (_lib.DcnDesc * 2)(dcn_desc(p, L.DCN_GROUP[0], {}), dcn_desc(p, L.DCN_GROUP[1], L.pitches(g), bump=v))
        n += refused(lib.ct_dcn_v2_group(arr, 2, 7, None), (L.dcn_limit_of(L.DCN_GROUP[1], v)[1],), ('dcn_group', v))
    px = L.MANY_PIXELS['conv_pixels']
    n += refused(lib.ct_conv2d(ctypes.byref(pixels_desc(p, px, ldx=px.ldx + 4)), None), ('2 GiB', '(x:'), 'conv_pixels x')
    n += refused(lib.ct_conv2d(ctypes.byref(pixels_desc(p, px, ldy=px.ldy + 4)), None), ('2 GiB', '(y:'), 'conv_pixels y')
    px = L.MANY_PIXELS['dcn_pixels']
    n += refused(lib.ct_dcn_v2(ctypes.byref(pixels_desc(p, px, W=px.W + 1)), None), ('H*W <= 2^23',), 'dcn_pixels')
    px = L.MANY_PIXELS['dcn_partials']
    assert px.H * px.W * px.Cout < 2 ** 29 == px.H * px.W * (px.Cout + 16)
    n += refused(lib.ct_dcn_v2(ctypes.byref(pixels_desc(p, px, Cout=px.Cout + 1)), None), ('a partial map of 2 GiB or more',), 'dcn_partials')
    ld = L.widest_batch_pitch(L.DCN_BWD_SHAPE[0] * L.DCN_BWD_SHAPE[3] * L.DCN_BWD_SHAPE[4])
    for v in L.DCN_BWD_VIEWS:
        n += refused(lib.ct_dcn_v2_backward(ctypes.byref(dcn_bwd_desc(p, {v: ld}, bump=v)), None), ('a view of 2 GiB or more',), 'dcn_bwd ' + v)
    ld = L.widest_batch_pitch(L.BN_SHAPE[0] * L.BN_SHAPE[1] * L.BN_SHAPE[2])
    for v, (field, entries) in L.BN_VIEWS.items():
        for entry, d in bn_descs(p, {v: ld}, bump=v):
            if entry in entries:
                n += refused(getattr(lib, entry)(ctypes.byref(d), None), (entry + ': a view of 2 GiB or more',), 'bn ' + v)
    for op, v in L.TRAIN_CASES:
        rc = train_rc(lib, p, op, {v: L.widest_batch_pitch(L.TRAIN_OPS[op][1][v])}, bump=v)
        n += refused(rc, (L.TRAIN_OPS[op][0] + ': a view of 2 GiB or more',), (op, v))
    ld = L.widest_batch_pitch(L.STEM_SHAPE[0] * L.STEM_SHAPE[1] * L.STEM_SHAPE[2])
    for v in L.STEM_VIEWS:
        for entry, (rc, msg) in stem_rcs(lib, p, v, ld + L.PITCH_STEP).items():
            assert rc == _lib.CT_ERR_ARG and (entry + ': a view of 2 GiB or more') in msg, (entry, v, rc, msg)
            n += 1
    assert n >= 65


def test_every_case_is_accepted():
    """just below its limit every case passes validation: the call then reaches the launch, which this test must not let happen on a
    GPU -- a child process that sees no device makes the calls, and gets the launch error of a machine without one"""
    from centertrack_amd import _lib
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.dirname(__file__)] + sys.path))
    code = ('import json, torch\n'
            'import test_limits_cpu as T\n'
            'from centertrack_amd import _lib\n'
            'if torch.cuda.device_count() > 0:\n'
            '    print(json.dumps("a device is visible: not launching")); raise SystemExit(0)\n'
            'lib = _lib.load(); keep, p = T.TC._ptr()\n'
            'print(json.dumps(T.accepted_calls(lib, p)))\n')
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert isinstance(out, dict), out
    assert set(out) == case_names()
    for name, rc in out.items():
        assert rc in (_lib.CT_OK, _lib.CT_ERR_LAUNCH), (name, rc)


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic

def test_the_pitches_worked_out_by_hand():
    assert L.widest_pitch(12 * 20, 64) == 2246320 and L.extent_bytes(240, 2246320, 64) == 2 ** 31 - 1472
    assert L.widest_batch_pitch(2 * 12 * 20) == 1118480 and 480 * 1118480 * 4 == 2 ** 31 - 2048
    assert L.pitches(L.LIMIT['dcn_fused_ldx'])['x'] == 2 ** 21 - 4 and L.extent_bytes(256, 2 ** 21 - 4, 64) == 2139091216
    assert L.pitches(L.LIMIT['dcn_map_ldy'])['y'] == 2 ** 23 - 4


def test_the_largest_offsets_fit_the_types_that_hold_them():
    n = 0
    for lim in L.LIMITS + [L.Limit('dcn_group', 'ct_dcn_v2_group', 'dcn', L.DCN_GROUP[1], ('x', 'y'), '')]:
        rows = L.offsets_formed(lim)
        assert rows, lim.name
        for what, value, holds, where in rows:
            assert 0 <= value <= holds, (lim.name, what, value, holds, where)
            n += 1
    assert n > 80


def test_the_exact_references_equal_float64_on_exact_inputs():
    """13 x 21 pixels: the band references of the many-pixel cases against F.conv2d / oracle.dcn_v2 in float64, bit for bit, and every
    value is an fp32 number -- so is every partial sum, whatever the order (multiples of 1/64 below 2^24 / 64)"""
    from oracle import dcn_v2 as odcn
    H, W = 13, 21
    for name, p in L.MANY_PIXELS.items():
        d = L.exact_inputs(p, torch.device('cpu'), H=H, W=W)
        x = d['x'].permute(0, 3, 1, 2).double()
        if p.entry == 'ct_conv2d':
            z, band = F.conv2d(x, d['w'].double()), L.exact_conv_band
        else:
            om = d['om'].permute(0, 3, 1, 2).double()
            z, band = odcn.dcn_v2_conv(x, om[:, :18].contiguous(), om[:, 18:].contiguous(), d['w'].double(), None), L.exact_dcn_band
            terms = 9 * p.Cin * 4 * 2 * 64                                # |x| <= 4, |w| <= 2, in units of 1/64
            assert terms < 2 ** 24
            z32 = odcn.dcn_v2_conv(x.float(), om[:, :18].float().contiguous(), om[:, 18:].float().contiguous(), d['w'], None)
            assert torch.equal(z32.double(), z), 'float32 in the oracle\'s order is not exact on these inputs'
        ref = torch.relu(z * d['scale'].double().view(1, -1, 1, 1) + d['shift'].double().view(1, -1, 1, 1))
        got = torch.cat([band(d, 0, r, min(H, r + 5)) for r in range(0, H, 5)]).permute(2, 0, 1)
        assert torch.equal(got, ref[0]), name
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) > 4, name
