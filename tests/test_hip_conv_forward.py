"""GPU: every launch ``ct_conv2d`` can make (tests/_conv_fwd.py: GPU_CASES, one case per regime of its table) against a float64
reference under the bound of the backward tests, min(1e-3, 4 max(e32, 2^-23 sqrt(K))) with e32 the error of the float32
reference (``winograd32`` for a Winograd launch) by the same measure; x is read from a channel slice of a NaN-filled buffer, every
output is written into a NaN-filled slice between guard channels.  Then what must not change a bit: PIPE 0 / 1, the XCD remap, a
repeat, the side outputs, the tile shape.  ``ct_maxpool2x2``, ``ct_upsample_add`` and the layout converters likewise, including the
two shapes whose grid is capped.  Every test prints its figures (``pytest -s``)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import _conv_fwd as C
from _guards import GUARD, NAN, guarded as _guarded, slice_of as _slice_of, take as _take      # (shared with the DCN forward tests)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def tuning(knobs):
    from centertrack_amd import _lib
    lib = _lib.load()
    try:
        for k, v in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), v), k)
        yield
    finally:
        for k, _ in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), C.KNOBS[k]), k)


def _guarded_nchw(shape, device, margin=64):
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * margin,), GUARD)
    flat[margin:margin + n] = NAN
    flat = flat.to(device)
    return flat, flat[margin:margin + n].view(*shape)


def _take_nchw(flat, y, what, margin=64):
    f = flat.cpu()
    assert bool((f[:margin] == GUARD).all()) and bool((f[-margin:] == GUARD).all()), '%s: wrote outside its tensor' % what
    y = y.cpu().clone()
    assert not bool(torch.isnan(y).any()), '%s: %d elements never written' % (what, int(torch.isnan(y).sum()))
    return y


def launch(case, device, knobs=(), sides=True):
    """one ``ct_conv2d`` of the case under its knobs (then ``knobs``) -> dict(y[, pool][, proj]) NCHW on the CPU"""
    from centertrack_amd import ops
    d = C.conv_inputs(case)
    p = C.plan_of(case)
    dev = lambda t: None if t is None else t.to(device)
    w = d['w'].to(device)
    kw = dict(scale=dev(d['scale']), shift=dev(d['shift']), relu=case.relu, split_k=case.split_k, algo=case.algo)
    if p['family'] == 'wino':
        kw['w_wino'] = ops.pack_winograd(w)
    if case.res:
        kw['res'] = _slice_of(d['res'], device, c0=8, tail=8)           # a pitch of its own
    flat = yv = None
    if case.nchw:
        flat, y = _guarded_nchw((case.N, case.Cout, p['Ho'], p['Wo']), device)
        kw.update(out_nchw=y, sig=case.sig, dep=case.dep, depth_scale=C.DEPTH_SCALE)
    else:
        yv = _guarded(case.N, p['Ho'], p['Wo'], case.Cout, device)
    pv = qv = None
    if sides and case.pool:
        pv = kw['pool'] = _guarded(case.N, case.H // 2, case.W // 2, case.Cin, device, c0=8)
    if sides and case.proj:
        qv = _guarded(case.N, p['Ho'], p['Wo'], case.Cout, device)
        kw['proj'] = (ops.pack_weight(d['pw'].to(device)), d['pscale'].to(device), d['pshift'].to(device), qv)
    with tuning(tuple(case.knobs) + tuple(knobs)):
        ops.conv2d(_slice_of(d['x'], device), ops.pack_weight(w), case.Cout, case.ks, case.stride, out=yv, **kw)
        torch.cuda.synchronize()
    out = dict(y=_take_nchw(flat, kw['out_nchw'], case.name) if case.nchw else _take(yv, case.name))
    if pv is not None:
        out['pool'] = _take(pv, case.name + ' pool')
    if qv is not None:
        out['proj'] = _take(qv, case.name + ' proj')
    return out


def same(a, b, what):
    for k in a:
        if k in b:
            assert torch.equal(a[k], b[k]), '%s: %s differs in %d elements' % (what, k, int((a[k] != b[k]).sum()))


def family_of(case):
    p = C.plan_of(case)
    return 'split-K' if p['splits'] > 1 else {'row': 'row-tiled', 'ksplit': 'K-split', 'wino': 'Winograd'}[p['family']]


@pytest.mark.parametrize('name', list(C.CASE))
def test_conv2d_case_against_float64(device, name):
    case = C.CASE[name]
    got, r64 = launch(case, device), C.reference64(case)
    bad = []
    for which in ('y', 'proj'):
        if which in got:
            e, e32, b = C.case_errors(case, got[which], which)
            print('CONVFWD %-34s %-9s %-4s err %.3e e32 %.3e bound %.3e ratio %.3f' % (name, family_of(case), which, e, e32, b, e / b))
            if not e <= b:
                bad.append('%s err %.3e > bound %.3e' % (which, e, b))
    keep = ~C.plain_channels(case)
    if keep.any():                                                       # sigmoid and depth channels, element-wise
        b = C.case_errors(case, got['y'])[2]
        a, r = got['y'][:, keep].double(), r64['y'][:, keep]
        worst = float(((a - r).abs() / (r.abs() + 1)).max())
        print('CONVFWD %-34s %-9s sig  worst %.3e bound %.3e' % (name, family_of(case), worst, b))
        if not worst <= b:
            bad.append('sigmoid / depth channels: %.3e > %.3e' % (worst, b))
    if 'pool' in got:
        assert torch.equal(got['pool'], r64['pool']), 'the pool side output is not F.max_pool2d of the input'
    assert not bad, '%s (%s): %s' % (name, case.why, bad)
    same(got, launch(case, device), name + ': a repeat of the launch')
    if case.pool or case.proj:
        same(got, launch(case, device, sides=False), name + ': without the side outputs')


ROW_CASES = [c.name for c in C.GPU_CASES if C.plan_of(c)['family'] == 'row']


@pytest.mark.parametrize('name', ROW_CASES)
def test_conv_pipe_0_and_1_are_bit_identical(device, name):
    case = C.CASE[name]
    same(launch(case, device, (('conv_pipe', 1),)), launch(case, device, (('conv_pipe', 0),)), name + ': conv_pipe 0 against 1')


@pytest.mark.parametrize('name', ['xcd_row', 'xcd_ksplit', 'xcd_wino'])
def test_xcd_remap_changes_no_value(device, name):
    case = C.CASE[name]
    assert C.plan_of(case)['xcdPer'] > 0 and C.plan_of(case, (('xcd_remap', 0),))['xcdPer'] == 0
    same(launch(case, device), launch(case, device, (('xcd_remap', 0),)), name + ': xcd_remap 1 against 0')


@pytest.mark.parametrize('ks,stride,Cin', [(1, 1, 64), (3, 1, 32), (3, 2, 48)])
def test_row_tiled_shapes_are_bit_identical_to_each_other(device, ks, stride, Cin):
    """at splits == 1 every row-tiled shape adds the same products in the same order (slab-major, tap-minor, one MFMA chain per output)"""
    H, W = (19, 21) if stride == 1 else (37, 41)
    base = C.mk('cross_k%ds%d' % (ks, stride), 2, H, W, Cin, 43, ks, stride, 1, why='algos 1..8 on one shape')
    first = launch(base, device)
    for algo in range(2, 9):
        same(first, launch(base._replace(algo=algo), device), 'algo %d against algo 1 (ks %d, stride %d)' % (algo, ks, stride))
    e, e32, b = C.case_errors(base, first['y'])
    assert e <= b, (e, b)


# ---------------------------------------------------------------------------------------------------------------------
# element-wise ops

@pytest.mark.parametrize('shape', C.POOL_SHAPES, ids=str)
def test_maxpool2x2(device, shape):
    from centertrack_amd import ops
    N, H, W, Cc, pitched = shape
    x = torch.relu(C.randn(31, N, Cc, H, W)).float()                     # a post-ReLU map: windows of equal values
    xv = _slice_of(x, device) if pitched else ops.View(x.permute(0, 2, 3, 1).contiguous().to(device))
    yv = _guarded(N, H // 2, W // 2, Cc, device)
    ops.maxpool2x2(xv, out=yv)
    torch.cuda.synchronize()
    assert torch.equal(_take(yv, 'pool'), F.max_pool2d(x, 2, 2))


@pytest.mark.parametrize('shape', C.UP_SHAPES, ids=str)
def test_upsample_add(device, shape):
    from centertrack_amd import ops
    N, H, W, Cc, f, pitched = shape
    x, w, skip = C.upsample_inputs(shape)
    r64, r32 = C.upsample_reference(shape, torch.float64), C.upsample_reference(shape, torch.float32)
    view = (lambda t: _slice_of(t, device)) if pitched else (lambda t: ops.View(t.permute(0, 2, 3, 1).contiguous().to(device)))
    yv = _guarded(N, H * f, W * f, Cc, device)
    ops.upsample_add(view(x), w.to(device), f, view(skip), out=yv)
    torch.cuda.synchronize()
    e, e32 = C.err(_take(yv, 'upsample'), r64), C.err(r32, r64)
    b = C.bound(e32, 4)
    print('CONVFWD %-34s %-9s y    err %.3e e32 %.3e bound %.3e ratio %.3f' % ('upsample%s' % (shape,), 'upsampler', e, e32, b, e / b))
    assert e <= b, (e, b)


@pytest.mark.parametrize('shape', C.LAYOUT_SHAPES, ids=str)
def test_layout_converters(device, shape):
    from centertrack_amd import _lib
    Cc, H, W = shape
    N, lib = 2, _lib.load()
    x = C.randn(51, N, Cc, H, W).float()
    c0, ld = 2, Cc + 5
    buf = torch.full((N, H, W, ld), GUARD)
    buf[..., c0:c0 + Cc] = NAN
    buf, xd = buf.to(device), x.to(device)
    _lib.check(lib.ct_nchw_to_nhwc(xd.data_ptr(), N, Cc, H, W, buf.data_ptr() + 4 * c0, ld, _lib.stream_ptr()), 'ct_nchw_to_nhwc')
    torch.cuda.synchronize()
    b = buf.cpu()
    assert bool((b[..., :c0] == GUARD).all()) and bool((b[..., c0 + Cc:] == GUARD).all()), 'wrote outside its slice'
    assert torch.equal(b[..., c0:c0 + Cc], x.permute(0, 2, 3, 1))
    flat, y = _guarded_nchw((N, Cc, H, W), device)
    _lib.check(lib.ct_nhwc_to_nchw(buf.data_ptr() + 4 * c0, N, Cc, H, W, ld, y.data_ptr(), _lib.stream_ptr()), 'ct_nhwc_to_nchw')
    torch.cuda.synchronize()
    assert torch.equal(_take_nchw(flat, y, 'nhwc_to_nchw'), x)
