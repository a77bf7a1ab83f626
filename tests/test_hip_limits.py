"""GPU: every kernel at the largest view its host check accepts (tests/_limits.py).  A wide view lies inside an arena of
tests/_arena.py -- 2 GiB of sentinel in front, 4 GiB behind, the other channels of every pixel sentinel too -- so an offset that is
wrong by a sign or a 32-bit wrap changes memory the test owns and is counted on the device.  Each case is held against the float64
reference and the bound of the entry point's own GPU test, min(1e-3, 4 max(e32, 2^-23 sqrt(K))) (bit equality where that test asserts
bit equality), and against the same inputs launched at an ordinary pitch, bit for bit, after the workspace query has shown that both
launches run the same plan; the same descriptor one pitch step up must be refused with the existing message, which returns before
any launch.  In order: ``ct_conv2d``; ``ct_dcn_v2`` and ``ct_dcn_v2_group``; the two many-pixel cases, where the limit is on the pixel
index, held bit for bit against plain torch ops in float64 on inputs for which fp32 is exact in any order; ``ct_dcn_v2_backward``;
``ct_bn_stats`` / ``ct_bn_act_apply`` / ``ct_bn_act_backward``; the pool, stride-2 conv, conv weight, up-sampling and mask-sigmoid
backward and the two slot kernels; the three stem entry points.  Every test prints its extent in bytes, the distance to the
limit, its peak device memory (below 32 GiB, asserted) and its time (``pytest -s``)."""
import contextlib
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

import _backbone_bwd as BB
import _conv_fwd as C
import _dcn_bwd as B_
import _dcn_fwd as D
import _limits as L
from _arena import Arena
from _guards import GUARD, NAN, guarded, slice_of, take

pytestmark = pytest.mark.gpu

MEMORY_CAP = 32 * 2 ** 30


@contextlib.contextmanager
def measured(name, device):
    """prints the test's wall time and peak device memory, asserts the 32 GiB cap, and returns the arenas to the driver"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(device)
        torch.cuda.empty_cache()
        print('LIMIT %-24s %.2f s, peak device memory %.2f GiB' % (name, time.perf_counter() - t0, peak / 2.0 ** 30))
    assert peak < MEMORY_CAP, '%s held %.2f GiB of device memory' % (name, peak / 2.0 ** 30)


@contextlib.contextmanager
def tuning(knobs, defaults):
    from centertrack_amd import _lib
    lib = _lib.load()
    try:
        for k, v in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), v), k)
        yield
    finally:
        for k, _ in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), defaults[k]), k)


def report(name, view, ld, px, Cc, words='2 GiB'):
    """prints the view's extent and its distance to 2 GiB; where the 2 GiB check is the one that binds (``words``: the refusal one
    step up), the last pixel lies within one pitch of it"""
    ext = L.extent_bytes(px, ld, Cc)
    print('LIMIT %-24s %-5s pitch %8d floats, %4d pixels: extent %d bytes, %d below 2 GiB, one pitch is %d bytes; one step up: %s'
          % (name, view, ld, px, ext, L.GIB2 - ext, ld * 4, 'refused (%s)' % words if words else 'no host check'))
    assert 0 < L.GIB2 - ext
    if words is None or '2 GiB' in words:
        assert L.GIB2 - ext <= ld * 4, 'the last pixel is not within one pitch of the limit'


def refused(call, desc, field, words):
    """the descriptor with ``field`` one pitch step up is refused, with ``words`` in the message, before any launch"""
    from centertrack_amd import _lib
    lib = _lib.load()
    old = getattr(desc, field)
    setattr(desc, field, old + L.PITCH_STEP)
    try:
        rc = call(ctypes.byref(desc), _lib.stream_ptr())
        msg = lib.ct_last_error().decode()
    finally:
        setattr(desc, field, old)
    assert rc == _lib.CT_ERR_ARG and all(w in msg for w in words), (field, rc, msg)


class Holder(object):
    """the views of one launch: an arena for a wide view, the host-built buffers of tests/_guards.py for the others"""

    def __init__(self, device, wide):
        self.device, self.wide, self.arenas, self.plain = device, wide, {}, {}

    def input(self, name, t, **kw):
        if name in self.wide:
            N, Cc, H, W = t.shape
            self.arenas[name] = Arena(N, H, W, Cc, self.wide[name], self.device).fill(t)
            return self.arenas[name].view
        self.plain[name] = slice_of(t, self.device, **kw)
        return self.plain[name]

    def inout(self, name, t, **kw):
        """a view an entry point rewrites in place: filled like an input, taken like an output"""
        if name in self.wide:
            return self.input(name, t)
        N, Cc, H, W = t.shape
        v = self.output(name, N, H, W, Cc, **kw)
        v.buf[..., v.c0:v.c0 + Cc] = t.permute(0, 2, 3, 1).to(self.device)
        return v

    def output(self, name, N, H, W, Cc, **kw):
        if name in self.wide:
            self.arenas[name] = Arena(N, H, W, Cc, self.wide[name], self.device)
            return self.arenas[name].view
        self.plain[name] = guarded(N, H, W, Cc, self.device, **kw)
        return self.plain[name]

    def take(self, name, what):
        if name in self.arenas:
            return self.arenas[name].take('%s %s' % (what, name))
        return take(self.plain[name], '%s %s' % (what, name))

    def inputs_intact(self, names, what):
        for name in names:
            if name in self.arenas:
                self.arenas[name].check('%s %s (an input)' % (what, name))

    def free(self):
        for a in self.arenas.values():
            a.free()
        self.arenas, self.plain = {}, {}


def same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: %s differs in %d elements' % (what, k, int((a[k] != b[k]).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# ct_conv2d

def conv_launch(lim, device, wide):
    """one ``ct_conv2d`` of the case with the views of ``wide`` (name -> pitch) in arenas -> (outputs NCHW on the CPU, workspace bytes)"""
    from centertrack_amd import _lib, ops
    lib, case = _lib.load(), lim.case
    d, p = C.conv_inputs(case), C.plan_of(case)
    h = Holder(device, wide)
    dev = lambda t: None if t is None else t.to(device)
    w = d['w'].to(device)
    kw = dict(scale=dev(d['scale']), shift=dev(d['shift']), relu=case.relu, split_k=case.split_k, algo=case.algo)
    if p['family'] == 'wino':
        kw['w_wino'] = ops.pack_winograd(w)
    if case.res:
        kw['res'] = h.input('res', d['res'], c0=8, tail=8)
    flat = None
    if case.nchw:
        n = case.N * case.Cout * p['Ho'] * p['Wo']
        flat = torch.full((n + 128,), GUARD)
        flat[64:64 + n] = NAN
        flat = flat.to(device)
        kw.update(out_nchw=flat[64:64 + n].view(case.N, case.Cout, p['Ho'], p['Wo']), sig=case.sig, dep=case.dep, depth_scale=C.DEPTH_SCALE)
    else:
        kw['out'] = h.output('y', case.N, p['Ho'], p['Wo'], case.Cout)
    if case.pool:
        kw['pool'] = h.output('pool', case.N, case.H // 2, case.W // 2, case.Cin, c0=8)
    if case.proj:
        kw['proj'] = (ops.pack_weight(d['pw'].to(device)), d['pscale'].to(device), d['pshift'].to(device),
                      h.output('proj', case.N, p['Ho'], p['Wo'], case.Cout))
    wp = ops.pack_weight(w)                                                # (the descriptor holds raw pointers: kept alive here)
    desc = ops.make_conv_desc(h.input('x', d['x']), wp, case.Cout, case.ks, case.stride, **kw)
    try:
        with tuning(case.knobs, C.KNOBS):
            need = lib.ct_conv2d_workspace_bytes(ctypes.byref(desc))
            assert need == p['bytes'], (lim.name, need, p['bytes'])
            for v in wide:
                refused(lib.ct_conv2d, desc, L.CONV_FIELD[v], ('2 GiB', '(%s:' % L.CONV_WORD[v]))
            _lib.check(lib.ct_conv2d(ctypes.byref(desc), _lib.stream_ptr()), 'ct_conv2d ' + lim.name)
            torch.cuda.synchronize()
        out = {}
        if case.nchw:
            f = flat.cpu()
            assert bool((f[:64] == GUARD).all()) and bool((f[-64:] == GUARD).all()), lim.name + ': wrote outside its NCHW tensor'
            out['y'] = f[64:-64].view(case.N, case.Cout, p['Ho'], p['Wo']).clone()
            assert not bool(torch.isnan(out['y']).any()), lim.name + ': NCHW elements never written'
        else:
            out['y'] = h.take('y', lim.name)
        for name in ('pool', 'proj'):
            if getattr(case, name):
                out[name] = h.take(name, lim.name)
        h.inputs_intact(('x', 'res'), lim.name)
    finally:
        h.free()
    return out, need


CONV_LIMITS = [l.name for l in L.LIMITS if l.kind == 'conv']


@pytest.mark.parametrize('name', CONV_LIMITS)
def test_conv2d_at_the_widest_pitch(device, name):
    lim = L.LIMIT[name]
    case, dims, wide = lim.case, L.conv_view_dims(lim.case), L.pitches(lim)
    with measured(name, device):
        for v, ld in wide.items():
            report(name, v, ld, *dims[v])
        if case.N > 1:
            px, Cc = dims['x']
            first, last = px * wide['x'] * 4, (case.N - 1) * px * wide['x'] * 4 + L.extent_bytes(px, wide['x'], Cc)
            print('LIMIT %-24s image 1 of x starts at byte %d, the batch view ends at byte %d' % (name, first, last))
            assert 2 ** 31 < first < last                 # (a 64-bit base per image: 32 bits do not hold ``last``)
        got, need = conv_launch(lim, device, wide)
        r64, bad = C.reference64(case), []
        for which in ('y', 'proj'):
            if which in got:
                e, e32, b = C.case_errors(case, got[which], which)
                print('LIMIT %-24s %-5s err %.3e e32 %.3e bound %.3e ratio %.3f' % (name, which, e, e32, b, e / b))
                if not e <= b:
                    bad.append('%s err %.3e > bound %.3e' % (which, e, b))
        if 'pool' in got:
            assert torch.equal(got['pool'], r64['pool']), 'the pool side output is not F.max_pool2d of the input'
        assert not bad, '%s (%s): %s' % (name, lim.why, bad)
        plain, need0 = conv_launch(lim, device, {})
        assert need0 == need
        same(got, plain, name + ': the widest pitch against an ordinary one')


# ---------------------------------------------------------------------------------------------------------------------
# ct_dcn_v2, ct_dcn_v2_group

DCN_FIELD = dict(x='ldx', y='ldy', om='ldom', up='up_ldy', skip='up_lds')
ALL_PHASES = 1 | 2 | 4


class Built(object):
    pass


def dcn_build(case, device, wide):
    """the descriptor of a case with the views of ``wide`` (name -> pitch) in arenas, its workspace filled with NaN"""
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    d = D.dcn_inputs(case)
    N, H, W, Cout = case.N, case.H, case.W, case.Cout
    b = Built()
    b.case, b.h = case, Holder(device, wide)
    h = b.h
    xv = h.input('x', d['x'])
    wp = ops.pack_weight(d['w'].to(device))
    own = case.src in D.OWN
    om = part = wop = wow = bo = None
    if own:
        wod = d['wo'].to(device)
        wop, bo = ops.pack_weight(wod), d['bo'].to(device)
        if case.src != 'fused':
            part = torch.full((D.offsets_bytes(N, H, W, case.Cin, D.FUSE_OFFSET[case.src]) // 4,), NAN, device=device)
        if case.src == 'wino':
            wow = ops.pack_winograd(wod)
    else:
        omt = torch.cat([d['off'], d['mask']], 1)
        if 'om' in wide:
            om = h.input('om', omt)
        else:
            buf = torch.full((N, H, W, case.ldom), NAN)
            buf[..., :27] = omt.permute(0, 2, 3, 1)
            om = ops.View(buf.to(device), 0, 27)
    yv = h.output('y', N, H, W, Cout)
    upt = None
    if case.up_f:
        f = case.up_f
        upt = (ops.upsample_weight(d['wup'].to(device)), f, h.input('skip', d['skip'], c0=8, tail=8), h.output('up', N, H * f, W * f, Cout, c0=8))
    scale, shift = d['scale'].to(device), d['shift'].to(device)
    b.desc = ops.make_dcn_desc(xv, om, wp, Cout, scale, shift, True, yv, split_k=case.split_k, algo=case.algo, w_off=wop if own else None,
                               b_off=bo, up=upt, om_partial=part, w_off_wino=wow)
    query = lib.ct_dcn_v2_group_workspace_bytes if case.entry == 'group' else lib.ct_dcn_v2_workspace_bytes
    b.need = query(ctypes.byref(b.desc))
    assert b.need == D.plan_of(case)['bytes'], (case.name, b.need)
    b.ws = torch.full((max(b.need, 4) // 4,), NAN, device=device)
    b.desc.workspace, b.desc.workspace_bytes = b.ws.data_ptr(), b.need
    b.keep = (wp, wop, wow, bo, om, part, scale, shift, upt)
    return b


def dcn_collect(b):
    torch.cuda.synchronize()
    case, h, out = b.case, b.h, {}
    try:
        if D.y_written(case):
            out['y'] = h.take('y', case.name)
        elif 'y' in h.arenas:
            h.arenas['y'].check(case.name + ' y (not produced)')
        if case.up_f:
            out['up'] = h.take('up', case.name)
        h.inputs_intact(('x', 'om', 'skip'), case.name)
    finally:
        h.free()
    return out


def dcn_launch(lim, device, wide):
    """one ``ct_dcn_v2`` of the case -> (outputs NCHW on the CPU, workspace bytes); with wide views, first the refusals one step up"""
    from centertrack_amd import _lib
    lib, case = _lib.load(), lim.case
    with tuning(case.knobs, D.KNOBS):
        b = dcn_build(case, device, wide)
        try:
            for v in wide:
                words = L.dcn_limit_of(case, v)[1]
                if words is not None:
                    refused(lib.ct_dcn_v2, b.desc, DCN_FIELD[v], (words,))
            _lib.check(lib.ct_dcn_v2(ctypes.byref(b.desc), _lib.stream_ptr()), 'ct_dcn_v2 ' + lim.name)
        except BaseException:
            b.h.free()
            raise
        return dcn_collect(b), b.need


def dcn_check(name, case, got):
    assert sorted(got) == sorted(D.outputs_of(case)), (name, sorted(got))
    bad = []
    for which in D.outputs_of(case):
        e, e32, b = D.case_errors(case, got[which], which)
        print('LIMIT %-24s %-5s err %.3e e32 %.3e bound %.3e ratio %.3f' % (name, which, e, e32, b, e / b))
        if not e <= b:
            bad.append('%s err %.3e > bound %.3e' % (which, e, b))
    assert not bad, '%s (%s): %s' % (name, case.why, bad)


DCN_LIMITS = [l.name for l in L.LIMITS if l.kind == 'dcn']


@pytest.mark.parametrize('name', DCN_LIMITS)
def test_dcn_v2_at_the_widest_pitch(device, name):
    lim = L.LIMIT[name]
    case, dims, wide = lim.case, L.dcn_view_dims(lim.case), L.pitches(lim)
    with measured(name, device):
        for v, ld in wide.items():
            report(name, v, ld, *dims[v], words=L.dcn_limit_of(case, v)[1])
        if D.plan_of(case)['family'] == 'persist':
            batch = case.N * case.H * case.W * wide['x'] * 4
            print('LIMIT %-24s x of the batch: %d bytes, %d below 4 GiB' % (name, batch, 2 ** 32 - batch))
            assert 0 < 2 ** 32 - batch <= case.N * case.H * case.W * L.PITCH_STEP * 4
        got, need = dcn_launch(lim, device, wide)
        dcn_check(name, case, got)
        plain, need0 = dcn_launch(lim, device, {})
        assert need0 == need
        same(got, plain, name + ': the widest pitch against an ordinary one')


def test_dcn_v2_group_with_one_layer_at_the_widest_pitch(device):
    """two layers of one tile shape in one call, the second with x and y at their widest pitches, against the layers launched singly"""
    from centertrack_amd import _lib
    lib = _lib.load()
    name = 'dcn_group'
    layers = L.DCN_GROUP
    wide = L.pitches(L.Limit(name, 'ct_dcn_v2_group', 'dcn', layers[1], ('x', 'y'), ''))
    with measured(name, device):
        for v, ld in wide.items():
            report(name, v, ld, *L.dcn_view_dims(layers[1])[v], words=L.dcn_limit_of(layers[1], v)[1])
        built = [dcn_build(layers[0], device, {}), dcn_build(layers[1], device, wide)]
        try:
            arr = (_lib.DcnDesc * 2)(*[b.desc for b in built])
            for v in wide:
                refused(lambda ref, s: lib.ct_dcn_v2_group(arr, 2, ALL_PHASES, s), arr[1], DCN_FIELD[v], (L.dcn_limit_of(layers[1], v)[1],))
            _lib.check(lib.ct_dcn_v2_group(arr, 2, ALL_PHASES, _lib.stream_ptr()), 'ct_dcn_v2_group')
        except BaseException:
            for b in built:
                b.h.free()
            raise
        got = [dcn_collect(b) for b in built]
        for c, out in zip(layers, got):
            dcn_check(name + ' ' + c.name, c, out)
            b = dcn_build(c, device, {})
            _lib.check(lib.ct_dcn_v2_group(ctypes.byref(b.desc), 1, ALL_PHASES, _lib.stream_ptr()), 'ct_dcn_v2_group ' + c.name)
            same(out, dcn_collect(b), c.name + ': in the group at the widest pitch against alone at an ordinary one')


# ---------------------------------------------------------------------------------------------------------------------
# the many-pixel cases

@pytest.mark.parametrize('name', list(L.MANY_PIXELS))
def test_the_largest_pixel_count(device, name):
    from centertrack_amd import _lib, ops
    lib, p = _lib.load(), L.MANY_PIXELS[name]
    conv = p.entry == 'ct_conv2d'
    with measured(name, device):
        d = L.exact_inputs(p, device)
        xa = Arena(p.N, p.H, p.W, p.Cin, p.ldx, device)
        xa.view.buf[..., :p.Cin] = d['x']
        ya = Arena(p.N, p.H, p.W, p.Cout, p.ldy, device)
        print('LIMIT %-24s %d pixels; x: extent %d bytes, %d below 2 GiB; y: extent %d bytes' % (
            name, p.H * p.W, xa.extent, L.GIB2 - xa.extent, ya.extent))
        wp = ops.pack_weight(d['w'])
        if conv:
            assert L.GIB2 - xa.extent == 64
            desc = ops.make_conv_desc(xa.view, wp, p.Cout, 1, 1, scale=d['scale'], shift=d['shift'], relu=True, out=ya.view, split_k=1, algo=p.algo)
            call, band = lib.ct_conv2d, L.exact_conv_band
            assert lib.ct_conv2d_workspace_bytes(ctypes.byref(desc)) == 0
            refused(call, desc, 'ldx', ('2 GiB', '(x:'))
            refused(call, desc, 'ldy', ('2 GiB', '(y:'))
        else:
            if name == 'dcn_pixels':
                oa = Arena(p.N, p.H, p.W, 27, 32, device)
                oa.view.buf[..., :27] = d['om']
                omv = oa.view
            else:                                                          # (the partial maps take the arena's place under the 32 GiB cap)
                oa, om = None, torch.full((p.N, p.H, p.W, 32), NAN, device=device)
                om[..., :27] = d['om']
                omv = ops.View(om, 0, 27)
            desc = ops.make_dcn_desc(xa.view, omv, wp, p.Cout, d['scale'], d['shift'], True, ya.view, split_k=p.split_k, algo=p.algo)
            call, band = lib.ct_dcn_v2, L.exact_dcn_band
            need = lib.ct_dcn_v2_workspace_bytes(ctypes.byref(desc))
            if name == 'dcn_pixels':
                assert p.H * p.W == L.DCN_PIXELS and need == 0
                field, words = 'W', 'H*W <= 2^23'                          # one more column: 2^23 + 2048 pixels
            else:                                                          # the partial maps in an arena of their own
                floats = p.H * p.W * p.Cout
                assert need == p.split_k * floats * 4 and floats < 2 ** 29 == p.H * p.W * (p.Cout + 16)
                wa = Arena(1, 1, p.split_k * p.H * p.W, p.Cout, p.Cout, device)
                desc.workspace, desc.workspace_bytes = wa.view.ptr, need
                print('LIMIT %-24s %d splits of %d floats of partials (%d bytes each, %d below 2 GiB)' % (name, p.split_k, floats, floats * 4, L.GIB2 - floats * 4))
                field, words = 'Cout', 'a partial map of 2 GiB or more'    # one more cout: the map grows to 128 couts, 2^29 floats
            setattr(desc, field, getattr(desc, field) + 1)
            desc.ldy += L.PITCH_STEP                                       # (room for the one more cout, and a workspace size that
            held = desc.workspace_bytes                                    #  passes the check in front of the one meant)
            desc.workspace_bytes = 1 << 40
            try:
                rc, msg = call(ctypes.byref(desc), _lib.stream_ptr()), lib.ct_last_error().decode()
            finally:
                setattr(desc, field, getattr(desc, field) - 1)
                desc.ldy -= L.PITCH_STEP
                desc.workspace_bytes = held
            assert rc == _lib.CT_ERR_ARG and words in msg, (rc, msg)
        _lib.check(call(ctypes.byref(desc), _lib.stream_ptr()), p.entry + ' ' + name)
        torch.cuda.synchronize()
        y = ya.take_device(name + ' y')
        xa.check(name + ' x (an input)')
        if name == 'dcn_partials':
            wa.check(name + ' partial maps')
        wrong = torch.zeros((), dtype=torch.int64, device=device)
        top = torch.zeros((), dtype=torch.float64, device=device)
        for n in range(p.N):
            for r0 in range(0, p.H, L.BAND):
                ref = band(d, n, r0, min(p.H, r0 + L.BAND))
                wrong += (y[n, r0:r0 + L.BAND].double() != ref).sum()
                top = torch.maximum(top, ref.abs().max())
        print('LIMIT %-24s %d of %d elements differ from the float64 reference (largest value %.2f)' % (name, int(wrong), y.numel(), float(top)))
        assert int(wrong) == 0 and float(top) > 4
        del y, d
        for a in (xa, ya) + ((oa,) if name == 'dcn_pixels' else ()) + ((wa,) if name == 'dcn_partials' else ()):
            a.free()


# ---------------------------------------------------------------------------------------------------------------------
# ct_dcn_v2_backward

_plain_cache = {}


def dcn_bwd_launch(device, wide):
    """one ``ct_dcn_v2_backward`` of L.DCN_BWD_SHAPE with the views of ``wide`` (name -> pitch) in arenas -> (gradients on the CPU,
    workspace bytes)"""
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    B, Cin, Cout, H, W, _ = L.DCN_BWD_SHAPE
    inp, g64, e32 = B_.truth_of_shape(L.DCN_BWD_SHAPE)
    x, off, mask, w, _, gy = inp
    h = Holder(device, wide)
    try:
        xv, gyv = h.input('x', x), h.input('gy', gy, c0=8, tail=8)
        if 'om' in wide:
            omv = h.input('om', torch.cat([off, mask], 1))
        else:
            om = torch.zeros((B, H, W, 32))
            om[..., :27] = torch.cat([off, mask], 1).permute(0, 2, 3, 1)
            omv = ops.View(om.to(device), 0, 27)
        gxv, gomv = h.output('gx', B, H, W, Cin, c0=8), h.output('gom', B, H, W, 27, c0=4, tail=4)
        gw, gb = torch.full((Cout, Cin, 3, 3), NAN, device=device), torch.full((Cout,), NAN, device=device)
        wT = ops.pack_weight_t(w.to(device))                              # (the descriptor holds raw pointers: kept alive here)
        desc = ops.make_dcn_bwd_desc(xv, omv, gyv, wT, gx=gxv, gom=gomv, gw=gw, gb=gb)
        need = lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(desc))
        ws = torch.full((max(need, 4) // 4,), NAN, device=device)
        if need:
            desc.workspace, desc.workspace_bytes = ws.data_ptr(), need
        for v in wide:
            refused(lib.ct_dcn_v2_backward, desc, L.DCN_BWD_VIEWS[v], ('a view of 2 GiB or more',))
        _lib.check(lib.ct_dcn_v2_backward(ctypes.byref(desc), _lib.stream_ptr()), 'ct_dcn_v2_backward')
        torch.cuda.synchronize()
        gom = h.take('gom', 'dcn_bwd')
        out = dict(x=h.take('gx', 'dcn_bwd'), offset=gom[:, :18].contiguous(), mask=gom[:, 18:].contiguous(), weight=gw.cpu(), bias=gb.cpu())
        h.inputs_intact(('x', 'om', 'gy'), 'dcn_bwd')
    finally:
        h.free()
    return out, need


@pytest.mark.parametrize('view', list(L.DCN_BWD_VIEWS))
def test_dcn_v2_backward_at_the_widest_pitch(device, view):
    shape = L.DCN_BWD_SHAPE
    B, Cin, Cout, H, W, _ = shape
    name = 'dcn_bwd_' + view
    with measured(name, device):
        ld = L.widest_batch_pitch(B * H * W)
        print('LIMIT %-24s %-5s pitch %8d floats, %4d pixels in the batch: %d bytes, %d below 2 GiB; one step up: refused'
              % (name, view, ld, B * H * W, B * H * W * ld * 4, L.GIB2 - B * H * W * ld * 4))
        _, g64, e32 = B_.truth_of_shape(shape)
        K = B_.terms(shape)
        got, need = dcn_bwd_launch(device, {view: ld})
        bad = []
        for n in B_.NAMES:
            e, b = B_.err(got[n], g64[n]), B_.bound(e32[n], K[n])
            print('LIMIT %-24s g_%-6s err %.3e e32 %.3e bound %.3e ratio %.3f' % (name, n, e, e32[n], b, e / b))
            if not e <= b:
                bad.append('g_%s err %.3e > bound %.3e' % (n, e, b))
        assert not bad, bad
        if 'dcn_bwd' not in _plain_cache:
            _plain_cache['dcn_bwd'] = dcn_bwd_launch(device, {})
        plain, need0 = _plain_cache['dcn_bwd']
        assert need0 == need
        for n in ('offset', 'mask', 'weight', 'bias'):                    # (g_x is summed with float atomics: held to the bound alone)
            assert torch.equal(got[n], plain[n]), 'g_%s at the widest %s differs from the ordinary pitch in %d elements' % (n, view, int((got[n] != plain[n]).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# ct_bn_stats, ct_bn_act_apply, ct_bn_act_backward

def bn_launch(device, wide):
    """batch statistics, BatchNorm + residual + ReLU and its backward on L.BN_SHAPE with the views of ``wide`` (name -> pitch) in
    arenas -> dict of results on the CPU"""
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    N, H, W, Cc = L.BN_SHAPE
    z, gamma, beta, rm, rv, gy, res = BB.bn_case(L.BN_SHAPE)
    h = Holder(device, wide)
    try:
        zv, rsv, gyv = h.input('z', z), h.input('res', res, c0=8, tail=8), h.input('gy', gy, c0=8, tail=4)
        yv, gzv, grv = h.output('y', N, H, W, Cc), h.output('gz', N, H, W, Cc, c0=8), h.output('gres', N, H, W, Cc, c0=12)
        g, b = gamma.to(device), beta.to(device)
        mean, var, invstd = (torch.full((Cc,), NAN, device=device) for _ in range(3))
        gg, gb = torch.full((Cc,), NAN, device=device), torch.full((Cc,), NAN, device=device)
        ds = ops._bn_desc(_lib.BnDesc, zv, mean, invstd)
        ds.var, ds.eps = var.data_ptr(), BB.EPS
        ws0 = ops._workspace(lib, 'ct_bn_workspace_bytes', ds, device)
        da = ops._bn_act_desc(zv, mean, invstd, g, b, rsv, True)
        da.y, da.ldy = yv.ptr, yv.ld
        db = ops._bn_act_desc(zv, mean, invstd, g, b, rsv, True, True)
        db.gy, db.ldgy, db.gz, db.ldgz, db.gres, db.ldgres = gyv.ptr, gyv.ld, gzv.ptr, gzv.ld, grv.ptr, grv.ld
        db.ggamma, db.gbeta = gg.data_ptr(), gb.data_ptr()
        ws1 = ops._workspace(lib, 'ct_bn_act_workspace_bytes', db, device)
        calls = (('ct_bn_stats', ds), ('ct_bn_act_apply', da), ('ct_bn_act_backward', db))
        for v in wide:
            field, entries = L.BN_VIEWS[v]
            for entry, d in calls:
                if entry in entries:
                    refused(getattr(lib, entry), d, field, (entry + ': a view of 2 GiB or more',))
        for entry, d in calls:
            _lib.check(getattr(lib, entry)(ctypes.byref(d), _lib.stream_ptr()), entry)
        torch.cuda.synchronize()
        out = dict(mean=mean.cpu(), var=var.cpu(), invstd=invstd.cpu(), gg=gg.cpu(), gb=gb.cpu(), y=h.take('y', 'bn'), gz=h.take('gz', 'bn'),
                   gr=h.take('gres', 'bn'))
        h.inputs_intact(('z', 'res', 'gy'), 'bn')
        keep = (ws0, ws1)
    finally:
        h.free()
    return out


@pytest.mark.parametrize('view', list(L.BN_VIEWS))
def test_batch_norm_at_the_widest_pitch(device, view):
    import test_hip_backbone_backward as TB
    N, H, W, Cc = L.BN_SHAPE
    P, name = N * H * W, 'bn_' + view
    with measured(name, device):
        ld = L.widest_batch_pitch(P)
        print('LIMIT %-24s %-5s pitch %8d floats, %4d pixels in the batch: %d bytes, %d below 2 GiB; one step up: refused'
              % (name, view, ld, P, P * ld * 4, L.GIB2 - P * ld * 4))
        case = BB.bn_case(L.BN_SHAPE)
        got = bn_launch(device, {view: ld})
        mask = got['y'] > 0
        free64, free32 = (TB.bn_reference(case, dt, True, True, True) for dt in (torch.float64, torch.float32))
        t64, t32 = (TB.bn_reference(case, dt, True, True, True, mask) for dt in (torch.float64, torch.float32))
        rep = BB.Report('LIMIT %-24s' % name)
        BB.check_mask(mask, free64['pre'], BB.err(free32['y'], free64['y']), name)
        rep.add('y', got['y'], free64['y'], free32['y'], P)
        rep.add('gz', got['gz'], t64['gz'], t32['gz'], P)
        rep.add('ggamma', got['gg'], t64['gg'], t32['gg'], P)
        rep.add('gbeta', got['gb'], t64['gb'], t32['gb'], P)
        rep.add('gres', got['gr'], t64['gr'], t32['gr'], P)
        assert torch.equal(got['gr'], torch.where(mask, case[5], torch.zeros_like(case[5])))          # a pure selection
        rep.check()
        if 'bn' not in _plain_cache:
            _plain_cache['bn'] = bn_launch(device, {})
        for k, v in _plain_cache['bn'].items():                              # bitwise reproducible, and a pitch changes no order
            assert torch.equal(got[k], v), '%s at the widest %s differs from the ordinary pitch in %d elements' % (k, view, int((got[k] != v).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# ct_maxpool2x2_backward, ct_conv2d_s2_backward, ct_upsample_add_backward, ct_dcn_mask_sigmoid_backward, ct_slot_gather, ct_slot_fold
#
# Each op below builds its views (``wide``: name -> pitch, in arenas), and returns ``call(bump)`` -- the C entry point on those
# buffers with the pitch of view ``bump`` one step up, or as it stands -- and ``collect()`` -> its results on the CPU.

def _pool_bwd(h, device):
    from centertrack_amd import _lib
    lib = _lib.load()
    N, H, W, Cc = L.TRAIN_SHAPES['pool_bwd']
    x = BB.tie_input(41, N, Cc, H, W)
    gy, add = BB.randn(42, N, Cc, H // 2, W // 2).float(), BB.randn(43, N, Cc, H, W).float()
    v = dict(x=h.input('x', x), gy=h.input('gy', gy, c0=8, tail=8), add=h.input('add', add), gx=h.output('gx', N, H, W, Cc))

    def call(bump=None):
        ld = dict((k, v[k].ld + (L.PITCH_STEP if k == bump else 0)) for k in v)
        return lib.ct_maxpool2x2_backward(v['x'].ptr, N, H, W, Cc, ld['x'], v['gy'].ptr, ld['gy'], v['add'].ptr, ld['add'], v['gx'].ptr, ld['gx'],
                                          _lib.stream_ptr())

    def collect():
        got = dict(gx=h.take('gx', 'pool_bwd'))
        xt = x.clone().requires_grad_()
        plain, = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, gy)
        assert torch.equal(got['gx'], plain + add), 'a pure selection plus one fp32 addition: bitwise'
        return got
    return call, collect, ('x', 'gy', 'add'), v


def _s2_bwd(h, device):
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    shape = L.TRAIN_SHAPES['s2_bwd']
    N, H, W, Cin, Cout = shape
    x, w, gy, ref = BB.s2_case(shape)
    v = dict(x=h.input('x', x), gy=h.input('gy', gy, c0=8, tail=8), gx=h.output('gx', N, H, W, Cin, c0=8))
    d = _lib.ConvS2BwdDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = v['x'].ptr, N, H, W, Cin, v['x'].ld
    d.gy, d.Cout, d.ldgy = v['gy'].ptr, Cout, v['gy'].ld
    wp = ops.pack_weight_s2t(w.to(device))
    d.w_s2t, d.gx, d.ldgx = wp.data_ptr(), v['gx'].ptr, v['gx'].ld
    ws = ops._workspace(lib, 'ct_conv2d_s2_backward_workspace_bytes', d, device)
    gw = torch.full((Cout, Cin, 3, 3), NAN, device=device)
    d.gw = gw.data_ptr()
    field = dict(x='ldx', gy='ldgy', gx='ldgx')

    def call(bump=None):
        if bump:
            setattr(d, field[bump], getattr(d, field[bump]) + L.PITCH_STEP)
        try:
            return lib.ct_conv2d_s2_backward(ctypes.byref(d), _lib.stream_ptr())
        finally:
            if bump:
                setattr(d, field[bump], getattr(d, field[bump]) - L.PITCH_STEP)

    def collect():
        got = dict(gx=h.take('gx', 's2_bwd'), gw=gw.cpu())
        rep = BB.Report('LIMIT s2_bwd')
        rep.add('gx', got['gx'], ref[torch.float64][0], ref[torch.float32][0], 4 * Cout)
        rep.add('gw', got['gw'], ref[torch.float64][1], ref[torch.float32][1], N * (H // 2) * (W // 2))
        rep.check()
        return got
    return call, collect, ('x', 'gy'), (v, wp, ws, gw)


def _up_bwd(h, device):
    import _neck_bwd as NB
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    N, H, W, Cc, f = L.TRAIN_SHAPES['up_bwd']
    x, w = NB.randn(51, N, Cc, H, W).float(), (NB.randn(52, Cc, 1, 2 * f, 2 * f) * 0.5 / f).float()
    skip, gy = NB.randn(53, N, Cc, H * f, W * f).float(), NB.randn(54, N, Cc, H * f, W * f).float()
    v = dict(x=h.input('x', x), gy=h.input('gy', gy, c0=8, tail=4), gx=h.output('gx', N, H, W, Cc, c0=8))
    d = _lib.UpsampleBwdDesc()
    d.gy, d.N, d.H, d.W, d.C, d.ldgy, d.f = v['gy'].ptr, N, H, W, Cc, v['gy'].ld, f
    wu = ops.upsample_weight(w.to(device))
    gw = torch.full((Cc, 1, 2 * f, 2 * f), NAN, device=device)
    d.w, d.gx, d.ldgx, d.x, d.ldx, d.gw = wu.data_ptr(), v['gx'].ptr, v['gx'].ld, v['x'].ptr, v['x'].ld, gw.data_ptr()
    ws = ops._workspace(lib, 'ct_upsample_add_backward_workspace_bytes', d, device)
    field = dict(x='ldx', gy='ldgy', gx='ldgx')

    def call(bump=None):
        if bump:
            setattr(d, field[bump], getattr(d, field[bump]) + L.PITCH_STEP)
        try:
            return lib.ct_upsample_add_backward(ctypes.byref(d), _lib.stream_ptr())
        finally:
            if bump:
                setattr(d, field[bump], getattr(d, field[bump]) - L.PITCH_STEP)

    def collect():
        got = dict(gx=h.take('gx', 'up_bwd'), gw=gw.cpu())
        ref = {}
        for dt in (torch.float64, torch.float32):
            t = [t_.to(dt).requires_grad_() for t_ in (x, w, skip)]
            ref[dt] = torch.autograd.grad(NB.upsample_add(t[0], t[1], f, t[2]), t[:2], gy.to(dt))
        rep = BB.Report('LIMIT up_bwd')
        rep.add('gx', got['gx'], ref[torch.float64][0], ref[torch.float32][0], 4 * f * f)
        rep.add('gw', got['gw'], ref[torch.float64][1], ref[torch.float32][1], N * H * W)
        rep.check()
        return got
    return call, collect, ('x', 'gy'), (v, wu, ws, gw)


def _cw_bwd(h, device):
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    N, H, W, Cin, Cout, ks = L.TRAIN_SHAPES['cw_bwd']
    x, gy = B_.randn(71, N, Cin, H, W).float(), B_.randn(72, N, Cout, H, W).float()
    v = dict(x=h.input('x', x), gy=h.input('gy', gy, c0=8, tail=8))
    d = _lib.ConvBwdWeightDesc()
    d.x, d.N, d.H, d.W, d.Cin, d.ldx = v['x'].ptr, N, H, W, Cin, v['x'].ld
    d.gy, d.Cout, d.ldgy, d.ks, d.stride = v['gy'].ptr, Cout, v['gy'].ld, ks, 1
    ws = ops._workspace(lib, 'ct_conv2d_backward_weight_workspace_bytes', d, device)
    gw, gb = torch.full((Cout, Cin, ks, ks), NAN, device=device), torch.full((Cout,), NAN, device=device)
    d.gw, d.gb = gw.data_ptr(), gb.data_ptr()
    field = dict(x='ldx', gy='ldgy')

    def call(bump=None):
        if bump:
            setattr(d, field[bump], getattr(d, field[bump]) + L.PITCH_STEP)
        try:
            return lib.ct_conv2d_backward_weight(ctypes.byref(d), _lib.stream_ptr())
        finally:
            if bump:
                setattr(d, field[bump], getattr(d, field[bump]) - L.PITCH_STEP)

    def collect():
        got = dict(gw=gw.cpu(), gb=gb.cpu())
        w64, w32 = (torch.nn.grad.conv2d_weight(x.to(dt), (Cout, Cin, ks, ks), gy.to(dt), padding=ks // 2) for dt in (torch.float64, torch.float32))
        rep = BB.Report('LIMIT cw_bwd')
        rep.add('gw', got['gw'], w64, w32, N * H * W)
        rep.add('gb', got['gb'], gy.double().sum((0, 2, 3)), gy.sum((0, 2, 3)), N * H * W)
        rep.check()
        return got
    return call, collect, ('x', 'gy'), (v, ws, gw, gb)


def _mask_sigmoid(h, device):
    from centertrack_amd import _lib
    lib = _lib.load()
    N, H, W = L.TRAIN_SHAPES['mask_sigmoid']
    g0, om = B_.randn(61, N, 27, H, W).float(), torch.cat([B_.randn(62, N, 18, H, W), torch.sigmoid(B_.randn(63, N, 9, H, W))], 1).float()
    v = dict(g=h.inout('g', g0, c0=4, tail=1), om=h.input('om', om, c0=8, tail=4))              # (g is rewritten in place: an input that is an output)

    def call(bump=None):
        ld = dict((k, v[k].ld + (L.PITCH_STEP if k == bump else 0)) for k in v)
        return lib.ct_dcn_mask_sigmoid_backward(v['g'].ptr, ld['g'], v['om'].ptr, ld['om'], N, H, W, _lib.stream_ptr())

    def collect():
        got = dict(g=h.take('g', 'mask_sigmoid'))
        assert torch.equal(got['g'][:, :18], g0[:, :18]), 'the offset channels are not touched'
        m64 = om[:, 18:].double()
        r64, r32 = g0[:, 18:].double() * m64 * (1 - m64), g0[:, 18:] * om[:, 18:] * (1 - om[:, 18:])
        e, e32 = B_.err(got['g'][:, 18:], r64), B_.err(r32, r64)
        print('LIMIT mask_sigmoid             err %.3e e32 %.3e bound %.3e' % (e, e32, B_.bound(e32, 1)))
        assert e <= B_.bound(e32, 1)
        return got
    return call, collect, ('om',), v


def _slots(fold):
    def build(h, device):
        import _heads_slots as S
        from centertrack_amd import _lib
        lib = _lib.load()
        N, H, W, M = L.TRAIN_SHAPES['slots']
        Cc = S.CIN
        (shape, ind) = S.CASES['random-3x8x8x17']
        assert shape == (N, H, W, M)
        gen = torch.Generator().manual_seed(23)
        feat, rows0 = torch.randn((N, Cc, H, W), generator=gen), torch.randn((N, 9 * Cc, 1, M), generator=gen)
        ind_d = ind.to(device)
        v = dict(map=(h.inout if fold else h.input)('map', feat, c0=8, tail=8))
        v['rows'] = h.input('rows', rows0, c0=0, tail=16) if fold else h.output('rows', N, 1, M, 9 * Cc, c0=0, tail=16)
        d = _lib.SlotDesc()
        d.map, d.N, d.H, d.W, d.C, d.ld = v['map'].ptr, N, H, W, Cc, v['map'].ld
        d.ind, d.M, d.rows, d.ldr = ind_d.data_ptr(), M, v['rows'].ptr, v['rows'].ld
        field = dict(map='ld', rows='ldr')
        entry = lib.ct_slot_fold if fold else lib.ct_slot_gather

        def call(bump=None):
            if bump:
                setattr(d, field[bump], getattr(d, field[bump]) + L.PITCH_STEP)
            try:
                return entry(ctypes.byref(d), _lib.stream_ptr())
            finally:
                if bump:
                    setattr(d, field[bump], getattr(d, field[bump]) - L.PITCH_STEP)

        def collect():
            x_nhwc = feat.permute(0, 2, 3, 1).contiguous()
            if fold:                                                        # cells no slot covers are not written: they keep their input
                got = dict(map=h.take('map', 'slot_fold'))
                P = rows0.permute(0, 2, 3, 1).reshape(N, M, 9, Cc)
                want = S.fold_owner_order(P, ind, x_nhwc)[0]
                assert torch.equal(got['map'].permute(0, 2, 3, 1).contiguous().view(torch.int32), want.contiguous().view(torch.int32)), 'slot_fold: not the owner-order sum'
            else:
                got = dict(rows=h.take('rows', 'slot_gather'))
                want = S.gather_ref(x_nhwc, ind).view(N, 1, M, 9 * Cc)
                assert torch.equal(got['rows'].permute(0, 2, 3, 1).contiguous().view(torch.int32), want.contiguous().view(torch.int32)), 'slot_gather: not torch indexing'
            return got
        return call, collect, (('rows',) if fold else ('map',)), (v, ind_d)
    return build


TRAIN_BUILDERS = dict(cw_bwd=_cw_bwd, pool_bwd=_pool_bwd, s2_bwd=_s2_bwd, up_bwd=_up_bwd, mask_sigmoid=_mask_sigmoid, slot_gather=_slots(False), slot_fold=_slots(True))


def train_launch(op, device, wide):
    from centertrack_amd import _lib
    lib = _lib.load()
    entry = L.TRAIN_OPS[op][0]
    h = Holder(device, wide)
    try:
        call, collect, inputs, keep = TRAIN_BUILDERS[op](h, device)
        for v in wide:
            rc, msg = call(v), lib.ct_last_error().decode()
            assert rc == _lib.CT_ERR_ARG and (entry + ': a view of 2 GiB or more') in msg, (op, v, rc, msg)
        _lib.check(call(), entry)
        torch.cuda.synchronize()
        out = collect()
        h.inputs_intact(inputs, op)
    finally:
        h.free()
    return out


@pytest.mark.parametrize('op,view', L.TRAIN_CASES, ids=lambda v: str(v))
def test_training_ops_at_the_widest_pitch(device, op, view):
    name = '%s_%s' % (op, view)
    with measured(name, device):
        px = L.TRAIN_OPS[op][1][view]
        ld = L.widest_batch_pitch(px)
        print('LIMIT %-24s %-5s pitch %8d floats, %4d pixels in the batch: %d bytes, %d below 2 GiB; one step up: refused'
              % (name, view, ld, px, px * ld * 4, L.GIB2 - px * ld * 4))
        got = train_launch(op, device, {view: ld})
        if op not in _plain_cache:
            _plain_cache[op] = train_launch(op, device, {})
        for k, v in _plain_cache[op].items():                               # bitwise reproducible ops: a pitch changes no order
            assert torch.equal(got[k], v), '%s: %s at the widest %s differs from the ordinary pitch in %d elements' % (op, k, view, int((got[k] != v).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# ct_stem_conv_forward, ct_stem_bn_relu_sum, ct_stem_conv_backward

class Bumped(object):
    """a view as the wrappers of centertrack_amd.ops read it, its pitch one step up: for the refusal, which returns before any launch"""

    def __init__(self, v):
        self.buf, self.c0, self.C, self.N, self.H, self.W, self.ptr, self.ld = v.buf, v.c0, v.C, v.N, v.H, v.W, v.ptr, v.ld + L.PITCH_STEP


def wrapper_refused(entry, fn, *args, **kw):
    from centertrack_amd import _lib
    with pytest.raises(_lib.CTError) as ei:
        fn(*args, **kw)
    msg = _lib.load().ct_last_error().decode()              # (the wrapper's workspace query runs the same check first, under its own name)
    assert msg.startswith(entry) and ': a view of 2 GiB or more' in msg, (entry, msg, str(ei.value))


def stem_launch(device, wide):
    """tests/test_hip_stem_backward.py::hip_ops on L.STEM_SHAPE (three stems, batch statistics) with the views of ``wide`` in arenas"""
    import _stem_bwd as SB
    from centertrack_amd import ops
    N, H, W = L.STEM_SHAPE
    stems = (0, 1, 2)
    sd, xs, gy = SB.case(L.STEM_SHAPE)
    h = Holder(device, wide)
    try:
        dx = [xs[s].to(device) for s in stems]
        dw = [sd[SB.PREFIX[s] + '0.weight'].to(device) for s in stems]
        zv = [h.output('z%d' % s, N, H, W, 16) for s in stems]
        if 'z1' in wide:
            wrapper_refused('ct_stem_conv_forward', ops.stem_conv_forward, dx, dw, out=[zv[0], Bumped(zv[1]), zv[2]])
        zs = ops.stem_conv_forward(dx, dw, out=zv)
        means, invstds, gammas, betas, var = [None] * 3, [None] * 3, [None] * 3, [None] * 3, [None] * 3
        for s in stems:
            p = SB.PREFIX[s]
            gammas[s], betas[s] = sd[p + '1.weight'].to(device), sd[p + '1.bias'].to(device)
            means[s], var[s], invstds[s] = ops.bn_stats(zs[s], BB.EPS)
        terms = [ops.bn_relu_apply(zs[s], means[s], invstds[s], gammas[s], betas[s]) for s in stems]
        yv = h.output('y', N, H, W, 16, c0=8, tail=8)
        if 'z1' in wide:
            wrapper_refused('ct_stem_bn_relu_sum', ops.stem_bn_relu_sum, [zs[0], Bumped(zs[1]), zs[2]], means, invstds, gammas, betas, out=yv)
        if 'y' in wide:
            wrapper_refused('ct_stem_bn_relu_sum', ops.stem_bn_relu_sum, zs, means, invstds, gammas, betas, out=Bumped(yv))
        ops.stem_bn_relu_sum(zs, means, invstds, gammas, betas, out=yv)
        gyv = slice_of(gy, device, c0=4, tail=4)
        gzs, gg, gb = [None] * 3, [None] * 3, [None] * 3
        for s in stems:
            gzs[s], gg[s], gb[s] = ops.bn_relu_backward(zs[s], gyv, means[s], invstds[s], gammas[s], betas[s], True)
        torch.cuda.synchronize()
        gzv = [h.input('gz%d' % s, gzs[s].to_nchw().cpu(), c0=0, tail=4) for s in stems]           # the gradients of z as views with a pitch
        gws = [torch.full((16, SB.CIN[s], 7, 7), NAN, device=device) for s in stems]
        gins = [torch.full((N, SB.CIN[s], H, W), NAN, device=device) for s in stems]
        if 'gz2' in wide:
            wrapper_refused('ct_stem_conv_backward', ops.stem_conv_backward, [gzv[0], gzv[1], Bumped(gzv[2])], dx, dw, need_w=(True,) * 3,
                            need_in=(True,) * 3, gws=gws, gins=gins)
        gw, gin = ops.stem_conv_backward(gzv, dx, dw, need_w=(True,) * 3, need_in=(True,) * 3, gws=gws, gins=gins)
        torch.cuda.synchronize()
        res = dict(y=h.take('y', 'stems'), stems={})
        for s in stems:
            res['stems'][s] = dict(z=h.take('z%d' % s, 'stems'), term=terms[s].to_nchw().cpu(), gw=gw[s].cpu(), gin=gin[s].cpu(), ggamma=gg[s].cpu(),
                                   gbeta=gb[s].cpu(), mean=means[s].cpu(), var=var[s].cpu())
        h.inputs_intact(['gz%d' % s for s in stems], 'stems')
    finally:
        h.free()
    return res


@pytest.mark.parametrize('view', list(L.STEM_VIEWS))
def test_stems_at_the_widest_pitch(device, view):
    import test_hip_stem_backward as TS
    N, H, W = L.STEM_SHAPE
    P, name = N * H * W, 'stem_' + view
    with measured(name, device):
        ld = L.widest_batch_pitch(P)
        print('LIMIT %-24s %-5s pitch %8d floats, %4d pixels in the batch: %d bytes, %d below 2 GiB; one step up: refused'
              % (name, view, ld, P, P * ld * 4, L.GIB2 - P * ld * 4))
        got = stem_launch(device, {view: ld})
        rep = BB.Report('LIMIT %-24s' % name)
        TS.compare(rep, L.STEM_SHAPE, (0, 1, 2), True, got)
        rep.check()
        if 'stems' not in _plain_cache:
            _plain_cache['stems'] = TS.hip_ops(L.STEM_SHAPE, (0, 1, 2), True, device)
        TS.same_bits(got, _plain_cache['stems'])                             # every op, every bit: a pitch changes no order
