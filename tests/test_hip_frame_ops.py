"""GPU: every launch of the kernels a frame runs besides the convolutions, the DCN and the heat-map decode -- ``ct_stem_forward_parts``,
``ct_heads_fused``, ``ct_flip_merge`` / ``ct_flip_images``, ``ct_render_pre_hm``, ``ct_decode_pose`` -- on the cases of
tests/_frame_ops.py, which tests/test_frame_ops_cpu.py proves to reach every row of its regime tables.  Float results (stem, heads)
against float64 under min(1e-3, 4 max(e32, 2^-23 sqrt(K))); selections and exact arithmetic (flip, key points, every bitwise form)
bit for bit, ``kps_score`` to rtol 1e-5 / atol 1e-7; the prior heat map to one float32 ulp with fewer than 1e-3 of the touched
pixels not bit-equal.  Outputs are written into NaN-filled buffers between guards of 7.0; inputs the launch must not read are NaN.
Every float comparison prints a ``FRAMEOPS`` line (``pytest -s``)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import _frame_ops as P

pytestmark = pytest.mark.gpu
NAN, GUARD, MARGIN = float('nan'), 7.0, 64


@contextlib.contextmanager
def tuning(knob, value):
    from centertrack_amd import _lib
    lib = _lib.load()
    try:
        _lib.check(lib.ct_set_tuning(knob.encode(), value), knob)
        yield
    finally:
        _lib.check(lib.ct_set_tuning(knob.encode(), P.KNOBS[knob]), knob)


def _guarded(shape, device, dtype=torch.float32):
    """(flat, view): a NaN-filled tensor of ``shape`` between two margins of 7.0"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * MARGIN,), GUARD, dtype=dtype)
    flat[MARGIN:MARGIN + n] = NAN
    flat = flat.to(device)
    return flat, flat[MARGIN:MARGIN + n].view(*shape)


def _take(flat, view, what):
    f = flat.cpu()
    assert bool((f[:MARGIN] == GUARD).all()) and bool((f[-MARGIN:] == GUARD).all()), '%s: wrote outside its tensor' % what
    return view.cpu().clone()


def _line(case, what, e, e32, b):
    print('FRAMEOPS %-22s %-8s err %.3e e32 %.3e bound %.3e ratio %.3f' % (case, what, e, e32, b, e / b))


# ---------------------------------------------------------------------------------------------------------------------
# the stem

def stem_launch(shape, mask, device, add=None, ldy=16, knob=0, what='stem'):
    """one ``ct_stem_forward_parts`` of the stems in ``mask`` -> (NCHW result on the CPU, the NHWC device buffer).  ``add``: None, or
    (NCHW CPU tensor, ldadd) copied into a NaN-padded buffer, or (NHWC device buffer, ldadd) used as it is"""
    from centertrack_amd import _lib
    N, H, W = shape
    d = P.stem_inputs(N, H, W)
    ins = [d['inp'][s].to(device).contiguous() if mask >> s & 1 else None for s in range(3)]
    ws = [d['w'][s].to(device).contiguous() if mask >> s & 1 else None for s in range(3)]
    sc, sh = d['scale'].to(device), d['shift'].to(device)
    addbuf, ldadd = None, 0
    if add is not None:
        t, ldadd = add
        if t.dim() == 4 and t.shape[1] == 16 and not t.is_cuda:
            addbuf = torch.full((N, H, W, ldadd), NAN)
            addbuf[..., :16] = t.permute(0, 2, 3, 1)
            addbuf = addbuf.to(device)
        else:
            addbuf = t
    flat, y = _guarded((N, H, W, ldy), device)
    p = lambda t: None if t is None else t.data_ptr()
    with tuning('stem_rows', knob):
        _lib.check(_lib.load().ct_stem_forward_parts(p(ins[0]), p(ins[1]), p(ins[2]), p(addbuf), ldadd, N, H, W, p(ws[0]), p(ws[1]), p(ws[2]),
                                                     sc.data_ptr(), sh.data_ptr(), y.data_ptr(), ldy, _lib.stream_ptr()), 'ct_stem_forward_parts')
        torch.cuda.synchronize()
    out = _take(flat, y, what)
    assert bool(torch.isnan(out[..., 16:]).all()), '%s: wrote past channel 16 of a pitch-%d output' % (what, ldy)
    got = out[..., :16].permute(0, 3, 1, 2).contiguous()
    assert not bool(torch.isnan(got).any()), '%s: %d elements NaN or never written' % (what, int(torch.isnan(got).sum()))
    return got, y


def _case_launch(c, device, knob=None):
    d = P.stem_inputs(c.N, c.H, c.W)
    return stem_launch((c.N, c.H, c.W), c.mask, device, (d['add'], c.ldadd) if c.add else None, c.ldy, c.knob if knob is None else knob, c.name)[0]


@pytest.mark.parametrize('name', list(P.STEM_CASE))
def test_stem_case_against_float64(device, name):
    c = P.STEM_CASE[name]
    got = _case_launch(c, device)
    e, e32, b = P.stem_errors(c, got)
    _line(name, 'stem', e, e32, b)
    assert e <= b, '%s (%s): err %.3e > bound %.3e' % (name, c.why, e, b)
    if c.knob == 16 or name.startswith('auto_') or name.startswith('geo_'):
        for rows in (8, 16):                                  # the tile height changes no bit, whichever the launch picked
            again = _case_launch(c, device, rows)
            assert torch.equal(got, again), '%s: %d-row tiles differ in %d elements' % (name, rows, int((got != again).sum()))


@pytest.mark.parametrize('chain', [(3, 4), (1, 2, 4)], ids=['x+img_then_hm', 'x_then_img_then_hm'])
def test_stem_chain_equals_the_single_launch(device, chain):
    """{x, pre_img} -> {pre_hm} (the frame's two launches) and {x} -> {pre_img} -> {pre_hm}: the bits of ONE launch of all three, through
    partial maps of pitch 24 and 16; every partial map inside the bound of its own stems"""
    shape = P.SUBSET_SHAPE
    single = stem_launch(shape, 7, device)[0]
    done, buf, ld = 0, None, 0
    for i, mask in enumerate(chain):
        ldy = 24 if i % 2 == 0 else 16
        got, nxt = stem_launch(shape, mask, device, None if buf is None else (buf, ld), ldy, what='chain %s step %d' % (chain, i))
        buf, ld, done = nxt, ldy, done | mask
        r64, e32, b = P.stem_refs(*shape, done, False)
        e = P.err(got, r64)
        _line('chain_%s' % ''.join(map(str, chain)), 'to_m%d' % done, e, e32, b)
        assert e <= b, (chain, done, e, b)
    assert done == 7 and torch.equal(got, single), int((got != single).sum())


REGRESSION_SHAPE = (2, 128, 256)                             # 256 workgroups: one per CU of the decode that ran before


def test_subset_launches_right_after_a_decode_are_finite_and_in_bound(device):
    """A REGRESSION CHECK, NOT THE PROOF.  Before the fix a padding k of stem_kernel read plane 0 of its LDS, which a launch without
    ``x`` never stages; the decode keeps ~flat-index words in LDS that are NaN patterns as floats, and NaN * 0 = NaN.  Whether a
    workgroup meets such a word depends on what ran on its CU before and cannot be arranged through the ABI, so this test can pass on
    a wrong kernel.  What proves the fix is tests/test_frame_ops_cpu.py: every k an active stem visits maps into a plane the launch
    staged, and the restated rule is the source's.  Here: the launches without x, with and without a partial map, each issued on the
    decode's stream right behind it, are finite and inside their bound."""
    from centertrack_amd import ops
    g = torch.Generator().manual_seed(77)
    hm = torch.rand((4, 8, 96, 96), generator=g).to(device)
    dec = ops.Decoder(hm, {'wh': torch.rand((4, 2, 96, 96), generator=g).to(device)}, 100)
    d = P.stem_inputs(*REGRESSION_SHAPE)
    for mask in (2, 4, 6):
        for add in (False, True):
            dec.run()                                        # (no synchronisation in between: the stem follows on the same stream)
            got = stem_launch(REGRESSION_SHAPE, mask, device, (d['add'], 16) if add else None, what='m%d after a decode' % mask)[0]
            assert bool(torch.isfinite(got).all())
            r64, e32, b = P.stem_refs(*REGRESSION_SHAPE, mask, add)
            e = P.err(got, r64)
            _line('after_decode_m%d%s' % (mask, '_add' if add else ''), 'stem', e, e32, b)
            assert e <= b, (mask, add, e, b)


def test_stem_rejects_an_empty_subset(device):
    from centertrack_amd import _lib
    y = torch.zeros((1, 8, 8, 16), device=device)
    v = torch.zeros((3, 16), device=device)
    rc = _lib.load().ct_stem_forward_parts(None, None, None, None, 0, 1, 8, 8, None, None, None, v.data_ptr(), v.data_ptr(), y.data_ptr(), 16, _lib.stream_ptr())
    assert rc == _lib.CT_ERR_ARG and b'no stem selected' in _lib.load().ct_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the fused heads

class HeadsCall(object):
    """the device tensors and the descriptor of a case, kept alive together"""

    def __init__(self, name, device):
        from centertrack_amd import _lib, ops
        c, d = P.HEADS_CASE[name], P.heads_inputs(name)
        nh = len(c.cout)
        c0 = 16 if c.ldx > 64 else 0
        x = torch.full((c.N, c.H, c.W, c.ldx), NAN)
        x[..., c0:c0 + 64] = d['x'].permute(0, 2, 3, 1)
        self.x = x.to(device)
        self.w0 = ops.pack_winograd(torch.cat(d['w0'], 0).to(device))
        self.b0 = torch.cat(d['b0'], 0).to(device)
        w2, b2 = torch.zeros((nh, 8, 256)), torch.zeros((nh, 8))
        for i, co in enumerate(c.cout):
            w2[i, :co], b2[i, :co] = d['w2'][i], d['b2'][i]
        self.w2, self.b2 = w2.to(device), b2.to(device)
        hd = _lib.HeadsDesc()
        hd.x, hd.N, hd.H, hd.W, hd.Cin, hd.ldx = self.x.data_ptr() + 4 * c0, c.N, c.H, c.W, 64, c.ldx
        hd.w0_winograd, hd.b0, hd.nheads, hd.w2, hd.b2 = self.w0.data_ptr(), self.b0.data_ptr(), nh, self.w2.data_ptr(), self.b2.data_ptr()
        for i in range(nh):
            hd.cout[i], hd.coff[i] = c.cout[i], c.coff[i]
        hd.sig_lo, hd.sig_hi, hd.dep_lo, hd.dep_hi = P.heads_ranges(c)
        hd.ctot, hd.depth_scale = c.ctot, P.DEPTH_SCALE
        self.c, self.hd, self.device = c, hd, device

    def run(self, order=None):
        from centertrack_amd import _lib
        c = self.c
        flat, out = _guarded((c.N, c.ctot, c.H, c.W), self.device)
        self.hd.out = out.data_ptr()
        with tuning('heads_order', P.KNOBS['heads_order'] if order is None else order):
            _lib.check(_lib.load().ct_heads_fused(ctypes.byref(self.hd), _lib.stream_ptr()), 'ct_heads_fused')
            torch.cuda.synchronize()
        return _take(flat, out, c.name)


@pytest.mark.parametrize('name', list(P.HEADS_CASE))
def test_heads_case_against_float64(device, name):
    c = P.HEADS_CASE[name]
    call = HeadsCall(name, device)
    got = call.run()
    gap = torch.from_numpy(P.heads_unowned(c))
    assert bool(torch.isnan(got[:, gap]).all()), '%s: channels no head owns were written' % name
    assert not bool(torch.isnan(got[:, ~gap]).any()), '%s: %d elements NaN or never written' % (name, int(torch.isnan(got[:, ~gap]).sum()))
    bad = []
    for i, e, e32, b in P.heads_errors(name, got):
        kind = 'sig' if i == c.sig else 'dep' if i == c.dep else 'plain'
        _line(name, 'h%d:%dch:%s' % (i, c.cout[i], kind), e, e32, b)
        if not e <= b:
            bad.append('head %d (%s) err %.3e > bound %.3e' % (i, kind, e, b))
    assert not bad, '%s (%s): %s' % (name, c.why, bad)
    for order in (0, 1, 2):                                  # the workgroup order is a speed knob only
        again = call.run(order)
        same = (got == again) | (torch.isnan(got) & torch.isnan(again))
        assert bool(same.all()), '%s: heads_order %d differs in %d elements' % (name, order, int((~same).sum()))


def test_heads_rejects_nine_heads(device):
    from centertrack_amd import _lib
    call = HeadsCall('one', device)
    out = torch.zeros((1, 2, 4, 16), device=device)
    call.hd.out, call.hd.nheads = out.data_ptr(), P.CT_MAX_FUSED_HEADS + 1
    assert _lib.load().ct_heads_fused(ctypes.byref(call.hd), _lib.stream_ptr()) == _lib.CT_ERR_ARG
    torch.cuda.synchronize()
    assert not bool(out.any())


# ---------------------------------------------------------------------------------------------------------------------
# flip_test

def _lay(arr, how, device, lead=0):
    """the float32 array [n, ...] on the device as ``how`` says: 'dense'; 'offset' (4 bytes past a 16-byte boundary); 'stride+1' (one
    float between the images); 'slices' is laid by the caller"""
    t = torch.from_numpy(np.array(arr))
    if how == 'dense':
        return t.to(device)
    if how == 'offset':
        flat = torch.full((t.numel() + 4,), NAN)
        flat[1:1 + t.numel()] = t.reshape(-1)
        return flat.to(device)[1:1 + t.numel()].view(t.shape)
    assert how == 'stride+1'
    per = t[0].numel()
    flat = torch.full((t.shape[0] * (per + 1),), NAN)
    v = flat.as_strided(t.shape, (per + 1,) + tuple(t[0].stride()))
    v.copy_(t)
    return flat.to(device).as_strided(t.shape, (per + 1,) + tuple(t[0].stride()))


def flip_launch(name, device):
    from centertrack_amd import _lib
    c, srcs = P.FLIP_CASE[name], P.flip_inputs(name)
    if c.src == 'slices':                                      # one tensor [2B, 1 + sum C + 2, h, w], every head a channel slice of it
        wide = torch.full((2 * c.B, 3 + sum(C for C, _ in c.heads), c.h, c.w), NAN)
        c0, dev = 1, []
        for s in srcs:
            wide[:, c0:c0 + s.shape[1]] = torch.from_numpy(np.array(s))
            c0 += s.shape[1]
        wide, c0 = wide.to(device), 1
        for s in srcs:
            dev.append(wide[:, c0:c0 + s.shape[1]])
            c0 += s.shape[1]
    else:
        dev = [_lay(s, c.src, device) for s in srcs]
    arr = (_lib.FlipHead * len(c.heads))()
    outs = []
    for i, (t, (C, mode)) in enumerate(zip(dev, c.heads)):
        assert t.stride(1) == c.h * c.w and t.stride(0) >= C * c.h * c.w
        outs.append(_guarded((c.B, C, c.h, c.w), device))
        arr[i].src, arr[i].dst, arr[i].src_batch_stride, arr[i].C, arr[i].mode = t.data_ptr(), outs[-1][1].data_ptr(), t.stride(0), C, mode
    aligned = all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in dev)
    assert (c.w % 4 == 0 and aligned) == P.flip_plan(c)['vec'], 'the buffers do not lie as the plan assumes'
    pairs = np.ascontiguousarray(c.pairs, np.int32).reshape(-1, 2)
    _lib.check(_lib.load().ct_flip_merge(arr, len(c.heads), pairs.ctypes.data if len(pairs) else None, len(pairs), c.B, c.h, c.w, _lib.stream_ptr()), 'ct_flip_merge')
    torch.cuda.synchronize()
    return [_take(f, v, '%s head %d' % (name, i)).numpy() for i, (f, v) in enumerate(outs)]


@pytest.mark.parametrize('name', list(P.FLIP_CASE))
def test_flip_merge_case_bit_for_bit(device, name):
    for i, (got, want) in enumerate(zip(flip_launch(name, device), P.flip_reference(name))):
        np.testing.assert_array_equal(got, want, err_msg='%s head %d' % (name, i))


def test_flip_merge_rejects_nine_heads(device):
    from centertrack_amd import _lib
    src, dst = torch.zeros((2, 1, 4, 4), device=device), torch.zeros((1, 1, 4, 4), device=device)
    arr = (_lib.FlipHead * 9)()
    for i in range(9):
        arr[i].src, arr[i].dst, arr[i].src_batch_stride, arr[i].C, arr[i].mode = src.data_ptr(), dst.data_ptr(), 16, 1, P.FLIP_AVG
    assert _lib.load().ct_flip_merge(arr, P.FLIP_MAX_HEADS + 1, None, 0, 1, 4, 4, _lib.stream_ptr()) == _lib.CT_ERR_ARG


@pytest.mark.parametrize('name', list(P.IMG_CASE))
def test_flip_images_case_bit_for_bit(device, name):
    from centertrack_amd import _lib
    c, x = P.IMG_CASE[name], P.img_inputs(name)
    src = _lay(x, c.src, device)
    assert (c.W % 4 == 0 and src.data_ptr() % 16 == 0) == P.img_plan(c)['vec']
    flat, dst = _guarded((c.rows, c.W), device)
    _lib.check(_lib.load().ct_flip_images(src.data_ptr(), dst.data_ptr(), c.rows, c.W, _lib.stream_ptr()), 'ct_flip_images')
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_take(flat, dst, name).numpy(), x[:, ::-1])


# ---------------------------------------------------------------------------------------------------------------------
# the prior heat map

@pytest.mark.parametrize('name', list(P.PHM_CASE))
def test_render_pre_hm_case(device, name):
    from centertrack_amd import _lib
    c = P.PHM_CASE[name]
    prm = torch.from_numpy(np.array(P.phm_params(name))).to(device)
    cnt = torch.tensor(c.counts, dtype=torch.int32).to(device)
    flat, out = _guarded((c.B * (2 if c.flipped else 1), 1, c.H, c.W), device)
    _lib.check(_lib.load().ct_render_pre_hm(prm.data_ptr(), cnt.data_ptr(), c.cap, c.B, c.H, c.W, out.data_ptr(), c.flipped, _lib.stream_ptr()), 'ct_render_pre_hm')
    torch.cuda.synchronize()
    got = _take(flat, out, name).numpy()
    assert not np.isnan(got).any() and (got >= 0).all(), name
    worst, differ, touched = P.phm_compare(name, got)
    print('FRAMEOPS %-22s pre_hm   worst %d ulp, %d of %d touched pixels not bit-equal (%.2e)' % (name, worst, differ, touched, differ / max(touched, 1)))
    assert worst <= 1, name
    assert differ < 1e-3 * touched or differ == 0, (name, differ, touched)
    if c.flipped:
        np.testing.assert_array_equal(got[c.B:], got[:c.B, :, :, ::-1])


# ---------------------------------------------------------------------------------------------------------------------
# the pose match

def _sliced(t, device):
    B, ch, h, w = t.shape
    wide = torch.full((B, ch + 3, h, w), NAN, device=device)
    wide[:, 2:2 + ch] = t.to(device)
    return wide[:, 2:2 + ch]


@pytest.mark.parametrize('name', list(P.POSE_CASE))
def test_pose_case_against_the_oracle(device, name):
    from centertrack_amd import _lib, ops
    c, want = P.POSE_CASE[name], P.pose_want(name)
    maps = {k: torch.from_numpy(np.array(v)) for k, v in P.pose_maps(name).items()}
    dev = {k: (_sliced(v, device) if c.sliced and k not in ('hm', 'hm_hp') else v.to(device)) for k, v in maps.items()}
    dec = ops.Decoder(dev['hm'], {k: v for k, v in dev.items() if k != 'hm'}, c.K)
    pd, J = dec.pose, c.J
    keys = P.pose_keys(c)
    for key, fld in (('stride:hps', 'hps'), ('stride:hp_offset', 'hp_offset'), ('stride:box_wh', 'box_wh'), ('stride:box_reg', 'box_reg'), ('stride:box_ltrb', 'box_ltrb')):
        if key in keys:                                      # the descriptor is what the table says it is
            dense = {'hps': 2 * J, 'hp_offset': 2, 'box_wh': 2, 'box_reg': 2, 'box_ltrb': 4}[fld] * P.POSE_HW[0] * P.POSE_HW[1]
            assert getattr(pd, fld) and getattr(pd, fld + '_batch_stride') > dense, key
    assert (pd.box_col >= 0) == ('box:row' in keys) and bool(pd.box_ltrb) == ('box:ltrb' in keys) and bool(pd.box_reg) == ('box:wh+reg' in keys)
    got = dec.unpack(dec.run().cpu().numpy())
    np.testing.assert_array_equal(dec.inds.cpu().numpy(), want['inds'])
    for k in ('scores', 'clses', 'xs', 'ys', 'hps') + (('bboxes',) if 'bboxes' in want else ()):
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s.%s' % (name, k))
    np.testing.assert_allclose(got['kps_score'], want['kps_score'], rtol=1e-5, atol=1e-7)
    if c.designed:
        for j, (xy, why) in P.POSE_WANT.items():
            np.testing.assert_array_equal(got['hps'][0, 0, 2 * j:2 * j + 2], np.array(xy, np.float32), err_msg=why)
    # the same into a caller's buffer of out_stride = 2 J + 4: the three trailing columns are not touched
    wide = type(pd).from_buffer_copy(pd)
    flat, out = _guarded((c.B, c.K, 2 * J + 4), device)
    wide.out, wide.out_stride = out.data_ptr(), 2 * J + 4
    _lib.check(_lib.load().ct_decode_pose(ctypes.byref(wide), _lib.stream_ptr()), 'ct_decode_pose')
    torch.cuda.synchronize()
    o = _take(flat, out, name + ' out_stride').numpy()
    assert np.isnan(o[..., 2 * J + 1:]).all(), 'wrote past column 2 J of a wider row'
    np.testing.assert_array_equal(o[..., :2 * J], got['hps'])
    np.testing.assert_array_equal(o[..., 2 * J], got['kps_score'])
