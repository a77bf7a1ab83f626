"""GPU: video frames as decoders deliver them.  Every comparison is exact.

The kernel: ct_preprocess_frames on a YUV frame == ct_preprocess_device on the frame converted as a whole (frames.nv12_to_bgr /
i420_to_bgr, themselves pinned against an independent formula by tests/test_video_frames_cpu.py) == the oracle's pre-processing
of the converted frame, mirrored output included; BGR24 == the parent on the same bytes, RGB24 == the parent on the reversed
channels; one launch for three frames == three launches.  The streams: VideoFrames through StreamDetector.step and Detector.run
against the list-of-ndarray route, with and without prefetch, from host and device memory, B = 2 with flip_test, native loop on
and off, and a staging that goes stale."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAME_SIZES = [(2, 2), (4, 6), (38, 54), (70, 126)]          # h, w; the last with padded pitches and an offset UV plane
OUT_SIZES = [(32, 32), (32, 64), (37, 53)]                   # H, W
MATS = ('bt601', 'bt709')
_STATE = {}


def _tools(device):
    """the normalisation table on the device and one launcher, shared by the kernel tests (each launch is waited for)"""
    if 'lut' not in _STATE:
        from centertrack_amd import _lib, frames as F
        from centertrack_amd.detector import MEAN, STD
        lut = np.empty((3, 256), np.float32)
        mean, std = np.ascontiguousarray(MEAN.reshape(-1)), np.ascontiguousarray(STD.reshape(-1))
        _lib.check(_lib.load().ct_preprocess_lut(mean.ctypes.data, std.ctypes.data, 3, lut.ctypes.data), 'lut')
        _STATE['lut'] = torch.from_numpy(lut).to(device)
        _STATE['launcher'] = F.FrameLauncher(device, 4)
    return _STATE['lut'], _STATE['launcher']


def frames_launch(device, items, dh, dw):
    """ONE ct_preprocess_frames launch for ``items`` = [(host VideoFrame, trans)]: float32 [n, 2 (plain, mirrored), 3, dh, dw]"""
    lut, launcher = _tools(device)
    devs = [torch.from_numpy(f.data.reshape(-1)).to(device) for f, _ in items]
    outs = torch.full((len(items), 2, 3, dh, dw), float('nan'), device=device)
    launcher.launch([f for f, _ in items], [d.data_ptr() for d in devs], [t for _, t in items],
                    [outs[i, 0].data_ptr() for i in range(len(items))], [outs[i, 1].data_ptr() for i in range(len(items))],
                    dw, dh, lut.data_ptr())
    torch.cuda.synchronize()
    return outs.cpu().numpy()


def parent_launch(device, bgr, trans, dh, dw):
    """ct_preprocess_device on a tightly packed uint8 [h,w,3] frame: float32 [2, 3, dh, dw]"""
    from centertrack_amd import _lib
    lut, _ = _tools(device)
    bgr = np.ascontiguousarray(bgr)
    h, w, _c = bgr.shape
    dev = torch.from_numpy(bgr).to(device)
    out = torch.full((2, 3, dh, dw), float('nan'), device=device)
    tr = np.ascontiguousarray(trans, np.float64)
    _lib.check(_lib.load().ct_preprocess_device(dev.data_ptr(), h, w, w * 3, 3, tr.ctypes.data, dw, dh, lut.data_ptr(),
                                                out[0].data_ptr(), out[1].data_ptr(), _lib.stream_ptr()), 'ct_preprocess_device')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_image(bgr, trans, dh, dw):
    from centertrack_amd.detector import MEAN, STD
    from oracle import image as oimage
    return oimage.pre_process_image(np.ascontiguousarray(bgr), np.asarray(trans, np.float64).reshape(2, 3), dw, dh, MEAN, STD,
                                    flip_test=True)


def maps_for(h, w, dh, dw):
    """name -> forward 2 x 3 map (source -> output)"""
    from centertrack_amd.image import get_affine_transform
    out = {'identity': np.array([[1, 0, 0], [0, 1, 0]], np.float64),
           'letterbox': np.asarray(get_affine_transform(np.array([w / 2., h / 2.], np.float32), float(max(h, w)), 0, (dw, dh)), np.float64),
           'shift': np.array([[1, 0, -1], [0, 1, 1]], np.float64)}              # one pixel: sx = x + 1 (parity flips), sy = y - 1
    if 2.5 * h + 2 <= dh and 2.5 * w + 2 <= dw:
        # x 2.5 about the centre: the magnified frame lies inside the output, the taps leave it on all four sides
        out['crop'] = np.array([[2.5, 0, (dw - 1) / 2. - 2.5 * (w - 1) / 2.], [0, 2.5, (dh - 1) / 2. - 2.5 * (h - 1) / 2.]], np.float64)
    else:
        # the frame is larger than what the output shows at x 2.5: one crop over the top-left corner, one over the bottom-right
        out['crop'] = np.array([[2.5, 0, 4.25], [0, 2.5, 3.75]], np.float64)
        out['crop_br'] = np.array([[2.5, 0, dw - 5.25 - 2.5 * (w - 1)], [0, 2.5, dh - 4.75 - 2.5 * (h - 1)]], np.float64)
    return out


def test_the_crops_leave_the_frame_on_every_side_and_meet_both_parities():
    """what the x 2.5 maps are designed to do, from the first tap floor((x - t) / 2.5) of each output column / row"""
    for (h, w) in FRAME_SIZES:
        for (dh, dw) in OUT_SIZES:
            m = maps_for(h, w, dh, dw)
            sides = set()
            for name in [n for n in m if n.startswith('crop')]:
                sx = np.floor((np.arange(dw) - m[name][0, 2]) / 2.5).astype(int)
                sy = np.floor((np.arange(dh) - m[name][1, 2]) / 2.5).astype(int)
                sides |= {s for s, hit in (('l', sx.min() < -1), ('r', sx.max() >= w), ('t', sy.min() < -1), ('b', sy.max() >= h)) if hit}
                ins_x, ins_y = sx[(sx >= 0) & (sx < w)], sy[(sy >= 0) & (sy < h)]
                assert {int(v) & 1 for v in ins_x} == {0, 1} and {int(v) & 1 for v in ins_y} == {0, 1}, (h, w, dh, dw, name)
            assert sides == set('lrtb'), (h, w, dh, dw, sides)


def make_frames(h, w, seed):
    """random plane bytes over the full range: the same YUV samples as NV12 and as I420, packed bytes as BGR and as RGB; the 70 x 126
    frame on padded surfaces (Y pitch 128, chroma behind a 256-byte aligned offset, packed pitch 384) whose padding holds garbage"""
    from centertrack_amd import frames as F
    rs = np.random.RandomState(seed)
    Y = rs.randint(0, 256, (h, w)).astype(np.uint8)
    U = rs.randint(0, 256, (h // 2, w // 2)).astype(np.uint8)
    V = rs.randint(0, 256, (h // 2, w // 2)).astype(np.uint8)
    packed = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    UV = np.stack((U, V), axis=2).reshape(h // 2, w)
    padded = (h, w) == (70, 126)

    def surface(planes, pitches, align):
        offs, off = [], 0
        for p, pitch in zip(planes, pitches):
            off = -(-off // align) * align
            offs.append(off)
            off += p.shape[0] * pitch
        buf = rs.randint(0, 256, off).astype(np.uint8)
        for p, pitch, o in zip(planes, pitches, offs):
            for r in range(p.shape[0]):
                buf[o + r * pitch:o + r * pitch + p.shape[1]] = p[r]
        return buf, tuple(offs)

    def frame(fmt, planes, pitches, matrix='bt601'):
        if not padded:
            data = np.concatenate([p.reshape(-1) for p in planes])
            return F.VideoFrame(data.reshape(h, w, 3) if fmt in ('bgr24', 'rgb24') else data.reshape(h * 3 // 2, w), fmt, matrix=matrix)
        buf, offs = surface(planes, pitches, 256)
        return F.VideoFrame(buf, fmt, height=h, width=w, pitches=pitches, offsets=offs, matrix=matrix)

    out = {'bgr24': frame('bgr24', [packed.reshape(h, 3 * w)], (384,)), 'rgb24': frame('rgb24', [packed.reshape(h, 3 * w)], (384,))}
    for m in MATS:
        out['nv12', m] = frame('nv12', [Y, UV], (128, 128), m)
        out['i420', m] = frame('i420', [Y, U, V], (128, 64, 64), m)
    tight = F.VideoFrame(np.concatenate((Y.reshape(-1), UV.reshape(-1))).reshape(h * 3 // 2, w), 'nv12')
    return out, packed, tight


@pytest.mark.parametrize('out_size', OUT_SIZES, ids=lambda s: 'out%dx%d' % s)
@pytest.mark.parametrize('frame_size', FRAME_SIZES, ids=lambda s: 'frame%dx%d' % s)
def test_kernel_equals_the_existing_path_on_the_converted_frame(device, frame_size, out_size):
    from centertrack_amd import frames as F
    (h, w), (dh, dw) = frame_size, out_size
    fr, packed, tight = make_frames(h, w, 100 + h)
    if (h, w) == (70, 126):
        assert fr['nv12', 'bt601'].pitches == (128, 128) and fr['nv12', 'bt601'].offsets[1] % 256 == 0 and fr['bgr24'].pitches == (384,)
    conv = {m: F.nv12_to_bgr(tight, matrix=m) for m in MATS}
    for m in MATS:
        np.testing.assert_array_equal(F.nv12_to_bgr(fr['nv12', m]), conv[m])
        np.testing.assert_array_equal(F.i420_to_bgr(fr['i420', m]), conv[m])
    assert not np.array_equal(conv['bt601'], conv['bt709'])
    if h * w >= 38 * 54:
        assert conv['bt601'].min() == 0 and conv['bt601'].max() == 255          # (the saturating branches are busy)
    maps = maps_for(h, w, dh, dw)
    for name, trans in maps.items():
        want = {m: parent_launch(device, conv[m], trans, dh, dw) for m in MATS}
        want['bgr24'] = parent_launch(device, packed, trans, dh, dw)
        want['rgb24'] = parent_launch(device, packed[:, :, ::-1], trans, dh, dw)
        for key, ref in want.items():
            src = {'bgr24': packed, 'rgb24': packed[:, :, ::-1]}.get(key, conv.get(key))
            np.testing.assert_array_equal(ref, oracle_image(src, trans, dh, dw), err_msg='parent vs oracle %s %s' % (name, key))
        if name == 'crop' and 'crop_br' not in maps:
            lut = _tools(device)[0].cpu().numpy()
            for cy_, cx_ in ((0, 0), (0, dw - 1), (dh - 1, 0), (dh - 1, dw - 1)):                  # outside on all four sides: 0 in B, G, R
                np.testing.assert_array_equal(want['bt601'][0, :, cy_, cx_], lut[:, 0])
        for key in ('bgr24', 'rgb24') + tuple((f, m) for f in ('nv12', 'i420') for m in MATS):
            got = frames_launch(device, [(fr[key], trans)], dh, dw)[0]
            ref = want[key if isinstance(key, str) else key[1]]
            assert not np.isnan(got).any()
            np.testing.assert_array_equal(got, ref, err_msg='%s %s' % (name, key))
            np.testing.assert_array_equal(got[1], got[0][:, :, ::-1])


def test_one_launch_for_three_frames_equals_three_launches(device):
    dh, dw = 37, 53
    a, b, c = make_frames(38, 54, 1)[0], make_frames(4, 6, 2)[0], make_frames(70, 126, 3)[0]
    items = [(a['nv12', 'bt709'], maps_for(38, 54, dh, dw)['letterbox']), (b['i420', 'bt601'], maps_for(4, 6, dh, dw)['crop']),
             (c['rgb24'], maps_for(70, 126, dh, dw)['crop_br'])]
    together = frames_launch(device, items, dh, dw)
    assert not np.isnan(together).any()
    for i, item in enumerate(items):
        np.testing.assert_array_equal(together[i], frames_launch(device, [item], dh, dw)[0], err_msg='frame %d' % i)
    assert not np.array_equal(together[0], together[2])


def test_packed_formats_equal_the_parent(device):
    from centertrack_amd import frames as F
    rs = np.random.RandomState(8)
    bgr = rs.randint(0, 256, (45, 67, 3)).astype(np.uint8)                  # (packed frames may have odd sizes)
    for (dh, dw) in OUT_SIZES:
        for name, trans in maps_for(45, 67, dh, dw).items():
            want = parent_launch(device, bgr, trans, dh, dw)
            np.testing.assert_array_equal(frames_launch(device, [(F.VideoFrame(bgr, 'bgr24'), trans)], dh, dw)[0], want, err_msg=name)
            rgb = np.ascontiguousarray(bgr[:, :, ::-1])
            np.testing.assert_array_equal(frames_launch(device, [(F.VideoFrame(rgb, 'rgb24'), trans)], dh, dw)[0], want, err_msg=name)
            assert not np.array_equal(frames_launch(device, [(F.VideoFrame(rgb, 'bgr24'), trans)], dh, dw)[0], want)


# ---------------------------------------------------------------------------------------------------------------------
# streams

def _stream_cases():
    return ['b1', 'b2_flip', 'b1_python_loop']


def _setup(case):
    """model, options, sizes and T frames per stream: packed BGR bytes and NV12 bytes, both random over the full range"""
    import scenarios as S
    from centertrack_amd import weights as W
    from centertrack_amd.detector import default_opt
    from centertrack_amd.model import DLASegHIP
    if case == 'b2_flip':
        heads = W.KITTI_HEADS
        sd = W.make_synthetic_state_dict(heads, seed=9, hm_gain=14.0)
        opt = default_opt(heads, track_thresh=0.4, flip_test=True, input_h=64, input_w=160)
        B, H, Wd, bgr_hw, yuv_hw, T = 2, 64, 160, (375, 1242), (374, 1242), 4        # (4:2:0 needs an even height: 374 of the 375 rows)
    else:
        cfg = S.e2e_config()
        heads, sd = cfg['heads'], S.e2e_state_dict(cfg)
        opt = default_opt(heads, track_thresh=cfg['track_thresh'], pre_thresh=cfg['pre_thresh'], input_h=cfg['H'], input_w=cfg['W'])
        B, H, Wd, bgr_hw, yuv_hw, T = 1, cfg['H'], cfg['W'], (cfg['orig_h'], cfg['orig_w']), (cfg['orig_h'], cfg['orig_w']), 4
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    rs = np.random.RandomState(5)
    base_bgr = rs.randint(0, 256, (B, bgr_hw[0], bgr_hw[1] + 8 * T, 3)).astype(np.uint8)
    base_yuv = rs.randint(0, 256, (B, yuv_hw[0] * 3 // 2, yuv_hw[1] + 8 * T)).astype(np.uint8)
    bgr = [[np.ascontiguousarray(base_bgr[s][:, 8 * t:8 * t + bgr_hw[1]]) for s in range(B)] for t in range(T)]
    yuv = [[np.ascontiguousarray(base_yuv[s][:, 8 * t:8 * t + yuv_hw[1]]) for s in range(B)] for t in range(T)]
    return dict(model=model, opt=opt, B=B, H=H, W=Wd, T=T, bgr=bgr, yuv=yuv, flip=bool(opt.flip_test))


def _run_route(det, helper, T, B, feed, prefetch, check=None):
    """T steps of ``det`` from a reset: ``feed(t)`` -> (list of B frames, the arrays their metas come from).  Returns per step the
    result arrays as bytes.  ``check(t, ctx)`` is called behind every step."""
    det.reset_tracking()
    fed = [feed(t) for t in range(T)]
    out = []
    for t in range(T):
        frames, shapes = fed[t]
        metas = [helper.frame_meta(x) for x in shapes]
        nxt = fed[t + 1][0] if (prefetch and t + 1 < T) else None
        res = det.step(frames, metas, prefetch=nxt)
        out.append([np.asarray(r).tobytes() if isinstance(r, np.ndarray) else repr(r) for r in res])
        if check is not None:
            check(t, det._ctx, metas)
    return out


@pytest.mark.parametrize('case', _stream_cases())
def test_streams_of_video_frames_equal_the_ndarray_route(device, case, monkeypatch):
    from centertrack_amd import _lib, detector as D, frames as F
    if case == 'b1_python_loop':
        monkeypatch.setattr(D, 'NATIVE_LOOP', False)
    c = _setup(case)
    B, T, H, W = c['B'], c['T'], c['H'], c['W']
    det = D.StreamDetector(c['opt'], model=c['model'], num_streams=B)
    helper = D.Detector(c['opt'], model=c['model'])
    conv = [[F.nv12_to_bgr(c['yuv'][t][s]) for s in range(B)] for t in range(T)]
    oracle = {}

    def slot_check(images):
        def check(t, ctx, metas):
            got = ctx.frames[(ctx.slot - 1) % ctx.nslots].cpu().numpy()
            for s in range(B):
                key = (id(images), t, s)
                if key not in oracle:
                    oracle[key] = oracle_image(images[t][s], metas[s]['trans_input'], H, W)
                np.testing.assert_array_equal(got[s], oracle[key][0], err_msg='slot frame, step %d stream %d' % (t, s))
                if c['flip']:
                    np.testing.assert_array_equal(got[B + s], oracle[key][1], err_msg='mirrored slot frame, step %d stream %d' % (t, s))
        return check

    # the yardsticks: plain arrays through _warp_frame / ct_preprocess_device
    want_bgr = _run_route(det, helper, T, B, lambda t: (c['bgr'][t], c['bgr'][t]), False, slot_check(c['bgr']))
    want_yuv = _run_route(det, helper, T, B, lambda t: (conv[t], conv[t]), False, slot_check(conv))
    assert want_bgr != want_yuv
    assert any(len(r) > 0 for step in want_bgr + want_yuv for r in step)
    native = det._ctx.loop is not None
    assert native == (case != 'b1_python_loop')

    vf_bgr = [[F.VideoFrame(c['bgr'][t][s]) for s in range(B)] for t in range(T)]
    vf_yuv = [[F.VideoFrame(c['yuv'][t][s], 'nv12') for s in range(B)] for t in range(T)]
    vf_dev = [[F.VideoFrame(torch.from_numpy(c['yuv'][t][s]).to(device), 'nv12') for s in range(B)] for t in range(T)]
    pin = []
    for t in range(T):                                       # NV12 in pinned memory: uploaded without a host copy
        row = []
        for s in range(B):
            buf = F.pinned_frame('nv12', conv[t][s].shape[0], conv[t][s].shape[1])
            buf[...] = c['yuv'][t][s]
            row.append(F.VideoFrame(buf, 'nv12'))
        pin.append(row)
    assert pin[0][0].pinned and not vf_yuv[0][0].pinned
    for prefetch in (False, True):
        tag = 'prefetch' if prefetch else 'plain'
        assert _run_route(det, helper, T, B, lambda t: (vf_bgr[t], c['bgr'][t]), prefetch, slot_check(c['bgr'])) == want_bgr, 'bgr ' + tag
        if native:                                           # the step behind the first took the native loop, frame written in place
            assert det._ctx.args[0].frame_kind == _lib.CT_FRAME_IN_PLACE
        assert _run_route(det, helper, T, B, lambda t: (vf_yuv[t], conv[t]), prefetch, slot_check(conv)) == want_yuv, 'nv12 host ' + tag
        assert _run_route(det, helper, T, B, lambda t: (pin[t], conv[t]), prefetch, slot_check(conv)) == want_yuv, 'nv12 pinned ' + tag
        assert _run_route(det, helper, T, B, lambda t: (vf_dev[t], conv[t]), prefetch, slot_check(conv)) == want_yuv, 'nv12 device ' + tag
    if B > 1:                                                # formats and sizes mixed across the streams of a step
        mixed = [[vf_yuv[t][0]] + vf_bgr[t][1:] for t in range(T)]
        src = [[conv[t][0]] + c['bgr'][t][1:] for t in range(T)]
        want = _run_route(det, helper, T, B, lambda t: (src[t], src[t]), False, slot_check(src))
        assert _run_route(det, helper, T, B, lambda t: (mixed[t], src[t]), True, slot_check(src)) == want


def test_a_stale_staging_is_not_used(device):
    """a frame staged with ``prefetch`` and then not passed: the results and the slot are those of the frame actually passed"""
    from centertrack_amd import detector as D, frames as F
    c = _setup('b1')
    det = D.StreamDetector(c['opt'], model=c['model'], num_streams=1)
    helper = D.Detector(c['opt'], model=c['model'])
    conv = [F.nv12_to_bgr(c['yuv'][t][0]) for t in range(c['T'])]
    order = [0, 3, 2, 1]                                      # what is passed; staged ahead is frame t + 1
    want = _run_route(det, helper, 4, 1, lambda t: ([conv[order[t]]], [conv[order[t]]]), False)
    vf = [F.VideoFrame(c['yuv'][t][0], 'nv12') for t in range(c['T'])]
    det.reset_tracking()
    got = []
    for t in range(4):
        x = vf[order[t]]
        meta = helper.frame_meta(conv[order[t]])
        res = det.step([x], [meta], prefetch=[vf[(t + 1) % 4]])           # step 0 stages 1 (3 is passed: stale), step 1 stages 2
        got.append([np.asarray(r).tobytes() for r in res])                 # (2 is passed: used), step 2 stages 3 (1 is passed: stale)
        ctx = det._ctx
        np.testing.assert_array_equal(ctx.frames[(ctx.slot - 1) % ctx.nslots].cpu().numpy()[0],
                                      oracle_image(conv[order[t]], meta['trans_input'], c['H'], c['W'])[0])
    assert got == want
    # an EQUAL frame in another object is not the staged one either
    det.reset_tracking()
    det.step([vf[0]], [helper.frame_meta(conv[0])], prefetch=[vf[1]])
    twin = F.VideoFrame(c['yuv'][1][0].copy(), 'nv12')
    assert D._raw_frame_source([twin], det._staged, det._ctx.slot) == D.RAW_UPLOAD
    assert D._raw_frame_source([vf[1]], det._staged, det._ctx.slot) == D.RAW_STAGED


def test_detector_run_on_a_video_frame(device):
    from centertrack_amd import detector as D, frames as F
    c = _setup('b1')
    det, ref = D.Detector(c['opt'], model=c['model']), D.Detector(c['opt'], model=c['model'])
    seen = 0
    for t in range(3):
        yuv = c['yuv'][t][0]
        got = det.run(F.VideoFrame(yuv, 'nv12'))['results']
        want = ref.run(F.nv12_to_bgr(yuv))['results']
        seen += len(want)
        key = lambda r: (int(r['tracking_id']), int(r['class']), float(r['score'])) + tuple(map(float, r['bbox'])) + tuple(map(float, r['ct']))
        assert [key(r) for r in got] == [key(r) for r in want]
    assert seen > 0
    meta = det.frame_meta(F.VideoFrame(c['yuv'][0][0], 'nv12'))
    assert (meta['height'], meta['width']) == (F.nv12_to_bgr(c['yuv'][0][0]).shape[:2])
