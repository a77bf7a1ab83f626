"""CPU: video frames as decoders deliver them -- the numpy statement of the colour conversion against this
file's own copy of the formula and of the ten integers, the frame layout with pitches and offsets, the ctypes descriptors against
the header, the argument refusals of ct_preprocess_frames (no device needed: everything is checked before anything is enqueued),
the staging decision, and the mutations of the reference conversion."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from centertrack_amd import _lib
from centertrack_amd import frames as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

# this file's own copy: (CY, CUB, CUG, CVG, CVR), 20 fractional bits
COEF = {'bt601': (1220542, 2116026, -409993, -852492, 1673527),
        'bt709': (1220542, 2214593, -223347, -558891, 1880097)}
MATS = ('bt601', 'bt709')


def sat8(v):
    return max(0, min(255, v))


def pixel(Y, U, V, matrix, floor16=True, rnd=1 << 19):
    """(B, G, R) of one sample in Python integers (>> on a negative int is an arithmetic shift)"""
    cy, cub, cug, cvg, cvr = COEF[matrix]
    y = (max(0, Y - 16) if floor16 else Y - 16) * cy
    u, v = U - 128, V - 128
    return (sat8((y + cub * u + rnd) >> 20), sat8((y + cug * u + cvg * v + rnd) >> 20), sat8((y + cvr * v + rnd) >> 20))


def convert(Y, U, V, matrix, swap=False, full_res_chroma=False, floor16=True, rnd=1 << 19):
    """the reference conversion on a Y plane [h,w] and chroma planes [h/2,w/2], pixel by pixel, with its mutations"""
    h, w = Y.shape
    out = np.zeros((h, w, 3), np.uint8)
    if swap:
        U, V = V, U
    for y in range(h):
        for x in range(w):
            cy_, cx_ = (min(y, U.shape[0] - 1), min(x, U.shape[1] - 1)) if full_res_chroma else (y >> 1, x >> 1)
            out[y, x] = pixel(int(Y[y, x]), int(U[cy_, cx_]), int(V[cy_, cx_]), matrix, floor16, rnd)
    return out


def pack_nv12(Y, U, V):
    h, w = Y.shape
    buf = np.zeros((h * 3 // 2, w), np.uint8)
    buf[:h] = Y
    buf[h:, 0::2], buf[h:, 1::2] = U, V
    return buf


def pack_i420(Y, U, V):
    h, w = Y.shape
    return np.concatenate((Y.reshape(-1), U.reshape(-1), V.reshape(-1))).reshape(h * 3 // 2, w)


def flat(Y, U, V):
    """a 2 x 2 frame of one (Y, U, V) sample"""
    return np.full((2, 2), Y, np.uint8), np.full((1, 1), U, np.uint8), np.full((1, 1), V, np.uint8)


def block_frame():
    """4 x 6: every 2 x 2 block has its own chroma, U and V differ everywhere, Y varies inside a block"""
    Y = (np.arange(24, dtype=np.int64).reshape(4, 6) * 9 + 2).astype(np.uint8)           # (2 .. 209: some below the floor of 16)
    U = np.array([[40, 90, 200], [128, 250, 16]], np.uint8)
    V = np.array([[220, 60, 100], [30, 128, 240]], np.uint8)
    return Y, U, V


# name -> (planes, expected B, G, R of pixel (0, 0) under bt601 or None)
KNOWN = {
    'black': (flat(16, 128, 128), (0, 0, 0)),
    'white': (flat(235, 128, 128), (255, 255, 255)),
    'y0': (flat(0, 128, 128), (0, 0, 0)),                   # below the floor: max(0, Y - 16)
    'y255': (flat(255, 128, 128), (255, 255, 255)),         # saturates at the top
    'y0_blue': (flat(0, 240, 128), None),                   # below the floor with a chroma term that shows it
    'red_sat': (flat(81, 90, 240), None),
    'cyan_sat': (flat(145, 54, 34), None),
    'blocks': (block_frame(), None),
}


def both(planes, matrix):
    Y, U, V = planes
    return (F.nv12_to_bgr(F.VideoFrame(pack_nv12(Y, U, V), 'nv12', matrix=matrix)),
            F.i420_to_bgr(F.VideoFrame(pack_i420(Y, U, V), 'i420', matrix=matrix)))


def test_the_integers_are_the_issues():
    assert F.MATRICES['bt601'] == COEF['bt601']
    assert F.MATRICES['bt709'] == COEF['bt709'] == tuple(int(round(c * 2 ** 20)) for c in (1.164, 2.112, -0.213, -0.533, 1.793))


@pytest.mark.parametrize('matrix', MATS)
@pytest.mark.parametrize('name', list(KNOWN))
def test_known_answers(name, matrix):
    planes, want00 = KNOWN[name]
    want = convert(*planes, matrix)
    nv, i4 = both(planes, matrix)
    np.testing.assert_array_equal(nv, want)
    np.testing.assert_array_equal(i4, want)
    if want00 is not None:                                  # (grey samples: the chroma terms vanish under both matrices)
        assert tuple(want[0, 0]) == want00


def test_single_channels_saturate_where_the_issue_says():
    """BT.601 red and cyan: channels that leave [0, 255] by ONE before the saturation, beside channels that stay inside"""
    def raw(Y, U, V, matrix):
        cy, cub, cug, cvg, cvr = COEF[matrix]
        y, u, v = (Y - 16) * cy + (1 << 19), U - 128, V - 128
        return ((y + cub * u) >> 20, (y + cug * u + cvg * v) >> 20, (y + cvr * v) >> 20)
    assert raw(81, 90, 240, 'bt601') == (-1, -1, 254) and pixel(81, 90, 240, 'bt601') == (0, 0, 254)
    assert raw(145, 54, 34, 'bt601') == (1, 256, 0) and pixel(145, 54, 34, 'bt601') == (1, 255, 0)
    assert raw(81, 90, 240, 'bt709') == (-5, 24, 276) and pixel(81, 90, 240, 'bt709') == (0, 24, 255)
    assert raw(145, 54, 34, 'bt709') == (-6, 216, -18) and pixel(145, 54, 34, 'bt709') == (0, 216, 0)
    assert tuple(convert(*KNOWN['red_sat'][0], 'bt601')[0, 0]) == (0, 0, 254)


def test_nv12_against_i420_plane_order():
    """the same bytes read as the other format give another picture: U / V order and interleaving are pinned"""
    Y, U, V = block_frame()
    want = convert(Y, U, V, 'bt601')
    assert not np.array_equal(F.nv12_to_bgr(pack_nv12(Y, V, U)), want)
    assert not np.array_equal(F.i420_to_bgr(pack_nv12(Y, U, V)), want)
    np.testing.assert_array_equal(F.nv12_to_bgr(pack_nv12(Y, U, V)), want)      # (plain arrays are taken tightly packed)


def _padded_nv12(h, w, ypitch, uvoff, uvpitch, seed):
    rs = np.random.RandomState(seed)
    tight = rs.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    buf = rs.randint(0, 256, uvoff + (h // 2) * uvpitch).astype(np.uint8)       # (padding holds garbage)
    for y in range(h):
        buf[y * ypitch:y * ypitch + w] = tight[y]
    for y in range(h // 2):
        buf[uvoff + y * uvpitch:uvoff + y * uvpitch + w] = tight[h + y]
    return tight, buf


def test_frame_layout_with_pitches_and_offsets():
    h, w = 70, 126
    uvoff = -(-(h * 128) // 256) * 256
    tight, buf = _padded_nv12(h, w, 128, uvoff, 128, 3)
    assert uvoff % 256 == 0 and uvoff >= h * 128
    padded = F.VideoFrame(buf, 'nv12', height=h, width=w, pitches=(128, 128), offsets=(0, uvoff))
    packed = F.VideoFrame(tight, 'nv12')
    assert (packed.height, packed.width, packed.pitches, packed.offsets) == (h, w, (w, w), (0, h * w))
    np.testing.assert_array_equal(F.nv12_to_bgr(padded), F.nv12_to_bgr(packed))
    # I420 with padded chroma planes
    rs = np.random.RandomState(4)
    t420 = rs.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    flat_ = t420.reshape(-1)
    Y, U, V = flat_[:h * w].reshape(h, w), flat_[h * w:h * w * 5 // 4].reshape(h // 2, w // 2), flat_[h * w * 5 // 4:].reshape(h // 2, w // 2)
    offs = (0, uvoff, uvoff + 64 * (h // 2))
    buf = np.zeros(offs[2] + 64 * (h // 2), np.uint8)
    for plane, off, pitch in ((Y, offs[0], 128), (U, offs[1], 64), (V, offs[2], 64)):
        for y in range(plane.shape[0]):
            buf[off + y * pitch:off + y * pitch + plane.shape[1]] = plane[y]
    np.testing.assert_array_equal(F.i420_to_bgr(F.VideoFrame(buf, 'i420', height=h, width=w, pitches=(128, 64, 64), offsets=offs)),
                                  F.i420_to_bgr(F.VideoFrame(t420, 'i420')))
    for bad in (dict(pitches=(125, 128), offsets=(0, uvoff)), dict(pitches=(128, 128), offsets=(0, buf.size))):
        with pytest.raises(_lib.CTError):
            F.VideoFrame(buf, 'nv12', height=h, width=w, **bad)
    with pytest.raises(_lib.CTError):
        F.VideoFrame(np.zeros((9, 5), np.uint8), 'nv12')                        # odd width


def test_ctypes_descriptors_match_the_header_layout(tmp_path):
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    checks = {'ct_frame_desc': (_lib.FrameDesc, ['plane', 'pitch', 'format', 'h', 'w', 'coef', 'reserved', 'M', 'out', 'out_flip']),
              'ct_frames_desc': (_lib.FramesDesc, ['staging_host', 'staging_dev', 'n', 'dst_w', 'dst_h', 'lut'])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {']
    for cname, (_, fields) in checks.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for name in ('CT_PIX_BGR24', 'CT_PIX_RGB24', 'CT_PIX_NV12', 'CT_PIX_I420', 'CT_FRAMES_MAX'):
        lines.append('printf("%s %%d\\n", %s);' % (name, name))
    lines += ['return 0; }']
    src = tmp_path / 'lay.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, (cls, fields) in checks.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in fields:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    for name in ('CT_PIX_BGR24', 'CT_PIX_RGB24', 'CT_PIX_NV12', 'CT_PIX_I420', 'CT_FRAMES_MAX'):
        assert int(got[name]) == getattr(_lib, name)
    assert F.FORMATS == dict(bgr24=0, rgb24=1, nv12=2, i420=3)


def _good_call(fmt=_lib.CT_PIX_NV12, h=4, w=6):
    """a call that passes every check, built on host memory: it is refused (or not) before any pointer is followed on a device"""
    keep = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(keep)
    arr = (_lib.FrameDesc * 2)()
    for d in arr:
        d.plane[0], d.plane[1], d.plane[2] = p, p + 1024, p + 2048
        d.pitch[0], d.pitch[1], d.pitch[2] = (3 * w if fmt in (_lib.CT_PIX_BGR24, _lib.CT_PIX_RGB24) else w), w, w // 2
        d.format, d.h, d.w = fmt, h, w
        d.coef[:] = COEF['bt601']
        d.M[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        d.out = p + 3072
    a = _lib.FramesDesc()
    a.staging_host, a.staging_dev = ctypes.addressof(arr), p
    a.n, a.dst_w, a.dst_h, a.lut = 1, 8, 8, p
    return a, arr, keep


REFUSALS = [
    ('odd w', lambda a, d: setattr(d, 'w', 5), b'even'),
    ('odd h', lambda a, d: setattr(d, 'h', 3), b'even'),
    ('pitch too small', lambda a, d: d.pitch.__setitem__(0, 5), b'pitch'),
    ('chroma pitch too small', lambda a, d: d.pitch.__setitem__(1, 5), b'pitch'),
    ('null plane', lambda a, d: d.plane.__setitem__(1, None), b'null plane'),
    ('unknown format', lambda a, d: setattr(d, 'format', 4), b'format 4'),
    ('n < 1', lambda a, d: setattr(a, 'n', 0), b' 0 frames'),
    ('n too large', lambda a, d: setattr(a, 'n', _lib.CT_FRAMES_MAX + 1), b' 1025 frames'),
    ('null output', lambda a, d: setattr(d, 'out', None), b'null output'),
    ('null staging', lambda a, d: setattr(a, 'staging_dev', None), b'null pointer'),
    ('output size', lambda a, d: setattr(a, 'dst_w', 0), b'output'),
    ('matrix', lambda a, d: d.M.__setitem__(2, float('nan')), b'finite'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_argument_refusals_without_a_device(case):
    lib = _lib.load()
    _, mutate, word = case
    a, arr, keep = _good_call()
    mutate(a, arr[0])
    assert lib.ct_preprocess_frames(ctypes.byref(a), None) == _lib.CT_ERR_ARG
    assert word in lib.ct_last_error(), lib.ct_last_error()
    assert lib.ct_preprocess_frames(None, None) == _lib.CT_ERR_ARG


def test_refusals_name_the_frame_and_i420_needs_its_third_plane():
    lib = _lib.load()
    a, arr, keep = _good_call()
    a.n = 2
    arr[1].w = 7                                            # the SECOND frame is the odd one
    assert lib.ct_preprocess_frames(ctypes.byref(a), None) == _lib.CT_ERR_ARG and b'frame 1' in lib.ct_last_error()
    a, arr, keep = _good_call(_lib.CT_PIX_I420)
    arr[0].plane[2] = None
    assert lib.ct_preprocess_frames(ctypes.byref(a), None) == _lib.CT_ERR_ARG and b'null plane 2' in lib.ct_last_error()
    a, arr, keep = _good_call(_lib.CT_PIX_I420)
    arr[0].pitch[2] = 2
    assert lib.ct_preprocess_frames(ctypes.byref(a), None) == _lib.CT_ERR_ARG and b'plane 2' in lib.ct_last_error()
    a, arr, keep = _good_call(_lib.CT_PIX_BGR24, h=3, w=5)   # packed frames may be odd; their row is 3 w bytes
    arr[0].pitch[0] = 14
    assert lib.ct_preprocess_frames(ctypes.byref(a), None) == _lib.CT_ERR_ARG and b'pitch' in lib.ct_last_error()


def test_staging_decision():
    from centertrack_amd.detector import RAW_STAGED, RAW_UPLOAD, _raw_frame_source
    a, b, c = (F.VideoFrame(np.zeros((2, 2, 3), np.uint8)) for _ in range(3))
    staged = F.StagedFrames([a, b], 1, [0, 0], None, [None, None], 0)
    assert _raw_frame_source([a, b], staged, 1) == RAW_STAGED
    assert _raw_frame_source([a, b], staged, 2) == RAW_UPLOAD                  # another slot
    assert _raw_frame_source([a, c], staged, 1) == RAW_UPLOAD                  # one element replaced (an equal frame, another object)
    assert _raw_frame_source([b, a], staged, 1) == RAW_UPLOAD
    assert _raw_frame_source([a], staged, 1) == RAW_UPLOAD                     # length mismatch
    assert _raw_frame_source([a, b, c], staged, 1) == RAW_UPLOAD
    assert _raw_frame_source([a, b], None, 1) == RAW_UPLOAD                    # nothing staged


MUTATIONS = {
    'U and V swapped': dict(swap=True),
    'chroma at (x, y)': dict(full_res_chroma=True),
    'no max(0, Y - 16)': dict(floor16=False),
    'rounding constant 0': dict(rnd=0),
}


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_mutation_changes_a_known_answer(name):
    changed = [k for k, (planes, _) in KNOWN.items() for m in MATS
               if not np.array_equal(convert(*planes, m, **MUTATIONS[name]), convert(*planes, m))]
    print('%s changes %s' % (name, sorted(set(changed))))
    assert changed
