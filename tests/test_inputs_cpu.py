"""CPU: ``InputBuilder`` (centertrack_amd/inputs.py) against the reference's own images
(tests/golden/inputs.npz): ``reference(encode(...))`` bit for bit, the draws and the two streams, the row range of
``encode``, pickling, refusals, and the argument checks of ct_build_inputs on fake pointers."""
import ctypes
import pickle
import random

import numpy as np
import pytest

import _inputs as I
from centertrack_amd import _lib
from centertrack_amd._lib import CTError
from centertrack_amd.inputs import InputBuilder, source_rows
from oracle.image import warp_affine_u8


@pytest.fixture(scope='module')
def gold():
    return I.golden()


def _samples(gold):
    for c in I.CASES:
        case = gold.cases[c]
        ib = gold.builder(case['cfg'])
        for i, s in enumerate(case['samples']):
            yield c, i, ib, s


def test_golden_file_holds_what_the_issue_asks_for(gold):
    a = gold.cases['A']
    assert len(a['samples']) == 6 and a['cfg']['tracking']
    assert {s['flipped'] for s in a['samples']} == {0, 1}
    assert len({tuple(c['order'].tolist()) for s in a['samples'] for c in s['calls']}) == 6
    assert all(s['pre_img'] is not None and len(s['trans']) == 4 for s in a['samples'])
    b = gold.cases['B']['samples']
    assert {int(np.sign(s['trans'][0][0, 1])) for s in b} == {-1, 1}                # rotated, either sign
    c = gold.cases['C']['samples'][0]
    assert (c['h'], c['w']) == (20, 28) and tuple(gold.cases['C']['cfg']['input_hw']) == (32, 48)
    assert all('order' not in call for s in gold.cases['D']['samples'] for call in s['calls'])
    assert max(max(g['cfg']['input_hw']) for g in gold.cases.values()) <= 48


def test_reference_of_encode_equals_the_golden_images_bit_for_bit(gold):
    n = 0
    for c, i, ib, s in _samples(gold):
        img, pre = gold.encode(ib, s)
        got = ib.reference(img)
        assert got.dtype == np.float32 and got.shape == s['image'].shape
        assert got.tobytes() == s['image'].tobytes(), (c, i, 'image', float(np.abs(got - s['image']).max()))
        if pre is not None:
            got = ib.reference(pre)
            assert got.tobytes() == s['pre_img'].tobytes(), (c, i, 'pre_img', float(np.abs(got - s['pre_img']).max()))
        n += 1
    assert n == 11


def test_draw_color_consumes_both_streams_like_color_aug(gold):
    for c, i, ib, s in _samples(gold):
        rng, py = gold.streams(s)
        for j, call in enumerate(s['calls']):
            st = rng.get_state()
            assert st[2] == int(call['rng_pos'][0]) and [st[3], st[4]] == call['rng_gauss'][:2].tolist(), (c, i, j)
            if 'order' in call:
                rec = ib.draw_color(rng, py)
                assert rec['order'].tolist() == call['order'].tolist(), (c, i, j)
                assert rec['alpha'].tobytes() == call['alpha'].tobytes(), (c, i, j)
                assert rec['light'].dtype == np.float64 and rec['light'].tobytes() == call['light'].tobytes(), (c, i, j)
            else:
                assert I.builder((ib.H, ib.W), no_color_aug=True).draw_color(rng, py) is None
            st = rng.get_state()
            assert st[2] == int(call['rng_pos'][1]) and [st[3], st[4]] == call['rng_gauss'][2:].tolist(), (c, i, j)
            assert I.next_of(rng) == call['rng_next'].reshape(-1)[0] and I.py_next_of(py) == call['py_next'].reshape(-1)[0], (c, i, j)


def test_a_recorded_colour_record_round_trips_and_none_means_no_augmentation(gold):
    s = gold.cases['A']['samples'][0]
    ib = gold.builder(gold.cases['A']['cfg'])
    img, _ = gold.encode(ib, s)
    plain = ib.reference(dict(img, color=None))
    assert plain.tobytes() != ib.reference(img).tobytes()
    warped = ib.warped_reference(img)
    want = ((warped.astype(np.float32) / np.float32(255.) - ib.mean) / ib.std).transpose(2, 0, 1)
    assert plain.tobytes() == np.ascontiguousarray(want).tobytes()


def _crop_equals_whole(ib, frame, trans, flipped):
    rec = ib.encode(frame, trans, flipped)
    whole = warp_affine_u8(frame[:, ::-1] if flipped else frame, trans, ib.W, ib.H)
    assert ib.warped_reference(rec).tobytes() == whole.tobytes()
    row0, nrows = rec['row0'], rec['rows'].shape[0]
    assert (row0, nrows) == source_rows(trans, frame.shape[0], ib.W, ib.H)
    # the range is tight up to the rounding of the corners: dropping its first or last row changes the warp somewhere,
    # unless that row only ever meets a zero weight
    return nrows, frame.shape[0]


def test_encode_row_range_on_every_golden_sample(gold):
    for c, i, ib, s in _samples(gold):
        t = s['trans']
        _crop_equals_whole(ib, I.source(s['seed'], s['h'], s['w']), t[0], bool(s['flipped']))
        if s['pre_img'] is not None:
            _crop_equals_whole(ib, I.source(s['pre_seed'], s['h'], s['w']), t[2], bool(s['flipped']))


def test_encode_row_range_on_a_sweep_of_scale_rotation_and_flip():
    ib = I.builder((40, 56))
    frame = I.source(7, 90, 70)
    saved = 0
    for aug_s in (0.6, 0.7, 0.85, 1.0, 1.15, 1.3):
        for rot in (0, -30, 17, 45, 90):
            for flipped in (False, True):
                for c in ((35., 45.), (10., 80.), (66., 5.)):
                    nrows, h = _crop_equals_whole(ib, frame, I.get_affine(c, 90 * aug_s, rot, (56, 40)), flipped)
                    saved += nrows < h
    assert saved > 20                                       # the crop does leave rows out


def test_what_a_crop_at_aug_s_06_uploads_of_a_1080p_frame():
    ib = I.builder((512, 512))
    t = I.get_affine((960., 540.), 1920 * 0.6, 0, (512, 512))
    row0, nrows = source_rows(t, 1080, 512, 512)
    # 0.6 * 1920 = 1152 source rows and columns map onto the 512 x 512 output: all 1080 rows are in reach in y, so the
    # saving of this configuration comes from a wide frame only when the crop is shorter than the frame
    assert (row0, nrows) == (0, 1080)
    t = I.get_affine((960., 540.), 1920 * 0.6, 0, (960, 544))
    row0, nrows = source_rows(t, 1080, 960, 544)
    assert 0.55 * 1080 < nrows < 0.65 * 1080 and row0 > 0


def test_records_pickle(gold):
    s = gold.cases['A']['samples'][1]
    ib = gold.builder(gold.cases['A']['cfg'])
    img, pre = gold.encode(ib, s)
    for rec in (img, pre):
        back = pickle.loads(pickle.dumps(rec))
        assert ib.reference(back).tobytes() == ib.reference(rec).tobytes()
        assert back['rows'].tobytes() == rec['rows'].tobytes() and back['flipped'] == rec['flipped']
    pickle.loads(pickle.dumps(ib.draw_color(np.random.RandomState(1), random.Random(1))))


def test_encode_and_render_refuse_bad_input(gold):
    ib = I.builder((16, 24))
    frame = I.source(3, 40, 56)
    t = I.get_affine((28., 20.), 56., 0, (24, 16))
    good = ib.encode(frame, t)
    with pytest.raises(CTError, match='uint8'):
        ib.encode(frame.astype(np.float32), t)
    with pytest.raises(CTError, match='uint8'):
        ib.encode(frame[:, :, :2], t)
    with pytest.raises(CTError, match=r'\[2, 3\]'):
        ib.encode(frame, np.eye(3))
    with pytest.raises(CTError, match='singular'):
        ib.encode(frame, np.array([[1., 2., 0.], [2., 4., 0.]]))
    with pytest.raises(CTError, match='not finite'):
        ib.encode(frame, np.array([[1., np.nan, 0.], [0., 1., 0.]]))
    with pytest.raises(CTError, match='fixed-point'):
        ib.encode(frame, np.array([[1e-9, 0., 0.], [0., 1e-9, 0.]]))
    with pytest.raises(CTError, match='permutation'):
        ib.encode(frame, t, color={'order': [0, 0, 2], 'alpha': [1., 1., 1.], 'light': [0., 0., 0.]})
    with pytest.raises(CTError, match='colour record'):
        ib.encode(frame, t, color={'order': [0, 1, 2]})
    # render refuses before it touches a device: none of these needs one
    with pytest.raises(CTError, match='empty batch'):
        ib.render([])
    with pytest.raises(CTError, match='disagree with the frame'):
        ib.render([(dict(good, row0=good['h']), None)])
    with pytest.raises(CTError, match='disagrees with its matrix'):
        ib.render([(dict(good, rows=good['rows'][2:], row0=good['row0'] + 2), None)])
    with pytest.raises(CTError, match='uint8'):
        ib.render([(dict(good, rows=good['rows'].astype(np.int16)), None)])
    with pytest.raises(CTError, match='not a record'):
        ib.render([({'rows': good['rows']}, None)])
    with pytest.raises(CTError, match='no image record'):
        ib.render([(None, good)])
    with pytest.raises(CTError, match='singular'):
        ib.render([(dict(good, trans=np.zeros((2, 3))), None)])
    with pytest.raises(CTError, match='no CPU fallback'):
        ib.render([(good, None)], device='cpu')
    with pytest.raises(CTError, match='float32 triples'):
        InputBuilder(I.make_opt((16, 24)), [0.4, 0.4], [0.2, 0.2, 0.2])


# ---- ct_build_inputs on fake pointers: every refusal happens on the host copy, before anything is enqueued -----------
def _desc(N=2, B=1, H=16, W=24, rows=(8, 8), w=10, h=12):
    words = N * _lib.CT_INPUTS_DESC_WORDS
    offs, total = [], words * 4
    for r in rows:
        offs.append(total)
        total += (r * 3 * w + 15) // 16 * 16
    buf = np.zeros(total // 4, np.int32)
    q = buf[:words].reshape(N, _lib.CT_INPUTS_DESC_WORDS)
    for n in range(N):
        q[n, 0], q[n, 1] = _lib.CT_INPUTS_STAGED, offs[n]
        q[n, 4:9] = h, w, 3 * w, 2, rows[n]
        q[n, 11:14] = (2, 0, 1)
        q[n].view(np.float64)[14:20] = [0.5, 0, 1, 0, 0.5, 2]
    d = _lib.InputsDesc()
    fake = 0x10000
    d.staging_host, d.staging_dev, d.bytes = buf.ctypes.data, fake, total
    d.B, d.N, d.H, d.W = B, N, H, W
    for c in range(3):
        d.mean[c], d.stdv[c] = 0.4, 0.25
    d.image, d.pre_img, d.warped, d.partials = fake, fake if N == 2 * B else None, fake, fake
    return d, buf, q


def test_ct_build_inputs_checks_its_arguments_before_anything_is_enqueued():
    lib = _lib.load()
    K = I.kernel_constants()
    assert (K['TW'], K['TH'], K['DESC']) == (_lib.CT_INPUTS_TILE_W, _lib.CT_INPUTS_TILE_H, _lib.CT_INPUTS_DESC_WORDS)
    assert lib.ct_build_inputs_partials(544, 960) == 15 * 34 == 510 and lib.ct_build_inputs_partials(512, 512) == 256
    assert lib.ct_build_inputs_partials(0, 5) == 0 and lib.ct_build_inputs_partials(1, 1) == 1

    def refused(d, word):
        assert lib.ct_build_inputs(ctypes.byref(d), None) == _lib.CT_ERR_ARG
        msg = lib.ct_last_error().decode()
        assert word in msg, (word, msg)

    assert lib.ct_build_inputs(None, None) == _lib.CT_ERR_ARG
    for field in ('staging_host', 'staging_dev', 'image', 'warped', 'partials'):
        d, buf, q = _desc()
        setattr(d, field, None)
        refused(d, 'null')
    d, buf, q = _desc()
    d.pre_img = None
    refused(d, 'pre_img')
    for field, v in (('B', 0), ('H', 0), ('W', -1), ('N', 3)):
        d, buf, q = _desc()
        setattr(d, field, v)
        refused(d, 'bad sizes')
    d, buf, q = _desc()
    d.bytes = 2 * _lib.CT_INPUTS_DESC_WORDS * 4 - 4
    refused(d, 'descriptors alone')
    d, buf, q = _desc()
    d.stdv[1] = 0.0
    refused(d, 'std')
    edits = [((0, 0), 7, 'kind'), ((1, 4), 0, 'source of'), ((0, 5), -3, 'source of'), ((0, 6), 29, 'stride'),
             ((1, 7), -1, 'outside the image'), ((0, 8), 11, 'outside the image'), ((1, 7), 12, 'outside the image'),
             ((0, 1), 8, 'beyond the buffer'), ((1, 1), 1 << 30, 'beyond the buffer'), ((0, 9), 2, '0 or 1'),
             ((0, 10), -1, '0 or 1'), ((1, 12), 2, 'permutation'), ((0, 13), 3, 'permutation')]
    for (n, k), v, word in edits:
        d, buf, q = _desc()
        q[n, k] = v
        refused(d, word)
    d, buf, q = _desc()
    q[1, 6] = 3 * 10 + 40                                       # a pitch the staged block does not hold
    refused(d, 'beyond the buffer')
    d, buf, q = _desc()
    q[0, 0], q[0, 2], q[0, 3] = _lib.CT_INPUTS_DEVICE, 0, 0
    refused(d, 'null pointer')
    for k, v, word in ((14, np.inf, 'not finite'), (19, np.nan, 'not finite')):
        d, buf, q = _desc()
        q[1].view(np.float64)[k] = v
        refused(d, word)
    d, buf, q = _desc()
    q[0].view(np.float64)[14:20] = [1, 2, 0, 2, 4, 0]
    refused(d, 'singular')
    # a rejected call leaves the staging buffer as it was (the matrices are inverted only after every check passed)
    d, buf, q = _desc()
    q[1, 9] = 5
    before = buf.copy()
    refused(d, '0 or 1')
    assert (buf == before).all()


def test_ctypes_descriptor_matches_the_header_layout(tmp_path):
    """``_lib.InputsDesc`` has the size and the field offsets a C compiler gives ``ct_inputs_desc``"""
    import os
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [f[0] for f in _lib.InputsDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ct_inputs_desc));']
    lines += ['printf("%s %%zu\\n", offsetof(ct_inputs_desc, %s));' % (f, f) for f in fields]
    lines += ['return 0; }']
    src, exe = tmp_path / 'lay.c', tmp_path / 'lay'
    src.write_text('\n'.join(lines))
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(I.ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.InputsDesc)
    for f in fields:
        assert int(got[f]) == getattr(_lib.InputsDesc, f).offset, f
