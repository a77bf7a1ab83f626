"""Training images on the device: ``image`` / ``pre_img`` of a batch from raw u8 frames.

The reference makes the image side of a sample in its DataLoader workers (``GenericDataset._get_input``,
src/lib/dataset/generic_dataset.py:317-327): ``cv2.warpAffine``, ``astype(float32) / 255.``, ``color_aug``
(src/lib/utils/image.py:211-243), ``(inp - mean) / std``, transpose -- twice with ``opt.tracking`` -- then collate and
``.to(device)`` of float32.  ``InputBuilder`` splits that work the way ``TargetBuilder`` splits the targets:

* ``draw_color`` (host): the random numbers of one ``color_aug`` call, drawn from the two streams in the reference's
  order, as a small record; a recorded one may be passed instead (as ``noise`` is to ``TargetBuilder.encode``).
* ``encode`` (host, per image, in a worker): picks the source ROWS the warp can read and yields a *record*: a picklable
  dict.  The frame is passed as loaded -- the flip is a flag, not a copy.
* ``render`` (device, per batch): packs descriptors and rows into pinned staging memory, uploads them with one
  asynchronous copy and writes ``image`` (and ``pre_img``) [B,3,H,W] float32 with the two launches of ``ct_build_inputs``
  (csrc/inputs.hip).  No host wait, no CPU fallback.
* ``reference`` (host): ``_get_input`` restated in numpy on the package's host warp.  The tests stand on it; ``render``
  never calls it.

A record holds

  ``rows``     uint8 [nrows, w, 3]  the rows ``row0 .. row0 + nrows - 1`` of the frame (numpy; or a CUDA tensor: a frame
                                    that is on the device already is used in place)
  ``h``, ``w``, ``row0``            the size of the WHOLE frame (its zero border stays where it was) and the first row
  ``trans``    float64 [2, 3]       ``trans_input``
  ``flipped``  bool
  ``color``    None (no colour augmentation: val split, ``no_color_aug``) or the record of ``draw_color``:
               ``order`` int32 [3] (0 brightness, 1 contrast, 2 saturation, as shuffled), ``alpha`` float64 [3] in call
               order, ``light`` float64 [3]

File decoding, the ``_get_aug_param`` draws and the flip of the annotations stay the caller's.
"""
import random

import numpy as np

from . import _lib
from ._lib import CTError

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
# GenericDataset._eig_val / _eig_vec (generic_dataset.py:43-50)
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352],
                    [-0.5832747, 0.00994535, -0.81221408],
                    [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
TILE_W, TILE_H = _lib.CT_INPUTS_TILE_W, _lib.CT_INPUTS_TILE_H
DESC_WORDS = _lib.CT_INPUTS_DESC_WORDS
FIXED_LIMIT = float(1 << 20)         # |source coordinate| the 10-bit fixed-point map holds in an int32


def affine_inverse(trans):
    """the dst -> src map of cv::warpAffine from ``trans`` [2,3]: OpenCV's own sequence of float64 operations
    (csrc/host_preprocess.cpp ct_affine_inverse; Python floats are float64 and never fused)"""
    M = [float(v) for v in np.asarray(trans, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1. / D if D != 0 else 0.
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def source_rows(trans, h, dst_w, dst_h):
    """(row0, nrows): the rows of an ``h``-row frame the warp to ``dst_w x dst_h`` can read.  The warp's integer source
    row of output pixel (x, y) is ``(rint((M4 y + M5) 1024) + 16 + rint(M3 x 1024)) >> 10``; both terms are monotone, so
    the extremes lie at the four corners; the second tap row widens the range by one, the image clips it."""
    M = affine_inverse(trans)
    sy = []
    for x in (0, dst_w - 1):
        bdelta = round(M[3] * x * 1024.0)
        for y in (0, dst_h - 1):
            Y0 = round((M[4] * y + M[5]) * 1024.0) + 16
            sy.append(max(-32768, min(32767, (Y0 + bdelta) >> 10)))
    lo, hi = max(min(sy), 0), min(max(sy) + 1, h - 1)
    return (lo, hi - lo + 1) if hi >= lo else (0, 0)


def _check_trans(trans, dst_w, dst_h, what):
    try:
        t = np.array(trans, np.float64)
    except (TypeError, ValueError) as e:
        raise CTError('InputBuilder: %s: trans_input is no matrix (%s)' % (what, e))
    if t.shape != (2, 3):
        raise CTError('InputBuilder: %s: trans_input must be [2, 3], got %s' % (what, t.shape))
    if not np.isfinite(t).all():
        raise CTError('InputBuilder: %s: trans_input has entries that are not finite' % what)
    if t[0, 0] * t[1, 1] - t[0, 1] * t[1, 0] == 0:
        raise CTError('InputBuilder: %s: singular matrix' % what)
    M = affine_inverse(t)
    reach = max(abs(M[0]) * dst_w + abs(M[1]) * dst_h + abs(M[2]), abs(M[3]) * dst_w + abs(M[4]) * dst_h + abs(M[5]))
    if not reach < FIXED_LIMIT:
        raise CTError('InputBuilder: %s: the map reaches source coordinate %.3g, beyond the fixed-point range' % (what, reach))
    return t


def _check_color(color, what):
    if color is None:
        return None
    try:
        order = np.asarray(color['order']).reshape(-1)
        alpha = np.asarray(color['alpha'], np.float64).reshape(-1)
        light = np.asarray(color['light'], np.float64).reshape(-1)
    except (KeyError, TypeError, ValueError, IndexError) as e:
        raise CTError('InputBuilder: %s: not a colour record of draw_color (%s)' % (what, e))
    if sorted(order.tolist()) != [0, 1, 2]:
        raise CTError('InputBuilder: %s: function order %s is no permutation of 0..2' % (what, order.tolist()))
    if alpha.shape != (3,) or light.shape != (3,) or not (np.isfinite(alpha).all() and np.isfinite(light).all()):
        raise CTError('InputBuilder: %s: colour record needs three finite alpha and three finite lighting values' % what)
    return {'order': order.astype(np.int32), 'alpha': alpha, 'light': light}


def _is_tensor(v):
    return type(v).__module__.startswith('torch') and hasattr(v, 'data_ptr')


class InputBuilder(object):
    def __init__(self, opt, mean, std, eig_val=None, eig_vec=None):
        self.opt = opt
        self.H, self.W = int(opt.input_h), int(opt.input_w)
        if self.H < 1 or self.W < 1:
            raise CTError('InputBuilder: opt.input_h and opt.input_w must be positive')
        self.no_color_aug = bool(getattr(opt, 'no_color_aug', False))
        self.mean = np.array(mean, np.float32).reshape(-1)
        self.std = np.array(std, np.float32).reshape(-1)
        if self.mean.shape != (3,) or self.std.shape != (3,) or not np.isfinite(self.mean).all() or \
                not np.isfinite(self.std).all() or (self.std == 0).any():
            raise CTError('InputBuilder: mean and std are float32 triples, std without zeros')
        self.eig_val = np.array(EIG_VAL if eig_val is None else eig_val, np.float32).reshape(3)
        self.eig_vec = np.array(EIG_VEC if eig_vec is None else eig_vec, np.float32).reshape(3, 3)
        self._ring = []
        self.last_upload_bytes = 0               # what the last render sent to the device (descriptors + source rows)

    # ------------------------------------------------------------------ host: the draws of one color_aug call
    def draw_color(self, data_rng, py_random=random):
        """The colour record of one image, consuming both streams exactly as ``color_aug`` does: ``random.shuffle`` of
        the three functions, one ``uniform(-0.4, 0.4)`` per function in shuffled order, then ``normal(scale=0.1,
        size=(3,))``.  None, and nothing drawn, with ``opt.no_color_aug`` (the reference does not call ``color_aug``)."""
        if self.no_color_aug:
            return None
        order = [BRIGHTNESS, CONTRAST, SATURATION]
        py_random.shuffle(order)
        alpha = [1. + data_rng.uniform(low=-0.4, high=0.4) for _ in order]
        light = np.dot(self.eig_vec, self.eig_val * data_rng.normal(scale=0.1, size=(3,)))
        return {'order': np.array(order, np.int32), 'alpha': np.array(alpha, np.float64),
                'light': np.asarray(light, np.float64)}

    # ------------------------------------------------------------------ host: encode
    def encode(self, img, trans_input, flipped=False, color=None):
        """The record of one image.  ``img``: the u8 HWC frame as loaded, NOT flipped by the caller (numpy; or a CUDA u8
        tensor, then the record keeps a view of it and ``render`` uploads nothing); ``trans_input``: float64 [2,3];
        ``flipped``: the reference warps ``img[:, ::-1]``; ``color``: a record of ``draw_color`` or None."""
        on_device = _is_tensor(img)
        shape = tuple(img.shape)
        dtype_ok = (str(img.dtype) == 'torch.uint8') if on_device else (isinstance(img, np.ndarray) and img.dtype == np.uint8)
        if not dtype_ok or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise CTError('InputBuilder.encode: img must be a uint8 [h, w, 3] frame, got %s %s'
                          % (getattr(img, 'dtype', type(img)), shape))
        t = _check_trans(trans_input, self.W, self.H, 'encode')
        color = _check_color(color, 'encode')
        h, w = shape[0], shape[1]
        row0, nrows = source_rows(t, h, self.W, self.H)
        rows = img[row0:row0 + nrows]
        if not on_device:
            rows = np.ascontiguousarray(rows)
        return {'rows': rows, 'h': h, 'w': w, 'row0': row0, 'trans': t, 'flipped': bool(flipped), 'color': color}

    # ------------------------------------------------------------------ records
    def _check(self, rec, what):
        """(on_device, stride, trans, color) of a record that is consistent with itself; raises otherwise"""
        try:
            rows, h, w, row0 = rec['rows'], int(rec['h']), int(rec['w']), int(rec['row0'])
            trans, flipped, color = rec['trans'], rec['flipped'], rec['color']
        except (KeyError, TypeError, ValueError) as e:
            raise CTError('InputBuilder: %s is not a record of encode (%s)' % (what, e))
        on_device = _is_tensor(rows)
        if on_device:
            ok = str(rows.dtype) == 'torch.uint8' and rows.dim() == 3
            strides = tuple(rows.stride()) if ok else ()
        else:
            ok = isinstance(rows, np.ndarray) and rows.dtype == np.uint8 and rows.ndim == 3
            strides = rows.strides if ok else ()
        if not ok:
            raise CTError('InputBuilder: %s: rows must be a uint8 [nrows, w, 3] array' % what)
        nrows = int(rows.shape[0])
        if h < 1 or w < 1 or tuple(rows.shape[1:]) != (w, 3) or row0 < 0 or row0 + nrows > h:
            raise CTError('InputBuilder: %s: rows %s at row %d disagree with the frame of %d x %d' %
                          (what, tuple(rows.shape), row0, h, w))
        if nrows and (strides[1] != 3 or strides[2] != 1 or strides[0] < 3 * w):
            raise CTError('InputBuilder: %s: rows must be dense pixels with a row pitch of at least 3 w (strides %s)'
                          % (what, strides))
        if flipped not in (False, True, 0, 1):
            raise CTError('InputBuilder: %s: flipped must be a bool' % what)
        t = _check_trans(trans, self.W, self.H, what)
        need0, need = source_rows(t, h, self.W, self.H)
        if need and (need0 < row0 or need0 + need > row0 + nrows):
            raise CTError('InputBuilder: %s: row range [%d, %d) disagrees with its matrix, the warp reads rows [%d, %d)'
                          % (what, row0, row0 + nrows, need0, need0 + need))
        return on_device, (int(strides[0]) if nrows else 3 * w), t, _check_color(color, what)

    # ------------------------------------------------------------------ host: the reference's _get_input from a record
    def _host_warp(self, img, trans):
        """cv2.warpAffine(img, trans, (W, H), INTER_LINEAR) through the package's host warp (ct_preprocess_image with
        mean 0 / std 1 returns float32(v / 255.), from which v is exact)"""
        import ctypes
        img = np.ascontiguousarray(img)
        out = np.empty((3, self.H, self.W), np.float32)
        t = np.ascontiguousarray(trans, np.float64)
        zero, one = np.zeros(3, np.float32), np.ones(3, np.float32)
        _lib.check(_lib.load().ct_preprocess_image(
            img.ctypes.data_as(ctypes.c_void_p), img.shape[0], img.shape[1], img.strides[0], 3,
            t.ctypes.data_as(ctypes.c_void_p), self.W, self.H, zero.ctypes.data_as(ctypes.c_void_p),
            one.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), 0), 'ct_preprocess_image')
        return np.ascontiguousarray(np.rint(out * 255.0).astype(np.uint8).transpose(1, 2, 0))

    def warped_reference(self, rec):
        """the u8 [H, W, 3] image after the warp (of the flipped frame, if the record says so), on the CPU"""
        on_device, _, t, _ = self._check(rec, 'record')
        rows = rec['rows'].cpu().numpy() if on_device else rec['rows']
        full = np.zeros((rec['h'], rec['w'], 3), np.uint8)
        full[rec['row0']:rec['row0'] + rows.shape[0]] = rows
        if rec['flipped']:
            full = full[:, ::-1]
        return self._host_warp(full, t)

    @staticmethod
    def color_aug(inp, color):
        """``color_aug`` (utils/image.py:235-243) on the float32 HWC image ``inp`` in place, with the draws of ``color``:
        numpy's float32 operations with the Python-float factors rounded to float32 once, the lighting added in float64"""
        gs = (np.float32(0.114) * inp[:, :, 0] + np.float32(0.587) * inp[:, :, 1]) + np.float32(0.299) * inp[:, :, 2]
        gs_mean = gs.mean()
        for f, alpha in zip(color['order'].tolist(), color['alpha'].tolist()):
            inp *= np.float32(alpha)
            if f == CONTRAST:
                inp += np.float32(gs_mean) * np.float32(1 - alpha)
            elif f == SATURATION:
                gs *= np.float32(1 - alpha)
                inp += gs[:, :, None]
        inp[...] = (inp.astype(np.float64) + color['light']).astype(np.float32)
        return inp

    def reference(self, rec):
        """the reference's ``_get_input`` for the record: float32 [3, H, W], on the CPU"""
        _, _, _, color = self._check(rec, 'record')
        inp = self.warped_reference(rec).astype(np.float32) / np.float32(255.)
        if color is not None:
            self.color_aug(inp, color)
        inp = (inp - self.mean.reshape(1, 1, 3)) / self.std.reshape(1, 1, 3)
        return np.ascontiguousarray(inp.transpose(2, 0, 1))

    # ------------------------------------------------------------------ device: render
    def output_specs(self, B, pre=True):
        """{name: shape} of the float32 tensors ``render`` produces for a batch of ``B``"""
        specs = {'image': (B, 3, self.H, self.W)}
        if pre:
            specs['pre_img'] = (B, 3, self.H, self.W)
        return specs

    def render(self, samples, out=None, debug=False, device=None):
        """The image tensors ``default_collate`` + ``.to(device)`` would have made of the reference's samples:
        ``{'image': [B,3,H,W] float32}`` plus ``'pre_img'`` when any sample has one (a sample without gets zeros there).
        ``samples``: a list of ``(img_record, pre_img_record or None)``.  ``out``: caller-owned tensors for exactly these
        keys (any contents; every element is written once).  ``debug``: also ``warped`` [N,H,W,3] u8 (the images after
        the warp, the ``image`` ones first, then the ``pre_img`` ones) and ``gs_mean`` [N] float32.  One pinned-to-device
        copy and two launches on the current stream, no host wait."""
        import torch
        from . import _staging, ops
        try:
            samples = [(s[0], s[1]) for s in samples]
        except (TypeError, IndexError, KeyError):
            raise CTError('InputBuilder.render: samples is a list of (img_record, pre_img_record or None)')
        B = len(samples)
        if B < 1:
            raise CTError('InputBuilder.render: empty batch')
        has_pre = any(p is not None for _, p in samples)
        recs = [s[0] for s in samples] + ([s[1] for s in samples] if has_pre else [])
        N = len(recs)
        checked = []
        for n, rec in enumerate(recs):
            if rec is None:
                if n < B:
                    raise CTError('InputBuilder.render: sample %d has no image record' % n)
                checked.append(None)
                continue
            checked.append(self._check(rec, 'sample %d %s' % (n % B, 'pre_img' if n >= B else 'image')))
        specs = self.output_specs(B, has_pre)
        on_dev = [r['rows'] for r, c in zip(recs, checked) if c is not None and c[0]]
        if out is not None:
            if sorted(out) != sorted(specs):
                raise CTError('InputBuilder.render: out must name exactly %s, got %s' % (sorted(specs), sorted(out)))
            for k, t in out.items():
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == specs[k]
                        and t.is_contiguous()):
                    raise CTError('InputBuilder.render: out[%r] must be a contiguous float32 CUDA tensor of shape %s'
                                  % (k, specs[k]))
            device = out['image'].device
            if any(t.device != device for t in out.values()):
                raise CTError('InputBuilder.render: the out tensors are on different devices')
        elif device is None:
            device = on_dev[0].device if on_dev else torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise CTError('InputBuilder.render runs on an MI355X only (device %s); no CPU fallback' % device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        for t in on_dev:
            if not t.is_cuda or t.device != device:
                raise CTError('InputBuilder.render: a device-resident source is on %s, the batch goes to %s' % (t.device, device))
        # ---- layout: N descriptors, then the staged rows, each block on a 16-byte boundary
        hdr = np.zeros((N, DESC_WORDS), np.int32)
        hdr64 = hdr.view(np.float64)                        # words 20..25: light = doubles 10..12; 28..39: trans = 14..19
        nbytes = N * DESC_WORDS * 4
        copies = []
        for n, (rec, c) in enumerate(zip(recs, checked)):
            q = hdr[n]
            if c is None:
                q[0] = _lib.CT_INPUTS_ZERO
                continue
            on_device, stride, t, color = c
            rows = rec['rows']
            nrows = int(rows.shape[0])
            q[4:9] = rec['h'], rec['w'], stride, rec['row0'], nrows
            if on_device:
                q[0] = _lib.CT_INPUTS_DEVICE
                ptr = rows.data_ptr() if nrows else 0
                q[2:4] = np.array([ptr & 0xffffffff, ptr >> 32], np.uint32).view(np.int32)
            else:
                q[0], q[1] = _lib.CT_INPUTS_STAGED, nbytes
                extent = (nrows - 1) * stride + 3 * rec['w'] if nrows else 0
                copies.append((nbytes, rows, stride))
                nbytes += (extent + 15) // 16 * 16
            q[9] = 1 if rec['flipped'] else 0
            q[11:14] = (0, 1, 2)
            if color is not None:
                q[10] = 1
                q[11:14] = color['order']
                q[14:17] = color['alpha'].astype(np.float32).view(np.int32)
                q[17:20] = (1.0 - color['alpha']).astype(np.float32).view(np.int32)   # 1 - alpha in double, rounded once
                hdr64[n, 10:13] = color['light']
            hdr64[n, 14:20] = t.reshape(6)
        if nbytes >= 1 << 31:
            raise CTError('InputBuilder.render: %d bytes of descriptors and source rows: 2 GiB or more in one batch' % nbytes)
        words = nbytes // 4
        entry = _staging.take(self._ring, words, torch.int32)
        buf = entry['host'].numpy()
        buf[:N * DESC_WORDS] = hdr.reshape(-1)
        buf8 = buf.view(np.uint8)
        for off, rows, stride in copies:
            nrows, w3 = int(rows.shape[0]), 3 * int(rows.shape[1])
            if nrows:
                dst = np.lib.stride_tricks.as_strided(buf8[off:], shape=(nrows, w3), strides=(stride, 1))
                dst[...] = np.lib.stride_tricks.as_strided(rows, shape=(nrows, w3), strides=(stride, 1))
        P = ((self.W + TILE_W - 1) // TILE_W) * ((self.H + TILE_H - 1) // TILE_H)
        with torch.cuda.device(device):
            if out is None:
                out = {k: torch.empty(shape, dtype=torch.float32, device=device) for k, shape in specs.items()}
            else:
                out = dict(out)
            dev = torch.empty(words, dtype=torch.int32, device=device)
            warped = torch.empty((N, self.H, self.W), dtype=torch.int32, device=device)
            partials = torch.empty(N * P, dtype=torch.float64, device=device)
            gs_mean = torch.empty(N, dtype=torch.float32, device=device) if debug else None
            ops.build_inputs(entry['host'], dev, nbytes, B, N, self.H, self.W, self.mean, self.std, out['image'],
                             out.get('pre_img'), warped, partials, gs_mean)
            entry['event'].record()
        self.last_upload_bytes = nbytes
        if debug:
            out['warped'] = warped.view(torch.uint8).view(N, self.H, self.W, 4)[..., :3]
            out['gs_mean'] = gs_mean
        return out
