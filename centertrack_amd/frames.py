"""Video frames as decoders deliver them: packed BGR / RGB and YUV 4:2:0 surfaces (NV12, I420),
in host memory or already on the device, pre-processed for all streams of a step by ONE launch of
``ct_preprocess_frames`` (csrc/frames.hip).

``VideoFrame`` describes one frame (planes, pitches, offsets, colour matrix); ``nv12_to_bgr`` / ``i420_to_bgr`` are the
numpy statement of the colour conversion the kernel applies per tap; ``pinned_frame`` hands out pinned memory a decoder
can write into, so that a frame is uploaded without a host copy; ``FrameStager`` uploads the BYTES of the next step's
frames on a copy stream while this step runs; ``FrameLauncher`` packs the descriptors and launches."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

FORMATS = {'bgr24': _lib.CT_PIX_BGR24, 'rgb24': _lib.CT_PIX_RGB24, 'nv12': _lib.CT_PIX_NV12, 'i420': _lib.CT_PIX_I420}
# (CY, CUB, CUG, CVG, CVR) with 20 fractional bits: the integers OpenCV publishes for BT.601 video range, and
# int(round(c * 2**20)) of BT.709's (1.164, 2.112, -0.213, -0.533, 1.793)
MATRICES = {'bt601': (1220542, 2116026, -409993, -852492, 1673527),
            'bt709': tuple(int(round(c * 2 ** 20)) for c in (1.164, 2.112, -0.213, -0.533, 1.793))}


def _plane_rows(fmt, h, w):
    """(rows, bytes per row) of each plane of a ``fmt`` frame of h x w pixels"""
    if fmt in ('bgr24', 'rgb24'):
        return [(h, 3 * w)]
    if fmt == 'nv12':
        return [(h, w), (h // 2, w)]
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


class VideoFrame(object):
    """One frame as a decoder delivers it.  ``data``: a C-contiguous uint8 numpy array or a torch.uint8 CUDA tensor that
    holds all planes; ``format``: 'bgr24', 'rgb24', 'nv12' or 'i420'.  Without ``pitches`` / ``offsets`` the planes are
    tightly packed and the size comes from the shape ([h,w,3] packed, [h*3//2, w] for 4:2:0); with them (bytes per row and
    byte offset of each plane, plus ``height`` / ``width``) any aligned decoder surface is described.  ``matrix``: 'bt601'
    or 'bt709' (video range).  A VideoFrame is a value: from handing it to ``step(prefetch=...)`` until the step that
    consumes it has returned, the caller does not write the buffer."""
    __slots__ = ('data', 'format', 'height', 'width', 'pitches', 'offsets', 'matrix', 'on_device', 'nbytes', '_pinned')

    def __init__(self, data, format='bgr24', height=None, width=None, pitches=None, offsets=None, matrix='bt601'):
        if format not in FORMATS:
            raise _lib.CTError('VideoFrame: format %r (one of %s)' % (format, ', '.join(sorted(FORMATS))))
        if matrix not in MATRICES:
            raise _lib.CTError('VideoFrame: matrix %r (bt601 or bt709)' % (matrix,))
        if torch.is_tensor(data):
            if data.dtype != torch.uint8 or data.device.type != 'cuda' or not data.is_contiguous():
                raise _lib.CTError('VideoFrame: a tensor must be a contiguous torch.uint8 CUDA tensor')
            self.on_device, shape, self.nbytes = True, tuple(data.shape), data.numel()
        elif isinstance(data, np.ndarray):
            if data.dtype != np.uint8 or not data.flags['C_CONTIGUOUS']:
                raise _lib.CTError('VideoFrame: an array must be C-contiguous uint8 (got %s)' % (data.dtype,))
            self.on_device, shape, self.nbytes = False, data.shape, data.nbytes
        else:
            raise _lib.CTError('VideoFrame: data is a numpy array or a CUDA tensor (got %s)' % type(data).__name__)
        packed = format in ('bgr24', 'rgb24')
        if height is None or width is None:
            if pitches is not None or offsets is not None:
                raise _lib.CTError('VideoFrame: pitches / offsets need height and width')
            if packed:
                if len(shape) != 3 or shape[2] != 3:
                    raise _lib.CTError('VideoFrame: a %s frame is [h,w,3] (got %s)' % (format, tuple(shape)))
                height, width = shape[0], shape[1]
            else:
                if len(shape) != 2 or shape[0] % 3:
                    raise _lib.CTError('VideoFrame: a %s frame is [h*3//2, w] (got %s)' % (format, tuple(shape)))
                height, width = shape[0] * 2 // 3, shape[1]
        height, width = int(height), int(width)
        if height <= 0 or width <= 0 or (not packed and (height % 2 or width % 2)):
            raise _lib.CTError('VideoFrame: a %s frame of %d x %d (4:2:0 needs even sizes)' % (format, height, width))
        rows = _plane_rows(format, height, width)
        if pitches is None:
            pitches = [r[1] for r in rows]
        if offsets is None:
            offsets, off = [], 0
            for (nr, _), p in zip(rows, pitches):
                offsets.append(off)
                off += nr * int(p)
        pitches, offsets = tuple(int(p) for p in pitches), tuple(int(o) for o in offsets)
        if len(pitches) != len(rows) or len(offsets) != len(rows):
            raise _lib.CTError('VideoFrame: a %s frame has %d plane(s)' % (format, len(rows)))
        for (nr, nb), p, o in zip(rows, pitches, offsets):
            if p < nb or o < 0 or o + (nr - 1) * p + nb > self.nbytes:
                raise _lib.CTError('VideoFrame: plane at offset %d, pitch %d (%d rows of %d bytes) outside the buffer of %d '
                                   'bytes' % (o, p, nr, nb, self.nbytes))
        self.data, self.format, self.height, self.width = data, format, height, width
        self.pitches, self.offsets, self.matrix, self._pinned = pitches, offsets, matrix, None

    @property
    def shape(self):
        return (self.height, self.width, 3)

    @property
    def pinned(self):
        """does a host frame sit in pinned memory (``pinned_frame``): asked of the runtime once"""
        if self._pinned is None:
            self._pinned = (not self.on_device) and bool(torch.from_numpy(self.data.reshape(-1)).is_pinned())
        return self._pinned

    def base_ptr(self):
        return int(self.data.data_ptr()) if self.on_device else int(self.data.ctypes.data)

    def planes(self):
        """numpy views [rows, bytes per row] of the planes of a host frame"""
        if self.on_device:
            raise _lib.CTError('VideoFrame.planes: the frame is on the device')
        flat = self.data.reshape(-1)
        return [np.lib.stride_tricks.as_strided(flat[o:], shape=(nr, nb), strides=(p, 1), writeable=False)
                for (nr, nb), p, o in zip(_plane_rows(self.format, self.height, self.width), self.pitches, self.offsets)]


def _as_frame(frame, fmt, matrix):
    return frame if isinstance(frame, VideoFrame) else VideoFrame(np.ascontiguousarray(frame), fmt, matrix=matrix or 'bt601')


def _yuv_to_bgr(Y, U, V, matrix):
    """the conversion of DESIGN.md section 27 on full-resolution planes; chroma nearest: pixel (x, y) takes (x >> 1, y >> 1)"""
    cy, cub, cug, cvg, cvr = MATRICES[matrix]
    h, w = Y.shape
    yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
    y = np.maximum(Y.astype(np.int64) - 16, 0) * cy + (1 << 19)
    u = U.astype(np.int64)[yy][:, xx] - 128
    v = V.astype(np.int64)[yy][:, xx] - 128
    bgr = np.stack(((y + cub * u) >> 20, (y + cug * u + cvg * v) >> 20, (y + cvr * v) >> 20), axis=2)
    return np.clip(bgr, 0, 255).astype(np.uint8)


def nv12_to_bgr(frame, matrix=None):
    """uint8 [h,w,3] B, G, R of an NV12 ``VideoFrame`` (or a tightly packed [h*3//2, w] array): the integer form OpenCV
    publishes for COLOR_YUV2BGR_NV12, which ``ct_preprocess_frames`` applies to every tap"""
    f = _as_frame(frame, 'nv12', matrix)
    if f.format != 'nv12':
        raise _lib.CTError('nv12_to_bgr: a %s frame' % f.format)
    Y, UV = f.planes()
    return _yuv_to_bgr(Y, UV[:, 0::2], UV[:, 1::2], matrix or f.matrix)


def i420_to_bgr(frame, matrix=None):
    """``nv12_to_bgr`` for planar I420 (Y, U, V planes)"""
    f = _as_frame(frame, 'i420', matrix)
    if f.format != 'i420':
        raise _lib.CTError('i420_to_bgr: a %s frame' % f.format)
    Y, U, V = f.planes()
    return _yuv_to_bgr(Y, U, V, matrix or f.matrix)


def pinned_frame(format, height, width):
    """a numpy view of pinned host memory shaped like a tightly packed ``format`` frame ([h,w,3] or [h*3//2, w]) for a
    decoder to write into: a ``VideoFrame`` over it is uploaded without any host copy"""
    if format not in FORMATS:
        raise _lib.CTError('pinned_frame: format %r' % (format,))
    shape = (height, width, 3) if format in ('bgr24', 'rgb24') else (height * 3 // 2, width)
    return torch.empty(shape, dtype=torch.uint8).pin_memory().numpy()         # (the view keeps the tensor alive)


# what ``FrameStager.stage`` returns: the frames (the objects themselves), the rotation slot they were staged for, the device
# address of each frame's first byte, the event behind the copies (None: copied on the consumer's own stream), the ring
# entries used, bytes that crossed the bus
StagedFrames = collections.namedtuple('StagedFrames', 'frames slot bases event entries nbytes')


class FrameStager(object):
    """Per stream a ring of ``turns`` >= 2 (pinned, device) byte buffers, grown on demand: the frame staged ahead never
    overwrites the one the running step reads.  Only BYTES travel ahead; the pre-process launch belongs to the step that
    consumes them.  Device-resident frames are not staged: the kernel reads them in place."""

    def __init__(self, device, streams, turns=2):
        assert turns >= 2
        self.device, self.turns = device, turns
        self.ring = [[[None, None, None] for _ in range(turns)] for _ in range(streams)]      # pinned, device, last reader
        self.turn = [0] * streams
        self.copy_stream = None

    def _entry(self, s, nbytes, need_pinned):
        k = self.turn[s]
        self.turn[s] = (k + 1) % self.turns
        e = self.ring[s][k]
        if e[1] is None or e[1].numel() < nbytes:
            e[1] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if need_pinned and (e[0] is None or e[0].numel() < nbytes):
            e[0] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return k, e

    def stage(self, frames, slot, ahead):
        """upload the bytes of ``frames`` (one per stream).  ``ahead``: on the stager's copy stream with an event recorded
        behind them; otherwise on the current stream, in front of the launch that reads them."""
        lib = _lib.load()
        if ahead:
            if self.copy_stream is None:
                self.copy_stream = torch.cuda.Stream(device=self.device)
            stream = self.copy_stream
        else:
            stream = torch.cuda.current_stream()
        sp = ctypes.c_void_p(stream.cuda_stream)
        bases, entries, moved = [], [], 0
        for s, f in enumerate(frames):
            if f.on_device:
                bases.append(f.base_ptr())
                entries.append(None)
                continue
            k, e = self._entry(s, f.nbytes, not f.pinned)
            if e[2] is not None:                    # the launch that last read this entry (another stream may have issued it)
                stream.wait_event(e[2])
                e[2] = None
            if f.pinned:
                src = f.base_ptr()
            else:
                e[0].numpy()[:f.nbytes] = f.data.reshape(-1)
                src = e[0].data_ptr()
            _lib.check(lib.ct_memcpy_async(e[1].data_ptr(), src, f.nbytes, 1, sp), 'H2D')
            bases.append(e[1].data_ptr())
            entries.append((s, k))
            moved += f.nbytes
        event = None
        if ahead:
            event = torch.cuda.Event()
            event.record(stream)
        return StagedFrames(list(frames), slot, bases, event, entries, moved)

    def read_by(self, staged, stream):
        """a launch on ``stream`` reads the entries of ``staged``: whoever writes them next waits for it"""
        ev = None
        for ent in staged.entries:
            if ent is not None:
                if ev is None:
                    ev = torch.cuda.Event()
                    ev.record(stream)
                self.ring[ent[0]][ent[1]][2] = ev

    def forget(self, staged):
        """a staging that will not be consumed: wait for its copies, so that nothing is in flight into the ring"""
        if staged is not None and staged.event is not None:
            staged.event.synchronize()


class FrameLauncher(object):
    """The descriptors of ``ct_preprocess_frames``: a pinned and a device buffer of ``turns`` x ``cap`` descriptors (a turn
    per call in rotation, so that a call never rewrites descriptors whose copy may still be pending), packed and launched
    by ``launch``."""

    def __init__(self, device, cap, turns=3):
        size = ctypes.sizeof(_lib.FrameDesc)
        self.cap, self.turns, self.turn = cap, turns, 0
        self.host = torch.zeros(turns * cap * size, dtype=torch.uint8).pin_memory()
        self.dev = torch.zeros(turns * cap * size, dtype=torch.uint8, device=device)
        self.descs = [(_lib.FrameDesc * cap).from_address(self.host.data_ptr() + t * cap * size) for t in range(turns)]
        self.args = _lib.FramesDesc()

    def launch(self, frames, bases, transes, outs, flips, dst_w, dst_h, lut_ptr, sp=None):
        """one launch for ``frames``: ``bases[i]`` the device address of frame i's first byte, ``transes[i]`` its forward 2x3
        trans_input, ``outs[i]`` / ``flips[i]`` the device addresses of its [3,dst_h,dst_w] float32 output and mirrored
        output (None: not written)"""
        n = len(frames)
        if n > self.cap:
            raise _lib.CTError('FrameLauncher: %d frames, built for %d' % (n, self.cap))
        t = self.turn
        self.turn = (t + 1) % self.turns
        arr = self.descs[t]
        for i, f in enumerate(frames):
            d = arr[i]
            for p in range(3):
                live = p < len(f.offsets)
                d.plane[p] = bases[i] + f.offsets[p] if live else None
                d.pitch[p] = f.pitches[p] if live else 0
            d.format, d.h, d.w = FORMATS[f.format], f.height, f.width
            d.coef[:] = MATRICES[f.matrix]
            d.M[:] = [float(v) for v in np.asarray(transes[i], np.float64).reshape(-1)]
            d.out, d.out_flip = outs[i], flips[i]
        a = self.args
        off = t * self.cap * ctypes.sizeof(_lib.FrameDesc)
        a.staging_host, a.staging_dev = self.host.data_ptr() + off, self.dev.data_ptr() + off
        a.n, a.dst_w, a.dst_h, a.lut = n, int(dst_w), int(dst_h), lut_ptr
        _lib.check(_lib.load().ct_preprocess_frames(ctypes.byref(a), sp if sp is not None else _lib.stream_ptr()),
                   'ct_preprocess_frames')
