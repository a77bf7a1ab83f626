"""Per-frame inference orchestration: the reference's ``Detector`` surface on the HIP path.

``Detector(opt)`` / ``run(image_or_path_or_tensor, meta={}) -> dict`` /
``reset_tracking()`` / ``.pre_process`` / ``.pause`` follow src/lib/detector.py:24-172,
455-458 so the class drops in under the reference's demo.py / test.py; the returned dict
has the same keys (``results, tot, load, pre, net, dec, post, merge, track, display``).
What changed underneath: the whole device side of one frame -- three
stems, DLA-34, 16 DCNv2 nodes, heads with fused sigmoid, flip merge, NMS + top-K +
gathers -- is a fixed launch sequence of libcentertrack_hip kernels replayed from ONE HIP
graph, and the 8-14 per-key D2H copies + 4 device syncs of detector.py:338-350 are one
packed [B,K,F] copy + one stream sync.

``StreamDetector`` is the batched extension the reference does not have (BASELINE
configs 3-5): B independent video streams advance one frame per call, each with its own
``Tracker`` / ``pre_images`` state; streams never mix (frames of one stream stay
sequential).  ``Detector`` is the B = 1 case.
"""
import ctypes
import math
import os
import time

import numpy as np
import torch

from . import _lib, fast_track, ops
NATIVE_LOOP = os.environ.get('CENTERTRACK_NATIVE_LOOP', '1') != '0'   # (A/B switch: 0 = the Python frame loop)
# split stem (round 3, measured and left OFF): the x / pre_img terms of frame t+1's stem launched behind frame t's graph, to
# run in the GPU time the host needs for the association of frame t.  Bit-identical (tests), but two A/B pairs on an
# MI355X showed no overlap: wall - graph grew from 11 us to 73-80 us for a 36 us pre-stage -- the kernel launched between
# two graph launches costs more in front-end transitions than the host gap it was meant to fill.
# CENTERTRACK_SPLIT_STEM_MAX = largest image batch it is used for (0 = never).
SPLIT_STEM_MAX = int(os.environ.get('CENTERTRACK_SPLIT_STEM_MAX', '0'))
HOST_FLAG = os.environ.get('CENTERTRACK_HOST_FLAG', '1') != '0'       # end-of-frame flag in pinned host memory (A/B switch)
HOST_ROWS = os.environ.get('CENTERTRACK_HOST_ROWS', '1') != '0'       # decode writes the rows to pinned host memory itself
from .frames import FrameLauncher, FrameStager, VideoFrame
from .image import (affine_transform, draw_umich_gaussian, gaussian_radius, get_affine_transform, make_meta)
from .model import create_model, load_model
from .post_process import generic_post_process
from .tracker import Tracker

# mean / std every dataset class of the reference shares (generic_dataset.py:39-42)
MEAN = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32).reshape(1, 1, 3)
STD = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32).reshape(1, 1, 3)
REST_FOCAL_LENGTH = {'nuscenes': 1200, 'kitti': 721.5377, 'kitti_tracking': 721.5377}
AVERAGE_FLIPS = ('hm', 'wh', 'dep', 'dim')
NEG_AVERAGE_FLIPS = ('amodel_offset',)
# left/right joint pairs of the COCO person key points (datasets/coco_hp.py:18-19)
COCO_FLIP_IDX = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


def trans_bbox(bbox, trans, width, height):
    """detector.py:242-251"""
    bbox = np.array(bbox, dtype=np.float32).copy()
    bbox[:2] = affine_transform(bbox[:2], trans)
    bbox[2:] = affine_transform(bbox[2:], trans)
    bbox[[0, 2]] = np.clip(bbox[[0, 2]], 0, width - 1)
    bbox[[1, 3]] = np.clip(bbox[[1, 3]], 0, height - 1)
    return bbox


def render_pre_hm(tracks, meta, pre_thresh, out=None, with_hm=True):
    """Prior heat-map from tracker state (detector.py:254-290): one max-splatted Gaussian
    per active track with score >= pre_thresh.  Returns (hm [H,W] f32, pre_inds list)."""
    inp_w, inp_h = meta['inp_width'], meta['inp_height']
    out_w, out_h = meta['out_width'], meta['out_height']
    hm = np.zeros((inp_h, inp_w), np.float32) if out is None else out
    if out is not None:
        hm[...] = 0
    inds = []
    for det in tracks:
        if det['score'] < pre_thresh or det['active'] == 0:
            continue
        bbox = trans_bbox(det['bbox'], meta['trans_input'], inp_w, inp_h)
        bbox_out = trans_bbox(det['bbox'], meta['trans_output'], out_w, out_h)
        h, w = bbox[3] - bbox[1], bbox[2] - bbox[0]
        if h > 0 and w > 0:
            radius = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
            ct = np.array([(bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2], dtype=np.float32)
            if with_hm:
                draw_umich_gaussian(hm, ct.astype(np.int32), radius)
            ct_out = np.array([(bbox_out[0] + bbox_out[2]) / 2, (bbox_out[1] + bbox_out[3]) / 2], dtype=np.int32)
            inds.append(int(ct_out[1] * out_w + ct_out[0]))
    return hm, inds


def imread_bgr(path):
    """``cv2.imread(path)`` (detector.py:66): the decoded image as uint8 [H,W,3] in BGR channel order.  cv2 is used
    when it is installed (bit-identical to the reference by construction); otherwise Pillow decodes the file -- lossless
    8-bit formats (PNG, BMP, PPM) give the same pixels, JPEG decoders may differ in the last bit of a pixel.  Like
    cv2.imread's default flags the Pillow path applies the EXIF orientation and drops an alpha channel; 16-bit and
    palette images go through Pillow's ``convert('RGB')``, whose rounding can differ from cv2's -- install cv2 for those."""
    try:
        import cv2
        img = cv2.imread(str(path))
        if img is None:
            raise _lib.CTError('cannot read image %r' % (path,))
        return img
    except ImportError:
        pass
    try:
        from PIL import Image
    except ImportError:
        raise _lib.CTError('reading image files needs cv2 or Pillow; pass the decoded uint8 BGR array instead')
    from PIL import ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)                       # cv2.imread rotates by the EXIF orientation tag
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def _own_option(opt, name, default=False):
    """an option this package adds to the reference's namespace: optional whoever built ``opt``"""
    return getattr(opt, name, default)


def _prefetchable(prefetch, shape):
    """may ``prefetch`` be uploaded ahead into a frame slot: a contiguous float32 host tensor of the frames' ``shape``"""
    return (prefetch is not None and torch.is_tensor(prefetch) and prefetch.device.type == 'cpu'
            and prefetch.dtype == torch.float32 and prefetch.is_contiguous() and tuple(prefetch.shape) == tuple(shape))


def _frame_source(images, uploaded, slot):
    """where this step's frame comes from, as a ``FrameStepArgs.frame_kind``: already in ``slot``, one DMA from a host or a
    device tensor, or a torch copy.  ``uploaded``: (tensor, version, slot) of the previous step's prefetch, or None."""
    # the SAME tensor object, unmodified since it was handed over (an in-place edit bumps ``_version``; a new
    # tensor at a recycled address is another object), uploaded into THIS slot
    if uploaded is not None and uploaded[0] is images and uploaded[1] == images._version and uploaded[2] == slot:
        return _lib.CT_FRAME_UPLOADED
    if images.dtype == torch.float32 and images.is_contiguous():
        return _lib.CT_FRAME_DEVICE if images.device.type == 'cuda' else _lib.CT_FRAME_HOST
    return _lib.CT_FRAME_IN_PLACE


RAW_STAGED, RAW_UPLOAD = 'staged', 'upload now'


def _raw_frame_source(frames, staged, slot):
    """where the bytes of this step's ``VideoFrame``s come from: RAW_STAGED only when every element is the same object that
    was staged for THIS slot (``staged``: the ``frames.StagedFrames`` of the previous step's ``prefetch``, or None), else
    RAW_UPLOAD -- the caller forgets a stale staging first"""
    if (staged is not None and staged.slot == slot and len(staged.frames) == len(frames)
            and all(a is b for a, b in zip(staged.frames, frames))):
        return RAW_STAGED
    return RAW_UPLOAD


def _is_video(frames):
    """is a list of raw frames a list of ``VideoFrame``s (True) or of plain arrays (False); a mixture is refused"""
    kinds = {isinstance(f, VideoFrame) for f in frames}
    if len(kinds) > 1:
        raise _lib.CTError('step(): a list of frames holds VideoFrames or plain arrays, not both')
    return kinds == {True}


class _HipGraph(object):
    """One captured frame (ct_graph_begin / ct_graph_end); ``replay()`` enqueues it on the current stream."""

    def __init__(self, fn, collect=True):
        lib = _lib.load()
        side = torch.cuda.Stream()                 # (the legacy default stream cannot be captured)
        side.wait_stream(torch.cuda.current_stream())
        sp = ctypes.c_void_p(side.cuda_stream)
        with _lib.capture_guard(collect=collect), torch.cuda.stream(side):
            _lib.check(lib.ct_graph_begin(sp), 'ct_graph_begin')
            try:
                fn()
            finally:
                self.exec = lib.ct_graph_end(sp)
        torch.cuda.current_stream().wait_stream(side)
        if not self.exec:
            raise _lib.CTError('ct_graph_end failed: %s' % lib.ct_last_error().decode())
        self._lib = lib

    def replay(self, sp=None):
        rc = self._lib.ct_graph_launch(self.exec, sp if sp is not None else _lib.stream_ptr())
        if rc:
            _lib.check(rc, 'ct_graph_launch')

    def __del__(self):
        try:
            self._lib.ct_graph_destroy(self.exec)
        except Exception:
            pass


class _FrameContext(object):
    """What a ``StreamDetector`` keeps per network input size: launch plan, static buffers, captured graphs, native frame
    loop.  It refers back to its detector (model, options, trackers), so the two form a reference cycle: a dropped
    detector is destroyed by the cyclic collector, which ``_lib.capture_guard`` keeps out of captures."""
    _METHODS = ('pre_stage', 'device_frame')
    __slots__ = ('det', 'hw', 'NB', 'plan', 'img_in', 'hm_in', 'render', 'flip_call', 'merged', 'done_flag', 'host_out',
                 'host_rows', 'decoder', 'row_layout', 'host_hm', 'max_blobs', 'pc_host', 'pc_dev', 'prm_host', 'cnt_host',
                 'prm_dev', 'cnt_dev', 'nslots', 'frames', 'slot', 'launched', 'partial', 'graphs', 'graph', 'raw',
                 'copy_stream', 'frame_ready', 'copy_sp', 'loop', 'loop_desc', 'loop_stream', 'loop_trackers', 'rows_keep',
                 'res_cap', 'res_buf', 'counts', 'tin', 'tinv', 'args')

    def __init__(self, det, H, W):
        tracking = bool(getattr(det.opt, 'tracking', False))
        with_img = tracking and bool(getattr(det.opt, 'pre_img', True))
        with_hm = tracking and bool(getattr(det.opt, 'pre_hm', False))
        # detector, input size, image batch, launch plan and its prior inputs; is the prior heat map rendered from blobs
        self.det, self.hw, self.NB = det, (H, W), det.B * (2 if det.flip else 1)
        self.plan = det.model.get_plan(self.NB, H, W, with_img, with_hm, True, det.sparse, sparse_pose=det.sparse_pose)
        (_, self.img_in, self.hm_in), self.render = self.plan['inputs'], det.native and with_hm
        # flip_test: the arguments of ct_flip_merge; the maps the decode reads (the plan's outputs without flip_test)
        self.flip_call, self.merged = None, self.plan['outputs']
        # decode: pinned flag and rows [B,K,F] (tensor, numpy view), decoder, native row layout, heat map of the Python host path
        self.done_flag = self.host_out = self.host_rows = self.decoder = self.row_layout = self.host_hm = None
        # blobs of the device-rendered prior heat map: triples of every stream + per-stream counts, host and device
        self.max_blobs = self.pc_host = self.pc_dev = self.prm_host = self.cnt_host = self.prm_dev = self.cnt_dev = None
        # rotating frame slots, slot of the NEXT frame, the frame the native loop launched ahead, split-stem maps per slot
        self.nslots = self.frames = self.launched = self.partial = None
        self.slot = 0
        # one captured graph per slot (None: eager launches), the first of them, raw HIP graphs or torch's (``capture``)
        self.graphs, self.graph, self.raw = None, None, False
        # upload stream of the Python frame loop with its event and raw handle, from the first prefetch on (``own_copy_stream``)
        self.copy_stream = self.frame_ready = self.copy_sp = None
        # the native frame loop and what it reads and writes through pointers (``make_loop``)
        self.loop = self.loop_desc = self.loop_stream = self.loop_trackers = self.rows_keep = None
        self.res_cap = self.res_buf = self.counts = self.tin = self.tinv = self.args = None
        if det.flip:
            self._build_flip_merge()
        self._build_decoder(with_hm)
        if self.render:
            self._build_blobs()
        self._build_slots()

    # bench.py, tools/ and the GPU tests read the context by subscript and bench.py cannot change: that is the only reason
    # for these two.  Inside the package use the attributes.
    def __getitem__(self, name):
        if name in self.__slots__ or name in self._METHODS:
            return getattr(self, name)
        raise KeyError(name)

    def get(self, name, default=None):
        return getattr(self, name) if name in self.__slots__ or name in self._METHODS else default

    def _build_flip_merge(self):
        """detector.py:311-332: averaged heads get a merged [B,c,h,w] map (ct_flip_merge, one launch for all of
        them); the heads the reference takes from the un-flipped image alone are read in place (first B images)"""
        B, outs = self.det.B, self.plan['outputs']
        modes = {'hps': _lib.CT_FLIP_JOINT_OFFSETS, 'hm_hp': _lib.CT_FLIP_JOINTS}
        modes.update({k: _lib.CT_FLIP_AVG for k in AVERAGE_FLIPS})
        modes.update({k: _lib.CT_FLIP_NEG_EVEN for k in NEG_AVERAGE_FLIPS})
        merged, fl = {}, []
        for k, v in outs.items():
            if k in modes:
                merged[k] = torch.empty((B,) + tuple(v.shape[1:]), device=self.det.device)
                fl.append((v, merged[k], modes[k]))
            else:
                merged[k] = v[:B]
        heads_arr = (_lib.FlipHead * len(fl))()
        for i, (v, m, mode) in enumerate(fl):
            assert v.stride(3) == 1 and v.stride(2) == v.shape[3] and v.stride(1) == v.shape[2] * v.shape[3]
            heads_arr[i].src, heads_arr[i].dst = v.data_ptr(), m.data_ptr()
            heads_arr[i].src_batch_stride, heads_arr[i].C, heads_arr[i].mode = v.stride(0), v.shape[1], mode
        pairs = np.ascontiguousarray(getattr(self.det.opt, 'flip_idx', COCO_FLIP_IDX), np.int32).reshape(-1, 2)
        self.flip_call = (heads_arr, len(fl), pairs, int(outs['hm'].shape[2]), int(outs['hm'].shape[3]))
        self.merged = merged

    def _build_decoder(self, with_hm):
        """the decode over the merged maps, its pinned rows and end-of-frame flag (detector.py:338-350 as one block)"""
        det, opt, merged = self.det, self.det.opt, self.merged
        dec_heads = {k: v for k, v in merged.items() if k != 'hm'}
        self.done_flag = torch.zeros((16,), dtype=torch.int32).pin_memory()      # (its own cache line)
        sparse = self.plan.get('sparse')
        if sparse is not None:
            sparse = dict(sparse, zero_tracking=bool(getattr(opt, 'zero_tracking', False)), flip=det.flip)
        sparse_pose = self.plan.get('sparse_pose')
        if sparse_pose is not None:
            sparse_pose = dict(sparse_pose, flip=det.flip, flip_pairs=getattr(opt, 'flip_idx', COCO_FLIP_IDX))
        F = ops.Decoder.row_floats(dec_heads, [n for n, *_ in sparse['heads']] if sparse else None, sparse_pose)
        self.host_out = torch.zeros((merged['hm'].shape[0], opt.K, F), dtype=torch.float32).pin_memory()
        # (round 3: the decode stores its rows straight into the pinned block and raises the end-of-frame flag itself --
        #  no D2H copy node and no flag kernel at the end of the frame graph; not with pose heads, whose kernels
        #  complete the rows after the decode)
        direct = HOST_FLAG and HOST_ROWS
        self.decoder = ops.Decoder(merged['hm'], dec_heads, opt.K, host_out=self.host_out if direct else None,
                                   done_flag=self.done_flag if direct else None, sparse=sparse, sparse_pose=sparse_pose)
        assert tuple(self.decoder.out.shape) == tuple(self.host_out.shape)
        self.host_rows = self.host_out.numpy()
        if with_hm and not det.native:
            self.host_hm = torch.zeros((self.NB, 1) + self.hw, dtype=torch.float32).pin_memory()
        if det.native:
            self.row_layout = fast_track.row_layout(self.decoder.layout)

    def _build_blobs(self):
        """blob triples of every stream followed by the per-stream counts: ONE pinned buffer, one H2D per frame"""
        B = self.det.B
        nblob = self.max_blobs = fast_track.max_blobs(self.det.opt.K)
        nprm = B * nblob * 3
        self.pc_host = torch.zeros((nprm + B,), dtype=torch.int32).pin_memory()
        self.pc_dev = torch.zeros((nprm + B,), dtype=torch.int32, device=self.det.device)
        self.prm_host, self.cnt_host = self.pc_host[:nprm].view(B, nblob, 3), self.pc_host[nprm:]
        self.prm_dev, self.cnt_dev = self.pc_dev[:nprm], self.pc_dev[nprm:]

    def _build_slots(self):
        """Frame buffers owned by THIS detector (the plan's activation buffers are shared by every detector of
        the model).  They ROTATE: the frame of step t is written into slot t % nslots and read as `pre_img` from
        there at step t+1, so the reference's `self.pre_images = images` (detector.py:148) costs no copy; with three
        slots the frame of step t+1 can be uploaded straight into ITS slot while the graph of step t still reads
        slots t and t-1 (round 3: no staging buffer, no device-to-device copy between upload and launch); one
        captured graph per slot."""
        H, W = self.hw
        self.nslots = 3 if self.img_in is not None else 2
        self.frames = [torch.zeros_like(self.plan['inputs'][0]) for _ in range(self.nslots)]
        self.graphs = [None] * self.nslots
        if self.img_in is not None and self.hm_in is not None and 0 < self.NB <= SPLIT_STEM_MAX:
            self.partial = [ops.new_view(self.NB, H, W, 16, self.det.device) for _ in range(self.nslots)]

    def own_copy_stream(self):
        """the Python frame loop's upload stream, created at the first prefetch"""
        if self.copy_stream is None:
            self.copy_stream, self.frame_ready = torch.cuda.Stream(device=self.det.device), torch.cuda.Event()
            self.copy_sp = ctypes.c_void_p(self.copy_stream.cuda_stream)

    def flip_slot(self, slot, sp=None):
        """the mirrored half of the batch in ``slot`` (detector.py:224-226), built from the frames already in HBM"""
        cur, B, (H, W) = self.frames[slot], self.det.B, self.hw
        _lib.check(_lib.load().ct_flip_images(cur.data_ptr(), cur[B:].data_ptr(), B * 3 * H, W,
                                              sp if sp is not None else _lib.stream_ptr()), 'ct_flip_images')

    def pre_stage(self, slot):
        """the part of a frame that does not depend on the tracker: the mirrored half of a flip_test batch and the
        x / pre_img terms of the stem.  The native loop runs it for frame t+1 behind the graph of frame t."""
        if self.partial is None:
            return
        if self.det.flip:
            self.flip_slot(slot)
        self.det.model.run_stem_partial(self.frames[slot], self.frames[(slot - 1) % self.nslots], self.partial[slot])

    def device_frame(self, slot=0, with_copies=False):
        """all device work of one frame; ``with_copies``: also the H2D of the prior-heat-map blobs and the D2H
        of the packed detections (fixed pinned buffers), so that a captured frame is ONE graph launch"""
        det, lib, (H, W), st = self.det, _lib.load(), self.hw, _lib.stream_ptr()
        cur = self.frames[slot]
        prev = self.frames[(slot - 1) % self.nslots] if self.img_in is not None else None
        if with_copies and self.render:
            _lib.check(lib.ct_memcpy_async(self.pc_dev.data_ptr(), self.pc_host.data_ptr(), self.pc_host.numel() * 4, 1, st), 'H2D')
        if self.render:
            _lib.check(lib.ct_render_pre_hm(self.prm_dev.data_ptr(), self.cnt_dev.data_ptr(), self.max_blobs, det.B, H, W,
                                            self.hm_in.data_ptr(), 1 if det.flip else 0, st), 'ct_render_pre_hm')
        if det.flip and self.partial is None:
            self.flip_slot(slot, st)
        det.model._run_plan(self.plan, inputs=(cur, prev, self.hm_in), stem_partial=self.partial[slot] if self.partial else None)
        if det.flip:
            arr, n, pairs, h, w = self.flip_call
            _lib.check(lib.ct_flip_merge(arr, n, pairs.ctypes.data, len(pairs), det.B, h, w, st), 'ct_flip_merge')
        if getattr(det.opt, 'zero_tracking', False) and 'tracking' in self.merged:      # decode.py:142-143 `*= 0`
            t = self.merged['tracking']
            for b in range(t.shape[0]):
                _lib.check(lib.ct_memset_async(t[b].data_ptr(), 0, t[b].numel() * 4, st), 'memset')
        self.decoder.run()
        if with_copies and not self.decoder.direct:
            _lib.check(lib.ct_memcpy_async(self.host_out.data_ptr(), self.decoder.out.data_ptr(), self.host_out.numel() * 4, 2, st), 'D2H')
            if HOST_FLAG:         # the native loop polls this flag instead of waiting in the runtime
                _lib.check(lib.ct_signal_host(self.done_flag.data_ptr(), 1, st), 'ct_signal_host')

    def capture(self):
        """warm-up on a side stream, then one graph per slot: raw HIP graphs, or torch's under CENTERTRACK_RAW_GRAPH=0"""
        try:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.pre_stage(0)
                self.device_frame(0)           # warm-up (lazy module loads must not happen in capture)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            # only C-ABI launches inside device_frame (no torch op, flip_test included): capture / replay
            # straight through HIP
            raw = os.environ.get('CENTERTRACK_RAW_GRAPH', '1') != '0'
            for sl in range(self.nslots):
                if raw:
                    g = _HipGraph(lambda: self.device_frame(sl, True), collect=(sl == 0))      # (garbage is collected once, ahead of the first capture)
                else:
                    g = torch.cuda.CUDAGraph()
                    with _lib.capture_guard(collect=False), torch.cuda.graph(g):
                        self.device_frame(sl)
                self.graphs[sl] = g
            self.raw = raw
        except Exception as e:
            # never degrade silently: the eager launches are the same kernels at a fraction of the frame rate
            if os.environ.get('CENTERTRACK_GRAPH_FALLBACK', '0') != '1':
                raise _lib.CTError('HIP graph capture of the frame failed (%s); pass use_graph=False or set '
                                   'CENTERTRACK_GRAPH_FALLBACK=1 to run eager launches' % (e,))
            import warnings
            warnings.warn('centertrack_amd: HIP graph capture failed (%s); using eager launches' % (e,))
            self.graphs = [None] * self.nslots
            torch.cuda.synchronize()
        self.graph = self.graphs[0]

    def make_loop(self):
        """the native frame loop (ct_frame_loop_*, csrc/frame_loop.hip) over this context's graphs / buffers / trackers"""
        det, lib, (H, W) = self.det, _lib.load(), self.hw
        B, K, F = self.decoder.out.shape
        d = _lib.FrameLoopDesc()
        d.B, d.K, d.F = int(B), int(K), int(F)
        self.loop_trackers = (ctypes.c_void_p * det.B)(*[f.h for f in det.fast])
        d.trackers = ctypes.cast(self.loop_trackers, ctypes.POINTER(ctypes.c_void_p))
        d.layout = self.row_layout
        d.out_thresh, d.pre_thresh = float(det.opt.out_thresh), float(det.opt.pre_thresh)
        d.inp_w, d.inp_h = int(W), int(H)
        d.host_rows = self.host_out.data_ptr()
        self.rows_keep = np.zeros(tuple(self.decoder.out.shape), np.float32)
        d.rows_keep = self.rows_keep.ctypes.data
        if self.render:
            d.blob_params, d.blob_counts, d.blob_cap = self.prm_host.data_ptr(), self.cnt_host.data_ptr(), self.max_blobs
        d.nslots = self.nslots
        for i in range(self.nslots):
            d.graphs[i], d.frames[i] = self.graphs[i].exec, self.frames[i].data_ptr()
        d.frame_bytes = det.B * 3 * H * W * 4
        self.loop_stream = torch.cuda.current_stream()
        d.stream = self.loop_stream.cuda_stream
        if self.partial is not None:
            P = det.model._prepare()
            d.pre.enabled = 1
            d.pre.N, d.pre.H, d.pre.W = self.NB, int(H), int(W)
            d.pre.w_x, d.pre.w_img = P['stem_w'][0].data_ptr(), P['stem_w'][1].data_ptr()
            d.pre.scale3, d.pre.shift3 = P['stem_scale'].data_ptr(), P['stem_shift'].data_ptr()
            for i in range(self.nslots):
                d.pre.partial[i] = self.partial[i].ptr
            d.pre.ldp = self.partial[0].ld
            d.pre.flip_B = det.B if det.flip else 0
        self.res_cap = det.fast[0].cap
        self.res_buf = np.zeros((det.B, self.res_cap), fast_track.TRACK_DTYPE)
        d.results, d.results_cap = self.res_buf.ctypes.data, self.res_cap
        d.done_flag = self.done_flag.data_ptr() if HOST_FLAG else None
        h = lib.ct_frame_loop_create(ctypes.byref(d))
        if not h:
            raise _lib.CTError('ct_frame_loop_create: %s' % lib.ct_last_error().decode())
        self.loop, self.loop_desc = ctypes.c_void_p(h), d
        self.counts = np.zeros(det.B, np.int32)
        self.tin, self.tinv = np.zeros((det.B, 6), np.float64), np.zeros((det.B, 6), np.float32)
        self.args = [_lib.FrameStepArgs(), _lib.FrameStepArgs()]
        for a in self.args:
            a.trans_input, a.trans_inv = self.tin.ctypes.data, self.tinv.ctypes.data

    def forget_upload(self, uploaded):
        """THE ordering rule of the frame slots, called from one place per frame path: a frame uploaded ahead (``uploaded``:
        its record, or None) that is not used as it stands is forgotten before anything else writes the slot it targeted"""
        if uploaded is not None and self.loop is not None:
            _lib.load().ct_frame_loop_forget_upload(self.loop)
        if uploaded is not None and self.copy_stream is not None:
            self.copy_stream.synchronize()

    def close(self):
        """wait for the device and destroy the native loop: the one place that does"""
        if self.loop is not None:
            torch.cuda.synchronize()
            _lib.load().ct_frame_loop_destroy(self.loop)      # (joins its helper threads)
            self.loop = None


class StreamDetector(object):
    """B independent streams, one frame each per ``step``."""
    supports_prefetch = True

    def __init__(self, opt, model=None, num_streams=1, use_graph=True, native_host=True):
        if not torch.cuda.is_available():
            raise _lib.CTError('centertrack_amd needs an MI355X (no CPU fallback)')
        _lib.load()
        self.opt = opt
        self.device = torch.device('cuda', torch.cuda.current_device())
        opt.device = self.device
        if model is None:
            model = create_model(opt.arch, opt.heads, opt.head_conv, opt=opt)
            if getattr(opt, 'load_model', ''):
                model = load_model(model, opt.load_model, opt)
        self.model = model.to(self.device).eval()
        self.B = num_streams
        self.flip = bool(getattr(opt, 'flip_test', False))
        # opt.sparse_heads (round 5, opt-in, NOT a reference flag): the regression heads are evaluated at the K winners of
        # the decode only instead of as dense maps (ct_sparse_heads_desc) -- same results (the decode reads nothing else of
        # them, decode.py:99-180), 1/5 of the heads' work.  flip_test: hm is merged as a map, the averaged regression heads are
        # evaluated in both images at the winner and its mirrored pixel.  Not with pose heads (hm_hp is a heat-map).
        self.sparse = bool(getattr(opt, 'sparse_heads', False)) and not ({'hps', 'hm_hp'} & set(opt.heads))
        # option sparse_pose_heads (opt-in, NOT a reference flag): the pose task's counterpart.  hm and hm_hp stay maps (both are
        # decoded as heat-maps); hps is evaluated at the K winners and hp_offset (else reg) at the K peaks of every joint map
        # (ct_decode_pose_sparse), reg / wh or ltrb / tracking at the winners like sparse_heads.  Not with an ltrb_amodal head:
        # the match gates a snapped joint with the wh / ltrb box (decode.py:123,137), which the rows then do not hold, and no
        # map is left to rebuild it from.  In every case it does not serve, the dense path runs unchanged.
        self.sparse_pose = (bool(_own_option(opt, 'sparse_pose_heads')) and {'hm', 'hps', 'hm_hp'} <= set(opt.heads)
                            and 'ltrb_amodal' not in opt.heads and int(getattr(self.model, 'head_conv', 0)) == 256)
        self.use_graph = use_graph
        self.trackers = [Tracker(opt) for _ in range(self.B)]
        # native host path (C++ post-process + association incl. the Hungarian / public-detection / pre_dets branches
        # + device-rendered prior heat-map, key points of the pose task); the reference-shaped Python path serves zero_pre_hm
        self.native = bool(native_host and getattr(opt, 'tracking', False) and 'tracking' in opt.heads
                           and not getattr(opt, 'zero_pre_hm', False))
        self.fast = [fast_track.FastTracker(opt.new_thresh, getattr(opt, 'max_age', -1), opt.K,
                                            hungarian=getattr(opt, 'hungarian', False),
                                            public_det=getattr(opt, 'public_det', False))
                     for _ in range(self.B)] if self.native else None
        self._last_dets = None
        self._prefetched = None    # (host tensor, its _version, slot) of a frame uploaded ahead by step(prefetch=...)
        self.started = [False] * self.B
        # device-side pre-processing of raw u8 frames (ct_preprocess_device): normalisation table + staging buffers
        lut = np.empty((3, 256), np.float32)
        mean, std = np.ascontiguousarray(MEAN.reshape(-1)), np.ascontiguousarray(STD.reshape(-1))
        _lib.check(_lib.load().ct_preprocess_lut(mean.ctypes.data, std.ctypes.data, 3, lut.ctypes.data), 'ct_preprocess_lut')
        self._lut = torch.from_numpy(lut).to(self.device)
        self._raw_bufs = {}
        # VideoFrames (frames.py): byte staging with its record of the frames uploaded ahead, descriptors + launch
        self._stager = self._launcher = self._staged = None
        self._carried = {}         # per stream: extras (3D fields) of tracks kept alive without a detection
        # optional hook: called with the packed device rows [B,K,F] right after the frame was launched (multi-GPU
        # all-gather, parallel.DetectionGatherer).  It may return a CUDA event after which the rows have been read: the
        # next frame's launch (which overwrites them) then waits for it on the device, so the hook is free to read the
        # rows from a side stream
        self.gather_fn = None
        self._rows_free = None
        self._ctx = None

    def __del__(self):
        try:
            ctx = self._ctx
            if ctx is not None and ctx.loop is not None:
                # (collected while the current stream is capturing -- somebody else's graph: waiting for the device here would
                #  invalidate that capture; the native loop is leaked instead.  The package's own captures keep the collector
                #  out altogether, _lib.capture_guard)
                if os.environ.get('CT_NO_CAPTURE_GUARD') != '1' and torch.cuda.is_current_stream_capturing():
                    return
                ctx.close()
        except Exception:
            pass

    # ---- per-shape device context (static buffers + captured graph) ----------------------
    def _context(self, H, W):
        if self._ctx is not None and self._ctx.hw == (H, W):
            return self._ctx
        if self._ctx is not None:
            self._ctx.close()                                  # another input size: a new loop below
        ctx = _FrameContext(self, H, W)
        if self.use_graph:
            ctx.capture()
        if ctx.raw and self.native and NATIVE_LOOP:
            ctx.make_loop()
        self._ctx = ctx
        return ctx

    def _warp_frame(self, s, image, meta, frames, H, W):
        """upload the raw u8 frame of stream ``s`` and warp / normalise it into ``frames[s]`` (and the mirrored copy
        into ``frames[B + s]`` under flip_test) on the device: detector.py:218-226 without the host warp"""
        lib = _lib.load()
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise _lib.CTError('raw frames must be uint8 HxWx3 (got %s %s)' % (image.dtype, image.shape))
        h, w, c = image.shape
        if (int(meta['inp_height']), int(meta['inp_width'])) != (H, W):
            raise _lib.CTError('all streams of a step must share the network input size')
        need = h * w * c
        bufs = self._raw_bufs.get(s)
        if bufs is None or bufs[0].numel() < need:
            bufs = (torch.empty(need, dtype=torch.uint8).pin_memory(),
                    torch.empty(need, dtype=torch.uint8, device=self.device))
            self._raw_bufs[s] = bufs
        host, dev = bufs
        host.numpy()[:need].reshape(h, w, c)[...] = image      # (pinned staging: the H2D below is a plain DMA)
        st = _lib.stream_ptr()
        _lib.check(lib.ct_memcpy_async(dev.data_ptr(), host.data_ptr(), need, 1, st), 'H2D')
        trans = np.ascontiguousarray(meta['trans_input'], np.float64)
        _lib.check(lib.ct_preprocess_device(dev.data_ptr(), h, w, w * c, c, trans.ctypes.data, W, H,
                                            self._lut.data_ptr(), frames[s].data_ptr(),
                                            frames[self.B + s].data_ptr() if self.flip else None, st),
                   'ct_preprocess_device')

    def _forget_staged(self):
        """VideoFrames staged ahead that will not be consumed as they stand"""
        staged, self._staged = self._staged, None
        if staged is not None:
            self._stager.forget(staged)

    def _stage_video_ahead(self, ns, prefetch):
        """the BYTES of the next step's VideoFrames, uploaded on the stager's copy stream while this frame runs; their
        pre-process launch belongs to the next step"""
        self._forget_staged()
        if self._stager is None:
            self._stager = FrameStager(self.device, self.B)
        self._staged = self._stager.stage(prefetch, ns, True)

    def _video_frames(self, ctx, slot, frames, metas):
        """a step's VideoFrames into ``ctx.frames[slot]`` on the current stream: the bytes staged ahead or uploaded now, one
        descriptor upload, ONE ``ct_preprocess_frames`` launch for all streams (and the mirrored copies under flip_test)"""
        B, (H, W), fr = self.B, ctx.hw, ctx.frames[slot]
        for m in metas:
            if (int(m['inp_height']), int(m['inp_width'])) != (H, W):
                raise _lib.CTError('all streams of a step must share the network input size')
        if self._stager is None:
            self._stager = FrameStager(self.device, B)
        if self._launcher is None:
            self._launcher = FrameLauncher(self.device, B)
        cur = torch.cuda.current_stream()
        staged = self._staged
        if _raw_frame_source(frames, staged, slot) == RAW_STAGED:
            self._staged = None
            cur.wait_event(staged.event)
        else:
            self._forget_staged()
            staged = self._stager.stage(frames, slot, False)
        plane = 3 * H * W * 4
        base = fr.data_ptr()
        self._launcher.launch(frames, staged.bases, [m['trans_input'] for m in metas],
                              [base + s * plane for s in range(B)],
                              [base + (B + s) * plane if self.flip else None for s in range(B)], W, H,
                              self._lut.data_ptr(), ctypes.c_void_p(cur.cuda_stream))
        self._stager.read_by(staged, cur)

    # ---- one frame for every stream -------------------------------------------------------
    def _meta_transforms(self, m):
        """float64 [6] network-input affine and float32 [6] inverse output affine (post_process.py:30) of a frame's
        meta, cached in the dict, keyed on the VALUES of c / s (an in-place edit or a recycled object id must not
        resurrect a stale transform)"""
        cached = m.get('_trans_inv')
        c_, s_ = m['c'], m['s']
        ident = (float(c_[0]), float(c_[1]), float(s_) if np.ndim(s_) == 0 else tuple(np.ravel(s_).tolist()),
                 m['out_width'], m['out_height'])
        if cached is None or cached[0] != ident:
            tinv = np.ascontiguousarray(get_affine_transform(
                m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1).astype(np.float32))
            m['_trans_inv'] = cached = (ident, tinv)
        return cached[1]

    def _gather(self, ctx):
        """the gather hook, called right behind this frame's launch; the event after which the rows have been read, if any"""
        ev = self.gather_fn(ctx.decoder.out) if self.gather_fn is not None else None
        return ev if isinstance(ev, torch.cuda.Event) else None

    @staticmethod
    def _fill_timers(timers, t0, t1, t2, post, track):
        """the reference's timer keys (detector.py:162-165); decode and merge are part of ``net`` here"""
        if timers is not None:
            timers.update({'pre': t1 - t0, 'net': t2 - t1, 'dec': 0.0, 'post': post, 'merge': 0.0, 'track': track})

    def _checked_submit(self, ctx, rc, what):
        """a submit can fail AFTER its graph launch (upload of the next frame, its pre-stage; frame_loop.hip: "the frame
        itself is in flight"): drain that frame and forget the half-issued upload before raising, so that the next
        step() finds an idle loop instead of failing with 'the previous frame was not finished' for ever.  The error text
        is read first -- the calls below would overwrite it."""
        if rc == 0:
            return
        lib = _lib.load()
        msg = lib.ct_last_error().decode('utf-8', 'replace')
        lib.ct_frame_loop_wait(ctx.loop)
        lib.ct_frame_loop_forget_upload(ctx.loop)
        ctx.launched = None
        self._prefetched = None
        raise _lib.CTError('%s failed (%d): %s' % (what, rc, msg))

    def _drop_launched(self, ctx):
        """a frame the native loop launched ahead will not be used (other frame handed over, reset): wait for it and
        give its slot back -- the trackers never saw it"""
        if ctx.loop is not None and ctx.launched is not None:
            _lib.check(_lib.load().ct_frame_loop_wait(ctx.loop), 'ct_frame_loop_wait')
            _lib.load().ct_frame_loop_forget_upload(ctx.loop)      # (also: whatever was pre-staged is stale)
            ctx.slot = (ctx.slot - 1) % ctx.nslots
            ctx.launched = None

    def _step_native(self, ctx, images, metas, timers, prefetch, prefetch_metas):
        """steady state of the native tracking path: the frame loop of csrc/frame_loop.hip.  With ``prefetch`` AND
        ``prefetch_metas`` the next frame is launched by the same native call that finishes this one.

        The loop launches its graphs on the stream that was current when the context was built (``loop_stream``).  A
        caller that steps under another ``torch.cuda.stream(...)`` is ordered against it explicitly: the loop stream
        first waits for whatever the caller's stream has enqueued (the producer of a device-resident ``images``), the
        torch-side work of the step (slot copy, gather hook) is issued on the loop stream, and the caller's stream
        waits for the loop stream on the way out."""
        cs = torch.cuda.current_stream()
        ls = ctx.loop_stream
        if cs != ls:
            ls.wait_stream(cs)
            try:
                with torch.cuda.stream(ls):
                    return self._step_native_on_loop_stream(ctx, images, metas, timers, prefetch, prefetch_metas)
            finally:
                cs.wait_stream(ls)
        return self._step_native_on_loop_stream(ctx, images, metas, timers, prefetch, prefetch_metas)

    def _native_stage_frame(self, ctx, cur, slot, images, metas):
        """the transforms of this frame's metas and where the loop finds the frame (``cur``: its FrameStepArgs)"""
        for s_ in range(self.B):
            ctx.tinv[s_] = self._meta_transforms(metas[s_]).reshape(-1)
            ctx.tin[s_] = np.asarray(metas[s_]['trans_input'], np.float64).reshape(-1)
        uploaded, self._prefetched = self._prefetched, None
        cur.slot, cur.frame, cur.next_frame = slot, None, None
        if isinstance(images, (list, tuple)):      # VideoFrames: pre-processed into the slot by a launch on the loop stream
            ctx.forget_upload(uploaded)
            self._video_frames(ctx, slot, images, metas)
            cur.frame_kind = _lib.CT_FRAME_IN_PLACE
            return
        self._forget_staged()
        cur.frame_kind = _frame_source(images, uploaded, slot)
        if cur.frame_kind != _lib.CT_FRAME_UPLOADED:
            ctx.forget_upload(uploaded)            # (a stale upload may still target this slot: drained BEFORE the copy)
        if cur.frame_kind in (_lib.CT_FRAME_DEVICE, _lib.CT_FRAME_HOST):
            cur.frame = images.data_ptr()
        elif cur.frame_kind == _lib.CT_FRAME_IN_PLACE:
            ctx.frames[slot][:self.B].copy_(images)

    def _native_results(self, ctx):
        """the track records the loop left per stream, copied: the loop rewrites its block with the next frame"""
        out = []
        for s_ in range(self.B):
            k = int(ctx.counts[s_])
            if k > ctx.res_cap:                                # (max_age > 0 lets the track list grow: re-read it)
                tmp = np.zeros(k, fast_track.TRACK_DTYPE)
                got = _lib.load().ct_tracker_get_tracks(self.fast[s_].h, tmp.ctypes.data, k)
                out.append(tmp[:min(got, k)])
            else:
                out.append(ctx.res_buf[s_, :k].copy())
        return out

    def _step_native_on_loop_stream(self, ctx, images, metas, timers, prefetch, prefetch_metas):
        lib = _lib.load()
        t0 = time.time()
        n, loop = ctx.nslots, ctx.loop
        launched = ctx.launched
        video = isinstance(images, (list, tuple))
        ahead = launched is not None and launched[0] is images and launched[1] == images._version
        if launched is not None and not ahead:
            self._drop_launched(ctx)
        cur, nxt = ctx.args
        if ahead:
            # this frame is already in flight; its prior heat-map was built with the metas promised last step
            if any(a is not b for a, b in zip(launched[2], metas)) and [self._meta_transforms(m).tobytes() for m in metas] != launched[3]:
                raise _lib.CTError('step(): the metas of this frame differ from the prefetch_metas promised for it')
            ctx.launched = None
            slot = (ctx.slot - 1) % n
        else:
            slot = ctx.slot
            self._native_stage_frame(ctx, cur, slot, images, metas)
        # (a float frame uploaded ahead is what ct_frame_loop_finish_submit launches: VideoFrames stage their bytes instead)
        can_prefetch = not video and _prefetchable(prefetch, images.shape)
        t1 = time.time()
        if ahead:
            if can_prefetch:            # the frame after the one in flight: its slot was last read by the finished frame
                _lib.check(lib.ct_frame_loop_upload(loop, (slot + 1) % n, prefetch.data_ptr()), 'ct_frame_loop_upload')
        else:
            if can_prefetch:
                cur.next_frame = prefetch.data_ptr()
            if self._rows_free is not None:                    # (left by a step of the Python path)
                ctx.loop_stream.wait_event(self._rows_free)
                self._rows_free = None
            self._checked_submit(ctx, lib.ct_frame_loop_submit(loop, ctypes.byref(cur)), 'ct_frame_loop_submit')
            ctx.slot = (slot + 1) % n
        if can_prefetch:
            self._prefetched = (prefetch, prefetch._version, (slot + 1) % n)
        elif self._stageable(prefetch):
            self._stage_video_ahead((slot + 1) % n, prefetch)
        # (the hook enqueues its reader of the device rows behind this frame's graph; the event it returns is waited
        # for ON THE STREAM right here, i.e. between this graph and the next one, whoever launches that)
        ev = self._gather(ctx)
        if ev is not None:
            ctx.loop_stream.wait_event(ev)
        counts = ctx.counts
        early = can_prefetch and prefetch_metas is not None and all(a is b for a, b in zip(prefetch_metas, metas))
        if early:
            # finish this frame and launch the next one in ONE native call: the GPU idles for the association only
            nxt.slot, nxt.frame_kind, nxt.frame, nxt.next_frame = (slot + 1) % n, _lib.CT_FRAME_UPLOADED, None, None
            ctx.slot = (slot + 1) % n            # (where the loop stands if the call below fails half-way)
            self._checked_submit(ctx, lib.ct_frame_loop_finish_submit(loop, ctypes.byref(cur), counts.ctypes.data,
                                                                      ctypes.byref(nxt)), 'ct_frame_loop_finish_submit')
            ctx.slot = (slot + 2) % n
            ctx.launched = (prefetch, prefetch._version, list(metas), [self._meta_transforms(m).tobytes() for m in metas])
            self._prefetched = None
        else:
            _lib.check(lib.ct_frame_loop_finish(loop, ctypes.byref(cur), counts.ctypes.data), 'ct_frame_loop_finish')
        t2 = time.time()
        self._last_dets = None
        out = self._native_results(ctx)
        self._fill_timers(timers, t0, t1, t2, 0.0, time.time() - t2)
        return out

    def step(self, images, metas, timers=None, prefetch=None, prefetch_metas=None):
        """images: float32 [B,3,H,W] (already normalised, like PrefetchDataset hands over), or a list of B raw
        uint8 HxWx3 frames, which are uploaded as bytes and warped / normalised on the device
        (``ct_preprocess_device``, bit-identical to ``Detector.pre_process``), or a list of B ``frames.VideoFrame``s -- BGR /
        RGB / NV12 / I420, host or device memory, formats and sizes free per stream -- whose bytes are uploaded (or read in
        place) and which ONE ``ct_preprocess_frames`` launch converts, warps and normalises for all streams (the same bits);
        metas: list of B ``meta`` dicts (image.make_meta).  Returns a list of B result lists.
        ``prefetch``: the float32 host tensor the NEXT call will pass as ``images`` (optional): its H2D copy is enqueued
        on a second HIP stream as soon as this frame's graph is launched and overlaps with it -- what the reference's
        ``DataLoader(pin_memory=True)`` + ``images.to(device, non_blocking=True)`` (test.py:74-76, detector.py:93-94) is
        for; the copy lands in the NEXT frame's own rotation slot, so the next call launches without any device copy.
        A list of B ``VideoFrame``s as ``prefetch`` has their BYTES uploaded ahead the same way (``frames.FrameStager``); the
        next call must pass the same objects, otherwise the staging is forgotten and the frames passed are uploaded then.
        ``prefetch_metas``: the metas the next call will pass (the same objects as ``metas`` for a video whose frames
        share one size): with them the native loop launches the next frame in the call that finishes this one."""
        opt = self.opt
        t0 = time.time()
        B = self.B
        raw_frames = isinstance(images, (list, tuple))
        video = raw_frames and _is_video(images)
        if not raw_frames and self.flip and images.shape[0] == 2 * B:
            # what the reference's pre_process hands over under --flip_test (detector.py:225-226: the frame and its
            # mirrored copy): the mirrored half is rebuilt on the device by the frame's first launch
            images = images[:B]
        assert len(images) == B and len(metas) == B
        if raw_frames:
            H, W = int(metas[0]['inp_height']), int(metas[0]['inp_width'])
        else:
            H, W = int(images.shape[2]), int(images.shape[3])
        ctx = self._context(H, W)
        if (ctx.loop is not None and all(self.started)
                and (video if raw_frames else tuple(images.shape) == (B, 3, H, W))
                and not getattr(opt, 'public_det', False) and not getattr(opt, 'zero_tracking', False)):
            return self._step_native(ctx, images, metas, timers, prefetch, prefetch_metas)
        self._drop_launched(ctx)
        # (torch.cuda.current_stream() costs ~5 us of host time per call and the GPU idles while the host prepares a
        # frame: looked up once per step)
        cur = torch.cuda.current_stream()
        sp = ctypes.c_void_p(cur.cuda_stream)
        slot = ctx.slot
        self._stage_frame(ctx, slot, images, metas, cur, sp)
        if bool(getattr(opt, 'tracking', False)):
            self._start_streams(ctx, slot, metas, sp)
            self._prior_heat_map(ctx, metas)
            self.started[:] = [True] * B                       # (only now: the heat map raises on a broken meta)
        t1 = time.time()
        self._launch(ctx, slot, cur, sp)
        self._prefetch_next(ctx, slot, prefetch)
        self._rows_free = self._gather(ctx)
        if ctx.raw:                                            # (the D2H of the rows is the graph's last node)
            _lib.check(_lib.load().ct_stream_synchronize(sp), 'ct_stream_synchronize')
        else:
            ctx.host_out.copy_(ctx.decoder.out, non_blocking=True)
            cur.synchronize()
        t2 = time.time()
        if ctx.rows_keep is not None:
            ctx.rows_keep[...] = ctx.host_rows                 # (last_dets reads the kept copy when a native loop exists)
        self._last_dets = None                                 # unpacked on demand (last_dets)
        results, t_post, t_track = self._associate(ctx, ctx.host_rows, metas)
        self._fill_timers(timers, t0, t1, t2, t_post, t_track)
        return results

    def _stage_frame(self, ctx, slot, images, metas, cur, sp):
        """``pre_process`` of raw frames on the device (detector.py:80-82, 218-226) or ``images.to(device)``
        (detector.py:93-94): the frame goes straight into its rotation slot (images [0, B); the mirrored images [B, 2B) of
        flip_test are built on the device by the frame's first launch, detector.py:224-226)"""
        B, (H, W), fr = self.B, ctx.hw, ctx.frames[slot]
        uploaded, self._prefetched = self._prefetched, None    # (a frame uploaded ahead serves the very next call only)
        source = None                                          # (raw frames)
        if not isinstance(images, (list, tuple)):
            if tuple(images.shape) != (B, 3, H, W):
                raise _lib.CTError('step() expects [%d,3,%d,%d] frames, got %s' % (B, H, W, tuple(images.shape)))
            source = _frame_source(images, uploaded, slot)
        if source == _lib.CT_FRAME_UPLOADED and ctx.loop is None:
            cur.wait_event(ctx.frame_ready)                    # uploaded by the previous step's ``prefetch``
        else:                     # (also THIS frame if the native loop's copy stream uploaded it: a wait on the host; rare path)
            ctx.forget_upload(uploaded)
        if source is None and _is_video(images):
            self._video_frames(ctx, slot, images, metas)
            return
        self._forget_staged()
        if source is None:
            for s in range(B):
                self._warp_frame(s, images[s], metas[s], fr, H, W)
        elif source in (_lib.CT_FRAME_HOST, _lib.CT_FRAME_DEVICE):
            # one DMA from wherever the caller keeps the frame: H2D for a host tensor (detector.py:93-94 -- pinned
            # memory makes it asynchronous), D2D for a resident one
            _lib.check(_lib.load().ct_memcpy_async(fr.data_ptr(), images.data_ptr(), images.numel() * 4,
                                                   1 if source == _lib.CT_FRAME_HOST else 0, sp), 'frame copy')
        elif source == _lib.CT_FRAME_IN_PLACE:
            fr[:B].copy_(images)

    def _start_streams(self, ctx, slot, metas, sp):
        """first frame of a stream (detector.py:97-103): ``pre_dets`` into its tracker, ``pre_images = images``"""
        B = self.B
        fresh = [s for s in range(B) if not self.started[s]]
        for s in fresh:
            pre_dets = metas[s].get('pre_dets', [])
            if self.native and len(pre_dets) > 0:
                self.fast[s].init_tracks(pre_dets)             # tracker.init_track, detector.py:101-102
            if not self.native:
                self.trackers[s].init_track(pre_dets)
        if ctx.img_in is not None:
            # first frame of a stream: pre_images = images (detector.py:99-103)
            fr, prev = ctx.frames[slot], ctx.frames[(slot - 1) % ctx.nslots]
            if fresh and self.flip:
                ctx.flip_slot(slot, sp)
            if len(fresh) == B:
                prev.copy_(fr)
            else:
                for s in fresh:
                    prev[s].copy_(fr[s])
                    if self.flip:
                        prev[B + s].copy_(fr[B + s])

    def _prior_heat_map(self, ctx, metas):
        """``_get_additional_inputs`` (detector.py:104-110, 254-290): the blobs of the native trackers, which the frame
        renders on the device, or ``render_pre_hm`` on the host and one H2D"""
        opt, B = self.opt, self.B
        if ctx.hm_in is not None and self.native:
            ph, ch = ctx.prm_host.numpy(), ctx.cnt_host.numpy()
            for s in range(B):
                m = metas[s]
                ch[s], _ = self.fast[s].prehm_params(opt.pre_thresh, m['trans_input'], m['inp_width'], m['inp_height'], out=ph[s])
            if not ctx.raw:                                    # (the raw graph carries this copy itself)
                ctx.pc_dev.copy_(ctx.pc_host, non_blocking=True)
        elif ctx.hm_in is not None:
            hh = ctx.host_hm
            for s in range(B):
                render_pre_hm(self.trackers[s].tracks, metas[s], opt.pre_thresh, out=hh[s, 0].numpy(),
                              with_hm=not getattr(opt, 'zero_pre_hm', False))
                if self.flip:
                    hh[B + s, 0].copy_(torch.flip(hh[s, 0], [1]))
            ctx.hm_in.copy_(hh, non_blocking=True)

    def _launch(self, ctx, slot, cur, sp):
        """``process`` (detector.py:118-119, 300-350): the pre-stage unless it ran ahead, then the frame as a raw graph,
        a torch graph or eager launches"""
        if self._rows_free is not None:                        # (a side-stream reader of the previous frame's rows)
            cur.wait_event(self._rows_free)
            self._rows_free = None
        if ctx.partial is not None:                            # the tracker-independent part (unless it ran ahead)
            if ctx.loop is not None:
                _lib.check(_lib.load().ct_frame_loop_prestage(ctx.loop, slot), 'ct_frame_loop_prestage')
            else:
                ctx.pre_stage(slot)
        if ctx.raw:
            ctx.graphs[slot].replay(sp)
        elif ctx.graphs[slot] is not None:
            ctx.graphs[slot].replay()
        else:
            ctx.device_frame(slot)
        ctx.slot = (slot + 1) % ctx.nslots                     # this frame is the next step's pre_img (detector.py:148)

    def _stageable(self, prefetch):
        """may ``prefetch`` be staged ahead as bytes: a list of one VideoFrame per stream"""
        return (isinstance(prefetch, (list, tuple)) and len(prefetch) == self.B
                and all(isinstance(f, VideoFrame) for f in prefetch))

    def _prefetch_next(self, ctx, slot, prefetch):
        """the next frame's ``images.to(device, non_blocking=True)`` (test.py:74-76, detector.py:93-94), one step early"""
        if self._stageable(prefetch):
            self._stage_video_ahead((slot + 1) % ctx.nslots, prefetch)
            return
        if not _prefetchable(prefetch, (self.B, 3) + ctx.hw):
            return
        # straight into the NEXT frame's slot: it was last read (as pre_img) by the previous frame's graph, which the
        # host has waited for -- the graph just launched reads this slot and the one before it only
        lib, ns = _lib.load(), (slot + 1) % ctx.nslots
        if ctx.loop is not None:                               # (the next step may be the native loop's: its copy stream)
            _lib.check(lib.ct_frame_loop_upload(ctx.loop, ns, prefetch.data_ptr()), 'ct_frame_loop_upload')
        else:
            ctx.own_copy_stream()
            _lib.check(lib.ct_memcpy_async(ctx.frames[ns].data_ptr(), prefetch.data_ptr(), prefetch.numel() * 4, 1, ctx.copy_sp), 'prefetch')
            ctx.frame_ready.record(ctx.copy_stream)
        self._prefetched = (prefetch, prefetch._version, ns)

    def _associate(self, ctx, rows, metas):
        """``post_process`` + ``merge_outputs`` + ``tracker.step`` per stream (detector.py:126-147, 371-377).  Returns
        the results and the seconds spent in post-processing and in association."""
        opt, results = self.opt, []
        if self.native:
            ta = time.time()
            for s in range(self.B):
                m = metas[s]
                tinv = self._meta_transforms(m)
                pub = m['cur_dets'] if getattr(opt, 'public_det', False) else None       # detector.py:141-142
                results.append(self.fast[s].step(rows[s], ctx.row_layout, opt.out_thresh, tinv, pub).copy())
            return results, 0.0, time.time() - ta
        dets = self.last_dets
        tracking = bool(getattr(opt, 'tracking', False))
        t_post = t_track = 0.0
        for s in range(self.B):
            ta = time.time()
            meta = metas[s]
            one = {k: v[s:s + 1] for k, v in dets.items()}
            res = generic_post_process(opt, one, [meta['c']], [meta['s']], meta['out_height'], meta['out_width'],
                                       opt.num_classes, [meta['calib']], meta['height'], meta['width'])[0]
            res = [r for r in res if r['score'] > opt.out_thresh]          # merge_outputs, detector.py:371-377
            tb = time.time()
            if tracking:
                public_det = meta['cur_dets'] if getattr(opt, 'public_det', False) else None   # (KeyError like the reference)
                res = self.trackers[s].step(res, public_det)
            t_post += tb - ta
            t_track += time.time() - tb
            results.append(res)
        return results, t_post, t_track

    @property
    def last_dets(self):
        """the reference's ``dets`` dict (decode.py:99-180) of the last step: numpy views of a per-frame COPY of the
        packed rows -- the pinned D2H buffer is overwritten by the next step, while the reference's
        ``.cpu().numpy()`` arrays (detector.py:349-350) stay valid for as long as a caller keeps the results"""
        if self._last_dets is None and self._ctx is not None:
            keep = self._ctx.rows_keep                 # (the native loop may already be writing the next frame's rows)
            self._last_dets = self._ctx.decoder.unpack((keep if keep is not None else self._ctx.host_rows).copy())
        return self._last_dets

    def reset_tracking(self, stream=None):
        if self._ctx is not None:
            self._drop_launched(self._ctx)
            self._ctx.forget_upload(self._prefetched)
        self._forget_staged()
        for s in (range(self.B) if stream is None else [stream]):
            self.trackers[s].reset()
            if self.fast is not None:
                self.fast[s].reset()
            self._carried.pop(s, None)
            self.started[s] = False
        self._prefetched = None

    def results_as_dicts(self, results, stream=0, meta=None):
        """one stream's result of ``step`` as the reference's list of dicts (``meta``: the frame's meta, whose
        ``calib`` yields the 3D location / yaw of the ddd heads)"""
        if isinstance(results, np.ndarray):
            carried = self._carried.setdefault(stream, {})
            tinv = meta['_trans_inv'][1] if (meta is not None and '_trans_inv' in meta) else None
            return fast_track.as_dicts(results, self.last_dets, stream, None if meta is None else meta.get('calib'),
                                       carried, tinv)
        return results


class Detector(object):
    """The reference's single-stream ``Detector`` API (src/lib/detector.py)."""

    def __init__(self, opt, model=None, use_graph=True, native_host=True):
        if not hasattr(opt, 'device'):
            opt.device = torch.device('cuda')
        self._init_host(opt)
        self.impl = StreamDetector(opt, model=model, num_streams=1, use_graph=use_graph, native_host=native_host)
        self.model = self.impl.model

    def _init_host(self, opt):
        """the host-side state ``pre_process`` / ``frame_meta`` / the prefetch-dict parser need (no device): what a
        DataLoader worker process of test.py:75 touches"""
        scales = list(getattr(opt, 'test_scales', [1.0]))
        if len(scales) != 1:
            # detector.py:78-133,371-377 loops over the scales and merges the detections before ONE tracker step; no
            # tracking experiment of the reference uses it (experiments/*.sh) and the fused frame (decode -> association
            # in one native call) has no multi-scale form: refuse instead of silently taking the first scale
            raise _lib.CTError('centertrack_amd.Detector supports one test scale (got test_scales=%s): multi-scale '
                               'testing (detector.py:78, merge_outputs) is not part of the accelerated path' % scales)
        self.opt = opt
        self.mean, self.std = MEAN, STD
        self.pause = not getattr(opt, 'no_pause', True)
        self.rest_focal_length = (REST_FOCAL_LENGTH.get(getattr(opt, 'dataset', ''), 1200)
                                  if getattr(opt, 'test_focal_length', -1) < 0 else opt.test_focal_length)
        self.cnt = 0

    @property
    def tracker(self):
        """the stream's tracker (``.id_count``, ``.tracks`` / ``.reset()`` like the reference's)"""
        return self.impl.fast[0] if self.impl.native else self.impl.trackers[0]

    def pre_process(self, image, scale, input_meta={}):
        """detector.py:207-239: crop / scale the original u8 HWC frame to the network input
        (``cv2.warpAffine(image, trans_input, (inp_w, inp_h), INTER_LINEAR)``), normalise, HWC -> CHW,
        optional flipped copy, and the ``meta`` dict.  Host code like the reference's (test.py runs it in
        DataLoader worker processes): ``ct_preprocess_image`` restates OpenCV's fixed-point warp (cv2 is not
        needed).  As in the reference, ``scale`` is accepted and ignored (``_transform_scale(image)`` is
        called with its default, detector.py:212-213)."""
        import ctypes
        opt = self.opt
        image = np.ascontiguousarray(image)
        height, width, ch = image.shape
        meta = self.frame_meta(image, input_meta)
        inp_h, inp_w = meta['inp_height'], meta['inp_width']
        flip = bool(getattr(opt, 'flip_test', False))
        out = np.empty((2 if flip else 1, ch, inp_h, inp_w), np.float32)
        trans = np.ascontiguousarray(meta['trans_input'], np.float64)
        mean = np.ascontiguousarray(self.mean.reshape(-1)[:ch], np.float32)
        std = np.ascontiguousarray(self.std.reshape(-1)[:ch], np.float32)
        _lib.check(_lib.load().ct_preprocess_image(
            image.ctypes.data_as(ctypes.c_void_p), height, width, image.strides[0], ch,
            trans.ctypes.data_as(ctypes.c_void_p), inp_w, inp_h, mean.ctypes.data_as(ctypes.c_void_p),
            std.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), 1 if flip else 0),
            'ct_preprocess_image')
        return torch.from_numpy(out), meta

    def frame_meta(self, image, input_meta={}):
        """the ``meta`` dict of detector.py:207-217,227-239 for a raw frame (c, s, trans_input, trans_output, calib,
        sizes; ``pre_dets`` / ``cur_dets`` carried over) -- everything pre_process returns except the pixels"""
        opt = self.opt
        if isinstance(image, VideoFrame):
            height, width = image.height, image.width
        elif image.dtype != np.uint8 or image.ndim != 3:
            raise _lib.CTError('pre_process expects a uint8 HxWxC image (got %s %s)' % (image.dtype, image.shape))
        else:
            height, width = image.shape[:2]
        meta = make_meta(getattr(opt, 'input_h', -1), getattr(opt, 'input_w', -1), height, width,
                         down_ratio=getattr(opt, 'down_ratio', 4), calib=input_meta.get('calib'),
                         focal_length=self.rest_focal_length, fix_res=bool(getattr(opt, 'fix_res', True)),
                         fix_short=getattr(opt, 'fix_short', 0), pad=getattr(opt, 'pad', 31))
        if 'pre_dets' in input_meta:
            meta['pre_dets'] = input_meta['pre_dets']
        if 'cur_dets' in input_meta:
            meta['cur_dets'] = input_meta['cur_dets']
        return meta

    def run(self, image_or_path_or_tensor, meta={}):
        start = time.time()
        x = image_or_path_or_tensor
        if isinstance(x, dict):                                # prefetch path, detector.py:66-70,84-92
            images, meta = self.parse_prefetched(x)
        elif torch.is_tensor(x):
            images = x
        elif isinstance(x, VideoFrame):                        # a decoder's frame: bytes up, converted and warped on the device
            images, meta = [x], self.frame_meta(x, meta)
        elif isinstance(x, (str, os.PathLike)) or isinstance(x, np.ndarray):
            if not isinstance(x, np.ndarray):                  # image file (detector.py:65-66; test.py:163)
                x = imread_bgr(x)
            # raw BGR frame (demo.py / README embedding)
            if getattr(self.opt, 'device_pre_process', True) and x.ndim == 3 and x.shape[2] == 3:
                images, meta = [x], self.frame_meta(x, meta)   # u8 upload + warp on the device
            else:
                images, meta = self.pre_process(x, 1.0, meta)
        else:
            raise _lib.CTError('run() takes an image path, a uint8 image array, a VideoFrame, a normalised tensor + meta, or a '
                               'pre-processed dict (got %s)' % type(x).__name__)
        loaded = time.time()
        timers = {}
        results = self.impl.results_as_dicts(self.impl.step(images, [meta], timers)[0], 0, meta)
        self.cnt += 1
        end = time.time()
        ret = {'results': results, 'tot': end - start, 'load': loaded - start, 'display': 0.0}
        ret.update(timers)
        return ret

    def parse_prefetched(self, x):
        """the dict test.py's ``PrefetchDataset`` yields through a DataLoader of batch size 1 (test.py:22-51,74-76:
        ``{'images': {scale: [1,B,3,H,W]}, 'image': ..., 'meta': {scale: {key: [1,...]}, 'pre_dets'/'cur_dets': ...}}``)
        -> (images [B,3,H,W], meta) exactly as detector.py:84-92 unpacks it"""
        scale = self.opt.test_scales[0] if hasattr(self.opt, 'test_scales') else 1.0
        images = x['images'][scale][0]
        meta = {k: (v.numpy()[0] if torch.is_tensor(v) else v) for k, v in x['meta'][scale].items()}
        for k in ('pre_dets', 'cur_dets'):
            if k in x['meta']:
                meta[k] = x['meta'][k]
        return images, meta

    def reset_tracking(self):
        self.impl.reset_tracking()


def default_opt(heads, **kw):
    """Namespace with the reference's flag names the hot path reads and the
    tracking-task threshold derivation of opts.py:280-289."""
    import types
    o = types.SimpleNamespace(
        arch='dla_34', heads=heads, head_conv=256, dla_node='dcn', head_kernel=3, load_model='',
        tracking=True, pre_img=True, pre_hm=True, zero_pre_hm=False, flip_test=False, K=100,
        track_thresh=0.3, out_thresh=-1.0, pre_thresh=-1.0, new_thresh=0.3, max_age=-1, hungarian=False,
        public_det=False, zero_tracking=False, depth_scale=1.0, down_ratio=4, num_classes=heads['hm'],
        test_scales=[1.0], model_output_list=False, no_pause=True, dataset='', test_focal_length=-1,
        input_h=512, input_w=512, fix_res=True, fix_short=0, pad=31, sparse_pose_heads=False)
    for k, v in kw.items():
        setattr(o, k, v)
    if o.tracking:
        o.out_thresh = max(o.track_thresh, o.out_thresh)
        o.pre_thresh = max(o.track_thresh, o.pre_thresh)
        o.new_thresh = max(o.track_thresh, o.new_thresh)
    return o
