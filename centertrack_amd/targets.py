"""Training targets on the device: heat maps and slot tensors of a batch from object lists.

The reference builds every training target in its DataLoader workers (``GenericDataset.__getitem__``,
src/lib/dataset/generic_dataset.py:76-152 with ``_get_pre_dets`` :205-255, ``_init_ret`` :330-370,
``_mask_ignore_or_crowd`` :386-398, ``_get_bbox_output`` :407-421, ``_add_instance`` :423-515, ``_add_rot`` :556-568):
a zero-filled ``[num_classes, h, w]`` heat map and a ``[1, H, W]`` prior heat map per sample, one numpy Gaussian per
object, collate, ``batch[k].to(device)``.  ``TargetBuilder`` splits that work where inference split it:

* ``encode`` (host, per sample, in a worker): the scalar per-object arithmetic of the functions above -- with numpy's
  dtypes at every step -- and nothing dense.  It yields a *record*: a dict of small numpy arrays (picklable;
  batching is a Python list of records).
* ``render`` (device, per batch): packs the records into pinned staging memory, uploads them with one asynchronous copy
  and writes every tensor of the batch with one launch of ``ct_build_targets`` (csrc/targets.hip).  No host wait, no
  CPU fallback.
* ``reference`` (host): the reference's ``ret`` dict from a record, maps drawn with ``image.draw_umich_gaussian``.  The
  tests stand on it; ``render`` never calls it.

A record holds

  ``counts``     int32 [4]      number of slot rows, heat-map blobs, ignore rectangles, pre_hm blobs
  ``slot_k``     int32 [n]      slot (= annotation index) of each slot row: skipped annotations leave holes
  ``slot_v``     int32 [n, S]   the packed slot values: the columns of ``TargetBuilder.outputs`` side by side, float32
                                values as their bit patterns, integer values as int32
  ``hm_blobs``   int32 [nb, 4]  plane, cx, cy, radius
  ``rects``      int32 [nr, 5]  plane or -1 (all planes), x0, y0, x1, y1 (inclusive): ignore / crowd regions
  ``pre_blobs``  int32 [np, 4]  cx, cy, radius, conf

The loaders, the augmentation parameters and the flip of the annotations (boxes and key points) stay the caller's (the
images of the batch: ``inputs.InputBuilder``); ``opt.dense_reg != 1`` is refused.

The pose task (``tracking,multi_pose``) is ``PoseTargetBuilder``: ``TargetBuilder`` itself keeps
refusing the pose heads (``hps``, ``hm_hp``, ``hp_offset``).  It restates ``_add_hps`` (generic_dataset.py:517-554) and
the ``hm_hp`` line of ``_mask_ignore_or_crowd`` (:396-398) in ``encode``, and its records have the same six arrays:

* the J planes of ``hm_hp`` are numbered ``C .. C+J-1`` behind the class planes: a visible joint inside the map is one
  more row of ``hm_blobs`` (plane ``C + j``, the truncated point, the object's radius), an unlabelled joint one more row
  of ``rects`` (plane ``C + j``, the object's clipped box), and an ignore / crowd annotation of class id <= 1 a row
  with plane -2 = all ``hm_hp`` planes (next to its row for ``hm``: -1 = all class planes, or one of them);
* ``hps`` / ``hps_mask`` [2J] are head columns of the slot row like ``wh``; the joint tensors -- ``hm_hp_mask`` [J],
  ``hp_offset`` [J,2], ``hp_ind`` [J] int64, ``hp_offset_mask`` [J,2], ``joint`` [J] int64 per object, which the
  reference shapes ``[max_objs*J, ..]`` -- are further columns of it: ``[B, max_objs*J, 2]`` is ``[B, max_objs, 2J]``
  in memory.

``render`` then goes through ``ct_build_pose_targets``: ``hm_hp`` [B,J,h,w] comes out of the same launch.
"""
import math

import numpy as np

from . import _lib
from ._lib import CTError
from .image import affine_transform, draw_umich_gaussian, gaussian_radius

CULL_CAP = _lib.CT_TARGETS_CULL_CAP          # blobs a workgroup culls into LDS per round (csrc/targets.hip)
TILE_W, TILE_H = 32, 8                       # pixel tile of a workgroup
MAX_RADIUS = 16384
MAX_OUT = _lib.CT_TARGETS_MAX_OUT

# (head, channels) in the order the reference's _init_ret creates them
HEAD_DIMS = (('reg', 2), ('wh', 2), ('tracking', 2), ('ltrb', 4), ('ltrb_amodal', 4), ('nuscenes_att', 8),
             ('velocity', 3), ('dep', 1), ('dim', 3), ('amodel_offset', 2))
HPS_AFTER = 'velocity'                       # _init_ret creates hps / hps_mask [2J] behind this head
ALL_HM, ALL_HM_HP = -1, -2                   # rectangle plane codes: every class plane / every hm_hp plane
POSE_HEADS = ('hps', 'hm_hp', 'hp_offset')
NO_NOISE = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0)    # no shift, kept (uniform 1 > lost_disturb), no false positive


def _default_att_range():
    groups = ([0, 1], [2, 3, 4], [5, 6, 7])  # the nuScenes attribute groups: cycle / pedestrian / vehicle states
    return {a: g for g in groups for a in g}


class _Draws(object):
    """the six numbers of one previous object, from a recorded row or from a RandomState in the reference's order"""

    def __init__(self, row, rng):
        self.row, self.rng = row, rng

    def head(self):
        if self.rng is not None:
            r = self.rng
            return r.randn(), r.randn(), r.random_sample()
        return float(self.row[0]), float(self.row[1]), float(self.row[2])

    def fp(self):
        return self.rng.random_sample() if self.rng is not None else float(self.row[3])

    def tail(self):
        if self.rng is not None:
            return self.rng.randn(), self.rng.randn()
        return float(self.row[4]), float(self.row[5])


class TargetBuilder(object):
    num_joints = 0                               # PoseTargetBuilder: J

    def __init__(self, opt, num_classes, max_objs, cat_ids, nuscenes_att_range=None):
        heads = list(opt.heads)
        bad = [h for h in POSE_HEADS if h in heads]
        if bad and not self.num_joints:
            raise CTError('TargetBuilder: the pose heads are not covered (%s); PoseTargetBuilder builds them'
                          % ', '.join(bad))
        if getattr(opt, 'dense_reg', 1) != 1:
            raise CTError('TargetBuilder: opt.dense_reg = %r is not supported (1 only)' % (opt.dense_reg,))
        if num_classes < 1 or max_objs < 1:
            raise CTError('TargetBuilder: num_classes and max_objs must be positive')
        self.opt = opt
        self.heads = heads
        self.num_classes, self.max_objs, self.cat_ids = int(num_classes), int(max_objs), cat_ids
        self.nuscenes_att_range = nuscenes_att_range if nuscenes_att_range is not None else _default_att_range()
        self.tracking = bool(getattr(opt, 'tracking', False))
        self.pre_hm = self.tracking and bool(getattr(opt, 'pre_hm', False))
        # (name, width, int64?, shape behind [B, max_objs]) of every slot tensor, in record-column order
        outs = [('ind', 1, True, ()), ('cat', 1, True, ()), ('mask', 1, False, ())]
        for h, d in self._head_dims():
            if h in heads:
                outs += [(h, d, False, (d,)), (h + '_mask', d, False, (d,))]
        outs += self._joint_outputs()
        if 'rot' in heads:
            outs += [('rotbin', 2, True, (2,)), ('rotres', 2, False, (2,)), ('rot_mask', 1, False, ())]
        self.outputs = outs
        self.columns, c = {}, 0
        for name, wd, _, _ in outs:
            self.columns[name] = c
            c += wd
        self.slot_words = c
        self._ring = []

    def _head_dims(self):
        return HEAD_DIMS

    def _joint_outputs(self):
        return []

    def _tail(self, name, tail):
        """the shape of a slot tensor behind the batch axis"""
        return (self.max_objs,) + tail

    # ------------------------------------------------------------------ host: encode
    @staticmethod
    def _box(b):
        return np.array([b[0], b[1], b[0] + b[2], b[1] + b[3]], dtype=np.float32)

    def _pre_dets(self, anns, trans, noise, rng):
        opt = self.opt
        H, W, down = opt.input_h, opt.input_w, opt.down_ratio
        cts, ids, blobs = [], [], []
        for j, ann in enumerate(anns):
            cls_id = int(self.cat_ids[ann['category_id']])
            if cls_id > self.num_classes or cls_id <= -99 or ('iscrowd' in ann and ann['iscrowd'] > 0):
                continue
            box = self._box(ann['bbox'])
            box[:2] = affine_transform(box[:2], trans)
            box[2:] = affine_transform(box[2:], trans)
            box[[0, 2]] = np.clip(box[[0, 2]], 0, W - 1)
            box[[1, 3]] = np.clip(box[[1, 3]], 0, H - 1)
            h, w = box[3] - box[1], box[2] - box[0]
            if not (h > 0 and w > 0):
                continue                         # draws nothing from the stream either
            draws = _Draws(noise[j] if noise is not None else NO_NOISE, rng)
            radius = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
            ct = np.array([(box[0] + box[2]) / 2, (box[1] + box[3]) / 2], dtype=np.float32)
            ct0 = ct.copy()
            n0, n1, u_lost = draws.head()
            ct[0] = ct[0] + n0 * opt.hm_disturb * w
            ct[1] = ct[1] + n1 * opt.hm_disturb * h
            conf = 1 if u_lost > opt.lost_disturb else 0
            ct_int = ct.astype(np.int32)         # truncates toward zero, also for the negative centres
            cts.append(ct / down if conf == 0 else ct0 / down)
            ids.append(ann['track_id'] if 'track_id' in ann else -1)
            if self.pre_hm:
                blobs.append((int(ct_int[0]), int(ct_int[1]), radius, conf))
            if draws.fp() < opt.fp_disturb and self.pre_hm:
                n2, n3 = draws.tail()
                ct2 = ct0.copy()
                ct2[0] = ct2[0] + n2 * 0.05 * w
                ct2[1] = ct2[1] + n3 * 0.05 * h
                ct2_int = ct2.astype(np.int32)
                blobs.append((int(ct2_int[0]), int(ct2_int[1]), radius, conf))
        return cts, ids, blobs

    def _bbox_output(self, box, trans_output):
        opt = self.opt
        bbox = self._box(box).copy()
        rect = np.array([[bbox[0], bbox[1]], [bbox[0], bbox[3]], [bbox[2], bbox[3]], [bbox[2], bbox[1]]],
                        dtype=np.float32)
        for t in range(4):
            rect[t] = affine_transform(rect[t], trans_output)
        bbox[:2] = rect[:, 0].min(), rect[:, 1].min()
        bbox[2:] = rect[:, 0].max(), rect[:, 1].max()
        amodal = bbox.copy()
        bbox[[0, 2]] = np.clip(bbox[[0, 2]], 0, opt.output_w - 1)
        bbox[[1, 3]] = np.clip(bbox[[1, 3]], 0, opt.output_h - 1)
        return bbox, amodal

    def _new_slot(self):
        return {name: np.zeros(wd, np.int64 if i64 else np.float32) for name, wd, i64, _ in self.outputs}

    def _pack_slot(self, slot):
        return np.concatenate([slot[name].astype(np.int32) if i64 else slot[name].view(np.int32)
                               for name, _, i64, _ in self.outputs])

    def _instance(self, slot, cls_id, bbox, amodal, ann, trans_output, aug_s, pre_cts, track_ids):
        """one object's slot values (None when the clipped box is empty) and its heat-map blob"""
        opt, heads = self.opt, self.heads
        h, w = bbox[3] - bbox[1], bbox[2] - bbox[0]
        if h <= 0 or w <= 0:
            return None
        radius = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
        ct = np.array([(bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2], dtype=np.float32)
        ct_int = ct.astype(np.int32)
        slot['cat'][0] = cls_id - 1
        slot['mask'][0] = 1
        if 'wh' in slot:
            slot['wh'][:] = 1. * w, 1. * h
            slot['wh_mask'][:] = 1
        slot['ind'][0] = ct_int[1] * opt.output_w + ct_int[0]
        if 'reg' in slot:
            slot['reg'][:] = ct - ct_int
            slot['reg_mask'][:] = 1
        if 'tracking' in heads:
            ids = track_ids if track_ids is not None else []
            if ann['track_id'] in ids:
                pre_ct = pre_cts[ids.index(ann['track_id'])]
                slot['tracking_mask'][:] = 1
                slot['tracking'][:] = pre_ct - ct_int
        if 'ltrb' in heads:
            slot['ltrb'][:] = bbox[0] - ct_int[0], bbox[1] - ct_int[1], bbox[2] - ct_int[0], bbox[3] - ct_int[1]
            slot['ltrb_mask'][:] = 1
        if 'ltrb_amodal' in heads:
            slot['ltrb_amodal'][:] = (amodal[0] - ct_int[0], amodal[1] - ct_int[1],
                                      amodal[2] - ct_int[0], amodal[3] - ct_int[1])
            slot['ltrb_amodal_mask'][:] = 1
        if 'nuscenes_att' in heads:
            if ('attributes' in ann) and ann['attributes'] > 0:
                att = int(ann['attributes'] - 1)
                slot['nuscenes_att'][att] = 1
                slot['nuscenes_att_mask'][self.nuscenes_att_range[att]] = 1
        if 'velocity' in heads:
            if ('velocity' in ann) and min(ann['velocity']) > -1000:
                slot['velocity'][:] = np.array(ann['velocity'], np.float32)[:3]
                slot['velocity_mask'][:] = 1
        if 'rot' in heads and 'alpha' in ann:
            slot['rot_mask'][0] = 1
            alpha = ann['alpha']
            if alpha < np.pi / 6. or alpha > 5 * np.pi / 6.:
                slot['rotbin'][0] = 1
                slot['rotres'][0] = alpha - (-0.5 * np.pi)
            if alpha > -np.pi / 6. or alpha < -5 * np.pi / 6.:
                slot['rotbin'][1] = 1
                slot['rotres'][1] = alpha - (0.5 * np.pi)
        if 'dep' in heads and 'depth' in ann:
            slot['dep_mask'][:] = 1
            slot['dep'][:] = ann['depth'] * aug_s
        if 'dim' in heads and 'dim' in ann:
            slot['dim_mask'][:] = 1
            slot['dim'][:] = ann['dim']
        if 'amodel_offset' in heads and 'amodel_center' in ann:
            centre = affine_transform(ann['amodel_center'], trans_output)
            slot['amodel_offset_mask'][:] = 1
            slot['amodel_offset'][:] = centre - ct_int
        return (cls_id - 1, int(ct_int[0]), int(ct_int[1]), radius)

    def _joints(self, slot, ann, trans_output, blob, bbox, blobs, rects):
        """the key points of one object (PoseTargetBuilder)"""

    def encode(self, anns, trans_output, height, width, aug_s=1, calib=None, pre_anns=None, trans_input_pre=None,
               trans_output_pre=None, noise=None, rng=None):
        """The record of one sample.  ``anns`` / ``pre_anns``: the annotation lists as the reference's object loop sees
        them (after the flip); ``trans_output`` / ``trans_input_pre``: float64 [2,3] affines; ``aug_s``: the scale
        augmentation (``dep``).  ``noise``: ``[len(pre_anns), 6]`` -- per previous annotation the two normal draws of the
        centre shift, the ``lost`` uniform, the ``fp`` uniform and the two normal draws of the false positive (rows of
        annotations that draw nothing, and the last two numbers where ``fp`` does not fire, are not read) -- or ``rng``,
        a ``numpy.random.RandomState`` consumed in the reference's order; neither: no disturbance.  ``height``, ``width``,
        ``calib`` and ``trans_output_pre`` are what the reference passes along without using them for the targets."""
        if noise is not None and rng is not None:
            raise CTError('TargetBuilder.encode: noise and rng are alternatives')
        pre_cts, track_ids, pre_blobs = None, None, []
        if self.tracking:
            if pre_anns is None or trans_input_pre is None:
                raise CTError('TargetBuilder.encode: opt.tracking needs pre_anns and trans_input_pre')
            if noise is not None:
                noise = np.asarray(noise, np.float64)
                if noise.shape != (len(pre_anns), 6):
                    raise CTError('TargetBuilder.encode: noise must be [len(pre_anns), 6], got %s' % (noise.shape,))
            pre_cts, track_ids, pre_blobs = self._pre_dets(pre_anns, trans_input_pre, noise, rng)
        slot_k, slot_v, blobs, rects = [], [], [], []
        for k in range(min(len(anns), self.max_objs)):
            ann = anns[k]
            cls_id = int(self.cat_ids[ann['category_id']])
            if cls_id > self.num_classes or cls_id <= -999:
                continue
            bbox, amodal = self._bbox_output(ann['bbox'], trans_output)
            if cls_id <= 0 or ('iscrowd' in ann and ann['iscrowd'] > 0):
                plane = -1 if cls_id == 0 else abs(cls_id) - 1
                if plane >= self.num_classes:
                    raise CTError('TargetBuilder.encode: ignore class %d has no heat-map plane' % cls_id)
                rects.append((plane, int(bbox[0]), int(bbox[1]), int(bbox[2]), int(bbox[3])))
                if self.num_joints and cls_id <= 1:
                    rects.append((ALL_HM_HP,) + rects[-1][1:])
                continue
            slot = self._new_slot()
            blob = self._instance(slot, cls_id, bbox, amodal, ann, trans_output, aug_s, pre_cts, track_ids)
            if blob is None:
                continue
            blobs.append(blob)
            self._joints(slot, ann, trans_output, blob, bbox, blobs, rects)
            slot_k.append(k)
            slot_v.append(self._pack_slot(slot))
        rec = {'slot_k': np.array(slot_k, np.int32).reshape(-1),
               'slot_v': np.array(slot_v, np.int32).reshape(-1, self.slot_words),
               'hm_blobs': np.array(blobs, np.int32).reshape(-1, 4),
               'rects': np.array(rects, np.int32).reshape(-1, 5),
               'pre_blobs': np.array(pre_blobs, np.int32).reshape(-1, 4)}
        rec['counts'] = np.array([len(slot_k), len(blobs), len(rects), len(pre_blobs)], np.int32)
        return rec

    # ------------------------------------------------------------------ host: the reference's ret from a record
    def _check(self, rec, what='record'):
        try:
            n = [int(v) for v in np.asarray(rec['counts']).reshape(-1)]
            shapes = [tuple(np.shape(rec[k])) for k in ('slot_k', 'slot_v', 'hm_blobs', 'rects', 'pre_blobs')]
        except (KeyError, TypeError, ValueError) as e:
            raise CTError('TargetBuilder: %s is not a record of encode (%s)' % (what, e))
        want = [(n[0],), (n[0], self.slot_words), (n[1], 4), (n[2], 5), (n[3], 4)] if len(n) == 4 else None
        if shapes != want:
            raise CTError('TargetBuilder: %s: counts %s disagree with its arrays %s' % (what, n, shapes))
        k = np.asarray(rec['slot_k'])
        if k.size and (k.min() < 0 or k.max() >= self.max_objs or np.unique(k).size != k.size):
            raise CTError('TargetBuilder: %s: slot indices outside [0, %d) or repeated' % (what, self.max_objs))

    def reference(self, rec):
        """the reference's ``ret`` (without the images) as numpy arrays, on the CPU"""
        self._check(rec)
        opt = self.opt
        ret = {}
        if self.pre_hm:
            pre = np.zeros((1, opt.input_h, opt.input_w), np.float32)
            for cx, cy, r, conf in rec['pre_blobs'].tolist():
                draw_umich_gaussian(pre[0], (cx, cy), r, k=conf)
            ret['pre_hm'] = pre
        C, J = self.num_classes, self.num_joints
        maps = np.zeros((C + J, opt.output_h, opt.output_w), np.float32)       # hm, then hm_hp: the record's planes
        for name, wd, i64, tail in self.outputs:
            full = np.zeros((self.max_objs, wd), np.int64 if i64 else np.float32)
            c = self.columns[name]
            for row, k in enumerate(rec['slot_k'].tolist()):
                v = np.ascontiguousarray(rec['slot_v'][row, c:c + wd])
                full[k] = v.astype(np.int64) if i64 else v.view(np.float32)
            ret[name] = full.reshape(self._tail(name, tail))
        for plane, x0, y0, x1, y1 in rec['rects'].tolist():
            which = plane if plane >= 0 else slice(C, C + J) if J and plane == ALL_HM_HP else slice(0, C)
            region = maps[which, y0:y1 + 1, x0:x1 + 1]
            np.maximum(region, 1, out=region)
        for plane, cx, cy, r in rec['hm_blobs'].tolist():
            draw_umich_gaussian(maps[plane], (cx, cy), r)
        ret['hm'] = maps[:C]
        if J:
            ret['hm_hp'] = maps[C:]
        return ret

    # ------------------------------------------------------------------ device: render
    def output_specs(self, B):
        """{name: (shape, torch dtype)} of everything ``render`` produces for a batch of ``B``"""
        import torch
        opt = self.opt
        specs = {'hm': ((B, self.num_classes, opt.output_h, opt.output_w), torch.float32)}
        if self.pre_hm:
            specs['pre_hm'] = ((B, 1, opt.input_h, opt.input_w), torch.float32)
        if self.num_joints:
            specs['hm_hp'] = ((B, self.num_joints, opt.output_h, opt.output_w), torch.float32)
        for name, _, i64, tail in self.outputs:
            specs[name] = ((B,) + self._tail(name, tail), torch.int64 if i64 else torch.float32)
        return specs

    def _staging(self, words):
        """a pinned int32 block no call in flight still reads: an idle ring entry that is large enough, else a new one
        (never a wait: ``event.query()`` only asks)"""
        import torch
        from . import _staging
        return _staging.take(self._ring, words, torch.int32)

    def render(self, records, device=None, out=None):
        """The batch ``default_collate`` + ``.to(device)`` would have made of the reference's samples (images excluded):
        a dict of CUDA tensors.  ``out``: caller-owned tensors (a subset of the keys, any contents) that are written
        instead of fresh ones; then exactly those are written and returned.  One pinned-to-device copy and one launch on
        the current stream, no host wait."""
        import torch
        from . import ops
        records = list(records)
        B = len(records)
        if B < 1:
            raise CTError('TargetBuilder.render: empty batch')
        for b, rec in enumerate(records):
            self._check(rec, 'record %d' % b)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise CTError('TargetBuilder.render runs on an MI355X only (device %s); no CPU fallback' % device)
        specs = self.output_specs(B)
        if out is None:
            out = {k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in specs.items()}
        else:
            for k, t in out.items():
                if k not in specs:
                    raise CTError('TargetBuilder.render: no output named %r' % (k,))
                shape, dt = specs[k]
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and tuple(t.shape) == shape
                        and t.is_contiguous()):
                    raise CTError('TargetBuilder.render: out[%r] must be a contiguous %s CUDA tensor of shape %s'
                                  % (k, dt, shape))
            if not out:
                raise CTError('TargetBuilder.render: out names no tensor')
            device = next(iter(out.values())).device
        M, S, nout = self.max_objs, self.slot_words, len(self.outputs)
        map_off = 8 * B
        col_off = map_off + B * M
        tab_off = col_off + S
        payload = tab_off + 4 * nout
        parts = [np.concatenate([np.asarray(r[k], np.int32).reshape(-1) for r in records])
                 for k in ('slot_v', 'hm_blobs', 'rects', 'pre_blobs')]
        counts = np.stack([np.asarray(r['counts'], np.int64) for r in records])          # [B, 4]
        strides = np.array([S, 4, 5, 4], np.int64)
        sizes = counts * strides
        base = payload + np.concatenate([[0], np.cumsum([p.size for p in parts])[:-1]])
        offs = base[None, :] + np.cumsum(sizes, 0) - sizes                                 # [B, 4] word offsets
        words = int(payload + sum(p.size for p in parts))
        entry = self._staging(words)
        buf = entry['host'].numpy()
        hdr = np.empty((B, 8), np.int64)
        hdr[:, 0::2], hdr[:, 1::2] = offs, counts
        buf[:map_off] = hdr.reshape(-1)
        smap = np.full((B, M), -1, np.int32)
        for b, r in enumerate(records):
            smap[b, np.asarray(r['slot_k'], np.int64)] = np.arange(int(counts[b, 0]), dtype=np.int32)
        buf[map_off:col_off] = smap.reshape(-1)
        tab = np.zeros((nout, 4), np.uint32)
        for t, (name, wd, i64, _) in enumerate(self.outputs):
            c = self.columns[name]
            buf[col_off + c:col_off + c + wd] = t
            ptr = out[name].data_ptr() if name in out else 0
            tab[t] = ptr & 0xffffffff, ptr >> 32, c | (wd << 16), 1 if i64 else 0
        buf[tab_off:payload] = tab.view(np.int32).reshape(-1)
        o = payload
        for p in parts:
            buf[o:o + p.size] = p
            o += p.size
        with torch.cuda.device(device):
            dev = torch.empty(words, dtype=torch.int32, device=device)
            if self.num_joints:
                ops.build_pose_targets(entry['host'], dev, words, B, M, S, nout, self.num_classes, self.num_joints,
                                       (self.opt.output_h, self.opt.output_w), out.get('hm'), out.get('pre_hm'),
                                       out.get('hm_hp'))
            else:
                ops.build_targets(entry['host'], dev, words, B, M, S, nout, out.get('hm'), out.get('pre_hm'))
            entry['event'].record()
        return out


class PoseTargetBuilder(TargetBuilder):
    """``TargetBuilder`` for the pose task: ``hps`` and ``hm_hp`` (both required), ``hp_offset`` optional as a head -- the
    reference creates its targets with ``hm_hp`` either way (generic_dataset.py:352-363).  The flip of the key points
    (``_flip_anns`` with the dataset's ``flip_idx``) is the caller's, like the flip of the boxes."""

    def __init__(self, opt, num_classes, max_objs, cat_ids, nuscenes_att_range=None, num_joints=17):
        heads = list(opt.heads)
        if ('hps' in heads) != ('hm_hp' in heads) or 'hps' not in heads:
            # hps alone: _add_hps writes ret['hp_offset'], which only hm_hp creates; hm_hp alone: no configuration
            raise CTError('PoseTargetBuilder: the heads must hold both hps and hm_hp (%s)' % ', '.join(heads))
        if getattr(opt, 'simple_radius', 0) > 0:
            raise CTError('PoseTargetBuilder: opt.simple_radius = %r is not supported (the reference calls a function '
                          'it does not define)' % (opt.simple_radius,))
        if int(num_joints) < 1:
            raise CTError('PoseTargetBuilder: num_joints must be positive')
        self.num_joints = int(num_joints)
        super(PoseTargetBuilder, self).__init__(opt, num_classes, max_objs, cat_ids, nuscenes_att_range)
        if self.slot_words > 0xffff or len(self.outputs) > MAX_OUT:
            raise CTError('PoseTargetBuilder: %d joints do not fit a slot row' % self.num_joints)

    def _head_dims(self):
        i = [h for h, _ in HEAD_DIMS].index(HPS_AFTER) + 1
        return HEAD_DIMS[:i] + (('hps', 2 * self.num_joints),) + HEAD_DIMS[i:]

    def _joint_outputs(self):
        J = self.num_joints
        return [('hm_hp_mask', J, False, ()), ('hp_offset', 2 * J, False, (2,)), ('hp_ind', J, True, ()),
                ('hp_offset_mask', 2 * J, False, (2,)), ('joint', J, True, ())]

    def _tail(self, name, tail):
        if name in ('hm_hp_mask', 'hp_offset', 'hp_ind', 'hp_offset_mask', 'joint'):
            return (self.max_objs * self.num_joints,) + tail
        return (self.max_objs,) + tail

    def _joints(self, slot, ann, trans_output, blob, bbox, blobs, rects):
        """_add_hps with numpy's dtypes: ``pts`` is float32; the affine map and the two differences are taken in float64
        and rounded once into their float32 slots; the in-bounds test is on the float32 point; int32 truncates"""
        opt, J, C = self.opt, self.num_joints, self.num_classes
        pts = (np.array(ann['keypoints'], np.float32).reshape(J, 3) if 'keypoints' in ann
               else np.zeros((J, 3), np.float32))
        ct_int = np.array(blob[1:3], np.int32)
        radius = blob[3]                         # hp_radius: the object's own radius
        for j in range(J):
            pts[j, :2] = affine_transform(pts[j, :2], trans_output)
            if pts[j, 2] > 0:
                if 0 <= pts[j, 0] < opt.output_w and 0 <= pts[j, 1] < opt.output_h:
                    slot['hps'][2 * j:2 * j + 2] = pts[j, :2].astype(np.float64) - ct_int
                    slot['hps_mask'][2 * j:2 * j + 2] = 1
                    pt_int = pts[j, :2].astype(np.int32)
                    slot['hp_offset'][2 * j:2 * j + 2] = pts[j, :2].astype(np.float64) - pt_int
                    slot['hp_ind'][j] = int(pt_int[1]) * opt.output_w + int(pt_int[0])
                    seen = 0 if pts[j, 2] == 1 else 1      # visibility 1: drawn, indexed, but not learnt from
                    slot['hp_offset_mask'][2 * j:2 * j + 2] = seen
                    slot['hm_hp_mask'][j] = seen
                    slot['joint'][j] = j
                    blobs.append((C + j, int(pt_int[0]), int(pt_int[1]), radius))
            else:
                rects.append((C + j, int(bbox[0]), int(bbox[1]), int(bbox[2]), int(bbox[3])))
