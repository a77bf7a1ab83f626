"""DLA-34 + DLAUp/IDAUp (DCNv2 nodes) + heads as a pre-planned sequence of HIP launches.

Mirrors the reference's model boundary: ``create_model(arch, heads,
head_conv, opt)`` / ``load_model`` (src/lib/model/model.py:24-90) and
``model(x, pre_img, pre_hm)[-1] -> {head: [B,c,h,w]}`` (base_model.py:73-91,
dla.py:593-640), with the reference's state-dict keys, so its ``.pth`` files load
unchanged.  Internally nothing of torch.nn runs: weights are BN-folded and packed
once into MFMA fragment order, activations are NHWC views, concatenations are
channel slices of shared buffers, and each frame is ~70 launches of
libcentertrack_hip kernels on the current stream (capturable in one HIP graph).
"""
import ctypes
import os
from collections import OrderedDict, namedtuple

import torch

from . import _lib, autotune, dcn_schedule, ops
from .dcn_schedule import SMALL_SLOT_WGS  # noqa: F401  (its home; kept importable from here)
from .ops import View
from .weights import CHANNELS, LEVELS, dla34_param_shapes

BN_EPS = 1e-5
FUSE_OFFSET = os.environ.get('CENTERTRACK_FUSE_OFFSET', '1') != '0'
WINOGRAD = os.environ.get('CENTERTRACK_WINOGRAD', '1') != '0'
FUSE_PROJ = os.environ.get('CENTERTRACK_FUSE_PROJ', '1') != '0'       # Tree.project computed by the tree1.conv1 launch (round 4)


def _fold_bn(sd, p):
    """eval-mode BatchNorm -> (scale, shift): y = x*scale + shift  """
    scale = sd[p + '.weight'].double() / torch.sqrt(sd[p + '.running_var'].double() + BN_EPS)
    shift = sd[p + '.bias'].double() - sd[p + '.running_mean'].double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


def _wino(w):
    """Winograd F(2x2,3x3) form of a 3x3 weight the stride-1 layers may be run with (autotuner's choice)"""
    ok = WINOGRAD and w.shape[2] == 3 and w.shape[1] % 64 == 0
    return ops.pack_winograd(w) if ok else None


class _Launch(object):
    """One pre-built C-ABI call of the frame (`keep` pins the tensors its raw pointers refer to; `out`: the view or NCHW
    tensor it writes, None for a group launch)."""
    __slots__ = ('fn', 'args', 'name', 'keep', 'out', 'ws_need')

    def __init__(self, name, fn, args, keep=(), out=None, ws_need=0):
        self.name, self.fn, self.args, self.keep = name, fn, args, keep
        self.out, self.ws_need = out, ws_need


def _conv_launch(name, d, keep, out, dev, tune):
    """The _Launch of one ct_conv2d call: ``d`` is the filled ConvDesc, the autotuner (``tune``) picks its launch shape
    and the library says how much split-K workspace that shape wants (_share_conv_workspace hands it out)."""
    if tune:
        autotune.tune_conv(d, dev)
    return _Launch(name, 'conv', d, keep, out=out, ws_need=_lib.load().ct_conv2d_workspace_bytes(ctypes.byref(d)))


def _share_conv_workspace(launches, dev):
    """split-K partials of the dense convs: one workspace shared by all of them (the launches of a frame are
    sequential); every DCN layer owns its workspace (the layers of a group run concurrently)"""
    need = max([l.ws_need for l in launches if l.fn == 'conv'] + [16])
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    for l in launches:
        if l.fn == 'conv':
            l.args.workspace, l.args.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return ws


class _Builder(object):
    """What the stages of one plan build share: the launch list, the batch, the device, whether the autotuner runs."""

    def __init__(self, N, dev, tune):
        self.N, self.dev, self.tune, self.launches = N, dev, tune, []

    def alloc(self, h, w, c):
        return ops.new_view(self.N, h, w, c, self.dev)

    def conv(self, name, d, keep, out):
        self.launches.append(_conv_launch(name, d, keep, out, self.dev, self.tune))
        return out

    def conv_bn(self, name, x, pk, cout, ks, stride=1, relu=True, res=None, out=None, **kw):
        """conv + folded BN (+ residual, ReLU) of the trunk; ``pk`` = (packed weight, scale, shift, Winograd form)"""
        wp, sc, sh, ww = pk
        d = ops.make_conv_desc(x, wp, cout, ks, stride, scale=sc, shift=sh, res=res, relu=relu, out=out,
                               w_wino=(ww if stride == 1 else None), **kw)
        return self.conv(name, d, (x, res, out, pk, kw.get('pool'), kw.get('proj')), out)


# The views of one DeformConv node of the IDAUp tree (dla.py:506-518): input view, output view, the fused IDAUp step
# ``up`` = (weight, f, skip view, output view) of a `proj` node.  What the schedule makes of it is in dcn_schedule.Planned.
_DcnLayer = namedtuple('_DcnLayer', 'name x cout out up')


class DLASegHIP(torch.nn.Module):
    """Drop-in for the reference ``DLASeg(34, heads, head_convs, opt)`` at inference.  Its heads can be fine-tuned on the
    frozen trunk through ``heads.HeadFinetuner``; the trunk has no backward."""

    def __init__(self, heads, head_conv=256, pre_img=True, pre_hm=True, depth_scale=1.0,
                 model_output_list=False):
        super().__init__()
        self.heads = OrderedDict(heads)
        if isinstance(head_conv, dict):       # reference passes {head: [256]}
            vals = {tuple(v) if isinstance(v, (list, tuple)) else (v,) for v in head_conv.values()}
            assert len(vals) == 1 and len(next(iter(vals))) == 1, 'only one head-conv layer is supported'
            head_conv = next(iter(vals))[0]
        self.head_conv = head_conv
        self.pre_img, self.pre_hm = pre_img, pre_hm
        self.depth_scale = depth_scale
        self.model_output_list = model_output_list
        # parameters/buffers registered under the reference's names so state_dict() matches
        self._names = []
        for key, shape, kind in dla34_param_shapes(self.heads, head_conv, pre_img, pre_hm):
            if kind == 'bn':
                for suf, val in (('weight', 1.0), ('bias', 0.0), ('running_mean', 0.0), ('running_var', 1.0)):
                    self._reg(key + '.' + suf, torch.full(shape, val))
                self._reg(key + '.num_batches_tracked', torch.tensor(0, dtype=torch.long))
            else:
                self._reg(key, torch.zeros(shape))
        self._prepared = None
        self._plans = {}

    def _reg(self, name, t):
        self.register_buffer(name.replace('.', '__'), t)
        self._names.append(name)

    # --- state dict with the reference's dotted keys ---------------------------------
    def state_dict(self, *a, **k):
        return OrderedDict((n, getattr(self, n.replace('.', '__'))) for n in self._names)

    def load_state_dict(self, sd, strict=True):
        missing = [n for n in self._names if n not in sd]
        unexpected = [k for k in sd if k not in set(self._names)]
        if strict and (missing or unexpected):
            raise RuntimeError('missing %s unexpected %s' % (missing[:5], unexpected[:5]))
        for n in self._names:
            if n in sd:
                buf = getattr(self, n.replace('.', '__'))
                if tuple(buf.shape) != tuple(sd[n].shape):
                    raise RuntimeError('shape mismatch for %s: %s vs %s' % (n, tuple(buf.shape), tuple(sd[n].shape)))
                buf.copy_(sd[n])
        self._prepared = None
        self._plans = {}
        return missing, unexpected

    # --- one-time weight preparation ----------------------------------------------------
    def _prepare(self):
        if self._prepared is not None:
            return self._prepared
        dev = next(self.buffers()).device
        if dev.type != 'cuda':
            raise _lib.CTError('DLASegHIP runs on an MI355X only: call .to("cuda") first (no CPU fallback)')
        _lib.load()
        sd = {k: v.to(dev) for k, v in self.state_dict().items()}
        P = {}

        def conv_bn(wkey, bnkey):
            sc, sh = _fold_bn(sd, bnkey)
            return ops.pack_weight(sd[wkey]), sc, sh, _wino(sd[wkey])

        P['stem_w'] = [sd['base.base_layer.0.weight'].contiguous(),
                       sd['base.pre_img_layer.0.weight'].contiguous() if self.pre_img else None,
                       sd['base.pre_hm_layer.0.weight'].contiguous() if self.pre_hm else None]
        sc3 = torch.ones(3, 16, device=dev)
        sh3 = torch.zeros(3, 16, device=dev)
        for i, (name, on) in enumerate((('base_layer', True), ('pre_img_layer', self.pre_img),
                                        ('pre_hm_layer', self.pre_hm))):
            if on:
                sc3[i], sh3[i] = _fold_bn(sd, 'base.%s.1' % name)
        P['stem_scale'], P['stem_shift'] = sc3.contiguous(), sh3.contiguous()
        P['level0'] = conv_bn('base.level0.0.weight', 'base.level0.1')
        P['level1'] = conv_bn('base.level1.0.weight', 'base.level1.1')

        def leaf(p, cin, cout):
            d = {'c11': conv_bn(p + '.tree1.conv1.weight', p + '.tree1.bn1'),
                 'c12': conv_bn(p + '.tree1.conv2.weight', p + '.tree1.bn2'),
                 'c21': conv_bn(p + '.tree2.conv1.weight', p + '.tree2.bn1'),
                 'c22': conv_bn(p + '.tree2.conv2.weight', p + '.tree2.bn2'),
                 'root': conv_bn(p + '.root.conv.weight', p + '.root.bn')}
            if cin != cout:
                d['proj'] = conv_bn(p + '.project.0.weight', p + '.project.1')
            return d

        for i in range(2, 6):
            p = 'base.level%d' % i
            if LEVELS[i] == 1:
                P[p] = leaf(p, CHANNELS[i - 1], CHANNELS[i])
            else:
                P[p + '.tree1'] = leaf(p + '.tree1', CHANNELS[i - 1], CHANNELS[i])
                P[p + '.tree2'] = leaf(p + '.tree2', CHANNELS[i], CHANNELS[i])

        def deform(p):
            sc, sh = _fold_bn(sd, p + '.actf.0')
            sh = (sd[p + '.conv.bias'].double() * sc.double() + sh.double()).float().contiguous()
            return {'w': ops.pack_weight(sd[p + '.conv.weight']), 'scale': sc, 'shift': sh,
                    'w_off': ops.pack_weight(sd[p + '.conv.conv_offset_mask.weight']),
                    'w_off_wino': _wino(sd[p + '.conv.conv_offset_mask.weight']),
                    'b_off': sd[p + '.conv.conv_offset_mask.bias'].contiguous()}

        for p, n in (('dla_up.ida_0', 1), ('dla_up.ida_1', 2), ('dla_up.ida_2', 3), ('ida_up', 2)):
            for k in range(1, n + 1):
                P['%s.proj_%d' % (p, k)] = deform('%s.proj_%d' % (p, k))
                P['%s.node_%d' % (p, k)] = deform('%s.node_%d' % (p, k))
                P['%s.up_%d' % (p, k)] = ops.upsample_weight(sd['%s.up_%d.weight' % (p, k)])
        self._prepared = P
        return P

    # --- head weights: packed the first time a plan asks for them -----------------------------------------
    def _packed(self, kind, names):
        """``_pack_<kind>`` of the heads ``names``, cached in the prepared dict under (kind, names): a trunk-only plan
        (heads.HeadFinetuner) packs no head weights, and load_state_dict / HeadFinetuner.commit() drop the packings
        with the dict."""
        P = self._prepare()
        key = (kind, tuple(names))
        if key not in P:
            P[key] = getattr(self, '_pack_' + kind)(self.state_dict(), list(names))
        return P[key]

    def _pack_first(self, sd, names):
        """(packed weight, Winograd form, bias) of the first layers of ``names``: they share their input -> one
        64 -> head_conv * len(names) conv"""
        w0 = torch.cat([sd[h + '.0.weight'] for h in names], 0)
        return ops.pack_weight(w0), _wino(w0), torch.cat([sd[h + '.0.bias'] for h in names], 0).contiguous()

    def _pack_tail(self, sd, names):
        """(packed weight, bias) of the 1x1 output layer of one head"""
        h, = names
        return ops.pack_weight(sd[h + '.2.weight']), sd[h + '.2.bias'].contiguous()

    def _pack_block_diag(self, sd, names):
        """(packed weight, bias) of all second (1x1) layers as ONE block-diagonal head_conv*nh -> sum(c) conv: a single
        launch reads the intermediate once and writes every head into channel slices of one NCHW tensor"""
        w2 = torch.block_diag(*[sd[h + '.2.weight'][:, :, 0, 0] for h in names])[:, :, None, None].contiguous()
        return ops.pack_weight(w2), torch.cat([sd[h + '.2.bias'] for h in names], 0).contiguous()

    def _pack_fused(self, sd, names):
        """(w0 Winograd-packed, b0, w2 [n,8,256], b2 [n,8]) of ct_heads_fused for the heads ``names``"""
        hc = self.head_conv
        dev = sd[names[0] + '.2.weight'].device
        w0s = torch.cat([sd[h + '.0.weight'] for h in names], 0)
        w2s = torch.zeros((len(names), 8, hc), device=dev)
        b2s = torch.zeros((len(names), 8), device=dev)
        for i, h in enumerate(names):
            c = self.heads[h]
            w2s[i, :c] = sd[h + '.2.weight'].reshape(c, hc)
            b2s[i, :c] = sd[h + '.2.bias']
        return (ops.pack_winograd(w0s), torch.cat([sd[h + '.0.bias'] for h in names], 0).contiguous(),
                w2s.contiguous(), b2s.contiguous())

    def _pack_point(self, sd, names):
        """one sparse head (_point_heads): direct-form packed conv3x3 weights (the Winograd form has no single-pixel
        evaluation), hidden bias, [c, 256] output layer, output bias"""
        h, = names
        c, hc = self.heads[h], self.head_conv
        return (ops.pack_weight(sd[h + '.0.weight']), sd[h + '.0.bias'].contiguous(),
                sd[h + '.2.weight'].reshape(c, hc).contiguous(), sd[h + '.2.bias'].contiguous())

    def _dense_split(self):
        """(small, big): heads with <= 8 output channels go into ONE launch for conv3x3 + ReLU + conv1x1 of all of them
        (ct_heads_fused: Winograd, head_conv 256); the remaining (wide) heads keep the two-launch form on their own
        channels.  ('hm_hp' stays out whatever its width: ct_heads_fused has ONE sigmoid range, taken by 'hm'; the
        per-head 1x1 tail applies hm_hp's sigmoid, detector.py:300-304)"""
        ok = WINOGRAD and self.head_conv == 256
        small = [h for h, c in self.heads.items() if ok and c <= 8 and h != 'hm_hp'][:_lib.CT_MAX_FUSED_HEADS]
        return small, [h for h in self.heads if h not in small]

    def _point_heads(self):
        """sparse heads (round 5, opt-in): the heads that can be evaluated at single pixels -- the regression heads the
        decode only reads at the K winners, hps and the joint offset head of the pose task; head_conv 256 only"""
        return [h for h in self.heads if self.head_conv == 256 and (h in _lib.HEAD_INDEX or h in ('hps', 'hp_offset'))]

    def _winner_heads(self, feat):
        """``plan['sparse']``: the regression heads ct_decode evaluates at the K winners (ct_sparse_heads_desc), None if there
        are none.  Dead heads are left out: generic_decode overwrites the wh box with the ltrb / ltrb_amodal box
        (decode.py:131-139,150-159) and `reg` only feeds the wh box (decode.py:102-110) -- neither reaches the returned dict,
        so with the MOT head set (opts.py:343-359 + --ltrb_amodal) they are not evaluated at all"""
        sp = [h for h in self._point_heads() if h in _lib.HEAD_INDEX]
        if {'ltrb', 'ltrb_amodal'} & set(self.heads):
            sp = [h for h in sp if h not in ('reg', 'wh')]
        heads = [(h,) + self._packed('point', [h]) for h in sp]
        return {'feat': feat, 'heads': heads, 'depth_scale': self.depth_scale} if sp else None

    # --- the plan: every launch of a frame, built in stages ------------------------------------------------
    def _build_plan(self, N, H, W, with_img, with_hm, fuse_sigmoid, sparse_heads=False, sparse_pose=False, *, trunk_only=False):
        """``sparse_pose`` (opt-in, pose head sets): hm and hm_hp are the only dense head launches; reg / wh or ltrb / tracking
        go to ``plan['sparse']`` like ``sparse_heads``, hps and the offset head to ``plan['sparse_pose']``.
        ``trunk_only``: the plan stops at ``plan['feat']``, the 64-channel feature map, and has no head launches
        (heads.HeadFinetuner trains the heads on it)"""
        P = self._prepare()
        dev = next(self.buffers()).device
        if H % 32 or W % 32:
            raise _lib.CTError('input %dx%d must be a multiple of 32 (reference pads to 32 too, opts.py:297)' % (H, W))
        b = _Builder(N, dev, autotune.enabled())
        # static inputs (copied into before each replay)
        x_in = torch.zeros((N, 3, H, W), device=dev)
        img_in = torch.zeros((N, 3, H, W), device=dev) if with_img else None
        hm_in = torch.zeros((N, 1, H, W), device=dev) if with_hm else None
        plan = {'launches': b.launches, 'inputs': (x_in, img_in, hm_in)}
        feats = self._plan_trunk(b, P, plan['inputs'], H, W)
        feat, plan['dcn_knobs'], plan['dcn_layers'] = self._plan_neck(b, P, feats, H, W)
        plan['feat'] = feat
        plan['sparse'], plan['sparse_pose'], plan['outputs'] = self._plan_heads(b, feat, fuse_sigmoid, sparse_heads,
                                                                               sparse_pose, trunk_only)
        ws = _share_conv_workspace(b.launches, dev)
        plan['ws'], plan['ws_need'] = [ws], ws.numel() * 4
        return plan

    def _plan_trunk(self, b, P, inputs, H, W):
        """The stems (dla.py:305-311, one launch), level0 / level1 and the four tree levels of DLA-34: returns the six
        level outputs."""
        x_in, img_in, hm_in = inputs
        s0 = b.alloc(H, W, 16)
        b.launches.append(_Launch('stem', 'stem', (x_in, img_in, hm_in, s0), out=s0))
        l0 = b.conv_bn('level0', s0, P['level0'], 16, 3, out=b.alloc(H, W, 16))
        l1 = b.conv_bn('level1', l0, P['level1'], 32, 3, stride=2, out=b.alloc(H // 2, W // 2, 32))
        feats = [l0, l1]
        for i in range(2, 6):
            x = feats[-1]
            p = 'base.level%d' % i
            cin, cout = CHANNELS[i - 1], CHANNELS[i]
            h, w = x.H // 2, x.W // 2
            out = b.alloc(h, w, cout)
            level_root = i >= 3
            if LEVELS[i] == 1:
                R = b.alloc(h, w, 2 * cout + (cin if level_root else 0))
                self._plan_leaf(b, p, x, P[p], cin, cout, 2, R, out, level_root=level_root)
            else:
                # Tree(levels=2): R2 = [y2 | y1 | bottom | x1]; the outer project is dead code (dla.py:218)
                R2 = b.alloc(h, w, 3 * cout + cin)
                bottom = R2.slice(2 * cout, cin)
                x1 = R2.slice(2 * cout + cin, cout)
                R1 = b.alloc(h, w, 2 * cout)
                self._plan_leaf(b, p + '.tree1', x, P[p + '.tree1'], cin, cout, 2, R1, x1, bottom=bottom, make_bottom=True)
                self._plan_leaf(b, p + '.tree2', x1, P[p + '.tree2'], cout, cout, 1, R2, out)
            feats.append(out)
        return feats

    def _plan_leaf(self, b, name, x, pk, cin, cout, stride, R, out, bottom=None, level_root=False, make_bottom=False):
        """Tree(levels=1).forward (dla.py:215-228) over the concat buffer R = [x2 | x1 | children].  ``bottom`` =
        Tree.downsample(x) (dla.py:207,217): a 2x2 max-pool that (round 3) tree1.conv1 -- the 3x3 stride-2 conv over
        the same x -- writes as a side output of its launch instead of a launch of its own (``make_bottom``: the
        caller owns the buffer and wants it filled here)."""
        h, w = x.H // stride, x.W // stride
        # round 4: Tree.project (conv1x1 + BN of the pooled input, dla.py:196-203,217-218) is a second output of the
        # tree1.conv1 launch -- same input patches, the pooling window is four taps of the 3x3 stride-2 window
        fuse_proj = FUSE_PROJ and stride == 2 and cin != cout
        if stride > 1 and bottom is None:
            if level_root:
                bottom = R.slice(2 * cout, cin)
                make_bottom = True
            elif not fuse_proj:
                bottom = b.alloc(h, w, cin)
                make_bottom = True
            # (else: the pooled tensor only feeds the projection and is never materialised)
        elif stride == 1:
            bottom = x
        pool = bottom if (stride > 1 and make_bottom) else None
        t = b.alloc(h, w, cout)
        x1 = R.slice(cout, cout)
        x2 = R.slice(0, cout)
        if fuse_proj:
            residual = b.alloc(h, w, cout)
            b.conv_bn(name + '.t1.conv1+project', x, pk['c11'], cout, 3, stride=stride, out=t, pool=pool,
                      proj=(pk['proj'][0], pk['proj'][1], pk['proj'][2], residual))
        else:
            b.conv_bn(name + '.t1.conv1', x, pk['c11'], cout, 3, stride=stride, out=t, pool=pool)
            if cin != cout:
                residual = b.conv_bn(name + '.project', bottom, pk['proj'], cout, 1, relu=False, out=b.alloc(h, w, cout))
            else:
                residual = bottom
        b.conv_bn(name + '.t1.conv2', t, pk['c12'], cout, 3, res=residual, out=x1)
        b.conv_bn(name + '.t2.conv1', x1, pk['c21'], cout, 3, out=t)
        b.conv_bn(name + '.t2.conv2', t, pk['c22'], cout, 3, res=x1, out=x2)
        return b.conv_bn(name + '.root', View(R.buf, R.c0, R.C), pk['root'], cout, 1, out=out)

    def _plan_neck(self, b, P, feats, H, W):
        """DLAUp.forward (dla.py:568-574) and the IDAUp of DLASeg.imgpre2feats (dla.py:631-640) over the level outputs:
        records the 16 DeformConv nodes, has them scheduled together and returns (the 64-channel feature view, the DCN
        schedule knobs, {node name: result view})."""
        dcn_layers, dcn_views = [], {}

        def deform(name, x, cout, out, up=None):
            """DeformConv.forward (dla.py:515-518): offset/mask conv -> DCNv2 -> BN -> ReLU; with ``up`` =
            (weight, f, skip view, output view) also the IDAUp step `up(.) + skip` (dla.py:543-545) that consumes a
            `proj` node.  Only recorded here, buffers as keys: the 16 nodes are scheduled together (dcn_schedule.plan)
            and materialised below (_schedule_dcn)."""
            dcn_layers.append(dcn_schedule.Layer(name, id(x.buf), x.C, x.H, x.W, cout, id(out.buf),
                                                 None if up is None else (up[1], id(up[2].buf), id(up[3].buf))))
            dcn_views[name] = _DcnLayer(name, x, cout, out, up)
            return out

        def ida(p, layers, startp, endp, o, up_f):
            """IDAUp.forward (dla.py:539-545)"""
            for i in range(startp + 1, endp):
                k = i - startp
                f = up_f[k]
                xi = layers[i]
                up = b.alloc(xi.H * f, xi.W * f, o)
                deform('%s.proj_%d' % (p, k), xi, o, b.alloc(xi.H, xi.W, o),
                       up=(P['%s.up_%d' % (p, k)], f, layers[i - 1], up))
                layers[i] = deform('%s.node_%d' % (p, k), up, o, b.alloc(up.H, up.W, o))

        layers = list(feats)                                   # DLAUp.forward, dla.py:568-574
        outs = [layers[-1]]
        ida('dla_up.ida_0', layers, 4, 6, 256, [1, 2]); outs.insert(0, layers[-1])
        ida('dla_up.ida_1', layers, 3, 6, 128, [1, 2, 2]); outs.insert(0, layers[-1])
        ida('dla_up.ida_2', layers, 2, 6, 64, [1, 2, 2, 2]); outs.insert(0, layers[-1])
        y = [outs[0], outs[1], outs[2]]                        # DLASeg.imgpre2feats, dla.py:631-640
        ida('ida_up', y, 0, 3, 64, [1, 2, 4])
        knobs, dcn_launches = self._tune_dcn_schedule(dcn_layers, dcn_views, b.N, H, W, b.dev, b.tune)
        b.launches.extend(dcn_launches)
        return y[-1], knobs, {v.name: (v.up[3] if v.up is not None else v.out) for v in dcn_views.values()}   # name -> result view

    def _plan_heads(self, b, feat, fuse_sigmoid, sparse_heads, sparse_pose, trunk_only):
        """Which heads are computed as maps and which at points: returns (``plan['sparse']``, ``plan['sparse_pose']``,
        the dense outputs) and appends the dense head launches (_plan_dense_heads)."""
        small, big = self._dense_split()
        point = self._point_heads()
        sparse = pose = None
        if sparse_pose:
            # hps is read at the K winners and the offset head at the K peaks of each joint map (decode.py:161-167, 21-28):
            # ct_decode_pose_sparse evaluates them there.  hm keeps the launch form of the sparse plans (fused, alone), hm_hp
            # its dense form (conv3x3 + 1x1 tail with the sigmoid), so winners and peaks are the dense path's
            hs = set(self.heads)
            if (sparse_heads or not {'hm', 'hps', 'hm_hp'} <= hs or 'ltrb_amodal' in hs or 'hps' not in point or not fuse_sigmoid
                    or 'hm' not in small or 'hm_hp' not in big):
                raise _lib.CTError('sparse pose heads need hm, hps and hm_hp heads with head_conv 256, no ltrb_amodal head '
                                   '(the match finds its gate box in the packed row) and the detector\'s fused epilogues')
            sparse = self._winner_heads(feat)
            off = 'hp_offset' if 'hp_offset' in hs else 'reg' if 'reg' in hs else None
            pose = {'feat': feat, 'hps': self._packed('point', ['hps']), 'off': self._packed('point', [off]) if off else None}
            small, big = ['hm'], ['hm_hp']
        if sparse_heads:
            # opt-in (detector only, never Module.forward): the regression heads the decode reads at the K winners are not
            # computed as maps -- ct_decode evaluates them at those pixels (ct_sparse_heads_desc)
            sparse = self._winner_heads(feat)
            if sparse is None or 'hm' not in self.heads or {'hps', 'hm_hp'} & set(self.heads) or not fuse_sigmoid:
                raise _lib.CTError('sparse heads need an hm head, regression heads with head_conv 256, no pose heads '
                                   'and the detector\'s fused epilogues')
            small = [h for h in small if not (h in _lib.HEAD_INDEX and h in point)]          # (the dead heads leave the dense launch too)
            if any(h in _lib.HEAD_INDEX and h in point for h in big):          # (more small heads than one fused launch holds: not with sparse heads)
                raise _lib.CTError('sparse heads: %s do not fit the fused-heads launch' % [h for h in big if h in point])
        if trunk_only:
            if sparse_heads or sparse_pose:
                raise _lib.CTError('a trunk-only plan has no heads, sparse or dense')
            return sparse, pose, OrderedDict()
        return sparse, pose, self._plan_dense_heads(b, feat, fuse_sigmoid, small, big)

    def _plan_dense_heads(self, b, feat, fuse_sigmoid, small, big):
        """Heads (base_model.py:24-65,86-90): every head of ``small`` in ONE ct_heads_fused launch (hidden 256-channel maps
        stay in the workgroups); the heads of ``big`` (80-class hm, hps, hm_hp; all of them without a fused launch) as one
        conv3x3 for all their first layers, then their 1x1 output layers."""
        N, dev, hc = b.N, b.dev, self.head_conv
        outputs = {}

        def channels(names, comb):
            """the outputs of ``names`` as channel-slice views of the combined tensor; returns ({head: channel range},
            the `sig` and the `dep` range of the launch that writes it).  'hm' takes the sigmoid range: there is one per
            launch, hm_hp -> its per-head tail"""
            rng, c0 = {}, 0
            for h in names:
                rng[h] = (c0, c0 + self.heads[h])
                outputs[h] = comb[:, c0:c0 + self.heads[h]]
                c0 += self.heads[h]
            on = rng if fuse_sigmoid else {}
            return rng, on.get('hm', (0, 0)), on.get('dep', (0, 0))

        if small:
            ctot = sum(self.heads[h] for h in small)
            comb = torch.empty((N, ctot, feat.H, feat.W), device=dev)
            hd = _lib.HeadsDesc()
            hd.x, hd.N, hd.H, hd.W, hd.Cin, hd.ldx = feat.ptr, N, feat.H, feat.W, feat.C, feat.ld
            pack = hs_w0, hs_b0, hs_w2, hs_b2 = self._packed('fused', small)
            hd.w0_winograd, hd.b0, hd.nheads = hs_w0.data_ptr(), hs_b0.data_ptr(), len(small)
            hd.w2, hd.b2, hd.out, hd.ctot = hs_w2.data_ptr(), hs_b2.data_ptr(), comb.data_ptr(), ctot
            hd.depth_scale = self.depth_scale
            rng, (hd.sig_lo, hd.sig_hi), (hd.dep_lo, hd.dep_hi) = channels(small, comb)
            for i, h in enumerate(small):
                hd.cout[i], hd.coff[i] = self.heads[h], rng[h][0]
            b.launches.append(_Launch('heads.fused[%s]' % ' + '.join(small), 'heads', hd, (feat, comb) + pack, out=comb))
        if big:
            wp, ww, b0 = pack = self._packed('first', big)
            mid = b.alloc(feat.H, feat.W, hc * len(big))
            b.conv('heads.0', ops.make_conv_desc(feat, wp, hc * len(big), 3, 1, shift=b0, relu=True, out=mid, w_wino=ww),
                   (feat, mid, pack), mid)
            ctot = sum(self.heads[h] for h in big)
            if big == list(self.heads) and ctot <= 32 and 'hm_hp' not in big:
                # every head is here (no fused launch, none evaluated at points) and they have few output channels (MOT 11,
                # KITTI 9, nuScenes 30): one block-diagonal conv over the whole intermediate
                comb = torch.empty((N, ctot, feat.H, feat.W), device=dev)
                _, sig, dep = channels(big, comb)
                wp, b2 = pack = self._packed('block_diag', big)
                b.conv('heads.2', ops.make_conv_desc(mid, wp, ctot, 1, 1, shift=b2, out_nchw=comb, sig=sig, dep=dep,
                                                     depth_scale=self.depth_scale), (mid, comb, pack), comb)
            else:
                # a wide head (COCO: 80 classes): the block-diagonal form would multiply its flops by the number of heads
                for j, h in enumerate(big):
                    outputs[h] = self._plan_head_tail(b, h, mid.slice(hc * j, hc), fuse_sigmoid)
        return OrderedDict((h, outputs[h]) for h in self.heads if h in outputs)

    def _plan_head_tail(self, b, h, hidden, fuse_sigmoid):
        """`heads.<h>.2`: the 1x1 output layer of one head over its ``hidden`` slice of the first layers' output, into
        an NCHW tensor of its own, with the head's own sigmoid / depth range"""
        c = self.heads[h]
        o = torch.empty((b.N, c, hidden.H, hidden.W), device=b.dev)
        wp, b2 = pack = self._packed('tail', [h])
        hsig = (0, c) if (fuse_sigmoid and h in ('hm', 'hm_hp')) else (0, 0)       # detector.py:300-304
        hdep = (0, c) if (fuse_sigmoid and h == 'dep') else (0, 0)
        d = ops.make_conv_desc(hidden, wp, c, 1, 1, shift=b2, out_nchw=o, sig=hsig, dep=hdep, depth_scale=self.depth_scale)
        return b.conv('heads.%s.2' % h, d, (hidden, o, pack), o)

    def run_stem_partial(self, x, pre_img, out):
        """the terms of the stem that do not depend on the tracker (dla.py:305-311: base_layer(x) + pre_img_layer(
        pre_img)) into the NHWC view ``out`` -- a detector runs this for frame t+1 while the host still associates
        frame t; ``_run_plan(..., stem_partial=out)`` then only adds the pre_hm term (bit-identical to one launch)"""
        P = self._prepare()
        lib = _lib.load()
        w = P['stem_w']
        rc = lib.ct_stem_forward_parts(x.data_ptr(), ops._p(pre_img), None, None, 0, x.shape[0], x.shape[2], x.shape[3],
                                       w[0].data_ptr(), ops._p(w[1]) if pre_img is not None else None, None,
                                       P['stem_scale'].data_ptr(), P['stem_shift'].data_ptr(), out.ptr, out.ld,
                                       _lib.stream_ptr())
        if rc != 0:
            _lib.check(rc, 'stem (x / pre_img terms)')

    def _run_plan(self, plan, inputs=None, stem_partial=None, launches=None):
        """Enqueue every launch of the plan on the current stream.  ``inputs`` = (x, pre_img, pre_hm) tensors to read
        instead of the plan's own static input buffers (a detector rotates its frame buffers so that the
        previous frame never has to be copied).  ``stem_partial``: NHWC view that already holds the x / pre_img terms
        of the stem (``run_stem_partial``): only the pre_hm term is computed, on top of it."""
        P = self._prepared
        lib = _lib.load()
        st = _lib.stream_ptr()
        for l in (plan['launches'] if launches is None else launches):      # (``launches``: a contiguous part of the plan, bench.py)
            if l.fn == 'conv':
                rc = lib.ct_conv2d(ctypes.byref(l.args), st)
            elif l.fn == 'dcn_group':
                arr, n, phases = l.args
                rc = lib.ct_dcn_v2_group(arr, n, phases, st)
            elif l.fn == 'heads':
                rc = lib.ct_heads_fused(ctypes.byref(l.args), st)
            elif l.fn == 'stem':
                x, img, hm, y = l.args
                if inputs is not None:
                    x, img, hm = inputs
                w = P['stem_w']
                if stem_partial is not None:
                    if hm is None:
                        raise _lib.CTError('a split stem needs the pre_hm input')
                    rc = lib.ct_stem_forward_parts(None, None, hm.data_ptr(), stem_partial.ptr, stem_partial.ld,
                                                   x.shape[0], x.shape[2], x.shape[3], None, None, w[2].data_ptr(),
                                                   P['stem_scale'].data_ptr(), P['stem_shift'].data_ptr(), y.ptr, y.ld, st)
                    if rc != 0:
                        _lib.check(rc, l.name)
                    continue
                rc = lib.ct_stem_forward(x.data_ptr(), ops._p(img), ops._p(hm), x.shape[0], x.shape[2], x.shape[3],
                                         w[0].data_ptr(), ops._p(w[1]) if img is not None else None,
                                         ops._p(w[2]) if hm is not None else None,
                                         P['stem_scale'].data_ptr(), P['stem_shift'].data_ptr(), y.ptr, y.ld, st)
            else:
                raise AssertionError(l.fn)
            if rc != 0:
                _lib.check(rc, l.name)

    # --- the 16 DeformConv nodes of DLAUp / IDAUp as grouped launches -------------------------------------
    def _schedule_dcn(self, layers, views, N, dev, knobs, tune=True):
        """Launch list of the 16 DCN nodes for one choice of ``knobs``: dcn_schedule.plan decides, this gives every
        planned layer its offset conv or `part` buffer, its ct_dcn_desc and its workspace, and every planned launch its
        _Launch.  ``views``: {layer name: _DcnLayer}."""
        lib = _lib.load()
        P = self._prepared
        sched = dcn_schedule.plan(layers, N, knobs, fuse_enabled=FUSE_OFFSET, winograd=WINOGRAD)
        descs, convs = {}, {}
        for name, p in sched.layers.items():
            pk = P[name]
            _, x, _, out, up = views[name]
            om = part = None
            if p.src in ('raw', 'map'):
                # a conv launch of this layer's own: 'raw' sums free to use the Winograd shapes (the bias and the mask
                # sigmoid are applied by the DCN launch), or the finished offset/mask map
                omv = ops.new_view(N, x.H, x.W, 32, dev)
                if p.src == 'raw':
                    part = omv.buf
                    d = ops.make_conv_desc(x, pk['w_off'], 27, 3, 1, out=omv, w_wino=pk['w_off_wino'])
                else:
                    om = omv
                    d = ops.make_conv_desc(x, pk['w_off'], 27, 3, 1, shift=pk['b_off'], out=om, sig=(18, 27))
                convs[name] = _conv_launch(name + '.offset', d, (x, omv, pk), omv, dev, tune)
            elif p.src != 'fused':                   # ('parts' / 'wino': written by the slot's OFFSETS launch)
                part = torch.empty((x.C // 64) * N * x.H * x.W * 32, dtype=torch.float32, device=dev)
            own = p.src != 'map'
            dd = ops.make_dcn_desc(x, om, pk['w'], p.layer.cout, pk['scale'], pk['shift'], True, out, up=up,
                                   split_k=p.splits, algo=3264, om_partial=part, raw_offsets=p.src == 'raw',
                                   w_off=pk['w_off'] if own else None, b_off=pk['b_off'] if own else None,
                                   w_off_wino=pk['w_off_wino'] if p.src == 'wino' else None)
            need_c = ctypes.c_size_t(0)
            _lib.check(lib.ct_dcn_v2_group_plan(ctypes.byref(dd), ctypes.byref(need_c), None), 'DCN layer ' + name)
            need = need_c.value
            if (need > 0) != p.use_ws:
                raise _lib.CTError('DCN layer %s: the library wants %d workspace bytes, the schedule planned %s'
                                   % (name, need, 'a workspace' if p.use_ws else 'none'))
            keep = [x, om, part, out, pk, up]
            if need:
                ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
                dd.workspace, dd.workspace_bytes = ws.data_ptr(), need
                keep.append(ws)
            descs[name] = (dd, keep)
        launches = []
        for l in sched.launches:
            if l.tag == 'conv':
                launches.append(convs[l.names[0]])
                continue
            arr = (_lib.DcnDesc * len(l.names))()
            for j, (name, algo) in enumerate(zip(l.names, l.algos)):
                ctypes.memmove(ctypes.byref(arr[j]), ctypes.byref(descs[name][0]), ctypes.sizeof(_lib.DcnDesc))
                arr[j].algo = algo
            launches.append(_Launch('%s[%s]' % (l.tag, ' + '.join(l.names)), 'dcn_group', (arr, len(l.names), l.phase),
                                    [descs[name][1] for name in l.names]))
        return launches

    def _time_launches(self, launches, reps=10):
        """device time (us) of a launch list, by graph replay on a side stream"""
        plan = {'launches': launches}
        ws = _share_conv_workspace(launches, next(self.buffers()).device)       # (alive until the timing is done)
        side =torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._run_plan(plan)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _lib.capture_guard(collect=False), torch.cuda.graph(g):
            for _ in range(reps):
                self._run_plan(plan)
        g.replay()
        torch.cuda.synchronize()
        best = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e3 / reps
            best = t if best is None else min(best, t)
        del g
        return best

    def _tune_dcn_schedule(self, layers, views, N, H, W, dev, tune):
        """Pick the knobs of the DCN schedule for this (batch, size) by timing the whole 16-node sequence (a HIP graph of
        exactly its launches) for every candidate of dcn_schedule.knob_grid; the choice is cached like the per-layer ones
        (pinned table / CENTERTRACK_TUNE_CACHE) because it fixes the fp32 summation order.  CENTERTRACK_DCN_KNOBS="a,b,c"
        forces one."""
        env = os.environ.get('CENTERTRACK_DCN_KNOBS', '')
        if env:
            knobs = tuple(int(v) for v in env.split(','))
            return knobs, self._schedule_dcn(layers, views, N, dev, knobs, tune)
        if not tune:
            knobs = (128, 4, 2, 1, 0, 0, 0)
            return knobs, self._schedule_dcn(layers, views, N, dev, knobs, tune)
        # dcnplan4: tables before the persistent launches (six knobs); dcnplan3: four knobs, no fine-split slots
        key, older = 'dcnplan5:%d,%d,%d' % (N, H, W), ('dcnplan4:%d,%d,%d' % (N, H, W), 'dcnplan3:%d,%d,%d' % (N, H, W))
        autotune._load_file()
        if os.environ.get('CENTERTRACK_DCN_RETUNE', '0') != '1':           # (tools/retune_dcn.py: measure again)
            for k in (key,) + older:
                if k in autotune._CACHE:
                    knobs = dcn_schedule.normalize(autotune._CACHE[k][:-1])
                    return knobs, self._schedule_dcn(layers, views, N, dev, knobs)
        verbose = os.environ.get('CENTERTRACK_TUNE_VERBOSE')
        best = None
        tried = []
        for knobs in dcn_schedule.knob_grid(layers, N):
            launches = self._schedule_dcn(layers, views, N, dev, knobs)
            us = self._time_launches(launches)
            if verbose:
                print('dcn schedule N=%d %dx%d knobs %s: %d launches, %.1f us' % (N, H, W, knobs, len(launches), us))
            tried.append((us, knobs))
            if best is None or us < best[0]:
                best = (us, knobs)
            del launches
        # second stage (dcn_schedule.persist_candidates), off unless CENTERTRACK_DCN_TUNE_PERSIST=1
        stage2 = os.environ.get('CENTERTRACK_DCN_TUNE_PERSIST', '0') == '1'
        for us0, knobs in dcn_schedule.persist_candidates(tried) if stage2 else ():
            launches = self._schedule_dcn(layers, views, N, dev, knobs)
            if any(l.fn == 'dcn_group' and int(l.args[0][0].algo) >= 50000 for l in launches):
                us = self._time_launches(launches)
                if verbose:
                    print('dcn schedule N=%d %dx%d knobs %s: %d launches, %.1f us (%.1f without)' % (N, H, W, knobs, len(launches), us, us0))
                if us < best[0]:
                    best = (us, knobs)
            del launches
        autotune._CACHE[key] = tuple(best[1]) + (round(best[0], 1),)
        autotune._save_file()
        return best[1], self._schedule_dcn(layers, views, N, dev, best[1])

    @staticmethod
    def plan_signature(plan):
        """Everything of a plan that fixes the fp32 summation order, as one string: per launch its name, kernel choice
        (algo) and split-K, the per-layer DCN tile / split / offset mode, the DCN schedule knobs.  Ranks of a multi-GPU
        job compare its hash (parallel.check_same_plan) before they start."""
        parts = ['dcn_knobs=%s' % (tuple(plan.get('dcn_knobs', ())),)]
        for l in plan['launches']:
            if l.fn == 'conv':
                parts.append('%s:conv:%d:%d' % (l.name, int(l.args.algo), int(l.args.split_k)))
            elif l.fn == 'dcn_group':
                arr, n, phases = l.args
                parts.append('%s:dcn:%d:%s' % (l.name, phases, ','.join(
                    '%d/%d/%d' % (int(arr[j].algo), int(arr[j].split_k), int(arr[j].fuse_offset)) for j in range(n))))
            else:
                parts.append('%s:%s' % (l.name, l.fn))
        return ';'.join(parts)

    def get_plan(self, N, H, W, with_img, with_hm, fuse_sigmoid=False, sparse_heads=False, *, trunk_only=False, sparse_pose=False):
        key = (N, H, W, with_img, with_hm, fuse_sigmoid, sparse_heads, trunk_only) + (('sparse_pose',) if sparse_pose else ())
        if key not in self._plans:
            self._plans[key] = self._build_plan(*key[:7], sparse_pose, trunk_only=trunk_only)
        return self._plans[key]

    def forward_plan(self, plan, x, pre_img=None, pre_hm=None):
        """Copy the inputs into the plan's static buffers and enqueue all launches."""
        xi, ii, hi = plan['inputs']
        xi.copy_(x)
        if ii is not None:
            ii.copy_(pre_img)
        if hi is not None:
            hi.copy_(pre_hm)
        self._run_plan(plan)
        return plan['outputs']

    @torch.no_grad()
    def forward(self, x, pre_img=None, pre_hm=None, fuse_sigmoid=False):
        """Reference signature (base_model.py:73): returns ``[ {head: tensor[B,c,h,w]} ]``
        (raw logits unless ``fuse_sigmoid``, in which case hm / dep carry the transforms of
        ``Detector._sigmoid_output``, detector.py:300-308).  Outputs are fresh tensors."""
        if pre_img is not None and not self.pre_img:
            raise _lib.CTError('model was built with pre_img=False')
        if pre_hm is not None and not self.pre_hm:
            raise _lib.CTError('model was built with pre_hm=False')
        N, _, H, W = x.shape
        plan = self.get_plan(N, H, W, pre_img is not None, pre_hm is not None, fuse_sigmoid)
        out = self.forward_plan(plan, x, pre_img, pre_hm)
        z = OrderedDict((k, v.clone()) for k, v in out.items())
        if self.model_output_list:
            return [[z[h] for h in sorted(self.heads)]]
        return [z]


def create_model(arch, head, head_conv, opt=None):
    """reference model.py:24-29; only the published architecture ``dla_34`` exists here."""
    if arch != 'dla_34':
        raise ValueError('centertrack_amd implements arch "dla_34" only (got %r)' % arch)
    if opt is not None and getattr(opt, 'dla_node', 'dcn') != 'dcn':
        raise ValueError('only dla_node="dcn" is implemented')
    if opt is not None and getattr(opt, 'head_kernel', 3) != 3:
        raise ValueError('only head_kernel=3 is implemented')
    return DLASegHIP(head, head_conv,
                     pre_img=getattr(opt, 'pre_img', True) if opt is not None else True,
                     pre_hm=getattr(opt, 'pre_hm', True) if opt is not None else True,
                     depth_scale=getattr(opt, 'depth_scale', 1.0) if opt is not None else 1.0,
                     model_output_list=getattr(opt, 'model_output_list', False) if opt is not None else False)


def load_model(model, model_path, opt=None, optimizer=None):
    """reference model.py:31-90: ``{'epoch', 'state_dict'[, 'optimizer']}`` checkpoint, ``module.`` prefix
    stripped, unknown keys dropped, missing keys keep their initialisation; a parameter whose shape differs -- or,
    under ``opt.reset_hm``, an ``hm*`` parameter with 80 / 1 rows -- is skipped, or with ``opt.reuse_hm`` cut /
    padded along its first axis (a COCO-pretrained heat-map head reused for another class count, model.py:49-63).
    With an ``optimizer`` it returns ``(model, optimizer, start_epoch)`` as the reference does (below)."""
    ckpt = torch.load(model_path, map_location='cpu')
    sd_in = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt
    if 'epoch' in ckpt:
        print('loaded {}, epoch {}'.format(model_path, ckpt['epoch']))
    sd = {}
    for k, v in sd_in.items():
        sd[k[7:] if k.startswith('module') and not k.startswith('module_list') else k] = v
    own = model.state_dict()
    reset_hm = bool(getattr(opt, 'reset_hm', False))
    reuse_hm = bool(getattr(opt, 'reuse_hm', False))
    keep = {}
    for k, v in sd.items():
        if k in own:
            mismatch = tuple(v.shape) != tuple(own[k].shape)
            if mismatch or (reset_hm and k.startswith('hm') and v.shape[0] in (80, 1)):
                if reuse_hm and tuple(v.shape[1:]) == tuple(own[k].shape[1:]):
                    print('Reusing parameter {}, required shape{}, loaded shape{}.'.format(
                        k, tuple(own[k].shape), tuple(v.shape)))
                    n = min(v.shape[0], own[k].shape[0])      # (the reference only ever cuts: `a < a` is never true)
                    merged = own[k].clone()
                    merged[:n] = v[:n]
                    keep[k] = merged
                else:
                    print('Skip loading parameter {}, required shape{}, loaded shape{}.'.format(
                        k, tuple(own[k].shape), tuple(v.shape)))
            else:
                keep[k] = v
        else:
            print('Drop parameter {}.'.format(k))
    for k in own:
        if k not in keep:
            print('No param {}.'.format(k))
    model.load_state_dict(keep, strict=False)
    if optimizer is None:
        return model
    # the resume branch, model.py:73-90.  Like the reference it does NOT load the optimizer state (that line is commented
    # out there): it takes the epoch and restarts the learning rate -- opt.lr times 0.1 once per passed lr_step, one
    # multiplication after the other, which in floating point is not main.py's opt.lr * 0.1 ** k.
    start_epoch = 0
    if getattr(opt, 'resume', False):
        if 'optimizer' in ckpt:
            start_epoch = ckpt['epoch']
            start_lr = opt.lr
            for step in opt.lr_step:
                if start_epoch >= step:
                    start_lr *= 0.1
            for param_group in optimizer.param_groups:
                param_group['lr'] = start_lr
            print('Resumed optimizer with start lr', start_lr)
        else:
            print('No optimizer parameters in checkpoint.')
    return model, optimizer, start_epoch


def save_model(path, epoch, model, optimizer=None):
    """reference model.py:92-101: ``{'epoch', 'state_dict'[, 'optimizer']}``"""
    if isinstance(model, torch.nn.DataParallel):
        state_dict = model.module.state_dict()
    else:
        state_dict = model.state_dict()
    data = {'epoch': epoch, 'state_dict': state_dict}
    if optimizer is not None:
        data['optimizer'] = optimizer.state_dict()
    torch.save(data, path)
