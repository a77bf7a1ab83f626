"""GPU: sparse pose heads (opt.sparse_pose_heads, ct_decode_pose_sparse; opt-in).  ``hps`` is evaluated at the K winners and the
joint offset head at the K peaks of every joint heat-map instead of as dense maps: the values against a float64 evaluation
of the same heads, the match behind them bit for bit against the dense ct_decode_pose fed with those very values, and the
detector against its dense self and against the oracle."""
import numpy as np
import pytest
import torch

import _sparse_heads as SH
import _sparse_pose as SP
from _dcn_bwd import bound
from _guards import NAN

pytestmark = pytest.mark.gpu


def _feature_view(feat, c0, pad, device):
    """``feat`` [N,64,h,w] as the channel slice [c0, c0 + 64) of an NHWC buffer of pitch c0 + 64 + pad, NaN everywhere else"""
    from centertrack_amd import ops
    N, _, h, w = feat.shape
    buf = torch.full((N, h, w, c0 + 64 + pad), NAN)
    buf[..., c0:c0 + 64] = feat.permute(0, 2, 3, 1)
    return ops.View(buf.to(device), c0, 64)


class _Run(object):
    """one case on the device: the sparse decoder's rows and compact values, the winners, the joint peaks taken independently.
    The feature map is a slice between NaN channels; the decoder runs once on its own zeroed workspace and once on the same
    workspace filled with NaN from end to end -- ct_decode_pose_sparse reads no byte of it that the call has not written -- and
    what is kept is the second run's (``zeroed``: rows and values of the first)."""

    def __init__(self, c, device, d=None):
        from centertrack_amd import ops
        self.c, self.d = c, SP.make_case(c) if d is None else d
        d = self.d
        dev = lambda t: t.to(device).contiguous()
        pack = lambda wts: (ops.pack_weight(dev(wts[0])), dev(wts[1]), dev(wts[2]), dev(wts[3]))
        self.hm, self.hm_hp = dev(d['hm']), dev(d['hm_hp'])
        self.maps = {k: dev(v) for k, v in d['maps'].items()}
        self.sparse_pose = {'feat': _feature_view(d['feat'], c.c0, c.pad, device), 'hps': pack(d['hps']),
                            'off': pack(d['off']) if d['off'] is not None else None, 'flip': c.flip, 'flip_pairs': c.pairs}
        self.dec = ops.Decoder(self.hm, dict(self.maps, hm_hp=self.hm_hp), c.K, sparse_pose=self.sparse_pose)
        assert self.dec.pose_ws.numel() * 8 >= SH.pose_workspace_bytes(c)
        self.zeroed = self._values(self.dec.run().cpu().numpy().copy())
        self.dec.pose_ws.view(torch.float32).fill_(NAN)
        self.dec.out.fill_(NAN)
        self.rows = self.dec.run().cpu().numpy().copy()
        self.hps, self.off = self._values(self.rows)[1:]
        self.ws = self.dec.pose_ws.view(torch.float32).cpu().clone()
        self.inds = self.dec.inds.cpu().clone()
        self._joint_peaks(device)

    def _values(self, rows):
        hps, off = self.dec.pose_values()
        return rows, hps.cpu().clone(), off.cpu().clone() if off is not None else None

    def part(self, name):
        """a part of the workspace after the run, by the carve of tests/_sparse_heads.py, as float32"""
        at, n = SH.pose_carve(self.c)[0][name]
        return self.ws[at // 4:(at + n) // 4]

    def _joint_peaks(self, device):
        from centertrack_amd import ops
        c = self.c
        jdec = ops.Decoder(self.hm_hp.view(c.B * c.J, 1, c.h, c.w), {}, c.K)          # decode.py:21: _topk_channel, on its own
        jdec.run()
        self.jinds = jdec.inds.cpu().clone()
        self.jscores = jdec.out[..., 0].cpu().clone()


_runs = {}


def _run(c, device):
    if c.name not in _runs:
        _runs[c.name] = _Run(c, device)
    return _runs[c.name]


def _report(what, got, ref64, ref32):
    norm = float(ref64.abs().max())
    e32 = float((ref32.double() - ref64).abs().max()) / norm
    err = float((got.double() - ref64).abs().max()) / norm
    b = bound(e32, SP.K_TERMS)
    print('%s: err %.3g, float32 reference %.3g, bound %.3g, ratio %.3f' % (what, err, e32, b, err / b))
    return err, b


@pytest.mark.parametrize('c', SP.CASES, ids=[c.name for c in SP.CASES])
def test_compact_values_against_float64(device, c):
    """hps at the winners (merged under flip) and the offset head at the joint peaks against the same heads evaluated in
    float64 on the CPU, relative to the head's largest value; the bound is the project's: 4 x the larger of the float32
    CPU evaluation's own error and 2^-23 sqrt(832).  Winners and peaks sit on the borders the case lifts."""
    r = _run(c, device)
    d = r.d
    x, y = r.inds % c.w, r.inds // c.w
    assert (y == 0).any() and (r.jinds % c.w == c.w - 1).any() and (r.jinds % c.w == 0).any(), \
        'a winner on row 0 and peaks on the first and the last column'
    if c.K >= 20:
        assert (x == 0).any() and (x == c.w - 1).any(), 'winners on both columns: under flip each reads the other border'
    # the slice sits between NaN channels and the workspace was NaN from end to end: finite means neither was read
    assert np.isfinite(r.rows).all() and bool(torch.isfinite(r.hps).all()) and (r.off is None or bool(torch.isfinite(r.off).all()))
    np.testing.assert_array_equal(r.rows.view(np.int32), r.zeroed[0].view(np.int32))
    assert torch.equal(r.hps.view(torch.int32), r.zeroed[1].view(torch.int32))
    assert r.off is None or torch.equal(r.off.view(torch.int32), r.zeroed[2].view(torch.int32))
    ref = [SP.hps_at_winners(d['feat'], d['hps'], c.B, r.inds, c.flip, c.pairs, t) for t in (torch.float64, torch.float32)]
    err, b = _report('%s hps' % c.name, r.hps.view(-1, 2 * c.J), *ref)
    assert err <= b
    if c.offset:
        ref = [SP.offsets_at_peaks(d['feat'], d['off'], c.B, c.J, r.jinds, t) for t in (torch.float64, torch.float32)]
        err, b = _report('%s offsets' % c.name, r.off.view(-1, 2), *ref)
        assert err <= b
        # a pixel that is a peak of several joints of an image: one value, bit for bit, wherever it stands in the list
        key = (torch.arange(c.B * c.J) // c.J).view(-1, 1) * (c.h * c.w) + r.jinds
        order = torch.argsort(key.reshape(-1), stable=True)
        ks, vs = key.reshape(-1)[order], r.off.view(-1, 2)[order]
        same = ks[1:] == ks[:-1]
        assert int(same.sum()) > 0 or c.J == 1 or c.K == 1           # (one joint, or one peak per joint: no pixel twice)
        assert torch.equal(vs[1:][same].view(torch.int32), vs[:-1][same].view(torch.int32))
    else:
        assert r.off is None


@pytest.mark.parametrize('c', SP.CASES, ids=[c.name for c in SP.CASES])
def test_rows_equal_the_dense_match_on_the_same_values(device, c):
    """plumbing, exact: the kernel's own compact values scattered into otherwise-zero hps / offset maps at the winner and peak
    pixels (the peaks taken by an independent decode of hm_hp), through the dense ct_decode_pose with the same box maps ->
    the same packed rows, key points and kps_score, bit for bit"""
    from centertrack_amd import ops
    r = _run(c, device)
    HW = c.h * c.w
    hps = torch.zeros((c.B, HW, 2 * c.J))
    hps[torch.arange(c.B).view(-1, 1), r.inds] = r.hps
    heads = dict(r.maps, hm_hp=r.hm_hp, hps=hps.permute(0, 2, 1).reshape(c.B, 2 * c.J, c.h, c.w).contiguous().to(device))
    if c.offset:
        off = torch.zeros((c.B, HW, 2))
        off[(torch.arange(c.B * c.J) // c.J).view(-1, 1), r.jinds] = r.off
        heads['hp_offset'] = off.permute(0, 2, 1).reshape(c.B, 2, c.h, c.w).contiguous().to(device)
    dense = ops.Decoder(r.hm, heads, c.K)
    want = dense.run().cpu().numpy()
    assert dense.layout == r.dec.layout and want.shape == r.rows.shape
    np.testing.assert_array_equal(r.rows.view(np.int32), want.view(np.int32))
    got = r.dec.unpack(r.rows)
    kps = r.hps.numpy().copy()
    kps[..., 0::2] += got['xs'][..., None]
    kps[..., 1::2] += got['ys'][..., None]
    snapped = kps != got['hps']
    weak = SP.weak_joint(c)
    others = snapped[..., 0::2]
    if weak is not None:
        assert not snapped[..., 2 * weak:2 * weak + 2].any()
        others = np.delete(others, weak, axis=-1)
    if others.size >= 100:          # (fewer joints than that cannot be asked to fall on both sides)
        assert snapped.any()
        assert 0.05 < others.mean() < 0.98, 'the gate box must decide both ways (%.2f snapped)' % others.mean()


def test_two_runs_give_the_same_bits(device):
    c = SP.CASES[1]
    r = _run(c, device)
    again = r.dec.run().cpu().numpy()
    np.testing.assert_array_equal(again.view(np.int32), r.rows.view(np.int32))
    fresh = _Run(c, device)
    np.testing.assert_array_equal(fresh.rows.view(np.int32), r.rows.view(np.int32))
    assert torch.equal(fresh.hps.view(torch.int32), r.hps.view(torch.int32))
    assert torch.equal(fresh.off.view(torch.int32), r.off.view(torch.int32))


def test_the_same_patch_gives_the_same_bits_in_another_image(device):
    """image 1 a copy of image 0 (features of both halves under flip, hm, hm_hp): the same winners and peaks stand K (37: another
    row of another tile) and J*K places further down the point lists, and carry the same hps and offset bits"""
    c = SP.CASE['b2_reg_wh_flip']
    d = dict(SP.make_case(c))
    for k in ('feat', 'hm', 'hm_hp'):
        d[k] = d[k].clone()
    d['feat'][1], d['feat'][c.B + 1] = d['feat'][0], d['feat'][c.B]
    d['hm'][1], d['hm_hp'][1] = d['hm'][0], d['hm_hp'][0]
    r = _Run(c, device, d)
    assert torch.equal(r.inds[0], r.inds[1]) and torch.equal(r.jinds[:c.J], r.jinds[c.J:])
    hps, off = r.hps.view(c.B, c.K, 2 * c.J), r.off.view(c.B, c.J * c.K, 2)
    assert torch.equal(hps[0].view(torch.int32), hps[1].view(torch.int32))
    assert torch.equal(off[0].view(torch.int32), off[1].view(torch.int32))
    assert (c.K % 16) and (c.J * c.K) % 16


@pytest.mark.parametrize('name', ['b2_reg_wh_flip', 'k1_three_jobs', 'j4_overlapping_pairs_slice'])
def test_three_jobs_in_one_launch_give_the_bits_of_each_job_alone(device, name):
    """the partial sums of a job do not depend on where its tiles start in the launch: hps in image b (ph0) against the case
    without flip and without the offset head -- one job --, the offset head (po) against the case without flip, where its
    job starts behind one hps job instead of two.  And pose_values_kernel restated on those partials in float32, operation
    for operation (quarters in order, + bias, the merge with the partner joint's pair, x negated): the compact values bit for
    bit, which also pins the partner table for pairs that share a joint."""
    c = SP.CASE[name]
    three = _run(c, device)
    assert len(SH.pose_jobs(c)[0]) == 3
    d = dict(SP.make_case(c))
    d['feat'] = d['feat'][:c.B]
    two = _Run(c._replace(flip=False), device, d)
    one = _Run(c._replace(flip=False, offset=None), device, dict(d, off=None))
    assert torch.equal(three.inds, one.inds) and torch.equal(three.inds, two.inds) and torch.equal(three.jinds, two.jinds)
    for part, other in (('ph0', one), ('ph0', two), ('po', two)):
        a, b = three.part(part), other.part(part)
        assert a.numel() > 0 and bool(torch.isfinite(a).all())
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), part
    BK, J2 = c.B * c.K, 2 * c.J
    quarters = lambda p, n: ((p.view(4, n)[0] + p.view(4, n)[1]) + p.view(4, n)[2]) + p.view(4, n)[3]
    b2 = three.d['hps'][3]
    v0 = (quarters(three.part('ph0'), BK * J2).view(BK, J2) + b2).view(BK, c.J, 2)
    v1 = (quarters(three.part('ph1'), BK * J2).view(BK, J2) + b2).view(BK, c.J, 2)
    partner = list(range(c.J))
    for u, v in c.pairs:
        partner[u], partner[v] = partner[v], partner[u]
    v1 = v1[:, partner] * torch.tensor([-1.0, 1.0])
    want = ((v0 + v1) * 0.5).view(BK, J2)
    assert torch.equal(three.hps.reshape(BK, J2).view(torch.int32), want.view(torch.int32))
    off = quarters(three.part('po'), BK * c.J * 2).view(-1, 2) + three.d['off'][3]
    assert torch.equal(three.off.reshape(-1, 2).view(torch.int32), off.view(torch.int32))
    assert torch.equal(one.hps.reshape(BK, J2).view(torch.int32), v0.reshape(BK, J2).view(torch.int32))


def _pose_model(heads):
    """the recipe of test_pose_tracking_stream_matches_oracle (tests/test_hip_e2e.py)"""
    from centertrack_amd import weights as W
    from centertrack_amd.model import DLASegHIP
    sd = W.make_synthetic_state_dict(heads, seed=21, hm_gain=14.0)
    sd['wh.2.bias'] = torch.full_like(sd['wh.2.bias'], 14.0)          # boxes wide enough for joints to snap
    sd['hps.2.weight'] = sd['hps.2.weight'] * 6
    model = DLASegHIP(heads)
    model.load_state_dict(sd)
    return sd, model


@pytest.mark.parametrize('flip', [False, True])
def test_sparse_pose_detector_against_dense_and_oracle(device, flip):
    """3 frames at 64x96: the winners and the track ids of the sparse detector are the dense detector's; key points and
    kps_score differ only where fp32 rounding flips a borderline snap (the allowance of the dense test against the oracle:
    at most 2 % of the coordinates off by more than 2e-2, kps_score to 2e-2); and the sparse detector passes that test's own
    assertions against the oracle"""
    from centertrack_amd import weights as W
    from centertrack_amd.detector import Detector, default_opt
    from centertrack_amd.image import make_meta
    from oracle import detector as odet
    heads = W.POSE_HEADS
    sd, model = _pose_model(heads)
    mk = lambda **kw: Detector(default_opt(heads, track_thresh=0.3, flip_test=flip, input_h=64, input_w=96, **kw), model=model)
    dense, det = mk(), mk(sparse_pose_heads=True)
    assert det.impl.sparse_pose and not dense.impl.sparse_pose and not det.impl.sparse and det.impl.native
    oopt = odet.default_opt(track_thresh=0.3, flip_test=flip, input_h=64, input_w=96, num_classes=1)
    oracle = odet.Detector(oopt, sd, heads)
    meta = make_meta(64, 96, 480, 720)
    g = torch.Generator().manual_seed(5)
    snapped = 0
    for t in range(3):
        img = torch.randn((1, 3, 64, 96), generator=g)
        rd = dense.run(img, dict(meta))
        ret = det.run(img, dict(meta))
        want = oracle.run(torch.cat((img, torch.flip(img, [3])), 0) if flip else img, dict(meta))
        dd, gd, od = dense.impl.last_dets, det.impl.last_dets, oracle.last_dets
        assert sorted(dd) == sorted(gd)
        for k in ('scores', 'xs', 'ys', 'clses'):
            np.testing.assert_array_equal(gd[k], dd[k], err_msg='frame %d %s' % (t, k))
        assert [int(r['tracking_id']) for r in ret['results']] == [int(r['tracking_id']) for r in rd['results']]
        bad = np.abs(gd['hps'] - dd['hps']) > 2e-2
        print('flip %s frame %d: %d of %d key-point coordinates differ from the dense detector\'s by more than 2e-2 (%.4f)'
              % (flip, t, bad.sum(), bad.size, bad.mean()))
        assert bad.mean() <= 0.02
        np.testing.assert_allclose(gd['kps_score'], dd['kps_score'], atol=2e-2)
        # against the oracle
        n = int((od['scores'][0] >= oopt.out_thresh).sum())
        assert n > 0 and len(want) > 0
        np.testing.assert_array_equal(gd['xs'][0, :n], od['xs'][0, :n])
        np.testing.assert_array_equal(gd['ys'][0, :n], od['ys'][0, :n])
        bad = np.abs(gd['hps'][0, :n] - od['hps'][0, :n]) > 2e-2
        assert bad.mean() <= 0.02, 'frame %d: %d of %d key-point coordinates differ' % (t, bad.sum(), bad.size)
        np.testing.assert_allclose(gd['kps_score'][0, :n], od['kps_score'][0, :n], atol=2e-2)
        assert [int(r['tracking_id']) for r in ret['results']] == [int(r['tracking_id']) for r in want]
        for a, b in zip(ret['results'], want):
            assert a['hps'].shape == (34,)
            assert np.mean(np.abs(a['hps'] - b['hps']) > 0.2) <= 0.1                  # image pixels (x7.5 the grid)
        reg = od['hps'][0, :n]
        snapped += int(np.sum(np.abs(reg - np.round(reg)) > 0))                        # (only a sanity count)
    assert snapped > 0
    plan = det.impl._ctx['plan']
    names = [l.name for l in plan['launches'] if l.fn == 'heads' or l.name.startswith('heads.')]
    assert plan['sparse'] is not None and plan['sparse_pose'] is not None
    assert names == ['heads.fused[hm]', 'heads.0', 'heads.hm_hp.2'], names
    assert sorted(plan['outputs']) == ['hm', 'hm_hp']
    assert [n for n, *_ in plan['sparse']['heads']] == ['reg', 'wh', 'tracking']


def test_the_flag_falls_back_to_dense_with_an_ltrb_amodal_head(device):
    """the gate box of the match is the wh / ltrb box; with an ltrb_amodal head the rows hold the amodal box instead and no map
    is left to rebuild it from: sparse_pose stays False and the dense path's results come back"""
    from collections import OrderedDict
    from centertrack_amd import weights as W
    from centertrack_amd.detector import StreamDetector, default_opt
    from centertrack_amd.image import make_meta
    heads = OrderedDict(list(W.POSE_HEADS.items()) + [('ltrb_amodal', 4)])
    sd, model = _pose_model(heads)
    mk = lambda **kw: StreamDetector(default_opt(heads, track_thresh=0.3, input_h=64, input_w=96, **kw), model=model, num_streams=1)
    dense, det = mk(), mk(sparse_pose_heads=True)
    assert not det.sparse_pose
    img = torch.randn((1, 3, 64, 96), generator=torch.Generator().manual_seed(5))
    meta = make_meta(64, 96, 480, 720)
    dense.step(img, [dict(meta)])
    det.step(img, [dict(meta)])
    assert det._ctx['plan'].get('sparse_pose') is None and 'hps' in det._ctx['plan']['outputs']
    for k, v in dense.last_dets.items():
        np.testing.assert_array_equal(det.last_dets[k], v, err_msg=k)
