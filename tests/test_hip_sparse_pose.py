"""GPU: sparse pose heads (opt.sparse_pose_heads, ct_decode_pose_sparse; opt-in).  ``hps`` is evaluated at the K winners and the
joint offset head at the K peaks of every joint heat-map instead of as dense maps: the values against a float64 evaluation
of the same heads, the match behind them bit for bit against the dense ct_decode_pose fed with those very values, and the
detector against its dense self and against the oracle."""
import numpy as np
import pytest
import torch

import _sparse_pose as SP
from _dcn_bwd import bound

pytestmark = pytest.mark.gpu


class _Run(object):
    """one case on the device: the sparse decoder's rows and compact values, the winners, the joint peaks taken independently"""

    def __init__(self, c, device):
        from centertrack_amd import ops
        self.c, self.d = c, SP.make_case(c)
        d = self.d
        dev = lambda t: t.to(device).contiguous()
        pack = lambda wts: (ops.pack_weight(dev(wts[0])), dev(wts[1]), dev(wts[2]), dev(wts[3]))
        self.hm, self.hm_hp = dev(d['hm']), dev(d['hm_hp'])
        self.maps = {k: dev(v) for k, v in d['maps'].items()}
        self.sparse_pose = {'feat': ops.view_from_nchw(dev(d['feat'])), 'hps': pack(d['hps']),
                            'off': pack(d['off']) if d['off'] is not None else None, 'flip': c.flip, 'flip_pairs': c.pairs}
        self.dec = ops.Decoder(self.hm, dict(self.maps, hm_hp=self.hm_hp), c.K, sparse_pose=self.sparse_pose)
        self.rows = self.dec.run().cpu().numpy().copy()
        hps, off = self.dec.pose_values()
        self.hps = hps.cpu().clone()
        self.off = off.cpu().clone() if off is not None else None
        self.inds = self.dec.inds.cpu().clone()
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
    assert (y == 0).any() and (r.jinds % c.w == c.w - 1).any(), 'a winner on row 0 and a peak on the last column'
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
        assert int(same.sum()) > 0
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
    assert snapped.any() and not snapped[..., 2 * SP.WEAK_JOINT:2 * SP.WEAK_JOINT + 2].any()
    others = np.delete(snapped[..., 0::2], SP.WEAK_JOINT, axis=-1)
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
