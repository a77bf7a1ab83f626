"""GPU: sparse heads (opt.sparse_heads, ct_sparse_heads_desc; round 5, opt-in).  The regression heads are evaluated at the
K winners of the decode only -- generic_decode reads nothing else of them (decode.py:99-180) -- so every packed row must
be what the dense path gives: the same winners (the hm map is the same launch), head values within fp32 rounding of the
dense Winograd launch (direct convolution here), and, against the CPU oracle at full size, the same assertions as the
dense full-size tests (tests/_parity.py: ranks / classes / ids identical, values within 1e-3 on the output grid).  Below them,
ct_decode with ct_sparse_heads_desc at the C-ABI level on the case table of tests/_sparse_heads.py: every field against a float64
evaluation of the same heads, from sliced feature views, into guarded rows, on a poisoned workspace."""
import numpy as np
import pytest
import torch

import _sparse_heads as SH
from _dcn_bwd import bound
from _guards import GUARD, NAN
from _parity import run_config

pytestmark = pytest.mark.gpu


def _pair(name, streams, **kw):
    import scenarios as S
    from _parity import calibrated_state_dict
    from centertrack_amd.detector import StreamDetector, default_opt
    from centertrack_amd.image import make_meta
    from centertrack_amd.model import DLASegHIP
    cfg = S.CONFIGS[name]
    heads = S.HEAD_SETS[cfg['heads']]
    sd = calibrated_state_dict(name, heads)
    dets = []
    kw = dict(kw)
    flip = kw.pop('flip_test', cfg['flip'])
    for sparse in (False, True):
        opt = default_opt(heads, track_thresh=cfg['track_thresh'], pre_thresh=cfg['pre_thresh'], sparse_heads=sparse,
                          flip_test=flip, **kw)
        model = DLASegHIP(heads)
        model.load_state_dict(sd)
        dets.append(StreamDetector(opt, model=model, num_streams=streams))
    return cfg, dets[0], dets[1], make_meta(cfg['H'], cfg['W'], 2 * cfg['H'], 2 * cfg['W'])


@pytest.mark.parametrize('name,streams,kw', [('mot17_512', 1, {}), ('mot17_512', 3, {'zero_tracking': True}),
                                              ('nusc_800x448', 2, {}), ('coco_512', 2, {}), ('mot17_544x960', 1, {}),
                                              ('kitti_1280x384', 2, {}), ('nusc_800x448', 1, {'flip_test': True})],
                         ids=['mot', 'mot_x3_zero_tracking', 'nusc_3d_heads', 'coco_80_classes', 'mot_544x960',
                              'kitti_flip_test', 'nusc_3d_heads_flip_test'])
def test_sparse_rows_equal_dense_rows(device, name, streams, kw):
    from _parity import scrolled_stream
    cfg, dense, sparse, meta = _pair(name, streams, **kw)
    assert sparse.sparse and not dense.sparse
    frames = [scrolled_stream(cfg['H'], cfg['W'], 4, 400 + 10 * s) for s in range(streams)]
    for t in range(4):
        x = torch.cat([frames[s][t] for s in range(streams)], 0)
        rd = dense.step(x, [dict(meta) for _ in range(streams)])
        rs = sparse.step(x, [dict(meta) for _ in range(streams)])
        a, b = dense.last_dets, sparse.last_dets
        assert sorted(a) == sorted(b)
        for k in ('scores', 'clses', 'xs', 'ys'):                    # the winners: same hm launch, same selection
            np.testing.assert_array_equal(a[k], b[k], err_msg='frame %d %s' % (t, k))
        for k in a:
            if k not in ('scores', 'clses', 'xs', 'ys', 'cts'):
                scale = max(1.0, float(np.abs(a[k]).max()))
                np.testing.assert_allclose(b[k], a[k], rtol=0, atol=2e-4 * scale, err_msg='frame %d %s' % (t, k))
        for s in range(streams):
            assert [int(r['tracking_id']) for r in rs[s]] == [int(r['tracking_id']) for r in rd[s]], (t, s)
    if kw.get('zero_tracking'):
        assert float(np.abs(sparse.last_dets['tracking']).max()) == 0.0
    plan = sparse._ctx['plan']
    names = [l.name for l in plan['launches'] if l.fn == 'heads' or l.name.startswith('heads.')]
    assert plan['sparse'] is not None and all('wh' not in n and 'tracking' not in n for n in names), names


# (streams picked like the dense full-size tests': no oracle score within 1e-5 of a threshold -- checked on the CPU, min 3.6e-4)
@pytest.mark.parametrize('name,streams,T,seed0', [('mot17_512', 1, 8, 331), ('nusc_800x448', 2, 3, 324), ('coco_512', 2, 3, 324),
                                                   ('kitti_1280x384', 2, 2, 317 + 7)])
def test_sparse_heads_match_oracle_at_full_size(device, name, streams, T, seed0):
    checks, swaps, det = run_config(name, streams, T, seed0=seed0, sparse_heads=True)
    assert det.sparse
    assert sum(c.frames for c in checks) == T * streams


@pytest.mark.parametrize('name,streams,sample,T', [('mot17_512', 16, (0, 8, 15), 3), ('nusc_800x448', 8, (0, 7), 3),
                                                    ('kitti_1280x384', 4, (0, 3), 2)])
def test_sparse_heads_on_the_benchmarked_many_stream_plans(device, name, streams, sample, T):
    """the many-stream launch plans (other conv tiles, Winograd raw-sum offset convs; tests/test_hip_plans.py) with sparse
    heads against the oracle: streams nobody picked, so a stream that meets a threshold tie is compared up to that frame"""
    from _parity import RANK_TIE_UNPICKED
    checks, swaps, det = run_config(name, streams, T, sample=sample, on_threshold_tie='stop', min_tracks=5,
                                    rank_tie=RANK_TIE_UNPICKED, sparse_heads=True)
    assert det.sparse
    assert sum(c.frames for c in checks) >= (2 * T * len(sample) + 2) // 3


def test_sparse_heads_are_refused_where_they_do_not_apply(device):
    import scenarios as S
    from centertrack_amd import weights as W
    from centertrack_amd.detector import StreamDetector, default_opt
    from centertrack_amd.model import DLASegHIP
    heads = W.KITTI_HEADS
    model = DLASegHIP(heads)
    model.load_state_dict(W.make_synthetic_state_dict(heads, seed=3))
    det = StreamDetector(default_opt(heads, flip_test=True, sparse_heads=True), model=model, num_streams=1)
    assert det.sparse                            # flip_test: hm merged as a map, averaged heads evaluated in both images
    pose = StreamDetector(default_opt(W.POSE_HEADS, sparse_heads=True), model=None if False else DLASegHIP(W.POSE_HEADS),
                          num_streams=1)
    assert not pose.sparse


# ---------------------------------------------------------------------------------------------------------------------
# ct_decode with ct_sparse_heads_desc at the C-ABI level: every case of tests/_sparse_heads.py against float64

class _MainRun(object):
    """one case on the device through ``ops.Decoder``, its descriptor then pointed at the caller's buffers of this test: the feature
    map is a channel slice at the case's pitch with NaN in every other channel; rows go with out_stride = F + 5 into a buffer of
    B*K + 3 rows filled with 7.0; the workspace is the exact size the library asks for with 64 floats of 7.0 behind it.  Of the
    workspace ct_decode reads nothing it has not written in the same call (candidates: stage 1 fills every slot; winner keys:
    stage 2; partials: every entry sparse_rows_kernel adds is written by sparse_heads_kernel) -- ``run(poison=True)`` fills the
    winner keys and the partials with NaN, ``run(poison=False)`` zeroes them, and both must give the same bits."""

    def __init__(self, c, device, K=None, host=False):
        from centertrack_amd import ops
        self.c, self.K = c, K or c.K
        d = SH.make_case(c)
        dev = lambda t: t.to(device).contiguous()
        N = d['feat'].shape[0]
        buf = torch.full((N, c.h, c.w, SH.ldf(c)), NAN)
        buf[..., c.c0:c.c0 + 64] = d['feat'].permute(0, 2, 3, 1)
        self.feat = ops.View(buf.to(device), c.c0, 64)
        assert self.feat.ld == SH.ldf(c) and self.feat.ptr % 16 == 0
        sparse = {'feat': self.feat, 'flip': c.flip, 'depth_scale': SH.DEPTH_SCALE, 'zero_tracking': c.zero_tracking,
                  'heads': [(n, ops.pack_weight(dev(w1)), dev(b1), dev(w2), dev(b2)) for n, w1, b1, w2, b2 in d['heads']]}
        self.hm = dev(d['hm'])
        self.dec = dec = ops.Decoder(self.hm, {}, self.K, sparse=sparse)
        self.F, self.stride, self.nrows = dec.F, dec.F + 5, c.B * self.K
        self.out = torch.full((self.nrows + 3, self.stride), GUARD, device=device)
        dec.desc.out, dec.desc.out_stride = self.out.data_ptr(), self.stride
        self.sel, keys, partials = SH.workspace_bytes(c._replace(K=self.K))
        self.nbytes = dec.desc.workspace_bytes
        assert self.nbytes == self.sel + keys + partials and self.sel % 4 == 0
        self.ws = torch.full((self.nbytes // 4 + 64,), GUARD, device=device)
        dec.desc.workspace = self.ws.data_ptr()
        self.host = None
        if host:
            self.host = torch.empty((self.nrows + 3, self.stride)).pin_memory()
            self.flag = torch.zeros((1,), dtype=torch.int32).pin_memory()
            self.counter = torch.zeros((4,), dtype=torch.int32, device=device)
            dec.desc.host_out, dec.desc.done_flag = self.host.data_ptr(), self.flag.data_ptr()
            dec.desc.done_counter = self.counter.data_ptr()

    def run(self, poison=True):
        """-> rows [B,K,F] (numpy), after checking that nothing but the rows was written"""
        import ctypes
        from centertrack_amd import _lib
        n = self.nbytes // 4
        self.ws[:n].zero_()
        if poison:
            self.ws[self.sel // 4:n] = NAN
        self.out.fill_(GUARD)
        if self.host is not None:
            self.host.fill_(GUARD)
            self.flag.zero_()
        _lib.check(_lib.load().ct_decode(ctypes.byref(self.dec.desc), _lib.stream_ptr()), 'ct_decode')
        torch.cuda.current_stream().synchronize()
        flat = self.out.cpu()
        assert bool((flat[:, self.F:] == GUARD).all()), 'the 5 floats behind a row were written'
        assert bool((flat[self.nrows:] == GUARD).all()), 'rows past B*K were written'
        assert bool((self.ws[n:] == GUARD).all()), 'the workspace was overrun'
        return flat[:self.nrows, :self.F].reshape(self.c.B, self.K, self.F).numpy().copy()


_main = {}


def _main_run(c, device):
    """(run, rows on the NaN-filled workspace, rows on the zeroed one), once per case"""
    if c.name not in _main:
        r = _MainRun(c, device)
        _main[c.name] = (r, r.run(True), r.run(False))
    return _main[c.name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize('c', SH.CASES, ids=[c.name for c in SH.CASES])
def test_ct_decode_sparse_against_torch_convolutions(device, c):
    """every non-integer field of the unpacked rows against the same heads evaluated densely in float64 on the CPU (F.conv2d, the
    dep transform and the flip_test merge in float64) and decoded by oracle.decode.generic_decode: the error relative to the
    field's largest reference value within the project's bound, 4 x the larger of the float32 CPU evaluation's own error and
    2^-23 sqrt(832).  scores / clses / xs / ys / inds bit for bit those of the dense decoder on float32 maps, and the oracle's.
    The feature slice lies between NaN channels and the winner keys and partials start as NaN: the rows are finite, and the
    same bits as on a zeroed workspace."""
    from centertrack_amd import ops
    run, rows, rows_zeroed = _main_run(c, device)
    assert np.isfinite(rows).all()
    np.testing.assert_array_equal(_bits(rows), _bits(rows_zeroed))
    got = run.dec.unpack(rows)
    r64, r32 = SH.reference(c, torch.float64), SH.reference(c, torch.float32)
    dense = ops.Decoder(run.hm, {n: v.to(device) for n, v in SH.head_maps(c, torch.float32).items()}, c.K)
    want = dense.unpack(dense.run().cpu().numpy())
    assert sorted(got) == sorted(want) and dense.layout == run.dec.layout
    for k in SH.INTEGER_FIELDS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    assert torch.equal(run.dec.inds.cpu(), dense.inds.cpu()) and torch.equal(dense.inds.cpu(), r64['inds'])
    for k in ('scores', 'clses', 'xs', 'ys'):
        np.testing.assert_array_equal(got[k], r32[k].numpy(), err_msg='%s against the oracle' % k)
    bad = []
    items = [(k, got[k].astype(np.float64)) + tuple(r[k].reshape(c.B, c.K, wd).double().numpy() for r in (r64, r32))
             for k, s, wd in run.dec.layout if k not in SH.INTEGER_FIELDS]
    # a box is coordinates of up to 40 around a size of a few pixels: its width and height as a field of their own, so that the
    # size heads are not judged at the coordinates' scale (the float32 reference's e32 carries the coordinates' rounding)
    size = lambda v: v[..., 2:4] - v[..., 0:2]
    items += [(k + ' size', size(g), size(a), size(b)) for k, g, a, b in items if k.startswith('bboxes')]
    for k, g64, ref64, ref32 in items:
        norm = float(np.abs(ref64).max())
        if norm == 0.0:                                       # zero_tracking: exactly zero, nothing to scale by
            assert not g64.any(), k
            print('%s %s: all zero, as the reference' % (c.name, k))
            continue
        e32 = float(np.abs(ref32 - ref64).max()) / norm
        err = float(np.abs(g64 - ref64).max()) / norm
        b = bound(e32, SH.K_TERMS)
        print('%s %s: err %.3g, float32 reference %.3g, bound %.3g, ratio %.3f' % (c.name, k, err, e32, b, err / b))
        if not err <= b:
            bad.append((k, err, b))
    assert not bad, bad


@pytest.mark.parametrize('c', [c for c in SH.CASES if c.C >= 2], ids=[c.name for c in SH.CASES if c.C >= 2])
def test_a_pixel_that_wins_in_two_classes_carries_the_same_bits(device, c):
    """the head values of a winner depend on its pixel alone (every row of the MFMA tile is the same k-ordered chain, every
    (winner, channel) of the tail the same two 32-term sums): two rows of one image at one pixel differ in score and class only"""
    run, rows, _ = _main_run(c, device)
    for b in range(c.B):
        pix = (rows[b, :, 3] * c.w + rows[b, :, 2]).astype(np.int64)
        pairs = [(i, j) for i in range(c.K) for j in range(i + 1, c.K) if pix[i] == pix[j]]
        assert len(pairs) >= 2 and all(rows[b, i, 1] != rows[b, j, 1] for i, j in pairs)
        for i, j in pairs:
            np.testing.assert_array_equal(_bits(rows[b, i, 2:]), _bits(rows[b, j, 2:]), err_msg='%s image %d rows %d %d' % (c.name, b, i, j))


_PLUS_ONE = [c for c in SH.CASES if c.K < 100 and c.K + 1 <= c.h * c.w]


@pytest.mark.parametrize('c', _PLUS_ONE, ids=[c.name for c in _PLUS_ONE])
def test_one_more_winner_leaves_the_first_K_rows_alone(device, c):
    """K + 1 winners: another tile count where K is a multiple of 16, another place in the partials for every winner of every
    image but the first -- the first K rows of every image keep their bits"""
    _, rows, _ = _main_run(c, device)
    more = _MainRun(c, device, K=c.K + 1).run(True)
    np.testing.assert_array_equal(_bits(more[:, :c.K, :4]), _bits(rows[:, :, :4]), err_msg='the winners')
    np.testing.assert_array_equal(_bits(more[:, :c.K]), _bits(rows))


@pytest.mark.parametrize('name', ['odd_K', 'ragged_map_3d_heads_x3'])
def test_host_rows_and_done_flag_through_the_rows_kernel(device, name):
    """host_out / done_flag with sparse heads are sparse_rows_kernel's job: after a stream sync the flag is 1, the pinned rows
    are the device rows bit for bit at the same pitch (and nothing else of the pinned buffer was written), the arrival counter
    is back to 0 (B = 1 never touches it) -- so a second run on the same descriptor raises the flag again"""
    c = SH.CASE[name]
    assert c.B in (1, 3)
    _, rows, _ = _main_run(c, device)
    run = _MainRun(c, device, host=True)
    for attempt in range(2):
        got = run.run(True)
        assert int(run.flag[0]) == 1, 'attempt %d' % attempt
        assert int(run.counter.cpu().abs().sum()) == 0
        np.testing.assert_array_equal(_bits(run.host.numpy()), _bits(run.out.cpu().numpy()))
        np.testing.assert_array_equal(_bits(got), _bits(rows))


def test_two_runs_and_a_fresh_decoder_give_the_same_bits(device):
    c = SH.CASE['all_heads_k17_slice']
    assert c.K % 16
    run, rows, _ = _main_run(c, device)
    np.testing.assert_array_equal(_bits(run.run(True)), _bits(rows))
    np.testing.assert_array_equal(_bits(_MainRun(c, device).run(True)), _bits(rows))
