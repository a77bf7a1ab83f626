"""GPU: every selection path, tie order and segment edge of the heat-map decode (centertrack_amd/csrc/decode.hip, csrc/pose.hip)
against the reference of tests/_decode_paths.py.  tests/test_decode_paths_cpu.py proves on the CPU that the cases run here reach
every label of the table.  The decode is a selection plus a few float32 operations: every comparison is bit for bit, except
``kps_score`` (rtol 1e-5, atol 1e-7: the summation order of torch.mean is not restated)."""
import numpy as np
import pytest
import torch

import _decode_paths as P

pytestmark = pytest.mark.gpu


def _sliced(t, device):
    """t [B,c,h,w] as a channel slice of a wider tensor: batch stride > c*h*w"""
    B, c, h, w = t.shape
    wide = torch.full((B, c + 3, h, w), 7.0, device=device)
    wide[:, 2:2 + c] = t.to(device)
    return wide[:, 2:2 + c]


def _tensors(case, device, hm=None):
    hm = torch.from_numpy(np.array(P.heat_map(case.name) if hm is None else hm))
    heads = {k: torch.from_numpy(np.array(v)) for k, v in P.head_maps(case.name).items()}
    dev_hm = _sliced(hm, device) if 'hm' in case.strided else hm.to(device)
    dev_heads = {k: (_sliced(v, device) if 'head' in case.strided and k == 'wh' else v.to(device)) for k, v in heads.items()}
    if case.strided:
        assert dev_hm.stride(0) > case.C * case.h * case.w and dev_heads['wh'].stride(0) > 2 * case.h * case.w
    return dev_hm, dev_heads


def _check(dec, packed, inds, want, what):
    got = dec.unpack(packed)
    np.testing.assert_array_equal(inds, want['inds'], err_msg=what + ' inds')
    assert set(want) - {'inds'} <= set(got), sorted(set(want) - set(got))
    for k, v in want.items():
        if k != 'inds':
            np.testing.assert_array_equal(got[k], v, err_msg='%s.%s' % (what, k))


@pytest.mark.parametrize('name', [c.name for c in P.CASES])
def test_decode_case_is_the_reference_bit_for_bit(device, name):
    from centertrack_amd import ops
    case = P.CASE[name]
    hm, heads = _tensors(case, device)
    dec = ops.Decoder(hm, heads, case.K)
    packed = dec.run()
    torch.cuda.synchronize()
    _check(dec, packed.cpu().numpy(), dec.inds.cpu().numpy(), P.reference(name), name)
    if case.distinct and all((P.nms(P.heat_map(name)[b:b + 1]) > 0).sum() >= case.K for b in range(case.B)):
        from oracle import decode as odecode
        maps = {'hm': torch.from_numpy(np.array(P.heat_map(name)))}
        maps.update((k, torch.from_numpy(np.array(v))) for k, v in P.head_maps(name).items())
        want = odecode.generic_decode(maps, K=case.K, return_inds=True)
        _check(dec, packed.cpu().numpy(), dec.inds.cpu().numpy(), {k: v.numpy() for k, v in want.items() if k != 'cts'}, name + ' (oracle)')


def _reuse_maps(where):
    shape_of, maps = P.REUSE[where]
    case = P.CASE[shape_of]
    out = []
    for make, end in maps:
        hm = make(case)
        out.append((end, hm, P.decode_with(hm, P.head_maps(case.name), case.K)))
    return case, out


@pytest.fixture(scope='module', params=['regs', 'mem'])
def reuse(request):
    return (request.param,) + _reuse_maps(request.param)


def test_a_reused_decoder_carries_nothing_from_one_path_to_the_next(device, reuse):
    """one Decoder on a fixed tensor, refilled in place: radix, then slow, then hist (regs) / bitonic (mem); the workspace is
    zeroed at construction only"""
    from centertrack_amd import ops
    where, case, maps = reuse
    hm, heads = _tensors(case, device)
    dec = ops.Decoder(hm, heads, case.K)
    for end, new, want in maps + maps[:1]:
        hm.copy_(torch.from_numpy(new))
        packed = dec.run().cpu().numpy()
        inds = dec.inds.cpu().numpy()
        _check(dec, packed, inds, want, '%s reused at %s' % (where, end))
        fresh = ops.Decoder(hm.clone(), heads, case.K)
        np.testing.assert_array_equal(fresh.run().cpu().numpy(), packed, err_msg=end)
        np.testing.assert_array_equal(fresh.inds.cpu().numpy(), inds, err_msg=end)


def test_a_captured_decoder_replays_every_path(device, reuse):
    """the same under graph capture and replay: the frame loop builds its Decoder once and replays it"""
    from centertrack_amd import ops
    where, case, maps = reuse
    hm, heads = _tensors(case, device)
    dec = ops.Decoder(hm, heads, case.K)
    dec.run()                                                # (first use outside the capture: kernel attributes are set once)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            dec.run()
    for end, new, want in maps + maps[:1]:
        hm.copy_(torch.from_numpy(new))
        g.replay()
        torch.cuda.synchronize()
        _check(dec, dec.out.cpu().numpy(), dec.inds.cpu().numpy(), want, '%s replayed at %s' % (where, end))


@pytest.mark.parametrize('name', ['mem_radix', 'const_160'])
def test_host_rows_equal_device_rows_on_the_long_paths(device, name):
    from centertrack_amd import ops
    case = P.CASE[name]
    hm, heads = _tensors(case, device)
    F = ops.Decoder.row_floats(heads)
    host = torch.zeros((case.B, case.K, F), dtype=torch.float32).pin_memory()
    flag = torch.zeros((16,), dtype=torch.int32).pin_memory()
    dec = ops.Decoder(hm, heads, case.K, host_out=host, done_flag=flag)
    assert dec.direct
    for rep in range(2):
        host.zero_()
        flag.zero_()
        out = dec.run()
        torch.cuda.synchronize()
        assert int(flag[0]) == 1 and int(dec.done_counter[0]) == 0
        np.testing.assert_array_equal(host.numpy(), out.cpu().numpy())
    _check(dec, host.numpy(), dec.inds.cpu().numpy(), P.reference(name), name + ' host rows')


def test_pose_thresholds_gate_edges_and_ties(device):
    """the designed joints of tests/_decode_paths.py::POSE_WANT (a peak of exactly 0.2f, a peak on the gate box's edge, two
    equidistant peaks, a joint map that takes the slow path, a constant joint map) and 2 x 40 x 17 ordinary ones"""
    from centertrack_amd import ops
    maps = {k: torch.from_numpy(np.array(v)).to(device) for k, v in P.pose_maps().items()}
    dec = ops.Decoder(maps['hm'], {k: v for k, v in maps.items() if k != 'hm'}, P.POSE['K'])
    got = dec.unpack(dec.run().cpu().numpy())
    want = P.pose_reference()
    np.testing.assert_array_equal(dec.inds.cpu().numpy(), want['inds'])
    for (det, j), (xy, why) in P.POSE_WANT.items():
        np.testing.assert_array_equal(got['hps'][0, det, 2 * j:2 * j + 2], np.array(xy, np.float32), err_msg=why)
    for k in ('scores', 'clses', 'xs', 'ys', 'bboxes', 'hps'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got['kps_score'], want['kps_score'], rtol=1e-5, atol=1e-7)
