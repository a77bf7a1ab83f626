"""CPU: the trainable stems (centertrack_amd/csrc/stem_train.hip) without a GPU -- the entry points refuse bad descriptors
before anything is launched, the restated launch plans (tests/_stem_bwd.py) agree with the workspace queries on every test and
bench shape, the GPU shape list reaches every regime of the table, and the float32 reference itself stays inside the mask cap
of ``_backbone_bwd.check_mask`` (0 flipped units) for the exact seeds, shapes and inputs the GPU tests use."""
import ctypes

import pytest
import torch

import _backbone_bwd as BB
import _stem_bwd as SB
from _dcn_bwd import err


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr(offset=0):
    buf = (ctypes.c_float * 64)()
    _ptr.keep.append(buf)
    return ctypes.cast(buf, ctypes.c_void_p).value + offset


_ptr.keep = []


def conv_desc(N=1, H=8, W=8, stems=(0, 1, 2), fwd=True, gw=(0, 1, 2), gin=()):
    from centertrack_amd import _lib
    d = _lib.StemConvDesc()
    d.N, d.H, d.W = N, H, W
    for s in stems:
        d.inp[s], d.w[s] = _ptr(), _ptr()
        if fwd:
            d.z[s], d.ldz[s] = _ptr(), 16
        else:
            d.gz[s], d.ldgz[s] = _ptr(), 16
            if s in gw:
                d.gw[s] = _ptr()
            if s in gin:
                d.gin[s] = _ptr()
    return d


def sum_desc(N=1, H=8, W=8, stems=(0, 1, 2)):
    from centertrack_amd import _lib
    d = _lib.StemSumDesc()
    d.N, d.H, d.W = N, H, W
    for s in stems:
        d.z[s], d.ldz[s] = _ptr(), 16
        d.mean[s], d.invstd[s], d.gamma[s], d.beta[s] = _ptr(), _ptr(), _ptr(), _ptr()
    d.y, d.ldy = _ptr(), 16
    return d


def refused(lib, fn, d, word):
    from centertrack_amd import _lib
    assert fn(ctypes.byref(d), None) == _lib.CT_ERR_ARG
    assert word.encode() in lib.ct_last_error(), lib.ct_last_error()


def test_forward_refusals(lib):
    from centertrack_amd import _lib
    fn = lib.ct_stem_conv_forward
    assert fn(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    refused(lib, fn, conv_desc(stems=(1, 2)), 'in[0]')                                     # a null stem 0
    d = conv_desc(); d.N = 0
    refused(lib, fn, d, 'bad shape')
    d = conv_desc(); d.w[1] = None
    refused(lib, fn, d, 'w[1]')                                                            # an input without its weight
    d = conv_desc(); d.z[2] = None
    refused(lib, fn, d, 'z[2]')
    d = conv_desc(); d.ldz[0] = 12
    refused(lib, fn, d, 'pitch')                                                           # below the channel count
    d = conv_desc(); d.ldz[1] = 18
    refused(lib, fn, d, 'multiple of 4')                                                   # a bad pitch
    d = conv_desc(); d.z[0] = _ptr(4)
    refused(lib, fn, d, '16-byte')                                                         # a misaligned map
    d = conv_desc(); d.inp[0] = _ptr(2)
    refused(lib, fn, d, '4-byte')
    refused(lib, fn, conv_desc(N=1, H=8192, W=4096), '2 GiB')                              # 2^25 pixels * 16 * 4 bytes
    d = conv_desc(N=1, H=4096, W=4096); d.ldz[2] = 32
    refused(lib, fn, d, '2 GiB')                                                           # the pitch counts


def test_sum_refusals(lib):
    from centertrack_amd import _lib
    fn = lib.ct_stem_bn_relu_sum
    assert fn(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    refused(lib, fn, sum_desc(stems=(1, 2)), 'z[0]')
    d = sum_desc(); d.H = -1
    refused(lib, fn, d, 'bad shape')
    d = sum_desc(); d.y = None
    refused(lib, fn, d, '(y)')
    d = sum_desc(); d.ldy = 8
    refused(lib, fn, d, 'pitch')
    d = sum_desc(); d.ldz[2] = 22
    refused(lib, fn, d, 'multiple of 4')
    d = sum_desc(); d.z[1] = _ptr(8)
    refused(lib, fn, d, '16-byte')
    d = sum_desc(); d.gamma[2] = None
    refused(lib, fn, d, 'stem 2')
    d = sum_desc(); d.invstd[0] = _ptr(4)
    refused(lib, fn, d, '16-byte')
    refused(lib, fn, sum_desc(N=2, H=4096, W=4096), '2 GiB')
    d = sum_desc(N=1, H=4096, W=4096); d.ldy = 32
    refused(lib, fn, d, '2 GiB')


def test_backward_refusals_and_workspace(lib):
    from centertrack_amd import _lib
    fn, query = lib.ct_stem_conv_backward, lib.ct_stem_conv_backward_workspace_bytes
    assert fn(None, None) == _lib.CT_ERR_ARG and query(None) == 0

    def both(d, word):
        refused(lib, fn, d, word)
        assert query(ctypes.byref(d)) == 0                                                 # 0 for a rejected descriptor

    both(conv_desc(fwd=False, gw=(), gin=()), 'no output')
    d = conv_desc(fwd=False); d.gz[1] = None
    both(d, 'without gz[1]')
    d = conv_desc(fwd=False); d.inp[0] = None
    both(d, 'in[0]')                                                                       # gw needs the input
    d = conv_desc(fwd=False, gw=(), gin=(0,)); d.w[0] = None
    both(d, 'w[0]')                                                                        # gin needs the weight
    d = conv_desc(fwd=False); d.ldgz[2] = 17
    both(d, 'multiple of 4')
    d = conv_desc(fwd=False); d.ldgz[0] = 4
    both(d, 'pitch')
    d = conv_desc(fwd=False); d.gz[0] = _ptr(4)
    both(d, '16-byte')
    d = conv_desc(fwd=False); d.gw[1] = _ptr(1)
    both(d, '4-byte')
    both(conv_desc(N=1, H=8192, W=4096, fwd=False), '2 GiB')
    d = conv_desc(N=0, fwd=False)
    both(d, 'bad shape')
    # a stem without outputs is not looked at: its gz may be anything
    d = conv_desc(fwd=False, gw=(0,)); d.ldgz[1] = 3; d.gz[2] = None
    assert query(ctypes.byref(d)) == SB.stem_plan(1, 8, 8, (0,))['bytes']
    # a weight gradient without its workspace
    d = conv_desc(fwd=False)
    need = query(ctypes.byref(d))
    assert need == SB.stem_plan(1, 8, 8)['bytes'] > 0
    assert fn(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = _ptr(), need - 4
    assert fn(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    d.workspace, d.workspace_bytes = _ptr(4), need
    assert fn(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    # image gradients alone need none
    assert query(ctypes.byref(conv_desc(fwd=False, gw=(), gin=(0, 1, 2)))) == 0


@pytest.mark.parametrize('shape', SB.SHAPES + SB.bench_shapes() + [(2, 64, 64), (4, 544, 960)], ids=SB.shape_id)
def test_the_restated_plan_against_the_workspace_query(lib, shape):
    for gw in [(0,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:
        d = conv_desc(*shape, fwd=False, gw=gw)
        assert lib.ct_stem_conv_backward_workspace_bytes(ctypes.byref(d)) == SB.stem_plan(*shape, gw_stems=gw)['bytes'], gw
    from centertrack_amd import _lib
    bd = _lib.BnDesc()
    bd.z, bd.N, bd.H, bd.W, bd.C, bd.ldz = _ptr(), shape[0], shape[1], shape[2], 16, 16
    assert lib.ct_bn_workspace_bytes(ctypes.byref(bd)) == SB.stem_plan(*shape)['bn']['bytes']


def test_the_gpu_shapes_reach_every_regime():
    assert SB.missing_regimes(SB.SHAPES) == []
    # each of the two largest entries is there for what nothing smaller reaches
    small = [s for s in SB.SHAPES if s[0] * s[1] * s[2] < 100000]
    assert SB.missing_regimes(small) == ['gw: grid capped, a ragged second round', 'sum: grid capped, a ragged second round']
    p = SB.stem_plan(2, 256, 260)
    assert (p['tiles'], p['slabs'], p['rounds'], p['quads']) == (576, 512, 2, 532480)
    assert SB.missing_regimes(SB.SHAPES[:4] + SB.SHAPES[5:]) == ['aligned MFMA tiles', 'gin: aligned tiles']


@pytest.mark.parametrize('training', [True, False], ids=['batch', 'running'])
@pytest.mark.parametrize('shape', SB.SHAPES, ids=SB.shape_id)
def test_the_float32_reference_flips_no_unit(shape, training):
    """the cap of ``check_mask`` (a mask may differ from float64's within 64 e32 of 0, on at most 0.1 % of a map) held by the
    float32 reference alone, for the seeds of the GPU tests: 0 flipped units in every stem"""
    sd, xs, _ = SB.case(shape)
    for s in range(3):
        r64, r32 = (SB.stem_reference(s, sd, xs[s], None, training, dt) for dt in (torch.float64, torch.float32))
        flipped, _ = BB.check_mask(r32['mask'], r64['pre'], err(r32['y'], r64['y']), 'stem %d' % s)
        assert flipped == 0, (shape, s, flipped)


@pytest.mark.parametrize('beta', ['zero', 'positive'])
def test_the_all_zero_heat_map_in_the_reference(beta):
    """the first frame of a video in training mode: z = 0, mean = 0, var = 0; with beta = 0 the pre-activation is exactly 0 and
    torch's ReLU passes no gradient; the weight gradient is exactly 0 either way and everything stays finite"""
    sd, xs, gy = SB.case((2, 20, 36), 'zero')
    sd['pre_hm_layer.1.bias'] = torch.zeros(16) if beta == 'zero' else torch.full((16,), 0.25)
    for dt in (torch.float64, torch.float32):
        r = SB.stem_reference(2, sd, xs[2], gy, True, dt)
        assert float(r['z'].abs().max()) == 0.0 and float(r['gw'].abs().max()) == 0.0
        assert all(bool(torch.isfinite(r[k]).all()) for k in ('y', 'gin', 'ggamma', 'gbeta'))
        if beta == 'zero':
            assert float(r['pre'].abs().max()) == 0.0 and float(r['gbeta'].abs().max()) == 0.0 and not bool(r['mask'].any())
        else:
            assert bool(r['mask'].all()) and float(r['gbeta'].abs().max()) > 0.0
