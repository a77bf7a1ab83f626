"""CPU: the C ABI of the DCNv2 backward (ct_dcn_v2_backward) -- exports, descriptor layout, host-side argument
validation -- and the opt-in switch of the differentiable path of centertrack_amd.dcn_v2.  No GPU call is made."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW = ['ct_dcn_v2_backward', 'ct_dcn_v2_backward_workspace_bytes', 'ct_packed_dcn_weight_t_elems', 'ct_pack_dcn_weight_t']


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def test_new_symbols_are_exported_and_listed(lib):
    from centertrack_amd import _lib
    assert lib.ct_version() == 103                  # new symbols, no layout change of an existing descriptor
    for n in NEW:
        assert hasattr(lib, n), 'missing export ' + n
        assert n in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'centertrack_hip.h')).read()
    for n in NEW + ['ct_dcn_bwd_desc', 'CT_DCN_BWD_INPUT', 'CT_DCN_BWD_OFFSET_MASK', 'CT_DCN_BWD_WEIGHT']:
        assert n in hdr, n
    assert lib.ct_packed_dcn_weight_t_elems(27, 64) == 9 * 4 * 2 * 256
    assert lib.ct_packed_dcn_weight_t_elems(64, 64) == lib.ct_packed_weight_elems(64, 64, 3)


def test_ctypes_backward_descriptor_matches_the_header_layout(tmp_path):
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [f for f, _ in _lib.DcnBwdDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ct_dcn_bwd_desc));',
             'printf("FLAGVALUES %d %d %d\\n", CT_DCN_BWD_INPUT, CT_DCN_BWD_OFFSET_MASK, CT_DCN_BWD_WEIGHT);']
    lines += ['printf("%s %%zu\\n", offsetof(ct_dcn_bwd_desc, %s));' % (f, f) for f in fields]
    lines += ['return 0; }']
    src = tmp_path / 'lay.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.DcnBwdDesc)
    assert got["FLAGVALUES"].split() == [str(v) for v in (_lib.CT_DCN_BWD_INPUT, _lib.CT_DCN_BWD_OFFSET_MASK,
                                                     _lib.CT_DCN_BWD_WEIGHT)]
    for f in fields:
        assert int(got[f]) == getattr(_lib.DcnBwdDesc, f).offset, f


def _desc(p, **kw):
    from centertrack_amd import _lib
    d = _lib.DcnBwdDesc()
    d.x = d.om = d.gy = d.wT_packed = d.gx = d.gom = d.gw = d.gb = d.workspace = p
    d.N, d.H, d.W, d.Cin, d.Cout = 1, 4, 4, 64, 64
    d.ldx, d.ldom, d.ldgy, d.ldgx, d.ldgom = 64, 32, 64, 64, 32
    d.flags = _lib.CT_DCN_BWD_INPUT | _lib.CT_DCN_BWD_OFFSET_MASK | _lib.CT_DCN_BWD_WEIGHT
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_backward_argument_validation_without_gpu(lib):
    """every rejected descriptor returns CT_ERR_ARG with a message BEFORE anything is launched (none of these calls
    reaches the device: the pointers are host memory)"""
    from centertrack_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rejected(d, word):
        assert lib.ct_dcn_v2_backward(ctypes.byref(d), None) == _lib.CT_ERR_ARG
        assert word in lib.ct_last_error(), lib.ct_last_error()

    assert lib.ct_dcn_v2_backward(None, None) == _lib.CT_ERR_ARG
    rejected(_lib.DcnBwdDesc(), b'flags')
    for name in ('x', 'om', 'gy', 'wT_packed', 'gx', 'gom', 'gw'):
        rejected(_desc(p, **{name: None}), b'null')
    rejected(_desc(p, Cin=48), b'Cin')
    rejected(_desc(p, Cin=0), b'Cin')
    rejected(_desc(p, Cout=0), b'shape')
    rejected(_desc(p, flags=8), b'flags')
    rejected(_desc(p, ldgx=32), b'ldgx')
    # 2 GiB and more in one view: 8192 x 1024 pixels x 64 channels x 4 B = 2 GiB exactly
    rejected(_desc(p, H=8192, W=1024), b'2 GiB')
    rejected(_desc(p, N=4, H=32768, W=32768), b'2 GiB')
    assert lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(_desc(p, H=8192, W=1024))) == 0
    # an accepted descriptor only fails on its workspace; gradients that are not asked for need no buffers
    d = _desc(p, workspace=None)
    need = lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(d))
    assert need >= (64 * 64 * 9 + 64) * 4 and need % ((64 * 64 * 9 + 64) * 4) == 0
    assert lib.ct_dcn_v2_backward(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    d = _desc(p, flags=_lib.CT_DCN_BWD_INPUT)
    assert lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.ct_pack_dcn_weight_t(None, p, 64, 64, None) == _lib.CT_ERR_ARG
    assert lib.ct_pack_dcn_weight_t(p, p, 64, 40, None) == _lib.CT_ERR_ARG


def test_trainable_switch_defaults_to_off_and_the_context_manager_restores_it():
    from centertrack_amd import dcn_v2
    assert dcn_v2.is_trainable() is False
    with dcn_v2.trainable():
        assert dcn_v2.is_trainable() is True
        with dcn_v2.trainable(False):
            assert dcn_v2.is_trainable() is False
        assert dcn_v2.is_trainable() is True
    assert dcn_v2.is_trainable() is False
    with pytest.raises(ValueError):
        with dcn_v2.trainable():
            raise ValueError('x')
    assert dcn_v2.is_trainable() is False
    assert dcn_v2.set_trainable(True) is False
    assert dcn_v2.set_trainable(False) is True
    assert dcn_v2.is_trainable() is False


def test_effective_offsets_put_the_float64_oracle_on_the_fp32_sample_positions():
    """(B 4, 64 -> 64, 128x128, offsets of scale 2 px): fed the fp32 offsets, the float64 oracle forms the exact sum where the
    float32 oracle and the kernel form fl32(base + d); where that rounds onto an integer the two pick different cells and
    g_offset, discontinuous there, differs by 20 % of its maximum.  With effective_offsets every position is the fp32 one."""
    import torch
    import _dcn_bwd as D
    shape = (4, 64, 64, 128, 128, 2.0)
    B, _, _, H, W, _ = shape
    inp = D.inputs(shape)
    off = inp[1]
    base = D.tap_bases(H, W).unsqueeze(0)
    pos32 = D.tap_bases(H, W, torch.float32).unsqueeze(0) + off              # as the float32 oracle and the kernel form it
    eff = D.effective_offsets(off, H, W)
    assert eff.dtype == torch.float64 and eff.shape == off.shape
    moved = (eff - off.double()).abs()
    assert 0.5 * off.numel() < int((moved > 0).sum()) and float(moved.max()) <= 2.0 ** -17      # half an ulp of 128
    L = torch.tensor([H, W] * 9, dtype=torch.float64).view(1, 18, 1, 1)

    def cells(pos):
        pos = pos.double()
        return torch.floor(pos), (pos > -1) & (pos < L)

    f32, in32 = cells(pos32)
    f64, in64 = cells(base + eff)
    assert torch.equal(pos32.double(), base + eff)                           # bit-identical positions ...
    assert torch.equal(f32, f64) and torch.equal(in32, in64)                 # ... so floor and `inside` agree on every sample
    fn, inn = cells(base + off.double())
    assert int((fn != f32).sum()) + int((inn != in32).sum()) > 0             # the exact sum does not
    g32 = D.oracle_grads(inp, torch.float32)
    naive = D.oracle_grads(inp, torch.float64)
    sharp = D.oracle_grads(inp, torch.float64, effective=True)
    for n in D.NAMES:
        print('oracle32 against float64 %s g_%-6s exact positions %.3e  fp32 positions %.3e'
              % (D.shape_id(shape), n, D.err(g32[n], naive[n]), D.err(g32[n], sharp[n])))
    assert D.err(g32['offset'], naive['offset']) > 0.1                       # 0.20: the problem
    assert D.err(g32['offset'], sharp['offset']) < 1e-5                      # 2.2e-7: the helper solves it
    for n in D.NAMES:
        assert D.err(g32[n], sharp[n]) < 1e-5, n


def _library_slabs(lib, shape):
    from centertrack_amd import _lib
    B, Cin, Cout, H, W = shape[:5]
    d = _desc(None, N=B, H=H, W=W, Cin=Cin, Cout=Cout, ldx=Cin, ldgy=Cout, ldgx=Cin, flags=_lib.CT_DCN_BWD_WEIGHT)
    need = lib.ct_dcn_v2_backward_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need % (4 * (Cout * Cin * 9 + Cout)) == 0, (shape, need)
    return need // (4 * (Cout * Cin * 9 + Cout))


def test_plan_mirror_matches_the_library(lib):
    """the Python restatement of make_plan cannot drift from the C code unnoticed: its slab count is the library's
    (workspace = slabs x (Cout*Cin*9 + Cout) floats).  CS, the channel split of the data kernel, is not observable
    through the ABI; its mirror is kept true by reading dcn_bwd.hip."""
    import _dcn_bwd as D
    extra = [(1, 64, 64, 4, 4, 0.0), (2, 64, 24, 12, 20, 2.0), (1, 256, 128, 8, 8, 0.0), (7, 96, 40, 33, 5, 1.0),
             (1, 32, 512, 100, 100, 1.0), (16, 512, 512, 64, 64, 1.0)]
    for shape in D.PLAN_SHAPES + extra:
        assert D.plan(*shape[:5])['slabs'] == _library_slabs(lib, shape), shape


def test_plan_shapes_reach_every_regime_of_the_plan():
    """the list the GPU test runs contains a shape for every branch of make_plan and of the kernels' tails; a change of
    the plan thresholds (or of the list) that moves a regime out of reach fails here, without a GPU"""
    import _dcn_bwd as D
    assert len(set(D.PLAN_SHAPES)) == len(D.PLAN_SHAPES)
    for ci, co, s in D.neck_shapes():
        assert (1, ci, co, s, s, 0.5 if s == 16 else 2.0) in D.PLAN_SHAPES
    missing = D.missing_regimes(D.PLAN_SHAPES)
    assert not missing, 'no shape of PLAN_SHAPES reaches: %s' % ', '.join(missing)
    # the check itself: without its only Cout = 512 shape the list is reported incomplete, by name
    assert D.missing_regimes([s for s in D.PLAN_SHAPES if s[2] != 512]) == ['Cout == 512']
    assert 'stepsPerWave % 4 == 3' in D.missing_regimes([s for s in D.PLAN_SHAPES if D.plan(*s[:5])['stepsPerWave'] % 4 != 3])
    for shape in D.PLAN_SHAPES:
        B, Cin, Cout, H, W, _ = shape
        assert Cin % 32 == 0 and 0 < Cout <= 512 and B * H * W * max(Cin, Cout) * 4 < 2 ** 31


def test_designed_positions_hold_every_pair_in_every_image():
    import torch
    import _dcn_bwd as D
    for B, H, W in ((3, 6, 7), (2, 8, 10)):
        pos, pair = D.designed_positions(B, H, W)
        assert bool((pos * 4 == torch.floor(pos * 4)).all())                  # multiples of 0.25: exact in fp32 and fp64
        off = (pos - D.tap_bases(H, W).unsqueeze(0)).float()
        assert torch.equal(D.effective_offsets(off, H, W), off.double())
        for n in range(B):
            assert sorted(set(pair[n].flatten().tolist())) == list(range(196))
