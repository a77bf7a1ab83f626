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
