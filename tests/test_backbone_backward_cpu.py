"""CPU: the host side of the trainable backbone (centertrack_amd/csrc/backbone_bwd.hip, centertrack_amd/csrc/bn_train.hip, centertrack_amd/dla_base.py) -- exports
and descriptor layouts, argument validation and workspace queries of the stride-2 convolution backward, BatchNorm-act and
max-pool-backward entry points, the restated plans against those queries, the names, shapes and initialisation of the drop-in
modules, what they refuse, the parity decomposition and the pool's tie rule as explicit float64 sums against autograd, and the
float32 reference's own ReLU masks and pool selections against the cap the GPU tests hold the HIP forward to.  Nothing here
launches a kernel."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _backbone_bwd as BB

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW = ['ct_conv2d_s2_backward', 'ct_conv2d_s2_backward_workspace_bytes', 'ct_packed_conv_weight_s2t_elems',
       'ct_pack_conv_weight_s2t', 'ct_bn_act_apply', 'ct_bn_act_backward', 'ct_bn_act_workspace_bytes', 'ct_maxpool2x2_backward']


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr():
    buf = (ctypes.c_float * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15                    # a 16-byte aligned address inside the buffer
    return buf, ctypes.c_void_p(addr)


def test_new_symbols_are_exported_and_declared(lib):
    from centertrack_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'centertrack_hip.h')).read(), flags=re.S)
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS and re.search(r'\b%s\s*\(' % n, hdr), n
    assert lib.ct_version() == 103
    assert 'backbone_bwd.hip' in __import__('centertrack_amd.build', fromlist=['SOURCES']).SOURCES


def test_ctypes_descriptors_match_the_header_layout(tmp_path):
    from centertrack_amd import _lib
    found = [shutil.which(c) for c in ('gcc', 'cc', 'clang')] + ['/opt/rocm/llvm/bin/clang', '/opt/rocm/lib/llvm/bin/clang']
    gcc = next((c for c in found if c and os.path.exists(c)), None)      # any C compiler: the one that builds the library last
    if gcc is None:
        pytest.skip('no C compiler')
    checks = {'ct_conv_s2_bwd_desc': _lib.ConvS2BwdDesc, 'ct_bn_act_desc': _lib.BnActDesc, 'ct_bn_desc': _lib.BnDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {']
    for cname, cls in checks.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['return 0; }']
    src, exe = tmp_path / 'lay.c', tmp_path / 'lay'
    src.write_text('\n'.join(lines))
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in checks.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    # ct_bn_act_desc is ct_bn_desc plus four fields: a prefix with the same offsets
    for f, _ in _lib.BnDesc._fields_:
        assert getattr(_lib.BnActDesc, f).offset == getattr(_lib.BnDesc, f).offset, f
    assert (_lib.CT_BN_BATCH_STATS, _lib.CT_BN_ACT_RELU) == (1, 2)


def _s2_desc(p, N=2, H=6, W=10, Cin=16, Cout=32):
    from centertrack_amd import _lib
    d = _lib.ConvS2BwdDesc()
    d.x = d.gy = d.w_s2t = d.gx = d.gw = p
    d.N, d.H, d.W, d.Cin, d.Cout = N, H, W, Cin, Cout
    d.ldx = d.ldgx = Cin
    d.ldgy = Cout
    return d


def test_conv_s2_backward_validates_its_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    call, query = lib.ct_conv2d_s2_backward, lib.ct_conv2d_s2_backward_workspace_bytes
    assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    assert query(None) == 0
    for field, value, word in (('H', 5, b'must be even'), ('W', 7, b'must be even'), ('H', 0, b'bad shape'), ('N', 0, b'bad shape'),
                               ('Cin', 24, b'Cin=24'), ('Cin', 0, b'Cin=0'), ('Cout', 40, b'Cout=40'), ('Cout', 8, b'Cout=8'),
                               ('flags', 1, b'flags=1'), ('ldgy', 28, b'pitch'), ('ldgx', 12, b'pitch'), ('ldx', 12, b'pitch'),
                               ('ldgy', 34, b'16-byte aligned'), ('ldx', 18, b'16-byte aligned'),
                               ('gy', None, b'null pointer (gy)'), ('gy', odd, b'16-byte aligned'), ('x', None, b'null pointer (x)'),
                               ('x', odd, b'16-byte aligned'), ('gx', odd, b'16-byte aligned'),
                               ('w_s2t', None, b'null pointer (w_s2t)')):
        d = _s2_desc(p)
        setattr(d, field, value)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, field
        assert word in lib.ct_last_error(), (field, lib.ct_last_error())
        if field in ('H', 'W', 'N', 'Cin', 'Cout', 'flags'):
            assert query(ctypes.byref(d)) == 0, field
    d = _s2_desc(p)
    d.gx = d.gw = None
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'no output' in lib.ct_last_error()
    d = _s2_desc(p, N=8, H=512, W=512, Cin=256, Cout=32)             # x: 8 * 512 * 512 pixels * 256 * 4 = 2^31
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error()
    assert query(ctypes.byref(d)) == 0
    d = _s2_desc(p, N=8, H=512, W=512, Cin=16, Cout=1024)            # gy: 8 * 256 * 256 pixels * 1024 * 4 = 2^31
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error()
    assert query(ctypes.byref(_s2_desc(p, N=8, H=512, W=512, Cin=240, Cout=32))) > 0
    d = _s2_desc(p)                                                  # gw needs the workspace
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    pack, elems = lib.ct_pack_conv_weight_s2t, lib.ct_packed_conv_weight_s2t_elems
    assert elems(32, 16) == 9 * 32 * 16 and elems(24, 16) == 0 and elems(32, 8) == 0 and elems(0, 16) == 0
    assert pack(None, p, 32, 16, None) == _lib.CT_ERR_ARG and b'null pointer' in lib.ct_last_error()
    assert pack(p, None, 32, 16, None) == _lib.CT_ERR_ARG
    assert pack(p, p, 24, 16, None) == _lib.CT_ERR_ARG and b'Cout=24' in lib.ct_last_error()
    assert pack(p, p, 32, 8, None) == _lib.CT_ERR_ARG and b'Cin=8' in lib.ct_last_error()


def _bn_desc(p, N=2, H=5, W=7, C=64, ld=None, flags=3):
    from centertrack_amd import _lib
    d = _lib.BnActDesc()
    for f in ('z', 'mean', 'var', 'invstd', 'gamma', 'beta', 'y', 'gy', 'gz', 'ggamma', 'gbeta', 'res', 'gres'):
        setattr(d, f, p)
    d.N, d.H, d.W, d.C = N, H, W, C
    d.ldz = d.ldy = d.ldgy = d.ldgz = d.ldr = d.ldgres = ld or C
    d.flags = flags
    return d


def test_bn_act_entry_points_validate_their_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    query = lib.ct_bn_act_workspace_bytes
    for name, call in (('apply', lib.ct_bn_act_apply), ('backward', lib.ct_bn_act_backward)):
        assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
        for field, value, word in (('C', 6, b'C=6'), ('C', 0, b'bad shape'), ('N', 0, b'bad shape'), ('ldz', 60, b'pitch'),
                                   ('ldz', 66, b'16-byte aligned'), ('z', None, b'null pointer (z)'), ('z', odd, b'16-byte aligned'),
                                   ('mean', None, b'null pointer (mean)'), ('invstd', None, b'null pointer (invstd)'),
                                   ('gamma', None, b'(gamma)'), ('beta', None, b'(beta)'), ('flags', 4, b'flags=4'),
                                   ('ldr', 60, b'pitch'), ('res', odd, b'16-byte aligned')):
            d = _bn_desc(p)
            setattr(d, field, value)
            assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, (name, field)
            assert word in lib.ct_last_error(), (name, field, lib.ct_last_error())
        d = _bn_desc(p, N=8, H=256, W=256, C=1024)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error(), name
        assert query(ctypes.byref(d)) == 0
    assert query(None) == 0
    assert query(ctypes.byref(_bn_desc(p, N=8, H=256, W=256, C=1020))) > 0
    d = _bn_desc(p)
    d.y = None
    assert lib.ct_bn_act_apply(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'(y)' in lib.ct_last_error()
    for field, word in (('gy', b'(gy)'), ('ldgy', b'pitch'), ('ldgz', b'pitch'), ('ldgres', b'pitch')):
        d = _bn_desc(p)
        setattr(d, field, 8 if field.startswith('ld') else None)
        assert lib.ct_bn_act_backward(ctypes.byref(d), None) == _lib.CT_ERR_ARG and word in lib.ct_last_error()
    d = _bn_desc(p)
    d.gz = d.gres = d.ggamma = d.gbeta = None
    assert lib.ct_bn_act_backward(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'no output' in lib.ct_last_error()
    d = _bn_desc(p)                                                  # every backward that sums needs the workspace
    assert lib.ct_bn_act_backward(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
    assert lib.ct_bn_act_backward(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE


def test_maxpool_backward_validates_its_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    call = lib.ct_maxpool2x2_backward

    def run(x=p, N=2, H=6, W=10, C=16, ldx=16, gy=p, ldgy=16, add=p, ldadd=16, gx=p, ldgx=16):
        return call(x, N, H, W, C, ldx, gy, ldgy, add, ldadd, gx, ldgx, None)
    for kw, word in ((dict(x=None), b'null pointer (x)'), (dict(gy=None), b'null pointer (gy)'), (dict(gx=None), b'null pointer (gx)'),
                     (dict(H=5), b'must be even'), (dict(W=9), b'must be even'), (dict(C=6), b'C=6'), (dict(N=0), b'bad shape'),
                     (dict(ldx=12), b'pitch'), (dict(ldgy=18), b'16-byte aligned'), (dict(ldadd=12), b'pitch'), (dict(ldgx=8), b'pitch'),
                     (dict(x=odd), b'16-byte aligned'), (dict(add=odd), b'16-byte aligned'), (dict(gx=odd), b'16-byte aligned'),
                     (dict(N=8, H=256, W=256, C=1024, ldx=1024, ldgy=1024, ldadd=1024, ldgx=1024), b'2 GiB')):
        assert run(**kw) == _lib.CT_ERR_ARG, kw
        assert word in lib.ct_last_error(), (kw, lib.ct_last_error())


def test_the_restated_plans_give_the_librarys_workspace_sizes(lib):
    keep, p = _ptr()
    s2 = list(BB.S2_SHAPES)
    bn = [(N, H, W, C) for N, H, W, C in BB.BN_SHAPES]
    for N, H, W in [(2, 64, 64)] + BB.bench_shapes():
        for call in BB.dla_units(N, H, W):
            (s2 if call[0] == 's2' else bn).append(call[1:])
    s2 += [(2, 8, 12, 32, 64), (2, 16, 24, 32, 64), (2, 16, 16, 64, 128)]          # the module cases
    assert len(set(s2)) >= 20 and len(set(bn)) >= 20
    for N, H, W, Cin, Cout in sorted(set(s2)):
        d = _s2_desc(p, N, H, W, Cin, Cout)
        assert lib.ct_conv2d_s2_backward_workspace_bytes(ctypes.byref(d)) == BB.s2_plan(N, H, W, Cin, Cout)['bytes'] > 0, (N, H, W, Cin, Cout)
        d.ldx = d.ldgx = Cin + 16                                    # the pitch does not change the plan
        d.gx = d.gw = None                                           # nor does what is asked for
        assert lib.ct_conv2d_s2_backward_workspace_bytes(ctypes.byref(d)) == BB.s2_plan(N, H, W, Cin, Cout)['bytes']
    for N, H, W, C in sorted(set(bn)):
        for flags in (0, 1, 2, 3):
            d = _bn_desc(p, N, H, W, C, flags=flags)
            assert lib.ct_bn_act_workspace_bytes(ctypes.byref(d)) == BB.bn_plan(N, H, W, C)['bytes'] > 0, (N, H, W, C)
    # the regimes the GPU shapes reach: one slab and several, a tile remainder in both axes, one cell row and column
    plans = [BB.s2_plan(*s) for s in BB.S2_SHAPES]
    assert [(v['gx_units'], v['gw_units'], v['slabs']) for v in plans] == [(2, 9, 1), (2, 36, 1), (24, 576, 1), (15, 9, 5)]
    assert BB.s2_plan(4, 512, 512, 16, 32)['slabs'] == 114 and BB.s2_plan(4, 32, 32, 256, 512)['slabs'] == 2


def _production_calls():
    """the stride-2 (N, H, W, Cin, Cout), BatchNorm (N, H, W, C) and pool (N, H, W, C) calls of a DLA-34 training step at the
    two shapes of the backbone benchmark"""
    s2, bn, pool = [], [], []
    for N, H, W in BB.bench_shapes():
        for call in BB.dla_units(N, H, W):
            (s2 if call[0] == 's2' else bn).append(call[1:])
        for lv in range(2, 6):                                       # the pool in front of every ``Tree`` reads the level below
            pool.append((N, H >> (lv - 1), W >> (lv - 1), BB.DLA34['channels'][lv - 1]))
    return sorted(set(s2)), sorted(set(bn)), sorted(set(pool))


def test_the_gpu_shapes_reach_every_regime_of_the_plans():
    """``_backbone_bwd.S2_REGIMES`` / ``POOL_REGIMES`` / ``BN_REGIMES`` against every shape the GPU op tests run; every new shape
    is there for a regime nothing else reaches; and what a production call reaches, a GPU shape reaches.  2048 * 256, the
    quad count from which ``ew_grid`` caps the element-wise grids, is not observable through the ABI: ``_neck_bwd.EW_CAP``
    mirrors it by reading."""
    s2_all, pool_all = BB.S2_SHAPES + BB.S2_PLAN_SHAPES, BB.POOL_SHAPES + BB.POOL_PLAN_SHAPES
    assert BB.missing_s2_regimes(s2_all) == []
    assert BB.missing_pool_regimes(pool_all) == []
    assert BB.missing_bn_regimes(BB.gpu_bn_shapes()) == []
    assert set(BB.missing_s2_regimes(BB.S2_SHAPES)) >= {
        'slabs from cdiv(1024, units)', 'stepsPerWave % 4 == 3', 'a whole idle slab',
        'nco < 4 in a cout group other than the first', 'Cin % 32 == 16 with more than one channel group',
        'Cout % 64 != 0 with Cout > 64', 'Wo % 16 == 0 and Ho % 4 == 0'}                           # what the toy shapes left out
    assert 'grid capped' in BB.missing_pool_regimes(BB.POOL_SHAPES)
    for i, s in enumerate(BB.S2_PLAN_SHAPES):
        assert BB.missing_s2_regimes(BB.S2_SHAPES + BB.S2_PLAN_SHAPES[:i] + BB.S2_PLAN_SHAPES[i + 1:]) != [], s
    s2, bn, pool = _production_calls()
    assert set(BB.reached_s2_regimes(s2)) <= set(BB.reached_s2_regimes(s2_all))
    assert set(BB.reached_bn_regimes(bn)) <= set(BB.reached_bn_regimes(BB.gpu_bn_shapes()))
    assert set(BB.reached_pool_regimes(pool)) <= set(BB.reached_pool_regimes(pool_all))
    assert {'slabs from cdiv(1024, units)', 'a whole idle wave'} <= set(BB.reached_s2_regimes(s2))   # production is past the toy sizes
    assert 'element-wise grid capped' in BB.reached_bn_regimes(bn) and 'grid capped' in BB.reached_pool_regimes(pool)
    # the figures the comments of the shape lists give
    a, b, c, d = (BB.s2_plan(*s) for s in BB.S2_PLAN_SHAPES)
    assert (a['gw_units'], a['wanted'], a['maxSlabs'], a['slabs'], a['stepsPerWave'], a['nsteps']) == (36, 29, 38, 29, 11, 1200)
    assert (a['idle_waves'], a['idle_slabs']) == (6, 1)
    assert (b['gw_units'], b['slabs'], b['stepsPerWave'], b['cogroups']) == (576, 2, 36, 8)
    assert (c['cgroups'], c['cogroups'], c['nco_last'], c['slabs']) == (2, 2, 1, 1)
    assert (d['Wo'], d['Ho'], d['gx_units'], d['stepsPerWave']) == (16, 4, 1, 4)
    assert BB.pool_plan(*BB.POOL_PLAN_SHAPES[0])['quads'] == 549120 and BB.pool_plan(*BB.POOL_PLAN_SHAPES[0])['ew_ragged']


def test_the_restated_plans_give_the_librarys_workspace_sizes_at_the_plan_shapes(lib):
    keep, p = _ptr()
    for N, H, W, Cin, Cout in BB.S2_PLAN_SHAPES:
        d = _s2_desc(p, N, H, W, Cin, Cout)
        assert lib.ct_conv2d_s2_backward_workspace_bytes(ctypes.byref(d)) == BB.s2_plan(N, H, W, Cin, Cout)['bytes'] > 0, (N, H, W, Cin, Cout)
        d.ldx, d.ldgx, d.ldgy = Cin + 32, Cin + 20, Cout + 8         # the pitches of the channel-slice test change no plan
        assert lib.ct_conv2d_s2_backward_workspace_bytes(ctypes.byref(d)) == BB.s2_plan(N, H, W, Cin, Cout)['bytes']
    for N, H, W, C in BB.BN_PLAN_SHAPES:
        for flags in (0, 1, 2, 3):
            d = _bn_desc(p, N, H, W, C, flags=flags)
            assert lib.ct_bn_act_workspace_bytes(ctypes.byref(d)) == BB.bn_plan(N, H, W, C)['bytes'] > 0, (N, H, W, C)


@pytest.mark.parametrize('batch', [True, False], ids=['batch-stats', 'running-stats'])
@pytest.mark.parametrize('shape', BB.BN_PLAN_SHAPES, ids=str)
def test_the_float32_reference_stays_inside_the_mask_cap_at_the_plan_shapes(shape, batch):
    """what tests/test_hip_backbone_backward.py holds the HIP forward's ReLU mask to (``check_mask``: flips only within 64 e32
    of 0, on at most 0.1 % of the map), held by the float32 CPU run of the same case with its residual"""
    case = BB.bn_case(shape)
    (pre64, y64), (pre32, y32) = (BB._neck_bwd.bn_free_run(case, dt, batch, residual=True) for dt in (torch.float64, torch.float32))
    flipped, near = BB.check_mask(pre32 > 0, pre64, BB.err(y32, y64), str(shape))
    print('%s: fp32 torch flips %d units, %d of %d within the threshold' % (shape, flipped, near, pre64.numel()))


def test_the_capped_pool_case_is_full_of_ties():
    """the tie rule at the shape whose grid is capped: torch's backward equals the explicit first-maximum sums bit for bit, and
    half of the windows tie"""
    N, H, W, C = BB.POOL_PLAN_SHAPES[0]
    x = BB.tie_input(41, N, C, H, W)
    assert BB.tie_fraction(x) >= 0.3
    gy = BB.randn(42, N, C, H // 2, W // 2).float()
    xt = x.clone().requires_grad_()
    gx, = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, gy)
    assert torch.equal(BB.pool_backward_formula(x, gy), gx)


def test_module_names_shapes_and_initialisation():
    from centertrack_amd import dla_base
    m = dla_base.dla34(pretrained=False, opt=BB.Opt())
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'dla34_base_keys.json')))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    assert [k for k, _ in m.named_buffers()] == [k for k, _ in want if BB.is_buffer(k)]
    # torch's defaults: Conv2d weights uniform in +-fan_in^-1/2 (kaiming_uniform, a = sqrt 5), BatchNorm 1 / 0 / 0 / 1 / 0
    for k, v in m.state_dict().items():
        leaf = k.rsplit('.', 1)[1]
        if v.dim() == 4:
            b = (v.shape[1] * v.shape[2] * v.shape[3]) ** -0.5
            assert float(v.abs().max()) <= b * (1 + 2.0 ** -22), k      # (the limit itself is rounded to fp32)
            if v.numel() >= 4096:
                assert abs(float(v.std()) / (b / 3 ** 0.5) - 1) < 0.05 and abs(float(v.mean())) < 0.05 * b, k
        elif leaf in ('weight', 'running_var'):
            assert bool((v == 1).all()), k
        else:
            assert bool((v == 0).all()), k
    assert all(mod.momentum == 0.1 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    assert all(mod.bias is None for mod in m.modules() if isinstance(mod, torch.nn.Conv2d))
    # without the optional stems their keys are absent, as in the reference
    plain = dla_base.DLA(BB.DLA34['levels'], BB.DLA34['channels'], opt=None)
    assert not any(k.startswith('pre_') for k in plain.state_dict())
    # signatures
    import inspect
    assert list(inspect.signature(dla_base.BasicBlock.__init__).parameters)[1:] == ['inplanes', 'planes', 'stride', 'dilation']
    assert list(inspect.signature(dla_base.Root.__init__).parameters)[1:] == ['in_channels', 'out_channels', 'kernel_size', 'residual']
    assert list(inspect.signature(dla_base.Tree.__init__).parameters)[1:] == [
        'levels', 'block', 'in_channels', 'out_channels', 'stride', 'level_root', 'root_dim', 'root_kernel_size', 'dilation',
        'root_residual']
    assert list(inspect.signature(dla_base.DLA.__init__).parameters)[1:] == [
        'levels', 'channels', 'num_classes', 'block', 'residual_root', 'linear_root', 'opt']
    assert list(inspect.signature(dla_base.DLA.forward).parameters)[1:] == ['x', 'pre_img', 'pre_hm']
    assert list(inspect.signature(dla_base.Tree.forward).parameters)[1:] == ['x', 'residual', 'children']
    assert list(inspect.signature(dla_base.BasicBlock.forward).parameters)[1:] == ['x', 'residual']
    assert dla_base.trace is None


def test_what_the_modules_refuse(tmp_path):
    from centertrack_amd import dla_base
    from centertrack_amd._lib import CTError
    with pytest.raises(CTError, match='dilation'):
        dla_base.BasicBlock(32, 32, 1, dilation=2)
    with pytest.raises(CTError, match='dilation'):
        dla_base.Tree(1, dla_base.BasicBlock, 32, 64, 2, dilation=2)
    with pytest.raises(CTError, match='BasicBlock'):
        dla_base.Tree(1, torch.nn.Identity, 32, 64, 2)
    with pytest.raises(CTError, match='BasicBlock'):
        dla_base.DLA(BB.DLA34['levels'], BB.DLA34['channels'], block=torch.nn.Identity, opt=BB.Opt())
    with pytest.raises(CTError, match='nothing is downloaded'):
        dla_base.dla34(pretrained=True, opt=BB.Opt())
    with pytest.raises(CTError, match='nothing is downloaded'):
        dla_base.dla34(opt=BB.Opt())                                  # the reference's default is pretrained=True
    m = dla_base.dla34(pretrained=False, opt=BB.Opt())
    with pytest.raises(CTError, match='local .pth'):
        m.load_pretrained_model()                                     # the reference would fetch dla34-ba72cf86 here
    # a local file loads as in the reference: non-strict, with an ``fc`` sized by the file's last tensor
    sd = {k: torch.full_like(v, 0.5) for k, v in m.state_dict().items() if k.startswith('level0.')}
    sd['fc.weight'], sd['fc.bias'] = torch.zeros(10, 512, 1, 1), torch.zeros(10)
    torch.save(sd, str(tmp_path / 'local.pth'))
    m.load_pretrained_model(data=str(tmp_path) + os.sep, name='local.pth')
    assert float(m.level0[0].weight.detach().mean()) == 0.5 and tuple(m.fc.weight.shape) == (10, 512, 1, 1)
    with pytest.raises(CTError, match='no CPU fallback'):
        dla_base.BasicBlock(32, 32)(torch.zeros(1, 32, 4, 4))


@pytest.mark.parametrize('shape', BB.S2_SHAPES + [(1, 2, 6, 16, 16)], ids=str)
def test_the_parity_decomposition_is_the_stride_2_input_gradient(shape):
    N, H, W, Cin, Cout = shape
    x = BB.randn(1, N, Cin, H, W).requires_grad_()
    w = BB.randn(2, Cout, Cin, 3, 3).requires_grad_()
    gy = BB.randn(3, N, Cout, H // 2, W // 2)
    gx, gw = torch.autograd.grad(F.conv2d(x, w, None, 2, 1), (x, w), gy)
    assert BB.err(BB.conv_s2_gx_formula(gy, w.detach(), H, W), gx) < 1e-13
    assert BB.err(BB.conv_s2_gw_formula(x.detach(), gy), gw) < 1e-13


def _tie_input(seed, N, C, H, W):
    """a post-ReLU map: most windows all zero, some with equal positive values, some -0.0"""
    x = torch.relu(BB.randn(seed, N, C, H, W) - 1.0)
    x[:, :, 0:2, 0:2] = 0.75                                          # a window of equal positive values
    x[:, 0::2, -2, -2] = -0.0                                         # -0.0 ahead of 0 in an all-zero window ties
    x[:, 1::2, -1, -1] = -0.0
    return x


@pytest.mark.parametrize('shape', BB.POOL_SHAPES, ids=str)
def test_the_tie_rule_is_torchs(shape):
    N, H, W, C = shape
    x = _tie_input(5, N, C, H, W)
    assert BB.tie_fraction(x) >= 0.3
    gy, add = BB.randn(6, N, C, H // 2, W // 2), BB.randn(7, N, C, H, W)
    for dt in (torch.float64, torch.float32):
        xt = x.to(dt).requires_grad_()
        y = F.max_pool2d(xt, 2, 2)
        gx, = torch.autograd.grad(y, xt, gy.to(dt))
        assert torch.equal(BB.pool_backward_formula(x.to(dt), gy.to(dt)), gx)
        assert torch.equal(BB.pool_backward_formula(x.to(dt), gy.to(dt), add.to(dt)), gx + add.to(dt))
    # equal values send the gradient to the top-left; -0.0 ties with 0
    flat = torch.zeros(1, 1, 2, 2, dtype=torch.float64)
    flat[0, 0, 0, 0] = -0.0
    for t in (torch.full((1, 1, 2, 2), 3.0, dtype=torch.float64), flat, -flat):
        t = t.clone().requires_grad_()
        g, = torch.autograd.grad(F.max_pool2d(t, 2, 2), t, torch.ones(1, 1, 1, 1, dtype=torch.float64))
        assert g.flatten().tolist() == [1.0, 0.0, 0.0, 0.0]
        assert BB.pool_selection(t.detach()).item() == 0


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('name', list(BB.MODULES))
def test_the_float32_reference_stays_inside_the_mask_and_selection_cap(name, training):
    """what the GPU tests hold the HIP forward's masks and selections to, held by the float32 CPU run of the construction for
    the seeds those tests use: a float64 run that is handed the float32 run's maps differs from the free float64 run only next
    to 0 / next to a tie, on at most 0.1 % of a map"""
    from centertrack_amd import dla_base
    sd = BB.random_params(BB.SEEDS[name], BB.MODULES[name][0](dla_base))
    inputs = BB.module_inputs(name, BB.SEEDS[name] + 1)
    free64, free32 = (BB.reference(name, sd, inputs, None, training, dt) for dt in (torch.float64, torch.float32))
    given = BB.reference(name, sd, inputs, None, training, torch.float64, maps=free32['tape'].out)
    flips, wins = BB.check_tape(name, given['tape'], free64['tape'], free32['tape'])
    print('%s %s: %d ReLU units flipped, %d pool windows differ' % (name, 'train' if training else 'eval', flips, wins))
    pools = free64['tape'].pools
    assert len(pools) == {'tree-1': 1, 'tree-2': 2, 'dla34': 6}.get(name, 0)
    if pools:                                                        # the pooled maps are post-ReLU: full of exact ties
        assert min(BB.tie_fraction(x) for x, _, _ in pools) > 0.01


def test_the_sgd_case_moves_every_parameter():
    """tests/test_hip_backbone_backward.py::test_tree_three_sgd_steps on the float64 construction alone: every tensor a
    gradient reaches moves by more than 5e-4 of its maximum in three steps, a hundred times the bound"""
    moved = BB.sgd_trajectory(torch.float64, None)[1]
    print({k: '%.1e' % v for k, v in moved.items()})
    assert all(v > 5e-4 for k, v in moved.items() if not k.startswith('project.'))
    assert all(v == 0.0 for k, v in moved.items() if k.startswith('project.') and not BB.is_buffer(k))
