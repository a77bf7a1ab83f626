"""CPU: the host side of the trainable neck (centertrack_amd/csrc/bn_train.hip, centertrack_amd/csrc/neck_bwd.hip, centertrack_amd/dla_up.py) -- exports and
descriptor layouts, argument validation and workspace queries of the BatchNorm, up-sampling-backward and mask-sigmoid entry
points, the restated slab plans against those queries, the names, shapes and initialisation of DeformConv / IDAUp / DLAUp, and
the float64 helper's up-sampling formula against autograd.  Nothing here launches a kernel."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _neck_bwd as NB

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NEW = ['ct_bn_stats', 'ct_bn_relu_apply', 'ct_bn_relu_backward', 'ct_bn_workspace_bytes', 'ct_upsample_add_backward',
       'ct_upsample_add_backward_workspace_bytes', 'ct_dcn_mask_sigmoid_backward']


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


def test_ctypes_descriptors_match_the_header_layout(tmp_path):
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    checks = {'ct_bn_desc': _lib.BnDesc, 'ct_upsample_bwd_desc': _lib.UpsampleBwdDesc}
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
    assert _lib.CT_BN_BATCH_STATS == 1


def _bn_desc(p, N=2, H=5, W=7, C=64, ld=None):
    from centertrack_amd import _lib
    d = _lib.BnDesc()
    for f in ('z', 'mean', 'var', 'invstd', 'gamma', 'beta', 'y', 'gy', 'gz', 'ggamma', 'gbeta'):
        setattr(d, f, p)
    d.N, d.H, d.W, d.C = N, H, W, C
    d.ldz = d.ldy = d.ldgy = d.ldgz = ld or C
    d.eps = 1e-5
    return d


def test_bn_entry_points_validate_their_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    query = lib.ct_bn_workspace_bytes
    calls = {'stats': lib.ct_bn_stats, 'apply': lib.ct_bn_relu_apply, 'backward': lib.ct_bn_relu_backward}
    for name, call in calls.items():
        assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
        for field, value, word in (('C', 6, b'C=6'), ('C', 0, b'bad shape'), ('N', 0, b'bad shape'), ('ldz', 60, b'pitch'),
                                   ('ldz', 66, b'16-byte aligned'), ('z', None, b'null pointer (z)'), ('z', odd, b'16-byte aligned'),
                                   ('mean', None, b'null pointer (mean)'), ('invstd', None, b'null pointer (invstd)'),
                                   ('flags', 2, b'flags=2')):
            d = _bn_desc(p)
            setattr(d, field, value)
            assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, (name, field)
            assert word in lib.ct_last_error(), (name, field, lib.ct_last_error())
        # a view of 2 GiB: 32-bit offsets cannot address it
        d = _bn_desc(p, N=8, H=256, W=256, C=1024)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error(), name
        assert query(ctypes.byref(d)) == 0
    assert query(None) == 0
    d = _bn_desc(p, N=8, H=256, W=256, C=1020)
    assert query(ctypes.byref(d)) > 0
    for field, word in (('gamma', b'(gamma)'), ('beta', b'(beta)'), ('y', b'(y)')):
        d = _bn_desc(p)
        setattr(d, field, None)
        assert lib.ct_bn_relu_apply(ctypes.byref(d), None) == _lib.CT_ERR_ARG and word in lib.ct_last_error()
    for field, word in (('gamma', b'(gamma)'), ('gy', b'(gy)'), ('ldgy', b'pitch'), ('ldgz', b'pitch')):
        d = _bn_desc(p)
        setattr(d, field, 8 if field.startswith('ld') else None)
        assert lib.ct_bn_relu_backward(ctypes.byref(d), None) == _lib.CT_ERR_ARG and word in lib.ct_last_error()
    d = _bn_desc(p)
    d.gz = d.ggamma = d.gbeta = None
    assert lib.ct_bn_relu_backward(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'no output' in lib.ct_last_error()
    d = _bn_desc(p)
    d.var = None
    assert lib.ct_bn_stats(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'(var)' in lib.ct_last_error()
    # statistics and every backward that sums need the workspace; the running-statistics gz alone does not reach that check
    for call in (lib.ct_bn_stats, lib.ct_bn_relu_backward):
        d = _bn_desc(p)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
        d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE


def _up_desc(p, N=2, H=5, W=7, C=64, f=2):
    from centertrack_amd import _lib
    d = _lib.UpsampleBwdDesc()
    d.gy = d.w = d.gx = d.x = d.gw = p
    d.N, d.H, d.W, d.C, d.f = N, H, W, C, f
    d.ldgy = d.ldgx = d.ldx = C
    return d


def test_upsample_backward_and_mask_sigmoid_validate_their_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    call, query = lib.ct_upsample_add_backward, lib.ct_upsample_add_backward_workspace_bytes
    assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    assert query(None) == 0
    for field, value, word in (('f', 3, b'f=3'), ('f', 1, b'f=1'), ('f', 16, b'f=16'), ('C', 6, b'C=6'), ('H', 0, b'bad shape'),
                               ('ldgy', 60, b'pitch'), ('ldgx', 60, b'pitch'), ('ldx', 62, b'pitch'), ('ldgy', 66, b'16-byte aligned'),
                               ('gy', None, b'null pointer (gy)'), ('gy', odd, b'16-byte aligned'), ('x', odd, b'16-byte aligned'),
                               ('w', None, b'null pointer (w)'), ('x', None, b'null pointer (x)')):
        d = _up_desc(p)
        setattr(d, field, value)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, field
        assert word in lib.ct_last_error(), (field, lib.ct_last_error())
        if field in ('f', 'C', 'H'):
            assert query(ctypes.byref(d)) == 0, field
    d = _up_desc(p)
    d.gx = d.gw = None
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'no output' in lib.ct_last_error()
    d = _up_desc(p, N=8, H=128, W=128, C=1024, f=2)                 # gy: 8 * 256 * 256 pixels * 1024 * 4 = 2^31
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error()
    assert query(ctypes.byref(d)) == 0
    d = _up_desc(p)                                                 # gw needs the workspace, gx alone does not
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    sig = lib.ct_dcn_mask_sigmoid_backward
    assert sig(None, 32, p, 32, 1, 4, 4, None) == _lib.CT_ERR_ARG and b'null pointer' in lib.ct_last_error()
    assert sig(p, 32, None, 32, 1, 4, 4, None) == _lib.CT_ERR_ARG
    assert sig(p, 24, p, 32, 1, 4, 4, None) == _lib.CT_ERR_ARG and b'pitch' in lib.ct_last_error()
    assert sig(p, 32, p, 32, 0, 4, 4, None) == _lib.CT_ERR_ARG and b'bad shape' in lib.ct_last_error()
    assert sig(p, 32, p, 32, 64, 512, 512, None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error()


def test_the_restated_plans_give_the_librarys_workspace_sizes(lib):
    keep, p = _ptr()
    bn = [(N, H, W, C) for N, H, W, C in NB.BN_SHAPES] + [(N, H, W, co) for N, H, W, ci, co in NB.DEFORM_SHAPES]
    up = [(N, H, W, C, f) for N, H, W, C in NB.UP_SHAPES for f in (2, 4, 8)]
    cfgs = [(NB.IDA['o'], NB.IDA['channels'], NB.IDA['up_f'], NB.IDA['N'], NB.IDA['sizes'])]
    cfgs += [(o, ch, uf, b, sizes) for _, b, o, ch, uf, sizes in NB.bench_shapes()]
    for i, o, inc, uf in NB.dlaup_structure(NB.DLAUP['channels'], NB.DLAUP['scales']):
        cfgs.append((o, inc, uf, NB.DLAUP['N'], NB.DLAUP['sizes'][-len(inc):]))
    for cfg in cfgs:
        for call in NB.ida_nodes(*cfg):
            (bn if call[0] == 'bn' else up).append(call[1:])
    assert len(set(bn)) >= 12 and len(set(up)) >= 12
    for N, H, W, C in sorted(set(bn)):
        d = _bn_desc(p, N, H, W, C)
        assert lib.ct_bn_workspace_bytes(ctypes.byref(d)) == NB.bn_plan(N, H, W, C)['bytes'] > 0, (N, H, W, C)
        d = _bn_desc(p, N, H, W, C, ld=C + 8)                       # the pitch does not change the plan
        assert lib.ct_bn_workspace_bytes(ctypes.byref(d)) == NB.bn_plan(N, H, W, C)['bytes']
    for N, H, W, C, f in sorted(set(up)):
        d = _up_desc(p, N, H, W, C, f)
        assert lib.ct_upsample_add_backward_workspace_bytes(ctypes.byref(d)) == NB.up_plan(N, H, W, C, f)['bytes'] > 0, (N, H, W, C, f)
    # the regimes the GPU shapes reach: one slab and several, one chunk and two, rows that do not fill the workgroup
    a, b, c = (NB.bn_plan(*s) for s in NB.BN_SHAPES)
    assert (a['cw'], a['rows'], a['chunks'], a['slabs']) == (16, 16, 1, 2)
    assert (b['cw'], b['rows'], b['chunks'], b['slabs']) == (33, 7, 1, 11) and 33 * 7 < 256
    assert (c['cw'], c['rows'], c['chunks'], c['slabs']) == (2, 128, 1, 5)
    assert NB.bn_plan(4, 128, 128, 64)['slabs'] == 512 and NB.bn_plan(1, 8, 8, 512)['chunks'] == 2
    u = [NB.up_plan(*s, 2) for s in NB.UP_SHAPES]
    assert [(v['chunks'], v['slabs']) for v in u] == [(1, 9), (1, 9), (3, 1)]


def _production_calls():
    """the BatchNorm (N, H, W, C) and up-sampling (N, H, W, C, f) calls of the two ``IDAUp`` of the neck benchmark, batch 1 and 4"""
    bn, up = [], []
    for _, b, o, ch, uf, sizes in NB.bench_shapes():
        for call in NB.ida_nodes(o, ch, uf, b, sizes):
            (bn if call[0] == 'bn' else up).append(call[1:])
    return sorted(set(bn)), sorted(set(up))


def test_the_gpu_shapes_reach_every_regime_of_the_plans():
    """``_neck_bwd.BN_REGIMES`` / ``UP_REGIMES`` against every shape the GPU op tests run; every new shape is there for a
    regime nothing else reaches; and what a production call reaches, a GPU shape reaches.  2048 * 256, the quad count from
    which ``ew_grid`` caps the element-wise grids, is not observable through the ABI: ``_neck_bwd.EW_CAP`` mirrors it by
    reading."""
    assert NB.missing_bn_regimes(NB.gpu_bn_shapes()) == []
    assert NB.missing_up_regimes(NB.gpu_up_shapes()) == []
    assert set(NB.missing_bn_regimes(NB.BN_SHAPES)) >= {
        'slabs from the grid target', 'slabs == 1', 'slabs == 512', 'chunks == 2', 'element-wise grid capped',
        'element-wise grid capped, total not a multiple of 2048 * 256'}                # what the toy shapes left out
    assert set(NB.missing_up_regimes([s + (f,) for s in NB.UP_SHAPES for f in (2, 4, 8)])) >= {
        'slabs from the grid target', 'up_gx grid capped'}
    for i, s in enumerate(NB.BN_PLAN_SHAPES):
        assert NB.missing_bn_regimes(NB.BN_SHAPES + NB.BN_PLAN_SHAPES[:i] + NB.BN_PLAN_SHAPES[i + 1:]) != [], s
    small = [s + (f,) for s in NB.UP_SHAPES for f in (2, 4, 8)]
    for i, s in enumerate(NB.UP_PLAN_SHAPES):
        rest = NB.UP_PLAN_SHAPES[:i] + NB.UP_PLAN_SHAPES[i + 1:]
        assert NB.missing_up_regimes(small + [t + (f,) for t, f in rest]) != [], s
    bn, up = _production_calls()
    assert set(NB.reached_bn_regimes(bn)) <= set(NB.reached_bn_regimes(NB.gpu_bn_shapes()))
    assert set(NB.reached_up_regimes(up)) <= set(NB.reached_up_regimes(NB.gpu_up_shapes()))
    assert {'slabs == 512', 'element-wise grid capped'} <= set(NB.reached_bn_regimes(bn))        # production is past the toy sizes
    # the figures the comments of the shape lists give
    a, b, c, d = (NB.bn_plan(*s) for s in NB.BN_PLAN_SHAPES)
    assert (a['slabs'], a['pixPerSlab'], a['last_slab_pixels'], a['quads'], a['ew_grid']) == (512, 384, 372, 786384, 2048)
    assert (b['chunks'], b['wanted'], b['slabs'], b['quads']) == (2, 256, 231, 591360)
    assert (c['cw'], c['dead_threads'], c['slabs'], c['quads']) == (33, 25, 484, 558360)
    assert (d['slabs'], d['last_slab_pixels'], d['pixPerSlab']) == (1, 240, 256)
    u = [NB.up_plan(*s, f) for s, f in NB.UP_PLAN_SHAPES]
    assert [(v['chunks'], v['wanted'], v['slabs']) for v in u] == [(1, 512, 480), (3, 171, 160), (1, 512, 512)]
    assert [v['ew_capped'] for v in u] == [False, False, True] and u[2]['quads'] == 540672
    assert NB.ew_plan(NB.EW_CAP - 1) == dict(quads=NB.EW_CAP - 1, ew_capped=False, ew_grid=2048, ew_ragged=False)
    assert NB.ew_plan(NB.EW_CAP)['ew_capped'] and not NB.ew_plan(NB.EW_CAP)['ew_ragged']


def test_the_restated_plans_give_the_librarys_workspace_sizes_at_the_plan_shapes(lib):
    keep, p = _ptr()
    for N, H, W, C in NB.BN_PLAN_SHAPES:
        for ld in (None, C + 8):
            d = _bn_desc(p, N, H, W, C, ld=ld)
            assert lib.ct_bn_workspace_bytes(ctypes.byref(d)) == NB.bn_plan(N, H, W, C)['bytes'] > 0, (N, H, W, C)
    for (N, H, W, C), f in NB.UP_PLAN_SHAPES:
        d = _up_desc(p, N, H, W, C, f)
        assert lib.ct_upsample_add_backward_workspace_bytes(ctypes.byref(d)) == NB.up_plan(N, H, W, C, f)['bytes'] > 0, (N, H, W, C, f)


@pytest.mark.parametrize('batch', [True, False], ids=['batch-stats', 'running-stats'])
@pytest.mark.parametrize('shape', NB.BN_PLAN_SHAPES, ids=str)
def test_the_float32_reference_stays_inside_the_mask_cap_at_the_plan_shapes(shape, batch):
    """what tests/test_hip_neck_backward.py holds the HIP forward's ReLU mask to (``check_mask``: flips only within 64 e32 of
    0, on at most 0.1 % of the map), held by the float32 CPU run of the same case"""
    case = NB.bn_case(shape)
    (pre64, y64), (pre32, y32) = (NB.bn_free_run(case, dt, batch) for dt in (torch.float64, torch.float32))
    flipped, near = NB.check_mask(pre32 > 0, pre64, NB.err(y32, y64), str(shape))
    print('%s: fp32 torch flips %d units, %d of %d within the threshold' % (shape, flipped, near, pre64.numel()))


def test_module_names_shapes_and_initialisation():
    from centertrack_amd import dla_up, model, weights
    from centertrack_amd._lib import CTError
    torch.manual_seed(5)
    ref = model.DLASegHIP(weights.MOT_HEADS).state_dict()
    ida = dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4])
    dup = dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8])
    for mod, prefix in ((ida, 'ida_up.'), (dup, 'dla_up.')):
        want = sorted((k, tuple(v.shape)) for k, v in ref.items() if k.startswith(prefix))
        got = sorted((prefix + k, tuple(v.shape)) for k, v in mod.state_dict().items())
        assert got == want and len(got) > 20, prefix
    assert set(NB.ida_params(1, 64, [64, 128, 256], [1, 2, 4])) == set(ida.state_dict())
    assert set(NB.dlaup_params(1, [64, 128, 256, 512], [1, 2, 4, 8])) == set(dup.state_dict())
    d = dla_up.DeformConv(128, 64)
    assert sorted(d.state_dict()) == sorted(NB.deform_keys(''))
    bn = d.actf[0]
    assert isinstance(bn, torch.nn.BatchNorm2d) and bn.momentum == 0.1 and bn.eps == 1e-5
    assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all()) and bool((bn.running_var == 1).all())
    assert float(d.conv.conv_offset_mask.weight.detach().abs().max()) == 0 and float(d.conv.conv_offset_mask.bias.detach().abs().max()) == 0
    assert isinstance(d.conv.conv_offset_mask, torch.nn.Conv2d) and float(d.conv.weight.detach().abs().max()) > 0
    for k, f in ((1, 2), (2, 4)):
        up = getattr(ida, 'up_%d' % k)
        assert isinstance(up, torch.nn.ConvTranspose2d) and up.groups == 64 and up.stride == (f, f) and up.padding == (f // 2, f // 2)
        c = (2 * f - 1 - f % 2) / (2.0 * f)
        want = torch.tensor([[(1 - abs(i / f - c)) * (1 - abs(j / f - c)) for j in range(2 * f)] for i in range(2 * f)])
        assert torch.allclose(up.weight[0, 0], want, atol=1e-7) and torch.equal(up.weight[63], up.weight[0])
    with pytest.raises(CTError):
        dla_up.IDAUp(64, [64, 128], [1, 3])
    with pytest.raises(CTError, match='no CPU fallback'):
        d(torch.zeros(1, 128, 4, 4))
    with pytest.raises(CTError, match='no CPU fallback'):
        ida([torch.zeros(1, 64, 8, 8), torch.zeros(1, 128, 4, 4), torch.zeros(1, 256, 2, 2)], 0, 3)


def test_the_upsampling_formula_of_the_helper_is_autograd():
    for (N, H, W, C), f in ((NB.UP_SHAPES[0], 2), (NB.UP_SHAPES[0], 4), (NB.UP_SHAPES[2], 8), ((1, 4, 5, 4), 8)):
        x = NB.randn(1, N, C, H, W).requires_grad_()
        w = NB.randn(2, C, 1, 2 * f, 2 * f).requires_grad_()
        skip = NB.randn(3, N, C, H * f, W * f).requires_grad_()
        gy = NB.randn(4, N, C, H * f, W * f)
        y = NB.upsample_add(x, w, f, skip)
        gx, gw, gs = torch.autograd.grad(y, (x, w, skip), gy)
        fx, fw = NB.upsample_backward_formula(x.detach(), w.detach(), f, gy)
        assert NB.err(fx, gx) < 1e-14 and NB.err(fw, gw) < 1e-14 and torch.equal(gs, gy)
        assert torch.equal(y, F.conv_transpose2d(x, w, stride=f, padding=f // 2, groups=C) + skip)


def test_the_reference_construction_meets_its_own_conditions():
    """what the GPU tests assume of the float64 / float32 constructions at the module shapes: designed sample coordinates
    stay 0.1 away from an integer, and fp32 torch flips no ReLU unit away from 0"""
    c = NB.IDA
    sd = NB.ida_params(11, c['o'], c['channels'], c['up_f'])
    layers = [NB.randn(20 + i, c['N'], ch, h, w).float() for i, (ch, (h, w)) in enumerate(zip(c['channels'], c['sizes']))]
    runs = {}
    for dt in (torch.float64, torch.float32):
        tr = NB.Trace()
        ls = [l.to(dt) for l in layers]
        with torch.no_grad():
            NB.ida(ls, NB.cast(sd, dt), '', 0, 3, True, tr)
        runs[dt] = tr
    t64, t32 = runs[torch.float64], runs[torch.float32]
    dmin = NB.min_integer_distance(t64)
    print('smallest distance of a designed sample coordinate from an integer: %.3f' % dmin)
    assert dmin >= 0.1
    for k in t64.pre:
        e = NB.err(t32.y[k], t64.y[k])
        flipped, near = NB.check_mask(t32.pre[k] > 0, t64.pre[k], e, k)
        print('%s: e32(y) %.2e, fp32 torch flips %d units, %d of %d within the threshold' % (k, e, flipped, near, t64.pre[k].numel()))


def test_modules_take_the_node_type_the_reference_model_passes():
    """the reference's ``DLASeg`` builds both with ``node_type = DLA_NODE['dcn']``, a (proj, node) pair of classes, and its
    ``DLAUp`` hands the pair on to every ``IDAUp``: a pair and a single class give the modules of the default"""
    from centertrack_amd import dla_up
    from centertrack_amd._lib import CTError
    D = dla_up.DeformConv

    def keys(m):
        return sorted((k, tuple(v.shape)) for k, v in m.state_dict().items())
    want_ida = keys(dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4]))
    want_dup = keys(dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8]))
    for nt in ((D, D), [D, D], D):
        assert keys(dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4], node_type=nt)) == want_ida
        dup = dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8], node_type=nt)
        assert keys(dup) == want_dup
        assert all(isinstance(getattr(dup.ida_2, n + '_3'), D) for n in ('proj', 'node'))
    for bad in ((D,), (D, D, D), (D, torch.nn.Identity), torch.nn.Identity):
        with pytest.raises(CTError, match='DeformConv only'):
            dla_up.DLAUp(2, [64, 128, 256, 512], [1, 2, 4, 8], node_type=bad)
        with pytest.raises(CTError, match='DeformConv only'):
            dla_up.IDAUp(64, [64, 128, 256], [1, 2, 4], node_type=bad)
