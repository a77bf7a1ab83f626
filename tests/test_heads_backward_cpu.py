"""CPU: the host side of the heads backward (centertrack_amd/csrc/heads_bwd.hip, centertrack_amd/heads.py) -- argument
validation of ct_conv2d_backward_weight / ct_heads_tail_backward and their workspace queries, the restated host plans
against those queries, the names, shapes and initialisation of ``FusedHeads``, and the exactness of the dyadic fixture the
GPU tests compare against bit for bit.  Nothing here launches a kernel."""
import ctypes

import pytest
import torch

import _heads_bwd as HB


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _cw_desc(p, N=2, H=11, W=13, Cin=64, Cout=1024, ks=3):
    from centertrack_amd import _lib
    d = _lib.ConvBwdWeightDesc()
    d.x = d.gy = d.gw = d.gb = p
    d.N, d.H, d.W, d.Cin, d.ldx, d.Cout, d.ldgy, d.ks, d.stride = N, H, W, Cin, Cin, Cout, Cout, ks, 1
    return d


def test_conv_backward_weight_validates_its_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    call, query = lib.ct_conv2d_backward_weight, lib.ct_conv2d_backward_weight_workspace_bytes
    assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    assert query(None) == 0
    good = _cw_desc(p)
    assert query(ctypes.byref(good)) == HB.cw_plan(2, 11, 13, 64, 1024, 3)['bytes'] > 0
    for field, value, word in (('ks', 5, b'ks=5'), ('ks', 2, b'ks=2'), ('stride', 2, b'stride=2'), ('Cin', 24, b'Cin=24'),
                               ('Cin', 0, b'Cin=0'), ('Cout', 0, b'bad shape'), ('N', 0, b'bad shape'), ('H', -1, b'bad shape'),
                               ('ldx', 48, b'pitch'), ('ldgy', 1000, b'pitch'), ('x', None, b'null pointer'),
                               ('gy', None, b'null pointer'), ('gw', None, b'null pointer')):
        d = _cw_desc(p)
        setattr(d, field, value)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, field
        assert word in lib.ct_last_error(), (field, lib.ct_last_error())
        if field not in ('x', 'gy', 'gw'):
            assert query(ctypes.byref(d)) == 0, field              # a rejected descriptor has no workspace size
    # a missing or too small workspace; gb is optional
    d = _cw_desc(p)
    d.gb = None
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    # a view of 2 GiB: one buffer descriptor cannot address it (N*H*W*ld*4 < 2^31)
    d = _cw_desc(p, N=8, H=256, W=256, Cin=64, Cout=1024)          # gy: 524288 pixels * 1024 * 4 = 2^31
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'2 GiB' in lib.ct_last_error()
    assert query(ctypes.byref(d)) == 0
    d = _cw_desc(p, N=8, H=256, W=256, Cin=64, Cout=1023)
    d.ldgy = 1023
    assert query(ctypes.byref(d)) > 0                               # one float per pixel below the limit


def _tail_desc(p, cs=(1, 2, 2, 4), N=2, H=11, W=13, hc=256, flags=3):
    from centertrack_amd import _lib
    arr = (_lib.HeadsTailHead * len(cs))()
    for i, c in enumerate(cs):
        arr[i].gout = arr[i].w2 = arr[i].gw2 = arr[i].gb2 = p
        arr[i].c = c
    d = _lib.HeadsTailBwdDesc()
    d.N, d.H, d.W, d.hc = N, H, W, hc
    d.heads, d.nheads = arr, len(cs)
    d.mid = d.gmid = p
    d.ldmid = d.ldgmid = hc * len(cs)
    d.flags = flags
    return d, arr


def test_heads_tail_backward_validates_its_arguments(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    call, query = lib.ct_heads_tail_backward, lib.ct_heads_tail_backward_workspace_bytes
    assert call(None, None) == _lib.CT_ERR_ARG and b'null descriptor' in lib.ct_last_error()
    assert query(None) == 0
    d, arr = _tail_desc(p)
    assert query(ctypes.byref(d)) == HB.tail_plan(2, 11, 13, 256, (1, 2, 2, 4))['bytes'] > 0
    for field, value, word in (('flags', 0, b'flags=0'), ('flags', 4, b'flags=4'), ('N', 0, b'bad shape'), ('hc', 0, b'bad shape'),
                               ('nheads', 0, b'nheads=0'), ('nheads', 17, b'nheads=17'), ('heads', None, b'nheads'),
                               ('ldmid', 1023, b'ldmid'), ('ldgmid', 1023, b'ldgmid'), ('mid', None, b'(mid)'),
                               ('gmid', None, b'(gmid)')):
        d, arr = _tail_desc(p)
        if field == 'heads':
            d.heads = ctypes.POINTER(_lib.HeadsTailHead)()
        else:
            setattr(d, field, value)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, field
        assert word in lib.ct_last_error(), (field, lib.ct_last_error())
        if field not in ('mid', 'gmid'):
            assert query(ctypes.byref(d)) == 0, field
    for field, word in (('gout', b'(gout)'), ('w2', b'(w2)')):
        d, arr = _tail_desc(p)
        setattr(arr[2], field, None)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and word in lib.ct_last_error() and b'head 2' in lib.ct_last_error()
    d, arr = _tail_desc(p)
    arr[1].c = 0
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'head 1 has c=0' in lib.ct_last_error()
    assert query(ctypes.byref(d)) == 0
    # the hidden gradient alone needs no workspace, no gw2 / gb2 and no ldgmid beyond its own flag
    d, arr = _tail_desc(p, flags=_lib.CT_HEADS_BWD_HIDDEN)
    assert query(ctypes.byref(d)) == 0
    # the weight gradients alone need no w2 and no gmid, but a workspace and at least one buffer
    d, arr = _tail_desc(p, flags=_lib.CT_HEADS_BWD_WEIGHT)
    d.gmid, d.ldgmid = None, 0
    for h in arr:
        h.w2 = None
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE and b'workspace' in lib.ct_last_error()
    d.workspace, d.workspace_bytes = p, query(ctypes.byref(d)) - 4
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_WORKSPACE
    for h in arr:
        h.gw2 = h.gb2 = None
    assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG and b'without a gw2 / gb2 buffer' in lib.ct_last_error()


def test_the_restated_plans_give_the_librarys_workspace_sizes(lib):
    """every shape of the GPU tests, the four benchmark configurations and the generic weight-gradient cases: slab count x
    slab size of the Python restatement == the query; and the shape list reaches the regimes its comment names"""
    from centertrack_amd import _lib
    keep, p = _ptr()
    cases = list(HB.SHAPES) + [((1, 128, 128), HB.MOT), ((4, 128, 128), HB.MOT), ((4, 112, 200), HB.NUSC),
                               ((4, 128, 128), HB.OrderedDict([('hm', 80), ('reg', 2), ('wh', 2)]))]
    for (N, H, W), heads in cases:
        cs = tuple(heads.values())
        d = _cw_desc(p, N, H, W, HB.CIN, HB.HC * len(cs), 3)
        assert lib.ct_conv2d_backward_weight_workspace_bytes(ctypes.byref(d)) == HB.cw_plan(N, H, W, HB.CIN, HB.HC * len(cs), 3)['bytes']
        t, arr = _tail_desc(p, cs, N, H, W)
        assert lib.ct_heads_tail_backward_workspace_bytes(ctypes.byref(t)) == HB.tail_plan(N, H, W, HB.HC, cs)['bytes']
    for ks in (1, 3):
        for cin in (16, 64, 256):
            for cout in (8, 72, 256):
                d = _cw_desc(p, 2, 9, 11, cin, cout, ks)
                assert lib.ct_conv2d_backward_weight_workspace_bytes(ctypes.byref(d)) == HB.cw_plan(2, 9, 11, cin, cout, ks)['bytes']
    cw = {HB.case_id(c): HB.cw_plan(*c[0], HB.CIN, HB.HC * len(c[1]), 3) for c in HB.SHAPES}
    tail = {HB.case_id(c): HB.tail_plan(*c[0], HB.HC, tuple(c[1].values())) for c in HB.SHAPES}
    ids = [HB.case_id(c) for c in HB.SHAPES]
    a, b, c, e, f, g = ids
    assert (cw[a]['units'], cw[a]['slabs'], cw[a]['capped'], cw[a]['stepsPerWave']) == (288, 3, True, 6)
    assert (tail[a]['slabs'], tail[a]['last_slab_pixels']) == (5, 30) and (2 * 11 * 13) % 4 == 2
    assert (cw[b]['units'], cw[b]['slabs'], cw[b]['capped']) == (72, 2, True) and tail[b]['slabs'] == 3
    assert (cw[c]['units'], cw[c]['slabs'], cw[c]['capped']) == (216, 1, True) and tail[c]['passes'] == [5, 3, 2]
    assert (cw[e]['units'], cw[e]['slabs'], cw[e]['capped'], cw[e]['stepsPerWave'], cw[e]['last_wave_steps']) == (720, 2, False, 40, 40)
    assert tail[e]['slabs'] == 20 and len(HB.NUSC) == 10 > _lib.CT_MAX_FUSED_HEADS
    assert (cw[f]['slabs'], cw[f]['capped'], cw[f]['stepsPerWave'], cw[f]['last_wave_steps']) == (2, False, 39, 37)
    assert (cw[g]['units'], cw[g]['slabs'], cw[g]['capped'], cw[g]['stepsPerWave'], cw[g]['last_wave_steps']) == (144, 8, False, 8, 8)
    assert tail[g]['slabs'] == 16


def test_the_gpu_cases_reach_every_regime_of_the_tail_plan(lib):
    """``_heads_bwd.TAIL_REGIMES`` against every case the GPU tests run through ct_heads_tail_backward; the new case is there for
    regimes nothing else reaches; what production reaches -- the MOT and nuScenes heads at batch 1 and 4 on 512 x 512 and
    800 x 448 -- a GPU case reaches; and the library's workspace query equals the restated plan at the new case"""
    keep, p = _ptr()
    assert HB.missing_tail_regimes(HB.tail_cases()) == []
    assert set(HB.missing_tail_regimes(HB.SHAPES)) == {
        'slabs from the grid target', 'pixPerSlab >= 128', 'a last slab of more than one tile whose last tile is ragged'}
    prod = [((n, h, w), hd) for n in (1, 4) for h, w in ((128, 128), (112, 200)) for hd in (HB.MOT, HB.NUSC)]
    assert set(HB.reached_tail_regimes(prod)) <= set(HB.reached_tail_regimes(HB.tail_cases()))
    assert 'pixPerSlab >= 128' in HB.reached_tail_regimes(prod)                       # production is past one tile per slab
    assert HB.tail_plan(4, 128, 128, HB.HC, tuple(HB.MOT.values()))['pixPerSlab'] == 128
    for (N, H, W), heads in prod + [HB.TAIL_CASE]:
        cs = tuple(heads.values())
        t, arr = _tail_desc(p, cs, N, H, W)
        assert lib.ct_heads_tail_backward_workspace_bytes(ctypes.byref(t)) == HB.tail_plan(N, H, W, HB.HC, cs)['bytes'] > 0
    (N, H, W), heads = HB.TAIL_CASE
    plan = HB.tail_plan(N, H, W, HB.HC, tuple(heads.values()))
    assert (plan['wanted'], plan['maxSlabs'], plan['pixPerSlab'], plan['slabs'], plan['last_slab_pixels']) == (64, 66, 128, 33, 86)
    assert len(heads) == 16 and H * W == 2091 and plan['passes'] == [2] * 16


def test_the_tail_truth_is_autograd():
    """``_heads_bwd.tail_truth`` (explicit sums over a hidden map that is given) against torch autograd of relu -> conv1x1 per
    head behind a 3x3 convolution, float64, on a small map"""
    case = ((2, 5, 7), HB.OrderedDict([('a', 20), ('b', 3)]))
    fx = HB.tail_fixture(case)
    want = HB.tail_truth(fx, torch.float64)
    nh = len(case[1])
    # a pre-activation whose ReLU is ``mid``: mid where it is positive, -1 elsewhere
    pre = torch.where(fx['mid'] > 0, fx['mid'], -torch.ones_like(fx['mid'])).double().requires_grad_()
    w2 = [fx['w2'][h].double().requires_grad_() for h in case[1]]
    b2 = [torch.zeros(c, dtype=torch.float64, requires_grad=True) for c in case[1].values()]
    mid = torch.relu(pre)
    tot = sum((HB.F.conv2d(mid[:, HB.HC * j:HB.HC * (j + 1)], w2[j], b2[j]) * fx['gout'][h].double()).sum() for j, h in enumerate(case[1]))
    g = torch.autograd.grad(tot, [pre] + w2 + b2)
    assert HB.err(want['gmid'], g[0]) < 1e-14
    for j, h in enumerate(case[1]):
        assert HB.err(want['w2'][h], g[1 + j]) < 1e-14 and HB.err(want['b2'][h], g[1 + nh + j]) < 1e-14
    x = torch.zeros(2, HB.CIN, 5, 7, dtype=torch.float64, requires_grad=True)
    gx, = torch.autograd.grad(HB.F.conv2d(x, fx['w0'].double(), padding=1), x, want['gmid'])
    assert HB.err(want['x'], gx) < 1e-14


def test_fused_heads_names_shapes_and_initialisation():
    from centertrack_amd import heads as HD, weights
    from centertrack_amd._lib import CTError
    for hs in (weights.MOT_HEADS, HB.NUSC, HB.POSE):
        torch.manual_seed(3)
        m = HD.FusedHeads(hs, head_conv={h: [256] for h in hs}, prior_bias=-2.19)
        want = [(k, shape) for k, shape, kind in weights.dla34_param_shapes(hs, 256) if k.split('.')[0] in hs]
        got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert got == want and len(got) == 4 * len(hs)
        assert [n for n, _ in m.named_parameters()] == [k for k, _ in want]
        for h in hs:
            w0, b0, w2, b2 = m.head_parameters(h)
            assert float(w0.detach().abs().max()) > 0 and float(w2.detach().abs().max()) > 0           # torch's Conv2d default
            if 'hm' in h:
                assert torch.all(b2 == -2.19)
            else:
                assert torch.all(b0 == 0) and torch.all(b2 == 0)
        # a checkpoint of the whole network loads with strict=False: the trunk keys are unexpected, nothing is missing
        sd = weights.make_synthetic_state_dict(hs) if hs is weights.MOT_HEADS else None
        if sd is not None:
            res = m.load_state_dict(sd, strict=False)
            assert not res.missing_keys and all(k.split('.')[0] not in hs for k in res.unexpected_keys)
            assert torch.equal(m.hm[2].weight, sd['hm.2.weight'])
    assert HD.FusedHeads({'hm': 1, 'hm_hp': 17}).hm_hp[2].bias.eq(-4.6).all()
    with pytest.raises(CTError):
        HD.FusedHeads({'hm': 1}, head_conv={'hm': [256, 256]})                      # two hidden layers
    with pytest.raises(CTError):
        HD.FusedHeads({'hm': 1, 'reg': 2}, head_conv={'hm': [256], 'reg': [128]})   # two widths
    with pytest.raises(CTError):
        HD.FusedHeads({'hm': 1}, head_conv={'hm': []})                              # no hidden layer


def test_a_cpu_tensor_raises():
    from centertrack_amd import heads as HD, ops
    from centertrack_amd._lib import CTError
    m = HD.FusedHeads({'hm': 1, 'reg': 2})
    with pytest.raises(CTError, match='no CPU fallback'):
        m(torch.zeros(1, 64, 8, 8))
    with pytest.raises(CTError, match='no CPU fallback'):
        m(ops.View(torch.zeros(1, 8, 8, 64)))
    with pytest.raises(CTError):
        m(torch.zeros(1, 64, 8, 8, dtype=torch.float64))


def test_the_dyadic_fixture_is_exact_in_fp32():
    """fp32 torch hidden == float64 hidden bit for bit at the issue's shape, with exact zeros and both signs"""
    case = ((2, 11, 13), HB.OrderedDict([('hm', 1), ('reg', 2), ('wh', 2)]))           # 768 hidden channels
    fx = HB.fixture(case)
    pre64 = torch.cat([HB.F.conv2d(fx['x'].double(), fx['w0'][h].double(), fx['b0'][h].double(), padding=1) for h in fx['heads']], 1)
    pre32 = torch.cat([HB.F.conv2d(fx['x'], fx['w0'][h], fx['b0'][h], padding=1) for h in fx['heads']], 1)
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)
    zeros, pos = float((pre64 == 0).double().mean()), float((pre64 > 0).double().mean())
    print('dyadic fixture: %.3f %% exact zeros, %.1f %% positive' % (100 * zeros, 100 * pos))
    assert 0 < zeros < 0.01 and 0.4 < pos < 0.6
    # every value is a multiple of 2^-9 far below 2^24 units
    assert torch.equal((pre64 * 512).round(), pre64 * 512) and float(pre64.abs().max()) * 512 < 2 ** 20
    # the shared truth of the GPU tests: same property on every shape
    for c in HB.SHAPES[:2]:
        _, t64, t32 = HB.truth(c)
        assert torch.equal(t32['mid'].double(), t64['mid'])
