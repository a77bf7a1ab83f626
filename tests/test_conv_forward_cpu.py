"""CPU: the host side of the forward convolutions (centertrack_amd/csrc/conv_mfma.hip, wino_mfma.hip) and of the element-wise
ops -- the regime table of tests/_conv_fwd.py against the list of cases the GPU tests run, the launches of the pinned tune table
and of the autotuner's candidates against that list, the restated plan against ``ct_conv2d_workspace_bytes``, the float32
references against the float64 one, and the 2 GiB-per-image check of ``ct_conv2d``.  Nothing here launches a kernel on a GPU: the
one call that passes validation runs in a child process that sees no device."""
import ctypes
import json
import os
import subprocess
import sys
import types

import pytest

import _conv_fwd as C

ROOT = C.ROOT


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # a 16-byte aligned address inside the buffer


def _desc(p, N, H, W, Cin, Cout, ks, stride, algo=0, split_k=0, proj=False, **kw):
    from centertrack_amd import _lib
    d = _lib.ConvDesc()
    d.x = d.w_packed = d.y = d.w_winograd = p
    d.N, d.H, d.W, d.Cin, d.ldx, d.Cout, d.ks, d.stride = N, H, W, Cin, Cin, Cout, ks, stride
    d.ldy = d.ldr = d.proj_ldy = Cout
    d.pool_ld = Cin
    d.algo, d.split_k, d.depth_scale = algo, split_k, 1.0
    if proj:
        d.proj_w_packed = d.proj_y = p
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the table and the lists

def test_every_regime_is_reached_by_a_gpu_case():
    assert C.missing_conv_regimes(C.GPU_CASES) == []
    assert C.missing_pool_regimes(C.POOL_SHAPES) == []
    assert C.missing_upsample_regimes(C.UP_SHAPES) == []
    assert C.missing_layout_regimes(C.LAYOUT_SHAPES) == []
    assert len(C.CONV_REGIMES) >= 300 and all(isinstance(v, str) and ('.hip' in v or '.h' in v) for v in C.CONV_REGIMES.values())
    for case in C.GPU_CASES:
        assert case.why and case.N * case.H * case.W * case.Cin <= 2 * 20 * 42 * 192, case.name


def test_no_case_is_redundant():
    """deleting any single entry leaves a regime unreached"""
    for i, case in enumerate(C.GPU_CASES):
        assert C.missing_conv_regimes(C.GPU_CASES[:i] + C.GPU_CASES[i + 1:]), case.name
    for shapes, missing in ((C.POOL_SHAPES, C.missing_pool_regimes), (C.UP_SHAPES, C.missing_upsample_regimes),
                            (C.LAYOUT_SHAPES, C.missing_layout_regimes)):
        for i, s in enumerate(shapes):
            assert missing(shapes[:i] + shapes[i + 1:]), s


def test_row_cases_follow_the_one_rule():
    """N = 2, Ho = TH + 3, Wo = 21, Cin = 48 NKK, Cout = BN + 27 for every row-tiled instantiation; a plain stride-2 case has odd
    H and W, one with side outputs H = 2 Ho and W = 2 Wo"""
    n = 0
    for case in C.GPU_CASES:
        if not case.name.startswith('row'):
            continue
        p = C.plan_of(case)
        n += 1
        assert p['family'] == 'row' and C.standard(case, p), case.name
        assert (case.N, p['Ho'], p['Wo'], case.Cin, case.Cout) == (2, p['TH'] + 3, 21, 48 * p['NKK'], p['BN'] + 27), case.name
        if case.stride == 2:
            assert (case.H, case.W) == ((2 * p['Ho'], 42) if (case.pool or case.proj) else (2 * p['Ho'] - 1, 41)), case.name
    assert n == 46 + 24                   # 8 shapes x (1x1 NKK 1 / 2 / 4, 3x3 NKK 1 / 2, stride 2) less NKK 4 on cfg 0 / 1, and 8 x 3 POOL


def test_production_launches_reach_only_tested_regimes():
    reached = set(C.reached_conv_regimes(C.GPU_CASES))
    launches = C.production_conv_launches()
    assert len(launches) > 500
    algos = set()
    for key, shape, proj, algo, sk in launches:
        keys = C.launch_keys(shape, proj, algo, sk)
        assert keys and keys <= reached, (key, sorted(keys - reached, key=str))
        algos.add(algo)
    assert {2, 3, 5, 6, 7, 8, 101, 102, 103, 104, 105, 201, 202, 205, 206, 207, 209, 211} <= algos


def test_autotune_candidates_reach_only_tested_regimes():
    """every (algo, split_k) the autotuner would time for the conv shapes of DLA-34 at 512x512, one stream (the table's keys)"""
    from centertrack_amd import _lib, autotune
    reached = set(C.reached_conv_regimes(C.GPU_CASES))
    seen, n = set(), 0
    for key, shape, proj, _, _ in C.production_conv_launches():
        N, H, W, Cin, Cout, ks, stride = shape
        if N != 1 or H != W or H not in (512, 256, 128, 64, 32, 16):
            continue
        nchw = int(key.split(',')[-1])
        d = types.SimpleNamespace(Cout=Cout, Cin=Cin, ks=ks, stride=stride, w_winograd=1 if key.startswith('convW') else None,
                                  flags=_lib.CT_OUT_NCHW if nchw else 0)
        for algo, sk in autotune._conv_candidates(d):
            keys = C.launch_keys(shape, proj, algo, sk)
            assert keys <= reached, (key, algo, sk, sorted(keys - reached, key=str))
            seen.add(algo)
            n += 1
    assert n > 200 and set(range(0, 9)) - {4} <= seen and set(range(101, 106)) <= seen and set(range(201, 212)) <= seen


# ---------------------------------------------------------------------------------------------------------------------
# the restated plan against the library

def _query(lib, p, shape, algo, sk, proj=False):
    return lib.ct_conv2d_workspace_bytes(ctypes.byref(_desc(p, *shape, algo=algo, split_k=sk, proj=proj)))


def test_the_restated_plan_gives_the_librarys_workspace_size(lib):
    keep, p = _ptr()
    for case in C.GPU_CASES:
        shape = (case.N, case.H, case.W, case.Cin, case.Cout, case.ks, case.stride)
        assert _query(lib, p, shape, case.algo, case.split_k, case.proj) == C.plan_of(case)['bytes'], case.name
    split = 0
    for key, shape, proj, algo, sk in C.production_conv_launches():
        want = C.conv_plan(*shape, algo=algo, split_k=sk, has_proj=proj)['bytes']
        assert _query(lib, p, shape, algo, sk, proj) == want, key
        assert _query(lib, p, shape, 0, 0, proj) == C.conv_plan(*shape, has_proj=proj)['bytes'], key
        split += want > 0
    assert split > 20


KNOB_SETTINGS = ([('conv_small_tiles', v) for v in (0, 64, 100000)] + [('splitk_target', v) for v in (64, 2048, 100000)]
                 + [('conv_ks', v) for v in (-2, -1, 0, 1, 2, 3, 4)] + [('conv_ks_below', v) for v in (0, 100000)]
                 + [('conv_ks_waves', v) for v in (1, 64, 100000)])


def test_the_restated_plan_follows_the_tuning_knobs(lib):
    keep, p = _ptr()
    shapes = sorted(set(s for _, s, _, _, _ in C.production_conv_launches()))[::9]
    shapes += [(c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride) for c in C.GPU_CASES[::7]]
    assert len(shapes) > 60
    changed = 0
    try:
        for knob, value in KNOB_SETTINGS:
            assert lib.ct_set_tuning(knob.encode(), value) == 0
            for shape in shapes:
                for sk in (0, 3):
                    want = C.conv_plan(*shape, algo=0, split_k=sk, knobs=((knob, value),))['bytes']
                    assert _query(lib, p, shape, 0, sk) == want, (knob, value, shape, sk)
                    changed += want != C.conv_plan(*shape, algo=0, split_k=sk)['bytes']
            assert lib.ct_set_tuning(knob.encode(), C.KNOBS[knob]) == 0
    finally:
        for knob, value in C.KNOBS.items():
            lib.ct_set_tuning(knob.encode(), value)
    assert changed > 50                    # the knobs move the plan: the comparison above is not one of zeros


# ---------------------------------------------------------------------------------------------------------------------
# the references

def test_the_float32_references_pass_their_own_bound():
    for case in C.GPU_CASES:
        r64 = C.reference64(case)
        for ref in (C.reference32(case), C.yardstick32(case)):
            for which in r64:
                if which == 'pool':
                    assert ref[which].equal(r64[which])
                    continue
                e, e32, b = C.case_errors(case, ref[which], which)
                assert e <= b and e32 < 2.5e-4, (case.name, which, e, b)      # (below the bound's cap of 1e-3 / 4)
        keep = ~C.plain_channels(case)
        if keep.any():                                                   # the sigmoid and depth channels, element-wise
            b = C.case_errors(case, r64['y'])[2]
            a, r = C.reference32(case)['y'][:, keep].double(), r64['y'][:, keep]
            assert bool(((a - r).abs() <= b * (r.abs() + 1)).all()), case.name


def test_the_bound_notices_one_wrong_element():
    """an element off by 1e-4 of the map's maximum -- a wrong edge pixel that is small in absolute terms -- misses every case's bound"""
    for case in C.GPU_CASES[::5]:
        y = C.reference32(case)['y'].clone()
        c = int(C.plain_channels(case).nonzero()[-1])
        y[-1, c, -1, -1] += 1e-4 * float(C.reference64(case)['y'][:, C.plain_channels(case)].abs().max())
        e, e32, b = C.case_errors(case, y)
        assert e > b and b < 5e-5, (case.name, e, b)


def test_winograd32_is_the_convolution():
    import torch
    import torch.nn.functional as F
    for N, Cin, Cout, H, W in ((2, 5, 7, 1, 1), (1, 3, 4, 7, 10), (2, 8, 3, 6, 1)):
        x, w = C.randn(1, N, Cin, H, W), C.randn(2, Cout, Cin, 3, 3)
        got = C.winograd32(x.float(), w.float())
        assert got.dtype == torch.float32 and C.err(got, F.conv2d(x, w, None, 1, 1)) < 5e-6


# ---------------------------------------------------------------------------------------------------------------------
# the 2 GiB check of ct_conv2d

def _over(px, Cc):
    """the smallest pitch (a multiple of 4) at which a view of ``px`` pixels and ``Cc`` channels reaches 2 GiB per image"""
    ld = Cc
    while ((px - 1) * ld + Cc) * 4 < 2 ** 31:
        ld += 4
    assert ((px - 1) * (ld - 4) + Cc) * 4 < 2 ** 31 or ld == Cc
    return ld


HOST_ALGOS = [('row', 1, 16, 1, 1), ('ksplit', 102, 64, 3, 1), ('wino', 202, 64, 3, 1)]          # (family, algo, Cin, ks, stride)
BELOW = {1: dict(N=1, H=4096, W=4096, Cin=16, Cout=16, ks=1, stride=1, ldx=32, ldy=32),       # ((2^24 - 1) * 32 + 16) * 4 = 2^31 - 64
         102: dict(N=1, H=2048, W=2048, Cin=64, Cout=64, ks=3, stride=1, ldx=128, ldy=128),  # ((2^22 - 1) * 128 + 64) * 4 = 2^31 - 256
         202: dict(N=1, H=2048, W=2048, Cin=64, Cout=64, ks=3, stride=1, ldx=128, ldy=128)}


@pytest.mark.parametrize('family,algo,Cin,ks,stride', HOST_ALGOS)
def test_conv2d_refuses_views_of_2_gib_per_image(lib, family, algo, Cin, ks, stride):
    from centertrack_amd import _lib
    keep, p = _ptr()
    S, px, Cout = 2048, 2048 * 2048, 32
    call = lib.ct_conv2d

    def refused(word, name, **kw):
        d = _desc(p, 1, kw.pop('H', S), kw.pop('W', S), kw.pop('Cin', Cin), Cout, kw.pop('ks', ks), kw.pop('stride', stride), algo=algo, split_k=1, **kw)
        assert call(ctypes.byref(d), None) == _lib.CT_ERR_ARG, (name, kw)
        msg = lib.ct_last_error()
        assert word in msg and (b'%s' % name.encode()) in msg, (name, msg)
    refused(b'2 GiB', 'x', ldx=_over(px, Cin))
    refused(b'2 GiB', 'y', ldy=_over(px, Cout))
    refused(b'2 GiB', 'res', res=p, ldr=_over(px, Cout))
    refused(b'pitch', 'of y', ldy=Cout - 4)
    refused(b'pitch', 'of res', res=p, ldr=Cout - 4)
    refused(b'pitch', 'of x', ldx=Cin - 4)
    if family == 'row':                                                  # the issue's example: 4096 x 4096 at pitch 32
        refused(b'2 GiB', 'x', H=4096, W=4096, ldx=32, Cin=32)
    if family != 'wino':                                                 # the side outputs of the 3x3 stride-2 shapes: 1024 x 1024 pixels
        refused(b'2 GiB', 'pool_y', ks=3, stride=2, pool_y=p, pool_ld=_over(px // 4, Cin))
        refused(b'2 GiB', 'proj_y', ks=3, stride=2, proj_w_packed=p, proj_y=p, proj_ldy=_over(px // 4, Cout))
    # just below the limit the views pass: the call then reaches the launch, which this test must not let happen on a GPU -- a
    # child process that sees no device makes it, and gets the launch error of a machine without one
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.dirname(__file__)] + sys.path))
    code = ('import ctypes, json, torch\n'
            'import test_conv_forward_cpu as T\n'
            'from centertrack_amd import _lib\n'
            'if torch.cuda.device_count() > 0:\n'
            '    print(json.dumps("a device is visible: not launching")); raise SystemExit(0)\n'
            'lib = _lib.load(); keep, p = T._ptr()\n'
            'rc = lib.ct_conv2d(ctypes.byref(T._desc(p, algo=%d, split_k=1, **T.BELOW[%d])), None)\n'
            'print(json.dumps([rc, lib.ct_last_error().decode()]))\n' % (algo, algo))
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert isinstance(out, list), out
    assert out[0] in (_lib.CT_OK, _lib.CT_ERR_LAUNCH), out
