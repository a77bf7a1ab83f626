"""CPU: the host side of the DCNv2 forward (centertrack_amd/csrc/dcn_mfma.hip) -- the regime table of tests/_dcn_fwd.py against
the cases the GPU tests run, the restated plan against ``ct_dcn_v2_workspace_bytes`` / ``ct_dcn_v2_group_workspace_bytes`` /
``ct_dcn_v2_group_plan`` / ``ct_dcn_v2_offsets_bytes`` over a generated sweep, the launches of the autotuner's candidates and of the
heuristic path at the seven neck shapes against the table, the float32 references against the float64 one, three mutations of the
float64 reference against every case's bound, every argument error of ``make_plan`` and ``launch_group``, and what the kernels can
address, pinned from both sides.  Nothing here launches a kernel on a GPU: the calls that pass validation run in a child process
that sees no device.

BM, NKK, the XCD fields and the persistent partition are not observable through the ABI (see tests/_dcn_fwd.py); the XCD decode
is checked here for being a bijection onto (split, cout block, pixel tile), which is what the kernel needs of it.

What the kernels can address (dcn_mfma.hip, by reading):
  * x, per image: one buffer descriptor of ((H*W - 1) ldx + Cin) * 4 bytes as ``unsigned`` -- wraps at 4 GiB; the offset/mask conv
    stages (ksplit_core.h, wino_mfma.hip) address an image with 31-bit offsets.  Refused from 2 GiB per image.
  * H*W and the pitches: ``dcn_tab_entry`` forms (y0 W + x0) * (ldx * 4) and the direct store (oy W + px) * ldy with ``__mul24``,
    exact while the pixel index stays below 2^23 and ldx * 4 / ldy below 2^23.  Refused: H*W > 2^23, ldx >= 2^21, ldy >= 2^23.
  * y, per image, direct store: a descriptor of ((H*W - 1) ldy + Cout) * 4 bytes whose dropped lanes get the byte offset 0x80000000,
    valid again once the view passes 2 GiB.  Refused from 2 GiB per image; the finishing launch of a split layer addresses y with
    64-bit offsets and has no such limit.
  * one split's partial map: a descriptor of Mtot * wsCout * 4 bytes with the same dropped offset.  The host used to refuse from
    2^30 floats (4 GiB); between 2 and 4 GiB a dropped lane stored inside the map.  Refused from 2^29 floats.
  * the IDAUp view: 32-bit pixel indices in dcn_reduce_kernel; refused from 2^32 elements (unchanged, now with a message of its own).
  * the packed weight: a descriptor sized 9 * Cin / 16 * NT KiB as an int with int byte offsets, in both kernels.  Refused from 2 GiB.
  * the persistent form: x of the whole batch below 4 GiB (unchanged); the offset/mask map of the whole batch lies behind one
    descriptor with dropped offsets: refused from 2 GiB.  (Partial maps hold 32 floats per pixel and 64 input channels, at most half
    of x: below 2 GiB whenever x is below 4.)
  * N * tiles * splits is an int in the kernels: a grid of 2^30 workgroups or more is refused."""
import ctypes
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import _dcn_fwd as D
from _dcn_bwd import neck_shapes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HUGE = 1 << 62


@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # a 16-byte aligned address inside the buffer


def _desc(p, N, H, W, Cin, Cout, algo=0, split_k=0, fuse_offset=0, up_f=0, **kw):
    from centertrack_amd import _lib
    d = _lib.DcnDesc()
    d.x = d.w_packed = d.y = d.om = d.workspace = p
    d.N, d.H, d.W, d.Cin, d.ldx, d.ldom, d.Cout, d.ldy = N, H, W, Cin, Cin, 32, Cout, Cout
    d.algo, d.split_k, d.fuse_offset, d.workspace_bytes = algo, split_k, fuse_offset, HUGE
    if fuse_offset:
        d.w_off_packed = d.b_off = p
        if fuse_offset >= 2:
            d.om_partial, d.om_partial_bytes = p, HUGE
    if up_f:
        d.up_w = d.up_skip = d.up_y = p
        d.up_f, d.up_lds, d.up_ldy = up_f, Cout, Cout
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the table and the lists

def test_every_regime_is_reached_by_a_gpu_case():
    assert D.missing_regimes(D.GPU_CASES, D.GROUPS) == []
    assert len(D.DCN_REGIMES) >= 90 and all(isinstance(v, str) and ('.hip' in v or '.py' in v) for v in D.DCN_REGIMES.values())
    got = D.all_keys(D.GPU_CASES, D.GROUPS)
    assert got <= set(D.DCN_REGIMES), sorted(got - set(D.DCN_REGIMES), key=str)
    for case in D.GPU_CASES + [c for g in D.GROUPS for c in g.layers]:
        assert case.why or case.entry == 'group'
        assert case.N <= 4 and case.H * case.W <= 24 * 24 and (case.Cin < 512 or case.H * case.W <= 42), case.name
    for g in D.GROUPS:
        assert g.why and 1 <= len(g.layers) <= 4


def test_no_case_is_redundant():
    """deleting any single case or group leaves a regime unreached"""
    for i, case in enumerate(D.GPU_CASES):
        assert D.missing_regimes(D.GPU_CASES[:i] + D.GPU_CASES[i + 1:], D.GROUPS), case.name
    for i, g in enumerate(D.GROUPS):
        assert D.missing_regimes(D.GPU_CASES, D.GROUPS[:i] + D.GROUPS[i + 1:]), g.name


def test_kernel_cases_follow_the_one_rule():
    n = 0
    for case in D.GPU_CASES:
        if case.name[:2] in ('k_', 'p_') and not case.name.startswith('p_om'):
            p = D.plan_of(case)
            n += 1
            assert D.standard(case, p) and (case.N, case.H, case.W, case.Cin, case.Cout) == (2, 2 * p['rows'] + 1, 21, 128, p['BN'] + 27), case.name
    assert n == len(D.TILE_KERNELS) + len(D.PERSIST_KERNELS) == 14


def test_half_of_the_map_cases_sample_the_designed_positions():
    maps = [c for c in D.GPU_CASES if c.src in ('map', 'slice')]
    n = sum(D.designed(c) for c in maps)
    assert len(maps) >= 20 and 0.3 * len(maps) <= n <= 0.7 * len(maps), (n, len(maps))
    for c in maps:
        if D.designed(c):
            off = D.dcn_inputs(c)['off']
            assert bool((off * 4 == (off * 4).round()).all())            # multiples of 0.25: the fp32 coordinate is exact


def test_the_xcd_order_is_a_bijection():
    """every (split, cout block, pixel tile) is computed by exactly one live workgroup, and XCD id % 8 contracts split % xsx only"""
    n = 0
    for case in D.GPU_CASES + [c for g in D.GROUPS for c in g.layers]:
        p = D.plan_of(case, (('dcn_xcd', 1),))
        if p['family'] != 'tile':
            continue
        seen = [D.xcd_decode(p, b) for b in range(p['grid'])]
        live = [s for s in seen if s is not None]
        assert sorted(live) == [(s, cb, t) for s in range(p['splits']) for cb in range(p['coutBlocks']) for t in range(p['ptiles'])], case.name
        assert p['padded'] == (len(live) < p['grid']) and p['grid'] % 8 == 0
        assert all(s[0] % p['xsx'] == (b & 7) % p['xsx'] for b, s in enumerate(seen) if s is not None)
        n += 1
    assert n > 40


# ---------------------------------------------------------------------------------------------------------------------
# the restated plan against the library

def _sweep():
    i = 0
    for N, H, W in ((1, 4, 4), (1, 16, 16), (2, 7, 19), (1, 32, 32), (3, 24, 24), (1, 64, 64), (4, 16, 32), (8, 64, 64)):
        for Cin in (32, 64, 96, 128, 160, 192, 256, 512):
            for Cout in (16, 40, 64, 91, 128, 160, 256, 320):
                for algo in D.ALGOS:
                    for sk in (0, 1, 2, 3, 4, 5, 8, 16):
                        for fo in (0, 1, 2, 3):
                            for grouped in (False, True):
                                i += 1
                                if i % 5 == 0:
                                    yield N, H, W, Cin, Cout, algo, sk, fo, grouped, (2 if (i % 3 == 0 and Cout % 4 == 0) else 0)


def test_the_restated_plan_gives_the_librarys_workspace_size_and_splits(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    n = ok = 0
    try:
        for bn in (0, 64, 128):
            assert lib.ct_set_tuning(b'dcn_bn', bn) == 0
            for N, H, W, Cin, Cout, algo, sk, fo, grouped, up_f in _sweep():
                if bn and n % 3:
                    n += 1
                    continue
                n += 1
                d = _desc(p, N, H, W, Cin, Cout, algo, sk, fo, up_f)
                try:
                    want = D.dcn_plan(N, H, W, Cin, Cout, algo, sk, fo, grouped, True, up_f > 0, (('dcn_bn', bn),))
                except ValueError:
                    want = None
                what = (bn, N, H, W, Cin, Cout, algo, sk, fo, grouped, up_f)
                assert lib.ct_dcn_v2_offsets_bytes(ctypes.byref(d)) == D.offsets_bytes(N, H, W, Cin, fo), what
                if grouped:
                    need, splits = ctypes.c_size_t(0), ctypes.c_int(0)
                    rc = lib.ct_dcn_v2_group_plan(ctypes.byref(d), ctypes.byref(need), ctypes.byref(splits))
                    if want is None:
                        assert rc == _lib.CT_ERR_ARG and lib.ct_dcn_v2_group_workspace_bytes(ctypes.byref(d)) == 0, what
                    else:
                        assert (rc, need.value, splits.value) == (0, want['bytes'], want['splits']), (what, rc, need.value, splits.value, want)
                        assert lib.ct_dcn_v2_group_workspace_bytes(ctypes.byref(d)) == want['bytes'], what
                else:
                    got = lib.ct_dcn_v2_workspace_bytes(ctypes.byref(d))
                    assert got == (want['bytes'] if want else 0), (what, got, want)
                ok += want is not None and want['bytes'] > 0
    finally:
        lib.ct_set_tuning(b'dcn_bn', D.KNOBS['dcn_bn'])
    assert n > 100000 and ok > 20000


def test_the_cases_plans_are_the_librarys(lib):
    keep, p = _ptr()
    for case in D.GPU_CASES + [c for g in D.GROUPS for c in g.layers]:
        try:
            for k, v in case.knobs:
                assert lib.ct_set_tuning(k.encode(), v) == 0
            d = _desc(p, case.N, case.H, case.W, case.Cin, case.Cout, case.algo, case.split_k, D.FUSE_OFFSET[case.src], case.up_f)
            query = lib.ct_dcn_v2_group_workspace_bytes if case.entry == 'group' else lib.ct_dcn_v2_workspace_bytes
            assert query(ctypes.byref(d)) == D.plan_of(case)['bytes'], case.name
            splits = ctypes.c_int(0)
            if case.entry == 'group':
                assert lib.ct_dcn_v2_group_plan(ctypes.byref(d), None, ctypes.byref(splits)) == 0 and splits.value == D.plan_of(case)['splits']
        finally:
            for k, _ in case.knobs:
                lib.ct_set_tuning(k.encode(), D.KNOBS[k])


def test_the_persistable_cases_are_those_the_library_accepts(lib):
    """``persistent_form`` picks every 32-pixel-tile case whose plan make_plan accepts under the persistent algo of its tile shape"""
    keep, p = _ptr()
    n = 0
    for case in D.GPU_CASES:
        q = D.plan_of(case)
        if q['family'] != 'tile' or q['BM'] != 32 or case.knobs:
            continue
        d = _desc(p, case.N, case.H, case.W, case.Cin, case.Cout, D._PERSIST_ALGO[(q['BN'], q['NKK'])], q['splits'], D.FUSE_OFFSET[case.src], case.up_f)
        rc = lib.ct_dcn_v2_group_plan(ctypes.byref(d), None, None)
        assert (rc == 0) == (D.persistent_form(case) is not None), (case.name, rc, lib.ct_last_error())
        n += 1
    assert n > 25
    assert {'nkk4_two_units', 'xcd_off', 'om_parts1', 'om_wino', 'om_slice', 'ldom31_h1', 'legacy_up', 'om_parts8'} <= set(D.PERSISTABLE)
    assert all(D.plan_of(c)['family'] == 'persist' for c in D.PERSISTABLE.values()) and len(D.PERSISTABLE) >= 20


def _plan_keys(p, up_f):
    """the regimes a launch with plan ``p`` reaches whatever its tensors hold"""
    keys = {('split-origin', p['origin'])}
    keys.add(('persist', p['WN'], p['NKK']) if p['family'] == 'persist' else ('kernel', p['BM'], p['WN'], p['fuse'], p['NKK']))
    if p['family'] == 'tile':
        keys |= {('steps', 'odd: the peeled last step' if s % 2 else 'even') for s in p['steps']}
        keys |= {('rot', r) for r in D.rots(p)}
        keys.add(('xcd', p['xsx'], 'padded ids' if p['padded'] else 'no padding'))
    if p['use_ws']:
        keys.add(('reduce', up_f))
    elif up_f:
        keys.add(('legacy_up',))
    return keys


def test_autotune_candidates_and_the_heuristic_path_reach_only_tested_regimes():
    """``autotune._dcn_candidates`` (no caller in the tree; the set ``ops.dcn_v2(algo=, split_k=)`` exposes) and algo 0 / split_k 0
    with a workspace -- what the drop-in module and the training forward launch -- at the seven neck shapes, 512 x 512, batch 1 and 4"""
    from centertrack_amd import autotune
    reached = D.all_keys(D.GPU_CASES, D.GROUPS)
    seen, n = set(), 0
    for N in (1, 4):
        for Cin, Cout, S in neck_shapes():
            for fo in (0, 1):
                d = types.SimpleNamespace(Cin=Cin, Cout=Cout, fuse_offset=fo)
                for algo, sk in autotune._dcn_candidates(d) + ([(0, 0)] if fo else []):
                    p = D.dcn_plan(N, S, S, Cin, Cout, algo, sk, fo)
                    keys = _plan_keys(p, 0)
                    assert keys <= reached, ((N, Cin, Cout, S), algo, sk, fo, sorted(keys - reached, key=str))
                    seen.add((algo, sk))
                    n += 1
    assert n > 250 and seen >= {(a, s) for a in (64, 128, 3264, 32128) for s in (1, 2, 4, 8, 16)} | {(0, 0)}


# ---------------------------------------------------------------------------------------------------------------------
# the references

ALL_CASES = D.GPU_CASES + [c for g in D.GROUPS for c in g.layers]


def test_sample_cols_is_the_oracles_dcn():
    from oracle import dcn_v2 as odcn
    case = D.CASE['ldom28_cin96']
    d = D.dcn_inputs(case)
    off, mask = D.offsets_and_mask(case, torch.float64)
    x, w = d['x'].double(), d['w'].double()
    z = torch.einsum('ock,bckp->bop', w.reshape(case.Cout, case.Cin, 9), D.sample_cols(x, off, mask)).view(case.N, case.Cout, case.H, case.W)
    assert D.err(z, odcn.dcn_v2_conv(x, off, mask, w, None)) < 1e-14


def test_the_float32_references_pass_their_own_bound():
    for case in ALL_CASES:
        r32 = D.reference32(case)
        assert D.outputs_of(case), case.name
        for which in D.outputs_of(case):
            e, e32, b = D.case_errors(case, r32[which], which)
            assert e <= b and b <= 1e-4, (case.name, which, e, b)


def test_the_bound_notices_a_fault():
    """a dropped (chunk, tap) term of one tile, an omitted split partial of one cout tile and exchanged fractions in the border
    cells each exceed the bound of every case, on that case's inputs"""
    for case in ALL_CASES:
        r64, muts = D.reference64(case), D.mutants64(case)
        assert len(muts) == 3, (case.name, sorted(muts))
        for what, out in muts.items():
            worst = max(D.err(out[w], r64[w]) / D.case_errors(case, r64[w], w)[2] for w in D.outputs_of(case))
            assert worst > 1.0, (case.name, what, worst)


# ---------------------------------------------------------------------------------------------------------------------
# argument errors: every CT_FAIL_ARG of make_plan and launch_group, with fake pointers and no launch

def test_every_argument_error_is_refused_before_a_launch(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    base = dict(N=1, H=8, W=16, Cin=64, Cout=64)

    def refused(word, want=_lib.CT_ERR_ARG, grouped=False, phases=7, n=1, **kw):
        args = dict(base)
        args.update((k, kw.pop(k)) for k in list(kw) if k in base or k in ('algo', 'split_k', 'fuse_offset', 'up_f'))
        d = _desc(p, **args, **kw)
        rc = lib.ct_dcn_v2_group((_lib.DcnDesc * 4)(d, d, d, d), n, phases, None) if grouped else lib.ct_dcn_v2(ctypes.byref(d), None)
        assert rc == want and word in lib.ct_last_error(), (word, kw, rc, lib.ct_last_error())
    # make_plan
    refused(b'null pointer', x=None)
    refused(b'null pointer', w_packed=None)
    refused(b'null pointer', y=None)
    refused(b'fuse_offset=4', fuse_offset=4)
    refused(b'fuse_offset=-1', fuse_offset=-1)
    refused(b'needs w_off_packed and b_off', fuse_offset=1, b_off=None)
    refused(b'needs w_off_packed and b_off', fuse_offset=2, w_off_packed=None)
    refused(b'fuse_offset needs Cin', fuse_offset=1, Cin=96)
    refused(b'bytes of om_partial', _lib.CT_ERR_WORKSPACE, fuse_offset=2, om_partial_bytes=16)
    refused(b'bytes of om_partial', _lib.CT_ERR_WORKSPACE, fuse_offset=3, om_partial=None)
    refused(b'null offset/mask map', om=None)
    refused(b'without up_skip / up_y', up_f=2, up_skip=None)
    refused(b'up_f=3', up_f=3)
    refused(b'16-byte aligned with Cout', up_f=2, Cout=62)
    refused(b'16-byte aligned with Cout', up_f=2, up_lds=66)
    refused(b'16-byte aligned with Cout', up_f=2, up_y=odd)
    refused(b'positive multiple of 32', Cin=48)
    refused(b'input view must be 16-byte aligned', x=odd)
    refused(b'input view must be 16-byte aligned', ldx=66)
    refused(b'>= 27 channels', ldom=26)
    refused(b'bad shape', Cout=0)
    refused(b'bad shape', H=0)
    refused(b'NCHW output unsupported', flags=_lib.CT_OUT_NCHW)
    refused(b'unknown algo', algo=7)
    refused(b'persistent shapes', algo=53264, fuse_offset=1)
    refused(b'layers of a group run on', grouped=True, algo=64, fuse_offset=1)
    refused(b'fuse_offset runs on the 32-pixel tiles', algo=128, fuse_offset=1)
    refused(b'64-channel-step shapes need Cin', algo=43264, Cin=96)
    refused(b'even number of', algo=53264, split_k=2)
    refused(b'even number of', algo=63264, split_k=1)
    refused(b'channel pitch of x', ldx=60)
    refused(b'channel pitch of y', ldy=60, split_k=1)                # (the direct store; a split layer's y goes through the reduce kernel)
    # launch_group and ct_dcn_v2_group
    refused(b'layers per launch', grouped=True, n=0)
    refused(b'layers per launch', grouped=True, n=5)
    refused(b'phases must be', grouped=True, phases=0)
    refused(b'phases must be', grouped=True, phases=8)
    refused(b'workspace bytes', _lib.CT_ERR_WORKSPACE, split_k=2, workspace_bytes=16)
    refused(b'workspace bytes', _lib.CT_ERR_WORKSPACE, split_k=2, workspace=None)
    d0, d1 = _desc(p, algo=3264, **base), _desc(p, algo=32128, **base)
    assert lib.ct_dcn_v2_group((_lib.DcnDesc * 2)(d0, d1), 2, 7, None) == _lib.CT_ERR_ARG and b'another tile shape' in lib.ct_last_error()
    assert lib.ct_dcn_v2_group_plan(None, None, None) == _lib.CT_ERR_ARG
    # (`the 64-channel-step shapes run on 32-pixel tiles` of launch_group cannot be reached: make_plan gives NKK 4 only to algo
    #  43264 / 432128, which set BM 32; the three `grid too large` lines of launch_group lie behind make_plan's own, pinned below)


# ---------------------------------------------------------------------------------------------------------------------
# what the kernels can address, from both sides

# the accepted side of each limit: descriptors a child process without a device passes to ct_dcn_v2 / ct_dcn_v2_group
BELOW = {
    'x view': dict(N=1, H=2048, W=2048, Cin=64, Cout=16, ldx=128, algo=3264, split_k=1),              # ((2^22 - 1) 128 + 64) 4 = 2^31 - 256
    'pixels': dict(N=1, H=2048, W=4096, Cin=32, Cout=16, ldx=32, algo=3264, split_k=1),               # H*W = 2^23 exactly
    'y view': dict(N=1, H=1024, W=1024, Cin=32, Cout=64, ldy=512, algo=3264, split_k=1),              # ((2^20 - 1) 512 + 64) 4 = 2^31 - 1792
    'ldx': dict(N=1, H=1, W=2, Cin=32, Cout=16, ldx=(1 << 21) - 4, algo=3264, split_k=1),
    'ldy': dict(N=1, H=1, W=2, Cin=32, Cout=16, ldy=(1 << 23) - 1, algo=3264, split_k=1),
    'partial map': dict(N=1, H=2048, W=2048, Cin=64, Cout=112, algo=3264, split_k=2),                 # 2^22 * 112 floats < 2^29
    'persistent om': dict(N=3, H=2048, W=2048, Cin=64, Cout=16, ldom=40, algo=53264, split_k=1),      # ((3 * 2^22 - 1) 40 + 27) 4 < 2^31
    'persistent x': dict(N=3, H=2048, W=2048, Cin=64, Cout=16, ldx=84, algo=53264, split_k=1),        # 3 * 2^22 * 84 * 4 = 2^32 - 2^26
    'y of a split layer': dict(N=1, H=2048, W=2048, Cin=64, Cout=16, ldy=256, algo=3264, split_k=2),  # 4 GiB of y through the reduce kernel
    # 2^22 pixels x 64 taps' worth of output pixels x pitch 12 = 2^32 - 2^30 elements; the partial map is 2^26 floats
    'IDAUp view': dict(N=1, H=2048, W=2048, Cin=64, Cout=12, algo=3264, split_k=2, up_f=8),
    'grid': dict(N=1 << 20, H=16, W=16, Cin=64, Cout=8128, algo=3264, split_k=1),                     # 2^23 pixel tiles x 127 cout blocks < 2^30
    'packed weight': dict(N=1, H=4, W=4, Cin=8192, Cout=7280, algo=3264, split_k=1),                  # 9 * 512 * 455 KiB = 2^31 - 512 KiB
}


def test_dcn_refuses_what_its_kernels_cannot_address(lib):
    from centertrack_amd import _lib
    keep, p = _ptr()

    def refused(word, grouped=False, **kw):
        d = _desc(p, **kw)
        rc = lib.ct_dcn_v2_group(ctypes.byref(d), 1, 7, None) if grouped else lib.ct_dcn_v2(ctypes.byref(d), None)
        assert rc == _lib.CT_ERR_ARG and word in lib.ct_last_error(), (word, kw, rc, lib.ct_last_error())
    B = BELOW
    refused(b'2 GiB or more per image (x', **dict(B['x view'], ldx=132))
    refused(b'24 bits', **dict(B['pixels'], W=4097))
    refused(b'24 bits', **dict(B['ldx'], ldx=1 << 21))
    refused(b'2 GiB or more per image (y', **dict(B['y view'], ldy=516))
    refused(b'24 bits', **dict(B['ldy'], ldy=1 << 23))
    refused(b'partial map', **dict(B['partial map'], Cout=128))                   # 2^22 * 128 = 2^29 floats: 2 GiB
    refused(b'partial map', grouped=True, **dict(B['partial map'], Cout=128))
    refused(b'offset/mask map of 2 GiB', **dict(B['persistent om'], ldom=44))
    refused(b'input view of 4 GiB', N=5, H=2048, W=2048, Cin=64, Cout=16, ldx=64, algo=53264, split_k=1)
    refused(b'input view of 4 GiB', **dict(B['persistent x'], ldx=88))
    refused(b'IDAUp output too large', **dict(B['IDAUp view'], up_lds=16))        # 2^28 output pixels at pitch 16: 2^32 elements
    refused(b'IDAUp output too large', **dict(B['IDAUp view'], up_ldy=16))
    refused(b'IDAUp output too large', grouped=True, **dict(B['IDAUp view'], up_ldy=16))
    refused(b'grid too large', **dict(B['grid'], Cout=8192))                      # 2^23 pixel tiles x 128 cout blocks = 2^30
    refused(b'packed weight of 2 GiB', **dict(B['packed weight'], Cout=7296))     # 9 * 512 * 456 KiB = 2^31 + 4 MiB
    # just below each limit the call passes validation and reaches the launch, which this test must not let happen on a GPU: a
    # child process that sees no device makes the calls, and gets the launch error of a machine without one
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.dirname(__file__)] + sys.path))
    code = ('import ctypes, json, torch\n'
            'import test_dcn_forward_cpu as T\n'
            'from centertrack_amd import _lib\n'
            'if torch.cuda.device_count() > 0:\n'
            '    print(json.dumps("a device is visible: not launching")); raise SystemExit(0)\n'
            'lib = _lib.load(); keep, p = T._ptr(); out = {}\n'
            'for name, kw in T.BELOW.items():\n'
            '    rc = lib.ct_dcn_v2(ctypes.byref(T._desc(p, **kw)), None)\n'
            '    out[name] = [rc, lib.ct_last_error().decode()]\n'
            'print(json.dumps(out))\n')
    r = subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert isinstance(out, dict) and sorted(out) == sorted(BELOW), out
    for name, (rc, msg) in out.items():
        assert rc in (_lib.CT_OK, _lib.CT_ERR_LAUNCH), (name, rc, msg)


# ---------------------------------------------------------------------------------------------------------------------
# production launches

def _pinned_schedules():
    table = json.load(open(os.path.join(ROOT, 'centertrack_amd', 'tune_table.json')))
    out = []
    for key, val in table.items():
        if key.startswith('dcnplan4:') or key.startswith('dcnplan5:'):
            N, H, W = [int(v) for v in key.split(':')[1].split(',')]
            out.append((key, N, H, W, tuple(int(v) for v in val[:-1])))
    return out


def _knob_grid(N, H, W):
    """the tuples model.py::_tune_dcn_schedule walks (restated: dcn_schedule.knob_grid is held against this), with the persistent
    second stage on top of every one of them"""
    layers = D.neck_layers(H, W)
    for fuse_max in (0, 64, 128, 256):
        for cps in (2, 4, 8):
            small = [t for t, w in D._slot_sizes(layers, N, cps)[0].items() if w < D.SMALL_SLOT_WGS]
            for nkk in (2, 4):
                for so in ((1, 2, 3) if fuse_max < 256 else (1,)):
                    for cs, un in (((0, 0), (0, 2)) + tuple((c, u) for c in (2, 1) if c < cps for u in (0, 1, 2)) if small else ((0, 0), (0, 2))):
                        yield (fuse_max, cps, nkk, so, cs, un, 0)
                        yield (fuse_max, cps, nkk, so, cs, un, 1)


def test_production_schedules_reach_only_tested_regimes():
    """the 16 neck layers as the model launches them (restated: tests/_dcn_fwd.py::neck_schedule, held against dcn_schedule.plan below
    and against the model's plan_signature by tests/test_hip_dcn_forward.py) for every pinned dcnplan4 / dcnplan5 entry and for the tuner's whole knob grid at
    the pinned sizes"""
    reached = D.all_keys(D.GPU_CASES, D.GROUPS)
    pinned = _pinned_schedules()
    assert len(pinned) >= 28
    n = 0
    for key, N, H, W, knobs in pinned:
        launches, info = D.neck_schedule(knobs, N, H, W)
        assert len(info) == 16
        keys = D.schedule_keys(launches, info, N)
        assert keys <= reached, (key, knobs, sorted(keys - reached, key=str))
    for N, H, W in sorted(set(p[1:4] for p in pinned)):
        for knobs in _knob_grid(N, H, W):
            launches, info = D.neck_schedule(knobs, N, H, W)
            keys = D.schedule_keys(launches, info, N)
            assert keys <= reached, ((N, H, W), knobs, sorted(keys - reached, key=str))
            n += 1
    assert n > 5000


# ---------------------------------------------------------------------------------------------------------------------
# the planner the model, the tuner and the tools use (centertrack_amd/dcn_schedule.py) against the restatement above

def _planner_layers(H, W):
    from centertrack_amd import dcn_schedule as S
    return [S.Layer(*ly) for ly in D.neck_layers(H, W)]


def _grid_both_ways(layers, N):
    """the tuner's first stage, each tuple also with split_offsets = 0 once, all of them without and with persistent launches"""
    from centertrack_amd import dcn_schedule as S
    for k in S.knob_grid(layers, N):
        for so in ((k[3], 0) if k[3] == 1 else (k[3],)):
            for persist in (0, 1):
                yield k[:3] + (so,) + k[4:6] + (persist,)


def _same_schedule(sched, launches, info, what):
    got = [(l.tag, list(l.names), l.phase, [(a, sched.layers[n].splits, D.FUSE_OFFSET[sched.layers[n].src]) for a, n in zip(l.algos, l.names)])
           for l in sched.launches if l.tag != 'conv']
    assert got == launches, what
    assert list(sched.layers) == list(info), what
    for name, p in sched.layers.items():
        i = info[name]
        assert (p.main, p.finish, p.fused, p.src, p.nkk, p.splits) == (i['main'], i['finish'], i['fused'], i['src'], i['nkk'], i['split_k']), (what, name)


def test_the_planner_is_the_restated_schedule():
    """dcn_schedule.plan on the 16 neck layers equals neck_schedule -- group launches as (tag, names, phase, (algo, split_k,
    fuse_offset)), per layer main / finish / fused / src / nkk / split_k -- for every pinned entry and for the tuner's grid, with
    split_offsets = 0 and the persistent stage on top, at every pinned size"""
    from centertrack_amd import dcn_schedule as S
    pinned = _pinned_schedules()
    for key, N, H, W, knobs in pinned:
        _same_schedule(S.plan(_planner_layers(H, W), N, knobs), *D.neck_schedule(knobs, N, H, W), what=(key, knobs))
    n = 0
    for N, H, W in sorted(set(p[1:4] for p in pinned)):
        layers = _planner_layers(H, W)
        for knobs in _grid_both_ways(layers, N):
            sched = S.plan(layers, N, knobs)
            launches, info = D.neck_schedule(knobs, N, H, W)
            _same_schedule(sched, launches, info, ((N, H, W), knobs))
            assert S.signature(sched) == D.schedule_signature(launches)
            n += 1
    assert n > 20000
    # the switch the package passes for CENTERTRACK_FUSE_OFFSET=0
    for knobs in ((128, 4, 2, 1, 0, 0, 0), (256, 8, 4, 1, 2, 2, 0)):
        _same_schedule(S.plan(_planner_layers(512, 512), 1, knobs, fuse_enabled=False), *D.neck_schedule(knobs, 1, 512, 512, fuse_enabled=False), what=knobs)


def test_knob_grid_is_the_tuners_first_stage_in_order():
    from centertrack_amd import dcn_schedule as S
    for N, H, W in sorted(set(p[1:4] for p in _pinned_schedules())):
        assert list(S.knob_grid(_planner_layers(H, W), N)) == [k for k in _knob_grid(N, H, W) if k[6] == 0], (N, H, W)
    # the second stage: the five fastest and every later schedule with all offset convs outside the MAIN launches, persist set
    tried = [(10.0 + i, (fm, 4, 2, 1, 0, un, 0)) for i, (fm, un) in enumerate([(128, 0), (0, 2), (64, 0), (0, 0), (256, 0), (128, 2), (0, 0), (0, 1), (64, 2)])]
    got = S.persist_candidates(list(reversed(tried)))
    assert got == [(us, k[:6] + (1,)) for us, k in tried[:5] + [tried[6]]]


def test_normalize_reads_every_table_generation():
    from centertrack_amd import dcn_schedule as S
    assert S.normalize((128, 4, 2)) == (128, 4, 2, 1, 0, 0, 0)
    assert S.normalize([64, 8, 4, 0]) == (64, 8, 4, 0, 0, 0, 0)
    assert S.normalize((0, 4, 4, 3, 2, 1)) == (0, 4, 4, 3, 2, 1, 0)
    assert S.normalize((0, 4, 2, 1, 0, 0, 1)) == (0, 4, 2, 1, 0, 0, 1)
    assert S.normalize((128.0, 4.0, 2.0, 1.0, 0.0, 0.0)) == (128, 4, 2, 1, 0, 0, 0) and all(type(v) is int for v in S.normalize((128.0, 4.0, 2.0)))


def test_the_planners_workspace_and_persist_rules_are_the_librarys(lib):
    """over every distinct (Cin, splits, nkk, fused, up) the grid reaches at the pinned sizes: ct_dcn_v2_group_plan reports workspace
    bytes exactly where the planner says use_ws, and accepts the persistent algo exactly where can_persist holds"""
    from centertrack_amd import dcn_schedule as S
    keep, ptr = _ptr()
    combos = {}
    for N, H, W in sorted(set(p[1:4] for p in _pinned_schedules())):
        layers = _planner_layers(H, W)
        for knobs in _grid_both_ways(layers, N):
            for p in S.plan(layers, N, knobs).layers.values():
                combos.setdefault((p.layer.Cin, p.splits, p.nkk, p.fused, p.layer.up is not None), (N, p))
    assert len(set(c[:4] for c in combos)) == 37 and any(c[4] for c in combos)
    for (Cin, splits, nkk, fused, up), (N, p) in sorted(combos.items()):
        ly, fo = p.layer, S.FUSE_OFFSET[p.src]
        need = ctypes.c_size_t(0)
        d = _desc(ptr, N, ly.H, ly.W, Cin, ly.cout, 3264, splits, fo, ly.up[0] if up else 0)
        assert lib.ct_dcn_v2_group_plan(ctypes.byref(d), ctypes.byref(need), None) == 0, (ly.name, lib.ct_last_error())
        assert (need.value > 0) == p.use_ws, (Cin, splits, nkk, fused, up, need.value)
        d = _desc(ptr, N, ly.H, ly.W, Cin, ly.cout, 63264 if nkk == 4 else 53264, splits, fo, ly.up[0] if up else 0)
        rc = lib.ct_dcn_v2_group_plan(ctypes.byref(d), None, None)
        assert (rc == 0) == S.can_persist(Cin, splits, nkk, fused), (Cin, splits, nkk, fused, up, rc, lib.ct_last_error())


@pytest.mark.parametrize('split_offsets', [0, 2])
def test_offset_convs_run_ahead_of_their_slots_groups(split_offsets):
    """one `.offset` conv entry per un-fused layer, in layer order, ahead of the OFFSETS / MAIN / FINISH groups of the layer's slot"""
    from centertrack_amd import dcn_schedule as S
    N, H, W = 1, 512, 512
    layers = _planner_layers(H, W)
    for knobs in ((128, 4, 2, split_offsets, 0, 0, 0), (0, 4, 4, split_offsets, 2, 1, 1), (64, 8, 4, split_offsets, 1, 2, 0)):
        sched = S.plan(layers, N, knobs)
        launches, info = D.neck_schedule(knobs, N, H, W)
        want = []
        for t in sorted(set(i['main'] for i in info.values()) | set(i['finish'] for i in info.values() if i['finish'] is not None)):
            want += [('conv', (ly.name,)) for ly in layers if info[ly.name]['main'] == t and not info[ly.name]['fused']]
            want += [(tag, tuple(names)) for tag, names, phase, _ in launches if info[names[0]]['finish' if phase == 2 else 'main'] == t]
        assert [(l.tag, l.names) for l in sched.launches] == want, knobs
        convs = [l for l in sched.launches if l.tag == 'conv']
        assert convs and all(l.phase == 0 and l.algos == () for l in convs)
        assert all(p.src == ('fused' if p.fused else 'raw' if split_offsets else 'map') for p in sched.layers.values())
