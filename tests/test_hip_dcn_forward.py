"""GPU: every launch ``ct_dcn_v2`` and ``ct_dcn_v2_group`` can make (tests/_dcn_fwd.py: GPU_CASES and GROUPS, one per regime of its
table) against a float64 reference of the whole operation under the bound of the backward tests, min(1e-3, 4 max(e32, 2^-23
sqrt(K))) with K = 9 Cin (+ 4 with an IDAUp step) and e32 the error of the float32 reference by the same measure.  x, the
offset/mask map and skip are read from channel slices of NaN-filled buffers, each at a pitch of its own; y and up_y are written
into NaN-filled slices between guard channels; workspaces and om_partial start as NaN.  Every test prints its figures (``pytest -s``).

Then what must not change a bit, asserted where the summation order is the same by reading dcn_mfma.hip:
  * a repeat of the launch;
  * dcn_xcd 0 against 1 (the id decode picks the tile, nothing else), one case per xsx, with and without padded ids;
  * the persistent form against the per-tile form (same tiles, same K order, same splits) at three slot counts;
  * a group against its layers launched singly, the three phases in one call against three calls, FINISH calls on other sets of
    layers than the MAIN call (a layer's workgroups do not depend on its neighbours);
  * the fused IDAUp finish against the plain finish followed by ``ops.upsample_add`` (dcn_reduce_kernel applies
    ct_epilogue_value and accumulates the taps jy, jx in upsample_add_kernel's order);
  * the workgroups with rot 1, 2, 3 against the same images launched one by one (256 workgroups each: rot 0).
Left to float64 alone: fuse_offset 0 fed the map of ``ops.conv2d(..., sig=(18, 27))`` against fuse_offset 1 / 2 / 3 -- ct_conv2d
picks its own tile shape and K split for the 27-channel conv and applies an exact sigmoid where the DCN kernel uses v_exp / v_rcp, so
the maps are not the same numbers; each source is checked against float64 on its own."""
import contextlib
import ctypes

import pytest
import torch

import _dcn_fwd as D
from _guards import NAN, guarded, slice_of, take, untouched

pytestmark = pytest.mark.gpu

ALL = 1 | 2 | 4                                    # CT_DCN_MAIN | CT_DCN_FINISH | CT_DCN_OFFSETS
MAIN, FINISH, OFFSETS = 1, 2, 4


@contextlib.contextmanager
def tuning(knobs):
    from centertrack_amd import _lib
    lib = _lib.load()
    try:
        for k, v in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), v), k)
        yield
    finally:
        for k, _ in knobs:
            _lib.check(lib.ct_set_tuning(k.encode(), D.KNOBS[k]), k)


class Built(object):
    pass


def build(case, device, inputs=None, up=True):
    """the descriptor of a case on fresh caller buffers"""
    from centertrack_amd import _lib, ops
    lib = _lib.load()
    d = inputs or D.dcn_inputs(case)
    N, H, W, Cout = case.N, case.H, case.W, case.Cout
    b = Built()
    b.case, b.xv = case, slice_of(d['x'], device)
    wp = ops.pack_weight(d['w'].to(device))
    own = case.src in D.OWN
    om = part = wop = wow = bo = None
    if own:
        wod = d['wo'].to(device)
        wop, bo = ops.pack_weight(wod), d['bo'].to(device)
        if case.src != 'fused':
            part = torch.full((D.offsets_bytes(N, H, W, case.Cin, D.FUSE_OFFSET[case.src]) // 4,), NAN, device=device)
        if case.src == 'wino':
            wow = ops.pack_winograd(wod)
        if case.src == 'raw':                       # raw sums by a plain conv launch: no bias, no sigmoid
            ops.conv2d(b.xv, wop, 27, 3, 1, out=ops.View(part.view(N, H, W, 32), 0, 27))
    else:
        omt = torch.cat([d['off'], d['mask']], 1)
        if case.src == 'slice':
            om = slice_of(omt, device, c0=8, tail=5)
        else:
            buf = torch.full((N, H, W, case.ldom), NAN)
            buf[..., :27] = omt.permute(0, 2, 3, 1)
            om = ops.View(buf.to(device), 0, 27)
    b.yv = guarded(N, H, W, Cout, device)
    b.upv = b.wt = b.sv = None
    upt = None
    if case.up_f:
        f = case.up_f
        b.wt, b.sv = ops.upsample_weight(d['wup'].to(device)), slice_of(d['skip'], device, c0=8, tail=8)
        if up:
            b.upv = guarded(N, H * f, W * f, Cout, device, c0=8)
            upt = (b.wt, f, b.sv, b.upv)
    scale, shift = d['scale'].to(device), d['shift'].to(device)
    b.desc = ops.make_dcn_desc(b.xv, om, wp, Cout, scale, shift, True, b.yv, split_k=case.split_k, algo=case.algo,
                               w_off=wop if (own and case.src != 'raw') else None, b_off=bo, up=upt, om_partial=part,
                               raw_offsets=case.src == 'raw', w_off_wino=wow)
    assert b.desc.fuse_offset == D.FUSE_OFFSET[case.src] and lib.ct_dcn_v2_offsets_bytes(ctypes.byref(b.desc)) == (part.numel() * 4 if part is not None else 0)
    query = lib.ct_dcn_v2_group_workspace_bytes if case.entry == 'group' else lib.ct_dcn_v2_workspace_bytes
    need = query(ctypes.byref(b.desc))
    if up or not case.up_f:
        assert need == D.plan_of(case)['bytes'], (case.name, need)
    b.ws = torch.full((max(need, 4) // 4,), NAN, device=device)
    b.desc.workspace, b.desc.workspace_bytes = b.ws.data_ptr(), need
    b.keep = (wp, wop, wow, bo, om, part, scale, shift, d)       # (the descriptor holds raw pointers)
    return b


def collect(b):
    """dict(y[, up]) NCHW on the CPU; a view the launch does not produce must be untouched"""
    torch.cuda.synchronize()
    out, case = {}, b.case
    produces_y = b.upv is None or D.y_written(case)
    if produces_y:
        out['y'] = take(b.yv, case.name + ' y')
    else:
        untouched(b.yv, case.name + ' y')
    if b.upv is not None:
        out['up'] = take(b.upv, case.name + ' up_y')
    return out


def run_single(case, device, inputs=None, up=True):
    from centertrack_amd import _lib
    lib = _lib.load()
    with tuning(case.knobs):
        b = build(case, device, inputs, up)
        _lib.check(lib.ct_dcn_v2(ctypes.byref(b.desc), _lib.stream_ptr()), 'ct_dcn_v2 ' + case.name)
        out = collect(b)
    return out, b


def run_group(layers, calls, device, knobs=()):
    """``calls``: [(layer indices, phases)] -> the outputs of every layer"""
    from centertrack_amd import _lib
    lib = _lib.load()
    with tuning(knobs):
        built = [build(c, device) for c in layers]
        for idx, phases in calls:
            arr = (_lib.DcnDesc * len(idx))(*[built[i].desc for i in idx])
            _lib.check(lib.ct_dcn_v2_group(arr, len(idx), phases, _lib.stream_ptr()), 'ct_dcn_v2_group %s phases %d' % (idx, phases))
        return [collect(b) for b in built]


def run(case, device):
    if case.entry == 'group':
        return run_group([case], [([0], ALL)], device, case.knobs)[0]
    return run_single(case, device)[0]


def same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), '%s: %s differs in %d elements' % (what, k, int((a[k] != b[k]).sum()))


def family_of(case):
    p = D.plan_of(case)
    return ('persist' if p['family'] == 'persist' else 'tile%dx%d' % (p['BM'], p['BN'])) + ('+split' if p['splits'] > 1 else '') + ('+up' if case.up_f else '')


def check(case, got):
    """err <= bound on every output the case produces, one DCNFWD line each"""
    assert sorted(got) == sorted(D.outputs_of(case)), (case.name, sorted(got))
    bad = []
    for which in D.outputs_of(case):
        e, e32, b = D.case_errors(case, got[which], which)
        print('DCNFWD %-24s %-18s %-2s err %.3e e32 %.3e bound %.3e ratio %.3f' % (case.name, family_of(case), which, e, e32, b, e / b))
        if not e <= b:
            bad.append('%s err %.3e > bound %.3e' % (which, e, b))
    assert not bad, '%s (%s): %s' % (case.name, case.why, bad)


@pytest.mark.parametrize('name', list(D.CASE))
def test_dcn_case_against_float64(device, name):
    case = D.CASE[name]
    got = run(case, device)
    check(case, got)
    same(got, run(case, device), name + ': a repeat of the launch')


def _calls(g):
    n = len(g.layers)
    every = list(range(n))
    if g.mode == 'one call':
        return [(every, ALL)]
    if g.mode == 'three calls':
        return [(every, OFFSETS), (every, MAIN), (every, FINISH)]
    # the OFFSETS call only on the layers that need one, MAIN on all (longest workgroups first), FINISH on two other sets
    need = [i for i, c in enumerate(g.layers) if c.src in ('parts', 'wino')]
    return [(need, OFFSETS), (every, MAIN), ([1, 3], FINISH), ([0, 2], FINISH)]


@pytest.mark.parametrize('name', list(D.GROUP))
def test_dcn_group_against_float64_and_single_launches(device, name):
    g = D.GROUP[name]
    plans = [D.plan_of(c) for c in g.layers]
    assert len(set((p['BM'], p['BN'], p['NKK'], p['family']) for p in plans)) == 1
    got = run_group(g.layers, _calls(g), device, g.knobs)
    for c, out in zip(g.layers, got):
        check(c, out)
    if g.mode != 'one call':
        for c, a, b in zip(g.layers, got, run_group(g.layers, [(list(range(len(g.layers))), ALL)], device, g.knobs)):
            same(a, b, '%s: %s against the three phases in one call' % (name, g.mode))
    # each layer alone through ct_dcn_v2, same tile shape and split: an up layer then writes y too (and, unsplit, finishes through
    # ct_upsample_add instead of the reduce kernel)
    for c, p, out in zip(g.layers, plans, got):
        one = c._replace(entry='single', split_k=p['splits'], name=c.name)
        alone, _ = run_single(one, device)
        for which in out:
            assert torch.equal(out[which], alone[which]), '%s layer %s: %s differs from the single launch' % (name, c.name, which)


def _xcd_cases():
    seen, names = set(), []
    for c in D.GPU_CASES:
        p = D.plan_of(c)
        key = (p['xsx'], p['padded'])
        if p['family'] == 'tile' and p['xsx'] and key not in seen and c.entry == 'single':
            seen.add(key)
            names.append(c.name)
    return names


@pytest.mark.parametrize('name', _xcd_cases())
def test_dcn_xcd_order_changes_no_bit(device, name):
    case = D.CASE[name]
    p0 = D.plan_of(case, (('dcn_xcd', 0),))
    assert D.plan_of(case)['xsx'] and not p0['xsx']
    on, _ = run_single(case._replace(knobs=case.knobs + (('dcn_xcd', 1),)), device)
    off, _ = run_single(case._replace(knobs=case.knobs + (('dcn_xcd', 0),)), device)
    same(on, off, name + ': dcn_xcd 1 against 0')


@pytest.mark.parametrize('name', list(D.PERSISTABLE))
def test_dcn_persistent_form_is_bit_identical_to_the_per_tile_form(device, name):
    """every case make_plan lets run persistent (tests/_dcn_fwd.py::persistent_form), not only those that carry a persistent algo: K splits
    in a single launch, maps at a pitch of 31 and as a slice, Winograd-written parts, H < 2 rows, Cout < BN, the legacy_up tail"""
    pers = D.PERSISTABLE[name]
    p = D.plan_of(pers)
    assert p['family'] == 'persist'
    tile = run(pers._replace(algo=D.tile_algo(pers)), device)
    for which, slots in D.slot_counts(p).items():
        per_col, grid = D.persist_partition([p], slots)
        assert grid <= max(slots, p['coutBlocks'] * p['splits']) and per_col[0] >= 1
        got = run(pers._replace(knobs=pers.knobs + (('dcn_slots', slots),)), device)
        same(got, tile, '%s: persistent at dcn_slots %d (%s: %d workgroups per column) against algo %d' % (name, slots, which, per_col[0], D.tile_algo(pers)))


@pytest.mark.parametrize('name', [c.name for c in D.GPU_CASES if c.up_f and D.plan_of(c)['use_ws']])
def test_dcn_fused_idaup_finish_equals_finish_then_upsample_add(device, name):
    from centertrack_amd import ops
    case = D.CASE[name]
    fused, _ = run_single(case, device)
    plain, b = run_single(case, device, up=False)
    upv = guarded(case.N, case.H * case.up_f, case.W * case.up_f, case.Cout, device, c0=8)
    ops.upsample_add(b.yv, b.wt, case.up_f, b.sv, out=upv)
    torch.cuda.synchronize()
    assert torch.equal(take(upv, name + ' upsample_add'), fused['up']), name
    e, e32, bd = D.case_errors(case, plain['y'], 'y')
    assert e <= bd, (name, e, bd)


def test_dcn_rot_workgroups_equal_the_images_launched_one_by_one(device):
    case = D.CASE['rot']
    p, d = D.plan_of(case), D.dcn_inputs(case)
    one = case._replace(N=1)
    p1 = D.plan_of(one)
    assert D.rots(p) == [0, 1, 2, 3] and D.rots(p1) == [0] and (p1['splits'], p1['chunksPerSplit']) == (p['splits'], p['chunksPerSplit'])
    whole, _ = run_single(case, device)
    for n in range(case.N):
        sub = dict((k, v[n:n + 1] if k in ('x', 'off', 'mask') else v) for k, v in d.items())
        got, _ = run_single(one, device, inputs=sub)
        assert torch.equal(got['y'][0], whole['y'][n]), 'image %d' % n


# ---------------------------------------------------------------------------------------------------------------------
# the real schedule: keeps tests/_dcn_fwd.py::neck_schedule (and with it test_production_schedules_reach_only_tested_regimes) honest

# between them: split_offsets 0, 1, 2 and 3 (every offset source), nkk 2 and 4, fine-split small slots with and without their offset
# convs moved out, persistent
SCHEDULE_KNOBS = [(128, 4, 2, 1, 0, 0, 0), (0, 4, 4, 3, 2, 1, 0), (64, 8, 4, 2, 1, 2, 0), (0, 4, 2, 1, 0, 0, 1), (0, 4, 4, 1, 0, 0, 1),
                  (128, 4, 2, 0, 0, 0, 0)]


@pytest.mark.parametrize('knobs', SCHEDULE_KNOBS, ids=lambda k: '-'.join(str(v) for v in k))
def test_the_models_dcn_schedule_is_the_restated_one(device, monkeypatch, knobs):
    from centertrack_amd import dcn_schedule as S, weights as Wt
    from centertrack_amd.model import DLASegHIP
    N, H, W = 1, 64, 96
    monkeypatch.setenv('CENTERTRACK_DCN_KNOBS', ','.join(str(v) for v in knobs))
    model = DLASegHIP(Wt.MOT_HEADS)
    model.load_state_dict(Wt.make_synthetic_state_dict(Wt.MOT_HEADS, seed=317, off_std=0.01))
    model = model.to(device)
    plan = model.get_plan(N, H, W, True, True, False)
    torch.cuda.synchronize()
    assert tuple(plan['dcn_knobs']) == tuple(knobs)
    got = [s for s in DLASegHIP.plan_signature(plan).split(';') if ':dcn:' in s]
    launches, info = D.neck_schedule(knobs, N, H, W)
    assert got == D.schedule_signature(launches), '\n'.join(['model:'] + got + ['restated:'] + D.schedule_signature(launches))
    # ... and the planner's (centertrack_amd/dcn_schedule.py), which the CPU tests hold against the restatement on the whole grid
    sched = S.plan([S.Layer(*ly) for ly in D.neck_layers(H, W)], N, knobs)
    assert got == S.signature(sched)
    assert [l.name for l in plan['launches'] if l.name.endswith('.offset')] == [l.names[0] + '.offset' for l in sched.launches if l.tag == 'conv']
    # every DCN descriptor has a workspace exactly where the planner said so
    seen = set()
    for l in plan['launches']:
        if l.fn == 'dcn_group':
            arr, n, _ = l.args
            for j, name in enumerate(l.name[l.name.index('[') + 1:-1].split(' + ')):
                has = bool(arr[j].workspace) and arr[j].workspace_bytes > 0
                assert has == sched.layers[name].use_ws and has == (info[name]['finish'] is not None), (l.name, name)
                seen.add(name)
    assert seen == set(sched.layers) and len(seen) == 16
    if knobs[3] == 0:
        assert any(p.src == 'map' for p in sched.layers.values()), 'no offset/mask map written by a conv launch in this schedule'
    if knobs[6]:
        assert any(t[0] >= 50000 for _, _, ph, triples in launches if ph == MAIN for t in triples), 'no persistent launch in this schedule'
