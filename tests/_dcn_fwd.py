"""Shared pieces of the DCNv2 forward tests (tests/test_dcn_forward_cpu.py, tests/test_hip_dcn_forward.py): the launch plan of
``ct_dcn_v2`` / ``ct_dcn_v2_group`` restated from ``make_plan``, ``ws_bytes``, ``ct_dcn_v2_offsets_bytes``, ``fill_args`` and the
persistent partition of ``launch_group`` (centertrack_amd/csrc/dcn_mfma.hip), the table of everything a launch branches on, the
list of cases the GPU tests run, float64 / float32 references of the whole operation (offset/mask conv + sigmoid where the
kernel owns them, DCNv2, scale / shift / ReLU, the IDAUp step) and the mutations of the float64 one.  No GPU, no ctypes.

What pins the restatement: ``ct_dcn_v2_workspace_bytes`` / ``ct_dcn_v2_group_workspace_bytes`` equal ``dcn_plan(...)['bytes']``,
``ct_dcn_v2_group_plan`` returns ``splits`` and ``ct_dcn_v2_offsets_bytes`` equals ``offsets_bytes`` (tests/test_dcn_forward_cpu.py).
BM, NKK, the XCD fields (xsx, pband, xper), the grid and the persistent partition are NOT observable through the ABI: BN is pinned
only where it changes the automatic split's tile count, the rest is mirrored by reading.

``autotune.tune_dcn`` and ``autotune._dcn_candidates`` have no caller in the tree (the model tunes whole schedules,
model.py::_tune_dcn_schedule); their candidate set (algo 0 / 64 / 128 / 3264 / 32128 x split_k 1 / 2 / 4 / 8 / 16) is still covered
here because ``ops.dcn_v2(algo=, split_k=)`` is public.

A regime is a hashable key; a case reaches the keys of ``case_keys`` / ``group_keys``.  Every case reaches at least one key that
no other case reaches."""
import zlib
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from _conv_fwd import winograd32
from _dcn_bwd import bound, cdiv, designed_positions, effective_offsets, err, randn, tap_bases  # noqa: F401

# ct_set_tuning values the DCN host code reads, with the defaults of api.cpp (g_tune)
KNOBS = OrderedDict([('dcn_bn', 0), ('dcn_slots', 1024), ('dcn_xcd', 1)])
ALGOS = (0, 64, 128, 3264, 32128, 43264, 432128, 53264, 532128, 63264, 632128)
FUSE_OFFSET = {'map': 0, 'slice': 0, 'fused': 1, 'parts': 2, 'wino': 2, 'raw': 3}
# the dcn_mfma_kernel<BM, WN, FUSE, NKK> and dcn_persist_kernel<WN, NKK> instantiations launch_group can pick
TILE_KERNELS = [(32, 1, False, 2), (32, 2, False, 2), (32, 1, True, 2), (32, 2, True, 2), (64, 2, False, 2), (64, 4, False, 2),
                (32, 1, False, 4), (32, 2, False, 4), (32, 1, True, 4), (32, 2, True, 4)]
PERSIST_KERNELS = [(1, 2), (2, 2), (1, 4), (2, 4)]


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan, restated

def offsets_bytes(N, H, W, Cin, fuse_offset):
    """ct_dcn_v2_offsets_bytes"""
    if fuse_offset not in (2, 3) or Cin % 64 or Cin <= 0 or N <= 0 or H <= 0 or W <= 0:
        return 0
    return (1 if fuse_offset == 3 else Cin // 64) * N * H * W * 32 * 4


def dcn_plan(N, H, W, Cin, Cout, algo=0, split_k=0, fuse_offset=0, grouped=False, has_workspace=True, up=False, knobs=()):
    """make_plan + ws_bytes + the XCD fields of fill_args + the grid of a MAIN launch of this layer alone.  ``origin``: where
    ``splits`` came from -- 'off', 'explicit-even', 'explicit-uneven' (the last split is shorter), 'clipped' (split_k > nunits),
    'auto-free' / 'auto-16' (the automatic split without / with its cap), 'grouped-default' (nchunks / 2)."""
    k = dict(KNOBS)
    k.update(dict(knobs))
    if algo not in ALGOS:
        raise ValueError('unknown algo %d' % algo)
    if Cin % 32 or Cin <= 0 or (fuse_offset and Cin % 64):
        raise ValueError('Cin=%d' % Cin)
    fuse = fuse_offset == 1
    parts = Cin // 64 if fuse_offset == 2 else (1 if fuse_offset == 3 else 0)
    NT, tilesX = cdiv(Cout, 16), cdiv(W, 16)
    BM, BN, NKK, persist, a = 64, 64, 2, False, algo
    if a in (53264, 532128, 63264, 632128):
        if fuse:
            raise ValueError('the persistent shapes read their offsets from a map')
        persist, a = True, {53264: 3264, 532128: 32128, 63264: 43264, 632128: 432128}[a]
    if a in (43264, 432128):
        NKK, a = 4, (3264 if a == 43264 else 32128)
    if grouped:
        if a not in (0, 3264, 32128) and not (a in (64, 128) and not fuse):
            raise ValueError('algo %d in a group' % algo)
        if a == 0:
            a = 3264
    if a == 3264:
        BM, BN = 32, 64
    elif a == 32128:
        BM, BN = 32, 128
    elif a == 128:
        BN = 128
    elif a == 64:
        BN = 64
    elif k['dcn_bn'] == 128 and Cout >= 128:
        BN = 128
    elif k['dcn_bn'] == 64:
        BN = 64
    elif Cout >= 128 and N * tilesX * cdiv(H, 4) * cdiv(Cout, 128) >= 512:
        BN = 128
    if fuse:
        if a in (64, 128):
            raise ValueError('fuse_offset runs on the 32-pixel tiles')
        if BM != 32:
            BM, BN = 32, 64
    if NKK == 4 and Cin % 64:
        raise ValueError('the 64-channel-step shapes need Cin % 64 == 0')
    rows = BM // 16
    tilesY, coutBlocks, nchunks = cdiv(H, rows), cdiv(Cout, BN), Cin // 32
    ptiles = N * tilesX * tilesY
    tiles = ptiles * coutBlocks
    splits, origin = split_k, 'explicit'
    if splits <= 0:
        splits, origin = 1, 'off'
        if grouped:
            splits, origin = nchunks // 2, 'grouped-default'
        elif has_workspace and tiles < 256:
            splits, origin = cdiv(512, tiles), 'auto-free'
            if splits > 16:
                splits, origin = 16, 'auto-16'
    upc = NKK // 2
    nunits = nchunks // upc
    if splits > nunits:
        splits, origin = nunits, 'clipped'
    splits = max(splits, 1)
    cps = cdiv(nunits, splits) * upc
    splits = cdiv(nchunks, cps)
    if splits == 1:
        origin = 'off'
    elif origin == 'explicit':
        origin = 'explicit-uneven' if nchunks % cps else 'explicit-even'
    use_ws = splits > 1 or (grouped and up)
    ups = cps // upc
    if persist and (BM != 32 or ups % 2 or nunits % ups):
        raise ValueError('persistent shape needs an even number of units per split')
    # steps of (chunk, tap) each split's workgroups run: the last split may be shorter
    steps = sorted(set((min(nunits, (s + 1) * ups) - s * ups) * 9 for s in range(splits)))
    p = dict(family='persist' if persist else 'tile', BM=BM, BN=BN, WN=BN * BM // 2048, NKK=NKK, fuse=fuse, parts=parts, NT=NT,
             tilesX=tilesX, tilesY=tilesY, rows=rows, coutBlocks=coutBlocks, nchunks=nchunks, nunits=nunits, chunksPerSplit=cps,
             unitsPerSplit=ups, splits=splits, origin=origin, use_ws=use_ws, ptiles=ptiles, tiles=tiles, steps=steps,
             bytes=splits * N * H * W * NT * 16 * 4 if use_ws else 0, Cout=Cout, Cin=Cin, N=N, H=H, W=W)
    # fill_args: the XCD-aware order (the persistent kernel does not read it)
    xsx = pband = xper = 0
    if k['dcn_xcd']:
        xsx = 1
        while xsx < 8 and splits % (2 * xsx) == 0:
            xsx *= 2
        pband = cdiv(ptiles, 8 // xsx)
        xper = coutBlocks * (splits // xsx) * pband
    p.update(xsx=xsx, pband=pband, xper=xper, grid=8 * xper if xsx else tiles * splits,
             padded=bool(xsx) and (8 // xsx) * pband > ptiles)
    return p


def xcd_decode(p, bid):
    """the XCD branch of dcn_mfma_kernel's id decode: layer-relative workgroup id -> (split, cout block, pixel tile) or None for
    an id of the padding"""
    xcd, j = bid & 7, bid >> 3
    cb, j = j % p['coutBlocks'], j // p['coutBlocks']
    sper = p['splits'] // p['xsx']
    sh, j = j % sper, j // sper
    split = (xcd & (p['xsx'] - 1)) + p['xsx'] * sh
    tile = (xcd // p['xsx']) * p['pband'] + j
    if j >= p['pband'] or tile >= p['ptiles']:
        return None
    return split, cb, tile


def live_ids(p):
    """layer-relative ids of the workgroups of a per-tile MAIN launch that do not exit at once"""
    if not p['xsx']:
        return list(range(p['grid']))
    return [b for b in range(p['grid']) if xcd_decode(p, b) is not None]


def rots(p, first=0):
    """values of ``rot = (blockIdx.x >> 8) & 3`` among the live workgroups of a layer whose ids start at ``first``"""
    return sorted(set(((first + b) >> 8) & 3 for b in live_ids(p)))


def persist_partition(plans, slots):
    """launch_group's partition of ``slots`` resident workgroups over the (cout block, K split) columns of the layers: the
    smallest makespan T with sum_i cols[i] * ceil(P[i] / floor(T / cost[i])) <= slots, by bisection -> (per_col, grid)"""
    cols = [p['coutBlocks'] * p['splits'] for p in plans]
    P = [p['ptiles'] for p in plans]
    cost = [p['unitsPerSplit'] * 9 + 3 for p in plans]
    lo, hi = max(cost), sum(c * n for c, n in zip(cost, P))
    slots = max(slots, sum(cols))

    def need(T):
        return sum(c * cdiv(n, T // k) for c, n, k in zip(cols, P, cost))
    while lo < hi:
        mid = (lo + hi) // 2
        if need(mid) <= slots:
            hi = mid
        else:
            lo = mid + 1
    per_col = [cdiv(n, lo // k) for n, k in zip(P, cost)]
    return per_col, sum(c * q for c, q in zip(cols, per_col))


def slot_counts(p):
    """name -> ``dcn_slots`` value: the slot counts a persistent launch of plan ``p`` is run at -- one workgroup per (cout block, K split)
    column, a small odd count above that, and the default"""
    cols = p['coutBlocks'] * p['splits']
    return OrderedDict([('columns', cols), ('small', 3 * cols + (2 if cols % 2 else 1)), ('default', KNOBS['dcn_slots'])])


def offsets_plan(p, wino):
    """the CT_DCN_OFFSETS launch of a fuse_offset == 2 layer: packed = dcn_mfma_kernel<32, 1, true> with offsOnly (one workgroup
    per 32-pixel tile and 64-channel chunk), Winograd = ct_wino_offsets_group"""
    return dict(family='offsets', form='wino' if wino else 'packed', grid=None if wino else p['N'] * p['tilesX'] * cdiv(p['H'], 2) * p['parts'])


def finish_plan(p, up_f):
    """the CT_DCN_FINISH launch of a layer that went through the workspace: dcn_reduce_kernel"""
    if up_f:
        rowBlocks, rows = (p['W'] * up_f * (p['Cout'] // 4) + 255) // 256, p['N'] * p['H'] * up_f
    else:
        rowBlocks, rows = (p['W'] * (p['NT'] * 4) + 255) // 256, p['N'] * p['H']
    return dict(family='finish', up_f=up_f, rowBlocks=rowBlocks, grid=rows * rowBlocks)


# ---------------------------------------------------------------------------------------------------------------------
# cases

# src: where the offsets come from -- 'map' (an [N,H,W,ldom] map), 'slice' (27 channels of a wider buffer), 'fused', 'parts' (the
# packed OFFSETS launch), 'wino' (its Winograd form), 'raw' (sums of another launch); entry: 'single' = ct_dcn_v2, 'group' = ct_dcn_v2_group
Case = namedtuple('Case', 'name N H W Cin Cout algo split_k src ldom up_f entry knobs why')
Group = namedtuple('Group', 'name layers mode knobs why')          # mode: 'one call' / 'three calls' / 'finish regrouped'


def mk(name, N, H, W, Cin, Cout, algo, split_k=1, src='map', ldom=32, up_f=0, entry='single', knobs=(), why=''):
    return Case(name, N, H, W, Cin, Cout, algo, split_k, src, ldom, up_f, entry, tuple(knobs), why)


def plan_of(case, extra_knobs=(), **kw):
    args = dict(algo=case.algo, split_k=case.split_k, fuse_offset=FUSE_OFFSET[case.src], grouped=case.entry == 'group',
                up=case.up_f > 0, knobs=tuple(case.knobs) + tuple(extra_knobs))
    args.update(kw)
    return dcn_plan(case.N, case.H, case.W, case.Cin, case.Cout, **args)


def tile_algo(case):
    """the per-tile algo of a persistent case (same tiles, same K order, same splits)"""
    return {53264: 3264, 532128: 32128, 63264: 43264, 632128: 432128}.get(case.algo, case.algo)


_PERSIST_ALGO = {(64, 2): 53264, (128, 2): 532128, (64, 4): 63264, (128, 4): 632128}


def persistent_form(case):
    """the case with the persistent algo of its own tile shape (same tiles, same K order, same splits), or None where make_plan
    refuses that: 64-pixel tiles, a fused offset conv, an odd or uneven number of step units per split"""
    p = plan_of(case)
    if p['family'] == 'persist':
        return case
    if p['BM'] != 32:
        return None
    try:
        q = plan_of(case, algo=_PERSIST_ALGO[(p['BN'], p['NKK'])])
    except ValueError:
        return None
    assert (q['BN'], q['NKK'], q['splits'], q['chunksPerSplit']) == (p['BN'], p['NKK'], p['splits'], p['chunksPerSplit'])
    return case._replace(algo=_PERSIST_ALGO[(p['BN'], p['NKK'])])


def y_written(case):
    """a layer whose IDAUp step runs in the finishing launch produces up_y only"""
    return not (case.up_f and plan_of(case)['use_ws'])


def standard(case, p):
    """the treatment every kernel instantiation gets: two images, two tiles each way with ragged last ones, Cin 128 in one split,
    Cout = BN + 27 (a partial last cout block, Cout % 16 = 11, n-tiles past NT), default knobs"""
    return (case.N == 2 and p['tilesX'] == 2 and case.W % 16 and p['tilesY'] > 1 and case.H % p['rows'] and case.Cin == 128
            and p['splits'] == 1 and case.Cout == p['BN'] + 27 and not case.knobs and not case.up_f)


def om_keys(case, p):
    """the persistent kernel fetches offsets and masks through code of its own (one descriptor for the batch)"""
    keys = set()
    if p['family'] == 'persist':
        return {('persist-om', 'map' if p['parts'] == 0 else ('one partial map' if p['parts'] == 1 else 'several partial maps'))}
    if case.src == 'map':
        keys.add(('om', 'map', case.ldom))
    elif case.src == 'slice':
        keys.add(('om', 'slice of a wider buffer'))
    elif case.src == 'fused':
        keys.add(('om', 'fused', 'Cin == 64' if case.Cin == 64 else 'Cin > 64'))
    elif case.src == 'parts':
        keys |= {('om', 'parts', p['parts']), ('offsets', 'packed')}
    elif case.src == 'wino':
        keys |= {('om', 'wino'), ('offsets', 'wino')}
    else:
        keys.add(('om', 'raw'))
    return keys


def layer_keys(case, first=0):
    """the regimes one layer reaches whatever launch it is part of"""
    p = plan_of(case)
    keys = om_keys(case, p)
    if p['family'] == 'persist':
        if standard(case, p):
            keys.add(('persist', p['WN'], p['NKK']))
        keys |= {('dcn_slots', v) for v in slot_counts(p)}                  # (test_hip_dcn_forward.py runs a persistent launch at each of these)
    else:
        if standard(case, p):
            keys.add(('kernel', p['BM'], p['WN'], p['fuse'], p['NKK']))
        for r in rots(p, first):
            keys.add(('rot', r))
        keys.add(('xcd', p['xsx'], 'padded ids' if p['padded'] else 'no padding') if p['xsx'] else ('xcd', 'off'))
    if p['use_ws']:
        keys.add(('reduce', case.up_f))
        if p['NT'] * 16 > case.Cout:
            keys.add(('reduce', 'wsCout > Cout'))
    elif case.up_f:
        keys.add(('legacy_up',))
    keys.add(('split-origin', p['origin']))
    if p['family'] == 'tile':
        for s in p['steps']:
            keys.add(('steps', 'odd: the peeled last step' if s % 2 else 'even'))
    if p['NKK'] == 4 and p['splits'] > 1 and p['unitsPerSplit'] >= 2:
        keys.add(('nkk4', 'a shorter last split' if p['nunits'] % p['unitsPerSplit'] else 'two or more units per split'))
    for name, v in (('W % 16 != 0', case.W % 16 and case.W > 16), ('W < 16', case.W < 16), ('H % rows != 0', case.H % p['rows'] and case.H > p['rows']),
                    ('H < rows', case.H < p['rows']), ('N > 1', case.N > 1)):
        if v:
            keys.add(('edge', name))
    for name, v in (('Cout % 16 != 0', case.Cout % 16), ('Cout % BN != 0', case.Cout % p['BN'] and case.Cout > p['BN']),
                    ('Cout < BN', case.Cout < p['BN'])):
        if v:
            keys.add(('cout', name))
    if case.Cin in (32, 96, 160, 192):
        keys.add(('cin', case.Cin))
    if dict(case.knobs).get('dcn_bn') and case.algo == 0 and case.entry == 'single':
        keys.add(('dcn_bn', dict(case.knobs)['dcn_bn']))
    return keys


def case_keys(case):
    return layer_keys(case)


def group_firsts(layers):
    """first workgroup id of every layer of a MAIN launch"""
    firsts, b = [], 0
    for c in layers:
        firsts.append(b)
        b += plan_of(c)['grid']
    return firsts


def group_keys(g):
    # (the regimes of its layers are credited to the single-layer cases: a group is there for what only a group can reach)
    keys = set()
    plans = [plan_of(c) for c in g.layers]
    for c, first in zip(g.layers, group_firsts(g.layers)):
        keys |= set(k for k in layer_keys(c, first) if k[0] == 'rot')
    keys.add(('group', 'layers', len(g.layers)))
    keys.add(('group', 'phases', 'in one call' if g.mode == 'one call' else 'in three calls'))
    if g.mode == 'finish regrouped':
        keys.add(('group', 'a FINISH call on another set of layers than the MAIN call'))
    if any(c.up_f and p['splits'] == 1 for c, p in zip(g.layers, plans)):
        keys.add(('group', 'an up layer with splits == 1'))
    if any(p['fuse'] for p in plans) and not all(p['fuse'] for p in plans):
        keys.add(('om', 'a FUSE instantiation running a layer without w_off'))
    if len(set(p['steps'][-1] for p in plans)) > 1:
        keys.add(('group', 'layers of different step counts'))
    if plans[0]['family'] == 'persist' and len(plans) > 1:
        keys.add(('group', 'persistent, several layers'))
    return keys


def dcn_regimes():
    """key -> where in the sources the branch lives"""
    r = OrderedDict()
    for key in TILE_KERNELS:
        r[('kernel',) + key] = 'dcn_mfma.hip: launch_group, the `p0.NKK == 4` / `fuse_any` / `p0.BM == 32` / `p0.BN == 128` ladder'
    for key in PERSIST_KERNELS:
        r[('persist',) + key] = 'dcn_mfma.hip: launch_group `else if (p0.persist)` -> dcn_persist_kernel<WN, NKK>'
    r[('offsets', 'packed')] = 'dcn_mfma.hip: launch_group `if (phases & CT_DCN_OFFSETS)`; dcn_mfma_kernel `if (FUSE && a.offsOnly)`'
    r[('offsets', 'wino')] = 'dcn_mfma.hip: launch_group `if (d->w_off_winograd)` -> wino_mfma.hip: ct_wino_offsets_group'
    for f in (0, 2, 4, 8):
        r[('reduce', f)] = 'dcn_mfma.hip: dcn_reduce_kernel `if (r.u.f == 0)`, `lf = 31 - __builtin_clz(f)`'
    r[('reduce', 'wsCout > Cout')] = 'dcn_mfma.hip: dcn_reduce_kernel `if (co >= e.Cout) break`; dcn_store_acc `co < a.wsCout`'
    r[('legacy_up',)] = 'dcn_mfma.hip: launch_group `else if (d->up_w) legacy_up = d` -> ct_upsample_add'
    for ld in range(27, 33):
        r[('om', 'map', ld)] = 'dcn_mfma.hip: dcn_mfma_kernel `omn + ((size_t)oy * a.W + ox) * a.ldom`; dcn_persist_kernel `opitch`'
    r[('om', 'slice of a wider buffer')] = 'dcn_mfma.hip: the same with ldom > 32 and a start inside the buffer'
    r[('om', 'fused', 'Cin == 64')] = 'dcn_mfma.hip: lds_bytes `single_chunk`; dcn_mfma_kernel `if (fuse)` ksplit_conv_tile'
    r[('om', 'fused', 'Cin > 64')] = 'dcn_mfma.hip: launch_group `if (p.fuse && d->Cin != 64) single_chunk = false`'
    for n in (1, 2, 4, 8):
        r[('om', 'parts', n)] = 'dcn_mfma.hip: dcn_mfma_kernel `if (parts)`, `for (sp = 1; sp < a.omSplits; ++sp)`'
    r[('om', 'wino')] = 'wino_mfma.hip: ct_wino_offsets_group writes the partial maps'
    r[('om', 'raw')] = 'dcn_mfma.hip: make_plan `d->fuse_offset == 3 ? 1`; launch_group `if (d->fuse_offset != 2) continue`'
    r[('om', 'a FUSE instantiation running a layer without w_off')] = 'dcn_mfma.hip: dcn_mfma_kernel `fuse = FUSE && a.w_off != nullptr`'
    for k in ('map', 'one partial map', 'several partial maps'):
        r[('persist-om', k)] = 'dcn_mfma.hip: dcn_persist_kernel om_fetch / table_build through the `ors` descriptor'
    for o in ('off', 'explicit-even', 'explicit-uneven', 'clipped', 'auto-free', 'auto-16', 'grouped-default'):
        r[('split-origin', o)] = 'dcn_mfma.hip: make_plan, `int splits = d->split_k` .. `p->splits = ct_cdiv(p->nchunks, p->chunksPerSplit)`'
    r[('steps', 'odd: the peeled last step')] = 'dcn_mfma.hip: dcn_mfma_kernel `if (s < nmax) step(..)`'
    r[('steps', 'even')] = 'dcn_mfma.hip: dcn_mfma_kernel `for (; s + 1 < nmax; s += 2)`'
    r[('nkk4', 'a shorter last split')] = 'dcn_mfma.hip: dcn_mfma_kernel `c_end = min(nunits, c_begin + a.chunksPerSplit / UPC2)` at NKK 4'
    r[('nkk4', 'two or more units per split')] = 'dcn_mfma.hip: make_plan `upc`, `nunits`; dcn_mfma_kernel `c_begin`, `c_end`'
    for e in ('W % 16 != 0', 'W < 16', 'H % rows != 0', 'H < rows', 'N > 1'):
        r[('edge', e)] = 'dcn_mfma.hip: dcn_mfma_kernel `in = it < E && oy < a.H && ox < a.W`; dcn_store_acc `px0 + e < a.W`, `oyb + mt >= a.H`'
    for e in ('Cout % 16 != 0', 'Cout % BN != 0', 'Cout < BN'):
        r[('cout', e)] = 'dcn_mfma.hip: `bvo[nt] = min(nt0 + nt, a.NT - 1)`; dcn_store_acc `co < e.Cout`'
    for c in (32, 96, 160, 192):
        r[('cin', c)] = 'dcn_mfma.hip: make_plan `p->nchunks = d->Cin / 32`'
    for v in range(4):
        r[('rot', v)] = 'dcn_mfma.hip: dcn_mfma_kernel `rot = (blockIdx.x >> 8) & 3`'
    r[('xcd', 'off')] = 'dcn_mfma.hip: fill_args `if (ct_tune_get(CT_TUNE_DCN_XCD))`; dcn_mfma_kernel `if (a.xsx && ..) else`'
    for x in (1, 2, 4, 8):
        for pad in (('no padding', 'padded ids') if x < 8 else ('no padding',)):          # (xsx 8: one band per XCD, pband = ptiles)
            r[('xcd', x, pad)] = 'dcn_mfma.hip: fill_args `xsx`, `pband`, `xper`; dcn_mfma_kernel `if (j >= a.pband || tile >= a.ptiles) return`'
    for n in (1, 2, 3, 4):
        r[('group', 'layers', n)] = 'dcn_mfma.hip: launch_group `for (i = 0; i < n; ++i)`; the kernels `if (i < g.n && bid >= g.first[i]) pi = i`'
    for m in ('in one call', 'in three calls'):
        r[('group', 'phases', m)] = 'dcn_mfma.hip: launch_group `phases & CT_DCN_OFFSETS / MAIN / FINISH`'
    r[('group', 'a FINISH call on another set of layers than the MAIN call')] = 'dcn_schedule.py: plan, the FINISH names of a slot'
    r[('group', 'an up layer with splits == 1')] = 'dcn_mfma.hip: make_plan `p->use_ws = (p->splits > 1 || (grouped && d->up_w))`'
    r[('group', 'layers of different step counts')] = 'dcn_schedule.py: plan, MAIN names sorted by steps; dcn_mfma.hip: per-layer nsteps'
    r[('group', 'persistent, several layers')] = 'dcn_mfma.hip: launch_group, the bisection over `slots` and `per_col`'
    for v in (64, 128):
        r[('dcn_bn', v)] = 'dcn_mfma.hip: make_plan `ct_tune_get(CT_TUNE_DCN_BN)`'
    for v in ('columns', 'small', 'default'):
        r[('dcn_slots', v)] = 'dcn_mfma.hip: launch_group `slots = ct_tune_get(CT_TUNE_DCN_SLOTS)`, `if (slots < all) slots = all`'
    return r


DCN_REGIMES = dcn_regimes()

_PERSIST_OF = {3264: 53264, 32128: 532128, 43264: 63264, 432128: 632128}
_ALGO_OF = {(32, 1, 2): 3264, (32, 2, 2): 32128, (64, 2, 2): 64, (64, 4, 2): 128, (32, 1, 4): 43264, (32, 2, 4): 432128}


def _gpu_cases():
    L = []
    # ---- one case per kernel instantiation: N = 2, H = 2 rows + 1, W = 21, Cin 128 in one split, Cout = BN + 27
    for BM, WN, FUSE, NKK in TILE_KERNELS:
        BN = 16 * WN * 128 // BM
        L.append(mk('k_bm%d_wn%d_%s_nkk%d' % (BM, WN, 'fuse' if FUSE else 'map', NKK), 2, 2 * (BM // 16) + 1, 21, 128, BN + 27,
                    _ALGO_OF[(BM, WN, NKK)], src='fused' if FUSE else 'map', why='dcn_mfma_kernel<%d, %d, %s, %d>' % (BM, WN, str(FUSE).lower(), NKK)))
    for WN, NKK in PERSIST_KERNELS:
        L.append(mk('p_wn%d_nkk%d' % (WN, NKK), 2, 5, 21, 128, 64 * WN + 27, _PERSIST_OF[_ALGO_OF[(32, WN, NKK)]],
                    why='dcn_persist_kernel<%d, %d>: 12 pixel tiles per column, bitwise against the per-tile form at three slot counts' % (WN, NKK)))
    # ---- where the offsets come from
    L.append(mk('om_fused_cin64', 1, 5, 17, 64, 64, 3264, src='fused', why='fused offset conv with one 64-channel chunk: the single-buffer scratch'))
    L.append(mk('om_parts1', 1, 3, 17, 64, 64, 3264, src='parts', why='K-split offset conv with ONE partial map: the sum loop does not run'))
    L.append(mk('om_parts2', 2, 3, 17, 128, 48, 3264, src='parts', why='two partial maps'))
    L.append(mk('om_parts4', 1, 6, 7, 256, 64, 3264, split_k=2, src='parts', why='four partial maps, two K splits'))
    L.append(mk('om_parts8', 1, 5, 6, 512, 64, 3264, split_k=8, src='parts', why='eight partial maps at Cin 512, eight K splits: xsx 8'))
    L.append(mk('om_wino', 2, 7, 19, 128, 64, 3264, src='wino', why='the OFFSETS launch in its Winograd form, odd map'))
    L.append(mk('om_raw', 1, 5, 17, 128, 64, 3264, src='raw', why='raw sums written by a plain conv launch: bias and sigmoid in the table build'))
    L.append(mk('p_om_parts2', 1, 5, 17, 128, 64, 53264, src='parts', why='persistent form reading two partial maps through its descriptor'))
    L.append(mk('p_om_raw', 1, 5, 17, 64, 64, 53264, src='raw', why='persistent form reading one raw map'))
    # ---- offset/mask map pitches 27 .. 31 and a slice, each on a Cin / shape edge of its own
    L.append(mk('ldom27_cin32', 1, 3, 5, 32, 16, 0, src='map', ldom=27, why='ldom 27; Cin 32: one chunk, 9 steps; a 3 x 5 map inside one 64-pixel tile'))
    L.append(mk('ldom28_cin96', 1, 5, 18, 96, 40, 3264, split_k=2, ldom=28, why='ldom 28; Cin 96 in two splits of 2 + 1 chunks'))
    L.append(mk('ldom29_cin160', 2, 3, 9, 160, 64, 64, split_k=2, ldom=29, why='ldom 29; Cin 160 in two splits of 3 + 2 chunks on 64-pixel tiles'))
    L.append(mk('ldom30_cin192_nkk4', 1, 4, 20, 192, 64, 43264, split_k=2, ldom=30, why='ldom 30; Cin 192 at NKK 4: three units in splits of 2 + 1'))
    L.append(mk('ldom31_h1', 2, 1, 33, 64, 24, 3264, ldom=31, why='ldom 31; H 1 < 2 rows, three tile columns'))
    L.append(mk('om_slice', 2, 4, 12, 64, 16, 3264, src='slice', why='the map is 27 channels inside a 40-channel buffer'))
    # ---- where the split count comes from
    L.append(mk('split_clipped', 1, 4, 16, 64, 64, 3264, split_k=5, why='split_k 5 > 2 chunks: clipped, one chunk per split (9 steps)'))
    L.append(mk('split_auto_free', 3, 24, 24, 96, 320, 0, split_k=0, why='automatic split: 180 tiles -> cdiv(512, 180) = 3 = nchunks'))
    L.append(mk('split_auto_16', 1, 4, 4, 512, 64, 0, split_k=0, why='automatic split: one tile -> 512 capped at 16 = nchunks'))
    L.append(mk('split_group_default', 1, 5, 17, 128, 64, 0, split_k=0, entry='group', why='a group layer with split_k 0: nchunks / 2 splits, algo 0 -> 3264'))
    L.append(mk('nkk4_two_units', 1, 4, 16, 256, 128, 432128, split_k=2, why='NKK 4, four units in two splits'))
    # ---- the finishing launch
    for f, (H, W) in ((2, (3, 18)), (4, (3, 5)), (8, (2, 3))):
        L.append(mk('reduce_up%d' % f, 2, H, W, 64, 20, 3264, split_k=2, up_f=f,
                    why='dcn_reduce_kernel with the IDAUp step f = %d, Cout 20 of wsCout 32; bitwise against reduce + upsample_add' % f))
    L.append(mk('legacy_up', 2, 3, 18, 64, 20, 3264, up_f=2, why='a single unsplit launch with an IDAUp step: ct_upsample_add on the finished output'))
    # ---- rot 1, 2, 3: 1 024 workgroups from split-K and cout blocks; each image alone is 256 workgroups (rot 0)
    L.append(mk('rot', 4, 16, 32, 256, 128, 3264, split_k=8, why='1 024 workgroups: rot 0 .. 3; bitwise against the four images launched one by one'))
    # ---- the XCD-aware order: xsx = gcd(splits, 8), with and without padded ids
    L.append(mk('xcd4_nopad', 1, 4, 16, 128, 64, 3264, split_k=4, why='xsx 4, 2 pixel tiles: no padding'))
    L.append(mk('xcd4_pad', 1, 6, 16, 128, 64, 3264, split_k=4, why='xsx 4, 3 pixel tiles in bands of 2: padded ids'))
    L.append(mk('xcd_off', 2, 5, 21, 128, 64, 3264, split_k=2, knobs=(('dcn_xcd', 0),), why='dcn_xcd 0: the plain id decode'))
    # ---- dcn_bn
    L.append(mk('bn128', 1, 7, 17, 64, 160, 0, knobs=(('dcn_bn', 128),), why='dcn_bn 128 with Cout >= 128: 64 px x 128 couts by the knob'))
    L.append(mk('bn64', 1, 7, 17, 64, 160, 0, knobs=(('dcn_bn', 64),), why='dcn_bn 64'))
    return L


def _groups():
    G = []
    G.append(Group('g1_up_unsplit', [mk('g1a', 2, 3, 18, 64, 20, 3264, src='fused', up_f=2, entry='group')], 'one call', (),
                   'one layer: an IDAUp step with splits == 1 is forced through the workspace; y stays untouched'))
    G.append(Group('g2_mixed_fuse', [mk('g2a', 1, 5, 17, 64, 64, 3264, src='fused', entry='group'),
                                     mk('g2b', 2, 3, 9, 128, 40, 3264, split_k=2, src='map', ldom=29, entry='group')], 'one call', (),
                   'a fused and an un-fused layer in one FUSE = true launch'))
    G.append(Group('g3_three_calls', [mk('g3a', 1, 6, 10, 128, 64, 43264, split_k=2, src='map', up_f=2, entry='group'),
                                      mk('g3b', 2, 5, 17, 256, 128, 43264, split_k=4, src='wino', entry='group'),
                                      mk('g3c', 1, 4, 20, 128, 64, 43264, split_k=1, src='parts', entry='group')], 'three calls', (),
                   'NKK 4, the three phases in three calls, Winograd and packed OFFSETS in one call'))
    G.append(Group('g4_regrouped', [mk('g4a', 1, 4, 6, 512, 64, 3264, split_k=4, src='parts', entry='group'),
                                    mk('g4b', 1, 6, 10, 128, 64, 3264, split_k=2, src='slice', up_f=2, entry='group'),
                                    mk('g4c', 2, 5, 17, 256, 128, 3264, split_k=4, src='map', entry='group'),
                                    mk('g4d', 1, 7, 18, 64, 64, 3264, split_k=2, src='raw', up_f=4, entry='group')], 'finish regrouped', (),
                   'four layers sorted by step count (36, 18, 18, 9); FINISH in two calls on other sets than MAIN'))
    G.append(Group('g5_persist', [mk('g5a', 2, 9, 21, 128, 64, 53264, split_k=1, src='map', up_f=2, entry='group'),
                                  mk('g5b', 3, 5, 17, 256, 128, 53264, split_k=2, src='wino', entry='group')], 'one call', (),
                   'two layers of different cost in one persistent launch'))
    return G


GPU_CASES = _gpu_cases()
GROUPS = _groups()
CASE = OrderedDict((c.name, c) for c in GPU_CASES)
GROUP = OrderedDict((g.name, g) for g in GROUPS)
assert len(CASE) == len(GPU_CASES) and len(GROUP) == len(GROUPS)


def all_keys(cases, groups):
    got = set()
    for c in cases:
        got |= case_keys(c)
    for g in groups:
        got |= group_keys(g)
    return got


def missing_regimes(cases, groups):
    got = all_keys(cases, groups)
    return [k for k in DCN_REGIMES if k not in got]


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references

_input_cache, _ref_cache = {}, {}
OWN = ('fused', 'parts', 'wino', 'raw')
W_OFF_SCALE, B_OFF_SCALE = 0.02, 0.2


def seed_of(case):
    return zlib.crc32(case.name.encode()) % 100000


def designed(case):
    """every other map case samples at the designed border / half-cell / integer positions, the rest at random offsets"""
    return case.src in ('map', 'slice') and seed_of(case) % 2 == 0


def dcn_inputs(case):
    """fp32 tensors of a case (NCHW), once per process"""
    if case.name not in _input_cache:
        s, N, H, W, Cin, Cout = seed_of(case), case.N, case.H, case.W, case.Cin, case.Cout
        x = randn(s, N, Cin, H, W)
        if s % 3 == 0:
            x = torch.relu(x)                                        # a post-ReLU map, the production input
        d = dict(x=x.float(), w=(randn(s + 1, Cout, Cin, 3, 3) * (9 * Cin) ** -0.5).float(), shift=randn(s + 3, Cout).float(),
                 scale=(torch.rand(Cout, generator=torch.Generator().manual_seed(s + 2), dtype=torch.float64) + 0.5).float())
        if case.src in OWN:
            d['wo'], d['bo'] = (randn(s + 4, 27, Cin, 3, 3) * W_OFF_SCALE).float(), (randn(s + 5, 27) * B_OFF_SCALE).float()
        else:
            if designed(case):
                pos, _ = designed_positions(N, H, W)
                d['off'] = (pos - tap_bases(H, W).unsqueeze(0)).float()            # (multiples of 0.25: exact)
            else:
                d['off'] = (randn(s + 4, N, 18, H, W) * (0.5, 1.0, 2.0, 3.0)[s % 4]).float()
            d['mask'] = torch.sigmoid(randn(s + 5, N, 9, H, W)).float()
        if case.up_f:
            f = case.up_f
            d['wup'], d['skip'] = (randn(s + 6, Cout, 1, 2 * f, 2 * f) * 0.5).float(), randn(s + 7, N, Cout, H * f, W * f).float()
        _input_cache[case.name] = d
    return _input_cache[case.name]


def offsets_and_mask(case, dt):
    """(offset [N,18,H,W], mask [N,9,H,W]) in ``dt``: the kernel's own offset conv restated (Winograd arithmetic for the Winograd
    launch in float32), or the given map -- in float64 at exactly the kernel's fp32 sample coordinates"""
    d = dcn_inputs(case)
    if case.src in OWN:
        x, wo = d['x'].to(dt), d['wo'].to(dt)
        om = winograd32(x, wo) if (case.src == 'wino' and dt == torch.float32) else F.conv2d(x, wo, None, 1, 1)
        om = om + d['bo'].to(dt).view(1, -1, 1, 1)
        return om[:, :18], torch.sigmoid(om[:, 18:])
    off = effective_offsets(d['off'], case.H, case.W) if dt == torch.float64 else d['off']
    return off, d['mask'].to(dt)


def sample_cols(x, offset, mask, swap_border=False):
    """[B, Ci, 9, H*W]: the masked bilinear samples of DCNv2 (oracle/dcn_v2.py's rules: strict at -1 and H, corners outside the
    map contribute nothing).  ``swap_border``: the row and column fractions exchanged for the samples in the first or last cell"""
    B, Ci, H, W = x.shape
    dt = x.dtype
    ho, wo = torch.arange(H, dtype=dt).view(1, H, 1), torch.arange(W, dtype=dt).view(1, 1, W)
    xf = x.reshape(B, Ci, H * W)
    cols = []
    for k in range(9):
        ys, xs = ho - 1 + k // 3 + offset[:, 2 * k], wo - 1 + k % 3 + offset[:, 2 * k + 1]
        inside = (ys > -1) & (xs > -1) & (ys < H) & (xs < W)
        y0, x0 = torch.floor(ys), torch.floor(xs)
        ly, lx = ys - y0, xs - x0
        if swap_border:
            edge = inside & ((y0 < 0) | (y0 >= H - 1) | (x0 < 0) | (x0 >= W - 1))
            ly, lx = torch.where(edge, lx, ly), torch.where(edge, ly, lx)
        y0, x0 = y0.long(), x0.long()
        val = 0
        for yy, xx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1) & inside
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, H * W)
            val = val + torch.gather(xf, 2, idx.expand(B, Ci, H * W)) * (wgt * ok.to(dt)).view(B, 1, H * W)
        cols.append(val * mask[:, k].reshape(B, 1, H * W))
    return torch.stack(cols, dim=2)


def finish(case, z, dt):
    """scale, shift, ReLU, and the depth-wise transposed conv onto ``skip`` -> dict(y[, up])"""
    d = dcn_inputs(case)
    y = torch.relu(z * d['scale'].to(dt).view(1, -1, 1, 1) + d['shift'].to(dt).view(1, -1, 1, 1))
    out = dict(y=y)
    if case.up_f:
        f = case.up_f
        out['up'] = F.conv_transpose2d(y, d['wup'].to(dt), None, f, f // 2, groups=case.Cout) + d['skip'].to(dt)
    return out


def _reference(case, dt):
    from oracle import dcn_v2 as odcn
    d = dcn_inputs(case)
    off, mask = offsets_and_mask(case, dt)
    return finish(case, odcn.dcn_v2_conv(d['x'].to(dt), off, mask, d['w'].to(dt), None), dt)


def reference64(case):
    if case.name not in _ref_cache:
        _ref_cache[case.name] = _reference(case, torch.float64)
    return _ref_cache[case.name]


def reference32(case):
    return _reference(case, torch.float32)


def terms(case):
    """K of the project's bound: 9 Cin products per output, four more with an IDAUp step"""
    return 9 * case.Cin + (4 if case.up_f else 0)


def outputs_of(case):
    return (['y'] if y_written(case) else []) + (['up'] if case.up_f else [])


_e32_cache = {}


def case_errors(case, got, which):
    """(err, e32, bound) of an output (NCHW) by the project's measure; e32 from the float32 reference, never from the kernel"""
    r64 = reference64(case)[which]
    if (case.name, which) not in _e32_cache:
        _e32_cache[(case.name, which)] = err(reference32(case)[which], r64)
    e32 = _e32_cache[(case.name, which)]
    return err(got.detach().cpu().double(), r64), e32, bound(e32, terms(case))


def mutants64(case):
    """{name: outputs} of three faulty float64 computations on the case's inputs: one (32-channel chunk, tap) term dropped for one
    32-pixel tile; one split's partial omitted for one 16-cout tile; the fractions exchanged in the first and last cell"""
    d, s, p = dcn_inputs(case), seed_of(case), plan_of(case)
    N, H, W, Cin, Cout = case.N, case.H, case.W, case.Cin, case.Cout
    x, w = d['x'].double(), d['w'].double().reshape(Cout, Cin, 9)
    off, mask = offsets_and_mask(case, torch.float64)
    cols = sample_cols(x, off, mask)

    def contract(c, ww=w):
        return torch.einsum('ock,bckp->bop', ww, c).view(N, -1, H, W)
    out = {}
    # (the tile, chunk and tap follow the case's seed; a dropped term that is zero everywhere -- all 32 samples outside -- moves on)
    tY, tX = cdiv(H, 2), cdiv(W, 16)
    for t in range(N * tY * tX * (Cin // 32) * 9):
        u = (s + t * 7) % (N * tY * tX * (Cin // 32) * 9)
        tap, u = u % 9, u // 9
        ch, u = u % (Cin // 32), u // (Cin // 32)
        tx, u = u % tX, u // tX
        ty, n = u % tY, u // tY
        sel = torch.zeros(H, W, dtype=torch.bool)
        sel[2 * ty:2 * ty + 2, 16 * tx:16 * tx + 16] = True
        part = cols[n, 32 * ch:32 * ch + 32, tap][:, sel.view(-1)]
        if float(part.abs().max()) > 0.1:
            c = cols.clone()
            c[n, 32 * ch:32 * ch + 32, tap] = c[n, 32 * ch:32 * ch + 32, tap] * (~sel).view(1, -1).double()
            out['a (chunk, tap) term dropped for one tile'] = finish(case, contract(c), torch.float64)
            break
    sp, nt = s % p['splits'], s % p['NT']
    c0, c1 = 32 * sp * p['chunksPerSplit'], min(Cin, 32 * (sp + 1) * p['chunksPerSplit'])
    z = contract(cols)
    z[:, 16 * nt:16 * nt + 16] -= contract(cols[:, c0:c1], w[16 * nt:16 * nt + 16, c0:c1])
    out['a split\'s partial omitted for one cout tile'] = finish(case, z, torch.float64)
    out['fractions exchanged in the first and last cell'] = finish(case, contract(sample_cols(x, off, mask, swap_border=True)), torch.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the production schedule, restated (model.py: the IDAUp tree of _build_plan; dcn_schedule.py: slot_sizes, plan).  It imports nothing
# of the package: tests/test_dcn_forward_cpu.py holds dcn_schedule.plan against it

CHANNELS = [16, 32, 64, 128, 256, 512]
SMALL_SLOT_WGS = 600
NeckLayer = namedtuple('NeckLayer', 'name x Cin H W cout out up')           # x / out: buffer ids; up = (f, skip buffer, output buffer) or None


def neck_layers(H, W):
    """the 16 DeformConv nodes of DLAUp + IDAUp in the reference's order; buffers 0 .. 5 are the backbone levels"""
    shape = dict((i, (CHANNELS[i], H >> i, W >> i)) for i in range(6))
    out = []

    def new(C, h, w):
        shape[len(shape)] = (C, h, w)
        return len(shape) - 1

    def deform(name, x, cout, up=None):
        C, h, w = shape[x]
        o = new(cout, h, w)
        out.append(NeckLayer(name, x, C, h, w, cout, o, up))
        return o

    def ida(p, layers, startp, endp, o, up_f):
        for i in range(startp + 1, endp):
            k = i - startp
            f, xi = up_f[k], layers[i]
            _, h, w = shape[xi]
            up = new(o, h * f, w * f)
            deform('%s.proj_%d' % (p, k), xi, o, up=(f, layers[i - 1], up))
            layers[i] = deform('%s.node_%d' % (p, k), up, o)
    layers = list(range(6))
    outs = [layers[-1]]
    for j, (startp, o, up_f) in enumerate(((4, 256, [1, 2]), (3, 128, [1, 2, 2]), (2, 64, [1, 2, 2, 2]))):
        ida('dla_up.ida_%d' % j, layers, startp, 6, o, up_f)
        outs.insert(0, layers[-1])
    ida('ida_up', [outs[0], outs[1], outs[2]], 0, 3, 64, [1, 2, 4])
    return out


def _slot_sizes(layers, N, cps):
    time_of, sizes, mains = {}, {}, []
    for ly in layers:
        main = time_of.get(ly.x, 0) // 2 + 1
        mains.append(main)
        splits = max(1, (ly.Cin // 32) // cps)
        if splits > 1 or ly.up is not None:
            fin = max(main, (time_of.get(ly.up[1], 0) + 1) // 2) if ly.up is not None else main
            done = 2 * fin + 1
        else:
            done = 2 * main
        time_of[ly.up[2] if ly.up is not None else ly.out] = done
        sizes[main] = sizes.get(main, 0) + N * cdiv(ly.H, 2) * cdiv(ly.W, 16) * cdiv(ly.cout, 64) * splits
    return sizes, mains


def neck_schedule(knobs, N, H, W, fuse_enabled=True):
    """what dcn_schedule.plan gives each neck layer for a knob tuple, and its group launches in order:
    [(tag, [layer names], phases, [(algo, split_k, fuse_offset)])], plus {name: dict(algo, split_k, fuse_offset, up_f, src, layer)}"""
    knobs = tuple(knobs) + (1, 0, 0, 0)[len(knobs) - 3:] if len(knobs) < 7 else tuple(knobs)
    fuse_max, cps, nkk, split_offsets, cps_small, small_unfuse, persist = knobs[:7]
    layers = neck_layers(H, W)
    sizes, mains = _slot_sizes(layers, N, cps)
    slot_cps = {}
    if cps_small and cps_small < cps:
        slot_cps = dict((t, cps_small) for t, wgs in sizes.items() if wgs < SMALL_SLOT_WGS)
    unfuse_slots = set()
    if small_unfuse == 2:
        unfuse_slots = set(m for ly, m in zip(layers, mains) if not (ly.Cin % 64 == 0 and ly.Cin <= fuse_max and fuse_enabled))
    time_of, slots, offs, info = {}, {}, {}, OrderedDict()
    for ly in layers:
        main = time_of.get(ly.x, 0) // 2 + 1
        c = slot_cps.get(main, cps)
        fused = (ly.Cin % 64 == 0 and ly.Cin <= fuse_max and fuse_enabled and not (small_unfuse and main in slot_cps)
                 and main not in unfuse_slots)
        lnkk = 2 if (c == 1 or ly.Cin % 64) else nkk
        splits = max(1, (ly.Cin // 32) // c)
        if fused:
            src = 'fused'
        elif split_offsets == 2 and ly.Cin % 64 == 0:
            src = 'raw'
        elif split_offsets and ly.Cin % 64 == 0:
            src = 'wino' if split_offsets == 3 else 'parts'
            offs.setdefault(main, []).append(ly.name)
        else:
            src = 'map'
        up_f = ly.up[0] if ly.up is not None else 0
        use_ws = dcn_plan(N, ly.H, ly.W, ly.Cin, ly.cout, 3264, splits, FUSE_OFFSET[src], True, True, up_f > 0)['bytes'] > 0
        if use_ws:
            finish = max(main, (time_of.get(ly.up[1], 0) + 1) // 2) if ly.up is not None else main
            done = 2 * finish + 1
        else:
            finish, done = None, 2 * main
        time_of[ly.up[2] if ly.up is not None else ly.out] = done
        info[ly.name] = dict(layer=ly, nkk=lnkk, split_k=splits, fuse_offset=FUSE_OFFSET[src], src=src, up_f=up_f, fused=fused, main=main, finish=finish)
        slots.setdefault(main, {'main': [], 'finish': []})['main'].append(ly.name)
        if finish is not None:
            slots.setdefault(finish, {'main': [], 'finish': []})['finish'].append(ly.name)
    launches = []

    def group(names, phases, tag):
        if phases == 1:
            names = sorted(names, key=lambda n: -cdiv(info[n]['layer'].Cin // 32, info[n]['split_k']))
        for i in range(0, len(names), 4):
            part = names[i:i + 4]

            def can_persist(n):
                cpsplit = cdiv(info[n]['layer'].Cin // 32, info[n]['split_k'])
                return not info[n]['fused'] and (info[n]['layer'].Cin // 32) % cpsplit == 0 and cpsplit % (4 if info[n]['nkk'] == 4 else 2) == 0
            pers = bool(persist) and phases == 1 and all(can_persist(n) for n in part)
            algos = [(43264 if info[n]['nkk'] == 4 else 3264) + (20000 if pers and info[n]['nkk'] == 4 else 50000 if pers else 0) for n in part]
            launches.append((tag, part, phases, [(a, info[n]['split_k'], info[n]['fuse_offset']) for a, n in zip(algos, part)]))
    for t in sorted(slots):
        if offs.get(t):
            group(offs[t], 4, 'dcn.offsets')
        if slots[t]['main']:
            group(slots[t]['main'], 1, 'dcn')
        if slots[t]['finish']:
            group(slots[t]['finish'], 2, 'dcn.finish')
    return launches, info


def schedule_signature(launches):
    """the ``dcn_group`` entries of model.plan_signature for these launches"""
    return ['%s[%s]:dcn:%d:%s' % (tag, ' + '.join(names), phases, ','.join('%d/%d/%d' % t for t in triples)) for tag, names, phases, triples in launches]


def schedule_keys(launches, info, N):
    """the regimes a production schedule reaches"""
    keys = set()
    mains = dict((tuple(names), triples) for tag, names, phases, triples in launches if phases == 1)
    for tag, names, phases, triples in launches:
        keys.add(('group', 'layers', len(names)))
        keys.add(('group', 'phases', 'in three calls'))
        cases = []
        for n, (algo, sk, fo) in zip(names, triples):
            ly, i = info[n]['layer'], info[n]
            cases.append(mk(n, N, ly.H, ly.W, ly.Cin, ly.cout, algo, sk, i['src'], 32, i['up_f'], 'group'))
        plans = [plan_of(c) for c in cases]
        if phases == 4:
            keys |= {('offsets', 'wino' if c.src == 'wino' else 'packed') for c in cases}
        elif phases == 2:
            keys |= {('reduce', c.up_f) for c in cases}
            if tuple(names) not in mains:
                keys.add(('group', 'a FINISH call on another set of layers than the MAIN call'))
            if any(c.up_f and p['splits'] == 1 for c, p in zip(cases, plans)):
                keys.add(('group', 'an up layer with splits == 1'))
        else:
            assert len(set((p['BM'], p['BN'], p['family']) for p in plans)) == 1, names
            fuse_any = any(p['fuse'] for p in plans)
            for c, p, first in zip(cases, plans, group_firsts(cases)):
                keys |= om_keys(c, p)
                keys.add(('split-origin', p['origin']))
                if p['family'] == 'persist':
                    keys |= {('persist', p['WN'], p['NKK']), ('dcn_slots', 'default')}
                else:
                    keys.add(('kernel', p['BM'], p['WN'], fuse_any, p['NKK']))
                    keys |= {('steps', 'odd: the peeled last step' if s % 2 else 'even') for s in p['steps']}
                    keys.add(('xcd', p['xsx'], 'padded ids' if p['padded'] else 'no padding'))
                if p['NKK'] == 4 and p['splits'] > 1 and p['unitsPerSplit'] >= 2:
                    keys.add(('nkk4', 'a shorter last split' if p['nunits'] % p['unitsPerSplit'] else 'two or more units per split'))
            if fuse_any and not all(p['fuse'] for p in plans):
                keys.add(('om', 'a FUSE instantiation running a layer without w_off'))
            if len(set(p['steps'][-1] for p in plans)) > 1:
                keys.add(('group', 'layers of different step counts'))
            if plans[0]['family'] == 'persist' and len(plans) > 1:
                keys.add(('group', 'persistent, several layers'))
    return keys


# every case that can run persistent, in its persistent form: the six that carry a persistent algo and the per-tile cases make_plan
# accepts under the 5xxxx / 6xxxx algo of their tile shape
PERSISTABLE = OrderedDict((c.name, persistent_form(c)) for c in GPU_CASES if persistent_form(c) is not None)
