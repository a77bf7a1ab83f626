"""Shared pieces of the forward-convolution tests (tests/test_conv_forward_cpu.py, tests/test_hip_conv_forward.py): the launch
plan of ``ct_conv2d`` restated from ``make_plan`` / ``ct_xcd_per`` (centertrack_amd/csrc/conv_mfma.hip, ct_common.h) and
``ct_conv2d_winograd`` (wino_mfma.hip), the table of everything a launch branches on, the list of cases the GPU tests run, the
launches the pinned tune table holds, float64 / float32 references and an fp32 restatement of Winograd F(2x2, 3x3); the same
for ``ct_maxpool2x2``, ``ct_upsample_add`` and the two layout converters.  No GPU, no ctypes.

What pins the restatement: ``ct_conv2d_workspace_bytes`` equals ``conv_plan(...)['bytes']`` (tests/test_conv_forward_cpu.py), which
fixes ``splits`` and ``NT``.  The tile shape (cfg) and the K-split id are NOT observable through the ABI: they are pinned only through
their effect on ``splits`` (the tile count of the automatic split, ``nchunks`` of the clip) and otherwise mirrored by reading.

A regime is a hashable key; a case reaches the keys of ``case_keys``.  ``GPU_CASES`` is built by rules so that every kernel
instantiation gets the same treatment, and every case reaches at least one key that no other case reaches."""
import json
import os
import zlib
from collections import OrderedDict, namedtuple

import torch
import torch.nn.functional as F

from _dcn_bwd import bound, cdiv, err, randn  # noqa: F401  (the project's error measure and bound)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

# ct_set_tuning values ct_conv2d reads, with the defaults of api.cpp (g_tune)
KNOBS = OrderedDict([('conv_cfg', -1), ('conv_pipe', 1), ('conv_small_tiles', 256), ('splitk_target', 512), ('conv_ks', -1),
                     ('conv_ks_below', 512), ('conv_ks_waves', 2048), ('xcd_remap', 0)])
KTH = [16, 8, 4, 4, 2, 4, 8, 4]                      # make_plan: kTH / kBN of the row-tiled shapes 0..7
KBN = [16, 32, 64, 128, 64, 32, 16, 16]
KKS = [(2, 2, 4), (1, 2, 4), (1, 2, 8), (2, 4, 4), (2, 2, 8)]        # kKs: {WM, WN, WK} of the K-split shapes 101..105
# ct_conv2d_winograd: algo -> (WM, WN, K-split wave groups, NB cout blocks walked per workgroup)
WINO = {201: (1, 4, 1, 1), 202: (1, 2, 1, 1), 203: (2, 2, 1, 1), 204: (2, 1, 1, 1), 205: (1, 2, 2, 1), 206: (1, 2, 4, 1),
        207: (1, 1, 4, 1), 208: (1, 2, 1, 2), 209: (1, 2, 1, 4), 210: (1, 2, 1, 5), 211: (1, 2, 1, 8)}
COMBOS = [(1, 1, 4), (1, 1, 2), (1, 1, 1), (3, 1, 2), (3, 1, 1), (3, 2, 1)]      # (KS, STRIDE, NKK) of launch_tile's callers


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan, restated

def xcd_per(coutBlocks, knobs):
    """ct_xcd_per (ct_common.h)"""
    return coutBlocks >> 3 if (knobs['xcd_remap'] and coutBlocks >= 16 and coutBlocks % 8 == 0) else 0


def ks_ok(ksid, Cin, stride):
    """make_plan's ks_ok: the K-split shape needs whole chunks, and 2 rows x 8 waves at stride 2 is too large a patch"""
    if not 0 <= ksid < len(KKS):
        return False
    WM, _, WK = KKS[ksid]
    return Cin % (16 * WK) == 0 and not (stride == 2 and WM == 2 and WK == 8)


def _wino_plan(N, H, W, Cin, Cout, algo, k):
    WM, WN, KSW, NB = WINO[algo]
    if Cin % 64 or (NB > 1 and Cin != 64):
        raise ValueError('algo %d cannot run Cin=%d' % (algo, Cin))
    nchunks = Cin // 64
    coutBlocks = cdiv(Cout, 16 * WN * NB)
    return dict(family='wino', algo=algo, WM=WM, WN=WN, WK=KSW, NB=NB, TH=4 * WM, BN=16 * WN * NB, multi=KSW > 1 or nchunks > 1,
                nchunks=nchunks, chunksPerSplit=nchunks, splits=1, single=nchunks == 1, coutBlocks=coutBlocks,
                xcdPer=xcd_per(coutBlocks, k), NT=cdiv(Cout, 16), tilesX=cdiv(W, 16), tilesY=cdiv(H, 4 * WM), Ho=H, Wo=W,
                bytes=0, origin='off', pipe=None, KS=3, S=1, Cout=Cout)


def conv_plan(N, H, W, Cin, Cout, ks, stride, algo=0, split_k=0, has_workspace=True, has_proj=False, knobs=()):
    """make_plan + ws_bytes + the launch's LDS choice.  ``origin``: where ``splits`` came from -- 'off', 'explicit', 'clipped'
    (split_k > nchunks), 'auto-free' / 'auto-half' / 'auto-32' (the automatic split with neither cap, nchunks / 2 or 32 binding)."""
    k = dict(KNOBS)
    k.update(dict(knobs))
    if 201 <= algo <= 211:
        return _wino_plan(N, H, W, Cin, Cout, algo, k)
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    NT, tilesX = cdiv(Cout, 16), cdiv(Wo, 16)

    def tiles_of(c):
        return N * tilesX * cdiv(Ho, KTH[c]) * cdiv(Cout, KBN[c])
    if Cout <= 16:
        cfg = 0
    elif Cout <= 32:
        cfg = 1 if tiles_of(1) >= k['conv_small_tiles'] else 5
    else:
        cfg = 4 if (tiles_of(2) < k['conv_small_tiles'] or tiles_of(2) >= 2048) else 2
    if k['conv_cfg'] >= 0:
        cfg = k['conv_cfg']
    if 1 <= algo <= 8:
        cfg = algo - 1
    elif algo != 0 and not 101 <= algo < 101 + len(KKS):
        raise ValueError('unknown algo %d' % algo)
    TH, BN = KTH[cfg], KBN[cfg]
    c16 = Cin // 16
    if ks == 1:
        nkk = 4 if c16 % 4 == 0 else (2 if c16 % 2 == 0 else 1)
        if cfg <= 1 and nkk > 2:
            nkk = 2                                                    # big pixel tiles: the LDS patch stays <= 64 KiB
    elif stride == 2:
        nkk = 1
    else:
        nkk = 2 if c16 % 2 == 0 else 1
    nchunks = c16 // nkk
    ksid, want = -1, k['conv_ks']
    if algo >= 101:
        want = algo - 101
        if not ks_ok(want, Cin, stride):
            raise ValueError('algo %d cannot run Cin=%d stride=%d' % (algo, Cin, stride))
    elif algo >= 1:
        want = -2
    if want >= 0:
        if ks_ok(want, Cin, stride):
            ksid = want
    elif want == -1 and split_k <= 0 and tiles_of(2) < k['conv_ks_below']:
        best = 0
        for i in (3, 0, 1, 4, 2):                                      # largest tile first
            WM, WN, WK = KKS[i]
            if not ks_ok(i, Cin, stride) or (16 * WN > NT * 16 and WN > 2):
                continue
            waves = N * tilesX * cdiv(Ho, WM) * cdiv(Cout, 16 * WN) * WK
            if waves >= k['conv_ks_waves']:
                ksid = i
                break
            if waves > best:
                best, ksid = waves, i
    if ksid >= 0:
        TH, BN, nchunks = KKS[ksid][0], 16 * KKS[ksid][1], Cin // (16 * KKS[ksid][2])
    tilesY, coutBlocks = cdiv(Ho, TH), cdiv(Cout, BN)
    tiles = N * tilesX * tilesY * coutBlocks
    splits, origin = split_k, 'explicit' if split_k > 1 else 'off'
    if ksid >= 0 and splits <= 0:
        splits = 1
    if splits <= 0:
        splits = 1
        if has_workspace and tiles < 256 and not has_proj:
            splits, origin = cdiv(k['splitk_target'], tiles), 'auto-free'
            maxs = nchunks // 2 if nchunks >= 2 else 1                # at least ~2 chunks per split
            if splits > maxs:
                splits, origin = maxs, 'auto-half'
            if splits > 32:
                splits, origin = 32, 'auto-32'
    if splits > nchunks:
        splits, origin = nchunks, 'clipped'
    splits = max(splits, 1)
    cps = cdiv(nchunks, splits)
    splits = cdiv(nchunks, cps)
    if splits == 1:
        origin = 'off'
    p = dict(family='ksplit' if ksid >= 0 else 'row', cfg=cfg, ksid=ksid, TH=TH, BN=BN, NKK=nkk, nchunks=nchunks, chunksPerSplit=cps,
             splits=splits, single=cps == 1, coutBlocks=coutBlocks, xcdPer=xcd_per(coutBlocks, k), NT=NT, tilesX=tilesX, tilesY=tilesY,
             tiles=tiles, Ho=Ho, Wo=Wo, bytes=splits * N * Ho * Wo * NT * 16 * 4 if splits > 1 else 0, origin=origin,
             pipe=k['conv_pipe'], KS=ks, S=stride, Cout=Cout)
    if ksid >= 0:
        p.update(WM=KKS[ksid][0], WN=KKS[ksid][1], WK=KKS[ksid][2])
    return p


# ---------------------------------------------------------------------------------------------------------------------
# cases

Case = namedtuple('Case', 'name N H W Cin Cout ks stride algo split_k knobs scale shift res relu nchw sig dep pool proj why')
DEPTH_SCALE = 2.0


def mk(name, N, H, W, Cin, Cout, ks, stride, algo, split_k=1, knobs=(), scale=True, shift=True, res=False, relu=False, nchw=False,
       sig=(0, 0), dep=(0, 0), pool=False, proj=False, why=''):
    return Case(name, N, H, W, Cin, Cout, ks, stride, algo, split_k, tuple(knobs), scale, shift, res, relu, nchw, tuple(sig),
                tuple(dep), pool, proj, why)


def plan_of(case, extra_knobs=()):
    return conv_plan(case.N, case.H, case.W, case.Cin, case.Cout, case.ks, case.stride, case.algo, case.split_k, True, case.proj,
                     tuple(case.knobs) + tuple(extra_knobs))


def case_plans(case):
    """the plans the GPU tests launch for a case: its own, and for a row-tiled launch the one with ``conv_pipe`` flipped (the
    bitwise PIPE 0 / 1 check runs every row-tiled case both ways)"""
    p = plan_of(case)
    if p['family'] != 'row':
        return [p]
    return [p, plan_of(case, (('conv_pipe', 1 - p['pipe']),))]


def side_of(pool, proj):
    return 'both' if pool and proj else ('pool' if pool else ('proj' if proj else None))


def chunk_class(p):
    """chunks one workgroup runs: what the buffer index and the K-split loop's unroll see"""
    n = p['chunksPerSplit']
    if p['family'] == 'row':
        return n if n < 3 else '>=3'
    if p['family'] == 'wino':
        return min(n, 3)
    if p['KS'] == 3:
        return min(n, 3)
    return n if n <= 5 else 3 + (n - 3) % 3                           # U = 3: six chunks and more repeat the tails of 3, 4, 5


def split_form(p):
    """what the kernel sees of a split: 'even', 'short-last' (nchunks % chunksPerSplit != 0) or 'cps1' (single LDS buffer)"""
    if p['chunksPerSplit'] == 1:
        return 'cps1'
    return 'short-last' if p['nchunks'] % p['chunksPerSplit'] else 'even'


def plan_keys(p, side=None):
    """the regimes a launch with plan ``p`` reaches whatever its tensors hold: kernel instantiation, chunk count, split"""
    keys = set()
    if p['family'] == 'row':
        combo = (p['KS'], p['S'], p['NKK'])
        keys.add(('row-pool', p['cfg'], side) if side else ('row',) + combo + (p['cfg'], p['pipe']))
        if p['splits'] > 1:
            keys.add(('row-split',) + combo + (split_form(p),))
        else:
            keys.add(('row-chunks',) + combo + (chunk_class(p),))
    elif p['family'] == 'ksplit':
        keys.add(('ksplit-pool', p['ksid'], side) if side else ('ksplit', p['ksid'], p['KS'], p['S']))
        if p['splits'] > 1:
            keys.add(('split', 'on a K-split kernel'))
        else:
            keys.add(('ksplit-chunks', p['KS'], chunk_class(p)))
    else:
        keys.add(('wino', p['algo']))
        if p['algo'] <= 204:
            keys.add(('wino-form', p['algo'], 'multi' if p['multi'] else 'single'))
        keys.add(('wino-chunks', chunk_class(p)))
    keys.add(('split-origin', p['origin']))
    if p['xcdPer'] > 0:
        keys.add(('xcd', p['family']))
    return keys


def standard(case, p):
    """the treatment every instantiation gets: two images, two tiles each way with ragged last ones (a one-row tile cannot be), exactly three chunks in one launch (two for the
    Winograd shapes that are compiled for one or several), default knobs, scale + shift into an NHWC slice (Winograd: plus residual
    and ReLU)"""
    ok = (case.N > 1 and p['tilesX'] > 1 and p['tilesY'] > 1 and (p['Ho'] % p['TH'] or p['TH'] == 1) and p['Wo'] % 16 and not case.knobs
          and case.scale and case.shift and not case.nchw)
    if p['family'] == 'wino':
        return bool(ok and case.res and case.relu)
    return bool(ok and p['splits'] == 1 and p['chunksPerSplit'] == 3 and not case.res and not case.relu)


def case_keys(case):
    """every regime a case reaches"""
    keys, side = set(), side_of(case.pool, case.proj)
    for p in case_plans(case):
        keys |= plan_keys(p, side)
    p, fam = plan_of(case), plan_of(case)['family']
    Ho, Wo = p['Ho'], p['Wo']
    # An instantiation is credited to the case that gives it the standard treatment only (``standard``), a split form to an explicit
    # split_k (the automatic cases are there for make_plan's arithmetic), and cfg 0 keeps its own chunk / split keys.
    drop = set()
    if not standard(case, p):
        drop |= {'row', 'row-pool', 'ksplit', 'ksplit-pool', 'wino', 'wino-form'}
    if p['origin'] != 'explicit' or (fam == 'row' and p['cfg'] == 0):
        drop.add('row-split')
    if fam == 'row' and p['cfg'] == 0:
        drop.add('row-chunks')
    keys = set(k for k in keys if k[0] not in drop)
    if fam in ('row', 'ksplit'):
        if Ho % p['TH']:
            keys.add((fam, 'ragged last tile row'))
        if Wo % 16:
            keys.add((fam, 'ragged last tile column'))
        if p['tilesY'] > 1:
            keys.add((fam, 'more than one tile row'))
        if p['tilesX'] > 1:
            keys.add((fam, 'more than one tile column'))
        if case.N > 1:
            keys.add((fam, 'N > 1'))
        if case.Cout % p['BN'] and case.Cout % 4:
            keys.add((fam, 'partial last cout block, Cout % 4 != 0'))
        if p['coutBlocks'] * (p['BN'] // 16) > p['NT']:
            keys.add((fam, 'n-tiles past NT (clamped bvo)'))
        if p['splits'] > 1 and p['single'] and (Ho % p['TH'] or Wo % 16):
            keys.add(('split', 'single LDS buffer with splits > 1 and a ragged tile'))
        where = ('cfg0',) if (fam == 'row' and p['cfg'] == 0) else ((p['KS'], p['S'], p['NKK']) if fam == 'row' else ('ksplit',))
        if fam == 'row' and p['cfg'] == 0:
            if p['splits'] == 1:
                keys.add(('cfg0-chunks', chunk_class(p)))
            elif p['origin'] == 'explicit':
                keys.add(('cfg0-split', split_form(p)))
        if p['splits'] > 1:
            if case.res:
                keys.add(('reduce', 'residual'))
            if case.nchw:
                keys.add(('reduce', 'NCHW output'))
            if case.sig[1] > case.sig[0]:
                keys.add(('reduce', 'sigmoid range'))
            if p['NT'] * 16 > case.Cout:
                keys.add(('reduce', 'wsCout > Cout'))
        else:
            kind = {(False, False): 'none', (True, False): 'scale only', (False, True): 'shift only',
                    (True, True): 'scale + shift'}[(case.scale, case.shift)]
            keys.add(('epi', where, kind))
            if case.res:
                keys.add(('epi', where, 'residual at its own pitch'))
            if case.relu:
                keys.add(('epi', where, 'ReLU'))
            if case.nchw:
                keys.add(('epi', where, 'NCHW, Wo % 4 == 0' if Wo % 4 == 0 else 'NCHW, Wo % 4 != 0'))
            for nm, (lo, hi) in (('sig', case.sig), ('dep', case.dep)):
                if hi > lo and lo % 16 and hi % 16 and lo // 16 == (hi - 1) // 16:
                    keys.add(('epi', where, '%s range inside one 16-cout tile' % nm))
    if fam == 'ksplit':
        T = p['WM'] * p['WN']
        if p['WM'] == 2 and Ho % 2:
            keys.add(('ksplit', 'WM = 2 with odd Ho'))
        if T < p['WK']:
            keys.add(('ksplit', 'T < WK (idle finalising waves)'))
        if T > p['WK']:
            keys.add(('ksplit', 'T > WK (NJ = 2)'))
    if fam == 'wino':
        H, W, th = case.H, case.W, p['TH']
        if H < th and W < 16:
            keys.add(('wino', 'map inside one tile'))
        if H == 1:
            keys.add(('wino', 'H == 1'))
        if W == 1:
            keys.add(('wino', 'W == 1'))
        if H > th and H % th:
            keys.add(('wino', 'ragged rows'))
        if W > 16 and W % 16:
            keys.add(('wino', 'ragged columns'))
        if p['NB'] > 1 and cdiv(case.Cout, 16 * p['WN']) % p['NB']:
            keys.add(('wino-nb-ends-inside', p['algo']))
        full = case.scale and case.shift and case.relu
        keys.add(('wino-epi', 'none' if not (case.scale or case.shift or case.res or case.relu) else
                  ('scale + shift + residual + ReLU' if full and case.res else ('no residual' if full else 'other'))))
        if case.res:
            keys.add(('wino', 'x, y and res at three pitches'))
    return keys


# ---------------------------------------------------------------------------------------------------------------------
# the regime table

def _feasible_row():
    """what make_plan can produce for a forced row-tiled shape: {(KS, S, NKK, cfg)}, {(KS, S, NKK, chunk class)}, {(KS, S, NKK,
    split form)}, and the same two for cfg 0 -- by enumeration over Cin = 16 .. 256 and split_k = 1 .. Cin / 16"""
    inst, chunks, forms, c0chunks, c0forms = set(), set(), set(), set(), set()
    for ks, s in ((1, 1), (3, 1), (3, 2)):
        for cfg in range(8):
            for c16 in range(1, 17):
                for sk in range(1, c16 + 1):
                    p = conv_plan(1, 8, 8, 16 * c16, 64, ks, s, cfg + 1, sk)
                    combo = (ks, s, p['NKK'])
                    inst.add(combo + (cfg,))
                    (forms if p['splits'] > 1 else chunks).add(combo + ((split_form if p['splits'] > 1 else chunk_class)(p),))
                    if cfg == 0:
                        (c0forms if p['splits'] > 1 else c0chunks).add((split_form if p['splits'] > 1 else chunk_class)(p))
    return inst, chunks, forms, c0chunks, c0forms


def conv_regimes():
    """key -> where in the sources the branch lives"""
    r = OrderedDict()
    inst, chunks, forms, c0chunks, c0forms = _feasible_row()
    for key in sorted(inst):
        for pipe in (0, 1):
            r[('row',) + key + (pipe,)] = 'conv_mfma.hip: ct_conv2d -> launch_tile<KS,STRIDE,NKK> -> launch_tile2<..,PIPE>(cfg); nkk: make_plan'
    for cfg in range(8):
        for side in ('pool', 'proj', 'both'):
            r[('row-pool', cfg, side)] = 'conv_mfma.hip: launch_cfg, `if (a.pool_y || a.proj_wp)` -> conv_mfma_kernel<..,POOL=true>'
    for key in sorted(chunks, key=str):
        r[('row-chunks',) + key] = 'conv_mfma.hip: conv_mfma_kernel chunk loop, `cur = (c - c_begin) & 1`; launch_cfg halves the LDS at 1'
    for key in sorted(forms, key=str):
        r[('row-split',) + key] = 'conv_mfma.hip: conv_mfma_kernel `c_end = min(a.nchunks, c_begin + a.chunksPerSplit)`, `if (a.ws)`'
    for n in sorted(c0chunks, key=str):
        r[('cfg0-chunks', n)] = 'conv_mfma.hip: the 256 px x 16 shape (largest LDS patch), chunk loop'
    for f in sorted(c0forms):
        r[('cfg0-split', f)] = 'conv_mfma.hip: the 256 px x 16 shape, split-K partials'
    for g in ('ragged last tile row', 'ragged last tile column', 'more than one tile row', 'more than one tile column', 'N > 1',
              'partial last cout block, Cout % 4 != 0', 'n-tiles past NT (clamped bvo)'):
        r[('row', g)] = 'conv_mfma.hip: conv_mfma_kernel block decode / `bvo[nt] = min(nt0 + nt, a.NT - 1)`; ct_common.h: ct_store_tile'
        r[('ksplit', g)] = 'conv_mfma.hip: conv_ksplit_kernel block decode; ksplit_core.h: bvo; ct_common.h: ct_store_tile'
    for i in range(len(KKS)):
        for ks, s in ((1, 1), (3, 1), (3, 2)):
            if ks_ok(i, 1280, s):
                r[('ksplit', i, ks, s)] = 'conv_mfma.hip: launch_ks<KS,STRIDE>(id) -> conv_ksplit_kernel; make_plan: ks_ok'
        if ks_ok(i, 1280, 2):
            for side in ('pool', 'proj', 'both'):
                r[('ksplit-pool', i, side)] = 'conv_mfma.hip: launch_ks_cfg `if (a.pool_y || a.proj_wp)`; ksplit_core.h: SIDE'
    for n in (1, 2, 3, 4, 5):
        r[('ksplit-chunks', 1, n)] = 'ksplit_core.h: `U = (S % R == 0) ? 1 : R` = 3 at ks 1, `for (c0 ..; c0 += U)` with `if (c < c_end)`'
    for n in (1, 2, 3):
        r[('ksplit-chunks', 3, n)] = 'ksplit_core.h: U = 1 at ks 3; `cur = (c - c_begin) & 1`; launch_ks_cfg: one buffer at 1 chunk'
    r[('ksplit', 'WM = 2 with odd Ho')] = 'conv_mfma.hip: fin_main `oy < a.epi.Ho`; ct_store_tile `if (oy >= e.Ho) return`'
    r[('ksplit', 'T < WK (idle finalising waves)')] = 'ksplit_core.h: `if (t < T)` of the reduction'
    r[('ksplit', 'T > WK (NJ = 2)')] = 'conv_mfma.hip: conv_ksplit_kernel `NJ = (WM * WN + WK - 1) / WK`'
    for o in ('off', 'explicit', 'clipped', 'auto-free', 'auto-half', 'auto-32'):
        r[('split-origin', o)] = 'conv_mfma.hip: make_plan, `int splits = d->split_k` .. `p->splits = ct_cdiv(..)`'
    r[('split', 'on a K-split kernel')] = 'conv_mfma.hip: conv_ksplit_kernel fin_main `if (a.ws)`'
    r[('split', 'single LDS buffer with splits > 1 and a ragged tile')] = 'conv_mfma.hip: launch_cfg `a.chunksPerSplit == 1`'
    for w in ('residual', 'NCHW output', 'sigmoid range', 'wsCout > Cout'):
        r[('reduce', w)] = 'conv_mfma.hip: splitk_reduce_kernel'
    for where in COMBOS + [('cfg0',)]:
        for e in ('none', 'scale only', 'shift only', 'scale + shift', 'residual at its own pitch', 'ReLU', 'NCHW, Wo % 4 == 0',
                  'NCHW, Wo % 4 != 0', 'sig range inside one 16-cout tile', 'dep range inside one 16-cout tile'):
            r[('epi', where, e)] = 'ct_common.h: ct_load_scale_shift, ct_store_tile, ct_epilogue_value'
    r[('epi', ('ksplit',), 'scale + shift')] = 'conv_mfma.hip: conv_ksplit_kernel psc / psh per finalised tile'
    for fam in ('row', 'ksplit', 'wino'):
        r[('xcd', fam)] = 'ct_common.h: ct_xcd_per, ct_block_cout `if (per)`'
    for a in sorted(WINO):
        r[('wino', a)] = 'wino_mfma.hip: ct_conv2d_winograd `switch (d->algo)`'
        if a <= 204:
            for form in ('single', 'multi'):
                r[('wino-form', a, form)] = 'wino_mfma.hip: launch_wino `a.nchunks > 1 ? ..<true> : ..<false>`'
        if WINO[a][3] > 1:
            r[('wino-nb-ends-inside', a)] = 'wino_mfma.hip: wino_body, the walk over NB cout blocks past Cout'
    for n in (1, 2, 3):
        r[('wino-chunks', n)] = 'wino_mfma.hip: wino_body `for (ch ..)`, `cur ^ 1`; launch_wino2: one patch buffer at 1 chunk'
    for g in ('map inside one tile', 'H == 1', 'W == 1', 'ragged rows', 'ragged columns', 'x, y and res at three pitches'):
        r[('wino', g)] = 'wino_mfma.hip: wino_body staging (zero padded patch) and the epilogue store'
    for e in ('none', 'no residual', 'scale + shift + residual + ReLU'):
        r[('wino-epi', e)] = 'wino_mfma.hip: wino_body epilogue (ct_epilogue_plain)'
    return r


CONV_REGIMES = conv_regimes()


def reached_conv_regimes(cases):
    got = set()
    for c in cases:
        got |= case_keys(c)
    return [k for k in CONV_REGIMES if k in got]


def missing_conv_regimes(cases):
    """keys of the table no case of the list reaches"""
    got = set(reached_conv_regimes(cases))
    return [k for k in CONV_REGIMES if k not in got]


# ---------------------------------------------------------------------------------------------------------------------
# the cases the GPU tests run

def _row_shape(cfg, ks, s, even=False):
    """N = 2, Ho = TH + 3, Wo = 21; a plain stride-2 case has odd H and W, one with side outputs H = 2 Ho, W = 2 Wo"""
    Ho, Wo = KTH[cfg] + 3, 21
    if s == 1:
        return 2, Ho, Wo
    return (2, 2 * Ho, 2 * Wo) if even else (2, 2 * Ho - 1, 2 * Wo - 1)


def _find_row(ks, s, nkk, cfgs, want):
    """the smallest (cfg, Cin, split_k) of a forced row-tiled launch whose plan satisfies ``want``"""
    for c16 in range(1, 17):
        for cfg in cfgs:
            for sk in range(1, c16 + 1):
                p = conv_plan(1, 8, 8, 16 * c16, 64, ks, s, cfg + 1, sk)
                if p['NKK'] == nkk and want(p):
                    return cfg, 16 * c16, sk
    return None


def _gpu_cases():
    inst, chunks, forms, c0chunks, c0forms = _feasible_row()
    L = []
    # ---- one case per row-tiled instantiation: three chunks, two ragged tiles each way, two images, Cout = BN + 27 (a partial
    # last block with Cout % 4 == 3; its n-tiles run past NT where BN >= 64); the PIPE 0 / 1 check runs each both ways
    for ks, s, nkk, cfg in sorted(inst):
        N, H, W = _row_shape(cfg, ks, s)
        L.append(mk('row_k%ds%d_nkk%d_cfg%d' % (ks, s, nkk, cfg), N, H, W, 48 * nkk, KBN[cfg] + 27, ks, s, cfg + 1,
                    why='conv_mfma_kernel<%d,%d,cfg %d,NKK %d> with PIPE 0 and 1' % (ks, s, cfg, nkk)))
    for cfg in range(8):
        for side in ('pool', 'proj', 'both'):
            N, H, W = _row_shape(cfg, 3, 2, even=True)
            L.append(mk('rowpool_cfg%d_%s' % (cfg, side), N, H, W, 48, KBN[cfg] + 27, 3, 2, cfg + 1, pool=side != 'proj',
                        proj=side != 'pool', why='POOL instantiation of cfg %d, side outputs: %s' % (cfg, side)))
    # ---- per (KS, STRIDE, NKK), on one tile shape (32 px x 64 where it can): one and two chunks, the three split forms, the epilogue
    pref = [4, 2, 5, 1, 0, 3, 6, 7]
    for ks, s, nkk in COMBOS:
        for n in (1, 2):
            if (ks, s, nkk, n) in chunks:
                cfg, Cin, sk = _find_row(ks, s, nkk, pref, lambda p, n=n: p['splits'] == 1 and p['chunksPerSplit'] == n)
                N, H, W = _row_shape(cfg, ks, s)
                L.append(mk('chunks%d_k%ds%d_nkk%d' % (n, ks, s, nkk), N, H, W, Cin, KBN[cfg] + 27, ks, s, cfg + 1,
                            why='%d chunk(s) per launch%s' % (n, ': one LDS buffer' if n == 1 else ': the buffer index never flips back')))
        for form in ('even', 'short-last', 'cps1'):
            if (ks, s, nkk, form) in forms:
                cfg, Cin, sk = _find_row(ks, s, nkk, pref, lambda p, f=form: p['splits'] > 1 and split_form(p) == f and p['origin'] == 'explicit')
                N, H, W = _row_shape(cfg, ks, s)
                L.append(mk('split_%s_k%ds%d_nkk%d' % (form, ks, s, nkk), N, H, W, Cin, KBN[cfg] + 27, ks, s, cfg + 1, split_k=sk,
                            why='explicit split_k %d, %s' % (sk, form)))
        cfg = 4 if (ks, s, nkk, 4) in inst else 1
        N, H, W = _row_shape(cfg, ks, s)
        L += _epilogue_cases('k%ds%d_nkk%d' % (ks, s, nkk), N, H, W, 48 * nkk, KBN[cfg] + 27, ks, s, cfg + 1)
    # ---- the same once more on cfg 0 (16 rows x 16 px: the largest LDS patch), 3x3 stride 2
    for n in (1, 2):
        cfg, Cin, sk = _find_row(3, 2, 1, [0], lambda p, n=n: p['splits'] == 1 and p['chunksPerSplit'] == n)
        L.append(mk('cfg0_chunks%d' % n, 2, 37, 41, Cin, 43, 3, 2, 1, why='cfg 0, %d chunk(s)' % n))
    for form in sorted(c0forms):
        cfg, Cin, sk = _find_row(3, 2, 1, [0], lambda p, f=form: p['splits'] > 1 and split_form(p) == f and p['origin'] == 'explicit')
        L.append(mk('cfg0_split_%s' % form, 2, 37, 41, Cin, 43, 3, 2, 1, split_k=sk, why='cfg 0, split_k %d, %s' % (sk, form)))
    L += _epilogue_cases('cfg0', 2, 37, 41, 48, 43, 3, 2, 1)
    # ---- K-split kernels: N = 2, Ho = 5 (odd: WM = 2 leaves a half tile), Wo = 21, three chunks, Cout = 16 WN + 27
    for i, (WM, WN, WK) in enumerate(KKS):
        for ks, s in ((1, 1), (3, 1), (3, 2)):
            if ks_ok(i, 48 * WK, s):
                H, W = (5, 21) if s == 1 else (9, 41)
                L.append(mk('ksplit%d_k%ds%d' % (i, ks, s), 2, H, W, 48 * WK, 16 * WN + 27, ks, s, 101 + i,
                            why='conv_ksplit_kernel<%d,%d,%d,%d,%d>' % (ks, s, WM, WN, WK)))
        if ks_ok(i, 48 * WK, 2):
            for side in ('pool', 'proj', 'both'):
                L.append(mk('ksplitpool%d_%s' % (i, side), 2, 10, 42, 48 * WK, 16 * WN + 27, 3, 2, 101 + i, pool=side != 'proj',
                            proj=side != 'pool', why='POOL instantiation of K-split id %d, side outputs: %s' % (i, side)))
    for n in (1, 2, 4, 5):
        L.append(mk('ksplit1_k1_chunks%d' % n, 2, 5, 21, 64 * n, 59, 1, 1, 102, why='1x1 K-split loop (unrolled by 3) with %d chunk(s)' % n))
    for n in (1, 2):
        L.append(mk('ksplit1_k3_chunks%d' % n, 2, 5, 21, 64 * n, 59, 3, 1, 102, why='3x3 K-split loop with %d chunk(s)' % n))
    # ---- where the split count comes from, and the reduce kernel's epilogue
    L.append(mk('split_clipped', 2, 5, 21, 128, 59, 3, 1, 102, split_k=5, why='split_k 5 > nchunks 2 on a K-split kernel: clipped, one chunk per split'))
    L.append(mk('split_auto_free', 2, 19, 21, 144, 107, 1, 1, 8, split_k=0, why='automatic split, 140 tiles: cdiv(512, 140) = 4 <= nchunks / 2 = 4'))
    L.append(mk('split_auto_half', 1, 4, 4, 128, 16, 1, 1, 1, split_k=0, why='automatic split, one tile: 512 cut to nchunks / 2 = 2'))
    L.append(mk('split_auto_32', 1, 4, 4, 2112, 16, 1, 1, 1, split_k=0,
                why='automatic split, one tile, nchunks 66: nchunks / 2 = 33 cut to 32 (at Cin 2048 nchunks / 2 is 32 itself and the line never assigns)'))
    L.append(mk('reduce_res_relu', 2, 5, 21, 256, 59, 3, 1, 102, split_k=2, res=True, relu=True,
                why='global split-K on top of a K-split kernel; splitk_reduce_kernel with residual and ReLU'))
    L.append(mk('reduce_nchw_sig', 2, 5, 21, 256, 59, 3, 1, 102, split_k=2, nchw=True, sig=(3, 9), dep=(17, 22),
                why='global split-K on top of a K-split kernel; splitk_reduce_kernel with NCHW output, sigmoid and depth ranges'))
    # ---- XCD remap: 16 cout blocks
    x1 = (('xcd_remap', 1),)
    L.append(mk('xcd_row', 2, 19, 21, 48, 256, 1, 1, 1, knobs=x1, why='xcd_remap = 1, 16 cout blocks of cfg 0'))
    L.append(mk('xcd_ksplit', 2, 5, 21, 192, 512, 1, 1, 102, knobs=x1, why='xcd_remap = 1, 16 cout blocks of K-split id 1'))
    L.append(mk('xcd_wino', 2, 11, 21, 64, 256, 3, 1, 204, knobs=x1, res=True, relu=True, why='xcd_remap = 1, 16 cout blocks of algo 204'))
    # ---- Winograd: N = 2, H = 4 WM + 3, W = 21, Cout = 16 WN NB + 27, scale + shift + residual + ReLU
    for a in sorted(WINO):
        WM, WN, KSW, NB = WINO[a]
        for Cin in (((64, 192) if a == 202 else (64, 128)) if a <= 204 else ((128,) if NB == 1 else (64,))):     # (202: three chunks, the patch buffer flips back)
            L.append(mk('wino%d_cin%d' % (a, Cin), 2, 4 * WM + 3, 21, Cin, 16 * WN * NB + 27, 3, 1, a, res=True, relu=True,
                        why='algo %d, %d chunk(s)%s' % (a, Cin // 64, ', Cout ends inside the walk' if NB > 1 else '')))
    L.append(mk('wino202_h1', 2, 1, 21, 64, 59, 3, 1, 202, res=True, relu=True, why='H == 1'))
    L.append(mk('wino202_w1', 2, 7, 1, 64, 59, 3, 1, 202, res=True, relu=True, why='W == 1'))
    L.append(mk('wino202_3x5', 2, 3, 5, 64, 59, 3, 1, 202, res=True, relu=True, why='a map inside one tile'))
    L.append(mk('wino202_epi_none', 2, 7, 21, 64, 59, 3, 1, 202, scale=False, shift=False, why='no epilogue'))
    L.append(mk('wino202_epi_nores', 2, 7, 21, 64, 59, 3, 1, 202, relu=True, why='scale + shift + ReLU, no residual'))
    return L


def _epilogue_cases(tag, N, H, W, Cin, Cout, ks, s, algo):
    pad = ks // 2
    Wo = (W + 2 * pad - ks) // s + 1
    W20 = W - 1 if s == 1 else W - 2                                  # Wo 21 -> 20
    assert Wo == 21 and (W20 + 2 * pad - ks) // s + 1 == 20
    return [mk('epi_none_' + tag, N, H, W, Cin, Cout, ks, s, algo, scale=False, shift=False, why='no epilogue operand'),
            mk('epi_scale_relu_' + tag, N, H, W, Cin, Cout, ks, s, algo, shift=False, relu=True, why='scale only, ReLU'),
            mk('epi_shift_res_' + tag, N, H, W, Cin, Cout, ks, s, algo, scale=False, res=True, why='shift only, residual at a pitch of its own'),
            mk('epi_nchw4_sig_' + tag, N, H, W20, Cin, Cout, ks, s, algo, nchw=True, sig=(3, 9), dep=(17, 22),
               why='NCHW with Wo 20 (vector store), sigmoid couts 3..8 and depth couts 17..21 inside their tiles'),
            mk('epi_nchw_' + tag, N, H, W, Cin, Cout, ks, s, algo, nchw=True, why='NCHW with Wo 21: scalar stores, the last quad straddles the row end')]


GPU_CASES = _gpu_cases()
CASE = OrderedDict((c.name, c) for c in GPU_CASES)
assert len(CASE) == len(GPU_CASES)


def relu_input(case):
    """half of the cases read a post-ReLU map, the production input"""
    return case.name in CASE and list(CASE).index(case.name) % 2 == 1


# ---------------------------------------------------------------------------------------------------------------------
# production launches

def production_conv_launches():
    """[(key, (N, H, W, Cin, Cout, ks, stride), has_proj, algo, split_k)] of every conv* key of the pinned tune table"""
    table = json.load(open(os.path.join(ROOT, 'centertrack_amd', 'tune_table.json')))
    out = []
    for key, val in table.items():
        if not key.startswith('conv'):
            continue
        head, nums = key.split(':')
        N, H, W, Cin, Cout, ks, stride = [int(v) for v in nums.split(',')][:7]
        out.append((key, (N, H, W, Cin, Cout, ks, stride), 'P' in head[4:], int(val[0]), int(val[1])))
    return out


def launch_keys(shape, has_proj, algo, split_k, knobs=()):
    """the regimes of ``plan_keys`` a production launch can reach: a 3x3 stride-2 launch may carry either side output"""
    N, H, W, Cin, Cout, ks, stride = shape
    p = conv_plan(N, H, W, Cin, Cout, ks, stride, algo, split_k, True, has_proj, knobs)
    keys = plan_keys(p, None)
    if ks == 3 and stride == 2 and H % 2 == 0 and W % 2 == 0 and p['family'] != 'wino':
        for side in (('proj', 'both') if has_proj else ('pool',)):
            keys |= plan_keys(p, side)
    if has_proj:
        keys = set(k for k in keys if k[0] not in ('row', 'ksplit') or len(k) < 4)      # (a projection launch is never plain)
    return keys


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references

_input_cache, _ref_cache = {}, {}


def seed_of(case):
    return zlib.crc32(case.name.encode()) % 100000


def conv_inputs(case):
    """fp32 tensors of a case (NCHW), once per process: x ~ N(0,1) (ReLU for every other case), w * (Cin ks^2)^-1/2, scale in
    [0.5, 1.5), shift, residual, and the projection's 1x1 weight / scale / shift"""
    if case.name not in _input_cache:
        s, pad = seed_of(case), case.ks // 2
        Ho, Wo = (case.H + 2 * pad - case.ks) // case.stride + 1, (case.W + 2 * pad - case.ks) // case.stride + 1
        x = randn(s, case.N, case.Cin, case.H, case.W)
        if relu_input(case):
            x = torch.relu(x)
        d = dict(x=x.float(), w=(randn(s + 1, case.Cout, case.Cin, case.ks, case.ks) * (case.Cin * case.ks ** 2) ** -0.5).float())
        d['scale'] = (torch.rand(case.Cout, generator=torch.Generator().manual_seed(s + 2), dtype=torch.float64) + 0.5).float() if case.scale else None
        d['shift'] = randn(s + 3, case.Cout).float() if case.shift else None
        d['res'] = randn(s + 4, case.N, case.Cout, Ho, Wo).float() if case.res else None
        if case.proj:
            d['pw'] = (randn(s + 5, case.Cout, case.Cin, 1, 1) * case.Cin ** -0.5).float()
            d['pscale'] = (torch.rand(case.Cout, generator=torch.Generator().manual_seed(s + 6), dtype=torch.float64) + 0.5).float()
            d['pshift'] = randn(s + 7, case.Cout).float()
        _input_cache[case.name] = d
    return _input_cache[case.name]


def epilogue(case, z, d, dt):
    """ct_epilogue_value in ``dt``: z * scale + shift + res, ReLU, sigmoid on [sig), the depth transform on [dep)"""
    if d['scale'] is not None:
        z = z * d['scale'].to(dt).view(1, -1, 1, 1)
    if d['shift'] is not None:
        z = z + d['shift'].to(dt).view(1, -1, 1, 1)
    if d['res'] is not None:
        z = z + d['res'].to(dt)
    if case.relu:
        z = torch.relu(z)
    z = z.clone()
    lo, hi = case.sig
    if hi > lo:
        z[:, lo:hi] = torch.sigmoid(z[:, lo:hi])
    lo, hi = case.dep
    if hi > lo:
        z[:, lo:hi] = (1.0 / (torch.sigmoid(z[:, lo:hi]) + 1e-6) - 1.0) * DEPTH_SCALE
    return z


def _reference(case, dt, conv=None):
    d = conv_inputs(case)
    x, w = d['x'].to(dt), d['w'].to(dt)
    z = F.conv2d(x, w, None, case.stride, case.ks // 2) if conv is None else conv(x, w)
    out = dict(y=epilogue(case, z, d, dt))
    if case.pool:
        out['pool'] = F.max_pool2d(d['x'], 2, 2)
    if case.proj:
        out['proj'] = (F.conv2d(F.max_pool2d(x, 2, 2), d['pw'].to(dt)) * d['pscale'].to(dt).view(1, -1, 1, 1)
                       + d['pshift'].to(dt).view(1, -1, 1, 1))
    return out


def reference64(case):
    """F.conv2d in float64 on the CPU with the epilogue restated in float64 -> dict(y[, pool][, proj]), once per process"""
    if case.name not in _ref_cache:
        _ref_cache[case.name] = _reference(case, torch.float64)
    return _ref_cache[case.name]


def reference32(case):
    return _reference(case, torch.float32)


_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
_BT = [[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]]
_AT = [[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]]


def winograd32(x, w):
    """conv3x3(x, w, stride 1, pad 1) by Winograd F(2x2, 3x3) in fp32 (Lavin & Gray): U = G g G^T, V = B^T d B per 4x4 input tile
    (stride 2), M = sum over Cin of U .* V in fp32, Y = A^T M A per 2x2 output tile"""
    assert x.dtype == torch.float32 and w.dtype == torch.float32
    G, BT, AT = torch.tensor(_G), torch.tensor(_BT), torch.tensor(_AT)
    N, C, H, W = x.shape
    th, tw = cdiv(H, 2), cdiv(W, 2)
    xp = F.pad(x, (1, 2 * tw - W + 1, 1, 2 * th - H + 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                            # [N, C, th, tw, 4, 4]
    V = BT @ d @ BT.t()
    U = G @ w @ G.t()                                                 # [Co, C, 4, 4]
    M = torch.einsum('nctwij,ocij->notwij', V, U)
    Y = AT @ M @ AT.t()                                               # [N, Co, th, tw, 2, 2]
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, w.shape[0], 2 * th, 2 * tw)
    return y[:, :, :H, :W].contiguous()


def yardstick32(case):
    """the fp32 computation whose error against float64 is the case's e32: ``winograd32`` for a Winograd launch, else F.conv2d"""
    if 201 <= case.algo <= 211:
        return _reference(case, torch.float32, winograd32)
    return reference32(case)


def plain_channels(case):
    """the couts outside the sigmoid and depth ranges (those two are checked element-wise)"""
    keep = torch.ones(case.Cout, dtype=torch.bool)
    for lo, hi in (case.sig, case.dep):
        keep[lo:hi] = False
    return keep


def case_errors(case, got, which='y'):
    """(err, e32, bound) of a result (NCHW) by the project's measure, over the plain channels of the main output"""
    r64, r32 = reference64(case)[which], yardstick32(case)[which]
    keep = plain_channels(case) if which == 'y' else slice(None)
    e = err(got.detach().cpu().double()[:, keep], r64[:, keep])
    e32 = err(r32[:, keep], r64[:, keep])
    return e, e32, bound(e32, case.Cin * (case.ks ** 2 if which == 'y' else 1))


# ---------------------------------------------------------------------------------------------------------------------
# the element-wise ops

GRID_CAP = 4096 * 256                                   # elementwise.hip: grid_for caps the grid at 256 * 16 workgroups of 256

# (N, H, W, C, pitched)
POOL_SHAPES = [(2, 7, 9, 4, True),            # odd H and W (the last row and column are dropped), one channel quad, slices of wider buffers
               (1, 6, 10, 132, False),        # 33 quads per pixel: the split of the index is a real division
               (2, 256, 520, 64, False)]      # 1 064 960 quads = 4096 * 256 + 16 384: the grid is capped, the second round ragged
# (N, H, W, C, f, pitched)
UP_SHAPES = [(2, 3, 5, 4, 2, True),           # f 2, one channel quad, x / skip / y slices of wider buffers
             (1, 2, 3, 132, 4, False),        # f 4, 33 quads
             (2, 1, 1, 8, 8, True),           # f 8 on a 1x1 input: every output pixel loses one tap on both axes
             (2, 64, 130, 64, 2, False)]      # 1 064 960 quads: capped grid, ragged second round
# (C, H, W): N = 2 and a pitch of C + 5
LAYOUT_SHAPES = [(1, 1, 1), (27, 5, 7), (33, 25, 41)]


def ew_plan(quads):
    capped = quads > GRID_CAP
    return dict(quads=quads, capped=capped, ragged=capped and quads % GRID_CAP != 0)


def pool_keys(s):
    N, H, W, C, pitched = s
    p = ew_plan(N * (H // 2) * (W // 2) * (C // 4))
    k = {'grid capped' if p['capped'] else 'grid uncapped', 'pitched' if pitched else 'unpitched'}
    k |= {n for n, v in (('capped grid, ragged second round', p['ragged']), ('odd H', H % 2), ('odd W', W % 2), ('C == 4', C == 4),
                         ('C == 132', C == 132)) if v}
    return k


def up_keys(s):
    N, H, W, C, f, pitched = s
    p = ew_plan(N * H * f * W * f * (C // 4))
    k = {'grid capped' if p['capped'] else 'grid uncapped', 'pitched' if pitched else 'unpitched', 'f == %d' % f,
         'border: one tap outside on one axis', 'border: one tap outside on both axes'}       # (every map has edges and corners)
    k |= {n for n, v in (('capped grid, ragged second round', p['ragged']), ('1x1 input: no pixel keeps all four taps', H == 1 and W == 1),
                         ('interior pixels: all four taps inside', H > 1 and W > 1), ('C == 4', C == 4), ('C == 132', C == 132)) if v}
    return k


def layout_keys(s):
    C, H, W = s
    return {'C == %d' % C, 'HW == %d' % (H * W)}


def pool_regimes():
    """elementwise.hip: maxpool2x2_kernel's grid-stride loop, grid_for's cap, Ho = H >> 1"""
    return ['grid uncapped', 'grid capped', 'capped grid, ragged second round', 'pitched', 'unpitched', 'odd H', 'odd W', 'C == 4', 'C == 132']


def upsample_regimes():
    """elementwise.hip: upsample_add_kernel's grid-stride loop, grid_for's cap, the `yy < 0 || yy >= H` / `xx < 0 || xx >= W` taps"""
    return ['grid uncapped', 'grid capped', 'capped grid, ragged second round', 'pitched', 'unpitched', 'f == 2', 'f == 4', 'f == 8',
            '1x1 input: no pixel keeps all four taps', 'interior pixels: all four taps inside', 'border: one tap outside on one axis',
            'border: one tap outside on both axes', 'C == 4', 'C == 132']


def layout_regimes():
    """elementwise.hip: the 32 x 32 LDS tile of nchw_to_nhwc_kernel / nhwc_to_nchw_kernel -- below, across and past one tile"""
    return ['C == 1', 'C == 27', 'C == 33', 'HW == 1', 'HW == 35', 'HW == 1025']


def _missing(regimes, keys_of, shapes):
    got = set()
    for s in shapes:
        got |= keys_of(s)
    return [r for r in regimes if r not in got]


def missing_pool_regimes(shapes):
    return _missing(pool_regimes(), pool_keys, shapes)


def missing_upsample_regimes(shapes):
    return _missing(upsample_regimes(), up_keys, shapes)


def missing_layout_regimes(shapes):
    return _missing(layout_regimes(), layout_keys, shapes)


def upsample_inputs(shape):
    N, H, W, C, f, _ = shape
    x, w = randn(41, N, C, H, W).float(), (randn(42, C, 1, 2 * f, 2 * f) * 0.5).float()
    return x, w, randn(43, N, C, H * f, W * f).float()


def upsample_reference(shape, dt):
    """depth-wise ConvTranspose2d(k = 2f, stride f, pad f / 2) + skip in ``dt``"""
    x, w, skip = upsample_inputs(shape)
    f = shape[4]
    return F.conv_transpose2d(x.to(dt), w.to(dt), None, f, f // 2, groups=shape[3]) + skip.to(dt)
