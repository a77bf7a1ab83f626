"""The schedule of the 16 DeformConv nodes of DLAUp / IDAUp as a pure function: which layers share a MAIN, FINISH or
OFFSETS launch, how K is split, where the offset convs run, which tile shape each launch uses -- and the knob tuples the
tuner times.  No torch, no library: model.py materialises what ``plan`` returns (buffers, descriptors, launches), the
tuner walks ``knob_grid`` / ``persist_candidates``, and the CPU tests hold all of it against the independent
restatement in tests/_dcn_fwd.py.  The schedule fixes the fp32 summation order, so it is pinned in tune_table.json and
compared between ranks (model.plan_signature).

Dataflow (dla.py:539-574): a `proj` node only reads a finished level; the IDAUp step behind it needs the previous node's
output as its skip tensor; a `node` reads that step's result.  Every layer is split in two launches' worth of work --
MAIN (gather + contraction, results or split-K partials) and FINISH (reduction + BN + ReLU + IDAUp step) -- and placed in
the earliest slot t (M_t at time 2t, F_t at time 2t+1) whose inputs exist: main(L) = first t with 2t > time(x);
finish(L) = first t' >= main(L) with 2t'+1 > time(skip).  The layers sharing a slot go out as ONE ct_dcn_v2_group launch
each for M_t and F_t: 8 + 7 launches for the 16 nodes instead of 16 + (offset convs) + 8 reductions, and at one stream
768 .. 1536 workgroups per launch instead of 128 .. 512.

knobs = (fuse_max_cin, chunks_per_split, nkk, split_offsets, cps_small, small_unfuse, persist):
  * the offset/mask conv is computed inside the DCN launch for Cin <= fuse_max_cin -- every workgroup of a split-K layer
    then repeats it over ALL input channels, 47 % of a 256-channel layer's time at one stream -- else ahead of the slot:
    K-split over 64-channel chunks in ONE CT_DCN_OFFSETS launch for all layers of the slot (split_offsets = 1, one
    workgroup per 32-pixel tile and chunk whatever Cin; split_offsets = 3: the same launch as Winograd F(2x2,3x3) tiles,
    one workgroup per 64-pixel block and chunk) or by one conv launch per layer (0; 2: a Winograd launch per layer writing
    raw sums, 2.25x fewer MFMAs: the bias and the mask sigmoid are applied by the DCN launch);
  * every workgroup contracts chunks_per_split 32-channel chunks, in steps of 16 * nkk channels (nkk = 2 / 4: 16 / 32
    MFMAs per wave between barriers);
  * cps_small = chunks per split of the SMALL slots: at one stream the three `proj` slots hold 256 .. 384 workgroups of
    18 (chunk, tap) steps each on 768 workgroup slots -- one wave per SIMD, nothing to hide the gather latency behind --
    while their layers go through the workspace anyway (IDAUp step in the finishing launch); splitting K twice as fine
    fills the chip and halves every workgroup's loop.  0 = off, 2 = two chunks per split, 1 = one chunk per split (then
    in 32-channel steps);
  * small_unfuse = 1: the layers of those slots also leave their offset convs to the slot's K-split OFFSETS launch (a
    fused conv would be repeated by every split); 2: every slot that needs an OFFSETS launch anyway (a layer above the
    fuse threshold) leaves ALL its offset convs to that launch -- a fused conv is repeated by every cout block and split
    of its layer;
  * persist = 1: MAIN launches as persistent launches (ct_dcn_desc.algo 5xxxx / 6xxxx: `dcn_slots` resident workgroups
    striding over the pixel tiles of their column, gathers / weights / the next sampling table running across tile
    boundaries) wherever every layer of the launch can (``can_persist``); bit-identical to the one-workgroup-per-tile
    launch."""
from collections import OrderedDict, namedtuple

SMALL_SLOT_WGS = 600      # a MAIN slot with fewer workgroups than this (of 768 resident ones) may split K finer
MAIN, FINISH, OFFSETS = 1, 2, 4                                           # ct_dcn_v2_group phases (_lib.CT_DCN_*)
FUSE_OFFSET = {'map': 0, 'fused': 1, 'parts': 2, 'wino': 2, 'raw': 3}     # ct_dcn_desc.fuse_offset of an offset source

# x / out: opaque hashable buffer keys; up = (f, skip key, result key) of the IDAUp step behind a `proj` node, or None
Layer = namedtuple('Layer', 'name x Cin H W cout out up')
# src: where the offsets and masks come from -- 'fused' (inside the MAIN launch), 'parts' / 'wino' (the slot's K-split
# OFFSETS launch, plain / Winograd), 'raw' (raw sums of a Winograd conv launch), 'map' (a conv launch writing the map)
Planned = namedtuple('Planned', 'layer main finish fused nkk splits use_ws src')
# tag 'conv': the `.offset` conv launch of names[0] (phase 0, no algos); else one ct_dcn_v2_group launch
Launch = namedtuple('Launch', 'tag names phase algos')
Schedule = namedtuple('Schedule', 'layers launches')                      # {name: Planned} in layer order, [Launch]


def normalize(knobs):
    """the 7-tuple of a 3-, 4-, 6- or 7-tuple: older tables hold fewer knobs (dcnplan3: four, dcnplan4: six)"""
    knobs = tuple(int(v) for v in knobs)
    return knobs + (1, 0, 0, 0)[len(knobs) - 3:]


class _Clock(object):
    """the one slot clock.  A split layer is readable one time step later, which rounds to the same next MAIN slot for
    a consumer that READS it; only a `proj` node whose SKIP input comes from a split layer finishes one slot later (at
    512x512: ida_up.node_1/2 move from slots 7/8 to 8/10 when the 64-channel nodes are split, cps = 1)"""

    def __init__(self):
        self.time_of = {}                        # buffer key -> time after which it is readable (backbone levels: 0)

    def main(self, ly):
        return self.time_of.get(ly.x, 0) // 2 + 1

    def finish(self, ly, main, use_ws):
        """FINISH slot of a layer that goes through its workspace (else None); its result becomes readable"""
        if use_ws:
            finish = max(main, (self.time_of.get(ly.up[1], 0) + 1) // 2) if ly.up is not None else main
            done = 2 * finish + 1
        else:
            finish, done = None, 2 * main
        self.time_of[ly.up[2] if ly.up is not None else ly.out] = done
        return finish


def _use_ws(ly, splits):
    """a layer goes through its workspace (and a FINISH launch) when K is split or an IDAUp step follows: the rule of
    ws_bytes in dcn_mfma.hip for a grouped layer (model.py holds it against ct_dcn_v2_group_plan)"""
    return splits > 1 or ly.up is not None


def slot_sizes(layers, N, cps):
    """({MAIN slot: workgroups}, [MAIN slot of each layer]) of the schedule with ``cps`` chunks per split everywhere"""
    clock, sizes, mains = _Clock(), {}, []
    for ly in layers:                            # (reference order: producers come first)
        main = clock.main(ly)
        mains.append(main)
        splits = max(1, (ly.Cin // 32) // cps)
        clock.finish(ly, main, _use_ws(ly, splits))
        tiles = N * ((ly.H + 1) // 2) * ((ly.W + 15) // 16) * ((ly.cout + 63) // 64)
        sizes[main] = sizes.get(main, 0) + tiles * splits
    return sizes, mains


def can_persist(Cin, splits, nkk, fused):
    """a layer can run in a persistent MAIN launch: no fused offset conv, equal splits, an even number of step units
    (32 channels at nkk 2, 64 at nkk 4) per split"""
    cpsplit = -(-(Cin // 32) // splits)
    return not fused and (Cin // 32) % cpsplit == 0 and cpsplit % (4 if nkk == 4 else 2) == 0


def plan(layers, N, knobs, fuse_enabled=True, winograd=True):
    """Schedule of ``layers`` for one knob tuple.  ``fuse_enabled`` / ``winograd``: the package's CENTERTRACK_FUSE_OFFSET
    / CENTERTRACK_WINOGRAD switches (without Winograd weights the 'raw' and 'wino' sources fall back to 'parts')."""
    fuse_max_cin, cps, nkk, split_offsets, cps_small, small_unfuse, persist = normalize(knobs)

    def fusable(ly):
        return ly.Cin % 64 == 0 and ly.Cin <= fuse_max_cin and fuse_enabled
    sizes, mains = slot_sizes(layers, N, cps)
    slot_cps = {}
    if cps_small and cps_small < cps:
        slot_cps = {t: cps_small for t, wgs in sizes.items() if wgs < SMALL_SLOT_WGS}
    unfuse_slots = {m for ly, m in zip(layers, mains) if not fusable(ly)} if small_unfuse == 2 else set()
    clock, planned = _Clock(), OrderedDict()
    slots = {}                                   # slot -> {'conv' / OFFSETS / MAIN / FINISH: [layer names]}
    for ly in layers:
        main = clock.main(ly)
        c = slot_cps.get(main, cps)
        # (a finely split layer would repeat a fused offset conv in every split: small_unfuse moves it to the slot's
        #  K-split OFFSETS launch instead)
        fused = fusable(ly) and not (small_unfuse and main in slot_cps) and main not in unfuse_slots
        if fused:
            src = 'fused'
        elif ly.Cin % 64 or not split_offsets:
            src = 'map'
        else:
            src = {2: 'raw', 3: 'wino'}.get(split_offsets, 'parts') if winograd else 'parts'
        splits = max(1, (ly.Cin // 32) // c)
        use_ws = _use_ws(ly, splits)
        finish = clock.finish(ly, main, use_ws)
        planned[ly.name] = Planned(ly, main, finish, fused, 2 if (c == 1 or ly.Cin % 64) else nkk, splits, use_ws, src)
        slot = slots.setdefault(main, {})
        if src in ('map', 'raw'):
            slot.setdefault('conv', []).append(ly.name)
        elif src != 'fused':
            slot.setdefault(OFFSETS, []).append(ly.name)
        slot.setdefault(MAIN, []).append(ly.name)
        if finish is not None:
            slots.setdefault(finish, {}).setdefault(FINISH, []).append(ly.name)
    launches = []

    def steps(name):
        p = planned[name]
        return -(-(p.layer.Cin // 32) // p.splits)
    for t in sorted(slots):
        launches.extend(Launch('conv', (name,), 0, ()) for name in slots[t].get('conv', ()))
        for phase, tag in ((OFFSETS, 'dcn.offsets'), (MAIN, 'dcn'), (FINISH, 'dcn.finish')):
            names = slots[t].get(phase, [])
            if phase == MAIN:
                # longest workgroups first: the dispatcher hands out workgroups in id order, so the layer whose
                # workgroups run the most (chunk, tap) steps starts first and the short ones fill the tail of the launch
                names = sorted(names, key=lambda n: -steps(n))
            for i in range(0, len(names), 4):
                part = [planned[n] for n in names[i:i + 4]]
                pers = bool(persist) and phase == MAIN and all(can_persist(p.layer.Cin, p.splits, p.nkk, p.fused) for p in part)
                launches.append(Launch(tag, tuple(p.layer.name for p in part), phase, tuple(
                    (43264 if p.nkk == 4 else 3264) + (20000 if pers and p.nkk == 4 else 50000 if pers else 0) for p in part)))
    return Schedule(planned, launches)


def signature(schedule):
    """the ``dcn_group`` entries of model.plan_signature for a schedule"""
    return ['%s[%s]:dcn:%d:%s' % (l.tag, ' + '.join(l.names), l.phase, ','.join(
        '%d/%d/%d' % (a, schedule.layers[n].splits, FUSE_OFFSET[schedule.layers[n].src]) for a, n in zip(l.algos, l.names)))
        for l in schedule.launches if l.phase]


def knob_grid(layers, N):
    """the tuner's first stage, in the order it times them (ties go to the earlier tuple).  split_offsets = 0 -- one
    conv launch per un-fused layer -- never won a sweep: 368 against 336 us at one stream, 1932 against 1818 us at eight;
    it stays reachable through CENTERTRACK_DCN_KNOBS.  Neither did 128-cout tiles for the layers with >= 128 couts in a
    MAIN launch of their own: 6866 against 6830 us at 32 streams, 1826 against 1806 at eight -- the second launch per
    slot costs what the wider tile gains."""
    for fuse_max in (0, 64, 128, 256):
        for cps in (2, 4, 8):
            small = any(w < SMALL_SLOT_WGS for w in slot_sizes(layers, N, cps)[0].values())
            fine = tuple((c, u) for c in (2, 1) if c < cps for u in (0, 1, 2)) if small else ()
            for nkk in (2, 4):
                for so in ((1, 2, 3) if fuse_max < 256 else (1,)):
                    for cs, un in ((0, 0), (0, 2)) + fine:
                        yield (fuse_max, cps, nkk, so, cs, un, 0)


def persist_candidates(tried):
    """second stage: the tuples to time again with persistent MAIN launches, from ``tried`` = [(us, knobs)] of the
    first -- the five best schedules and every schedule that keeps all offset convs out of the MAIN launches (the only
    layers a persistent launch takes).  Off by default in the tuner: over the 28 pinned shapes the persistent form lost
    everywhere, by 1 .. 8 % (profiles/r06_z_persistent_vs_per_tile_all_shapes.txt)."""
    tried = sorted(tried)
    return [(us, k[:6] + (1,)) for us, k in tried[:5] + [t for t in tried[5:] if t[1][0] == 0 and t[1][5] == 0]]
