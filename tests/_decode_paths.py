"""The heat-map decode (centertrack_amd/csrc/decode.hip: stage 1, stage 2a, stage 2; csrc/pose.hip reuses it for the joint maps)
restated for the tests: the host schedule, a model of which way every kernel ends on a given heat map, the reference of the
operation, six mutations of that reference, and the case list tests/test_decode_paths_cpu.py proves complete and
tests/test_hip_decode_paths.py runs on the GPU.  No GPU, no ctypes.

THE SCHEDULE (``schedule``; pick_seg, pick_groups, ct_decode): seg = 1024, halved while B*C*ceil(h*w/seg) < 256 and seg > 256;
nseg = ceil(h*w/seg); M2 = C*nseg*K candidate slots per image; G = 0 when M2 <= SLICE, else ceil(M2/SLICE) stage-2a slices per
image, after which stage 2 reads G*K slots; workspace = (B*M2 + B*G*K) * 8 bytes.

THE MODEL (``image_paths``) follows the keys (score bits : ~flat index) through the three kernels and returns the labels reached:
  stage 1   s1:seg256 / s1:seg512 / s1:seg1024; s1:all (a segment with <= K survivors: compacted) / s1:rank (more: rank counting
            keeps K); s1:ragged (short last segment); s1:midrow (a segment starts inside a row)
  stage 2a  per slice, select_topk_regs: 2a:hist (rc == K), 2a:few (rc == -1, keep_all), 2a:radix (rc == -2)
  stage 2   regs (slots <= SEL_U * 1024, histogram select first) or mem, crossed with hist, bitonic (total <= FCAP), rank
            (per-thread-maxima threshold, n <= FCAP), radix (n > FCAP), slow (fewer than K positive survivors).  mem:hist cannot
            exist: the histogram select only runs on keys held in registers.
and, so that every case of the list is there for a reason the table can name:
  tie:<label>        the K-th and the (K+1)-th score of what <label> selects from are EQUAL: the cut is decided by index alone.
                     For a stage-2a slice and for a stage-2 end it stands IN PLACE of <label>, which then means a cut between
                     distinct scores
  sel:clamp:hist / sel:clamp:overflow   the boundary bin of a histogram select is bin 1023 holding scores >= 1.0 (sel_bin clamps),
                     ranked there / overflowing TIECAP
  geo:h=1, geo:w=1, geo:K=HW, geo:w=4096   stage-1 geometry;  win:corners  all four corners of a class are among K < h*w winners
  seam:halo-decides  without the halo row across a segment seam the K winners would differ
  in:hm-strided, in:head-strided   channel slices of wider tensors (batch stride > C*h*w)

THE ORDER NOBODY CONTROLS.  Inside a compacted stage-1 segment and inside a stage-2a output block the slot order is the order in
which waves reach an atomicAdd (npos / nwin / rslot).  Stage 2's threshold path ranks the maxima of the first 256 threads, thread t
owning slots t, t + 1024, ...: whether its filtered count n fits FCAP (rank) or not (radix) depends on that order.  The model takes
``order``: None = pixel order, else the seed of a permutation applied within every compacted segment and within every slice.
THE RULE: a case counts as reaching <x>:rank only if under order None and under every one of the 16 seeds n <= FCAP / 2; it counts
as reaching <x>:radix only if n > FCAP follows from the code whatever the order -- K > 256, where no thread can have rank K - 1
among 256 maxima, L stays 1 and n == total > FCAP.  Anything between is labelled <x>:rank-or-radix, which is not in the table.

THE REFERENCE (``reference``): 3x3 NMS as heat * (max_pool2d(heat) == heat) on the CPU, the exact total order (score descending,
flat index cls*h*w + pixel ascending) via np.lexsort, head gathers and the box arithmetic of decode.py:99-159 in float32.
``mutated`` gives the six wrong decodes a..f; MUTATION_CASE names the case that must tell each from the reference."""
import collections
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

# constexpr ints of decode.hip (tests/test_decode_paths_cpu.py reads them back from the source)
SEG_MAX, MAXK, FCAP, SLICE, SEL_U, SEL_BINS, TIECAP = 1024, 512, 4096, 8192, 8, 1024, 1024
NT = 1024                      # threads of a stage-2 / 2a workgroup
ORDER_SEEDS = tuple(range(16))

LABELS = collections.OrderedDict([
    ('s1:seg256', 'decode.hip pick_seg: fewer than 256 workgroups at 512-pixel segments'),
    ('s1:seg512', 'decode.hip pick_seg: 256 workgroups reached at 512 but not at 1024 pixels'),
    ('s1:seg1024', 'decode.hip pick_seg: SEG_MAX'),
    ('s1:all', 'decode_stage1_kernel: n <= K, the compacted list is the output'),
    ('s1:rank', 'decode_stage1_kernel: n > K, rank counting'),
    ('s1:ragged', 'decode_stage1_kernel: p_hi clipped to h*w'),
    ('s1:midrow', 'decode_stage1_kernel: p_lo % w != 0'),
    ('2a:hist', 'decode_stage2a_kernel: select_topk_regs returns K'),
    ('2a:few', 'decode_stage2a_kernel: rc == -1, keep_all'),
    ('2a:radix', 'decode_stage2a_kernel: rc == -2, radix_select_kth over the slice'),
    ('regs:hist', 'decode_stage2_kernel: in_regs, rc == K'),
    ('regs:bitonic', 'decode_stage2_kernel: in_regs, rc == -2, total <= FCAP'),
    ('regs:rank', 'decode_stage2_kernel: in_regs, rc == -2, threshold + rank counting over filt'),
    ('regs:radix', 'decode_stage2_kernel: in_regs, rc == -2, n > FCAP, radix_select_kth over the slots'),
    ('regs:slow', 'decode_stage2_kernel: in_regs, rc == -1, radix_select_kth over all pixels'),
    ('mem:bitonic', 'decode_stage2_kernel: !in_regs, total <= FCAP'),
    ('mem:rank', 'decode_stage2_kernel: !in_regs, threshold + rank counting'),
    ('mem:radix', 'decode_stage2_kernel: !in_regs, n > FCAP'),
    ('mem:slow', 'decode_stage2_kernel: !in_regs, total < K'),
    ('tie:s1:rank', 'decode_stage1_kernel: rank counting cuts between equal scores'),
    ('tie:regs:hist', 'select_topk_regs: the boundary-bin ranking cuts between equal scores'),
    ('tie:regs:bitonic', 'decode_stage2_kernel: the bitonic sort orders equal scores at the cut'),
    ('tie:regs:rank', 'decode_stage2_kernel: threshold + rank counting cut between equal scores'),
    ('tie:regs:radix', 'decode_stage2_kernel: the radix threshold of the slots cuts between equal scores'),
    ('tie:2a:radix', 'decode_stage2a_kernel: the radix threshold of a slice cuts between equal scores'),
    ('tie:mem:radix', 'decode_stage2_kernel: the radix threshold behind stage 2a cuts between equal scores'),
    ('sel:clamp:hist', 'decode.hip sel_bin: scores >= 1.0 clamped into bin 1023, ranked there'),
    ('sel:clamp:overflow', 'decode.hip sel_bin: more than TIECAP clamped keys in bin 1023'),
    ('geo:h=1', 'decode_stage1_kernel: no row above or below'),
    ('geo:w=1', 'decode_stage1_kernel: one pixel per row, seg + 2 rows staged'),
    ('geo:K=HW', 'decode.hip check: the smallest map K allows'),
    ('geo:w=4096', 'ct_decode: the widest accepted row, 72 KiB of LDS'),
    ('win:corners', 'decode_stage1_kernel / key_from_map: the 3x3 window clipped on two sides'),
    ('seam:halo-decides', 'decode_stage1_kernel: r_lo = y_lo - 1, r_hi = y_hi + 1'),
    ('in:hm-strided', 'ct_decode: hm_batch_stride'),
    ('in:head-strided', 'ct_decode: head_batch_stride'),
])
# a label of the cross product stage 2 x (hist, bitonic, rank, radix, slow) that no input can reach, with the reason
UNREACHABLE = {'mem:hist': 'select_topk_regs needs the keys in registers: M2 <= SEL_U * 1024'}


def cdiv(a, b):
    return -(-a // b)


def schedule(B, C, h, w, K):
    HW = h * w
    seg = SEG_MAX
    while seg > 256 and B * C * cdiv(HW, seg) < 256:
        seg >>= 1
    nseg = cdiv(HW, seg)
    M2 = C * nseg * K
    G = 0 if M2 <= SLICE else cdiv(M2, SLICE)
    return dict(seg=seg, nseg=nseg, M2=M2, G=G, slots2=G * K if G else M2, bytes=(B * M2 + B * G * K) * 8)


# ---------------------------------------------------------------------------------------------------------------------
# keys

def nms(hm):
    t = torch.from_numpy(np.array(hm, np.float32))
    return (t * (F.max_pool2d(t, 3, 1, 1) == t).float()).numpy()


def f2ord(s):
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keys_of(flat_scores):
    idx = np.arange(flat_scores.size, dtype=np.uint64)
    return (f2ord(flat_scores).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)


def key_score(k):
    o = (np.asarray(k, np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(np.float32)


def _desc(a):
    return np.sort(a)[::-1]


# ---------------------------------------------------------------------------------------------------------------------
# the model

def _live_first(rows, rng):
    """every row's non-zero keys first: in slot order (rng None) or in a random order"""
    dead = rows == 0
    if rng is None:
        o = np.argsort(dead, axis=1, kind='stable')
    else:
        r = rng.random(rows.shape)
        r[dead] = 2.0
        o = np.argsort(r, axis=1)
    return np.take_along_axis(rows, o, 1)


def _stage1(s, K, seg, rng, labels):
    """s [C,HW] NMS'd scores of one image -> the image's M2 slots, final-form keys (class in the index: stage 2 / 2a add it)"""
    C, HW = s.shape
    nseg = cdiv(HW, seg)
    keys = np.where(s.reshape(-1) > 0, keys_of(s.reshape(-1)), np.uint64(0)).reshape(C, HW)
    keys = np.pad(keys, ((0, 0), (0, nseg * seg - HW))).reshape(C * nseg, seg)
    n = (keys != 0).sum(1)
    ranked = n > K
    srt = np.sort(keys, axis=1)[:, ::-1]
    width = min(K, seg)
    slots = np.zeros((C * nseg, K), np.uint64)
    slots[:, :width] = np.where(ranked[:, None], srt[:, :width], _live_first(keys, rng)[:, :width])
    if (~ranked).any():
        labels.add('s1:all')
    if ranked.any():
        labels.add('s1:rank')
        r = srt[ranked]
        if ((r[:, K - 1] >> np.uint64(32)) == (r[:, K] >> np.uint64(32))).any():
            labels.add('tie:s1:rank')
    return slots.reshape(-1)


def _select(live, K):
    """select_topk_regs on the non-zero keys ``live``: (rc, clamped) with rc 'hist' / 'few' / 'overflow'"""
    if live.size < K:
        return 'few', False
    sc = key_score(live)
    bins = np.clip((sc * np.float32(SEL_BINS)).astype(np.int64), 0, SEL_BINS - 1)
    hist = np.bincount(bins, minlength=SEL_BINS)
    incl = np.cumsum(hist[::-1])[::-1]
    bstar = int(np.nonzero(incl >= K)[0].max())
    clamped = bstar == SEL_BINS - 1 and bool((sc[bins == bstar] >= 1.0).any())
    return ('overflow' if hist[bstar] > TIECAP else 'hist'), clamped


def _cut_is_tied(live, K):
    if live.size <= K:
        return False
    d = _desc(live)
    return bool((d[K - 1] >> np.uint64(32)) == (d[K] >> np.uint64(32)))


def _stage2a(slots, K, rng, labels):
    out = []
    for lo in range(0, slots.size, SLICE):
        sl = slots[lo:lo + SLICE]
        live = sl[sl != 0]
        rc, clamped = _select(live, K)
        end = '2a:' + {'hist': 'hist', 'few': 'few', 'overflow': 'radix'}[rc]
        labels.add('tie:' + end if _cut_is_tied(live, K) else end)
        if clamped:
            labels.add('sel:clamp:' + ('hist' if rc == 'hist' else 'overflow'))
        keep = live if rc == 'few' else _desc(live)[:K]
        block = np.zeros((1, K), np.uint64)
        block[0, :keep.size] = keep
        out.append(_live_first(block, rng)[0] if rng is not None else block[0])
    return np.concatenate(out)


def _threshold_count(slots, K):
    """n of decode_stage2_kernel's threshold path: keys >= the K-th largest of the first 256 threads' maxima (L = 1 without one)"""
    pad = cdiv(slots.size, NT) * NT - slots.size
    lmax = np.pad(slots, (0, pad)).reshape(-1, NT).max(0)[:256]
    top = _desc(lmax[lmax != 0])
    L = top[K - 1] if top.size >= K else np.uint64(1)
    return int(((slots >= L) & (slots != 0)).sum())


def _stage2(slots, K, labels, info):
    live = slots[slots != 0]
    info['total'] = int(live.size)
    where = 'regs' if slots.size <= SEL_U * NT else 'mem'
    if where == 'regs':
        rc, clamped = _select(live, K)
        if clamped:
            labels.add('sel:clamp:' + ('hist' if rc == 'hist' else 'overflow'))
        if rc == 'hist':
            return 'regs:hist'
        if rc == 'few':
            return 'regs:slow'
    if live.size < K:
        return where + ':slow'
    if live.size <= FCAP:
        return where + ':bitonic'
    info['n'] = _threshold_count(slots, K)
    return where + ':threshold'


def nms_without_halo(hm_b, seg):
    """mutation d: every stage-1 segment sees the rows it has pixels in and no halo row"""
    C, h, w = hm_b.shape
    t = torch.from_numpy(np.array(hm_b, np.float32))
    out = np.empty((C, h * w), np.float32)
    for p_lo in range(0, h * w, seg):
        p_hi = min(h * w, p_lo + seg)
        y_lo, y_hi = p_lo // w, (p_hi - 1) // w
        sub = t[:, y_lo:y_hi + 1]
        kept = (sub * (F.max_pool2d(sub[None], 3, 1, 1)[0] == sub).float()).reshape(C, -1).numpy()
        out[:, p_lo:p_hi] = kept[:, p_lo - y_lo * w:p_hi - y_lo * w]
    return out.reshape(C, h, w)


def select(scores, K, cls_desc=False, pix_desc=False):
    """flat indices of the K first of [C,HW] scores in the order (score descending, class, pixel)"""
    C, HW = scores.shape
    flat = scores.reshape(-1)
    cand = np.arange(flat.size)
    if flat.size > 4 * K:                                    # (only what reaches the K-th score can be among the first K)
        cand = np.nonzero(flat >= np.partition(flat, flat.size - K)[flat.size - K])[0]
    cls, pix = np.divmod(cand, HW)
    return cand[np.lexsort((-pix if pix_desc else pix, -cls if cls_desc else cls, -flat[cand]))[:K]]


def image_paths(hm_b, B, K, order=None, strided=(), kernels_only=False):
    """(labels, info) of one image [C,h,w] decoded as part of a batch of B; ``kernels_only`` leaves out the labels that do not
    depend on ``order``"""
    C, h, w = hm_b.shape
    sch = schedule(B, C, h, w, K)
    seg, HW = sch['seg'], h * w
    rng = None if order is None else np.random.default_rng(order)
    labels = {'s1:seg%d' % seg} | {'in:%s-strided' % s for s in strided}
    info = dict(sch)
    if HW % seg:
        labels.add('s1:ragged')
    if any(p % w for p in range(0, HW, seg)):
        labels.add('s1:midrow')
    for name, hit in (('geo:h=1', h == 1), ('geo:w=1', w == 1), ('geo:K=HW', K == HW), ('geo:w=4096', w == 4096)):
        if hit:
            labels.add(name)
    s = nms(hm_b[None])[0].reshape(C, HW)
    slots = _stage1(s, K, seg, rng, labels)
    if sch['G']:
        slots = _stage2a(slots, K, rng, labels)
    end = _stage2(slots, K, labels, info)
    info['end'] = end
    info['tied'] = _cut_is_tied(slots[slots != 0], K)
    labels.add('tie:' + end if info['tied'] and not end.endswith(':slow') and not end.endswith(':threshold') else end)
    if kernels_only:
        return labels, info
    win = select(s, K)
    corners = np.array([0, w - 1, HW - w, HW - 1])
    if K < HW and any(np.isin(c * HW + corners, win).all() for c in range(C)):
        labels.add('win:corners')
    if sorted(select(nms_without_halo(hm_b, seg).reshape(C, HW), K)) != sorted(win):
        labels.add('seam:halo-decides')
    return labels, info


# ---------------------------------------------------------------------------------------------------------------------
# the reference and its mutations

def _strict_nms(hm):
    """mutation c: a pixel is kept only where it is the ONLY maximum of its window"""
    t = torch.from_numpy(np.array(hm, np.float32))
    B, C, h, w = t.shape
    pad = F.pad(t, (1, 1, 1, 1), value=float('-inf'))
    n_ge = sum((pad[:, :, dy:dy + h, dx:dx + w] >= t).float() for dy in range(3) for dx in range(3))
    return (t * (n_ge == 1).float()).numpy()


def gather_rows(heads, b, pix, xs0, ys0):
    """decode.py:99-159 for one image in float32: the fields of the packed row that follow (score, cls, xs0, ys0)"""
    out = {}
    HW = next(iter(heads.values())).shape[2] * next(iter(heads.values())).shape[3] if heads else 0

    def at(name):
        return heads[name][b].reshape(heads[name].shape[1], HW)[:, pix].T.astype(np.float32)          # [K, ch]
    half, two = np.float32(0.5), np.float32(2)
    xs, ys = xs0 + half, ys0 + half
    if 'reg' in heads:
        reg = at('reg')
        xs, ys = xs0 + reg[:, 0], ys0 + reg[:, 1]
    if 'wh' in heads:
        wh = np.maximum(at('wh'), np.float32(0))
        out['bboxes'] = np.stack([xs - wh[:, 0] / two, ys - wh[:, 1] / two, xs + wh[:, 0] / two, ys + wh[:, 1] / two], 1)
    for name, key in (('ltrb', 'bboxes'), ('ltrb_amodal', 'bboxes_amodal')):
        if name in heads:
            v = at(name)
            out[key] = np.stack([xs0 + v[:, 0], ys0 + v[:, 1], xs0 + v[:, 2], ys0 + v[:, 3]], 1)
    if 'ltrb_amodal' in heads:
        out['bboxes'] = out['bboxes_amodal']
    for name in ('tracking', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity'):
        if name in heads:
            out[name] = at(name)
    return out


def decode_with(hm, heads, K, mutation=None, B_sched=None):
    """the reference decode of hm [B,C,h,w] (numpy float32) -> dict of [B,K,...] arrays; ``mutation`` in 'a'..'f' or None"""
    B, C, h, w = hm.shape
    HW = h * w
    if mutation == 'c':
        s = _strict_nms(hm)
    elif mutation == 'd':
        seg = schedule(B if B_sched is None else B_sched, C, h, w, K)['seg']
        s = np.stack([nms_without_halo(hm[b], seg) for b in range(B)])
    else:
        s = nms(hm)
    rows = collections.defaultdict(list)
    for b in range(B):
        sb = s[b].reshape(C, HW)
        if mutation == 'e':                                  # per-class top K, the scores tied across the cut dropped
            sb = sb.copy()
            for c in range(C):
                o = select(sb[c:c + 1], HW)
                if HW > K and sb[c, o[K - 1]] == sb[c, o[K]]:
                    sb[c, sb[c] == sb[c, o[K]]] = -1.0
                sb[c, o[K:]] = -1.0
        win = select(sb, K + 1 if mutation == 'f' else K, cls_desc=mutation == 'b', pix_desc=mutation == 'a')
        if mutation == 'f':
            win = np.concatenate([win[:K - 1], win[K:]])
        cls, pix = np.divmod(win, HW)
        xs0, ys0 = (pix % w).astype(np.float32), (pix // w).astype(np.float32)
        rows['inds'].append(pix.astype(np.int64))
        rows['scores'].append(sb.reshape(-1)[win])
        rows['clses'].append(cls.astype(np.float32))
        rows['xs'].append(xs0)
        rows['ys'].append(ys0)
        for k, v in gather_rows(heads, b, pix, xs0, ys0).items():
            rows[k].append(v)
    return {k: np.stack(v) for k, v in rows.items()}


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@contextlib.contextmanager
def documented_tie_order():
    """oracle.decode with torch.topk replaced by the documented order: score descending, then lower index (the oracle's
    second top-K runs over [class][rank], so lower class comes first).  Where scores are distinct it changes nothing."""
    real = torch.topk

    def topk(x, k, *a, **kw):
        idx = torch.from_numpy(np.argsort(-x.numpy(), axis=-1, kind='stable')[..., :k].copy())
        return x.gather(-1, idx), idx
    torch.topk = topk
    try:
        yield
    finally:
        torch.topk = real


# ---------------------------------------------------------------------------------------------------------------------
# heat maps

def _distinct(rng, shape):
    """distinct float32 values in (0, 1): a permutation of an arithmetic sequence"""
    n = int(np.prod(shape))
    return ((rng.permutation(n).astype(np.float64) + 1) / (n + 1)).reshape(shape)


def _per_image(fn):
    """B > 1: a different seed per image"""
    def make(case):
        return np.stack([fn(case, np.random.default_rng([case.seed, b])) for b in range(case.B)]).astype(np.float32)
    return make


@_per_image
def random_map(case, rng):
    return _distinct(rng, (case.C, case.h, case.w)) * 0.98 + 0.001


@_per_image
def clustered_map(case, rng):
    """a peak on every other pixel, both ways, all inside histogram bin 615: distinct float32 values by construction (int32 bit
    patterns 2 apart; the bin is 16384 patterns wide)"""
    hm = (_distinct(rng, (case.C, case.h, case.w)) * 0.3).astype(np.float32)
    ph, pw = (case.h + 1) // 2, (case.w + 1) // 2
    assert 2 * case.C * ph * pw < 16384
    rank = rng.permutation(case.C * ph * pw).astype(np.int32).reshape(case.C, ph, pw)
    base = np.full((case.C, ph, pw), 615.0 / 1024.0, np.float32)
    hm[:, 0::2, 0::2] = (base.view(np.int32) + 2 * rank).view(np.float32)
    return hm


def isolated_peaks(npeaks):
    @_per_image
    def make(case, rng):
        hm = np.zeros((case.C, case.h, case.w), np.float32)
        cy, cx = (case.h + 2) // 3, (case.w + 2) // 3
        cell = rng.permutation(case.C * cy * cx)[:npeaks]
        c, r = np.divmod(cell, cy * cx)
        hm[c, 3 * (r // cx), 3 * (r % cx)] = (_distinct(rng, (npeaks,)) * 0.9 + 0.05).astype(np.float32)
        return hm
    return make


def constant_map(case):
    return np.full((case.B, case.C, case.h, case.w), 0.5, np.float32)


@_per_image
def saturated_map(case, rng):
    """30 % of the pixels exactly 1.0f"""
    hm = (_distinct(rng, (case.C, case.h, case.w)) * 0.98 + 0.001).astype(np.float32)
    hm[rng.random(hm.shape) < 0.3] = 1.0
    return hm


@_per_image
def over_range_map(case, rng):
    return _distinct(rng, (case.C, case.h, case.w)) * 3.0


@_per_image
def seam_map(case, rng):
    """17 x 30, 256-pixel segments: the seam lies inside row 8 between columns 15 and 16"""
    assert (case.h, case.w) == (17, 30)
    hm = (_distinct(rng, (case.C, case.h, case.w)) * 0.1).astype(np.float32)
    hm[0, 8, 15] = hm[0, 8, 16] = 0.9          # equal neighbours on either side of the seam: both survive
    hm[0, 8, 10] = hm[0, 9, 10] = 0.8          # ... and across the seam between a segment's last row and the halo
    hm[0, 8, 5], hm[0, 9, 6] = 0.7, 0.75       # its only larger neighbour lies in the next segment's first row: suppressed
    hm[0, 8, 22], hm[0, 7, 23] = 0.6, 0.65     # ... in the previous segment's last row: suppressed
    return hm


@_per_image
def border_map(case, rng):
    hm = (_distinct(rng, (case.C, case.h, case.w)) * 0.1).astype(np.float32)
    h, w = case.h, case.w
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    for c in range(case.C):
        for i, (y, x) in enumerate(spots):
            hm[c, y, x] = 0.95 - 0.05 * i - 0.01 * c
    return hm


def legacy_cluster(case):
    """tests/test_hip_ops.py::test_decode_selection_paths_full_size, dense == 'cluster', restated value for value"""
    name, B, C, h, w = case.name, case.B, case.C, case.h, case.w
    g = torch.Generator().manual_seed(len(name) * 131 + C)
    n = B * C * h * w
    distinct = ((torch.randperm(n, generator=g).double() + 1) / (n + 1)).view(B, C, h, w)
    hm = (distinct * 0.2).float()
    ph, pw = (h + 2) // 3, (w + 2) // 3
    for c in range(C):
        rank = torch.randperm(B * ph * pw, generator=g).double().view(B, ph, pw)
        hm[:, c, 0::3, 0::3] = ((300 + 10 * c) / 1024.0 + 1e-5 + 2e-7 * rank).float()
    return hm.numpy()


Case = collections.namedtuple('Case', 'name B C h w K make seed heads strided distinct why')


def _case(name, B, C, h, w, K, make, why, heads=('reg', 'wh', 'tracking'), strided=(), distinct=True):
    return Case(name, B, C, h, w, K, make, sum(map(ord, name)), heads, strided, distinct, why)


NUSC_HEADS = ('reg', 'wh', 'ltrb_amodal', 'tracking', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity')
HEAD_CH = dict(reg=2, wh=2, tracking=2, ltrb=4, ltrb_amodal=4, dep=1, rot=8, dim=3, amodel_offset=2, nuscenes_att=8, velocity=3)

CASES = [
    # every end of stage 2 beyond regs:hist, with distinct scores and with none
    _case('regs_rank', 1, 1, 160, 160, 80, clustered_map, 'seg 256, M2 8000, rc -2, 6400 candidates: threshold + rank counting'),
    _case('regs_radix', 10, 1, 144, 192, 300, clustered_map, 'seg 1024, M2 8100, 6912 candidates, K > 256: the radix fallback of stage 2'),
    _case('mem_rank', 1, 80, 144, 144, 200, random_map, 'G 42, stage 2 reads 8400 slots from memory; the last slice keeps all'),
    _case('mem_radix', 1, 80, 64, 64, 512, random_map, 'G 20, 10240 slots, K > 256'),
    _case('mem_bitonic', 1, 80, 144, 144, 200, isolated_peaks(1500), '1500 candidates behind stage 2a'),
    _case('mem_slow', 1, 80, 144, 144, 200, isolated_peaks(50), '50 candidates behind stage 2a'),
    _case('const_160', 1, 1, 160, 160, 80, constant_map, '8000 tied keys: every path orders by index alone', distinct=False),
    _case('const_small', 1, 2, 20, 24, 40, constant_map, 'the boundary-bin ranking by index alone', distinct=False),
    # ... and the radix thresholds of stage 2 and stage 2a, which the table above reaches with distinct scores only
    _case('const_radix', 10, 1, 144, 192, 300, constant_map, '8100 tied keys per image, K > 256: the radix threshold by index alone', distinct=False),
    _case('const_mem', 1, 80, 64, 64, 512, constant_map, '20 slices of 8192 tied keys, then 10240: both radix thresholds by index alone', distinct=False),
    # the owners of 2a:radix and regs:bitonic stay where they are: tests/test_hip_ops.py::test_decode_selection_paths_full_size
    _case('cluster_mot', 1, 1, 128, 128, 100, legacy_cluster, 'every score in one bin, ~1850 candidates'),
    _case('cluster_coco', 2, 20, 128, 128, 100, legacy_cluster, 'every class in one bin: the radix fallback of stage 2a'),
    # scores at and past the top of the histogram
    _case('saturated', 1, 1, 64, 64, 100, saturated_map, 'more than TIECAP keys of exactly 1.0f in bin 1023', distinct=False),
    _case('over_range', 1, 1, 48, 48, 50, over_range_map, 'scores up to 3.0 clamped into bin 1023 and ranked there'),
    # stage-1 geometry
    _case('seam_17x30', 1, 1, 17, 30, 12, seam_map, 'mid-row seam, ragged tail, plateaus and suppression across the seam', distinct=False),
    _case('row_1x600', 1, 2, 1, 600, 30, random_map, 'h == 1'),
    _case('col_600x1', 1, 2, 600, 1, 30, random_map, 'w == 1'),
    _case('all_3x3', 2, 1, 3, 3, 9, random_map, 'K == h*w'),
    _case('wide_2x4096', 1, 1, 2, 4096, 16, random_map, 'w == 4096'),
    _case('seg_512', 1, 16, 90, 100, 20, random_map, '288 workgroups at 512 pixels, 144 at 1024'),
    _case('borders', 2, 2, 13, 21, 16, border_map, 'peaks on all four corners and borders', heads=NUSC_HEADS),
    _case('strided', 2, 3, 20, 24, 8, random_map, 'hm and wh are channel slices of wider tensors', strided=('hm', 'head')),
]
CASE = {c.name: c for c in CASES}

# the maps the reuse tests refill a built Decoder with: (shape of, map, the stage-2 end the model must give)
REUSE = {
    'regs': ('regs_radix', [(clustered_map, 'regs:radix'), (isolated_peaks(20), 'regs:slow'), (random_map, 'regs:hist')]),
    'mem': ('mem_radix', [(random_map, 'mem:radix'), (isolated_peaks(50), 'mem:slow'), (isolated_peaks(1500), 'mem:bitonic')]),
}

MUTATIONS = {
    'a': 'ties broken by the higher pixel',
    'b': 'ties broken by the higher class',
    'c': 'NMS with a strict maximum (plateaus dropped)',
    'd': 'NMS without the halo row across a segment seam',
    'e': 'per-class top K truncated to K before the global merge, ties dropped at the cut',
    'f': 'the K-th winner replaced by the (K+1)-th',
}
MUTATION_CASE = {'a': 'const_160', 'b': 'const_small', 'c': 'seam_17x30', 'd': 'seam_17x30', 'e': 'saturated', 'f': 'regs_radix'}


@functools.lru_cache(maxsize=None)
def heat_map(name):
    case = CASE[name]
    hm = np.ascontiguousarray(case.make(case), np.float32)
    assert hm.shape == (case.B, case.C, case.h, case.w) and (hm >= 0).all()
    hm.setflags(write=False)
    return hm


@functools.lru_cache(maxsize=None)
def head_maps(name):
    case = CASE[name]
    rng = np.random.default_rng([case.seed, 1000])
    out = collections.OrderedDict()
    for hd in case.heads:
        shape = (case.B, HEAD_CH[hd], case.h, case.w)
        # reg in (0, 1), wh in (-1, 8) (negative sizes are clipped, decode.py:117), the rest N(0, 2)
        v = rng.random(shape) if hd == 'reg' else rng.random(shape) * 9 - 1 if hd == 'wh' else rng.standard_normal(shape) * 2
        out[hd] = v.astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    case = CASE[name]
    return decode_with(heat_map(name), head_maps(name), case.K)


def mutated(name, mutation):
    case = CASE[name]
    return decode_with(heat_map(name), head_maps(name), case.K, mutation)


def paths_of(hm, K, order=None, strided=()):
    """[(labels, info)] per image of hm [B,C,h,w]"""
    return [image_paths(hm[b], hm.shape[0], K, order, strided) for b in range(hm.shape[0])]


def classify_threshold(hm, K):
    """the order rule of the module docstring for every image that ends in the threshold path: {image: (label, [n per order])}"""
    out = {}
    first = paths_of(hm, K)
    for b, (labels, info) in enumerate(first):
        if not info['end'].endswith(':threshold'):
            continue
        ns = [info['n']] + [image_paths(hm[b], hm.shape[0], K, seed, kernels_only=True)[1]['n'] for seed in ORDER_SEEDS]
        where = info['end'].split(':')[0]
        if K > 256 and info['total'] > FCAP:
            kind = 'radix'
        elif max(ns) <= FCAP // 2:
            kind = 'rank'
        else:
            kind = 'rank-or-radix'
        out[b] = (where + ':' + kind, ns)
    return out, first


@functools.lru_cache(maxsize=None)
def case_labels(name):
    """(the labels the case reaches in any of its images, {image: info}): the threshold path resolved by the order rule"""
    case = CASE[name]
    hm = heat_map(name)
    thr, first = classify_threshold(hm, case.K)
    labels, infos = set(), {}
    for b, (lab, info) in enumerate(first):
        lab = set(lab)
        if b in thr:
            lab.discard(info['end'])
            end, ns = thr[b]
            lab.add('tie:' + end if info['tied'] else end)
            info = dict(info, end=end, ns=ns)
        labels |= lab
        infos[b] = info
    return frozenset(labels | {'in:%s-strided' % s for s in case.strided}), infos


def owners(cases=None):
    """{label: [names of the cases that reach it]}"""
    out = collections.OrderedDict((k, []) for k in LABELS)
    for c in (CASES if cases is None else cases):
        for lab in case_labels(c.name)[0]:
            out.setdefault(lab, []).append(c.name)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the pose case: a Decoder with hps and hm_hp at 24 x 40, B = 2, K = 40, no offset head (centres and peaks at +0.5, so the
# designed coordinates are exact)

POSE = dict(B=2, h=24, w=40, K=40, J=17)
# image 0: detection 0 at (x 10, y 10), wh (12, 12): gate box 4.5 .. 16.5 both ways; detection 1 at (x 20, y 2), wh (10, 6):
# gate box x 15.5 .. 25.5, y -0.5 .. 5.5
POSE_WANT = {        # (detection, joint): (the key point the reference must give, what decides it)
    (0, 0): ((12.0, 10.0), 'pose:thresh-equal: the only peak near scores exactly 0.2f, not strong (s > 0.2): regressed joint kept'),
    (0, 1): ((4.5, 10.5), 'pose:gate-edge: a strong peak exactly on the left edge (hx < bl is false): snapped'),
    (0, 2): ((12.5, 10.5), 'pose:equidistant: two strong peaks at distance 2, the earlier (higher score) wins like torch.min'),
    (0, 3): ((13.5, 13.5), 'pose:joint-slow: 5 positive peaks < K, the joint decode takes the slow path, zero-score peaks dropped'),
    (1, 4): ((20.5, 0.5), 'pose:joint-ties: a constant joint map, its K peaks are the K lowest pixels'),
}


@functools.lru_cache(maxsize=None)
def pose_maps():
    B, h, w, K, J = (POSE[k] for k in ('B', 'h', 'w', 'K', 'J'))
    rng = np.random.default_rng(4040)
    hm = (_distinct(rng, (B, 1, h, w)) * 0.9).astype(np.float32)
    wh = (rng.random((B, 2, h, w)) * 9 + 1).astype(np.float32)
    hps = (rng.standard_normal((B, 2 * J, h, w)) * 3).astype(np.float32)
    hm_hp = _distinct(rng, (B, J, h, w)).astype(np.float32)
    hm[0, 0, 10, 10], hm[0, 0, 2, 20] = 0.99, 0.98
    wh[0, :, 10, 10], wh[0, :, 2, 20] = (12.0, 12.0), (10.0, 6.0)
    weak = lambda: (_distinct(rng, (h, w)) * 0.15).astype(np.float32)
    hm_hp[0, 0] = weak()
    hm_hp[0, 0, 10, 12] = np.float32(0.2)
    hps[0, 0:2, 10, 10] = (2.0, 0.0)
    hm_hp[0, 1] = weak()
    hm_hp[0, 1, 10, 4] = 0.8
    hps[0, 2:4, 10, 10] = (-5.0, 1.0)
    hm_hp[0, 2] = weak()
    hm_hp[0, 2, 10, 12], hm_hp[0, 2, 10, 8] = 0.7, 0.6
    hps[0, 4:6, 10, 10] = (0.5, 0.5)
    hm_hp[0, 3] = 0.0
    for (y, x), v in zip(((13, 13), (3, 30), (20, 5), (21, 33), (5, 25)), (0.9, 0.8, 0.7, 0.6, 0.5)):
        hm_hp[0, 3, y, x] = v
    hps[0, 6:8, 10, 10] = (3.0, 3.0)
    hm_hp[0, 4] = 0.5
    hps[0, 8:10, 2, 20] = (0.2, -1.7)
    maps = collections.OrderedDict([('hm', hm), ('wh', wh), ('hps', hps), ('hm_hp', hm_hp)])
    for v in maps.values():
        v.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def pose_reference():
    """oracle.decode.generic_decode per image as tests/test_hip_ops.py::test_decode_pose_branch_variants uses it, under the
    documented tie order"""
    from oracle import decode as odecode
    with documented_tie_order():
        want = odecode.generic_decode({k: torch.from_numpy(v.copy()) for k, v in pose_maps().items()}, K=POSE['K'], return_inds=True)
    return {k: v.numpy() for k, v in want.items()}
