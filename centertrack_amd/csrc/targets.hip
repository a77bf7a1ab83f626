// Training targets on the device: the dense maps and the slot tensors of a training batch from
// the compact per-sample records of centertrack_amd/targets.py, in ONE launch behind ONE host-to-device copy.
//
// What the reference does per sample in a DataLoader worker (src/lib/dataset/generic_dataset.py:205-255, 330-515:
// zero-fill hm [C,h,w] and pre_hm [1,H,W], splat one Gaussian per object with numpy, collate, .to(device)) splits here:
// the scalar per-object arithmetic stays on the host (TargetBuilder.encode) and yields blob / rectangle / slot lists;
// this file turns the lists of a whole batch into every tensor of the batch.
//
// Dense part: render_pre_hm_kernel's scheme (elementwise.hip) generalised.  A workgroup owns a 32x8 pixel tile of one
// plane of one image -- the C class planes at output resolution, then the one pre_hm plane at input resolution.  It culls
// the image's blobs against (plane, tile) into LDS with wave ballots, CULL_CAP at a time (the number of blobs is not
// bounded), and each pixel takes max over the survivors of float32(exp(-(dx^2+dy^2) / (2 sigma^2)) * conf), sigma =
// (2r+1)/6, in float64 like numpy; then the same for the ignore rectangles (a pixel inside one is 1).  max is
// commutative and both only ever raise a value, so the order of the reference's loop does not matter.
// Slot part: one thread per output element of every slot tensor; a hole (slot map -1) is 0.
// Every output element is written exactly once by one thread: no memset, no atomics on global memory, no
// read-modify-write; outputs may hold garbage beforehand and two calls agree in every bit.
//
// Pose (ct_build_pose_targets): hm_hp [B,J,h,w] is J more planes of the output grid behind the C
// class planes, numbered C .. C+J-1 in the blob and rectangle lists; rectangle code -2 covers all of them (-1: all class
// planes).  The reference (generic_dataset.py:541-553, :396-398) draws one Gaussian per visible joint, writes
// hm_hp[j, y, x] = 1 at a visibility-1 joint -- where the Gaussian's peak already is 1 -- and raises the object's box
// to 1 on the plane of an unlabelled joint, so hm_hp is the max over Gaussians and rectangles like hm and the order
// does not matter here either.  The joint tensors [B, max_objs*J, ..] are [B, max_objs, J ..] in memory: plain
// columns of a slot row, written by the slot part unchanged.  The kernel is a template on POSE, so that the launch of
// ct_build_targets carries none of it.
#include <stdint.h>

#include "ct_common.h"

namespace {

constexpr int TGT_TW = 32, TGT_TH = 8, TGT_CAP = CT_TARGETS_CULL_CAP;
constexpr int TGT_MAX_RADIUS = 16384;          // dx^2 + dy^2 <= 2^29 stays an int
constexpr int TGT_MAX_CENTRE = 1 << 28;        // cx +- r stays an int

struct TgtArgs {
    const int *buf;
    float *hm, *pre, *hp;
    int B, C, J, h, w, H, W, max_objs, S;
    int hmTilesX, hmTilesY, preTilesX, preTilesY;
    unsigned hmBlocks, hpBlocks, preBlocks;
    int map_off, col_off, tab_off;
    long long slotElems;
};

// append the items of the lanes with `hit` to the LDS list (wave ballot: one LDS atomic per wave)
__device__ __forceinline__ void tgt_push(bool hit, int a, int b, int c, int d, int *item, int *nitem)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long mask = __ballot(hit);
    int base = 0;
    if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) base = atomicAdd(nitem, (int)__popcll(mask));
        base = __shfl(base, leader);
    }
    if (hit) {
        const int s = base + (int)__popcll(mask & ((1ull << lane) - 1ull));
        item[4 * s] = a; item[4 * s + 1] = b; item[4 * s + 2] = c; item[4 * s + 3] = d;
    }
}

template <bool POSE>
__global__ __launch_bounds__(256) void build_targets_kernel(TgtArgs a)
{
    __shared__ int item[TGT_CAP * 4];
    __shared__ int nitem;
    const int *buf = a.buf;
    unsigned bid = blockIdx.x;
    const unsigned hpBlocks = POSE ? a.hpBlocks : 0u;
    if (bid >= a.hmBlocks + hpBlocks + a.preBlocks) {
        // ---- slot tensors: element e = ((b * max_objs + k) * S + column)
        const long long e = (long long)(bid - a.hmBlocks - hpBlocks - a.preBlocks) * 256 + threadIdx.x;
        if (e >= a.slotElems) return;
        const int c = (int)(e % a.S);
        const long long bk = e / a.S;
        const int b = (int)(bk / a.max_objs);
        const int *tab = buf + a.tab_off + 4 * buf[a.col_off + c];
        const unsigned long long ptr = (unsigned long long)(unsigned)tab[0] | ((unsigned long long)(unsigned)tab[1] << 32);
        if (!ptr) return;                       // a tensor the caller did not ask for
        const int col0 = tab[2] & 0xffff, width = tab[2] >> 16;
        const int row = buf[a.map_off + bk];
        const int word = row < 0 ? 0 : buf[(size_t)buf[8 * b] + (size_t)row * a.S + c];
        const size_t o = (size_t)bk * width + (c - col0);
        if (tab[3]) ((long long *)ptr)[o] = (long long)word;
        else ((int *)ptr)[o] = word;
        return;
    }
    // ---- dense maps
    // (workgroups: the hm planes of every image, then -- POSE -- the hm_hp planes, then pre_hm)
    const bool isHp = POSE && bid >= a.hmBlocks && bid < a.hmBlocks + hpBlocks;
    const bool isPre = bid >= a.hmBlocks + hpBlocks;
    int tilesX, tilesY, Hm, Wm, plane;
    if (isPre) { bid -= a.hmBlocks + hpBlocks; tilesX = a.preTilesX; tilesY = a.preTilesY; Hm = a.H; Wm = a.W; }
    else { if (isHp) bid -= a.hmBlocks; tilesX = a.hmTilesX; tilesY = a.hmTilesY; Hm = a.h; Wm = a.w; }
    const int tx = bid % tilesX; bid /= tilesX;
    const int ty = bid % tilesY; bid /= tilesY;
    int b;
    if (isPre) { plane = 0; b = (int)bid; }
    else if (isHp) { plane = a.C + (int)(bid % a.J); b = (int)(bid / a.J); }
    else { plane = bid % a.C; b = (int)(bid / a.C); }
    const int *hdr = buf + 8 * b;
    const int x0 = tx * TGT_TW, y0 = ty * TGT_TH;
    const int x = x0 + (threadIdx.x & (TGT_TW - 1)), y = y0 + (threadIdx.x / TGT_TW);
    float v = 0.0f;
    // Gaussians: hm blobs are (plane, cx, cy, r) with conf 1, pre_hm blobs (cx, cy, r, conf)
    const int *p = buf + (isPre ? hdr[6] : hdr[2]);
    const int n = isPre ? hdr[7] : hdr[3];
    for (int c0 = 0; c0 < n; c0 += TGT_CAP) {
        const int c1 = min(n, c0 + TGT_CAP);
        if (threadIdx.x == 0) nitem = 0;
        __syncthreads();
        for (int i0 = c0; i0 < c1; i0 += 256) {
            const int i = i0 + threadIdx.x;
            int cx = 0, cy = 0, r = -1, conf = 0;
            bool ok = false;
            if (i < c1) {
                const int q0 = p[4 * i], q1 = p[4 * i + 1], q2 = p[4 * i + 2], q3 = p[4 * i + 3];
                if (isPre) { cx = q0; cy = q1; r = q2; conf = q3; ok = conf > 0; }
                else { cx = q1; cy = q2; r = q3; conf = 1; ok = q0 == plane; }
            }
            const bool hit = ok && r >= 0 && cx + r >= x0 && cx - r < x0 + TGT_TW && cy + r >= y0 && cy - r < y0 + TGT_TH;
            tgt_push(hit, cx, cy, r, conf, item, &nitem);
        }
        __syncthreads();
        const int m = nitem;
        for (int i = 0; i < m; ++i) {
            const int cx = item[4 * i], cy = item[4 * i + 1], r = item[4 * i + 2], conf = item[4 * i + 3];
            const int dx = x - cx, dy = y - cy;
            if (dx < -r || dx > r || dy < -r || dy > r) continue;
            const double sigma = (double)(2 * r + 1) / 6.0;
            const double g = exp(-(double)(dx * dx + dy * dy) / (2.0 * sigma * sigma));
            v = fmaxf(v, (float)(g * (double)conf));
        }
        __syncthreads();
    }
    if (!isPre) {
        // ignore rectangles (plane, -1 = all class planes or -2 = all hm_hp planes; x0, y0, x1, y1), corners inclusive
        const int all = isHp ? -2 : -1;
        const int *q = buf + hdr[4];
        const int nr = hdr[5];
        for (int c0 = 0; c0 < nr; c0 += TGT_CAP) {
            const int c1 = min(nr, c0 + TGT_CAP);
            if (threadIdx.x == 0) nitem = 0;
            __syncthreads();
            for (int i0 = c0; i0 < c1; i0 += 256) {
                const int i = i0 + threadIdx.x;
                int rx0 = 0, ry0 = 0, rx1 = -1, ry1 = -1;
                bool ok = false;
                if (i < c1) {
                    const int pl = q[5 * i];
                    rx0 = q[5 * i + 1]; ry0 = q[5 * i + 2]; rx1 = q[5 * i + 3]; ry1 = q[5 * i + 4];
                    ok = POSE ? (pl == all || pl == plane) : (pl < 0 || pl == plane);
                }
                const bool hit = ok && rx1 >= x0 && rx0 < x0 + TGT_TW && ry1 >= y0 && ry0 < y0 + TGT_TH;
                tgt_push(hit, rx0, ry0, rx1, ry1, item, &nitem);
            }
            __syncthreads();
            const int m = nitem;
            for (int i = 0; i < m; ++i)
                if (x >= item[4 * i] && x <= item[4 * i + 2] && y >= item[4 * i + 1] && y <= item[4 * i + 3]) v = 1.0f;
            __syncthreads();
        }
    }
    if (x >= Wm || y >= Hm) return;
    if (isPre) a.pre[((size_t)b * Hm + y) * Wm + x] = v;
    else if (isHp) a.hp[(((size_t)b * a.J + (plane - a.C)) * Hm + y) * Wm + x] = v;
    else a.hm[(((size_t)b * a.C + plane) * Hm + y) * Wm + x] = v;
}

// a list of `n` items of `stride` words at word `off` lies inside [lo, words)
bool list_ok(long long off, long long n, int stride, long long lo, long long words)
{
    return n >= 0 && off >= lo && off <= words && n <= (words - off) / stride;
}

#define TGT_FAIL(fmt, ...) CT_FAIL_ARG("%s: " fmt, fn, ##__VA_ARGS__)

// Both entry points.  `fn` names the caller in the messages.  pose: hm_hp [B,J,h,w] (may be null: not asked for) and
// J >= 0 planes behind the C class planes; the lists may then name planes [0, C + J) and, with J > 0, rectangle code -2.
int build_impl(const char *fn, const ct_targets_desc *d, bool pose, float *hm_hp, int J, void *stream)
{
    if (!d->staging_host || !d->staging_dev) TGT_FAIL("null staging pointer");
    if (d->B <= 0 || d->max_objs <= 0 || d->slot_words <= 0 || d->slot_words > 0xffff || d->nout <= 0 ||
        d->nout > CT_TARGETS_MAX_OUT)
        TGT_FAIL("bad sizes (B %d, max_objs %d, slot_words %d, nout %d)", d->B, d->max_objs, d->slot_words, d->nout);
    if (d->hm && (d->C <= 0 || d->h <= 0 || d->w <= 0)) TGT_FAIL("bad hm shape");
    if (d->pre_hm && (d->H <= 0 || d->W <= 0)) TGT_FAIL("bad pre_hm shape");
    if (pose) {
        if (J < 0 || J > 4096) TGT_FAIL("bad J %d", J);
        if (hm_hp && J <= 0) TGT_FAIL("hm_hp given with J %d", J);
        if (hm_hp && (d->C <= 0 || d->C > (1 << 20) || d->h <= 0 || d->w <= 0)) TGT_FAIL("bad hm_hp shape");
    }
    const bool planes = d->hm || hm_hp;            // the lists are read by plane
    const int P = d->C + J, all_lo = J > 0 ? -2 : -1;
    const int B = d->B, M = d->max_objs, S = d->slot_words;
    const long long words = (long long)d->words;
    const long long map_off = 8LL * B, col_off = map_off + (long long)B * M, tab_off = col_off + S;
    const long long payload = tab_off + 4LL * d->nout;
    if (words < payload || words >= (1LL << 30))
        TGT_FAIL("staging buffer of %lld words, the header alone takes %lld", words, payload);
    const int *s = d->staging_host;
    // the output table and the column map agree with each other
    bool any_slot = false;
    for (int t = 0; t < d->nout; ++t) {
        const int *tab = s + tab_off + 4 * t;
        const int col0 = tab[2] & 0xffff, width = tab[2] >> 16;
        if (width < 1 || col0 + width > S || (tab[3] != 0 && tab[3] != 1))
            TGT_FAIL("output %d: bad column range / element type", t);
        for (int c = col0; c < col0 + width; ++c)
            if (s[col_off + c] != t) TGT_FAIL("column %d is not mapped to output %d", c, t);
        any_slot = any_slot || tab[0] || tab[1];
    }
    for (int c = 0; c < S; ++c)
        if (s[col_off + c] < 0 || s[col_off + c] >= d->nout) TGT_FAIL("column %d maps to no output", c);
    if (!any_slot && !d->hm && !d->pre_hm && !hm_hp) TGT_FAIL("null pointer: no output tensor given");
    for (int b = 0; b < B; ++b) {
        const int *h = s + 8 * b;
        if (!list_ok(h[0], h[1], S, payload, words) || !list_ok(h[2], h[3], 4, payload, words) ||
            !list_ok(h[4], h[5], 5, payload, words) || !list_ok(h[6], h[7], 4, payload, words))
            TGT_FAIL("image %d: counts beyond the buffer", b);
        for (int k = 0; k < M; ++k) {
            const int row = s[map_off + (long long)b * M + k];
            if (row < -1 || row >= h[1]) TGT_FAIL("image %d slot %d: row %d of %d", b, k, row, h[1]);
        }
        for (int i = 0; i < h[3]; ++i) {
            const int *q = s + h[2] + 4 * i;
            if (planes && (q[0] < 0 || q[0] >= P)) TGT_FAIL("image %d blob %d: plane %d outside [0, %d)", b, i, q[0], P);
            if (q[3] < 0 || q[3] > TGT_MAX_RADIUS || q[1] < -TGT_MAX_CENTRE || q[1] > TGT_MAX_CENTRE ||
                q[2] < -TGT_MAX_CENTRE || q[2] > TGT_MAX_CENTRE)
                TGT_FAIL("image %d blob %d: centre / radius out of range", b, i);
        }
        for (int i = 0; i < h[5]; ++i) {
            const int *q = s + h[4] + 5 * i;
            if (planes && (q[0] < all_lo || q[0] >= P))
                TGT_FAIL("image %d rectangle %d: plane %d outside [%d, %d)", b, i, q[0], all_lo, P);
        }
        for (int i = 0; i < h[7]; ++i) {
            const int *q = s + h[6] + 4 * i;
            if (q[2] < 0 || q[2] > TGT_MAX_RADIUS || q[0] < -TGT_MAX_CENTRE || q[0] > TGT_MAX_CENTRE ||
                q[1] < -TGT_MAX_CENTRE || q[1] > TGT_MAX_CENTRE)
                TGT_FAIL("image %d pre_hm blob %d: centre / radius out of range", b, i);
        }
    }
    TgtArgs a;
    a.buf = d->staging_dev; a.hm = d->hm; a.pre = d->pre_hm; a.hp = hm_hp;
    a.B = B; a.C = d->C; a.J = J; a.h = d->h; a.w = d->w; a.H = d->H; a.W = d->W; a.max_objs = M; a.S = S;
    a.hmTilesX = a.hmTilesY = a.preTilesX = a.preTilesY = 1;
    long long hmBlocks = 0, hpBlocks = 0, preBlocks = 0;
    if (planes) { a.hmTilesX = ct_cdiv(d->w, TGT_TW); a.hmTilesY = ct_cdiv(d->h, TGT_TH); }
    if (d->hm) hmBlocks = (long long)B * d->C * a.hmTilesX * a.hmTilesY;
    if (hm_hp) hpBlocks = (long long)B * J * a.hmTilesX * a.hmTilesY;
    if (d->pre_hm) {
        a.preTilesX = ct_cdiv(d->W, TGT_TW); a.preTilesY = ct_cdiv(d->H, TGT_TH);
        preBlocks = (long long)B * a.preTilesX * a.preTilesY;
    }
    a.slotElems = any_slot ? (long long)B * M * S : 0;
    const long long slotBlocks = (a.slotElems + 255) / 256;
    const long long blocks = hmBlocks + hpBlocks + preBlocks + slotBlocks;
    if (blocks >= (1LL << 31)) TGT_FAIL("%lld workgroups: batch too large for one launch", blocks);
    a.hmBlocks = (unsigned)hmBlocks; a.hpBlocks = (unsigned)hpBlocks; a.preBlocks = (unsigned)preBlocks;
    a.map_off = (int)map_off; a.col_off = (int)col_off; a.tab_off = (int)tab_off;
    if (hipMemcpyAsync(d->staging_dev, d->staging_host, (size_t)words * 4, hipMemcpyHostToDevice, (hipStream_t)stream) !=
        hipSuccess) {
        ct_set_error("%s: upload failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return CT_ERR_LAUNCH;
    }
    if (pose) hipLaunchKernelGGL(build_targets_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(build_targets_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

}  // namespace

extern "C" size_t ct_build_targets_header_words(int B, int max_objs, int slot_words, int nout)
{
    if (B <= 0 || max_objs <= 0 || slot_words <= 0 || nout <= 0) return 0;
    return (size_t)8 * B + (size_t)B * max_objs + (size_t)slot_words + (size_t)4 * nout;
}

extern "C" int ct_build_targets(const ct_targets_desc *d, void *stream)
{
    if (!d) CT_FAIL_ARG("ct_build_targets: null descriptor");
    return build_impl("ct_build_targets", d, false, nullptr, 0, stream);
}

extern "C" int ct_build_pose_targets(const ct_pose_targets_desc *d, void *stream)
{
    if (!d) CT_FAIL_ARG("ct_build_pose_targets: null descriptor");
    return build_impl("ct_build_pose_targets", &d->base, true, d->hm_hp, d->J, stream);
}
