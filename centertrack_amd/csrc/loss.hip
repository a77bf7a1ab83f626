// The CenterTrack training loss (GenericLoss: trainer.py:20-86, model/losses.py) on raw head outputs, forward and
// backward, for gfx950.  DESIGN.md section 10.
//
//   forward  = loss_dense_fwd_kernel    one pass over logits and target of every focal head: per-workgroup partial sums
//            + loss_slot_reduce_kernel  one workgroup per head: everything indexed by (b, m), the sum of the partials,
//                                       the per-head loss
//   backward = loss_slot_reduce_kernel  the denominators only (mask sums, row counts)
//            + loss_dense_bwd_kernel    one pass that writes dL/dx of every focal head and zero-fills the other maps
//            + loss_slot_scatter_kernel the slot values; duplicates are summed by their lowest slot
//
// No atomics and no host reads anywhere.  Every sum has a fixed shape: a thread adds its own elements in ascending
// index order, a wave adds its lanes by a shuffle tree, a workgroup adds its waves in wave order, and the finishing
// step gives partial i to thread i and repeats the same tree -- none of it depends on timing or placement.
#include "ct_common.h"

#define LOSS_DENSE_THREADS 256
#define LOSS_SLOT_THREADS 1024
#define LOSS_MAX_PARTIALS 1024           // per focal head: one per thread of the finishing workgroup
#define LOSS_DEN_FLOATS 4                // workspace floats per head in front of the partials

struct LossHeadDev {
    const float *x, *target, *mask;
    const long long *ind, *cat;
    float *grad;
    int kind, C, M;
    int vec;                             // x, target and grad are 16-byte aligned: float4 path
    int fwd_blk0, fwd_nblk;              // this head's workgroups of loss_dense_fwd_kernel (focal heads only)
    int bwd_blk0, bwd_nblk;              // ... of loss_dense_bwd_kernel (heads with a gradient buffer)
    int slot_blk0, slot_nblk;            // ... of loss_slot_scatter_kernel
    int part0;                           // first partial of this head in the workspace (floats)
};

struct LossArgs {
    LossHeadDev h[CT_LOSS_MAX_HEADS];
    int nheads, B, HW, fwd;
    float *ws;
    float *loss;
    const float *up;
};

#define P_LO 1e-4f
#define P_HI 0.9999f

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// sum over the workgroup, the same value in every thread
__device__ __forceinline__ float block_sum(float v, float *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += sh[i];
    return t;
}

// ---- the dense focal pass --------------------------------------------------------------------------------------------
__device__ __forceinline__ float focal_neg(float x, float gt)
{
    const float s = sigmoidf_(x);
    const float p = ct_clamp_prop(s, P_LO, P_HI);
    float w = 1.f - gt;
    w *= w;
    w *= w;
    return logf(1.f - p) * p * p * w;
}

// d/dx of focal_neg; exactly 0 where the clamp is active (torch's clamp backward)
__device__ __forceinline__ float focal_neg_grad(float x, float gt)
{
    const float p = sigmoidf_(x);
    if (p < P_LO || p > P_HI) return 0.f;
    float w = 1.f - gt;
    w *= w;
    w *= w;
    const float q = 1.f - p;
    return w * p * p * (2.f * q * logf(q) - p);
}

__device__ __forceinline__ int find_head(const LossArgs &a, int bid, int which)
{
    for (int i = 0; i < a.nheads; ++i) {
        const int b0 = which == 0 ? a.h[i].fwd_blk0 : which == 1 ? a.h[i].bwd_blk0 : a.h[i].slot_blk0;
        const int nb = which == 0 ? a.h[i].fwd_nblk : which == 1 ? a.h[i].bwd_nblk : a.h[i].slot_nblk;
        if (bid >= b0 && bid < b0 + nb) return i;
    }
    return -1;
}

__global__ __launch_bounds__(LOSS_DENSE_THREADS) void loss_dense_fwd_kernel(LossArgs a)
{
    __shared__ float sh[LOSS_DENSE_THREADS / 64];
    const int hi = find_head(a, blockIdx.x, 0);
    if (hi < 0) return;
    const LossHeadDev &h = a.h[hi];
    const int j = blockIdx.x - h.fwd_blk0, tid = threadIdx.x;
    const size_t n = (size_t)a.B * h.C * a.HW, step = (size_t)h.fwd_nblk * LOSS_DENSE_THREADS;
    float acc = 0.f;
    if (h.vec) {
        const size_t nv = n >> 2;
        const float4 *xv = (const float4 *)h.x, *gv = (const float4 *)h.target;
        for (size_t i = (size_t)j * LOSS_DENSE_THREADS + tid; i < nv; i += step) {
            const float4 x = xv[i], g = gv[i];
            acc += focal_neg(x.x, g.x);
            acc += focal_neg(x.y, g.y);
            acc += focal_neg(x.z, g.z);
            acc += focal_neg(x.w, g.w);
        }
        if (j == 0) {
            const size_t i = (nv << 2) + tid;
            if (i < n) acc += focal_neg(h.x[i], h.target[i]);
        }
    } else {
        for (size_t i = (size_t)j * LOSS_DENSE_THREADS + tid; i < n; i += step) acc += focal_neg(h.x[i], h.target[i]);
    }
    const float t = block_sum(acc, sh);
    if (tid == 0) a.ws[h.part0 + j] = t;
}

__global__ __launch_bounds__(LOSS_DENSE_THREADS) void loss_dense_bwd_kernel(LossArgs a)
{
    const int hi = find_head(a, blockIdx.x, 1);
    if (hi < 0) return;
    const LossHeadDev &h = a.h[hi];
    const int j = blockIdx.x - h.bwd_blk0, tid = threadIdx.x;
    const size_t n = (size_t)a.B * h.C * a.HW, step = (size_t)h.bwd_nblk * LOSS_DENSE_THREADS;
    const bool focal = h.kind == CT_LOSS_FOCAL;
    float sc = 0.f;
    if (focal) {                                   // loss = -(pos + neg) / num_pos, or -neg without a positive
        const float np = a.ws[hi * LOSS_DEN_FLOATS];
        sc = -a.up[hi] / (np == 0.f ? 1.f : np);
    }
    if (h.vec) {
        const size_t nv = n >> 2;
        const float4 *xv = (const float4 *)h.x, *gv = (const float4 *)h.target;
        float4 *ov = (float4 *)h.grad;
        for (size_t i = (size_t)j * LOSS_DENSE_THREADS + tid; i < nv; i += step) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (focal) {
                const float4 x = xv[i], g = gv[i];
                o.x = sc * focal_neg_grad(x.x, g.x);
                o.y = sc * focal_neg_grad(x.y, g.y);
                o.z = sc * focal_neg_grad(x.z, g.z);
                o.w = sc * focal_neg_grad(x.w, g.w);
            }
            ov[i] = o;
        }
        if (j == 0) {
            const size_t i = (nv << 2) + tid;
            if (i < n) h.grad[i] = focal ? sc * focal_neg_grad(h.x[i], h.target[i]) : 0.f;
        }
    } else {
        for (size_t i = (size_t)j * LOSS_DENSE_THREADS + tid; i < n; i += step)
            h.grad[i] = focal ? sc * focal_neg_grad(h.x[i], h.target[i]) : 0.f;
    }
}

// ---- everything indexed by (b, m) ------------------------------------------------------------------------------------
__device__ __forceinline__ float smooth_l1(float d)
{
    const float ad = fabsf(d);
    return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

// cross entropy of the two logits (z0, z1) against class t
__device__ __forceinline__ float ce2(float z0, float z1, int t)
{
    const float mx = fmaxf(z0, z1);
    return mx + logf(expf(z0 - mx) + expf(z1 - mx)) - (t ? z1 : z0);
}

// One workgroup per head.  Writes den[head][0..2] (what the backward divides by) and, in the forward, loss[head].
//   focal: den0 = num_pos      L1 / depth / BCE: den0 = sum(mask) + 1e-4      rot: den0 = B*M, den1 / den2 = rows with a
//   non-zero target bin 1 / 2
__global__ __launch_bounds__(LOSS_SLOT_THREADS) void loss_slot_reduce_kernel(LossArgs a)
{
    __shared__ float sh[LOSS_SLOT_THREADS / 64];
    const int hi = blockIdx.x, tid = threadIdx.x;
    const LossHeadDev &h = a.h[hi];
    const int B = a.B, HW = a.HW, M = h.M, C = h.C;
    float *den = a.ws + hi * LOSS_DEN_FLOATS;
    const bool fwd = a.fwd != 0;
    if (h.kind == CT_LOSS_FOCAL) {
        float pos = 0.f, np = 0.f, neg = 0.f;
        for (int e = tid; e < B * M; e += LOSS_SLOT_THREADS) {
            const long long ind = h.ind[e], cat = h.cat[e];
            if (ind < 0 || ind >= HW || cat < 0 || cat >= C) continue;
            const float mk = h.mask[e];
            np += mk;
            if (fwd) {
                const float s = sigmoidf_(h.x[((size_t)(e / M) * C + (size_t)cat) * HW + (size_t)ind]);
                const float p = ct_clamp_prop(s, P_LO, P_HI), q = 1.f - p;
                pos += logf(p) * q * q * mk;
            }
        }
        if (fwd)
            for (int i = tid; i < h.fwd_nblk; i += LOSS_SLOT_THREADS) neg += a.ws[h.part0 + i];
        np = block_sum(np, sh);
        if (fwd) {
            pos = block_sum(pos, sh);
            neg = block_sum(neg, sh);
        }
        if (tid == 0) {
            den[0] = np;
            if (fwd) a.loss[hi] = np == 0.f ? -neg : -(pos + neg) / np;
        }
    } else if (h.kind == CT_LOSS_ROT) {
        float ce = 0.f, r1 = 0.f, n1 = 0.f, r2 = 0.f, n2 = 0.f;
        for (int e = tid; e < B * M; e += LOSS_SLOT_THREADS) {
            const long long ind = h.ind[e];
            const bool ok = ind >= 0 && ind < HW;
            const int t1 = ok && h.cat[2 * e] != 0, t2 = ok && h.cat[2 * e + 1] != 0;
            n1 += (float)t1;
            n2 += (float)t2;
            if (!fwd) continue;
            const float mk = ok ? h.mask[e] : 0.f;
            float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (ok) {
                const float *px = h.x + (size_t)(e / M) * 8 * HW + (size_t)ind;
                for (int c = 0; c < 8; ++c) x[c] = px[(size_t)c * HW];
            }
            ce += ce2(x[0] * mk, x[1] * mk, t1);
            ce += ce2(x[4] * mk, x[5] * mk, t2);
            if (t1) {
                const float r = h.target[2 * e];
                r1 += smooth_l1(x[2] - sinf(r));
                r1 += smooth_l1(x[3] - cosf(r));
            }
            if (t2) {
                const float r = h.target[2 * e + 1];
                r2 += smooth_l1(x[6] - sinf(r));
                r2 += smooth_l1(x[7] - cosf(r));
            }
        }
        n1 = block_sum(n1, sh);
        n2 = block_sum(n2, sh);
        if (fwd) {
            ce = block_sum(ce, sh);
            r1 = block_sum(r1, sh);
            r2 = block_sum(r2, sh);
        }
        if (tid == 0) {
            const float rows = (float)(B * M);
            den[0] = rows;
            den[1] = n1;
            den[2] = n2;
            if (fwd) a.loss[hi] = ce / rows + (n1 > 0.f ? r1 / n1 : 0.f) + (n2 > 0.f ? r2 / n2 : 0.f);
        }
    } else {
        float num = 0.f, ms = 0.f;
        for (int e = tid; e < B * M * C; e += LOSS_SLOT_THREADS) {
            const int bm = e / C, c = e - bm * C;
            const long long ind = h.ind[bm];
            if (ind < 0 || ind >= HW) continue;
            const float mk = h.mask[e];
            ms += mk;
            if (!fwd) continue;
            const float x = h.x[((size_t)(bm / M) * C + c) * HW + (size_t)ind], t = h.target[e];
            if (h.kind == CT_LOSS_BCE) {
                num += mk * (fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))));
            } else {
                const float pred = h.kind == CT_LOSS_L1_DEPTH ? 1.f / (sigmoidf_(x) + 1e-6f) - 1.f : x;
                num += fabsf(pred * mk - t * mk);
            }
        }
        ms = block_sum(ms, sh);
        if (fwd) num = block_sum(num, sh);
        if (tid == 0) {
            den[0] = ms + 1e-4f;
            if (fwd) a.loss[hi] = num / (ms + 1e-4f);
        }
    }
}

// d(up * loss) / d(x[b, c, ind]) of slot bm = b*M + m alone (focal: c is the slot's class)
__device__ __forceinline__ float slot_grad(const LossHeadDev &h, int HW, int b, int bm, int c, int ind, const float *den,
                                           float up)
{
    const float *px = h.x + (size_t)b * h.C * HW + (size_t)ind;
    switch (h.kind) {
    case CT_LOSS_FOCAL: {
        const float np = den[0];
        if (np == 0.f) return 0.f;
        const float p = sigmoidf_(px[(size_t)c * HW]);
        if (p < P_LO || p > P_HI) return 0.f;
        const float q = 1.f - p;
        return -up / np * h.mask[bm] * (q * q * (q - 2.f * p * logf(p)));
    }
    case CT_LOSS_ROT: {
        const int half = c >> 2, base = c & 4, j = c & 3;
        const int t = h.cat[2 * bm + half] != 0;
        if (j < 2) {
            const float mk = h.mask[bm];
            const float z0 = px[(size_t)base * HW] * mk, z1 = px[(size_t)(base + 1) * HW] * mk;
            const float mx = fmaxf(z0, z1), e0 = expf(z0 - mx), e1 = expf(z1 - mx);
            const float pj = (j ? e1 : e0) / (e0 + e1);
            return up * (pj - (j == t ? 1.f : 0.f)) * mk / den[0];
        }
        if (!t) return 0.f;
        const float r = h.target[2 * bm + half];
        const float d = px[(size_t)c * HW] - (j == 2 ? sinf(r) : cosf(r));
        return up * (fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : d))) / den[1 + half];      // (a NaN residual stays NaN, as in torch)
    }
    case CT_LOSS_BCE: {
        const int e = bm * h.C + c;
        return up * h.mask[e] * (sigmoidf_(px[(size_t)c * HW]) - h.target[e]) / den[0];
    }
    default: {
        const int e = bm * h.C + c;
        const float mk = h.mask[e], x = px[(size_t)c * HW];
        float pred = x, dpred = 1.f;
        if (h.kind == CT_LOSS_L1_DEPTH) {
            const float s = sigmoidf_(x), u = s + 1e-6f;
            pred = 1.f / u - 1.f;
            dpred = -s * (1.f - s) / (u * u);
        }
        const float v = pred * mk - h.target[e] * mk;
        const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
        return up * sg * mk * dpred / den[0];
    }
    }
}

// One workgroup per (head, image, 256 slots).  keys[] = the element a slot names (ind, for focal heads class*HW + ind),
// -1 for a slot out of range.  The lowest slot of a key sums every slot of that key in ascending order and stores once;
// on a focal head it adds the sum onto what the dense pass wrote.
__global__ __launch_bounds__(256) void loss_slot_scatter_kernel(LossArgs a)
{
    extern __shared__ int keys[];
    const int hi = find_head(a, blockIdx.x, 2);
    if (hi < 0) return;
    const LossHeadDev &h = a.h[hi];
    const int HW = a.HW, M = h.M, C = h.C, tid = threadIdx.x;
    const int chunks = (M + 255) / 256, local = blockIdx.x - h.slot_blk0;
    const int b = local / chunks, m = (local - b * chunks) * 256 + tid;
    const bool focal = h.kind == CT_LOSS_FOCAL;
    for (int i = tid; i < M; i += 256) {
        const long long ind = h.ind[b * M + i];
        int key = (ind >= 0 && ind < HW) ? (int)ind : -1;
        if (focal && key >= 0) {
            const long long cat = h.cat[b * M + i];
            key = (cat >= 0 && cat < C) ? (int)cat * HW + key : -1;
        }
        keys[i] = key;
    }
    __syncthreads();
    if (m >= M) return;
    const int k = keys[m];
    if (k < 0) return;
    for (int i = 0; i < m; ++i)
        if (keys[i] == k) return;
    const float *den = a.ws + hi * LOSS_DEN_FLOATS;
    const float up = a.up[hi];
    const int ind = focal ? k % HW : k;
    float *pg = h.grad + (size_t)b * C * HW + (size_t)ind;
    if (focal) {
        const int cat = k / HW;
        float sum = 0.f;
        for (int i = m; i < M; ++i)
            if (keys[i] == k) sum += slot_grad(h, HW, b, b * M + i, cat, ind, den, up);
        pg[(size_t)cat * HW] += sum;
    } else {
        for (int c = 0; c < C; ++c) {
            float sum = 0.f;
            for (int i = m; i < M; ++i)
                if (keys[i] == k) sum += slot_grad(h, HW, b, b * M + i, c, ind, den, up);
            pg[(size_t)c * HW] = sum;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int loss_plan(const ct_loss_desc *d, LossArgs *a, bool backward, size_t *ws_floats, int *max_m, const char *who)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", who);
    if (!d->heads) CT_FAIL_ARG("%s: null head array", who);
    if (d->nheads <= 0 || d->nheads > CT_LOSS_MAX_HEADS)
        CT_FAIL_ARG("%s: nheads=%d must be in 1..%d", who, d->nheads, CT_LOSS_MAX_HEADS);
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) CT_FAIL_ARG("%s: B=%d H=%d W=%d must be positive", who, d->B, d->H, d->W);
    a->nheads = d->nheads;
    a->B = d->B;
    a->HW = d->H * d->W;
    a->fwd = backward ? 0 : 1;
    a->ws = (float *)d->workspace;
    a->loss = d->loss;
    a->up = d->grad_loss;
    size_t parts = (size_t)CT_LOSS_MAX_HEADS * LOSS_DEN_FLOATS;
    int fwd_blk = 0, bwd_blk = 0, slot_blk = 0;
    *max_m = 0;
    for (int i = 0; i < d->nheads; ++i) {
        const ct_loss_head &s = d->heads[i];
        LossHeadDev &h = a->h[i];
        if (s.kind < CT_LOSS_FOCAL || s.kind > CT_LOSS_ROT) CT_FAIL_ARG("%s: head %d: unknown kind %d", who, i, s.kind);
        if (s.C <= 0 || s.M <= 0) CT_FAIL_ARG("%s: head %d: C=%d M=%d must be positive", who, i, s.C, s.M);
        if (s.M > CT_LOSS_MAX_SLOTS) CT_FAIL_ARG("%s: head %d: M=%d above CT_LOSS_MAX_SLOTS=%d", who, i, s.M, CT_LOSS_MAX_SLOTS);
        if (!s.logits || !s.target || !s.mask || !s.ind) CT_FAIL_ARG("%s: head %d: null logits / target / mask / ind", who, i);
        if (s.kind == CT_LOSS_FOCAL && !s.cat) CT_FAIL_ARG("%s: head %d: a focal head needs cat", who, i);
        if (s.kind == CT_LOSS_ROT && s.C != 8) CT_FAIL_ARG("%s: head %d: a rot head has C = 8, got %d", who, i, s.C);
        if (s.kind == CT_LOSS_ROT && !s.cat) CT_FAIL_ARG("%s: head %d: a rot head needs cat (rotbin)", who, i);
        const size_t chw = (size_t)s.C * d->H * d->W;
        if (chw >= ((size_t)1 << 31) || (size_t)d->B * s.M * s.C >= ((size_t)1 << 31))
            CT_FAIL_ARG("%s: head %d: C*H*W and B*M*C must stay below 2^31", who, i);
        h.x = s.logits; h.target = s.target; h.mask = s.mask; h.ind = s.ind; h.cat = s.cat; h.grad = s.grad;
        h.kind = s.kind; h.C = s.C; h.M = s.M;
        const bool focal = s.kind == CT_LOSS_FOCAL;
        uintptr_t al = (uintptr_t)s.logits | (uintptr_t)s.grad;
        if (focal) al |= (uintptr_t)s.target;
        h.vec = (al & 15) == 0;
        const size_t n = (size_t)d->B * chw, per = (size_t)LOSS_DENSE_THREADS * 4;
        size_t nb = (n / 4 + per - 1) / per;
        nb = nb < 1 ? 1 : nb > LOSS_MAX_PARTIALS ? LOSS_MAX_PARTIALS : nb;
        h.fwd_blk0 = fwd_blk; h.fwd_nblk = focal ? (int)nb : 0;
        fwd_blk += h.fwd_nblk;
        h.part0 = (int)parts;
        parts += h.fwd_nblk;
        h.bwd_blk0 = bwd_blk; h.bwd_nblk = s.grad ? (int)nb : 0;
        bwd_blk += h.bwd_nblk;
        h.slot_blk0 = slot_blk; h.slot_nblk = s.grad ? d->B * ct_cdiv(s.M, 256) : 0;
        slot_blk += h.slot_nblk;
        if (s.grad && s.M > *max_m) *max_m = s.M;
    }
    *ws_floats = parts;
    return CT_OK;
}

static int loss_check_ws(const ct_loss_desc *d, size_t ws_floats, const char *who)
{
    const size_t need = ws_floats * sizeof(float);
    if (!d->workspace || d->workspace_bytes < need) {
        ct_set_error("%s: workspace of %zu bytes needed (ct_generic_loss_workspace_bytes), got %zu", who, need,
                     d->workspace ? d->workspace_bytes : (size_t)0);
        return CT_ERR_WORKSPACE;
    }
    return CT_OK;
}

extern "C" size_t ct_generic_loss_workspace_bytes(const ct_loss_desc *d)
{
    LossArgs a;
    size_t wsf;
    int mm;
    if (loss_plan(d, &a, false, &wsf, &mm, "ct_generic_loss_workspace_bytes") != CT_OK) return 0;
    return wsf * sizeof(float);
}

extern "C" int ct_generic_loss_forward(const ct_loss_desc *d, void *stream)
{
    static const char *who = "ct_generic_loss_forward";
    LossArgs a;
    size_t wsf;
    int mm;
    int rc = loss_plan(d, &a, false, &wsf, &mm, who);
    if (rc != CT_OK) return rc;
    if (!d->loss) CT_FAIL_ARG("%s: null loss output", who);
    if ((rc = loss_check_ws(d, wsf, who)) != CT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const LossHeadDev &last = a.h[a.nheads - 1];
    const int fwd_blocks = last.fwd_blk0 + last.fwd_nblk;
    if (fwd_blocks) {
        hipLaunchKernelGGL(loss_dense_fwd_kernel, dim3((unsigned)fwd_blocks), dim3(LOSS_DENSE_THREADS), 0, s, a);
        CT_CHECK_LAUNCH("ct_generic_loss_forward (dense)");
    }
    hipLaunchKernelGGL(loss_slot_reduce_kernel, dim3((unsigned)a.nheads), dim3(LOSS_SLOT_THREADS), 0, s, a);
    CT_CHECK_LAUNCH("ct_generic_loss_forward (slots)");
    return CT_OK;
}

extern "C" int ct_generic_loss_backward(const ct_loss_desc *d, void *stream)
{
    static const char *who = "ct_generic_loss_backward";
    LossArgs a;
    size_t wsf;
    int mm;
    int rc = loss_plan(d, &a, true, &wsf, &mm, who);
    if (rc != CT_OK) return rc;
    if (!d->grad_loss) CT_FAIL_ARG("%s: null grad_loss", who);
    if ((rc = loss_check_ws(d, wsf, who)) != CT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const LossHeadDev &last = a.h[a.nheads - 1];
    const int bwd_blocks = last.bwd_blk0 + last.bwd_nblk, slot_blocks = last.slot_blk0 + last.slot_nblk;
    if (!bwd_blocks) return CT_OK;                 // no head asks for a gradient
    hipLaunchKernelGGL(loss_slot_reduce_kernel, dim3((unsigned)a.nheads), dim3(LOSS_SLOT_THREADS), 0, s, a);
    CT_CHECK_LAUNCH("ct_generic_loss_backward (denominators)");
    hipLaunchKernelGGL(loss_dense_bwd_kernel, dim3((unsigned)bwd_blocks), dim3(LOSS_DENSE_THREADS), 0, s, a);
    CT_CHECK_LAUNCH("ct_generic_loss_backward (dense)");
    hipLaunchKernelGGL(loss_slot_scatter_kernel, dim3((unsigned)slot_blocks), dim3(256), (size_t)mm * sizeof(int), s, a);
    CT_CHECK_LAUNCH("ct_generic_loss_backward (slots)");
    return CT_OK;
}
