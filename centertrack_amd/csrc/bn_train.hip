// Training-mode BatchNorm for gfx950, fp32, NHWC views with a channel pitch: the statistics, and BatchNorm (+ residual)
// (+ ReLU) forward and backward.  One implementation over ct_bn_act_desc serves the neck (ct_bn_relu_*: the ReLU, no residual),
// the backbone (ct_bn_act_*) and the stems.  Specification: torch.autograd of F.batch_norm (+ res) (+ relu).  DESIGN.md
// sections 12 and 13.
//
//   * bn_reduce_kernel<MODE>: per-channel sums over the N*H*W pixels.  A workgroup owns one slab of pixels and one chunk
//     of up to 64 channel quads; thread (row r, quad q) adds the pixels r, r + rows, ... of the slab in ascending order
//     (16-byte loads), the rows are added through LDS in row order, and the workgroup stores its partial into slab
//     `blockIdx.x` of the workspace.  bn_finalize_kernel<MODE> adds the slabs in slab order.
//       MODE 0: sum (z - z[pixel 0]) -> mean.  MODE 1: sum (z - mean)^2 -> biased variance, invstd (two passes, never E[x^2] - E[x]^2).
//   * bn_act_reduce_kernel / bn_act_finalize_kernel: the same plan for sum g and sum g * xhat -> gbeta, ggamma, with g = gy
//     where the recomputed output is > 0 (all of gy without the ReLU).
//     These three kernels are instantiated on <ReLU, residual> and chosen on the host: as branches at run time the two cost
//     the neck's element-wise passes 1-2 % (measured on an MI355X at [8,256,256,64]).
//   * bn_act_apply_kernel: y = fma(z - mean, a, beta) (+ res) (max 0), a = gamma * invstd (bn_pre of ct_train.h: the backward
//     recomputes the same bits from the same four vectors, so its mask is the forward's).
//   * bn_act_bwd_kernel: gz = a * (g - mean(g) - xhat * mean(g * xhat)) with batch statistics, a * g with running ones; gres = g.
//     <.., EXT>: the two sums and the reciprocal of the count come from the caller's device pointers (ct_bn_*_backward_apply:
//     sums and a count over the batches of all ranks) where the one-call backward reads the workspace tail and 1.0f / P.
//   * bn_merge_kernel: the statistics of `world` shards (rows of [mean | var | pixel count]) pooled into those of their
//     union, in double, the rows in row order.
// No atomics anywhere; slab counts depend on the shapes only: every result is bitwise equal from run to run.
// Every view is addressed with 32-bit element offsets, so a view stays below 2 GiB (checked on the host).
#include <stddef.h>
#include <string.h>

#include "ct_train.h"

namespace {

struct BnArgs {
    const float *z, *gy, *gamma, *beta;
    float *mean, *invstd;                        // written by the statistics, read by the rest
    const float *res;
    float *y, *gz, *gres, *ggamma, *gbeta, *ws;
    int P, C, ldz, ldy, ldgy, ldgz, ldr, ldgres;
    int cw, rows, pixPerSlab, slabs, batchStats;
    float eps;                                   // the statistics only
    float *var;
    const float *extSums, *extInvCount;          // bn_act_bwd_kernel<.., EXT = true> only
    float *resid;                                // bn_finalize_kernel<.., ROW = true> only
    long long *count;
};

template <int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(BnArgs a)
{
    __shared__ f32x4 red[256];
    const int q = threadIdx.x % a.cw, r = threadIdx.x / a.cw;
    const int c = ((int)blockIdx.y * a.cw + q) * 4;
    const bool live = r < a.rows && c < a.C;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const int p0 = (int)blockIdx.x * a.pixPerSlab, p1 = min(a.P, p0 + a.pixPerSlab);
        // MODE 0: the pivot, pixel 0 of the view (a sum of z - pivot keeps a channel of mean 100, std 0.01 exact where a sum of
        // z loses it)
        const f32x4 mean = ld4((MODE == 0 ? a.z : a.mean) + c);
        for (int p = p0 + r; p < p1; p += a.rows) {
            const f32x4 z = ld4(a.z + p * a.ldz + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = z[i] - mean[i];
                s0[i] = MODE == 0 ? s0[i] + d : fmaf(d, d, s0[i]);
            }
        }
    }
    red[threadIdx.x] = s0;
    __syncthreads();
    if (r != 0 || c >= a.C) return;
    for (int k = 1; k < a.rows; ++k) {
        const f32x4 v = red[k * a.cw + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) s0[i] += v[i];
    }
    st4(a.ws + (size_t)blockIdx.x * 2 * a.C + c, s0);
}

// ROW (ct_bn_stats_row): the same mean, variance and invstd, and beside them what a merge with other shards needs -- the part
// of pivot + s0 / P that the rounding of the mean to float dropped (the two-sum of Knuth: mean + resid is that sum exactly), and
// the pixel count as an integer, twice (16 bytes with every byte defined).
template <int MODE, bool ROW = false>
__global__ __launch_bounds__(256) void bn_finalize_kernel(BnArgs a)
{
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    float s0 = 0.0f;
    for (int j = 0; j < a.slabs; ++j) s0 += a.ws[(size_t)j * 2 * a.C + c];
    if (MODE == 0) {
        if (ROW) {
            const float pivot = a.z[c], q = s0 / (float)a.P, m = pivot + q, bb = m - pivot;
            a.mean[c] = m;
            a.resid[c] = (pivot - (m - bb)) + (q - bb);
        } else {
            a.mean[c] = a.z[c] + s0 / (float)a.P;
        }
    } else {
        const float v = s0 / (float)a.P;
        a.var[c] = v;
        a.invstd[c] = 1.0f / sqrtf(v + a.eps);
        if (ROW && c == 0) a.count[0] = a.count[1] = (long long)a.P;
    }
}

// the incoming gradient behind the activation: the forward's own bits decide the mask (torch's ReLU: 0 at exactly 0)
template <bool RELU, bool RES>
__device__ __forceinline__ float act_grad(float z, float mean, float ka, float beta, float r, float gy)
{
    if (!RELU) return gy;
    float t = bn_pre(z, mean, ka, beta);
    if (RES) t += r;
    return !(t <= 0.0f) ? gy : 0.0f;           // (a NaN pre-activation passes gy: torch's threshold_backward)
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_act_reduce_kernel(BnArgs a)
{
    __shared__ f32x4 red[2][256];
    const int q = threadIdx.x % a.cw, r = threadIdx.x / a.cw;
    const int c = ((int)blockIdx.y * a.cw + q) * 4;
    const bool live = r < a.rows && c < a.C;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const int p0 = (int)blockIdx.x * a.pixPerSlab, p1 = min(a.P, p0 + a.pixPerSlab);
        const f32x4 mean = ld4(a.mean + c), istd = ld4(a.invstd + c), ga = ld4(a.gamma + c), be = ld4(a.beta + c);
        f32x4 ka;
#pragma unroll
        for (int i = 0; i < 4; ++i) ka[i] = ga[i] * istd[i];
        for (int p = p0 + r; p < p1; p += a.rows) {
            const f32x4 z = ld4(a.z + p * a.ldz + c), gy = ld4(a.gy + p * a.ldgy + c);
            f32x4 rv = {0.f, 0.f, 0.f, 0.f};
            if (RES) rv = ld4(a.res + p * a.ldr + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float g = act_grad<RELU, RES>(z[i], mean[i], ka[i], be[i], rv[i], gy[i]);
                const float xh = (z[i] - mean[i]) * istd[i];
                s0[i] += g;
                s1[i] = fmaf(g, xh, s1[i]);
            }
        }
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    if (r != 0 || c >= a.C) return;
    for (int k = 1; k < a.rows; ++k) {
        const f32x4 v = red[0][k * a.cw + q], u = red[1][k * a.cw + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s0[i] += v[i];
            s1[i] += u[i];
        }
    }
    float *slab = a.ws + (size_t)blockIdx.x * 2 * a.C;
    st4(slab + c, s0);
    st4(slab + a.C + c, s1);
}

__global__ __launch_bounds__(256) void bn_act_finalize_kernel(BnArgs a)
{
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    float s0 = 0.0f, s1 = 0.0f;
    for (int j = 0; j < a.slabs; ++j) {
        s0 += a.ws[(size_t)j * 2 * a.C + c];
        s1 += a.ws[(size_t)j * 2 * a.C + a.C + c];
    }
    float *sums = a.ws + (size_t)a.slabs * 2 * a.C;      // what the second pass reads
    sums[c] = s0;
    sums[a.C + c] = s1;
    if (a.gbeta) a.gbeta[c] = s0;
    if (a.ggamma) a.ggamma[c] = s1;
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_act_apply_kernel(BnArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (RES) rv = ld4(a.res + p * a.ldr + c);
        f32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = bn_pre(z[i], mean[i], ga[i] * istd[i], be[i]);
            if (RES) t += rv[i];
            y[i] = RELU ? ct_relu(t) : t;
        }
        st4(a.y + p * a.ldy + c, y);
    }
}

template <bool RELU, bool RES, bool EXT = false>
__global__ __launch_bounds__(256) void bn_act_bwd_kernel(BnArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    const float *sums = EXT ? a.extSums : a.ws + (size_t)a.slabs * 2 * a.C;
    const float invP = EXT ? *a.extInvCount : 1.0f / (float)a.P;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c), gy = ld4(a.gy + p * a.ldgy + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (RES) rv = ld4(a.res + p * a.ldr + c);
        f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = sg;
        if (a.batchStats && a.gz) {
            sg = ld4(sums + c);
            sgx = ld4(sums + a.C + c);
        }
        f32x4 gz, gr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ka = ga[i] * istd[i];
            const float g = act_grad<RELU, RES>(z[i], mean[i], ka, be[i], rv[i], gy[i]);
            gr[i] = g;
            if (a.batchStats) {
                const float xh = (z[i] - mean[i]) * istd[i];
                gz[i] = ka * ((g - sg[i] * invP) - xh * (sgx[i] * invP));
            } else {
                gz[i] = ka * g;
            }
        }
        if (a.gz) st4(a.gz + p * a.ldgz + c, gz);
        if (a.gres) st4(a.gres + p * a.ldgres + c, gr);
    }
}

struct MergeArgs {
    const float *rows;
    float *mean, *var, *invstd, *unbiased, *invCount;
    long long *count;
    int world, C, ld;
    float eps;
    const float *gamma, *beta;                   // with betaShifted, or all three NULL
    float *betaShifted;
};

// Row r = [mean_r[C] | var_r[C] | resid_r[C] | P_r], P_r the bits of a 64-bit integer behind the 3 C floats (ct_bn_stats_row).
// One thread per channel walks the rows in row order: pooled moments in double, one rounding to float per result.
//   A shard's mean is a float: at mean 100 its rounding is 4e-6, and the between-shard term (mean_r - mean)^2 of a channel of
//   std 0.01 -- differences of 1e-3 -- would carry it into the variance at 2 * 1e-3 * 4e-6 / 1e-4 = 8e-5 of its value, where
//   one process on the whole batch is good to 1e-7.  So the merge reads mean_r + resid_r, the shard's mean before that
//   rounding, and takes var_r -- the shard's variance about its ROUNDED mean -- back to the true mean: var_r - resid_r^2.
//   One row alone is handed back as it is: the bits of ct_bn_stats.
// invstd comes from the rounded variance with the expression of bn_finalize_kernel<1>.
//   The merged mean is a float as well, and every kernel behind it forms fma(z - mean, a, beta) (bn_pre): at mean 100, std 0.01
//   a = gamma * invstd is of order 100 and multiplies the mean's rounding into y (measured: 3.59e-5 of max|y| at 2x33x65x8, all of
//   that case's error).  What the rounding dropped, lo = mean - float(mean), is known here in double, and y = a (z - mean - lo)
//   + beta = fma(z - mean, a, beta - a lo): betaShifted = fma(-a, lo, beta) carries it through the unchanged kernels, forward
//   and backward alike (the mask is recomputed from the same vector).  One row alone: lo = 0 and betaShifted = beta.
__global__ __launch_bounds__(256) void bn_merge_kernel(MergeArgs a)
{
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const bool refine = a.world > 1;
    long long total = 0;
    double sm = 0.0;
    for (int r = 0; r < a.world; ++r) {
        const float *row = a.rows + (size_t)r * a.ld;
        const long long n = *reinterpret_cast<const long long *>(row + 3 * a.C);
        total += n;
        sm += (double)n * ((double)row[c] + (refine ? (double)row[2 * a.C + c] : 0.0));
    }
    const double N = (double)total, mean = sm / N;
    double sv = 0.0, sb = 0.0;
    for (int r = 0; r < a.world; ++r) {
        const float *row = a.rows + (size_t)r * a.ld;
        const double n = (double)*reinterpret_cast<const long long *>(row + 3 * a.C);
        const double rho = refine ? (double)row[2 * a.C + c] : 0.0;
        const double d = ((double)row[c] + rho) - mean;
        sv += n * ((double)row[a.C + c] - rho * rho);
        sb += n * d * d;
    }
    // (var_r - rho^2 may leave a negative rounding residue on a constant channel: only that is clamped -- a NaN stays a NaN,
    // as in ct_bn_stats and torch, where fmax would hand back the 0)
    const double pooled = (sv + sb) / N, var = pooled < 0.0 ? 0.0 : pooled;
    const float v = (float)var;
    a.mean[c] = (float)mean;
    a.var[c] = v;
    a.invstd[c] = 1.0f / sqrtf(v + a.eps);
    a.unbiased[c] = (float)(var * N / (double)(total - 1));
    if (a.betaShifted) {
        const float lo = (float)(mean - (double)(float)mean), ka = a.gamma[c] * a.invstd[c];
        a.betaShifted[c] = refine ? fmaf(-ka, lo, a.beta[c]) : a.beta[c];
    }
    if (c == 0) {
        *a.invCount = (float)(1.0 / N);
        if (a.count) *a.count = total;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host

struct BnPlan {
    int P, cw, rows, chunks, slabs, pixPerSlab;
};

int make_bn_plan(const char *fn, const ct_bn_act_desc *d, BnPlan *p)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->C % 4) CT_FAIL_ARG("%s: C=%d must be a multiple of 4", fn, d->C);
    if (d->flags & ~(CT_BN_BATCH_STATS | CT_BN_ACT_RELU))
        CT_FAIL_ARG("%s: flags=%d (a combination of CT_BN_BATCH_STATS, CT_BN_ACT_RELU)", fn, d->flags);
    const double px = (double)d->N * d->H * d->W;
    int ld = d->ldz;
    if (d->y && d->ldy > ld) ld = d->ldy;
    if (d->gy && d->ldgy > ld) ld = d->ldgy;
    if (d->gz && d->ldgz > ld) ld = d->ldgz;
    if (d->res && d->ldr > ld) ld = d->ldr;
    if (d->gres && d->ldgres > ld) ld = d->ldgres;
    if (px * (ld > d->C ? ld : d->C) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernels address a view with 32-bit offsets", fn, px);
    const int C4 = d->C / 4;
    p->P = (int)px;
    p->cw = C4 < 64 ? C4 : 64;
    p->rows = 256 / p->cw;
    p->chunks = ct_cdiv(C4, p->cw);
    int slabs = ct_cdiv(512, p->chunks);
    const int maxSlabs = ct_cdiv(p->P, p->rows * 4);          // at least four pixels for each thread
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->pixPerSlab = ct_cdiv(ct_cdiv(p->P, slabs), p->rows) * p->rows;
    p->slabs = ct_cdiv(p->P, p->pixPerSlab);
    return CT_OK;
}

size_t bn_ws_bytes(const ct_bn_act_desc *d, const BnPlan &p) { return (size_t)(p.slabs + 1) * 2 * d->C * sizeof(float); }

BnArgs bn_args(const ct_bn_act_desc *d, const BnPlan &p)
{
    BnArgs a;
    a.z = d->z; a.gy = d->gy; a.gamma = d->gamma; a.beta = d->beta; a.mean = d->mean; a.invstd = d->invstd; a.res = d->res;
    a.y = d->y; a.gz = d->gz; a.gres = d->gres; a.ggamma = d->ggamma; a.gbeta = d->gbeta; a.ws = d->workspace;
    a.P = p.P; a.C = d->C; a.ldz = d->ldz; a.ldy = d->ldy; a.ldgy = d->ldgy; a.ldgz = d->ldgz; a.ldr = d->ldr; a.ldgres = d->ldgres;
    a.cw = p.cw; a.rows = p.rows; a.pixPerSlab = p.pixPerSlab; a.slabs = p.slabs;
    a.batchStats = (d->flags & CT_BN_BATCH_STATS) != 0;
    a.eps = d->eps; a.var = d->var;
    a.extSums = nullptr; a.extInvCount = nullptr; a.resid = nullptr; a.count = nullptr;
    return a;
}

// the <ReLU, residual> instantiation of `kernel` that the descriptor asks for
#define BN_LAUNCH(kernel, d, grid, s, a)                                                                   \
    do {                                                                                                   \
        const bool relu__ = (d)->flags & CT_BN_ACT_RELU;                                                   \
        if (relu__ && (d)->res) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, s, a);        \
        else if (relu__) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, s, a);              \
        else if ((d)->res) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, s, a);            \
        else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, s, a);                         \
    } while (0)

// ct_bn_desc is the head of ct_bn_act_desc field for field: its entry points run on a copy widened with zeros (no residual,
// no gres) and `flags` on top of its own CT_BN_BATCH_STATS
static_assert(offsetof(ct_bn_act_desc, res) == sizeof(ct_bn_desc) && offsetof(ct_bn_act_desc, flags) == offsetof(ct_bn_desc, flags),
              "ct_bn_desc must be a prefix of ct_bn_act_desc");

int widen(const char *fn, const ct_bn_desc *d, int flags, ct_bn_act_desc *w)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->flags & ~CT_BN_BATCH_STATS) CT_FAIL_ARG("%s: flags=%d (0 or CT_BN_BATCH_STATS)", fn, d->flags);
    memset(w, 0, sizeof *w);
    memcpy(w, d, sizeof *d);
    w->flags |= flags;
    return CT_OK;
}

int check_bn_common(const char *fn, const ct_bn_act_desc *d)
{
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_vec(fn, "gamma", d->gamma));
    CT_TRY(check_vec(fn, "beta", d->beta));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    if (d->res) CT_TRY(check_view(fn, "res", d->res, d->ldr, d->C));
    return CT_OK;
}

int bn_apply(const char *fn, const ct_bn_act_desc *d, void *stream)
{
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_bn_common(fn, d));
    CT_TRY(check_view(fn, "y", d->y, d->ldy, d->C));
    BN_LAUNCH(bn_act_apply_kernel, d, dim3(ew_grid(p.P * (d->C / 4))), (hipStream_t)stream, bn_args(d, p));
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

// `query`: the workspace query of the entry point, for its message
int bn_backward(const char *fn, const char *query, const ct_bn_act_desc *d, void *stream)
{
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_bn_common(fn, d));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->C));
    if (!d->gz && !d->gres && !d->ggamma && !d->gbeta) CT_FAIL_ARG("%s: no output asked for (a gradient buffer)", fn);
    if (d->gz) CT_TRY(check_view(fn, "gz", d->gz, d->ldgz, d->C));
    if (d->gres) CT_TRY(check_view(fn, "gres", d->gres, d->ldgres, d->C));
    const bool batch = d->flags & CT_BN_BATCH_STATS;
    const bool sums = d->ggamma || d->gbeta || (d->gz && batch);
    if (sums) CT_TRY(check_workspace(fn, query, d->workspace, d->workspace_bytes, bn_ws_bytes(d, p)));
    hipStream_t s = (hipStream_t)stream;
    const BnArgs a = bn_args(d, p);
    if (sums) {
        BN_LAUNCH(bn_act_reduce_kernel, d, dim3((unsigned)p.slabs, (unsigned)p.chunks), s, a);
        CT_CHECK_LAUNCH(fn);
        hipLaunchKernelGGL(bn_act_finalize_kernel, dim3((unsigned)ct_cdiv(d->C, 256)), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH(fn);
    }
    if (d->gz || d->gres) {
        BN_LAUNCH(bn_act_bwd_kernel, d, dim3(ew_grid(p.P * (d->C / 4))), s, a);
        CT_CHECK_LAUNCH(fn);
    }
    return CT_OK;
}

// the second half of bn_backward on its own: gz and gres from sums and a count the caller owns
int bn_backward_apply(const char *fn, const ct_bn_act_desc *d, const float *sums, const float *inv_count, void *stream)
{
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_bn_common(fn, d));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->C));
    if (!(d->flags & CT_BN_BATCH_STATS)) CT_FAIL_ARG("%s: flags=%d without CT_BN_BATCH_STATS (running statistics need no sums)", fn, d->flags);
    if (!d->gz && !d->gres) CT_FAIL_ARG("%s: no output asked for (gz or gres)", fn);
    if (d->gz) CT_TRY(check_view(fn, "gz", d->gz, d->ldgz, d->C));
    if (d->gres) CT_TRY(check_view(fn, "gres", d->gres, d->ldgres, d->C));
    CT_TRY(check_vec(fn, "sums", sums));
    if (!inv_count) CT_FAIL_ARG("%s: null pointer (inv_count)", fn);
    if (misaligned(inv_count, 3)) CT_FAIL_ARG("%s: inv_count must be 4-byte aligned", fn);
    BnArgs a = bn_args(d, p);
    a.extSums = sums;
    a.extInvCount = inv_count;
    const dim3 grid(ew_grid(p.P * (d->C / 4)));
    hipStream_t s = (hipStream_t)stream;
    const bool relu = d->flags & CT_BN_ACT_RELU;
    if (relu && d->res) hipLaunchKernelGGL((bn_act_bwd_kernel<true, true, true>), grid, dim3(256), 0, s, a);
    else if (relu) hipLaunchKernelGGL((bn_act_bwd_kernel<true, false, true>), grid, dim3(256), 0, s, a);
    else if (d->res) hipLaunchKernelGGL((bn_act_bwd_kernel<false, true, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((bn_act_bwd_kernel<false, false, true>), grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

}  // namespace

extern "C" int ct_bn_merge_stats(const ct_bn_merge_desc *d, void *stream)
{
    const char *fn = "ct_bn_merge_stats";
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->C <= 0 || d->C % 4) CT_FAIL_ARG("%s: C=%d must be a positive multiple of 4", fn, d->C);
    if (d->world < 1) CT_FAIL_ARG("%s: world=%d (at least one row)", fn, d->world);
    if (!(d->eps >= 0.0f)) CT_FAIL_ARG("%s: eps=%g", fn, (double)d->eps);
    if (d->ld < 3 * d->C + 2 || d->ld % 2)
        CT_FAIL_ARG("%s: row pitch %d (an even number of floats, at least 3 C + 2 = %d: mean, var, resid and a 64-bit count)", fn, d->ld, 3 * d->C + 2);
    if (!d->rows) CT_FAIL_ARG("%s: null pointer (rows)", fn);
    if (misaligned(d->rows, 7)) CT_FAIL_ARG("%s: rows must be 8-byte aligned", fn);
    if (!d->mean || !d->var || !d->invstd || !d->unbiased || !d->inv_count)
        CT_FAIL_ARG("%s: null pointer (mean, var, invstd, unbiased or inv_count)", fn);
    if (misaligned(d->mean, 3) || misaligned(d->var, 3) || misaligned(d->invstd, 3) || misaligned(d->unbiased, 3) ||
        misaligned(d->inv_count, 3) || misaligned(d->count, 7))
        CT_FAIL_ARG("%s: the outputs must be 4-byte aligned, count 8-byte aligned", fn);
    if ((d->gamma || d->beta || d->beta_shifted) && !(d->gamma && d->beta && d->beta_shifted))
        CT_FAIL_ARG("%s: gamma, beta and beta_shifted go together (all three or none)", fn);
    if (misaligned(d->gamma, 3) || misaligned(d->beta, 3) || misaligned(d->beta_shifted, 3))
        CT_FAIL_ARG("%s: gamma, beta and beta_shifted must be 4-byte aligned", fn);
    MergeArgs a;
    a.gamma = d->gamma; a.beta = d->beta; a.betaShifted = d->beta_shifted;
    a.rows = d->rows; a.mean = d->mean; a.var = d->var; a.invstd = d->invstd; a.unbiased = d->unbiased;
    a.invCount = d->inv_count; a.count = d->count; a.world = d->world; a.C = d->C; a.ld = d->ld; a.eps = d->eps;
    hipLaunchKernelGGL(bn_merge_kernel, dim3((unsigned)ct_cdiv(d->C, 256)), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

extern "C" int ct_bn_relu_backward_apply(const ct_bn_desc *d, const float *sums, const float *inv_count, void *stream)
{
    ct_bn_act_desc w;
    CT_TRY(widen("ct_bn_relu_backward_apply", d, CT_BN_ACT_RELU, &w));
    return bn_backward_apply("ct_bn_relu_backward_apply", &w, sums, inv_count, stream);
}

extern "C" int ct_bn_act_backward_apply(const ct_bn_act_desc *d, const float *sums, const float *inv_count, void *stream)
{
    return bn_backward_apply("ct_bn_act_backward_apply", d, sums, inv_count, stream);
}

extern "C" size_t ct_bn_workspace_bytes(const ct_bn_desc *d)
{
    ct_bn_act_desc w;
    if (widen("ct_bn_workspace_bytes", d, 0, &w) != CT_OK) return 0;
    return ct_bn_act_workspace_bytes(&w);
}

extern "C" size_t ct_bn_act_workspace_bytes(const ct_bn_act_desc *d)
{
    BnPlan p;
    if (make_bn_plan("ct_bn_act_workspace_bytes", d, &p) != CT_OK) return 0;
    return bn_ws_bytes(d, p);
}

// ct_bn_stats (row == NULL) and ct_bn_stats_row (mean, var, the mean's residual and the count go into `row`)
static int bn_stats(const char *fn, const ct_bn_desc *desc, float *row, void *stream)
{
    ct_bn_act_desc w;
    const ct_bn_act_desc *d = &w;
    BnPlan p;
    CT_TRY(widen(fn, desc, 0, &w));
    if (row) {
        w.mean = row;
        w.var = row + w.C;
    }
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "var", d->var));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    if (!(d->eps >= 0.0f)) CT_FAIL_ARG("%s: eps=%g", fn, (double)d->eps);
    CT_TRY(check_workspace(fn, "ct_bn_workspace_bytes", d->workspace, d->workspace_bytes, bn_ws_bytes(d, p)));
    hipStream_t s = (hipStream_t)stream;
    BnArgs a = bn_args(d, p);
    if (row) {
        a.resid = row + 2 * d->C;
        a.count = reinterpret_cast<long long *>(row + 3 * d->C);
    }
    const dim3 grid((unsigned)p.slabs, (unsigned)p.chunks), fin((unsigned)ct_cdiv(d->C, 256));
    hipLaunchKernelGGL(bn_reduce_kernel<0>, grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (sum)");
    if (row) hipLaunchKernelGGL((bn_finalize_kernel<0, true>), fin, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(bn_finalize_kernel<0>, fin, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (mean)");
    hipLaunchKernelGGL(bn_reduce_kernel<1>, grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (squares)");
    if (row) hipLaunchKernelGGL((bn_finalize_kernel<1, true>), fin, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(bn_finalize_kernel<1>, fin, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (variance)");
    return CT_OK;
}

extern "C" int ct_bn_stats(const ct_bn_desc *d, void *stream) { return bn_stats("ct_bn_stats", d, nullptr, stream); }

extern "C" int ct_bn_stats_row(const ct_bn_desc *d, float *row, void *stream)
{
    if (!row) CT_FAIL_ARG("ct_bn_stats_row: null pointer (row)");
    if (misaligned(row)) CT_FAIL_ARG("ct_bn_stats_row: row must be 16-byte aligned");
    return bn_stats("ct_bn_stats_row", d, row, stream);
}

extern "C" int ct_bn_relu_apply(const ct_bn_desc *d, void *stream)
{
    ct_bn_act_desc w;
    CT_TRY(widen("ct_bn_relu_apply", d, CT_BN_ACT_RELU, &w));
    return bn_apply("ct_bn_relu_apply", &w, stream);
}

extern "C" int ct_bn_relu_backward(const ct_bn_desc *d, void *stream)
{
    ct_bn_act_desc w;
    CT_TRY(widen("ct_bn_relu_backward", d, CT_BN_ACT_RELU, &w));
    return bn_backward("ct_bn_relu_backward", "ct_bn_workspace_bytes", &w, stream);
}

extern "C" int ct_bn_act_apply(const ct_bn_act_desc *d, void *stream) { return bn_apply("ct_bn_act_apply", d, stream); }

extern "C" int ct_bn_act_backward(const ct_bn_act_desc *d, void *stream)
{
    return bn_backward("ct_bn_act_backward", "ct_bn_act_workspace_bytes", d, stream);
}
