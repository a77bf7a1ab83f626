// The trainable neck (DeformConv / IDAUp / DLAUp, dla.py:506-574) for gfx950, fp32, NHWC views with a channel pitch:
// BatchNorm statistics, BatchNorm + ReLU forward and backward, the backward of ct_upsample_add and the sigmoid derivative
// of the DCN mask channels.  Specification: torch.autograd of F.batch_norm + relu and of F.conv_transpose2d(groups = C).
// DESIGN.md section 12.
//
//   * bn_reduce_kernel<MODE>: per-channel sums over the N*H*W pixels.  A workgroup owns one slab of pixels and one chunk
//     of up to 64 channel quads; thread (row r, quad q) adds the pixels r, r + rows, ... of the slab in ascending order
//     (16-byte loads), the rows are added through LDS in row order, and the workgroup stores its partial into slab
//     `blockIdx.x` of the workspace.  bn_finalize_kernel<MODE> adds the slabs in slab order.
//       MODE 0: sum (z - z[pixel 0]) -> mean.  MODE 1: sum (z - mean)^2 -> biased variance, invstd (two passes, never E[x^2] - E[x]^2).
//       MODE 2: sum g and sum g * xhat with g = gy where the recomputed pre-activation is > 0 -> gbeta, ggamma.
//   * bn_relu_apply_kernel: y = max(0, fma(z - mean, a, beta)), a = gamma * invstd (bn_pre below: the backward recomputes
//     the same bits from the same four vectors).
//   * bn_relu_bwd_kernel: gz = a * (g - mean(g) - xhat * mean(g * xhat)) with batch statistics, a * g with running ones.
//   * up_gx_kernel: gx[n,iy,ix,c] = sum_{ky,kx < 2f} gy[n, iy*f - f/2 + ky, ix*f - f/2 + kx, c] * w[ky,kx,c], a gather in
//     tap order.  up_gw_kernel<F>: gw[c,ky,kx] = sum_{n,iy,ix} x * gy; a workgroup owns a slab of input pixels and 16
//     channel quads, thread (tap lane t, quad q) keeps F*F/4 taps in registers and walks the slab's pixels in ascending
//     order; up_gw_reduce_kernel adds the slabs in slab order into the module's [C,1,2f,2f] layout.
//   * mask_sigmoid_bwd_kernel: g *= m * (1 - m) on channels 18..26 of the offset/mask gradient.
// No atomics anywhere; slab counts depend on the shapes only: every result is bitwise equal from run to run.
// Every view is addressed with 32-bit element offsets, so a view stays below 2 GiB (checked on the host).
#include "ct_common.h"

namespace {

const double VIEW_LIMIT = 2147483648.0;

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// The pre-activation of BatchNorm that forward and backward share, a = gamma * invstd.  The difference comes first: z - mean
// is exact where z lies within a factor of two of the mean, so what is left of a channel with |mean| >> std is the rounding
// of the fp32 mean itself times a.  The folded form fma(z, a, fma(-mean, a, beta)) rounds the shift at the size of mean * a
// on top of that: at mean 100, std 0.01 half an ulp of 1e4, 5e-4 of a pre-activation of order 1.
__device__ __forceinline__ float bn_pre(float z, float mean, float a, float beta) { return fmaf(z - mean, a, beta); }

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm

struct BnArgs {
    const float *z, *gy, *gamma, *beta;
    float *mean, *var, *invstd;
    float *y, *gz, *ggamma, *gbeta, *ws;
    int P, C, ldz, ldy, ldgy, ldgz;
    int cw, rows, pixPerSlab, slabs, batchStats;
    float eps;
};

template <int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(BnArgs a)
{
    __shared__ f32x4 red[MODE == 2 ? 2 : 1][256];      // the second sum exists in mode 2 only
    const int q = threadIdx.x % a.cw, r = threadIdx.x / a.cw;
    const int c = ((int)blockIdx.y * a.cw + q) * 4;
    const bool live = r < a.rows && c < a.C;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const int p0 = (int)blockIdx.x * a.pixPerSlab, p1 = min(a.P, p0 + a.pixPerSlab);
        f32x4 mean = {0.f, 0.f, 0.f, 0.f}, istd = mean, ka = mean, be = mean;
        if (MODE == 0) mean = ld4(a.z + c);                      // the pivot: pixel 0 of the view (a sum of z - pivot keeps
        if (MODE >= 1) mean = ld4(a.mean + c);                  // a channel of mean 100, std 0.01 exact where a sum of z loses it)
        if (MODE == 2) {
            istd = ld4(a.invstd + c);
            const f32x4 ga = ld4(a.gamma + c);
            be = ld4(a.beta + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) ka[i] = ga[i] * istd[i];
        }
        for (int p = p0 + r; p < p1; p += a.rows) {
            const f32x4 z = ld4(a.z + p * a.ldz + c);
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s0[i] += z[i] - mean[i];
            } else if (MODE == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = z[i] - mean[i];
                    s0[i] = fmaf(d, d, s0[i]);
                }
            } else {
                const f32x4 gy = ld4(a.gy + p * a.ldgy + c);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float g = bn_pre(z[i], mean[i], ka[i], be[i]) > 0.0f ? gy[i] : 0.0f;      // torch's ReLU: 0 at exactly 0
                    const float xh = (z[i] - mean[i]) * istd[i];
                    s0[i] += g;
                    s1[i] = fmaf(g, xh, s1[i]);
                }
            }
        }
    }
    red[0][threadIdx.x] = s0;
    if (MODE == 2) red[1][threadIdx.x] = s1;
    __syncthreads();
    if (r != 0 || c >= a.C) return;
    for (int k = 1; k < a.rows; ++k) {
        const f32x4 v = red[0][k * a.cw + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) s0[i] += v[i];
        if (MODE == 2) {
            const f32x4 u = red[1][k * a.cw + q];
#pragma unroll
            for (int i = 0; i < 4; ++i) s1[i] += u[i];
        }
    }
    float *slab = a.ws + (size_t)blockIdx.x * 2 * a.C;
    st4(slab + c, s0);
    if (MODE == 2) st4(slab + a.C + c, s1);
}

template <int MODE>
__global__ __launch_bounds__(256) void bn_finalize_kernel(BnArgs a)
{
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    float s0 = 0.0f, s1 = 0.0f;
    for (int j = 0; j < a.slabs; ++j) {
        s0 += a.ws[(size_t)j * 2 * a.C + c];
        if (MODE == 2) s1 += a.ws[(size_t)j * 2 * a.C + a.C + c];
    }
    if (MODE == 0) {
        a.mean[c] = a.z[c] + s0 / (float)a.P;
    } else if (MODE == 1) {
        const float v = s0 / (float)a.P;
        a.var[c] = v;
        a.invstd[c] = 1.0f / sqrtf(v + a.eps);
    } else {
        float *sums = a.ws + (size_t)a.slabs * 2 * a.C;      // what the second pass reads
        sums[c] = s0;
        sums[a.C + c] = s1;
        if (a.gbeta) a.gbeta[c] = s0;
        if (a.ggamma) a.ggamma[c] = s1;
    }
}

__global__ __launch_bounds__(256) void bn_relu_apply_kernel(BnArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[i] = fmaxf(bn_pre(z[i], mean[i], ga[i] * istd[i], be[i]), 0.0f);
        }
        st4(a.y + p * a.ldy + c, y);
    }
}

__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(BnArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    const float *sums = a.ws + (size_t)a.slabs * 2 * a.C;
    const float invP = 1.0f / (float)a.P;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c), gy = ld4(a.gy + p * a.ldgy + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = sg;
        if (a.batchStats) {
            sg = ld4(sums + c);
            sgx = ld4(sums + a.C + c);
        }
        f32x4 gz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ka = ga[i] * istd[i];
            const float g = bn_pre(z[i], mean[i], ka, be[i]) > 0.0f ? gy[i] : 0.0f;
            if (a.batchStats) {
                const float xh = (z[i] - mean[i]) * istd[i];
                gz[i] = ka * ((g - sg[i] * invP) - xh * (sgx[i] * invP));
            } else {
                gz[i] = ka * g;
            }
        }
        st4(a.gz + p * a.ldgz + c, gz);
    }
}

struct BnPlan {
    int P, cw, rows, chunks, slabs, pixPerSlab;
};

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

int make_bn_plan(const char *fn, const ct_bn_desc *d, BnPlan *p)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->C % 4) CT_FAIL_ARG("%s: C=%d must be a multiple of 4", fn, d->C);
    if (d->flags & ~CT_BN_BATCH_STATS) CT_FAIL_ARG("%s: flags=%d (0 or CT_BN_BATCH_STATS)", fn, d->flags);
    const double px = (double)d->N * d->H * d->W;
    int ld = d->ldz;
    if (d->y && d->ldy > ld) ld = d->ldy;
    if (d->gy && d->ldgy > ld) ld = d->ldgy;
    if (d->gz && d->ldgz > ld) ld = d->ldgz;
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

// a view the call reads or writes: non-null, 16-byte aligned, pitch a multiple of 4 and at least C
int check_view(const char *fn, const char *name, const void *ptr, int ld, int C)
{
    if (!ptr) CT_FAIL_ARG("%s: null pointer (%s)", fn, name);
    if (ld < C) CT_FAIL_ARG("%s: channel pitch of %s (%d) below the channel count %d", fn, name, ld, C);
    if (ld % 4 || misaligned(ptr)) CT_FAIL_ARG("%s: %s must be 16-byte aligned with a pitch that is a multiple of 4", fn, name);
    return CT_OK;
}

int check_vec(const char *fn, const char *name, const void *ptr)
{
    if (!ptr) CT_FAIL_ARG("%s: null pointer (%s)", fn, name);
    if (misaligned(ptr)) CT_FAIL_ARG("%s: %s must be 16-byte aligned", fn, name);
    return CT_OK;
}

#define CT_TRY(e) do { const int rc__ = (e); if (rc__ != CT_OK) return rc__; } while (0)

size_t bn_ws_bytes(const ct_bn_desc *d, const BnPlan &p) { return (size_t)(p.slabs + 1) * 2 * d->C * sizeof(float); }

int check_bn_ws(const char *fn, const ct_bn_desc *d, const BnPlan &p)
{
    const size_t need = bn_ws_bytes(d, p);
    if (!d->workspace || d->workspace_bytes < need || misaligned(d->workspace)) {
        ct_set_error("%s: a 16-byte aligned workspace of %zu bytes needed (ct_bn_workspace_bytes), got %zu", fn, need,
                     d->workspace ? d->workspace_bytes : (size_t)0);
        return CT_ERR_WORKSPACE;
    }
    return CT_OK;
}

BnArgs bn_args(const ct_bn_desc *d, const BnPlan &p)
{
    BnArgs a;
    a.z = d->z; a.gy = d->gy; a.gamma = d->gamma; a.beta = d->beta;
    a.mean = d->mean; a.var = d->var; a.invstd = d->invstd;
    a.y = d->y; a.gz = d->gz; a.ggamma = d->ggamma; a.gbeta = d->gbeta; a.ws = d->workspace;
    a.P = p.P; a.C = d->C; a.ldz = d->ldz; a.ldy = d->ldy; a.ldgy = d->ldgy; a.ldgz = d->ldgz;
    a.cw = p.cw; a.rows = p.rows; a.pixPerSlab = p.pixPerSlab; a.slabs = p.slabs;
    a.batchStats = (d->flags & CT_BN_BATCH_STATS) != 0;
    a.eps = d->eps;
    return a;
}

unsigned ew_grid(int total) { return (unsigned)(total < 2048 * 256 ? ct_cdiv(total, 256) : 2048); }

// ---------------------------------------------------------------------------------------------------------------------
// backward of ct_upsample_add

struct UpArgs {
    const float *gy, *w, *x;
    float *gx, *gw, *ws;
    int N, H, W, C, f, ldgy, ldgx, ldx;
    int pixPerSlab, slabs;
};

__global__ __launch_bounds__(256) void up_gx_kernel(UpArgs a)
{
    const int C4 = a.C >> 2, total = a.N * a.H * a.W * C4;
    const int f = a.f, kw = 2 * f, pad = f >> 1, Ho = a.H * f, Wo = a.W * f;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const int ix = p % a.W, t = p / a.W, iy = t % a.H, n = t / a.H;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < kw; ++ky) {
            const int oy = iy * f - pad + ky;
            if (oy < 0 || oy >= Ho) continue;
            for (int kx = 0; kx < kw; ++kx) {
                const int ox = ix * f - pad + kx;
                if (ox < 0 || ox >= Wo) continue;
                const f32x4 g = ld4(a.gy + ((n * Ho + oy) * Wo + ox) * a.ldgy + c);
                const f32x4 wv = ld4(a.w + (ky * kw + kx) * a.C + c);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(g[i], wv[i], acc[i]);
            }
        }
        st4(a.gx + p * a.ldgx + c, acc);
    }
}

template <int F>
__global__ __launch_bounds__(256) void up_gw_kernel(UpArgs a)
{
    constexpr int NT = F * F / 4;                  // taps of a thread: 4 F^2 taps over 16 tap lanes
    constexpr int KW = 2 * F;
    const int q = threadIdx.x & 15, t = threadIdx.x >> 4;
    const int c = ((int)blockIdx.y * 16 + q) * 4;
    if (c >= a.C) return;
    const int Ho = a.H * F, Wo = a.W * F, Pin = a.N * a.H * a.W;
    const int p0 = (int)blockIdx.x * a.pixPerSlab, p1 = min(Pin, p0 + a.pixPerSlab);
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = p0; p < p1; ++p) {
        const int ix = p % a.W, r = p / a.W, iy = r % a.H, n = r / a.H;
        const f32x4 xv = ld4(a.x + p * a.ldx + c);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int tap = j * 16 + t;
            const int oy = iy * F - F / 2 + tap / KW, ox = ix * F - F / 2 + tap % KW;
            if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
            const f32x4 g = ld4(a.gy + ((n * Ho + oy) * Wo + ox) * a.ldgy + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = fmaf(xv[i], g[i], acc[j][i]);
        }
    }
    float *slab = a.ws + (size_t)blockIdx.x * (4 * F * F) * a.C;
#pragma unroll
    for (int j = 0; j < NT; ++j) st4(slab + (j * 16 + t) * a.C + c, acc[j]);
}

// ws [slabs][4f^2][C] -> gw [C][4f^2]
__global__ __launch_bounds__(256) void up_gw_reduce_kernel(UpArgs a)
{
    const int taps = 4 * a.f * a.f, total = taps * a.C;
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float s = 0.0f;
    for (int j = 0; j < a.slabs; ++j) s += a.ws[(size_t)j * total + i];
    const int tap = i / a.C, c = i - tap * a.C;
    a.gw[c * taps + tap] = s;
}

struct UpPlan {
    int Pin, chunks, slabs, pixPerSlab;
};

int make_up_plan(const ct_upsample_bwd_desc *d, UpPlan *p)
{
    const char *fn = "ct_upsample_add_backward";
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->f != 2 && d->f != 4 && d->f != 8) CT_FAIL_ARG("%s: f=%d unsupported (2, 4 or 8)", fn, d->f);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->C % 4) CT_FAIL_ARG("%s: C=%d must be a multiple of 4", fn, d->C);
    const double pin = (double)d->N * d->H * d->W, pout = pin * d->f * d->f;
    const int ldin = d->ldx > d->ldgx ? d->ldx : d->ldgx;
    if (pout * (d->ldgy > d->C ? d->ldgy : d->C) * 4.0 >= VIEW_LIMIT || pin * ldin * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*fH*fW=%.0f pixels): the kernels address a view with 32-bit offsets", fn, pout);
    p->Pin = d->N * d->H * d->W;
    p->chunks = ct_cdiv(d->C / 4, 16);
    int slabs = ct_cdiv(512, p->chunks);
    const int maxSlabs = ct_cdiv(p->Pin, 8);                  // at least eight input pixels per slab
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->pixPerSlab = ct_cdiv(p->Pin, slabs);
    p->slabs = ct_cdiv(p->Pin, p->pixPerSlab);
    return CT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the sigmoid of the DCN mask channels

__global__ __launch_bounds__(256) void mask_sigmoid_bwd_kernel(float *g, int ldg, const float *om, int ldom, int total)
{
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p = i / 9, j = 18 + (i - p * 9);
    const float m = om[p * ldom + j];
    g[p * ldg + j] *= m * (1.0f - m);
}

}  // namespace

extern "C" size_t ct_bn_workspace_bytes(const ct_bn_desc *d)
{
    BnPlan p;
    if (!d || make_bn_plan("ct_bn_workspace_bytes", d, &p) != CT_OK) return 0;
    return bn_ws_bytes(d, p);
}

extern "C" int ct_bn_stats(const ct_bn_desc *d, void *stream)
{
    const char *fn = "ct_bn_stats";
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "var", d->var));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    if (!(d->eps >= 0.0f)) CT_FAIL_ARG("%s: eps=%g", fn, (double)d->eps);
    CT_TRY(check_bn_ws(fn, d, p));
    hipStream_t s = (hipStream_t)stream;
    const BnArgs a = bn_args(d, p);
    const dim3 grid((unsigned)p.slabs, (unsigned)p.chunks), fin((unsigned)ct_cdiv(d->C, 256));
    hipLaunchKernelGGL(bn_reduce_kernel<0>, grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (sum)");
    hipLaunchKernelGGL(bn_finalize_kernel<0>, fin, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (mean)");
    hipLaunchKernelGGL(bn_reduce_kernel<1>, grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (squares)");
    hipLaunchKernelGGL(bn_finalize_kernel<1>, fin, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH("ct_bn_stats (variance)");
    return CT_OK;
}

extern "C" int ct_bn_relu_apply(const ct_bn_desc *d, void *stream)
{
    const char *fn = "ct_bn_relu_apply";
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_view(fn, "y", d->y, d->ldy, d->C));
    CT_TRY(check_vec(fn, "gamma", d->gamma));
    CT_TRY(check_vec(fn, "beta", d->beta));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    const BnArgs a = bn_args(d, p);
    hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(ew_grid(p.P * (d->C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH("ct_bn_relu_apply");
    return CT_OK;
}

extern "C" int ct_bn_relu_backward(const ct_bn_desc *d, void *stream)
{
    const char *fn = "ct_bn_relu_backward";
    BnPlan p;
    CT_TRY(make_bn_plan(fn, d, &p));
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->C));
    CT_TRY(check_vec(fn, "gamma", d->gamma));
    CT_TRY(check_vec(fn, "beta", d->beta));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    if (!d->gz && !d->ggamma && !d->gbeta) CT_FAIL_ARG("%s: no output asked for (gz / ggamma / gbeta)", fn);
    if (d->gz) CT_TRY(check_view(fn, "gz", d->gz, d->ldgz, d->C));
    const bool batch = d->flags & CT_BN_BATCH_STATS;
    const bool sums = d->ggamma || d->gbeta || (d->gz && batch);
    if (sums) CT_TRY(check_bn_ws(fn, d, p));
    hipStream_t s = (hipStream_t)stream;
    const BnArgs a = bn_args(d, p);
    if (sums) {
        hipLaunchKernelGGL(bn_reduce_kernel<2>, dim3((unsigned)p.slabs, (unsigned)p.chunks), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_relu_backward (sums)");
        hipLaunchKernelGGL(bn_finalize_kernel<2>, dim3((unsigned)ct_cdiv(d->C, 256)), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_relu_backward (reduce)");
    }
    if (d->gz) {
        hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(ew_grid(p.P * (d->C / 4))), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_relu_backward (gz)");
    }
    return CT_OK;
}

extern "C" size_t ct_upsample_add_backward_workspace_bytes(const ct_upsample_bwd_desc *d)
{
    UpPlan p;
    if (!d || make_up_plan(d, &p) != CT_OK) return 0;
    return (size_t)p.slabs * 4 * d->f * d->f * d->C * sizeof(float);
}

extern "C" int ct_upsample_add_backward(const ct_upsample_bwd_desc *d, void *stream)
{
    const char *fn = "ct_upsample_add_backward";
    UpPlan p;
    CT_TRY(make_up_plan(d, &p));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->C));
    if (!d->gx && !d->gw) CT_FAIL_ARG("%s: no output asked for (gx / gw)", fn);
    if (d->gx) {
        CT_TRY(check_view(fn, "gx", d->gx, d->ldgx, d->C));
        CT_TRY(check_vec(fn, "w", d->w));
    }
    if (d->gw) {
        CT_TRY(check_view(fn, "x", d->x, d->ldx, d->C));
        const size_t need = (size_t)p.slabs * 4 * d->f * d->f * d->C * sizeof(float);
        if (!d->workspace || d->workspace_bytes < need || misaligned(d->workspace)) {
            ct_set_error("%s: a 16-byte aligned workspace of %zu bytes needed (ct_upsample_add_backward_workspace_bytes), got %zu",
                         fn, need, d->workspace ? d->workspace_bytes : (size_t)0);
            return CT_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    UpArgs a;
    a.gy = d->gy; a.w = d->w; a.x = d->x; a.gx = d->gx; a.gw = d->gw; a.ws = d->workspace;
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.f = d->f; a.ldgy = d->ldgy; a.ldgx = d->ldgx; a.ldx = d->ldx;
    a.pixPerSlab = p.pixPerSlab; a.slabs = p.slabs;
    if (d->gx) {
        hipLaunchKernelGGL(up_gx_kernel, dim3(ew_grid(p.Pin * (d->C / 4))), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_upsample_add_backward (gx)");
    }
    if (d->gw) {
        const dim3 grid((unsigned)p.slabs, (unsigned)p.chunks);
        if (d->f == 2) hipLaunchKernelGGL(up_gw_kernel<2>, grid, dim3(256), 0, s, a);
        else if (d->f == 4) hipLaunchKernelGGL(up_gw_kernel<4>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(up_gw_kernel<8>, grid, dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_upsample_add_backward (gw)");
        hipLaunchKernelGGL(up_gw_reduce_kernel, dim3((unsigned)ct_cdiv(4 * d->f * d->f * d->C, 256)), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_upsample_add_backward (reduce)");
    }
    return CT_OK;
}

extern "C" int ct_dcn_mask_sigmoid_backward(float *g, int ldg, const float *om, int ldom, int N, int H, int W, void *stream)
{
    const char *fn = "ct_dcn_mask_sigmoid_backward";
    if (!g || !om) CT_FAIL_ARG("%s: null pointer (g / om)", fn);
    if (N <= 0 || H <= 0 || W <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (ldg < 27 || ldom < 27) CT_FAIL_ARG("%s: channel pitch below 27 (g / om)", fn);
    const double px = (double)N * H * W;
    if (px * (ldg > ldom ? ldg : ldom) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernel addresses a view with 32-bit offsets", fn, px);
    const int total = N * H * W * 9;
    hipLaunchKernelGGL(mask_sigmoid_bwd_kernel, dim3((unsigned)ct_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, g, ldg, om,
                       ldom, total);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}
