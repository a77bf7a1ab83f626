// The trainable DLA-34 backbone (BasicBlock / Root / Tree / DLA, dla.py:38-66,154-316) for gfx950, fp32, NHWC views with a
// channel pitch: the backward of the 3x3 stride-2 convolution, BatchNorm with an optional residual and an optional ReLU,
// forward and backward, and the backward of the 2x2 max-pool.  Specification: torch.autograd of F.conv2d(stride 2, pad 1),
// of F.batch_norm (+ res) (+ relu) and of F.max_pool2d(2, 2).  DESIGN.md section 13.
//
//   * conv_s2_gx_kernel: gx[n,iy,ix,ci] = sum gy[n,oy,ox,co] * w[co,ci,ky,kx] over iy + 1 - ky = 2 oy, ix + 1 - kx = 2 ox, on
//     v_mfma_f32_16x16x4_f32 with no zero-inserted map and no scatter.  Cell (cy,cx) of the output grid owns the 2x2 input
//     pixels (2cy+a, 2cx+b); along one axis a = 0 meets tap 1 at cy, a = 1 meets tap 2 at cy and tap 0 at cy + 1: the nine
//     taps appear once per cell.  A workgroup owns 4 rows x 16 columns of cells of one image and 32 input channels; it stages
//     the gy tile plus one halo row and column (zero outside the map) 64 couts at a time in LDS, wave r runs the nine tap
//     GEMMs of cell row r (A = gy from LDS, B = the weight in ct_pack_conv_weight_s2t's fragment order straight from global,
//     K = Cout in ascending order) into 4 parities x 2 channel tiles and stores 2x2 pixels per cell.
//   * conv_s2_gw_kernel: gw[co,ci,ky,kx] = sum_{n,oy,ox} gy[n,oy,ox,co] * x[n,2oy-1+ky,2ox-1+kx,ci]: the plan of
//     conv_bwd_weight_kernel (heads_bwd.hip) with the strided tap -- a workgroup owns one (tap, 32 input channels, up to 64
//     couts) block and one K slab of output pixels, its four waves split the slab, are summed through LDS in wave order and
//     the partial block goes to slab `blockIdx.y` of the workspace; s2_slab_reduce_kernel adds the slabs in slab order.
//   * bn_act_reduce_kernel / bn_act_finalize_kernel / bn_act_apply_kernel / bn_act_bwd_kernel: the kernels of neck_bwd.hip
//     (same plan, same order of every sum, same bn_pre) with y = fma(z - mean, a, beta) (+ res) (max 0), the mask recomputed from
//     the same bits, and gres = g.  With the ReLU and no residual the results are those of ct_bn_relu_* bit for bit.
//   * maxpool_bwd_kernel: thread = one 2x2 window and channel quad; the window's gradient goes to its first maximum in
//     row-major order (torch's rule: a later value wins only if it is greater or NaN), the other three get 0, plus `add`.
// No atomics anywhere; slab counts depend on the shapes only: every result is bitwise equal from run to run.
// Every view is addressed with 32-bit offsets or one buffer descriptor, so a view stays below 2 GiB (checked on the host).
#include "ct_common.h"

namespace {

constexpr int SENTINEL = (int)0x80000000;     // vector offset of a zero-reading buffer access (ct_common.h)
const double VIEW_LIMIT = 2147483648.0;

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t view_rsrc(const float *p, size_t pixels, int ld, int C)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, (int)(((pixels - 1) * ld + C) * 4u), 0x00020000);
}

__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, int voff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}

// the pre-activation of BatchNorm that forward and backward share, a = gamma * invstd (neck_bwd.hip's, which says why the
// difference comes first)
__device__ __forceinline__ float bn_pre(float z, float mean, float a, float beta) { return fmaf(z - mean, a, beta); }

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

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

unsigned ew_grid(int total) { return (unsigned)(total < 2048 * 256 ? ct_cdiv(total, 256) : 2048); }

// ---------------------------------------------------------------------------------------------------------------------
// the 3x3 stride-2 convolution

constexpr int GX_TW = 16;        // cells of a workgroup along x: the M of one MFMA
constexpr int GX_TH = 4;         // cell rows of a workgroup: one per wave
constexpr int GX_KC = 64;        // couts per staged chunk
constexpr int GX_KS = 68;        // LDS pitch of a staged pixel (floats)

struct S2Args {
    const float *x, *gy, *wt;
    float *gx, *ws;
    int N, H, W, Cin, Cout, ldx, ldgy, ldgx;
    int Ho, Wo, tilesX, tilesY, cgroups;
    int NT, stepsPerWave;
    size_t slabStride;
};

__global__ __launch_bounds__(256) void pack_s2t_kernel(const float *w, float *packed, int Cout, int Cin)
{
    const int total = Cout * Cin * 9;
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    // packed[tap][Cout/4][Cin/16][lane = (co % 4) * 16 + ci % 16]
    const int lane = i & 63;
    int r = i >> 6;
    const int c16 = r % (Cin / 16);
    r /= Cin / 16;
    const int k4 = r % (Cout / 4), tap = r / (Cout / 4);
    const int co = k4 * 4 + (lane >> 4), ci = c16 * 16 + (lane & 15);
    packed[i] = w[((size_t)co * Cin + ci) * 9 + tap];
}

__global__ __launch_bounds__(256) void conv_s2_gx_kernel(S2Args a)
{
    __shared__ __attribute__((aligned(16))) float tile[(GX_TH + 1) * (GX_TW + 1) * GX_KS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int unit = blockIdx.x;
    const int cig = unit % a.cgroups;
    unit /= a.cgroups;
    const int tx = unit % a.tilesX;
    unit /= a.tilesX;
    const int ty = unit % a.tilesY, n = unit / a.tilesY;
    const int cy0 = ty * GX_TH, cx0 = tx * GX_TW;
    const int c16 = a.Cin >> 4, k4n = a.Cout >> 2;
    const bool has1 = cig * 2 + 1 < c16;                    // (Cin % 32 == 16: the last group is one tile wide)
    const int nct = has1 ? 2 : 1;
    f32x4 acc[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[p][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Cout; k0 += GX_KC) {
        __syncthreads();
        for (int i = threadIdx.x; i < (GX_TH + 1) * (GX_TW + 1) * (GX_KC / 4); i += 256) {
            const int q = i & 15, p = i >> 4;
            const int r = p / (GX_TW + 1), c = p - r * (GX_TW + 1);
            const int oy = cy0 + r, ox = cx0 + c, co = k0 + q * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (oy < a.Ho && ox < a.Wo && co < a.Cout) v = ld4(a.gy + ((n * a.Ho + oy) * a.Wo + ox) * a.ldgy + co);
            st4(tile + p * GX_KS + q * 4, v);
        }
        __syncthreads();
        const int kmax = min(GX_KC, a.Cout - k0);
        const float *t = tile + (wave * (GX_TW + 1) + (lane & 15)) * GX_KS + (lane >> 4);
        for (int kk = 0; kk < kmax; kk += 4) {
            const float a00 = t[kk], a01 = t[kk + GX_KS], a10 = t[kk + (GX_TW + 1) * GX_KS], a11 = t[kk + (GX_TW + 2) * GX_KS];
            const float *wb = a.wt + ((size_t)((k0 + kk) >> 2) * c16 + cig * 2) * 64 + lane;
            const size_t tapStride = (size_t)k4n * c16 * 64;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                if (ct < nct) {                                      // (uniform)
                    float w[9];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) w[tap] = wb[tap * tapStride + ct * 64];
                    // parity (a, b) of the cell's pixel (2cy + a, 2cx + b); tap = ky * 3 + kx
                    acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a00, w[4], acc[0][ct], 0, 0, 0);
                    acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a00, w[5], acc[1][ct], 0, 0, 0);
                    acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a01, w[3], acc[1][ct], 0, 0, 0);
                    acc[2][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a00, w[7], acc[2][ct], 0, 0, 0);
                    acc[2][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a10, w[1], acc[2][ct], 0, 0, 0);
                    acc[3][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a00, w[8], acc[3][ct], 0, 0, 0);
                    acc[3][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a01, w[6], acc[3][ct], 0, 0, 0);
                    acc[3][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a10, w[2], acc[3][ct], 0, 0, 0);
                    acc[3][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a11, w[0], acc[3][ct], 0, 0, 0);
                }
            }
        }
    }
    const int cy = cy0 + wave;
    if (cy >= a.Ho) return;
    const int ci = cig * 32 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int cx = cx0 + (lane >> 4) * 4 + e;
        if (cx >= a.Wo) continue;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float *dst = a.gx + ((n * a.H + 2 * cy + (p >> 1)) * a.W + 2 * cx + (p & 1)) * a.ldgx + ci;
            dst[0] = acc[p][0][e];
            if (has1) dst[16] = acc[p][1][e];
        }
    }
}

constexpr int W_TILES = 8;       // accumulator tiles of a wave: 2 channel tiles x 4 cout tiles

__global__ __launch_bounds__(256) void conv_s2_gw_kernel(S2Args a)
{
    __shared__ float red[3][W_TILES][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HWo = a.Ho * a.Wo;
    const int total = a.N * HWo;
    int unit = blockIdx.x;
    const int k = unit % 9;
    unit /= 9;
    const int cig = unit % a.cgroups, cog = unit / a.cgroups;
    const int ky = k / 3, kx = k - ky * 3;
    const int nco = min(4, a.NT - cog * 4);
    const __amdgpu_buffer_rsrc_t xrs = view_rsrc(a.x, (size_t)a.N * a.H * a.W, a.ldx, a.Cin);
    const __amdgpu_buffer_rsrc_t gyrs = view_rsrc(a.gy, (size_t)total, a.ldgy, a.Cout);
    const int c0 = cig * 32 + (lane & 15);
    const bool has1 = c0 + 16 < a.Cin;
    f32x4 acc[W_TILES];
#pragma unroll
    for (int i = 0; i < W_TILES; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (total + 3) >> 2;
    const int s0 = min(nsteps, ((int)blockIdx.y * 4 + wave) * a.stepsPerWave);
    const int s1 = min(nsteps, s0 + a.stepsPerWave);
    // four steps (16 output pixels) per round: the loads of all four are in flight together
    for (int st = s0; st < s1; st += 4) {
        float col[4][2], g[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int gp = (st + u) * 4 + (lane >> 4);
            const bool live = st + u < s1 && gp < total;
            const int n = gp / HWo, pix = gp - n * HWo, oy = pix / a.Wo, ox = pix - oy * a.Wo;
            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
            const bool inside = live && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const int xo = ((n * a.H + iy) * a.W + ix) * a.ldx;
            col[u][0] = bload(xrs, inside ? (xo + c0) * 4 : SENTINEL);
            col[u][1] = bload(xrs, (inside && has1) ? (xo + c0 + 16) * 4 : SENTINEL);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int co = (cog * 4 + ct) * 16 + (lane & 15);
                g[u][ct] = bload(gyrs, (live && ct < nco) ? (gp * a.ldgy + co) * 4 : SENTINEL);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (ct < nco) {                                  // (uniform)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][0], acc[ct], 0, 0, 0);
                    acc[4 + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][1], acc[4 + ct], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' partial blocks, summed in wave order
    if (wave) {
#pragma unroll
        for (int i = 0; i < W_TILES; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave - 1][i][e][lane] = acc[i][e];
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int i = 0; i < W_TILES; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = ((acc[i][e] + red[0][i][e][lane]) + red[1][i][e][lane]) + red[2][i][e][lane];
    float *slab = a.ws + (size_t)blockIdx.y * a.slabStride;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        if (ct >= nco) break;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = (cog * 4 + ct) * 16 + (lane >> 4) * 4 + e;
            slab[((size_t)co * a.Cin + c0) * 9 + k] = acc[ct][e];
            if (has1) slab[((size_t)co * a.Cin + c0 + 16) * 9 + k] = acc[4 + ct][e];
        }
    }
}

__global__ __launch_bounds__(256) void s2_slab_reduce_kernel(const float *ws, int slabs, size_t slabStride, float *gw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slabStride) return;
    float s = 0.0f;
    for (int j = 0; j < slabs; ++j) s += ws[(size_t)j * slabStride + i];
    gw[i] = s;
}

struct S2Plan {
    int Ho, Wo, tilesX, tilesY, cgroups, gxUnits;
    int NT, gwUnits, slabs, stepsPerWave;
    size_t slabStride;
};

int make_s2_plan(const char *fn, const ct_conv_s2_bwd_desc *d, S2Plan *p)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->H % 2 || d->W % 2) CT_FAIL_ARG("%s: H=%d, W=%d must be even", fn, d->H, d->W);
    if (d->Cin <= 0 || d->Cin % 16) CT_FAIL_ARG("%s: Cin=%d must be a positive multiple of 16", fn, d->Cin);
    if (d->Cout <= 0 || d->Cout % 16) CT_FAIL_ARG("%s: Cout=%d must be a positive multiple of 16", fn, d->Cout);
    if (d->flags) CT_FAIL_ARG("%s: flags=%d (reserved, 0)", fn, d->flags);
    p->Ho = d->H / 2;
    p->Wo = d->W / 2;
    const double pin = (double)d->N * d->H * d->W, pout = pin / 4;
    int ldin = d->Cin;
    if (d->ldx > ldin) ldin = d->ldx;
    if (d->gx && d->ldgx > ldin) ldin = d->ldgx;
    if (pin * ldin * 4.0 >= VIEW_LIMIT || pout * (d->ldgy > d->Cout ? d->ldgy : d->Cout) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernels address a view with 32-bit offsets", fn, pin);
    p->tilesX = ct_cdiv(p->Wo, GX_TW);
    p->tilesY = ct_cdiv(p->Ho, GX_TH);
    p->cgroups = ct_cdiv(d->Cin, 32);
    const double gxUnits = (double)d->N * p->tilesX * p->tilesY * p->cgroups;
    p->NT = d->Cout / 16;
    const double gwUnits = 9.0 * p->cgroups * ct_cdiv(p->NT, 4);
    if (gxUnits > 2147483647.0 || gwUnits > 2147483647.0) CT_FAIL_ARG("%s: grid too large", fn);
    p->gxUnits = (int)gxUnits;
    p->gwUnits = (int)gwUnits;
    const int nsteps = ct_cdiv(d->N * p->Ho * p->Wo, 4);
    int slabs = ct_cdiv(1024, p->gwUnits);
    const int maxSlabs = ct_cdiv(nsteps, 32);           // at least 8 steps for each of the four waves
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->slabs = slabs;
    p->stepsPerWave = ct_cdiv(nsteps, slabs * 4);
    p->slabStride = (size_t)d->Cout * d->Cin * 9;
    return CT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm (+ residual) (+ ReLU)

struct BnActArgs {
    const float *z, *gy, *gamma, *beta, *mean, *invstd, *res;
    float *y, *gz, *gres, *ggamma, *gbeta, *ws;
    int P, C, ldz, ldy, ldgy, ldgz, ldr, ldgres;
    int cw, rows, pixPerSlab, slabs, batchStats, relu;
};

// the incoming gradient behind the activation: the forward's own bits decide the mask (torch's ReLU: 0 at exactly 0)
__device__ __forceinline__ float act_grad(const BnActArgs &a, float z, float mean, float ka, float beta, float r, float gy)
{
    if (!a.relu) return gy;
    float t = bn_pre(z, mean, ka, beta);
    if (a.res) t += r;
    return t > 0.0f ? gy : 0.0f;
}

__global__ __launch_bounds__(256) void bn_act_reduce_kernel(BnActArgs a)
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
            if (a.res) rv = ld4(a.res + p * a.ldr + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float g = act_grad(a, z[i], mean[i], ka[i], be[i], rv[i], gy[i]);
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

__global__ __launch_bounds__(256) void bn_act_finalize_kernel(BnActArgs a)
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

__global__ __launch_bounds__(256) void bn_act_apply_kernel(BnActArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (a.res) rv = ld4(a.res + p * a.ldr + c);
        f32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = bn_pre(z[i], mean[i], ga[i] * istd[i], be[i]);
            if (a.res) t += rv[i];
            y[i] = a.relu ? fmaxf(t, 0.0f) : t;
        }
        st4(a.y + p * a.ldy + c, y);
    }
}

__global__ __launch_bounds__(256) void bn_act_bwd_kernel(BnActArgs a)
{
    const int C4 = a.C >> 2, total = a.P * C4;
    const float *sums = a.ws + (size_t)a.slabs * 2 * a.C;
    const float invP = 1.0f / (float)a.P;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const f32x4 z = ld4(a.z + p * a.ldz + c), gy = ld4(a.gy + p * a.ldgy + c);
        const f32x4 ga = ld4(a.gamma + c), be = ld4(a.beta + c), mean = ld4(a.mean + c), istd = ld4(a.invstd + c);
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (a.res) rv = ld4(a.res + p * a.ldr + c);
        f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = sg;
        if (a.batchStats && a.gz) {
            sg = ld4(sums + c);
            sgx = ld4(sums + a.C + c);
        }
        f32x4 gz, gr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ka = ga[i] * istd[i];
            const float g = act_grad(a, z[i], mean[i], ka, be[i], rv[i], gy[i]);
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

struct BnPlan {
    int P, cw, rows, chunks, slabs, pixPerSlab;
};

// make_bn_plan of neck_bwd.hip for the wider descriptor: the same slabs, so the same sums
int make_bn_act_plan(const char *fn, const ct_bn_act_desc *d, BnPlan *p)
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

size_t bn_act_ws_bytes(const ct_bn_act_desc *d, const BnPlan &p) { return (size_t)(p.slabs + 1) * 2 * d->C * sizeof(float); }

BnActArgs bn_act_args(const ct_bn_act_desc *d, const BnPlan &p)
{
    BnActArgs a;
    a.z = d->z; a.gy = d->gy; a.gamma = d->gamma; a.beta = d->beta; a.mean = d->mean; a.invstd = d->invstd; a.res = d->res;
    a.y = d->y; a.gz = d->gz; a.gres = d->gres; a.ggamma = d->ggamma; a.gbeta = d->gbeta; a.ws = d->workspace;
    a.P = p.P; a.C = d->C; a.ldz = d->ldz; a.ldy = d->ldy; a.ldgy = d->ldgy; a.ldgz = d->ldgz; a.ldr = d->ldr; a.ldgres = d->ldgres;
    a.cw = p.cw; a.rows = p.rows; a.pixPerSlab = p.pixPerSlab; a.slabs = p.slabs;
    a.batchStats = (d->flags & CT_BN_BATCH_STATS) != 0;
    a.relu = (d->flags & CT_BN_ACT_RELU) != 0;
    return a;
}

int check_bn_act_common(const char *fn, const ct_bn_act_desc *d)
{
    CT_TRY(check_view(fn, "z", d->z, d->ldz, d->C));
    CT_TRY(check_vec(fn, "gamma", d->gamma));
    CT_TRY(check_vec(fn, "beta", d->beta));
    CT_TRY(check_vec(fn, "mean", d->mean));
    CT_TRY(check_vec(fn, "invstd", d->invstd));
    if (d->res) CT_TRY(check_view(fn, "res", d->res, d->ldr, d->C));
    return CT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the 2x2 max-pool

struct PoolArgs {
    const float *x, *gy, *add;
    float *gx;
    int N, Ho, Wo, C, ldx, ldgy, ldadd, ldgx;
};

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(PoolArgs a)
{
    const int C4 = a.C >> 2, total = a.N * a.Ho * a.Wo * C4;
    const int W = a.Wo * 2;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx / C4, c = (idx - p * C4) * 4;
        const int ox = p % a.Wo, t = p / a.Wo, oy = t % a.Ho, n = t / a.Ho;
        const int p00 = (n * a.Ho * 2 + oy * 2) * W + ox * 2;
        const int pix[4] = {p00, p00 + 1, p00 + W, p00 + W + 1};        // row-major order of the window
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ld4(a.x + pix[j] * a.ldx + c);
        const f32x4 g = ld4(a.gy + p * a.ldgy + c);
        int sel[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float best = v[0][i];
            int s = 0;
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const float u = v[j][i];
                if (u > best || u != u) {                                // torch: a later value wins if greater or NaN
                    best = u;
                    s = j;
                }
            }
            sel[i] = s;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = sel[i] == j ? 0.0f + g[i] : 0.0f;
            if (a.add) {
                const f32x4 ad = ld4(a.add + pix[j] * a.ldadd + c);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] += ad[i];
            }
            st4(a.gx + pix[j] * a.ldgx + c, o);
        }
    }
}

}  // namespace

extern "C" size_t ct_packed_conv_weight_s2t_elems(int Cout, int Cin)
{
    if (Cout <= 0 || Cin <= 0 || Cout % 16 || Cin % 16) return 0;
    return (size_t)Cout * Cin * 9;
}

extern "C" int ct_pack_conv_weight_s2t(const float *w_oihw, float *packed, int Cout, int Cin, void *stream)
{
    const char *fn = "ct_pack_conv_weight_s2t";
    if (!w_oihw || !packed) CT_FAIL_ARG("%s: null pointer (w_oihw / packed)", fn);
    if (Cout <= 0 || Cout % 16) CT_FAIL_ARG("%s: Cout=%d must be a positive multiple of 16", fn, Cout);
    if (Cin <= 0 || Cin % 16) CT_FAIL_ARG("%s: Cin=%d must be a positive multiple of 16", fn, Cin);
    if ((double)Cout * Cin * 9 > 2147483647.0) CT_FAIL_ARG("%s: more than 2^31 - 1 weights", fn);
    hipLaunchKernelGGL(pack_s2t_kernel, dim3((unsigned)ct_cdiv(Cout * Cin * 9, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw,
                       packed, Cout, Cin);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

extern "C" size_t ct_conv2d_s2_backward_workspace_bytes(const ct_conv_s2_bwd_desc *d)
{
    S2Plan p;
    if (!d || make_s2_plan("ct_conv2d_s2_backward_workspace_bytes", d, &p) != CT_OK) return 0;
    return (size_t)p.slabs * p.slabStride * sizeof(float);
}

extern "C" int ct_conv2d_s2_backward(const ct_conv_s2_bwd_desc *d, void *stream)
{
    const char *fn = "ct_conv2d_s2_backward";
    S2Plan p;
    CT_TRY(make_s2_plan(fn, d, &p));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->Cout));
    if (!d->gx && !d->gw) CT_FAIL_ARG("%s: no output asked for (gx / gw)", fn);
    if (d->gx) {
        CT_TRY(check_view(fn, "gx", d->gx, d->ldgx, d->Cin));
        CT_TRY(check_vec(fn, "w_s2t", d->w_s2t));
    }
    if (d->gw) {
        CT_TRY(check_view(fn, "x", d->x, d->ldx, d->Cin));
        const size_t need = (size_t)p.slabs * p.slabStride * sizeof(float);
        if (!d->workspace || d->workspace_bytes < need || misaligned(d->workspace)) {
            ct_set_error("%s: a 16-byte aligned workspace of %zu bytes needed (ct_conv2d_s2_backward_workspace_bytes), got %zu", fn,
                         need, d->workspace ? d->workspace_bytes : (size_t)0);
            return CT_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    S2Args a;
    a.x = d->x; a.gy = d->gy; a.wt = d->w_s2t; a.gx = d->gx; a.ws = d->workspace;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.ldx = d->ldx; a.ldgy = d->ldgy; a.ldgx = d->ldgx;
    a.Ho = p.Ho; a.Wo = p.Wo; a.tilesX = p.tilesX; a.tilesY = p.tilesY; a.cgroups = p.cgroups;
    a.NT = p.NT; a.stepsPerWave = p.stepsPerWave; a.slabStride = p.slabStride;
    if (d->gw) {
        hipLaunchKernelGGL(conv_s2_gw_kernel, dim3((unsigned)p.gwUnits, (unsigned)p.slabs), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_conv2d_s2_backward (weight)");
        hipLaunchKernelGGL(s2_slab_reduce_kernel, dim3((unsigned)((p.slabStride + 255) / 256)), dim3(256), 0, s, d->workspace, p.slabs,
                           p.slabStride, d->gw);
        CT_CHECK_LAUNCH("ct_conv2d_s2_backward (reduce)");
    }
    if (d->gx) {
        hipLaunchKernelGGL(conv_s2_gx_kernel, dim3((unsigned)p.gxUnits), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_conv2d_s2_backward (input)");
    }
    return CT_OK;
}

extern "C" size_t ct_bn_act_workspace_bytes(const ct_bn_act_desc *d)
{
    BnPlan p;
    if (!d || make_bn_act_plan("ct_bn_act_workspace_bytes", d, &p) != CT_OK) return 0;
    return bn_act_ws_bytes(d, p);
}

extern "C" int ct_bn_act_apply(const ct_bn_act_desc *d, void *stream)
{
    const char *fn = "ct_bn_act_apply";
    BnPlan p;
    CT_TRY(make_bn_act_plan(fn, d, &p));
    CT_TRY(check_bn_act_common(fn, d));
    CT_TRY(check_view(fn, "y", d->y, d->ldy, d->C));
    const BnActArgs a = bn_act_args(d, p);
    hipLaunchKernelGGL(bn_act_apply_kernel, dim3(ew_grid(p.P * (d->C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

extern "C" int ct_bn_act_backward(const ct_bn_act_desc *d, void *stream)
{
    const char *fn = "ct_bn_act_backward";
    BnPlan p;
    CT_TRY(make_bn_act_plan(fn, d, &p));
    CT_TRY(check_bn_act_common(fn, d));
    CT_TRY(check_view(fn, "gy", d->gy, d->ldgy, d->C));
    if (!d->gz && !d->gres && !d->ggamma && !d->gbeta) CT_FAIL_ARG("%s: no output asked for (gz / gres / ggamma / gbeta)", fn);
    if (d->gz) CT_TRY(check_view(fn, "gz", d->gz, d->ldgz, d->C));
    if (d->gres) CT_TRY(check_view(fn, "gres", d->gres, d->ldgres, d->C));
    const bool batch = d->flags & CT_BN_BATCH_STATS;
    const bool sums = d->ggamma || d->gbeta || (d->gz && batch);
    if (sums) {
        const size_t need = bn_act_ws_bytes(d, p);
        if (!d->workspace || d->workspace_bytes < need || misaligned(d->workspace)) {
            ct_set_error("%s: a 16-byte aligned workspace of %zu bytes needed (ct_bn_act_workspace_bytes), got %zu", fn, need,
                         d->workspace ? d->workspace_bytes : (size_t)0);
            return CT_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const BnActArgs a = bn_act_args(d, p);
    if (sums) {
        hipLaunchKernelGGL(bn_act_reduce_kernel, dim3((unsigned)p.slabs, (unsigned)p.chunks), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_act_backward (sums)");
        hipLaunchKernelGGL(bn_act_finalize_kernel, dim3((unsigned)ct_cdiv(d->C, 256)), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_act_backward (reduce)");
    }
    if (d->gz || d->gres) {
        hipLaunchKernelGGL(bn_act_bwd_kernel, dim3(ew_grid(p.P * (d->C / 4))), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_bn_act_backward (gz)");
    }
    return CT_OK;
}

extern "C" int ct_maxpool2x2_backward(const float *x, int N, int H, int W, int C, int ldx, const float *gy, int ldgy,
                                      const float *add, int ldadd, float *gx, int ldgx, void *stream)
{
    const char *fn = "ct_maxpool2x2_backward";
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (H % 2 || W % 2) CT_FAIL_ARG("%s: H=%d, W=%d must be even", fn, H, W);
    if (C % 4) CT_FAIL_ARG("%s: C=%d must be a multiple of 4", fn, C);
    CT_TRY(check_view(fn, "x", x, ldx, C));
    CT_TRY(check_view(fn, "gy", gy, ldgy, C));
    CT_TRY(check_view(fn, "gx", gx, ldgx, C));
    if (add) CT_TRY(check_view(fn, "add", add, ldadd, C));
    int ld = ldx > ldgx ? ldx : ldgx;
    if (add && ldadd > ld) ld = ldadd;
    const double px = (double)N * H * W;
    if (px * ld * 4.0 >= VIEW_LIMIT || px / 4 * ldgy * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernel addresses a view with 32-bit offsets", fn, px);
    PoolArgs a;
    a.x = x; a.gy = gy; a.add = add; a.gx = gx;
    a.N = N; a.Ho = H / 2; a.Wo = W / 2; a.C = C; a.ldx = ldx; a.ldgy = ldgy; a.ldadd = ldadd; a.ldgx = ldgx;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_grid(N * a.Ho * a.Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}
