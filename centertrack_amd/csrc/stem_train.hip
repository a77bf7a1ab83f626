// The three 7x7 stems of DLA (base_layer, pre_img_layer, pre_hm_layer; Cin 3 / 3 / 1 -> 16) for training, fp32, no atomics:
//   * stem_conv_fwd_kernel: z_s = conv7x7(in_s, w_s), pad 3, no bias, one NHWC [N,H,W,16] map per stem.  The GEMM of stem.hip
//     (M = pixels, N = 16 couts, K = 49 Cin padded to 4 on v_mfma_f32_16x16x4_f32; a workgroup of 4 waves owns 8 x 32 pixels, its
//     input planes with a 3-pixel zero-padded halo and the weights sit in LDS, an A operand is one LDS read at plane[tab[k] +
//     pixel]), without the BatchNorm fold: training-mode BatchNorm needs the raw z.  One launch walks the stems present.
//   * stem_sum_kernel: y = sum_s max(0, fma(z_s - mean_s, a_s, beta_s)), a_s = gamma_s * invstd_s, in the order x, pre_img,
//     pre_hm; each term is ct_bn_relu_apply's expression (bn_pre of ct_train.h), so the backward's recomputed mask is the forward's.
//   * stem_gw_kernel: gw_s[co, j] = sum_p gz_s[p, co] * patch_s[p, j], j = (ci, ky, kx): M = 16 couts, N = 49 Cin columns in
//     16-column tiles (10 / 4), K = pixels.  A workgroup stages the planes of an 8 x 32 pixel tile (+ halo) in LDS, reads gz as
//     the A operand straight from the NHWC map, each wave owns two rows of the tile (16 steps of 4 pixels); workgroup b walks the
//     tiles b, b + slabs, ... and keeps its sums in registers, the waves are added through LDS in wave order and the workgroup
//     writes slab b of the workspace.  stem_gw_reduce_kernel adds the slabs in slab order into OIHW.
//   * stem_gin_kernel: gin_s[n,ci,y,x] = sum_{ky,kx,co} gz_s[n,y-ky+3,x-kx+3,co] * w_s[co,ci,ky,kx]: a 16 x 16 pixel tile of gz
//     (+ halo) and the weights in LDS, one thread per pixel, FMAs in (ky, kx, co) order.  Plain on purpose: training never asks
//     for an image gradient.
// Slab counts depend on the shapes only: every result is bitwise equal from run to run.  DESIGN.md section 14.
#include "ct_train.h"

namespace {

constexpr int TW = 32, TH = 8;                 // pixel tile of the two MFMA kernels
constexpr int PW = 40, PH = TH + 6;            // plane pitch 40 (38 used: the k -> k + 1 wrap lands on another bank), rows
constexpr int PS = PH * PW;                    // floats per plane
constexpr int GW_SLAB_CAP = 512;               // workgroups per stem of the weight gradient
constexpr int GT = 16, GP = GT + 6, GLD = 20;  // image gradient: tile, tile + halo, LDS pitch of one pixel's 16 couts

__host__ __device__ constexpr int cin_of(int s) { return s == 2 ? 1 : 3; }

struct StemTrainArgs {
    const float *in[3];          // NCHW planes; forward / gw
    const float *w[3];           // OIHW [16,Cin,7,7]; forward / gin
    float *z[3];                 // forward output
    const float *gz[3];          // backward input
    int ldz[3], ldgz[3];
    float *gw[3], *gin[3];
    float *ws;
    size_t wsoff[3];             // floats: first slab of stem s
    int act[3], nact;            // stems of this launch (blockIdx.y -> stem)
    int N, H, W, tilesX, tilesY, tiles, slabs;
};

// the input planes of stem s, image n, tile origin (oy0, ox0): rows oy0 - 3 .. oy0 + TH + 2, columns ox0 - 3 .. ox0 + TW + 2
template <int CIN>
__device__ __forceinline__ void stage_planes(float *planes, const float *src, int n, int oy0, int ox0, int H, int W, int tid)
{
    const size_t HW = (size_t)H * W;
    for (int it = tid; it < CIN * PH * 38; it += 256) {
        const int c = it / (PH * 38), r = it - c * (PH * 38);
        const int py = r / 38, px = r - py * 38;
        const int iy = oy0 - 3 + py, ix = ox0 - 3 + px;
        float v = 0.0f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = src[((size_t)n * CIN + c) * HW + (size_t)iy * W + ix];
        planes[c * PS + py * PW + px] = v;
    }
}

__device__ __forceinline__ int patch_offset(int j, int K)      // column j = (ci, ky, kx) -> offset of its tap in the planes
{
    if (j >= K) return 0;
    const int c = j / 49, r = j - c * 49;
    return c * PS + (r / 7) * PW + (r % 7);
}

// ---------------------------------------------------------------------------------------------------------------------
// forward

template <int CIN>
__device__ __forceinline__ void fwd_stem(const StemTrainArgs &a, int s, float *planes, float *wl, int *tab, int n, int oy0, int ox0)
{
    constexpr int K = CIN * 49, K4 = (K + 3) / 4 * 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    stage_planes<CIN>(planes, a.in[s], n, oy0, ox0, a.H, a.W, tid);
    for (int it = tid; it < K4 * 16; it += 256) {              // weights transposed to [k][16], zero behind K
        const int k = it >> 4, j = it & 15;
        wl[it] = k < K ? a.w[s][j * K + k] : 0.0f;
    }
    for (int k = tid; k < K4; k += 256) tab[k] = patch_offset(k, K);
    __syncthreads();
    // wave -> rows 2w, 2w + 1 of the tile; m-tile mt -> (row 2w + mt / 2, column block mt & 1)
    int pbase[4];
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        pbase[mt] = (2 * wave + (mt >> 1)) * PW + (mt & 1) * 16 + li;
        acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 4
    for (int st = 0; st < K4 / 4; ++st) {
        const int k = 4 * st + lg;
        const int off = tab[k];
        const float b = wl[k * 16 + li];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(planes[off + pbase[mt]], b, acc[mt], 0, 0, 0);
    }
    float *z = a.z[s];
    const int ld = a.ldz[s];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int oy = oy0 + 2 * wave + (mt >> 1);
        if (oy >= a.H) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ox = ox0 + (mt & 1) * 16 + lg * 4 + e;
            if (ox < a.W) z[(((size_t)n * a.H + oy) * a.W + ox) * ld + li] = acc[mt][e];
        }
    }
}

__global__ __launch_bounds__(256) void stem_conv_fwd_kernel(StemTrainArgs a)
{
    __shared__ float planes[3 * PS];
    __shared__ float wl[148 * 16];
    __shared__ int tab[148];
    int bid = blockIdx.x;
    const int tx = bid % a.tilesX; bid /= a.tilesX;
    const int ty = bid % a.tilesY; bid /= a.tilesY;
    const int n = bid, oy0 = ty * TH, ox0 = tx * TW;
    for (int i = 0; i < a.nact; ++i) {                          // (uniform)
        const int s = a.act[i];
        if (i) __syncthreads();                                 // the previous stem's reads of the LDS are over
        if (s == 2) fwd_stem<1>(a, s, planes, wl, tab, n, oy0, ox0);
        else fwd_stem<3>(a, s, planes, wl, tab, n, oy0, ox0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm + ReLU of every stem and their sum

struct StemSumArgs {
    const float *z[3], *mean[3], *invstd[3], *gamma[3], *beta[3];
    int ldz[3];
    float *y;
    int ldy, P;
};

__global__ __launch_bounds__(256) void stem_sum_kernel(StemSumArgs a)
{
    const int total = a.P * 4;
    for (int idx = (int)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int)gridDim.x * 256) {
        const int p = idx >> 2, c = (idx & 3) * 4;
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (!a.z[s]) continue;
            const f32x4 z = ld4(a.z[s] + (size_t)p * a.ldz[s] + c);
            const f32x4 ga = ld4(a.gamma[s] + c), be = ld4(a.beta[s] + c), mean = ld4(a.mean[s] + c), istd = ld4(a.invstd[s] + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = ct_relu(bn_pre(z[i], mean[i], ga[i] * istd[i], be[i]));
                y[i] = s == 0 ? t : y[i] + t;
            }
        }
        st4(a.y + (size_t)p * a.ldy + c, y);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient

template <int CIN>
__device__ __forceinline__ void gw_stem(const StemTrainArgs &a, int s, float *planes, float *red)
{
    constexpr int K = CIN * 49, NT = (K + 15) / 16, NCP = NT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    int tabv[NT];
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        tabv[t] = patch_offset(16 * t + li, K);                 // (a column behind K reads tap 0: its sums are never read)
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float *gz = a.gz[s];
    const int ld = a.ldgz[s];
    for (int tile = blockIdx.x; tile < a.tiles; tile += a.slabs) {
        int b = tile;
        const int tx = b % a.tilesX; b /= a.tilesX;
        const int ty = b % a.tilesY; b /= a.tilesY;
        const int n = b, oy0 = ty * TH, ox0 = tx * TW;
        if (tile != (int)blockIdx.x) __syncthreads();           // the previous tile's reads of the planes are over
        stage_planes<CIN>(planes, a.in[s], n, oy0, ox0, a.H, a.W, tid);
        __syncthreads();
#pragma unroll 2
        for (int st = 0; st < 16; ++st) {                       // wave -> rows 2w, 2w + 1; step -> 4 pixels of a row
            const int row = 2 * wave + (st >> 3), col = (st & 7) * 4 + lg;
            const int oy = oy0 + row, ox = ox0 + col;
            float g = 0.0f;
            if (oy < a.H && ox < a.W) g = gz[(((size_t)n * a.H + oy) * a.W + ox) * ld + li];
            const int pix = row * PW + col;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g, planes[tabv[t] + pix], acc[t], 0, 0, 0);
        }
    }
    // waves 1, 2, 3 are added to wave 0 in that order
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) red[(lg * 4 + e) * NCP + 16 * t + li] = acc[t][e];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][e] += red[(lg * 4 + e) * NCP + 16 * t + li];
        }
    }
    if (wave == 0) {
        float *slab = a.ws + a.wsoff[s] + (size_t)blockIdx.x * 16 * NCP;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) slab[(lg * 4 + e) * NCP + 16 * t + li] = acc[t][e];
    }
}

__global__ __launch_bounds__(256) void stem_gw_kernel(StemTrainArgs a)
{
    __shared__ float planes[3 * PS];
    __shared__ float red[16 * 160];
    const int s = a.act[blockIdx.y];
    if (s == 2) gw_stem<1>(a, s, planes, red);
    else gw_stem<3>(a, s, planes, red);
}

__global__ __launch_bounds__(256) void stem_gw_reduce_kernel(StemTrainArgs a)
{
    const int s = a.act[blockIdx.y];
    const int K = cin_of(s) * 49, NCP = (K + 15) / 16 * 16;
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= 16 * K) return;
    const int co = i / K, j = i - co * K;
    const float *p = a.ws + a.wsoff[s] + co * NCP + j;
    float sum = 0.0f;
    for (int b = 0; b < a.slabs; ++b) sum += p[(size_t)b * 16 * NCP];
    a.gw[s][i] = sum;
}

// ---------------------------------------------------------------------------------------------------------------------
// image gradient

template <int CIN>
__device__ __forceinline__ void gin_stem(const StemTrainArgs &a, int s, float *gzt, float *wl)
{
    constexpr int K = CIN * 49;
    const int tid = threadIdx.x;
    const int gtx = (a.W + GT - 1) / GT, gty = (a.H + GT - 1) / GT;
    int b = blockIdx.x;
    const int tx = b % gtx; b /= gtx;
    const int ty = b % gty; b /= gty;
    const int n = b, y0 = ty * GT, x0 = tx * GT;
    for (int i = tid; i < 16 * K; i += 256) {                   // w[co][r] -> wl[r][co], r = (ci, ky, kx)
        const int co = i / K, r = i - co * K;
        wl[r * 16 + co] = a.w[s][i];
    }
    const float *gz = a.gz[s];
    const int ld = a.ldgz[s];
    for (int i = tid; i < GP * GP * 4; i += 256) {
        const int q = i & 3, p = i >> 2;
        const int py = p / GP, px = p - py * GP;
        const int gy = y0 - 3 + py, gx = x0 - 3 + px;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = ld4(gz + (((size_t)n * a.H + gy) * a.W + gx) * ld + 4 * q);
        st4(gzt + p * GLD + 4 * q, v);
    }
    __syncthreads();
    const int lx = tid & 15, ly = tid >> 4;
    float acc[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.0f;
    for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx) {
            const float *g = gzt + ((ly + 6 - ky) * GP + (lx + 6 - kx)) * GLD;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 gv = ld4(g + 4 * q);
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) {
                    const f32x4 wv = ld4(wl + (ci * 49 + ky * 7 + kx) * 16 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[ci] = fmaf(gv[i], wv[i], acc[ci]);
                }
            }
        }
    const int y = y0 + ly, x = x0 + lx;
    if (y < a.H && x < a.W) {
        const size_t HW = (size_t)a.H * a.W;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) a.gin[s][((size_t)n * CIN + ci) * HW + (size_t)y * a.W + x] = acc[ci];
    }
}

__global__ __launch_bounds__(256) void stem_gin_kernel(StemTrainArgs a)
{
    __shared__ __attribute__((aligned(16))) float gzt[GP * GP * GLD];
    __shared__ __attribute__((aligned(16))) float wl[147 * 16];
    const int s = a.act[blockIdx.y];
    if (s == 2) gin_stem<1>(a, s, gzt, wl);
    else gin_stem<3>(a, s, gzt, wl);
}

// ---------------------------------------------------------------------------------------------------------------------
// host

int check_shape(const char *fn, int N, int H, int W, int maxld)
{
    if (N <= 0 || H <= 0 || W <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    const double px = (double)N * H * W;
    if (px * (maxld > 16 ? maxld : 16) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): a 16-channel view stays below 2 GiB", fn, px);
    return CT_OK;
}

// a 16-channel NHWC view: 16-byte aligned, pitch a multiple of 4 and at least 16
int check_map(const char *fn, const char *name, int s, const void *ptr, int ld)
{
    if (ld < 16) CT_FAIL_ARG("%s: channel pitch of %s[%d] (%d) below the channel count 16", fn, name, s, ld);
    if (ld % 4 || misaligned(ptr)) CT_FAIL_ARG("%s: %s[%d] must be 16-byte aligned with a pitch that is a multiple of 4", fn, name, s);
    return CT_OK;
}

int check_plain(const char *fn, const char *name, int s, const void *ptr)
{
    if (!ptr) CT_FAIL_ARG("%s: null pointer (%s[%d])", fn, name, s);
    if (misaligned(ptr, 3)) CT_FAIL_ARG("%s: %s[%d] must be 4-byte aligned", fn, name, s);
    return CT_OK;
}

void tile_plan(StemTrainArgs *a, int N, int H, int W)
{
    a->N = N; a->H = H; a->W = W;
    a->tilesX = ct_cdiv(W, TW);
    a->tilesY = ct_cdiv(H, TH);
    a->tiles = N * a->tilesX * a->tilesY;                       // (< 2^31 / (64 * 1): the view limit)
    a->slabs = a->tiles < GW_SLAB_CAP ? a->tiles : GW_SLAB_CAP;
}

int max3(const int *v, const void *const *used)
{
    int m = 0;
    for (int s = 0; s < 3; ++s)
        if (used[s] && v[s] > m) m = v[s];
    return m;
}

// validation of ct_stem_conv_backward without the workspace; fills the launch arguments
int make_bwd_plan(const char *fn, const ct_stem_conv_desc *d, StemTrainArgs *a, int *ngw, int *ngin, size_t *ws_floats)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    const void *used[3] = {d->gz[0], d->gz[1], d->gz[2]};
    CT_TRY(check_shape(fn, d->N, d->H, d->W, max3(d->ldgz, used)));
    tile_plan(a, d->N, d->H, d->W);
    *ngw = *ngin = 0;
    *ws_floats = 0;
    for (int s = 0; s < 3; ++s) {
        a->in[s] = d->in[s]; a->w[s] = d->w[s]; a->gz[s] = d->gz[s]; a->ldgz[s] = d->ldgz[s];
        a->gw[s] = d->gw[s]; a->gin[s] = d->gin[s]; a->z[s] = nullptr; a->ldz[s] = 0; a->wsoff[s] = 0;
        if (!d->gw[s] && !d->gin[s]) continue;
        if (!d->gz[s]) CT_FAIL_ARG("%s: an output of stem %d asked for without gz[%d]", fn, s, s);
        CT_TRY(check_map(fn, "gz", s, d->gz[s], d->ldgz[s]));
        if (d->gw[s]) {
            CT_TRY(check_plain(fn, "in", s, d->in[s]));
            CT_TRY(check_plain(fn, "gw", s, d->gw[s]));
            a->wsoff[s] = *ws_floats;
            *ws_floats += (size_t)a->slabs * 16 * ((cin_of(s) * 49 + 15) / 16 * 16);
            ++*ngw;
        }
        if (d->gin[s]) {
            CT_TRY(check_plain(fn, "w", s, d->w[s]));
            CT_TRY(check_plain(fn, "gin", s, d->gin[s]));
            ++*ngin;
        }
    }
    if (!*ngw && !*ngin) CT_FAIL_ARG("%s: no output asked for (gw / gin)", fn);
    return CT_OK;
}

}  // namespace

extern "C" int ct_stem_conv_forward(const ct_stem_conv_desc *d, void *stream)
{
    const char *fn = "ct_stem_conv_forward";
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (!d->in[0]) CT_FAIL_ARG("%s: null pointer (in[0]): the image stem is part of every call", fn);
    const void *used[3] = {d->in[0], d->in[1], d->in[2]};
    CT_TRY(check_shape(fn, d->N, d->H, d->W, max3(d->ldz, used)));
    StemTrainArgs a;
    tile_plan(&a, d->N, d->H, d->W);
    a.nact = 0;
    a.ws = nullptr;
    for (int s = 0; s < 3; ++s) {
        a.in[s] = d->in[s]; a.w[s] = d->w[s]; a.z[s] = d->z[s]; a.ldz[s] = d->ldz[s];
        a.gz[s] = nullptr; a.ldgz[s] = 0; a.gw[s] = a.gin[s] = nullptr; a.wsoff[s] = 0; a.act[s] = 0;
    }
    for (int s = 0; s < 3; ++s) {
        if (!d->in[s]) continue;
        CT_TRY(check_plain(fn, "in", s, d->in[s]));
        CT_TRY(check_plain(fn, "w", s, d->w[s]));
        if (!d->z[s]) CT_FAIL_ARG("%s: null pointer (z[%d])", fn, s);
        CT_TRY(check_map(fn, "z", s, d->z[s], d->ldz[s]));
        a.act[a.nact++] = s;
    }
    hipLaunchKernelGGL(stem_conv_fwd_kernel, dim3((unsigned)a.tiles), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

extern "C" int ct_stem_bn_relu_sum(const ct_stem_sum_desc *d, void *stream)
{
    const char *fn = "ct_stem_bn_relu_sum";
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (!d->z[0]) CT_FAIL_ARG("%s: null pointer (z[0]): the image stem is part of every call", fn);
    const void *used[3] = {d->z[0], d->z[1], d->z[2]};
    int m = max3(d->ldz, used);
    if (d->ldy > m) m = d->ldy;
    CT_TRY(check_shape(fn, d->N, d->H, d->W, m));
    if (!d->y) CT_FAIL_ARG("%s: null pointer (y)", fn);
    CT_TRY(check_map(fn, "y", 0, d->y, d->ldy));
    StemSumArgs a;
    for (int s = 0; s < 3; ++s) {
        a.z[s] = d->z[s]; a.ldz[s] = d->ldz[s];
        a.mean[s] = d->mean[s]; a.invstd[s] = d->invstd[s]; a.gamma[s] = d->gamma[s]; a.beta[s] = d->beta[s];
        if (!d->z[s]) continue;
        CT_TRY(check_map(fn, "z", s, d->z[s], d->ldz[s]));
        const void *vec[4] = {d->mean[s], d->invstd[s], d->gamma[s], d->beta[s]};
        for (int i = 0; i < 4; ++i) {
            if (!vec[i]) CT_FAIL_ARG("%s: null pointer (mean / invstd / gamma / beta of stem %d)", fn, s);
            if (misaligned(vec[i])) CT_FAIL_ARG("%s: mean / invstd / gamma / beta of stem %d must be 16-byte aligned", fn, s);
        }
    }
    a.y = d->y; a.ldy = d->ldy; a.P = d->N * d->H * d->W;
    hipLaunchKernelGGL(stem_sum_kernel, dim3(ew_grid(a.P * 4)), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

extern "C" size_t ct_stem_conv_backward_workspace_bytes(const ct_stem_conv_desc *d)
{
    StemTrainArgs a;
    int ngw, ngin;
    size_t wsf;
    if (make_bwd_plan("ct_stem_conv_backward_workspace_bytes", d, &a, &ngw, &ngin, &wsf) != CT_OK) return 0;
    return wsf * sizeof(float);
}

extern "C" int ct_stem_conv_backward(const ct_stem_conv_desc *d, void *stream)
{
    const char *fn = "ct_stem_conv_backward";
    StemTrainArgs a;
    int ngw, ngin;
    size_t wsf;
    CT_TRY(make_bwd_plan(fn, d, &a, &ngw, &ngin, &wsf));
    if (ngw) CT_TRY(check_workspace(fn, "ct_stem_conv_backward_workspace_bytes", d->workspace, d->workspace_bytes, wsf * sizeof(float)));
    a.ws = d->workspace;
    hipStream_t st = (hipStream_t)stream;
    if (ngw) {
        a.nact = 0;
        for (int s = 0; s < 3; ++s)
            if (d->gw[s]) a.act[a.nact++] = s;
        hipLaunchKernelGGL(stem_gw_kernel, dim3((unsigned)a.slabs, (unsigned)a.nact), dim3(256), 0, st, a);
        CT_CHECK_LAUNCH("ct_stem_conv_backward (gw)");
        hipLaunchKernelGGL(stem_gw_reduce_kernel, dim3((unsigned)ct_cdiv(16 * 147, 256), (unsigned)a.nact), dim3(256), 0, st, a);
        CT_CHECK_LAUNCH("ct_stem_conv_backward (reduce)");
    }
    if (ngin) {
        a.nact = 0;
        for (int s = 0; s < 3; ++s)
            if (d->gin[s]) a.act[a.nact++] = s;
        const long blocks = (long)d->N * ct_cdiv(d->H, GT) * ct_cdiv(d->W, GT);
        hipLaunchKernelGGL(stem_gin_kernel, dim3((unsigned)blocks, (unsigned)a.nact), dim3(256), 0, st, a);
        CT_CHECK_LAUNCH("ct_stem_conv_backward (gin)");
    }
    return CT_OK;
}
