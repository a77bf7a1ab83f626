// The trainable DLA-34 backbone (BasicBlock / Root / Tree / DLA, dla.py:38-66,154-316) for gfx950, fp32, NHWC views with a
// channel pitch: the backward of the 3x3 stride-2 convolution and of the 2x2 max-pool.  Specification: torch.autograd of
// F.conv2d(stride 2, pad 1) and of F.max_pool2d(2, 2).  Its BatchNorm (+ residual) (+ ReLU) is bn_train.hip.  DESIGN.md
// section 13.
//
//   * conv_s2_gx_kernel: gx[n,iy,ix,ci] = sum gy[n,oy,ox,co] * w[co,ci,ky,kx] over iy + 1 - ky = 2 oy, ix + 1 - kx = 2 ox, on
//     v_mfma_f32_16x16x4_f32 with no zero-inserted map and no scatter.  Cell (cy,cx) of the output grid owns the 2x2 input
//     pixels (2cy+a, 2cx+b); along one axis a = 0 meets tap 1 at cy, a = 1 meets tap 2 at cy and tap 0 at cy + 1: the nine
//     taps appear once per cell.  A workgroup owns 4 rows x 16 columns of cells of one image and 32 input channels; it stages
//     the gy tile plus one halo row and column (zero outside the map) 64 couts at a time in LDS, wave r runs the nine tap
//     GEMMs of cell row r (A = gy from LDS, B = the weight in ct_pack_conv_weight_s2t's fragment order straight from global,
//     K = Cout in ascending order) into 4 parities x 2 channel tiles and stores 2x2 pixels per cell.
//   * gw[co,ci,ky,kx] = sum_{n,oy,ox} gy[n,oy,ox,co] * x[n,2oy-1+ky,2ox-1+kx,ci] is conv_bwd_weight_kernel<2> of heads_bwd.hip
//     (ct_conv_s2_weight_launch, ct_train.h): slabs of output pixels to the workspace, added in slab order.
//   * maxpool_bwd_kernel: thread = one 2x2 window and channel quad; the window's gradient goes to its first maximum in
//     row-major order (torch's rule: a later value wins only if it is greater or NaN), the other three get 0, plus `add`.
// No atomics anywhere; slab counts depend on the shapes only: every result is bitwise equal from run to run.
// Every view is addressed with 32-bit offsets or one buffer descriptor, so a view stays below 2 GiB (checked on the host).
#include "ct_train.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// the 3x3 stride-2 convolution

constexpr int GX_TW = 16;        // cells of a workgroup along x: the M of one MFMA
constexpr int GX_TH = 4;         // cell rows of a workgroup: one per wave
constexpr int GX_KC = 64;        // couts per staged chunk
constexpr int GX_KS = 68;        // LDS pitch of a staged pixel (floats)

struct S2Args {
    const float *gy, *wt;
    float *gx;
    int N, H, W, Cin, Cout, ldgy, ldgx;
    int Ho, Wo, tilesX, tilesY, cgroups;
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

struct S2Plan {
    int Ho, Wo, tilesX, tilesY, cgroups, gxUnits;
    CwPlan w;                    // the weight gradient: K = N*Ho*Wo in slabs of Cout*Cin*9 floats
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
    if (gxUnits > 2147483647.0) CT_FAIL_ARG("%s: grid too large", fn);
    p->gxUnits = (int)gxUnits;
    return ct_conv_weight_plan(fn, d->N * p->Ho * p->Wo, d->Cin, d->Cout, 9, false, &p->w);
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
    return (size_t)p.w.slabs * p.w.slabStride * sizeof(float);
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
        CT_TRY(check_workspace(fn, "ct_conv2d_s2_backward_workspace_bytes", d->workspace, d->workspace_bytes,
                               (size_t)p.w.slabs * p.w.slabStride * sizeof(float)));
        CT_TRY(ct_conv_s2_weight_launch(d, p.w, stream));
    }
    if (d->gx) {
        S2Args a;
        a.gy = d->gy; a.wt = d->w_s2t; a.gx = d->gx;
        a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.ldgy = d->ldgy; a.ldgx = d->ldgx;
        a.Ho = p.Ho; a.Wo = p.Wo; a.tilesX = p.tilesX; a.tilesY = p.tilesY; a.cgroups = p.cgroups;
        hipLaunchKernelGGL(conv_s2_gx_kernel, dim3((unsigned)p.gxUnits), dim3(256), 0, (hipStream_t)stream, a);
        CT_CHECK_LAUNCH("ct_conv2d_s2_backward (input)");
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
