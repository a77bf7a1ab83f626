// The trainable neck (DeformConv / IDAUp / DLAUp, dla.py:506-574) for gfx950, fp32, NHWC views with a channel pitch:
// the backward of ct_upsample_add and the sigmoid derivative of the DCN mask channels.  Specification: torch.autograd of
// F.conv_transpose2d(groups = C).  Its BatchNorm + ReLU is bn_train.hip.  DESIGN.md section 12.
//
//   * up_gx_kernel: gx[n,iy,ix,c] = sum_{ky,kx < 2f} gy[n, iy*f - f/2 + ky, ix*f - f/2 + kx, c] * w[ky,kx,c], a gather in
//     tap order.  up_gw_kernel<F>: gw[c,ky,kx] = sum_{n,iy,ix} x * gy; a workgroup owns a slab of input pixels and 16
//     channel quads, thread (tap lane t, quad q) keeps F*F/4 taps in registers and walks the slab's pixels in ascending
//     order; up_gw_reduce_kernel adds the slabs in slab order into the module's [C,1,2f,2f] layout.
//   * mask_sigmoid_bwd_kernel: g *= m * (1 - m) on channels 18..26 of the offset/mask gradient.
// No atomics anywhere; slab counts depend on the shapes only: every result is bitwise equal from run to run.
// Every view is addressed with 32-bit element offsets, so a view stays below 2 GiB (checked on the host).
#include "ct_train.h"

namespace {

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
        CT_TRY(check_workspace(fn, "ct_upsample_add_backward_workspace_bytes", d->workspace, d->workspace_bytes,
                               (size_t)p.slabs * 4 * d->f * d->f * d->C * sizeof(float)));
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
