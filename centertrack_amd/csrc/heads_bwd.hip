// Backward of the heads (base_model.py:24-65: per head conv3x3 64 -> hc + bias, ReLU, conv1x1 hc -> c + bias) for gfx950, fp32:
// ct_conv2d_backward_weight and ct_heads_tail_backward.  Specification: torch.autograd of that nn.Sequential.  DESIGN.md
// section 11.  The input gradient of the first layer is a plain ct_conv2d of the hidden gradient with the transposed, flipped
// weight and has no kernel here.
//
//   * conv_bwd_weight_kernel<STRIDE>: gw[co, ci, tap] = sum_p gy[p, co] * x[STRIDE * p + tap, ci] (pad ks / 2, zero outside the
//     image), K = all pixels of gy, on v_mfma_f32_16x16x4_f32.  <1> is ct_conv2d_backward_weight; <2> (3x3, no bias) is the weight
//     half of ct_conv2d_s2_backward (backbone_bwd.hip), launched through ct_conv_s2_weight_launch (ct_train.h).
//     The plan is dcn_bwd_weight_kernel's (dcn_bwd.hip): a workgroup
//     owns one (tap, 32 input channels, up to 64 couts) block of the output and one K slab of pixels; its four waves split the
//     slab, each stepping 4 pixels per MFMA (A = gy^T, B = the shifted x, both straight from global through buffer descriptors:
//     a tap outside the image carries the sentinel offset and reads 0), are summed through LDS in wave order, and the workgroup
//     stores its partial block into slab `blockIdx.y` of the workspace.  Units of tap 0 / channel block 0 also accumulate the
//     bias gradient (B = 1).  slab_reduce_kernel sums the slabs in slab order into gw (OIHW) and gb.
//   * heads_tail_gmid_kernel: gmid[p, i*hc + k] = mid[p, i*hc + k] > 0 ? sum_c w2[i][c][k] * gout[i][c][p] : 0.  One workgroup =
//     32 pixels of one head, thread = hidden channel; the logit gradients (NCHW) of 16 channels at a time are staged in LDS
//     and read back as broadcasts; the sum over c runs in channel order.
//   * heads_tail_weight_kernel: gw2[i][c][k] = sum_p gout[i][c][p] * mid[p, i*hc + k], gb2[i][c] = sum_p gout[i][c][p].  One
//     workgroup = (pixel slab, head, 16 logit channels, 256 hidden channels); thread = hidden channel, 16 accumulators, the
//     pixels of the slab in ascending order; the partials go to slab `blockIdx.x` of the workspace and heads_tail_reduce_kernel
//     adds them in slab order.
// No atomics anywhere: every result is bitwise equal from run to run.
#include "ct_train.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// the weight gradient of a convolution

struct CwArgs {
    const float *x, *gy;
    float *ws;
    int N, H, W, Cin, Cout, ldx, ldgy;      // H, W: the grid of gy
    int NT, cgroups;
    int stepsPerWave;   // 4-pixel steps per wave
    size_t slabStride;  // floats per slab: Cout*Cin*ks*ks (+ Cout with a bias tail)
    int Hi, Wi;         // stride 2: the grid of x (2H, 2W)
    int ks, withBias;   // stride 1
};

// STRIDE 1: ks 1 or 3, pad ks / 2, any Cout, optional bias; 12 accumulator tiles of a wave: 2 channel tiles x 4 cout tiles + 4
// bias tiles.  STRIDE 2: ks 3, pad 1, Cout % 16 == 0, no bias: 8 tiles.
template <int STRIDE>
__global__ __launch_bounds__(256) void conv_bwd_weight_kernel(CwArgs a)
{
    constexpr int W_TILES = STRIDE == 1 ? 12 : 8;
    __shared__ float red[3][W_TILES][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = a.H * a.W;
    const int total = a.N * HW;
    const int taps = STRIDE == 1 ? a.ks * a.ks : 9;
    int unit = blockIdx.x;
    const int k = unit % taps;
    unit /= taps;
    const int cig = unit % a.cgroups, cog = unit / a.cgroups;
    const int dy = (STRIDE == 2 || a.ks == 3) ? k / 3 - 1 : 0, dx = (STRIDE == 2 || a.ks == 3) ? k % 3 - 1 : 0;
    const bool withBias = STRIDE == 1 && a.withBias && k == 0 && cig == 0;
    const int nco = min(4, a.NT - cog * 4);
    const __amdgpu_buffer_rsrc_t xrs = view_rsrc(a.x, STRIDE == 1 ? (size_t)total : (size_t)a.N * a.Hi * a.Wi, a.ldx, a.Cin);
    const __amdgpu_buffer_rsrc_t gyrs = view_rsrc(a.gy, (size_t)total, a.ldgy, a.Cout);
    const int c0 = cig * 32 + (lane & 15);
    const bool has1 = c0 + 16 < a.Cin;                       // (Cin % 32 == 16: the last group is one tile wide)
    f32x4 acc[W_TILES];
#pragma unroll
    for (int i = 0; i < W_TILES; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (total + 3) >> 2;
    const int s0 = min(nsteps, ((int)blockIdx.y * 4 + wave) * a.stepsPerWave);
    const int s1 = min(nsteps, s0 + a.stepsPerWave);
    // four steps (16 pixels of gy) per round: the loads of all four are in flight together
    for (int st = s0; st < s1; st += 4) {
        float col[4][2], g[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int gp = (st + u) * 4 + (lane >> 4);
            const bool live = st + u < s1 && gp < total;
            const int n = gp / HW, pix = gp - n * HW, h = pix / a.W, w = pix - h * a.W;
            bool inside;
            int xo;
            if constexpr (STRIDE == 1) {
                inside = live && h + dy >= 0 && h + dy < a.H && w + dx >= 0 && w + dx < a.W;
                xo = (gp + dy * a.W + dx) * a.ldx;           // the shifted pixel of the same image
            } else {
                const int iy = 2 * h + dy, ix = 2 * w + dx;
                inside = live && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
                xo = ((n * a.Hi + iy) * a.Wi + ix) * a.ldx;
            }
            col[u][0] = bload(xrs, inside ? (xo + c0) * 4 : SENTINEL);
            col[u][1] = bload(xrs, (inside && has1) ? (xo + c0 + 16) * 4 : SENTINEL);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int co = (cog * 4 + ct) * 16 + (lane & 15);
                g[u][ct] = bload(gyrs, (live && ct < nco && (STRIDE == 2 || co < a.Cout)) ? (gp * a.ldgy + co) * 4 : SENTINEL);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (ct < nco) {                                  // (uniform)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][0], acc[ct], 0, 0, 0);
                    acc[4 + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][1], acc[4 + ct], 0, 0, 0);
                    if constexpr (STRIDE == 1) {
                        if (withBias) acc[8 + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], 1.0f, acc[8 + ct], 0, 0, 0);
                    }
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
            if (STRIDE == 1 && co >= a.Cout) continue;
            slab[((size_t)co * a.Cin + c0) * taps + k] = acc[ct][e];
            if (has1) slab[((size_t)co * a.Cin + c0 + 16) * taps + k] = acc[4 + ct][e];
            if constexpr (STRIDE == 1) {
                if (withBias && (lane & 15) == 0) slab[(size_t)a.Cout * a.Cin * taps + co] = acc[8 + ct][e];
            }
        }
    }
}

// ws [slabs][slabStride] -> gw (the first nw floats of a slab) and gb (the rest, where asked for), slabs added in slab order
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *ws, int slabs, size_t slabStride, size_t nw, float *gw,
                                                          float *gb)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slabStride) return;
    if (i >= nw && !gb) return;
    float s = 0.0f;
    for (int j = 0; j < slabs; ++j) s += ws[(size_t)j * slabStride + i];
    if (i < nw) gw[i] = s;
    else gb[i - nw] = s;
}

int launch_cw(const char *fn, int stride, CwArgs a, const CwPlan &p, float *gw, float *gb, hipStream_t s)
{
    a.NT = p.NT; a.cgroups = p.cgroups; a.stepsPerWave = p.stepsPerWave; a.slabStride = p.slabStride;
    const dim3 grid((unsigned)p.units, (unsigned)p.slabs);
    if (stride == 1) hipLaunchKernelGGL(conv_bwd_weight_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_bwd_weight_kernel<2>, grid, dim3(256), 0, s, a);
    CT_CHECK_LAUNCH(fn);
    const size_t nw = (size_t)a.Cout * a.Cin * a.ks * a.ks;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((p.slabStride + 255) / 256)), dim3(256), 0, s, a.ws, p.slabs, p.slabStride,
                       nw, gw, gb);
    CT_CHECK_LAUNCH(fn);
    return CT_OK;
}

int make_cw_plan(const ct_conv_bwd_weight_desc *d, CwPlan *p, bool needBuffers)
{
    const char *fn = "ct_conv2d_backward_weight";
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->ks != 1 && d->ks != 3) CT_FAIL_ARG("%s: ks=%d unsupported (1 or 3)", fn, d->ks);
    if (d->stride != 1) CT_FAIL_ARG("%s: stride=%d unsupported (1)", fn, d->stride);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->Cin % 16 || d->Cin <= 0) CT_FAIL_ARG("%s: Cin=%d must be a positive multiple of 16", fn, d->Cin);
    if (needBuffers && (!d->x || !d->gy || !d->gw)) CT_FAIL_ARG("%s: null pointer (x / gy / gw)", fn);
    if (d->ldx < d->Cin || d->ldgy < d->Cout) CT_FAIL_ARG("%s: channel pitch below the channel count (x / gy)", fn);
    const double px = (double)d->N * d->H * d->W;
    if (px * (d->ldx > d->ldgy ? d->ldx : d->ldgy) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernel addresses every view through one buffer descriptor", fn, px);
    return ct_conv_weight_plan(fn, (int)px, d->Cin, d->Cout, d->ks * d->ks, true, p);
}

// ---------------------------------------------------------------------------------------------------------------------
// the 1x1 layers of the heads and the ReLU in front of them

constexpr int CC = 16;           // logit channels per pass
constexpr int TP = 32;           // pixels per workgroup of the hidden-gradient kernel
constexpr int TW = 64;           // pixels per LDS tile of the weight-gradient kernel

struct TailHead {
    const float *gout, *w2;
    float *gw2, *gb2;
    int c;
    int off;                     // first float of the head in a slab: [c * hc weights][c biases]
};

struct TailArgs {
    TailHead h[CT_LOSS_MAX_HEADS];
    const float *mid;
    float *gmid, *ws;
    int nheads, hc, ldmid, ldgmid, HW, total;
    int pixPerSlab, slabs, kblocks;
    size_t slabStride;
};

// g[p][cc] = gout[c0 + cc][t0 + p] for the `npx` pixels from t0 below pend, 0 elsewhere (NCHW source: coalesced along the pixels)
template <int NP>
__device__ __forceinline__ void stage_gout(float (*g)[CC], const TailHead &hd, int c0, int t0, int pend, int HW)
{
    for (int i = threadIdx.x; i < NP * CC; i += 256) {
        const int p = i % NP, cc = i / NP;
        const int gp = t0 + p, c = c0 + cc;
        float v = 0.0f;
        if (gp < pend && c < hd.c) {
            const int n = gp / HW;
            v = hd.gout[((size_t)n * hd.c + c) * HW + (gp - n * HW)];
        }
        g[p][cc] = v;
    }
}

__global__ __launch_bounds__(256) void heads_tail_gmid_kernel(TailArgs a)
{
    __shared__ __attribute__((aligned(16))) float g[TP][CC];
    const int head = blockIdx.y;
    const TailHead &hd = a.h[head];
    const int k = blockIdx.z * 256 + threadIdx.x;
    const bool kok = k < a.hc;
    const int p0 = blockIdx.x * TP;
    float s[TP];
#pragma unroll
    for (int p = 0; p < TP; ++p) s[p] = 0.0f;
    for (int cb = 0; cb < hd.c; cb += CC) {
        float w[CC];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) w[cc] = (kok && cb + cc < hd.c) ? hd.w2[(size_t)(cb + cc) * a.hc + k] : 0.0f;
        __syncthreads();
        stage_gout<TP>(g, hd, cb, p0, a.total, a.HW);
        __syncthreads();
#pragma unroll
        for (int p = 0; p < TP; ++p) {
#pragma unroll
            for (int q = 0; q < CC / 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(&g[p][q * 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[p] = fmaf(w[q * 4 + j], v[j], s[p]);
            }
        }
    }
    if (!kok) return;
    const size_t ch = (size_t)head * a.hc + k;
#pragma unroll
    for (int p = 0; p < TP; ++p) {
        const int gp = p0 + p;
        if (gp < a.total) {
            const float m = a.mid[(size_t)gp * a.ldmid + ch];
            a.gmid[(size_t)gp * a.ldgmid + ch] = !(m <= 0.0f) ? s[p] : 0.0f;      // torch's ReLU: gradient 0 at exactly 0, passed where mid is NaN
        }
    }
}

__global__ __launch_bounds__(256) void heads_tail_weight_kernel(TailArgs a)
{
    __shared__ __attribute__((aligned(16))) float g[TW][CC];
    const int head = blockIdx.y;
    const TailHead &hd = a.h[head];
    if (!hd.gw2 && !hd.gb2) return;                            // (uniform: a head nobody asked for)
    const int kb = blockIdx.z % a.kblocks, cb = (blockIdx.z / a.kblocks) * CC;
    if (cb >= hd.c) return;                                    // (uniform: the grid is sized for the widest head)
    const int k = kb * 256 + threadIdx.x;
    const bool kok = k < a.hc;
    const int pa = blockIdx.x * a.pixPerSlab;
    const int pb = min(a.total, pa + a.pixPerSlab);
    float acc[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
    float bsum = 0.0f;
    const float *mp = a.mid + (size_t)head * a.hc + (kok ? k : 0);
    for (int t0 = pa; t0 < pb; t0 += TW) {
        __syncthreads();
        stage_gout<TW>(g, hd, cb, t0, pb, a.HW);
        __syncthreads();
        if (kb == 0 && threadIdx.x < CC)
            for (int p = 0; p < TW; ++p) bsum += g[p][threadIdx.x];
        // eight pixels per round, their hidden values loaded first; a pixel past the slab's end re-reads the last one against
        // a zero row of g
        for (int p = 0; p < TW; p += 8) {
            float m[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) m[u] = mp[(size_t)min(t0 + p + u, pb - 1) * a.ldmid];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
#pragma unroll
                for (int q = 0; q < CC / 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(&g[p + u][q * 4]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[q * 4 + j] = fmaf(v[j], m[u], acc[q * 4 + j]);
                }
            }
        }
    }
    float *slab = a.ws + (size_t)blockIdx.x * a.slabStride + hd.off;
    if (kok) {
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
            if (cb + cc < hd.c) slab[(size_t)(cb + cc) * a.hc + k] = acc[cc];
    }
    if (kb == 0 && threadIdx.x < CC && cb + (int)threadIdx.x < hd.c) slab[(size_t)hd.c * a.hc + cb + threadIdx.x] = bsum;
}

__global__ __launch_bounds__(256) void heads_tail_reduce_kernel(TailArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.slabStride) return;
    int h = 0;
    while (h + 1 < a.nheads && i >= (size_t)a.h[h + 1].off) ++h;
    float *gw2 = a.h[h].gw2, *gb2 = a.h[h].gb2;
    const size_t j = i - a.h[h].off, nw = (size_t)a.h[h].c * a.hc;
    float *dst = j < nw ? (gw2 ? gw2 + j : nullptr) : (gb2 ? gb2 + (j - nw) : nullptr);
    if (!dst) return;
    float s = 0.0f;
    for (int t = 0; t < a.slabs; ++t) s += a.ws[(size_t)t * a.slabStride + i];
    *dst = s;
}

struct TailPlan {
    int kblocks, zdim, slabs, pixPerSlab;
    size_t slabStride;
};

int make_tail_plan(const ct_heads_tail_bwd_desc *d, TailPlan *p, bool needBuffers)
{
    if (!d) CT_FAIL_ARG("ct_heads_tail_backward: null descriptor");
    if (d->flags & ~(CT_HEADS_BWD_HIDDEN | CT_HEADS_BWD_WEIGHT) || !d->flags)
        CT_FAIL_ARG("ct_heads_tail_backward: flags=%d (a combination of CT_HEADS_BWD_HIDDEN, _WEIGHT)", d->flags);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->hc <= 0) CT_FAIL_ARG("ct_heads_tail_backward: bad shape");
    if ((double)d->N * d->H * d->W > 2147483647.0) CT_FAIL_ARG("ct_heads_tail_backward: N*H*W above 2^31 - 1 pixels");
    if (d->nheads < 1 || d->nheads > CT_LOSS_MAX_HEADS || !d->heads)
        CT_FAIL_ARG("ct_heads_tail_backward: nheads=%d (1 .. %d, with a head array)", d->nheads, CT_LOSS_MAX_HEADS);
    const bool hidden = d->flags & CT_HEADS_BWD_HIDDEN, weight = d->flags & CT_HEADS_BWD_WEIGHT;
    const double chans = (double)d->nheads * d->hc;
    if (d->ldmid < chans) CT_FAIL_ARG("ct_heads_tail_backward: ldmid=%d below nheads*hc", d->ldmid);
    if (hidden && d->ldgmid < chans) CT_FAIL_ARG("ct_heads_tail_backward: ldgmid=%d below nheads*hc", d->ldgmid);
    if (needBuffers && !d->mid) CT_FAIL_ARG("ct_heads_tail_backward: null pointer (mid)");
    if (needBuffers && hidden && !d->gmid) CT_FAIL_ARG("ct_heads_tail_backward: null pointer (gmid)");
    double stride = 0.0;
    int allWgs = 0, maxChunks = 0, asked = 0;
    p->kblocks = ct_cdiv(d->hc, 256);
    for (int i = 0; i < d->nheads; ++i) {
        const ct_heads_tail_head &h = d->heads[i];
        if (h.c <= 0) CT_FAIL_ARG("ct_heads_tail_backward: head %d has c=%d", i, h.c);
        if (needBuffers && !h.gout) CT_FAIL_ARG("ct_heads_tail_backward: head %d: null pointer (gout)", i);
        if (needBuffers && hidden && !h.w2) CT_FAIL_ARG("ct_heads_tail_backward: head %d: null pointer (w2)", i);
        stride += (double)h.c * (d->hc + 1);
        const int chunks = ct_cdiv(h.c, CC);
        if (chunks > maxChunks) maxChunks = chunks;
        allWgs += chunks * p->kblocks;
        if (h.gw2 || h.gb2) ++asked;
    }
    if (stride > 2147483647.0) CT_FAIL_ARG("ct_heads_tail_backward: more than 2^31 - 1 head parameters");
    if (needBuffers && weight && !asked) CT_FAIL_ARG("ct_heads_tail_backward: CT_HEADS_BWD_WEIGHT without a gw2 / gb2 buffer");
    if ((double)maxChunks * p->kblocks > 65535.0) CT_FAIL_ARG("ct_heads_tail_backward: grid too large");
    p->zdim = maxChunks * p->kblocks;
    p->slabStride = (size_t)stride;
    // slabs and workspace are sized for every head, asked for or not: the query and the call agree whatever buffers are given
    const int total = d->N * d->H * d->W;
    int slabs = ct_cdiv(2048, allWgs);
    const int maxSlabs = ct_cdiv(total, TW);
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->pixPerSlab = ct_cdiv(ct_cdiv(total, slabs), TW) * TW;
    p->slabs = ct_cdiv(total, p->pixPerSlab);
    return CT_OK;
}

}  // namespace

extern "C" size_t ct_conv2d_backward_weight_workspace_bytes(const ct_conv_bwd_weight_desc *d)
{
    CwPlan p;
    if (!d || make_cw_plan(d, &p, false) != CT_OK) return 0;
    return (size_t)p.slabs * p.slabStride * sizeof(float);
}

extern "C" int ct_conv2d_backward_weight(const ct_conv_bwd_weight_desc *d, void *stream)
{
    CwPlan p;
    const int rc = make_cw_plan(d, &p, true);
    if (rc != CT_OK) return rc;
    const size_t need = (size_t)p.slabs * p.slabStride * sizeof(float);
    if (!d->workspace || d->workspace_bytes < need) {
        ct_set_error("ct_conv2d_backward_weight: workspace of %zu bytes needed (ct_conv2d_backward_weight_workspace_bytes), got %zu",
                     need, d->workspace ? d->workspace_bytes : (size_t)0);
        return CT_ERR_WORKSPACE;
    }
    CwArgs a;
    a.x = d->x; a.gy = d->gy; a.ws = d->workspace;
    a.N = d->N; a.H = a.Hi = d->H; a.W = a.Wi = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.ldx = d->ldx; a.ldgy = d->ldgy;
    a.ks = d->ks; a.withBias = d->gb != nullptr;
    return launch_cw("ct_conv2d_backward_weight", 1, a, p, d->gw, d->gb, (hipStream_t)stream);
}

int ct_conv_weight_plan(const char *fn, int pixels, int Cin, int Cout, int taps, bool biasTail, CwPlan *p)
{
    p->NT = ct_cdiv(Cout, 16);
    p->cgroups = ct_cdiv(Cin, 32);
    const double units = (double)taps * p->cgroups * ct_cdiv(p->NT, 4);
    if (units > 2147483647.0) CT_FAIL_ARG("%s: grid too large", fn);
    p->units = (int)units;
    const int nsteps = ct_cdiv(pixels, 4);
    int slabs = ct_cdiv(1024, p->units);
    const int maxSlabs = ct_cdiv(nsteps, 32);           // at least 8 steps for each of the four waves
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->slabs = slabs;
    p->stepsPerWave = ct_cdiv(nsteps, slabs * 4);
    p->slabStride = (size_t)Cout * Cin * taps + (biasTail ? Cout : 0);
    return CT_OK;
}

int ct_conv_s2_weight_launch(const ct_conv_s2_bwd_desc *d, const CwPlan &p, void *stream)
{
    CwArgs a;
    a.x = d->x; a.gy = d->gy; a.ws = d->workspace;
    a.N = d->N; a.H = d->H / 2; a.W = d->W / 2; a.Hi = d->H; a.Wi = d->W;
    a.Cin = d->Cin; a.Cout = d->Cout; a.ldx = d->ldx; a.ldgy = d->ldgy;
    a.ks = 3; a.withBias = 0;
    return launch_cw("ct_conv2d_s2_backward (weight)", 2, a, p, d->gw, nullptr, (hipStream_t)stream);
}

extern "C" size_t ct_heads_tail_backward_workspace_bytes(const ct_heads_tail_bwd_desc *d)
{
    TailPlan p;
    if (!d || !(d->flags & CT_HEADS_BWD_WEIGHT) || make_tail_plan(d, &p, false) != CT_OK) return 0;
    return (size_t)p.slabs * p.slabStride * sizeof(float);
}

extern "C" int ct_heads_tail_backward(const ct_heads_tail_bwd_desc *d, void *stream)
{
    TailPlan p;
    const int rc = make_tail_plan(d, &p, true);
    if (rc != CT_OK) return rc;
    const bool hidden = d->flags & CT_HEADS_BWD_HIDDEN, weight = d->flags & CT_HEADS_BWD_WEIGHT;
    if (weight) {
        const size_t need = (size_t)p.slabs * p.slabStride * sizeof(float);
        if (!d->workspace || d->workspace_bytes < need) {
            ct_set_error("ct_heads_tail_backward: workspace of %zu bytes needed (ct_heads_tail_backward_workspace_bytes), got %zu",
                         need, d->workspace ? d->workspace_bytes : (size_t)0);
            return CT_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    TailArgs a;
    int off = 0;
    for (int i = 0; i < CT_LOSS_MAX_HEADS; ++i) {
        TailHead &h = a.h[i];
        if (i < d->nheads) {
            const ct_heads_tail_head &src = d->heads[i];
            h.gout = src.gout; h.w2 = src.w2; h.c = src.c; h.off = off;
            h.gw2 = weight ? src.gw2 : nullptr;
            h.gb2 = weight ? src.gb2 : nullptr;
            off += src.c * (d->hc + 1);
        } else {
            h.gout = h.w2 = nullptr; h.gw2 = h.gb2 = nullptr; h.c = 0; h.off = off;
        }
    }
    a.mid = d->mid; a.gmid = d->gmid; a.ws = d->workspace;
    a.nheads = d->nheads; a.hc = d->hc; a.ldmid = d->ldmid; a.ldgmid = d->ldgmid; a.HW = d->H * d->W; a.total = d->N * d->H * d->W;
    a.pixPerSlab = p.pixPerSlab; a.slabs = p.slabs; a.kblocks = p.kblocks; a.slabStride = p.slabStride;
    if (hidden) {
        hipLaunchKernelGGL(heads_tail_gmid_kernel, dim3((unsigned)ct_cdiv(a.total, TP), (unsigned)d->nheads, (unsigned)p.kblocks),
                           dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_heads_tail_backward (hidden)");
    }
    if (weight) {
        hipLaunchKernelGGL(heads_tail_weight_kernel, dim3((unsigned)p.slabs, (unsigned)d->nheads, (unsigned)p.zdim), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_heads_tail_backward (weight)");
        hipLaunchKernelGGL(heads_tail_reduce_kernel, dim3((unsigned)((p.slabStride + 255) / 256)), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_heads_tail_backward (reduce)");
    }
    return CT_OK;
}
