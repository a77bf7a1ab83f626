// Backward of the modulated deformable 3x3 convolution (DCNv2; stride 1, pad 1, dilation 1, one deformable group, fp32)
// for gfx950: ct_dcn_v2_backward.  Specification: torch.autograd of oracle/dcn_v2.py::dcn_v2_conv.  DESIGN.md section 9.
//
// No column buffer in global memory: the [pixels, 9*Cin] matrices `gcol` (gradient of the sampled columns) and `col`
// (the modulated samples) only ever exist as MFMA operands / accumulators in registers.
//
//   * dcn_bwd_data_kernel: one workgroup = 16 consecutive pixels of one image (flattened H*W, so any W works) and 3 * CS waves:
//     wave = (taps 3 tg .. 3 tg + 2, every CS-th 16-channel tile of the input; CS = 1, 2 or 4, more for layers with few pixel
//     tiles).  Per (tap, channel tile):
//       gcol[16 px, 16 ci] = gy[16 px, Cout] . W[Cout, (ci, tap)]     v_mfma_f32_16x16x4_f32, A = the gy tile staged once in
//                                                                     LDS, B = the transposed fragment packing
//                                                                     (ct_pack_dcn_weight_t), one 1 KiB block per 16 couts
//     The accumulator layout (lane: channel ci0 + (lane & 15), pixels 4*(lane >> 4) + e) is used as it stands: the lane
//     gathers the four corners of its 4 (pixel, tap) samples through a buffer descriptor (a corner outside the image carries
//     the sentinel offset and reads 0; the loads are issued ahead of the MFMA chain), adds its share of g_mask / g_dy / g_dx
//     into 12 registers that live across the whole channel loop, and adds gcol * m * (corner weight) into g_x with no-return
//     global_atomic_add_f32: one wave instruction = 4 cells x 16 consecutive channels (4 x 64 B; measured at the chip-wide
//     atomic rate).  Corners with a zero bilinear weight (every sample of a zero-initialised
//     conv_offset_mask has three of them) and invalid corners issue no atomic.  After the channel loop one 16-lane butterfly
//     and a sum over the CS waves through LDS, in split order, finish the three sums: the sum over Cin completes inside the
//     workgroup, g_offset / g_mask are plain stores and bitwise reproducible.  (An LDS-pre-summed scatter was measured slower
//     and is not here: DESIGN.md section 9.)
//   * dcn_bwd_weight_kernel: g_weight[co, ci, k] = sum_p gy[p, co] * m_k(p) * val[p, ci, k], K = all pixels of the batch.
//     A workgroup owns one (tap, 32 input channels, up to 64 couts) block of the output and one K slab of pixels; its four
//     waves split the slab, each stepping 4 pixels per MFMA (A = gy^T straight from global, B = the lane's own re-gathered
//     modulated sample), are summed through LDS in wave order, and the workgroup stores its partial block into slab
//     `blockIdx.y` of the workspace.  Units of tap 0 / channel block 0 also accumulate g_bias (B = 1).
//   * dcn_bwd_reduce_kernel sums the slabs in slab order into g_weight (OIHW) and g_bias.  No float atomics on this side.
#include "ct_train.h"

namespace {

struct BwdArgs {
    const float *x, *om, *gy, *wT;
    float *gx, *gom, *ws;
    int N, H, W, Cin, Cout;
    int ldx, ldom, ldgy, ldgx, ldgom;
    int NT;             // CoutPad / 16
    int tilesPerImg;    // data kernel: 16-pixel tiles per image
    int CS;             // data kernel: channel splits = waves / 3 (1, 2 or 4)
    int slabs;          // weight kernel: K slabs (gridDim.y)
    int stepsPerWave;   // weight kernel: 4-pixel steps per wave
    size_t slabStride;  // floats per slab: Cout*Cin*9 + Cout
};

// One bilinear sample of tap k at pixel (n, h, w): the linear cell index (over the batch) of corner 00 -- corner ab is cell
// base + a * W + b --, one validity bit per corner (bit 2a + b; a cleared bit = contributes 0), the weights and the mask.  ys is formed as the oracle forms it (exact small integer + one fp32 add), so floor picks the same cell.
struct Samp {
    int base, ok;
    float hy, hx, ly, lx, m;
};

__device__ __forceinline__ Samp make_samp(__amdgpu_buffer_rsrc_t omrs, bool live, int gp, int n, int h, int w, int k,
                                          int H, int W, int ldom)
{
    Samp s;
    const int ob = live ? gp * ldom * 4 : SENTINEL;
    const float dy = bload(omrs, ob + 8 * k), dx = bload(omrs, ob + 8 * k + 4);
    s.m = bload(omrs, ob + 4 * (18 + k));
    const float ys = (float)(h - 1 + k / 3) + dy, xs = (float)(w - 1 + k % 3) + dx;
    const bool inside = live && ys > -1.0f && xs > -1.0f && ys < (float)H && xs < (float)W;
    const float fy = floorf(ys), fx = floorf(xs);
    s.ly = inside ? ys - fy : 0.0f;
    s.lx = inside ? xs - fx : 0.0f;
    s.hy = inside ? 1.0f - s.ly : 0.0f;
    s.hx = inside ? 1.0f - s.lx : 0.0f;
    const int y0 = inside ? (int)fy : -2, x0 = inside ? (int)fx : -2;
    const bool y0ok = y0 >= 0 && y0 <= H - 1, y1ok = y0 + 1 >= 0 && y0 + 1 <= H - 1;
    const bool x0ok = x0 >= 0 && x0 <= W - 1, x1ok = x0 + 1 >= 0 && x0 + 1 <= W - 1;
    s.base = (n * H + y0) * W + x0;
    s.ok = (y0ok && x0ok ? 1 : 0) | (y0ok && x1ok ? 2 : 0) | (y1ok && x0ok ? 4 : 0) | (y1ok && x1ok ? 8 : 0);
    return s;
}

// byte offset of channel c4 / 4 of corner `corner` (0..3 = 00, 01, 10, 11) in the x view, or the sentinel
__device__ __forceinline__ int cell_off(const Samp &s, int corner, int W, int ld4, int c4)
{
    return (s.ok >> corner & 1) ? (s.base + (corner >> 1) * W + (corner & 1)) * ld4 + c4 : SENTINEL;
}

template <bool GX, bool GOM>
__global__ __launch_bounds__(768) void dcn_bwd_data_kernel(BwdArgs a)
{
    extern __shared__ float gyt[];                        // [16 pixels][ldg]: the tile's gy, zero past the image / Cout
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tg = wave % 3, split = wave / 3;            // taps 3 tg .. 3 tg + 2, channel tiles split, split + CS, ..
    const int HW = a.H * a.W;
    const int n = blockIdx.x / a.tilesPerImg;
    const int p0 = (blockIdx.x % a.tilesPerImg) * 16;
    const int CP = a.NT * 16, ldg = CP + 4;
    float *red = gyt + 16 * ldg;                          // [CS][9 taps][16 pixels][3]: the channel splits' partial sums
    for (int i = threadIdx.x; i < 16 * CP; i += blockDim.x) {
        const int p = i / CP, c = i - p * CP;
        float v = 0.0f;
        if (p0 + p < HW && c < a.Cout) v = a.gy[((size_t)n * HW + p0 + p) * a.ldgy + c];
        gyt[p * ldg + c] = v;
    }
    __syncthreads();
    const size_t pixels = (size_t)a.N * HW;
    const __amdgpu_buffer_rsrc_t xrs = view_rsrc(a.x, pixels, a.ldx, a.Cin);
    const __amdgpu_buffer_rsrc_t omrs = view_rsrc(a.om, pixels, a.ldom, 27);
    const int ld4 = a.ldx * 4;
    const int c16 = a.Cin >> 4;
    const float *arow = gyt + (lane & 15) * ldg + 4 * (lane >> 4);
    for (int t = 0; t < 3; ++t) {
        const int k = tg * 3 + t;
        Samp s[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int pix = p0 + (lane >> 4) * 4 + e;
            const int h = pix / a.W;
            s[e] = make_samp(omrs, pix < HW, n * HW + pix, n, h, pix - h * a.W, k, a.H, a.W, a.ldom);
        }
        float sm[4] = {0.f, 0.f, 0.f, 0.f}, sy[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
        for (int cit = split; cit < c16; cit += a.CS) {
            const int c = cit * 16 + (lane & 15);
            float v[4][4];                                // the gather is in flight under the MFMA chain
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[e][q] = bload(xrs, cell_off(s[e], q, a.W, ld4, c * 4));
            }
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const f32x4 *wp = reinterpret_cast<const f32x4 *>(a.wT) + ((size_t)(k * c16 + cit) * a.NT) * 64 + lane;
            f32x4 b0 = wp[0], b1 = wp[a.NT > 1 ? 64 : 0];      // weight fragments two steps ahead of their MFMAs
            for (int cb = 0; cb < a.NT; ++cb) {
                const f32x4 af = *reinterpret_cast<const f32x4 *>(arow + cb * 16);
                const f32x4 bf = b0;
                b0 = b1;
                b1 = wp[(size_t)min(cb + 2, a.NT - 1) * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = acc[e];
                const float v00 = v[e][0], v01 = v[e][1], v10 = v[e][2], v11 = v[e][3];
                if (GOM) {
                    // explicit fmaf: the same bits whether or not the g_x half is compiled into the kernel
                    const float top = fmaf(s[e].hx, v00, s[e].lx * v01), bot = fmaf(s[e].hx, v10, s[e].lx * v11);
                    sm[e] = fmaf(g, fmaf(s[e].hy, top, s[e].ly * bot), sm[e]);
                    sy[e] = fmaf(g, bot - top, sy[e]);
                    sx[e] = fmaf(g, fmaf(s[e].hy, v01 - v00, s[e].ly * (v11 - v10)), sx[e]);
                }
                if (GX) {
                    const float gm = g * s[e].m;
                    const float w00 = s[e].hy * s[e].hx, w01 = s[e].hy * s[e].lx, w10 = s[e].ly * s[e].hx, w11 = s[e].ly * s[e].lx;
                    float *cell = a.gx + (size_t)s[e].base * a.ldgx + c;      // (only dereferenced under a set validity bit)
                    const size_t row = (size_t)a.W * a.ldgx;
                    if ((s[e].ok & 1) && w00 != 0.0f) unsafeAtomicAdd(cell, gm * w00);
                    if ((s[e].ok & 2) && w01 != 0.0f) unsafeAtomicAdd(cell + a.ldgx, gm * w01);
                    if ((s[e].ok & 4) && w10 != 0.0f) unsafeAtomicAdd(cell + row, gm * w10);
                    if ((s[e].ok & 8) && w11 != 0.0f) unsafeAtomicAdd(cell + row + a.ldgx, gm * w11);
                }
            }
        }
        if (GOM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    sm[e] += __shfl_xor(sm[e], d);
                    sy[e] += __shfl_xor(sy[e], d);
                    sx[e] += __shfl_xor(sx[e], d);
                }
                if ((lane & 15) == 0) {
                    float *o = red + ((split * 9 + k) * 16 + (lane >> 4) * 4 + e) * 3;
                    o[0] = s[e].m * sy[e];
                    o[1] = s[e].m * sx[e];
                    o[2] = sm[e];
                }
            }
        }
    }
    if (!GOM) return;
    __syncthreads();
    // the channel splits' partial sums in split order -> channels 2k, 2k+1, 18+k of the gradient map
    for (int i = threadIdx.x; i < 9 * 16 * 3; i += blockDim.x) {
        const int q = i % 3, p = (i / 3) & 15, k = i / 48;
        if (p0 + p >= HW) continue;
        float sum = red[i];
        for (int sp = 1; sp < a.CS; ++sp) sum += red[sp * 432 + i];
        a.gom[((size_t)n * HW + p0 + p) * a.ldgom + (q == 2 ? 18 + k : 2 * k + q)] = sum;
    }
}

constexpr int W_TILES = 12;      // accumulator tiles of a weight-kernel wave: 2 channel tiles x 4 cout tiles + 4 bias tiles

__global__ __launch_bounds__(256) void dcn_bwd_weight_kernel(BwdArgs a)
{
    __shared__ float red[3][W_TILES][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = a.H * a.W;
    const int total = a.N * HW;
    int unit = blockIdx.x;
    const int k = unit % 9;
    unit /= 9;
    const int cgroups = a.Cin >> 5;
    const int cig = unit % cgroups, cog = unit / cgroups;
    const bool withBias = k == 0 && cig == 0;
    const int nco = min(4, a.NT - cog * 4);
    const size_t pixels = (size_t)total;
    const __amdgpu_buffer_rsrc_t xrs = view_rsrc(a.x, pixels, a.ldx, a.Cin);
    const __amdgpu_buffer_rsrc_t omrs = view_rsrc(a.om, pixels, a.ldom, 27);
    const __amdgpu_buffer_rsrc_t gyrs = view_rsrc(a.gy, pixels, a.ldgy, a.Cout);
    const int ld4 = a.ldx * 4;
    f32x4 acc[W_TILES];
#pragma unroll
    for (int i = 0; i < W_TILES; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (total + 3) >> 2;
    const int s0 = min(nsteps, ((int)blockIdx.y * 4 + wave) * a.stepsPerWave);
    const int s1 = min(nsteps, s0 + a.stepsPerWave);
    // four steps (16 pixels) per round, in phases, so that the offset/mask loads, then the gathers and gy loads of all four are
    // in flight together: one step alone is a chain of three dependent memory round trips
    for (int st = s0; st < s1; st += 4) {
        Samp s[4];
        int gp[4];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            gp[u] = (st + u) * 4 + (lane >> 4);
            live[u] = st + u < s1 && gp[u] < total;
            const int n = gp[u] / HW, pix = gp[u] - n * HW, h = pix / a.W;
            s[u] = make_samp(omrs, live[u], gp[u], n, h, pix - h * a.W, k, a.H, a.W, a.ldom);
        }
        float col[4][2], g[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c4 = (cig * 32 + i * 16 + (lane & 15)) * 4;
                const float v00 = bload(xrs, cell_off(s[u], 0, a.W, ld4, c4)), v01 = bload(xrs, cell_off(s[u], 1, a.W, ld4, c4));
                const float v10 = bload(xrs, cell_off(s[u], 2, a.W, ld4, c4)), v11 = bload(xrs, cell_off(s[u], 3, a.W, ld4, c4));
                col[u][i] = s[u].m * (s[u].hy * (s[u].hx * v00 + s[u].lx * v01) + s[u].ly * (s[u].hx * v10 + s[u].lx * v11));
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int co = (cog * 4 + ct) * 16 + (lane & 15);
                g[u][ct] = bload(gyrs, (live[u] && ct < nco && co < a.Cout) ? (gp[u] * a.ldgy + co) * 4 : SENTINEL);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (ct < nco) {                                  // (uniform)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][0], acc[ct], 0, 0, 0);
                    acc[4 + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], col[u][1], acc[4 + ct], 0, 0, 0);
                    if (withBias) acc[8 + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[u][ct], 1.0f, acc[8 + ct], 0, 0, 0);
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
            if (co >= a.Cout) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ci = cig * 32 + i * 16 + (lane & 15);
                slab[((size_t)co * a.Cin + ci) * 9 + k] = acc[i * 4 + ct][e];
            }
            if (withBias && (lane & 15) == 0) slab[(size_t)a.Cout * a.Cin * 9 + co] = acc[8 + ct][e];
        }
    }
}

__global__ __launch_bounds__(256) void dcn_bwd_reduce_kernel(const float *ws, int slabs, size_t slabStride, size_t nw,
                                                             float *gw, float *gb)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slabStride) return;
    float s = 0.0f;
    for (int j = 0; j < slabs; ++j) s += ws[(size_t)j * slabStride + i];
    if (i < nw) gw[i] = s;
    else if (gb) gb[i - nw] = s;
}

__global__ __launch_bounds__(256) void zero_view_kernel(float *y, size_t pixels, int C, int ld)
{
    const size_t total = pixels * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) y[(i / C) * ld + i % C] = 0.0f;
}

__global__ __launch_bounds__(256) void pack_weight_t_kernel(const float *w, float *p, int Cout, int Cin, int NT)
{
    // p[((tap*Cin16 + c16)*NT + cb)*256 + lane*4 + j] = w[co = 16 cb + 4 (lane >> 4) + j][ci = 16 c16 + (lane & 15)][tap]
    const size_t total = (size_t)9 * (Cin >> 4) * NT * 256;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx & 3, lane = (idx >> 2) & 63;
    size_t t = idx >> 8;
    const int cb = t % NT;
    t /= NT;
    const int c16 = t % (Cin >> 4);
    const int tap = (int)(t / (Cin >> 4));
    const int co = cb * 16 + 4 * (lane >> 4) + j, ci = c16 * 16 + (lane & 15);
    p[idx] = (co < Cout) ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.0f;
}

struct BwdPlan {
    int NT, tilesPerImg, CS, slabs, stepsPerWave, units;
    size_t slabStride;
};

int make_plan(const ct_dcn_bwd_desc *d, BwdPlan *p, bool needBuffers)
{
    if (!d) CT_FAIL_ARG("ct_dcn_v2_backward: null descriptor");
    if (d->flags & ~(CT_DCN_BWD_INPUT | CT_DCN_BWD_OFFSET_MASK | CT_DCN_BWD_WEIGHT) || !d->flags)
        CT_FAIL_ARG("ct_dcn_v2_backward: flags=%d (a combination of CT_DCN_BWD_INPUT, _OFFSET_MASK, _WEIGHT)", d->flags);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) CT_FAIL_ARG("ct_dcn_v2_backward: bad shape");
    if (d->Cin % 32 || d->Cin <= 0) CT_FAIL_ARG("ct_dcn_v2_backward: Cin=%d must be a positive multiple of 32", d->Cin);
    if (d->Cout > 512) CT_FAIL_ARG("ct_dcn_v2_backward: Cout=%d above 512 (the gy tile of the data kernel lives in LDS)", d->Cout);
    const bool data = d->flags & (CT_DCN_BWD_INPUT | CT_DCN_BWD_OFFSET_MASK);
    if (needBuffers) {
        if (!d->x || !d->om || !d->gy) CT_FAIL_ARG("ct_dcn_v2_backward: null pointer (x / om / gy)");
        if (data && !d->wT_packed) CT_FAIL_ARG("ct_dcn_v2_backward: null pointer (wT_packed)");
        if ((d->flags & CT_DCN_BWD_INPUT) && !d->gx) CT_FAIL_ARG("ct_dcn_v2_backward: null pointer (gx)");
        if ((d->flags & CT_DCN_BWD_OFFSET_MASK) && !d->gom) CT_FAIL_ARG("ct_dcn_v2_backward: null pointer (gom)");
        if ((d->flags & CT_DCN_BWD_WEIGHT) && !d->gw) CT_FAIL_ARG("ct_dcn_v2_backward: null pointer (gw)");
        if (data && ((uintptr_t)d->wT_packed & 15)) CT_FAIL_ARG("ct_dcn_v2_backward: wT_packed must be 16-byte aligned");
    }
    if (d->ldx < d->Cin || d->ldgy < d->Cout || d->ldom < 27) CT_FAIL_ARG("ct_dcn_v2_backward: channel pitch below the channel count (x / gy / om)");
    if ((d->flags & CT_DCN_BWD_INPUT) && d->ldgx < d->Cin) CT_FAIL_ARG("ct_dcn_v2_backward: ldgx=%d below Cin", d->ldgx);
    if ((d->flags & CT_DCN_BWD_OFFSET_MASK) && d->ldgom < 27) CT_FAIL_ARG("ct_dcn_v2_backward: ldgom=%d below 27", d->ldgom);
    const double px = (double)d->N * d->H * d->W;
    const int maxld = d->ldx > d->ldgy ? (d->ldx > d->ldom ? d->ldx : d->ldom) : (d->ldgy > d->ldom ? d->ldgy : d->ldom);
    const int maxldo = d->ldgx > d->ldgom ? d->ldgx : d->ldgom;
    if (px * (maxld > maxldo ? maxld : maxldo) * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("ct_dcn_v2_backward: a view of 2 GiB or more (N*H*W=%.0f pixels): the kernels address every view through one buffer descriptor", px);
    p->NT = ct_cdiv(d->Cout, 16);
    p->tilesPerImg = ct_cdiv(d->H * d->W, 16);
    if ((double)d->N * p->tilesPerImg > 2147483647.0) CT_FAIL_ARG("ct_dcn_v2_backward: grid too large");
    // few pixel tiles (the deep levels of the neck): split the channel tiles over 2 or 4 wave triples of the workgroup
    const long tiles = (long)d->N * p->tilesPerImg;
    p->CS = (tiles >= 1024 || d->Cin < 64) ? 1 : (tiles >= 512 || d->Cin < 128) ? 2 : 4;
    p->units = 9 * (d->Cin / 32) * ct_cdiv(p->NT, 4);
    const int nsteps = ct_cdiv(d->N * d->H * d->W, 4);
    int slabs = ct_cdiv(1024, p->units);
    const int maxSlabs = ct_cdiv(nsteps, 32);           // at least 8 steps for each of the four waves
    if (slabs > maxSlabs) slabs = maxSlabs;
    if (slabs < 1) slabs = 1;
    p->slabs = slabs;
    p->stepsPerWave = ct_cdiv(nsteps, slabs * 4);
    p->slabStride = (size_t)d->Cout * d->Cin * 9 + d->Cout;
    return CT_OK;
}

}  // namespace

extern "C" size_t ct_packed_dcn_weight_t_elems(int Cout, int Cin)
{
    if (Cout <= 0 || Cin <= 0) return 0;
    return (size_t)9 * (Cin / 16) * ct_cdiv(Cout, 16) * 256;
}

extern "C" int ct_pack_dcn_weight_t(const float *w_oihw, float *packed, int Cout, int Cin, void *stream)
{
    if (!w_oihw || !packed) CT_FAIL_ARG("ct_pack_dcn_weight_t: null pointer");
    if (Cin % 16 || Cin <= 0 || Cout <= 0) CT_FAIL_ARG("ct_pack_dcn_weight_t: Cin=%d must be a positive multiple of 16", Cin);
    const size_t total = ct_packed_dcn_weight_t_elems(Cout, Cin);
    hipLaunchKernelGGL(pack_weight_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_oihw,
                       packed, Cout, Cin, ct_cdiv(Cout, 16));
    CT_CHECK_LAUNCH("ct_pack_dcn_weight_t");
    return CT_OK;
}

extern "C" size_t ct_dcn_v2_backward_workspace_bytes(const ct_dcn_bwd_desc *d)
{
    BwdPlan p;
    if (!d || !(d->flags & CT_DCN_BWD_WEIGHT) || make_plan(d, &p, false) != CT_OK) return 0;
    return (size_t)p.slabs * p.slabStride * sizeof(float);
}

extern "C" int ct_dcn_v2_backward(const ct_dcn_bwd_desc *d, void *stream)
{
    BwdPlan p;
    const int rc = make_plan(d, &p, true);
    if (rc != CT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    BwdArgs a;
    a.x = d->x; a.om = d->om; a.gy = d->gy; a.wT = d->wT_packed;
    a.gx = d->gx; a.gom = d->gom; a.ws = d->workspace;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.ldx = d->ldx; a.ldom = d->ldom; a.ldgy = d->ldgy; a.ldgx = d->ldgx; a.ldgom = d->ldgom;
    a.NT = p.NT; a.tilesPerImg = p.tilesPerImg; a.CS = p.CS; a.slabs = p.slabs; a.stepsPerWave = p.stepsPerWave; a.slabStride = p.slabStride;
    if (d->flags & CT_DCN_BWD_WEIGHT) {
        const size_t need = (size_t)p.slabs * p.slabStride * sizeof(float);
        if (!d->workspace || d->workspace_bytes < need) {
            ct_set_error("ct_dcn_v2_backward: workspace of %zu bytes needed (ct_dcn_v2_backward_workspace_bytes), got %zu", need,
                         d->workspace ? d->workspace_bytes : (size_t)0);
            return CT_ERR_WORKSPACE;
        }
    }
    if (d->flags & (CT_DCN_BWD_INPUT | CT_DCN_BWD_OFFSET_MASK)) {
        const bool gx = d->flags & CT_DCN_BWD_INPUT, gom = d->flags & CT_DCN_BWD_OFFSET_MASK;
        if (gx) {
            const size_t px = (size_t)d->N * d->H * d->W;
            const size_t blocks = (px * d->Cin + 255) / 256;
            hipLaunchKernelGGL(zero_view_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, d->gx, px, d->Cin, d->ldgx);
        }
        const dim3 grid((unsigned)(d->N * p.tilesPerImg));
        const size_t lds = ((size_t)16 * (p.NT * 16 + 4) + (size_t)p.CS * 432) * sizeof(float);
        const dim3 block(192 * p.CS);
        if (gx && gom) hipLaunchKernelGGL((dcn_bwd_data_kernel<true, true>), grid, block, lds, s, a);
        else if (gx) hipLaunchKernelGGL((dcn_bwd_data_kernel<true, false>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((dcn_bwd_data_kernel<false, true>), grid, block, lds, s, a);
        CT_CHECK_LAUNCH("ct_dcn_v2_backward (data)");
    }
    if (d->flags & CT_DCN_BWD_WEIGHT) {
        hipLaunchKernelGGL(dcn_bwd_weight_kernel, dim3((unsigned)p.units, (unsigned)p.slabs), dim3(256), 0, s, a);
        CT_CHECK_LAUNCH("ct_dcn_v2_backward (weight)");
        const size_t nw = (size_t)d->Cout * d->Cin * 9;
        hipLaunchKernelGGL(dcn_bwd_reduce_kernel, dim3((unsigned)((p.slabStride + 255) / 256)), dim3(256), 0, s, d->workspace,
                           p.slabs, p.slabStride, nw, d->gw, d->gb);
        CT_CHECK_LAUNCH("ct_dcn_v2_backward (reduce)");
    }
    return CT_OK;
}
