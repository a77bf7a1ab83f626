// Training images on the device: `image` and `pre_img` of a training batch from raw u8 frames, in
// TWO launches behind ONE host-to-device copy.
//
// What the reference does per sample in a DataLoader worker (GenericDataset._get_input,
// src/lib/dataset/generic_dataset.py:317-327: cv2.warpAffine, astype(float32) / 255., color_aug of
// src/lib/utils/image.py:211-243 -- three passes over the image plus a grey image and its mean --, (x - mean) / std,
// transpose; twice with opt.tracking; collate, .to(device) of 12 bytes per pixel) splits here: the host keeps the scalar
// draws and the choice of the source rows the warp can read (InputBuilder.encode, centertrack_amd/inputs.py), this file
// does everything per pixel.
//
// Pass 1 (inputs_warp_kernel): a workgroup owns a 64 x 16 tile of one output image, a thread four pixels of one column
// (rows y, y+4, y+8, y+12).  OpenCV's fixed-point warp (csrc/ct_warp.h, the arithmetic of preprocess_kernel); the flip is
// the mirrored source column w-1-sx, taken after the border test; taps outside the whole image -- and outside the rows
// that were uploaded -- are 0.  B, G, R go into one word of warped[N][H][W]; the float32 grey values of the tile are
// added in double in a fixed order (a thread's four pixels, a fixed butterfly across the wave, the four waves in order)
// into ONE partial per workgroup.
// Pass 2 (inputs_colour_kernel): the same tiles.  A workgroup adds its image's partials in a fixed pattern (lane l of wave
// 0 takes partials l, l+64, ... in index order, then the same butterfly): the same bits in every workgroup and every run.
// gs_mean = float32(sum / (H W)); then the reference's chain per pixel in float32 with contraction off, and three
// coalesced float32 plane stores.  510 partials (4 KB) at 544 x 960, 256 (2 KB) at 512 x 512, read by a workgroup
// that reads 4 KB of warped pixels and writes 12 KB.
// Every output element is written exactly once by one thread: no memset, no atomics, outputs may hold garbage beforehand
// and two calls agree in every bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ct_common.h"
#include "ct_warp.h"

namespace {

constexpr int IN_TW = CT_INPUTS_TILE_W, IN_TH = CT_INPUTS_TILE_H, IN_DESC = CT_INPUTS_DESC_WORDS;
constexpr int IN_ROWS_PER_THREAD = IN_TH / 4;         // 256 threads: 64 columns x 4 rows, IN_TH / 4 steps of 4 rows
static_assert(IN_TW == 64 && IN_TH % 4 == 0, "a wave owns a row of the tile");

struct InArgs {
    const int *buf;
    float *out[2];
    unsigned *warped;
    double *partials;
    float *gs_mean;
    float mean[3], stdv[3];
    int B, N, H, W, tilesX, P;
};

// float32(v) / 255f, correctly rounded: what `inp.astype(np.float32) / 255.` gives (NOT the float64 table of the
// inference pre-process)
__device__ __forceinline__ float in_unit(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

// cv2.cvtColor(BGR2GRAY) of the float32 image as the golden generator states it: left to right, no FMA
__device__ __forceinline__ float in_grey(float b, float g, float r)
{
#pragma clang fp contract(off)
    return 0.114f * b + 0.587f * g + 0.299f * r;
}

__device__ __forceinline__ double in_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void inputs_warp_kernel(InArgs a)
{
#pragma clang fp contract(off)
    __shared__ double wsum[4];
    const int n = blockIdx.x / a.P, tile = blockIdx.x % a.P;
    const int *d = a.buf + (size_t)n * IN_DESC;
    const int kind = d[0];
    const int x = (tile % a.tilesX) * IN_TW + (threadIdx.x & 63);
    const int ybase = (tile / a.tilesX) * IN_TH + (threadIdx.x >> 6);
    const int h = d[4], w = d[5], stride = d[6], row0 = d[7], nrows = d[8];
    const bool flipped = d[9] != 0;
    const uint8_t *src = kind == CT_INPUTS_STAGED
        ? (const uint8_t *)a.buf + (unsigned)d[1]
        : (const uint8_t *)((unsigned long long)(unsigned)d[2] | ((unsigned long long)(unsigned)d[3] << 32));
    const double *M = (const double *)(d + 28);
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < IN_ROWS_PER_THREAD; ++r) {
        const int y = ybase + 4 * r;
        if (x >= a.W || y >= a.H) continue;
        unsigned word = 0;
        if (kind != CT_INPUTS_ZERO) {
            const CtWarpTaps t = ct_warp_taps(M, x, y);
            const int sx = t.sx, sy = t.sy;
            const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
            // rows: inside the whole image (h) AND among the rows that are present
            const bool y0 = sy >= 0 && sy < h && sy >= row0 && sy < row0 + nrows;
            const bool y1 = sy + 1 >= 0 && sy + 1 < h && sy + 1 >= row0 && sy + 1 < row0 + nrows;
            const uint8_t *r0 = src + (size_t)(y0 ? sy - row0 : 0) * stride;
            const uint8_t *r1 = src + (size_t)(y1 ? sy + 1 - row0 : 0) * stride;
            const int c0 = (x0 ? (flipped ? w - 1 - sx : sx) : 0) * 3;
            const int c1 = (x1 ? (flipped ? w - 2 - sx : sx + 1) : 0) * 3;
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int p00 = (x0 && y0) ? r0[c0 + c] : 0;
                const int p01 = (x1 && y0) ? r0[c1 + c] : 0;
                const int p10 = (x0 && y1) ? r1[c0 + c] : 0;
                const int p11 = (x1 && y1) ? r1[c1 + c] : 0;
                v[c] = ct_warp_blend(t, p00, p01, p10, p11);
            }
            word = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16);
            acc += (double)in_grey(in_unit(v[0]), in_unit(v[1]), in_unit(v[2]));
        }
        a.warped[((size_t)n * a.H + y) * a.W + x] = word;
    }
    acc = in_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partials[(size_t)n * a.P + tile] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(256) void inputs_colour_kernel(InArgs a)
{
#pragma clang fp contract(off)
    __shared__ float mean_s;
    const int n = blockIdx.x / a.P, tile = blockIdx.x % a.P;
    const int *d = a.buf + (size_t)n * IN_DESC;
    const int kind = d[0];
    const bool colour = kind != CT_INPUTS_ZERO && d[10] != 0;
    const bool need_mean = kind != CT_INPUTS_ZERO && (colour || a.gs_mean != nullptr);        // (uniform)
    float gs_mean = 0.0f;
    if (need_mean) {
        if (threadIdx.x < 64) {
            const double *p = a.partials + (size_t)n * a.P;
            double s = 0.0;
            for (int i = threadIdx.x; i < a.P; i += 64) s += p[i];
            s = in_wave_sum(s);
            if (threadIdx.x == 0) mean_s = (float)(s / (double)((long long)a.H * a.W));
        }
        __syncthreads();
        gs_mean = mean_s;
    }
    if (a.gs_mean && tile == 0 && threadIdx.x == 0) a.gs_mean[n] = gs_mean;
    const int x = (tile % a.tilesX) * IN_TW + (threadIdx.x & 63);
    const int ybase = (tile / a.tilesX) * IN_TH + (threadIdx.x >> 6);
    const int f0 = d[11], f1 = d[12], f2 = d[13];
    const float al0 = __int_as_float(d[14]), al1 = __int_as_float(d[15]), al2 = __int_as_float(d[16]);
    const float om0 = __int_as_float(d[17]), om1 = __int_as_float(d[18]), om2 = __int_as_float(d[19]);
    const double *light = (const double *)(d + 20);
    const double l0 = light[0], l1 = light[1], l2 = light[2];
    const int slot = n / a.B, b = n % a.B;
    const size_t plane = (size_t)a.H * a.W;
    float *out = a.out[slot] + (size_t)b * 3 * plane;
#pragma unroll
    for (int r = 0; r < IN_ROWS_PER_THREAD; ++r) {
        const int y = ybase + 4 * r;
        if (x >= a.W || y >= a.H) continue;
        const size_t o = (size_t)y * a.W + x;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (kind != CT_INPUTS_ZERO) {
            const unsigned word = a.warped[(size_t)n * plane + o];
            v0 = in_unit(word & 255u); v1 = in_unit((word >> 8) & 255u); v2 = in_unit((word >> 16) & 255u);
            if (colour) {
                const float gs = in_grey(v0, v1, v2);          // once, before any function runs
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int f = k == 0 ? f0 : (k == 1 ? f1 : f2);
                    const float al = k == 0 ? al0 : (k == 1 ? al1 : al2);
                    const float om = k == 0 ? om0 : (k == 1 ? om1 : om2);
                    if (f == 0) {                               // brightness_: image *= alpha
                        v0 = v0 * al; v1 = v1 * al; v2 = v2 * al;
                    } else {                                    // blend_: image *= alpha; other *= 1 - alpha; image += other
                        const float other = (f == 1 ? gs_mean : gs) * om;          // contrast_: gs_mean; saturation_: gs
                        v0 = v0 * al + other; v1 = v1 * al + other; v2 = v2 * al + other;
                    }
                }
                // lighting_: float32 image += float64 vector, added in float64
                v0 = (float)((double)v0 + l0); v1 = (float)((double)v1 + l1); v2 = (float)((double)v2 + l2);
            }
            v0 = __fdiv_rn(v0 - a.mean[0], a.stdv[0]);
            v1 = __fdiv_rn(v1 - a.mean[1], a.stdv[1]);
            v2 = __fdiv_rn(v2 - a.mean[2], a.stdv[2]);
        }
        out[o] = v0; out[plane + o] = v1; out[2 * plane + o] = v2;
    }
}

bool in_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace

extern "C" size_t ct_build_inputs_partials(int H, int W)
{
    if (H <= 0 || W <= 0) return 0;
    return (size_t)ct_cdiv(W, IN_TW) * (size_t)ct_cdiv(H, IN_TH);
}

extern "C" int ct_build_inputs(const ct_inputs_desc *d, void *stream)
{
    if (!d) CT_FAIL_ARG("ct_build_inputs: null descriptor");
    if (!d->staging_host || !d->staging_dev) CT_FAIL_ARG("ct_build_inputs: null staging pointer");
    if (!d->image || !d->warped || !d->partials) CT_FAIL_ARG("ct_build_inputs: null pointer (image / warped / partials)");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || (d->N != d->B && d->N != 2 * (long long)d->B))
        CT_FAIL_ARG("ct_build_inputs: bad sizes (B %d, N %d, H %d, W %d): N is B or 2 B", d->B, d->N, d->H, d->W);
    if ((d->N == d->B) != (d->pre_img == nullptr))
        CT_FAIL_ARG("ct_build_inputs: null pointer: pre_img goes with N = 2 B and only with it");
    for (int c = 0; c < 3; ++c)
        if (!in_finite(d->mean[c]) || !in_finite(d->stdv[c]) || d->stdv[c] == 0.0f)
            CT_FAIL_ARG("ct_build_inputs: mean / std of channel %d not finite or std 0", c);
    const long long N = d->N, header = N * IN_DESC * 4, bytes = (long long)d->bytes;
    if (bytes < header || bytes >= (1LL << 31) || (bytes & 3))
        CT_FAIL_ARG("ct_build_inputs: staging buffer of %lld bytes (a multiple of 4 below 2 GiB), the descriptors alone take %lld",
                    bytes, header);
    const long long P = (long long)ct_build_inputs_partials(d->H, d->W);
    if (N * P >= (1LL << 31)) CT_FAIL_ARG("ct_build_inputs: %lld workgroups: batch too large for one launch", N * P);
    for (int n = 0; n < d->N; ++n) {
        const int *q = d->staging_host + (size_t)n * IN_DESC;
        const int kind = q[0];
        if (kind != CT_INPUTS_STAGED && kind != CT_INPUTS_DEVICE && kind != CT_INPUTS_ZERO)
            CT_FAIL_ARG("ct_build_inputs: image %d: kind %d", n, kind);
        if (kind == CT_INPUTS_ZERO) continue;
        const long long h = q[4], w = q[5], stride = q[6], row0 = q[7], nrows = q[8];
        if (h <= 0 || w <= 0) CT_FAIL_ARG("ct_build_inputs: image %d: source of %lld x %lld", n, h, w);
        if (stride < 3 * w) CT_FAIL_ARG("ct_build_inputs: image %d: stride %lld below 3 w = %lld", n, stride, 3 * w);
        if (row0 < 0 || nrows < 0 || row0 + nrows > h)
            CT_FAIL_ARG("ct_build_inputs: image %d: rows [%lld, %lld) outside the image of %lld rows", n, row0, row0 + nrows, h);
        const long long extent = nrows > 0 ? (nrows - 1) * stride + 3 * w : 0;
        if (kind == CT_INPUTS_STAGED) {
            const long long off = q[1];
            if (off < header || off > bytes || extent > bytes - off)
                CT_FAIL_ARG("ct_build_inputs: image %d: rows at offset %lld (%lld bytes) beyond the buffer of %lld", n, off,
                            extent, bytes);
        } else if (nrows > 0 && q[2] == 0 && q[3] == 0) {
            CT_FAIL_ARG("ct_build_inputs: image %d: null pointer for a source on the device", n);
        }
        if ((q[9] != 0 && q[9] != 1) || (q[10] != 0 && q[10] != 1))
            CT_FAIL_ARG("ct_build_inputs: image %d: flipped %d / colour %d are 0 or 1", n, q[9], q[10]);
        unsigned seen = 0;
        for (int k = 0; k < 3; ++k)
            if (q[11 + k] >= 0 && q[11 + k] <= 2) seen |= 1u << q[11 + k];
        if (seen != 7u)
            CT_FAIL_ARG("ct_build_inputs: image %d: function order (%d, %d, %d) is no permutation of 0..2", n, q[11], q[12], q[13]);
        double T[6];
        memcpy(T, q + 28, sizeof T);
        for (int i = 0; i < 6; ++i)
            if (!in_finite(T[i])) CT_FAIL_ARG("ct_build_inputs: image %d: matrix entry %d is not finite", n, i);
        if (T[0] * T[4] - T[1] * T[3] == 0.0) CT_FAIL_ARG("ct_build_inputs: image %d: singular matrix", n);
    }
    // dst -> src maps, inverted like cv::warpAffine does (host, float64), over the forward maps
    for (int n = 0; n < d->N; ++n) {
        int *q = d->staging_host + (size_t)n * IN_DESC;
        if (q[0] == CT_INPUTS_ZERO) continue;
        double T[6], M[6];
        memcpy(T, q + 28, sizeof T);
        ct_affine_inverse(T, M);
        memcpy(q + 28, M, sizeof M);
    }
    InArgs a;
    a.buf = d->staging_dev; a.out[0] = d->image; a.out[1] = d->pre_img;
    a.warped = d->warped; a.partials = d->partials; a.gs_mean = d->gs_mean;
    for (int c = 0; c < 3; ++c) { a.mean[c] = d->mean[c]; a.stdv[c] = d->stdv[c]; }
    a.B = d->B; a.N = d->N; a.H = d->H; a.W = d->W; a.tilesX = ct_cdiv(d->W, IN_TW); a.P = (int)P;
    if (hipMemcpyAsync(d->staging_dev, d->staging_host, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream) !=
        hipSuccess) {
        ct_set_error("ct_build_inputs: upload failed: %s", hipGetErrorString(hipGetLastError()));
        return CT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(inputs_warp_kernel, dim3((unsigned)(N * P)), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH("ct_build_inputs (warp)");
    hipLaunchKernelGGL(inputs_colour_kernel, dim3((unsigned)(N * P)), dim3(256), 0, (hipStream_t)stream, a);
    CT_CHECK_LAUNCH("ct_build_inputs (colour)");
    return CT_OK;
}
