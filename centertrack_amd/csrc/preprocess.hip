// Device-side image pre-processing: the cv2.warpAffine + normalise + HWC->CHW
// (+ flipped copy) of Detector.pre_process (src/lib/detector.py:207-239) as one kernel, so that a raw u8 frame
// is uploaded (1 byte / sample) instead of the normalised fp32 tensor and the host spends no time warping.
//
// Same arithmetic as csrc/host_preprocess.cpp (OpenCV's published fixed-point warpAffine / remapBilinear for
// CV_8U: inverse map in 10-bit fixed point, 1/32-pixel coordinates, 15-bit integer tap weights, +2^14 >> 15),
// evaluated per output pixel.  The float64 row / column terms are computed with contraction off (no FMA:
// the host rounds the product and the sum separately) and converted with round-half-even like lrint();
// the normalisation ((v / 255. - mean) / std).astype(float32) has only 256 possible inputs per channel and
// comes from a table the host builds with exactly the host path's float64 expression (ct_preprocess_lut),
// so host and device pre-processing produce identical bits.
//
// One thread per output pixel (x fastest): 4 taps x C byte loads (the source is read through L2; a
// down-scaling crop touches each source byte at most once), C coalesced fp32 plane stores (+ C mirrored).
// HBM-bound: algorithmic bytes = min(h*w, 4*dst_h*dst_w)*C source bytes + 4*C*dst_h*dst_w (x2 with flip).
#include <stdint.h>

#include "ct_common.h"
#include "ct_warp.h"

namespace {

struct PreArgs {
    const uint8_t *img;
    const float *lut;      // [C][256]
    float *out, *out_flip;
    double M[6];           // inverse map (dst -> src)
    int h, w, stride, C, dw, dh;
};

__global__ __launch_bounds__(256) void preprocess_kernel(PreArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dw || y >= a.dh) return;
    const CtWarpTaps t = ct_warp_taps(a.M, x, y);       // (csrc/ct_warp.h, shared with inputs.hip)
    const int sx = t.sx, sy = t.sy;
    const bool x0 = sx >= 0 && sx < a.w, x1 = sx + 1 >= 0 && sx + 1 < a.w;
    const bool y0 = sy >= 0 && sy < a.h, y1 = sy + 1 >= 0 && sy + 1 < a.h;
    const uint8_t *r0 = a.img + (size_t)(y0 ? sy : 0) * a.stride;
    const uint8_t *r1 = a.img + (size_t)(y1 ? sy + 1 : 0) * a.stride;
    const int c0 = (x0 ? sx : 0) * a.C, c1 = (x1 ? sx + 1 : 0) * a.C;
    const size_t plane = (size_t)a.dw * a.dh;
    const size_t o = (size_t)y * a.dw + x, of = (size_t)y * a.dw + (a.dw - 1 - x);
    for (int c = 0; c < a.C; ++c) {
        const int p00 = (x0 && y0) ? r0[c0 + c] : 0;
        const int p01 = (x1 && y0) ? r0[c1 + c] : 0;
        const int p10 = (x0 && y1) ? r1[c0 + c] : 0;
        const int p11 = (x1 && y1) ? r1[c1 + c] : 0;
        const int v = ct_warp_blend(t, p00, p01, p10, p11);
        const float f = a.lut[c * 256 + v];
        a.out[c * plane + o] = f;
        if (a.out_flip) a.out_flip[c * plane + of] = f;
    }
}

}  // namespace

extern "C" int ct_preprocess_lut(const float *mean, const float *stdv, int channels, float *lut)
{
    if (!mean || !stdv || !lut || channels < 1 || channels > 4) CT_FAIL_ARG("ct_preprocess_lut: bad argument");
    for (int c = 0; c < channels; ++c)
        for (int v = 0; v < 256; ++v)   // ((x / 255. - mean) / std).astype(float32): float64, one rounding at the end
            lut[c * 256 + v] = (float)(((double)v / 255.0 - (double)mean[c]) / (double)stdv[c]);
    return CT_OK;
}

extern "C" int ct_preprocess_device(const uint8_t *img, int h, int w, int stride, int channels, const double *trans,
                                    int dst_w, int dst_h, const float *lut, float *out, float *out_flip, void *stream)
{
    if (!img || !trans || !lut || !out) CT_FAIL_ARG("ct_preprocess_device: null pointer");
    if (h <= 0 || w <= 0 || dst_w <= 0 || dst_h <= 0 || channels < 1 || channels > 4 || stride < w * channels)
        CT_FAIL_ARG("ct_preprocess_device: bad shape");
    PreArgs a;
    ct_affine_inverse(trans, a.M);      // host, float64 (host_preprocess.cpp)
    a.img = img; a.lut = lut; a.out = out; a.out_flip = out_flip;
    a.h = h; a.w = w; a.stride = stride; a.C = channels; a.dw = dst_w; a.dh = dst_h;
    hipLaunchKernelGGL(preprocess_kernel, dim3(ct_cdiv(dst_w, 64), ct_cdiv(dst_h, 4)), dim3(256), 0,
                       (hipStream_t)stream, a);
    CT_CHECK_LAUNCH("ct_preprocess_device");
    return CT_OK;
}
