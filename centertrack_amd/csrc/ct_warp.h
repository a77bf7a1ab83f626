// The per-pixel arithmetic of OpenCV's fixed-point warpAffine / remapBilinear for CV_8U on the device, shared by the
// inference pre-process (preprocess.hip) and the training inputs (inputs.hip); csrc/host_preprocess.cpp is the host form.
// Inverse map in 10-bit fixed point, 1/32-pixel coordinates, 15-bit integer tap weights, +2^14 >> 15.  The float64 row /
// column terms are computed with contraction off (the host rounds the product and the sum separately) and converted with
// round-half-even like lrint().
#pragma once
#include <hip/hip_runtime.h>

struct CtWarpTaps {
    int sx, sy;                 // source pixel of the first tap (saturated to a short like OpenCV's map)
    int w00, w01, w10, w11;     // weights of (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1)
};

// taps of output pixel (x, y) under the inverse map M (dst -> src, ct_affine_inverse)
__device__ __forceinline__ CtWarpTaps ct_warp_taps(const double *M, int x, int y)
{
#pragma clang fp contract(off)
    const double AB = 1024.0;
    const int adelta = __double2int_rn(M[0] * (double)x * AB);
    const int bdelta = __double2int_rn(M[3] * (double)x * AB);
    const int X0 = __double2int_rn((M[1] * (double)y + M[2]) * AB) + 16;
    const int Y0 = __double2int_rn((M[4] * (double)y + M[5]) * AB) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    CtWarpTaps t;
    t.sx = max(-32768, min(32767, X >> 5));
    t.sy = max(-32768, min(32767, Y >> 5));
    const int fx = X & 31, fy = Y & 31;
    t.w00 = (32 - fx) * (32 - fy) * 32; t.w01 = fx * (32 - fy) * 32;
    t.w10 = (32 - fx) * fy * 32; t.w11 = fx * fy * 32;
    return t;
}

// the blended, rounded and saturated u8 value of four taps (taps outside the image are passed as 0)
__device__ __forceinline__ int ct_warp_blend(const CtWarpTaps &t, int p00, int p01, int p10, int p11)
{
    const int v = (p00 * t.w00 + p01 * t.w01 + p10 * t.w10 + p11 * t.w11 + (1 << 14)) >> 15;
    return max(0, min(255, v));
}
