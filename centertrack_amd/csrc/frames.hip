// Video frames as decoders deliver them: the pre-processing of preprocess.hip for ALL frames of a step in
// ONE launch, from packed BGR / RGB or from YUV 4:2:0 surfaces (NV12, I420), host-staged or already on the device.
//
// A frame is described by a ct_frame_desc (format, up to three plane pointers with their pitches, h, w, the five colour
// coefficients, the map, the two output pointers); the step's descriptors sit in one pinned buffer, go up with one asynchronous
// copy and are read by one launch -- the pattern of ct_build_inputs / ct_build_targets.  Grid z is the frame: format, sizes
// and pointers are uniform per workgroup (scalar loads, no divergence inside a wave), frames of different sizes and formats
// share the launch; all frames share the output size.
//
// Arithmetic: ct_warp_taps / ct_warp_blend (csrc/ct_warp.h) and the ct_preprocess_lut table, i.e. preprocess_kernel's.  A YUV
// tap is converted to u8 B, G, R FIRST -- the integer form OpenCV publishes for COLOR_YUV2BGR_NV12: chroma nearest at
// (x >> 1, y >> 1), Y' = max(0, Y - 16), 20 fractional bits, + 2^19, arithmetic shift, saturation -- and blended afterwards;
// a tap outside the frame is B = G = R = 0, not the conversion of YUV zeros.  The output is therefore, to the bit, what
// ct_preprocess_device gives on the frame converted as a whole.
//
// One thread per output pixel, x fastest, 64 x 4 pixels per workgroup like preprocess_kernel.  Bound by bytes: a 4:2:0 tap
// costs one Y byte plus a chroma pair that the 2 x 2 taps of a pixel mostly share -- the two taps of a row have the same
// chroma column whenever sx is even, the two rows the same chroma row whenever sy is even -- so a shared sample is loaded once
// and the other loads are predicated off: 4 Y bytes + 1 .. 4 chroma pairs per pixel against 12 bytes for packed BGR.
#include <stdint.h>
#include <string.h>

#include "ct_common.h"
#include "ct_warp.h"

namespace {

struct FrArgs {
    const ct_frame_desc *desc;   // [n], device copy
    const float *lut;            // [3][256]
    int dw, dh;
};

// u8 B, G, R of one (Y, U, V) sample into p[0 .. 2].  The three values stay in registers of their own: packed into one word
// (b | g << 8 | r << 16) hipcc folds shift, saturation and packing of two of them into ONE packed instruction of gfx950, and
// the channel in its upper byte came out wrong on an MI355X where it saturates at 255.
__device__ __forceinline__ void fr_yuv_bgr(int *p, int Y, int U, int V, int cy, int cub, int cug, int cvg, int cvr)
{
    const int y = max(0, Y - 16) * cy + (1 << 19), u = U - 128, v = V - 128;
    p[0] = max(0, min(255, (y + cub * u) >> 20));
    p[1] = max(0, min(255, (y + cug * u + cvg * v) >> 20));
    p[2] = max(0, min(255, (y + cvr * v) >> 20));
}

__global__ __launch_bounds__(256) void frames_kernel(FrArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dw || y >= a.dh) return;
    const ct_frame_desc *__restrict__ d = a.desc + blockIdx.z;             // (uniform: scalar loads)
    const int fmt = d->format, h = d->h, w = d->w;
    const CtWarpTaps t = ct_warp_taps(d->M, x, y);
    const int sx = t.sx, sy = t.sy;
    const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
    const bool y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
    // taps outside the frame read pixel 0 of an inside row / column (always a valid address) and count as 0
    const int cx0 = x0 ? sx : 0, cx1 = x1 ? sx + 1 : 0, ry0 = y0 ? sy : 0, ry1 = y1 ? sy + 1 : 0;
    int p00[3], p01[3], p10[3], p11[3];     // B, G, R of the four taps
    if (fmt == CT_PIX_BGR24 || fmt == CT_PIX_RGB24) {
        const uint8_t *r0 = d->plane[0] + (size_t)ry0 * d->pitch[0], *r1 = d->plane[0] + (size_t)ry1 * d->pitch[0];
        const int o0 = fmt == CT_PIX_RGB24 ? 2 : 0, o2 = 2 - o0;           // RGB: channels 0 and 2 exchanged on load
        const int c0 = cx0 * 3, c1 = cx1 * 3;
        p00[0] = r0[c0 + o0]; p00[1] = r0[c0 + 1]; p00[2] = r0[c0 + o2];
        p01[0] = r0[c1 + o0]; p01[1] = r0[c1 + 1]; p01[2] = r0[c1 + o2];
        p10[0] = r1[c0 + o0]; p10[1] = r1[c0 + 1]; p10[2] = r1[c0 + o2];
        p11[0] = r1[c1 + o0]; p11[1] = r1[c1 + 1]; p11[2] = r1[c1 + o2];
    } else {
        const uint8_t *yr0 = d->plane[0] + (size_t)ry0 * d->pitch[0], *yr1 = d->plane[0] + (size_t)ry1 * d->pitch[0];
        // chroma: U at up[col * us], V at vp[col * us] of chroma row (row >> 1); NV12 interleaves them in plane 1
        const bool nv12 = fmt == CT_PIX_NV12;
        const uint8_t *up = d->plane[1], *vp = nv12 ? d->plane[1] + 1 : d->plane[2];
        const int us = nv12 ? 2 : 1;
        const size_t upitch = (size_t)d->pitch[1], vpitch = (size_t)(nv12 ? d->pitch[1] : d->pitch[2]);
        const int k0 = (cx0 >> 1) * us, k1 = (cx1 >> 1) * us, q0 = ry0 >> 1, q1 = ry1 >> 1;
        const bool same_col = k1 == k0, same_row = q1 == q0;
        int u00, v00, u01, v01, u10, v10, u11, v11;
        u00 = up[q0 * upitch + k0]; v00 = vp[q0 * vpitch + k0];
        u01 = u00; v01 = v00;
        if (!same_col) { u01 = up[q0 * upitch + k1]; v01 = vp[q0 * vpitch + k1]; }
        u10 = u00; v10 = v00; u11 = u01; v11 = v01;
        if (!same_row) {
            u10 = up[q1 * upitch + k0]; v10 = vp[q1 * vpitch + k0];
            u11 = u10; v11 = v10;
            if (!same_col) { u11 = up[q1 * upitch + k1]; v11 = vp[q1 * vpitch + k1]; }
        }
        const int cy = d->coef[0], cub = d->coef[1], cug = d->coef[2], cvg = d->coef[3], cvr = d->coef[4];
        fr_yuv_bgr(p00, yr0[cx0], u00, v00, cy, cub, cug, cvg, cvr);
        fr_yuv_bgr(p01, yr0[cx1], u01, v01, cy, cub, cug, cvg, cvr);
        fr_yuv_bgr(p10, yr1[cx0], u10, v10, cy, cub, cug, cvg, cvr);
        fr_yuv_bgr(p11, yr1[cx1], u11, v11, cy, cub, cug, cvg, cvr);
    }
    const bool in00 = x0 && y0, in01 = x1 && y0, in10 = x0 && y1, in11 = x1 && y1;
    const size_t plane = (size_t)a.dw * a.dh;
    const size_t o = (size_t)y * a.dw + x, of = (size_t)y * a.dw + (a.dw - 1 - x);
    float *out = d->out, *out_flip = d->out_flip;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = ct_warp_blend(t, in00 ? p00[c] : 0, in01 ? p01[c] : 0, in10 ? p10[c] : 0, in11 ? p11[c] : 0);
        const float f = a.lut[c * 256 + v];
        out[c * plane + o] = f;
        if (out_flip) out_flip[c * plane + of] = f;
    }
}

bool fr_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace

extern "C" int ct_preprocess_frames(const ct_frames_desc *d, void *stream)
{
    if (!d) CT_FAIL_ARG("ct_preprocess_frames: null descriptor");
    if (!d->staging_host || !d->staging_dev || !d->lut) CT_FAIL_ARG("ct_preprocess_frames: null pointer (staging / lut)");
    if (d->n < 1 || d->n > CT_FRAMES_MAX) CT_FAIL_ARG("ct_preprocess_frames: %d frames (1 .. %d)", d->n, CT_FRAMES_MAX);
    if (d->dst_w <= 0 || d->dst_h <= 0 || ct_cdiv(d->dst_h, 4) > 65535)       // (grid y)
        CT_FAIL_ARG("ct_preprocess_frames: output of %d x %d", d->dst_h, d->dst_w);
    for (int n = 0; n < d->n; ++n) {
        const ct_frame_desc *f = d->staging_host + n;
        if (f->format != CT_PIX_BGR24 && f->format != CT_PIX_RGB24 && f->format != CT_PIX_NV12 && f->format != CT_PIX_I420)
            CT_FAIL_ARG("ct_preprocess_frames: frame %d: format %d", n, f->format);
        if (f->h <= 0 || f->w <= 0) CT_FAIL_ARG("ct_preprocess_frames: frame %d: %d x %d", n, f->h, f->w);
        if (!f->out) CT_FAIL_ARG("ct_preprocess_frames: frame %d: null output", n);
        const bool yuv = f->format == CT_PIX_NV12 || f->format == CT_PIX_I420;
        const int planes = f->format == CT_PIX_I420 ? 3 : (yuv ? 2 : 1);
        if (yuv && ((f->w | f->h) & 1))
            CT_FAIL_ARG("ct_preprocess_frames: frame %d: a 4:2:0 frame of %d x %d (h and w are even)", n, f->h, f->w);
        for (int p = 0; p < planes; ++p) {
            if (!f->plane[p]) CT_FAIL_ARG("ct_preprocess_frames: frame %d: null plane %d", n, p);
            const long long row = !yuv ? 3LL * f->w : (p == 0 || f->format == CT_PIX_NV12 ? (long long)f->w : f->w / 2);
            if (f->pitch[p] < row)
                CT_FAIL_ARG("ct_preprocess_frames: frame %d: pitch %d of plane %d below the row's %lld bytes", n, f->pitch[p], p, row);
        }
        for (int i = 0; i < 6; ++i)
            if (!fr_finite(f->M[i])) CT_FAIL_ARG("ct_preprocess_frames: frame %d: matrix entry %d is not finite", n, i);
    }
    // dst -> src maps, inverted like cv::warpAffine does (host, float64), over the forward maps
    for (int n = 0; n < d->n; ++n) {
        double T[6];
        memcpy(T, d->staging_host[n].M, sizeof T);
        ct_affine_inverse(T, d->staging_host[n].M);
    }
    if (hipMemcpyAsync(d->staging_dev, d->staging_host, (size_t)d->n * sizeof(ct_frame_desc), hipMemcpyHostToDevice,
                       (hipStream_t)stream) != hipSuccess) {
        ct_set_error("ct_preprocess_frames: upload failed: %s", hipGetErrorString(hipGetLastError()));
        return CT_ERR_LAUNCH;
    }
    FrArgs a;
    a.desc = d->staging_dev; a.lut = d->lut; a.dw = d->dst_w; a.dh = d->dst_h;
    hipLaunchKernelGGL(frames_kernel, dim3(ct_cdiv(d->dst_w, 64), ct_cdiv(d->dst_h, 4), d->n), dim3(256), 0,
                       (hipStream_t)stream, a);
    CT_CHECK_LAUNCH("ct_preprocess_frames");
    return CT_OK;
}
