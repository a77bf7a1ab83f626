// The point-evaluation core of sparse_heads_kernel (decode.hip) and point_eval_kernel (sparse_pose.hip), which differ in where
// their points come from and in their conv1x1 tails: conv3x3 64 -> 256 + bias + ReLU of a head at 16 points, one quarter of the
// hidden channels per workgroup of 4 waves -- a [16 x 576] x [576 x 64] product on mfma_f32_16x16x4f32.  Every row of the tile
// is the same k-ordered fma chain (k = tap, slab, channel): a point's hidden values depend on its pixel alone.
#pragma once
#include "ct_common.h"

constexpr int PT_HID = 256;              // hidden channels of a head (head_conv, opts.py:294-295)
constexpr int PT_A_FLOATS = 36 * 256;    // LDS patches A: [tap * 4 + slab][16 points][16 ch], swizzled
constexpr int PT_HD_LD = 68;             // LDS hidden tile Hd: [16 points][PT_HD_LD], this quarter's 64 activations per point
constexpr int PT_HD_FLOATS = 16 * PT_HD_LD;

// This wave's weights: the 36 (tap, slab) fragments of 1 KiB for n-tile 4 * quarter + wave of a ct_pack_conv_weight
// [256,64,3,3] weight, all requested at once (callers issue this before they read their points); returns the lane's hidden bias
__device__ __forceinline__ float pt_load_weights(f32x4 (&bq)[36], const float *w1, const float *b1, int quarter, int wave, int lane)
{
    const float *wp = w1 + ((size_t)(quarter * 4 + wave) << 8) + (lane << 2);
#pragma unroll
    for (int st = 0; st < 36; ++st) bq[st] = *reinterpret_cast<const f32x4 *>(wp + (size_t)st * (16 << 8));
    return b1[quarter * 64 + wave * 16 + (lane & 15)];
}

// The 16 points' 3x3 x 64 patches into A: 16 x 9 x 16 float4 items over 256 threads.  point(m, fb, y, x) gives point m's image
// (its [h][w][ldf] base) and centre; y < 0: no point, a row of zeros, like every tap outside the map (padding 1).
// `barrier`: a workgroup barrier between the loads and the LDS stores, for a caller whose previous pass may still read A.
template <typename Point>
__device__ __forceinline__ void pt_gather_patches(float *A, int tid, int h, int w, int ldf, bool barrier, Point point)
{
    f32x4 pv[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int it = tid + 256 * j;
        const int m = it / 144, rem = it - m * 144;
        const int tap = rem >> 4, q = rem & 15;
        const float *fb;
        int cy, cx;
        point(m, fb, cy, cx);
        const int y = cy + tap / 3 - 1, x = cx + tap % 3 - 1;
        const bool ok = y >= 0 && y < h && x >= 0 && x < w && cy >= 0;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(fb + (ok ? ((size_t)y * w + x) * ldf + q * 4 : 0));
        pv[j] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (barrier) __syncthreads();
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int it = tid + 256 * j;
        const int m = it / 144, rem = it - m * 144;
        const int tap = rem >> 4, q = rem & 15;
        *reinterpret_cast<f32x4 *>(A + (tap * 4 + (q >> 2)) * 256 + m * 16 + (((q & 3) ^ ((m >> 1) & 2)) << 2)) = pv[j];
    }
}

// A x this wave's weights -> Hd: the 36 x 4 MFMA chain in k order, + bias, ReLU
__device__ __forceinline__ void pt_hidden_tile(float *Hd, const float *A, const f32x4 (&bq)[36], float bias1, int wave, int lane)
{
    const int li = lane & 15, lg = lane >> 4;
    const int aoff = li * 16 + ((lg ^ ((li >> 1) & 2)) << 2);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < 36; ++st) {
        const f32x4 af = *reinterpret_cast<const f32x4 *>(A + st * 256 + aoff);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bq[st][e], acc, 0, 0, 0);
    }
    // C layout: row (point) = lg * 4 + e, column (hidden channel of this quarter) = 16 * wave + li
#pragma unroll
    for (int e = 0; e < 4; ++e) Hd[(lg * 4 + e) * PT_HD_LD + wave * 16 + li] = fmaxf(acc[e] + bias1, 0.0f);
}
