// What the training kernels share (dcn_bwd.hip, heads_bwd.hip, bn_train.hip, neck_bwd.hip, backbone_bwd.hip, stem_train.hip):
// vector and buffer-descriptor accessors, the BatchNorm pre-activation, the host checks of a view and a workspace, and the
// launch of the convolution weight gradient of heads_bwd.hip.
#pragma once
#include "ct_common.h"

// ---- device

constexpr int SENTINEL = (int)0x80000000;     // vector offset of a dropped / zero-reading buffer access (ct_common.h)

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// one descriptor over a whole NHWC view of `pixels` pixels, `C` channels at pitch `ld`
__device__ __forceinline__ __amdgpu_buffer_rsrc_t view_rsrc(const float *p, size_t pixels, int ld, int C)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, (int)(((pixels - 1) * ld + C) * 4u), 0x00020000);
}

__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, int voff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}

// The pre-activation of BatchNorm that forward and backward share, a = gamma * invstd.  The difference comes first: z - mean
// is exact where z lies within a factor of two of the mean, so what is left of a channel with |mean| >> std is the rounding
// of the fp32 mean itself times a.  The folded form fma(z, a, fma(-mean, a, beta)) rounds the shift at the size of mean * a
// on top of that: at mean 100, std 0.01 half an ulp of 1e4, 5e-4 of a pre-activation of order 1.
__device__ __forceinline__ float bn_pre(float z, float mean, float a, float beta) { return fmaf(z - mean, a, beta); }

// ---- host

// (VIEW_LIMIT, the 2 GiB bound of a view: ct_common.h)

#define CT_TRY(e) do { const int rc__ = (e); if (rc__ != CT_OK) return rc__; } while (0)

static inline bool misaligned(const void *p, uintptr_t mask = 15) { return ((uintptr_t)p & mask) != 0; }

// a view the call reads or writes: non-null, 16-byte aligned, pitch a multiple of 4 and at least C
static inline int check_view(const char *fn, const char *name, const void *ptr, int ld, int C)
{
    if (!ptr) CT_FAIL_ARG("%s: null pointer (%s)", fn, name);
    if (ld < C) CT_FAIL_ARG("%s: channel pitch of %s (%d) below the channel count %d", fn, name, ld, C);
    if (ld % 4 || misaligned(ptr)) CT_FAIL_ARG("%s: %s must be 16-byte aligned with a pitch that is a multiple of 4", fn, name);
    return CT_OK;
}

static inline int check_vec(const char *fn, const char *name, const void *ptr)
{
    if (!ptr) CT_FAIL_ARG("%s: null pointer (%s)", fn, name);
    if (misaligned(ptr)) CT_FAIL_ARG("%s: %s must be 16-byte aligned", fn, name);
    return CT_OK;
}

// the workspace of a call: `need` bytes as `query` reports them
static inline int check_workspace(const char *fn, const char *query, const void *ptr, size_t bytes, size_t need)
{
    if (!ptr || bytes < need || misaligned(ptr)) {
        ct_set_error("%s: a 16-byte aligned workspace of %zu bytes needed (%s), got %zu", fn, need, query, ptr ? bytes : (size_t)0);
        return CT_ERR_WORKSPACE;
    }
    return CT_OK;
}

// workgroups of a grid-stride kernel over `total` items, 256 threads each
static inline unsigned ew_grid(int total) { return (unsigned)(total < 2048 * 256 ? ct_cdiv(total, 256) : 2048); }

// ---- the weight gradient of a convolution (heads_bwd.hip): conv_bwd_weight_kernel<STRIDE> and slab_reduce_kernel.
// `pixels` = the pixels of gy (K of the GEMM); a slab holds Cout*Cin*taps floats, plus Cout for the bias with `biasTail`.
struct CwPlan {
    int NT, cgroups, units, slabs, stepsPerWave;
    size_t slabStride;
};
int ct_conv_weight_plan(const char *fn, int pixels, int Cin, int Cout, int taps, bool biasTail, CwPlan *p);
// gw of conv3x3(x, w, stride 2, pad 1) for a descriptor its caller has validated; `p` = the plan over N*(H/2)*(W/2) pixels, 9 taps
int ct_conv_s2_weight_launch(const ct_conv_s2_bwd_desc *d, const CwPlan &p, void *stream);
