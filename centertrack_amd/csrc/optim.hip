// Fused optimizer step: torch.optim.Adam / torch.optim.SGD for every tensor of an optimizer in one
// launch.  The work is cut into chunks of CT_OPTIM_CHUNK elements; `prefix` (behind the records in the same upload) holds
// the number of chunks in front of every tensor, and a workgroup finds the tensor of its chunk by binary search in it:
// uniform loads only, so the search runs on the scalar unit.  Memory-bound: 16 bytes per lane where the tensor's pointers
// allow it, the grid capped and strided.  Plain loads and stores, no atomics, no LDS.
#include "ct_common.h"

namespace {

constexpr int OPT_CHUNK = CT_OPTIM_CHUNK, OPT_THREADS = 256, OPT_MAX_BLOCKS = 2048;
static_assert(sizeof(ct_optim_rec) == CT_OPTIM_REC_BYTES && (CT_OPTIM_REC_BYTES & (CT_OPTIM_REC_BYTES - 1)) == 0,
              "ct_optim_rec: fixed power-of-two size");
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is whole passes of 16-byte lanes");

// One element, in torch's order and rounding: every product and sum rounded on its own (no fused multiply-add).
template <int KIND>
__device__ __forceinline__ void optim_update(float &p, float g, float &m, float &v, const float *s, bool first, bool has_m)
{
#pragma clang fp contract(off)
    if (KIND == CT_OPTIM_ADAM) {
        const float wd = s[6];
        if (wd != 0.0f) g = g + wd * p;
        m = m + s[0] * (g - m);
        v = s[1] * v + (s[2] * g) * g;
        const float denom = sqrtf(v) / s[4] + s[5];
        p = p + (-s[3]) * (m / denom);
    } else {
        const float wd = s[2];
        if (wd != 0.0f) g = g + wd * p;
        if (has_m) {
            m = first ? g : s[1] * m + g;
            g = m;
        }
        p = p + (-s[0]) * g;
    }
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const ct_optim_rec *recs, const int *prefix, int n)
{
    const int total = prefix[n];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = n;                          // prefix[lo] <= c < prefix[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= c) lo = mid;
            else hi = mid;
        }
        const ct_optim_rec &r = recs[lo];
        const long long base = (long long)(c - prefix[lo]) * OPT_CHUNK;
        const long long left = r.numel - base;
        if (left <= 0) continue;                     // (a table that disagrees with itself: touch nothing)
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        float s[CT_OPTIM_SCALARS];
#pragma unroll
        for (int i = 0; i < CT_OPTIM_SCALARS; ++i) s[i] = r.s[i];
        const bool first = r.first != 0, has_m = r.m != nullptr;
        float *p = r.p + base;
        const float *g = r.g + base;
        float *m = has_m ? r.m + base : nullptr;
        float *v = KIND == CT_OPTIM_ADAM ? r.v + base : nullptr;
        // base is a multiple of 4 elements: a chunk is 16-byte aligned exactly when its tensor is
        const uintptr_t bits = (uintptr_t)r.p | (uintptr_t)r.g | (uintptr_t)r.m | (KIND == CT_OPTIM_ADAM ? (uintptr_t)r.v : 0);
        int done = 0;
        if ((bits & 15) == 0) {
            const int n4 = cnt >> 2;
            for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
                f32x4 pv = reinterpret_cast<const f32x4 *>(p)[i];
                const f32x4 gv = reinterpret_cast<const f32x4 *>(g)[i];
                f32x4 mv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
                if (has_m && !(KIND == CT_OPTIM_SGD && first)) mv = reinterpret_cast<const f32x4 *>(m)[i];
                if (KIND == CT_OPTIM_ADAM) vv = reinterpret_cast<const f32x4 *>(v)[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pv[e], me = mv[e], ve = vv[e];
                    optim_update<KIND>(pe, gv[e], me, ve, s, first, has_m);
                    pv[e] = pe; mv[e] = me; vv[e] = ve;
                }
                reinterpret_cast<f32x4 *>(p)[i] = pv;
                if (has_m) reinterpret_cast<f32x4 *>(m)[i] = mv;
                if (KIND == CT_OPTIM_ADAM) reinterpret_cast<f32x4 *>(v)[i] = vv;
            }
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < cnt; i += OPT_THREADS) {
            float pe = p[i], me = 0.f, ve = 0.f;
            if (has_m && !(KIND == CT_OPTIM_SGD && first)) me = m[i];
            if (KIND == CT_OPTIM_ADAM) ve = v[i];
            optim_update<KIND>(pe, g[i], me, ve, s, first, has_m);
            p[i] = pe;
            if (has_m) m[i] = me;
            if (KIND == CT_OPTIM_ADAM) v[i] = ve;
        }
    }
}

}  // namespace

extern "C" int ct_optim_step(const void *table, int n, long long chunks, int kind, void *stream)
{
    if (!table) CT_FAIL_ARG("ct_optim_step: null table");
    if (n <= 0 || n > CT_OPTIM_MAX_TENSORS) CT_FAIL_ARG("ct_optim_step: %d tensors outside [1, %d]", n, CT_OPTIM_MAX_TENSORS);
    if (chunks < n || chunks >= (1LL << 31))
        CT_FAIL_ARG("ct_optim_step: %lld chunks for %d tensors outside [n, 2^31)", chunks, n);
    if (kind != CT_OPTIM_ADAM && kind != CT_OPTIM_SGD) CT_FAIL_ARG("ct_optim_step: kind %d is neither Adam nor SGD", kind);
    const ct_optim_rec *recs = (const ct_optim_rec *)table;
    const int *prefix = (const int *)(recs + n);
    const unsigned grid = (unsigned)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    if (kind == CT_OPTIM_ADAM)
        hipLaunchKernelGGL(optim_step_kernel<CT_OPTIM_ADAM>, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, recs, prefix, n);
    else
        hipLaunchKernelGGL(optim_step_kernel<CT_OPTIM_SGD>, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, recs, prefix, n);
    CT_CHECK_LAUNCH("ct_optim_step");
    return CT_OK;
}
