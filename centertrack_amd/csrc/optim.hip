// Fused optimizer step: torch.optim.Adam / torch.optim.SGD for every tensor of an optimizer in one
// launch.  The work is cut into chunks of CT_OPTIM_CHUNK elements; `prefix` (behind the records in the same upload) holds
// the number of chunks in front of every tensor, and a workgroup finds the tensor of its chunk by binary search in it:
// uniform loads only, so the search runs on the scalar unit.  Memory-bound: 16 bytes per lane where the tensor's pointers
// allow it, the grid capped and strided.  Plain loads and stores, no atomics, no LDS.
//
// The guarded step: ct_optim_norms walks the same table twice -- per-chunk sums of squares and
// non-finite counts, then one workgroup that adds them in a fixed order and writes the clip coefficient and the skip
// decision into ct_optim_guard -- and ct_optim_step_guarded is the step kernel with GUARDED = true, reading both.  Still no
// atomics; the only LDS is the 96 bytes through which pass 1 adds its four waves.
//
// Data-parallel training: ct_optim_pack_grads walks the table once more, in front of the two, and
// gathers every gradient (rec.src), scaled, into the flat buffer rec.g points into; the replicas all-reduce that buffer
// and the kernels above read it through rec.g, unchanged.
#include "ct_common.h"

#include <cstring>

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

// g * coef of the guarded step: one float32 product, rounded on its own
__device__ __forceinline__ float optim_clip(float g, float coef)
{
#pragma clang fp contract(off)
    return g * coef;
}

// The skipped step of SGD: nothing moves, but a momentum buffer this step was to create is filled with zeros, so that
// the next step's m = momentum * m + g is torch's first m = g.
__device__ __forceinline__ void optim_zero_first_buffers(const ct_optim_rec *recs, const int *prefix, int n)
{
    const int total = prefix[n];
    for (long long cl = blockIdx.x; cl < total; cl += gridDim.x) {
        const int c = (int)cl;
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= c) lo = mid;
            else hi = mid;
        }
        const ct_optim_rec &r = recs[lo];
        if (r.first == 0 || r.m == nullptr) continue;
        const long long base = (long long)(c - prefix[lo]) * OPT_CHUNK;
        const long long left = r.numel - base;
        if (left <= 0) continue;
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        float *m = r.m + base;
        int done = 0;
        if (((uintptr_t)r.m & 15) == 0) {
            const int n4 = cnt >> 2;
            for (int i = threadIdx.x; i < n4; i += OPT_THREADS) reinterpret_cast<f32x4 *>(m)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < cnt; i += OPT_THREADS) m[i] = 0.f;
    }
}

template <int KIND, bool GUARDED>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const ct_optim_rec *recs, const int *prefix, int n,
                                                                 const ct_optim_guard *guard)
{
    float coef = 1.0f;
    if (GUARDED) {                                   // uniform loads: every workgroup takes the same branch
        if (guard->skip != 0) {
            if (KIND == CT_OPTIM_SGD) optim_zero_first_buffers(recs, prefix, n);
            return;
        }
        coef = guard->coef;
    }
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
                    optim_update<KIND>(pe, GUARDED ? optim_clip(gv[e], coef) : gv[e], me, ve, s, first, has_m);
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
            optim_update<KIND>(pe, GUARDED ? optim_clip(g[i], coef) : g[i], me, ve, s, first, has_m);
            p[i] = pe;
            if (has_m) m[i] = me;
            if (KIND == CT_OPTIM_ADAM) v[i] = ve;
        }
    }
}

// ---- ct_optim_norms ----------------------------------------------------------------------------------------------
struct norm_part {                                   // one per chunk (pass 1) and one per tensor (pass 2), 16 bytes
    double sumsq;
    long long nonfinite;                             // (a chunk's count fits an int: the high word is the zero word)
};
static_assert(sizeof(norm_part) == 16, "norm_part: one 16-byte store");
constexpr int NORM_WAVES = OPT_THREADS / 64, NORM_PASSES = OPT_CHUNK / (4 * OPT_THREADS);
constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;

__device__ __forceinline__ int optim_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// Pass 1.  Lane l owns elements 4 (l + 256 k) + e, k = 0..3, e = 0..3, whatever the alignment, and adds them in that
// order; elements past the chunk's end count as +0.0, which changes no bit of a sum of squares.
__global__ __launch_bounds__(OPT_THREADS) void optim_norms_kernel(const ct_optim_rec *recs, const int *prefix, int n,
                                                                  norm_part *part, int chunks)
{
    __shared__ double sh_sum[2][NORM_WAVES];
    __shared__ int sh_bad[2][NORM_WAVES];
    const int total = prefix[n] < chunks ? prefix[n] : chunks;     // part holds `chunks` records: never past them
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    for (long long cl = blockIdx.x; cl < total; cl += gridDim.x, par ^= 1) {
        const int c = (int)cl;
        int lo = 0, hi = n;                          // prefix[lo] <= c < prefix[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= c) lo = mid;
            else hi = mid;
        }
        const ct_optim_rec &r = recs[lo];
        const long long base = (long long)(c - prefix[lo]) * OPT_CHUNK;
        const long long left = r.numel - base;
        const int cnt = left <= 0 ? 0 : left < OPT_CHUNK ? (int)left : OPT_CHUNK;   // (0: a table that disagrees with itself)
        const float *g = r.g + base;
        const bool vec = ((uintptr_t)r.g & 15) == 0;
        double acc = 0.0;
        int bad = 0;
#pragma unroll
        for (int k = 0; k < NORM_PASSES; ++k) {
            const int e0 = (threadIdx.x + k * OPT_THREADS) * 4;
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec && e0 + 4 <= cnt) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + e0);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = gv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e0 + e < cnt) x[e] = g[e0 + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)x[e];
                acc += d * d;                        // the product is exact: fused or not, the same bits
                bad += optim_nonfinite(x[e]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc += __shfl_xor(acc, o);
            bad += __shfl_xor(bad, o);
        }
        if (lane == 0) {
            sh_sum[par][wave] = acc;
            sh_bad[par][wave] = bad;
        }
        __syncthreads();                             // one barrier per chunk: the next chunk writes the other half
        if (threadIdx.x == 0) {
            double s = sh_sum[par][0];
            int b = sh_bad[par][0];
#pragma unroll
            for (int w = 1; w < NORM_WAVES; ++w) {
                s += sh_sum[par][w];
                b += sh_bad[par][w];
            }
            part[c] = norm_part{s, (long long)b};
        }
    }
}

// in[first .. last) added in index order on top of (s, f) by one wave: 64 records per load, then a serial chain
__device__ __forceinline__ void optim_add_in_order(const norm_part *in, long long first, long long last, int lane, double &s,
                                                   long long &f)
{
    long long fl = 0;                                // the counts are integers: any order
    for (long long i = first; i < last; i += 64) {
        norm_part v{0.0, 0};
        if (i + lane < last) v = in[i + lane];
        fl += v.nonfinite;
        const int cnt = last - i < 64 ? (int)(last - i) : 64;
        const int lo = __double2loint(v.sumsq), hi = __double2hiint(v.sumsq);
        for (int l = 0; l < cnt; ++l)                // l is uniform: two scalar lane reads and one add per record
            s += __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fl += __shfl_xor(fl, o);
    f += fl;
}

// Pass 2: one workgroup.  Wave w adds the chunks of tensors w, w + 16, .. in chunk order; then wave 0 adds the tensors
// in tensor order and lane 0 writes the guard.
__global__ __launch_bounds__(FIN_THREADS) void optim_norms_finish_kernel(const int *prefix, int n, const norm_part *part,
                                                                         norm_part *tens, double *per_tensor,
                                                                         ct_optim_guard *guard, double max_norm,
                                                                         int skip_nonfinite, int chunks)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int t = wave; t < n; t += FIN_WAVES) {
        double s = 0.0;
        long long f = 0;
        const int last = prefix[t + 1] < chunks ? prefix[t + 1] : chunks;
        optim_add_in_order(part, prefix[t], last, lane, s, f);
        if (lane == 0) {
            tens[t] = norm_part{s, f};
            if (per_tensor) per_tensor[t] = s;
        }
    }
    __syncthreads();                                 // the per-tensor records, written by this workgroup, are visible to it
    if (wave != 0) return;
    double S = 0.0;
    long long F = 0;
    optim_add_in_order(tens, 0, n, lane, S, F);
    if (lane != 0) return;
    const double norm = sqrt(S);
    const bool skip = F > 0 && skip_nonfinite != 0;
    float coef = 1.0f;
    if (max_norm > 0.0 && F == 0) {
        const double c = max_norm / (norm + 1e-6);
        if (c < 1.0) coef = (float)c;
    }
    guard->sumsq = S;
    guard->norm = norm;
    guard->nonfinite = F;
    guard->coef = coef;
    guard->skip = skip ? 1 : 0;
    guard->steps += 1;
    if (skip) guard->skipped += 1;
    if (coef < 1.0f && !skip) guard->clipped += 1;
    if (F > 0) {
        guard->nonfinite_steps += 1;
    } else {
        guard->norm_sum += norm;
        if (norm > guard->norm_max) guard->norm_max = norm;
    }
}

// ---- ct_optim_pack_grads -------------------------------------------------------------------------------------------
// The gather of data-parallel training: g[i] = src[i] * scale over whole chunks of the flat buffer
// g points into, the tail of a tensor's last chunk written as +0.0.  Lane l owns elements 4 (l + 256 k) + e of a chunk, as
// in pass 1 of the norms; a chunk of g is 16-byte aligned exactly when the flat buffer is.
__global__ __launch_bounds__(OPT_THREADS) void optim_pack_kernel(const ct_optim_rec *recs, const int *prefix, int n, float scale)
{
    const int total = prefix[n];
    for (long long cl = blockIdx.x; cl < total; cl += gridDim.x) {
        const int c = (int)cl;
        int lo = 0, hi = n;                          // prefix[lo] <= c < prefix[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= c) lo = mid;
            else hi = mid;
        }
        const ct_optim_rec &r = recs[lo];
        const long long base = (long long)(c - prefix[lo]) * OPT_CHUNK;
        const long long left = r.numel - base;
        if (left <= 0 || r.src == nullptr || r.g == nullptr) continue;   // (a table that disagrees with itself: touch nothing)
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        const float *src = r.src + base;
        float *g = const_cast<float *>(r.g) + base;
        const bool vec_in = ((uintptr_t)r.src & 15) == 0, vec_out = ((uintptr_t)r.g & 15) == 0;
#pragma unroll
        for (int k = 0; k < NORM_PASSES; ++k) {
            const int e0 = (threadIdx.x + k * OPT_THREADS) * 4;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (vec_in && e0 + 4 <= cnt) {
                x = *reinterpret_cast<const f32x4 *>(src + e0);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = optim_clip(x[e], scale);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e0 + e < cnt) x[e] = optim_clip(src[e0 + e], scale);
            }
            if (vec_out) {
                *reinterpret_cast<f32x4 *>(g + e0) = x;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e0 + e] = x[e];
            }
        }
    }
}

const char *optim_refuse(const char *who, const void *table, int n, long long chunks, int kind)
{
    static thread_local char msg[160];
    if (!table) snprintf(msg, sizeof msg, "%s: null table", who);
    else if (n <= 0 || n > CT_OPTIM_MAX_TENSORS) snprintf(msg, sizeof msg, "%s: %d tensors outside [1, %d]", who, n, CT_OPTIM_MAX_TENSORS);
    else if (chunks < n || chunks >= (1LL << 31))
        snprintf(msg, sizeof msg, "%s: %lld chunks for %d tensors outside [n, 2^31)", who, chunks, n);
    else if (kind != CT_OPTIM_ADAM && kind != CT_OPTIM_SGD) snprintf(msg, sizeof msg, "%s: kind %d is neither Adam nor SGD", who, kind);
    else return nullptr;
    return msg;
}

template <bool GUARDED>
int optim_launch(const char *who, const void *table, int n, long long chunks, int kind, const ct_optim_guard *guard, void *stream)
{
    if (const char *why = optim_refuse(who, table, n, chunks, kind)) CT_FAIL_ARG("%s", why);
    if (GUARDED && !guard) CT_FAIL_ARG("%s: null guard", who);
    const ct_optim_rec *recs = (const ct_optim_rec *)table;
    const int *prefix = (const int *)(recs + n);
    const unsigned grid = (unsigned)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    if (kind == CT_OPTIM_ADAM)
        hipLaunchKernelGGL((optim_step_kernel<CT_OPTIM_ADAM, GUARDED>), dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                           recs, prefix, n, guard);
    else
        hipLaunchKernelGGL((optim_step_kernel<CT_OPTIM_SGD, GUARDED>), dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                           recs, prefix, n, guard);
    CT_CHECK_LAUNCH(who);
    return CT_OK;
}

}  // namespace

extern "C" int ct_optim_step(const void *table, int n, long long chunks, int kind, void *stream)
{
    return optim_launch<false>("ct_optim_step", table, n, chunks, kind, nullptr, stream);
}

extern "C" int ct_optim_step_guarded(const void *table, int n, long long chunks, int kind, const ct_optim_guard *guard,
                                     void *stream)
{
    return optim_launch<true>("ct_optim_step_guarded", table, n, chunks, kind, guard, stream);
}

extern "C" int ct_optim_pack_grads(const void *table, int n, long long chunks, float scale, void *stream)
{
    if (const char *why = optim_refuse("ct_optim_pack_grads", table, n, chunks, CT_OPTIM_ADAM)) CT_FAIL_ARG("%s", why);
    unsigned bits;
    memcpy(&bits, &scale, sizeof bits);
    if ((bits & 0x7f800000u) == 0x7f800000u) CT_FAIL_ARG("ct_optim_pack_grads: scale %g is not finite", (double)scale);
    const ct_optim_rec *recs = (const ct_optim_rec *)table;
    const int *prefix = (const int *)(recs + n);
    const unsigned grid = (unsigned)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    hipLaunchKernelGGL(optim_pack_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, recs, prefix, n, scale);
    CT_CHECK_LAUNCH("ct_optim_pack_grads");
    return CT_OK;
}

extern "C" size_t ct_optim_norms_workspace_bytes(int n, long long chunks)
{
    if (n <= 0 || n > CT_OPTIM_MAX_TENSORS || chunks < n || chunks >= (1LL << 31)) return 0;
    return sizeof(norm_part) * ((size_t)chunks + (size_t)n);
}

extern "C" int ct_optim_norms(const void *table, int n, long long chunks, double max_norm, int skip_nonfinite,
                              double *per_tensor, ct_optim_guard *guard, void *workspace, size_t workspace_bytes, void *stream)
{
    if (const char *why = optim_refuse("ct_optim_norms", table, n, chunks, CT_OPTIM_ADAM)) CT_FAIL_ARG("%s", why);
    if (!guard) CT_FAIL_ARG("ct_optim_norms: null guard");
    if (!workspace) CT_FAIL_ARG("ct_optim_norms: null workspace");
    const size_t need = ct_optim_norms_workspace_bytes(n, chunks);
    if (workspace_bytes < need) CT_FAIL_ARG("ct_optim_norms: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (max_norm != max_norm) CT_FAIL_ARG("ct_optim_norms: max_norm is NaN");
    if (((uintptr_t)workspace & 15) != 0) CT_FAIL_ARG("ct_optim_norms: workspace is not 16-byte aligned");
    const ct_optim_rec *recs = (const ct_optim_rec *)table;
    const int *prefix = (const int *)(recs + n);
    norm_part *part = (norm_part *)workspace, *tens = part + chunks;
    const unsigned grid = (unsigned)(chunks < OPT_MAX_BLOCKS ? chunks : OPT_MAX_BLOCKS);
    hipLaunchKernelGGL(optim_norms_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, recs, prefix, n, part, (int)chunks);
    CT_CHECK_LAUNCH("ct_optim_norms");
    hipLaunchKernelGGL(optim_norms_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, prefix, n,
                       (const norm_part *)part, tens, per_tensor, guard, max_norm, skip_nonfinite, (int)chunks);
    CT_CHECK_LAUNCH("ct_optim_norms");
    return CT_OK;
}

