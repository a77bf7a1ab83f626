// Sparse heads of the pose task (opt.sparse_pose_heads, opt-in; no reference equivalent).  generic_decode reads `hps` at the K
// winners only (decode.py:161-167) and the joint offset head -- `hp_offset`, else `reg` -- at the K peaks of every joint
// heat-map (decode.py:21-28): B*K + B*J*K pixels of B*h*w.  ct_decode_pose_sparse never makes those two maps:
//
//   1. the joint decode of ct_decode_pose, unchanged (csrc/pose.hip: hm_hp as B*J one-class images through ct_decode);
//   2. point_eval_kernel: conv3x3 64 -> 256 + bias + ReLU + conv1x1 256 -> c of a head at a LIST of points -- up to three
//      lists in one launch: hps at the winners of image b, hps at their mirrored pixels in image flip_B + b (flip_test),
//      the offset head at the joint peaks.  The contraction is the shared core of csrc/point_heads.h, which
//      sparse_heads_kernel (csrc/decode.hip) calls too: one workgroup = 16 points x one quarter of the 256 hidden channels,
//      the wave's weights requested before the points are read.  The kernel's own part is the tail: any c <= 64 output
//      channels (hps has 2J = 34), the quarter's slice of the 1x1 weights staged in LDS, partials laid out
//      [quarter][point][c].  A point's value depends on its pixel alone, not on its place in a tile or in the launch: every
//      row of the MFMA tile is the same k-ordered fma chain and every (point, channel) of the tail the same 64-term sum;
//   3. pose_values_kernel: the four quarters summed in order (no atomics), + bias, and for hps under flip_test the merge of
//      ct_flip_merge's CT_FLIP_JOINT_OFFSETS at the point: (a + s * b) / 2 with b the partner joint's pair of the mirrored
//      image, x negated -> compact hps [B*K][2J] and offsets [B*J*K][2];
//   4. pose_match_kernel / pose_score_kernel (csrc/pose.hip) reading the compact values instead of maps.
// Every peak is evaluated, also those the match drops (score <= 0.2): the compact buffers are complete, and K peaks of 17 joints
// are 107 tiles -- one round of workgroups.
#include <stdint.h>

#include "ct_common.h"
#include "point_heads.h"

namespace {

constexpr int PT_MAX_C = 64;         // output channels of the widest head the tail takes
constexpr int PT_MAX_JOBS = 3;
constexpr int PT_MAX_JOINTS = 32;

struct PtJob {                       // one head at one point list
    const float *w1, *b1, *w2;       // ct_pack_conv_weight [256,64,3,3], [256], [c][256]
    const long long *idx;            // [P] flat pixels; point r lies in image img0 + r / per_image
    float *partial;                  // [4 quarters][P][c]
    int P, per_image, img0, mirror, c, tile0;
};

struct PtArgs {
    const float *feat; int ldf; size_t feat_bs;
    int h, w, njobs;
    PtJob job[PT_MAX_JOBS];
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void point_eval_kernel(PtArgs a)
{
    __shared__ __attribute__((aligned(16))) float A[PT_A_FLOATS];         // the 16 points' patches (point_heads.h)
    __shared__ __attribute__((aligned(16))) float Hd[PT_HD_FLOATS];       // this quarter's 64 hidden activations per point
    __shared__ float W2[PT_MAX_C * 65];                                   // this quarter's [c][64] slice of the 1x1 weights
    __shared__ int wy[16], wx[16], wi[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quarter = blockIdx.x & 3;
    const int tile = blockIdx.x >> 2;
    int ji = 0;
    for (int q = 1; q < a.njobs; ++q)
        if (tile >= a.job[q].tile0) ji = q;
    const PtJob &jb = a.job[ji];
    const int r0 = (tile - jb.tile0) * 16;
    const int HW = a.h * a.w;
    f32x4 bq[36];
    const float bias1 = pt_load_weights(bq, jb.w1, jb.b1, quarter, wave, lane);            // (requested before the points are read)
    const int cout = jb.c;
    for (int i = tid; i < cout * 64; i += 256) W2[(i >> 6) * 65 + (i & 63)] = jb.w2[(size_t)(i >> 6) * PT_HID + quarter * 64 + (i & 63)];
    if (tid < 16) {
        const int r = r0 + tid;
        int y = -4, x = -4, img = 0;
        if (r < jb.P) {
            const long long p = jb.idx[r];
            if (p >= 0 && p < HW) {                               // (anything else is no pixel: a row of zeros)
                y = (int)p / a.w; x = (int)p - y * a.w;
                if (jb.mirror) x = a.w - 1 - x;
                img = jb.img0 + r / jb.per_image;
            }
        }
        wy[tid] = y; wx[tid] = x; wi[tid] = img;
    }
    __syncthreads();
    // ---- the 16 points' patches (rows past P: zero), each from its own image, the mirror already in wx ----
    pt_gather_patches(A, tid, a.h, a.w, a.ldf, false, [&](int m, const float *&img, int &y, int &x) {
        img = a.feat + (size_t)wi[m] * a.feat_bs; y = wy[m]; x = wx[m];
    });
    __syncthreads();
    pt_hidden_tile(Hd, A, bq, bias1, wave, lane);
    __syncthreads();
    // ---- this quarter's share of conv1x1 256 -> c: one lane per (point, channel), its 64 hidden values in order ----
    for (int o = tid; o < 16 * cout; o += 256) {
        const int m = o / cout, c = o - m * cout;
        const float *hh = Hd + m * PT_HD_LD, *ww = W2 + c * 65;
        float sum = 0.f;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) sum += hh[j] * ww[j];
        const int r = r0 + m;
        if (r < jb.P) jb.partial[((size_t)quarter * jb.P + r) * cout + c] = sum;
    }
}

struct ValArgs {
    const float *ph0, *ph1, *po;     // partials: hps in image b, hps in the mirrored image (flip_test), the offset head
    const float *hps_b2, *off_b2;
    float *chps, *coff;              // [B*K][2J], [B*J*K][2]
    int nh, no, J2, BK, BJK;         // nh = B*K*2J values of hps, no = B*J*K*2 of the offset head (0: none)
    unsigned char partner[PT_MAX_JOINTS];
};

// quarters summed in order: deterministic
__device__ __forceinline__ float sum_quarters(const float *p, size_t q_stride, size_t at)
{
    float v = p[at];
    v += p[q_stride + at];
    v += p[2 * q_stride + at];
    v += p[3 * q_stride + at];
    return v;
}

__global__ __launch_bounds__(256) void pose_values_kernel(ValArgs a)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.nh) {
        const int pt = i / a.J2, c = i - pt * a.J2;
        const size_t qs = (size_t)a.BK * a.J2;
        float v = sum_quarters(a.ph0, qs, i) + a.hps_b2[c];
        if (a.ph1) {                                              // flip_lr_off at the point (csrc/flip.hip)
            const int cs = 2 * a.partner[c >> 1] + (c & 1);
            const float v1 = sum_quarters(a.ph1, qs, (size_t)pt * a.J2 + cs) + a.hps_b2[cs];
            const float sgn = (c & 1) ? 1.0f : -1.0f;
            v = (v + sgn * v1) * 0.5f;
        }
        a.chps[i] = v;
    } else if (i - a.nh < a.no) {
        const int o = i - a.nh;
        a.coff[o] = sum_quarters(a.po, (size_t)a.BJK * 2, o) + a.off_b2[o & 1];
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int check(const ct_pose_sparse_desc *d, const char *who)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", who);
    const ct_pose_desc *b = &d->base;
    if (b->hps || b->hp_offset)
        CT_FAIL_ARG("%s: base.hps and base.hp_offset must be NULL (the heads are evaluated from their weights, a map beside them is ambiguous)", who);
    int rc = ct_pose_check(b, who, 1);
    if (rc != CT_OK) return rc;
    if (b->num_joints < 1 || b->num_joints > PT_MAX_JOINTS) CT_FAIL_ARG("%s: num_joints=%d out of range (1..%d)", who, b->num_joints, PT_MAX_JOINTS);
    rc = ct_check_sparse_feat(who, d->feat, d->ldf, d->flip_B, b->B);
    if (rc != CT_OK) return rc;
    if (!ct_sparse_head_ok(d->hps_w1, d->hps_b1, d->hps_w2, d->hps_b2, false)) CT_FAIL_ARG("%s: the hps head is incomplete", who);
    if (!ct_sparse_head_ok(d->off_w1, d->off_b1, d->off_w2, d->off_b2, true))
        CT_FAIL_ARG("%s: the offset head is incomplete (all four pointers, or none for +0.5)", who);
    if (d->flip_B > 0) {
        if (!d->flip_pairs || d->num_pairs < 0) CT_FAIL_ARG("%s: flip_B needs flip_pairs (num_pairs may be 0)", who);
        for (int k = 0; k < 2 * d->num_pairs; ++k)
            if (d->flip_pairs[k] < 0 || d->flip_pairs[k] >= b->num_joints) CT_FAIL_ARG("%s: bad joint pair %d", who, k / 2);
    }
    return CT_OK;
}

struct Carve {                       // the workspace, in order
    size_t chps, coff, jrows, jinds, sc, ph0, ph1, po, inner, total;
};

int carve(const ct_pose_sparse_desc *d, Carve *c)
{
    const ct_pose_desc *b = &d->base;
    ct_decode_desc jd;
    ct_pose_joint_desc(b, &jd);
    const size_t inner = ct_decode_workspace_bytes(&jd);
    if (!inner) return CT_ERR_ARG;
    const size_t BK = (size_t)b->B * b->K, BJK = BK * b->num_joints, J2 = (size_t)2 * b->num_joints;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    c->chps = take(BK * J2 * sizeof(float));
    c->coff = take(BJK * 2 * sizeof(float));
    c->jrows = take(BJK * 4 * sizeof(float));
    c->jinds = take(BJK * sizeof(int64_t));
    c->sc = take(BJK * sizeof(float));
    c->ph0 = take(4 * BK * J2 * sizeof(float));
    c->ph1 = take(d->flip_B > 0 ? 4 * BK * J2 * sizeof(float) : 0);
    c->po = take(d->off_w1 ? 4 * BJK * 2 * sizeof(float) : 0);
    c->inner = take(inner);
    c->total = at;
    return CT_OK;
}

}  // namespace

extern "C" int ct_decode_pose_sparse_workspace_bytes(const ct_pose_sparse_desc *d, size_t *bytes)
{
    if (!bytes) CT_FAIL_ARG("ct_decode_pose_sparse_workspace_bytes: null result pointer");
    *bytes = 0;
    int rc = check(d, "ct_decode_pose_sparse_workspace_bytes");
    if (rc != CT_OK) return rc;
    Carve c;
    rc = carve(d, &c);
    if (rc != CT_OK) return rc;
    *bytes = c.total;
    return CT_OK;
}

extern "C" int ct_decode_pose_sparse(const ct_pose_sparse_desc *d, void *stream)
{
    int rc = check(d, "ct_decode_pose_sparse");
    if (rc != CT_OK) return rc;
    const ct_pose_desc *b = &d->base;
    if (!b->out) CT_FAIL_ARG("ct_decode_pose_sparse: null output");
    if (b->out_stride && b->out_stride < 2 * b->num_joints + 1) CT_FAIL_ARG("ct_decode_pose_sparse: out_stride %d too small", b->out_stride);
    Carve c;
    rc = carve(d, &c);
    if (rc != CT_OK) return rc;
    if (!b->workspace || b->workspace_bytes < c.total) {
        ct_set_error("ct_decode_pose_sparse: needs %zu workspace bytes, got %zu", c.total, b->workspace_bytes);
        return CT_ERR_WORKSPACE;
    }
    // (every argument error has returned: a refused call leaves nothing enqueued)
    char *ws = (char *)b->workspace;
    float *jrows = (float *)(ws + c.jrows);
    int64_t *jinds = (int64_t *)(ws + c.jinds);
    ct_decode_desc jd;
    ct_pose_joint_desc(b, &jd);
    jd.out = jrows; jd.inds = jinds;
    jd.workspace = ws + c.inner; jd.workspace_bytes = b->workspace_bytes - c.inner;
    rc = ct_decode(&jd, stream);           // 1. K peaks of every joint heat-map
    if (rc != CT_OK) return rc;
    const int J = b->num_joints, BK = b->B * b->K, BJK = BK * J;
    const bool flip = d->flip_B > 0, off = d->off_w1 != nullptr;
    PtArgs pa;
    pa.feat = d->feat; pa.ldf = d->ldf; pa.feat_bs = (size_t)b->h * b->w * d->ldf;
    pa.h = b->h; pa.w = b->w; pa.njobs = 0;
    int tiles = 0;
    auto job = [&](const float *w1, const float *b1, const float *w2, const int64_t *idx, size_t partial, int P, int per_image,
                   int img0, int mirror, int ch) {
        PtJob &j = pa.job[pa.njobs++];
        j.w1 = w1; j.b1 = b1; j.w2 = w2; j.idx = (const long long *)idx; j.partial = (float *)(ws + partial);
        j.P = P; j.per_image = per_image; j.img0 = img0; j.mirror = mirror; j.c = ch; j.tile0 = tiles;
        tiles += ct_cdiv(P, 16);
    };
    job(d->hps_w1, d->hps_b1, d->hps_w2, b->inds, c.ph0, BK, b->K, 0, 0, 2 * J);
    if (flip) job(d->hps_w1, d->hps_b1, d->hps_w2, b->inds, c.ph1, BK, b->K, d->flip_B, 1, 2 * J);
    if (off) job(d->off_w1, d->off_b1, d->off_w2, jinds, c.po, BJK, J * b->K, 0, 0, 2);      // (image b alone: single_flips)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(point_eval_kernel, dim3((unsigned)(tiles * 4)), dim3(256), 0, s, pa);
    CT_CHECK_LAUNCH("ct_decode_pose_sparse(points)");
    ValArgs va;
    va.ph0 = (const float *)(ws + c.ph0); va.ph1 = flip ? (const float *)(ws + c.ph1) : nullptr;
    va.po = off ? (const float *)(ws + c.po) : nullptr;
    va.hps_b2 = d->hps_b2; va.off_b2 = d->off_b2;
    va.chps = (float *)(ws + c.chps); va.coff = (float *)(ws + c.coff);
    va.J2 = 2 * J; va.BK = BK; va.BJK = BJK; va.nh = BK * 2 * J; va.no = off ? BJK * 2 : 0;
    for (int j = 0; j < PT_MAX_JOINTS; ++j) va.partner[j] = (unsigned char)j;
    for (int k = 0; flip && k < d->num_pairs; ++k) {
        // successive swaps like the reference's loop over flip_idx (ct_flip_merge does the same)
        const int u = d->flip_pairs[2 * k], v = d->flip_pairs[2 * k + 1];
        const unsigned char t = va.partner[u]; va.partner[u] = va.partner[v]; va.partner[v] = t;
    }
    hipLaunchKernelGGL(pose_values_kernel, dim3((unsigned)ct_cdiv(va.nh + va.no, 256)), dim3(256), 0, s, va);
    CT_CHECK_LAUNCH("ct_decode_pose_sparse(values)");
    return ct_pose_match(b, jrows, jinds, (float *)(ws + c.sc), va.chps, off ? va.coff : nullptr, stream);
}
