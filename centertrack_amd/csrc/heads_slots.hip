// The heads of a training step at the object slots only: ct_slot_gather and ct_slot_fold, the two
// memory kernels around contractions that the existing entry points run (ct_conv2d, ct_heads_tail_backward,
// ct_conv2d_backward_weight with ks 1 over a map [N,1,M,9*C]).  Specification: F.unfold at the slots and its transpose.
//
//   gather  rows[n, m, tap, c] = map[n, y + ky - 1, x + kx - 1, c],  (y, x) = divmod(ind[n, m], W), tap = ky * 3 + kx;
//           0 outside the map; a whole row of 0 for a slot outside [0, H*W).  One 16-byte load and store per lane.
//   fold    map[n, y + ky - 1, x + kx - 1, c] += rows[n, m, tap, c], without atomics: one workgroup (one wave) per slot.  It
//           lists the valid slots of its image within two cells of its own in ascending slot order (ballot compaction into
//           LDS), and owns a cell of its 3x3 neighbourhood when it is the first of the list that covers the cell -- the rule
//           loss_slot_scatter_kernel has for duplicate slots.  The owner starts from the patch value of that first slot, adds
//           those of the further covering slots in list order and stores map + sum once: every cell has one writer, one order.
#include "ct_train.h"

namespace {

constexpr int SLOT_MAX_M = 8192;           // the fold's list: 4 bytes of LDS per slot of an image

struct SlotArgs {
    float *map;
    const long long *ind;
    float *rows;
    int N, H, W, C, ld, M, ldr;
};

__global__ __launch_bounds__(256) void slot_gather_kernel(SlotArgs a, int total)
{
    const int c4n = a.C >> 2, perRow = 9 * c4n;
    const long long HW = (long long)a.H * a.W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int row = i / perRow, r = i - row * perRow;
        const int tap = r / c4n, c = (r - tap * c4n) << 2;
        const int n = row / a.M;
        const long long k = a.ind[row];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k >= 0 && k < HW) {
            const int y = (int)(k / a.W), x = (int)(k - (long long)y * a.W);
            const int ky = tap / 3, kx = tap - ky * 3;
            const int yy = y + ky - 1, xx = x + kx - 1;
            if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = ld4(a.map + (((size_t)n * a.H + yy) * a.W + xx) * a.ld + c);
        }
        st4(a.rows + (size_t)row * a.ldr + tap * a.C + c, v);
    }
}

__global__ __launch_bounds__(64) void slot_fold_kernel(SlotArgs a)
{
    extern __shared__ int near_[];         // slot * 32 + (dy + 2) * 5 + dx + 2 of the valid slots within two cells, ascending
    const int n = blockIdx.x / a.M, m = blockIdx.x - n * a.M, lane = threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    const long long *ind = a.ind + (size_t)n * a.M;
    const long long k = ind[m];
    if (k < 0 || k >= HW) return;          // (the whole workgroup)
    const int y = (int)(k / a.W), x = (int)(k - (long long)y * a.W);
    int cnt = 0;
    for (int base = 0; base < a.M; base += 64) {
        const int mm = base + lane;
        int code = -1;
        if (mm < a.M) {
            const long long kk = ind[mm];
            if (kk >= 0 && kk < HW) {
                const int yy = (int)(kk / a.W), xx = (int)(kk - (long long)yy * a.W);
                const int dy = yy - y, dx = xx - x;
                if (dy >= -2 && dy <= 2 && dx >= -2 && dx <= 2) code = (dy + 2) * 5 + dx + 2;
            }
        }
        const unsigned long long mask = __ballot(code >= 0);
        if (code >= 0) near_[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = mm * 32 + code;
        cnt += __popcll(mask);
    }
    __syncthreads();
    const int c4n = a.C >> 2, items = 9 * c4n;
    const float *img = a.rows + (size_t)n * a.M * a.ldr;
    for (int i = lane; i < items; i += 64) {
        const int tap = i / c4n, c = (i - tap * c4n) << 2;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int yc = y + ky - 1, xc = x + kx - 1;
        if (yc < 0 || yc >= a.H || xc < 0 || xc >= a.W) continue;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        bool first = true, owner = true;
        for (int j = 0; j < cnt; ++j) {
            const int e = near_[j], mm = e >> 5, code = e & 31;
            const int ty = ky - (code / 5 - 2), tx = kx - (code % 5 - 2);     // the tap of slot mm that lands on (yc, xc)
            if (ty < 0 || ty > 2 || tx < 0 || tx > 2) continue;
            const f32x4 v = ld4(img + (size_t)mm * a.ldr + (ty * 3 + tx) * a.C + c);
            if (first) {
                if (mm != m) { owner = false; break; }
                acc = v;
                first = false;
            } else {
                acc += v;
            }
        }
        if (!owner) continue;
        float *p = a.map + (((size_t)n * a.H + yc) * a.W + xc) * a.ld + c;
        st4(p, ld4(p) + acc);
    }
}

int check_slots(const char *fn, const ct_slot_desc *d)
{
    if (!d) CT_FAIL_ARG("%s: null descriptor", fn);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) CT_FAIL_ARG("%s: bad shape", fn);
    if (d->M < 1 || d->M > SLOT_MAX_M) CT_FAIL_ARG("%s: M=%d slots per image (1 .. %d)", fn, d->M, SLOT_MAX_M);
    if (d->C % 4) CT_FAIL_ARG("%s: C=%d must be a multiple of 4", fn, d->C);
    CT_TRY(check_view(fn, "map", d->map, d->ld, d->C));
    CT_TRY(check_view(fn, "rows", d->rows, d->ldr, 9 * d->C));
    if (!d->ind) CT_FAIL_ARG("%s: null pointer (ind)", fn);
    if (misaligned(d->ind, 7)) CT_FAIL_ARG("%s: ind must be 8-byte aligned", fn);
    const double px = (double)d->N * d->H * d->W, slots = (double)d->N * d->M;
    if (px * d->ld * 4.0 >= VIEW_LIMIT || slots * d->ldr * 4.0 >= VIEW_LIMIT)
        CT_FAIL_ARG("%s: a view of 2 GiB or more (N*H*W=%.0f pixels, N*M=%.0f slots)", fn, px, slots);
    return CT_OK;
}

SlotArgs slot_args(const ct_slot_desc *d)
{
    SlotArgs a;
    a.map = d->map; a.ind = d->ind; a.rows = d->rows;
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.ld = d->ld; a.M = d->M; a.ldr = d->ldr;
    return a;
}

}  // namespace

extern "C" int ct_slot_gather(const ct_slot_desc *d, void *stream)
{
    CT_TRY(check_slots("ct_slot_gather", d));
    const int total = d->N * d->M * 9 * (d->C / 4);              // below 2^29: the rows view stays below 2 GiB
    hipLaunchKernelGGL(slot_gather_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, slot_args(d), total);
    CT_CHECK_LAUNCH("ct_slot_gather");
    return CT_OK;
}

extern "C" int ct_slot_fold(const ct_slot_desc *d, void *stream)
{
    CT_TRY(check_slots("ct_slot_fold", d));
    hipLaunchKernelGGL(slot_fold_kernel, dim3((unsigned)(d->N * d->M)), dim3(64), (size_t)d->M * sizeof(int), (hipStream_t)stream,
                       slot_args(d));
    CT_CHECK_LAUNCH("ct_slot_fold");
    return CT_OK;
}
