/*
 * centertrack_hip.h -- C ABI of libcentertrack_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary B5 of SURVEY.md section 8(b): these entry points are what the reference's
 * Python hot path binds instead of its PyTorch/cuDNN ops and the un-vendored DCNv2
 * CUDA extension.  Each function cites the reference interface it replaces
 * (paths relative to xingyizhou/CenterTrack).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch's allocator); the
 *     library never allocates, frees or synchronises; work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream); graph-capture safe.
 *   - return 0 on success, non-zero (CT_ERR_*) on error; ct_last_error() describes it.
 *   - activations inside the pipeline are fp32 NHWC "views": base pointer already
 *     offset to the first channel, `ld` = channel pitch in floats (>= C), so a
 *     layer can read/write a channel slice of a wider concat buffer in place
 *     (replaces torch.cat in Root.forward, dla.py:166).  Model inputs/outputs at the
 *     boundary are the reference's NCHW fp32 tensors.
 */
#ifndef CENTERTRACK_HIP_H
#define CENTERTRACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CT_OK 0
#define CT_ERR_ARG 1      /* bad shape / alignment / unsupported configuration */
#define CT_ERR_LAUNCH 2   /* hipLaunch failure (message holds hipGetErrorString) */
#define CT_ERR_WORKSPACE 3

/* epilogue flags */
#define CT_RELU 1
#define CT_OUT_NCHW 2      /* write y as NCHW [N,Cout,Ho,Wo] instead of an NHWC view */

/* ABI version of THIS header: bumped whenever a descriptor struct changes layout or a tuning key changes meaning.  A
 * binding compares it with ct_version() of the loaded library before the first descriptor call (centertrack_amd/_lib.py
 * does).  100 = rounds 1-3; 101 = ct_conv_desc.proj_* (fused Tree.project), key "stem_rows", box probes;
 * 102 = ct_decode_desc.sparse (sparse heads); 103 = the ct_calib_* box probes left this header and the library (they are
 * diagnostics of the measuring box: tools/micro/probes.hip -> tools/micro/libct_probes.so; ct_dcn_desc.w_off_winograd).
 * Added under 103 without a layout change: ct_dcn_desc.algo 53264 / 532128 / 63264 / 632128 (persistent DCN launch), the
 * tuning keys "dcn_slots" and "dcn_xcd"; ct_dcn_bwd_desc and ct_dcn_v2_backward (a new descriptor and new symbols);
 * ct_loss_head / ct_loss_desc and ct_generic_loss_* (the training loss: new descriptors and new symbols);
 * ct_conv_bwd_weight_desc / ct_heads_tail_bwd_desc, ct_conv2d_backward_weight and ct_heads_tail_backward (the backward of
 * the heads: new descriptors and new symbols). */
#define CT_ABI_VERSION 103

const char *ct_last_error(void);
int ct_version(void);                      /* CT_ABI_VERSION the library was built with */
/* Experiment knobs of the launch heuristics (process-global; not part of the reference's
 * interface): "conv_cfg" (-1 auto, 0..5 force a tile shape), "conv_pipe" (0/1 pinned B prefetch),
 * "conv_small_tiles" (below this many workgroups pick the smaller tile), "splitk_target"
 * (workgroups aimed at when splitting K), "dcn_bn" (0 auto, 64, 128), "conv_ks" (-1 auto, -2 never,
 * 0..4 force a K-split-in-workgroup tile), "conv_ks_below" / "conv_ks_waves" (K-split kernel is
 * used below this many 64x64 tiles / sized to reach this many waves), "xcd_remap" (0/1 XCD-aware workgroup order of
 * the wide layers), "heads_order" (0 = tile-major, 1 = head-major, 2 = head-major and
 * XCD-affine [default]: workgroup order of ct_heads_fused), "stem_rows" (0 auto,
 * 8 / 16: rows of 32 pixels per workgroup of ct_stem_forward), "dcn_slots" (resident workgroups of the persistent
 * DCN launches, algo 5xxxx / 6xxxx: 1024 = four per CU), "dcn_xcd" (0/1 [default]: XCD-aware workgroup order of the DCN
 * MAIN launches -- every XCD's L2 sees its own K splits and a band of consecutive pixel tiles). */
int ct_set_tuning(const char *key, int value);

/* ---- weight packing ---------------------------------------------------------------
 * MFMA-ready layout [tap][Cin/16][CoutPad/16][4][16][4] (CoutPad = Cout rounded up to
 * 16, zero filled): for one (tap, 16-channel slab, 16-cout tile) the 64 lanes of a wave
 * read one contiguous 1 KiB block, lane l holding cout (l&15), channels 4*(l>>4)..+3.
 * Source: the reference's OIHW conv weight (nn.Conv2d.weight / DCN.weight,
 * dla.py:38-66,154-172,506-518; base_model.py:24-40).  Cin must be a multiple of 16. */
size_t ct_packed_weight_elems(int Cout, int Cin, int ks);
int ct_pack_conv_weight(const float *w_oihw, float *packed, int Cout, int Cin, int ks, void *stream);
/* Winograd F(2x2,3x3) form of a 3x3 weight: U = G g G^T per (cout, cin), 16 positions in the same fragment
 * order [pos][Cin/16][CoutPad/16][4][16][4] (used by ct_conv2d algo 201 / 202). */
size_t ct_packed_winograd_elems(int Cout, int Cin);
int ct_pack_winograd_weight(const float *w_oihw, float *packed, int Cout, int Cin, void *stream);

/* ---- dense convolution (implicit GEMM on fp32 MFMA) -------------------------------
 * Replaces nn.Conv2d + eval-mode nn.BatchNorm2d (+ residual add) (+ ReLU) of BasicBlock /
 * Root / Tree.project / _make_conv_level (dla.py:38-66,154-172,206-213,293-303), the
 * DCN offset/mask conv (upstream dcn_v2.py DCN.conv_offset_mask) and the head convs
 * (base_model.py:24-65,86-90; sigmoid / depth transform of detector.py:300-308 fused).
 *   y = act( conv(x, w) * scale[c] + shift[c] + res )   ks in {1,3}, stride in {1,2},
 *   pad = ks/2; scale/shift NULL => 1/0.  Channels [sig_lo,sig_hi) get a sigmoid,
 *   channels [dep_lo,dep_hi) get 1/(sigmoid(v)+1e-6)-1 times depth_scale.  */
typedef struct ct_conv_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *w_packed; int Cout, ks, stride;
    const float *scale; const float *shift;
    const float *res; int ldr;
    float *y; int ldy;
    int flags;
    int sig_lo, sig_hi;
    int dep_lo, dep_hi; float depth_scale;
    float *workspace; size_t workspace_bytes;   /* split-K partials; may be NULL (no split) */
    int split_k;                                /* 0 = choose automatically */
    int algo;                                   /* 0 = heuristic; 1..8 = tile shape 0..7 of the row-tiled
                                                   kernel; 101..105 = K-split-in-workgroup shape 0..4
                                                   (CT_ERR_ARG if the shape cannot run this layer); 201..211 =
                                                   Winograd F(2x2,3x3) with 64px x 64 / 64 x 32 / 128 x 32 /
                                                   128 x 16 (pixels x couts) per workgroup, 205..207: 64 x 32
                                                   / 64 x 32 / 64 x 16 with K split over 2 / 4 / 4 wave groups,
                                                   208..211: 64 x 32 walking 2 / 4 / 5 / 8 cout blocks per workgroup
                                                   on one input transform (Cin == 64)
                                                   (3x3 stride 1, Cin % 64 == 0, NHWC output, needs w_winograd);
                                                   picked per layer by the host-side autotuner */
    const float *w_winograd;                    /* ct_pack_winograd_weight() of the same OIHW weight, or NULL */
    /* optional side output of a 3x3 stride-2 conv (round 3): the 2x2 / stride-2 max-pool of its INPUT, NHWC [N, H/2, W/2,
     * Cin] (pitch pool_ld) -- Tree.downsample (dla.py:207, nn.MaxPool2d(2, 2)) of the tensor tree1.conv1 reads; every
     * input pixel passes through the workgroups' LDS patches anyway, so the pool costs no launch and no extra read.
     * H and W must be even; NULL = off. */
    float *pool_y; int pool_ld;
    /* optional second output of a 3x3 stride-2 conv (round 4): Tree.project of the pooled input -- nn.Conv2d(Cin, Cout, 1,
     * bias=False) + eval-mode BatchNorm, no ReLU, applied to Tree.downsample(x) = max_pool2d(x, 2, 2) (dla.py:196-203,
     * 207, 217-218: the residual tree1 adds) -- computed by the workgroups of this launch from the input patches they
     * stage anyway (the 2x2 window of an output pixel is four taps of its 3x3 stride-2 window): one launch and one read
     * of the input less per DLA level.  proj_w_packed: ct_pack_conv_weight of the [Cout, Cin, 1, 1] weight (the SAME
     * Cout as this conv); proj_y: NHWC [N, H/2, W/2, Cout] view (pitch proj_ldy); proj_scale / proj_shift NULL => 1 / 0.
     * H and W must be even, no split-K.  NULL = off. */
    const float *proj_w_packed; const float *proj_scale; const float *proj_shift;
    float *proj_y; int proj_ldy;
} ct_conv_desc;
int ct_conv2d(const ct_conv_desc *d, void *stream);
size_t ct_conv2d_workspace_bytes(const ct_conv_desc *d);

/* ---- the heads of the network, fused ------------------------------------------------------------------
 * Replaces the per-head nn.Sequential(conv3x3 64 -> 256 + bias, ReLU, conv1x1 256 -> c + bias) of BaseModel
 * (src/lib/model/networks/base_model.py:24-65,86-90) for every listed head, with Detector._sigmoid_output
 * (src/lib/detector.py:300-308) on the channels [sig_lo,sig_hi) / [dep_lo,dep_hi) of `out`, in ONE launch: the
 * 256-channel hidden maps (16.8 MB per head and frame at 512x512) stay inside the workgroups.  x: NHWC feature map
 * (64 channels, pitch ldx); w0_winograd: ct_pack_winograd_weight() of the heads' first-layer weights concatenated
 * along Cout ([nheads*256, 64, 3, 3]); b0 [nheads*256]; w2 [nheads][8][256] = the heads' 1x1 weights, rows >= cout[i]
 * zero; b2 [nheads][8]; head i writes channels coff[i] .. coff[i]+cout[i]-1 of out (NCHW [N, ctot, H, W]).  Heads
 * with more than 8 output channels (hm of an 80-class model, hps, hm_hp) go through ct_conv2d. */
#define CT_MAX_FUSED_HEADS 8
typedef struct ct_heads_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *w0_winograd; const float *b0;
    int nheads;
    const float *w2; const float *b2;
    int cout[CT_MAX_FUSED_HEADS], coff[CT_MAX_FUSED_HEADS];
    float *out; int ctot;
    int sig_lo, sig_hi, dep_lo, dep_hi; float depth_scale;
} ct_heads_desc;
int ct_heads_fused(const ct_heads_desc *d, void *stream);

/* ---- modulated deformable convolution v2 (3x3, stride 1, pad 1, dil 1, dg 1) -------
 * Replaces DCNv2's _ext.dcn_v2_forward (modulated_deformable_im2col + SGEMM; upstream
 * src/cuda/dcn_v2_cuda.cu, dcn_v2_im2col_cuda.cu) as called from DeformConv.forward,
 * dla.py:513-518, with the following BatchNorm + ReLU fused:
 *   y[p,co] = act( (sum_{k,ci} W[co,ci,k] * m_k(p) * bilinear(x[.,ci], p + tap_k + d_k(p)))
 *                  * scale[co] + shift[co] )      (DCN bias folded into shift by the caller)
 * `om` is the NHWC offset/mask map [N,H,W,>=27] (ld = ldom): channels 2k,2k+1 = (dy,dx)
 * of tap k, channel 18+k = mask AFTER sigmoid (produced by ct_conv2d with sig_lo=18). */
typedef struct ct_dcn_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *om; int ldom;
    const float *w_packed; int Cout;
    const float *scale; const float *shift;
    float *y; int ldy;
    int flags;                                  /* CT_RELU */
    float *workspace; size_t workspace_bytes;
    int split_k;
    int algo;                                   /* 0 = heuristic; 64 / 128 = 64-pixel tile x 64 / 128 couts per
                                                   workgroup; 3264 / 32128 = 32-pixel tile x 64 / 128 couts;
                                                   43264 / 432128 = the same stepping through 64 instead of 32
                                                   channels per barrier (Cin % 64 == 0);
                                                   53264 / 532128 / 63264 / 632128 = 3264 / 32128 / 43264 / 432128 as a
                                                   PERSISTENT launch: "dcn_slots" resident workgroups, each striding over
                                                   the pixel tiles of one (cout block, K split) column with the gathers,
                                                   weight loads and the next tile's sampling table running across tile
                                                   boundaries; needs fuse_offset != 1 and an even number of step units
                                                   per split; bit-identical to the non-persistent code */
    int fuse_offset;                            /* 1: compute DCN.conv_offset_mask (+ mask sigmoid) inside this launch
                                                   from w_off_packed [27,Cin,3,3 packed] / b_off [27]; `om` is then
                                                   unused (may be NULL); needs Cin % 64 == 0 and a 32-pixel tile.
                                                   2: the same conv K-split over Cin / 64 chunks by the CT_DCN_OFFSETS
                                                   launch (one workgroup per 32-pixel tile and chunk, whatever Cin) into
                                                   om_partial; the main launch sums the chunks (+ bias, mask sigmoid)
                                                   while it builds its sampling table; `om` unused.
                                                   3: om_partial holds ONE map of raw sums (no bias, no sigmoid; channel
                                                   pitch 32) written by any earlier launch -- e.g. ct_conv2d's Winograd
                                                   shapes, which have no sigmoid epilogue; the main launch adds b_off and
                                                   the mask sigmoid (w_off_packed is not read) */
    const float *w_off_packed; const float *b_off;
    /* optional fused IDAUp step (dla.py:543-545) for a `proj` DCN: when up_w != NULL the layer's result goes
     * through ct_upsample_add(result, up_w, up_f, up_skip) into up_y; with split-K the reduction kernel does
     * it directly from the partials (`y` is then never written), otherwise `y` holds the DCN output. */
    const float *up_w; int up_f; const float *up_skip; int up_lds; float *up_y; int up_ldy;
    float *om_partial; size_t om_partial_bytes; /* fuse_offset == 2: [Cin/64][N,H,W,32] floats, 3: [N,H,W,32] = ct_dcn_v2_offsets_bytes(d) */
    const float *w_off_winograd;                /* (ABI 103) fuse_offset == 2 only, optional: conv_offset_mask.weight packed by
                                                   ct_pack_winograd_weight.  The CT_DCN_OFFSETS launch then runs the K-split
                                                   offset/mask convs of ALL such layers of the group as ONE Winograd F(2x2,3x3)
                                                   launch (one workgroup per 64-pixel block and 64-channel chunk, 2.25x fewer
                                                   MFMAs than the direct form); same partial maps, same consumer */
} ct_dcn_desc;
int ct_dcn_v2(const ct_dcn_desc *d, void *stream);
size_t ct_dcn_v2_workspace_bytes(const ct_dcn_desc *d);
size_t ct_dcn_v2_offsets_bytes(const ct_dcn_desc *d);   /* 0 unless fuse_offset == 2 or 3 */
/* Up to 4 INDEPENDENT DeformConv layers in one launch (+ one reduce launch that finishes all of them): the IDAUp /
 * DLAUp tree (dla.py:539-574) has several layers ready at the same time -- every `proj_i` only needs a finished
 * level, `node_i` of different IDAUp stages do not depend on each other -- and at one stream each of them alone
 * cannot fill 256 CUs.  All layers run on the same 32-pixel tile shape (algo 0 / 3264 / 32128 / 43264 / 432128);
 * split_k == 0 gives every workgroup two 32-channel chunks (64 input channels), so the layers of a group finish
 * together whatever their Cin; fuse_offset is per layer; a fused IDAUp step (up_w) always goes through the
 * workspace (y is then not written).  Each layer needs its OWN workspace of ct_dcn_v2_group_workspace_bytes(d)
 * bytes (the layers run concurrently).  `phases`: CT_DCN_MAIN | CT_DCN_FINISH runs both launches back to back;
 * the two may also be issued separately, with different groupings -- the IDAUp step of a `proj` needs its skip
 * tensor (the previous node's output) only in the finishing launch, so the contraction can start before that
 * tensor exists.  Results are bit-identical to ct_dcn_v2 with the same split_k. */
enum { CT_DCN_MAIN = 1,      /* the gather + contraction launch (results or split-K partials) */
       CT_DCN_FINISH = 2,    /* the launch that finishes the layers holding partials: reduction + BN + ReLU (+ IDAUp step) */
       CT_DCN_OFFSETS = 4    /* the K-split offset/mask convs of the layers with fuse_offset == 2 (no-op for the others);
                                must precede CT_DCN_MAIN of the same layers */ };
int ct_dcn_v2_group(const ct_dcn_desc *descs, int n, int phases, void *stream);
size_t ct_dcn_v2_group_workspace_bytes(const ct_dcn_desc *d);
/* The same query with an error code: ct_dcn_v2_group_workspace_bytes returns 0 both for "no workspace needed" and for
 * a descriptor the launch would reject; this one validates the descriptor as a member of a group launch (workspace /
 * output pointers may still be NULL) and returns CT_OK with *workspace_bytes (0 = the layer finishes in its MAIN
 * launch) and *splits (K splits the launch will use), or the launch's error code (see ct_last_error). */
int ct_dcn_v2_group_plan(const ct_dcn_desc *d, size_t *workspace_bytes, int *splits);

/* ---- backward of the modulated deformable convolution (training through the drop-in DCN module) --------------
 * Replaces DCNv2's _ext.dcn_v2_backward (upstream src/cuda/dcn_v2_cuda.cu: modulated_deformable_col2im,
 * _col2im_coord and two SGEMMs over a [9*Cin, H*W] column buffer per image) for y = ct_dcn_v2(x, om, w) + bias with no
 * scale / ReLU, same geometry as the forward (3x3, stride 1, pad 1, dil 1, dg 1, Cin % 32 == 0), without a column
 * buffer.  The specification is torch.autograd of oracle/dcn_v2.py::dcn_v2_conv; at an integer sample position the
 * offset gradient is the one-sided derivative towards the next cell, as upstream's.
 *   x, gy, gx: NHWC views [N,H,W,Cin] / [N,H,W,Cout] / [N,H,W,Cin]; om / gom: the offset/mask map of the forward and
 *   its gradient, [N,H,W,>=27] (channels 2k, 2k+1 = d/d(dy,dx) of tap k, 18+k = d/d(mask AFTER the sigmoid); further
 *   channels of gom are not written); gw: OIHW [Cout,Cin,3,3]; gb: [Cout] or NULL.
 *   wT_packed: DCN.weight in the transposed fragment layout [tap][Cin/16][CoutPad/16][64 lanes][4] of
 *   ct_pack_dcn_weight_t -- lane l, element j = w[co = 16*cb + 4*(l>>4) + j][ci = 16*c16 + (l&15)][tap] -- the B operand
 *   of gcol = gy . W; needed for CT_DCN_BWD_INPUT / CT_DCN_BWD_OFFSET_MASK only.
 *   flags: which gradients to compute; buffers of the others may be NULL and are not touched.  CT_DCN_BWD_WEIGHT needs a
 *   workspace of ct_dcn_v2_backward_workspace_bytes(d) bytes (K-slab partials).  gx is zero-filled by the call and then
 *   accumulated with float atomics: it is NOT bitwise reproducible from run to run; gom, gw and gb are.
 *   Every view must stay below 2 GiB (N*H*W*ld*4): the kernels address a view through one buffer descriptor. */
#define CT_DCN_BWD_INPUT 1        /* gx */
#define CT_DCN_BWD_OFFSET_MASK 2  /* gom */
#define CT_DCN_BWD_WEIGHT 4       /* gw (+ gb when not NULL) */
typedef struct ct_dcn_bwd_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *om; int ldom;
    const float *gy; int Cout, ldgy;
    const float *wT_packed;
    float *gx; int ldgx;
    float *gom; int ldgom;
    float *gw; float *gb;
    float *workspace; size_t workspace_bytes;
    int flags;
} ct_dcn_bwd_desc;
int ct_dcn_v2_backward(const ct_dcn_bwd_desc *d, void *stream);
size_t ct_dcn_v2_backward_workspace_bytes(const ct_dcn_bwd_desc *d);   /* 0 without CT_DCN_BWD_WEIGHT or for a rejected descriptor */
size_t ct_packed_dcn_weight_t_elems(int Cout, int Cin);
int ct_pack_dcn_weight_t(const float *w_oihw, float *packed, int Cout, int Cin, void *stream);

/* ---- the training loss (GenericLoss, trainer.py:20-86 + model/losses.py), forward and backward (additions under ABI
 * 103).  Every head map is the RAW head output (logits), fp32 NCHW [B,C,H,W], contiguous; ind / cat are int64, masks and
 * targets fp32.  One call serves all heads of a stack; the number of launches does not depend on the head count
 * (forward 2, backward 3).  No host synchronisation, no atomics: every sum goes through per-workgroup partials that are
 * added in a fixed order, so losses and gradients are bitwise equal from run to run.
 *   kind                target            mask        ind     cat               loss
 *   CT_LOSS_FOCAL       [B,C,H,W]         [B,M]       [B,M]   [B,M] class       FastFocalLoss on clamp(sigmoid(x), 1e-4, 1-1e-4)
 *   CT_LOSS_L1          [B,M,C]           [B,M,C]     [B,M]   NULL              sum|x*mask - target*mask| / (sum(mask) + 1e-4)
 *   CT_LOSS_L1_DEPTH    [B,M,C]           [B,M,C]     [B,M]   NULL              the same on 1 / (sigmoid(x) + 1e-6) - 1
 *   CT_LOSS_BCE         [B,M,C]           [B,M,C]     [B,M]   NULL              sum(mask * bce_with_logits) / (sum(mask) + 1e-4)
 *   CT_LOSS_ROT (C = 8) [B,M,2] rotres    [B,M]       [B,M]   [B,M,2] rotbin    compute_rot_loss (losses.py:161-192)
 * A slot whose ind is outside [0, H*W) or (focal) whose cat is outside [0, C) reads and writes nothing and counts as a
 * slot with mask 0 (for CT_LOSS_ROT: mask 0 and rotbin 0) -- the reference raises there, which needs a host sync.
 * Backward: grad_loss[i] is the incoming gradient of loss[i] (a DEVICE pointer, e.g. weights[head] / num_stacks times
 * d(tot)); heads[i].grad receives d/d(logits) for the WHOLE map [B,C,H,W] (zero away from the slots for the slot
 * kinds) or is NULL to skip that head.  Slots of one image that name the same element are summed in ascending slot
 * order by the lowest of them, which does one plain store.
 * workspace: ct_generic_loss_workspace_bytes(d) bytes, the same for both calls (the backward does not need the forward's
 * contents). */
#define CT_LOSS_FOCAL 0
#define CT_LOSS_L1 1
#define CT_LOSS_L1_DEPTH 2
#define CT_LOSS_BCE 3
#define CT_LOSS_ROT 4
#define CT_LOSS_MAX_HEADS 16
#define CT_LOSS_MAX_SLOTS 8192    /* largest M of one head (hp_ind: max_objs * 17) */
typedef struct ct_loss_head {
    int kind;
    const float *logits; int C;
    const float *target;
    const float *mask;
    const long long *ind;
    const long long *cat;
    int M;
    float *grad;                  /* backward only */
} ct_loss_head;
typedef struct ct_loss_desc {
    int B, H, W;
    const ct_loss_head *heads; int nheads;      /* HOST array */
    float *loss;                  /* DEVICE [nheads], forward only */
    const float *grad_loss;       /* DEVICE [nheads], backward only */
    void *workspace; size_t workspace_bytes;
} ct_loss_desc;
int ct_generic_loss_forward(const ct_loss_desc *d, void *stream);
int ct_generic_loss_backward(const ct_loss_desc *d, void *stream);
size_t ct_generic_loss_workspace_bytes(const ct_loss_desc *d);   /* 0 for a rejected descriptor */

/* ---- backward of the heads (base_model.py:24-65: per head conv3x3 64 -> hc + bias, ReLU, conv1x1 hc -> c + bias); additions
 * under ABI 103.  The training forward is ct_conv2d twice (the un-fused heads plan: one 3x3 conv into an NHWC hidden map
 * `mid` [N,H,W,nheads*hc] with bias and ReLU, one 1x1 conv per head into NCHW logits).  Backward, all fp32, no atomics, every
 * result bitwise equal from run to run:
 *   1. ct_heads_tail_backward: logit gradients -> hidden gradient gmid (through the ReLU), gw2, gb2
 *   2. ct_conv2d_backward_weight(x = feature map, gy = gmid, ks = 3): gw0, gb0
 *   3. the input gradient is ct_conv2d(gmid, ct_pack_conv_weight(w0T), Cout = Cin of the heads, ks = 3) with
 *      w0T[ci][co][ky][kx] = w0[co][ci][2-ky][2-kx]: no new entry point.
 *
 * ct_conv2d_backward_weight: the weight (and bias) gradient of y = conv(x, w) + b, ks in {1, 3}, stride 1, pad ks / 2,
 * Cin % 16 == 0, any Cout -- a general convolution weight gradient, not a special of the heads.
 *   x: NHWC view [N,H,W,Cin] (pitch ldx); gy: NHWC view [N,H,W,Cout] (pitch ldgy), the gradient of y;
 *   gw: OIHW [Cout,Cin,ks,ks], the layout of nn.Conv2d.weight; gb: [Cout] or NULL (not computed).
 *   The contraction over K = N*H*W pixels runs on the fp32 MFMA in K slabs whose partial sums go to `workspace`
 *   (ct_conv2d_backward_weight_workspace_bytes(d) bytes; 0 for a rejected descriptor); a second launch adds the slabs in
 *   slab order.  Both views must stay below 2 GiB (N*H*W*ld*4): the kernel addresses a view through one buffer descriptor. */
typedef struct ct_conv_bwd_weight_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *gy; int Cout, ldgy;
    int ks, stride;                             /* stride must be 1 */
    float *gw; float *gb;
    float *workspace; size_t workspace_bytes;
} ct_conv_bwd_weight_desc;
int ct_conv2d_backward_weight(const ct_conv_bwd_weight_desc *d, void *stream);
size_t ct_conv2d_backward_weight_workspace_bytes(const ct_conv_bwd_weight_desc *d);
/* ct_heads_tail_backward: for nheads <= CT_LOSS_MAX_HEADS heads of any width c over one hidden map,
 *   gmid[p, i*hc + k] = mid[p, i*hc + k] > 0 ? sum_c w2[i][c][k] * gout[i][c][p] : 0     (CT_HEADS_BWD_HIDDEN)
 *   gw2[i][c][k] = sum_p gout[i][c][p] * mid[p, i*hc + k],  gb2[i][c] = sum_p gout[i][c][p]   (CT_HEADS_BWD_WEIGHT)
 *   gout: the head's logit gradient, NCHW [N,c,H,W] contiguous -- what ct_generic_loss_backward writes into
 *   ct_loss_head.grad; w2: [c,hc] = the 1x1 weight; mid: the hidden map AFTER the ReLU, NHWC view [N,H,W,nheads*hc] (pitch
 *   ldmid); gmid: NHWC view of the same shape (pitch ldgmid, which may differ; channels beyond nheads*hc are not
 *   written).  The ReLU convention is torch's: gradient 0 where the hidden value is exactly 0.
 *   flags select what is computed; buffers of the other part may be NULL and are not touched.  With CT_HEADS_BWD_WEIGHT a
 *   head whose gw2 and gb2 are both NULL is skipped, and either may be NULL on its own.  The sums over the pixels go through
 *   per-workgroup partials in `workspace` (ct_heads_tail_backward_workspace_bytes(d) bytes; 0 without CT_HEADS_BWD_WEIGHT
 *   or for a rejected descriptor; it does not depend on which gw2 / gb2 are given) that a second launch adds in a fixed
 *   order.  Every view is addressed with 64-bit offsets: no 2 GiB limit here, N*H*W < 2^31. */
#define CT_HEADS_BWD_HIDDEN 1     /* gmid */
#define CT_HEADS_BWD_WEIGHT 2     /* gw2 / gb2 of the heads that give a buffer */
typedef struct ct_heads_tail_head {
    const float *gout; int c;
    const float *w2;              /* CT_HEADS_BWD_HIDDEN only */
    float *gw2; float *gb2;       /* CT_HEADS_BWD_WEIGHT only; NULL = not computed */
} ct_heads_tail_head;
typedef struct ct_heads_tail_bwd_desc {
    int N, H, W, hc;
    const ct_heads_tail_head *heads; int nheads;      /* HOST array */
    const float *mid; int ldmid;
    float *gmid; int ldgmid;
    float *workspace; size_t workspace_bytes;
    int flags;
} ct_heads_tail_bwd_desc;
int ct_heads_tail_backward(const ct_heads_tail_bwd_desc *d, void *stream);
size_t ct_heads_tail_backward_workspace_bytes(const ct_heads_tail_bwd_desc *d);

/* ---- the heads at the object slots (training with slot heads); additions under ABI 103.  A head the loss
 * reads at batch['ind'] only is evaluated at those M cells per image: the im2col rows of the 3x3, pad 1 first layer are
 * gathered into a map [N,1,M,9*C] on which the head is two 1x1 convolutions -- ct_conv2d, ct_heads_tail_backward and
 * ct_conv2d_backward_weight with ks = 1 do all the arithmetic -- and the input gradient's patches are folded back.
 *   map:  NHWC view [N,H,W,C] at pitch ld (C % 4 == 0, ld % 4 == 0, 16-byte aligned)
 *   ind:  int64 [N,M], the cell y * W + x of a slot; a value outside [0, H*W) is an invalid slot
 *   rows: [N*M] rows of 9*C floats at pitch ldr (ldr % 4 == 0, 16-byte aligned), rows[n,m,ky*3+kx,c]
 * ct_slot_gather writes rows[n,m,tap,c] = map[n, y+ky-1, x+kx-1, c], 0 for a tap outside the map and a whole row of 0 for an
 * invalid slot; it writes nothing beyond the 9*C floats of a row.  A copy: exact.
 * ct_slot_fold adds rows into map, map[n, y+ky-1, x+kx-1, c] += rows[n,m,tap,c], without atomics.  Every touched cell has one
 * owner, the lowest valid slot whose 3x3 neighbourhood covers it; the owner takes the patch value of that slot, adds those of
 * the further covering slots in ascending slot order and stores map + sum once.  The float32 value of every cell is therefore
 * defined exactly and equal from run to run; duplicates (up to all M slots on one cell) are summed, invalid slots contribute
 * nothing, a cell no slot covers is not written.
 * Both return CT_ERR_ARG before any launch for a null descriptor or pointer, a non-positive shape, M outside [1, 8192], a pitch
 * below the channel count, a misaligned view, or a view of 2 GiB or more (N*H*W*ld*4, N*M*ldr*4). */
typedef struct ct_slot_desc {
    float *map; int N, H, W, C, ld;             /* read by ct_slot_gather, updated by ct_slot_fold */
    const long long *ind; int M;
    float *rows; int ldr;                       /* written by ct_slot_gather, read by ct_slot_fold */
} ct_slot_desc;
int ct_slot_gather(const ct_slot_desc *d, void *stream);
int ct_slot_fold(const ct_slot_desc *d, void *stream);

/* ---- the trainable neck (DeformConv / IDAUp / DLAUp, dla.py:506-574); additions under ABI 103.  All fp32 on NHWC views with
 * a channel pitch (ld >= C, C % 4 == 0, ld % 4 == 0, 16-byte aligned pointers, channel slices allowed).  No atomics: every sum
 * runs thread -> workgroup -> slab in a fixed order, slab counts depend on the shapes only, every result is bitwise equal from
 * run to run.  A view stays below 2 GiB (N*H*W*ld*4): the kernels address it with 32-bit offsets.
 *
 * ct_bn_desc serves three calls over one pre-activation map z [N,H,W,C]:
 *   ct_bn_stats:          mean[c], var[c] (biased, two passes: sum of z - z[pixel 0], then sum of squared deviations), invstd[c] = 1/sqrt(var + eps)
 *   ct_bn_relu_apply:     y = max(0, fma(z - mean, a, beta)), a = gamma * invstd
 *   ct_bn_relu_backward:  g = gy where the recomputed pre-activation is > 0, else 0 (torch's ReLU: 0 at exactly 0);
 *                         gbeta = sum g, ggamma = sum g * xhat, xhat = (z - mean) * invstd;
 *                         gz = a * (g - mean(g) - xhat * mean(g * xhat)) with CT_BN_BATCH_STATS, a * g without
 *   mean / invstd are what the forward used (batch or running statistics).  gz, ggamma, gbeta may each be NULL (not computed;
 *   a frozen gamma / beta still gives the batch-statistics gz).  ct_bn_stats and ct_bn_relu_backward need
 *   ct_bn_workspace_bytes(d) bytes of workspace (0 for a rejected descriptor); ct_bn_relu_apply needs none. */
#define CT_BN_BATCH_STATS 1
typedef struct ct_bn_desc {
    const float *z; int N, H, W, C, ldz;
    float *mean; float *var; float *invstd;     /* [C] each; var: ct_bn_stats only */
    float eps;                                  /* ct_bn_stats only */
    const float *gamma; const float *beta;      /* [C] */
    float *y; int ldy;                          /* ct_bn_relu_apply */
    const float *gy; int ldgy;                  /* ct_bn_relu_backward */
    float *gz; int ldgz;
    float *ggamma; float *gbeta;
    float *workspace; size_t workspace_bytes;
    int flags;
} ct_bn_desc;
int ct_bn_stats(const ct_bn_desc *d, void *stream);
int ct_bn_relu_apply(const ct_bn_desc *d, void *stream);
int ct_bn_relu_backward(const ct_bn_desc *d, void *stream);
size_t ct_bn_workspace_bytes(const ct_bn_desc *d);
/* ct_upsample_add_backward: the backward of ct_upsample_add for the output gradient gy [N,fH,fW,C] (H, W = the INPUT grid):
 *   gx[n,iy,ix,c] = sum_{ky,kx < 2f} gy[n, iy*f - f/2 + ky, ix*f - f/2 + kx, c] * w[ky,kx,c]     (w: ct_upsample_add's [2f,2f,C])
 *   gw[c,ky,kx]   = sum_{n,iy,ix} x[n,iy,ix,c] * gy[same index]            (gw: the module's [C,1,2f,2f] layout)
 *   gx / gw may be NULL (not computed; w is needed for gx, x for gw).  The gradient of the skip input is gy itself.  gw goes
 *   through per-slab partials in `workspace` (ct_upsample_add_backward_workspace_bytes(d) bytes; 0 for a rejected descriptor). */
typedef struct ct_upsample_bwd_desc {
    const float *gy; int N, H, W, C, ldgy;
    int f;
    const float *w;
    float *gx; int ldgx;
    const float *x; int ldx;
    float *gw;
    float *workspace; size_t workspace_bytes;
} ct_upsample_bwd_desc;
int ct_upsample_add_backward(const ct_upsample_bwd_desc *d, void *stream);
size_t ct_upsample_add_backward_workspace_bytes(const ct_upsample_bwd_desc *d);
/* g[p, 18 + j] *= m * (1 - m), m = om[p, 18 + j], j < 9: the sigmoid of the DCN mask channels, in place on the offset/mask
 * gradient of ct_dcn_v2_backward (om = the forward's map, mask after the sigmoid) */
int ct_dcn_mask_sigmoid_backward(float *g, int ldg, const float *om, int ldom, int N, int H, int W, void *stream);

/* ---- the trainable backbone (BasicBlock / Root / Tree / DLA, dla.py:38-66,154-316); additions under ABI 103.  All fp32 on NHWC
 * views with a channel pitch under the rules of the neck block above (C % 4 == 0, ld % 4 == 0, 16-byte aligned pointers, channel
 * slices allowed, a view below 2 GiB).  No atomics: every sum has a fixed order, slab counts depend on the shapes only, every
 * result is bitwise equal from run to run.  The unit of the backbone is conv (ks 1 | 3, stride 1 | 2, no bias) -> BatchNorm
 * (-> + residual) (-> ReLU); its forward is ct_conv2d + ct_bn_stats + ct_bn_act_apply, its backward ct_bn_act_backward, then
 * ct_conv2d_backward_weight and a ct_conv2d with the transposed, flipped weight (stride 1) or ct_conv2d_s2_backward (stride 2).
 *
 * ct_conv2d_s2_backward: the gradients of y = conv3x3(x, w, stride 2, pad 1), H and W even, Cin % 16 == 0, Cout % 16 == 0.
 *   x: [N,H,W,Cin] (needed for gw); gy: [N,H/2,W/2,Cout]; gx: [N,H,W,Cin] or NULL; gw: OIHW [Cout,Cin,3,3] or NULL.
 *   gx[n,iy,ix,ci] = sum gy[n,oy,ox,co] * w[co,ci,ky,kx] over iy + 1 - ky = 2 oy, ix + 1 - kx = 2 ox -- on the fp32 MFMA at the
 *     forward's flop count: cell (cy,cx) of the output grid owns the input pixels (2cy+a, 2cx+b), which read gy at (cy..cy+1,
 *     cx..cx+1) only; per axis a = 0 meets tap 1 at cy, a = 1 tap 2 at cy and tap 0 at cy + 1, so the nine taps appear once per
 *     cell; gy outside the map counts as zero.  Needs w_s2t = ct_pack_conv_weight_s2t(w): [tap][Cout/4][Cin/16][64 lanes],
 *     lane l = w[co = 4*k4 + (l>>4)][ci = 16*c16 + (l&15)][tap] (ct_packed_conv_weight_s2t_elems(Cout, Cin) = 9*Cout*Cin floats).
 *   gw[co,ci,ky,kx] = sum_{n,oy,ox} gy[n,oy,ox,co] * x[n,2oy-1+ky,2ox-1+kx,ci] (zero outside the image): K = N*(H/2)*(W/2) in
 *     slabs to `workspace` (ct_conv2d_s2_backward_workspace_bytes(d) bytes, 0 for a rejected descriptor; not needed for gx
 *     alone), a second launch adds the slabs in slab order.
 *   flags: reserved, 0. */
typedef struct ct_conv_s2_bwd_desc {
    const float *x; int N, H, W, Cin, ldx;
    const float *gy; int Cout, ldgy;
    const float *w_s2t;
    float *gx; int ldgx;
    float *gw;
    float *workspace; size_t workspace_bytes;
    int flags;
} ct_conv_s2_bwd_desc;
int ct_conv2d_s2_backward(const ct_conv_s2_bwd_desc *d, void *stream);
size_t ct_conv2d_s2_backward_workspace_bytes(const ct_conv_s2_bwd_desc *d);
size_t ct_packed_conv_weight_s2t_elems(int Cout, int Cin);   /* 0 unless Cout % 16 == 0 and Cin % 16 == 0 */
int ct_pack_conv_weight_s2t(const float *w_oihw, float *packed, int Cout, int Cin, void *stream);
/* ct_bn_act_desc = ct_bn_desc plus an optional residual and an optional ReLU, over one pre-activation map z [N,H,W,C]:
 *   ct_bn_act_apply:     t = fma(z - mean, a, beta), a = gamma * invstd (ct_bn_relu_apply's); y = t + res when
 *                        res != NULL; y = max(0, y) with CT_BN_ACT_RELU
 *   ct_bn_act_backward:  g = gy where the recomputed y is > 0, else 0 (torch's ReLU: 0 at exactly 0), or g = gy without the
 *                        ReLU; gres = g; gbeta, ggamma, gz from g as in ct_bn_relu_backward (CT_BN_BATCH_STATS: through the
 *                        batch statistics).  gz, gres, ggamma, gbeta may each be NULL (not computed).
 *   mean / invstd are what the forward used (ct_bn_stats on a ct_bn_desc of the same map, or the running statistics).  With the
 *   ReLU and no residual these are ct_bn_relu_apply / _backward (which widen their ct_bn_desc and run the same code).  The backward needs
 *   ct_bn_act_workspace_bytes(d) bytes (0 for a rejected descriptor) whenever it sums: for ggamma, gbeta or a batch-statistics
 *   gz.  var and eps are not read. */
#define CT_BN_ACT_RELU 2
typedef struct ct_bn_act_desc {
    const float *z; int N, H, W, C, ldz;
    float *mean; float *var; float *invstd;
    float eps;
    const float *gamma; const float *beta;
    float *y; int ldy;
    const float *gy; int ldgy;
    float *gz; int ldgz;
    float *ggamma; float *gbeta;
    float *workspace; size_t workspace_bytes;
    int flags;                                  /* CT_BN_BATCH_STATS | CT_BN_ACT_RELU */
    const float *res; int ldr;                  /* residual added behind the affine map, or NULL */
    float *gres; int ldgres;                    /* its gradient (backward), or NULL */
} ct_bn_act_desc;
int ct_bn_act_apply(const ct_bn_act_desc *d, void *stream);
int ct_bn_act_backward(const ct_bn_act_desc *d, void *stream);
size_t ct_bn_act_workspace_bytes(const ct_bn_act_desc *d);
/* Synchronised BatchNorm (statistics over the batches of all ranks of a data-parallel job); additions under ABI 103.
 * ct_bn_stats_row: ct_bn_stats of the map of `d` (d->mean and d->var are not read; invstd, eps and the workspace as there),
 *   written as the row a merge takes, 3 C + 4 floats, 16-byte aligned:
 *     [ mean[C] | var[C] (biased) | resid[C] | P, P ]
 *   mean, var and invstd have the bits of ct_bn_stats; mean + resid is the mean before its rounding to float; P = N*H*W as a
 *   64-bit integer, stored twice (the row is a multiple of 16 bytes with every byte defined: a gather moves bytes).
 * ct_bn_merge_stats: `world` such rows on the device, row r at rows + r * ld floats, one per rank in rank order (ld >= 3 C + 2,
 *   even; rows 8-byte aligned).  Per channel, in double, the rows added in row order, each result rounded to float once:
 *     m_r = mean_r + resid_r;  v_r = var_r - resid_r^2  (the variance about the rounded mean, taken to the true one)
 *     N = sum P_r;  mean = sum P_r m_r / N;  var = (sum P_r v_r + sum P_r (m_r - mean)^2) / N
 *     invstd = 1 / sqrt(var + eps) from the rounded var, as ct_bn_stats forms it;
 *     unbiased = var N / (N - 1);  *inv_count = 1 / N;  *count = N (count may be NULL)
 *   The counts live on the device, so the host cannot check them: N >= 2 with every P_r >= 1 is the CALLER's contract (N = 1
 *   leaves Inf or NaN in unbiased, N <= 0 in everything).  A non-finite mean_r or var_r makes that channel's results
 *   non-finite, as ct_bn_stats on the whole batch would; only a negative rounding residue of var is clamped to 0.
 *     beta_shifted = fma(-gamma * invstd, mean - float(mean), beta)  (with gamma, beta, beta_shifted given): the kernels behind
 *       the merge form fma(z - mean, a, beta) with the FLOAT mean; handed beta_shifted in the place of beta, forward and
 *       backward alike, they compute a (z - mean_in_double) + beta.  gbeta and ggamma are not affected.
 *   world == 1 hands the row's mean and var back bit for bit (resid is not applied) and beta_shifted = beta.  The same rows give the same bits on
 *   every rank and in every run.
 * ct_bn_act_backward_apply / ct_bn_relu_backward_apply: the second half of ct_bn_act_backward / ct_bn_relu_backward under
 *   CT_BN_BATCH_STATS.  The first half is that call with gz = gres = NULL: it leaves sum g in gbeta and sum g * xhat in ggamma.
 *   sums = [ sum g [C] | sum g * xhat [C] ] (16-byte aligned) and *inv_count are device memory of the caller: with sums added
 *   over the ranks and inv_count from ct_bn_merge_stats,
 *     gz = a * (g - inv_count * sum g - xhat * inv_count * sum g * xhat);  gres = g
 *   No workspace; ggamma, gbeta, var, eps are not read. */
typedef struct ct_bn_merge_desc {
    const float *rows; int world, C, ld;
    float eps;
    float *mean; float *var; float *invstd; float *unbiased;   /* [C] each */
    float *inv_count;                                          /* [1] */
    long long *count;                                          /* [1] or NULL */
    const float *gamma; const float *beta;                     /* [C] each, with beta_shifted; or all three NULL */
    float *beta_shifted;                                       /* [C]: beta - gamma * invstd * (mean - float(mean)) */
} ct_bn_merge_desc;
int ct_bn_stats_row(const ct_bn_desc *d, float *row, void *stream);
int ct_bn_merge_stats(const ct_bn_merge_desc *d, void *stream);
int ct_bn_act_backward_apply(const ct_bn_act_desc *d, const float *sums, const float *inv_count, void *stream);
int ct_bn_relu_backward_apply(const ct_bn_desc *d, const float *sums, const float *inv_count, void *stream);
/* ct_maxpool2x2_backward: the backward of ct_maxpool2x2 (H, W = the INPUT grid, even).  x: the pool's input [N,H,W,C]; gy:
 *   [N,H/2,W/2,C]; gx [N,H,W,C]: each window's gradient goes to its first maximum in row-major order (torch's rule: a window of
 *   equal values sends it to the top-left, -0.0 ties with 0, a NaN wins), the other three elements get 0; `add` (a view of the
 *   shape of gx, or NULL) is summed in -- a Tree's input gradient is the stride-2 conv's gx plus the pool's.  Every gx element
 *   is written exactly once. */
int ct_maxpool2x2_backward(const float *x, int N, int H, int W, int C, int ldx, const float *gy, int ldgy,
                           const float *add, int ldadd, float *gx, int ldgx, void *stream);

/* ---- the trainable 7x7 stems (base_layer / pre_img_layer / pre_hm_layer, dla.py:238-267,305-311); additions under ABI 103.
 * Specialised to Cout = 16 and Cin = 3, 3, 1 (index s = 0 image, 1 previous image, 2 prior heat-map).  Inputs and image
 * gradients are the reference's contiguous NCHW planes, weights and weight gradients OIHW [16,Cin,7,7]; every 16-channel map is
 * an NHWC view with a pitch under the rules of the neck block above (ld >= 16, ld % 4 == 0, 16-byte aligned pointers, a view
 * below 2 GiB).  All fp32, no atomics, every sum in a fixed order, slab counts from the shapes only: bitwise equal from run to
 * run.  The forward of a training step is ct_stem_conv_forward, ct_bn_stats per stem, ct_stem_bn_relu_sum; since y is a plain
 * sum, each stem's output gradient is gy itself: the backward is ct_bn_relu_backward(z_s, gy) per stem, then
 * ct_stem_conv_backward.
 *
 * ct_stem_conv_forward: for every s with in[s] != NULL (in[0] must be given): z[s] = conv7x7(in[s], w[s]), pad 3, no bias -- the
 *   raw convolution output that training-mode BatchNorm needs -- on the fp32 MFMA, one launch for all stems present.
 * ct_stem_conv_backward: for every s, from gz[s] (the gradient of z[s]):
 *   gw[s][co,ci,ky,kx] = sum_{n,y,x} gz[s][n,y,x,co] * in[s][n,ci,y+ky-3,x+kx-3] (zero outside the image) when gw[s] != NULL: on
 *     the fp32 MFMA, partial sums in slabs of `workspace` (ct_stem_conv_backward_workspace_bytes(d) bytes, 0 for a rejected
 *     descriptor or when no gw is asked for), a second launch adds the slabs in slab order; one pair of launches for all stems;
 *   gin[s][n,ci,y,x] = sum_{ky,kx,co} gz[s][n,y-ky+3,x-kx+3,co] * w[s][co,ci,ky,kx] when gin[s] != NULL (needs w[s], not in[s]).
 *   Nothing is read, written or launched for an output that is NULL; at least one must be asked for.
 * ct_stem_bn_relu_sum: y = sum_s max(0, fma(z[s] - mean[s], a, beta[s])), a = gamma[s] * invstd[s], over the stems with
 *   z[s] != NULL (z[0] must be given), added in the order 0, 1, 2; each term has the bits of ct_bn_relu_apply. */
typedef struct ct_stem_conv_desc {
    int N, H, W;
    const float *in[3];                         /* [N,Cin,H,W]; forward, gw */
    const float *w[3];                          /* [16,Cin,7,7]; forward, gin */
    float *z[3]; int ldz[3];                    /* forward: the outputs [N,H,W,16] */
    const float *gz[3]; int ldgz[3];            /* backward: the gradients of z */
    float *gw[3];                               /* backward: [16,Cin,7,7] or NULL */
    float *gin[3];                              /* backward: [N,Cin,H,W] or NULL */
    float *workspace; size_t workspace_bytes;   /* backward with a gw */
} ct_stem_conv_desc;
int ct_stem_conv_forward(const ct_stem_conv_desc *d, void *stream);
int ct_stem_conv_backward(const ct_stem_conv_desc *d, void *stream);
size_t ct_stem_conv_backward_workspace_bytes(const ct_stem_conv_desc *d);
typedef struct ct_stem_sum_desc {
    int N, H, W;
    const float *z[3]; int ldz[3];
    const float *mean[3]; const float *invstd[3]; const float *gamma[3]; const float *beta[3];     /* [16] each, 16-byte aligned */
    float *y; int ldy;
} ct_stem_sum_desc;
int ct_stem_bn_relu_sum(const ct_stem_sum_desc *d, void *stream);

/* ---- the three 7x7 stems, fused --------------------------------------------------
 * Replaces DLA.forward's base_layer / pre_img_layer / pre_hm_layer and their sum
 * (dla.py:238-267,305-311): y = sum_s relu(bn_s(conv7x7_s(in_s))), inputs NCHW
 * ([N,3,H,W], [N,3,H,W] or NULL, [N,1,H,W] or NULL), output NHWC [N,H,W,16] (ld = ldy).
 * w_s: OIHW [16,Cin_s,7,7]; scale_s/shift_s: folded BN [16]. */
int ct_stem_forward(const float *x, const float *pre_img, const float *pre_hm, int N, int H, int W,
                    const float *w_x, const float *w_img, const float *w_hm,
                    const float *scale3, const float *shift3,   /* [3][16] each */
                    float *y, int ldy, void *stream);
/* The same with any subset of the three stems (a NULL input skips its stem), accumulated on top of `add` (NHWC, 16
 * channels, pitch ldadd; NULL = 0).  The terms are added in the order x, pre_img, pre_hm, so a launch of {x, pre_img}
 * into a partial map followed by a launch of {pre_hm} with add = that map is bit-identical to ct_stem_forward: the
 * detector runs the first for frame t+1 -- those two terms do not depend on the tracker (dla.py:305-311) -- while
 * the host still associates frame t. */
int ct_stem_forward_parts(const float *x, const float *pre_img, const float *pre_hm, const float *add, int ldadd,
                          int N, int H, int W, const float *w_x, const float *w_img, const float *w_hm,
                          const float *scale3, const float *shift3, float *y, int ldy, void *stream);

/* ---- glue ops ---------------------------------------------------------------------- */
/* nn.MaxPool2d(2,2) of Tree.downsample (dla.py:207-208,216), NHWC views */
int ct_maxpool2x2(const float *x, int N, int H, int W, int C, int ldx, float *y, int ldy, void *stream);
/* IDAUp step `up(proj) + skip` (dla.py:529-532,543-545): depth-wise ConvTranspose2d
 * (kernel 2f, stride f, padding f/2, groups=C, no bias) of x [N,H,W,C] plus skip [N,fH,fW,C]
 * -> y [N,fH,fW,C].  w = the module's weight [C,1,2f,2f] transposed once to [2f,2f,C]. */
int ct_upsample_add(const float *x, int N, int H, int W, int C, int ldx, const float *w, int f,
                    const float *skip, int lds, float *y, int ldy, void *stream);
/* layout converters for the NCHW drop-in ops */
int ct_nchw_to_nhwc(const float *x, int N, int C, int H, int W, float *y, int ldy, void *stream);
int ct_nhwc_to_nchw(const float *x, int N, int C, int H, int W, int ldx, float *y, void *stream);

/* ---- heat-map decode ----------------------------------------------------------------
 * Replaces generic_decode (src/lib/model/decode.py:83-182, non-pose heads) with its
 * helpers _nms / _topk / _tranpose_and_gather_feat (src/lib/model/utils.py:16-87):
 * 3x3 max-pool pseudo-NMS, exact top-K over all classes/pixels (ties: lower class, then
 * lower pixel index first), gathers of every regression head, box assembly, into ONE
 * packed buffer (replaces the 8-14 D2H copies of detector.py:349-350).
 * hm: NCHW [B,C,h,w] post-sigmoid.  heads[i]: NCHW [B,head_ch[i],h,w] or NULL.
 * Head order / packed layout: see ct_decode_layout(). */
enum { CT_HEAD_REG = 0, CT_HEAD_WH, CT_HEAD_TRACKING, CT_HEAD_LTRB, CT_HEAD_LTRB_AMODAL,
       CT_HEAD_DEP, CT_HEAD_ROT, CT_HEAD_DIM, CT_HEAD_AMODEL_OFFSET, CT_HEAD_NUSCENES_ATT,
       CT_HEAD_VELOCITY, CT_NUM_HEADS };
/* Sparse heads (round 5, opt-in; no reference equivalent -- the reference computes every head as a dense map,
 * base_model.py:86-90, and then reads it at K pixels, decode.py:99-180): the regression heads listed here are evaluated
 * at the K winners of every image only, after the selection, and the packed rows are assembled from those values; their
 * entries in ct_decode_desc.heads must be NULL.  feat: DEVICE NHWC view of the 64-channel feature map the heads read
 * (dla.py:631-640), image 0, channel pitch ldf (16-byte aligned, >= 64), images h * w * ldf floats apart.  Per head:
 * head[i] = CT_HEAD_* id; w1 = conv3x3 64 -> 256 weights in ct_pack_conv_weight layout, b1 [256]; w2 = conv1x1 weights
 * [c][256] row-major, b2 [c].  The dep head gets the dense epilogue's transform (1 / (sigmoid(v) + 1e-6) - 1) *
 * depth_scale (detector.py:305-307); zero_tracking != 0 zeroes the tracking output (decode.py:95-96).  Two launches behind
 * the selection: the heads' partial products at the winners, then the rows (+ host copy + end-of-frame flag).
 * The workspace of ct_decode is scratch from end to end, with or without sparse heads: candidate slots, winner keys [B][K]
 * and the partials are each written by the call before it reads them, so the caller need not clear any byte of it.  The
 * one thing that must be zero before the first launch is *done_counter, which is not part of the workspace. */
typedef struct ct_sparse_heads_desc {
    const float *feat; int ldf;
    int nheads;
    int head[CT_NUM_HEADS];
    const float *w1[CT_NUM_HEADS], *b1[CT_NUM_HEADS], *w2[CT_NUM_HEADS], *b2[CT_NUM_HEADS];
    float depth_scale;
    int zero_tracking;
    /* flip_test (detector.py:311-332): flip_B = B when feat holds 2 * B images (image B + b = the mirrored frame of stream
     * b), else 0; flip_mode[i]: 0 = the head is read from image b alone (reg, tracking, ltrb*, rot, ...), 1 = averaged
     * with the mirrored image's value at the mirrored pixel (wh, dep, dim), 2 = the same with the even (x) channels of the
     * mirrored value negated (amodel_offset) */
    int flip_B;
    int flip_mode[CT_NUM_HEADS];
} ct_sparse_heads_desc;
typedef struct ct_decode_desc {
    const float *hm; int B, C, h, w, K;
    const float *heads[CT_NUM_HEADS];
    float *out;                /* [B,K,F] floats, F = ct_decode_row_floats(heads present) */
    int64_t *inds;             /* [B,K] flat pixel indices (may be NULL) */
    void *workspace; size_t workspace_bytes;
    /* floats between consecutive images of hm / of each head map; 0 = densely packed ([B,c,h,w] contiguous).
     * Lets the head maps be channel slices of one wider NCHW tensor (all heads written by one conv launch). */
    size_t hm_batch_stride; size_t head_batch_stride[CT_NUM_HEADS];
    int out_stride;            /* floats between consecutive rows of out; 0 = F (lets a wider row carry the pose fields) */
    /* optional (round 3): the same rows ALSO stored straight into pinned HOST memory (same pitch), and *done_flag (pinned
     * HOST int) set to 1 with system-scope release once every image's rows are there -- the frame graph then needs
     * neither a D2H copy node nor a separate flag kernel behind the decode.  done_counter: DEVICE unsigned, zero before
     * the first launch (the last workgroup resets it).  All three NULL: device rows only. */
    float *host_out; int *done_flag; unsigned *done_counter;
    const ct_sparse_heads_desc *sparse;    /* HOST pointer, NULL = every head is a dense map (ABI 102) */
} ct_decode_desc;
/* row layout: score, cls, xs0, ys0, then for each present field in this order:
 * bbox[4] (if wh|ltrb|ltrb_amodal), bbox_amodal[4] (if ltrb_amodal), tracking[2], dep[1],
 * rot[8], dim[3], amodel_offset[2], nuscenes_att[8], velocity[3] */
int ct_decode_row_floats(const ct_decode_desc *d);
size_t ct_decode_workspace_bytes(const ct_decode_desc *d);
int ct_decode(const ct_decode_desc *d, void *stream);

/* ---- pose branch of the decode ------------------------------------
 * Replaces the `'hps' in output` branch of generic_decode (src/lib/model/decode.py:161-171) with
 * _update_kps_with_hm (decode.py:11-81) and _topk_channel (src/lib/model/utils.py:60-69).  Runs after ct_decode on
 * the same frame: rows / inds are ct_decode's outputs (row pitch row_floats).  The box a snapped joint must lie in
 * (decode.py:45-57) is generic_decode's LOCAL `bboxes` -- the wh box, overridden by the ltrb box (decode.py:123,137),
 * never the ltrb_amodal box (that one only replaces ret['bboxes'], decode.py:159):
 *   box_col >= 4  column of that box in a packed row (rows of a model without an ltrb_amodal head);
 *   box_col == -1 the rows do not hold it (their box columns carry the amodal box, or there is none): it is rebuilt
 *                 from the heads box_ltrb [B,4,h,w], else box_wh [B,2,h,w] (+ box_reg [B,2,h,w], NULL = +0.5), with
 *                 ct_decode's own expressions; all three NULL = the box-less variant (decode.py:60-71): the box is the
 *                 extent of the detection's regressed joints widened by 25 % per side (r and b grow from the already
 *                 widened l and t, as in the reference).
 * hps: NCHW [B,2J,h,w]; hm_hp: NCHW
 * [B,J,h,w] post-sigmoid, densely packed; hp_offset: NCHW [B,2,h,w] (the hp_offset head, else the reg
 * head, else NULL = +0.5).  out: [B,K,2J+1] = refined key points (x0,y0,x1,y1,...) then kps_score
 * (with out_stride it may point into the packed rows themselves: one buffer, one D2H).
 * Peaks of hm_hp with exactly equal scores rank lower pixel first (torch.topk: unspecified). */
typedef struct ct_pose_desc {
    const float *rows; int row_floats, box_col;
    const int64_t *inds;
    int B, h, w, K, num_joints;
    const float *hps, *hm_hp, *hp_offset;
    size_t hps_batch_stride, hm_hp_batch_stride, hp_offset_batch_stride;   /* floats between images; 0 = dense */
    float *out; int out_stride;            /* floats between consecutive rows of out; 0 = 2J+1 */
    void *workspace; size_t workspace_bytes;
    const float *box_wh, *box_reg, *box_ltrb;                              /* box_col == -1, see above */
    size_t box_wh_batch_stride, box_reg_batch_stride, box_ltrb_batch_stride;   /* floats between images; 0 = dense */
} ct_pose_desc;
size_t ct_decode_pose_workspace_bytes(const ct_pose_desc *d);
int ct_decode_pose(const ct_pose_desc *d, void *stream);
/* Sparse pose heads (opt-in; no reference equivalent): ct_decode_pose without the hps and offset maps.  The reference reads
 * hps at the K winners (decode.py:161-167) and the offset head at the K peaks of every joint map (decode.py:21-28); here
 * both heads are evaluated at exactly those pixels from their weights -- conv3x3 64 -> 256 (zero padding) + bias + ReLU +
 * conv1x1 + bias over feat, the NHWC feature map of ct_sparse_heads_desc (same feat / ldf / flip_B semantics).
 * base: as for ct_decode_pose, with hps and hp_offset NULL; hm_hp stays a dense map (the merged one when flip_B > 0) and
 * the gate box comes from the rows (box_col) or the box maps as before.
 * hps_*: w1 in ct_pack_conv_weight layout [256,64,3,3], b1 [256], w2 [2J][256] row-major, b2 [2J].  off_*: the hp_offset
 * head (else the reg head) likewise with w2 [2][256]; all four NULL = no offset head (+0.5).
 * flip_B > 0: hps is also evaluated in image flip_B + b at the mirrored pixel (y, w-1-x) and merged like ct_flip_merge's
 * CT_FLIP_JOINT_OFFSETS with the HOST joint pairs flip_pairs [num_pairs][2]; the offset head reads image b alone.
 * 1 <= num_joints <= 32.  Launches: the joint decode, the point evaluation, its reduction, match, score -- all on `stream`,
 * no host wait, bitwise reproducible.  Every argument error returns before the first launch.
 * The workspace begins with the values the match read: merged hps [B,K,2J] floats (before the centre is added), then at
 * the next multiple of 256 bytes the offsets [B*J,K,2] (undefined without an offset head: never written, never read).
 * Like ct_decode's, the workspace is scratch from end to end: no byte of it has to be cleared by the caller. */
typedef struct ct_pose_sparse_desc {
    ct_pose_desc base;
    const float *feat; int ldf; int flip_B;
    const float *hps_w1, *hps_b1, *hps_w2, *hps_b2;
    const float *off_w1, *off_b1, *off_w2, *off_b2;
    const int *flip_pairs; int num_pairs;
} ct_pose_sparse_desc;
int ct_decode_pose_sparse_workspace_bytes(const ct_pose_sparse_desc *d, size_t *bytes);
int ct_decode_pose_sparse(const ct_pose_sparse_desc *d, void *stream);

/* ---- prior heat-map rendering on device ------------------------------------------------
 * Replaces the numpy Gaussian splatting + full-map H2D of Detector._get_additional_inputs
 * (src/lib/detector.py:254-290; draw_umich_gaussian / gaussian2D, src/lib/utils/image.py:
 * 130-154): out[b,0,y,x] = max over the stream's blobs (cx, cy, r) with |x-cx|<=r, |y-cy|<=r
 * of float32(exp(-(dx^2+dy^2) / (2*((2r+1)/6)^2))) (evaluated in float64 like numpy).
 * params: device int32 [B][cap][3]; counts: device int32 [B]; out: [B(*2),1,H,W] fp32; with
 * also_flipped the W-mirrored map of stream b is written to out[B+b] (flip_test). */
int ct_render_pre_hm(const int *params, const int *counts, int cap, int B, int H, int W, float *out,
                     int also_flipped, void *stream);

/* ---- flip_test on the device ------------------------------------------------------------
 * Replaces Detector._flip_output (src/lib/detector.py:311-332) with flip_tensor / flip_lr / flip_lr_off
 * (src/lib/model/utils.py:28-50) and the `np.concatenate((images, images[:, :, :, ::-1]))` of
 * Detector.pre_process (detector.py:224-226) for B streams: the network runs on [B originals ; B mirrored images].
 * ct_flip_merge: for every listed head  dst[b,c,y,x] = (src[b,c,y,x] + sgn(c) * src[B+b, perm(c), y, w-1-x]) / 2
 * (bit-identical to the reference's fp32 add + divide).  Heads the reference takes from image 0 alone (reg,
 * tracking, ltrb, ltrb_amodal, rot, nuscenes_att, velocity, hp_offset) are not listed: read the first B images.
 * src: NCHW maps of the 2B images, each image's [C,h,w] block dense, src_batch_stride floats between images;
 * dst: dense [B,C,h,w].  flip_idx: HOST int32 [npairs][2] left/right joint pairs (dataset.flip_idx; NULL / 0 when
 * no pose head is listed).  At most 8 heads per call. */
enum { CT_FLIP_AVG = 0,            /* hm, wh, dep, dim */
       CT_FLIP_NEG_EVEN = 1,       /* amodel_offset: mirrored x offsets change sign */
       CT_FLIP_JOINTS = 2,         /* hm_hp [J]: partner joint's map (flip_lr) */
       CT_FLIP_JOINT_OFFSETS = 3   /* hps [2J]: partner joint's (x, y), x negated (flip_lr_off) */ };
typedef struct ct_flip_head {
    const float *src; float *dst;
    size_t src_batch_stride;
    int C, mode;
} ct_flip_head;
int ct_flip_merge(const ct_flip_head *heads, int nheads, const int *flip_idx, int npairs, int B, int h, int w,
                  void *stream);
/* dst[r, x] = src[r, W-1-x] for `rows` rows of W floats (the mirrored input batch: rows = B*3*H) */
int ct_flip_images(const float *src, float *dst, size_t rows, int W, void *stream);

/* ---- host side of a frame (CPU, no device work) ----------------------------------------
 * Replaces generic_post_process (src/lib/utils/post_process.py:21-91), Detector.merge_outputs
 * (src/lib/detector.py:371-377) and Tracker.step with greedy_assignment
 * (src/lib/utils/tracker.py:28-138, private detections) for the packed rows of ct_decode, and
 * the per-track part of Detector._get_additional_inputs (detector.py:254-290). */
typedef struct ct_row_layout {      /* float offsets inside one packed row; -1 = field absent */
    int score, cls, cts, tracking, bbox, amodel_offset;
} ct_row_layout;
typedef struct ct_track {
    float score; int cls;           /* class is 1-based like the reference's item['class'] */
    float ct[2], tracking[2], bbox[4];
    int tracking_id, age, active;
    int row;                        /* source row in the packed decode buffer (-1: carried-over track) */
} ct_track;
void *ct_tracker_create(float new_thresh, int max_age);
void ct_tracker_destroy(void *tracker);
void ct_tracker_reset(void *tracker);
int ct_tracker_num_tracks(void *tracker);
int ct_tracker_id_count(void *tracker);
int ct_tracker_get_tracks(void *tracker, ct_track *out, int cap);
/* rows: HOST pointer [K,F]; trans_inv: float32 [2,3] output-grid -> image affine; returns the number of tracks
 * after the step (the reference's list is unbounded: with max_age > 0 unmatched tracks accumulate) or -1; at most
 * cap of them are written to out -- a caller that gets n > cap grows its buffer and reads ct_tracker_get_tracks */
int ct_tracker_step(void *tracker, const float *rows, int K, int F, const ct_row_layout *lay, float out_thresh,
                    const float *trans_inv, ct_track *out, int cap);
/* Remaining branches of the reference's Tracker (src/lib/utils/tracker.py): hungarian != 0 = optimal assignment
 * instead of greedy (:52-55,63-73, through ct_linear_assignment), public_det != 0 = new tracks only where one of
 * the frame's provided detections supports them (:83-101); ct_tracker_init_tracks = init_track (:13-26: items with
 * score > new_thresh start tracks; score, cls, ct, bbox are read); ct_tracker_step_public = ct_tracker_step with the
 * frame's public detection centres (float32 [n_public,2], image coordinates; NULL / 0 otherwise);
 * ct_tracker_step_dets = Tracker.step on detections that are already in image space (score, cls, ct, tracking, bbox). */
int ct_tracker_set_mode(void *tracker, int hungarian, int public_det);
int ct_tracker_init_tracks(void *tracker, const ct_track *items, int n);
int ct_tracker_step_public(void *tracker, const float *rows, int K, int F, const ct_row_layout *lay, float out_thresh,
                           const float *trans_inv, const float *public_cts, int n_public, ct_track *out, int cap);
int ct_tracker_step_dets(void *tracker, const ct_track *dets, int n, const float *public_cts, int n_public,
                         ct_track *out, int cap);
/* Key points of the pose task (`hps`, src/lib/utils/post_process.py:51-54): n (x, y) pairs on the output grid ->
 * image coordinates with the same float32 [2,3] affine and operation order as the boxes / centres of
 * ct_tracker_step (transform_preds_with_trans, src/lib/utils/image.py:20-26); returns n or -1. */
int ct_transform_points(const float *trans_inv, const float *xy, int n, float *out);
/* (cx, cy, radius) int32 triples of the next frame's prior heat-map; trans_input float64 [2,3] */
int ct_tracker_prehm_params(void *tracker, float pre_thresh, const double *trans_input, int inp_w, int inp_h,
                            int *params, int cap);

/* Minimum-cost assignment of an nr x nc float64 cost matrix (row-major): what the reference's --hungarian branch
 * gets from linear_assignment (src/lib/utils/tracker.py:2,55 -- sklearn's removed module, scipy's
 * linear_sum_assignment in every current environment; same pairs, same tie-breaking).  rows / cols: min(nr, nc)
 * pairs sorted by row; returns their number or -1. */
int ct_linear_assignment(const double *cost, int nr, int nc, int *rows, int *cols);

/* ---- runtime helpers of the per-frame host loop (no reference equivalent: they replace the torch
 * dispatcher on the four runtime calls a frame needs).  ct_graph_begin/end capture everything enqueued on
 * `stream` in between (the launches of one frame) into an executable HIP graph; ct_graph_launch replays it. */
int ct_graph_begin(void *stream);
void *ct_graph_end(void *stream);               /* executable graph handle, NULL on error */
int ct_graph_launch(void *graph_exec, void *stream);
void ct_graph_destroy(void *graph_exec);
int ct_memcpy_async(void *dst, const void *src, size_t bytes, int kind /*0 D2D, 1 H2D, 2 D2H*/, void *stream);
int ct_memset_async(void *dst, int value, size_t bytes, void *stream);      /* DEVICE memory (zero_tracking) */
int ct_stream_synchronize(void *stream);
/* One-thread kernel that stores `value` to *flag (pinned HOST memory, system-scope release): appended to a frame graph
 * behind its last copy node, it lets the host see the end of the frame by polling a cache line instead of waiting in
 * the runtime (ct_frame_loop_wait) -- and independently of work that was enqueued behind the graph for the next frame. */
int ct_signal_host(int *flag, int value, void *stream);
/* ---- the host loop of one frame of B streams, natively (round 3) ----------------------------------------------
 * Replaces, for the steady state of the tracking path, the per-frame host work of Detector.run
 * (src/lib/detector.py:139-165: process -> post_process -> merge_outputs -> tracker.step -> pre_images = images, and
 * the per-track part of _get_additional_inputs, detector.py:254-290, of the NEXT run): no interpreter between the end
 * of frame t and the launch of frame t+1.  The caller (centertrack_amd/detector.py) describes the loop once:
 * B trackers, the packed-row layout, the pinned host blocks the frame graph's copy nodes use (host_rows: destination
 * of its last node; blob_params / blob_counts: source of its first node, NULL without a prior heat-map), one
 * executable graph (ct_graph_end) and one DEVICE frame buffer per rotation slot -- frame t lives in slot t % nslots
 * and is read as pre_img from there by the graph of slot (t+1) % nslots -- and the result buffers.
 *   ct_frame_loop_submit   prior-heat-map blobs from the trackers, the frame into slot `slot` (frame_kind: copy from
 *                          DEVICE / pinned HOST memory, already IN_PLACE, or UPLOADED = wait on the device for the upload
 *                          the previous submit started), graph launch, upload of `next_frame` (pinned HOST) into the
 *                          next slot on a copy stream;
 *   ct_frame_loop_wait     block until the frame in flight finished (rows are in host_rows);
 *   ct_frame_loop_finish   wait + post-process / association of every stream: counts[b] tracks in
 *                          results[b * results_cap ..] (n > results_cap: grow and read ct_tracker_get_tracks);
 *                          CT_ERR_ARG when no frame is in flight (a second association of stale rows would age the
 *                          tracks); a failure on a helper thread is reported with its own message and stream index;
 *   (a submit that fails AFTER its graph launch -- upload / pre-stage of the next frame -- leaves the frame in
 *    flight: drain it with ct_frame_loop_wait or _finish before the next submit)
 *   ct_frame_loop_finish_submit   both, back to back (frame t+1 = the frame uploaded ahead);
 *   ct_frame_loop_upload   the upload alone (when the frame in flight was launched by a finish_submit and the caller
 *                          only now learns the frame after it).
 * trans_input: float64 [B][2][3] network-input affine of each stream's frame (prior heat-map); trans_inv: float32
 * [B][2][3] output-grid -> image affine (post-process).  One frame in flight at a time. */
enum { CT_FRAME_DEVICE = 0, CT_FRAME_HOST = 1, CT_FRAME_IN_PLACE = 2, CT_FRAME_UPLOADED = 3 };
typedef struct ct_prestage_desc {          /* the part of a frame that does not depend on the tracker (round 3): the mirrored
                                              half of a flip_test batch and the x / pre_img terms of the stem
                                              (ct_stem_forward_parts into a partial map the frame graph completes).  The loop
                                              runs it for frame t+1 right behind the graph of frame t -- while the host
                                              still associates frame t -- whenever frame t+1 has been uploaded by then. */
    int enabled;
    int N, H, W;                           /* images of a frame batch (mirrored half included), input size */
    const float *w_x, *w_img, *scale3, *shift3;
    float *partial[3]; int ldp;            /* NHWC [N,H,W,16] partial stem maps, one per rotation slot */
    int flip_B;                            /* > 0: images [0, flip_B) of the slot are mirrored into [flip_B, 2 flip_B) first */
} ct_prestage_desc;
typedef struct ct_frame_loop_desc {
    int B, K, F;
    void *const *trackers;                 /* [B] ct_tracker_create handles */
    ct_row_layout layout;
    float out_thresh, pre_thresh;
    int inp_w, inp_h;
    const float *host_rows;                /* pinned HOST [B,K,F] */
    float *rows_keep;                      /* HOST [B,K,F] or NULL: finish copies the rows here first and works on the copy,
                                              so that results / the decode dict of frame t stay valid while the graph of
                                              frame t+1 (launched by the same call) overwrites host_rows */
    int *blob_params, *blob_counts;        /* pinned HOST [B][blob_cap][3], [B]; NULL = no prior heat-map */
    int blob_cap;
    int nslots;                            /* 1 .. 3 */
    void *graphs[3];
    float *frames[3];
    size_t frame_bytes;                    /* bytes of one frame batch as the caller hands it over ([B,3,H,W] fp32) */
    void *stream;
    ct_track *results; int results_cap;    /* HOST [B][results_cap] */
    int *done_flag;                        /* pinned HOST int the frame graphs set to 1 with their last node (ct_signal_host),
                                              or NULL: wait through the runtime */
    ct_prestage_desc pre;
} ct_frame_loop_desc;
typedef struct ct_frame_step_args {
    int slot, frame_kind;
    const float *frame;                    /* DEVICE / HOST source (frame_kind 0 / 1), else ignored */
    const float *next_frame;               /* pinned HOST frame to upload for the next call, or NULL */
    const double *trans_input;
    const float *trans_inv;
} ct_frame_step_args;
void *ct_frame_loop_create(const ct_frame_loop_desc *d);      /* NULL on error */
void ct_frame_loop_destroy(void *loop);
int ct_frame_loop_submit(void *loop, const ct_frame_step_args *a);
int ct_frame_loop_wait(void *loop);
int ct_frame_loop_finish(void *loop, const ct_frame_step_args *a, int *counts);
int ct_frame_loop_finish_submit(void *loop, const ct_frame_step_args *cur, int *counts, const ct_frame_step_args *next);
int ct_frame_loop_upload(void *loop, int slot, const float *frame);   /* upload a pinned HOST frame into `slot` on the copy stream
                                                                         (the frame a later submit names with CT_FRAME_UPLOADED) */
int ct_frame_loop_prestage(void *loop, int slot); /* run the pre-stage of `slot` now unless it already ran (callers that launch a
                                                     frame graph themselves) */
int ct_frame_loop_pending_slot(void *loop);      /* slot an upload is pending for, or -1 */
int ct_frame_loop_in_flight(void *loop);         /* slot of the frame in flight, or -1 */
void ct_frame_loop_forget_upload(void *loop);    /* drop a pending upload (waits for the copy) */

/* ---- image pre-processing (CPU, like the reference's: it runs in DataLoader worker processes) -----
 * Replaces the cv2.warpAffine + normalise + HWC->CHW (+ flipped copy) of Detector.pre_process
 * (src/lib/detector.py:207-239).  img: HOST u8 [h, w, channels] (row pitch `stride` bytes); trans: float64
 * [2,3] trans_input; out: HOST fp32 [channels (*2 if flip_copy), dst_h, dst_w]. */
int ct_preprocess_image(const uint8_t *img, int h, int w, int stride, int channels, const double *trans,
                        int dst_w, int dst_h, const float *mean, const float *stdv, float *out, int flip_copy);

/* ---- the same pre-processing on the device (no reference equivalent: there the warp
 * is cv2 on the CPU and the fp32 result is uploaded, detector.py:218-226,338).  A raw u8 frame is uploaded
 * instead and warped / normalised / transposed (+ mirrored) by one kernel; results are bit-identical to
 * ct_preprocess_image.  img: DEVICE u8 [h, w, channels] (row pitch `stride` bytes); trans: HOST float64 [2,3]
 * trans_input; lut: DEVICE fp32 [channels][256], the normalisation table ct_preprocess_lut fills on the HOST
 * (lut[c][v] = float(((double)v / 255. - mean[c]) / std[c])); out: DEVICE fp32 [channels, dst_h, dst_w];
 * out_flip: optional DEVICE plane set of the same shape that receives the left-right mirrored copy
 * (flip_test, detector.py:225-226) or NULL. */
int ct_preprocess_lut(const float *mean, const float *stdv, int channels, float *lut_host);
int ct_preprocess_device(const uint8_t *img, int h, int w, int stride, int channels, const double *trans,
                         int dst_w, int dst_h, const float *lut, float *out, float *out_flip, void *stream);

/* ---- video frames as decoders deliver them (an addition under ABI 103) ------------------
 * ct_preprocess_device for ALL frames of a step in ONE launch, from packed BGR / RGB or from YUV 4:2:0 surfaces.
 * staging_host: n descriptors in pinned HOST memory; the call checks every argument on them, inverts each map in
 * place like cv::warpAffine does, uploads them with ONE asynchronous copy (staging_host -> staging_dev, enqueued by
 * the call itself) and launches once; frames of different sizes and formats share the launch, the output size
 * dst_h x dst_w is common.  Per frame: out DEVICE fp32 [3, dst_h, dst_w], out_flip the mirrored copy or NULL.
 * Planes are DEVICE u8 with a row pitch in bytes:
 *   CT_PIX_BGR24   plane 0: [h, w, 3] packed B, G, R
 *   CT_PIX_RGB24   the same with channels 0 and 2 exchanged on load
 *   CT_PIX_NV12    plane 0: Y [h, w]; plane 1: U, V interleaved [h / 2, w]
 *   CT_PIX_I420    plane 0: Y [h, w]; plane 1: U [h / 2, w / 2]; plane 2: V [h / 2, w / 2]
 * Colour conversion (binding; the integer form OpenCV publishes for COLOR_YUV2BGR_NV12): chroma nearest, pixel
 * (x, y) uses U, V at (x >> 1, y >> 1); Y' = max(0, Y - 16), u = U - 128, v = V - 128, coef = CY, CUB, CUG, CVG, CVR:
 *   B = sat8((Y' CY + CUB u + 2^19) >> 20),  G = sat8((Y' CY + CUG u + CVG v + 2^19) >> 20),
 *   R = sat8((Y' CY + CVR v + 2^19) >> 20)   (signed 32-bit, arithmetic shift)
 * Each of the four taps is converted and saturated first and blended afterwards; a tap outside the frame is 0 in
 * B, G, R.  The result equals ct_preprocess_device on the frame converted as a whole, bit for bit.
 * CT_ERR_ARG before anything is enqueued: null pointers, n outside [1, CT_FRAMES_MAX], non-positive sizes, an
 * unknown format, a null plane the format reads, a pitch below the row's bytes, odd h or w of a 4:2:0 frame, a
 * matrix entry that is not finite. */
#define CT_PIX_BGR24 0
#define CT_PIX_RGB24 1
#define CT_PIX_NV12 2
#define CT_PIX_I420 3
#define CT_FRAMES_MAX 1024
typedef struct ct_frame_desc {
    const uint8_t *plane[3];        /* DEVICE planes (unused ones ignored) */
    int pitch[3];                   /* bytes per row of each plane */
    int format, h, w;               /* CT_PIX_*; size of the frame in pixels */
    int coef[5];                    /* CY, CUB, CUG, CVG, CVR (4:2:0 formats) */
    int reserved;
    double M[6];                    /* trans_input, the forward 2 x 3 map; the call writes the inverse over it */
    float *out, *out_flip;
} ct_frame_desc;
typedef struct ct_frames_desc {
    ct_frame_desc *staging_host;    /* pinned HOST [n] */
    ct_frame_desc *staging_dev;     /* DEVICE [n] */
    int n, dst_w, dst_h;
    const float *lut;               /* DEVICE fp32 [3][256] (ct_preprocess_lut) */
} ct_frames_desc;
int ct_preprocess_frames(const ct_frames_desc *d, void *stream);

/* ---- training targets on the device -------------------------------------------------
 * Replaces, for a whole batch, the dense part of the reference's GenericDataset.__getitem__
 * (src/lib/dataset/generic_dataset.py:205-255 _get_pre_dets, :330-370 _init_ret, :386-398 _mask_ignore_or_crowd,
 * :423-515 _add_instance; draw_umich_gaussian, src/lib/utils/image.py:139-154) plus default_collate and
 * batch[k].to(device): heat maps hm [B,C,h,w] and pre_hm [B,1,H,W] and every slot tensor [B,max_objs,...] are
 * written by ONE launch from the packed records of the batch, uploaded by ONE asynchronous copy
 * (staging_host -> staging_dev, `words` int32 words, enqueued by the call itself).
 * The staging buffer, int32 words (centertrack_amd/targets.py packs it):
 *   [8 b ..]      per image: slot_off, n_slots, blob_off, n_blobs, rect_off, n_rects, pre_off, n_pre
 *                 (offsets in words from the start of the buffer, all at or behind the header)
 *   [8 B ..]      slot map [B][max_objs]: row of the image's slot list that fills slot k, or -1 = hole (zeros)
 *   [.. ]         column map [slot_words]: index of the output a column of a slot row belongs to
 *   [.. ]         output table [nout][4]: destination pointer (low, high word; 0 = not asked for),
 *                 first column | width << 16, 1 = int64 destination (sign-extended) / 0 = 32-bit copy
 *   slot rows     [n_slots][slot_words] words (float32 bit patterns and int32 values)
 *   hm blobs      [n_blobs][4]  plane, cx, cy, radius         (Gaussian peak 1)
 *   rectangles    [n_rects][5]  plane or -1 = all planes, x0, y0, x1, y1 (inclusive): pixels set to 1
 *   pre_hm blobs  [n_pre][4]    cx, cy, radius, conf          (Gaussian peak conf)
 * A pixel is max over its Gaussians of float32(exp(-(dx^2+dy^2) / (2 ((2r+1)/6)^2)) * conf) evaluated in float64,
 * |dx|, |dy| <= r, and 1 inside a rectangle.  hm / pre_hm may be NULL (not written).  Everything is validated on the
 * host copy before the upload: CT_ERR_ARG for null pointers, non-positive sizes, a plane outside [0, C), counts or
 * offsets beyond the buffer, a radius outside [0, 16384].  Every output element is written exactly once: the
 * outputs need no initialisation and two calls agree bit for bit. */
#define CT_TARGETS_CULL_CAP 256     /* blobs / rectangles a workgroup culls into LDS per round */
#define CT_TARGETS_MAX_OUT 32
typedef struct ct_targets_desc {
    const int *staging_host;        /* pinned HOST copy of the buffer (read by the validation and by the copy) */
    int *staging_dev;               /* DEVICE buffer of the same size */
    size_t words;
    int B, C, h, w;                 /* hm [B,C,h,w] */
    int H, W;                       /* pre_hm [B,1,H,W] */
    int max_objs, slot_words, nout;
    float *hm, *pre_hm;
} ct_targets_desc;
size_t ct_build_targets_header_words(int B, int max_objs, int slot_words, int nout);   /* 0 on bad sizes */
int ct_build_targets(const ct_targets_desc *d, void *stream);

/* ---- pose training targets (an addition under ABI 103) ----------------------------------
 * ct_build_targets plus the key-point heat map hm_hp [B,J,h,w] of the reference's _add_hps
 * (src/lib/dataset/generic_dataset.py:517-554) and the hm_hp line of _mask_ignore_or_crowd (:396-398), in the SAME
 * launch behind the SAME copy.  Same staging buffer; the J hm_hp planes are numbered C .. C+J-1 behind the class
 * planes: a blob (plane, cx, cy, radius) with plane >= C is a joint's Gaussian, a rectangle's plane may be any of
 * [0, C+J), -1 = all class planes or -2 = all hm_hp planes.  The joint tensors (hm_hp_mask, hp_offset, hp_ind,
 * hp_offset_mask, joint: [B, max_objs*J, ..] = [B, max_objs, J ..] in memory) are columns of the slot rows like
 * any other.  hm_hp may be NULL (not asked for); J says how many planes the lists may name either way, and J = 0
 * accepts exactly what ct_build_targets accepts.  CT_ERR_ARG, before the upload, for J < 0, hm_hp with J <= 0, a
 * blob plane outside [0, C+J), a rectangle plane outside [-2, C+J) (J = 0: [-1, C)), and everything
 * ct_build_targets refuses. */
typedef struct ct_pose_targets_desc {
    ct_targets_desc base;           /* every field as for ct_build_targets */
    float *hm_hp;                   /* DEVICE fp32 [B,J,h,w] or NULL */
    int J;
} ct_pose_targets_desc;
int ct_build_pose_targets(const ct_pose_targets_desc *d, void *stream);

/* ---- training images on the device (additions under ABI 103) ---------------------------
 * Replaces, for a whole batch, GenericDataset._get_input (src/lib/dataset/generic_dataset.py:317-327:
 * cv2.warpAffine, astype(float32) / 255., color_aug of src/lib/utils/image.py:211-243, (x - mean) / std,
 * HWC -> CHW), the flip of the frame (:90,107), default_collate and .to(device), for `image` and `pre_img`
 * together: N = B or 2 B images of H x W in TWO launches behind ONE asynchronous copy (staging_host ->
 * staging_dev, `bytes` bytes, enqueued by the call itself).
 * The staging buffer (centertrack_amd/inputs.py packs it): N descriptors of CT_INPUTS_DESC_WORDS int32 words,
 * image n = slot * B + b (slot 0: image, slot 1: pre_img), then the u8 source rows of the images that are not
 * on the device yet.  Words of a descriptor:
 *   0        kind: CT_INPUTS_STAGED (rows in this buffer), CT_INPUTS_DEVICE (rows on the device) or
 *            CT_INPUTS_ZERO (no source: the output image is 0.0f everywhere, nothing else is read)
 *   1        byte offset of the rows from the start of the buffer (staged), at or behind the descriptors
 *   2, 3     device address of the rows (device), low and high word
 *   4 .. 8   h, w of the WHOLE source image, row pitch in bytes (>= 3 w), row0, nrows: the rows
 *            [row0, row0 + nrows) of the image are present; taps on other rows, like taps outside the image, are 0
 *   9        flipped (0 / 1): the source column is mirrored, w - 1 - sx, as if img[:, ::-1] were warped
 *   10       colour augmentation on (0 / 1)
 *   11 .. 13 the order of the three functions: 0 brightness, 1 contrast, 2 saturation (a permutation)
 *   14 .. 16 float32 alpha of each function in call order;  17 .. 19 float32(1 - alpha), formed in double
 *   20 .. 25 the lighting vector, 3 float64 (B, G, R)
 *   28 .. 39 trans_input, 6 float64 (the forward 2 x 3 map; the call inverts it like cv::warpAffine and writes
 *            the inverse over it in staging_host before the copy)
 * Pass 1 warps with OpenCV's fixed-point arithmetic (bit-identical to ct_preprocess_image) into `warped`
 * [N][H][W] (B, G, R in the low three bytes of a word) and stores one float64 partial sum of the float32 grey
 * value per CT_INPUTS_TILE_W x CT_INPUTS_TILE_H tile into `partials` [N][ct_build_inputs_partials(H, W)];
 * pass 2 adds an image's partials in index order, forms gs_mean and writes float32 NCHW planes: every element
 * of image [B,3,H,W] (and pre_img, if given) exactly once.  No memset, no atomics, no host wait; the arguments
 * are checked on staging_host before anything is enqueued. */
#define CT_INPUTS_DESC_WORDS 48
#define CT_INPUTS_TILE_W 64
#define CT_INPUTS_TILE_H 16
#define CT_INPUTS_STAGED 0
#define CT_INPUTS_DEVICE 1
#define CT_INPUTS_ZERO 2
typedef struct ct_inputs_desc {
    int *staging_host;              /* pinned HOST copy of the buffer */
    int *staging_dev;               /* DEVICE buffer of the same size */
    size_t bytes;
    int B, N, H, W;                 /* N = B (image only) or 2 B (image and pre_img) */
    float mean[3], stdv[3];         /* the dataset's mean / std (B, G, R) */
    float *image, *pre_img;         /* DEVICE fp32 [B,3,H,W]; pre_img NULL when N = B */
    unsigned *warped;               /* DEVICE scratch [N][H][W] */
    double *partials;               /* DEVICE scratch [N][ct_build_inputs_partials(H, W)] */
    float *gs_mean;                 /* optional DEVICE [N]: the mean grey value of each warped image */
} ct_inputs_desc;
size_t ct_build_inputs_partials(int H, int W);          /* partial sums per image; 0 on bad sizes */
int ct_build_inputs(const ct_inputs_desc *d, void *stream);

/* ---- fused optimizer step (an addition under ABI 103) ------------------------------------
 * torch.optim.Adam / torch.optim.SGD (the reference's two optimizers, src/main.py:17-26) for EVERY tensor of an
 * optimizer in ONE launch, whatever their number, sizes and parameter groups.  `table` is a DEVICE buffer the caller
 * has uploaded (centertrack_amd/optim.py packs it): n records of CT_OPTIM_REC_BYTES bytes, then n + 1 int32 words,
 * prefix[t] = number of CT_OPTIM_CHUNK-element chunks of the tensors before t (prefix[0] = 0, prefix[n] = all chunks).
 * A workgroup takes chunks c, c + grid, ..: it finds c's tensor by binary search in the prefix and updates elements
 * [(c - prefix[t]) * CT_OPTIM_CHUNK, ..) of it -- with 16-byte loads and stores when p, g, m, v are all 16-byte
 * aligned, element by element otherwise and for the last numel % 4 elements.  Every element of p, m, v is read once
 * and written once, nothing outside [ptr, ptr + numel) is touched; no atomics, no LDS, no workspace.
 * The scalars are per tensor and float32, formed by the host in double from the tensor's own integer step t:
 *   Adam  s[0] 1 - beta1, s[1] beta2, s[2] 1 - beta2, s[3] lr / (1 - beta1^t), s[4] sqrt(1 - beta2^t), s[5] eps,
 *         s[6] weight_decay:    g' = g + wd p (wd != 0);  m += s0 (g' - m);  v = s1 v + (s2 g') g';
 *                               p += -s3 (m / (sqrt(v) / s4 + s5))
 *   SGD   s[0] lr, s[1] momentum, s[2] weight_decay; first != 0: the buffer is created by this step:
 *                               g' = g + wd p (wd != 0);  m = first ? g' : s1 m + g';  p += -s0 m
 *         (m NULL: no momentum, p += -s0 g')
 * in float32 in this order, without contraction, division and square root correctly rounded (the non-capturable
 * branch of torch/optim/adam.py::_single_tensor_adam and torch/optim/sgd.py::_single_tensor_sgd).
 * CT_ERR_ARG before anything is enqueued: a null table, n outside [1, CT_OPTIM_MAX_TENSORS], chunks outside
 * [n, 2^31), a kind outside the enum.  `chunks` (= prefix[n]) only sizes the grid: the kernel reads the prefix. */
#define CT_OPTIM_ADAM 0
#define CT_OPTIM_SGD 1
#define CT_OPTIM_CHUNK 4096
#define CT_OPTIM_REC_BYTES 128
#define CT_OPTIM_SCALARS 8
#define CT_OPTIM_MAX_TENSORS (1 << 20)
typedef struct ct_optim_rec {
    float *p;                       /* DEVICE fp32 [numel], updated in place */
    const float *g;                 /* gradient */
    float *m;                       /* exp_avg / momentum_buffer */
    float *v;                       /* exp_avg_sq (Adam; NULL for SGD) */
    long long numel;                /* > 0 */
    float s[CT_OPTIM_SCALARS];
    int first;                      /* SGD: this step creates the momentum buffer */
    int reserved[11];
    const float *src;               /* ct_optim_pack_grads only: where g is gathered from (the last 8 bytes; else NULL) */
} ct_optim_rec;
int ct_optim_step(const void *table, int n, long long chunks, int kind, void *stream);

/* ---- gradient gather for data-parallel training (an addition under ABI 103) ----------------
 * One launch that gathers the gradient of every tensor of the table into ONE flat buffer, so that the exchange between
 * replicas is one collective.  Tensor t lives in the flat buffer at element offset prefix[t] * CT_OPTIM_CHUNK -- the
 * chunk prefix the table already carries, so every tensor starts 16-byte aligned when the buffer does -- and the
 * record's g points there; src is the tensor the gradient is read from (p.grad).  For chunk c of tensor t:
 *   g[i] = src[i] * scale   (i < numel; one float32 product, no contraction)
 *   g[i] = +0.0             (numel <= i < chunks_t * CT_OPTIM_CHUNK: the tail of the tensor's last chunk)
 * so g must have room for whole chunks, and the packed buffer is a function of the gradients alone.  The walk is
 * ct_optim_step's (grid min(chunks, 2048), strided, binary search in the prefix); 16-byte loads when src is 16-byte
 * aligned, 16-byte stores when g is, element by element otherwise.  src is never written; a record whose src is NULL
 * is left alone.  No atomics, no LDS, no workspace.  ct_optim_step, ct_optim_step_guarded and ct_optim_norms never
 * read src: run on the same table afterwards, they read the gathered (and reduced) gradient through g.
 * CT_ERR_ARG before anything is enqueued: a null table, n outside [1, CT_OPTIM_MAX_TENSORS], chunks outside
 * [n, 2^31), a scale that is NaN or +-Inf. */
int ct_optim_pack_grads(const void *table, int n, long long chunks, float scale, void *stream);

/* ---- guarded optimizer step (an addition under ABI 103) -----------------------------------
 * The global gradient norm, torch.nn.utils.clip_grad_norm_'s clip coefficient and a "skip the step when a gradient is
 * not finite" decision, all formed and consumed on the device: no host read between the norm and the update.
 *
 * ct_optim_norms makes two launches over the table ct_optim_step reads (only g and numel of a record are used; p, m, v
 * are never read).
 *   Pass 1 walks the chunks as ct_optim_step does (grid min(chunks, 2048), strided, binary search in the prefix).  For
 *   chunk c it forms the sum of (double)g[i] * (double)g[i] -- every product is exact in double -- and counts the
 *   elements that are NaN or +-Inf, with 16-byte loads when the record's g is 16-byte aligned, element by element
 *   otherwise and for the last numel % 4 elements.  The order of the additions is fixed and does not depend on the
 *   alignment: lane l of 256 adds elements 4 (l + 256 k) + e in the order k = 0..3, e = 0..3; the 64 lanes of a wave
 *   are added in a butterfly (xor 32, 16, .. 1), the four waves in the order ((w0 + w1) + w2) + w3 through LDS.  One
 *   16-byte record per chunk (the double, the int count, a zero word) is stored at workspace[c].
 *   Pass 2 is one launch of one workgroup, whatever the data: the chunk partials of tensor t are added in chunk order
 *   into per-tensor sums (stored behind the chunk records in the workspace, and in per_tensor[t] when per_tensor is
 *   not NULL: n doubles, the SUM OF SQUARES of tensor t), the per-tensor sums in tensor order into S, the counts into
 *   F.  All in double, no atomics.  The chunking comes from the prefix alone and the orders are fixed, so S has the
 *   same bits from run to run and whatever the grid of pass 1.
 * Pass 2 then writes *guard (DEVICE memory; the caller allocates it once and zeroes it once):
 *   sumsq = S, norm = sqrt(S), nonfinite = F, skip = (F > 0 && skip_nonfinite),
 *   coef = 1.0f when max_norm <= 0 or F > 0; otherwise c = max_norm / (norm + 1e-6) in double and
 *          coef = c < 1 ? (float)c : 1.0f   (clip_grad_norm_'s rule),
 *   and the running counters only this launch updates: steps += 1; nonfinite_steps += (F > 0); skipped += skip;
 *   clipped += (coef < 1 && !skip); on steps with F == 0, norm_sum += norm and norm_max = max(norm_max, norm).
 *
 * ct_optim_step_guarded is ct_optim_step reading guard->skip and guard->coef (uniform loads) first.  skip != 0: no byte
 * of p, m, v is written -- except that the momentum buffer of an SGD record with first != 0 is filled with zeros, so
 * that the NEXT step's m = momentum m + g gives the m = g of torch's first step.  Otherwise g' = g * coef (one float32
 * product, no contraction) takes the place of g and the arithmetic of ct_optim_step follows unchanged; coef = 1.0f
 * gives ct_optim_step's bits.  The gradient tensors are NEVER written: clip_grad_norm_ scales .grad in place, this
 * does not, so p.grad after the step still holds the unclipped gradient.
 *
 * CT_ERR_ARG before anything is enqueued: what ct_optim_step refuses (ct_optim_norms takes no kind), a null guard, a
 * null workspace, workspace_bytes below ct_optim_norms_workspace_bytes(n, chunks), a max_norm that is NaN.
 * ct_optim_norms_workspace_bytes is 16 (chunks + n), and 0 for an n or chunks the calls refuse. */
typedef struct ct_optim_guard {
    double sumsq, norm;             /* of the last ct_optim_norms */
    double norm_sum, norm_max;      /* running, over the steps with nonfinite == 0 */
    long long nonfinite;            /* of the last ct_optim_norms: elements that are NaN or +-Inf */
    long long steps, skipped, clipped, nonfinite_steps;     /* running */
    float coef;                     /* what ct_optim_step_guarded multiplies every gradient element by */
    int skip;                       /* != 0: ct_optim_step_guarded leaves p, m, v alone */
} ct_optim_guard;
size_t ct_optim_norms_workspace_bytes(int n, long long chunks);
int ct_optim_norms(const void *table, int n, long long chunks, double max_norm, int skip_nonfinite, double *per_tensor,
                   ct_optim_guard *guard, void *workspace, size_t workspace_bytes, void *stream);
int ct_optim_step_guarded(const void *table, int n, long long chunks, int kind, const ct_optim_guard *guard, void *stream);

#ifdef __cplusplus
}
#endif
#endif
