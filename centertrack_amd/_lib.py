"""ctypes binding of libcentertrack_hip.so (the C ABI of include/centertrack_hip.h).

No torch types cross the boundary: tensors are passed as raw device pointers
(``tensor.data_ptr()``) plus sizes, and the HIP stream as ``void*``.  There is NO CPU
fallback: if the shared library is missing or a call fails this raises."""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CENTERTRACK_LIB') or os.path.join(_PKG, 'libcentertrack_hip.so')   # (override: debugging builds)

c_float_p = ctypes.c_void_p      # device pointers are opaque to the host
NUM_HEADS = 11
(HEAD_REG, HEAD_WH, HEAD_TRACKING, HEAD_LTRB, HEAD_LTRB_AMODAL, HEAD_DEP, HEAD_ROT, HEAD_DIM,
 HEAD_AMODEL_OFFSET, HEAD_NUSCENES_ATT, HEAD_VELOCITY) = range(NUM_HEADS)
HEAD_INDEX = {'reg': HEAD_REG, 'wh': HEAD_WH, 'tracking': HEAD_TRACKING, 'ltrb': HEAD_LTRB,
              'ltrb_amodal': HEAD_LTRB_AMODAL, 'dep': HEAD_DEP, 'rot': HEAD_ROT, 'dim': HEAD_DIM,
              'amodel_offset': HEAD_AMODEL_OFFSET, 'nuscenes_att': HEAD_NUSCENES_ATT,
              'velocity': HEAD_VELOCITY}
HEAD_CH = {'reg': 2, 'wh': 2, 'tracking': 2, 'ltrb': 4, 'ltrb_amodal': 4, 'dep': 1, 'rot': 8, 'dim': 3,
           'amodel_offset': 2, 'nuscenes_att': 8, 'velocity': 3}

CT_RELU = 1
CT_OUT_NCHW = 2
CT_DCN_MAIN, CT_DCN_FINISH, CT_DCN_OFFSETS = 1, 2, 4
CT_OK, CT_ERR_ARG, CT_ERR_LAUNCH, CT_ERR_WORKSPACE = 0, 1, 2, 3


class ConvDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('w_packed', ctypes.c_void_p), ('Cout', ctypes.c_int), ('ks', ctypes.c_int),
                ('stride', ctypes.c_int),
                ('scale', ctypes.c_void_p), ('shift', ctypes.c_void_p),
                ('res', ctypes.c_void_p), ('ldr', ctypes.c_int),
                ('y', ctypes.c_void_p), ('ldy', ctypes.c_int),
                ('flags', ctypes.c_int),
                ('sig_lo', ctypes.c_int), ('sig_hi', ctypes.c_int),
                ('dep_lo', ctypes.c_int), ('dep_hi', ctypes.c_int), ('depth_scale', ctypes.c_float),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('split_k', ctypes.c_int), ('algo', ctypes.c_int), ('w_winograd', ctypes.c_void_p),
                ('pool_y', ctypes.c_void_p), ('pool_ld', ctypes.c_int),
                ('proj_w_packed', ctypes.c_void_p), ('proj_scale', ctypes.c_void_p), ('proj_shift', ctypes.c_void_p),
                ('proj_y', ctypes.c_void_p), ('proj_ldy', ctypes.c_int)]


class DcnDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('om', ctypes.c_void_p), ('ldom', ctypes.c_int),
                ('w_packed', ctypes.c_void_p), ('Cout', ctypes.c_int),
                ('scale', ctypes.c_void_p), ('shift', ctypes.c_void_p),
                ('y', ctypes.c_void_p), ('ldy', ctypes.c_int),
                ('flags', ctypes.c_int),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('split_k', ctypes.c_int), ('algo', ctypes.c_int), ('fuse_offset', ctypes.c_int),
                ('w_off_packed', ctypes.c_void_p), ('b_off', ctypes.c_void_p),
                ('up_w', ctypes.c_void_p), ('up_f', ctypes.c_int), ('up_skip', ctypes.c_void_p), ('up_lds', ctypes.c_int),
                ('up_y', ctypes.c_void_p), ('up_ldy', ctypes.c_int),
                ('om_partial', ctypes.c_void_p), ('om_partial_bytes', ctypes.c_size_t),
                ('w_off_winograd', ctypes.c_void_p)]


CT_DCN_BWD_INPUT, CT_DCN_BWD_OFFSET_MASK, CT_DCN_BWD_WEIGHT = 1, 2, 4


class DcnBwdDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('om', ctypes.c_void_p), ('ldom', ctypes.c_int),
                ('gy', ctypes.c_void_p), ('Cout', ctypes.c_int), ('ldgy', ctypes.c_int),
                ('wT_packed', ctypes.c_void_p),
                ('gx', ctypes.c_void_p), ('ldgx', ctypes.c_int),
                ('gom', ctypes.c_void_p), ('ldgom', ctypes.c_int),
                ('gw', ctypes.c_void_p), ('gb', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('flags', ctypes.c_int)]


CT_LOSS_FOCAL, CT_LOSS_L1, CT_LOSS_L1_DEPTH, CT_LOSS_BCE, CT_LOSS_ROT = range(5)
CT_LOSS_MAX_HEADS = 16
CT_LOSS_MAX_SLOTS = 8192


class LossHead(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int), ('logits', ctypes.c_void_p), ('C', ctypes.c_int),
                ('target', ctypes.c_void_p), ('mask', ctypes.c_void_p), ('ind', ctypes.c_void_p),
                ('cat', ctypes.c_void_p), ('M', ctypes.c_int), ('grad', ctypes.c_void_p)]


class LossDesc(ctypes.Structure):
    _fields_ = [('B', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('heads', ctypes.POINTER(LossHead)), ('nheads', ctypes.c_int),
                ('loss', ctypes.c_void_p), ('grad_loss', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


CT_HEADS_BWD_HIDDEN, CT_HEADS_BWD_WEIGHT = 1, 2


class ConvBwdWeightDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('gy', ctypes.c_void_p), ('Cout', ctypes.c_int), ('ldgy', ctypes.c_int),
                ('ks', ctypes.c_int), ('stride', ctypes.c_int),
                ('gw', ctypes.c_void_p), ('gb', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class HeadsTailHead(ctypes.Structure):
    _fields_ = [('gout', ctypes.c_void_p), ('c', ctypes.c_int), ('w2', ctypes.c_void_p),
                ('gw2', ctypes.c_void_p), ('gb2', ctypes.c_void_p)]


class HeadsTailBwdDesc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('hc', ctypes.c_int),
                ('heads', ctypes.POINTER(HeadsTailHead)), ('nheads', ctypes.c_int),
                ('mid', ctypes.c_void_p), ('ldmid', ctypes.c_int),
                ('gmid', ctypes.c_void_p), ('ldgmid', ctypes.c_int),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('flags', ctypes.c_int)]


CT_BN_BATCH_STATS = 1


class BnDesc(ctypes.Structure):
    _fields_ = [('z', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('C', ctypes.c_int), ('ldz', ctypes.c_int),
                ('mean', ctypes.c_void_p), ('var', ctypes.c_void_p), ('invstd', ctypes.c_void_p),
                ('eps', ctypes.c_float),
                ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p),
                ('y', ctypes.c_void_p), ('ldy', ctypes.c_int),
                ('gy', ctypes.c_void_p), ('ldgy', ctypes.c_int),
                ('gz', ctypes.c_void_p), ('ldgz', ctypes.c_int),
                ('ggamma', ctypes.c_void_p), ('gbeta', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('flags', ctypes.c_int)]


class UpsampleBwdDesc(ctypes.Structure):
    _fields_ = [('gy', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('C', ctypes.c_int), ('ldgy', ctypes.c_int), ('f', ctypes.c_int),
                ('w', ctypes.c_void_p),
                ('gx', ctypes.c_void_p), ('ldgx', ctypes.c_int),
                ('x', ctypes.c_void_p), ('ldx', ctypes.c_int),
                ('gw', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


CT_BN_ACT_RELU = 2


class ConvS2BwdDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('gy', ctypes.c_void_p), ('Cout', ctypes.c_int), ('ldgy', ctypes.c_int),
                ('w_s2t', ctypes.c_void_p),
                ('gx', ctypes.c_void_p), ('ldgx', ctypes.c_int),
                ('gw', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('flags', ctypes.c_int)]


class BnActDesc(ctypes.Structure):
    _fields_ = BnDesc._fields_ + [('res', ctypes.c_void_p), ('ldr', ctypes.c_int),
                                  ('gres', ctypes.c_void_p), ('ldgres', ctypes.c_int)]


class BnMergeDesc(ctypes.Structure):
    _fields_ = [('rows', ctypes.c_void_p), ('world', ctypes.c_int), ('C', ctypes.c_int), ('ld', ctypes.c_int),
                ('eps', ctypes.c_float),
                ('mean', ctypes.c_void_p), ('var', ctypes.c_void_p), ('invstd', ctypes.c_void_p), ('unbiased', ctypes.c_void_p),
                ('inv_count', ctypes.c_void_p), ('count', ctypes.c_void_p),
                ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p), ('beta_shifted', ctypes.c_void_p)]


class StemConvDesc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('inp', ctypes.c_void_p * 3), ('w', ctypes.c_void_p * 3),
                ('z', ctypes.c_void_p * 3), ('ldz', ctypes.c_int * 3),
                ('gz', ctypes.c_void_p * 3), ('ldgz', ctypes.c_int * 3),
                ('gw', ctypes.c_void_p * 3), ('gin', ctypes.c_void_p * 3),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t)]


class StemSumDesc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('z', ctypes.c_void_p * 3), ('ldz', ctypes.c_int * 3),
                ('mean', ctypes.c_void_p * 3), ('invstd', ctypes.c_void_p * 3),
                ('gamma', ctypes.c_void_p * 3), ('beta', ctypes.c_void_p * 3),
                ('y', ctypes.c_void_p), ('ldy', ctypes.c_int)]


CT_MAX_FUSED_HEADS = 8


class HeadsDesc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Cin', ctypes.c_int), ('ldx', ctypes.c_int),
                ('w0_winograd', ctypes.c_void_p), ('b0', ctypes.c_void_p), ('nheads', ctypes.c_int),
                ('w2', ctypes.c_void_p), ('b2', ctypes.c_void_p),
                ('cout', ctypes.c_int * CT_MAX_FUSED_HEADS), ('coff', ctypes.c_int * CT_MAX_FUSED_HEADS),
                ('out', ctypes.c_void_p), ('ctot', ctypes.c_int),
                ('sig_lo', ctypes.c_int), ('sig_hi', ctypes.c_int), ('dep_lo', ctypes.c_int), ('dep_hi', ctypes.c_int),
                ('depth_scale', ctypes.c_float)]


class SparseHeadsDesc(ctypes.Structure):
    _fields_ = [('feat', ctypes.c_void_p), ('ldf', ctypes.c_int), ('nheads', ctypes.c_int),
                ('head', ctypes.c_int * NUM_HEADS),
                ('w1', ctypes.c_void_p * NUM_HEADS), ('b1', ctypes.c_void_p * NUM_HEADS),
                ('w2', ctypes.c_void_p * NUM_HEADS), ('b2', ctypes.c_void_p * NUM_HEADS),
                ('depth_scale', ctypes.c_float), ('zero_tracking', ctypes.c_int),
                ('flip_B', ctypes.c_int), ('flip_mode', ctypes.c_int * NUM_HEADS)]


class DecodeDesc(ctypes.Structure):
    _fields_ = [('hm', ctypes.c_void_p), ('B', ctypes.c_int), ('C', ctypes.c_int), ('h', ctypes.c_int),
                ('w', ctypes.c_int), ('K', ctypes.c_int),
                ('heads', ctypes.c_void_p * NUM_HEADS),
                ('out', ctypes.c_void_p), ('inds', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('hm_batch_stride', ctypes.c_size_t), ('head_batch_stride', ctypes.c_size_t * NUM_HEADS),
                ('out_stride', ctypes.c_int),
                ('host_out', ctypes.c_void_p), ('done_flag', ctypes.c_void_p), ('done_counter', ctypes.c_void_p),
                ('sparse', ctypes.POINTER(SparseHeadsDesc))]


class PoseDesc(ctypes.Structure):
    _fields_ = [('rows', ctypes.c_void_p), ('row_floats', ctypes.c_int), ('box_col', ctypes.c_int),
                ('inds', ctypes.c_void_p),
                ('B', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int), ('K', ctypes.c_int),
                ('num_joints', ctypes.c_int),
                ('hps', ctypes.c_void_p), ('hm_hp', ctypes.c_void_p), ('hp_offset', ctypes.c_void_p),
                ('hps_batch_stride', ctypes.c_size_t), ('hm_hp_batch_stride', ctypes.c_size_t),
                ('hp_offset_batch_stride', ctypes.c_size_t),
                ('out', ctypes.c_void_p), ('out_stride', ctypes.c_int),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
                ('box_wh', ctypes.c_void_p), ('box_reg', ctypes.c_void_p), ('box_ltrb', ctypes.c_void_p),
                ('box_wh_batch_stride', ctypes.c_size_t), ('box_reg_batch_stride', ctypes.c_size_t),
                ('box_ltrb_batch_stride', ctypes.c_size_t)]


class PoseSparseDesc(ctypes.Structure):
    _fields_ = [('base', PoseDesc), ('feat', ctypes.c_void_p), ('ldf', ctypes.c_int), ('flip_B', ctypes.c_int),
                ('hps_w1', ctypes.c_void_p), ('hps_b1', ctypes.c_void_p), ('hps_w2', ctypes.c_void_p), ('hps_b2', ctypes.c_void_p),
                ('off_w1', ctypes.c_void_p), ('off_b1', ctypes.c_void_p), ('off_w2', ctypes.c_void_p), ('off_b2', ctypes.c_void_p),
                ('flip_pairs', ctypes.c_void_p), ('num_pairs', ctypes.c_int)]


class FlipHead(ctypes.Structure):
    _fields_ = [('src', ctypes.c_void_p), ('dst', ctypes.c_void_p), ('src_batch_stride', ctypes.c_size_t),
                ('C', ctypes.c_int), ('mode', ctypes.c_int)]


CT_FLIP_AVG, CT_FLIP_NEG_EVEN, CT_FLIP_JOINTS, CT_FLIP_JOINT_OFFSETS = range(4)


class RowLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ('score', 'cls', 'cts', 'tracking', 'bbox', 'amodel_offset')]


class Track(ctypes.Structure):
    _fields_ = [('score', ctypes.c_float), ('cls', ctypes.c_int), ('ct', ctypes.c_float * 2),
                ('tracking', ctypes.c_float * 2), ('bbox', ctypes.c_float * 4),
                ('tracking_id', ctypes.c_int), ('age', ctypes.c_int), ('active', ctypes.c_int),
                ('row', ctypes.c_int)]


class PrestageDesc(ctypes.Structure):
    _fields_ = [('enabled', ctypes.c_int), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('w_x', ctypes.c_void_p), ('w_img', ctypes.c_void_p), ('scale3', ctypes.c_void_p), ('shift3', ctypes.c_void_p),
                ('partial', ctypes.c_void_p * 3), ('ldp', ctypes.c_int), ('flip_B', ctypes.c_int)]


class FrameLoopDesc(ctypes.Structure):
    _fields_ = [('B', ctypes.c_int), ('K', ctypes.c_int), ('F', ctypes.c_int),
                ('trackers', ctypes.POINTER(ctypes.c_void_p)),
                ('layout', RowLayout),
                ('out_thresh', ctypes.c_float), ('pre_thresh', ctypes.c_float),
                ('inp_w', ctypes.c_int), ('inp_h', ctypes.c_int),
                ('host_rows', ctypes.c_void_p), ('rows_keep', ctypes.c_void_p),
                ('blob_params', ctypes.c_void_p), ('blob_counts', ctypes.c_void_p), ('blob_cap', ctypes.c_int),
                ('nslots', ctypes.c_int),
                ('graphs', ctypes.c_void_p * 3), ('frames', ctypes.c_void_p * 3),
                ('frame_bytes', ctypes.c_size_t),
                ('stream', ctypes.c_void_p),
                ('results', ctypes.c_void_p), ('results_cap', ctypes.c_int), ('done_flag', ctypes.c_void_p),
                ('pre', PrestageDesc)]


class FrameStepArgs(ctypes.Structure):
    _fields_ = [('slot', ctypes.c_int), ('frame_kind', ctypes.c_int),
                ('frame', ctypes.c_void_p), ('next_frame', ctypes.c_void_p),
                ('trans_input', ctypes.c_void_p), ('trans_inv', ctypes.c_void_p)]


CT_FRAME_DEVICE, CT_FRAME_HOST, CT_FRAME_IN_PLACE, CT_FRAME_UPLOADED = range(4)


CT_TARGETS_CULL_CAP = 256
CT_TARGETS_MAX_OUT = 32


class TargetsDesc(ctypes.Structure):
    _fields_ = [('staging_host', ctypes.c_void_p), ('staging_dev', ctypes.c_void_p), ('words', ctypes.c_size_t),
                ('B', ctypes.c_int), ('C', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('max_objs', ctypes.c_int), ('slot_words', ctypes.c_int), ('nout', ctypes.c_int),
                ('hm', ctypes.c_void_p), ('pre_hm', ctypes.c_void_p)]


class PoseTargetsDesc(ctypes.Structure):
    _fields_ = [('base', TargetsDesc), ('hm_hp', ctypes.c_void_p), ('J', ctypes.c_int)]


CT_INPUTS_DESC_WORDS = 48
CT_INPUTS_TILE_W, CT_INPUTS_TILE_H = 64, 16
CT_INPUTS_STAGED, CT_INPUTS_DEVICE, CT_INPUTS_ZERO = range(3)


class InputsDesc(ctypes.Structure):
    _fields_ = [('staging_host', ctypes.c_void_p), ('staging_dev', ctypes.c_void_p), ('bytes', ctypes.c_size_t),
                ('B', ctypes.c_int), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('mean', ctypes.c_float * 3), ('stdv', ctypes.c_float * 3),
                ('image', ctypes.c_void_p), ('pre_img', ctypes.c_void_p), ('warped', ctypes.c_void_p),
                ('partials', ctypes.c_void_p), ('gs_mean', ctypes.c_void_p)]


CT_PIX_BGR24, CT_PIX_RGB24, CT_PIX_NV12, CT_PIX_I420 = range(4)
CT_FRAMES_MAX = 1024


class FrameDesc(ctypes.Structure):
    _fields_ = [('plane', ctypes.c_void_p * 3), ('pitch', ctypes.c_int * 3),
                ('format', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('coef', ctypes.c_int * 5), ('reserved', ctypes.c_int),
                ('M', ctypes.c_double * 6), ('out', ctypes.c_void_p), ('out_flip', ctypes.c_void_p)]


class FramesDesc(ctypes.Structure):
    _fields_ = [('staging_host', ctypes.c_void_p), ('staging_dev', ctypes.c_void_p),
                ('n', ctypes.c_int), ('dst_w', ctypes.c_int), ('dst_h', ctypes.c_int),
                ('lut', ctypes.c_void_p)]


CT_OPTIM_ADAM, CT_OPTIM_SGD = range(2)
CT_OPTIM_CHUNK = 4096
CT_OPTIM_REC_BYTES = 128
CT_OPTIM_SCALARS = 8
CT_OPTIM_MAX_TENSORS = 1 << 20


class OptimRec(ctypes.Structure):
    _fields_ = [('p', ctypes.c_void_p), ('g', ctypes.c_void_p), ('m', ctypes.c_void_p), ('v', ctypes.c_void_p),
                ('numel', ctypes.c_longlong), ('s', ctypes.c_float * CT_OPTIM_SCALARS), ('first', ctypes.c_int),
                ('reserved', ctypes.c_int * 11), ('src', ctypes.c_void_p)]


class OptimGuard(ctypes.Structure):
    _fields_ = [('sumsq', ctypes.c_double), ('norm', ctypes.c_double), ('norm_sum', ctypes.c_double),
                ('norm_max', ctypes.c_double), ('nonfinite', ctypes.c_longlong), ('steps', ctypes.c_longlong),
                ('skipped', ctypes.c_longlong), ('clipped', ctypes.c_longlong), ('nonfinite_steps', ctypes.c_longlong),
                ('coef', ctypes.c_float), ('skip', ctypes.c_int)]


class SlotDesc(ctypes.Structure):
    _fields_ = [('map', ctypes.c_void_p), ('N', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('C', ctypes.c_int), ('ld', ctypes.c_int),
                ('ind', ctypes.c_void_p), ('M', ctypes.c_int),
                ('rows', ctypes.c_void_p), ('ldr', ctypes.c_int)]


ABI_VERSION = 103       # CT_ABI_VERSION of include/centertrack_hip.h

EXPORTS = ['ct_last_error', 'ct_version', 'ct_set_tuning', 'ct_packed_weight_elems', 'ct_pack_conv_weight',
           'ct_packed_winograd_elems', 'ct_pack_winograd_weight', 'ct_conv2d',
           'ct_conv2d_workspace_bytes', 'ct_heads_fused', 'ct_dcn_v2', 'ct_dcn_v2_workspace_bytes', 'ct_dcn_v2_offsets_bytes', 'ct_dcn_v2_group', 'ct_dcn_v2_group_workspace_bytes', 'ct_dcn_v2_group_plan',
           'ct_dcn_v2_backward', 'ct_dcn_v2_backward_workspace_bytes', 'ct_packed_dcn_weight_t_elems', 'ct_pack_dcn_weight_t',
           'ct_generic_loss_forward', 'ct_generic_loss_backward', 'ct_generic_loss_workspace_bytes',
           'ct_conv2d_backward_weight', 'ct_conv2d_backward_weight_workspace_bytes', 'ct_heads_tail_backward',
           'ct_heads_tail_backward_workspace_bytes', 'ct_bn_stats', 'ct_bn_relu_apply', 'ct_bn_relu_backward', 'ct_bn_workspace_bytes',
           'ct_upsample_add_backward', 'ct_upsample_add_backward_workspace_bytes', 'ct_dcn_mask_sigmoid_backward',
           'ct_conv2d_s2_backward', 'ct_conv2d_s2_backward_workspace_bytes', 'ct_packed_conv_weight_s2t_elems', 'ct_pack_conv_weight_s2t',
           'ct_bn_act_apply', 'ct_bn_act_backward', 'ct_bn_act_workspace_bytes', 'ct_maxpool2x2_backward', 'ct_stem_forward',
           'ct_stem_conv_forward', 'ct_stem_conv_backward', 'ct_stem_conv_backward_workspace_bytes', 'ct_stem_bn_relu_sum',
           'ct_maxpool2x2', 'ct_upsample_add', 'ct_nchw_to_nhwc', 'ct_nhwc_to_nchw',
           'ct_decode_row_floats', 'ct_decode_workspace_bytes', 'ct_decode', 'ct_decode_pose_workspace_bytes',
           'ct_decode_pose', 'ct_decode_pose_sparse_workspace_bytes', 'ct_decode_pose_sparse', 'ct_render_pre_hm',
           'ct_tracker_create', 'ct_tracker_destroy', 'ct_tracker_reset', 'ct_tracker_num_tracks',
           'ct_tracker_id_count', 'ct_tracker_get_tracks', 'ct_tracker_step', 'ct_tracker_prehm_params', 'ct_linear_assignment', 'ct_tracker_set_mode', 'ct_tracker_init_tracks',
           'ct_tracker_step_public', 'ct_tracker_step_dets', 'ct_transform_points',
           'ct_preprocess_image', 'ct_preprocess_lut', 'ct_preprocess_device', 'ct_preprocess_frames', 'ct_graph_begin', 'ct_graph_end', 'ct_graph_launch', 'ct_graph_destroy',
           'ct_memcpy_async', 'ct_memset_async', 'ct_stream_synchronize', 'ct_flip_merge', 'ct_flip_images',
           'ct_frame_loop_create', 'ct_frame_loop_destroy', 'ct_frame_loop_submit', 'ct_frame_loop_wait', 'ct_frame_loop_finish',
           'ct_frame_loop_finish_submit', 'ct_frame_loop_upload', 'ct_frame_loop_pending_slot', 'ct_frame_loop_in_flight',
           'ct_frame_loop_forget_upload', 'ct_frame_loop_prestage', 'ct_stem_forward_parts', 'ct_signal_host',
           'ct_build_targets', 'ct_build_targets_header_words', 'ct_build_pose_targets', 'ct_build_inputs', 'ct_build_inputs_partials',
           'ct_optim_step', 'ct_slot_gather', 'ct_slot_fold',
           'ct_optim_norms_workspace_bytes', 'ct_optim_norms', 'ct_optim_step_guarded', 'ct_optim_pack_grads',
           'ct_bn_stats_row', 'ct_bn_merge_stats', 'ct_bn_act_backward_apply', 'ct_bn_relu_backward_apply']

_lib = None


class CTError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises if it has not been built: the product path
    never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CTError('%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                      '(hipcc --offload-arch=gfx950); there is no CPU fallback' % LIB_PATH)
    # torch first: its wheel bundles its own libamdhip64 / HSA runtime, and the library must bind to THAT copy (same
    # soname as /opt/rocm's).  Loaded the other way round (this library, then torch) the process ends up with the
    # system runtime under torch's allocator and every launch fails with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.ct_last_error.restype = ctypes.c_char_p
    lib.ct_version.restype = i
    if lib.ct_version() != ABI_VERSION:      # the ctypes structs below mirror ONE header version (tests/test_cabi.py)
        raise CTError('%s is ABI version %d, this binding was written against %d: rebuild it (python -m '
                      'centertrack_amd.build)' % (LIB_PATH, lib.ct_version(), ABI_VERSION))
    lib.ct_set_tuning.argtypes = [ctypes.c_char_p, i]
    lib.ct_packed_weight_elems.restype = sz
    lib.ct_packed_weight_elems.argtypes = [i, i, i]
    lib.ct_pack_conv_weight.argtypes = [p, p, i, i, i, p]
    lib.ct_packed_winograd_elems.restype = sz
    lib.ct_packed_winograd_elems.argtypes = [i, i]
    lib.ct_pack_winograd_weight.argtypes = [p, p, i, i, p]
    lib.ct_conv2d.argtypes = [ctypes.POINTER(ConvDesc), p]
    lib.ct_conv2d_workspace_bytes.restype = sz
    lib.ct_conv2d_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.ct_heads_fused.argtypes = [ctypes.POINTER(HeadsDesc), p]
    lib.ct_dcn_v2.argtypes = [ctypes.POINTER(DcnDesc), p]
    lib.ct_dcn_v2_workspace_bytes.restype = sz
    lib.ct_dcn_v2_workspace_bytes.argtypes = [ctypes.POINTER(DcnDesc)]
    lib.ct_dcn_v2_offsets_bytes.restype = sz
    lib.ct_dcn_v2_offsets_bytes.argtypes = [ctypes.POINTER(DcnDesc)]
    lib.ct_dcn_v2_group.argtypes = [ctypes.POINTER(DcnDesc), i, i, p]
    lib.ct_dcn_v2_group_workspace_bytes.restype = sz
    lib.ct_dcn_v2_group_workspace_bytes.argtypes = [ctypes.POINTER(DcnDesc)]
    lib.ct_dcn_v2_group_plan.argtypes = [ctypes.POINTER(DcnDesc), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    lib.ct_dcn_v2_backward.argtypes = [ctypes.POINTER(DcnBwdDesc), p]
    lib.ct_dcn_v2_backward_workspace_bytes.restype = sz
    lib.ct_dcn_v2_backward_workspace_bytes.argtypes = [ctypes.POINTER(DcnBwdDesc)]
    lib.ct_packed_dcn_weight_t_elems.restype = sz
    lib.ct_packed_dcn_weight_t_elems.argtypes = [i, i]
    lib.ct_pack_dcn_weight_t.argtypes = [p, p, i, i, p]
    lib.ct_generic_loss_forward.argtypes = [ctypes.POINTER(LossDesc), p]
    lib.ct_generic_loss_backward.argtypes = [ctypes.POINTER(LossDesc), p]
    lib.ct_generic_loss_workspace_bytes.restype = sz
    lib.ct_generic_loss_workspace_bytes.argtypes = [ctypes.POINTER(LossDesc)]
    lib.ct_conv2d_backward_weight.argtypes = [ctypes.POINTER(ConvBwdWeightDesc), p]
    lib.ct_conv2d_backward_weight_workspace_bytes.restype = sz
    lib.ct_conv2d_backward_weight_workspace_bytes.argtypes = [ctypes.POINTER(ConvBwdWeightDesc)]
    lib.ct_heads_tail_backward.argtypes = [ctypes.POINTER(HeadsTailBwdDesc), p]
    lib.ct_heads_tail_backward_workspace_bytes.restype = sz
    lib.ct_heads_tail_backward_workspace_bytes.argtypes = [ctypes.POINTER(HeadsTailBwdDesc)]
    lib.ct_bn_stats.argtypes = [ctypes.POINTER(BnDesc), p]
    lib.ct_bn_relu_apply.argtypes = [ctypes.POINTER(BnDesc), p]
    lib.ct_bn_relu_backward.argtypes = [ctypes.POINTER(BnDesc), p]
    lib.ct_bn_workspace_bytes.restype = sz
    lib.ct_bn_workspace_bytes.argtypes = [ctypes.POINTER(BnDesc)]
    lib.ct_upsample_add_backward.argtypes = [ctypes.POINTER(UpsampleBwdDesc), p]
    lib.ct_upsample_add_backward_workspace_bytes.restype = sz
    lib.ct_upsample_add_backward_workspace_bytes.argtypes = [ctypes.POINTER(UpsampleBwdDesc)]
    lib.ct_dcn_mask_sigmoid_backward.argtypes = [p, i, p, i, i, i, i, p]
    lib.ct_conv2d_s2_backward.argtypes = [ctypes.POINTER(ConvS2BwdDesc), p]
    lib.ct_conv2d_s2_backward_workspace_bytes.restype = sz
    lib.ct_conv2d_s2_backward_workspace_bytes.argtypes = [ctypes.POINTER(ConvS2BwdDesc)]
    lib.ct_packed_conv_weight_s2t_elems.restype = sz
    lib.ct_packed_conv_weight_s2t_elems.argtypes = [i, i]
    lib.ct_pack_conv_weight_s2t.argtypes = [p, p, i, i, p]
    lib.ct_bn_act_apply.argtypes = [ctypes.POINTER(BnActDesc), p]
    lib.ct_bn_act_backward.argtypes = [ctypes.POINTER(BnActDesc), p]
    lib.ct_bn_act_workspace_bytes.restype = sz
    lib.ct_bn_act_workspace_bytes.argtypes = [ctypes.POINTER(BnActDesc)]
    lib.ct_bn_stats_row.argtypes = [ctypes.POINTER(BnDesc), p, p]
    lib.ct_bn_merge_stats.argtypes = [ctypes.POINTER(BnMergeDesc), p]
    lib.ct_bn_act_backward_apply.argtypes = [ctypes.POINTER(BnActDesc), p, p, p]
    lib.ct_bn_relu_backward_apply.argtypes = [ctypes.POINTER(BnDesc), p, p, p]
    lib.ct_maxpool2x2_backward.argtypes = [p, i, i, i, i, i, p, i, p, i, p, i, p]
    lib.ct_stem_conv_forward.argtypes = [ctypes.POINTER(StemConvDesc), p]
    lib.ct_stem_conv_backward.argtypes = [ctypes.POINTER(StemConvDesc), p]
    lib.ct_stem_conv_backward_workspace_bytes.restype = sz
    lib.ct_stem_conv_backward_workspace_bytes.argtypes = [ctypes.POINTER(StemConvDesc)]
    lib.ct_stem_bn_relu_sum.argtypes = [ctypes.POINTER(StemSumDesc), p]
    lib.ct_stem_forward.argtypes = [p, p, p, i, i, i, p, p, p, p, p, p, i, p]
    lib.ct_stem_forward_parts.argtypes = [p, p, p, p, i, i, i, i, p, p, p, p, p, p, i, p]
    lib.ct_maxpool2x2.argtypes = [p, i, i, i, i, i, p, i, p]
    lib.ct_upsample_add.argtypes = [p, i, i, i, i, i, p, i, p, i, p, i, p]
    lib.ct_nchw_to_nhwc.argtypes = [p, i, i, i, i, p, i, p]
    lib.ct_nhwc_to_nchw.argtypes = [p, i, i, i, i, i, p, p]
    lib.ct_decode_row_floats.argtypes = [ctypes.POINTER(DecodeDesc)]
    lib.ct_decode_workspace_bytes.restype = sz
    lib.ct_decode_workspace_bytes.argtypes = [ctypes.POINTER(DecodeDesc)]
    lib.ct_decode.argtypes = [ctypes.POINTER(DecodeDesc), p]
    lib.ct_decode_pose_workspace_bytes.restype = sz
    lib.ct_decode_pose_workspace_bytes.argtypes = [ctypes.POINTER(PoseDesc)]
    lib.ct_decode_pose.argtypes = [ctypes.POINTER(PoseDesc), p]
    lib.ct_decode_pose_sparse_workspace_bytes.argtypes = [ctypes.POINTER(PoseSparseDesc), ctypes.POINTER(sz)]
    lib.ct_decode_pose_sparse.argtypes = [ctypes.POINTER(PoseSparseDesc), p]
    lib.ct_render_pre_hm.argtypes = [p, p, i, i, i, i, p, i, p]
    lib.ct_tracker_create.restype = p
    lib.ct_tracker_create.argtypes = [ctypes.c_float, i]
    lib.ct_tracker_destroy.restype = None
    lib.ct_tracker_destroy.argtypes = [p]
    lib.ct_tracker_reset.restype = None
    lib.ct_tracker_reset.argtypes = [p]
    lib.ct_tracker_num_tracks.argtypes = [p]
    lib.ct_tracker_id_count.argtypes = [p]
    lib.ct_tracker_get_tracks.argtypes = [p, p, i]
    lib.ct_tracker_step.argtypes = [p, p, i, i, ctypes.POINTER(RowLayout), ctypes.c_float, p, p, i]
    lib.ct_tracker_prehm_params.argtypes = [p, ctypes.c_float, p, i, i, p, i]
    lib.ct_linear_assignment.argtypes = [p, i, i, p, p]
    lib.ct_tracker_set_mode.argtypes = [p, i, i]
    lib.ct_tracker_init_tracks.argtypes = [p, p, i]
    lib.ct_tracker_step_public.argtypes = [p, p, i, i, ctypes.POINTER(RowLayout), ctypes.c_float, p, p, i, p, i]
    lib.ct_tracker_step_dets.argtypes = [p, p, i, p, i, p, i]
    lib.ct_transform_points.argtypes = [p, p, i, p]
    lib.ct_preprocess_image.argtypes = [p, i, i, i, i, p, i, i, p, p, p, i]
    lib.ct_preprocess_lut.argtypes = [p, p, i, p]
    lib.ct_preprocess_device.argtypes = [p, i, i, i, i, p, i, i, p, p, p, p]
    lib.ct_preprocess_frames.argtypes = [ctypes.POINTER(FramesDesc), p]
    lib.ct_graph_begin.argtypes = [p]
    lib.ct_graph_end.restype = p
    lib.ct_graph_end.argtypes = [p]
    lib.ct_graph_launch.argtypes = [p, p]
    lib.ct_graph_destroy.restype = None
    lib.ct_graph_destroy.argtypes = [p]
    lib.ct_memcpy_async.argtypes = [p, p, sz, i, p]
    lib.ct_stream_synchronize.argtypes = [p]
    lib.ct_memset_async.argtypes = [p, i, sz, p]
    lib.ct_signal_host.argtypes = [p, i, p]
    lib.ct_flip_merge.argtypes = [ctypes.POINTER(FlipHead), i, p, i, i, i, i, p]
    lib.ct_flip_images.argtypes = [p, p, sz, i, p]
    lib.ct_frame_loop_create.restype = p
    lib.ct_frame_loop_create.argtypes = [ctypes.POINTER(FrameLoopDesc)]
    lib.ct_frame_loop_destroy.restype = None
    lib.ct_frame_loop_destroy.argtypes = [p]
    lib.ct_frame_loop_submit.argtypes = [p, ctypes.POINTER(FrameStepArgs)]
    lib.ct_frame_loop_wait.argtypes = [p]
    lib.ct_frame_loop_finish.argtypes = [p, ctypes.POINTER(FrameStepArgs), p]
    lib.ct_frame_loop_finish_submit.argtypes = [p, ctypes.POINTER(FrameStepArgs), p, ctypes.POINTER(FrameStepArgs)]
    lib.ct_frame_loop_upload.argtypes = [p, i, p]
    lib.ct_frame_loop_pending_slot.argtypes = [p]
    lib.ct_frame_loop_prestage.argtypes = [p, i]
    lib.ct_frame_loop_in_flight.argtypes = [p]
    lib.ct_frame_loop_forget_upload.restype = None
    lib.ct_frame_loop_forget_upload.argtypes = [p]
    lib.ct_build_targets_header_words.restype = sz
    lib.ct_build_targets_header_words.argtypes = [i, i, i, i]
    lib.ct_build_targets.argtypes = [ctypes.POINTER(TargetsDesc), p]
    lib.ct_build_pose_targets.argtypes = [ctypes.POINTER(PoseTargetsDesc), p]
    lib.ct_build_inputs_partials.restype = sz
    lib.ct_build_inputs_partials.argtypes = [i, i]
    lib.ct_build_inputs.argtypes = [ctypes.POINTER(InputsDesc), p]
    lib.ct_optim_step.argtypes = [p, i, ctypes.c_longlong, i, p]
    lib.ct_optim_norms_workspace_bytes.restype = sz
    lib.ct_optim_norms_workspace_bytes.argtypes = [i, ctypes.c_longlong]
    lib.ct_optim_norms.argtypes = [p, i, ctypes.c_longlong, ctypes.c_double, i, p, p, p, sz, p]
    lib.ct_optim_step_guarded.argtypes = [p, i, ctypes.c_longlong, i, p, p]
    lib.ct_optim_pack_grads.argtypes = [p, i, ctypes.c_longlong, ctypes.c_float, p]
    lib.ct_slot_gather.argtypes = [ctypes.POINTER(SlotDesc), p]
    lib.ct_slot_fold.argtypes = [ctypes.POINTER(SlotDesc), p]
    # CENTERTRACK_TUNE="key=value,key=value": launch-heuristic knobs of ct_set_tuning (A/B runs)
    for kv in filter(None, os.environ.get('CENTERTRACK_TUNE', '').split(',')):
        k, _, v = kv.partition('=')
        if lib.ct_set_tuning(k.strip().encode(), int(v)) != 0:
            raise CTError('CENTERTRACK_TUNE: %s' % lib.ct_last_error().decode())
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        raise CTError('%s failed (code %d): %s' % (what or 'libcentertrack_hip call', rc,
                                                  load().ct_last_error().decode()))


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


import contextlib as _contextlib


@_contextlib.contextmanager
def capture_guard(collect=True):
    """No run of the cyclic garbage collector while a stream is capturing.  A detector that is only reachable through reference
    cycles (its context holds closures over itself) is destroyed whenever the collector happens to run; its ``__del__`` waits for
    the device and destroys HIP objects, and such a call in the middle of a capture invalidates the capture ("operation failed due
    to a previous error during capture") -- in whichever test or request happens to be capturing at that moment (round 6: 13
    cascading failures in some runs of the GPU suite, none in others).  Garbage is collected BEFORE the capture instead, as
    ``torch.cuda.graph`` does on entry."""
    import gc
    if os.environ.get('CT_NO_CAPTURE_GUARD') == '1':        # (tests only: shows what the guard prevents)
        yield
        return
    if collect:             # (``torch.cuda.graph`` collects on entry itself: its call sites pass False)
        gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()

