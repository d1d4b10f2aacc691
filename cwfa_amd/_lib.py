"""ctypes binding of libcwfa_hip.so (C ABI: include/cwfa_hip.h).

There is NO fallback: if the shared library is missing or a symbol cannot be resolved, importing an op raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcwfa_hip.so")

CLAMP = {"NONE": 0, "ATAN": 1, "TANH": 2, "SIGMOID": 3}
ACT = {None: 0, "none": 0, "elu": 1, "prelu": 2, "gelu": 3, "relu": 4}
CHAIN_MAX = 8

c_f32p = C.c_void_p
c_i64p = C.c_void_p
c_f64p = C.c_void_p


class AffineStage(C.Structure):
    _fields_ = [("s_raw", c_f32p), ("t", c_f32p), ("s_bs", C.c_int64), ("t_bs", C.c_int64), ("clamp_kind", C.c_int),
                ("clamp", C.c_float), ("pre_scale", C.c_float), ("t_neg_div_sqrt2", C.c_int), ("perm", c_i64p),
                ("perm_axis", C.c_int), ("gin", C.c_int)]


class Chain(C.Structure):
    _fields_ = [("n_stages", C.c_int), ("stage", AffineStage * CHAIN_MAX), ("src_c", C.c_void_p), ("src_h", C.c_void_p)]


class ChainGrads(C.Structure):
    _fields_ = [("ds", c_f32p * CHAIN_MAX), ("dt", c_f32p * CHAIN_MAX), ("ds_bs", C.c_int64 * CHAIN_MAX),
                ("dt_bs", C.c_int64 * CHAIN_MAX)]


class ConvOpts(C.Structure):
    _fields_ = [("bias", c_f32p), ("act", C.c_int), ("prelu_alpha", c_f32p), ("residual", c_f32p), ("res_bs", C.c_int64),
                ("act2", C.c_int), ("in_scale", c_f32p), ("in_shift", c_f32p), ("in_affine_bs", C.c_int), ("in_add", c_f32p),
                ("in_add_bs", C.c_int64), ("upshuffle2", C.c_int), ("in_blocked8", C.c_int), ("out_blocked8", C.c_int),
                ("in_cat", c_f32p), ("in_cat_bs", C.c_int64), ("in_cat_from", C.c_int), ("in_cat_c1", C.c_int), ("out_stats", c_f64p), ("prelu_per_channel", C.c_int),
                ("out_sample_stats", c_f64p)]


class Couple(C.Structure):
    _fields_ = [("x", c_f32p), ("y", c_f32p), ("x_bs", C.c_int64), ("y_bs", C.c_int64), ("n", C.c_int), ("clamp_kind", C.c_int),
                ("clamp", C.c_float), ("pre_scale", C.c_float), ("rev", C.c_int), ("logdet", c_f64p), ("in_blocked8", C.c_int)]


class EvalAffine(C.Structure):
    _fields_ = [("enabled", C.c_int), ("scale", C.c_float), ("std", C.c_float), ("mean", C.c_float)]


class EvalPost(C.Structure):
    _fields_ = [("normalize", C.c_int), ("threshold", C.c_int), ("norm_sub", C.c_float), ("norm_div", C.c_float),
                ("vol_min", C.c_float), ("lower", C.c_float), ("upper", C.c_float), ("clamp_value", C.c_float)]


LION_MAX_TENSORS = 96              # CWFA_LION_MAX_TENSORS
LION_BLOCK_ELEMS = 4096            # CWFA_LION_BLOCK_ELEMS


class LionTensor(C.Structure):
    _fields_ = [("p", c_f32p), ("g", c_f32p), ("m", c_f32p), ("numel", C.c_int64)]


class LionTable(C.Structure):
    _fields_ = [("n", C.c_int), ("t", LionTensor * LION_MAX_TENSORS)]


NLL_MAX_LEVELS = 8                 # CWFA_NLL_MAX_LEVELS


class NllLevels(C.Structure):
    _fields_ = [("n", C.c_int), ("level", c_f32p * NLL_MAX_LEVELS), ("bs", C.c_int64 * NLL_MAX_LEVELS)]


EXTREMA_STRIDE = 12                # CWFA_EXTREMA_STRIDE
SELECT_WORKSPACE_BYTES = 8448      # CWFA_SELECT_WORKSPACE_BYTES
PREP_MAX_BINS = 10239              # CWFA_PREP_MAX_BINS
PREP_MOMENTS_WORKSPACE = 4096      # CWFA_PREP_MOMENTS_WORKSPACE (doubles)
PREP_VOL = {"none": 0, "two": 1, "le": 2, "maxnorm": 3, "max_only": 4}          # CWFA_PREP_VOL_*
PREP_APPLY = {"clamp_zero": 0, "sub_div": 1, "div_mul": 2}                      # CWFA_PREP_*
DECONV_PRE = {None: 0, "none": 0, "relu": 1}                                    # CWFA_DECONV_PRE_*
DECONV_POST = {None: 0, "none": 0, "abs": 1}                                    # CWFA_DECONV_POST_*
DECONV_ACCEL_UNITS = 1024          # CWFA_DECONV_ACCEL_UNITS
DECONV_UPDATE_UNITS = 256          # CWFA_DECONV_UPDATE_UNITS
DECONV_NLL_WORKSPACE_BYTES = 8192  # CWFA_DECONV_NLL_WORKSPACE_BYTES
ACTIVITY_KIND = {"std": 0, "range": 1, "peak": 2, "snr": 3}                     # CWFA_ACTIVITY_*
CORR_FORWARD = {6: 3, 8: 4, 26: 13}                                            # CWFA_CORR_*: neighbours -> forward offsets K
NMAX_MAX_DIST = 16                # CWFA_NMAX_MAX_DIST
SELECT_FORM = {"auto": 0, "lds": 1, "stream": 2}                                # cwfa_temporal_select's `form`
SHIFT_MODE = {"bilinear": 0, "nearest": 1}                                      # cwfa_reg_shift's `mode`
VIEW_MODEL = {"axial": 0, "free": 1}                                            # cwfa_reg_fit_views_f64's `model`
REG_MAX_VIEWS = 254               # a label is a byte; label L is the rest of the frame
REG_MAX_BLOCKS = 4096             # REG_MAX_BLOCKS of register_internal.h: the blocks of a grid
FOOTPRINT_SELECT_MAX = 1 << 15   # CWFA_FOOTPRINT_SELECT_MAX
DEMIX_PAIR_BYTES = 48             # CWFA_DEMIX_PAIR_BYTES
REGRESS_MAX_K = 16                # CWFA_REGRESS_MAX_K
REGRESS_WANT = {"corr": 1, "beta": 2, "t": 4, "r2": 8}                          # CWFA_REGRESS_CORR .. CWFA_REGRESS_R2
REGRESS_STATUS = {1: "collinear or constant", 2: "non-finite", 3: "row count"}  # CWFA_REGRESS_COLLINEAR ..

# name -> (restype, argtypes); must list EVERY function declared in include/cwfa_hip.h (tests/test_boundary.py checks)
i, i64, f, d, p = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p
SIGNATURES = {
    "cwfa_version": (i, []),
    "cwfa_last_error": (C.c_char_p, []),
    "cwfa_set_option": (i, [C.c_char_p, i]),
    "cwfa_haar1d_fwd_f32": (i, [p, p, p, i, i, i64, i64, i64, i64, p]),
    "cwfa_haar1d_inv_f32": (i, [p, p, p, i, i, i64, i64, i64, i64, p]),
    "cwfa_haar2d_fwd_f32": (i, [p, p, i, i, i, i, i, f, p]),
    "cwfa_haar2d_inv_f32": (i, [p, p, i, i, i, i, i, f, p]),
    "cwfa_haar3d_fwd_f32": (i, [p, p, i, i, i, i, i, f, i64, p]),
    "cwfa_haar3d_inv_f32": (i, [p, p, i, i, i, i, i, f, i64, p]),
    "cwfa_gather_f32": (i, [p, p, p, i, i, i, i, i, i64, i64, p]),
    "cwfa_affine_f32": (i, [p, p, C.POINTER(AffineStage), i, i, i, i, i, i64, i64, p, p, p]),
    "cwfa_channel_affine_f32": (i, [p, p, p, p, i, p, p, i, i, i64, i64, i64, p]),
    "cwfa_chain_inv_f32": (i, [p, p, p, C.POINTER(Chain), i, i, i, i, i64, i64, i64, p, p]),
    "cwfa_chain_inv_var_f32": (i, [p, p, C.POINTER(Chain), f, f, i, i, i, i, i64, i64, p]),
    "cwfa_chain_inv_roi_cov_f32": (i, [p, C.POINTER(Chain), f, i, i, i, i, i, p, i, p, i, p, i64, p]),
    "cwfa_rand_uniform_f32": (i, [p, i, i64, i64, C.c_uint64, C.c_uint32, C.c_uint32, p]),
    "cwfa_rand_trunc_normal_f32": (i, [p, i, i64, i64, f, C.c_uint64, C.c_uint32, C.c_uint32, p]),
    "cwfa_chain_inv_samples_f32": (i, [p, p, p, C.POINTER(Chain), i, i, i, i, i, i64, i64, i64, i64, i64, i64, f, C.c_uint64, C.c_uint32,
                                       C.c_uint32, p]),
    "cwfa_chain_nll_map_f32": (i, [p, p, p, p, C.POINTER(Chain), i, i, i, i, i64, i64, i64, i64, p, p]),
    "cwfa_nll_compose_f32": (i, [C.POINTER(NllLevels), p, i, i, i64, i64, p]),
    "cwfa_chain_fwd_f32": (i, [p, p, p, C.POINTER(Chain), p, i, i, i, i, i64, i64, i64, p, p, p]),
    "cwfa_conv2d_packed_floats": (i64, [i, i, i]),
    "cwfa_conv2d_pack_f32": (i, [p, p, i, i, i, i, p]),
    "cwfa_conv2d_f32": (i, [p, p, p, i, i, i, i, i, i, i64, i64, C.POINTER(ConvOpts), p]),
    "cwfa_subnet_pack1x1_f32": (i, [p, p, p]),
    "cwfa_subnet_layer_tape_f32": (i, [p, p, p, p, p, p, p, i, i, i, i64, i64, i64, p]),
    "cwfa_subnet_layer_f32": (i, [p, p, p, p, p, p, i, i, i, i64, i64, p]),
    "cwfa_conv3d_1k1_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i, p]),
    "cwfa_conv3d_1k1_split_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i, p]),
    "cwfa_channel_stats_f32": (i, [p, p, i, i, i64, i64, p]),
    "cwfa_bn_fold_f32": (i, [p, d, p, p, p, p, f, p, i, p, p, i, p]),
    "cwfa_maxpool_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, p]),
    "cwfa_sample_stats_f32": (i, [p, p, i, i64, p]),
    "cwfa_layernorm_apply_f32": (i, [p, p, p, p, f, p, i, i64, p]),
    "cwfa_convnext_tail_f32": (i, [p, p, p, p, f, p, p, p, p, p, p, p, i, p, i, i, i64, i64, i64, i64, i64, p]),
    "cwfa_attention_combine_f32": (i, [p, p, p, p, p, p, p, p, i, i, i64, p]),
    "cwfa_scale_channels_f32": (i, [p, p, p, i, i, i64, p]),
    "cwfa_axpby_f32": (i, [p, p, f, f, p, i64, p]),
    "cwfa_bn_running_update_f32": (i, [p, C.c_double, f, p, p, p, i, p]),
    "cwfa_bn_finish_f32": (i, [p, d, p, p, p, f, i, p, p, f, p, p, f, f, i, p, p, i, i, p]),
    "cwfa_chain_bwd_f32": (i, [p, p, C.POINTER(Chain), C.POINTER(ChainGrads), p, p, i, i, i, i, i64, i64, i64, f, f, i, p, p]),
    "cwfa_affine_bwd_f32": (i, [p, p, C.POINTER(AffineStage), i, i, i, i, i, i64, i64, p, p, p, p, p]),
    "cwfa_chain_inv_bwd_f32": (i, [p, p, C.POINTER(Chain), C.POINTER(ChainGrads), i, i, i, i, i64, i64, f, i, i, p, p, p, p]),
    "cwfa_conv2d_wgrad_workspace_bytes": (i64, [i, i, i, i, i, i]),
    "cwfa_conv2d_wgrad_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, i64, i64, f, p]),
    "cwfa_elu_bwd_f32": (i, [p, p, p, p, i, i64, i64, i64, i64, i64, p]),
    "cwfa_conv3d_hidden_fwd_f32": (i, [p, p, p, p, i, i, i, i, i, p]),
    "cwfa_conv3d_hidden_bwd_f32": (i, [p, p, p, p, p, p, i, i, i, i, i, p]),
    "cwfa_conv3d_input_bwd_f32": (i, [p, p, p, i, i, i, i, i, p]),
    "cwfa_conv3d_wgrad_workspace_bytes": (i64, [i, i, i, i]),
    "cwfa_conv3d_wgrad_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, i, f, p]),
    "cwfa_prelu_bwd_f32": (i, [p, p, p, p, p, i, i64, i64, i64, i64, p]),
    "cwfa_plane_affine_f32": (i, [p, p, p, i, p, p, i, i, i64, i64, i64, i64, p]),
    "cwfa_bn_bwd_stats_f32": (i, [p, p, p, p, i, i, i64, i64, i64, p]),
    "cwfa_bn_act_bwd_f32": (i, [p, p, p, i, p, p, p, p, p, i, i, i64, i64, i64, i64, p]),
    "cwfa_maxpool2_bwd_f32": (i, [p, p, p, p, i, i, i, i, p]),
    "cwfa_gelu_f32": (i, [p, p, p, i64, i, p]),
    "cwfa_layernorm_bwd_f32": (i, [p, p, p, p, p, p, p, p, p, i, i64, p]),
    "cwfa_attention_bwd_f32": (i, [p, p, p, p, p, p, p, p, p, i, i, i64, p]),
    "cwfa_split_workspace_bytes": (i64, [i, i, i64]),
    "cwfa_split_input_f32": (i, [p, p, i, i, i64, i64, p, p, i64, p, i64, p]),
    "cwfa_conv_split_packed_bytes": (i64, [i, i, i]),
    "cwfa_conv_split_pack_f32": (i, [p, p, i, i, i, i, p]),
    "cwfa_conv_split_f32": (i, [p, p, p, i, i, i, i, i, i, i64, C.POINTER(ConvOpts), p]),
    "cwfa_conv3x3_split_packed_bytes": (i64, [i, i]),
    "cwfa_conv3x3_split_pack_f32": (i, [p, p, i, i, p]),
    "cwfa_conv3x3_split_f32": (i, [p, p, p, i, i, i, i, i, i64, i64, C.POINTER(ConvOpts), p]),
    "cwfa_conv7x7_split_packed_bytes": (i64, [i, i]),
    "cwfa_conv7x7_split_pack_f32": (i, [p, p, i, i, p]),
    "cwfa_conv7x7_split_f32": (i, [p, p, p, i, i, i, i, i, i64, i64, C.POINTER(ConvOpts), p]),
    "cwfa_couple_rows": (i, [i, p]),
    "cwfa_conv3x3_split_couple_f32": (i, [p, p, p, i, i, i, i, i64, C.POINTER(Couple), p]),
    "cwfa_subnet_layer_split_packed_bytes": (i64, []),
    "cwfa_subnet_layer_split_pack_f32": (i, [p, p, p, p]),
    "cwfa_subnet_layer_split_f32": (i, [p, p, p, p, p, i, i, i, i64, i64, i, p]),
    "cwfa_subnet_layer_split_tape_f32": (i, [p, p, p, p, p, p, i, i, i, i64, i64, i64, p]),
    "cwfa_conv3x3_out_split_packed_bytes": (i64, [i]),
    "cwfa_conv3x3_out_split_pack_f32": (i, [p, p, i, p]),
    "cwfa_conv3x3_out_split_f32": (i, [p, p, p, p, i, i, i, i, i64, i64, i, p]),
    "cwfa_subnet_layer_first_packed_bytes": (i64, []),
    "cwfa_subnet_layer_first_pack_f32": (i, [p, p, p, i, p, p]),
    "cwfa_subnet_layer_first_f32": (i, [p, p, p, p, p, p, i, i, i, i, i64, i64, i64, i, p]),
    "cwfa_extract_views_f32": (i, [p, p, p, i, i, i, i, i, i, f, f, i64, p]),
    "cwfa_eval_splits": (i64, [i, i64]),
    "cwfa_volume_extrema_f32": (i, [p, p, p, p, i, i64, i64, i64, C.POINTER(EvalAffine), p]),
    "cwfa_volume_metrics_f32": (i, [p, p, p, p, i, i64, i64, i64, C.POINTER(EvalAffine), f, f, f, p]),
    "cwfa_mip3_f32": (i, [p, p, p, p, p, p, i, i, i, i, i64, i64, i, C.POINTER(EvalAffine), C.POINTER(EvalPost), p]),
    "cwfa_projection_compose_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, i, p]),
    "cwfa_roi_means_f32": (i, [p, p, p, i, i, i, i, i, i64, p]),
    "cwfa_select_positive_f32": (i, [p, i, i64, i64, i64, p, p, p, p]),
    "cwfa_prep_volumes_f16": (i, [p, p, p, i, i, i, i, i, i, i, i, i, f, f, i, p]),
    "cwfa_prep_frames_f32": (i, [p, p, i, i, i, i, i, i, i, p]),
    "cwfa_histogram_f32": (i, [p, i64, f, f, p, i, p, i, p]),
    "cwfa_prep_apply_f32": (i, [p, i64, i, f, f, i, p]),
    "cwfa_moments_f64": (i, [p, i64, d, p, p, i, p]),
    "cwfa_stack_mean_std_f32": (i, [p, p, p, i, i64, i64, p]),
    "cwfa_lion_step_f32": (i, [C.POINTER(LionTable), f, f, f, f, p, p, p]),
    "cwfa_wmse_workspace_bytes": (i64, [i64]),
    "cwfa_wmse_loss_f32": (i, [p, p, p, f, f, p, p, p, i64, p]),
    "cwfa_select_nonzero_f32": (i, [p, i, i64, i64, i64, p, p, p, p]),
    "cwfa_deconv_spectrum_mul_c64": (i, [p, p, p, i, i64, i, i, p]),
    "cwfa_deconv_project_f32": (i, [p, p, i, i, i, i, i, i, i, i, i, i, i, p]),
    "cwfa_deconv_ratio_f32": (i, [p, p, p, p, i64, p]),
    "cwfa_deconv_clamp_f32": (i, [p, i64, p, p, f, p]),
    "cwfa_deconv_update_f32": (i, [p, p, i, i, i, i, p]),
    "cwfa_deconv_update_accel_f32": (i, [p, p, p, p, p, p, i64, i, i, i, i, p]),
    "cwfa_deconv_alpha_f64": (i, [p, i64, d, p, p]),
    "cwfa_deconv_predict_f32": (i, [p, p, p, p, i, i, i, i, p]),
    "cwfa_deconv_poisson_nll_f32": (i, [p, p, i64, p, i64, i64, p, p]),
    "cwfa_deconv_update_map_f32": (i, [p, p, p, p, p, i64, i, i, i, i, p]),
    "cwfa_deconv_update_accel_map_f32": (i, [p, p, p, p, p, p, p, p, i64, p, i64, i, i, i, i, p]),
    "cwfa_deconv_penalty_f64": (i, [p, i64, p, i64, i64, p]),
    "cwfa_activity_update_f32": (i, [p, p, p, p, p, p, i, i64, i64, i, p]),
    "cwfa_activity_finish_f32": (i, [p, p, p, p, p, i64, i, p, p, p, i64, p]),
    "cwfa_local_maxima_f32": (i, [p, i, i, i, f, i, i, i, i, i, i, p, p, i64, p, p]),
    "cwfa_activity_update_corr_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i64, i, i, p]),
    "cwfa_activity_corr_finish_f32": (i, [p, p, p, i64, i, i, i, i, p, p]),
    "cwfa_rand_poisson_f32": (i, [p, p, i, i64, i64, i64, p, p, C.c_uint64, C.c_uint32, C.c_uint32, p]),
    "cwfa_temporal_select": (i, [p, i, i, i64, i64, p, p, C.POINTER(C.c_int), i, p, i, p]),
    "cwfa_temporal_select_lds_frames": (i, [i, i]),
    "cwfa_frame_dots_workspace_bytes": (i64, [i, i64]),
    "cwfa_frame_dots": (i, [p, i, i, i64, i64, p, p, p, i, p]),
    "cwfa_sparse_residual": (i, [p, i, i, i64, i64, p, p, p, p, i, p]),
    "cwfa_reg_window": (i, [p, i, i, i, i, i64, p, p, p, p]),
    "cwfa_reg_whiten_c64": (i, [p, p, i, i64, f, p, p]),
    "cwfa_reg_peak_f32": (i, [p, i, i, i, i64, i, i, i, p, p, p, p]),
    "cwfa_reg_shift": (i, [p, i, i, i, i, i64, p, i, f, p, p]),
    "cwfa_reg_upsample_workspace_bytes": (i64, [i, i, i, i]),
    "cwfa_reg_upsample_c64": (i, [p, i, i, i, i64, p, i, i, p, p, p, p, p]),
    "cwfa_reg_fine_peak_f64": (i, [p, p, i, i, i, i, p, p, p]),
    "cwfa_reg_window_views": (i, [p, i, i, i, i, i64, p, i, i, i, p, p, p, p]),
    "cwfa_reg_label_map": (i, [p, i, i, i, i, i, p, p]),
    "cwfa_reg_fit_views_f64": (i, [p, p, p, i, i, d, d, i, p, p, p, p]),
    "cwfa_reg_shift_labeled": (i, [p, i, i, i, i, i64, p, p, i, i, f, p, p]),
    "cwfa_reg_window3d_f32": (i, [p, i, i, i, i, i64, p, p, p, p, p]),
    "cwfa_reg_peak3d_f32": (i, [p, i, i, i, i, i64, i, i, i, i, p, p, p, p]),
    "cwfa_reg_shift3d_f32": (i, [p, i, i, i, i, i64, p, i, f, p, p]),
    "cwfa_reg_window_blocks3d_f32": (i, [p, i, i, i, i, i64, p, i, i, i, i, i, i, p, p, p, p, p]),
    "cwfa_reg_field_fill": (i, [p, p, p, i, i, i, i, d, p, p, p, p]),
    "cwfa_reg_warp3d_f32": (i, [p, i, i, i, i, i64, p, i, i, i, p, p, p, p, p, p, i, f, p, p]),
    "cwfa_reg_fit_rigid_f64": (i, [p, p, p, i, i, d, d, p, p, p, p]),
    "cwfa_reg_rigid3d_f32": (i, [p, i, i, i, i, i64, p, f, f, i, f, p, p]),
    "cwfa_roi_mark_u8": (i, [p, i, p, i, i, i, p]),
    "cwfa_roi_weighted_sums_f32": (i, [p, p, p, p, p, i, i, i, i, i, i64, p]),
    "cwfa_roi_shell_sums_f32": (i, [p, p, p, p, p, p, i, i, i, i, i, i64, p]),
    "cwfa_footprint_update_f32": (i, [p, p, p, p, p, p, p, p, i, i, i, i, i, i64, i, p]),
    "cwfa_footprint_corr_f32": (i, [p, p, p, i, i64, i, p, p]),
    "cwfa_footprint_select_f32": (i, [p, p, p, p, i, f, p, p, p, p]),
    "cwfa_sliding_quantile_limits": (i, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cwfa_sliding_quantile_f64": (i, [p, i, i, i64, i, i, p, i, p]),
    "cwfa_trace_select_f64": (i, [p, i, i, i64, C.POINTER(C.c_int), i, p, p]),
    "cwfa_ar1_deconv_workspace_bytes": (i64, [i, i]),
    "cwfa_ar1_deconv_f64": (i, [p, i, i, i64, d, p, p, p, p, p, p, p]),
    "cwfa_footprint_overlaps_f32": (i, [p, p, p, i, p, i64, p, p, p]),
    "cwfa_demix_plan_create": (i, [p, p, i, p, i64, C.POINTER(C.c_void_p)]),
    "cwfa_demix_plan_destroy": (i, [p]),
    "cwfa_demix_coeffs_f64": (i, [p, p, i64, p, p, i, p, p]),
    "cwfa_demix_solve_f64": (i, [p, i64, p, i, i, p, i, d, i, p, p]),
    "cwfa_activity_update_regress_f32": (i, [p, p, p, p, p, p, p, p, i, i, i64, i64, i, p]),
    "cwfa_regress_rows_f64": (i, [p, i, i, p, p, p, i, p]),
    "cwfa_regress_design_f64": (i, [p, p, p, i64, i, d, p, p, p, p]),
    "cwfa_regress_finish_f32": (i, [p, p, p, p, p, p, i64, i, i64, i, p, p, p, p, p]),
}
del i, i64, f, d, p

_lib = None


class CwfaHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CwfaHipError(
                f"{LIB_PATH} not found: build the HIP extension first (python -m cwfa_amd.build, or "
                f"__graft_entry__.build()).  cwfa_amd has no CPU / PyTorch fallback.")
        # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be in the process BEFORE our library so that both bind
        # to the SAME HIP runtime (we launch on torch's streams).  Loaded the other way round the system runtime wins
        # and torch then finds no device.
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError if the symbol is missing -> loud
            fn.restype = res
            fn.argtypes = args
        if h.cwfa_version() < 100:
            raise CwfaHipError("libcwfa_hip.so is older than this Python layer")
        _lib = h
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cwfa_last_error()
        raise CwfaHipError(f"{what or 'libcwfa_hip'} failed (code {rc}): {msg.decode() if msg else ''}")
