"""ctypes binding of libevk.so (include/evk.h).  There is NO fallback: if the HIP library is missing or cannot be
loaded the product fails loudly -- build it with `python -m event_utils_amd.csrc.build` (or __graft_entry__.build())."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_ENV_DATA = getattr(os.environ, "_data", None)     # posix: {bytes: bytes}, the dict behind os.environ (kept in step by setenv / monkeypatch)
_ENV_KEYS = {}


def getenv(name, default):
    """os.environ.get(name, default) without its per-call encode / decode machinery (~0.7 us each, seven of them on the
    path of one public call: with synchronous error reports the host's share of a call is on the critical path)."""
    if _ENV_DATA is None or type(_ENV_DATA) is not dict:
        return os.environ.get(name, default)
    k = _ENV_KEYS.get(name)
    if k is None:
        k = _ENV_KEYS[name] = os.fsencode(name)
    v = _ENV_DATA.get(k)
    return default if v is None else os.fsdecode(v)


LIB_PATH = os.environ.get("EVK_LIB_PATH") or os.path.join(_HERE, "csrc", "libevk.so")   # EVK_LIB_PATH: A/B builds

EVK_IWE_ABS_POLARITY = 1
EVK_IWE_GRADIENT = 2
EVK_IWE_COMPACT = 16
EVK_POST_MIX, EVK_POST_BLUR_IWE, EVK_POST_VALUE, EVK_POST_NONE = 1, 2, 4, 8
EVK_MAX_RADIUS = 32
EVK_VOXEL_OVERWRITE, EVK_VOXEL_SPLIT_POLARITY, EVK_VOXEL_T_FROM_EVENTS = 1, 2, 4
EVK_VOXEL2_PARTITION_ONLY, EVK_VOXEL2_TILES_ONLY, EVK_VOXEL2_NO_XCD_ORDER, EVK_VOXEL2_SHARE_CU = 16, 32, 64, 128
EVK_VOXEL_DETERMINISTIC = 256
EVK_IMAGE2_NO_FIXED = 512
EVK_VOXEL2_REC4, EVK_VOXEL2_REC8, EVK_VOXEL2_NO_COUNT, EVK_VOXEL2_WG512 = 1024, 2048, 4096, 8192
EVK_VOXEL2_LIVE = 16384
EVK_COLUMNS_UNALIGNED = 65536
EVK_VOXEL2_NO_COUNT2 = 32768
EVK_STAGE_SHARE_CU, EVK_STAGE_STATS, EVK_STAGE_COMPACT, EVK_STAGE_LEGACY_SCATTER = 8, 16, 32, 64
EVK_SELECT_I16, EVK_SELECT_I32, EVK_SELECT_I64, EVK_SELECT_F32, EVK_SELECT_F64 = 0, 1, 2, 3, 4
EVK_SELECT_BOX, EVK_SELECT_NOT_HOT, EVK_SELECT_MASK, EVK_SELECT_RANDOM, EVK_SELECT_FLAGS = 0, 1, 2, 3, 4
EVK_DENOISE_MAX_RADIUS, EVK_DENOISE_WAVE_RUN = 3, 4096
EVK_DENOISE_WALK_DEFAULT, EVK_DENOISE_WALK_STREAM, EVK_DENOISE_WALK_PIXEL = 0, 1, 2
EVK_TSURF_MAX_RADIUS = 4
EVK_TSURF_EXP, EVK_TSURF_LINEAR, EVK_TSURF_AGE = 0, 1, 2
EVK_CORNER_BORDER = 4
EVK_CORNER_WINDOW_COUNT, EVK_CORNER_WINDOW_TIME = 0, 1
EVK_PLANEFLOW_MAX_RADIUS, EVK_PLANEFLOW_MAX_ITERATIONS = 4, 8
EVK_RECONSTRUCT_WAVE_RUN = 1024
EVK_SIMULATE_MAX_STEPS = 65536
EVK_EMVS_NEAREST, EVK_EMVS_BILINEAR, EVK_EMVS_BILINEAR_MAX_EVENTS = 0, 1, 1 << 24
EVK_STEREO_MAX_DISPARITIES, EVK_STEREO_MAX_RADIUS = 256, 7
EVK_SGM_MAX_COST, EVK_SGM_MAX_PENALTY, EVK_SGM_AGGREGATE, EVK_SGM_MATCH = 1 << 22, 1 << 20, 0, 1
EVK_TRACK_L2, EVK_TRACK_HUBER, EVK_TRACK_MAX_POSES, EVK_TRACK_SUMS = 0, 1, 16, 29
EVK_TRACK_CONVERGED, EVK_TRACK_STALLED, EVK_TRACK_MAX_EVALS, EVK_TRACK_LOST = 0, 1, 2, 3
EVK_CAMERA_NONE, EVK_CAMERA_RADTAN, EVK_CAMERA_EQUIDISTANT = 0, 1, 2
EVK_CAMERA_FORWARD, EVK_CAMERA_INVERSE = 0, 1
EVK_CAMERA_NEAREST, EVK_CAMERA_SUBPIXEL, EVK_CAMERA_BILINEAR = 0, 1, 1
EVK_CAMERA_U8, EVK_CAMERA_F32, EVK_CAMERA_F64 = 0, 1, 2
EVK_PHILOX_SUBSET, EVK_PHILOX_RANDOM_XY, EVK_PHILOX_RANDOM_TP = 1, 2, 3
EVK_PHILOX_CORR_CHOICE, EVK_PHILOX_CORR_XY, EVK_PHILOX_CORR_T = 4, 5, 6
EVK_T_F32, EVK_T_F64 = 0, 1
EVK_WARP_ROTATION, EVK_WARP_XYZTHETA = 1, 2
EVK_WARP_ANGULAR_VELOCITY, EVK_WARP_PLANAR_FLOW = 3, 4
EVK_IWE_DIRECT = 32
EVK_WARP_LINVEL = 0        # the linear flow in the entries that take it (evk_tsimg_warp_*, evk_tsobj_grad_*)
EVK_FLOWTS_FORWARD, EVK_FLOWTS_BACKWARD = 0, 1
EVK_FLOWCM_ABS = 1
EVK_FLOWCM_VARIANCE, EVK_FLOWCM_MEAN_SQUARE = 0, 1
EVK_SEG_MAX_CLUSTERS, EVK_SEG_POLARITY = 8, 1
EVK_G_IDENT, EVK_G_EXP, EVK_G_STEP, EVK_G_EXPNEG = 0, 1, 2, 3
EVK_P_U8_PM1, EVK_P_U8, EVK_P_I8, EVK_P_F32 = 0, 1, 2, 3
EVK_RAW_EVT3, EVK_RAW_EVT2, EVK_RAW_TS_US, EVK_RAW_TS_SECONDS = 3, 2, 0, 1
EVK_RAW_CHUNK, EVK_RAW_SCAN_WIDTH, EVK_RAW_DIRECT_STORES = 4096, 256, 1

P = c_void_p  # every device / host pointer crosses as void*

# evk_seg_*: model, the four columns, n, t_ref, host_params, L, probs, bounds, canvas, flags
_SEG_HEAD = [c_int, P, P, P, P, c_int64, c_double, P, c_int, P, c_double, c_double, c_int, c_int, c_uint32]

# name -> argtypes (restype is int unless noted); mirrors include/evk.h one-to-one
SIGNATURES = {
    "evk_image_nearest_i32": [P, P, P, c_int64, c_int, c_int, P, P, P],
    "evk_image_nearest_f64": [P, P, P, c_int64, c_int, c_int, P, P, P],
    "evk_image_nearest_f32": [P, P, P, c_int64, c_int, c_int, c_float, c_float, P, P, P],
    "evk_image_bilinear_f32": [P, P, P, c_int64, c_int, c_int, c_float, c_float, P, P, P],
    "evk_splat_indexed_f32": [P, P, P, P, P, c_int64, c_int, c_int, P, P, P],
    "evk_splat_drv_indexed_f32": [P, P, P, P, P, P, c_int, c_int64, c_int, c_int, P, P, P],
    "evk_image_drv_f64": [P, P, P, P, P, c_int64, c_int, c_int, c_float, c_float, P, P, P, P],
    "evk_image_gather_bilinear_f64": [P, P, c_int64, P, c_int, c_int, P, P, P],
    "evk_image_gather_bilinear_f64img": [P, P, c_int64, P, c_int, c_int, P, P, P],
    "evk_timestamp_images_f32": [P, P, P, P, c_int64, c_int, c_int, c_float, c_float, c_int, c_float, c_float, P, P, P],
    "evk_voxel_f32": [P, P, P, P, c_int64, c_float, c_float, c_int, c_int, c_int, P, P, P],
    "evk_voxel_from_events_f32": [P, P, P, P, c_int64, c_int, c_int, c_int, P, P, P],
    "evk_voxel_segments_f32": [P, P, P, P, P, c_int, c_int64, c_int, c_int, c_int, P, P, P],
    "evk_voxel_f64": [P, P, P, P, c_int64, c_double, c_double, c_int, c_int, c_int, P, P, P],
    "evk_warp_linvel_f64": [P, P, P, c_int64, c_double, c_double, c_double, P, P, P, P, P],
    "evk_warp_flow_field_f32": [P, P, P, c_int64, P, c_int, c_int, c_float, P, P, P],
    "evk_bounds_mask_f64": [P, P, c_int64, c_double, c_double, c_double, c_double, P, P],
    "evk_iwe_linvel_f32": [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, c_double, c_int, c_int,
                           c_uint32, c_double, P, P, P],
    "evk_iwe_linvel_f64": [P, P, P, P, c_int64, c_double, c_double, c_double, c_double, c_double, c_int, c_int,
                           c_uint32, c_double, P, P, P],
    "evk_gaussian_filter_f32": [P, P, P, c_int, P, P, c_int, P],
    "evk_gaussian_filter_wide_f32": [P, P, P, c_int, P, P, c_int, P],
    "evk_variance_f32": [P, c_int64, P, P, c_int64, P],
    "evk_variance_grad_f32": [P, P, c_int64, P, P, c_int64, P],
    "evk_objective_variance_f32": [P, c_int, c_int, P, c_int, P, P, c_int64, P],
    "evk_objective_variance_grad_f32": [P, P, c_int, c_int, P, c_int, c_uint32, P, P, c_int64, P],
    "evk_cmax_variance_tiled_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_int, c_int, c_uint32, c_double, c_double, c_double, P, c_int,
                                    c_uint32, P, c_int64, P, P, P, c_int64, P, c_int, P, P],
    "evk_cmax_bfgs_variance_tiled_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_double, c_double, c_double, c_double,
                                         c_int, c_int, c_uint32, c_double, c_double, c_double, P, c_int, c_uint32, P, c_int64,
                                         P, P, P, c_int64, P, P, P, P, P, c_int, P],
    "evk_bfgs2_minimize": [P, P, P, P, P, P, c_int],
    "evk_iwe_linvel_tiled_batch3_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double,
                                        c_double, P, P, c_double, c_double, c_int, c_int, c_uint32, c_double, c_double,
                                        c_double, P, c_int64, P, P],
    "evk_objective_variance_planes_f32": [P, c_int, c_int, c_int, P, c_int, P, P, c_int64, P],
    "evk_cmax_variance_batch3_tiled_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double,
                                           c_double, P, P, c_double, c_double, c_int, c_int, c_uint32, c_double, c_double,
                                           c_double, P, c_int, P, c_int64, P, P, P, c_int64, P, c_int, P, P],
    "evk_objective_stats_f32": [P, c_int, c_int, P, c_int, c_double, c_double, P, P, c_int64, P],
    "evk_objective_variance_fg_f32": [P, P, c_int, c_int, P, c_int, c_uint32, P, P, c_int64, P],
    "evk_objective_gradsums_f32": [P, P, c_int, c_int, P, c_int, c_uint32, c_int, c_double, P, P, c_int64, P],
    "evk_spectral_norm_sq_f32": [P, c_int, c_int, P, P, c_int64, P],
    "evk_timestamp_image_add_f64": [P, P, P, c_int64, c_int, c_int, P, P, P, P],
    "evk_event_image_add_f64": [P, P, P, c_int64, c_int, c_int, P, P, P],
    "evk_dense_rank_f64": [P, c_int64, P, P, c_int64, P],
    "evk_minmax_normalise_f64": [P, c_int64, P, P, P],
    "evk_polarity_weights_f32": [P, c_int64, P, P, P],
    "evk_narrow_f64_f32": [P, c_int64, c_double, P, P, P],
    "evk_abs_max": [P, c_int, c_int64, P, P],
    "evk_searchsorted_left": [P, c_int, c_int64, P, c_int64, P, P],
    "evk_timestamp_planes_init_f32": [P, c_int64, P],
    "evk_timestamp_finalise_f32": [P, c_int64, P, P, P],
    "evk_abs": [P, c_int, c_int64, P, P],
    "evk_bucket_num_tiles": [c_int, c_int, c_int, c_int],
    "evk_bucket_events_f32": [P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int64, P, c_int, P],
    "evk_bucket_events_native_f32": [P, P, c_int, P, c_int, c_double, P, c_int, c_int64, c_int, c_int, c_int, c_int, c_int,
                                     P, P, P, c_int64, P, c_int, P],
    "evk_native_to_columns_f32": [P, P, c_int, P, c_int, c_double, P, c_int, c_int64, P, P, P, P, P],
    "evk_voxel_tiled_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, P, P, c_int64, P],
    "evk_voxel2_f32": [P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, P, P, P, c_int64,
                       P, P, c_uint32, P],
    "evk_voxel2_native_f32": [P, P, c_int, P, c_int, c_double, P, c_int, c_int64, c_int, c_int, c_int, c_int, c_float,
                              c_float, c_int, c_int, P, P, P, c_int64, P, P, c_uint32, P],
    "evk_normalise_time_f32": [P, c_int64, c_float, c_float, c_int, P, P],
    "evk_voxel2_band_f32": [c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int64, P],
    "evk_image2_nearest_i32": [P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int64, P, P, c_uint32, P],
    "evk_image2_nearest_f32": [P, P, P, c_int64, c_int, c_int, c_float, c_float, c_int, c_int, c_int, P, P, P, c_int64, P, P,
                               c_uint32, P],
    "evk_image2_bilinear_f32": [P, P, P, c_int64, c_int, c_int, c_float, c_float, c_int, c_int, c_int, P, P, P, c_int64, P, P,
                                c_uint32, P],
    "evk_image2_splat_indexed_f32": [P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int64, P, P, c_uint32, P],
    "evk_image2_splat_drv_indexed_f32": [P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int64, P, P, c_uint32,
                                         P],
    "evk_image2_drv_f64": [P, P, P, P, P, c_int64, c_int, c_int, c_float, c_float, c_int, c_int, c_int, P, P, P, P, c_int64, P, P,
                           c_uint32, P],
    "evk_timestamp_images2_f32": [P, P, P, P, c_int64, c_int, c_int, c_float, c_float, c_int, c_float, c_float, c_int, c_int,
                                  c_int, P, P, P, c_int64, P, P, c_uint32, P],
    "evk_comm_unique_id": [P],
    "evk_comm_init": [P, c_int, c_int, P],
    "evk_comm_destroy": [P],
    "evk_objective_variance_rows_f32": [P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_uint32, P, P, c_int64, P],
    "evk_compact_records_f32": [P, c_int64, c_int, c_int, c_int, c_int, P, P, P],
    "evk_allreduce_f32": [P, c_int64, P, P],
    "evk_allreduce_i32": [P, c_int64, P, P],
    "evk_select_compact": [c_int, c_int, P, P, c_int64, P, P, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int64, P, P],
    "evk_select_to_i32": [c_int, P, c_int64, P, P, P],
    "evk_hot_pixels": [P, c_int, c_int, c_int, c_int, c_int64, P, P, c_int64, P],
    "evk_mask_multiply_f64": [c_int, P, c_int64, c_double, P, P, P],
    "evk_random_subset": [c_uint64, c_uint32, c_int64, c_int64, P, c_int64, P],
    "evk_denoise_group": [P, P, P, c_int64, c_int, c_int, c_int, P, c_int64, P, P],
    "evk_denoise_support": [c_int, P, c_int64, c_int, c_int, c_int, c_double, c_int, c_int, c_int, c_int, P, P, P, P],
    "evk_denoise_refractory": [c_int, P, c_int64, c_int, c_int, c_int, c_double, c_int, P, P, P],
    "evk_tsurf_check_sorted": [c_int, P, c_int64, P, P],
    "evk_tsurf_global": [c_int, P, c_int64, c_int, c_int, c_int, c_int64, P, P, c_int, c_double, P, P, P],
    "evk_tsurf_local": [c_int, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_double, c_int, c_int, P, c_int64, P, P, P],
    "evk_tsurf_hats": [c_int, P, c_int64, c_int, c_int, c_int, c_int, c_double, c_double, c_int, P, P, c_int64, P, P, P],
    "evk_corner_fast": [c_int, P, c_int64, c_int, c_int, c_int, P, c_int64, P, P, P],
    "evk_corner_harris": [c_int, P, c_int64, c_int, c_int, c_int, c_int, c_int64, c_double, c_double, P, c_int64, P, P, P],
    "evk_planeflow_fit": [c_int, P, c_int64, c_int, c_int, c_int, c_int, c_double, c_int, c_int, c_double, c_int, c_int, c_double, P,
                          c_int64, P, P, P, P, P],
    "evk_planeflow_field": [c_int64, c_int, c_int, c_int, P, P, P, P, P, P],
    "evk_reconstruct": [c_int, P, P, c_int64, c_int, c_int, c_double, c_double, c_double, c_double, P, c_int, P, P, c_int64, P, P,
                        c_int64, c_int, P, P, P],
    "evk_simulate_count": [P, P, c_int, c_int, c_int, c_double, c_double, P, P, c_double, P, P, P, P, P],
    "evk_simulate_emit": [P, P, c_int, c_int, c_int, c_double, c_double, P, P, c_double, P, P, P, c_int64, c_double, c_int, P, P, P, P,
                          P],
    "evk_simulate_sort": [P, P, c_int64, c_int, c_int, c_int, c_double, c_double, P, c_int64, P, P, P, P, P],
    "evk_emvs_packet_times": [c_int, P, c_int64, c_int64, P, P],
    "evk_emvs_band_rows": [c_int, c_int],
    "evk_emvs_band_cols": [c_int, c_int],
    "evk_emvs_chunks": [c_int64, c_int, c_int, c_int],
    "evk_emvs_votes": [c_int, P, P, c_int64, c_int64, P, c_int64, P, P, c_int, c_double, c_double, c_double, c_double, c_int, c_int,
                       c_int, c_int, P, P, P],
    "evk_emvs_depth_map": [P, P, c_int, c_int, c_int, c_int, c_int64, c_int, P, P, P, P, P, P],
    "evk_stereo_quantise": [P, c_int64, c_double, P, P],
    "evk_stereo_cost_volume": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "evk_stereo_match": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_int, P, P, P, P, P, P],
    "evk_sgm_aggregate": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P],
    "evk_sgm_match_volume": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int, c_int, P, P, P, P, P, P],
    "evk_track_terms": [P, c_int64, P, c_int, c_int, c_double, c_double, c_double, c_double, P, c_int, c_int, c_double, P, P, P],
    "evk_track_residuals": [P, c_int64, P, c_int, c_int, c_double, c_double, c_double, c_double, P, P, P, P, P],
    "evk_track_register": [P, c_int64, P, c_int, c_int, c_double, c_double, c_double, c_double, P, c_int, c_double, c_int, c_int64, c_double,
                           P, P, P, P, P, P],
    "evk_camera_points": [c_int, c_int, P, c_int64, c_int, c_int, P, c_int, c_double, P, P, P],
    "evk_camera_rectify_lookup": [c_int, P, P, c_int64, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P],
    "evk_camera_remap": [P, c_int, c_int64, c_int, c_int, P, P, c_int, c_int, c_int, c_double, P, P],
    "evk_raw_decode_plan": [P, c_int64, c_int, P, P, c_int64, P, P, P],
    "evk_raw_decode_write": [P, c_int64, c_int, P, c_int64, P, P, P, P, P, c_int, c_int, c_int, c_uint32, P],
    "evk_philox4x32": [c_uint64, c_uint32, c_uint64, c_int64, P, P],
    "evk_augment_bounds": [c_int, P, c_int, P, c_int, P, c_int64, P, P, c_int64, P],
    "evk_random_events": [c_uint64, P, c_int64, c_int, P, P, P, P, P],
    "evk_correlated_events": [c_uint64, P, P, P, P, c_int64, P, c_int64, c_double, c_double, P, P, P, P, P, P],
    "evk_sort_events_f64": [P, P, P, P, c_int64, P, P, P, P, P, c_int64, P, P],
    "evk_iwe_linvel_tiled_f32": [P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_double,
                                 c_double, c_double, c_double, c_int, c_int, c_uint32, c_double, c_double, c_double, P, c_int64,
                                 P, P, P],
    "evk_voxel_windows_f32": [P, P, c_int, c_int, P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, P, P],
    "evk_pack_window_events_f32": [P, P, c_int, c_int, P, c_int, P, c_int, P, P, c_int, P, P],
    "evk_robust_norm_f32": [P, c_int64, c_int64, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, P, P, P],
    "evk_warp_param_f64": [c_int, P, P, P, c_int64, c_double, P, P, P, P, P, P],
    "evk_iwe_param_f32": [c_int, P, P, P, P, c_int64, c_double, P, c_double, c_double, c_int, c_int, c_uint32, c_double, P, P, P],
    "evk_iwe_param_f64": [c_int, P, P, P, P, c_int64, c_double, P, c_double, c_double, c_int, c_int, c_uint32, c_double, P, P, P],
    "evk_objective_gradsums_planes_f32": [P, P, c_int, c_int, c_int, c_int, c_double, P, P, c_int64, P],
    "evk_tsimg_warp_f32": [c_int, P, P, P, P, c_int64, c_double, c_double, c_double, P, c_double, c_double, c_int, c_int, c_uint32,
                           P, P, P],
    "evk_tsimg_warp_f64": [c_int, P, P, P, P, c_int64, c_double, c_double, c_double, P, c_double, c_double, c_int, c_int, c_uint32,
                           P, P, P],
    "evk_tsimg_average_f32": [P, c_int, c_int, P, P],
    "evk_tsobj_post_f32": [P, c_int, c_int, P, P, c_int, P, P, P, P, c_int64, P],
    "evk_tsobj_grad_f32": [c_int, P, P, P, P, c_int64, c_double, c_double, c_double, P, c_double, c_double, c_int, c_int, P, P, P,
                           c_int64, P],
    "evk_tsobj_grad_f64": [c_int, P, P, P, P, c_int64, c_double, c_double, c_double, P, c_double, c_double, c_int, c_int, P, P, P,
                           c_int64, P],
    "evk_flowts_time_constants_f32": [P, P, c_int, c_int64, c_int, P, P],
    "evk_flowts_warp_f32": [P, P, P, P, P, c_int, c_int64, P, c_int, c_int, P, P, P, P],
    "evk_flowts_grad_f32": [P, P, P, P, P, c_int, c_int64, P, c_int, c_int, P, P, P, P, P, P],
    "evk_flowcm_warp_f32": [P, P, P, P, P, c_int, c_int64, P, c_int, c_int, P, c_double, c_uint32, P, P, P, P],
    "evk_flowcm_post_f32": [P, c_int, c_int, P, P, c_int, c_int, P, P, P, P, c_int64, P],
    "evk_flowcm_grad_f32": [P, P, P, P, P, c_int, c_int64, P, c_int, c_int, P, c_double, c_uint32, P, P, P, P, P, P],
    "evk_seg_splat_f32": _SEG_HEAD + [P, P, P],
    "evk_seg_splat_f64": _SEG_HEAD + [P, P, P],
    "evk_seg_grad_f32": _SEG_HEAD + [P, P, P, c_int64, P],
    "evk_seg_grad_f64": _SEG_HEAD + [P, P, P, c_int64, P],
    "evk_seg_assign_f32": _SEG_HEAD + [P, P, P, P],
    "evk_seg_assign_f64": _SEG_HEAD + [P, P, P, P],
}
_SPECIAL = {
    "evk_version": ([], c_int),
    "evk_error_string": ([c_int], c_char_p),
    "evk_reduce_scratch_bytes": ([], c_int64),
    "evk_bucket_scratch_bytes": ([c_int], c_int64),
    "evk_compact_records_bytes": ([c_int64], c_int64),
    "evk_iwe_tiled_staging_bytes": ([c_int, c_int64, c_int, c_int, c_int, c_int], c_int64),
    "evk_voxel_tiled_staging_bytes": ([c_int, c_int64, c_int, c_int, c_int], c_int64),
    "evk_bucket_index_len": ([c_int, c_int64], c_int64),
    "evk_bucket_max_items": ([c_int, c_int64], c_int),
    "evk_comm_unique_id_bytes": ([], c_int),
    "evk_voxel2_max_tiles": ([], c_int),
    "evk_voxel2_index_len": ([c_int, c_int64], c_int64),
    "evk_voxel2_scratch_bytes": ([c_int, c_int64, c_int, c_int, c_int], c_int64),
    "evk_voxel2_num_tiles": ([c_int, c_int, c_int, c_int], c_int),
    "evk_voxel2_fits": ([c_int, c_int, c_int, c_int, c_int], c_int),
    "evk_num_cu": ([], c_int),
    "evk_image2_scratch_bytes": ([c_int, c_int64, c_int, c_int], c_int64),
    "evk_timestamp_images2_scratch_bytes": ([c_int, c_int64, c_int, c_int], c_int64),
    "evk_image2_indexed_scratch_bytes": ([c_int, c_int64, c_int, c_int], c_int64),
    "evk_dense_rank_scratch_bytes": ([c_int64], c_int64),
    "evk_spectral_scratch_bytes": ([c_int, c_int], c_int64),
    "evk_minmax_scratch_bytes": ([], c_int64),
    "evk_select_scratch_bytes": ([c_int64], c_int64),
    "evk_hot_pixels_scratch_bytes": ([], c_int64),
    "evk_denoise_scratch_bytes": ([c_int64, c_int, c_int, c_int], c_int64),
    "evk_tsurf_scratch_bytes": ([c_int64], c_int64),
    "evk_stereo_scratch_bytes": ([c_int, c_int, c_int, c_int], c_int64),
    "evk_sgm_scratch_bytes": ([c_int, c_int, c_int, c_int, c_int], c_int64),
    "evk_track_scratch_bytes": ([c_int64, c_int], c_int64),
    "evk_raw_decode_scratch_bytes": ([c_int64], c_int64),
    "evk_augment_bounds_scratch_bytes": ([], c_int64),
    "evk_sort_events_scratch_bytes": ([c_int64], c_int64),
    "evk_simulate_sort_scratch_bytes": ([c_int64, c_int, c_int, c_int, c_double, c_double], c_int64),
    "evk_iwe_param_band_rows": ([c_int, c_uint32, c_int, c_int], c_int),
    "evk_tsimg_band_rows": ([c_uint32, c_int, c_int], c_int),
    "evk_seg_band_rows": ([c_int, c_uint32, c_int, c_int], c_int),
    "evk_seg_grad_scratch_bytes": ([], c_int64),
}


class EvkError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library (loads on first use; raises if it is not built -- never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise EvkError("libevk.so is not built (%s missing): run `python -m event_utils_amd.csrc.build`; "
                           "event_utils_amd has no CPU fallback" % LIB_PATH)
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise EvkError("cannot load %s: %s" % (LIB_PATH, e))
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_int
        for name, (argtypes, restype) in _SPECIAL.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().evk_error_string(rc)
        raise EvkError("%s failed: %s (code %d)" % (what or "evk call", msg.decode() if msg else "?", rc))


def call(name, *args):
    check(getattr(lib(), name)(*args), name)
