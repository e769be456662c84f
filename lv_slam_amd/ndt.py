"""Host-side mirror of the reference registration interface over the C-ABI (include/mi355_ndt.h).

`NormalDistributionsTransform` keeps the method names, argument meaning and error behaviour of
pclomp::/pclpca::NormalDistributionsTransform (include/ndt_omp/ndt_omp.h:69-277,
include/ndt_pca/ndt_pca.h) and of the pcl::Registration base it derives from, so a user of
lv_slam's `reg.setInputTarget(..); reg.setInputSource(..); reg.align(out, guess)` sequence
(src/lidar_odometry/scan_matching_odom_nodelet.cpp:109-119,197,220-226) finds the same surface.
All computation happens in libmi355ndt.so (hand-written HIP, gfx950).  There is no CPU fallback:
loading fails loudly if the library is missing, construction fails if no GPU is usable.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI355NDT_LIB: another build of the same library (A/B runs of kernel variants)
LIB_PATH = os.environ.get("MI355NDT_LIB") or os.path.join(_HERE, "libmi355ndt.so")

# pclomp::NeighborSearchMethod (include/ndt_omp/ndt_omp.h:51-56)
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
VARIANT_OMP, VARIANT_PCA = 0, 1

OK = 0
ERR = {-1: "bad handle", -2: "bad argument", -3: "HIP error", -4: "target grid unusable", -5: "no HIP device",
       -6: "unsupported configuration", -7: "target/source not set"}


class NDTError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {ERR.get(code, code)}" + (f" ({detail})" if detail else ""))


class Params(C.Structure):
    _fields_ = [("resolution", C.c_float), ("step_size", C.c_double), ("outlier_ratio", C.c_double),
                ("trans_epsilon", C.c_double), ("max_iterations", C.c_int), ("neighbor_mode", C.c_int),
                ("variant", C.c_int), ("min_points_per_voxel", C.c_int), ("min_covar_eigvalue_mult", C.c_double)]


class Result(C.Structure):
    _fields_ = [("final_colmajor", C.c_float * 16), ("trans_probability", C.c_double), ("score", C.c_double),
                ("iterations", C.c_int), ("converged", C.c_int), ("sweeps", C.c_int), ("status", C.c_int),
                ("hits_last", C.c_longlong)]


class Voxel(C.Structure):
    _fields_ = [("idx", C.c_int32), ("n", C.c_int32), ("mean", C.c_double * 3), ("icov", C.c_float * 9),
                ("weight", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("sweep_ms", C.c_double), ("sweep_launches", C.c_longlong), ("sweep_alg_bytes", C.c_double),
                ("sweep_hits", C.c_longlong), ("sweep_points", C.c_longlong), ("build_ms", C.c_double),
                ("build_launches", C.c_longlong), ("build_alg_bytes", C.c_double), ("update_ms", C.c_double),
                ("update_launches", C.c_longlong), ("async_fallbacks", C.c_longlong), ("stream_launches", C.c_longlong),
                ("stream_carried", C.c_longlong), ("stream_redone", C.c_longlong), ("cloud_uploads", C.c_longlong), ("cloud_upload_bytes", C.c_longlong),
                ("cloud_transfers", C.c_longlong), ("cloud_promotions", C.c_longlong),
                ("stream_reserved_slots", C.c_longlong), ("stream_launch_slots", C.c_longlong), ("score_only_sweeps", C.c_longlong),
                ("async_waves_per_simd", C.c_longlong), ("async_launch_slots", C.c_longlong)]


class InfParams(C.Structure):
    """mi355ndt_inf_params: the parameters of InformationMatrixCalculator (information_matrix_calculator.cpp:11-20)."""
    _fields_ = [("use_const_inf_matrix", C.c_int), ("const_stddev_x", C.c_double), ("const_stddev_q", C.c_double), ("var_gain_a", C.c_double),
                ("min_stddev_x", C.c_double), ("max_stddev_x", C.c_double), ("min_stddev_q", C.c_double), ("max_stddev_q", C.c_double),
                ("fitness_score_thresh", C.c_double)]


class OutlierParams(C.Structure):
    _fields_ = [("method", C.c_int), ("mean_k", C.c_int), ("stddev_mul", C.c_double), ("radius", C.c_double), ("min_neighbors", C.c_int)]


class OutlierStats(C.Structure):
    _fields_ = [("n_in", C.c_longlong), ("n_valid", C.c_longlong), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double)]


class GicpParams(C.Structure):
    """mi355ndt_gicp_params: pclomp::GeneralizedIterativeClosestPoint's parameters (gicp_omp.h:110-120)."""
    _fields_ = [("k_correspondences", C.c_int), ("gicp_epsilon", C.c_double), ("rotation_epsilon", C.c_double), ("transformation_epsilon", C.c_double),
                ("max_iterations", C.c_int), ("max_inner_iterations", C.c_int), ("corr_dist_threshold", C.c_double)]


class GicpResult(C.Structure):
    _fields_ = [("final_colmajor", C.c_float * 16), ("converged", C.c_int), ("iterations", C.c_int), ("inner_status", C.c_int), ("n_matched", C.c_int),
                ("delta", C.c_double)]


class IcpParams(C.Structure):
    """mi355ndt_icp_params: pcl::IterativeClosestPoint's parameters (pcl::Registration's constructor values)."""
    _fields_ = [("transformation_epsilon", C.c_double), ("max_iterations", C.c_int), ("euclidean_fitness_epsilon", C.c_double),
                ("corr_dist_threshold", C.c_double), ("min_number_correspondences", C.c_int), ("use_reciprocal_correspondences", C.c_int)]


class KnnParams(C.Structure):
    """mi355ndt_knn_params: k (1 .. 64), max_range (kept iff (double)d2 <= max_range^2; +inf: no limit), query_order (KNN_ORDER_*)."""
    _fields_ = [("k", C.c_int), ("max_range", C.c_double), ("query_order", C.c_int)]


class IcpResult(C.Structure):
    _fields_ = [("final_colmajor", C.c_float * 16), ("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("matches", C.c_int),
                ("mse", C.c_double)]


class PrefilterParams(C.Structure):
    """mi355ndt_prefilter_params: PrefilteringNodelet's distance filter, VoxelGrid leaf and base_link move (`extended` lies where the
    compiler's padding lay: the layout is what it was)."""
    _fields_ = [("use_distance_filter", C.c_int), ("extended", C.c_int), ("distance_near", C.c_double), ("distance_far", C.c_double),
                ("downsample_resolution", C.c_float), ("use_transform", C.c_int), ("transform_colmajor", C.c_float * 16)]


class PrefilterParamsEx(C.Structure):
    """mi355ndt_prefilter_params_ex: the nodelet's down-sampling method and vertical-angle calibration behind a PrefilterParams whose
    `extended` says so; every call that takes a PrefilterParams pointer takes byref(ex.base)."""
    _fields_ = [("base", PrefilterParams), ("downsample_method", C.c_int), ("use_angle_calibration", C.c_int), ("angle_calibration_rad", C.c_double)]


class PrefilterParamsEx2(C.Structure):
    """mi355ndt_prefilter_params_ex2: the byte offset of the records' intensity behind a PrefilterParamsEx whose base.extended says so
    (PREFILTER_EXTENDED2); every call that takes a PrefilterParams pointer takes byref(ex2.ex.base)."""
    _fields_ = [("ex", PrefilterParamsEx), ("intensity_offset_bytes", C.c_int), ("reserved", C.c_int)]


class SeqParams(C.Structure):
    _fields_ = [("keyframe_delta_trans", C.c_double), ("keyframe_delta_angle", C.c_double), ("keyframe_delta_time", C.c_double)]


class SeqFrame(C.Structure):
    _fields_ = [("odom_colmajor", C.c_double * 16), ("tf_s2k_colmajor", C.c_float * 16), ("trans_probability", C.c_double),
                ("dx", C.c_double), ("da", C.c_double), ("dt", C.c_double), ("key_id", C.c_int), ("new_keyframe", C.c_int),
                ("iterations", C.c_int), ("converged", C.c_int), ("aligns", C.c_int), ("pad", C.c_int)]


class SeqStats(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("build_ms", C.c_double), ("track_ms", C.c_double), ("aligns", C.c_longlong),
                ("update_launches", C.c_longlong)]


# every symbol include/mi355_ndt.h declares
SYMBOLS = [
    "mi355ndt_version", "mi355ndt_device_count", "mi355ndt_host_numa_node", "mi355ndt_default_params", "mi355ndt_create", "mi355ndt_destroy",
    "mi355ndt_set_params", "mi355ndt_get_params", "mi355ndt_set_stream", "mi355ndt_last_error",
    "mi355ndt_set_target", "mi355ndt_set_source", "mi355ndt_promote_source_to_target", "mi355ndt_align", "mi355ndt_get_aligned", "mi355ndt_get_incremental",
    "mi355ndt_get_partial_rows",
    "mi355ndt_get_fitness_score", "mi355ndt_fitness_score_T", "mi355ndt_prefilter", "mi355ndt_use_prefiltered", "mi355ndt_derivatives", "mi355ndt_compute_hessian", "mi355ndt_derivatives_T", "mi355ndt_get_grid", "mi355ndt_get_voxels", "mi355ndt_get_build_buffer",
    "mi355ndt_batch_reserve", "mi355ndt_batch_set_target", "mi355ndt_batch_set_source", "mi355ndt_batch_set_clouds", "mi355ndt_batch_bind_device",
    "mi355ndt_batch_build_targets", "mi355ndt_batch_align", "mi355ndt_batch_size", "mi355ndt_batch_pose_records", "mi355ndt_batch_fitness_scores",
    "mi355ndt_profile_enable", "mi355ndt_profile_reset", "mi355ndt_profile_get", "mi355ndt_synchronize",
    "mi355ndt_set_latency_mode", "mi355ndt_sequence_run",
    "mi355ndt_calculate_score", "mi355ndt_convert_transform", "mi355ndt_set_option", "mi355ndt_get_option",
    "mi355ndt_stream_begin", "mi355ndt_stream_submit", "mi355ndt_stream_submit_host", "mi355ndt_stream_collect", "mi355ndt_stream_end", "mi355ndt_stream_pose_records", "mi355ndt_pack_pose_records",
    "mi355ndt_map_cloud",
    "mi355ndt_window_keyframe", "mi355ndt_keyframe_add", "mi355ndt_keyframe_get", "mi355ndt_keyframe_release", "mi355ndt_keyframe_count",
    "mi355ndt_map_cloud_keyframes", "mi355ndt_batch_set_target_keyframe", "mi355ndt_batch_set_source_keyframe",
    "mi355ndt_keyframe_fitness_scores", "mi355ndt_inf_params_default", "mi355ndt_information_matrix",
    "mi355ndt_outlier_params_default", "mi355ndt_prefilter_outliers", "mi355ndt_batch_remove_outliers", "mi355ndt_sequence_run_raw_outliers",
    "mi355ndt_prefilter_params_default", "mi355ndt_batch_prefilter", "mi355ndt_batch_get_cloud", "mi355ndt_sequence_run_raw",
    "mi355ndt_prefilter_p", "mi355ndt_prefilter_params_ex_default",
    "mi355ndt_prefilter_params_ex2_default", "mi355ndt_batch_get_cloud_i",
    "mi355ndt_keyframe_from_prefiltered", "mi355ndt_keyframe_from_slot", "mi355ndt_window_keyframe_ids",
    "mi355ndt_gicp_params_default", "mi355ndt_gicp_set_params", "mi355ndt_gicp_set_target", "mi355ndt_gicp_set_source", "mi355ndt_gicp_set_target_keyframe",
    "mi355ndt_gicp_set_source_keyframe", "mi355ndt_gicp_covariances", "mi355ndt_gicp_correspondences", "mi355ndt_gicp_cost", "mi355ndt_gicp_align",
    "mi355ndt_gicp_get_aligned",
    "mi355ndt_gicp_batch_reserve", "mi355ndt_gicp_batch_set_source", "mi355ndt_gicp_batch_set_source_keyframe", "mi355ndt_gicp_batch_align",
    "mi355ndt_gicp_batch_get_aligned", "mi355ndt_gicp_batch_stats",
    "mi355ndt_icp_params_default", "mi355ndt_icp_set_params", "mi355ndt_icp_set_target", "mi355ndt_icp_set_source", "mi355ndt_icp_set_target_keyframe",
    "mi355ndt_icp_set_source_keyframe", "mi355ndt_icp_correspondences", "mi355ndt_icp_align", "mi355ndt_icp_get_aligned",
    "mi355ndt_icp_batch_reserve", "mi355ndt_icp_batch_set_source", "mi355ndt_icp_batch_set_source_keyframe", "mi355ndt_icp_batch_align",
    "mi355ndt_icp_batch_get_aligned", "mi355ndt_icp_batch_stats",
    "mi355ndt_knn_params_default", "mi355ndt_keyframe_knn", "mi355ndt_keyframe_knn_ids", "mi355ndt_keyframe_radius_search",
    "mi355ndt_batch_score_poses",
]
SCORE_POSES_MAX_ITEMS = 65536  # MI355NDT_SCORE_POSES_MAX_ITEMS: items of one mi355ndt_batch_score_poses
KNN_ORDER_AUTO, KNN_ORDER_INPUT, KNN_ORDER_CELL = 0, 1, 2   # MI355NDT_KNN_ORDER_*: how keyframe_knn deals its queries to the lanes; no result word depends on it
KNN_MAX_K = 64                 # MI355NDT_KNN_MAX_K
ICP_BATCH_MAX = 64             # MI355NDT_ICP_BATCH_MAX: slots of one mi355ndt_icp_batch_align
ICP_STATES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES"]   # mi355ndt_icp_state
GICP_BATCH_MAX = 64            # MI355NDT_GICP_BATCH_MAX: slots of one mi355ndt_gicp_batch_align
GICP_TARGET, GICP_SOURCE = 0, 1  # mi355ndt_gicp_covariances' role
OPT_ASYNC_ALIGN = 2            # mi355ndt_option: 1 (default) = one persistent launch per batch align, 0 = lockstep (update, sweep) rounds; same bits
OPT_DEBUG_ASYNC_ABORT = 3      # mi355ndt_option (test hook): the wave that claims this position of ring 0 gives up -> the batch is re-run in rounds
OPT_DEBUG_ASYNC_RINGS = 6      # mi355ndt_option (test hook): bit x clear -> ring x of a one-launch align has no workgroups of its own
OPT_STREAM_RESERVE = 5         # mi355ndt_option: workgroup slots the stream's launches leave free for the next batch's build (0 = off)
OPT_STREAM_THRESHOLD = 4       # mi355ndt_option: pairs a stream launch hands over to the next one (-1 = auto, 0 = none)
WARN_TOLERANCE_ARITH = 1       # mi355ndt_result.status under OPT_ARITH = 1: fewer than 4,096 hits at the final pose, or stopped at the iteration cap
OPT_ARITH = 7                  # mi355ndt_option: 0 = the reference recipe's arithmetic, one rounding per operation (default), 1 = tolerance arithmetic (held to 1e-4 m / 1e-5 rad, not to bits)
OPT_SWEEP_WAVES = 14           # mi355ndt_option: waves per SIMD of the exact ndt_omp / DIRECT7 body in the one-launch align: 0 = automatic (default), 2, 3 (the lean body); no result word depends on it
OPT_F32_SUM_ORDER = 1          # mi355ndt_option: 0 = (t0 + t1) + t2 (canonical), 1 = (t0 + t2) + t1 (Eigen 3.3 SSE predux pairing)
OPT_SCORE_ONLY_LAST_SWEEP = 8  # mi355ndt_option: 1 (default) = the one-launch align's last sweep of a pair evaluates the score alone, 0 = all 43 sums; same bits
OPT_KF_FITNESS_CELL_MM = 9     # mi355ndt_option: cell size [mm] of the index keyframe_fitness_scores builds over a searched keyframe (default 100); no result bit depends on it
OPT_OUTLIER_CELL_MM = 10       # mi355ndt_option: cell size [mm] of the index prefilter_outliers builds over the prefilter result in every call (default 100); no result bit depends on it
OPT_PREFILTER_GROUP = 11      # mi355ndt_option: raw clouds per group of batch_prefilter (0, the default: by the engine's scratch budget); no result word depends on it
OPT_POSE_MODEL = 12           # mi355ndt_option: 0 (default) = ndt_omp_impl2.hpp, the SE(3) tangent; 1 = ndt_omp_impl.hpp, the Euler-angle pose model (lockstep rounds, ndt_omp, dead More-Thuente)
POSE_MODELS = {"se3": 0, "euler": 1}
OPT_NDT_CLASS = 13            # mi355ndt_option: 0 (default) = pclomp::NormalDistributionsTransform; 1 = pcl::NormalDistributionsTransform, PCL's f64 class (registration_method = NDT): radius search, Euler pose vector, f64 evaluation
NDT_CLASSES = {"omp": 0, "pcl": 1}
OPT_GROUND_CLASS = 15         # mi355ndt_option: 0 (default) = off; 1 / 2 / 3 = pclomp_ground::NormalDistributionsTransformGround with flag_class 1 (horizontal leaves) / 2 (vertical leaves) / 0 (every point): gated sweeps, doubled g and H, masked Newton steps
GROUND_CLASSES = {None: 0, "horizontal": 1, "vertical": 2, "all": 3}
GROUND_FLAG_CLASS = {1: 1, 2: 2, 0: 3}   # the reference's flag_class -> the option's value
PREFILTER_EXTENDED = 0x50467832  # MI355NDT_PREFILTER_EXTENDED: PrefilterParams.extended of the base of a PrefilterParamsEx
PREFILTER_EXTENDED2 = 0x50467833  # MI355NDT_PREFILTER_EXTENDED2: PrefilterParams.extended of the base of a PrefilterParamsEx2
DOWNSAMPLE_VOXELGRID = 0       # pcl::VoxelGrid, the prefiltering nodelet's default downsample_method
DOWNSAMPLE_APPROX_VOXELGRID = 1  # pcl::ApproximateVoxelGrid
ANGLE_CALIBRATION_RAD = 0.11 * math.pi / 180   # vertical_angle_calibration's constant (prefiltering_nodelet.cpp:190)
OUTLIER_STATISTICAL = 1        # pcl::StatisticalOutlierRemoval, the prefiltering nodelet's in-code default
OUTLIER_RADIUS = 2             # pcl::RadiusOutlierRemoval (the reference builds it and never runs it)

_LIB = None


def load_library(path: str = LIB_PATH):
    """dlopen libmi355ndt.so; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(path)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    L.mi355ndt_version.restype = C.c_char_p
    L.mi355ndt_last_error.restype = C.c_char_p
    L.mi355ndt_last_error.argtypes = [vp]
    L.mi355ndt_default_params.argtypes = [C.POINTER(Params)]
    L.mi355ndt_host_numa_node.argtypes = [i]
    L.mi355ndt_create.argtypes = [C.POINTER(Params), i, C.POINTER(vp)]
    L.mi355ndt_destroy.argtypes = [vp]
    L.mi355ndt_set_params.argtypes = [vp, C.POINTER(Params)]
    L.mi355ndt_get_params.argtypes = [vp, C.POINTER(Params)]
    L.mi355ndt_set_stream.argtypes = [vp, vp]
    L.mi355ndt_set_target.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_set_source.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_promote_source_to_target.argtypes = [vp]
    L.mi355ndt_align.argtypes = [vp, vp, C.POINTER(Result)]
    L.mi355ndt_get_aligned.argtypes = [vp, vp, sz]
    L.mi355ndt_get_incremental.argtypes = [vp, i, vp, vp]
    L.mi355ndt_get_partial_rows.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int)]
    L.mi355ndt_get_fitness_score.argtypes = [vp, C.c_double, vp, vp]
    L.mi355ndt_fitness_score_T.argtypes = [vp, vp, C.c_double, vp, vp]
    L.mi355ndt_prefilter.argtypes = [vp, vp, sz, sz, i, C.c_double, C.c_double, C.c_float, vp, sz, sz, C.POINTER(sz)]
    L.mi355ndt_use_prefiltered.argtypes = [vp, i]
    L.mi355ndt_outlier_params_default.argtypes = [C.POINTER(OutlierParams)]
    L.mi355ndt_prefilter_outliers.argtypes = [vp, C.POINTER(OutlierParams), vp, vp, sz, sz, C.POINTER(sz), C.POINTER(OutlierStats)]
    L.mi355ndt_batch_remove_outliers.argtypes = [vp, i, i, i, C.POINTER(OutlierParams), vp, vp, vp, vp]
    L.mi355ndt_sequence_run_raw_outliers.argtypes = [vp, i, vp, vp, sz, vp, C.POINTER(PrefilterParams), C.POINTER(OutlierParams), C.POINTER(SeqParams), vp, vp,
                                                     C.POINTER(SeqStats), vp, vp]
    L.mi355ndt_prefilter_params_default.argtypes = [C.POINTER(PrefilterParams)]
    L.mi355ndt_prefilter_params_ex_default.argtypes = [C.POINTER(PrefilterParamsEx)]
    L.mi355ndt_prefilter_p.argtypes = [vp, vp, sz, sz, C.POINTER(PrefilterParams), vp, sz, sz, C.POINTER(sz)]
    L.mi355ndt_batch_prefilter.argtypes = [vp, i, i, vp, vp, vp, vp, sz, C.POINTER(PrefilterParams), vp, vp]
    L.mi355ndt_batch_get_cloud.argtypes = [vp, i, i, vp, sz, sz, C.POINTER(sz)]
    L.mi355ndt_prefilter_params_ex2_default.argtypes = [C.POINTER(PrefilterParamsEx2)]
    L.mi355ndt_batch_get_cloud_i.argtypes = [vp, i, i, vp, sz, sz, i, C.POINTER(sz)]
    L.mi355ndt_keyframe_from_prefiltered.argtypes = [vp, C.POINTER(i)]
    L.mi355ndt_keyframe_from_slot.argtypes = [vp, i, i, C.POINTER(i)]
    L.mi355ndt_window_keyframe_ids.argtypes = [vp, i, vp, vp, C.c_float, i, C.POINTER(i), C.POINTER(sz)]
    L.mi355ndt_sequence_run_raw.argtypes = [vp, i, vp, vp, sz, vp, C.POINTER(PrefilterParams), C.POINTER(SeqParams), vp, vp, C.POINTER(SeqStats), vp, vp]
    L.mi355ndt_gicp_params_default.argtypes = [C.POINTER(GicpParams)]
    L.mi355ndt_gicp_set_params.argtypes = [vp, C.POINTER(GicpParams)]
    L.mi355ndt_gicp_set_target.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_gicp_set_source.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_gicp_set_target_keyframe.argtypes = [vp, i]
    L.mi355ndt_gicp_set_source_keyframe.argtypes = [vp, i]
    L.mi355ndt_gicp_covariances.argtypes = [vp, i, vp, sz]
    L.mi355ndt_gicp_correspondences.argtypes = [vp, vp, vp, vp, vp, C.POINTER(i)]
    L.mi355ndt_gicp_cost.argtypes = [vp, vp, vp, C.POINTER(C.c_double), vp]
    L.mi355ndt_gicp_align.argtypes = [vp, vp, C.POINTER(GicpResult)]
    L.mi355ndt_gicp_get_aligned.argtypes = [vp, vp, sz]
    L.mi355ndt_gicp_batch_reserve.argtypes = [vp, i]
    L.mi355ndt_gicp_batch_set_source.argtypes = [vp, i, vp, sz, sz]
    L.mi355ndt_gicp_batch_set_source_keyframe.argtypes = [vp, i, i]
    L.mi355ndt_gicp_batch_align.argtypes = [vp, vp, vp]
    L.mi355ndt_gicp_batch_get_aligned.argtypes = [vp, i, vp, sz]
    L.mi355ndt_gicp_batch_stats.argtypes = [vp, C.POINTER(i), vp]
    L.mi355ndt_icp_params_default.argtypes = [C.POINTER(IcpParams)]
    L.mi355ndt_icp_set_params.argtypes = [vp, C.POINTER(IcpParams)]
    L.mi355ndt_icp_set_target.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_icp_set_source.argtypes = [vp, vp, sz, sz]
    L.mi355ndt_icp_set_target_keyframe.argtypes = [vp, i]
    L.mi355ndt_icp_set_source_keyframe.argtypes = [vp, i]
    L.mi355ndt_icp_correspondences.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(i)]
    L.mi355ndt_icp_align.argtypes = [vp, vp, C.POINTER(IcpResult)]
    L.mi355ndt_icp_get_aligned.argtypes = [vp, vp, sz]
    L.mi355ndt_icp_batch_reserve.argtypes = [vp, i]
    L.mi355ndt_icp_batch_set_source.argtypes = [vp, i, vp, sz, sz]
    L.mi355ndt_icp_batch_set_source_keyframe.argtypes = [vp, i, i]
    L.mi355ndt_icp_batch_align.argtypes = [vp, vp, vp]
    L.mi355ndt_icp_batch_get_aligned.argtypes = [vp, i, vp, sz]
    L.mi355ndt_icp_batch_stats.argtypes = [vp, C.POINTER(i), vp]
    L.mi355ndt_knn_params_default.argtypes = [C.POINTER(KnnParams)]
    L.mi355ndt_keyframe_knn.argtypes = [vp, i, vp, sz, sz, vp, C.POINTER(KnnParams), vp, vp, vp]
    L.mi355ndt_keyframe_knn_ids.argtypes = [vp, i, vp, vp, vp, C.POINTER(KnnParams), sz, vp, vp, vp]
    L.mi355ndt_keyframe_radius_search.argtypes = [vp, i, vp, sz, sz, vp, C.c_double, i, i, vp, vp, vp]
    L.mi355ndt_map_cloud.argtypes = [vp, i, vp, vp, sz, vp, C.c_double, vp, sz, sz, C.POINTER(sz)]
    L.mi355ndt_window_keyframe.argtypes = [vp, i, vp, vp, sz, i, vp, C.c_float, C.POINTER(i), C.POINTER(sz)]
    L.mi355ndt_keyframe_add.argtypes = [vp, vp, sz, sz, i, C.POINTER(i)]
    L.mi355ndt_keyframe_get.argtypes = [vp, i, vp, sz, sz, i, C.POINTER(sz)]
    L.mi355ndt_keyframe_release.argtypes = [vp, i]
    L.mi355ndt_keyframe_count.argtypes = [vp]
    L.mi355ndt_map_cloud_keyframes.argtypes = [vp, i, vp, vp, C.c_double, vp, sz, sz, C.POINTER(sz)]
    L.mi355ndt_batch_set_target_keyframe.argtypes = [vp, i, i]
    L.mi355ndt_batch_set_source_keyframe.argtypes = [vp, i, i]
    L.mi355ndt_keyframe_fitness_scores.argtypes = [vp, i, vp, vp, vp, C.c_double, vp, vp]
    L.mi355ndt_inf_params_default.argtypes = [C.POINTER(InfParams)]
    L.mi355ndt_inf_params_default.restype = None
    L.mi355ndt_information_matrix.argtypes = [C.POINTER(InfParams), C.c_double, vp]
    L.mi355ndt_derivatives.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mi355ndt_derivatives_T.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.mi355ndt_compute_hessian.argtypes = [vp, vp, vp]
    L.mi355ndt_get_grid.argtypes = [vp, i, vp, vp, vp, vp]
    L.mi355ndt_get_voxels.argtypes = [vp, i, vp, sz]
    L.mi355ndt_get_build_buffer.argtypes = [vp, i, i, vp, sz, C.POINTER(sz)]
    L.mi355ndt_batch_reserve.argtypes = [vp, i, sz, sz]
    L.mi355ndt_batch_set_target.argtypes = [vp, i, vp, sz, sz]
    L.mi355ndt_batch_set_source.argtypes = [vp, i, vp, sz, sz]
    L.mi355ndt_batch_set_clouds.argtypes = [vp, i, i, vp, vp, vp, vp, sz, i]
    L.mi355ndt_batch_bind_device.argtypes = [vp, i, vp, vp, sz, vp, vp, sz]
    L.mi355ndt_batch_build_targets.argtypes = [vp]
    L.mi355ndt_batch_align.argtypes = [vp, vp, vp]
    L.mi355ndt_batch_size.argtypes = [vp]
    L.mi355ndt_batch_pose_records.argtypes = [vp, i, i, vp, sz]
    L.mi355ndt_batch_fitness_scores.argtypes = [vp, vp, C.c_double, vp, vp]
    L.mi355ndt_batch_score_poses.argtypes = [vp, i, vp, vp, vp, vp]
    L.mi355ndt_profile_enable.argtypes = [vp, i]
    L.mi355ndt_profile_reset.argtypes = [vp]
    L.mi355ndt_profile_get.argtypes = [vp, C.POINTER(Profile)]
    L.mi355ndt_synchronize.argtypes = [vp]
    L.mi355ndt_set_latency_mode.argtypes = [vp, i]
    L.mi355ndt_sequence_run.argtypes = [vp, i, vp, vp, sz, vp, C.POINTER(SeqParams), vp, vp, C.POINTER(SeqStats)]
    L.mi355ndt_calculate_score.argtypes = [vp, vp, sz, sz, C.POINTER(C.c_double)]
    L.mi355ndt_convert_transform.argtypes = [vp, vp]
    L.mi355ndt_set_option.argtypes = [vp, i, i]
    L.mi355ndt_get_option.argtypes = [vp, i, C.POINTER(i)]
    L.mi355ndt_stream_begin.argtypes = [vp, i, i, sz, sz]
    L.mi355ndt_stream_submit.argtypes = [vp, i, vp, vp, sz, vp, vp, sz, vp, C.POINTER(C.c_longlong)]
    L.mi355ndt_stream_submit_host.argtypes = [vp, i, vp, vp, vp, vp, sz, vp, i, C.POINTER(C.c_longlong)]
    L.mi355ndt_stream_collect.argtypes = [vp, C.c_longlong, vp]
    L.mi355ndt_stream_end.argtypes = [vp]
    L.mi355ndt_stream_pose_records.argtypes = [vp, vp, sz, i, i]
    L.mi355ndt_pack_pose_records.argtypes = [vp, i, i, i, vp, sz]
    _LIB = L
    return L


def default_params(**kw) -> Params:
    p = Params()
    load_library().mi355ndt_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_inf_params(**kw) -> InfParams:
    """The defaults of InformationMatrixCalculator's constructor (fitness_score_thresh 0.5; the reference's load() says 2.5)."""
    p = InfParams()
    load_library().mi355ndt_inf_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"no information matrix parameter {k!r}")
        setattr(p, k, v)
    return p


def information_matrix(fitness: float, params: InfParams | None = None, **kw) -> np.ndarray:
    """The weighting half of InformationMatrixCalculator::calc_information_matrix (information_matrix_calculator.cpp:27-51) for one fitness
    score: the 6x6 f64 information matrix, quirks of the reference included (mi355ndt_information_matrix).  Parameters: an InfParams, or
    the constructor's defaults with `kw` overriding fields.  Host arithmetic: no engine, no GPU."""
    p = params if params is not None else default_inf_params(**kw)
    if params is not None and kw:
        raise TypeError("give either params or keyword overrides")
    out = np.zeros(36, np.float64)
    rc = load_library().mi355ndt_information_matrix(C.byref(p), float(fitness), out.ctypes.data_as(C.c_void_p))
    if rc != OK:
        raise NDTError(rc, "information_matrix")
    return out.reshape(6, 6)


def default_gicp_params(**kw) -> GicpParams:
    """The constructor's values of pclomp::GeneralizedIterativeClosestPoint (gicp_omp.h:110-120), `kw` overriding fields."""
    p = GicpParams()
    load_library().mi355ndt_gicp_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"no GICP parameter {k!r}")
        setattr(p, k, v)
    return p


def default_icp_params(**kw) -> IcpParams:
    """pcl::Registration's constructor values as pcl::IterativeClosestPoint starts with them, `kw` overriding fields."""
    p = IcpParams()
    load_library().mi355ndt_icp_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"no ICP parameter {k!r}")
        setattr(p, k, v)
    return p


def _icp_result_dict(r: IcpResult) -> dict:
    return dict(final=np.array(r.final_colmajor, np.float32).reshape(4, 4).T.copy(), converged=bool(r.converged), iterations=r.iterations,
                state=r.state, matches=r.matches, mse=r.mse)


def _as_points(cloud) -> np.ndarray:
    """Accept [N,3]/[N,4+] float arrays (PCL-like records: x,y,z first); returns C-contiguous f32."""
    a = np.asarray(cloud)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be [N,>=3] (x,y,z first)")
    return np.ascontiguousarray(a, dtype=np.float32)


def _colmajor(M) -> np.ndarray:
    M = np.asarray(M, dtype=np.float32)
    if M.shape != (4, 4):
        raise ValueError("transform must be 4x4")
    return np.ascontiguousarray(M.T).ravel()      # column-major flattening (Eigen::Matrix4f layout)


_DOWNSAMPLE_METHODS = {"VOXELGRID": DOWNSAMPLE_VOXELGRID, "APPROX_VOXELGRID": DOWNSAMPLE_APPROX_VOXELGRID}


def _prefilter_params(distance_near, distance_far, downsample_resolution, use_distance_filter, transform, downsample_method="VOXELGRID",
                      angle_calibration=False, intensity=False):
    """The keywords of Engine.batch_prefilter / sequence_run_raw / prefilter_p as a PrefilterParamsEx, whose `base` the calls are given (no
    library call: a bad transform, an unknown downsample_method and a non-finite calibration angle are refused here).  downsample_method:
    the nodelet's strings ("NONE" is downsample_resolution <= 0); angle_calibration: False, True (the reference's 0.11 degrees) or the
    angle in radians.  intensity: the same behind a PrefilterParamsEx2 that names column 3 of the records (byte 12) as their intensity; its
    ex.base is what the calls are given (_base_ref)."""
    if intensity:
        x2 = PrefilterParamsEx2()
        x2.ex = _prefilter_params(distance_near, distance_far, downsample_resolution, use_distance_filter, transform, downsample_method, angle_calibration)
        x2.ex.base.extended, x2.intensity_offset_bytes, x2.reserved = PREFILTER_EXTENDED2, 12, 0
        return x2
    if downsample_method not in _DOWNSAMPLE_METHODS:
        raise ValueError(f"downsample_method must be one of {list(_DOWNSAMPLE_METHODS)} (no down-sampling: downsample_resolution <= 0)")
    switch = isinstance(angle_calibration, (bool, np.bool_))
    rad = ANGLE_CALIBRATION_RAD if switch else float(angle_calibration)
    if not math.isfinite(rad):
        raise ValueError("angle_calibration must be False, True or a finite angle in radians")
    x = PrefilterParamsEx()
    p = x.base
    p.use_distance_filter, p.extended = int(bool(use_distance_filter)), PREFILTER_EXTENDED
    p.distance_near, p.distance_far, p.downsample_resolution = float(distance_near), float(distance_far), float(downsample_resolution)
    t = np.eye(4, dtype=np.float32) if transform is None else transform
    p.transform_colmajor[:] = [float(v) for v in _colmajor(t)]
    p.use_transform = int(transform is not None)
    x.downsample_method = _DOWNSAMPLE_METHODS[downsample_method]
    x.use_angle_calibration = int(bool(angle_calibration)) if switch else 1
    x.angle_calibration_rad = rad
    return x


def _base_ref(prm):
    """byref of the PrefilterParams at the head of a PrefilterParamsEx or a PrefilterParamsEx2: what every C call takes"""
    return C.byref(prm.ex.base if isinstance(prm, PrefilterParamsEx2) else prm.base)


_OUTLIER_KEYS = ("method", "mean_k", "stddev_mul", "radius", "min_neighbors")


def _outlier_params(method="STATISTICAL", mean_k=20, stddev_mul=1.0, radius=0.8, min_neighbors=2) -> OutlierParams:
    """The keywords of Engine.batch_remove_outliers as an OutlierParams (no library call)."""
    if isinstance(method, str):                    # (an unknown name becomes 0, which the library refuses with its own message)
        method = {"STATISTICAL": OUTLIER_STATISTICAL, "RADIUS": OUTLIER_RADIUS}.get(method.upper(), 0)
    return OutlierParams(int(method), int(mean_k), float(stddev_mul), float(radius), int(min_neighbors))


def _outlier_dict(outlier) -> OutlierParams:
    """The `outlier` dict of Engine.batch_prefilter / sequence_run_raw (empty: the nodelet's in-code defaults); an unknown key is refused here."""
    if not isinstance(outlier, dict):
        raise ValueError("outlier must be a dict of batch_remove_outliers' keywords (may be empty)")
    unknown = sorted(set(outlier) - set(_OUTLIER_KEYS))
    if unknown:
        raise ValueError(f"outlier: unknown key(s) {unknown}; known: {list(_OUTLIER_KEYS)}")
    return _outlier_params(**outlier)


def _cloud_table(clouds, widen=False):
    """A list of clouds as (kept arrays, pointers uint64[n], counts uint64[n], the records' one stride).  The C calls take one stride: with
    `widen`, clouds of narrower records are copied into records as wide as the widest; without it, differing strides are refused."""
    arrs = [_as_points(c) for c in clouds]
    widths = {a.shape[1] for a in arrs if a.shape[0]} or {3}
    if len(widths) != 1:
        if not widen:
            raise ValueError("all clouds of a call must share one record stride")
        wide = max(widths)
        arrs = [a if a.shape[1] == wide or not a.shape[0] else np.concatenate([a, np.zeros((a.shape[0], wide - a.shape[1]), np.float32)], axis=1) for a in arrs]
    return (arrs, np.array([a.ctypes.data if a.shape[0] else 0 for a in arrs], np.uint64), np.array([a.shape[0] for a in arrs], np.uint64),
            4 * max(widths))


def _seq_frames_out(out, res) -> list:
    return [dict(odom=np.array(f.odom_colmajor, np.float64).reshape(4, 4).T.copy(), tf_s2k=np.array(f.tf_s2k_colmajor, np.float32).reshape(4, 4).T.copy(),
                 trans_probability=f.trans_probability, test=(f.dx, f.da, f.dt), key_id=f.key_id, new_keyframe=bool(f.new_keyframe),
                 iterations=f.iterations, converged=bool(f.converged), aligns=f.aligns, result=_result_dict(r)) for f, r in zip(out, res)]


def _result_dict(r: Result) -> dict:
    return dict(final=np.array(r.final_colmajor, np.float32).reshape(4, 4).T.copy(),
                trans_probability=r.trans_probability, score=r.score, iterations=r.iterations,
                converged=bool(r.converged), sweeps=r.sweeps, status=r.status, hits_last=r.hits_last)


# mi355ndt_build_buffer: name -> (number, element type) of Engine.get_build_buffer
GRIDDESC_DTYPE = np.dtype([("min_b", "<i4", 3), ("max_b", "<i4", 3), ("div_b", "<i4", 3), ("mul1", "<i4"), ("mul2", "<i4"), ("leaf", "<f4"), ("inv_leaf", "<f4"),
                           ("ncells", "<i4"), ("nwords", "<i4"), ("status", "<i4"), ("n_voxels", "<i4"), ("word_off", "<u4"), ("rec_off", "<u4")])
BITWORD_DTYPE = np.dtype([("bits", "<u8"), ("prefix", "<u4"), ("pad", "<u4")])
RECF_DTYPE = np.dtype([("mh", "<f4", 3), ("ml", "<f4", 3), ("c", "<f4", 6), ("pad", "<f4", 3), ("weight", "<i4")])
BUILD_BUFFERS = {
    "minmax": (0, np.dtype("<u4")), "griddesc": (1, GRIDDESC_DTYPE), "words": (2, BITWORD_DTYPE), "keys": (3, np.dtype("<u4")), "ids": (4, np.dtype("<u4")),
    "head_cnt": (5, np.dtype("<u4")), "heads": (6, np.dtype("<u4")), "seg_start": (7, np.dtype("<u4")), "sums": (8, np.dtype("<f8")), "cent": (9, np.dtype("<f4")),
    "vox_idx": (10, np.dtype("<i4")), "vox_n": (11, np.dtype("<i4")), "icov64": (12, np.dtype("<f8")), "kd_weight": (13, np.dtype("<i4")),
    "recs_fast": (14, RECF_DTYPE), "sorted_points": (15, np.dtype("<f4")), "info": (16, np.dtype("<u4")), "geometry": (17, np.dtype("<u8")),
}
GROUND_BUILD_BUFFERS = {"leaf_class": (18, np.dtype("u1"))}   # enum mi355ndt_build_buffer_ground: what a build under OPT_GROUND_CLASS = 1 / 2 makes beside those


class Engine:
    """Thin RAII wrapper of one mi355ndt_handle (one GPU, one stream)."""

    def __init__(self, params: Params | None = None, device: int = 0):
        self.lib = load_library()
        self.h = C.c_void_p()
        rc = self.lib.mi355ndt_create(C.byref(params) if params is not None else None, device, C.byref(self.h))
        if rc != OK:
            self.h = None
            raise NDTError(rc, "mi355ndt_create")
        self._keep = []
        self._gicp_n = [0, 0]                       # points of the GICP surface's target and source
        self._gicp_batch_n = []                     # points of the GICP batch's slots
        self._icp_n = [0, 0]                        # points of the ICP surface's target and source
        self._icp_batch_n = []                      # points of the ICP batch's slots

    def close(self):
        if getattr(self, "h", None):
            self.lib.mi355ndt_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, where):
        if rc != OK:
            raise NDTError(rc, where, (self.lib.mi355ndt_last_error(self.h) or b"").decode())

    # -- parameters
    def get_params(self) -> Params:
        p = Params()
        self._chk(self.lib.mi355ndt_get_params(self.h, C.byref(p)), "get_params")
        return p

    def set_params(self, p: Params):
        self._chk(self.lib.mi355ndt_set_params(self.h, C.byref(p)), "set_params")

    def set_stream(self, stream_ptr: int | None):
        self._chk(self.lib.mi355ndt_set_stream(self.h, C.c_void_p(stream_ptr or 0)), "set_stream")

    # -- single registration
    def set_target(self, cloud):
        a = _as_points(cloud)
        self._chk(self.lib.mi355ndt_set_target(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "set_target")

    def promote_source_to_target(self):
        """the cloud last set as source becomes the target, device to device (the nodelet's keyframe switch, scan_matching_odom_nodelet.cpp:240-243)"""
        self._chk(self.lib.mi355ndt_promote_source_to_target(self.h), "promote_source_to_target")

    def set_source(self, cloud):
        a = _as_points(cloud)
        self._n_src = a.shape[0]
        self._chk(self.lib.mi355ndt_set_source(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "set_source")

    def align(self, guess) -> dict:
        g = _colmajor(guess)
        r = Result()
        self._chk(self.lib.mi355ndt_align(self.h, g.ctypes.data_as(C.c_void_p), C.byref(r)), "align")
        return _result_dict(r)

    def get_aligned(self) -> np.ndarray:
        out = np.zeros((self._n_src, 3), np.float32)
        self._chk(self.lib.mi355ndt_get_aligned(self.h, out.ctypes.data_as(C.c_void_p), 12), "get_aligned")
        return out

    def get_incremental(self, pair: int = 0):
        """(transformation_, previous_transformation_) of the last align: f32 exp(delta_p) of the last two Newton steps."""
        a, b = np.zeros(16, np.float32), np.zeros(16, np.float32)
        self._chk(self.lib.mi355ndt_get_incremental(self.h, pair, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)), "get_incremental")
        return a.reshape(4, 4).T.copy(), b.reshape(4, 4).T.copy()

    def partial_rows(self) -> np.ndarray:
        """[pairs, rows per pair, 44] f64: the partial rows (score, g, H, hits) the last sweep of every pair of the bound batch left on the device."""
        rpp = C.c_int()
        self._chk(self.lib.mi355ndt_get_partial_rows(self.h, None, 0, C.byref(rpp)), "get_partial_rows")
        B = self.lib.mi355ndt_batch_size(self.h)
        out = np.zeros((B, rpp.value, 44), np.float64)
        self._chk(self.lib.mi355ndt_get_partial_rows(self.h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(rpp)), "get_partial_rows")
        return out

    def fitness_score(self, max_range: float = float("inf"), T=None):
        """getFitnessScore(max_range); T = explicit 4x4 transform (default: final pose of the last align)."""
        s, n = C.c_double(), C.c_longlong()
        mr = 1.7976931348623157e308 if max_range == float("inf") else float(max_range)
        if T is None:
            self._chk(self.lib.mi355ndt_get_fitness_score(self.h, mr, C.byref(s), C.byref(n)), "get_fitness_score")
        else:
            t = _colmajor(T)
            self._chk(self.lib.mi355ndt_fitness_score_T(self.h, t.ctypes.data_as(C.c_void_p), mr, C.byref(s), C.byref(n)), "fitness_score_T")
        return s.value, n.value

    def calculate_score(self, cloud) -> float:
        """calculateScore(cloud) (ndt_omp.h:232): negative log-likelihood of an ALREADY TRANSFORMED cloud against the target grid."""
        a = _as_points(cloud)
        s = C.c_double()
        self._chk(self.lib.mi355ndt_calculate_score(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0] if a.shape[0] else 12, C.byref(s)), "calculate_score")
        return s.value

    def set_option(self, option: int, value: int):
        self._chk(self.lib.mi355ndt_set_option(self.h, option, value), "set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int()
        self._chk(self.lib.mi355ndt_get_option(self.h, option, C.byref(v)), "get_option")
        return v.value

    def prefilter(self, cloud, distance_near=0.5, distance_far=100.0, downsample_resolution=0.1, use_distance_filter=True,
                  fetch=True, outlier=None, intensity=False):
        """PrefilteringNodelet distance_filter + VoxelGrid downsample (defaults of launch/dlo_kitti.launch:30-36).
        Returns the filtered [M,3] cloud (or just M when fetch=False; the result stays on the GPU for use_prefiltered).
        outlier: a dict of prefilter_outliers' keywords (may be empty: the nodelet's in-code defaults) -- the nodelet's third stage runs on
        the resident result before anything is fetched, and what is returned is what prefilter_outliers returns.
        intensity: prefilter_p's keyword (the call then goes through prefilter_p: clouds are [N,4] in and out)."""
        if intensity:
            out = self.prefilter_p(cloud, distance_near, distance_far, downsample_resolution, use_distance_filter, fetch=fetch and outlier is None,
                                   intensity=True)
            return out if outlier is None else self.prefilter_outliers(**{"fetch": fetch, "intensity": True, **outlier})
        a = _as_points(cloud)
        n_out = C.c_size_t()
        if outlier is not None:
            self.prefilter(a, distance_near, distance_far, downsample_resolution, use_distance_filter, fetch=False)
            return self.prefilter_outliers(**{"fetch": fetch, **outlier})
        out = np.zeros((a.shape[0], 3), np.float32) if fetch else None
        self._chk(self.lib.mi355ndt_prefilter(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0] if a.shape[0] else 12,
                                              int(use_distance_filter), float(distance_near), float(distance_far),
                                              float(downsample_resolution), out.ctypes.data_as(C.c_void_p) if fetch else None,
                                              a.shape[0], 12, C.byref(n_out)), "prefilter")
        self._pf_count, self._pf_ch = n_out.value, 3
        return out[: n_out.value].copy() if fetch else n_out.value

    def prefilter_p(self, cloud, distance_near=0.5, distance_far=100.0, downsample_resolution=0.1, use_distance_filter=True, transform=None,
                    downsample_method="VOXELGRID", angle_calibration=False, fetch=True, intensity=False):
        """mi355ndt_prefilter_p: prefilter with the nodelet's whole parameter set (batch_prefilter's keywords) over one cloud.  The result is
        resident as after prefilter: use_prefiltered and prefilter_outliers follow.  Returns the filtered [M,3] cloud (M when fetch=False).
        intensity: column 3 of the [N,>=4] cloud is the points' intensity and goes through the chain (PointXYZI: averaged per voxel, zeroed
        by the calibration); the result is [M,4] and stays resident with its fourth row."""
        prm = _prefilter_params(distance_near, distance_far, downsample_resolution, use_distance_filter, transform, downsample_method, angle_calibration,
                                intensity)
        a = self._records(cloud, intensity)
        n_out = C.c_size_t()
        w = 4 if intensity else 3
        out = np.zeros((a.shape[0], w), np.float32) if fetch else None
        self._chk(self.lib.mi355ndt_prefilter_p(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], 4 * a.shape[1], _base_ref(prm),
                                                out.ctypes.data_as(C.c_void_p) if fetch else None, a.shape[0], 4 * w, C.byref(n_out)), "prefilter_p")
        self._pf_count, self._pf_ch = n_out.value, w
        return out[: n_out.value].copy() if fetch else n_out.value

    def prefilter_outliers(self, method="STATISTICAL", mean_k=20, stddev_mul=1.0, radius=0.8, min_neighbors=2, fetch=True, return_stats=False,
                           intensity=False):
        """PrefilteringNodelet::outlier_removal over the resident prefilter result, in place (mi355ndt_prefilter_outliers): "STATISTICAL"
        (pcl::StatisticalOutlierRemoval, the nodelet's in-code default) or "RADIUS" (pcl::RadiusOutlierRemoval -- which the reference never
        runs: prefiltering_nodelet.cpp:71-78).  Returns the surviving [M,3] cloud (or just M when fetch=False); with return_stats also a
        dict: dist (f32 per input point, input order), n_in, n_valid, mean, stddev, threshold (zeros for RADIUS).
        intensity: the survivors come back as [M,4] with their intensities (zeros when the resident result carries none); without it
        [M,3], whatever the resident result carries."""
        if isinstance(method, str):                # (an unknown name becomes 0, which the library refuses with its own message)
            method = {"STATISTICAL": OUTLIER_STATISTICAL, "RADIUS": OUTLIER_RADIUS}.get(method.upper(), 0)
        prm = OutlierParams(int(method), int(mean_k), float(stddev_mul), float(radius), int(min_neighbors))
        n_in = getattr(self, "_pf_count", 0)
        n_out, st = C.c_size_t(), OutlierStats()
        w = max(4 if intensity else 3, getattr(self, "_pf_ch", 3))       # (a resident intensity row is written out: the records hold it)
        out = np.zeros((n_in, w), np.float32) if fetch else None
        dist = np.zeros(n_in, np.float32) if return_stats else None
        self._chk(self.lib.mi355ndt_prefilter_outliers(self.h, C.byref(prm), dist.ctypes.data_as(C.c_void_p) if return_stats else None,
                                                       out.ctypes.data_as(C.c_void_p) if fetch else None, n_in, 4 * w, C.byref(n_out),
                                                       C.byref(st)), "prefilter_outliers")
        self._pf_count = n_out.value
        res = np.ascontiguousarray(out[: n_out.value, : 4 if intensity else 3]) if fetch else n_out.value
        if not return_stats:
            return res
        return res, dict(dist=dist, n_in=st.n_in, n_valid=st.n_valid, mean=st.mean, stddev=st.stddev, threshold=st.threshold)

    def use_prefiltered(self, as_target: bool):
        """setInputTarget / setInputSource with the last prefilter result, device to device."""
        self._chk(self.lib.mi355ndt_use_prefiltered(self.h, 2 if as_target else 1), "use_prefiltered")
        if not as_target:
            self._n_src = self._pf_count

    def map_cloud(self, clouds, poses, resolution, fetch=True):
        """MapCloudGenerator::generate(keyframes, resolution): keyframe k's cloud ([N_k,>=3], x,y,z first) moved by poses[k] (4x4, f64;
        cast to f32 as the reference does), every point fed in keyframe order into an OctreePointCloud(resolution), the occupied voxel
        centres returned as [M,3] float32 in getOccupiedVoxelCenters' order (M alone with fetch=False).  None for an empty keyframe list
        (the reference returns nullptr).  tools/map_cloud_ref.py is the CPU restatement it equals bit for bit."""
        clouds = [np.ascontiguousarray(_as_points(c)[:, :3]) for c in clouds]
        P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        if P.shape[0] != len(clouds):
            raise ValueError("one 4x4 pose per cloud")
        if not clouds:
            self._chk(self.lib.mi355ndt_map_cloud(self.h, 0, None, None, 12, None, float(resolution), None, 0, 12, C.byref(C.c_size_t())),
                      "map_cloud")
            return None
        K = len(clouds)
        ptrs = (C.c_void_p * K)(*[c.ctypes.data for c in clouds])
        counts = (C.c_size_t * K)(*[c.shape[0] for c in clouds])
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(K, 16)        # column-major per keyframe
        n = sum(c.shape[0] for c in clouds)
        out = np.empty((max(n, 1), 3), np.float32) if fetch else None
        n_out = C.c_size_t()
        self._chk(self.lib.mi355ndt_map_cloud(self.h, K, ptrs, counts, 12, pcm.ctypes.data_as(C.c_void_p), float(resolution),
                                              out.ctypes.data_as(C.c_void_p) if fetch else None, n, 12, C.byref(n_out)), "map_cloud")
        return out[: n_out.value].copy() if fetch else n_out.value

    # -- keyframes that stay on the device
    @staticmethod
    def _records(cloud, intensity: bool) -> np.ndarray:
        """C-contiguous f32 records, x, y, z first and -- with `intensity` -- the intensity in column 3."""
        a = _as_points(cloud)
        if intensity and a.shape[1] < 4:
            raise ValueError("intensity=True needs [N,>=4] records (x, y, z, intensity)")
        return a

    def window_keyframe(self, scans, rel_poses, leaf: float = 0.1, intensity: bool = False):
        """The window map of GlobalGraphNodelet::cloud_callback (global_graph_nodelet.cpp:202-244) as one keyframe on the device: scan 0 as it
        is, scan k moved by rel_poses[k] (4x4 f64, w_odom.inverse() * odom_k; rel_poses[0] is ignored), appended in order, VoxelGrid(leaf).
        scans: [N_k,>=3] float arrays sharing one record layout (column 3 = intensity with intensity=True).  Returns (keyframe id, points);
        the cloud stays on the device (keyframe_get fetches it).  tools/window_map_ref.py is the CPU restatement it equals bit for bit."""
        recs = [self._records(c, intensity) for c in scans]
        K = len(recs)
        if K == 0:
            raise ValueError("a window has at least one scan")
        widths = {r.shape[1] for r in recs}
        if len(widths) != 1:
            raise ValueError("all scans of a window must share one record layout")
        P = np.ascontiguousarray(np.asarray(rel_poses, np.float64).reshape(-1, 4, 4))
        if P.shape[0] != K:
            raise ValueError("one 4x4 relative pose per scan")
        ptrs = (C.c_void_p * K)(*[r.ctypes.data for r in recs])
        counts = (C.c_size_t * K)(*[r.shape[0] for r in recs])
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(K, 16)        # column-major per scan
        kid, n_out = C.c_int(-1), C.c_size_t()
        self._chk(self.lib.mi355ndt_window_keyframe(self.h, K, ptrs, counts, 4 * widths.pop(), 12 if intensity else -1,
                                                    pcm.ctypes.data_as(C.c_void_p), float(leaf), C.byref(kid), C.byref(n_out)), "window_keyframe")
        return kid.value, n_out.value

    def window_keyframe_ids(self, ids, rel_poses, leaf: float = 0.1, intensity: bool = False):
        """window_keyframe over resident scans (mi355ndt_window_keyframe_ids): scan k is keyframe ids[k] as it is stored (keyframe_add,
        keyframe_from_prefiltered, keyframe_from_slot); the same rules, the same words, and nothing is uploaded.  intensity: a keyframe of
        four channels (a scan stored with three contributes +0).  An id may appear twice.  The scans' keyframes are left as they were.
        Returns (keyframe id, points)."""
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        K = ids.shape[0]
        if K == 0:
            raise ValueError("a window has at least one scan")
        P = np.ascontiguousarray(np.asarray(rel_poses, np.float64).reshape(-1, 4, 4))
        if P.shape[0] != K:
            raise ValueError("one 4x4 relative pose per scan")
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(K, 16)        # column-major per scan
        kid, n_out = C.c_int(-1), C.c_size_t()
        self._chk(self.lib.mi355ndt_window_keyframe_ids(self.h, K, ids.ctypes.data_as(C.c_void_p), pcm.ctypes.data_as(C.c_void_p), float(leaf),
                                                        int(bool(intensity)), C.byref(kid), C.byref(n_out)), "window_keyframe_ids")
        return kid.value, n_out.value

    def keyframe_from_prefiltered(self) -> int:
        """The resident prefilter result (after prefilter / prefilter_p / prefilter_outliers) becomes a keyframe, device to device, with
        its intensity when it has one; returns its id.  The result stays resident."""
        kid = C.c_int(-1)
        self._chk(self.lib.mi355ndt_keyframe_from_prefiltered(self.h, C.byref(kid)), "keyframe_from_prefiltered")
        return kid.value

    def keyframe_from_slot(self, pair: int, target: bool) -> int:
        """The cloud batch slot `pair` holds on its target (or source) side becomes a keyframe, device to device, with its intensity when
        the slot carries one (batch_prefilter / sequence_run_raw with intensity=True); returns its id.  The slot is left as it was."""
        kid = C.c_int(-1)
        self._chk(self.lib.mi355ndt_keyframe_from_slot(self.h, int(pair), 2 if target else 1, C.byref(kid)), "keyframe_from_slot")
        return kid.value

    def keyframe_add(self, cloud, intensity: bool = False) -> int:
        """A host cloud as it is becomes a resident keyframe; returns its id."""
        a = self._records(cloud, intensity)
        kid = C.c_int(-1)
        self._chk(self.lib.mi355ndt_keyframe_add(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], 4 * a.shape[1], 12 if intensity else -1,
                                                 C.byref(kid)), "keyframe_add")
        return kid.value

    def keyframe_get(self, kid: int, intensity: bool = False, fetch: bool = True):
        """The keyframe's cloud as [N,3] (or [N,4] with the intensity; zeros for a keyframe without one) float32; fetch=False: N alone."""
        n = C.c_size_t()
        self._chk(self.lib.mi355ndt_keyframe_get(self.h, int(kid), None, 0, 12, -1, C.byref(n)), "keyframe_get")
        if not fetch:
            return n.value
        w = 4 if intensity else 3
        out = np.zeros((n.value, w), np.float32)
        if n.value:
            self._chk(self.lib.mi355ndt_keyframe_get(self.h, int(kid), out.ctypes.data_as(C.c_void_p), n.value, 4 * w, 12 if intensity else -1,
                                                     C.byref(n)), "keyframe_get")
        return out

    def keyframe_release(self, kid: int):
        self._chk(self.lib.mi355ndt_keyframe_release(self.h, int(kid)), "keyframe_release")

    def keyframe_count(self) -> int:
        n = self.lib.mi355ndt_keyframe_count(self.h)
        if n < 0:
            raise NDTError(n, "keyframe_count")
        return n

    def map_cloud_keyframes(self, ids, poses, resolution, fetch=True):
        """map_cloud over resident keyframes (ids from window_keyframe / keyframe_add): the same centres, word for word, with no upload."""
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        K = len(ids)
        P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        if P.shape[0] != K:
            raise ValueError("one 4x4 pose per keyframe")
        if K == 0:
            self._chk(self.lib.mi355ndt_map_cloud_keyframes(self.h, 0, None, None, float(resolution), None, 0, 12, C.byref(C.c_size_t())),
                      "map_cloud_keyframes")
            return None
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(K, 16)
        n = sum(self.keyframe_get(k, fetch=False) for k in ids) if fetch else 0       # an upper bound of the centres: the points
        out = np.empty((max(n, 1), 3), np.float32) if fetch else None
        n_out = C.c_size_t()
        self._chk(self.lib.mi355ndt_map_cloud_keyframes(self.h, K, ids.ctypes.data_as(C.c_void_p), pcm.ctypes.data_as(C.c_void_p), float(resolution),
                                                        out.ctypes.data_as(C.c_void_p) if fetch else None, n, 12, C.byref(n_out)), "map_cloud_keyframes")
        return out[: n_out.value].copy() if fetch else n_out.value

    def keyframe_fitness_scores(self, ids1, ids2, relposes, max_range: float = float("inf")):
        """InformationMatrixCalculator::calc_fitness_score for E graph edges between resident keyframes in one call: keyframe ids1[e] is
        searched, keyframe ids2[e] is moved by relposes[e] (4x4 f64, cast to f32 as the reference does).  Returns (scores float64[E],
        inliers int64[E]): word for word fitness_score(T=relposes[e]) of a one-pair engine with cloud1 as target and cloud2 as source;
        (DBL_MAX, 0) where nothing is in range or a keyframe is empty.  Nothing is uploaded; the first call that searches a keyframe
        builds its index, which stays with it."""
        a = np.ascontiguousarray(ids1, np.int32).ravel()
        b = np.ascontiguousarray(ids2, np.int32).ravel()
        E = len(a)
        P = np.asarray(relposes, np.float64).reshape(-1, 4, 4)
        if len(b) != E or P.shape[0] != E:
            raise ValueError("one id of each side and one 4x4 relative pose per edge")
        mr = 1.7976931348623157e308 if max_range == float("inf") else float(max_range)
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(E, 16)        # column-major per edge
        scores = np.zeros(max(E, 1), np.float64)
        inliers = np.zeros(max(E, 1), np.int64)
        self._chk(self.lib.mi355ndt_keyframe_fitness_scores(self.h, E, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                                            pcm.ctypes.data_as(C.c_void_p), mr, scores.ctypes.data_as(C.c_void_p),
                                                            inliers.ctypes.data_as(C.c_void_p)), "keyframe_fitness_scores")
        return scores[:E], inliers[:E]

    # -- exact k-nearest and radius search over resident keyframes (pcl::KdTreeFLANN over a keyframe that stays on the device)
    @staticmethod
    def _knn_out(n: int, k: int):
        """result arrays as the library leaves untouched slots: id -1, d2 +inf, count 0"""
        return np.full((n, k), -1, np.int32), np.full((n, k), np.inf, np.float32), np.zeros(n, np.int32)

    def keyframe_knn(self, kid: int, queries, k: int, max_range: float = float("inf"), T=None, query_order: int = KNN_ORDER_AUTO):
        """The k nearest searchable points of resident keyframe `kid` for every query ([n,>=3] floats, moved by the 4x4 f32 pose T when
        given): (ids [n,k] int32, d2 [n,k] float32, counts [n] int32), ascending (d2, id) -- a tie goes to the lower point id -- kept iff
        (double)d2 <= max_range^2; unused slots hold -1 / +inf.  tools/knn_ref.py restates every word.  The keyframe stays on the device."""
        q = _as_points(queries) if len(queries) else np.zeros((0, 3), np.float32)
        n = q.shape[0]
        p = KnnParams(int(k), float(max_range), int(query_order))
        ids, d2, cnt = self._knn_out(n, max(int(k), 1))
        t = _colmajor(T) if T is not None else None
        self._chk(self.lib.mi355ndt_keyframe_knn(self.h, int(kid), q.ctypes.data_as(C.c_void_p), n, 4 * q.shape[1],
                                                 t.ctypes.data_as(C.c_void_p) if t is not None else None, C.byref(p),
                                                 ids.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)), "keyframe_knn")
        return ids, d2, cnt

    def keyframe_knn_ids(self, searched_ids, query_ids, relposes, k: int, max_range: float = float("inf"), query_order: int = KNN_ORDER_AUTO,
                         total_queries: int | None = None):
        """keyframe_knn for E (searched keyframe, query keyframe, 4x4 f64 pose) items in one launch chain and one wait, the queries read
        in place (nothing is uploaded); the poses are cast to f32 as keyframe_fitness_scores casts them.  Returns (ids, d2, counts)
        concatenated in item order; total_queries (default: asked of the store) must be the sum of the query keyframes' counts."""
        a = np.ascontiguousarray(searched_ids, np.int32).ravel()
        b = np.ascontiguousarray(query_ids, np.int32).ravel()
        E = len(a)
        P = np.asarray(relposes, np.float64).reshape(-1, 4, 4)
        if len(b) != E or P.shape[0] != E:
            raise ValueError("one id of each side and one 4x4 relative pose per item")
        if total_queries is None:
            total_queries = sum(self.keyframe_get(int(x), fetch=False) for x in b)
        pcm = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(E, 16)        # column-major per item
        p = KnnParams(int(k), float(max_range), int(query_order))
        ids, d2, cnt = self._knn_out(int(total_queries), max(int(k), 1))
        self._chk(self.lib.mi355ndt_keyframe_knn_ids(self.h, E, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), pcm.ctypes.data_as(C.c_void_p),
                                                     C.byref(p), int(total_queries), ids.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p),
                                                     cnt.ctypes.data_as(C.c_void_p)), "keyframe_knn_ids")
        return ids, d2, cnt

    def keyframe_radius_search(self, kid: int, queries, radius: float, max_nn: int, T=None, query_order: int = KNN_ORDER_AUTO):
        """Radius search over resident keyframe `kid`: within iff d2 < (float)(radius * radius), strictly.  counts [n] = ALL the searchable
        points within; (ids, d2) [n,max_nn] = the max_nn nearest of them in ascending (d2, id), unused slots -1 / +inf."""
        q = _as_points(queries) if len(queries) else np.zeros((0, 3), np.float32)
        n = q.shape[0]
        ids, d2, cnt = self._knn_out(n, max(int(max_nn), 1))
        t = _colmajor(T) if T is not None else None
        self._chk(self.lib.mi355ndt_keyframe_radius_search(self.h, int(kid), q.ctypes.data_as(C.c_void_p), n, 4 * q.shape[1],
                                                           t.ctypes.data_as(C.c_void_p) if t is not None else None, float(radius), int(max_nn),
                                                           int(query_order), ids.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p),
                                                           cnt.ctypes.data_as(C.c_void_p)), "keyframe_radius_search")
        return ids, d2, cnt

    # -- GICP (pclomp::GeneralizedIterativeClosestPoint, registration_method = GICP_OMP): one pair, synchronous (the batch form follows)
    def gicp_set_params(self, p: GicpParams):
        self._chk(self.lib.mi355ndt_gicp_set_params(self.h, C.byref(p)), "gicp_set_params")

    def _gicp_set(self, role: int, cloud=None, kid=None):
        name = "gicp_set_target" if role == GICP_TARGET else "gicp_set_source"
        if kid is not None:
            fn = self.lib.mi355ndt_gicp_set_target_keyframe if role == GICP_TARGET else self.lib.mi355ndt_gicp_set_source_keyframe
            self._chk(fn(self.h, int(kid)), name + "_keyframe")
            n = self.keyframe_get(int(kid), fetch=False)
        else:
            a = _as_points(cloud)
            fn = self.lib.mi355ndt_gicp_set_target if role == GICP_TARGET else self.lib.mi355ndt_gicp_set_source
            self._chk(fn(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), name)
            n = a.shape[0]
        self._gicp_n[role] = int(n)

    def gicp_set_target(self, cloud=None, keyframe=None):
        """the target cloud: a host cloud, or a resident keyframe by id (its covariances stay with the keyframe)"""
        self._gicp_set(GICP_TARGET, cloud, keyframe)

    def gicp_set_source(self, cloud=None, keyframe=None):
        self._gicp_set(GICP_SOURCE, cloud, keyframe)

    def gicp_covariances(self, role: int, fetch: bool = True):
        """computeCovariances of the target (GICP_TARGET) or source (GICP_SOURCE): [n, 3, 3] f64, zeros for a non-finite point"""
        n = self._gicp_n[role]
        out = np.zeros((n, 3, 3), np.float64)
        self._chk(self.lib.mi355ndt_gicp_covariances(self.h, role, out.ctypes.data_as(C.c_void_p) if fetch else None, n), "gicp_covariances")
        return out if fetch else None

    def gicp_correspondences(self, guess, T=None):
        """one pass of the matching loop: (idx [n_src] int32, -1 = none; M [n_src, 3, 3] f64; m)"""
        n = self._gicp_n[GICP_SOURCE]
        g = _colmajor(guess)
        t = _colmajor(T) if T is not None else None
        idx, M, m = np.zeros(n, np.int32), np.zeros((n, 3, 3), np.float64), C.c_int(0)
        self._chk(self.lib.mi355ndt_gicp_correspondences(self.h, g.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p) if t is not None else None,
                                                         idx.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), C.byref(m)), "gicp_correspondences")
        return idx, M, m.value

    def gicp_cost(self, x, base):
        """fdf over the resident correspondences at the state x[6] with base transformation `base`: (f, g[6])"""
        xx = np.ascontiguousarray(x, np.float64)
        b = _colmajor(base)
        f, g = C.c_double(0.0), np.zeros(6, np.float64)
        self._chk(self.lib.mi355ndt_gicp_cost(self.h, xx.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(f), g.ctypes.data_as(C.c_void_p)), "gicp_cost")
        return f.value, g

    def gicp_align(self, guess) -> dict:
        g = _colmajor(guess)
        r = GicpResult()
        self._chk(self.lib.mi355ndt_gicp_align(self.h, g.ctypes.data_as(C.c_void_p), C.byref(r)), "gicp_align")
        return dict(final=np.array(r.final_colmajor, np.float32).reshape(4, 4).T.copy(), converged=bool(r.converged), iterations=r.iterations,
                    inner_status=r.inner_status, n_matched=r.n_matched, delta=r.delta)

    def gicp_get_aligned(self) -> np.ndarray:
        out = np.zeros((self._gicp_n[GICP_SOURCE], 3), np.float32)
        if len(out):
            self._chk(self.lib.mi355ndt_gicp_get_aligned(self.h, out.ctypes.data_as(C.c_void_p), 12), "gicp_get_aligned")
        return out

    # -- GICP, all candidates of a loop check in one lockstep batch (the target and the parameters are the single-pair surface's)
    def gicp_batch_reserve(self, n_slots: int):
        self._chk(self.lib.mi355ndt_gicp_batch_reserve(self.h, int(n_slots)), "gicp_batch_reserve")
        self._gicp_batch_n = [0] * int(n_slots)

    def gicp_batch_set_source(self, slot: int, cloud=None, keyframe=None):
        """candidate `slot`: a host cloud, or a resident keyframe by id (its index and covariances stay with the keyframe)"""
        if keyframe is not None:
            self._chk(self.lib.mi355ndt_gicp_batch_set_source_keyframe(self.h, int(slot), int(keyframe)), "gicp_batch_set_source_keyframe")
            n = self.keyframe_get(int(keyframe), fetch=False)
        else:
            a = _as_points(cloud)
            self._chk(self.lib.mi355ndt_gicp_batch_set_source(self.h, int(slot), a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "gicp_batch_set_source")
            n = a.shape[0]
        self._gicp_batch_n[int(slot)] = int(n)

    def gicp_batch_align(self, guesses) -> list:
        """one lockstep align of every slot from guesses [K,4,4]: gicp_align's dict per slot, the same bytes as the single-pair surface gives"""
        K = len(self._gicp_batch_n)
        G = np.asarray(guesses, np.float32)
        if G.shape != (K, 4, 4):
            raise ValueError(f"guesses must be [{K},4,4]")
        g = np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(max(K, 1), 16) if K else np.zeros((1, 16), np.float32)
        res = (GicpResult * max(K, 1))()
        self._chk(self.lib.mi355ndt_gicp_batch_align(self.h, g.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)), "gicp_batch_align")
        return [dict(final=np.array(r.final_colmajor, np.float32).reshape(4, 4).T.copy(), converged=bool(r.converged), iterations=r.iterations,
                     inner_status=r.inner_status, n_matched=r.n_matched, delta=r.delta) for r in res[:K]]

    def gicp_batch_get_aligned(self, slot: int) -> np.ndarray:
        if not 0 <= int(slot) < len(self._gicp_batch_n):
            self._chk(self.lib.mi355ndt_gicp_batch_get_aligned(self.h, int(slot), np.zeros(3, np.float32).ctypes.data_as(C.c_void_p), 12), "gicp_batch_get_aligned")
        out = np.zeros((self._gicp_batch_n[int(slot)], 3), np.float32)
        if len(out):
            self._chk(self.lib.mi355ndt_gicp_batch_get_aligned(self.h, int(slot), out.ctypes.data_as(C.c_void_p), 12), "gicp_batch_get_aligned")
        return out

    def gicp_batch_stats(self):
        """(rounds, requests[K]) of the last batch align: waits on the device; device requests (matching passes + cost evaluations) per slot"""
        K = len(self._gicp_batch_n)
        rounds, req = C.c_int(0), np.zeros(max(K, 1), np.int32)
        self._chk(self.lib.mi355ndt_gicp_batch_stats(self.h, C.byref(rounds), req.ctypes.data_as(C.c_void_p)), "gicp_batch_stats")
        return rounds.value, req[:K].copy()

    # -- ICP (pcl::IterativeClosestPoint, registration_method = ICP): one pair, synchronous (the batch form follows)
    def icp_set_params(self, p: IcpParams):
        self._chk(self.lib.mi355ndt_icp_set_params(self.h, C.byref(p)), "icp_set_params")

    def _icp_set(self, role: int, cloud=None, kid=None):
        name = "icp_set_target" if role == GICP_TARGET else "icp_set_source"
        if kid is not None:
            fn = self.lib.mi355ndt_icp_set_target_keyframe if role == GICP_TARGET else self.lib.mi355ndt_icp_set_source_keyframe
            self._chk(fn(self.h, int(kid)), name + "_keyframe")
            n = self.keyframe_get(int(kid), fetch=False)
        else:
            a = _as_points(cloud)
            fn = self.lib.mi355ndt_icp_set_target if role == GICP_TARGET else self.lib.mi355ndt_icp_set_source
            self._chk(fn(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), name)
            n = a.shape[0]
        self._icp_n[role] = int(n)

    def icp_set_target(self, cloud=None, keyframe=None):
        """the target cloud: a host cloud, or a resident keyframe by id (searched through the keyframe's one index)"""
        self._icp_set(GICP_TARGET, cloud, keyframe)

    def icp_set_source(self, cloud=None, keyframe=None):
        """the source cloud: a host cloud, or a resident keyframe by id (never written: the working cloud is the surface's own)"""
        self._icp_set(GICP_SOURCE, cloud, keyframe)

    def icp_correspondences(self, guess, T=None):
        """one step on a fresh working cloud T (guess p): (idx [n] int32, -1 = none; d2 [n] f32, 0 where unmatched; sums [16] f64; m)"""
        n = self._icp_n[GICP_SOURCE]
        g = _colmajor(guess)
        t = _colmajor(T) if T is not None else None
        idx, d2, sums, m = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32), np.zeros(16, np.float64), C.c_int(0)
        self._chk(self.lib.mi355ndt_icp_correspondences(self.h, g.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p) if t is not None else None,
                                                        idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p),
                                                        C.byref(m)), "icp_correspondences")
        return idx[:n], d2[:n], sums, m.value

    def icp_align(self, guess) -> dict:
        """align(output, guess): final, converged, iterations, state (mi355ndt_icp_state; names: ICP_STATES), matches, mse"""
        g = _colmajor(guess)
        r = IcpResult()
        self._chk(self.lib.mi355ndt_icp_align(self.h, g.ctypes.data_as(C.c_void_p), C.byref(r)), "icp_align")
        return _icp_result_dict(r)

    def icp_get_aligned(self) -> np.ndarray:
        out = np.zeros((max(self._icp_n[GICP_SOURCE], 1), 3), np.float32)
        self._chk(self.lib.mi355ndt_icp_get_aligned(self.h, out.ctypes.data_as(C.c_void_p), 12), "icp_get_aligned")
        return out[: self._icp_n[GICP_SOURCE]]

    # -- ICP, all candidates of a loop check in one batch (the target and the parameters are the single-pair surface's)
    def icp_batch_reserve(self, n_slots: int):
        self._chk(self.lib.mi355ndt_icp_batch_reserve(self.h, int(n_slots)), "icp_batch_reserve")
        self._icp_batch_n = [0] * int(n_slots)

    def icp_batch_set_source(self, slot: int, cloud=None, keyframe=None):
        """candidate `slot`: a host cloud, or a resident keyframe by id"""
        if keyframe is not None:
            self._chk(self.lib.mi355ndt_icp_batch_set_source_keyframe(self.h, int(slot), int(keyframe)), "icp_batch_set_source_keyframe")
            n = self.keyframe_get(int(keyframe), fetch=False)
        else:
            a = _as_points(cloud)
            self._chk(self.lib.mi355ndt_icp_batch_set_source(self.h, int(slot), a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "icp_batch_set_source")
            n = a.shape[0]
        self._icp_batch_n[int(slot)] = int(n)

    def icp_batch_align(self, guesses) -> list:
        """one batch align of every slot from guesses [K,4,4]: icp_align's dict per slot, the same bytes as the single-pair surface gives"""
        K = len(self._icp_batch_n)
        G = np.asarray(guesses, np.float32)
        if G.shape != (K, 4, 4):
            raise ValueError(f"guesses must be [{K},4,4]")
        g = np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(max(K, 1), 16) if K else np.zeros((1, 16), np.float32)
        res = (IcpResult * max(K, 1))()
        self._chk(self.lib.mi355ndt_icp_batch_align(self.h, g.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)), "icp_batch_align")
        return [_icp_result_dict(r) for r in res[:K]]

    def icp_batch_get_aligned(self, slot: int) -> np.ndarray:
        n = self._icp_batch_n[int(slot)] if 0 <= int(slot) < len(self._icp_batch_n) else 0
        out = np.zeros((max(n, 1), 3), np.float32)
        self._chk(self.lib.mi355ndt_icp_batch_get_aligned(self.h, int(slot), out.ctypes.data_as(C.c_void_p), 12), "icp_batch_get_aligned")
        return out[:n]

    def icp_batch_stats(self):
        """(rounds, requests[K]) of the last batch align: waits on the device; steps per slot"""
        K = len(self._icp_batch_n)
        rounds, req = C.c_int(0), np.zeros(max(K, 1), np.int32)
        self._chk(self.lib.mi355ndt_icp_batch_stats(self.h, C.byref(rounds), req.ctypes.data_as(C.c_void_p)), "icp_batch_stats")
        return rounds.value, req[:K].copy()

    # -- parity hooks
    def derivatives(self, p):
        p = np.ascontiguousarray(p, np.float64)
        s, hits = C.c_double(), C.c_longlong()
        g, H = np.zeros(6), np.zeros(36)
        self._chk(self.lib.mi355ndt_derivatives(self.h, p.ctypes.data_as(C.c_void_p), C.byref(s), g.ctypes.data_as(C.c_void_p),
                                                H.ctypes.data_as(C.c_void_p), C.byref(hits)), "derivatives")
        return s.value, g, H.reshape(6, 6), hits.value

    def compute_hessian(self, p):
        """computeHessian (ndt_omp_impl2.hpp:622-679) at tangent p -> H[6,6] f64."""
        p = np.ascontiguousarray(p, np.float64)
        H = np.zeros(36)
        self._chk(self.lib.mi355ndt_compute_hessian(self.h, p.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)), "compute_hessian")
        return H.reshape(6, 6)

    def derivatives_T(self, T, Rj):
        t = _colmajor(T)
        r = np.ascontiguousarray(np.asarray(Rj, np.float32)).ravel()
        s, hits = C.c_double(), C.c_longlong()
        g, H = np.zeros(6), np.zeros(36)
        self._chk(self.lib.mi355ndt_derivatives_T(self.h, t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.byref(s),
                                                  g.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p), C.byref(hits)), "derivatives_T")
        return s.value, g, H.reshape(6, 6), hits.value

    def get_grid(self, pair: int = 0):
        mn, mx, dv = (np.zeros(3, np.int32) for _ in range(3))
        nv = C.c_int()
        self._chk(self.lib.mi355ndt_get_grid(self.h, pair, mn.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p),
                                             dv.ctypes.data_as(C.c_void_p), C.byref(nv)), "get_grid")
        return mn, mx, dv, nv.value

    def get_voxels(self, pair: int = 0) -> np.ndarray:
        nv = self.get_grid(pair)[3]
        arr = (Voxel * max(nv, 1))()
        self._chk(self.lib.mi355ndt_get_voxels(self.h, pair, C.cast(arr, C.c_void_p), nv), "get_voxels")
        dt = np.dtype([("idx", "<i4"), ("n", "<i4"), ("mean", "<f8", 3), ("icov", "<f4", 9), ("weight", "<i4")], align=True)
        assert dt.itemsize == C.sizeof(Voxel)
        return np.frombuffer(bytes(arr), dtype=dt)[:nv].copy()

    def get_build_buffer(self, which, pair: int = 0) -> np.ndarray:
        """One target's part of one buffer of the last synchronous batch_build_targets (mi355ndt_get_build_buffer), decoded by BUILD_BUFFERS:
        `which` is a name of that table or its number.  Read-only; NDTError -2 for a buffer the build did not make."""
        table = {**BUILD_BUFFERS, **GROUND_BUILD_BUFFERS}
        code, dt = table[which] if isinstance(which, str) else next(v for v in table.values() if v[0] == which)
        nb = C.c_size_t(0)
        self._chk(self.lib.mi355ndt_get_build_buffer(self.h, code, pair, None, 0, C.byref(nb)), "get_build_buffer")
        raw = np.zeros(max(nb.value, 1), np.uint8)
        self._chk(self.lib.mi355ndt_get_build_buffer(self.h, code, pair, raw.ctypes.data_as(C.c_void_p), nb.value, C.byref(nb)), "get_build_buffer")
        return raw[:nb.value].view(dt).copy()

    # -- batch
    def batch_reserve(self, n_pairs, max_target_pts, max_source_pts):
        self._chk(self.lib.mi355ndt_batch_reserve(self.h, n_pairs, max_target_pts, max_source_pts), "batch_reserve")

    def batch_set_target(self, pair, cloud):
        a = _as_points(cloud)
        self._chk(self.lib.mi355ndt_batch_set_target(self.h, pair, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "batch_set_target")

    def batch_set_source(self, pair, cloud):
        a = _as_points(cloud)
        self._chk(self.lib.mi355ndt_batch_set_source(self.h, pair, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]), "batch_set_source")

    def batch_set_target_keyframe(self, pair: int, kid: int):
        """batch_set_target with a resident keyframe, device to device."""
        self._chk(self.lib.mi355ndt_batch_set_target_keyframe(self.h, pair, int(kid)), "batch_set_target_keyframe")

    def batch_set_source_keyframe(self, pair: int, kid: int):
        self._chk(self.lib.mi355ndt_batch_set_source_keyframe(self.h, pair, int(kid)), "batch_set_source_keyframe")

    def batch_set_target_raw(self, pair: int, ptr: int, n: int, stride: int):
        """batch_set_target on a raw host pointer (records `stride` bytes apart); thread-safe across different pairs."""
        self._chk(self.lib.mi355ndt_batch_set_target(self.h, pair, C.c_void_p(ptr), n, stride), "batch_set_target")

    def batch_set_source_raw(self, pair: int, ptr: int, n: int, stride: int):
        self._chk(self.lib.mi355ndt_batch_set_source(self.h, pair, C.c_void_p(ptr), n, stride), "batch_set_source")

    def batch_set_clouds_raw(self, first_pair: int, tgt_ptrs, tgt_counts, src_ptrs, src_counts, stride: int, threads: int = 8):
        """mi355ndt_batch_set_clouds: arrays of host pointers / point counts (numpy uint64), one per pair; either side may be None."""
        n = len(tgt_ptrs if tgt_ptrs is not None else src_ptrs)
        arr = lambda a: None if a is None else np.ascontiguousarray(a, np.uint64)
        tp, tc, sp, sc = arr(tgt_ptrs), arr(tgt_counts), arr(src_ptrs), arr(src_counts)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.mi355ndt_batch_set_clouds(self.h, first_pair, n, ptr(tp), ptr(tc), ptr(sp), ptr(sc), stride, threads), "batch_set_clouds")

    def batch_prefilter(self, targets, sources, first_pair=0, distance_near=0.5, distance_far=100.0, downsample_resolution=0.1,
                        use_distance_filter=True, transform=None, outlier=None, downsample_method="VOXELGRID", angle_calibration=False,
                        intensity=False):
        """mi355ndt_batch_prefilter: lists of RAW clouds ([N,>=3], x,y,z first; either list may be None) through PrefilteringNodelet's distance
        filter and VoxelGrid down-sampling (Engine.prefilter's rules and keyword defaults) into the batch slots first_pair ...; batch_reserve
        comes first, sized for the FILTERED clouds.  transform: a 4x4 applied to every raw point first (the nodelet's base_link move).
        downsample_method: "VOXELGRID" or "APPROX_VOXELGRID" (pcl::ApproximateVoxelGrid: a cell may come out more than once, a slot may need
        as many points as the raw cloud has); angle_calibration: False, True (the nodelet's 0.11 degrees) or radians -- the nodelet's
        vertical_angle_calibration, after the move and before the gate.
        outlier: a dict of batch_remove_outliers' keywords (may be empty: the nodelet's in-code defaults) -- the nodelet's third stage runs
        over the same slots and sides right after, and the counts returned are those after both stages.
        intensity: column 3 of the [N,>=4] clouds is the points' intensity and goes through the chain into the slots' intensity rows
        (batch_get_cloud(intensity=True), keyframe_from_slot); the outlier stage keeps the survivors'.
        Returns (target counts, source counts) after the filter, None for a side not given."""
        if intensity:
            for c in list(targets or []) + list(sources or []):
                self._records(c, True)
        if targets is None and sources is None:
            raise ValueError("give targets, sources or both")
        if targets is not None and sources is not None and len(targets) != len(sources):
            raise ValueError("one source per target")
        oprm = None if outlier is None else _outlier_dict(outlier)
        prm = _prefilter_params(distance_near, distance_far, downsample_resolution, use_distance_filter, transform, downsample_method, angle_calibration,
                                intensity)
        n = len(targets if targets is not None else sources)
        both = _cloud_table(list(targets or []) + list(sources or []), widen=True)     # (one stride for the whole call)
        nt = len(targets) if targets is not None else 0
        tabs = [None if targets is None else (both[1][:nt].copy(), both[2][:nt].copy()), None if sources is None else (both[1][nt:].copy(), both[2][nt:].copy())]
        outs = [None if t is None else np.zeros(max(n, 1), np.uint64) for t in tabs]
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        tt, ts = tabs
        self._chk(self.lib.mi355ndt_batch_prefilter(self.h, int(first_pair), n, ptr(tt and tt[0]), ptr(tt and tt[1]), ptr(ts and ts[0]), ptr(ts and ts[1]),
                                                    both[3], _base_ref(prm), ptr(outs[0]), ptr(outs[1])), "batch_prefilter")
        if oprm is not None:
            self._chk(self.lib.mi355ndt_batch_remove_outliers(self.h, int(first_pair), n, (2 if targets is not None else 0) | (1 if sources is not None else 0),
                                                              C.byref(oprm), ptr(outs[0]), ptr(outs[1]), None, None), "batch_remove_outliers")
        return tuple(None if o is None else [int(c) for c in o[:n]] for o in outs)

    def batch_remove_outliers(self, first_pair=0, n=None, targets=True, sources=True, method="STATISTICAL", mean_k=20, stddev_mul=1.0, radius=0.8,
                              min_neighbors=2, return_stats=False):
        """mi355ndt_batch_remove_outliers: PrefilteringNodelet::outlier_removal over the clouds batch slots first_pair .. first_pair + n - 1
        hold (n=None: to the end of the batch), in place, whatever route filled them -- prefilter_outliers' rules and keywords per cloud
        ("RADIUS" is the filter the reference builds and never runs: prefiltering_nodelet.cpp:71-78), all clouds of a group in one launch
        chain.  Returns (target counts, source counts), None for a side not asked for; with return_stats also (target stats, source stats):
        per cloud a dict n_in, n_valid, mean, stddev, threshold (zeros for RADIUS and for an empty slot)."""
        sides = (2 if targets else 0) | (1 if sources else 0)
        if not sides:
            raise ValueError("give targets, sources or both")
        prm = _outlier_params(method, mean_k, stddev_mul, radius, min_neighbors)
        first_pair = int(first_pair)
        if n is None:
            n = self.lib.mi355ndt_batch_size(self.h) - first_pair
        n = int(n)
        m = max(n, 1)
        cnt = [np.zeros(m, np.uint64) if targets else None, np.zeros(m, np.uint64) if sources else None]
        st = [(OutlierStats * m)() if targets and return_stats else None, (OutlierStats * m)() if sources and return_stats else None]
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        sp = lambda a: None if a is None else C.cast(a, C.c_void_p)
        self._chk(self.lib.mi355ndt_batch_remove_outliers(self.h, first_pair, n, sides, C.byref(prm), ptr(cnt[0]), ptr(cnt[1]), sp(st[0]), sp(st[1])),
                  "batch_remove_outliers")
        counts = tuple(None if c is None else [int(v) for v in c[:n]] for c in cnt)
        if not return_stats:
            return counts
        return counts + tuple(None if a is None else [{k: getattr(a[j], k) for k, _ in OutlierStats._fields_} for j in range(n)] for a in st)

    def batch_get_cloud(self, pair: int, target: bool, intensity: bool = False) -> np.ndarray:
        """The points batch slot `pair` holds on its target (or source) side, [M,3] f32, whatever route filled it.  intensity: [M,4], with
        the intensities batch_prefilter(intensity=True) left in the slot (zeros for a slot filled by any other route)."""
        role, m = 2 if target else 1, C.c_size_t()
        self._chk(self.lib.mi355ndt_batch_get_cloud(self.h, int(pair), role, None, 0, 12, C.byref(m)), "batch_get_cloud")
        if intensity:
            out = np.zeros((m.value, 4), np.float32)
            self._chk(self.lib.mi355ndt_batch_get_cloud_i(self.h, int(pair), role, out.ctypes.data_as(C.c_void_p), m.value, 16, 12, C.byref(m)),
                      "batch_get_cloud_i")
            return out
        out = np.zeros((m.value, 3), np.float32)
        self._chk(self.lib.mi355ndt_batch_get_cloud(self.h, int(pair), role, out.ctypes.data_as(C.c_void_p), m.value, 12, C.byref(m)), "batch_get_cloud")
        return out

    def batch_bind_device(self, d_targets_ptr: int, target_counts, target_pitch: int, d_sources_ptr: int, source_counts, source_pitch: int):
        """Zero-copy device buffers laid out [pair][3][pitch] float32.  The caller keeps them alive."""
        tc = np.ascontiguousarray(target_counts, np.int32)
        sc = np.ascontiguousarray(source_counts, np.int32)
        assert len(tc) == len(sc)
        self._chk(self.lib.mi355ndt_batch_bind_device(self.h, len(tc), C.c_void_p(d_targets_ptr), tc.ctypes.data_as(C.c_void_p), target_pitch,
                                                      C.c_void_p(d_sources_ptr), sc.ctypes.data_as(C.c_void_p), source_pitch), "batch_bind_device")

    def batch_build_targets(self):
        self._chk(self.lib.mi355ndt_batch_build_targets(self.h), "batch_build_targets")

    def batch_align(self, guesses) -> list[dict]:
        G = np.asarray(guesses, np.float32)
        n = self.lib.mi355ndt_batch_size(self.h)
        if G.shape == (4, 4):
            G = np.broadcast_to(G, (n, 4, 4))
        if G.shape != (n, 4, 4):
            raise ValueError(f"guesses must be [{n},4,4]")
        gc = np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(n, 16)
        res = (Result * n)()
        self._chk(self.lib.mi355ndt_batch_align(self.h, gc.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)), "batch_align")
        return [_result_dict(r) for r in res]

    def batch_align_raw(self, guesses_colmajor: np.ndarray, res_array):
        """Allocation-free variant for timing loops: guesses [n,16] f32 C-contiguous, res_array = (Result*n)()."""
        self._chk(self.lib.mi355ndt_batch_align(self.h, guesses_colmajor.ctypes.data_as(C.c_void_p), C.cast(res_array, C.c_void_p)), "batch_align")

    def batch_pose_records(self, id_base: int, id_stride: int, d_records_ptr: int, capacity: int):
        """96-byte pose records of the last batch_align, packed on the device into a caller-owned device buffer (dist.py layout)."""
        self._chk(self.lib.mi355ndt_batch_pose_records(self.h, id_base, id_stride, C.c_void_p(d_records_ptr), capacity), "batch_pose_records")

    def batch_fitness_scores(self, max_range: float = float("inf"), T=None):
        """getFitnessScore(max_range) of every batch slot in one call: (scores float64[n], inliers int64[n]).  T = [n,4,4], one [4,4]
        for all pairs, or None = each pair's final pose of the last batch_align (identity before any).  Bit for bit fitness_score() of a
        one-pair engine holding the same clouds and transform; a pair with an empty source or target scores (DBL_MAX, 0), where
        fitness_score() refuses."""
        n = self.lib.mi355ndt_batch_size(self.h)
        if n < 0:
            raise NDTError(n, "batch_fitness_scores")
        mr = 1.7976931348623157e308 if max_range == float("inf") else float(max_range)
        t = None
        if T is not None:
            M = np.asarray(T, np.float32)
            if M.shape == (4, 4):
                M = np.broadcast_to(M, (n, 4, 4))
            if M.shape != (n, 4, 4):
                raise ValueError(f"T must be [{n},4,4] or [4,4]")
            t = np.ascontiguousarray(np.transpose(M, (0, 2, 1))).reshape(n, 16)
        scores = np.zeros(max(n, 1), np.float64)
        inliers = np.zeros(max(n, 1), np.int64)
        self._chk(self.lib.mi355ndt_batch_fitness_scores(self.h, None if t is None else t.ctypes.data_as(C.c_void_p), mr,
                                                         scores.ctypes.data_as(C.c_void_p), inliers.ctypes.data_as(C.c_void_p)),
                  "batch_fitness_scores")
        return scores[:n], inliers[:n]

    def batch_score_poses(self, pairs, poses):
        """The score and the hit count of one derivative sweep for every (pair of the bound batch, 4x4 f32 pose) item, in one call
        (mi355ndt_batch_score_poses): (scores float64[n], hits int64[n]).  pairs: n slot indices, in any order, repeated or left out at
        will; poses: [n,4,4], or one [4,4] for all items.  Item e's two words are bit for bit derivatives_T(poses[e], any Rj) of a one-pair
        engine holding pair pairs[e]'s clouds; no gradient, no Hessian, and nothing of the batch's align state changes.  Not a call of the
        reference: loop_closure.verify_candidates_search picks start poses with it."""
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).ravel())
        n = int(pr.shape[0])
        M = np.asarray(poses, np.float32)
        if M.shape == (4, 4):
            M = np.broadcast_to(M, (n, 4, 4))
        if M.shape != (n, 4, 4):
            raise ValueError(f"poses must be [{n},4,4] or [4,4]")
        t = np.ascontiguousarray(np.transpose(M, (0, 2, 1))).reshape(n, 16)
        scores = np.zeros(max(n, 1), np.float64)
        hits = np.zeros(max(n, 1), np.int64)
        self._chk(self.lib.mi355ndt_batch_score_poses(self.h, n, pr.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                      scores.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)), "batch_score_poses")
        return scores[:n], hits[:n]

    def synchronize(self):
        self._chk(self.lib.mi355ndt_synchronize(self.h), "synchronize")

    # -- stream mode: batches overlap on the GPU (mi355ndt_stream_*)
    def stream_begin(self, n_contexts: int, max_pairs: int, max_target_pts: int, max_source_pts: int):
        self._chk(self.lib.mi355ndt_stream_begin(self.h, n_contexts, max_pairs, max_target_pts, max_source_pts), "stream_begin")

    def stream_submit(self, d_targets_ptr: int, target_counts, target_pitch: int, d_sources_ptr: int, source_counts, source_pitch: int,
                      guesses_colmajor: np.ndarray) -> int:
        """Enqueue one batch (device-resident SoA buffers as in batch_bind_device; they must stay unchanged until the batch is collected).
        Returns the batch id at once."""
        tc = np.ascontiguousarray(target_counts, np.int32)
        sc = np.ascontiguousarray(source_counts, np.int32)
        g = np.ascontiguousarray(guesses_colmajor, np.float32)
        assert len(tc) == len(sc) and g.size == 16 * len(tc)
        bid = C.c_longlong(-1)
        self._chk(self.lib.mi355ndt_stream_submit(self.h, len(tc), C.c_void_p(d_targets_ptr), tc.ctypes.data_as(C.c_void_p), target_pitch,
                                                  C.c_void_p(d_sources_ptr), sc.ctypes.data_as(C.c_void_p), source_pitch,
                                                  g.ctypes.data_as(C.c_void_p), C.byref(bid)), "stream_submit")
        return bid.value

    def stream_submit_host_raw(self, tgt_ptrs, tgt_counts, src_ptrs, src_counts, stride: int, guesses_colmajor: np.ndarray, threads: int = 8) -> int:
        """Enqueue one batch of HOST clouds (arrays of record pointers and point counts, as batch_set_clouds_raw takes them); returns the batch id
        as soon as the caller's memory is no longer needed."""
        tp = np.ascontiguousarray(tgt_ptrs, np.uint64); sp = np.ascontiguousarray(src_ptrs, np.uint64)
        tc = np.ascontiguousarray(tgt_counts, np.uint64); sc = np.ascontiguousarray(src_counts, np.uint64)
        g = np.ascontiguousarray(guesses_colmajor, np.float32)
        assert len(tp) == len(sp) == len(tc) == len(sc) and g.size == 16 * len(tp)
        bid = C.c_longlong(-1)
        self._chk(self.lib.mi355ndt_stream_submit_host(self.h, len(tp), tp.ctypes.data_as(C.c_void_p), tc.ctypes.data_as(C.c_void_p), sp.ctypes.data_as(C.c_void_p),
                                                       sc.ctypes.data_as(C.c_void_p), C.c_size_t(stride), g.ctypes.data_as(C.c_void_p), int(threads), C.byref(bid)), "stream_submit_host")
        return bid.value

    def stream_pose_records(self, d_records_ptr: int, capacity: int, id_base: int, id_stride: int):
        """The NEXT submitted batch's 96-byte pose records go into this device buffer, written by the device as the pairs finish."""
        self._chk(self.lib.mi355ndt_stream_pose_records(self.h, C.c_void_p(d_records_ptr), capacity, id_base, id_stride), "stream_pose_records")

    def stream_collect_raw(self, batch_id: int, res_array):
        """Block until every pair of the batch is finalised; res_array = (Result * n_pairs)()."""
        self._chk(self.lib.mi355ndt_stream_collect(self.h, batch_id, C.cast(res_array, C.c_void_p)), "stream_collect")

    def stream_collect(self, batch_id: int, n_pairs: int) -> list[dict]:
        res = (Result * n_pairs)()
        self.stream_collect_raw(batch_id, res)
        return [_result_dict(r) for r in res]

    def stream_end(self):
        self._chk(self.lib.mi355ndt_stream_end(self.h), "stream_end")

    # -- latency mode
    def set_latency_mode(self, on: bool = True):
        """Opt-in fine-grained sweep for small batches (a single registration above all); see mi355ndt_set_latency_mode."""
        self._chk(self.lib.mi355ndt_set_latency_mode(self.h, int(on)), "set_latency_mode")

    def sequence_run(self, frames, stamps, keyframe_delta_trans=5.0, keyframe_delta_angle=0.17, keyframe_delta_time=1.0, raw_records=False):
        """mi355ndt_sequence_run: a run of frames tracked on the device the way ScanMatchingOdomNodelet::matching_s2k tracks them
        (scan_matching_odom_nodelet.cpp:192-261).  frames: list of [N,>=3] float arrays (x,y,z first); stamps: seconds.
        Returns (list of per-frame dicts, stats dict); raw_records=True returns the (SeqFrame * n, Result * n) arrays in place of the dicts."""
        clouds = [_as_points(f) for f in frames]
        n = len(clouds)
        strides = {c.strides[0] for c in clouds if c.shape[0]} or {12}       # (numpy gives empty arrays zero strides)
        if len(strides) != 1:
            raise ValueError("all frames must share one record stride")
        ptrs = np.array([c.ctypes.data for c in clouds], np.uint64)
        cnts = np.array([c.shape[0] for c in clouds], np.uint64)
        st = np.ascontiguousarray(stamps, np.float64)
        if len(st) != n:
            raise ValueError("one stamp per frame")
        sp = SeqParams(keyframe_delta_trans, keyframe_delta_angle, keyframe_delta_time)
        out, res, stats = (SeqFrame * n)(), (Result * n)(), SeqStats()
        self._chk(self.lib.mi355ndt_sequence_run(self.h, n, ptrs.ctypes.data_as(C.c_void_p), cnts.ctypes.data_as(C.c_void_p), strides.pop(),
                                                 st.ctypes.data_as(C.c_void_p), C.byref(sp), C.cast(out, C.c_void_p), C.cast(res, C.c_void_p),
                                                 C.byref(stats)), "sequence_run")
        return ((out, res) if raw_records else _seq_frames_out(out, res)), {k: getattr(stats, k) for k, _ in SeqStats._fields_}

    def sequence_run_raw(self, frames, stamps, keyframe_delta_trans=5.0, keyframe_delta_angle=0.17, keyframe_delta_time=1.0,
                         distance_near=0.5, distance_far=100.0, downsample_resolution=0.1, use_distance_filter=True, transform=None, raw_records=False,
                         outlier=None, downsample_method="VOXELGRID", angle_calibration=False, intensity=False):
        """mi355ndt_sequence_run_raw: sequence_run over RAW scans, the batch prefilter (batch_prefilter's keywords) in front and no scan
        downloaded in between.  outlier: a dict of batch_remove_outliers' keywords (may be empty: the nodelet's in-code defaults) -- the
        nodelet's third stage runs between the prefilter and the run (mi355ndt_sequence_run_raw_outliers); the filtered counts and
        prefilter_ms then cover both stages.  intensity: batch_prefilter's keyword -- the frames' slots (target side) carry the filtered
        intensities afterwards; the run itself does not look at them.  Returns (list of per-frame dicts, stats dict with prefilter_ms added, filtered counts); raw_records=True
        returns the (SeqFrame * n, Result * n) arrays in place of the dicts."""
        prm = _prefilter_params(distance_near, distance_far, downsample_resolution, use_distance_filter, transform, downsample_method, angle_calibration,
                                intensity)
        oprm = None if outlier is None else _outlier_dict(outlier)
        if intensity:
            for f in frames:
                self._records(f, True)
        clouds, ptrs, cnts, stride = _cloud_table(frames)
        n = len(clouds)
        st = np.ascontiguousarray(stamps, np.float64)
        if len(st) != n:
            raise ValueError("one stamp per frame")
        sp = SeqParams(keyframe_delta_trans, keyframe_delta_angle, keyframe_delta_time)
        out, res, stats = (SeqFrame * n)(), (Result * n)(), SeqStats()
        filtered, pf_ms = np.zeros(max(n, 1), np.uint64), C.c_double()
        head = (self.h, n, ptrs.ctypes.data_as(C.c_void_p), cnts.ctypes.data_as(C.c_void_p), stride, st.ctypes.data_as(C.c_void_p), _base_ref(prm))
        tail = (C.byref(sp), C.cast(out, C.c_void_p), C.cast(res, C.c_void_p), C.byref(stats), filtered.ctypes.data_as(C.c_void_p), C.byref(pf_ms))
        if oprm is None:
            self._chk(self.lib.mi355ndt_sequence_run_raw(*head, *tail), "sequence_run_raw")
        else:
            self._chk(self.lib.mi355ndt_sequence_run_raw_outliers(*head, C.byref(oprm), *tail), "sequence_run_raw_outliers")
        sd = {k: getattr(stats, k) for k, _ in SeqStats._fields_}
        sd["prefilter_ms"] = pf_ms.value
        return ((out, res) if raw_records else _seq_frames_out(out, res)), sd, [int(c) for c in filtered[:n]]

    # -- profiling
    def profile_enable(self, on=True):
        self._chk(self.lib.mi355ndt_profile_enable(self.h, int(on)), "profile_enable")

    def profile_reset(self):
        self._chk(self.lib.mi355ndt_profile_reset(self.h), "profile_reset")

    def profile_get(self) -> dict:
        p = Profile()
        self._chk(self.lib.mi355ndt_profile_get(self.h, C.byref(p)), "profile_get")
        return {k: getattr(p, k) for k, _ in Profile._fields_}


class NormalDistributionsTransform:
    """Drop-in mirror of pclomp::NormalDistributionsTransform / pclpca::NormalDistributionsTransform.

    variant=VARIANT_OMP -> include/ndt_omp/ndt_omp.h ; variant=VARIANT_PCA -> include/ndt_pca/ndt_pca.h.
    Method names (including the reference's `setOulierRatio` spelling) follow ndt_omp.h:109-203 and
    pcl::Registration.  PCL-style error behaviour: no exceptions for a failed registration --
    `hasConverged()` reports it; exceptions are reserved for API misuse and HIP failures.

    pose_model="se3" (default) is include/ndt_omp/ndt_omp_impl2.hpp, the implementation lv_slam compiles; pose_model="euler" is
    include/ndt_omp/ndt_omp_impl.hpp, the Euler-angle NDT a host gets by changing the include line of src/ndt_omp/ndt_omp.cpp
    (mi355ndt_set_option(MI355NDT_OPT_POSE_MODEL, 1): variant OMP, step_size > trans_epsilon / 2).

    ndt_class="omp" (default) is pclomp's class; ndt_class="pcl" is pcl::NormalDistributionsTransform, the class select_registration_method
    hands out for registration_method = NDT (mi355ndt_set_option(MI355NDT_OPT_NDT_CLASS, 1)): the Euler pose vector, the radius search and an
    f64 evaluation.  PCL's class has neither setNeighborhoodSearchMethod nor setNumThreads, and neither has this object then.

    ground_class="horizontal" | "vertical" | "all" (default None: off) is pclomp_ground::NormalDistributionsTransformGround with flag_class
    1 | 2 | 0 (mi355ndt_set_option(MI355NDT_OPT_GROUND_CLASS, 1 | 2 | 3)): variant OMP, DIRECT1 / DIRECT7 / DIRECT26, step_size > trans_epsilon / 2.
    """

    _NOT_IN_PCL = ("setNeighborhoodSearchMethod", "setNumThreads")

    def __getattribute__(self, name):
        if name in NormalDistributionsTransform._NOT_IN_PCL and object.__getattribute__(self, "__dict__").get("_ndt_class") == "pcl":
            raise AttributeError(f"pcl::NormalDistributionsTransform has no {name}")
        return object.__getattribute__(self, name)

    def __init__(self, variant: int = VARIANT_OMP, device: int = 0, pose_model: str = "se3", ndt_class: str = "omp", engine: "Engine | None" = None,
                 ground_class: "str | None" = None):
        if ground_class not in GROUND_CLASSES:
            raise ValueError("ground_class must be None, 'horizontal', 'vertical' or 'all'")
        if pose_model not in POSE_MODELS:
            raise ValueError(f"pose_model must be one of {sorted(POSE_MODELS)}")
        if ndt_class not in NDT_CLASSES:
            raise ValueError(f"ndt_class must be one of {sorted(NDT_CLASSES)}")
        self._ndt_class = ndt_class
        self._prm = default_params(variant=variant)           # ctor defaults, ndt_omp_impl2.hpp:53-83
        if engine is None:
            self._eng = Engine(self._prm, device)
        else:                                                 # an engine the caller shares with other surfaces (its keyframe store, its stream)
            self._eng = engine
            self._eng.set_params(self._prm)
        if POSE_MODELS[pose_model]:
            self._eng.set_option(OPT_POSE_MODEL, POSE_MODELS[pose_model])
        if NDT_CLASSES[ndt_class]:
            self._eng.set_option(OPT_NDT_CLASS, NDT_CLASSES[ndt_class])
        if GROUND_CLASSES[ground_class]:
            self._eng.set_option(OPT_GROUND_CLASS, GROUND_CLASSES[ground_class])
        self._final = np.eye(4, dtype=np.float32)
        self._converged = False
        self._nr_iterations = 0
        self._trans_probability = 0.0
        self._has_target = False
        self._has_source = False
        self._last = None

    def _push(self):
        self._eng.set_params(self._prm)

    # ---- setters / getters of ndt_omp.h
    def setNumThreads(self, n: int):            # ndt_omp.h:109 -- OpenMP thread count; meaningless on the GPU, accepted
        self._num_threads = int(n)

    def setResolution(self, resolution: float):  # ndt_omp.h:126-136: re-voxelises only if changed AND a source is set (`if (input_) init();`), as the engine does
        if np.float32(resolution) != np.float32(self._prm.resolution):
            self._prm.resolution = float(resolution)
            self._push()

    def getResolution(self) -> float:
        return float(self._prm.resolution)

    def setStepSize(self, step_size: float):
        self._prm.step_size = float(step_size)
        self._push()

    def getStepSize(self) -> float:
        return self._prm.step_size

    def setOulierRatio(self, outlier_ratio: float):   # [sic] ndt_omp.h:181
        self._prm.outlier_ratio = float(outlier_ratio)
        self._push()

    def getOulierRatio(self) -> float:
        return self._prm.outlier_ratio

    def setNeighborhoodSearchMethod(self, method: int):
        self._prm.neighbor_mode = int(method)
        self._push()

    def setTransformationEpsilon(self, eps: float):    # pcl::Registration
        self._prm.trans_epsilon = float(eps)
        self._push()

    def setMaximumIterations(self, n: int):            # pcl::Registration
        self._prm.max_iterations = int(n)
        self._push()

    def setLatencyMode(self, on: bool = True):         # not in the reference: mi355ndt_set_latency_mode (opt-in fine-grained sweep)
        self._eng.set_latency_mode(on)

    def getTransformationProbability(self) -> float:
        return self._trans_probability

    def getTargetCells(self) -> np.ndarray:
        """pclpca getTargetCells() (ndt_pca.h:129-133): the searchable leaves of the target grid, in std::map order."""
        return self._eng.get_voxels(0)

    def getFinalNumIteration(self) -> int:
        return self._nr_iterations

    # ---- pcl::Registration surface
    def setInputTarget(self, cloud):             # ndt_omp.h:116-121 -> init()
        self._eng.set_target(cloud)
        self._has_target = True

    def setInputSource(self, cloud):
        self._eng.set_source(cloud)
        self._has_source = True

    def align(self, guess=None) -> np.ndarray:
        """align(output, guess): returns the output cloud (source moved by the final pose, [N,3] f32)."""
        if not (self._has_target and self._has_source):
            # pcl::Registration::initCompute() fails -> PCL prints an error and returns with converged_ unchanged
            self._converged = False
            return np.zeros((0, 3), np.float32)
        G = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32)
        r = self._eng.align(G)
        if r["status"] == WARN_TOLERANCE_ARITH:      # the tolerance arithmetic on a registration it is not meant for: once more in the default arithmetic
            self._eng.set_option(OPT_ARITH, 0)
            try:
                r = self._eng.align(G)
            finally:
                self._eng.set_option(OPT_ARITH, 1)
        self._last = r
        self._final = r["final"]
        self._converged = r["converged"]
        self._nr_iterations = r["iterations"]
        self._trans_probability = r["trans_probability"]
        return self._eng.get_aligned()

    def getFinalTransformation(self) -> np.ndarray:
        return self._final.copy()

    def calculateScore(self, cloud) -> float:
        """ndt_omp.h:232 / ndt_pca.h:244: negative log-likelihood of an already transformed cloud (lower is better)."""
        if not self._has_target:
            raise NDTError(-7, "calculateScore")
        return self._eng.calculate_score(cloud)

    @staticmethod
    def convertTransform(x) -> np.ndarray:
        """static convertTransform (ndt_omp.h:209-228): [x, y, z, roll, pitch, yaw] -> 4x4 f32 (Translation * Rx * Ry * Rz)."""
        v = np.ascontiguousarray(x, np.float64)
        if v.shape != (6,):
            raise ValueError("x must have six entries: x, y, z, roll, pitch, yaw")
        out = np.zeros(16, np.float32)
        rc = load_library().mi355ndt_convert_transform(v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        if rc != OK:
            raise NDTError(rc, "convert_transform")
        return out.reshape(4, 4).T.copy()

    def setArithmetic(self, mode: int):                # not in the reference: mi355ndt_set_option(MI355NDT_OPT_ARITH)
        self._eng.set_option(OPT_ARITH, int(mode))

    def setF32SumOrder(self, order: int):              # not in the reference: mi355ndt_set_option(MI355NDT_OPT_F32_SUM_ORDER)
        self._eng.set_option(OPT_F32_SUM_ORDER, int(order))

    def getLastIncrementalTransformation(self) -> np.ndarray:
        """pcl::Registration::getLastIncrementalTransformation(): transformation_ = f32 exp(delta_p) of the last step (impl2:163)."""
        return self._eng.get_incremental(0)[0] if self._last is not None else np.eye(4, dtype=np.float32)

    def hasConverged(self) -> bool:
        return bool(self._converged)

    def getFitnessScore(self, max_range: float = float("inf")) -> float:
        """pcl::Registration::getFitnessScore (loop_detector.hpp:256): mean squared NN distance within max_range."""
        if not (self._has_target and self._has_source):
            return 1.7976931348623157e308
        return self._eng.fitness_score(max_range)[0]

    @property
    def engine(self) -> Engine:
        return self._eng


class NormalDistributionsTransformGround(NormalDistributionsTransform):
    """pclomp_ground::NormalDistributionsTransformGround (include/ndt_omp/ndt_ground.h): the setters of NormalDistributionsTransform, which are
    the reference's (ndt_ground.h has ndt_omp.h's), over MI355NDT_OPT_GROUND_CLASS.  flag_class is the reference's number and 1 by default, the
    value its computeTransformation hard-codes: 1 horizontal leaves, 2 vertical leaves, 0 every point."""

    def __init__(self, flag_class: int = 1, device: int = 0, engine: "Engine | None" = None):
        if flag_class not in GROUND_FLAG_CLASS:
            raise ValueError("flag_class must be 0, 1 or 2")
        super().__init__(VARIANT_OMP, device, engine=engine, ground_class={v: k for k, v in GROUND_CLASSES.items()}[GROUND_FLAG_CLASS[flag_class]])
        self._flag_class = flag_class

    def getFlagClass(self) -> int:
        return self._flag_class

