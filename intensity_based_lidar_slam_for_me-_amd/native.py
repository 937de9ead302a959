"""ctypes binding of ``liblislam.so`` (the C ABI declared in ``include/lislam.h`` and ``include/lislam_feeds.h``).

The HIP library is the only compute path: if it is missing this module raises, it never falls
back to a CPU implementation.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liblislam.so")

OK = 0
ERR_ARG, ERR_DEVICE, ERR_CAPACITY, ERR_STATE = -1, -2, -3, -4

OUT_IMAGE_RANGE, OUT_IMAGE_INTENSITY, OUT_CLOUD_TRACK, OUT_LASER_CLOUD = 0, 1, 2, 3
OUT_CURVATURE, OUT_LABEL, OUT_LINE_OFFSETS = 4, 5, 6
OUT_SHARP, OUT_LESS_SHARP, OUT_FLAT, OUT_LESS_FLAT = 7, 8, 9, 10
OUT_PARA, OUT_POSE, OUT_STATS = 11, 12, 13
OUT_ORB_T, OUT_ORB_STATS, OUT_ORB_KEYPOINTS, OUT_ORB_POINTS, OUT_ORB_DESCRIPTORS = 14, 15, 16, 17, 18
OUT_GROUND, OUT_GROUND_PLANE, OUT_GROUND_INFO = 19, 20, 21
OUT_CORNER_LAST, OUT_SURF_LAST, OUT_FULL_RES_END = 22, 23, 24  # after odometry in DISTORTION_TO_END only
DISTORTION_OFF, DISTORTION_QUERIES, DISTORTION_TO_END = 0, 1, 2  # lislam_set_distortion

KERNELS = ("k_scan_front", "k_scan_lines", "k_scan_compact", "k_target_index", "k_odom_assoc", "k_odom_lm",
           "k_odom_chain", "k_odom_to_end", "k_target_index_round")

EXPORTED_SYMBOLS = (
    "lislam_ctx_create", "lislam_ctx_destroy", "lislam_last_error", "lislam_synchronize",
    "lislam_set_stream", "lislam_get_stream", "lislam_scan_registration", "lislam_odom_create",
    "lislam_odom_destroy", "lislam_odom_step", "lislam_odom_status", "lislam_batch_create", "lislam_batch_destroy",
    "lislam_batch_upload", "lislam_batch_upload_async", "lislam_batch_download_cloud", "lislam_batch_input_device_ptr", "lislam_batch_extract",
    "lislam_batch_odometry", "lislam_batch_set_timing", "lislam_batch_kernel_times",
    "lislam_batch_download", "lislam_eval_factors", "lislam_eval_factors_raw", "lislam_set_tie_order", "lislam_set_odometry_schedule", "lislam_set_engine_shape", "lislam_batch_odometry_status",
    "lislam_batch_odometry_engine", "lislam_batch_odometry_abort_code", "lislam_device_queue_count",
    "lislam_set_engine_pairing", "lislam_set_engine_segment", "lislam_batch_odometry_paired", "lislam_set_distortion",
    "lislam_map_create", "lislam_map_destroy", "lislam_map_build", "lislam_map_add_points", "lislam_map_size",
    "lislam_map_points", "lislam_map_nearest_search", "lislam_map_associate", "lislam_normal_equations",
    "lislam_pose_solve", "lislam_voxel_grid", "lislam_mapopt_step", "lislam_mapopt_step_corner", "lislam_laser_mapping",
    "lislam_map_set_timing", "lislam_map_kernel_times",
    "lislam_orb_detect", "lislam_orb_match", "lislam_intensity_tracker_create", "lislam_intensity_tracker_destroy",
    "lislam_intensity_tracker_step", "lislam_batch_intensity_odometry", "lislam_batch_orb_cascade_info", "lislam_batch_ground", "lislam_ground_extract",
    "lislam_lmap_create", "lislam_lmap_destroy", "lislam_lmap_step", "lislam_lmap_counts", "lislam_lmap_points",
    "lislam_batch_odometry_gated", "lislam_odom_step_gated", "lislam_batch_mapopt", "lislam_batch_mapopt_corner", "lislam_loop_icp", "lislam_odom_fuser_create", "lislam_odom_fuser_destroy", "lislam_odom_fuse",
    "lislam_keyframes_create", "lislam_keyframes_destroy", "lislam_keyframes_size", "lislam_keyframes_add_clouds",
    "lislam_keyframes_add_batch", "lislam_keyframes_download", "lislam_loop_verify",
    "lislam_place_create", "lislam_place_destroy", "lislam_place_size", "lislam_place_add_clouds", "lislam_place_add_batch",
    "lislam_place_detect", "lislam_place_distance", "lislam_place_download",
    "lislam_bow_create", "lislam_bow_destroy", "lislam_bow_size", "lislam_bow_add", "lislam_bow_add_batch",
    "lislam_bow_detect", "lislam_bow_score", "lislam_bow_transform", "lislam_bow_download",
    "lislam_bow_trainer_create", "lislam_bow_trainer_destroy", "lislam_bow_trainer_size", "lislam_bow_trainer_add",
    "lislam_bow_trainer_add_batch", "lislam_bow_train", "lislam_bow_trainer_vocabulary",
    "lislam_pgo_create", "lislam_pgo_destroy", "lislam_pgo_size", "lislam_pgo_add_nodes", "lislam_pgo_set_prior",
    "lislam_pgo_add_edges", "lislam_pgo_add_batch", "lislam_pgo_edges", "lislam_pgo_linearize", "lislam_pgo_optimize",
    "lislam_pgo_poses",
    "lislam_mapwin_create", "lislam_mapwin_destroy", "lislam_mapwin_size", "lislam_mapwin_push", "lislam_mapwin_keyframe",
    "lislam_mapwin_match", "lislam_mapwin_records", "lislam_mapopt_step_window", "lislam_orb_detect_map",
    "lislam_batch_mapopt_window",
    "lislam_keysel_create", "lislam_keysel_destroy", "lislam_keysel_step", "lislam_keysel_step_batch", "lislam_keysel_state",
)
# include/lislam_feeds.h: the feeds for a list of scans
FEED_SYMBOLS = ("lislam_keyframes_add_batch_scans", "lislam_place_add_batch_scans", "lislam_bow_add_batch_scans",
                "lislam_pgo_add_keyframes", "lislam_pgo_add_batch_scans")

MAP_KERNELS = ("k_knn", "k_fit", "k_lm_eval", "k_lm_step", "map_rebuild", "map_downsample", "k_orb_pyramid",
               "k_orb_fast", "k_orb_select", "k_orb_finish", "k_orb_blur", "k_orb_desc", "k_orb_match", "k_orb_lm",
               "k_ground_screen", "k_ground_ransac", "k_ground_extract", "k_lc_step", "k_lc_apply", "k_fuse",
               "k_orb_roiblur", "k_lm_solve", "k_mw_match", "k_mw_select", "k_mw_gate")

MATCH_LINE, MATCH_PLANE = 0, 1
PLACE_DESC, PLACE_RING_KEY, PLACE_SECTOR_KEY = 0, 1, 2
PLACE_KERNELS = ("k_sc_describe", "k_sc_finish", "k_sc_detect", "k_sc_distance")
BOW_WORDS, BOW_VALUES = 0, 1
BOW_KERNELS = ("k_bow_words", "k_bow_vector", "k_bow_query", "k_bow_select", "k_bow_score", "k_bow_gather", "k_bow_scan_list")
BOW_TRAIN_MAX_L, BOW_TRAIN_MAX_DESCRIPTORS = 10, 1 << 23
BOW_PHASES = ("seed", "assign", "means", "partition")
BOW_TRAIN_KERNELS = ("k_bowt_ingest", "k_bowt_locate", "k_bowt_seed", "k_bowt_assign", "k_bowt_means", "k_bowt_majority",
                     "k_bowt_tilecount", "k_bowt_offsets", "k_bowt_scatter", "k_bowt_ni")
PGO_CONVERGED, PGO_LAMBDA_LIMIT, PGO_MAX_ITERATIONS = 0, 1, 2
PGO_KERNELS = ("k_pgo_linearize", "k_pgo_assemble", "k_pgo_sum", "k_pgo_factor", "k_pgo_cg", "k_pgo_retract",
               "k_pgo_add_batch", "k_pgo_pose6d", "k_pgo_add_keyframes")
KEYSEL_KERNELS = ("k_keysel", "k_kf_gather")  # the selector and the keyframe pool's list feed


class Config(ctypes.Structure):
    _fields_ = [("n_scans", ctypes.c_int32), ("width", ctypes.c_int32), ("min_range", ctypes.c_float),
                ("max_iterations", ctypes.c_int32), ("want_images", ctypes.c_int32)]


class PointLayout(ctypes.Structure):
    _fields_ = [("point_step", ctypes.c_uint32), ("off_x", ctypes.c_uint32), ("off_y", ctypes.c_uint32),
                ("off_z", ctypes.c_uint32), ("off_intensity", ctypes.c_uint32)]


_fp = ctypes.POINTER(ctypes.c_float)
_i32 = ctypes.c_int32
_i32p = ctypes.POINTER(ctypes.c_int32)


class ScanOut(ctypes.Structure):
    _fields_ = [("laser_cloud", _fp), ("cap_laser_cloud", _i32), ("n_laser_cloud", _i32),
                ("sharp", _fp), ("cap_sharp", _i32), ("n_sharp", _i32),
                ("less_sharp", _fp), ("cap_less_sharp", _i32), ("n_less_sharp", _i32),
                ("flat", _fp), ("cap_flat", _i32), ("n_flat", _i32),
                ("less_flat", _fp), ("cap_less_flat", _i32), ("n_less_flat", _i32),
                ("image_range", ctypes.POINTER(ctypes.c_uint8)), ("image_intensity", ctypes.POINTER(ctypes.c_uint8)),
                ("cloud_track", _fp)]


class MapConfig(ctypes.Structure):
    _fields_ = [("downsample_size", ctypes.c_float), ("cell_size", ctypes.c_float)]


class IcpConfig(ctypes.Structure):
    """lislam_icp_config: loop_closure_parameters (config/spot.yaml:26-33) + the ICP settings of
    intensity_feature_tracker.cpp:219-232; defaults = spot.yaml."""

    _fields_ = [("use_crop", _i32), ("crop_size", ctypes.c_float), ("use_downsample", _i32),
                ("voxel_size", ctypes.c_float), ("max_correspondence_distance", ctypes.c_float),
                ("max_iterations", _i32), ("transformation_epsilon", ctypes.c_double),
                ("euclidean_fitness_epsilon", ctypes.c_double), ("fitness_threshold", ctypes.c_double)]

    def __init__(self, use_crop=False, crop_size=200.0, use_downsample=True, voxel_size=0.25,
                 max_correspondence_distance=100.0, max_iterations=100, transformation_epsilon=1e-6,
                 euclidean_fitness_epsilon=1e-6, fitness_threshold=0.5):
        super().__init__(int(use_crop), crop_size, int(use_downsample), voxel_size, max_correspondence_distance,
                         max_iterations, transformation_epsilon, euclidean_fitness_epsilon, fitness_threshold)


class PlaceConfig(ctypes.Structure):
    """lislam_place_config: SCManager's parameters; defaults = Scancontext.h:77-96."""

    _fields_ = [("lidar_height", ctypes.c_double), ("max_radius", ctypes.c_double), ("search_ratio", ctypes.c_double),
                ("dist_thres", ctypes.c_double), ("num_ring", _i32), ("num_sector", _i32), ("num_exclude_recent", _i32),
                ("num_candidates", _i32), ("tree_making_period", _i32)]

    def __init__(self, lidar_height=2.0, max_radius=80.0, search_ratio=0.1, dist_thres=0.13, num_ring=20, num_sector=60,
                 num_exclude_recent=50, num_candidates=10, tree_making_period=50):
        super().__init__(lidar_height, max_radius, search_ratio, dist_thres, num_ring, num_sector, num_exclude_recent,
                         num_candidates, tree_making_period)


class BowTrainConfig(ctypes.Structure):
    """lislam_bow_train_config; defaults = DBoW3's constructor (k 10, L 5)."""

    _fields_ = [("k", _i32), ("L", _i32), ("max_iterations", _i32), ("seed", ctypes.c_uint64)]

    def __init__(self, k=10, L=5, max_iterations=100, seed=0):
        super().__init__(k, L, max_iterations, seed)


class BowTrainStats(ctypes.Structure):
    """lislam_bow_train_stats."""

    _fields_ = [("profile", _i32), ("n_nodes", _i32), ("n_words", _i32), ("n_zero_words", _i32), ("n_levels", _i32),
                ("level_steps", _i32 * 10), ("level_clustered", _i32 * 10), ("level_iterations", _i32 * 10),
                ("level_capped", _i32 * 10), ("level_ms", ctypes.c_double * 10), ("phase_ms", (ctypes.c_double * 4) * 10),
                ("weights_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class BowConfig(ctypes.Structure):
    """lislam_bow_config: detectLoop's thresholds; defaults = the constants it compiles with
    (loop_closure_handler.cpp:127-188)."""

    _fields_ = [("min_loop_bow_threshold", ctypes.c_double), ("index_score_threshold", ctypes.c_double),
                ("min_loop_search_gap", _i32), ("max_results", _i32), ("min_frame_index", _i32), ("loop_index_bound", _i32)]

    def __init__(self, min_loop_bow_threshold=0.0155, index_score_threshold=0.015, min_loop_search_gap=50, max_results=4,
                 min_frame_index=5, loop_index_bound=6):
        super().__init__(min_loop_bow_threshold, index_score_threshold, min_loop_search_gap, max_results, min_frame_index,
                         loop_index_bound)


class PgoConfig(ctypes.Structure):
    """lislam_pgo_config: the Levenberg-Marquardt loop and its CG solve (include/lislam.h)."""

    _fields_ = [("max_iterations", _i32), ("cg_max_iterations", _i32), ("lambda_init", ctypes.c_double),
                ("rel_cost_tol", ctypes.c_double), ("cg_rel_tol", ctypes.c_double)]

    def __init__(self, max_iterations=50, cg_max_iterations=0, lambda_init=1e-4, rel_cost_tol=1e-10, cg_rel_tol=1e-12):
        super().__init__(max_iterations, cg_max_iterations, lambda_init, rel_cost_tol, cg_rel_tol)


class KeyselConfig(ctypes.Structure):
    """lislam_keysel_config: getKeyframe's two gates; defaults = config/spot.yaml:35-36."""

    _fields_ = [("time_interval", ctypes.c_double), ("distance_interval", ctypes.c_double)]

    def __init__(self, time_interval=0.3, distance_interval=0.3):
        super().__init__(time_interval, distance_interval)


class Frame(ctypes.Structure):
    _fields_ = [("sharp", _fp), ("n_sharp", _i32), ("less_sharp", _fp), ("n_less_sharp", _i32),
                ("flat", _fp), ("n_flat", _i32), ("less_flat", _fp), ("n_less_flat", _i32)]


_LIB = None


def _preload_torch_runtime():
    """Load torch's HIP runtime first (when torch is importable) so that liblislam binds to the
    same libamdhip64 instance as torch in processes that use both."""
    if os.environ.get("LISLAM_NO_TORCH"):
        return
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional plumbing
        pass


def load(path: str = LIB_PATH):
    """Load the HIP library; raises if it is missing (no CPU fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise RuntimeError(f"liblislam.so not built ({path}); run __graft_entry__.build()")
    _preload_torch_runtime()
    L = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    L.lislam_ctx_create.argtypes = [ctypes.POINTER(Config), _i32, ctypes.POINTER(vp)]
    L.lislam_ctx_destroy.argtypes = [vp]
    L.lislam_last_error.argtypes = [vp]
    L.lislam_last_error.restype = ctypes.c_char_p
    L.lislam_synchronize.argtypes = [vp]
    L.lislam_set_stream.argtypes = [vp, vp]
    L.lislam_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.lislam_scan_registration.argtypes = [vp, vp, ctypes.POINTER(PointLayout), ctypes.POINTER(ScanOut)]
    L.lislam_odom_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.lislam_odom_destroy.argtypes = [vp]
    L.lislam_odom_step.argtypes = [vp, ctypes.POINTER(Frame), vp, vp, vp]
    L.lislam_odom_status.argtypes = [vp, ctypes.POINTER(_i32)]
    L.lislam_batch_create.argtypes = [vp, _i32, ctypes.POINTER(vp)]
    L.lislam_batch_destroy.argtypes = [vp]
    L.lislam_batch_upload.argtypes = [vp, vp, _i32, ctypes.POINTER(PointLayout)]
    L.lislam_batch_upload_async.argtypes = [vp, vp, _i32, ctypes.POINTER(PointLayout)]
    L.lislam_batch_input_device_ptr.argtypes = [vp, ctypes.POINTER(vp)]
    L.lislam_batch_extract.argtypes = [vp, _i32]
    L.lislam_batch_odometry.argtypes = [vp, _i32, _i32]
    L.lislam_batch_set_timing.argtypes = [vp, _i32]
    L.lislam_batch_kernel_times.argtypes = [vp, _fp, _i32p, _i32p]
    L.lislam_batch_download.argtypes = [vp, _i32, _i32, vp, _i32, _i32p]
    L.lislam_batch_download_cloud.argtypes = [vp, _i32, _i32, vp, ctypes.POINTER(PointLayout), _i32, _i32p]
    L.lislam_eval_factors.argtypes = [vp, _i32, vp, vp, vp, vp, vp, vp]
    L.lislam_eval_factors_raw.argtypes = [vp, _i32, vp, vp, vp, vp, vp, vp, vp]
    L.lislam_set_tie_order.argtypes = [vp, _i32]
    L.lislam_set_odometry_schedule.argtypes = [vp, _i32]
    L.lislam_set_engine_shape.argtypes = [vp, _i32, _i32]
    L.lislam_batch_odometry_status.argtypes = [vp, ctypes.POINTER(_i32)]
    L.lislam_batch_odometry_engine.argtypes = [vp, ctypes.POINTER(_i32)]
    L.lislam_set_engine_pairing.argtypes = [vp, _i32]
    L.lislam_set_engine_segment.argtypes = [vp, _i32]
    L.lislam_set_distortion.argtypes = [vp, _i32]
    L.lislam_batch_odometry_paired.argtypes = [vp, ctypes.POINTER(_i32)]
    L.lislam_batch_odometry_abort_code.argtypes = [vp, ctypes.POINTER(_i32)]
    L.lislam_device_queue_count.argtypes = [_i32, ctypes.POINTER(_i32)]
    i64, i64p = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.lislam_map_create.argtypes = [vp, ctypes.POINTER(MapConfig), ctypes.POINTER(vp)]
    L.lislam_map_destroy.argtypes = [vp]
    L.lislam_map_build.argtypes = [vp, vp, i64, _i32]
    L.lislam_map_add_points.argtypes = [vp, vp, i64, _i32, _i32, i64p]
    L.lislam_map_size.argtypes = [vp, i64p]
    L.lislam_map_points.argtypes = [vp, vp, i64, i64p]
    L.lislam_map_nearest_search.argtypes = [vp, vp, _i32, _i32, _i32, ctypes.c_float, vp, vp, vp]
    L.lislam_map_associate.argtypes = [vp, _i32, vp, _i32, _i32, vp, vp, vp]
    L.lislam_normal_equations.argtypes = [vp, vp, vp, _i32, vp, vp]
    L.lislam_pose_solve.argtypes = [vp, vp, vp, _i32, vp, _i32, vp]
    L.lislam_voxel_grid.argtypes = [vp, vp, _i32, ctypes.c_float, vp, _i32p]
    L.lislam_mapopt_step.argtypes = [vp, vp, _i32, vp, vp, vp, vp]
    L.lislam_mapopt_step_corner.argtypes = [vp, vp, vp, _i32, vp, _i32, vp, vp, vp, vp]
    L.lislam_laser_mapping.argtypes = [vp, vp, vp, _i32, vp, _i32, vp, vp]
    L.lislam_orb_detect.argtypes = [vp, vp, vp, vp, _i32, _i32, _i32, vp, vp, vp, _i32, _i32p]
    L.lislam_orb_match.argtypes = [vp, vp, _i32, vp, _i32, vp, _i32p]
    L.lislam_intensity_tracker_create.argtypes = [vp, _i32, _i32, _i32, vp, ctypes.POINTER(vp)]
    L.lislam_intensity_tracker_destroy.argtypes = [vp]
    L.lislam_intensity_tracker_step.argtypes = [vp, vp, vp, vp, vp]
    L.lislam_batch_intensity_odometry.argtypes = [vp, _i32, _i32, vp]
    L.lislam_batch_orb_cascade_info.argtypes = [vp, _i32p]
    L.lislam_batch_ground.argtypes = [vp, _i32]
    L.lislam_lmap_create.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.POINTER(vp)]
    L.lislam_lmap_destroy.argtypes = [vp]
    L.lislam_lmap_step.argtypes = [vp, vp, _i32, vp, _i32, vp, vp, vp, vp]
    L.lislam_lmap_counts.argtypes = [vp, vp, vp]
    L.lislam_lmap_points.argtypes = [vp, _i32, vp, i64, i64p]
    L.lislam_ground_extract.argtypes = [vp, vp, ctypes.POINTER(PointLayout), vp, _i32, _i32p, vp, vp]
    L.lislam_batch_odometry_gated.argtypes = [vp, _i32, _i32, vp]
    L.lislam_odom_step_gated.argtypes = [vp, vp, _i32, vp, vp, vp]
    L.lislam_batch_mapopt.argtypes = [vp, vp, _i32, vp, vp, vp, vp]
    L.lislam_batch_mapopt_corner.argtypes = [vp, vp, vp, _i32, vp, vp, vp, vp]
    L.lislam_loop_icp.argtypes = [vp, ctypes.POINTER(IcpConfig), vp, _i32, vp, vp, vp, _i32, vp, vp, vp, vp, vp]
    L.lislam_keyframes_create.argtypes = [vp, _i32, ctypes.c_int64, ctypes.POINTER(vp)]
    L.lislam_keyframes_destroy.argtypes = [vp]
    L.lislam_keyframes_size.argtypes = [vp, _i32p, ctypes.POINTER(ctypes.c_int64)]
    L.lislam_keyframes_add_clouds.argtypes = [vp, vp, vp, _i32]
    L.lislam_keyframes_add_batch.argtypes = [vp, vp, _i32, _i32]
    L.lislam_keyframes_download.argtypes = [vp, _i32, vp, _i32, _i32p]
    L.lislam_loop_verify.argtypes = [vp, ctypes.POINTER(IcpConfig), _i32, vp, vp, _i32, vp, vp, vp, vp, vp]
    L.lislam_odom_fuser_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.lislam_odom_fuser_destroy.argtypes = [vp]
    L.lislam_odom_fuse.argtypes = [vp, vp, vp, vp, _i32, vp]
    L.lislam_place_create.argtypes = [vp, ctypes.POINTER(PlaceConfig), _i32, ctypes.POINTER(vp)]
    L.lislam_place_destroy.argtypes = [vp]
    L.lislam_place_size.argtypes = [vp, _i32p]
    L.lislam_place_add_clouds.argtypes = [vp, vp, vp, _i32]
    L.lislam_place_add_batch.argtypes = [vp, vp, _i32, _i32]
    L.lislam_place_detect.argtypes = [vp, _i32, _i32, vp, vp, vp, vp, vp]
    L.lislam_place_distance.argtypes = [vp, vp, vp, _i32, vp, vp]
    L.lislam_place_download.argtypes = [vp, _i32, _i32, vp, _i32, _i32p]
    L.lislam_bow_create.argtypes = [vp, _i32, vp, vp, vp, ctypes.POINTER(BowConfig), _i32, _i32, ctypes.POINTER(vp)]
    L.lislam_bow_destroy.argtypes = [vp]
    L.lislam_bow_size.argtypes = [vp, _i32p]
    L.lislam_bow_add.argtypes = [vp, vp, vp, _i32]
    L.lislam_bow_add_batch.argtypes = [vp, vp, _i32, _i32]
    L.lislam_bow_detect.argtypes = [vp, _i32, _i32, vp, vp, vp, vp]
    L.lislam_bow_score.argtypes = [vp, vp, vp, _i32, vp]
    L.lislam_bow_transform.argtypes = [vp, vp, _i32, vp, vp]
    L.lislam_bow_download.argtypes = [vp, _i32, _i32, vp, _i32, _i32p]
    L.lislam_bow_trainer_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.lislam_bow_trainer_destroy.argtypes = [vp]
    L.lislam_bow_trainer_size.argtypes = [vp, _i32p, _i32p]
    L.lislam_bow_trainer_add.argtypes = [vp, vp, vp, _i32]
    L.lislam_bow_trainer_add_batch.argtypes = [vp, vp, _i32, _i32]
    L.lislam_bow_train.argtypes = [vp, ctypes.POINTER(BowTrainConfig), _i32p, ctypes.POINTER(BowTrainStats)]
    L.lislam_bow_trainer_vocabulary.argtypes = [vp, _i32, vp, vp, vp]
    L.lislam_pgo_create.argtypes = [vp, ctypes.POINTER(PgoConfig), _i32, _i32, ctypes.POINTER(vp)]
    L.lislam_pgo_destroy.argtypes = [vp]
    L.lislam_pgo_size.argtypes = [vp, _i32p, _i32p]
    L.lislam_pgo_add_nodes.argtypes = [vp, vp, _i32]
    L.lislam_pgo_set_prior.argtypes = [vp, _i32, vp, vp]
    L.lislam_pgo_add_edges.argtypes = [vp, vp, vp, vp, vp, vp, _i32]
    L.lislam_pgo_add_batch.argtypes = [vp, vp, _i32, _i32, vp]
    L.lislam_pgo_edges.argtypes = [vp, _i32, _i32, vp, vp, vp, vp, vp]
    L.lislam_pgo_linearize.argtypes = [vp, vp, vp, vp, vp, vp]
    L.lislam_pgo_optimize.argtypes = [vp, vp, vp]
    L.lislam_pgo_poses.argtypes = [vp, _i32, _i32, vp, vp]
    L.lislam_mapwin_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.lislam_mapwin_destroy.argtypes = [vp]
    L.lislam_mapwin_size.argtypes = [vp, _i32p]
    L.lislam_mapwin_push.argtypes = [vp, vp, vp, _i32, vp]
    L.lislam_mapwin_keyframe.argtypes = [vp, _i32, vp, vp, _i32, _i32p, vp]
    L.lislam_mapwin_match.argtypes = [vp, vp, _i32, vp]
    L.lislam_mapwin_records.argtypes = [vp, vp, vp, _i32, vp, vp, _i32, _i32p, vp, vp]
    L.lislam_mapopt_step_window.argtypes = [vp, vp, vp, vp, _i32, vp, _i32, vp, vp, _i32, vp, vp, vp, vp]
    L.lislam_orb_detect_map.argtypes = [vp, vp, vp, vp, _i32, _i32, _i32, vp, vp, vp, _i32, _i32p]
    L.lislam_batch_mapopt_window.argtypes = [vp, vp, vp, vp, _i32, _i32, vp, vp, vp, vp, vp]
    L.lislam_keysel_create.argtypes = [vp, ctypes.POINTER(KeyselConfig), ctypes.POINTER(vp)]
    L.lislam_keysel_destroy.argtypes = [vp]
    L.lislam_keysel_step.argtypes = [vp, vp, vp, vp, _i32, vp, _i32p, vp, vp]
    L.lislam_keysel_step_batch.argtypes = [vp, vp, _i32, _i32, vp, vp, _i32p, vp, vp]
    L.lislam_keysel_state.argtypes = [vp, _i32p, vp, vp]
    L.lislam_keyframes_add_batch_scans.argtypes = [vp, vp, vp, _i32]
    L.lislam_place_add_batch_scans.argtypes = [vp, vp, vp, _i32]
    L.lislam_bow_add_batch_scans.argtypes = [vp, vp, vp, _i32]
    L.lislam_pgo_add_keyframes.argtypes = [vp, vp, _i32, vp, _i32, vp]
    L.lislam_pgo_add_batch_scans.argtypes = [vp, vp, vp, _i32, vp]
    L.lislam_map_set_timing.argtypes = [vp, _i32]
    L.lislam_map_kernel_times.argtypes = [vp, _fp, _i32p]
    for name in EXPORTED_SYMBOLS + FEED_SYMBOLS:
        getattr(L, name).restype = getattr(L, name).restype or ctypes.c_int
    L.lislam_last_error.restype = ctypes.c_char_p
    _LIB = L
    return L


class LislamError(RuntimeError):
    pass


def check(rc: int, ctx=None, what: str = ""):
    if rc != OK:
        msg = ""
        if ctx:
            raw = load().lislam_last_error(ctx)
            msg = raw.decode() if raw else ""
        raise LislamError(f"{what} failed with status {rc}: {msg}")


def ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)
