"""ctypes loader for libaria_orb_hip.so (the C-ABI declared in include/aria_orb_hip.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARIA_ORB_HIP_LIBRARY: tests and profiling tools point this binding at the variants build (libaria_orb_hip_variants.so,
# `make -C aria_slam_amd/csrc variants`), the only library that knows the ARIA_* kernel / tuning switches. The product
# library itself reads no environment variable.
_SO = os.environ.get("ARIA_ORB_HIP_LIBRARY") or os.path.join(_HERE, "libaria_orb_hip.so")
_SO_VARIANTS = os.path.join(_HERE, "libaria_orb_hip_variants.so")

# byte-for-byte aria::core::KeyPoint / aria::core::Match (reference include/core/Types.hpp:9-15, :97-101)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4")])
MATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])

ARIA_OK = 0
ARIA_E_OUTPUT_TOO_SMALL = -5
ARIA_E_NOT_PENDING = -8

# every symbol include/aria_orb_hip.h declares
EXPORTS = [
    "aria_status_string", "aria_abi_version", "aria_last_hip_error",
    "aria_orb_default_config", "aria_orb_create", "aria_orb_destroy", "aria_orb_set_max_features",
    "aria_orb_get_max_features", "aria_orb_kp_capacity", "aria_orb_rows_needed", "aria_orb_fetch_last", "aria_orb_extract", "aria_orb_extract_async",
    "aria_orb_sync", "aria_orb_extract_batch_device", "aria_orb_check", "aria_orb_stream", "aria_orb_slow_path_blocks",
    "aria_orb_set_profiling", "aria_orb_set_stage_event", "aria_orb_get_profile", "aria_matcher_set_profiling", "aria_matcher_get_profile",
    "aria_orb_level_info", "aria_orb_resize_table", "aria_orb_pyramid_bands", "aria_orb_debug_read_level", "aria_orb_algorithmic_bytes",
    "aria_matcher_default_config", "aria_matcher_create", "aria_matcher_destroy", "aria_matcher_match",
    "aria_matcher_knn2", "aria_matcher_match_batch_device", "aria_matcher_match_db_device",
    "aria_matcher_stream", "aria_matcher_sync", "aria_synth_frame_pair", "aria_synth_sequence",
    "aria_flag_keypoints_device", "aria_matcher_match_batch_filtered_device", "aria_matcher_match_multi", "aria_matcher_count_good_multi", "aria_kfdb_create", "aria_kfdb_destroy", "aria_kfdb_size",
    "aria_kfdb_add", "aria_kfdb_add_device", "aria_kfdb_info", "aria_kfdb_fetch", "aria_kfdb_scan",
    "aria_orb_last_device", "aria_matcher_match_device", "aria_matcher_retain_device", "aria_matcher_resident_rows",
    "aria_matcher_match_device_async", "aria_matcher_finish", "aria_kfdb_match", "aria_stream_create", "aria_stream_destroy",
    "aria_orb_fast_blur_kernel", "aria_flag_keypoints_shifted_device",
    # ABI 4: device memory, staging copies and events for hosts that do not link the HIP runtime (host/ BatchFrontEnd)
    "aria_device_count", "aria_device_alloc", "aria_device_free", "aria_host_alloc_pinned", "aria_host_free_pinned",
    "aria_copy_h2d_async", "aria_copy_d2h_async", "aria_copy_d2d_async", "aria_fill_async", "aria_stream_synchronize",
    "aria_event_create", "aria_event_destroy", "aria_event_record", "aria_stream_wait_event", "aria_event_synchronize",
    "aria_event_elapsed_ms", "aria_matcher_knn_kernel",
    # two-view relative pose (essential-matrix RANSAC + recoverPose), additive to ABI 4
    "aria_pose_default_config", "aria_pose_create", "aria_pose_destroy", "aria_pose_stream", "aria_pose_check",
    "aria_pose_estimate", "aria_pose_estimate_batch_device", "aria_pose_debug_hypotheses",
    # two-view triangulation and point map (Mapper::triangulate + filters), additive to ABI 4
    "aria_map_default_config", "aria_map_create", "aria_map_destroy", "aria_map_stream", "aria_map_check",
    "aria_map_triangulate", "aria_map_triangulate_batch_device", "aria_map_points_needed", "aria_map_size",
    "aria_map_capacity", "aria_map_clear", "aria_map_reserve", "aria_map_read", "aria_map_device_points",
    "aria_map_filter_outliers", "aria_map_filter_distance",
    # fundamental-matrix RANSAC (findFundamentalMat FM_RANSAC, loop verification), additive to ABI 4
    "aria_fund_default_config", "aria_fund_create", "aria_fund_destroy", "aria_fund_stream", "aria_fund_check",
    "aria_fund_estimate", "aria_fund_estimate_batch_device", "aria_fund_debug_hypotheses",
    # SE(3) pose-graph optimisation (PoseGraphOptimizer: LM over VertexSE3 / EdgeSE3), additive to ABI 4
    "aria_graph_default_config", "aria_graph_create", "aria_graph_destroy", "aria_graph_stream", "aria_graph_check",
    "aria_graph_optimize", "aria_graph_optimize_batch_device", "aria_graph_debug_linearize",
    # visual-inertial fusion (SensorFusion EKF + IMUPreintegrator), additive to ABI 4
    "aria_fuse_default_config", "aria_fuse_create", "aria_fuse_destroy", "aria_fuse_stream", "aria_fuse_check",
    "aria_fuse_filter_init", "aria_fuse_run_batch_device", "aria_fuse_run", "aria_fuse_visual_from_pose_device",
    "aria_fuse_preintegrate_batch_device", "aria_fuse_preintegrate",
    # trajectory evaluation (ground-truth sampling, ATE / RPE, Umeyama alignment), additive to ABI 4
    "aria_eval_default_config", "aria_eval_create", "aria_eval_destroy", "aria_eval_stream", "aria_eval_check",
    "aria_eval_sample_truth_device", "aria_eval_sample_truth", "aria_eval_batch_device", "aria_eval_batch",
    # object detector around the network (TRTInference preprocess / postprocess + NMSBoxes), additive to ABI 4
    "aria_det_default_config", "aria_det_create", "aria_det_destroy", "aria_det_stream", "aria_det_check",
    "aria_det_device_buffers", "aria_det_preprocess_batch_device", "aria_det_postprocess_batch_device", "aria_det_preprocess",
    "aria_det_postprocess", "aria_det_resize_table", "aria_det_algorithmic_bytes",
    # sparse stereo on rectified pairs (depth per keypoint, metric scale of a relative pose), additive to ABI 4
    "aria_stereo_default_config", "aria_stereo_create", "aria_stereo_destroy", "aria_stereo_stream", "aria_stereo_check",
    "aria_stereo_match_batch_device", "aria_stereo_match", "aria_stereo_scale_batch_device", "aria_stereo_scale_pose",
    # undistortion and stereo rectification (radtan maps, batch remap in HBM, keypoints), additive to ABI 4
    "aria_rect_default_config", "aria_rect_create", "aria_rect_destroy", "aria_rect_stream", "aria_rect_check",
    "aria_rect_stereo_geometry", "aria_rect_remap_batch_device", "aria_rect_remap", "aria_rect_points_batch_device",
    "aria_rect_points", "aria_rect_get_map", "aria_rect_algorithmic_bytes",
    # dense stereo on rectified pairs (census + SGM disparity and depth maps, keypoint sampling), additive to ABI 4
    "aria_dense_default_config", "aria_dense_create", "aria_dense_destroy", "aria_dense_stream", "aria_dense_check",
    "aria_dense_compute_batch_device", "aria_dense_compute", "aria_dense_sample_batch_device", "aria_dense_sample",
    "aria_dense_pairs_in_flight", "aria_dense_scratch_bytes_per_pair", "aria_dense_algorithmic_bytes",
    # dense depth fusion (TSDF volume from depth maps along the trajectory, surface points), additive to ABI 4
    "aria_tsdf_default_config", "aria_tsdf_create", "aria_tsdf_destroy", "aria_tsdf_stream", "aria_tsdf_check", "aria_tsdf_clear",
    "aria_tsdf_integrate_batch_device", "aria_tsdf_integrate", "aria_tsdf_extract_points_device", "aria_tsdf_extract_points",
    "aria_tsdf_device_voxels", "aria_tsdf_read_box", "aria_tsdf_volume_bytes", "aria_tsdf_algorithmic_bytes",
    # path planning (traversability grid from the TSDF volume, clearance and cost, goal fields, paths), additive to ABI 4
    "aria_nav_default_config", "aria_nav_create", "aria_nav_destroy", "aria_nav_stream", "aria_nav_check",
    "aria_nav_update_from_volume_device", "aria_nav_set_cells_device", "aria_nav_set_cells", "aria_nav_read_cells",
    "aria_nav_read_clearance", "aria_nav_read_costs", "aria_nav_solve_device", "aria_nav_trace_device", "aria_nav_plan",
    "aria_nav_device_fields", "aria_nav_read_field", "aria_nav_read_rounds", "aria_nav_field_bytes",
    # obstacle alerts (depth zones and detection boxes measured exactly, priorities, cooldowns, events), additive to ABI 4
    "aria_alert_default_config", "aria_alert_create", "aria_alert_destroy", "aria_alert_stream", "aria_alert_check",
    "aria_alert_dets_seen", "aria_alert_measure_batch_device", "aria_alert_arbitrate_batch_device", "aria_alert_run_batch_device",
    "aria_alert_measure", "aria_alert_arbitrate", "aria_alert_run", "aria_alert_zone_bounds", "aria_alert_algorithmic_bytes",
    # absolute pose from the point map (6-point DLT RANSAC + Gauss-Newton, map association), additive to ABI 4
    "aria_pnp_default_config", "aria_pnp_create", "aria_pnp_destroy", "aria_pnp_stream", "aria_pnp_check",
    "aria_pnp_estimate", "aria_pnp_estimate_batch_device", "aria_pnp_debug_hypotheses", "aria_pnp_associate_batch_device",
    "aria_pnp_set_solver", "aria_pnp_get_solver",
    # local bundle adjustment (batched windows, Schur-complement LM over poses and points), additive to ABI 4
    "aria_ba_default_config", "aria_ba_create", "aria_ba_destroy", "aria_ba_stream", "aria_ba_check",
    "aria_ba_optimize", "aria_ba_optimize_batch_device", "aria_ba_debug_linearize", "aria_ba_window_from_chain_device",
    # ray casting of the TSDF volume (depth, normal, gray and shaded views at a batch of poses), additive to ABI 4
    "aria_ray_default_config", "aria_ray_create", "aria_ray_destroy", "aria_ray_stream", "aria_ray_check",
    "aria_ray_update_from_volume_device", "aria_ray_cast_batch_device", "aria_ray_cast", "aria_ray_algorithmic_bytes",
    # frame-to-model tracking (batched point-to-plane ICP against the ray-cast model view), additive to ABI 4
    "aria_icp_default_config", "aria_icp_create", "aria_icp_destroy", "aria_icp_stream", "aria_icp_check",
    "aria_icp_track_batch_device", "aria_icp_track", "aria_icp_debug_system_device", "aria_icp_algorithmic_bytes",
    # mesh of the TSDF volume (watertight marching tetrahedra: vertices and triangles), additive to ABI 4
    "aria_mesh_default_config", "aria_mesh_create", "aria_mesh_destroy", "aria_mesh_stream", "aria_mesh_check",
    "aria_mesh_update_from_volume_device", "aria_mesh_extract_device", "aria_mesh_extract", "aria_mesh_scratch_bytes",
    "aria_mesh_algorithmic_bytes",
    # guided matching (landmarks projected by a predicted pose, window search, local-map PnP input), additive to ABI 4
    "aria_proj_default_config", "aria_proj_create", "aria_proj_destroy", "aria_proj_stream", "aria_proj_check",
    "aria_proj_search_batch_device", "aria_proj_search", "aria_proj_landmarks_from_map_device",
    # place recognition (flat binary bag-of-words vocabulary, ring database of bags, scored top-K), additive to ABI 4
    "aria_bow_default_config", "aria_bow_create", "aria_bow_destroy", "aria_bow_stream", "aria_bow_check", "aria_bow_words",
    "aria_bow_train_device", "aria_bow_train", "aria_bow_set_vocabulary", "aria_bow_get_vocabulary", "aria_bow_save", "aria_bow_load",
    "aria_bow_transform_batch_device", "aria_bow_add_batch_device", "aria_bow_add", "aria_bow_add_device", "aria_bow_size",
    "aria_bow_info", "aria_bow_query_batch_device", "aria_bow_query", "aria_bow_query_device",
    # loop alignment (batched Sim(3) RANSAC of the landmarks two keyframes own, join with the point map), additive to ABI 4
    "aria_sim3_default_config", "aria_sim3_create", "aria_sim3_destroy", "aria_sim3_stream", "aria_sim3_check",
    "aria_sim3_estimate", "aria_sim3_estimate_batch_device", "aria_sim3_debug_hypotheses", "aria_sim3_associate_batch_device",
    # Sim(3) pose-graph optimisation and map correction after a loop (7-DoF LM, the arena moved by anchor keyframe), additive to ABI 4
    "aria_sgraph_default_config", "aria_sgraph_create", "aria_sgraph_destroy", "aria_sgraph_stream", "aria_sgraph_check",
    "aria_sgraph_optimize", "aria_sgraph_optimize_batch_device", "aria_sgraph_debug_linearize",
    "aria_sgraph_vertices_from_pose_device", "aria_sgraph_poses_from_vertices_device", "aria_sgraph_correct_map_device",
    "aria_sgraph_correct_points_device",
]


class OrbConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("max_width", C.c_int),
                ("max_height", C.c_int), ("max_features", C.c_int), ("max_batch", C.c_int),
                ("blur_tie_mode", C.c_int), ("cand_cap_scale", C.c_int), ("level_size_mode", C.c_int)]


class MatcherConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("max_query", C.c_int),
                ("max_train", C.c_int)]


class PoseConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("hypotheses", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("threshold_px", C.c_double), ("distance_thresh", C.c_double), ("seed", C.c_uint64)]


# aria_pose_result (192 bytes)
POSE_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("E", "<f8", (9,)), ("n_matches", "<i4"),
                              ("n_inliers", "<i4"), ("n_pose_inliers", "<i4"), ("best_hypothesis", "<i4"),
                              ("refined", "<i4"), ("valid", "<i4")])


class PnpConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("hypotheses", C.c_int),
                ("refine_iters", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("threshold_px", C.c_double), ("seed", C.c_uint64)]


# aria_pnp_corr (32 bytes) and aria_pnp_result (128 bytes)
PNP_CORR_DTYPE = np.dtype([("X", "<f8", (3,)), ("u", "<f4"), ("v", "<f4")])
PNP_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("rms_px", "<f8"), ("n_corr", "<i4"), ("n_inliers", "<i4"),
                             ("best_hypothesis", "<i4"), ("iterations", "<i4"), ("refined", "<i4"), ("valid", "<i4")])


class Sim3Config(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("hypotheses", C.c_int),
                ("refine_iters", C.c_int), ("fix_scale", C.c_int), ("reserved", C.c_int), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("threshold_px", C.c_double), ("min_scale", C.c_double),
                ("max_scale", C.c_double), ("seed", C.c_uint64)]


# aria_sim3_corr (64 bytes) and aria_sim3_result (136 bytes)
SIM3_CORR_DTYPE = np.dtype([("X1", "<f8", (3,)), ("X2", "<f8", (3,)), ("u1", "<f4"), ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4")])
SIM3_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("s", "<f8"), ("rms_px", "<f8"), ("n_corr", "<i4"),
                              ("n_inliers", "<i4"), ("best_hypothesis", "<i4"), ("iterations", "<i4"), ("refined", "<i4"),
                              ("valid", "<i4")])


class BaConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("huber_px", C.c_double), ("min_depth", C.c_double),
                ("max_iterations", C.c_int), ("max_windows", C.c_int)]


# aria_ba_obs (16 bytes) and aria_ba_result (56 bytes)
BA_OBS_DTYPE = np.dtype([("point", "<i4"), ("pose", "<i4"), ("u", "<f4"), ("v", "<f4")])
BA_RESULT_DTYPE = np.dtype([("chi2_initial", "<f8"), ("chi2_final", "<f8"), ("lambda", "<f8"), ("rms_px", "<f8"),
                            ("n_obs_used", "<i4"), ("iterations_done", "<i4"), ("trials", "<i4"), ("stop_reason", "<i4"),
                            ("valid", "<i4"), ("reserved", "<i4")])


class FundConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("hypotheses", C.c_int),
                ("threshold_px", C.c_double), ("seed", C.c_uint64)]


class GraphConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("max_graphs", C.c_int),
                ("max_vertices", C.c_int), ("max_edges", C.c_int), ("pcg_max_iters", C.c_int), ("pcg_rel_tol", C.c_double)]


class GraphEdge(C.Structure):
    _fields_ = [("from_", C.c_int32), ("to", C.c_int32), ("info_scale", C.c_double), ("Z", C.c_double * 12)]


class GraphResult(C.Structure):
    _fields_ = [("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_", C.c_double),
                ("iterations_done", C.c_int), ("trials", C.c_int), ("pcg_iterations", C.c_int), ("valid", C.c_int),
                ("stop_reason", C.c_int), ("reserved", C.c_int)]


# aria_graph_edge (112 bytes) and aria_graph_result (48 bytes)
GRAPH_EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("info_scale", "<f8"), ("Z", "<f8", (12,))])
GRAPH_RESULT_DTYPE = np.dtype([("chi2_initial", "<f8"), ("chi2_final", "<f8"), ("lambda", "<f8"), ("iterations_done", "<i4"),
                               ("trials", "<i4"), ("pcg_iterations", "<i4"), ("valid", "<i4"), ("stop_reason", "<i4"),
                               ("reserved", "<i4")])


class SgraphConfig(C.Structure):
    _fields_ = GraphConfig._fields_ + [("fix_scale", C.c_int), ("reserved", C.c_int)]


# aria_sgraph_vertex (104 bytes), aria_sgraph_edge (120 bytes), aria_sgraph_result (48 bytes: aria_graph_result's layout) and
# aria_sgraph_correct_stats (16 bytes)
SGRAPH_VERTEX_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("s", "<f8")])
SGRAPH_EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("info_scale", "<f8"), ("Z", "<f8", (12,)), ("s", "<f8")])
SGRAPH_RESULT_DTYPE = np.dtype(GRAPH_RESULT_DTYPE.descr)
SGRAPH_STATS_DTYPE = np.dtype([("moved", "<i4"), ("left_alone", "<i4"), ("refused", "<i4"), ("reserved", "<i4")])


class FuseConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("gravity", C.c_double * 3),
                ("accel_noise", C.c_double), ("gyro_noise", C.c_double), ("accel_bias_walk", C.c_double),
                ("gyro_bias_walk", C.c_double), ("pos_noise", C.c_double), ("rot_noise", C.c_double)]


class ImuSample(C.Structure):
    _fields_ = [("t", C.c_double), ("accel", C.c_double * 3), ("gyro", C.c_double * 3)]


class FuseVisual(C.Structure):
    _fields_ = [("t", C.c_double), ("R", C.c_double * 9), ("p", C.c_double * 3), ("accept", C.c_int), ("reserved", C.c_int)]


class FuseFilter(C.Structure):
    _fields_ = [("p", C.c_double * 3), ("v", C.c_double * 3), ("q", C.c_double * 4), ("ba", C.c_double * 3),
                ("bg", C.c_double * 3), ("P", C.c_double * 225), ("last_imu_time", C.c_double),
                ("last_visual_time", C.c_double), ("gravity", C.c_double * 3), ("accel_noise", C.c_double),
                ("gyro_noise", C.c_double), ("accel_bias_walk", C.c_double), ("gyro_bias_walk", C.c_double),
                ("pos_noise", C.c_double), ("rot_noise", C.c_double), ("initialized", C.c_int), ("reserved", C.c_int)]


class FuseState(C.Structure):
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("v", C.c_double * 3), ("q", C.c_double * 4), ("ba", C.c_double * 3),
                ("bg", C.c_double * 3), ("P_diag", C.c_double * 15), ("n_predicted", C.c_int), ("n_skipped", C.c_int),
                ("n_ignored", C.c_int), ("n_updates", C.c_int), ("initialized", C.c_int), ("valid", C.c_int)]


class PreintResult(C.Structure):
    _fields_ = [("delta_p", C.c_double * 3), ("delta_v", C.c_double * 3), ("delta_q", C.c_double * 4), ("dt_sum", C.c_double),
                ("cov", C.c_double * 81), ("n_used", C.c_int), ("valid", C.c_int)]


# aria_imu_sample (56 bytes), aria_fuse_visual (112), aria_fuse_filter (2024), aria_fuse_state (280), aria_preint_result (744)
IMU_SAMPLE_DTYPE = np.dtype([("t", "<f8"), ("accel", "<f8", (3,)), ("gyro", "<f8", (3,))])
FUSE_VISUAL_DTYPE = np.dtype([("t", "<f8"), ("R", "<f8", (9,)), ("p", "<f8", (3,)), ("accept", "<i4"), ("reserved", "<i4")])
FUSE_FILTER_DTYPE = np.dtype([("p", "<f8", (3,)), ("v", "<f8", (3,)), ("q", "<f8", (4,)), ("ba", "<f8", (3,)), ("bg", "<f8", (3,)),
                              ("P", "<f8", (225,)), ("last_imu_time", "<f8"), ("last_visual_time", "<f8"),
                              ("gravity", "<f8", (3,)), ("accel_noise", "<f8"), ("gyro_noise", "<f8"),
                              ("accel_bias_walk", "<f8"), ("gyro_bias_walk", "<f8"), ("pos_noise", "<f8"), ("rot_noise", "<f8"),
                              ("initialized", "<i4"), ("reserved", "<i4")])
FUSE_STATE_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("v", "<f8", (3,)), ("q", "<f8", (4,)), ("ba", "<f8", (3,)),
                             ("bg", "<f8", (3,)), ("P_diag", "<f8", (15,)), ("n_predicted", "<i4"), ("n_skipped", "<i4"),
                             ("n_ignored", "<i4"), ("n_updates", "<i4"), ("initialized", "<i4"), ("valid", "<i4")])
PREINT_RESULT_DTYPE = np.dtype([("delta_p", "<f8", (3,)), ("delta_v", "<f8", (3,)), ("delta_q", "<f8", (4,)), ("dt_sum", "<f8"),
                                ("cov", "<f8", (81,)), ("n_used", "<i4"), ("valid", "<i4")])


class EvalConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("align_mode", C.c_int),
                ("rpe_delta", C.c_int)]


class EvalTruth(C.Structure):
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("q", C.c_double * 4), ("v", C.c_double * 3), ("bg", C.c_double * 3),
                ("ba", C.c_double * 3)]


class EvalResult(C.Structure):
    _fields_ = [("ate_raw", C.c_double), ("rpe_raw", C.c_double), ("scale", C.c_double), ("R", C.c_double * 9),
                ("t", C.c_double * 3), ("sigma", C.c_double * 3), ("ate_rmse", C.c_double), ("ate_mean", C.c_double),
                ("ate_max", C.c_double), ("rpe_aligned", C.c_double), ("n_poses", C.c_int), ("n_used", C.c_int),
                ("n_rpe_pairs", C.c_int), ("align_valid", C.c_int), ("valid", C.c_int), ("reserved", C.c_int)]


# aria_eval_truth (136 bytes) and aria_eval_result (200 bytes)
EVAL_TRUTH_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("q", "<f8", (4,)), ("v", "<f8", (3,)), ("bg", "<f8", (3,)),
                             ("ba", "<f8", (3,))])
EVAL_RESULT_DTYPE = np.dtype([("ate_raw", "<f8"), ("rpe_raw", "<f8"), ("scale", "<f8"), ("R", "<f8", (9,)), ("t", "<f8", (3,)),
                              ("sigma", "<f8", (3,)), ("ate_rmse", "<f8"), ("ate_mean", "<f8"), ("ate_max", "<f8"),
                              ("rpe_aligned", "<f8"), ("n_poses", "<i4"), ("n_used", "<i4"), ("n_rpe_pairs", "<i4"),
                              ("align_valid", "<i4"), ("valid", "<i4"), ("reserved", "<i4")])
EVAL_ALIGN_NONE, EVAL_ALIGN_SE3, EVAL_ALIGN_SIM3 = 0, 1, 2
EVAL_EST_POSE12, EVAL_EST_FUSE_STATE, EVAL_EST_XYZ = 0, 1, 2


class DetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("input_w", C.c_int), ("input_h", C.c_int),
                ("max_batch", C.c_int), ("max_candidates", C.c_int), ("out_half", C.c_int), ("reserved", C.c_int)]


# aria_detection == aria::core::Detection (24 bytes) and aria_box (16 bytes)
DETECTION_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"), ("class_id", "<i4")])
BOX_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
DET_MAX_CANDIDATES, DET_MAX_CLASS_IDS = 1024, 32


# aria_fund_result (96 bytes)
FUND_RESULT_DTYPE = np.dtype([("F", "<f8", (9,)), ("n_matches", "<i4"), ("n_inliers", "<i4"), ("n_models", "<i4"),
                              ("best_hypothesis", "<i4"), ("best_root", "<i4"), ("valid", "<i4")])


class MapConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double),
                ("min_parallax_deg", C.c_double), ("max_reproj_px", C.c_double), ("capacity", C.c_int64),
                ("min_pose_inliers", C.c_int), ("reserved", C.c_int)]


# aria_map_point (72 bytes)
MAP_POINT_DTYPE = np.dtype([("id", "<u8"), ("X", "<f8", (3,)), ("quality", "<f8"), ("err", "<f4", (2,)), ("pair", "<i4"),
                            ("match", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("gray", "u1"), ("pad", "u1", (7,))])


class StereoConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("baseline", C.c_double), ("min_disparity", C.c_double),
                ("max_disparity", C.c_double), ("band_factor", C.c_double), ("median_factor", C.c_double),
                ("th_hamming", C.c_int), ("sad_half_window", C.c_int), ("sad_slide", C.c_int), ("max_octave_diff", C.c_int),
                ("min_scale_matches", C.c_int), ("reserved", C.c_int)]


class ProjConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("min_depth", C.c_double), ("radius_px", C.c_double), ("ratio", C.c_float),
                ("th_hamming", C.c_int), ("max_octave_diff", C.c_int), ("reserved", C.c_int)]


# aria_proj_landmark (64 bytes), aria_proj_obs (24 bytes) and aria_proj_pair (8 bytes)
PROJ_LANDMARK_DTYPE = np.dtype([("X", "<f8", (3,)), ("desc", "u1", (32,)), ("octave", "<i4"), ("source", "<i4")])
PROJ_OBS_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("kp_idx", "<i4"), ("hamming", "<i4"), ("second", "<i4"), ("flags", "<i4")])
PROJ_PAIR_DTYPE = np.dtype([("landmark", "<i4"), ("keypoint", "<i4")])


class BowConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("words", C.c_int), ("rows", C.c_int),
                ("capacity", C.c_int), ("top_k", C.c_int), ("min_frames_between", C.c_int), ("train_iters", C.c_int)]


# aria_bow_hit (32 bytes)
BOW_HIT_DTYPE = np.dtype([("index", "<i4"), ("reserved", "<i4"), ("id", "<i8"), ("S", "<i8"), ("score", "<f8")])


# aria_stereo_obs (32 bytes) and aria_stereo_scale (16 bytes)
STEREO_OBS_DTYPE = np.dtype([("u_right", "<f4"), ("disparity", "<f4"), ("depth", "<f4"), ("X", "<f4"), ("Y", "<f4"),
                             ("right_idx", "<i4"), ("hamming", "<i4"), ("sad", "<i4")])
STEREO_SCALE_DTYPE = np.dtype([("scale", "<f8"), ("n_used", "<i4"), ("valid", "<i4")])


class RectCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 5),
                ("R", C.c_double * 9)]


class RectConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("src_width", C.c_int),
                ("src_height", C.c_int), ("dst_width", C.c_int), ("dst_height", C.c_int), ("n_cameras", C.c_int),
                ("cam", RectCamera * 2), ("new_fx", C.c_double), ("new_fy", C.c_double), ("new_cx", C.c_double),
                ("new_cy", C.c_double), ("fill", C.c_int), ("model", C.c_int)]


RECT_MODEL_RADTAN, RECT_MODEL_KB4 = 0, 1


class DenseConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("baseline", C.c_double), ("num_disparities", C.c_int), ("P1", C.c_int),
                ("P2", C.c_int), ("uniqueness", C.c_int), ("lr_max_diff", C.c_int), ("max_width", C.c_int),
                ("max_height", C.c_int), ("reserved", C.c_int), ("scratch_bytes", C.c_int64)]


class TsdfConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("max_weight", C.c_int), ("min_weight", C.c_int), ("reserved", C.c_int), ("voxel", C.c_float),
                ("trunc", C.c_float), ("origin", C.c_float * 3), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("reserved2", C.c_float), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


# aria_tsdf_voxel (8 bytes) and aria_tsdf_point (16 bytes)
TSDF_VOXEL_DTYPE = np.dtype([("tsdf", "<f4"), ("weight", "<u2"), ("gray", "u1"), ("reserved", "u1")])
TSDF_POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("gray", "u1"), ("axis", "u1"), ("weight", "<u2")])


class MeshConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("min_weight", C.c_int), ("voxel", C.c_float), ("origin", C.c_float * 3)]


# aria_mesh_vertex (16 bytes) and aria_mesh_triangle (12 bytes)
MESH_VERTEX_DTYPE = np.dtype([("X", "<f4", (3,)), ("gray", "u1"), ("dir", "u1"), ("weight", "<u2")])
MESH_TRIANGLE_DTYPE = np.dtype([("v", "<u4", (3,))])


class RayConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("min_weight", C.c_int), ("skip", C.c_int), ("voxel", C.c_float), ("origin", C.c_float * 3),
                ("near", C.c_float), ("far", C.c_float), ("step", C.c_float), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class IcpConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("min_depth", C.c_float), ("max_depth", C.c_float), ("dist_max", C.c_float),
                ("reach", C.c_float), ("min_corr", C.c_int), ("n_levels", C.c_int), ("min_pivot", C.c_double), ("eps", C.c_double),
                ("stride", C.c_int * 4), ("iterations", C.c_int * 4)]


# aria_icp_result (32 bytes)
ICP_RESULT_DTYPE = np.dtype([("valid", "<i4"), ("iterations_run", "<i4"), ("n_corr", "<i4"), ("level", "<i4"), ("rms", "<f8"),
                             ("delta", "<f8")])
ICP_TERMS = 29


# aria_ray_view (16 bytes) and the ARIA_RAY_* plane bits of aria_ray_algorithmic_bytes
RAY_VIEW_DTYPE = np.dtype([("n_hit", "<i4"), ("n_ended", "<i4"), ("nearest", "<f4"), ("valid", "<i4")])
RAY_DEPTH, RAY_NORMAL, RAY_GRAY, RAY_SHADE = 1, 2, 4, 8


class NavConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("up_axis", C.c_int), ("band0", C.c_int), ("band1", C.c_int), ("min_weight", C.c_int),
                ("occ_tsdf", C.c_float), ("occ_count", C.c_int), ("free_count", C.c_int), ("clear_radius", C.c_int),
                ("block_d2", C.c_int), ("soft_d2", C.c_int), ("penalty", C.c_int), ("unknown_penalty", C.c_int),
                ("allow_unknown", C.c_int), ("max_goals", C.c_int), ("voxel", C.c_float), ("origin", C.c_float * 3),
                ("reserved", C.c_int)]


# aria_nav_record (16 bytes); the states of a cell, the statuses of a query, the field value of an unreachable cell
NAV_RECORD_DTYPE = np.dtype([("cost", "<i4"), ("n_cells", "<i4"), ("min_d2", "<i4"), ("status", "<i4")])
NAV_FREE, NAV_OCCUPIED, NAV_UNKNOWN = 0, 1, 2
NAV_OK, NAV_UNREACHABLE, NAV_OUT_OF_GRID, NAV_TRUNCATED = 0, 1, 2, 3
NAV_INF = 0x7FFFFFFF


class AlertConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("stream", C.c_void_p), ("width", C.c_int), ("height", C.c_int),
                ("zone_top", C.c_int), ("zone_bottom", C.c_int), ("max_dets", C.c_int), ("min_valid", C.c_int),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("zone_pct_num", C.c_int), ("zone_pct_den", C.c_int),
                ("det_pct_num", C.c_int), ("det_pct_den", C.c_int), ("zone_alert_m", C.c_float), ("default_depth", C.c_float),
                ("crit_m", C.c_float), ("high_m", C.c_float), ("medium_m", C.c_float), ("beep_m", C.c_float),
                ("obstacle_dangerous", C.c_int), ("n_dangerous", C.c_int), ("dangerous", C.c_int * 32),
                ("max_events_per_frame", C.c_int), ("reserved", C.c_int), ("cooldown_ns", C.c_int64 * 4)]


# aria_alert_meas (16 bytes), aria_alert_event (32 bytes), aria_alert_state (2320 bytes) and the values they hold
ALERT_MEAS_DTYPE = np.dtype([("distance", "<f4"), ("n_valid", "<i4"), ("k", "<i4"), ("flags", "<i4")])
ALERT_EVENT_DTYPE = np.dtype([("frame", "<i4"), ("source", "<i4"), ("class_id", "<i4"), ("direction", "<i4"), ("priority", "<i4"),
                              ("distance", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
ALERT_STATE_DTYPE = np.dtype([("last_ns", "<i8", (256,)), ("last_prio1", "u1", (256,)), ("events_total", "<i8"), ("reserved", "<i8")])
ALERT_SOURCES, ALERT_MAX_DETS = 64, 61
ALERT_LOW, ALERT_MEDIUM, ALERT_HIGH, ALERT_CRITICAL = 0, 1, 2, 3
ALERT_CENTER, ALERT_LEFT, ALERT_RIGHT = 0, 1, 2
ALERT_BEEP, ALERT_CRITICAL_ALERT, ALERT_INTERRUPT, ALERT_NO_DEPTH = 1, 2, 4, 8
ALERT_MEAS_SOURCE, ALERT_MEAS_OK = 1, 2


# right_idx of a record sampled from a dense map (ARIA_DENSE_NO_KEYPOINT) and the disparity of an invalid pixel in 1/16 px
DENSE_NO_KEYPOINT = 0x7FFFFFFF
DENSE_INVALID = -16


# an entry of the rectification map: qx | qy << 16 in 1/32 px, RECT_INVALID = no source
RECT_MAP_DTYPE = np.dtype("<u4")
RECT_INVALID = 0xFFFFFFFF


class AriaError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        detail = ""
        try:
            detail = load_library().aria_last_hip_error().decode()
        except Exception:
            pass
        super().__init__("%s failed: %s (%d)%s" % (where, status_string(status), status,
                                                   (" [" + detail + "]") if detail else ""))


def library_path():
    return _SO


def build_library(force=False):
    """Compile the gfx950 shared library in-tree with hipcc (cross-compiles without a GPU)."""
    if force and os.path.exists(_SO):
        os.remove(_SO)
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s"])
    return _SO


def build_variants_library():
    """Compile libaria_orb_hip_variants.so (-DARIA_VARIANTS: superseded kernels + ARIA_* switches) and return its path."""
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s", "variants"])
    return _SO_VARIANTS


_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so; this library links the system one. If both copies end up in
    one process (library loaded first, torch imported later) the second runtime finds no device. So when a torch
    installation is present, map its copy first: the loader then satisfies our NEEDED libamdhip64.so.7 from it and a
    later `import torch` reuses it too. Without torch nothing happens and the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if not spec or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Load the HIP library. Never falls back to anything else: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback." % _SO)
    _preload_torch_hip_runtime()
    L = C.CDLL(_SO)
    L.aria_status_string.restype = C.c_char_p
    L.aria_last_hip_error.restype = C.c_char_p
    L.aria_orb_stream.restype = C.c_void_p
    L.aria_matcher_stream.restype = C.c_void_p
    L.aria_orb_destroy.restype = None
    L.aria_matcher_destroy.restype = None
    L.aria_orb_destroy.argtypes = [C.c_void_p]
    L.aria_matcher_destroy.argtypes = [C.c_void_p]
    L.aria_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.POINTER(C.c_int)]
    L.aria_orb_extract_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.aria_orb_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.aria_orb_extract_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.aria_orb_check.argtypes = [C.c_void_p]
    L.aria_orb_slow_path_blocks.argtypes = [C.c_void_p, C.c_int]
    L.aria_orb_slow_path_blocks.restype = C.c_longlong
    L.aria_orb_stream.argtypes = [C.c_void_p]
    L.aria_orb_set_max_features.argtypes = [C.c_void_p, C.c_int]
    L.aria_orb_get_max_features.argtypes = [C.c_void_p]
    L.aria_orb_kp_capacity.argtypes = [C.c_void_p]
    L.aria_orb_rows_needed.argtypes = [C.c_void_p]
    L.aria_orb_fetch_last.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.aria_orb_level_info.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.aria_orb_resize_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.aria_orb_debug_read_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.aria_orb_algorithmic_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.aria_matcher_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                     C.c_int, C.POINTER(C.c_int)]
    L.aria_orb_fast_blur_kernel.argtypes = [C.c_void_p]
    L.aria_orb_fast_blur_kernel.restype = C.c_char_p
    L.aria_matcher_knn_kernel.argtypes = [C.c_void_p]
    L.aria_matcher_knn_kernel.restype = C.c_char_p
    L.aria_orb_last_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.aria_matcher_match_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                            C.c_int, C.POINTER(C.c_int)]
    L.aria_matcher_retain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.aria_matcher_resident_rows.argtypes = [C.c_void_p]
    L.aria_matcher_match_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.aria_matcher_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.aria_matcher_knn2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.aria_matcher_match_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int]
    L.aria_matcher_match_db_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_int64, C.c_double, C.c_void_p]
    L.aria_flag_keypoints_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_void_p]
    L.aria_flag_keypoints_shifted_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.aria_matcher_match_batch_filtered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                           C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                           C.c_void_p, C.c_int, C.c_void_p]
    L.aria_orb_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.aria_orb_set_stage_event.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.aria_orb_get_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64)]
    L.aria_matcher_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.aria_matcher_get_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int64)]
    L.aria_matcher_stream.argtypes = [C.c_void_p]
    L.aria_matcher_sync.argtypes = [C.c_void_p]
    for prefix in STAGES:
        if hasattr(L, "aria_%s_create" % prefix):   # absent from A/B builds of the extractor sources alone (tools/build_ab.sh)
            globals()["_bind_" + prefix](L)
    L.aria_synth_frame_pair.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.aria_synth_sequence.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    _lib = L
    return L


# Every stage handle, by the prefix of its C entry points (aria_<prefix>_create, ...), in the order the stages were added.
STAGES = ("pose", "map", "fund", "graph", "fuse", "eval", "det", "stereo", "rect", "dense", "tsdf", "nav", "alert", "pnp", "ba", "ray",
          "icp", "mesh", "proj", "bow", "sim3", "sgraph")


def _bind_handle(L, prefix):
    """The prototypes every stage handle has: aria_<prefix>_default_config / _create / _destroy / _stream / _check."""
    fn = lambda name: getattr(L, "aria_%s_%s" % (prefix, name))   # noqa: E731
    fn("default_config").restype = None
    fn("default_config").argtypes = [C.c_void_p]
    fn("create").argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    fn("destroy").restype = None
    fn("destroy").argtypes = [C.c_void_p]
    fn("stream").restype = C.c_void_p
    fn("stream").argtypes = [C.c_void_p]
    fn("check").argtypes = [C.c_void_p]


def _bind_pose(L):
    _bind_handle(L, "pose")
    L.aria_pose_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]
    L.aria_pose_estimate_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p]
    L.aria_pose_debug_hypotheses.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]


def _bind_map(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "map")
    L.aria_map_triangulate.argtypes = [p, p, i, p, i, p, i, i, p, p, p, i, i, i, p, i, p]
    L.aria_map_triangulate_batch_device.argtypes = [p, p, p, p, p, i64, p, p, i, i, i, i, p, p, p, p, i64, i, i, i, p]
    L.aria_map_points_needed.argtypes = [p, C.POINTER(C.c_int64)]
    L.aria_map_size.argtypes = [p, C.POINTER(C.c_int64)]
    L.aria_map_capacity.restype = i64
    L.aria_map_capacity.argtypes = [p]
    L.aria_map_clear.argtypes = [p]
    L.aria_map_reserve.argtypes = [p, i64]
    L.aria_map_read.argtypes = [p, i64, i64, p]
    L.aria_map_device_points.restype = p
    L.aria_map_device_points.argtypes = [p]
    L.aria_map_filter_outliers.argtypes = [p]
    L.aria_map_filter_distance.argtypes = [p, C.c_double]


def _bind_fund(L):
    p, i = C.c_void_p, C.c_int
    _bind_handle(L, "fund")
    L.aria_fund_estimate.argtypes = [p, p, i, p, i, p, i, i, i, p, p]
    L.aria_fund_estimate_batch_device.argtypes = [p, p, p, p, p, C.c_int64, p, p, i, i, i, i, p, p, p, p]
    L.aria_fund_debug_hypotheses.argtypes = [p, p, i, p, i, p, i, i, i, p, p, p, p]


def _bind_graph(L):
    p, i = C.c_void_p, C.c_int
    _bind_handle(L, "graph")
    L.aria_graph_optimize.argtypes = [p, p, i, i, p, i, i, p]
    L.aria_graph_optimize_batch_device.argtypes = [p, p, p, p, p, p, i, i, p]
    L.aria_graph_debug_linearize.argtypes = [p, p, i, i, p, i, p, p, p, p]


def _bind_fuse(L):
    p, i = C.c_void_p, C.c_int
    _bind_handle(L, "fuse")
    L.aria_fuse_filter_init.argtypes = [p, p]
    L.aria_fuse_run_batch_device.argtypes = [p, p, p, p, i, p, p, p, i, i, p]
    L.aria_fuse_run.argtypes = [p, p, p, i, p, p, i, p]
    L.aria_fuse_visual_from_pose_device.argtypes = [p, p, p, i, i, p]
    L.aria_fuse_preintegrate_batch_device.argtypes = [p, p, i, p, p, i, p, p]
    L.aria_fuse_preintegrate.argtypes = [p, p, i, p, p, i, p, p]


def _bind_eval(L):
    p, i = C.c_void_p, C.c_int
    _bind_handle(L, "eval")
    L.aria_eval_sample_truth_device.argtypes = [p, p, i, p, i, p, p]
    L.aria_eval_sample_truth.argtypes = [p, p, i, p, i, p, p]
    L.aria_eval_batch_device.argtypes = [p, p, i, p, i, i, p, i, i, p, i, i, p, p]
    L.aria_eval_batch.argtypes = [p, p, i, p, i, i, p, i, i, p, i, i, p, p]


def _bind_det(L):
    p, i, f = C.c_void_p, C.c_int, C.c_float
    _bind_handle(L, "det")
    L.aria_det_check.argtypes = [p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.aria_det_device_buffers.argtypes = [p] + [C.POINTER(C.c_void_p)] * 6
    L.aria_det_preprocess_batch_device.argtypes = [p, p, i, i, i, i, C.c_int64, i, i, p]
    L.aria_det_postprocess_batch_device.argtypes = [p, p, i, i, i, i, f, f, p, i, p, p, i, p, p, i]
    L.aria_det_preprocess.argtypes = [p, p, i, i, i, i, i, p]
    L.aria_det_postprocess.argtypes = [p, p, i, i, i, f, f, p, i, p, i, C.POINTER(C.c_int), p, i, C.POINTER(C.c_int)]
    L.aria_det_resize_table.argtypes = [i, i, p, i]
    L.aria_det_algorithmic_bytes.restype = C.c_int64
    L.aria_det_algorithmic_bytes.argtypes = [i, i, i, i, i, i]


def _bind_stereo(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "stereo")
    L.aria_stereo_match_batch_device.argtypes = [p, p, p, i64, i, i, i, p, p, p, p, p, p, i64, i, p, p, p, i]
    L.aria_stereo_match.argtypes = [p, p, p, i, i, i, p, p, i, p, p, i, p, p, C.POINTER(C.c_int)]
    L.aria_stereo_scale_batch_device.argtypes = [p, p, p, p, p, i, i, p, p, p, p, i64, i, p]
    L.aria_stereo_scale_pose.argtypes = [p, p, p, p, i, i, p, i, p, i, p]


def _bind_rect(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "rect")
    L.aria_rect_stereo_geometry.argtypes = [p, p, p, p, p, C.POINTER(C.c_double)]
    L.aria_rect_remap_batch_device.argtypes = [p, i, p, i64, i, i, p, i64, i]
    L.aria_rect_remap.argtypes = [p, i, p, i, p, i]
    L.aria_rect_points_batch_device.argtypes = [p, i, p, p, i64, i, p]
    L.aria_rect_points.argtypes = [p, i, p, i, p]
    L.aria_rect_get_map.argtypes = [p, i, p, i]
    L.aria_rect_algorithmic_bytes.restype = i64
    L.aria_rect_algorithmic_bytes.argtypes = [i, i]


def _bind_dense(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "dense")
    L.aria_dense_compute_batch_device.argtypes = [p, p, p, i64, i, i, i, i, p, i64, i, p, i64, i]
    L.aria_dense_compute.argtypes = [p, p, p, i, i, i, p, p]
    L.aria_dense_sample_batch_device.argtypes = [p, p, i64, i, i, i, p, p, i64, i, p]
    L.aria_dense_sample.argtypes = [p, p, i, i, i, p, i, p]
    L.aria_dense_pairs_in_flight.argtypes = [p]
    L.aria_dense_scratch_bytes_per_pair.restype = i64
    L.aria_dense_scratch_bytes_per_pair.argtypes = [i, i]
    L.aria_dense_algorithmic_bytes.restype = i64
    L.aria_dense_algorithmic_bytes.argtypes = [i, i]


def _bind_tsdf(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "tsdf")
    L.aria_tsdf_clear.argtypes = [p]
    L.aria_tsdf_integrate_batch_device.argtypes = [p, p, i64, i, i, i, p, p, p, i64, i, i]
    L.aria_tsdf_integrate.argtypes = [p, p, i, i, i, p, p, i]
    L.aria_tsdf_extract_points_device.argtypes = [p, p, i64, p]
    L.aria_tsdf_extract_points.argtypes = [p, p, i64, C.POINTER(i64)]
    L.aria_tsdf_device_voxels.restype = p
    L.aria_tsdf_device_voxels.argtypes = [p]
    L.aria_tsdf_read_box.argtypes = [p, i, i, i, i, i, i, p]
    L.aria_tsdf_volume_bytes.restype = i64
    L.aria_tsdf_volume_bytes.argtypes = [i, i, i]
    L.aria_tsdf_algorithmic_bytes.restype = i64
    L.aria_tsdf_algorithmic_bytes.argtypes = [i, i, i, i, i, i]


def _bind_icp(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "icp")
    L.aria_icp_track_batch_device.argtypes = [p, p, i64, i, p, i64, i, p, i64, i, p, p, p, i, i, i, p, p]
    L.aria_icp_track.argtypes = [p, p, p, p, p, p, i, i, p, p]
    L.aria_icp_debug_system_device.argtypes = [p, p, i64, i, p, i64, i, p, i64, i, p, p, i, i, i, i, p]
    L.aria_icp_algorithmic_bytes.restype = i64
    L.aria_icp_algorithmic_bytes.argtypes = [p, i, i, i]


def _bind_ray(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "ray")
    L.aria_ray_update_from_volume_device.argtypes = [p, p]
    L.aria_ray_cast_batch_device.argtypes = [p, p, p, i, i, i, p, i64, i, p, i64, i, p, i64, i, p, i64, i, p]
    L.aria_ray_cast.argtypes = [p, p, i, i, p, p, p, p, p]
    L.aria_ray_algorithmic_bytes.restype = i64
    L.aria_ray_algorithmic_bytes.argtypes = [i, i, i, i]


def _bind_mesh(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "mesh")
    L.aria_mesh_update_from_volume_device.argtypes = [p, p]
    L.aria_mesh_extract_device.argtypes = [p, p, i64, p, i64, p]
    L.aria_mesh_extract.argtypes = [p, p, i64, p, i64, p]
    L.aria_mesh_scratch_bytes.restype = i64
    L.aria_mesh_scratch_bytes.argtypes = [i, i, i]
    L.aria_mesh_algorithmic_bytes.restype = i64
    L.aria_mesh_algorithmic_bytes.argtypes = [i, i, i, i64, i64]


def _bind_nav(L):
    p, i = C.c_void_p, C.c_int
    _bind_handle(L, "nav")
    L.aria_nav_update_from_volume_device.argtypes = [p, p]
    L.aria_nav_set_cells_device.argtypes = [p, p]
    L.aria_nav_set_cells.argtypes = [p, p]
    L.aria_nav_read_cells.argtypes = [p, p]
    L.aria_nav_read_clearance.argtypes = [p, p]
    L.aria_nav_read_costs.argtypes = [p, p]
    L.aria_nav_solve_device.argtypes = [p, p, i]
    L.aria_nav_trace_device.argtypes = [p, p, i, p, p, i]
    L.aria_nav_plan.argtypes = [p, p, i, p, i, p, p, i]
    L.aria_nav_device_fields.restype = p
    L.aria_nav_device_fields.argtypes = [p]
    L.aria_nav_read_field.argtypes = [p, i, p]
    L.aria_nav_read_rounds.argtypes = [p, p, i]
    L.aria_nav_field_bytes.restype = C.c_int64
    L.aria_nav_field_bytes.argtypes = [i, i, i]


def _bind_alert(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "alert")
    L.aria_alert_dets_seen.argtypes = [p]
    L.aria_alert_measure_batch_device.argtypes = [p, p, i64, i, i, p, p, i, p]
    L.aria_alert_arbitrate_batch_device.argtypes = [p, p, i, p, i, p, p, p, i, p, p, i, p]
    L.aria_alert_run_batch_device.argtypes = [p, p, i64, i, i, p, p, i, p, i, p, p, p, i, p]
    L.aria_alert_measure.argtypes = L.aria_alert_measure_batch_device.argtypes
    L.aria_alert_arbitrate.argtypes = L.aria_alert_arbitrate_batch_device.argtypes
    L.aria_alert_run.argtypes = L.aria_alert_run_batch_device.argtypes
    L.aria_alert_zone_bounds.argtypes = [i, p]
    L.aria_alert_algorithmic_bytes.restype = i64
    L.aria_alert_algorithmic_bytes.argtypes = [i, i, i, i]


def _bind_ba(L):
    p, i, d = C.c_void_p, C.c_int, C.c_double
    _bind_handle(L, "ba")
    L.aria_ba_optimize.argtypes = [p, p, p, i, p, p, i, p, i, i, p, p]
    L.aria_ba_optimize_batch_device.argtypes = [p, p, p, p, p, p, p, p, p, i, i, i, i, i, p, p]
    L.aria_ba_debug_linearize.argtypes = [p, p, p, i, p, p, i, p, i, d, C.POINTER(d), C.POINTER(i), p, p, p, p]
    L.aria_ba_window_from_chain_device.argtypes = [p, p, p, p, i, i, i, p, p, p, p, C.c_int64, p, p, i, i, i, i, p, p, p, p, p]


def _bind_sim3(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "sim3")
    L.aria_sim3_estimate.argtypes = [p, p, i, i, p, p]
    L.aria_sim3_estimate_batch_device.argtypes = [p, p, p, i, i, i, p, p]
    L.aria_sim3_debug_hypotheses.argtypes = [p, p, i, i, p, p, p, p, p]
    L.aria_sim3_associate_batch_device.argtypes = [p, p, p, p, i, i, p, p, p, p, p, p, i64, p, p, i, i, p, p, p]


def _bind_sgraph(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "sgraph")
    L.aria_sgraph_optimize.argtypes = [p, p, i, i, p, i, i, p]
    L.aria_sgraph_optimize_batch_device.argtypes = [p, p, p, p, p, p, i, i, p]
    L.aria_sgraph_debug_linearize.argtypes = [p, p, i, i, p, i, p, p, p, p]
    L.aria_sgraph_vertices_from_pose_device.argtypes = [p, p, p, i]
    L.aria_sgraph_poses_from_vertices_device.argtypes = [p, p, p, i]
    L.aria_sgraph_correct_map_device.argtypes = [p, p, p, i, i, p, p, i, p]
    L.aria_sgraph_correct_points_device.argtypes = [p, p, i64, p, i, i, p, p, i, p]


def _bind_pnp(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "pnp")
    L.aria_pnp_estimate.argtypes = [p, p, i, i, p, p]
    L.aria_pnp_estimate_batch_device.argtypes = [p, p, p, i, i, i, p, p]
    L.aria_pnp_debug_hypotheses.argtypes = [p, p, i, i, p, p, p, p]
    L.aria_pnp_associate_batch_device.argtypes = [p, p, i, i, p, p, i64, p, p, i, i, p, p, p]
    L.aria_pnp_set_solver.argtypes = [p, i]
    L.aria_pnp_get_solver.argtypes = [p]


def _bind_bow(L):
    p, i, i64, ll, ip = C.c_void_p, C.c_int, C.c_int64, C.c_longlong, C.POINTER(C.c_int)
    _bind_handle(L, "bow")
    L.aria_bow_words.argtypes = [p]
    L.aria_bow_train_device.argtypes = [p, p, p, i, i64, ip]
    L.aria_bow_train.argtypes = [p, p, p, i, i64, ip]
    L.aria_bow_set_vocabulary.argtypes = [p, p, p, i]
    L.aria_bow_get_vocabulary.argtypes = [p, p, p, ip]
    L.aria_bow_save.argtypes = [p, C.c_char_p]
    L.aria_bow_load.argtypes = [p, C.c_char_p]
    L.aria_bow_transform_batch_device.argtypes = [p, p, p, i, i64, p, p]
    L.aria_bow_add_batch_device.argtypes = [p, p, p, p, i]
    L.aria_bow_add.argtypes = [p, ll, p, i]
    L.aria_bow_add_device.argtypes = [p, ll, p, i]
    L.aria_bow_size.argtypes = [p]
    L.aria_bow_info.argtypes = [p, i, C.POINTER(ll), ip]
    L.aria_bow_query_batch_device.argtypes = [p, p, p, p, i, p, p]
    L.aria_bow_query.argtypes = [p, ll, p, i, p, ip]
    L.aria_bow_query_device.argtypes = [p, ll, p, i, p, ip]


def _bind_proj(L):
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    _bind_handle(L, "proj")
    L.aria_proj_search_batch_device.argtypes = [p, p, p, p, p, i64, i, i, p, i, p, i, i, p, p, p, p]
    L.aria_proj_search.argtypes = [p, p, p, p, i, i, i, p, i, p, p, p, C.POINTER(C.c_int)]
    L.aria_proj_landmarks_from_map_device.argtypes = [p, p, i64, i64, i, i, p, p, p, i64, i, p, p]


def status_string(status):
    return load_library().aria_status_string(int(status)).decode()


def abi_version():
    return load_library().aria_abi_version()


def check(status, where):
    if status != ARIA_OK:
        raise AriaError(status, where)


def level_info(max_features, width, height):
    """[(level_width, level_height, quota, scale)] x 8 -- host-only plan geometry."""
    L = load_library()
    out = []
    for l in range(8):
        lw, lh, q, s = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        check(L.aria_orb_level_info(max_features, width, height, l, C.byref(lw), C.byref(lh), C.byref(q), C.byref(s)),
              "aria_orb_level_info")
        out.append((lw.value, lh.value, q.value, s.value))
    return out


def resize_table(width, height, level, axis):
    """(offsets, next-pixel weights in 1/256) of the INTER_LINEAR_EXACT table of `level` along `axis`."""
    buf = np.zeros(4096, np.uint32)
    n = load_library().aria_orb_resize_table(width, height, level, axis, buf.ctypes.data, len(buf))
    if n < 0:
        raise AriaError(n, "aria_orb_resize_table")
    return (buf[:n] & 0xFFFF).astype(np.int32), (buf[:n] >> 16).astype(np.int32)


def pyramid_bands(width, height):
    """(bands[nb, 8, 4] = {comp_lo, comp_n, own_lo, own_n}, band_rows, lds_bytes) of the fused pyramid kernel."""
    buf = np.zeros(300 * 32, np.int32)
    bh, lds = C.c_int(), C.c_int()
    L = load_library()
    L.aria_orb_pyramid_bands.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    n = L.aria_orb_pyramid_bands(width, height, buf.ctypes.data, len(buf), C.byref(bh), C.byref(lds))
    if n < 0:
        raise AriaError(n, "aria_orb_pyramid_bands")
    return buf[:n].reshape(-1, 8, 4).copy(), bh.value, lds.value


def algorithmic_bytes(width, height, n_keypoints):
    be, bf = C.c_int64(), C.c_int64()
    check(load_library().aria_orb_algorithmic_bytes(width, height, n_keypoints, C.byref(be), C.byref(bf)),
          "aria_orb_algorithmic_bytes")
    return be.value, bf.value


def synth_frame_pair(seed, width=640, height=480):
    """Synthetic frame pair of SURVEY.md 8(d): B shows A's content moved by (+3, +2) px."""
    a = np.empty((height, width), np.uint8)
    b = np.empty((height, width), np.uint8)
    check(load_library().aria_synth_frame_pair(seed, width, height, a.ctypes.data, b.ctypes.data), "aria_synth_frame_pair")
    return a, b


def synth_sequence(seed0, n_pairs, width=640, height=480, out=None, n_threads=None):
    """2*n_pairs frames A(seed0), B(seed0), A(seed0+1), ... as one (2*n_pairs, H, W) uint8 array."""
    if out is None:
        out = np.empty((2 * n_pairs, height, width), np.uint8)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size == 2 * n_pairs * height * width
    if n_threads is None:
        n_threads = max(1, min(32, len(os.sched_getaffinity(0))))
    check(load_library().aria_synth_sequence(seed0, n_pairs, width, height, out.ctypes.data, n_threads), "aria_synth_sequence")
    return out
