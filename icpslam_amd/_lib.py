"""ctypes binding of include/icpgpu.h (libicpgpu.so).  Fails loudly when the HIP library is missing:
there is no CPU or PyTorch fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ICPGPU_FLAVOUR=dev: the development flavour (libicpgpu_dev.so, built with -DICPGPU_DEV_SWITCHES: kernel variants, tuning
# constants and test modes behind environment switches -- icpslam_amd/csrc/icp_env.h).  A process loads ONE flavour; the
# tests of the development modes run in sub-processes (tests/conftest.py: the dev_flavour fixture).  Default: the release library.
FLAVOUR = "dev" if os.environ.get("ICPGPU_FLAVOUR", "") == "dev" else "release"
LIB_PATH = os.path.join(_HERE, "libicpgpu_dev.so" if FLAVOUR == "dev" else "libicpgpu.so")
if os.environ.get("ICPGPU_LIB_PATH"):   # A/B builds of an experiment (scripts/): an explicit library file
    LIB_PATH = os.environ["ICPGPU_LIB_PATH"]

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_NO_INPUT, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
P2P_SVD, GICP, P2PLANE, NDT = 0, 1, 2, 3
NDT_LINE_SEARCH_PCL18, NDT_LINE_SEARCH_MORE_THUENTE = 0, 1      # icpgpu_ndt_line_search
# icpgpu_ndt_mt_exit: how a More-Thuente search ends (TRIAL = not yet)
MT_TRIAL, MT_WOLFE, MT_INTERVAL, MT_TRIAL_CAP, MT_NAN_STEP, MT_NON_FINITE = 0, 1, 2, 3, 4, 5
GICP_INNER_EXACT, GICP_INNER_QUADRATIC = 0, 1
GICP_SOLVER_NONE, GICP_SOLVER_HOST, GICP_SOLVER_DEVICE, GICP_SOLVER_QUADRATIC = 0, 1, 2, 3
HEADER_VERSION = 1002          # the icpgpu.h these mirrors were written against (ICPGPU_HEADER_VERSION)
NN_AUTO, NN_BRUTE, NN_GRID = 0, 1, 2
REJECT_MEDIAN_DISTANCE, REJECT_TRIMMED, REJECT_ONE_TO_ONE, REJECT_SURFACE_NORMAL = 1, 2, 3, 4   # icpgpu_rejector_kind
REJECT_SAMPLE_CONSENSUS = 5    # ... a stage that waits on the host (include/icpgpu.h "sample-consensus rejector")
RSAC_DRAWS = 16                # ICPGPU_RSAC_DRAWS
RSAC_MAX_ITERATIONS = 65536    # ICPGPU_RSAC_MAX_ITERATIONS
MAX_REJECTORS = 4
SOR_MAX_K = 63                 # ICPGPU_SOR_MAX_K
SEARCH_MAX_K = 64              # ICPGPU_SEARCH_MAX_K
SAC_MAX_ITERATIONS = 1 << 20   # ICPGPU_SAC_MAX_ITERATIONS
SCP_MAX_ITERATIONS = 1 << 20   # ICPGPU_SCP_MAX_ITERATIONS
SCP_CHUNK = 65536              # ICPGPU_SCP_CHUNK
SCP_MAX_SAMPLES = 8            # ICPGPU_SCP_MAX_SAMPLES
SCP_INVALID, SCP_PREREJECTED, SCP_NO_TRANSFORM, SCP_EVALUATED = 0, 1, 2, 3   # ICPGPU_SCP_*
SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE = 0, 15   # pcl::SacModel's values
SAC_RANSAC = 0                 # pcl's method_types.h
# ICPGPU_SACMODEL_CYLINDER / _NORMAL_PLANE: pcl::SacModel's values by the order of PCL 1.8's model_types.h (PCL itself is not
# installed where this was written, so no PCL build has confirmed them)
SACMODEL_CYLINDER, SACMODEL_NORMAL_PLANE = 5, 11
SAC_CYLINDER_ITERATIONS = 10   # ICPGPU_SAC_CYLINDER_ITERATIONS
SAC_STOP_PASSES, SAC_STOP_CHOLESKY, SAC_STOP_NOT_FINITE, SAC_STOP_SMALL_STEP, SAC_STOP_NO_DECREASE = 1, 2, 3, 4, 5   # ICPGPU_SAC_STOP_*
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3   # icpgpu_morph_op
PMF_MAX_PASSES = 32            # ICPGPU_PMF_MAX_PASSES
SEGMENTS_HOST, SEGMENTS_CLUSTERS, SEGMENTS_REGIONS = 0, 1, 2   # ICPGPU_SEGMENTS_*
SEGMENT_OK, SEGMENT_EMPTY = 0, 1                               # ICPGPU_SEGMENT_*
SEGMENT_CHUNK = 64             # ICPGPU_SEGMENT_CHUNK
FPS_ONE_WORKGROUP_MAX = 16384  # ICPGPU_FPS_ONE_WORKGROUP_MAX
SUBSET_PASS_THROUGH, SUBSET_CROP_BOX, SUBSET_UNIFORM_SAMPLING, SUBSET_FARTHEST_POINT_SAMPLING = 1, 2, 3, 4   # ICPGPU_SUBSET_*
FPS_PATH_ONE, FPS_PATH_MANY = 1, 2                             # ICPGPU_FPS_PATH_*
STATE_NAMES = {0: "NOT_CONVERGED", 1: "ITERATIONS", 2: "TRANSFORM", 3: "ABS_MSE", 4: "REL_MSE",
               5: "NO_CORRESPONDENCES"}


class Params(C.Structure):
    _fields_ = [("method", C.c_int32), ("max_iterations", C.c_int32), ("transformation_epsilon", C.c_double),
                ("max_correspondence_distance", C.c_double), ("euclidean_fitness_epsilon", C.c_double),
                ("min_correspondences", C.c_int32), ("force_iterations", C.c_int32), ("nn_mode", C.c_int32),
                ("brute_variant", C.c_int32), ("gicp_inner", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("convergence_state", C.c_int32), ("n_correspondences", C.c_uint32), ("mse_last", C.c_double),
                ("fitness", C.c_double), ("t_total_ms", C.c_double), ("t_device_ms", C.c_double),
                ("gicp_solver", C.c_int32), ("reserved0", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("nn_launches", C.c_uint64), ("nn_ms", C.c_double), ("nn_pairs", C.c_uint64),
                ("nn_bytes", C.c_uint64), ("reduce_launches", C.c_uint64), ("reduce_ms", C.c_double),
                ("reduce_bytes", C.c_uint64), ("transform_launches", C.c_uint64), ("transform_ms", C.c_double),
                ("transform_bytes", C.c_uint64), ("iterations", C.c_uint64), ("aligns", C.c_uint64),
                ("grid_launches", C.c_uint64), ("grid_ms", C.c_double), ("grid_bytes", C.c_uint64),
                ("grid_builds", C.c_uint64), ("grid_build_ms", C.c_double), ("grid_fallback_points", C.c_uint64),
                ("voxel_launches", C.c_uint64), ("voxel_ms", C.c_double), ("voxel_bytes", C.c_uint64),
                ("gicp_cov_launches", C.c_uint64), ("gicp_cov_ms", C.c_double), ("gicp_cost_launches", C.c_uint64),
                ("map_inserts", C.c_uint64), ("map_insert_ms", C.c_double), ("map_points_in", C.c_uint64),
                ("map_nn_launches", C.c_uint64), ("map_nn_ms", C.c_double),
                ("nn_timed", C.c_uint64), ("grid_timed", C.c_uint64), ("reduce_timed", C.c_uint64),
                ("grid_bounded", C.c_uint64), ("gicp_eval_ms", C.c_double), ("gicp_eval_corr", C.c_uint64), ("gicp_cov_points", C.c_uint64),
                ("targets_recognised", C.c_uint64), ("brute_bound_violations", C.c_uint64),
                ("brute_bound_worst", C.c_double), ("gicp_device_solves", C.c_uint64),
                ("grid_adopted", C.c_uint64), ("sources_adopted", C.c_uint64), ("gicp_host_solves", C.c_uint64),
                ("gicp_solver_choice", C.c_uint64), ("gicp_quadratic_solves", C.c_uint64),
                ("cov_grids_unchecked", C.c_uint64), ("cov_grids_rebuilt", C.c_uint64), ("voxel_views_direct", C.c_uint64)]


class Rejector(C.Structure):
    _fields_ = [("kind", C.c_int32), ("min_correspondences", C.c_int32), ("value", C.c_double)]


class SegmentRecord(C.Structure):
    _fields_ = [("count", C.c_int64), ("status", C.c_int32), ("first", C.c_int32), ("K", C.c_double * 3), ("moments", C.c_double * 9),
                ("centroid", C.c_double * 3), ("cov", C.c_double * 6), ("eigenvalues", C.c_double * 3), ("axes", C.c_double * 9),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("obb_lo", C.c_double * 3), ("obb_hi", C.c_double * 3),
                ("obb_position", C.c_double * 3), ("obb_dims", C.c_double * 3)]


class Pose(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("quat", C.c_double * 4)]


# every symbol include/icpgpu.h declares (tests/test_abi.py checks the header against this list)
EXPORTS = [
    "icpgpu_create_abi", "icpgpu_destroy", "icpgpu_last_error", "icpgpu_version", "icpgpu_default_params_sz", "icpgpu_struct_sizes",
    "icpgpu_calibrate", "icpgpu_set_params", "icpgpu_get_params", "icpgpu_set_source", "icpgpu_set_target",
    "icpgpu_set_source_device", "icpgpu_set_target_device", "icpgpu_promote_source_to_target", "icpgpu_align", "icpgpu_align_view",
    "icpgpu_fingerprint", "icpgpu_cloud_sizes", "icpgpu_align_batch_multi_sz", "icpgpu_multi_last_error",
    "icpgpu_fitness", "icpgpu_align_batch", "icpgpu_nn", "icpgpu_reduce", "icpgpu_sweep_sums", "icpgpu_solve", "icpgpu_transform",
    "icpgpu_profile_reset", "icpgpu_profile_get", "icpgpu_profile_set_sampling", "icpgpu_get_stream", "icpgpu_synchronize",
    "icpgpu_voxel_grid", "icpgpu_voxel_plan", "icpgpu_voxel_grid_fetch", "icpgpu_voxel_grid_view", "icpgpu_set_source_voxel_filtered", "icpgpu_gicp_covariances",
    "icpgpu_gicp_quadratic_eval", "icpgpu_gicp_quadratic_sums",
    "icpgpu_pose_from_matrix", "icpgpu_pose_to_matrix", "icpgpu_pose_compose", "icpgpu_pose_inverse", "icpgpu_posegraph_create",
    "icpgpu_posegraph_destroy", "icpgpu_posegraph_set_initial_pose", "icpgpu_posegraph_push",
    "icpgpu_posegraph_num_poses", "icpgpu_posegraph_num_keyframes", "icpgpu_posegraph_get_pose",
    "icpgpu_posegraph_get_keyframe", "icpgpu_posegraph_get_edge", "icpgpu_posegraph_write_g2o",
    "icpgpu_map_set_search", "icpgpu_map_reset", "icpgpu_map_add_points", "icpgpu_map_add_source", "icpgpu_map_size", "icpgpu_map_get_points",
    "icpgpu_map_nn_target", "icpgpu_count_candidates", "icpgpu_count_candidates_read",
    "icpgpu_set_target_normals", "icpgpu_normals", "icpgpu_reduce_point_to_plane", "icpgpu_solve_point_to_plane",
    "icpgpu_set_ndt_params", "icpgpu_get_ndt_params", "icpgpu_ndt_transformation_probability", "icpgpu_ndt_cells",
    "icpgpu_ndt_derivatives", "icpgpu_ndt_step", "icpgpu_set_ndt_line_search", "icpgpu_get_ndt_line_search", "icpgpu_ndt_gradient",
    "icpgpu_ndt_line_search_replay", "icpgpu_ndt_line_search_trace",
    "icpgpu_set_correspondence_rejectors", "icpgpu_get_correspondence_rejectors", "icpgpu_correspondences", "icpgpu_rejector_stats",
    "icpgpu_set_reciprocal_correspondences", "icpgpu_get_reciprocal_correspondences", "icpgpu_reciprocal_stats",
    "icpgpu_set_rejector_sac_seed", "icpgpu_get_rejector_sac_seed", "icpgpu_correspondence_rejector_sample_consensus",
    "icpgpu_rejector_sac_fetch",
    "icpgpu_statistical_outlier_removal", "icpgpu_statistical_outlier_removal_view", "icpgpu_radius_outlier_removal",
    "icpgpu_radius_outlier_removal_view", "icpgpu_outlier_stats", "icpgpu_outlier_fetch",
    "icpgpu_search_set_input", "icpgpu_search_size", "icpgpu_search_knn", "icpgpu_search_radius",
    "icpgpu_normal_estimation",
    "icpgpu_fpfh_estimation",
    "icpgpu_feature_knn",
    "icpgpu_euclidean_cluster_extraction", "icpgpu_cluster_fetch",
    "icpgpu_region_growing", "icpgpu_region_fetch",
    "icpgpu_segment_moments", "icpgpu_segment_stats",
    "icpgpu_scp_align", "icpgpu_scp_fetch", "icpgpu_scp_stats",
    "icpgpu_iss_keypoints", "icpgpu_iss_fetch", "icpgpu_iss_stats",
    "icpgpu_boundary_estimation", "icpgpu_iss_keypoints_border", "icpgpu_iss_fetch_border",
    "icpgpu_moving_least_squares", "icpgpu_mls_fetch", "icpgpu_mls_stats",
    "icpgpu_pass_through", "icpgpu_pass_through_view", "icpgpu_crop_box", "icpgpu_crop_box_view", "icpgpu_crop_box_matrix",
    "icpgpu_uniform_sampling", "icpgpu_uniform_sampling_view", "icpgpu_farthest_point_sampling", "icpgpu_farthest_point_sampling_view",
    "icpgpu_subset_fetch", "icpgpu_subset_removed", "icpgpu_subset_stats",
    "icpgpu_sac_plane_segmentation", "icpgpu_sac_fetch", "icpgpu_sac_stats", "icpgpu_sac_extract", "icpgpu_sac_extract_view",
    "icpgpu_sac_segmentation_from_normals", "icpgpu_sac_normals_fetch", "icpgpu_sac_normals_stats",
    "icpgpu_morphological_operator", "icpgpu_progressive_morphological_filter", "icpgpu_pmf_fetch", "icpgpu_pmf_stats", "icpgpu_pmf_extract",
    "icpgpu_pmf_extract_view",
    "icpgpu_set_source_normals", "icpgpu_set_p2plane_symmetric", "icpgpu_get_p2plane_symmetric",
    "icpgpu_reduce_symmetric_point_to_plane", "icpgpu_solve_symmetric_point_to_plane",
]

_lib = None


class IcpGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"icpgpu error {code}: {msg}")
        self.code = code


def load():
    """dlopen libicpgpu.so and declare the prototypes. Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C icpslam_amd/csrc`). icpslam_amd has no fallback path.")
    try:  # share torch's HIP runtime when torch is in the process (same SONAME)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.icpgpu_create_abi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t]
    L.icpgpu_struct_sizes.argtypes = [C.POINTER(C.c_size_t)]
    L.icpgpu_struct_sizes.restype = None
    L.icpgpu_calibrate.argtypes = [vp, C.POINTER(C.c_int)]
    L.icpgpu_destroy.argtypes = [vp]
    L.icpgpu_last_error.argtypes = [vp]
    L.icpgpu_last_error.restype = C.c_char_p
    L.icpgpu_version.argtypes = []
    L.icpgpu_default_params_sz.argtypes = [C.POINTER(Params), C.c_size_t]
    L.icpgpu_default_params_sz.restype = None
    L.icpgpu_set_params.argtypes = [vp, C.POINTER(Params)]
    L.icpgpu_get_params.argtypes = [vp, C.POINTER(Params)]
    L.icpgpu_set_source.argtypes = [vp, fp, C.c_size_t]
    L.icpgpu_set_target.argtypes = [vp, fp, C.c_size_t]
    L.icpgpu_set_source_device.argtypes = [vp, vp, C.c_size_t]
    L.icpgpu_set_target_device.argtypes = [vp, vp, C.c_size_t]
    L.icpgpu_promote_source_to_target.argtypes = [vp]
    L.icpgpu_fingerprint.argtypes = [fp, C.c_size_t]
    L.icpgpu_fingerprint.restype = C.c_uint64
    L.icpgpu_cloud_sizes.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.icpgpu_align.argtypes = [vp, fp, fp, C.c_int, C.POINTER(Result)]
    L.icpgpu_align_view.argtypes = [vp, fp, C.c_int, C.POINTER(Result), C.POINTER(fp), C.POINTER(C.c_size_t)]
    L.icpgpu_fitness.argtypes = [vp, C.c_double, dp]
    L.icpgpu_align_batch.argtypes = [vp, C.c_size_t, C.POINTER(fp), C.POINTER(C.c_size_t), C.POINTER(fp),
                                     C.POINTER(C.c_size_t), C.c_int, C.POINTER(Result)]
    L.icpgpu_align_batch_multi_sz.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(Params), C.c_size_t, C.POINTER(fp),
                                              C.POINTER(C.c_size_t), C.POINTER(fp), C.POINTER(C.c_size_t), C.c_int,
                                              C.POINTER(Result), dp, C.c_int, C.c_size_t, C.c_size_t]
    L.icpgpu_multi_last_error.argtypes = []
    L.icpgpu_multi_last_error.restype = C.c_char_p
    L.icpgpu_nn.argtypes = [vp, fp, ip, fp]
    L.icpgpu_reduce.argtypes = [vp, fp, C.c_double, dp]
    L.icpgpu_sweep_sums.argtypes = [vp, fp, C.c_double, dp]
    L.icpgpu_solve.argtypes = [dp, dp]
    L.icpgpu_transform.argtypes = [vp, fp, fp]
    L.icpgpu_gicp_covariances.argtypes = [vp, C.c_int, dp]
    L.icpgpu_gicp_quadratic_eval.argtypes = [dp, fp, dp, dp, dp]
    L.icpgpu_gicp_quadratic_sums.argtypes = [vp, fp, dp]
    L.icpgpu_voxel_plan.argtypes = [fp, fp, C.c_float, ip, ip, ip]
    L.icpgpu_set_target_normals.argtypes = [vp, fp, C.c_size_t]
    L.icpgpu_normals.argtypes = [vp, C.c_int, fp]
    L.icpgpu_reduce_point_to_plane.argtypes = [vp, fp, C.c_double, dp]
    L.icpgpu_solve_point_to_plane.argtypes = [dp, dp]
    L.icpgpu_set_source_normals.argtypes = [vp, fp, C.c_size_t]
    L.icpgpu_set_p2plane_symmetric.argtypes = [vp, C.c_int, C.c_int]
    L.icpgpu_get_p2plane_symmetric.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.icpgpu_reduce_symmetric_point_to_plane.argtypes = [vp, fp, C.c_double, C.c_int, dp]
    L.icpgpu_solve_symmetric_point_to_plane.argtypes = [dp, dp]
    L.icpgpu_set_ndt_params.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.icpgpu_get_ndt_params.argtypes = [vp, dp, dp, dp]
    L.icpgpu_ndt_transformation_probability.argtypes = [vp, dp]
    L.icpgpu_ndt_cells.argtypes = [vp, C.c_size_t, fp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]
    L.icpgpu_ndt_derivatives.argtypes = [vp, dp, dp]
    L.icpgpu_ndt_step.argtypes = [dp, dp, C.c_double, C.c_double, dp, dp, fp]
    L.icpgpu_set_ndt_line_search.argtypes = [vp, C.c_int]
    L.icpgpu_get_ndt_line_search.argtypes = [vp, ip]
    L.icpgpu_ndt_gradient.argtypes = [vp, dp, dp]
    L.icpgpu_ndt_line_search_replay.argtypes = [C.c_double] * 5 + [dp, dp, C.c_int, dp, ip]
    L.icpgpu_ndt_line_search_trace.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int32), dp, dp, dp, C.POINTER(C.c_size_t)]
    L.icpgpu_set_correspondence_rejectors.argtypes = [vp, C.POINTER(Rejector), C.c_size_t]
    L.icpgpu_get_correspondence_rejectors.argtypes = [vp, C.POINTER(Rejector), C.POINTER(C.c_size_t)]
    L.icpgpu_correspondences.argtypes = [vp, fp, ip, fp]
    L.icpgpu_rejector_stats.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), fp, C.POINTER(C.c_size_t)]
    L.icpgpu_set_reciprocal_correspondences.argtypes = [vp, C.c_int]
    L.icpgpu_get_reciprocal_correspondences.argtypes = [vp, C.POINTER(C.c_int)]
    L.icpgpu_reciprocal_stats.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.icpgpu_set_rejector_sac_seed.argtypes = [vp, C.c_uint64]
    L.icpgpu_get_rejector_sac_seed.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.icpgpu_correspondence_rejector_sample_consensus.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, ip, ip, C.c_size_t, C.c_double, C.c_int,
                                                                  C.c_uint64, ip, C.POINTER(C.c_size_t), fp]
    L.icpgpu_rejector_sac_fetch.argtypes = [vp, C.c_size_t, ip, dp, dp, ip, ip, ip, ip, fp, ip, fp, C.POINTER(C.c_size_t), ip]
    L.icpgpu_voxel_grid.argtypes = [vp, fp, C.c_size_t, C.c_float, fp, C.POINTER(C.c_size_t)]
    L.icpgpu_voxel_grid_fetch.argtypes = [vp, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.icpgpu_voxel_grid_view.argtypes = [vp, fp, C.c_size_t, C.c_float, C.POINTER(fp), C.POINTER(C.c_size_t)]
    L.icpgpu_set_source_voxel_filtered.argtypes = [vp, fp, C.c_size_t, C.c_float, C.POINTER(C.c_size_t)]
    L.icpgpu_statistical_outlier_removal.argtypes = [vp, fp, C.c_size_t, C.c_int, C.c_double, C.c_int, fp, C.POINTER(C.c_size_t)]
    L.icpgpu_statistical_outlier_removal_view.argtypes = [vp, fp, C.c_size_t, C.c_int, C.c_double, C.c_int, C.POINTER(fp), C.POINTER(C.c_size_t)]
    L.icpgpu_radius_outlier_removal.argtypes = [vp, fp, C.c_size_t, C.c_double, C.c_int, C.c_int, fp, C.POINTER(C.c_size_t)]
    L.icpgpu_radius_outlier_removal_view.argtypes = [vp, fp, C.c_size_t, C.c_double, C.c_int, C.c_int, C.POINTER(fp), C.POINTER(C.c_size_t)]
    L.icpgpu_outlier_stats.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_size_t)]
    L.icpgpu_outlier_fetch.argtypes = [vp, C.c_size_t, fp, ip, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.icpgpu_search_set_input.argtypes = [vp, fp, C.c_size_t]
    L.icpgpu_search_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.icpgpu_search_knn.argtypes = [vp, fp, C.c_size_t, C.c_int, ip, fp, ip]
    L.icpgpu_search_radius.argtypes = [vp, fp, C.c_size_t, C.c_double, C.c_int, C.c_size_t, C.POINTER(C.c_int64), ip, fp, C.POINTER(C.c_size_t)]
    L.icpgpu_normal_estimation.argtypes = [vp, fp, C.c_size_t, C.c_int, C.c_double, fp, fp, ip, fp]
    L.icpgpu_fpfh_estimation.argtypes = [vp, fp, fp, C.c_size_t, C.c_int, C.c_double, fp, ip, fp]
    L.icpgpu_feature_knn.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, C.c_int, ip, fp, ip]
    L.icpgpu_euclidean_cluster_extraction.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.icpgpu_cluster_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64), ip, ip, ip]
    L.icpgpu_region_growing.argtypes = [vp, fp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.icpgpu_region_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64), ip, ip, ip, ip, ip]
    szp = C.POINTER(C.c_size_t)
    L.icpgpu_sac_plane_segmentation.argtypes = [vp, C.c_double, C.c_int, C.c_double, C.c_uint64, C.c_int, dp, C.c_double, fp, szp, ip, ip]
    L.icpgpu_sac_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, ip, ip, ip, ip, fp, dp, szp]
    L.icpgpu_sac_stats.argtypes = [vp, ip]
    L.icpgpu_sac_segmentation_from_normals.argtypes = [vp, C.c_int, fp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                                                       C.c_uint64, C.c_int, dp, C.c_double, fp, ip, szp, ip, ip]
    L.icpgpu_sac_normals_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, ip, ip, ip, ip, fp, szp, dp, dp, ip, ip]
    L.icpgpu_sac_normals_stats.argtypes = [vp, ip]
    L.icpgpu_segment_moments.argtypes = [vp, C.c_int, C.c_size_t, C.POINTER(C.c_int64), ip, C.c_size_t, C.c_void_p]
    L.icpgpu_segment_stats.argtypes = [vp, ip]
    L.icpgpu_iss_keypoints.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, szp]
    L.icpgpu_iss_fetch.argtypes = [vp, C.c_size_t, ip, fp, ip, dp, dp, dp]
    L.icpgpu_iss_stats.argtypes = [vp, ip]
    L.icpgpu_boundary_estimation.argtypes = [vp, fp, fp, C.c_size_t, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_uint8), ip, ip, ip]
    L.icpgpu_iss_keypoints_border.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, fp, C.c_double, szp]
    L.icpgpu_iss_fetch_border.argtypes = [vp, ip, ip]
    L.icpgpu_moving_least_squares.argtypes = [vp, fp, C.c_size_t, C.c_double, C.c_int, C.c_double, fp, fp, ip, szp]
    L.icpgpu_mls_fetch.argtypes = [vp, C.c_size_t, ip, ip, dp, dp]
    L.icpgpu_mls_stats.argtypes = [vp, ip]
    L.icpgpu_sac_extract.argtypes = [vp, C.c_int, fp, szp]
    L.icpgpu_sac_extract_view.argtypes = [vp, C.c_int, C.POINTER(fp), szp]
    L.icpgpu_morphological_operator.argtypes = [vp, C.c_double, C.c_int, fp]
    L.icpgpu_progressive_morphological_filter.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, szp, ip]
    L.icpgpu_pmf_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, ip, fp, fp, ip, ip]
    L.icpgpu_pmf_stats.argtypes = [vp, ip, C.POINTER(C.c_uint64)]
    L.icpgpu_pmf_extract.argtypes = [vp, C.c_int, fp, szp]
    L.icpgpu_pmf_extract_view.argtypes = [vp, C.c_int, C.POINTER(fp), szp]
    L.icpgpu_scp_align.argtypes = [vp, fp, C.c_size_t, fp, fp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, fp, szp, fp, ip, fp]
    L.icpgpu_scp_fetch.argtypes = [vp, C.c_size_t, C.c_size_t, ip, ip, ip, fp, ip, dp, fp, ip, ip]
    L.icpgpu_scp_stats.argtypes = [vp, ip, ip, dp]
    L.icpgpu_pass_through.argtypes = [vp, fp, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_int, fp, szp]
    L.icpgpu_pass_through_view.argtypes = [vp, fp, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(fp), szp]
    L.icpgpu_crop_box.argtypes = [vp, fp, C.c_size_t, fp, fp, fp, C.c_int, fp, szp]
    L.icpgpu_crop_box_view.argtypes = [vp, fp, C.c_size_t, fp, fp, fp, C.c_int, C.POINTER(fp), szp]
    L.icpgpu_crop_box_matrix.argtypes = [fp, fp, fp, fp]
    L.icpgpu_uniform_sampling.argtypes = [vp, fp, C.c_size_t, C.c_float, fp, szp]
    L.icpgpu_uniform_sampling_view.argtypes = [vp, fp, C.c_size_t, C.c_float, C.POINTER(fp), szp]
    L.icpgpu_farthest_point_sampling.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_int64, fp, szp]
    L.icpgpu_farthest_point_sampling_view.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_int64, C.POINTER(fp), szp]
    L.icpgpu_subset_fetch.argtypes = [vp, C.c_size_t, ip, fp, szp, szp]
    L.icpgpu_subset_removed.argtypes = [vp, C.c_size_t, ip, szp]
    L.icpgpu_subset_stats.argtypes = [vp, ip, ip, ip, ip]
    pp, lp = C.POINTER(Pose), C.POINTER(C.c_long)
    L.icpgpu_pose_from_matrix.argtypes = [fp, pp]
    L.icpgpu_pose_to_matrix.argtypes = [pp, fp]
    L.icpgpu_pose_compose.argtypes = [pp, pp, pp]
    L.icpgpu_pose_inverse.argtypes = [pp, pp]
    L.icpgpu_posegraph_create.argtypes = [C.POINTER(vp), C.c_double, dp]
    L.icpgpu_posegraph_destroy.argtypes = [vp]
    L.icpgpu_posegraph_set_initial_pose.argtypes = [vp, pp]
    L.icpgpu_posegraph_push.argtypes = [vp, fp, C.c_int, lp]
    L.icpgpu_posegraph_num_poses.argtypes = [vp]
    L.icpgpu_posegraph_num_keyframes.argtypes = [vp]
    L.icpgpu_posegraph_get_pose.argtypes = [vp, C.c_long, pp]
    L.icpgpu_posegraph_get_keyframe.argtypes = [vp, C.c_long, pp, lp]
    L.icpgpu_posegraph_get_edge.argtypes = [vp, C.c_long, pp]
    L.icpgpu_posegraph_write_g2o.argtypes = [vp, C.c_char_p]
    sp = C.POINTER(C.c_size_t)
    L.icpgpu_map_set_search.argtypes = [vp, C.c_int]
    L.icpgpu_map_reset.argtypes = [vp, C.c_double]
    L.icpgpu_map_add_points.argtypes = [vp, fp, C.c_size_t, fp, sp]
    L.icpgpu_map_add_source.argtypes = [vp, fp, sp]
    L.icpgpu_map_size.argtypes = [vp, sp]
    L.icpgpu_map_get_points.argtypes = [vp, fp, C.c_size_t, sp]
    L.icpgpu_map_nn_target.argtypes = [vp, fp, fp, fp, sp]
    L.icpgpu_profile_reset.argtypes = [vp]
    L.icpgpu_profile_get.argtypes = [vp, C.POINTER(Profile)]
    L.icpgpu_profile_set_sampling.argtypes = [vp, C.c_int]
    L.icpgpu_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.icpgpu_synchronize.argtypes = [vp]
    L.icpgpu_count_candidates.argtypes = [vp, C.c_int]
    L.icpgpu_count_candidates_read.argtypes = [vp, C.POINTER(C.c_uint64)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name in ("icpgpu_posegraph_num_poses", "icpgpu_posegraph_num_keyframes"):
            fn.restype = C.c_long
        elif name not in ("icpgpu_last_error", "icpgpu_default_params_sz", "icpgpu_struct_sizes", "icpgpu_fingerprint", "icpgpu_multi_last_error"):
            fn.restype = C.c_int
    # The three names icpgpu.h defines as MACROS over the sized entry points (include/icpgpu.h, "ABI rule"): the same spelling here,
    # with THESE mirrors' sizes -- a library whose structs have grown copies only what the mirrors hold.
    sizes = (C.sizeof(Params), C.sizeof(Result), C.sizeof(Profile))
    L.icpgpu_create = lambda out, device: L.icpgpu_create_abi(out, device, HEADER_VERSION, *sizes)
    L.icpgpu_default_params = lambda p: L.icpgpu_default_params_sz(p, sizes[0])
    L.icpgpu_align_batch_multi = lambda *a: L.icpgpu_align_batch_multi_sz(*a, sizes[0], sizes[1])
    _lib = L
    return L
