/*
 * icpgpu.h -- C-ABI of libicpgpu.so: MI355X (gfx950) ICP scan-matching core.
 *
 * Drop-in boundary for the one data-parallel hot path of YoshuaNava/icpslam: the per-scan
 * registration the reference delegates to a PCL `Registration` object at
 *   /root/reference/src/icpslam/icp_odometer.cpp:188-201   (IcpOdometer::laserCloudCallback)
 *   /root/reference/src/icpslam/octree_mapper.cpp:104-117  (OctreeMapper::estimateTransformICP)
 * The reference has no FFI/plugin registry; the interface it binds is the 10-call PCL protocol
 *   ctor -> setMaximumIterations -> setTransformationEpsilon -> setMaxCorrespondenceDistance ->
 *   setRANSACIterations(0) -> setInputSource -> setInputTarget -> align(out) ->
 *   getFinalTransformation -> hasConverged -> getFitnessScore.
 * Each entry point below names the protocol call (reference file:line) it replaces.  A header-only
 * C++ shim with exactly those method names lives in include/icpgpu_registration.hpp; the
 * reference-side edit is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; every function returns an int status
 *     (0 = ICPGPU_OK, < 0 = error) and never throws or aborts.  Non-convergence is NOT an error:
 *     it is reported as result.converged == 0, like PCL's hasConverged().
 *   - clouds are `pcl::PointXYZ` arrays: 16-byte stride float {x, y, z, pad}; pad is ignored on
 *     input and written as 1.0f on output.
 *   - transforms are float[16] column-major 4x4 (memory layout of Eigen::Matrix4f), mapping
 *     source -> target, i.e. the T the reference chains at icp_odometer.cpp:112-113.
 *   - one context = one device + one HIP stream + scratch; distinct contexts may be used from
 *     different threads concurrently (the odometer callback thread and the mapper main-loop
 *     thread, /root/reference/src/icpslam_node.cpp:9); a single context is not re-entrant.
 *   - there is no CPU fallback: without a usable gfx950 device icpgpu_create() fails.
 */
#ifndef ICPGPU_H
#define ICPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPGPU_VERSION_MAJOR 1
#define ICPGPU_VERSION_MINOR 2
#define ICPGPU_HEADER_VERSION (ICPGPU_VERSION_MAJOR * 1000 + ICPGPU_VERSION_MINOR)
/* ABI rule (1.0).  icpgpu_params, icpgpu_result and icpgpu_profile only ever GROW AT THE END, and the library never assumes the
 * caller's structs are as long as its own: the caller's sizeof of the three travels with icpgpu_create (the macro below hands them
 * to icpgpu_create_abi) and every entry point that reads or writes one of them through that context copies min(caller's, library's)
 * bytes -- fields the caller does not know are not written, fields the library does not know read as zero.  The two entry points
 * without a context take the sizes themselves (icpgpu_default_params_sz, icpgpu_align_batch_multi_sz; macros below).
 * icpgpu_create_abi refuses a header of another MAJOR version (ICPGPU_ERR_UNSUPPORTED).  Until 0.4 the structs grew in place with
 * nothing but a comment to protect an older caller; the unsized symbols of those versions (icpgpu_create, icpgpu_default_params,
 * icpgpu_align_batch_multi) are NOT exported any more, so a binary built against a 0.x header fails at load time instead of
 * overrunning its structs.  History: 1.2 ICPGPU_P2PLANE, icpgpu_set_target_normals, icpgpu_normals, icpgpu_reduce_point_to_plane,
 * icpgpu_solve_point_to_plane; added under 1.2: ICPGPU_NDT, icpgpu_set_ndt_params, icpgpu_get_ndt_params,
 * icpgpu_ndt_transformation_probability, icpgpu_ndt_cells, icpgpu_ndt_derivatives, icpgpu_ndt_step, icpgpu_set_ndt_line_search,
 * icpgpu_get_ndt_line_search, icpgpu_ndt_gradient, icpgpu_ndt_line_search_replay, icpgpu_ndt_line_search_trace (no struct changed); also added under
 * 1.2: the correspondence rejectors -- icpgpu_rejector, icpgpu_set_correspondence_rejectors, icpgpu_get_correspondence_rejectors,
 * icpgpu_correspondences, icpgpu_rejector_stats, and reciprocal correspondences -- icpgpu_set_reciprocal_correspondences,
 * icpgpu_get_reciprocal_correspondences, icpgpu_reciprocal_stats, and the outlier filters -- icpgpu_statistical_outlier_removal,
 * icpgpu_radius_outlier_removal, their _view forms, icpgpu_outlier_stats, icpgpu_outlier_fetch, and the neighbour search --
 * icpgpu_search_set_input, icpgpu_search_size, icpgpu_search_knn, icpgpu_search_radius, and normal estimation --
 * icpgpu_normal_estimation, and euclidean clustering -- icpgpu_euclidean_cluster_extraction, icpgpu_cluster_fetch, and region growing -- icpgpu_region_growing, icpgpu_region_fetch, and segment moments -- icpgpu_segment_moments, icpgpu_segment_stats, and plane segmentation --
 * icpgpu_sac_plane_segmentation, icpgpu_sac_fetch, icpgpu_sac_stats, icpgpu_sac_extract, icpgpu_sac_extract_view, and segmentation from normals --
 * icpgpu_sac_segmentation_from_normals, icpgpu_sac_normals_fetch, icpgpu_sac_normals_stats, and the ground filter -- icpgpu_morphological_operator,
 * icpgpu_progressive_morphological_filter, icpgpu_pmf_fetch, icpgpu_pmf_stats, icpgpu_pmf_extract, icpgpu_pmf_extract_view, and ISS keypoints --
 * icpgpu_iss_keypoints, icpgpu_iss_fetch, icpgpu_iss_stats, icpgpu_iss_keypoints_border, icpgpu_iss_fetch_border, and boundary
 * estimation -- icpgpu_boundary_estimation, and moving least squares -- icpgpu_moving_least_squares, icpgpu_mls_fetch, icpgpu_mls_stats, and fast point feature histograms -- icpgpu_fpfh_estimation, and the symmetric point-to-plane objective with the surface-normal rejector -- icpgpu_set_source_normals,
 * icpgpu_set_p2plane_symmetric, icpgpu_get_p2plane_symmetric, icpgpu_reduce_symmetric_point_to_plane,
 * icpgpu_solve_symmetric_point_to_plane, ICPGPU_REJECT_SURFACE_NORMAL, and the sample-consensus rejector -- ICPGPU_REJECT_SAMPLE_CONSENSUS,
 * icpgpu_set_rejector_sac_seed, icpgpu_get_rejector_sac_seed, icpgpu_correspondence_rejector_sample_consensus, icpgpu_rejector_sac_fetch,
 * and the cropping and sampling filters -- icpgpu_pass_through, icpgpu_crop_box, icpgpu_crop_box_matrix, icpgpu_uniform_sampling,
 * icpgpu_farthest_point_sampling, their _view forms, icpgpu_subset_fetch, icpgpu_subset_removed, icpgpu_subset_stats,
 * and the diagnostic icpgpu_sweep_sums (no struct changed); 1.1 icpgpu_align_view, icpgpu_voxel_grid_view (result clouds as views of the pinned staging
 * buffer), icpgpu_profile.voxel_views_direct; 1.0 icpgpu_result.gicp_solver, icpgpu_calibrate, sized entry points; 0.4 icpgpu_params.gicp_inner,
 * icpgpu_profile.gicp_quadratic_solves; 0.3 icpgpu_profile (sources_adopted, gicp_host_solves, gicp_solver_choice). */

/* ---- environment ---------------------------------------------------------------------------------
 * Production switches, read by every build of libicpgpu.so (none of them changes a result, except ICPGPU_GICP_INNER):
 *   ICPGPU_WAIT_TIMEOUT_MS        deadline of every host wait for the device (mailbox, gather); default 30000
 *   ICPGPU_BATCH_THREADS          host threads of icpgpu_align_batch (default: chosen from the CPUs this process may use)
 *   ICPGPU_BATCH_DEPTH            pairs per lock-step group (point-to-point; default 8) / alignments a thread keeps in flight
 *   ICPGPU_BATCH_GROUPS           lock-step groups in flight on the GPU, over all host threads together (default 8)
 *   ICPGPU_RECOGNISE=0            icpgpu_set_target / icpgpu_set_source always upload (no content recognition)
 *   ICPGPU_GICP_SERVER=0          every GICP cost evaluation is its own kernel launch (no resident evaluation server)
 *   ICPGPU_GICP_DEVICE=0|1|auto   GICP's inner BFGS on the host over the evaluation server (0), or in the resident device solver (1);
 *                                 auto (the default) = the host loop for single alignments, the device solver for the runs of a
 *                                 batch -- a fixed rule since 1.0 (until 0.4 a context timed both over its first alignments);
 *                                 icpgpu_calibrate measures on request.  Same bits either way; the solver an alignment ran on is
 *                                 in icpgpu_result.gicp_solver, the context's setting in icpgpu_profile.gicp_solver_choice
 *   ICPGPU_GICP_INNER=exact|quadratic  overrides icpgpu_params.gicp_inner (see icpgpu_gicp_inner below: QUADRATIC moves a GICP
 *                                 result within the stated tolerance, not bit for bit)
 *   ICPGPU_MAILBOX=pairs|release  how results reach the host (default: a self-test at context creation picks it)
 *   ICPGPU_DEBUG=1                diagnostics on stderr
 *   LOCAL_WORLD_SIZE              (torch.distributed.run) processes sharing this host's CPUs
 * Development switches (kernel variants, tuning constants, test modes) exist only in libicpgpu_dev.so: icpslam_amd/csrc/icp_env.h. */

typedef struct icpgpu_ctx icpgpu_ctx; /* opaque */

typedef enum {
  ICPGPU_OK = 0,
  ICPGPU_ERR_INVALID_ARG = -1,
  ICPGPU_ERR_NO_DEVICE = -2,   /* no HIP device / not gfx950 / runtime missing */
  ICPGPU_ERR_HIP = -3,         /* a HIP call failed; see icpgpu_last_error() */
  ICPGPU_ERR_OOM = -4,
  ICPGPU_ERR_NO_INPUT = -5,    /* align/fitness before set_source/set_target */
  ICPGPU_ERR_UNSUPPORTED = -6
} icpgpu_status;

/* Solver. The reference instantiates pcl::GeneralizedIterativeClosestPoint (icp_odometer.cpp:188,
 * octree_mapper.cpp:104); BASELINE.json's north_star specifies point-to-point ICP
 * (pcl::IterativeClosestPoint semantics), which is the primary mode.
 * ICPGPU_P2PLANE (1.2) is pcl::IterativeClosestPointWithNormals with TransformationEstimationPointToPlaneLLS -- the "ICP that uses
 * the surface" the reference wonders about at icp_odometer.cpp:187: the point-to-point loop (correspondences, rejection, convergence
 * criteria, result fields) with the linearised point-to-plane solve in place of Umeyama.  The target's normals are the caller's
 * (icpgpu_set_target_normals: PCL's semantics exactly, for PointNormal clouds -- icpgpu_normal_estimation below computes them as
 * pcl::NormalEstimation does, with k or a radius, a viewpoint and the curvature) or ESTIMATED on the device: NOT
 * pcl::NormalEstimation's eigen33 solve but GICP's plane -- the 20 nearest neighbours and the raw covariance computeCovariances
 * forms, the same Eigen JacobiSVD restatement, the third left singular vector (the one computeCovariances scales by epsilon), rounded
 * to float and turned towards the viewpoint (0, 0, 0) as flipNormalTowardsViewpoint does; points that get GICP's identity marker
 * (non-finite, or every point of a cloud with fewer than 20 finite points) get a NaN normal, and a pair whose target normal is not
 * finite is a correspondence that adds nothing to the solve (PCL's skip).  A singular system (a zero pivot or a non-finite
 * solution: one plane and nothing else) -- undefined in PCL -- ends the alignment with converged = 0, ICPGPU_NOT_CONVERGED and
 * the last finite transform.  Single alignments only: icpgpu_align_batch* return ICPGPU_ERR_UNSUPPORTED.  Parity against PCL
 * binaries is unpinned, like every other mode's. */
/* ICPGPU_NDT (added under 1.2) is pcl::NormalDistributionsTransform over pcl::VoxelGridCovariance (PCL 1.8): the target's points are
 * binned into cells of the voxel filter's keys at leaf = resolution; every cell of >= 6 points gets a Gaussian (mean, PCL's
 * covariance with its smallest eigenvalues raised to 0.01 x the largest, inverse); a Newton loop over p = (tx, ty, tz, roll, pitch,
 * yaw) maximises the sum over source points and cells within `resolution` of the transformed point of the Gauss-fitted score.
 * Parameters: icpgpu_set_ndt_params (resolution 1.0, step_size 0.1, outlier_ratio 0.55 by default) and icpgpu_params'
 * max_iterations and transformation_epsilon (PCL's NDT sets 35 and 0.1; the C++ shim does the same); min_correspondences and
 * max_correspondence_distance are not used (fitness keeps its own range).  Result: T = the float transform of the final p,
 * iterations = getFinalNumIteration(), converged = 1 as PCL's, except 0 when the Newton step is NaN (T is then the last finite
 * transform, state ICPGPU_NOT_CONVERGED); state ICPGPU_CONV_ITERATIONS on the iteration cap, ICPGPU_CONV_TRANSFORM on a step below
 * epsilon or a zero step, ICPGPU_CONV_NO_CORRESPONDENCES (T = the guess) when no (point, cell) pair contributes at the guess;
 * n_correspondences = the pairs of the last evaluation; mse_last = NaN.  Two deliberate deviations from PCL 1.8: cells with a
 * negative or zero eigenvalue or a non-finite inverse are dropped (PCL keeps them searchable), and a target whose cell index
 * would overflow int32 at this resolution is refused with ICPGPU_ERR_INVALID_ARG (PCL passes through).  DESIGN.md states the
 * contract rule by rule.  Single alignments only: icpgpu_align_batch* return ICPGPU_ERR_UNSUPPORTED. */
typedef enum { ICPGPU_P2P_SVD = 0, ICPGPU_GICP = 1, ICPGPU_P2PLANE = 2, ICPGPU_NDT = 3 } icpgpu_method;

/* GICP's inner minimisation (PCL: estimateRigidTransformationBFGS, ~35 cost evaluations per outer iteration).
 *   EXACT      every evaluation is a pass over the correspondences with PCL's arithmetic (points transformed in float32); the
 *              registration is bit-identical to the CPU restatement the tests compare with.  The default.
 *   QUADRATIC  the correspondences are reduced ONCE per outer iteration to the 73 coefficients of the quadratic form the cost is
 *              when the transformed points are taken as real numbers; BFGS -- the same solver -- then runs on the host without a
 *              device round trip (2-3x the scans/s of the reference's pipeline).  The result differs from EXACT's by what PCL's
 *              float32 rounding of the transformed points contributes: within 1e-4 / 1e-3 m on most pairs, about as far from
 *              PCL's evaluation as that evaluation moves when its own sums are re-ordered (profiles/r05_gicp_quadratic.txt).
 * ICPGPU_GICP_INNER=exact|quadratic in the environment overrides the parameter (an unchanged binary can opt in). */
typedef enum { ICPGPU_GICP_INNER_EXACT = 0, ICPGPU_GICP_INNER_QUADRATIC = 1 } icpgpu_gicp_inner;

/* Correspondence search strategy; every mode returns the exact nearest neighbour. */
typedef enum {
  ICPGPU_NN_AUTO = 0,
  ICPGPU_NN_BRUTE = 1, /* LDS-tiled brute force (north_star) */
  ICPGPU_NN_GRID = 2   /* uniform-grid accelerated exact search */
} icpgpu_nn_mode;

/* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
typedef enum {
  ICPGPU_NOT_CONVERGED = 0,
  ICPGPU_CONV_ITERATIONS = 1,
  ICPGPU_CONV_TRANSFORM = 2,
  ICPGPU_CONV_ABS_MSE = 3,
  ICPGPU_CONV_REL_MSE = 4,
  ICPGPU_CONV_NO_CORRESPONDENCES = 5
} icpgpu_convergence_state;

typedef struct {
  int32_t method;                     /* icpgpu_method */
  int32_t max_iterations;             /* setMaximumIterations: icp_odometer.cpp:189 (10), octree_mapper.cpp:105 (30) */
  double transformation_epsilon;      /* setTransformationEpsilon: icp_odometer.cpp:190 (1e-6) */
  double max_correspondence_distance; /* setMaxCorrespondenceDistance: icp_odometer.cpp:191 (1.0 m) */
  double euclidean_fitness_epsilon;   /* PCL default -DBL_MAX: relative-MSE test off (never set by the reference) */
  int32_t min_correspondences;        /* PCL default 3 (P2P) / 4 (GICP) */
  int32_t force_iterations;           /* != 0: run exactly max_iterations (benchmarking; no PCL equivalent) */
  int32_t nn_mode;                    /* icpgpu_nn_mode */
  int32_t brute_variant;              /* brute-force search: 0 = matrix-core kernel for large clouds (default: lower bound on the bf16
                                       * matrix path), 1 = plain-VALU kernel always, 2 = the bound in f32 MFMAs; identical results */
  int32_t gicp_inner;                 /* icpgpu_gicp_inner (GICP only); 0 = EXACT */
} icpgpu_params;

typedef struct {
  float T[16];                /* getFinalTransformation(): icp_odometer.cpp:199, octree_mapper.cpp:115 */
  int32_t converged;          /* hasConverged(): icp_odometer.cpp:201, octree_mapper.cpp:117 */
  int32_t iterations;
  int32_t convergence_state;  /* icpgpu_convergence_state */
  uint32_t n_correspondences; /* accepted pairs in the last iteration */
  double mse_last;            /* mean squared correspondence distance of the last iteration (m^2) */
  double fitness;             /* getFitnessScore(): icp_odometer.cpp:201; NaN unless requested */
  double t_total_ms;          /* host wall time of the align call */
  double t_device_ms;         /* kernel time of the call on the context's stream: HIP-event time of the TIMED sweeps
                               * (icpgpu_profile_set_sampling), scaled to all sweeps of the call.  An estimate: timings are
                               * read without blocking, and one that was not ready at the end of the call counts towards
                               * the next one; 0 when none of the call's sweeps was a timed one (icpgpu_profile_get always waits and is exact) */
  int32_t gicp_solver;        /* GICP: where the inner BFGS of this alignment's LAST outer iteration ran -- icpgpu_gicp_solver;
                               * 0 for point-to-point alignments and alignments that never reached a minimisation -- 1.0 */
  int32_t reserved0;
} icpgpu_result;
typedef enum {
  ICPGPU_GICP_SOLVER_NONE = 0,
  ICPGPU_GICP_SOLVER_HOST = 1,      /* BFGS on the host, every evaluation a round trip to the resident evaluation server */
  ICPGPU_GICP_SOLVER_DEVICE = 2,    /* the whole BFGS inside gicp_solve_kernel */
  ICPGPU_GICP_SOLVER_QUADRATIC = 3  /* gicp_inner = QUADRATIC: one device pass, BFGS on the host on the quadratic form */
} icpgpu_gicp_solver;

/* Kernel-level accounting since the last icpgpu_profile_reset(); times are HIP-event times on the
 * context's own stream (this is what bench.py's roofline object is computed from). */
typedef struct {
  uint64_t nn_launches;       /* brute-force correspondence-search launches (a2) */
  double nn_ms;               /* summed duration of the TIMED ones (nn_timed of them, see icpgpu_profile_set_sampling) */
  uint64_t nn_pairs;          /* point pairs evaluated by those launches */
  uint64_t nn_bytes;          /* algorithmic bytes: 16*(N_s+N_t) + 8*N_s per launch */
  uint64_t reduce_launches;   /* rejection + covariance reduction launches (a3+a4) */
  double reduce_ms;
  uint64_t reduce_bytes;
  uint64_t transform_launches; /* a6 */
  double transform_ms;
  uint64_t transform_bytes;
  uint64_t iterations;        /* ICP iterations executed */
  uint64_t aligns;            /* align calls */
  uint64_t grid_launches;     /* grid-accelerated correspondence launches (a2, with a3+a4 fused inside ICP iterations) */
  double grid_ms;
  uint64_t grid_bytes;        /* algorithmic bytes: 16*(N_s+N_t) + output per launch */
  uint64_t grid_builds;       /* target grid (re)builds: bbox + counting sort */
  double grid_build_ms;       /* host time inside the builds (two host round trips each; the last kernels overlap the caller) */
  uint64_t grid_fallback_points; /* points finished by the brute-force kernel (no neighbour within the cutoff) */
  uint64_t voxel_launches;    /* voxel-grid filter runs */
  double voxel_ms;            /* key + sort + flag/scan + centroid kernels */
  uint64_t voxel_bytes;       /* algorithmic bytes: 16*N in + 16*N_out */
  uint64_t gicp_cov_launches; /* GICP: per-cloud 20-NN covariance passes (and P2PLANE's normal estimates: the same kernels) */
  double gicp_cov_ms;
  uint64_t gicp_cost_launches; /* GICP: BFGS function/gradient evaluations (one device reduction each; with gicp_inner = QUADRATIC they
                               * run on the host, and gicp_eval_ms then holds the passes' and the minimisations' wall time) */
  uint64_t map_inserts;       /* f4: addPointsToMap batches */
  double map_insert_ms;
  uint64_t map_points_in;     /* points offered to the map */
  uint64_t map_nn_launches;   /* f4: nn-cloud builds */
  double map_nn_ms;
  uint64_t nn_timed;          /* launches behind nn_ms / grid_ms / reduce_ms: kernel timing is sampled, because the three */
  uint64_t grid_timed;        /*   event records around a sweep are barrier packets that cost 6-7 us per iteration */
  uint64_t reduce_timed;
  uint64_t grid_bounded;      /* grid sweeps whose searches were pruned by the neighbours the previous sweep found */
  double gicp_eval_ms;        /* GICP: host wall time of the BFGS cost evaluations, command written -> 13 sums merged (the
                               * evaluations are dependent host <-> device round trips; this is what a registration waits for) */
  uint64_t gicp_eval_corr;    /* correspondences those evaluations reduced over, summed (88 algorithmic bytes each) */
  uint64_t gicp_cov_points;   /* points whose covariances the gicp_cov passes computed (16 B read + 48 B written each, + the 20-NN search) */
  uint64_t targets_recognised; /* icpgpu_set_target calls that found the cloud already in HBM (no upload, no rebuild) */
  uint64_t brute_bound_violations; /* test mode ICPGPU_MFMA_CHECK_BOUND=1 of the bf16 matrix-core search: pairs whose lower bound */
  double brute_bound_worst;        /*   exceeded what their own exact distance allows (must stay 0); worst excess / (P^2 + |v|^2) seen */
  uint64_t gicp_device_solves;     /* GICP outer iterations whose whole inner BFGS ran on the device (gicp_solve_kernel) */
  uint64_t grid_adopted;           /* GICP: targets whose correspondence search took over the grid their covariances were computed
                                    * over instead of building a second one (same keys: the search is exact whatever the cells) */
  uint64_t sources_adopted;        /* icpgpu_set_source calls that found the buffer to be the context's last voxel-filter result,
                                    * still in HBM (no upload, no bounding-box pass) -- version 0.3 */
  uint64_t gicp_host_solves;       /* GICP outer iterations whose inner BFGS ran on the host (over the evaluation server) -- 0.3 */
  uint64_t gicp_solver_choice;     /* the solver single GICP alignments of this context run on: 1 = host loop, 2 = device solver; never 0
                                    * since 1.0 (set at icpgpu_create from ICPGPU_GICP_DEVICE, changed only by icpgpu_calibrate) -- 0.3 */
  uint64_t gicp_quadratic_solves;  /* GICP outer iterations solved on the quadratic form (icpgpu_params.gicp_inner = QUADRATIC) -- 0.4 */
  uint64_t cov_grids_unchecked;    /* GICP: covariance grids built without waiting for their occupancy statistics (a containing box from
                                    * the voxel filter + the last cloud's cell size; the statistics are checked at the alignment's first
                                    * wait) -- 1.0 */
  uint64_t cov_grids_rebuilt;      /* ... of which the check failed: rebuilt the waiting way, the alignment started over -- 1.0 */
  uint64_t voxel_views_direct;     /* icpgpu_voxel_grid_view calls whose points reached the host in front of the cell count (the others
                                    * went through the copy engine: sort path, pass-through, a result beyond the staging buffer) -- 1.1 */
} icpgpu_profile;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* replaces: construction of the stack `icp` object, icp_odometer.cpp:188 / octree_mapper.cpp:104.
 * Unlike the reference (fresh object per scan) a context is meant to be created once and reused. */
int icpgpu_create_abi(icpgpu_ctx** out_ctx, int device_id, int header_version, size_t sizeof_params, size_t sizeof_result,
                      size_t sizeof_profile);
#define icpgpu_create(out_ctx, device_id) \
  icpgpu_create_abi((out_ctx), (device_id), ICPGPU_HEADER_VERSION, sizeof(icpgpu_params), sizeof(icpgpu_result), sizeof(icpgpu_profile))
int icpgpu_destroy(icpgpu_ctx* ctx);
const char* icpgpu_last_error(const icpgpu_ctx* ctx); /* ctx may be NULL: last create() error */
int icpgpu_version(void);                             /* major*1000 + minor */

/* ---- parameters (icp_odometer.cpp:189-192, octree_mapper.cpp:105-108) ----------------------- */
void icpgpu_default_params_sz(icpgpu_params* p, size_t sizeof_params); /* PCL defaults + the reference's odometer constants */
#define icpgpu_default_params(p) icpgpu_default_params_sz((p), sizeof(icpgpu_params))
/* what THIS library's structs measure: {sizeof(icpgpu_params), sizeof(icpgpu_result), sizeof(icpgpu_profile)} (bindings that
 * mirror the structs by hand -- ctypes, JNA -- check themselves against it) */
void icpgpu_struct_sizes(size_t out3[3]);
int icpgpu_set_params(icpgpu_ctx* ctx, const icpgpu_params* p);
int icpgpu_get_params(const icpgpu_ctx* ctx, icpgpu_params* p);

/* ---- inputs --------------------------------------------------------------------------------- */
/* replaces setInputSource (icp_odometer.cpp:193, octree_mapper.cpp:109): copies n points H2D;
 * the caller keeps ownership. n may be 0. */
int icpgpu_set_source(icpgpu_ctx* ctx, const float* xyzw, size_t n);
/* replaces setInputTarget (icp_odometer.cpp:194, octree_mapper.cpp:110). PCL rejects an empty
 * target; here n == 0 is accepted and align() then reports converged = 0 with T = identity. */
int icpgpu_set_target(icpgpu_ctx* ctx, const float* xyzw, size_t n);
/* The reference hands scan k-1's SOURCE cloud back as scan k's TARGET (`*prev_cloud_ = *curr_cloud_`,
 * icp_odometer.cpp:209, then setInputTarget(prev_cloud_) at :194): icpgpu_set_target recognises a buffer
 * whose content (size, then a 64-bit content fingerprint) is the context's current source or target and
 * keeps what it has in HBM -- the cloud, its search grid, its GICP covariances -- instead of uploading
 * and rebuilding (the promote path for the source; nothing at all for the unchanged target of a rejected
 * scan); the source stays set (as a device-side copy) either way.  Call set_target BEFORE set_source when both change
 * (after set_source the previous source is gone and there is nothing to recognise).  icpgpu_fingerprint is that fingerprint of
 * a host buffer (n points of 16 bytes); icpgpu_cloud_sizes reports what a context holds (the C++ shim's
 * context pool picks the context whose source has the new target's size).
 * ASSUMPTION: recognition compares sizes and the 64-bit fingerprint (an additive, non-cryptographic mix of every point's bits
 * and index), not the bytes: two different clouds of equal size collide with probability ~2^-64 per comparison, and an
 * adversarial cloud could be constructed.  ICPGPU_RECOGNISE=0 in the environment makes icpgpu_set_target always upload.
 * icpgpu_set_source recognises in the same way (and under the same switch) the result of the context's last icpgpu_voxel_grid
 * when the caller hands it back: see icpgpu_voxel_grid below. */
unsigned long long icpgpu_fingerprint(const float* xyzw, size_t n);
int icpgpu_cloud_sizes(const icpgpu_ctx* ctx, size_t* n_source, size_t* n_target);
/* same, for clouds already resident in this device's HBM (zero copy; must stay valid and
 * unmodified until replaced; 16-byte aligned). */
int icpgpu_set_source_device(icpgpu_ctx* ctx, const void* d_xyzw, size_t n);
int icpgpu_set_target_device(icpgpu_ctx* ctx, const void* d_xyzw, size_t n);
/* make the current source the next target without a copy (the reference's
 * `*prev_cloud_ = *curr_cloud_`, icp_odometer.cpp:209). */
int icpgpu_promote_source_to_target(icpgpu_ctx* ctx);

/* ---- the hot path --------------------------------------------------------------------------- */
/* replaces align(out) + getFinalTransformation + hasConverged [+ getFitnessScore]
 * (icp_odometer.cpp:198-201, octree_mapper.cpp:114-117).
 *   guess     : float[16] initial transform or NULL (= identity; the reference never passes one)
 *   out_xyzw  : host buffer for the aligned source cloud (n_source * 16 bytes) or NULL to skip the
 *               D2H copy (the reference only publishes it for debugging, icp_odometer.cpp:216-218)
 *   want_fitness : != 0 also evaluates getFitnessScore() (one more NN sweep)                     */
int icpgpu_align(icpgpu_ctx* ctx, const float* guess, float* out_xyzw, int want_fitness, icpgpu_result* result);
/* the same, the aligned cloud handed out as a VIEW: *view_xyzw points at *n_out points in the context's pinned staging buffer
 * (written there by the transform kernel itself, in front of the fitness sweep), valid until the context's next call.  For a
 * caller that owns a container to fill -- align(output) resizes `output` (icp_odometer.cpp:196-198): `output.points.assign(view,
 * view + n)` is one pass where resize + copy are two.  1.1 */
int icpgpu_align_view(icpgpu_ctx* ctx, const float* guess, int want_fitness, icpgpu_result* result, const float** view_xyzw,
                      size_t* n_out);

/* replaces getFitnessScore(max_range) (icp_odometer.cpp:201) using the last align's transform. */
int icpgpu_fitness(icpgpu_ctx* ctx, double max_range, double* out_fitness);

/* Many independent scan pairs through one context (BASELINE config 4/5).  Pair k registers
 * src[k] (n_src[k] points) onto tgt[k]; all pointers are host pointers.  Iterations of different
 * pairs are interleaved on the device so the per-iteration host solve of one pair overlaps the
 * kernels of others.  results[k] is filled for every k. */
int icpgpu_align_batch(icpgpu_ctx* ctx, size_t n_pairs, const float* const* src, const size_t* n_src,
                       const float* const* tgt, const size_t* n_tgt, int want_fitness, icpgpu_result* results);

/* The same over the GPUs of one node, from ONE process (the reference is a single C++ process,
 * /root/reference/src/icpslam_node.cpp:3-14): entry r of `devices` gets the contiguous shard r of the pairs (sizes differ by
 * at most one) and its own host thread driving icpgpu_align_batch on a context the library keeps for that entry; no data
 * is exchanged during the solve.  results[k] is filled for every k.  With a communicator the result records -- 23 float64 =
 * 184 B per pair: pair id, iterations, converged, state, n_corr, mse, fitness, T[16] row-major -- are then all-gathered
 * across the devices (each shard padded to the largest) and the checked copy of entry 0 is returned in `records`
 * (n_pairs x 23 doubles):
 *   ICPGPU_COMM_NONE  no gather (records may be NULL)
 *   ICPGPU_COMM_RCCL  ncclCommInitAll over `devices` + one ncclAllGather (librccl is loaded on first use, not linked)
 *   ICPGPU_COMM_HOST  the same buffers, exchanged through host memory (tests on one GPU: a device may be named twice)
 * params NULL keeps the contexts' parameters.  Errors: status code + icpgpu_multi_last_error() (per calling thread). */
enum { ICPGPU_COMM_NONE = 0, ICPGPU_COMM_RCCL = 1, ICPGPU_COMM_HOST = 2 };
int icpgpu_align_batch_multi_sz(const int* devices, int n_devices, const icpgpu_params* params, size_t n_pairs,
                                const float* const* src, const size_t* n_src, const float* const* tgt, const size_t* n_tgt,
                                int want_fitness, icpgpu_result* results, double* records, int communicator, size_t sizeof_params,
                                size_t sizeof_result);
#define icpgpu_align_batch_multi(devices, n_devices, params, n_pairs, src, n_src, tgt, n_tgt, want_fitness, results, records, comm) \
  icpgpu_align_batch_multi_sz((devices), (n_devices), (params), (n_pairs), (src), (n_src), (tgt), (n_tgt), (want_fitness), (results), \
                              (records), (comm), sizeof(icpgpu_params), sizeof(icpgpu_result))
const char* icpgpu_multi_last_error(void);

/* ---- kernel-level entry points (used by the parity tests; same kernels as align) ------------- */
/* a2: idx[i], d2[i] = exact nearest neighbour of T*source[i] in target (lowest index on ties);
 * idx = -1, d2 = +inf when the target is empty or the point is non-finite. */
int icpgpu_nn(icpgpu_ctx* ctx, const float* T, int32_t* idx, float* d2);
/* a3+a4: over pairs of the last icpgpu_nn/align NN sweep with (double)d2 <= max_dist^2:
 * sums = {n, sum p(3), sum q(3), sum q p^T (9, row = q), sum d2}, p = T*source[i], q = target[idx[i]]. */
int icpgpu_reduce(icpgpu_ctx* ctx, const float* T, double max_dist, double sums[17]);
/* One sweep of a P2P_SVD alignment at T, by the alignment's own path: the alignment's opening (the target's grid for the context's
 * max_correspondence_distance where nn_mode asks for one, the cell-ordered source from 100000 points on), then exactly what iteration
 * k of icpgpu_align launches for the gate (double)d2 <= max_dist^2 -- the grid search with the fused reduction, or the keys and
 * their reduction where no grid serves max_dist (brute force, a gate above the grid's), or the rejectors' keys step -- and the 17
 * sums it receives, in icpgpu_reduce's layout.  Calls on unchanged clouds are bounded by the previous sweep's neighbours as an
 * alignment's later iterations are; the sums never depend on it.  T NULL = identity.  An empty target: 17 zeros, no sweep.
 * ICPGPU_ERR_INVALID_ARG: sums NULL, max_dist not finite, another method.  icpgpu_profile shows which path ran (grid_launches,
 * nn_launches, grid_bounded).  Diagnostic entry (tests); it leaves the last alignment's transform and record alone.  Added under 1.2 */
int icpgpu_sweep_sums(icpgpu_ctx* ctx, const float* T, double max_dist, double sums[17]);
/* a5 (host): Umeyama without scaling from the 17 sums -> double[16] column-major. */
int icpgpu_solve(const double sums[17], double Tk[16]);
/* a6: out = T * source (w = 1), pcl::transformPointCloud (icp_odometer.cpp:205). */
int icpgpu_transform(icpgpu_ctx* ctx, const float* T, float* out_xyzw);

/* a11 (GICP mode): per-point regularised covariances U diag(1,1,1e-3) U^T of the 20 nearest neighbours
 * (pcl::GeneralizedIterativeClosestPoint::computeCovariances); out6 = n x {xx, xy, xz, yy, yz, zz}.
 * GICP needs at least 20 FINITE points per cloud: with fewer (PCL's kd-tree holds the finite points only, its nearestKSearch(20) then
 * comes back short) the cloud is too small -- ICPGPU_ERR_INVALID_ARG here, and icpgpu_align / icpgpu_align_batch end as for a cloud
 * of fewer than 20 points: not converged, T = I, 0 iterations. */
int icpgpu_gicp_covariances(icpgpu_ctx* ctx, int of_target, double* out6);
/* ---- point-to-plane mode (ICPGPU_P2PLANE, 1.2) ------------------------------------------------------ */
/* replaces setInputTarget's normals: pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal> reads them from the target
 * cloud's normal_x/y/z.  n float4 {nx, ny, nz, pad} (pad ignored), n == the target's size; copied, in force until the target changes
 * (icpgpu_set_target -- recognised or not --, icpgpu_set_target_device, icpgpu_promote_source_to_target, icpgpu_map_nn_target drop
 * them).  Without them P2PLANE estimates the target's normals at its first alignment after the target changed and keeps them while
 * the target is the same cloud (a target icpgpu_set_target recognises included). */
int icpgpu_set_target_normals(icpgpu_ctx* ctx, const float* nxyzw, size_t n);
/* the mirror for the source (added under 1.2): n float4 {nx, ny, nz, pad}, n == the source's size; copied.  They are read by the
 * symmetric objective and by the surface-normal rejector (below), never by plain P2PLANE.  No source set: ICPGPU_ERR_NO_INPUT; another
 * n or a null pointer: ICPGPU_ERR_INVALID_ARG.  The normals belong to the cloud they came with: every call that replaces the source
 * drops them (icpgpu_set_source -- adopted from the voxel filter or not --, icpgpu_set_source_device,
 * icpgpu_set_source_voxel_filtered).  icpgpu_promote_source_to_target MOVES them: they become the new target's supplied normals
 * (as if icpgpu_set_target_normals had been called), so the odometer's per-scan protocol computes a scan's normals once; without
 * supplied source normals promote drops the target's as before.  An icpgpu_set_target that recognises the source's content leaves
 * them with the source and hands the target none.  Where source normals are needed and none were supplied they are estimated as
 * P2PLANE estimates the target's (GICP's plane; >= 20 points, else ICPGPU_ERR_INVALID_ARG). */
int icpgpu_set_source_normals(icpgpu_ctx* ctx, const float* nxyzw, size_t n);
/* the normals P2PLANE uses for the target (of_target != 0: the caller's if set, else the estimate) or the source's (the caller's if set, else the estimate);
 * out_nxyzw = n float4 {nx, ny, nz, 0}, NaN for marker points (pcl::NormalEstimation's output slot; see ICPGPU_P2PLANE).
 * (pcl::NormalEstimation itself -- k or radius neighbourhoods, a viewpoint, curvature -- is icpgpu_normal_estimation.)
 * Estimating needs >= 20 points: ICPGPU_ERR_INVALID_ARG otherwise, as icpgpu_gicp_covariances. */
int icpgpu_normals(icpgpu_ctx* ctx, int of_target, float* out_nxyzw);
/* the counterpart of icpgpu_reduce: over pairs of the last icpgpu_nn sweep with (double)d2 <= max_dist^2, s = T * source[i] (float),
 * d = target[idx], n = its normal -- TransformationEstimationPointToPlaneLLS::estimateRigidTransformation's sums in float64:
 * sums = {n, sum d2, the 21 upper-triangle entries of A^T A over (a, b, c, nx, ny, nz) row by row, the 6 of A^T r} (DESIGN.md
 * section 3 fixes the float expressions of a, b, c, r).  Same kernels and bits as an alignment's iterations. */
int icpgpu_reduce_point_to_plane(icpgpu_ctx* ctx, const float* T, double max_dist, double sums[29]);
/* (host) the symmetrised A^T A inverted as Eigen's 6x6 inverse() does (partial-pivot LU, float64), x = (A^T A)^-1 A^T r,
 * Tk = constructTransformationMatrix(x0..x5) = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] column-major with correctly rounded sin / cos.
 * A zero pivot or a non-finite x: ICPGPU_ERR_INVALID_ARG and Tk = identity (the singular-system rule above). */
int icpgpu_solve_point_to_plane(const double sums[29], double Tk[16]);

/* ---- symmetric objective for ICPGPU_P2PLANE (added under 1.2) ----------------------------------------------------- */
/* replaces IterativeClosestPointWithNormals::setUseSymmetricObjective / setEnforceSameDirectionNormals over
 * TransformationEstimationSymmetricPointToPlaneLLS (PCL >= 1.10; Rusinkiewicz 2019).  Defaults: off, enforce_same_direction = 1
 * (PCL's).  ICPGPU_P2P_SVD, ICPGPU_GICP and ICPGPU_NDT ignore the flag (PCL's other classes have no such setter); icpgpu_align_batch
 * returns ICPGPU_ERR_UNSUPPORTED with the flag on, as for a rejector chain.  The loop is P2PLANE's untouched -- search, accept rule,
 * reciprocal test, rejector chain, min_correspondences, convergence criteria, result fields, fitness -- only the reduction and the
 * solve differ.  With the flag off an alignment launches exactly the kernels it launched before the flag existed.
 *   Per pair past the gate and the chain, with the float transform T of the iteration:
 *     p = T * source[i] (as everywhere), q = target[j], n2 = the target's normal[j],
 *     n1 = R(T) * the source's normal[i]: n1.x = fma(m02, nz, fma(m01, ny, m00 * nx)), ... (rotated, not renormalised, as PCL)
 *   and then in float32, every product, sum and difference rounded on its own:
 *     dot = (n1.x n2.x + n1.y n2.y) + n1.z n2.z
 *     n   = (enforce_same_direction && !(dot >= 0)) ? n1 - n2 : n1 + n2          m = p + q
 *     c   = (m.y n.z - m.z n.y,  m.z n.x - m.x n.z,  m.x n.y - m.y n.x)
 *     r   = ((q.x - p.x) n.x + (q.y - p.y) n.y) + (q.z - p.z) n.z               v = (c.x, c.y, c.z, n.x, n.y, n.z)
 *   sums = {count, sum d2, the 21 upper-triangle entries of sum v v^T row by row, the 6 of sum v r}: icpgpu_reduce_point_to_plane's
 *   layout, float64 sums of float64 products of the widened floats.  A pair whose n has a non-finite component adds to count and
 *   sum d2 only (PCL's `continue`; P2PLANE's rule).
 *   Solve (host, float64): x = (sum v v^T)^-1 sum v r by icpgpu_solve_point_to_plane's linear algebra (the same code); with
 *   R = Rz(x2) Ry(x1) Rx(x0) as constructTransformationMatrix writes it (correctly rounded sin / cos),
 *   Tk = ([R | 0] * [I | (x3, x4, x5)]) * [R | 0] -- rotation R R, translation R t -- two 4x4 products in that order: PCL's
 *   rotation_z * rotation_y * rotation_x * translation * rotation_z * rotation_y * rotation_x.  A zero or NaN pivot or a non-finite
 *   x is the singular-system rule: ICPGPU_ERR_INVALID_ARG and Tk = identity from icpgpu_solve_symmetric_point_to_plane,
 *   NOT_CONVERGED with the last finite transform from an alignment.
 *   DEVIATION: PCL solves this system with ldlt().solve(); the partial-pivot LU inverse differs from it in rounding only, and one
 *   restatement of the linear algebra serves both objectives.
 * A null context: ICPGPU_ERR_INVALID_ARG (the getter: also when both outputs are NULL; either may be). */
int icpgpu_set_p2plane_symmetric(icpgpu_ctx* ctx, int on, int enforce_same_direction);
int icpgpu_get_p2plane_symmetric(const icpgpu_ctx* ctx, int* on, int* enforce_same_direction);
/* icpgpu_reduce_point_to_plane's counterpart: the symmetric sums over the last icpgpu_nn sweep (the context's flag is not read) */
int icpgpu_reduce_symmetric_point_to_plane(icpgpu_ctx* ctx, const float* T, double max_dist, int enforce_same_direction, double sums[29]);
int icpgpu_solve_symmetric_point_to_plane(const double sums[29], double Tk[16]); /* host only */

/* ---- correspondence rejectors (added under 1.2) ------------------------------------------------------------------- */
/* replaces pcl::Registration::addCorrespondenceRejector with pcl::registration::CorrespondenceRejectorMedianDistance, ...Trimmed,
 * ...OneToOne and ...SurfaceNormal (PCL 1.8).  A context holds an ordered chain of at most ICPGPU_MAX_REJECTORS rejectors, empty by default.  In every
 * iteration of ICPGPU_P2P_SVD and ICPGPU_P2PLANE the chain runs on the correspondences that passed the distance gate
 * ((double)d2 <= max_correspondence_distance^2), in the order given, each stage on what the one before it left; the solve,
 * n_correspondences, mse_last, the convergence criteria and the min_correspondences test see what remains.  getFitnessScore
 * (icpgpu_fitness, want_fitness) is untouched, as in PCL.  A correspondence's distance is the float32 squared distance of the search.
 *   MEDIAN_DISTANCE  value = the median factor (finite, >= 0; PCL's default 1.0).  With the n surviving d2 sorted ascending,
 *                    median = sorted[n / 2] (PCL's nth_element at size() / 2); a pair stays iff (double)d2 <= (double)median * factor.
 *   TRIMMED          value = the overlap ratio in [0, 1] (PCL's default 0.5), min_correspondences >= 0 (PCL's default 0):
 *                    m = min(n, max(min_correspondences, (unsigned)(ratio * (float)n))), ratio and product in float32; a pair stays
 *                    iff d2 <= the m-th smallest d2; m = 0 keeps nothing.  DEVIATION: pairs that tie with the m-th smallest ALL stay,
 *                    so more than m can remain; PCL keeps exactly m, and which of the tied ones is whatever std::nth_element leaves
 *                    (unspecified).  The sets are equal whenever the m-th and (m + 1)-th distances differ.
 *   ONE_TO_ONE       of the surviving pairs that share a target index the one with the smallest d2 stays.  DEVIATION: among equal
 *                    d2 the lowest source index (the caller's order) stays; PCL's std::sort leaves that unspecified.
 *   SURFACE_NORMAL   value = the threshold, the cosine of the largest accepted angle between the normals (PCL's setThreshold; finite).
 *                    With n1 = R(T) * the source's normal[i] (this iteration's T; the symmetric objective's expression above),
 *                    n2 = the target's normal[j] and dot = (n1.x n2.x + n1.y n2.y) + n1.z n2.z in float32, a pair stays iff
 *                    (double)dot > value: strict, as in PCL; a NaN dot is rejected.  Normals are the caller's
 *                    (icpgpu_set_source_normals / icpgpu_set_target_normals) or estimated (>= 20 points per cloud, else the
 *                    alignment or icpgpu_correspondences returns ICPGPU_ERR_INVALID_ARG).  One launch per stage; cut = 0.
 * With no surviving pair (n = 0) every rejector keeps nothing.  ICPGPU_GICP and ICPGPU_NDT ignore the chain, as PCL's
 * GeneralizedIterativeClosestPoint::computeTransformation and NormalDistributionsTransform never read correspondence_rejectors_.
 * icpgpu_align_batch with a non-empty chain returns ICPGPU_ERR_UNSUPPORTED for every method (the lock-step kernels fuse the
 * reduction); icpgpu_align_batch_multi runs on contexts of the library's own, which never carry a chain.  With an empty chain an
 * alignment launches exactly the kernels it launched before rejectors existed.  SAMPLE_CONSENSUS is a stage of another kind -- it
 * waits on the host -- and has a section of its own below.  Not provided: the var-trimmed and feature rejectors. */
typedef enum {
  ICPGPU_REJECT_MEDIAN_DISTANCE = 1,
  ICPGPU_REJECT_TRIMMED = 2,
  ICPGPU_REJECT_ONE_TO_ONE = 3,
  ICPGPU_REJECT_SURFACE_NORMAL = 4,
  ICPGPU_REJECT_SAMPLE_CONSENSUS = 5 /* "sample-consensus rejector" below */
} icpgpu_rejector_kind;
#define ICPGPU_MAX_REJECTORS 4
typedef struct {
  int32_t kind;                /* icpgpu_rejector_kind */
  int32_t min_correspondences; /* TRIMMED: min_correspondences; SAMPLE_CONSENSUS: carries max_iterations (1 .. ICPGPU_RSAC_MAX_ITERATIONS) */
  double value;                /* MEDIAN_DISTANCE: factor; TRIMMED: overlap ratio; ONE_TO_ONE: unused; SURFACE_NORMAL: threshold;
                                  SAMPLE_CONSENSUS: the inlier threshold (finite, >= 0) */
} icpgpu_rejector;
/* the whole chain at once; n = 0 clears it.  A bad kind or value, n > ICPGPU_MAX_REJECTORS or a null context:
 * ICPGPU_ERR_INVALID_ARG, and the chain in force stays. */
int icpgpu_set_correspondence_rejectors(icpgpu_ctx* ctx, const icpgpu_rejector* rejectors, size_t n);
/* *n = the chain's length; out (nullable) must hold ICPGPU_MAX_REJECTORS entries */
int icpgpu_get_correspondence_rejectors(const icpgpu_ctx* ctx, icpgpu_rejector* out, size_t* n);
/* the chain's counterpart of icpgpu_nn: what one iteration at transform T (NULL = identity) hands to the solve, per source point in
 * the caller's order -- idx[i] = the target index and d2[i] its squared distance, or idx = -1, d2 = +inf for a pair the gate or the
 * chain removed.  Same kernels as an alignment's iterations; any method's context. */
int icpgpu_correspondences(icpgpu_ctx* ctx, const float* T, int32_t* idx, float* d2);
/* per stage of the chain, for the last iteration of the context's last P2P_SVD / P2PLANE alignment or its last
 * icpgpu_correspondences call, whichever came later: the pairs that entered the stage, the pairs it kept, and its cut as a float d2
 * (MEDIAN_DISTANCE: the median, getMedianDistance(); TRIMMED: the m-th smallest d2; 0 where there is none: ONE_TO_ONE, no pair in,
 * m = 0, SURFACE_NORMAL).  *n_stages = their number; nothing is copied when it exceeds capacity.  Any output array may be NULL. */
int icpgpu_rejector_stats(const icpgpu_ctx* ctx, size_t capacity, uint32_t* pairs_in, uint32_t* pairs_out, float* cut, size_t* n_stages);

/* ---- reciprocal correspondences (added under 1.2) ---------------------------------------------------------------- */
/* replaces pcl::Registration::setUseReciprocalCorrespondences (PCL 1.8: CorrespondenceEstimation::determineReciprocalCorrespondences
 * as IterativeClosestPoint drives it).  Off by default.  When on, in every iteration of ICPGPU_P2P_SVD and ICPGPU_P2PLANE, with
 * x_i = T * source[i] rounded to float as the search and icpgpu_transform round it:
 *   1. forward, as always: j = the nearest target point of x_i (lowest target index among equals), d2 its float32 squared distance;
 *      the pair passes the gate iff (double)d2 <= max_correspondence_distance^2.
 *   2. reverse: k = the nearest of ALL x_* of this iteration to target[j], by the same float32 expression (which is symmetric bit
 *      for bit: the reverse distance of x_i is the pair's d2).  A non-finite x_k is nobody's neighbour.
 *   3. the pair stays iff k == i.  (PCL's second test, reverse distance <= the gate, is implied: the reverse distance is <= d2.)
 * DEVIATION: among x_* at equal distance from target[j] the lowest source index (the caller's order) is the neighbour; PCL's
 * kd-tree leaves that unspecified.  The same kind of deviation as ONE_TO_ONE's, and the kept set is a subset of ONE_TO_ONE's.
 * The rejector chain then runs on what is left, as PCL runs rejectors after estimation; the solve, n_correspondences, mse_last, the
 * convergence criteria and the min_correspondences test see the remainder; getFitnessScore is untouched.  icpgpu_correspondences
 * shows gate, then reciprocal, then chain.  ICPGPU_GICP and ICPGPU_NDT ignore the flag (PCL's classes never read
 * use_reciprocal_correspondence_).  icpgpu_align_batch with the flag set returns ICPGPU_ERR_UNSUPPORTED for every method, as with a
 * chain; icpgpu_align_batch_multi's own contexts never carry it.  With the flag off an alignment launches exactly the kernels it
 * launched before the flag existed.  A null context (or a null `on` of the getter): ICPGPU_ERR_INVALID_ARG. */
int icpgpu_set_reciprocal_correspondences(icpgpu_ctx* ctx, int on);
int icpgpu_get_reciprocal_correspondences(const icpgpu_ctx* ctx, int* on);
/* the pairs past the gate and the pairs past the reciprocal test, for the last iteration of the context's last P2P_SVD / P2PLANE
 * alignment or its last icpgpu_correspondences call, whichever came later (the lifetime of icpgpu_rejector_stats); zeroes when that
 * run had the flag off.  Either output may be NULL. */
int icpgpu_reciprocal_stats(const icpgpu_ctx* ctx, uint32_t* pairs_in, uint32_t* pairs_out);

/* ---- sample-consensus rejector (added under 1.2) ------------------------------------------------------------------ */
/* replaces pcl::registration::CorrespondenceRejectorSampleConsensus<PointXYZ> (PCL 1.8): setInlierThreshold, setMaximumIterations,
 * setInputSource, setInputTarget, getRemainingCorrespondences, getBestTransformation -- RANSAC over a list of pairs with a rigid
 * transform as the model.  It removes STRUCTURED outliers (a parked car that moved, a repeated facade): pairs that are close and
 * merely inconsistent with one rigid motion, which the distance-based rejectors cannot see.  It is a stage of the chain
 * (ICPGPU_REJECT_SAMPLE_CONSENSUS) and a call of its own (icpgpu_correspondence_rejector_sample_consensus), the latter behind
 * descriptor matching: icpgpu_feature_knn(k = 1) -> this call -> best_T16.  The rule restates getRemainingCorrespondences,
 * SampleConsensusModelRegistration and RandomSampleConsensus::computeModel; each departure is a DEVIATION.  Parity with PCL binaries
 * is unpinned; tests/rsac_restated.py is what the kernels are compared with, bit for bit.
 * CORE.  It works on m pairs (P_r, Q_r) of float4 points, r = 0 .. m - 1.
 * HYPOTHESIS t = 0 .. max_iterations - 1.  Draws use the splitmix generator of the plane-segmentation section.  A hypothesis gets up
 * to ICPGPU_RSAC_DRAWS = 16 redraws d = 0 .. 15 of three ranks: with the counter (48 t + 3 d + c + 1) in place of that section's
 * (3 t + c + 1), rank_c = ((z >> 32) * m) >> 32 for c = 0, 1, 2.  A draw is GOOD iff the three ranks differ, all six points are
 * finite, the three pairwise squared distances among the sampled P points each satisfy (double)d2 > sample_d2, strictly, with d2 the
 * search section's float32 expression fma(dz, dz, fma(dy, dy, dx * dx)) (PCL's isSampleGood), and m >= 3.  The first good draw is the
 * sample; with none the hypothesis is INVALID (count = -1, ranks -1), and it counts as an iteration.  DEVIATION: PCL redraws up to
 * 1000 times from rand() and skips failed models; here a hypothesis is a pure function of (seed, t, the pairs).
 * SAMPLE DISTANCE (PCL's computeSampleDistanceThreshold).  The nine sums of the plane refinement's rule over the FINITE P_r, about
 * K = the first finite P: differences in float32, terms exact in double, each sum the exact sum rounded once (moments9).  With n the
 * number of finite P_r, means and covariances in double by that section's formulas, then the cyclic Jacobi (8 sweeps).  Eigenvalues
 * below 0 count as 0 (DEVIATION: PCL takes sqrt of whatever eigen33 returns).  s = ((sqrt(e0) + sqrt(e1)) + sqrt(e2)) / 3.0 with the
 * eigenvalues ascending, in double, sqrt correctly rounded; sample_d2 = s * s.  Without a finite P: moments9 and sample_d2 are 0.
 * TRANSFORM.  As the SCP section's: the 17 sums {3, sum p, sum q, sum q p^T, 0} of the sample's three pairs, taken in sample order
 * in double, go through the host's Umeyama solve (icpgpu_solve's arithmetic); the result is rounded to float32, column-major.  A
 * solve that fails or a result that is not finite makes the hypothesis INVALID (it keeps its ranks; its transform reads as zeros).
 * INLIER.  p' = H p by the fma chain of DESIGN.md section 3, d2 = the search's float32 expression over (p', q).  A pair is an inlier
 * iff (double)d2 < inlier_threshold * inlier_threshold (the product in double), strictly; a pair with a non-finite point never is.
 * count[t] is an exact integer.
 * LOOP.  The plane section's loop word for word, with n = m in w = count / (double)m and probability fixed at 0.99 (PCL's rejector
 * has no setter for it).  `iterations` is the t at which it stops.
 * RESULT.  status 0: m = 0, nothing is kept.  status 1: no t has count > 0 -- this covers m < 3, max_iterations = 0 and a threshold
 * of 0 -- EVERY pair stays and best_T is the identity (PCL's remaining = original).  status 2: the best count is below 3; again
 * every pair stays and best_T is the identity.  status 3: a pair stays iff it is an inlier of the best hypothesis' transform, which is
 * best_T (getBestTransformation()).
 * AS A STAGE.  kind = ICPGPU_REJECT_SAMPLE_CONSENSUS, value = the inlier threshold (finite, >= 0; PCL's default 0.05),
 * min_correspondences = max_iterations (1 .. ICPGPU_RSAC_MAX_ITERATIONS; PCL's default 1000).  DEVIATION: a STAGE with max_iterations = 0
 * is ICPGPU_ERR_INVALID_ARG of icpgpu_set_correspondence_rejectors -- it would keep every pair and pay a wait for it, and an entry
 * {5, 0, value} is what a caller that never filled in min_correspondences sends (a chain written before this kind existed was
 * refused with it); the call of its own accepts max_iterations = 0 (status 1).  ICPGPU_RSAC_MAX_ITERATIONS = 65536: the
 * per-hypothesis record a run keeps on the host (76 bytes each) stays under 5 MB, and the device holds one batch of 64 at a time.
 * The seed is the context's (icpgpu_set_rejector_sac_seed; default 12345, the fixed seed of PCL's non-random RandomSampleConsensus)
 * and is used afresh in every iteration, as PCL constructs a fresh model per call.  The stage runs wherever the chain runs --
 * ICPGPU_P2P_SVD, ICPGPU_P2PLANE, the symmetric objective, icpgpu_correspondences, after the reciprocal stage -- on the pairs the
 * stages before it left, in ascending source index: P_r = x_i = T * source[i], rounded as the search rounds it, Q_r = target[j].  It
 * then empties the keys of the pairs it rejects, as the surface-normal stage does; icpgpu_rejector_stats reports pairs_in = m and
 * pairs_out for it, cut = 0.  ICPGPU_GICP and ICPGPU_NDT go on ignoring the chain and icpgpu_align_batch goes on refusing one.
 * HOST WAITS.  This stage, unlike the others, WAITS ON THE HOST INSIDE AN ITERATION: the sequential loop runs on the host over
 * counts the device takes 64 hypotheses at a time, and the host solves each batch's transforms.  A run of the core waits
 *     1 + 2 B
 * times, B = the batches of 64 hypotheses the loop enters (it enters batch b iff it has not stopped before t = 64 b): one wait for m
 * and moments9, then per batch one for the 17-sum records and one for the counts.  With m < 3 no draw can be good: every hypothesis
 * is INVALID by rule, `iterations` = max_iterations and B = 0.  A stage over an empty source or target, and a call with n_pairs = 0,
 * launch nothing and wait 0 times.  The call of its own waits once more when `kept` is not NULL (the flags' way back).  A chain
 * WITHOUT a stage of this kind queues exactly the launches it queued before the stage existed.
 * THE CALL.  icpgpu_correspondence_rejector_sample_consensus takes two host clouds and a pair list; the same core with
 * P_r = source[index_query[r]], Q_r = target[index_match[r]].  kept[r] (n_pairs int32 flags; may be NULL) = 1 iff pair r stays,
 * *n_kept their number, best_T16 the transform (column-major).  It is defined pair by pair, so duplicated pairs and repeated query
 * indices are ordinary input.  DEVIATION: PCL maps inliers back through the source index, which is undefined for a repeated query
 * index.  ICPGPU_ERR_INVALID_ARG (and a previous result is dropped): an index outside its cloud, a null array against a non-zero
 * size, a threshold that is not finite or is negative, max_iterations outside 0 .. ICPGPU_RSAC_MAX_ITERATIONS, a null n_kept or
 * best_T16.
 * FETCH.  icpgpu_rejector_sac_fetch hands out, for the LAST RUN OF THE CORE on the context -- the call, icpgpu_correspondences, or the
 * last iteration of the last P2P_SVD / P2PLANE alignment with such a stage (the LAST such stage of a chain that has several) -- m,
 * sample_d2, moments9, iterations, status, count[0 .. iterations), per evaluated hypothesis its three ranks (iterations x 3) and its
 * float transform (iterations x 16, column-major), best_t (-1 without one), best_T16, the number kept and the host waits.  Any output
 * may be NULL; with counts, ranks or transforms and capacity_iterations < iterations nothing is written and the call is
 * ICPGPU_ERR_INVALID_ARG, as without a result.
 * ISOLATION.  As the plane section's paragraph: the result lives in buffers of its own and depends on the pairs and the arguments
 * alone.  It reads no search cloud (icpgpu_search_set_input leaves it) and disturbs nothing else of the
 * context; unfetched clustering, segmentation, ISS and ground-filter results survive it and it survives them.
 * Not provided: setRefineModel(true), setSaveInliers / getInliersIndices. */
#define ICPGPU_RSAC_DRAWS 16
#define ICPGPU_RSAC_MAX_ITERATIONS 65536
int icpgpu_set_rejector_sac_seed(icpgpu_ctx* ctx, uint64_t seed);
int icpgpu_get_rejector_sac_seed(const icpgpu_ctx* ctx, uint64_t* seed);
int icpgpu_correspondence_rejector_sample_consensus(icpgpu_ctx* ctx, const float* source_xyzw, size_t n_s, const float* target_xyzw, size_t n_t,
                                                    const int32_t* index_query, const int32_t* index_match, size_t n_pairs,
                                                    double inlier_threshold, int max_iterations, uint64_t seed,
                                                    int32_t* kept /* n_pairs int32 flags, may be NULL */, size_t* n_kept, float best_T16[16]);
int icpgpu_rejector_sac_fetch(icpgpu_ctx* ctx, size_t capacity_iterations, int32_t* m, double* sample_d2, double moments9[9],
                              int32_t* iterations, int32_t* status, int32_t* counts /* iterations */, int32_t* ranks /* iterations x 3 */,
                              float* transforms /* iterations x 16 */, int32_t* best_t, float best_T16[16], size_t* n_kept,
                              int32_t* host_waits);

/* ---- NDT mode (ICPGPU_NDT, added under 1.2) --------------------------------------------------------------------- */
/* setResolution / setStepSize / setOulierRatio.  resolution > 0, step_size > 0, 0 < outlier_ratio < 1, else ICPGPU_ERR_INVALID_ARG.
 * A changed resolution rebuilds the target's cells at the next alignment; the cells are otherwise kept while the target is the same
 * cloud (a target icpgpu_set_target recognises included; a new or promoted target rebuilds them). */
int icpgpu_set_ndt_params(icpgpu_ctx* ctx, double resolution, double step_size, double outlier_ratio);
int icpgpu_get_ndt_params(const icpgpu_ctx* ctx, double* resolution, double* step_size, double* outlier_ratio);
/* getTransformationProbability(): the last NDT alignment's final score / the number of source points (NaN before one) */
int icpgpu_ndt_transformation_probability(const icpgpu_ctx* ctx, double* out);
/* the target's valid cells at the current resolution, ascending cell key: centroid_xyzw (float4: the voxel filter's centroid of the
 * cell, w = 1), mean3 (double), icov6 (xx, xy, xz, yy, yz, zz), n_points.  *n_cells = their number; nothing is copied when it
 * exceeds capacity (call with capacity 0 to size the buffers).  Any output pointer may be NULL. */
int icpgpu_ndt_cells(icpgpu_ctx* ctx, size_t capacity, float* centroid_xyzw, double* mean3, double* icov6, int32_t* n_points,
                     size_t* n_cells);
/* one derivative pass at p = (tx, ty, tz, roll, pitch, yaw), the source transformed by the float T(p): sums = {pairs, score,
 * gradient (6), Hessian upper triangle row by row (21)}.  Same kernels and bits as an alignment's evaluations. */
int icpgpu_ndt_derivatives(icpgpu_ctx* ctx, const double p[6], double sums[29]);
/* (host) one Newton step from the sums at p: delta = pseudo-inverse(H) (-g) (JacobiSVD's threshold), the direction flipped to
 * descend, the step a = clamp(|delta|, eps / 2, step_size) -> p_out = p + a delta / |delta|, *step = a, T_out = T(p_out) (float,
 * column-major).  Returns 0 for a step (a = 0, p_out = p when g . delta is exactly 0), 1 when |delta| is 0 and 2 when it is NaN
 * (p_out = p, *step = 0, T_out = T(p): the loop stops). */
int icpgpu_ndt_step(const double sums[29], const double p[6], double step_size, double eps, double p_out[6], double* step,
                    float T_out[16]);
/* The step rule of the NDT Newton loop, per context (added under 1.2).  PCL18 (default): PCL 1.8's computeStepLengthMT, whose
 * More-Thuente loop never runs -- the step is the Newton length clamped to [eps / 2, step_size], one derivative pass per iteration.
 * MORE_THUENTE: the same function with its loop running (More & Thuente 1994; mu 1e-4, nu 0.9, at most 10 loop trials): the first
 * trial is a 29-term pass, every further trial a score-and-gradient pass (icpgpu_ndt_gradient), and one 29-term pass at the accepted
 * pose when a loop trial was accepted.  Everything else (direction, stopping test, result fields) is the same in both modes; DESIGN.md
 * (f6) states the rule and its two deviations (a NaN candidate step, a non-finite trial).  Any other mode: ICPGPU_ERR_INVALID_ARG.
 * icpgpu_align_batch* refuse NDT in both modes. */
typedef enum { ICPGPU_NDT_LINE_SEARCH_PCL18 = 0, ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE = 1 } icpgpu_ndt_line_search;
int icpgpu_set_ndt_line_search(icpgpu_ctx* ctx, int mode);
int icpgpu_get_ndt_line_search(const icpgpu_ctx* ctx, int* mode);
/* the trial pass at p: sums = {pairs, score, gradient (6)}, the same bits as the first 8 of icpgpu_ndt_derivatives at p */
int icpgpu_ndt_gradient(icpgpu_ctx* ctx, const double p[6], double sums[8]);
/* How a More-Thuente search ends (icpgpu_ndt_line_search_replay's return value; TRIAL = not yet). */
typedef enum {
  ICPGPU_NDT_MT_TRIAL = 0,      /* not ended: *step is the next trial's step */
  ICPGPU_NDT_MT_WOLFE = 1,      /* psi(a) <= 0 and phi'(a) <= -nu phi'(0) (PCL's sufficient decrease and curvature tests) */
  ICPGPU_NDT_MT_INTERVAL = 2,   /* updateIntervalMT found the interval converged (or it starts converged: step_max < step_min) */
  ICPGPU_NDT_MT_TRIAL_CAP = 3,  /* 10 loop trials */
  ICPGPU_NDT_MT_NAN_STEP = 4,   /* the next candidate step is NaN: the last trial is accepted (deviation) */
  ICPGPU_NDT_MT_NON_FINITE = 5  /* a trial's phi or phi' is not finite: the previous trial is accepted, the first trial itself
                                   when it is the one (deviation) */
} icpgpu_ndt_mt_exit;
/* (host) the More-Thuente search replayed from what its trials observed: phi_0 = -score at p, d_phi_0 = -(g . d) < 0 for the
 * descending unit direction d, step_init = |delta|, step_max = step_size, step_min = eps / 2; phi[i], d_phi[i] (i < n) = -score and
 * -(g . d) at trial i.  Returns ICPGPU_NDT_MT_TRIAL with *step = trial n's step and *trial = n, or the exit with *step = the
 * accepted step and *trial = the accepted trial's index; ICPGPU_ERR_INVALID_ARG for a non-finite phi_0, d_phi_0 >= 0 or not finite,
 * a null pointer, or observations past the exit. */
int icpgpu_ndt_line_search_replay(double phi_0, double d_phi_0, double step_init, double step_max, double step_min, const double* phi,
                                  const double* d_phi, int n, double* step, int* trial);
/* the last NDT alignment's line-search trials (MORE_THUENTE; none under PCL18), in order: the Newton iteration (0-based), the step,
 * phi = -score and phi' = -(g . d).  *n_trials = their number; nothing is copied when it exceeds capacity.  Any output may be NULL. */
int icpgpu_ndt_line_search_trace(const icpgpu_ctx* ctx, size_t capacity, int32_t* iteration, double* step, double* phi, double* d_phi,
                                 size_t* n_trials);

/* ICPGPU_GICP_DEVICE=auto only: time GICP's two inner solvers on THIS box with the context's current source, target and parameters
 * (method GICP; a few alignments whose results are discarded) and keep the faster for the context's single alignments from now on.
 * *choice (nullable) = icpgpu_gicp_solver.  Never called implicitly: without it the fixed rule above holds, so two identical runs
 * take identical paths from their first alignment on.  Results cannot depend on the choice (same bits, tests/test_gpu_gicp.py). */
int icpgpu_calibrate(icpgpu_ctx* ctx, int* choice);
/* One evaluation of the QUADRATIC inner objective on the host (no device): sums = 75 double-double numbers as (hi, lo) pairs
 * (icpslam_amd/csrc/icp_gicp_quadratic.h: 60 A, 12 Bq, cq, m, sum d2), base16 = the guess (column-major float 4x4), x = (tx, ty,
 * tz, roll, pitch, yaw) -> f and its gradient as BFGS sees them.  A diagnostic entry: tests check the algebra with it. */
int icpgpu_gicp_quadratic_eval(const double* sums150, const float* base16, const double* x6, double* f, double* g6);
/* The device half of the same mode, alone: correspondences of T * source in the target (d2 < max_correspondence_distance^2), their
 * Mahalanobis matrices at T's rotation, and the 75 sums of the quadratic form as (hi, lo) pairs.  Diagnostic entry (tests). */
int icpgpu_gicp_quadratic_sums(icpgpu_ctx* ctx, const float* T, double* sums150);

/* ---- the step before the path: voxel-grid down-sampling -------------------- */
/* replaces IcpOdometer::voxelFilterCloud = pcl::VoxelGrid<PointXYZ>::filter with leaf (L, L, L)
 * (/root/reference/src/icpslam/icp_odometer.cpp:96-101,177; leaf 0.2 m in config/icpslam.yaml:14):
 * one output point per occupied cell = mean of its points, ascending cell-index order, pad = 1.0f;
 * non-finite points are skipped; if the cell index space overflows int32 the input is returned
 * unchanged (PCL's "leaf size is too small" behaviour). out_xyzw must hold n points. */
int icpgpu_voxel_grid(icpgpu_ctx* ctx, const float* xyzw, size_t n, float leaf, float* out_xyzw, size_t* n_out);
/* (host, no device) the filter's plan for a cloud whose finite points have the bounding box [lo3, hi3]: *verdict = 0 the cell index
 * fits int32 and the cloud is filtered, 1 no finite point (lo > hi on an axis; empty result), 2 PCL's "leaf size is too small" (the
 * input is returned), 3 filtered although the index wraps in int32 as PCL's does (the float extents pass PCL's test, the integer
 * ones are a cell wider); minb3 / divb3 = PCL's min_b_ / div_b_ for 0 and 3.  The one definition the filter itself uses on host
 * and device (icpslam_amd/csrc/icp_voxel_plan.h; DESIGN.md section 2 states the rule).  A diagnostic entry: tests check the rule
 * with it.  leaf must be positive and finite, no pointer null: ICPGPU_ERR_INVALID_ARG otherwise. */
int icpgpu_voxel_plan(const float* lo3, const float* hi3, float leaf, int32_t* verdict, int32_t* minb3, int32_t* divb3);
/* two-step form for callers that size their output by the result (pcl::VoxelGrid::filter resizes `output`): pass
 * out_xyzw = NULL above -- *n_out is the number of voxels, the filtered cloud stays in HBM -- then fetch it into a
 * buffer of `capacity` >= *n_out points.  Valid until the context's next voxel-filter call. */
int icpgpu_voxel_grid_fetch(icpgpu_ctx* ctx, float* out_xyzw, size_t capacity, size_t* n_out);
/* one-step form of the same (1.1): filter, and hand the result out as a VIEW -- *view_xyzw points at *n_out points in the context's
 * pinned staging buffer, valid until the context's next call.  The points are written there by a kernel queued behind the filter's
 * last one and arrive in front of the cell count the host waits for anyway: no second round trip, no copy engine
 * (pcl::VoxelGrid::filter(output): `output.points.assign(view, view + n)`).  The cloud also stays in HBM, and icpgpu_set_source
 * recognises the host copy, exactly as after icpgpu_voxel_grid. */
int icpgpu_voxel_grid_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, float leaf, const float** view_xyzw, size_t* n_out);
/* the odometer's pre-step fused with setInputSource: upload, filter on the device, and make the
 * filtered cloud the source without a round trip to the host (icp_odometer.cpp:177 then :193). */
int icpgpu_set_source_voxel_filtered(icpgpu_ctx* ctx, const float* xyzw, size_t n, float leaf, size_t* n_out);

/* ---- outlier removal (added under 1.2) ---------------------------------------------------------------------------- */
/* replaces pcl::StatisticalOutlierRemoval<PointXYZ>::filter and pcl::RadiusOutlierRemoval<PointXYZ>::filter (PCL 1.8), the filters a
 * LIDAR front end puts between VoxelGrid and the registration.  The rules below restate PCL 1.8; parity with PCL binaries is
 * unpinned, as for every solver here (tests/outlier_restated.py is what the kernels are compared with, bit for bit).
 * COMMON.  Points are float4; a point is finite when x, y and z are.  d2(i, j) is the squared distance of DESIGN.md section 3 with no
 * transform: dx = q.x - p.x, ...; d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32.  Only finite points are searchable.  The output
 * is the kept points in input order (copyPointCloud over the kept indices), the w component carried through.
 * STATISTICAL (mean_k, stddev_mult, negative; PCL's constructor defaults 1, 0.0, false).  For a finite point i take the mean_k + 1
 * smallest d2(i, j) over all finite j, i itself included; drop the smallest (PCL's nn_dists[0], the query); add sqrtf (float32,
 * correctly rounded) of the rest in ascending order into a double; divide by mean_k in double and round to float32: dist[i].  Only
 * the multiset of distances enters: there is no tie rule to define.  A non-finite point gets dist = 0 and is not counted in n_valid
 * (PCL's behaviour: such a point compares against the threshold like any other, so it usually stays).  mean = sum / n_valid,
 * var = (sq_sum - sum * sum / n_valid) / (n_valid - 1), stddev = sqrt(var), threshold = mean + stddev_mult * stddev, all float64,
 * IEEE, each operation rounded on its own.  sum and sq_sum are the EXACT sums of dist[i] and dist[i] * dist[i] (exact in float64)
 * over all i, rounded once -- a stated deviation: PCL adds sequentially in index order.  Point i is removed when
 * (!negative && dist[i] > threshold) || (negative && dist[i] <= threshold), dist widened to double, IEEE comparisons: a NaN
 * threshold (a variance rounded below zero) removes nothing in either mode.
 *   DEVIATION 1: fewer than mean_k + 1 finite points is ICPGPU_ERR_INVALID_ARG (PCL reads past the end of nn_dists there).
 *   DEVIATION 2: mean_k outside 1 .. ICPGPU_SOR_MAX_K (one candidate per lane of a wave) is ICPGPU_ERR_INVALID_ARG.
 * A cloud the k-NN grid cannot index (tight clusters in a wide volume) is searched without it up to 65536 points, as GICP's
 * covariances are; beyond that ICPGPU_ERR_UNSUPPORTED.
 * RADIUS (radius, min_pts, negative; PCL's defaults 0.0, 1, false).  r2 = (float)(radius * radius), the product in double
 * (KdTreeFLANN::radiusSearch).  For a finite point, k = the number of finite j, itself included, with d2(i, j) < r2 -- strict, as in
 * FLANN's radius result set.  A non-finite point has k = 0 (DEVIATION: PCL asserts there).  Point i is removed when
 * (!negative && k <= min_pts) || (negative && k > min_pts).  A radius that is not finite or is negative, or min_pts < 0, is
 * ICPGPU_ERR_INVALID_ARG.  radius = 0 is legal: r2 = 0 and k = 0 for every point.
 * n = 0 is ICPGPU_OK with *n_out = 0.  out_xyzw must hold n points (NULL: only the count; icpgpu_outlier_fetch has the indices).  A
 * view points at *n_out points in the context's pinned staging buffer and is valid until the context's next call, like the voxel
 * filter's.  The filters leave the context's source, target, grids, covariances, NDT cells, voxel-filter result and recognition
 * fingerprints as they were: an alignment after a filter call returns the bits it returned before it.  Not provided:
 * keep_organized / setUserFilterValue. */
#define ICPGPU_SOR_MAX_K 63
int icpgpu_statistical_outlier_removal(icpgpu_ctx* ctx, const float* xyzw, size_t n, int mean_k, double stddev_mult, int negative,
                                       float* out_xyzw, size_t* n_out);
int icpgpu_statistical_outlier_removal_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, int mean_k, double stddev_mult, int negative,
                                            const float** view_xyzw, size_t* n_out);
int icpgpu_radius_outlier_removal(icpgpu_ctx* ctx, const float* xyzw, size_t n, double radius, int min_pts, int negative,
                                  float* out_xyzw, size_t* n_out);
int icpgpu_radius_outlier_removal_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, double radius, int min_pts, int negative,
                                       const float** view_xyzw, size_t* n_out);
/* observers of the LAST outlier filter call on this context (what getRemovedIndices and a debugger would want); a refused call
 * leaves nothing to observe (ICPGPU_ERR_INVALID_ARG).  icpgpu_outlier_stats: the statistical filter's mean, stddev, threshold and
 * n_valid (zeroes after n = 0); after the radius filter ICPGPU_ERR_INVALID_ARG.  Any output may be NULL. */
int icpgpu_outlier_stats(const icpgpu_ctx* ctx, double* mean, double* stddev, double* threshold, size_t* n_valid);
/* measure[i] for every input point (STATISTICAL: dist[i]; RADIUS: (float)k) and the kept points' indices, ascending.  *n_in and
 * *n_kept are always set.  measure / kept_index may be NULL; with both NULL the call only reports the sizes (ICPGPU_OK whatever the
 * capacity).  Otherwise nothing is copied when n_in exceeds capacity (ICPGPU_ERR_INVALID_ARG). */
int icpgpu_outlier_fetch(icpgpu_ctx* ctx, size_t capacity, float* measure, int32_t* kept_index, size_t* n_in, size_t* n_kept);

/* ---- neighbour search (added under 1.2) ---------------------------------------------------------------------------- */
/* replaces pcl::search::KdTree<PointXYZ> / pcl::KdTreeFLANN<PointXYZ>: setInputCloud, nearestKSearch, radiusSearch -- "which points of
 * this cloud are the k nearest to this point" and "which lie within r of it", for any number of queries in one call.  A context
 * holds one SEARCH CLOUD of its own (icpgpu_search_set_input), separate from source, target and the filters' scratch.  The rules
 * restate FLANN's exact search as PCL calls it; parity with PCL binaries is unpinned (tests/search_restated.py is what the kernels are
 * compared with, bit for bit).
 * COMMON.  Points and queries are float4; a point is finite when x, y and z are.  d2 is the squared distance of DESIGN.md section 3
 * with no transform, the query as p and the cloud point as q: dx = q.x - p.x, ...; d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32
 * (the outlier filters' d2).  Only finite cloud points are searchable.
 *   ORDER: a neighbour's key is ((uint64)bits(d2) << 32) | index.  Results are ascending by key: by distance, and among equal
 *   distances the lowest cloud index first.  DEVIATION: FLANN leaves the order of equal distances unspecified (and so which of
 *   several equidistant points make a list of k); this is the rule icpgpu_nn follows for its one neighbour.
 *   queries_xyzw == NULL means "the search cloud's own points, in its order"; n_q must then be 0 or n.
 *   A non-finite query finds nothing (DEVIATION: PCL asserts).  n_q = 0 is ICPGPU_OK.
 * SET_INPUT copies the cloud (the caller's buffer is free on return) and builds its k-NN grid, whose cells come from the cloud's own
 * density as for the statistical outlier filter; the neighbours are exact whatever the cells.  n = 0 is legal: every query then
 * finds nothing.  A cloud the grid cannot index (tight clusters in a wide volume) is searched without it up to 65536 points; beyond
 * that ICPGPU_ERR_UNSUPPORTED, and the context has no search cloud.  A call replaces the previous search cloud whatever it returns.
 * icpgpu_search_knn / _radius without a search cloud: ICPGPU_ERR_INVALID_ARG.  icpgpu_search_size: the search cloud's points and how
 * many of them are finite (either may be NULL; ICPGPU_ERR_INVALID_ARG and zeroes without a search cloud).
 * K-NEAREST.  k must be in 1 .. ICPGPU_SEARCH_MAX_K, else ICPGPU_ERR_INVALID_ARG.  Row i of idx / d2 (k entries, row-major; both must
 * hold n_q * k) holds the m = min(k, n_finite) smallest keys of query i; the other slots hold idx = -1, d2 = +inf.  n_found[i] = m,
 * or 0 for a non-finite query; n_found may be NULL.  Fewer than k finite points is not an error: PCL returns a short list too.  A
 * query that is a cloud point finds itself first (d2 = 0), as in PCL.
 * RADIUS.  r2 = (float)(radius * radius), the product in double; a neighbour qualifies iff d2 < r2, strict (both as for
 * icpgpu_radius_outlier_removal).  radius not finite or negative, or max_nn < 0: ICPGPU_ERR_INVALID_ARG.  radius = 0 finds nothing.
 * max_nn = 0 keeps every qualifying neighbour; max_nn > 0 keeps the max_nn smallest keys among them, for any positive value.
 * The output is CSR: row_start has n_q + 1 entries, row_start[0] = 0; row i is idx / d2 [row_start[i], row_start[i + 1]), ascending
 * by key; *n_total = row_start[n_q].  row_start and n_total must not be NULL.  When *n_total > capacity, or idx / d2 are NULL and
 * *n_total > 0, row_start and *n_total are still written, nothing goes to idx / d2, and the call returns ICPGPU_ERR_INVALID_ARG: the
 * caller sizes its arrays and calls again (a call that finds nothing at all has nothing to deliver and is ICPGPU_OK).  A total
 * beyond INT32_MAX is ICPGPU_ERR_UNSUPPORTED (row_start is then all zero and *n_total 0).
 * ISOLATION.  The search calls leave the context's source, target, every grid, the covariances, the NDT cells, the voxel-filter and
 * outlier-filter results and the recognition fingerprints as they were, and a search's answers depend on the search cloud and the
 * call's arguments alone, not on anything the context did before. */
#define ICPGPU_SEARCH_MAX_K 64
int icpgpu_search_set_input(icpgpu_ctx* ctx, const float* xyzw, size_t n);
int icpgpu_search_size(const icpgpu_ctx* ctx, size_t* n, size_t* n_finite);
int icpgpu_search_knn(icpgpu_ctx* ctx, const float* queries_xyzw, size_t n_q, int k, int32_t* idx, float* d2, int32_t* n_found);
int icpgpu_search_radius(icpgpu_ctx* ctx, const float* queries_xyzw, size_t n_q, double radius, int max_nn, size_t capacity,
                         int64_t* row_start, int32_t* idx, float* d2, size_t* n_total);

/* ---- normal estimation (added under 1.2) --------------------------------------------------------------------------- */
/* replaces pcl::NormalEstimation<PointXYZ, Normal>: setInputCloud, setSearchSurface, setKSearch / setRadiusSearch, setViewPoint,
 * compute -- a surface normal and a curvature per query point from the neighbours the neighbour search finds for it.  The context's
 * SEARCH CLOUD (icpgpu_search_set_input) is the search surface; the queries are the input cloud.  queries_xyzw == NULL means the
 * search cloud's own points (n_q must then be 0 or n), as in icpgpu_search_knn.  Parity with PCL binaries is unpinned;
 * tests/normals_restated.py is what the kernels are compared with, bit for bit.
 * MODE.  Exactly one of k (1 .. ICPGPU_SEARCH_MAX_K) and radius (finite, > 0) is set, the other is 0: both set, neither set, or a
 * value outside its range is ICPGPU_ERR_INVALID_ARG (PCL refuses both set as well).
 * NEIGHBOURS.  For query i the neighbours j_0 .. j_(m-1) are exactly the row icpgpu_search_knn(k) returns, or the row
 * icpgpu_search_radius(radius, max_nn = 0) returns: the same set in the same order -- ascending by the key (bits(d2) << 32 | index),
 * d2 < r2 strict with r2 = (float)(radius * radius); a cloud point among the queries finds itself first.  The order matters: the
 * sums below are float32 and sequential.
 * MOMENTS.  PCL's computeMeanAndCovarianceMatrix with Matrix3f, taken about the first neighbour.  DEVIATION from PCL 1.8, which
 * takes the moments about the origin: its float32 cancellation turns the normal of a 0.3 m planar patch 120 m from the sensor by more
 * than a radian (0.05 rad at 50 m; tests/test_normals_host.py measures both), about the first neighbour it stays within 1e-3 rad.
 * With K = cloud point j_0 (for a cloud's own point: the point itself) and q = cloud point j_t, for t = 0 .. m-1 in order:
 *   dx = q.x - K.x, dy = q.y - K.y, dz = q.z - K.z; nine float32 accumulators from 0:
 *   a0 += dx*dx, a1 += dx*dy, a2 += dx*dz, a3 += dy*dy, a4 += dy*dz, a5 += dz*dz, a6 += dx, a7 += dy, a8 += dz;
 * then a_i /= (float)m, and xx = a0 - a6*a6, xy = a1 - a6*a7, xz = a2 - a6*a8, yy = a3 - a7*a7, yz = a4 - a7*a8, zz = a5 - a8*a8;
 * centroid = (a6 + K.x, a7 + K.y, a8 + K.z).  Every product, sum, difference and quotient is float32 and rounded on its own.
 * PLANE.  DEVIATION: not pcl::eigen33's closed form (its atan2f / cosf / sinf are not portable bit for bit).  The six entries are
 * widened to float64 and decomposed by the NDT cells' cyclic Jacobi (8 sweeps over (0,1), (0,2), (1,2); a rotation whose
 * off-diagonal entry is exactly 0 is skipped).  lambda_min is the smallest diagonal entry, the lowest index among equals; the normal
 * is that column of V rounded to float32; tr = (xx + yy) + zz in float32; curvature = tr != 0 ? fabsf((float)lambda_min / tr) : 0
 * (PCL's solvePlaneParameters).
 * ORIENTATION.  flipNormalTowardsViewpoint with the QUERY point p: vx = vp.x - p.x, ...; cos = (vx*nx + vy*ny) + vz*nz in float32,
 * every operation rounded; all three components are negated when cos < 0, cos == 0 leaves them.  viewpoint3 == NULL means (0, 0, 0);
 * a non-finite viewpoint is ICPGPU_ERR_INVALID_ARG (DEVIATION: PCL computes on).
 * NO NORMAL.  {nx, ny, nz, curvature} are all NaN when the query is non-finite, when m < 3 (k = 1, k = 2, an empty ball, fewer than
 * three finite cloud points), or when one of the six covariance entries is not finite -- where PCL writes NaN and clears is_dense.
 * Coincident neighbours are defined, not refused: the zero matrix gives V = I, the normal (1, 0, 0) before orientation, curvature 0.
 * OUTPUT.  out_nxyzc: n_q float4 {nx, ny, nz, curvature}, required when n_q > 0 -- pcl::Normal's content; it can be handed to
 * icpgpu_set_target_normals as it is (the fourth float is ignored there).  n_neighbours (may be NULL): n_q counts, m always, 0 for
 * a non-finite query.  moments9 (may be NULL): n_q x {xx, xy, xz, yy, yz, zz, cx, cy, cz}; NaN when m < 3 or the query is
 * non-finite, otherwise the computed values even where they are not finite.
 * LIMITS.  No search cloud, a null out_nxyzc, n_q against null queries: ICPGPU_ERR_INVALID_ARG.  With a radius, neighbours beyond
 * INT32_MAX in all: ICPGPU_ERR_UNSUPPORTED.  A cloud the grid refuses is searched without it up to 65536 points (beyond that
 * icpgpu_search_set_input has already refused it).  n_q = 0 is ICPGPU_OK.  Radius rows of thousands of entries (a raw scan's near
 * field) are slow, as in icpgpu_search_radius.
 * ISOLATION.  Like the search calls: the source, the target, every grid, the covariances, P2PLANE's cached normals
 * (icpgpu_normals), the NDT cells and the filters' results stay as they were, and the answers depend on the search cloud and the
 * arguments alone.  One host wait per call with k, two at most with a radius. */
int icpgpu_normal_estimation(icpgpu_ctx* ctx, const float* queries_xyzw, size_t n_q, int k, double radius, const float* viewpoint3,
                             float* out_nxyzc, int32_t* n_neighbours, float* moments9);

/* ---- fast point feature histograms (added under 1.2) --------------------------------------------------------------- */
/* replaces pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33>: setInputCloud, setInputNormals, setSearchSurface, setKSearch /
 * setRadiusSearch, compute -- a 33-bin descriptor per query point from the angles between its neighbours' normals, the feature that
 * global registration (re-localisation, loop closure) matches where no initial guess exists.  The context's SEARCH CLOUD
 * (icpgpu_search_set_input) is the search surface; normals_nxyzc are ITS normals, n float4 in icpgpu_normal_estimation's output format
 * (the fourth float is ignored); the queries are the input cloud.  queries_xyzw == NULL means the search cloud's own points (n_q must
 * then be 0 or n), as in icpgpu_normal_estimation.  Parity with PCL binaries is unpinned; tests/fpfh_restated.py is what the kernels
 * are compared with, bit for bit.  The rules are PCL 1.8's (fpfh.hpp, pfh_tools.cpp), made order-independent or portable where PCL is
 * not.
 * MODE.  Exactly one of k (2 .. ICPGPU_SEARCH_MAX_K) and radius (finite, > 0) is set, the other is 0: both set, neither set, or a
 * value outside its range is ICPGPU_ERR_INVALID_ARG.
 * ROWS.  The row of cloud point p is exactly icpgpu_search_knn(k)'s or icpgpu_search_radius(radius, max_nn = 0)'s row for p over the
 * search cloud: the same set in the same order, p (or a coincident point of lower index) first; its length is m_p.  With queries
 * given, the row of query q is the same call's row for q, of length m_q; without, it is the cloud point's row.
 * PAIR FEATURES of (p, j), j an entry of p's row whose index is not p.  Every operation is float32 and rounded on its own; dots are
 * (x x' + y y') + z z'; P are points, n normals:
 *   1. d = P_j - P_p; f4 = sqrtf((d.x d.x + d.y d.y) + d.z d.z).
 *   2. The pair is SKIPPED when f4 == 0 (a coincident point), or when a component of n_p or n_j is not finite.
 *   3. a1 = (n_p . d) / f4, a2 = (n_j . d) / f4.
 *   4. Swap iff fabsf(a1) < fabsf(a2): then n1 = n_j, n2 = n_p, d = -d, f3 = -a2; otherwise n1 = n_p, n2 = n_j, f3 = a1.
 *      DEVIATION: PCL compares acos(fabs(a1)) > acos(fabs(a2)) -- the same order without the libm call, differing only where acos
 *      rounds two arguments together or an argument exceeds 1.
 *   5. v = d x n1 = (d.y n1.z - d.z n1.y, d.z n1.x - d.x n1.z, d.x n1.y - d.y n1.x); vn = sqrtf((v.x v.x + v.y v.y) + v.z v.z).  The
 *      pair is SKIPPED when vn == 0 (d parallel to n1).
 *   6. v /= vn, a division per component; w = n1 x v, written as v above.
 *   7. f2 = v . n2; y = w . n2; x = n1 . n2.  (PCL's f1 is atan2f(y, x).)
 * BINS.  b2 = clamp((int)floor(11.0 * (((double)f2 + 1.0) * 0.5)), 0, 10) and the same for b3 from f3: float64, as PCL's expression
 * promotes; the clamp is taken on the double, and a NaN lands in bin 0.  b1 is PCL's floor(11 (atan2f(y, x) + pi) / (2 pi)) computed
 * WITHOUT atan2f, whose bits are not portable: a sector test against the ten interior bin edges.  The edge directions
 * (c_k, s_k) = (cos, sin)(2 pi k / 11), k = 1 .. 10, are the float32 constants ICPGPU_FPFH_EDGE_COS / _SIN below.  With
 * (a, b) = (-x, -y), edge k counts as passed iff c_k * b - s_k * a >= 0, the two products and the difference float32 and rounded on
 * their own.  When b >= 0 (true for -0) the test runs on edges 1 .. 5; otherwise (b < 0, or b NaN) edges 1 .. 5 count as passed and
 * the test runs on edges 6 .. 10.  b1 is the number of passed edges.  x = y = 0 of either sign gives bin 5, as atan2f(0, 0) = 0 does.
 *   DEVIATION: pairs within rounding of an edge may land in the neighbouring bin, and an angle of exactly +pi (y = +0, x < 0) lands
 *   in bin 0, where PCL clamps it into bin 10.
 * SPFH of cloud point p: 33 floats.  c[b] are the integer counts of the non-skipped pairs' bins b1, 11 + b2 and 22 + b3;
 * incr = 100.0f / (float)(m_p - 1); spfh[b] = c[b] == 0 ? 0 : (float)c[b] * incr.  DEVIATION: PCL adds incr c times; this differs by
 * rounding only, and the counts do not depend on the order of the pairs.  A row with m_p < 2 (and so a non-finite point, whose row is
 * empty) has an all-zero SPFH.  The SPFH is computed for EVERY cloud point; PCL computes it for the union of the queries'
 * neighbours, which gives the same values where they are used.
 * FPFH of query q, over its row in row order: entries with d2 == 0 are skipped (PCL's rule: the point itself, every coincident point
 * and with them the point's own SPFH); w = 1.0f / d2; for each bin h[b] += spfh[j][b] * w, product and sum in float32.  Then per
 * sub-histogram (bins 0 .. 10, 11 .. 21, 22 .. 32) s = ((..((double)h[0] + h[1]) + ..) + h[10]) in float64, and when s != 0 every bin
 * of it is multiplied by (float)(100.0 / s), in float32.  DEVIATION: PCL sums the products as they are made, in float32; this sums
 * the finished bins and differs by rounding only.  Nothing else is special-cased: a subnormal d2 gives whatever inf / NaN the
 * arithmetic yields.  A non-finite query gives 33 NaN and n_neighbours = 0; an empty row, or a row of only coincident entries, gives
 * 33 zeros.
 * OUTPUT.  out_fpfh: n_q x 33 floats, required when n_q > 0 -- pcl::FPFHSignature33's histogram.  n_neighbours (may be NULL): m_q.
 * spfh (may be NULL): n x 33, every cloud point's SPFH.
 * LIMITS.  ICPGPU_ERR_INVALID_ARG: no search cloud; null normals with n > 0; null out_fpfh with n_q > 0; n_q against null queries;
 * both or neither of k and radius, or one outside its range.  With a radius, neighbours beyond INT32_MAX in all (of the cloud's rows
 * or of the queries'): ICPGPU_ERR_UNSUPPORTED.  A cloud the grid refuses is searched without it, as in icpgpu_normal_estimation.
 * n_q = 0 is ICPGPU_OK and writes nothing.  Not provided: setIndices, other bin counts.
 * ISOLATION.  The call has buffers of its own in the context's search state for the normals and the two histograms, and otherwise
 * uses the search calls' scratch.  Its answers depend on the search cloud and the arguments alone; it leaves
 * the source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud
 * as they were, and an unfetched clustering or plane segmentation result survives it.
 * HOST WAITS.  With k: one, with or without queries.  With a radius: one more per search, for the totals that size its rows -- two
 * without queries, three with. */
#define ICPGPU_FPFH_BINS 33 /* 11 + 11 + 11: pcl::FPFHSignature33 */
#define ICPGPU_FPFH_EDGE_COS                                                                                                         \
  { 0x1.aeb8c8p-1f, 0x1.a9628ep-2f, -0x1.2375f6p-3f, -0x1.4f49e8p-1f, -0x1.eb42aap-1f, -0x1.eb42aap-1f, -0x1.4f49e8p-1f, -0x1.2375f6p-3f, \
    0x1.a9628ep-2f, 0x1.aeb8c8p-1f }
#define ICPGPU_FPFH_EDGE_SIN                                                                                                         \
  { 0x1.14ceep-1f, 0x1.d1bb48p-1f, 0x1.fac9ep-1f, 0x1.82f19cp-1f, 0x1.207e8p-2f, -0x1.207e8p-2f, -0x1.82f19cp-1f, -0x1.fac9ep-1f,      \
    -0x1.d1bb48p-1f, -0x1.14ceep-1f }
int icpgpu_fpfh_estimation(icpgpu_ctx* ctx, const float* normals_nxyzc /* n float4, the search cloud's */, const float* queries_xyzw, size_t n_q,
                           int k, double radius, float* out_fpfh /* n_q x 33 */, int32_t* n_neighbours /* n_q, may be NULL */,
                           float* spfh /* n x 33, may be NULL */);

/* ---- boundary estimation (added under 1.2) ------------------------------------------------------------------------- */
/* replaces pcl::BoundaryEstimation<PointXYZ, Normal, Boundary>: setInputCloud, setInputNormals, setSearchSurface, setKSearch /
 * setRadiusSearch, setAngleThreshold, compute -- "does this point lie on the rim of the sampled surface": an occlusion shadow, the
 * edge of the field of view, the end of a wall.  PCL's isBoundaryPoint projects a point's neighbours onto its tangent plane, takes
 * atan2f of each, sorts the angles and tests "largest gap > angle_threshold".  atan2f's bits are not portable (the problem of FPFH's
 * bin 1), so the rule is restated here without it and without any dependence on order.  Parity with PCL binaries is unpinned;
 * tests/boundary_restated.py is what the kernel is compared with, bit for bit.
 * ROWS.  The context's SEARCH CLOUD (icpgpu_search_set_input) is the search surface; the queries are the input cloud;
 * queries_xyzw == NULL means the search cloud's own points (n_q must then be 0 or n).  Exactly one of k (1 .. ICPGPU_SEARCH_MAX_K)
 * and radius (finite, > 0) is set, the other is 0.  The row of query q is exactly icpgpu_search_knn(k)'s or
 * icpgpu_search_radius(radius, max_nn = 0)'s row for q: the same entries; m_q is its length (n_neighbours[q]).
 * NORMALS.  normals_nxyzc are the QUERIES' normals: n_q float4 in icpgpu_normal_estimation's output format, the fourth float ignored
 * (PCL indexes normals_ by the input cloud as well).  They are taken as given and are not normalised.
 * FRAME.  PCL's getCoordinateSystemOnPlane (Eigen's unitOrthogonal) in float32, every operation rounded on its own.  With n the
 * normal: near = |n.x| <= 1e-5f * |n.z| and |n.y| <= 1e-5f * |n.z|.  If not near: inv = 1.0f / sqrtf(n.x n.x + n.y n.y) and
 * v = (-n.y * inv, n.x * inv, 0).  Otherwise inv = 1.0f / sqrtf(n.y n.y + n.z n.z) and v = (0, -n.z * inv, n.y * inv).  Then
 * u = n x v = (n.y v.z - n.z v.y, n.z v.x - n.x v.z, n.x v.y - n.y v.x), two products and a difference per component.
 * DIRECTIONS.  For every entry j of the row: d = P_j - P_q per component in float32; x_j = (u.x d.x + u.y d.y) + u.z d.z and y_j the
 * same with v.  The entry is SKIPPED when all three components of d are 0 (the point itself and coincident points, as in PCL), when
 * x_j or y_j is not finite (what a zero or a non-finite normal produces), or when x_j == 0 and y_j == 0 (a neighbour straight along
 * the normal; DEVIATION: PCL gives it the angle atan2f(0, 0) = 0).  The remaining entries are the row's directions;
 * n_directions[q] is their number.  It is reported as 0 where the rule below does not look at the row: a non-finite query and m_q < 3.
 * SECTOR TEST.  c = cos(angle_threshold), taken once on the host in double (the plane segmentation's eps_angle is the precedent);
 * c2 = c * c.  For directions a and b every product below is taken in double from the float32 values, where it is exact, and each
 * sum or difference is rounded once (the library is built with -ffp-contract=off):
 *   cr = xa yb - ya xb,  dt = xa xb + ya yb,  na = xa xa + ya ya,  nb = xb xb + yb yb.
 * b lies IN a's SECTOR iff cr >= 0, and not (cr == 0 and dt > 0) -- the same direction -- and
 *   for c >= 0:  dt >= 0 and dt * dt >= (c2 * na) * nb;     for c < 0:  dt >= 0 or dt * dt <= (c2 * na) * nb
 * (double products, rounded).  Mathematically: the angle from a to b, turning from u towards v, lies in (0, angle_threshold].  The
 * signs of cr and dt are exact.
 * BOUNDARY.  boundary[q] = 1 iff the query is finite, m_q >= 3 (PCL's indices.size() < 3 rule), n_directions[q] >= 1, and some
 * direction a has no direction b in its sector; else 0.  This is PCL's "largest gap between angularly consecutive neighbours >
 * angle_threshold", a single direction counting as a gap of 2 pi, and it does not depend on any order.  witness[q] is the lowest
 * cloud index among such a, or -1 where boundary[q] = 0: an output so that tests compare more than one bit per point.
 * DEVIATIONS from PCL 1.8.  No atan2f and no sort: results differ from PCL only where a gap is within rounding of the threshold.  A
 * lattice's gap of exactly pi / 2 counts as ABOVE angle_threshold = M_PI / 2 (the double is below pi / 2: cos(M_PI / 2) > 0), where
 * PCL's float32 comparison says the opposite.  angle_threshold must be finite and in (0, pi]; anything else is
 * ICPGPU_ERR_INVALID_ARG.  An empty row gives 0, where PCL writes NaN.
 * OUTPUT.  boundary: n_q bytes, required when n_q > 0 -- pcl::Boundary's boundary_point.  n_neighbours, n_directions, witness (each
 * may be NULL): n_q int32.
 * LIMITS.  ICPGPU_ERR_INVALID_ARG: no search cloud; null normals or a null boundary with n_q > 0; n_q against null queries; both or
 * neither of k and radius, or one outside its range.  With a radius, neighbours beyond INT32_MAX in all: ICPGPU_ERR_UNSUPPORTED.  A
 * cloud the grid refuses is searched without it, as in icpgpu_normal_estimation.  n_q = 0 is ICPGPU_OK and writes nothing.  The test
 * is quadratic in the row (an interior point leaves after a fraction of its pairs): rows of thousands of entries are slow.
 * ISOLATION.  As icpgpu_fpfh_estimation: the call has buffers of its own in the context's search state for the normals and the
 * results and otherwise uses the search calls' scratch.  Its answers depend on the search cloud and the arguments alone (DESIGN.md
 * section 9b); it leaves the source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters' results
 * and the search cloud as they were, and unfetched clustering, segmentation, sample-consensus and ISS results survive it.
 * HOST WAITS.  One with k, two with a radius (the totals that size the rows, then the results). */
int icpgpu_boundary_estimation(icpgpu_ctx* ctx, const float* normals_nxyzc /* n_q float4 */, const float* queries_xyzw, size_t n_q, int k,
                               double radius, double angle_threshold, uint8_t* boundary /* n_q */, int32_t* n_neighbours /* may be NULL */,
                               int32_t* n_directions /* may be NULL */, int32_t* witness /* may be NULL */);

/* ---- feature-space k-nearest (added under 1.2) -------------------------------------------------------------------- */
/* replaces pcl::KdTreeFLANN<pcl::FPFHSignature33>: setInputCloud, nearestKSearch -- and, with it, feature-space
 * pcl::registration::CorrespondenceEstimation: "which descriptors of that cloud are the k nearest to this descriptor", for any number
 * of query descriptors in one call.  It is the matching step of global registration, between icpgpu_fpfh_estimation and a
 * sample-consensus alignment.  The rules restate FLANN's exact search with the L2 distance; parity with PCL binaries is unpinned
 * (tests/scp_restated.py: feature_knn is what the kernel is compared with, bit for bit).
 * ROWS.  target_feat holds n_t rows and query_feat n_q rows of ICPGPU_FPFH_BINS = 33 floats, row-major, as icpgpu_fpfh_estimation
 * writes them.  The dimension is fixed.  A row is finite when all 33 of its components are.
 * DISTANCE.  For query row q and target row t, every operation float32 and rounded on its own except the fused ones:
 *     d_b = q[b] - t[b];  d2 = d_0 * d_0;  d2 = fmaf(d_b, d_b, d2) for b = 1, 2, ... 32, in that order.
 * This is ONE definition per pair, whatever the kernel's tiling.  A d2 that overflows is +inf, and the pair is still a neighbour.
 * ORDER.  A neighbour's key is the search section's: ((uint64)bits(d2) << 32) | target row index.  Row i of idx / d2 (k entries,
 * row-major; both must hold n_q * k) holds the m = min(k, finite target rows) smallest keys of query i, ascending: by distance, and
 * among equal distances the lowest target index first (DEVIATION: FLANN leaves the order of equal distances unspecified).  The other
 * slots hold idx = -1, d2 = +inf.  n_found[i] = m; n_found may be NULL.
 * NON-FINITE ROWS.  A target row with a non-finite component is never a neighbour.  A query row with a non-finite component finds
 * nothing: n_found = 0, the whole row -1 / +inf (DEVIATION: PCL asserts).  icpgpu_fpfh_estimation writes such rows (33 NaN) for
 * non-finite points.
 * LIMITS.  k must be in 1 .. ICPGPU_SEARCH_MAX_K, else ICPGPU_ERR_INVALID_ARG.  n_t = 0 (every query finds nothing) and n_q = 0
 * (nothing is written) are ICPGPU_OK.  A null target_feat with n_t > 0, a null query_feat, idx or d2 with n_q > 0:
 * ICPGPU_ERR_INVALID_ARG.  The search is exhaustive: n_q * n_t chains of 33 terms on the vector ALUs.  A certified low-precision
 * pre-filter on the matrix cores, as the brute-force nearest neighbour has, is not provided.
 * ISOLATION.  The call neither uses nor touches the search cloud: its descriptors and rows live in buffers of its own.  It leaves the
 * source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud as
 * they were; an unfetched clustering or plane segmentation result survives it; and its answers depend on its arguments alone
 * (DESIGN.md section 9b).  One host wait per call. */
int icpgpu_feature_knn(icpgpu_ctx* ctx, const float* target_feat /* n_t x 33 */, size_t n_t, const float* query_feat /* n_q x 33 */,
                       size_t n_q, int k, int32_t* idx /* n_q x k */, float* d2 /* n_q x k */, int32_t* n_found /* n_q, may be NULL */);

/* ---- euclidean clustering (added under 1.2) ------------------------------------------------------------------------ */
/* replaces pcl::EuclideanClusterExtraction<PointXYZ>: setInputCloud, setClusterTolerance, setMinClusterSize, setMaxClusterSize,
 * extract -- "which points of this cloud belong together".  The call works on the context's SEARCH CLOUD (icpgpu_search_set_input), as
 * normal estimation does.  Parity with PCL binaries is unpinned; tests/cluster_restated.py is what the kernels are compared with, bit
 * for bit -- the answer is a partition of integers and there is no tolerance anywhere.
 * GRAPH.  The vertices are the search cloud's finite points.  Points i != j are joined iff d2(i, j) < r2, strict, with the search
 * section's d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32 and r2 = (float)(tolerance * tolerance), the product in double: the rule
 * of icpgpu_search_radius.  d2 is exactly symmetric in its two points (the differences change sign, the squares do not), so the graph
 * is undirected and its connected components are well defined.  Coincident points have d2 = 0 and are joined for any tolerance whose
 * r2 is above 0.  With tolerance = 0 every finite point is a component of its own (PCL's radiusSearch finds nothing there and the
 * seed stays alone).
 * COMPONENT.  A connected component of that graph; its name is the lowest cloud index in it.  As sets these are exactly what PCL
 * 1.8's extractEuclideanClusters collects with its seed queue (tests/cluster_restated.py: pcl_literal).  Non-finite points are in no
 * component and cannot bridge two of them; their component and label are -1 (DEVIATION: PCL asserts or misbehaves on a non-finite
 * seed).
 * CLUSTER.  A component is emitted iff min_size <= size <= max_size.  All values of the two ints are accepted, as in PCL; with
 * max_size < min_size nothing is emitted.  A component larger than max_size is dropped whole, never truncated.
 * ORDER.  Clusters come out by size descending (PCL's extract() sorts by size); DEVIATION: among equal sizes, which PCL leaves to
 * std::sort, the lowest component name comes first.  Inside a cluster the indices are ascending (DEVIATION: PCL 1.8 leaves them in
 * queue order).  labels[i] is the rank of i's cluster in that order, -1 when i's component was not emitted or i is not finite.
 * CALLS.  icpgpu_euclidean_cluster_extraction computes and KEEPS the result in buffers of its own in the context, and returns the
 * number of clusters and of points in them after one host wait; icpgpu_cluster_fetch copies it out, any number of times.
 * cluster_start / indices are CSR like the radius search's rows: cluster_start has n_clusters + 1 entries, cluster_start[0] = 0, and
 * cluster r is indices[cluster_start[r], cluster_start[r + 1]).  labels and component hold n entries each; either may be NULL.
 * ICPGPU_ERR_INVALID_ARG: no search cloud; a tolerance that is not finite or is negative; a null count pointer; a fetch without a
 * result (none computed, the last call refused, or the search cloud replaced since); a fetch with capacity_clusters < n_clusters or
 * capacity_indices < n_clustered, or null cluster_start, or null indices with n_clustered > 0 -- nothing is written then.  An empty
 * cloud is ICPGPU_OK with zero clusters, and so is a cloud with no finite point.
 * LIMITS.  A cloud the grid refuses is clustered without it (up to the 65536 points icpgpu_search_set_input admits then).  A tolerance
 * whose ball spans more than 8 grid cells is handled as in icpgpu_search_radius: the whole cloud is swept per point, which is slow.
 * Not provided: setIndices.
 * ISOLATION.  The result depends on the search cloud and the three arguments alone.  The call leaves the
 * source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud itself
 * as they were.  A later icpgpu_search_* or icpgpu_normal_estimation call does not disturb a result that has not been fetched yet;
 * icpgpu_search_set_input drops it, whatever it returns. */
int icpgpu_euclidean_cluster_extraction(icpgpu_ctx* ctx, double tolerance, int min_size, int max_size, size_t* n_clusters,
                                        size_t* n_clustered);
int icpgpu_cluster_fetch(icpgpu_ctx* ctx, size_t capacity_clusters, size_t capacity_indices, int64_t* cluster_start /* n_clusters + 1 */,
                         int32_t* indices /* n_clustered */, int32_t* labels /* n, may be NULL */, int32_t* component /* n, may be NULL */);

/* ---- region growing (added under 1.2) ------------------------------------------------------------------------------- */
/* replaces pcl::RegionGrowing<PointXYZ, Normal>: setInputCloud, setInputNormals, setNumberOfNeighbours, setSmoothnessThreshold,
 * setCurvatureThreshold, setCurvatureTestFlag, setMinClusterSize, setMaxClusterSize, extract -- "which points of this cloud lie on one
 * smooth surface".  The call works on the context's SEARCH CLOUD (icpgpu_search_set_input), as clustering does.  PCL's algorithm is a
 * sequential seed queue whose regions depend on the order the points are visited in; this section defines an ORDER-FREE RULE instead,
 * stated as a deviation as the cluster order rules are.  tests/region_restated.py is what the kernels are compared with, bit for bit
 * -- the answer is a partition of integers and there is no tolerance anywhere; its pcl_literal transcribes PCL 1.8's loop, and
 * DESIGN.md section 3 has how far the two are apart on scans.
 * INPUTS.  normals_nxyzc: n float4 {nx, ny, nz, curvature}, one per search-cloud point, required -- what icpgpu_normal_estimation
 * writes.  k in 1 .. ICPGPU_SEARCH_MAX_K: PCL's setNumberOfNeighbours (default 30).  smoothness_cos: the COSINE of PCL's theta; the
 * call takes the cosine itself so that no kernel calls a libm cosine -- the shims compute (float)cos((double)theta).
 * curvature_threshold, min_size, max_size: PCL's.
 * PARTICIPANT.  A finite point whose four normal floats are finite.  Every other point is in no region: kind = -1, region = -1,
 * label = -1, and it cannot bridge two regions.
 * ROW.  row(i) is exactly the row icpgpu_search_knn(k) returns for point i as a query: i itself (or a lower-indexed duplicate of it)
 * first, equal distances in index order.
 * SMOOTH.  smooth(i, j): dot = (nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j in float32, every product and sum rounded on its own -- exactly
 * symmetric in i and j; smooth = fabsf(dot) >= smoothness_cos.  (PCL rejects dot < threshold.)  Antiparallel normals join, as in PCL.
 * CORE.  A participant with !(curvature > curvature_threshold): PCL's test for "may continue as a seed".  A threshold of +inf makes
 * every participant core, which is setCurvatureTestFlag(false).
 * CORE GRAPH.  Cores i != j are joined iff smooth(i, j) and (j is in row(i) or i is in row(j)).  A region's cores are a connected
 * component of this graph, and the region's name is its lowest core index.
 * BORDER.  A participant j that is not core attaches through a core i only when j is in row(i) and smooth(i, j) holds.  Among those
 * cores it takes the one with the smallest key ((uint64)bits(d2) << 32) | i, where d2 is row(i)'s own d2 for j, and joins that core's
 * region: kind = 1, anchor[j] = i.
 * SINGLE.  A non-core participant that no core claims is a region of its own, named by its own index: kind = 0.
 * EMISSION AND ORDER.  Exactly the clustering section's rules: a region is emitted iff min_size <= size <= max_size; size descending,
 * the lowest name first among equals, ascending indices inside a region; labels[i] = the rank of i's region or -1.  Any ints are
 * accepted; max_size < min_size emits nothing.
 * DEVIATIONS from PCL 1.8.  (1) The neighbour relation is symmetrised for cores; PCL follows row(i) only, from whichever seed it
 * visits first.  (2) A border point goes to its nearest listing core, not to the first region that reaches it.  (3) Unclaimed
 * non-core points stay single; in PCL such a point seeds a region and collects its unlabelled smooth neighbours once.  (4) Regions
 * come out in size order; PCL uses seed order.  (5) Non-finite points and normals are defined, not asserted.
 * A RELATION THAT HOLDS EXACTLY.  PCL's propagation edges between cores are a subset of the core graph's edges, so all core points of
 * any region PCL's literal loop grows from a core initial seed lie in ONE region of this rule (tests/test_region_host.py).
 * CALLS.  icpgpu_region_growing computes and KEEPS the result in buffers of its own in the context, and returns the number of regions
 * and of points in them after ONE host wait (the k-nearest rows are queued without one); icpgpu_region_fetch copies it out, any
 * number of times.  region_start / indices are CSR as icpgpu_cluster_fetch's; labels, region (the name of the point's region, emitted
 * or not, -1: none), kind (2 core, 1 border, 0 single, -1 none) and anchor (the claiming core of a border point, else -1) hold n
 * entries each and may be NULL.
 * ICPGPU_ERR_INVALID_ARG: no search cloud; null normals with n > 0; k outside its range; a NaN smoothness_cos or curvature_threshold;
 * a null count pointer; a fetch without a result (none computed, the last call refused, or the search cloud replaced since); a fetch
 * with capacity_regions < n_regions or capacity_indices < n_in_regions, or null region_start, or null indices with n_in_regions > 0
 * -- nothing is written then.  An empty cloud, or a cloud with no participant, is ICPGPU_OK with zero regions.
 * LIMITS.  A cloud the grid refuses is handled as in clustering: its rows come from the search's whole-cloud kernel.
 * Not provided: setIndices, setSmoothModeFlag(false), setResidualTestFlag(true) -- the shims throw or raise on these.
 * ISOLATION.  The result depends on the search cloud and the arguments alone.  The call leaves the source, the
 * target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud itself as they
 * were.  Later icpgpu_search_*, normal estimation, clustering, plane segmentation, ground filter, ISS and moving least squares calls
 * do not disturb a result that has not been fetched yet, nor it theirs: the rows go through the search calls' scratch, everything
 * it keeps -- its copy of the normals included -- lives in buffers of its own.  icpgpu_search_set_input drops it, whatever it
 * returns. */
int icpgpu_region_growing(icpgpu_ctx* ctx, const float* normals_nxyzc /* n float4 */, int k, float smoothness_cos, float curvature_threshold,
                          int min_size, int max_size, size_t* n_regions, size_t* n_in_regions);
int icpgpu_region_fetch(icpgpu_ctx* ctx, size_t capacity_regions, size_t capacity_indices, int64_t* region_start /* n_regions + 1 */,
                        int32_t* indices /* n_in_regions */, int32_t* labels /* n, may be NULL */, int32_t* region /* n, may be NULL */,
                        int32_t* kind /* n, may be NULL: 2 core, 1 border, 0 single, -1 none */, int32_t* anchor /* n, may be NULL */);

/* ---- segment moments (added under 1.2) ------------------------------------------------------------------------------ */
/* replaces, for EVERY segment of a segmentation in one call, pcl::MomentOfInertiaEstimation<PointXYZ> -- setInputCloud, setIndices,
 * compute, getAABB, getOBB, getEigenValues, getEigenVectors, getMassCenter -- and the per-cluster calls that follow a clustering in
 * PCL pipelines: compute3DCentroid, getMinMax3D, computeMeanAndCovarianceMatrix, pcl::PCA.  The call works on the context's SEARCH
 * CLOUD (icpgpu_search_set_input), n points.  Parity with PCL binaries is unpinned; tests/segment_restated.py is what the kernels are
 * compared with, bit for bit.
 * SOURCE.  ICPGPU_SEGMENTS_HOST: the caller's CSR -- segment r lists indices[segment_start[r] .. segment_start[r + 1]), with
 * segment_start[0] = 0, the offsets non-decreasing and every index in [0, n).  Segments may overlap, repeat an index (it counts as often
 * as it is listed), be unsorted or be empty.  ICPGPU_SEGMENTS_CLUSTERS / ICPGPU_SEGMENTS_REGIONS: the result of the last
 * icpgpu_euclidean_cluster_extraction / icpgpu_region_growing over this search cloud, fetched or not, read WHERE IT LIES on the
 * device: nothing is copied to the host or back.  segment_start and indices must then be NULL and n_segments must equal the result's
 * count (a check); record r describes cluster / region r in emitted order.
 * POINTS.  A listed point whose x, y or z is not finite is skipped.  count = the number of finite listed entries.  K = the first finite
 * listed entry of the segment in list order, first = its cloud index.  A segment without one has status = ICPGPU_SEGMENT_EMPTY,
 * count = 0 and every other field zero (first included); every other segment has status = ICPGPU_SEGMENT_OK.
 * SUMS (the plane refinement's rule, restated for a segment).  For every finite listed entry q, (dx, dy, dz) = q - K in float32; the
 * nine sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz take their terms in double, where each term is exact, and each sum
 * is the EXACT sum rounded once: moments9.  They are accumulated in double-double in a FIXED order: the segment's entries are cut at
 * the multiples of ICPGPU_SEGMENT_CHUNK = 64 of their position in the whole list (all segments' entries, one after the other) into
 * pieces; a piece starts with one value per entry, the term or zero for a skipped entry, and is folded in six rounds d = 1, 2, 4, 8,
 * 16, 32: in a round every position p of the piece with p + d inside the piece becomes x[p] + x[p + d], all positions at once; the
 * piece's sum is its first position's.  A segment's pieces are then folded: lane l of 64 adds the pieces l, l + 64, ... in ascending
 * order, starting from zero, and in six rounds d = 32, 16, 8, 4, 2, 1 every lane l < d becomes x[l] + x[l + d]; lane 0 holds the
 * sum.  Two runs give the same bits.  RANGE: with dmax the largest
 * and dmin the smallest non-zero |dx|, |dy| or |dz| of the segment, every sum is the exact one whenever
 * count * (dmax / dmin) < 2^28 (sufficient, not necessary: every difference is a multiple of 2^-24 dmin, every term of 2^-48 dmin^2,
 * and the low parts, at most count^2 dmax^2 2^-53, must stay below 2^53 such units; a factor 4 is kept back) -- 25 entries between
 * 1e-5 and 100 m, or 8000 between 1 mm and 30 m, are inside it; beyond it a sum is that fixed order's double-double result, within
 * an ulp of the exact sum.
 * FINISH.  In double, every operation rounded, with m = count: the means m_a = S_a / m; cov_ab = S_ab / m - m_a m_b, the NORMALISED
 * covariance (divided by m, not by m - 1), cov6 = xx, xy, xz, yy, yz, zz; centroid = K + mean.  The cyclic Jacobi of normal
 * estimation (8 sweeps) gives three eigenvalues with their columns.  ORDER: major >= middle >= minor by eigenvalue, the lower column
 * index first among equals (columns 0 and 1, then 1 and 2, then 0 and 1 change places iff the later one's eigenvalue is strictly
 * larger).  SIGNS: the major and the middle axis are each negated when their component of largest magnitude, the lowest index among
 * equal magnitudes, is negative; minor = major x middle, (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), every product and
 * difference rounded.  eigenvalues3 = major, middle, minor; axes9 = the three axes as rows.  DEVIATION: PCL leaves the order among
 * ties and the signs to Eigen, and scales nothing differently.  Coincident points give a zero matrix and the identity.
 * AXIS-ALIGNED BOX.  aabb_min / aabb_max: the minimum and maximum of the finite listed float32 coordinates themselves, -0 ordered
 * below +0 (the ground filter's sign-flipped integer keys).  Exact and order-free.
 * ORIENTED BOX.  For every finite listed entry and each axis a (major, middle, minor): u_a = (dx e_ax + dy e_ay) + dz e_az in double,
 * d the same float32 difference from K widened, every product and sum rounded on its own.  obb_lo / obb_hi: the minimum and maximum
 * of u_a, -0 below +0, order-free; obb_dims = hi - lo; with c_a = (hi_a + lo_a) / 2,
 * obb_position = K + ((c_0 e_0 + c_1 e_1) + c_2 e_2) per component, in double.  The box's rotation is axes9 (rows).
 * RECORD.  icpgpu_segment_record below; sizeof_record travels with the call (the ABI rule of this header): a size no 1.x header had
 * is refused.
 * ICPGPU_ERR_INVALID_ARG: no search cloud; an unknown source; HOST with a null segment_start, a segment_start that is not a
 * non-decreasing sequence from 0, null indices with a non-zero total, or an index outside [0, n); CLUSTERS / REGIONS with no result
 * (none computed, the last call refused, or the search cloud replaced since), another count, or non-NULL arrays; a null out with
 * n_segments > 0; a wrong sizeof_record.  Nothing is written then.  n_segments = 0 is ICPGPU_OK.  ICPGPU_ERR_UNSUPPORTED: more than
 * 2^31 - 1 listed entries or segments.
 * CALLS.  One host wait per call, the delivery of the records; icpgpu_segment_stats reports the host waits of the last call.
 * Not provided: getMomentOfInertia / getEccentricity (the angle-step sweep of axes), setIndices on top of a segment list -- the
 * shims throw or raise on these.
 * ISOLATION.  The result depends on the search cloud and the arguments alone.  The call keeps nothing; its
 * scratch is its own.  It leaves the source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters'
 * results and the search cloud as they were, and with them unfetched clustering, region growing, plane segmentation, ground filter,
 * ISS and moving least squares results -- the very cluster or region result it reads included. */
#define ICPGPU_SEGMENTS_HOST 0
#define ICPGPU_SEGMENTS_CLUSTERS 1
#define ICPGPU_SEGMENTS_REGIONS 2
#define ICPGPU_SEGMENT_OK 0
#define ICPGPU_SEGMENT_EMPTY 1
#define ICPGPU_SEGMENT_CHUNK 64
typedef struct icpgpu_segment_record {
  int64_t count;          /* finite listed entries */
  int32_t status;         /* ICPGPU_SEGMENT_OK / ICPGPU_SEGMENT_EMPTY */
  int32_t first;          /* K's cloud index */
  double K[3];
  double moments[9];      /* the sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz about K */
  double centroid[3];
  double cov[6];          /* xx, xy, xz, yy, yz, zz */
  double eigenvalues[3];  /* major, middle, minor */
  double axes[9];         /* rows: major, middle, minor */
  float aabb_min[3];
  float aabb_max[3];
  double obb_lo[3];       /* along the axes, about K */
  double obb_hi[3];
  double obb_position[3]; /* the oriented box's centre */
  double obb_dims[3];     /* its extents along major, middle, minor */
} icpgpu_segment_record;
int icpgpu_segment_moments(icpgpu_ctx* ctx, int source, size_t n_segments, const int64_t* segment_start /* n_segments + 1 */,
                           const int32_t* indices, size_t sizeof_record, icpgpu_segment_record* out /* n_segments */);
int icpgpu_segment_stats(const icpgpu_ctx* ctx, int32_t* host_waits);

/* ---- plane segmentation (added under 1.2) --------------------------------------------------------------------------- */
/* replaces pcl::SACSegmentation<PointXYZ> with SACMODEL_PLANE or SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC -- setInputCloud,
 * setDistanceThreshold, setMaxIterations, setProbability, setOptimizeCoefficients, setAxis, setEpsAngle, segment -- and
 * pcl::ExtractIndices<PointXYZ> over its result: "which points lie on the dominant plane", the ground of a driving scan, to be taken
 * away before icpgpu_euclidean_cluster_extraction.  The call works on the context's SEARCH CLOUD (icpgpu_search_set_input), as normal
 * estimation and clustering do.  Parity with PCL binaries is unpinned; tests/sac_restated.py is what the kernels are compared with,
 * bit for bit.
 * HYPOTHESES.  DEVIATION: RANSAC's samples come from a counter-based generator and not from rand(): hypothesis t is a pure function of
 * (seed, t, n), so a batch of hypotheses can be evaluated at once and still equal the sequential loop.  For t = 0, 1, ... and c = 0,
 * 1, 2, in uint64 arithmetic modulo 2^64:
 *     z = seed + (3 t + c + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     z ^= z >> 31;  sample[c] = ((z >> 32) * n) >> 32
 * with n the search cloud's size, NaN rows included.  A hypothesis is INVALID when two of its indices are equal, when one of its
 * points is not finite, or when the cross product below has a squared norm that is 0 or not finite (DEVIATION: a restatement of
 * PCL's collinearity test).
 * MODEL.  Every operation is float32 and rounded on its own: u = p1 - p0, v = p2 - p0, c = (u.y v.z - u.z v.y, u.z v.x - u.x v.z,
 * u.x v.y - u.y v.x), l2 = (c.x c.x + c.y c.y) + c.z c.z, l = sqrtf(l2), n = c / l (a division per component),
 * d = -((n.x p0.x + n.y p0.y) + n.z p0.z).  The coefficients are (n.x, n.y, n.z, d).
 * AXIS.  With axis3 != NULL (SACMODEL_PERPENDICULAR_PLANE) the axis is normalised in double, a = axis / sqrt((x x + y y) + z z), and a
 * hypothesis is also INVALID unless |(a.x n.x + a.y n.y) + a.z n.z| >= cos(eps_angle), everything in double and cos the C library's:
 * PCL's isModelValid without its acos.  eps_angle is ignored without an axis.
 * INLIER.  s = fmaf(n.z, q.z, fmaf(n.y, q.y, n.x * q.x)) + d; a finite point q is an inlier iff (double)fabsf(s) < distance_threshold,
 * strict, as in PCL's countWithinDistance.  Non-finite points are never inliers.  count[t] is the number of inliers of hypothesis t, or
 * -1 for an INVALID one.
 * LOOP.  The answer equals this sequential loop: k = +inf, no best; for t = 0, 1, ...: stop before t when t >= max_iterations or
 * (double)t >= k; if count[t] > 0 and count[t] > the best count so far (strictly), t becomes the best and, with that count,
 * w = count / (double)n, p = 1 - (w w) w clamped to [DBL_EPSILON, 1 - DBL_EPSILON], k = log(1 - probability) / log(p) with the C
 * library's log.  `iterations` is the t at which the loop stopped.  DEVIATIONS: an INVALID sample counts as an iteration (PCL skips
 * up to 10 max_iterations of them); k starts at infinity, not at 1; (w w) w stands for pow(w, 3).  No best means no model: the call
 * is ICPGPU_OK with zero inliers, zero coefficients and found = 0 (PCL prints an error and returns empty outputs).
 * REFINEMENT (PCL's optimize_coefficients; runs when optimize_coefficients != 0 and the best hypothesis has at least 3 inliers).
 * K = cloud[sample[0]] of the best hypothesis; for every inlier q, (dx, dy, dz) = q - K in float32; the nine sums of dx dx, dx dy,
 * dx dz, dy dy, dy dz, dz dz, dx, dy, dz take their terms in double, where each term is exact, and each sum is the EXACT sum rounded
 * once (the statistical outlier filter's rule for sum and sq_sum): moments9.  Then in double, every operation rounded, with m the
 * number of inliers: the means m_a = S_a / m, the covariances cov_ab = S_ab / m - m_a m_b, the cyclic Jacobi of normal estimation
 * (8 sweeps, the smallest diagonal entry, the lowest index among equals, that column rounded to float32).  The refined normal is
 * negated when its float32 dot product with the unrefined normal, (x x' + y y') + z z', is below 0 (PCL leaves the sign to the eigen
 * solver).  d = (float)-((n.x c.x + n.y c.y) + n.z c.z) in double with c = K + mean in double.  The inliers are then selected again
 * with the refined coefficients under the same inlier rule, as PCL's segment() re-selects: those coefficients and inliers are the
 * answer.  With an axis the refined model is not validated again.
 * OUTPUT.  The inlier indices are ascending.  icpgpu_sac_plane_segmentation computes and KEEPS the result in the context and returns
 * the coefficients, the number of inliers, the iterations and found; icpgpu_sac_fetch copies the rest out, any number of times: the
 * inliers, count[0 .. iterations), the best hypothesis' sample and t (-1 without a model), the unrefined coefficients, moments9
 * (zeros when no refinement ran) and the unrefined inlier count.  Any output of the fetch may be NULL; with inliers and
 * capacity_inliers < n_inliers, or counts and capacity_counts < iterations, nothing is written.  icpgpu_sac_stats reports the host waits
 * of the last call (one per batch of 64 hypotheses, two more for a refinement).
 * EXTRACT.  icpgpu_sac_extract copies out the search cloud's points that are (negative = 0) or are not (negative = 1) among the
 * inliers, in cloud order: pcl::ExtractIndices with setNegative.  With negative = 1 non-finite rows are kept: they are "not
 * inliers".  out_xyzw may be NULL (the count alone).  The _view form hands out a view of the pinned staging buffer under the outlier
 * filters' view rule: valid until the next call on the context; NULL for an empty result.
 * ICPGPU_ERR_INVALID_ARG: no search cloud; a threshold that is not finite or is negative; max_iterations outside
 * 0 .. ICPGPU_SAC_MAX_ITERATIONS; probability not strictly inside (0, 1); with an axis: an axis that is not finite or has zero length, an
 * eps_angle that is not finite or is negative; a null coeff4, n_inliers, iterations or found; a fetch or an extract without a result
 * (none computed, the last call refused, or the search cloud replaced since); a null n_out or view pointer.  max_iterations = 0,
 * fewer than three finite points, a threshold of 0 and an empty cloud are all ICPGPU_OK with no model.
 * Not provided: SAC_LMEDS / MSAC, setIndices; the normal-aware plane and the cylinder are the next section's.
 * ISOLATION.  The result depends on the search cloud and the arguments alone; the call needs no grid and works
 * on a cloud the grid refuses.  It leaves the source, the target, every grid, the covariances, the cached normals, the NDT cells, the
 * filters' results, the search cloud and a clustering result as they were; an unfetched clustering result survives a segmentation and
 * an unfetched segmentation result survives a clustering, a search and a normal estimation.  icpgpu_search_set_input drops it,
 * whatever it returns. */
#define ICPGPU_SAC_MAX_ITERATIONS (1 << 20)
int icpgpu_sac_plane_segmentation(icpgpu_ctx* ctx, double distance_threshold, int max_iterations, double probability, uint64_t seed,
                                  int optimize_coefficients, const double* axis3 /* NULL: SACMODEL_PLANE */, double eps_angle, float coeff4[4],
                                  size_t* n_inliers, int32_t* iterations, int32_t* found);
int icpgpu_sac_fetch(icpgpu_ctx* ctx, size_t capacity_inliers, size_t capacity_counts, int32_t* inliers /* n_inliers */,
                     int32_t* counts /* iterations */, int32_t best_sample3[3], int32_t* best_t, float coeff_unrefined4[4], double moments9[9],
                     size_t* n_unrefined_inliers);
int icpgpu_sac_stats(const icpgpu_ctx* ctx, int32_t* host_waits);
int icpgpu_sac_extract(icpgpu_ctx* ctx, int negative, float* out_xyzw, size_t* n_out);
int icpgpu_sac_extract_view(icpgpu_ctx* ctx, int negative, const float** view_xyzw, size_t* n_out);

/* ---- segmentation from normals (added under 1.2) -------------------------------------------------------------------- */
/* replaces pcl::SACSegmentationFromNormals<PointXYZ, Normal> with SACMODEL_NORMAL_PLANE or SACMODEL_CYLINDER and SAC_RANSAC --
 * setInputCloud, setInputNormals, setDistanceThreshold, setNormalDistanceWeight, setRadiusLimits, setMaxIterations, setProbability,
 * setOptimizeCoefficients, setAxis, setEpsAngle, segment: a plane that does not take in the foot of a wall, and then the poles,
 * trunks and pipes of what remains.  The call works on the context's SEARCH CLOUD and on normals_nxyzc, n rows (nx, ny, nz,
 * curvature) for its n points -- icpgpu_normal_estimation's output as it is.  Parity with PCL binaries is unpinned;
 * tests/sac_normals_restated.py is what the kernels are compared with, bit for bit.  Everything the plane section states holds
 * here unless this section says otherwise; every float32 and float64 operation below is rounded on its own, and fmaf is the only
 * fused one.
 * SAMPLES.  The plane section's generator.  NORMAL_PLANE draws three indices with the plane's counter 3 t + c + 1: with the same
 * seed it proposes the triples of icpgpu_sac_plane_segmentation.  CYLINDER draws two with the counter 2 t + c + 1, c = 0, 1.  A
 * hypothesis is INVALID when two indices are equal, a sampled point is not finite, for the cylinder a sampled normal's x, y or z is
 * not finite, or the model below is degenerate.  INVALID counts as an iteration (count = -1).
 * NORMAL_PLANE MODEL.  The plane section's MODEL, operation for operation; four coefficients.  No axis: axis3 != NULL is refused.
 * CYLINDER MODEL.  Seven coefficients (A, dir, r): a point on the axis, the unit direction, the radius.  With (p1, n1), (p2, n2) the
 * two samples and their normals, in float32: w = p1 - p2; a = (n1.x n1.x + n1.y n1.y) + n1.z n1.z, and in the same order b = n1 . n2,
 * c = n2 . n2, d = n1 . w, e = n2 . w; den = a c - b b; sc = (b e - c d) / den, tc = (a e - b d) / den; A = p1 + sc n1, B = p2 + tc n2
 * (a product and a sum per component): the points of closest approach of the two normal lines, PCL's construction (DEVIATION: PCL
 * offsets the first line's origin by n1, which moves A along its line and nothing else).  u = B - A, l2 = (u.x u.x + u.y u.y) +
 * u.z u.z, l = sqrtf(l2), dir = u / l (a division per component); v = p1 - A, x = v x dir (components a b - c d),
 * r = sqrtf((x.x x.x + x.y x.y) + x.z x.z).  INVALID when den <= 0 or den is not finite (parallel lines); when l2 == 0 or l2 is not
 * finite (the closest points coincide: samples on one cross-section); when a component of A or r is not finite; unless radius_min =
 * radius_max = 0, when (double)r < radius_min or (double)r > radius_max; with axis3 != NULL, the axis normalised as the plane
 * section's, when |(a.x dir.x + a.y dir.y) + a.z dir.z| < cos(eps_angle) in double.  DEVIATION: each of these is an exact comparison
 * and not one of PCL's tolerances.
 * THE ANGLE (icpslam_amd/csrc/icp_angle.h).  DEVIATION: PCL takes acos of a normalised dot product, which is portable neither across
 * C libraries nor onto the device.  For a normal m and a direction g, in float32: x = m x g, y = sqrtf((x.x x.x + x.y x.y) + x.z x.z),
 * X = fabsf((m.x g.x + m.y g.y) + m.z g.z), theta = A(y, X), the angle between the two lines folded into [0, pi/2]:
 *     A(y, X) = 0 when y == 0;  P(y / X) when y <= X;  H - P(X / y) when y > X, H = 0x1.921fb6p+0f, the float32 image of pi / 2
 *     P(t) = fmaf(t s, R, t), s = t t, R = C8, then R = fmaf(R, s, Ck) for k = 7 .. 0, with
 *     C0 .. C8 = -0x1.55551ep-2f, 0x1.998bbcp-3f, -0x1.23e71cp-3f, 0x1.be6df6p-4f, -0x1.525702p-4f, 0x1.c7f87cp-5f, -0x1.db5118p-6f,
 *                0x1.414704p-7f, -0x1.97ba58p-10f
 * so theta is exactly 0 for parallel and exactly H for perpendicular directions.  |A(y, X) - atan2(y, X)| <= 2^-22 for finite
 * arguments that are not both 0 (2 ulp of pi / 2 asserted, 1.31 measured: tests/test_sac_normals_host.py).  Neither m nor g is
 * normalised: the angle does not depend on their lengths.  A NaN that an overflow makes here fails the inlier test.
 * DISTANCE.  W = (float)normal_distance_weight.  For a point q with normal row (m, c): NORMAL_PLANE: d_e = fabsf(s) with the plane
 * section's s, g = the plane's normal, w = W (1 - c) (PCL's curvature weighting).  CYLINDER: v = q - A, x = v x dir, dist =
 * sqrtf((x.x x.x + x.y x.y) + x.z x.z), d_e = fabsf(dist - r); t = (v.x dir.x + v.y dir.y) + v.z dir.z, g = v - t dir (a product and
 * a difference per component), w = W.  val = w theta + (1 - w) d_e, evaluated as (w * theta) + ((1 - w) * d_e); q is an inlier iff
 * (double)val < distance_threshold, strict.  A point that is not finite, a normal row with a non-finite x, y, z or curvature, and
 * for the cylinder a g that is (0, 0, 0) (a point on the axis) are never inliers.  With W = 0 and finite normal rows whose
 * products do not overflow, NORMAL_PLANE is icpgpu_sac_plane_segmentation byte for byte.
 * LOOP.  The plane section's LOOP; for the cylinder p = 1 - w w, the sample size being 2.
 * REFINEMENT (optimize_coefficients != 0).  NORMAL_PLANE, with at least 3 inliers: the plane section's REFINEMENT (moments9, the
 * Jacobi, the sign rule), then the inliers are selected again under this section's DISTANCE.  CYLINDER, with at least 5 inliers --
 * DEVIATION: PCL runs Eigen's Levenberg-Marquardt; this is a Gauss-Newton on rho_q = dist(q, axis) - r over the unrefined inliers
 * in a five-parameter chart.  e = the coordinate with the largest |dir_e| of the unrefined model, the lowest index among equals;
 * ia < ib the other two; K = the best sample's first point.  The axis is P + s D with P_e = K_e, D_e = 1 and the parameters p =
 * (P_ia, P_ib, D_ia, D_ib, r), started in double from the unrefined coefficients: D_i = dir_i / dir_e, P_i = A_i + ((K_e - A_e) /
 * dir_e) dir_i, r.  A PASS at p is one device pass over the inliers giving 21 sums: per inlier, in float64, v = (double)q - P,
 * c = v x D, cn = sqrt((c.x c.x + c.y c.y) + c.z c.z), L2 = (D.x D.x + D.y D.y) + D.z D.z, L = sqrt(L2); with cn == 0: rho = -r,
 * J = (0, 0, 0, 0, -1); else dist = cn / L, rho = dist - r, den = cn L, u = D x c, w = c x v, JP_j = -u_j / den, JD_j = w_j / den -
 * (dist D_j) / L2, J = (JP_ia, JP_ib, JD_ia, JD_ib, -1); the terms are J_i J_j for i <= j row by row (15), J_i rho (5), rho rho.
 * Each sum is accumulated in double-double in a fixed order and rounded once: within 1e-12 of the sum of its terms' magnitudes
 * from the exact sum.  Pass 0 is taken at the start.  Then, while fewer than ICPGPU_SAC_CYLINDER_ITERATIONS passes were taken: the
 * host solves (J^T J) delta = -J^T rho by Cholesky (L L^T, column by column, each inner sum subtracted term by term in index
 * order; forward then backward substitution) -- a pivot that is not > 0 stops (STOP_CHOLESKY); a non-finite p + delta stops
 * (STOP_NOT_FINITE); max |delta_i| <= 1e-12 (1 + max |p_i|) stops (STOP_SMALL_STEP); otherwise a pass is taken at p + delta, and the
 * step is kept only if that pass's sum of rho rho is strictly smaller -- if not, p stays and the loop stops (STOP_NO_DECREASE).
 * Reaching the pass limit is STOP_PASSES.  So the final sum of squares is never above the unrefined one.  The refined
 * coefficients: A = (float)P, dir = (float)(sgn D / sqrt((D.x D.x + D.y D.y) + D.z D.z)) with sgn = -1 when the unrefined dir_e < 0,
 * r = (float)fabs(r).  Neither the radius limits nor the axis are validated again.  Then the inliers are selected again.
 * OUTPUT.  As the plane section's.  n_coeff is 4 or 7 (0 without a model), the unused entries of coeff7 are 0.
 * icpgpu_sac_normals_fetch copies out the inliers, count[0 .. iterations), the best sample (the third entry -1 for a cylinder) and
 * t, the unrefined coefficients and inlier count, moments9 (NORMAL_PLANE's refinement, else zeros), cylinder_sums (21 per pass,
 * room for 21 * ICPGPU_SAC_CYLINDER_ITERATIONS doubles, zeros beyond the passes taken), the number of passes and the stop reason (0:
 * no cylinder refinement ran).  Any output may be NULL; capacities as icpgpu_sac_fetch.  The result is "the last segmentation":
 * icpgpu_sac_extract and icpgpu_sac_extract_view work on it, icpgpu_sac_fetch refuses it, and icpgpu_sac_normals_fetch refuses a
 * plane segmentation's result (ICPGPU_ERR_INVALID_ARG, nothing written).  icpgpu_sac_normals_stats: the host waits of the last call
 * -- one per batch of 64 hypotheses entered; NORMAL_PLANE's refinement two more; the cylinder's one per pass and one more.
 * ICPGPU_ERR_INVALID_ARG (nothing written, a previous segmentation result gone): every refusal of the plane call; a model that is
 * neither of the two; null normals; a normal_distance_weight outside [0, 1] or not finite; radius limits that are negative, not
 * finite, or radius_max < radius_min unless both are 0; an axis with NORMAL_PLANE; with CYLINDER the plane call's axis refusals.
 * An empty cloud, max_iterations = 0, a threshold of 0 and fewer finite points than the sample size are ICPGPU_OK with no model.
 * Not provided: the other models, SAC_LMEDS / MSAC, setIndices.
 * ISOLATION.  As the plane section's: the result depends on the search cloud, the normals and the arguments alone, lives in the
 * segmentation's own buffers (the caller's normals are copied there), needs no grid, and leaves everything else in the context as
 * it was.  It replaces a plane segmentation's result and is replaced by one; icpgpu_search_set_input drops it. */
#define ICPGPU_SACMODEL_CYLINDER 5       /* pcl::SacModel's values (PCL 1.8 model_types.h) */
#define ICPGPU_SACMODEL_NORMAL_PLANE 11
#define ICPGPU_SAC_CYLINDER_ITERATIONS 10
#define ICPGPU_SAC_STOP_PASSES 1
#define ICPGPU_SAC_STOP_CHOLESKY 2
#define ICPGPU_SAC_STOP_NOT_FINITE 3
#define ICPGPU_SAC_STOP_SMALL_STEP 4
#define ICPGPU_SAC_STOP_NO_DECREASE 5
int icpgpu_sac_segmentation_from_normals(icpgpu_ctx* ctx, int model, const float* normals_nxyzc /* n float4, the search cloud's */,
                                         double distance_threshold, double normal_distance_weight, double radius_min, double radius_max,
                                         int max_iterations, double probability, uint64_t seed, int optimize_coefficients,
                                         const double* axis3 /* may be NULL */, double eps_angle, float coeff7[7], int32_t* n_coeff,
                                         size_t* n_inliers, int32_t* iterations, int32_t* found);
int icpgpu_sac_normals_fetch(icpgpu_ctx* ctx, size_t capacity_inliers, size_t capacity_counts, int32_t* inliers /* n_inliers */,
                             int32_t* counts /* iterations */, int32_t best_sample3[3], int32_t* best_t, float coeff_unrefined7[7],
                             size_t* n_unrefined_inliers, double moments9[9], double* cylinder_sums /* 21 * ICPGPU_SAC_CYLINDER_ITERATIONS */,
                             int32_t* cylinder_passes, int32_t* cylinder_stop);
int icpgpu_sac_normals_stats(const icpgpu_ctx* ctx, int32_t* host_waits);

/* ---- ground filter (added under 1.2) -------------------------------------------------------------------------------- */
/* replaces pcl::applyMorphologicalOperator<PointXYZ> and pcl::ProgressiveMorphologicalFilter<PointXYZ> -- setInputCloud,
 * setMaxWindowSize, setSlope, setMaxDistance, setInitialDistance, setCellSize, setBase, setExponential, extract -- and
 * pcl::ExtractIndices<PointXYZ> over its result: "which points are ground" where the ground slopes, crowns or ripples and is no
 * plane.  Both calls work on the context's SEARCH CLOUD (icpgpu_search_set_input), as clustering and plane segmentation do.  Parity
 * with PCL binaries is unpinned; tests/pmf_restated.py is what the kernels are compared with, bit for bit.  Everything is float32,
 * every operation rounded on its own, unless said otherwise.
 * BOX.  For a centre p and a window w (float32): h = w / 2.0f, lo = p - h and hi = p + h per axis x and y, each rounded once.  A
 * finite point q is in p's box iff lo.x <= q.x and q.x <= hi.x and lo.y <= q.y and q.y <= hi.y: inclusive bounds, as in PCL's
 * boxSearch; z does not take part.  A point with a non-finite x, y or z is in no box and has no box.  A finite point is always in its
 * own box.  After rounding the relation need NOT be symmetric: q in p's box does not imply p in q's (p - h and q + h round apart).
 * EXTREMUM.  min and max over a box's members are taken in the total order of finite floats in which -0.0f is below +0.0f: the
 * order of the integer keys bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000).  The result's bits are therefore defined.
 * OPERATOR (icpgpu_morphological_operator; the window is (float)resolution), over an active set A of finite points.  ERODE:
 * out[i] = min z[j] over the j in A inside i's box.  DILATE: the same with max.  OPEN: e = ERODE(z), then out[i] = max e[j] over
 * the same boxes.  CLOSE: d = DILATE(z), then out[i] = min d[j].  Boxes always come from the input x, y.  Points outside A keep
 * their own z (its bits) on output.  For the entry point A is every finite point; inside the filter it is the current ground.
 * SCHEDULE (extract's loop).  The parameters arrive as doubles and each is rounded to float32 once (PCL's setters take floats);
 * max_window_size is converted to float32.  it = 0, window = 0; while window < max_window_size:
 *     exponential: window = (float)((double)cell * (2.0 * B + 1.0)), B = base^it by `it` successive double multiplications of 1.0 with
 *                  (double)base.  DEVIATION: PCL calls std::pow on floats; the two are equal for base 2.
 *     linear:      window = cell * (2.0f * (float)(it + 1) * base + 1.0f), float32, left to right.
 *     threshold:   thr = initial_distance when it == 0, else slope * (window - previous window) * cell + initial_distance, float32,
 *                  left to right; then if (thr > max_distance) thr = max_distance.
 *     append (window, thr); ++it.
 * PASSES.  The ground starts as every finite point.  For every schedule entry, in order: o = OPEN(z) over the current ground with
 * that window; point i stays iff z[i] - o[i] < thr (one float32 subtraction, a strict comparison; a NaN difference removes the
 * point).  With initial_distance = 0 the first pass's threshold is 0 and a point stays only where o[i] > z[i]; wherever the box
 * relation is symmetric around i (i is in the box of every member of its own box) e[j] <= z[i] for all of them, so o[i] <= z[i] and
 * the point is removed: on such clouds the first pass removes every point.
 * removed_at[i] is the pass that removed i, -1 for a ground point, -2 for a non-finite point (DEVIATION: PCL keeps non-finite
 * points' indices in the ground).  The ground indices are ascending.
 * OUTPUT.  icpgpu_progressive_morphological_filter computes and KEEPS the result in the context and returns the number of ground
 * points and of passes; icpgpu_pmf_fetch copies the rest out, any number of times: the ground indices, the schedule's windows and
 * thresholds, the ground's size after each pass and removed_at (n entries).  Any output of the fetch may be NULL; with
 * capacity_ground < n_ground or capacity_passes < n_passes nothing is written.  icpgpu_pmf_stats reports the host waits of the last
 * filter or operator call on this search cloud, whichever was later: exactly one, whatever the number of passes (the schedule is
 * known before anything is launched and the ground's size stays on the device between passes), and none for an empty cloud or a
 * schedule without a pass.  ARGUMENT ADDED to the proposed icpgpu_pmf_stats(ctx, host_waits): point_tests (may be NULL), the exact
 * point tests the last filter call's rim scans made (0 after an operator call) -- the figure that says what the cell table saves
 * over testing every pair, which no other entry point could report.
 * EXTRACT.  icpgpu_pmf_extract copies out the search cloud's points that are (negative = 0) or are not (negative = 1) in the ground,
 * in cloud order: pcl::ExtractIndices with setNegative.  With negative = 1 non-finite rows are kept: they are "not ground".
 * out_xyzw may be NULL (the count alone).  The _view form hands out a view of the pinned staging buffer under the outlier filters'
 * view rule: valid until the next call on the context; NULL for an empty result.
 * ICPGPU_ERR_INVALID_ARG (nothing is kept and a previous filter result is dropped): no search cloud; a parameter that is not finite
 * after rounding; cell_size <= 0; a negative slope, initial_distance or max_distance; exponential with base <= 1 or linear with
 * base <= 0 (PCL would loop for ever); a schedule of more than ICPGPU_PMF_MAX_PASSES passes; a window that is not finite; a null
 * n_ground or n_passes; for the operator a resolution that is not finite or is <= 0 as a float, an op outside 0 .. 3, a null out_z;
 * a fetch or an extract without a result (none computed, the last filter call refused, or the search cloud replaced since); a null
 * n_out or view pointer.  max_window_size <= 0 is ICPGPU_OK with zero passes and every finite point ground; an empty cloud and a
 * cloud without a finite point are ICPGPU_OK with zero ground points.
 * Not provided: setIndices, pcl::ApproximateProgressiveMorphologicalFilter, batch entry points.
 * ISOLATION.  The result depends on the search cloud and the arguments alone; the calls need no grid and work
 * on a cloud the grid refuses.  They leave the source, the target, every grid, the covariances, the cached normals, the NDT cells,
 * the filters' results, the search cloud and a clustering, plane segmentation, sample-consensus, ISS or moving least squares result as
 * they were; an unfetched result of any of those survives a ground filter call, an unfetched ground filter result survives those
 * calls and icpgpu_morphological_operator.  icpgpu_search_set_input drops it, whatever it returns. */
#define ICPGPU_PMF_MAX_PASSES 32
typedef enum { ICPGPU_MORPH_ERODE = 0, ICPGPU_MORPH_DILATE = 1, ICPGPU_MORPH_OPEN = 2, ICPGPU_MORPH_CLOSE = 3 } icpgpu_morph_op;
int icpgpu_morphological_operator(icpgpu_ctx* ctx, double resolution, int op, float* out_z /* n */);
int icpgpu_progressive_morphological_filter(icpgpu_ctx* ctx, int max_window_size, double slope, double initial_distance, double max_distance,
                                            double cell_size, double base, int exponential, size_t* n_ground, int32_t* n_passes);
int icpgpu_pmf_fetch(icpgpu_ctx* ctx, size_t capacity_ground, size_t capacity_passes, int32_t* ground /* n_ground */,
                     float* window_sizes /* n_passes */, float* height_thresholds /* n_passes */, int32_t* ground_after /* n_passes */,
                     int32_t* removed_at /* n */);
int icpgpu_pmf_stats(const icpgpu_ctx* ctx, int32_t* host_waits, uint64_t* point_tests);
int icpgpu_pmf_extract(icpgpu_ctx* ctx, int negative, float* out_xyzw, size_t* n_out);
int icpgpu_pmf_extract_view(icpgpu_ctx* ctx, int negative, const float** view_xyzw, size_t* n_out);

/* ---- sample-consensus alignment with pre-rejection (added under 1.2) ------------------------------------------------ */
/* replaces pcl::SampleConsensusPrerejective<PointXYZ, PointXYZ, FPFHSignature33>: setInputSource, setSourceFeatures, setInputTarget,
 * setTargetFeatures, setNumberOfSamples, setCorrespondenceRandomness, setSimilarityThreshold, setMaxCorrespondenceDistance,
 * setInlierFraction, setMaximumIterations, align, hasConverged, getFinalTransformation, getInliers, getFitnessScore -- the pose of one
 * cloud in another WITHOUT an initial guess, from matched descriptors: re-localisation and loop closure, and the start every ICP of
 * this library needs.  The chain icpgpu_voxel_grid -> icpgpu_normal_estimation -> icpgpu_fpfh_estimation -> icpgpu_scp_align -> ICP is
 * a global registration.  The TARGET is the context's SEARCH CLOUD (icpgpu_search_set_input), whose grid scores a hypothesis;
 * target_feat are its n descriptors (n x 33 floats); the source cloud (n_s float4) and its n_s descriptors are arguments.  Parity
 * with PCL binaries is unpinned; tests/scp_restated.py is what the kernels are compared with, bit for bit.  The rules are PCL 1.8's
 * loop (sample_consensus_prerejective.hpp); each departure is a DEVIATION.
 * CORRESPONDENCES.  Row i of the source is exactly icpgpu_feature_knn(target_feat, n, source_feat, n_s, k_correspondences)'s row, of
 * length m_i = n_found[i].  DEVIATION: the rows are computed for every source point up front (and stay on the device); PCL fills
 * them lazily per sampled point.  The values are the same.
 * HYPOTHESIS t = 0 .. max_iterations - 1.  DEVIATION, as in plane segmentation: the draws come from that section's counter-based
 * generator, so a hypothesis is a pure function of (seed, t, sizes).  With nr = nr_samples, draw c = 0 .. 2 nr - 1 is
 *     z = seed + ((2 nr) t + c + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     z ^= z >> 31;  u_c = z >> 32
 * in uint64 arithmetic modulo 2^64.  Source index s_c = (u_c * n_s) >> 32 for c < nr; target pick j_c = (u_(nr + c) * m_(s_c)) >> 32,
 * and the target index is entry j_c of row s_c (-1 when m_(s_c) = 0).  PCL draws without repetition; here a repetition makes the
 * hypothesis INVALID.  Per-hypothesis status:
 *   ICPGPU_SCP_INVALID       two equal source indices, a sampled source or target point that is not finite, or an m of 0;
 *   ICPGPU_SCP_PREREJECTED   the polygon test below failed;
 *   ICPGPU_SCP_NO_TRANSFORM  the solve below gave no finite transform;
 *   ICPGPU_SCP_EVALUATED     scored.
 * An INVALID sample counts as an iteration.
 * PRE-REJECTION (CorrespondenceRejectorPoly::thresholdPolygon).  For the nr edges (c, (c + 1) mod nr): ds and dt are the squared
 * lengths between the two sampled source points and between the two sampled target points, the search section's
 * d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32; lo = the smaller, hi = the larger; the edge passes iff
 * lo / hi >= (float)(similarity_threshold * similarity_threshold), ONE float32 division, the product in double.  A NaN (0 / 0) fails.
 * All edges must pass.
 * TRANSFORM.  The 17 sums of icpgpu_solve {nr, sum p, sum q, sum q p^T, 0} over the nr pairs (p the source point, q the target
 * point), every term and sum in double, accumulated in sample order, go through the host's Umeyama solve (icpgpu_solve); the result
 * is rounded to float32, column-major.  The DEVICE does not solve: the host does, for every hypothesis that survives the
 * pre-rejection.  KNOWN COST: with a low similarity threshold that is up to 65536 small SVDs per chunk on one host thread.
 * FITNESS (getFitness).  For every source point p: p' = T p by the fma chain of DESIGN.md section 3; the nearest finite target point
 * by key over the search cloud; p is an INLIER iff d2 < r2, strictly, with r2 = (float)(d * d), d = max_correspondence_distance, the
 * product in double (the radius search's rule).  A non-finite source point, or one with a non-finite image, is never an inlier, but
 * counts in n_s.  count_t is an exact integer.  S_t is the sum of the inliers' d2 taken in double: the EXACT sum rounded once (the
 * outlier filter's and the plane refinement's rule), accumulated in double-double in a fixed order.  RANGE: the sum is exact whenever
 * count^2 * (the largest inlier d2 / the smallest non-zero inlier d2) < 2^80 -- 2^20 inliers between 1e-8 and 1e4 m^2 are inside it;
 * beyond it S_t is that fixed order's double-double result, within an ulp of the exact sum.  error_t = (float)(S_t / (double)count_t)
 * when count_t > 0, FLT_MAX otherwise.
 * CHOICE.  Going through t ascending, t becomes the best iff count_t > 0, (float)count_t / (float)n_s >= (float)inlier_fraction, and
 * error_t < the best error so far, strictly, starting from FLT_MAX.  PCL has no early stop and neither does this: max_iterations
 * hypotheses are always considered.  No best: converged = 0, T = identity, zero inliers, fitness = FLT_MAX, and out_xyzw is the
 * source under the identity.  Otherwise converged = 1 and T16 (column-major), the inlier indices (ascending), fitness = error and the
 * aligned source out_xyzw (n_s float4, w = 1; may be NULL) are the best hypothesis'.  DEVIATION: a guess is not provided.
 * CALLS.  icpgpu_scp_align computes and KEEPS the result in the context.  It runs in chunks of ICPGPU_SCP_CHUNK hypotheses: the device
 * samples and pre-rejects a chunk; one host wait; the host solves the survivors; the device scores them 64 at a time, every launch
 * queued; one host wait; after the last chunk one pass over the best hypothesis and one more wait.  Host waits: two per chunk (one
 * where nothing survives) plus one for the best hypothesis' pass; an empty source has no chunks and no pass: 0 waits, and
 * max_iterations = 0 with a source has the pass alone: 1.  icpgpu_scp_stats reports them, the number of EVALUATED hypotheses and the
 * host's solve time in ms.  The per-chunk results reach pageable host memory, where the runtime may wait inside a copy: the count is of
 * the call's own waits.
 * icpgpu_scp_fetch hands out, any number of times, per hypothesis t in [0, max_iterations): status, the nr source and the nr target
 * indices (t-major), the float transform (16, column-major; zeros unless EVALUATED), count, S and error; best_t (-1 without one) and
 * the inliers.  Any output may be NULL; with a per-hypothesis output and capacity_hypotheses < max_iterations, or inliers and
 * capacity_inliers < n_inliers, nothing is written and the call is ICPGPU_ERR_INVALID_ARG.
 * ICPGPU_ERR_INVALID_ARG: no search cloud; nr_samples outside 3 .. ICPGPU_SCP_MAX_SAMPLES; k_correspondences outside
 * 1 .. ICPGPU_SEARCH_MAX_K; a similarity_threshold or inlier_fraction outside [0, 1] or not finite; a distance that is not finite or is
 * negative; max_iterations outside 0 .. ICPGPU_SCP_MAX_ITERATIONS; a null cloud or descriptor array against a non-zero size; a null
 * T16, n_inliers, fitness or converged; a fetch or stats without a result (none computed, the last call refused, or the search cloud
 * replaced since).  max_iterations = 0, an empty source and an empty target are ICPGPU_OK with converged = 0.
 * LIMITS.  A target the grid refuses is scored without it (up to the 65536 points icpgpu_search_set_input admits then): every source
 * point sweeps the whole cloud per hypothesis.  So does a correspondence distance whose ball spans more than 8 grid cells, as in
 * icpgpu_search_radius: both are slow.
 * ISOLATION.  As plane segmentation: the result lives in buffers of its own, depends on the search cloud and the arguments alone
 * (DESIGN.md section 9b), survives searches, normal and FPFH estimations, feature searches, clusterings and segmentations, and they
 * survive it; icpgpu_search_set_input drops it, whatever it returns.  The source, the target, every grid and everything an alignment
 * reads stay as they were. */
#define ICPGPU_SCP_CHUNK 65536
#define ICPGPU_SCP_MAX_ITERATIONS (1 << 20)
#define ICPGPU_SCP_MAX_SAMPLES 8
#define ICPGPU_SCP_INVALID 0
#define ICPGPU_SCP_PREREJECTED 1
#define ICPGPU_SCP_NO_TRANSFORM 2
#define ICPGPU_SCP_EVALUATED 3
int icpgpu_scp_align(icpgpu_ctx* ctx, const float* source_xyzw, size_t n_s, const float* source_feat /* n_s x 33 */,
                     const float* target_feat /* n x 33, the search cloud's */, int nr_samples, int k_correspondences,
                     double similarity_threshold, double max_correspondence_distance, double inlier_fraction, int max_iterations, uint64_t seed,
                     float T16[16], size_t* n_inliers, float* fitness, int32_t* converged, float* out_xyzw /* n_s float4, may be NULL */);
int icpgpu_scp_fetch(icpgpu_ctx* ctx, size_t capacity_hypotheses, size_t capacity_inliers, int32_t* status, int32_t* source_idx /* it x nr */,
                     int32_t* target_idx /* it x nr */, float* transforms /* it x 16 */, int32_t* counts, double* sums, float* errors,
                     int32_t* best_t, int32_t* inliers /* n_inliers */);
int icpgpu_scp_stats(const icpgpu_ctx* ctx, int32_t* host_waits, int32_t* evaluated, double* host_solve_ms);

/* ---- ISS keypoints (added under 1.2) -------------------------------------------------------------------------------- */
/* replaces pcl::ISSKeypoint3D<PointXYZ, PointXYZ> (PCL 1.8, keypoints/impl/iss_3d.hpp): setInputCloud, setSalientRadius,
 * setNonMaxRadius, setThreshold21, setThreshold32, setMinNeighbors, compute, and -- through icpgpu_iss_keypoints_border, BORDER
 * ESTIMATION below -- setBorderRadius, setNormalRadius, setNormals, setAngleThreshold -- "at which points of this cloud are
 * descriptors worth computing", the stage in front of icpgpu_fpfh_estimation at keypoints.  The call works on the context's SEARCH
 * CLOUD (icpgpu_search_set_input), as clustering and plane segmentation do.  Parity with PCL binaries is unpinned;
 * tests/iss_restated.py is what the kernels are compared with, bit for bit.
 * BALLS.  For both radii r2 = (float)(radius * radius), the product in double.  A finite cloud point j is in the ball of point i iff
 * d2(i, j) < r2, strict, with the search section's float32 d2.  The point itself and points coincident with it are in its ball.
 * Non-finite points are in no ball and have an empty one.  As sets these are exactly the rows of icpgpu_search_radius(radius,
 * max_nn = 0) with the cloud's own points as queries; no row is ever materialised, and memory is O(n) whatever the radii.
 * SCATTER (PCL's getScatterMatrix).  For each j in the salient ball of i, (dx, dy, dz) = P_j - P_i in float32.  The six products
 * dx dx, dx dy, dx dz, dy dy, dy dz, dz dz are taken in double, where each is exact, and each of the six sums is the EXACT sum rounded
 * once (the rule of the plane refinement's nine sums and the statistical outlier filter's sum and sq_sum): scatter6, in that order.
 * DEVIATION: PCL takes the differences in double and adds rounded products in the neighbours' order; this rule does not depend on
 * any order.  The sums are not divided by the count, as in PCL.  n_salient[i] is the size of the salient ball.  When
 * n_salient[i] < min_neighbors the scatter is reported as six zeros and the point has no saliency.
 * EIGENVALUES.  The cyclic Jacobi of normal estimation on the symmetric matrix of the six sums: 8 sweeps, the same expressions.
 * DEVIATION: PCL uses Eigen's SelfAdjointEigenSolver.  eigenvalues3[i] = the diagonal (d0, d1, d2) sorted descending by the network
 * "swap (d0, d1) if d0 < d1; swap (d1, d2) if d1 < d2; swap (d0, d1) if d0 < d1": (e1, e2, e3).  saliency[i] = e3 iff all three
 * eigenvalues are finite, e3 >= 0, n_salient[i] >= min_neighbors, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 -- double divisions,
 * strict comparisons, a NaN quotient fails -- and 0 otherwise.  A skipped point (non-finite, or with too few neighbours) reports the
 * eigenvalues 0, 0, 0.
 * NON-MAXIMA SUPPRESSION.  Point i is a keypoint iff saliency[i] > 0, its non-max ball holds at least min_neighbors points, and no j
 * in that ball has saliency[j] > saliency[i].  The comparison is strict, so equal maxima within one ball are all keypoints, as in
 * PCL.  Neither the non-max ball's size nor the maximum is an output.
 * OUTPUT.  The keypoint indices are ascending; keypoints_xyzw holds those rows of the search cloud, bit for bit.
 * icpgpu_iss_keypoints computes and KEEPS the result in buffers of its own in the context and returns the number of keypoints after
 * one host wait; icpgpu_iss_fetch copies out any subset of it, any number of times: every pointer may be NULL.  n_salient and saliency
 * hold n entries, scatter6 n x 6, eigenvalues3 n x 3.  With keypoint_index or keypoints_xyzw requested and capacity_keypoints <
 * n_keypoints nothing is written and the fetch returns ICPGPU_ERR_INVALID_ARG.  icpgpu_iss_stats reports the host waits of the last
 * compute call: one, for the count (more with border estimation: below).
 * ICPGPU_ERR_INVALID_ARG: no search cloud; a radius that is not finite or is <= 0; a gamma that is not finite; min_neighbors < 0; a
 * null n_keypoints; a fetch or stats without a result (none computed, the last call refused, or the search cloud replaced since).  An
 * empty cloud and a cloud with no finite point are ICPGPU_OK with no keypoints.
 * LIMITS.  A cloud the grid refuses is walked without it (up to the 65536 points icpgpu_search_set_input admits then), and a radius
 * whose ball spans more than 8 grid cells is handled as in icpgpu_search_radius: the whole cloud is swept per point, which is slow.
 * All three paths give the same bits.
 * BORDER ESTIMATION (icpgpu_iss_keypoints_border; PCL 1.8's getBoundaryPoints and detectKeypoints).  With border_radius > 0, points
 * near the rim of the scan are no keypoints: a half-empty ball has an anisotropic scatter matrix wherever it lies.
 *   NORMALS.  normals_nxyzc: the cloud's normals, n float4 as icpgpu_normal_estimation returns them; or NULL with normal_radius > 0
 *   (finite): exactly what icpgpu_normal_estimation(NULL, n, k = 0, normal_radius, viewpoint NULL) returns, computed and kept on the
 *   device.  NULL normals with a normal_radius that is not > 0 is ICPGPU_ERR_INVALID_ARG.
 *   EDGE.  edge[i] = 1 iff point i is finite, its border ball (d2 < (float)(border_radius * border_radius): the cloud's own radius row)
 *   holds at least min_neighbors points, and the boundary rule of the section "boundary estimation" on that row, with the normal n_i
 *   and angle_threshold, says 1 (so the row also holds at least 3).  The kernel is icpgpu_boundary_estimation's.
 *   BORDER.  border[i] = 1 iff point i is finite and some j in its border ball, itself included, has edge[j] = 1.
 *   A border point is skipped as PCL skips it: its scatter6, eigenvalues3 and saliency are zeros; n_salient[i] is still the size of
 *   its salient ball.  Non-maxima suppression, the count and icpgpu_iss_fetch are unchanged; icpgpu_iss_fetch serves either compute
 *   call.  icpgpu_iss_fetch_border copies out edge and border (n int32 each, either may be NULL); after icpgpu_iss_keypoints, or with
 *   border_radius == 0, both are zeros.
 *   border_radius == 0 gives icpgpu_iss_keypoints' result bit for bit; normals, normal_radius and angle_threshold are then ignored.
 *   Refused (ICPGPU_ERR_INVALID_ARG): a border_radius that is negative or not finite; with border_radius > 0, an angle_threshold that
 *   is not finite or outside (0, pi].  The border radius's neighbours beyond INT32_MAX in all: ICPGPU_ERR_UNSUPPORTED.
 *   HOST WAITS, as icpgpu_iss_stats reports them: border_radius == 0: one (the count).  Normals given: two (the totals that size the
 *   border radius's rows, the count).  Normals computed: three (the totals of the normal radius's rows as well).
 *   MEMORY.  The border path materialises the border radius's rows (and the normal radius's): it is O(n + neighbours), not O(n).
 * Not provided: setIndices, and a search surface other than the input (PCL indexes input_ with surface_'s indices and is only
 * meaningful when the two are one cloud).
 * ISOLATION.  The result depends on the search cloud and the arguments alone.  Both compute calls leave the
 * source, the target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud as
 * they were.  Unfetched clustering, segmentation and sample-consensus results survive them, and their own result -- edge and border
 * included -- survives searches, normal, FPFH and boundary estimations, clusterings and segmentations: the border path's rows go
 * through the search calls' scratch, everything it keeps lives in the ISS state's own buffers.  icpgpu_search_set_input drops it,
 * whatever it returns. */
int icpgpu_iss_keypoints(icpgpu_ctx* ctx, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                         int min_neighbors, size_t* n_keypoints);
int icpgpu_iss_fetch(icpgpu_ctx* ctx, size_t capacity_keypoints, int32_t* keypoint_index /* n_keypoints */,
                     float* keypoints_xyzw /* n_keypoints float4 */, int32_t* n_salient /* n */, double* scatter6 /* n x 6 */,
                     double* eigenvalues3 /* n x 3 */, double* saliency /* n */);
int icpgpu_iss_stats(const icpgpu_ctx* ctx, int32_t* host_waits);
int icpgpu_iss_keypoints_border(icpgpu_ctx* ctx, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                                int min_neighbors, double border_radius, double angle_threshold,
                                const float* normals_nxyzc /* n float4 or NULL */, double normal_radius, size_t* n_keypoints);
int icpgpu_iss_fetch_border(icpgpu_ctx* ctx, int32_t* edge /* n, may be NULL */, int32_t* border /* n, may be NULL */);

/* ---- moving least squares (added under 1.2) ------------------------------------------------------------------------- */
/* replaces pcl::MovingLeastSquares<PointXYZ, PointNormal> (PCL 1.8, surface/impl/mls.hpp) with UpsamplingMethod NONE: setInputCloud,
 * setSearchRadius, setPolynomialOrder / setPolynomialFit, setSqrGaussParam, setComputeNormals, process, getCorrespondingIndices --
 * "every point moved onto a weighted polynomial fitted to its radius neighbourhood, the normal taken from the fit", the stage in front
 * of icpgpu_normal_estimation on a scan with range noise.  The context's SEARCH CLOUD (icpgpu_search_set_input) is the surface.
 * queries_xyzw == NULL means the search cloud's own points, in their order (n_q must then be 0 or n): PCL's case.  Given queries are
 * projected onto the cloud's surface; PCL has no spelling for this.  Parity with PCL binaries is unpinned; tests/mls_restated.py is
 * what the kernels are compared with, bit for bit.  Every operation below is a float64 IEEE operation rounded on its own (no fused
 * multiply-add), in the order written; float32 inputs are widened first.
 * ARGUMENTS.  radius is finite and > 0.  order is in 0 .. ICPGPU_MLS_MAX_ORDER; orders 0 and 1 mean the plane projection alone
 * (setPolynomialFit(false), and later PCL's "order > 1" rule).  sqr_gauss_param -- s below -- is 0 or finite and > 0; 0 means radius *
 * radius, PCL's default.  out_nxyzc may be NULL (setComputeNormals(false)).  ICPGPU_ERR_INVALID_ARG: anything else; no search cloud;
 * null queries with n_q neither 0 nor n; with n_q > 0 a null out_xyzw, out_index or n_out.  n_q = 0 is ICPGPU_OK with *n_out = 0.
 * The rows' entries beyond INT32_MAX in all: ICPGPU_ERR_UNSUPPORTED, as for the other consumers of rows.
 * ROW.  The row of query i is icpgpu_search_radius(radius, max_nn = 0)'s row, the same set in the same order: the finite cloud points
 * with d2 < r2, strict, r2 = (float)(radius * radius), ascending by (d2, index).  m is its length, j_0 its first entry.  A non-finite
 * query has an empty row.
 * WSUM.  Every sum over a row is taken by one rule.  Entry t, counted from 0 in row order, is added into partial t mod 64; the 64
 * partials start at +0.0 and each takes its entries in ascending t.  Then, for mask = 32, 16, 8, 4, 2, 1, every partial l becomes
 * partial[l] + partial[l ^ mask], all 64 at once.  The sum is partial 0 (all 64 hold the same bits: IEEE addition commutes).
 * PLANE (needs m >= 3).  K = cloud point j_0.  Per entry d = q - K per component, q the entry's cloud point.  Nine WSUMs in the order of
 * normal estimation's a0 .. a8 -- dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz -- each divided by (double)m.  Covariance:
 * xx = a0 - a6 a6, xy = a1 - a6 a7, xz = a2 - a6 a8, yy = a3 - a7 a7, yz = a4 - a7 a8, zz = a5 - a8 a8.  Centroid c = (a6 + K.x,
 * a7 + K.y, a8 + K.z).  The cyclic Jacobi of normal estimation (8 sweeps, the same expressions) runs on the covariance; lambda_min is
 * the smallest diagonal entry, the lowest index among equals, and the plane's normal N that column of the eigenvector matrix, kept in
 * double.  tr = (xx + yy) + zz; curvature = tr != 0 ? fabsf((float)(lambda_min / tr)) : 0.  With P the query and e = P - c:
 * dist = (e.x N.x + e.y N.y) + e.z N.z, and Q = P - dist N per component is the query's projection onto the plane.
 * DEVIATION: PCL takes the moments about the centroid in two passes and decomposes with eigen33.
 * FRAME (Eigen's unitOrthogonal).  If |N.x| > 1e-12 |N.z| or |N.y| > 1e-12 |N.z|: inv = 1 / sqrt(N.x N.x + N.y N.y), V = (-N.y inv,
 * N.x inv, 0).  Otherwise inv = 1 / sqrt(N.y N.y + N.z N.z), V = (0, -N.z inv, N.y inv).  U = N x V: (N.y V.z - N.z V.y, N.z V.x -
 * N.x V.z, N.x V.y - N.y V.x).
 * FIT (when order >= 2 and m >= nc = (order + 1)(order + 2) / 2).  Per entry: de = q - Q; dd = (de.x de.x + de.y de.y) + de.z de.z;
 * w = EXP_NEG((-dd) / s); u = de . U, v = de . V, f = de . N, a dot being (x x' + y y') + z z'.  The monomials come in PCL's order --
 * for ui in 0 .. order: for vi in 0 .. order - ui: P_j = u^ui v^vi -- the powers made by repeated multiplication from 1.0 (u^3 =
 * ((1 u) u) u) and P_j their product; for order 2 that is 1, v, v^2, u, u v, u^2.  pw_a = P_a w.  A_ab = WSUM(pw_a P_b) for b <= a;
 * b_a = WSUM(pw_a f).  DEVIATION: PCL rounds dd to float32 first and calls libm's exp.
 * EXP_NEG(a), a <= 0.  NaN stays NaN; a < -708.0 gives 0.0.  Otherwise k = rint(a * 0x1.71547652b82fep+0); r = (a - k *
 * 0x1.62e42feep-1) - k * 0x1.a39ef35793c76p-33; p = c_13, then p = p * r + c_n for n = 12 .. 0, c_n the double nearest 1 / n!; the
 * result is ldexp(p, (int)k).  No libm exp: within 1 ulp of a correctly rounded one on [-708, 0], and EXP_NEG(0) = 1.
 * SOLVE (A c = b by Cholesky).  For j = 0 .. nc - 1: s = A_jj, then s = s - L_jk L_jk for k < j ascending, L_jj = sqrt(s); for i > j:
 * s = A_ij, then s = s - L_ik L_jk for k < j ascending, L_ij = s / L_jj.  Forward, for i = 0 .. nc - 1: s = b_i, then s = s - L_ik y_k
 * for k < i ascending, y_i = s / L_ii.  Backward, for i = nc - 1 .. 0: s = y_i, then s = s - L_ki c_k for k > i ascending, c_i = s /
 * L_ii.  Nothing is special-cased: a pivot that is not positive yields the NaN or infinity the arithmetic yields (a NaN's sign
 * and payload are the processor's, not the rule's).
 * RESULT.  status: 0 dropped (m < 3); 1 plane only (order 0 or 1, or m < nc); 2 polynomial; 3 fit refused.  When the fit ran and c_0
 * is finite the status is 2, the point is Q + c_0 N and the normal (N - c_(order+1) U) - c_1 V, per component -- NOT normalised or
 * oriented: PCL 1.8's NONE branch.  Otherwise the fit's status is 3, PCL's pcl_isfinite(c_vec[0]) rule.  With status 1 and 3 the
 * point is Q and the normal N.
 * OUTPUT.  The kept queries are those with status != 0, in query order.  out_xyzw: their points rounded to float32, w = 1.
 * out_nxyzc: {nx, ny, nz, curvature}, the normal rounded to float32.  out_index: the query's index (PCL's
 * corresponding_input_indices).  *n_out: their number.  The caller's arrays hold n_q entries; nothing is written past n_out.
 * icpgpu_mls_fetch returns the last call's per-query record, any number of times; each pointer may be NULL: status and n_neighbours
 * (m), n_q entries each; plane7 = {N.x, N.y, N.z, c.x, c.y, c.z, lambda_min}, NaN at status 0; coeff10 = c_0 .. c_(nc-1), then NaN
 * up to 10, and all NaN unless the fit ran.  Without a result (none computed, the last call refused, or the search cloud replaced
 * since) or with capacity < n_q the fetch returns ICPGPU_ERR_INVALID_ARG and writes nothing.  icpgpu_mls_stats reports the host
 * waits of the last call, and is refused the same way without a result.
 * HOST WAITS.  Two: the totals that size the rows, then the results; the kept count travels with the results.  (n_q = 0: none.)
 * LIMITS.  A cloud the grid refuses and a radius of more than 8 grid cells are handled as in icpgpu_search_radius: the same bits.
 * MEMORY.  O(n_q + the rows' entries); the order-3 fit keeps 65 doubles per query on the device.
 * Not provided: upsampling methods (SAMPLE_LOCAL_PLANE, RANDOM_UNIFORM_DENSITY, VOXEL_GRID_DILATION, DISTINCT_CLOUD), setDilation*,
 * setIndices, getMLSResults (icpgpu_mls_fetch returns this library's record instead), and k-nearest neighbourhoods (PCL's MLS has
 * none either).
 * ISOLATION.  The answers depend on the search cloud and the arguments alone.  The call leaves the source, the
 * target, every grid, the covariances, the cached normals, the NDT cells, the filters' results and the search cloud as they were.
 * Unfetched clustering, segmentation, sample-consensus and ISS results survive it, and its own record survives searches, normal,
 * FPFH and boundary estimations, clusterings, segmentations, sample-consensus alignments and ISS calls: the rows go through the
 * search calls' scratch, everything it keeps lives in buffers of its own.  icpgpu_search_set_input drops it, whatever it returns. */
#define ICPGPU_MLS_MAX_ORDER 3
int icpgpu_moving_least_squares(icpgpu_ctx* ctx, const float* queries_xyzw /* n_q float4 or NULL */, size_t n_q, double radius, int order,
                                double sqr_gauss_param, float* out_xyzw /* n_q float4 */, float* out_nxyzc /* n_q float4, may be NULL */,
                                int32_t* out_index /* n_q */, size_t* n_out);
int icpgpu_mls_fetch(icpgpu_ctx* ctx, size_t capacity /* >= n_q */, int32_t* status /* n_q */, int32_t* n_neighbours /* n_q */,
                     double* plane7 /* n_q x 7 */, double* coeff10 /* n_q x 10 */);
int icpgpu_mls_stats(const icpgpu_ctx* ctx, int32_t* host_waits);

/* ---- cropping and sampling filters (added under 1.2) ---------------------------------------------------------------- */
/* replaces pcl::PassThrough<PointXYZ>, pcl::CropBox<PointXYZ>, pcl::UniformSampling<PointXYZ> (PCL 1.8) and
 * pcl::FarthestPointSampling<PointXYZ> (PCL 1.12): the filters that keep a SUBSET OF THE INPUT ROWS -- what a LIDAR front end runs
 * before the voxel filter (range, height, the vehicle's own body) and what picks the points descriptors are computed at.  The rules
 * below restate PCL; parity with PCL binaries is unpinned (tests/sampling_restated.py is what the kernels are compared with, bit for
 * bit).
 * COMMON.  Every call takes a host cloud (n float4), uploads it into a buffer of this section's own and writes the kept rows, w
 * carried through, into the pinned staging buffer.  out_xyzw must hold n rows (n_samples for the farthest point sampling) or be
 * NULL (the count alone); a _view form hands out a view of the staging buffer under the outlier filters' view rule: valid until the
 * context's next call, NULL for an empty result.  n = 0 is ICPGPU_OK with an empty result; n > INT32_MAX - 4096 is
 * ICPGPU_ERR_INVALID_ARG.  A row is finite when x, y and z are.  A NON-FINITE ROW IS NEVER KEPT by any of the four, in either mode:
 * PCL's behaviour for PassThrough and CropBox -- and NOT icpgpu_sac_extract's, whose negative mode returns every row outside the
 * inliers, non-finite ones included.  One host wait per call (none for an empty result).
 * PASS THROUGH (field, lo, hi, negative; PCL's defaults: no field, FLT_MIN, FLT_MAX, false).  field 0, 1, 2 = x, y, z; field -1 is
 * PCL's empty field name: only the non-finite rows are removed and `negative` is ignored.  With v the field's float, a finite row
 * is removed when (!negative && (v < lo || v > hi)) || (negative && v >= lo && v <= hi): float32 comparisons, both ends inclusive,
 * as in PCL 1.8's applyFilterIndices.  lo > hi is legal and keeps nothing in positive mode.  A NaN limit or another field is
 * ICPGPU_ERR_INVALID_ARG; infinite limits are legal.
 * CROP BOX (min3, max3, T, negative).  q = p without T; with T (16 floats, column-major, as everywhere in this header) q is
 * xform_point's three fma chains, the arithmetic of icpgpu_transform.  A finite row is outside iff q.a < min.a or q.a > max.a on an
 * axis -- a NaN q (an infinite entry of T) is therefore INSIDE, as PCL's comparisons make it.  Positive mode keeps the inside rows,
 * negative mode the outside ones.  A NaN corner is ICPGPU_ERR_INVALID_ARG.  icpgpu_crop_box_matrix (host only) composes what PCL's
 * CropBox applies in three float steps -- the user transform, the translation, the inverse of the rotation -- into that one matrix:
 * M = R^-1 * Tr(-translation) * transform with R = Rz(rotation.z) * Ry(rotation.y) * Rx(rotation.x), pcl::getTransformation's order,
 * R^-1 = R's transpose; (Rz Ry) Rx, Tr * transform and R^-1 * (Tr * transform) are 4 x 4 products in double, each entry added from
 * the left, and the result is rounded to float32 ONCE.  DEVIATION: PCL rounds after each of its three steps.
 * UNIFORM SAMPLING (leaf > 0, finite; else ICPGPU_ERR_INVALID_ARG).  inv = 1 / leaf in float32.  The lattice is the voxel filter's
 * plan (icpgpu_voxel_plan) over the finite rows' box: its min_b and div_b.  The plan's verdict without a finite point gives an empty
 * result; PCL's "leaf size is too small" verdict and the wrapped cell index are ICPGPU_ERR_UNSUPPORTED -- a stated DEVIATION: PCL's
 * UniformSampling has no such test and lets the index wrap.  The cell of a finite row is i_a = (int)floorf(p.a * inv), the cell's
 * centre c_a = ((float)i_a + 0.5f) * leaf, each operation rounded; d = p - c in float32 and d2 = fma(dz, dz, fma(dy, dy, dx * dx)).
 * Each occupied cell keeps the row with the smallest (d2 bits, index) key -- the search's 64-bit key: ties go to the lowest index.
 * The output is in ascending index order.  DEVIATIONS: PCL emits in unordered_map order; PCL 1.8's expression, as far as it could be
 * recalled without its source at hand, subtracts the cell's integer coordinates instead of its centre -- the rule here is the one
 * PCL's own comment names, "closer to the leaf center".  More than 2^30 rows: ICPGPU_ERR_UNSUPPORTED (the cell table's index).
 * FARTHEST POINT SAMPLING (n_samples, first_index: setSample and the first point).  m[i] = +inf for every finite row; non-finite
 * rows take no part.  s_0 = first_index, or the lowest finite row with first_index = -1.  For j = 1 .. n_samples - 1: every
 * unselected finite i takes m[i] = min(m[i], d2(i, s_(j-1))) with the outlier filters' d2, and s_j is the unselected finite row
 * with the largest m, ties to the lowest index -- so duplicates of selected points come last, lowest index first.  The output and
 * the kept indices are in SELECTION order.  n_samples = 0 is ICPGPU_OK and empty; n_samples above the number of finite rows (PCL
 * throws there), a first_index outside the cloud or one that names a non-finite row is ICPGPU_ERR_INVALID_ARG.  DEVIATIONS: squared
 * distances instead of distances (the square root can merge two distinct d2 into a tie); the first point is an argument, not
 * mt19937's draw; n_samples == n is still returned in selection order.  Two kernel shapes compute the same bits: one workgroup that
 * runs all samples in one launch for n <= ICPGPU_FPS_ONE_WORKGROUP_MAX, one launch per sample over many workgroups above it;
 * icpgpu_subset_stats says which ran.
 * OBSERVERS of the LAST call of this section on the context; a refused call leaves nothing to observe (ICPGPU_ERR_INVALID_ARG).
 * icpgpu_subset_fetch: the kept rows' indices -- ascending for the crops and the uniform sampling, in selection order for the
 * farthest point sampling -- and one float per kept row: uniform sampling, the row's d2 to its cell's centre; farthest point
 * sampling, the row's d2 to the already selected set when it was chosen, +inf for the first; the crops, 0.  *n_in and *n_kept are
 * always set; either output may be NULL, with both NULL the call only reports the sizes; nothing is written when n_kept exceeds
 * capacity (ICPGPU_ERR_INVALID_ARG).  icpgpu_subset_removed: the complement, ascending (getRemovedIndices), under the same
 * capacity rule.  icpgpu_subset_stats: kind (ICPGPU_SUBSET_*), the call's host waits and kernel launches, and path
 * (ICPGPU_FPS_PATH_*; 0 for the other filters) -- a silent fall-back cannot pass as agreement.
 * ISOLATION.  The calls read nothing but their arguments.  They leave the source, the target, every grid, the
 * covariances, the normals, the NDT cells, the voxel and outlier filters' results, the search cloud and every unfetched clustering,
 * segmentation, ground filter, ISS and MLS result as they were; their own result survives all of those calls and is replaced only
 * by the next call of this section.
 * Not provided: setKeepOrganized / setUserFilterValue, setIndices, RandomSample, NormalSpaceSampling, CovarianceSampling, and a
 * crop fused into icpgpu_set_source_voxel_filtered. */
#define ICPGPU_FPS_ONE_WORKGROUP_MAX 16384
#define ICPGPU_SUBSET_PASS_THROUGH 1
#define ICPGPU_SUBSET_CROP_BOX 2
#define ICPGPU_SUBSET_UNIFORM_SAMPLING 3
#define ICPGPU_SUBSET_FARTHEST_POINT_SAMPLING 4
#define ICPGPU_FPS_PATH_ONE 1
#define ICPGPU_FPS_PATH_MANY 2
int icpgpu_pass_through(icpgpu_ctx* ctx, const float* xyzw, size_t n, int field, float lo, float hi, int negative, float* out_xyzw,
                        size_t* n_out);
int icpgpu_pass_through_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, int field, float lo, float hi, int negative,
                             const float** view_xyzw, size_t* n_out);
int icpgpu_crop_box(icpgpu_ctx* ctx, const float* xyzw, size_t n, const float* min3, const float* max3,
                    const float* T /* 16 floats or NULL */, int negative, float* out_xyzw, size_t* n_out);
int icpgpu_crop_box_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, const float* min3, const float* max3,
                         const float* T /* 16 floats or NULL */, int negative, const float** view_xyzw, size_t* n_out);
int icpgpu_crop_box_matrix(const float* transform16 /* NULL = identity */, const float* translation3, const float* rotation3,
                           float* out16);
int icpgpu_uniform_sampling(icpgpu_ctx* ctx, const float* xyzw, size_t n, float leaf, float* out_xyzw, size_t* n_out);
int icpgpu_uniform_sampling_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, float leaf, const float** view_xyzw, size_t* n_out);
int icpgpu_farthest_point_sampling(icpgpu_ctx* ctx, const float* xyzw, size_t n, size_t n_samples, int64_t first_index,
                                   float* out_xyzw, size_t* n_out);
int icpgpu_farthest_point_sampling_view(icpgpu_ctx* ctx, const float* xyzw, size_t n, size_t n_samples, int64_t first_index,
                                        const float** view_xyzw, size_t* n_out);
int icpgpu_subset_fetch(icpgpu_ctx* ctx, size_t capacity, int32_t* kept_index, float* measure, size_t* n_in, size_t* n_kept);
int icpgpu_subset_removed(icpgpu_ctx* ctx, size_t capacity, int32_t* removed_index, size_t* n_removed);
int icpgpu_subset_stats(const icpgpu_ctx* ctx, int32_t* kind, int32_t* host_waits, int32_t* launches, int32_t* path);

/* ---- the mapper's target: a one-point-per-voxel map and its "nn cloud"  -------- */
/* replaces OctreeMapper's pcl::octree::OctreePointCloudSearch map
 * (/root/reference/src/icpslam/octree_mapper.cpp:55-59 resetMap, :62-69 addPointsToMap,
 *  :72-90 approxNearestNeighbors, :133-172 refineTransformAndGrowMap; octree_resolution_ 0.5 m, :41).
 * The map belongs to the context and lives in HBM.
 *   reset        resetMap(): empty map with voxel size `resolution` (> 0).
 *   add_points   addPointsToMap(transformCloudToPoseFrame(cloud, pose)): p = pose * x (float, the a6
 *                contract); going through the points IN ORDER, p is appended to the map iff its voxel
 *                holds no point yet.  Voxels are the cells floor((p - origin) / resolution) (double) of
 *                the lattice whose origin is (first point ever added) - resolution -- PCL's octree
 *                bounding-box rule (first box p +- resolution / 2, widened to 2 voxels by getKeyBitSize).  Non-finite points are skipped.  pose NULL = identity.
 *   add_source   the same for the context's current source cloud (already in HBM).
 *   nn_target    approxNearestNeighbors + transformCloudToPoseFrame(.., raw_pose.inverse()) + setInputTarget:
 *                for every source point s (in order) the map point nearest to pose * s -- EXACT, lowest map
 *                index among equals, where PCL's approxNearestSearch is a heuristic -- moved by pose_inv,
 *                becomes the context's TARGET cloud (device to device).  Source points whose image is not
 *                finite are dropped, like the reference's "result_index < 0".  nn_out_xyzw (nullable) must
 *                hold n_source points; *n_nn = points in the nn cloud.  An empty map gives an empty target. */
/*   set_search   which neighbour nn_target collects: ICPGPU_MAP_SEARCH_EXACT (default, above) or ICPGPU_MAP_SEARCH_PCL_APPROX =
 *                what octree_mapper.cpp:84 literally calls, OctreePointCloudSearch::approxNearestSearch: from the root of
 *                PCL's octree (bounding box grown point by point as adoptBoundingBoxToPoint does) to the existing child
 *                whose voxel centre is nearest to the query (float squared distance, first child on ties), down to a leaf,
 *                whose point is returned -- a heuristic that misses the true neighbour for ~40 % of a scan's points.
 *                The exact search gives the better registration; this one restates the reference's own search (octree
 *                geometry per PCL 1.8's adoptBoundingBoxToPoint + getKeyBitSize; like every PCL restatement here it is
 *                unpinned against a PCL build). */
enum { ICPGPU_MAP_SEARCH_EXACT = 0, ICPGPU_MAP_SEARCH_PCL_APPROX = 1 };
int icpgpu_map_set_search(icpgpu_ctx* ctx, int mode);
int icpgpu_map_reset(icpgpu_ctx* ctx, double resolution);
int icpgpu_map_add_points(icpgpu_ctx* ctx, const float* xyzw, size_t n, const float* pose, size_t* n_added);
int icpgpu_map_add_source(icpgpu_ctx* ctx, const float* pose, size_t* n_added);
int icpgpu_map_size(icpgpu_ctx* ctx, size_t* n);
int icpgpu_map_get_points(icpgpu_ctx* ctx, float* out_xyzw, size_t capacity, size_t* n);
int icpgpu_map_nn_target(icpgpu_ctx* ctx, const float* pose, const float* pose_inv, float* nn_out_xyzw, size_t* n_nn);

/* ---- the data contract after the path: pose chain, keyframes, pose graph ---- */
/* SE(3) pose as the reference's Pose6DOF keeps it (/root/reference/include/utils/pose6DOF.h):
 * position + unit quaternion (x, y, z, w). Host-only arithmetic in double; no GPU involved. */
typedef struct {
  double pos[3];
  double quat[4]; /* x, y, z, w */
} icpgpu_pose;
typedef struct icpgpu_posegraph icpgpu_posegraph; /* opaque */

/* Pose6DOF(T): pose6DOF.cpp:185-190 (T = float[16] column-major as returned in icpgpu_result.T). */
int icpgpu_pose_from_matrix(const float* T, icpgpu_pose* out);
/* Pose6DOF::compose (operator+): pose6DOF.cpp:98-105.  Pose6DOF::inverse: pose6DOF.cpp:117-122. */
/* Pose6DOF::toTFTransform -> the Matrix4f pcl_ros::transformPointCloud applies (pose6DOF.cpp:254-259): column-major float */
int icpgpu_pose_to_matrix(const icpgpu_pose* p, float* T);
int icpgpu_pose_compose(const icpgpu_pose* a, const icpgpu_pose* b, icpgpu_pose* out);
int icpgpu_pose_inverse(const icpgpu_pose* a, icpgpu_pose* out);

/* Sequence bookkeeping of IcpOdometer::updateICPOdometry (icp_odometer.cpp:109-113) + the keyframe and
 * edge rules of IcpSlam::mainLoop / addNewKeyframe (icpslam.cpp:143-152, 70-89).
 *   keyframe_distance  : KFS_DIST_THRESH (icpslam.h:36, 0.3 m); < 0 = default
 *   information_diag6  : icp_information_matrix (config/icpslam.yaml:21); NULL = that default */
int icpgpu_posegraph_create(icpgpu_posegraph** out, double keyframe_distance, const double* information_diag6);
int icpgpu_posegraph_destroy(icpgpu_posegraph* g);
int icpgpu_posegraph_set_initial_pose(icpgpu_posegraph* g, const icpgpu_pose* p); /* IcpOdometer::setInitialPose */
/* one registration result per scan, in scan order. accepted = hasConverged() && fitness < 20
 * (icp_odometer.cpp:201); rejected scans leave the chain untouched. *keyframe_id = new keyframe or -1. */
int icpgpu_posegraph_push(icpgpu_posegraph* g, const float* T, int accepted, long* keyframe_id);
long icpgpu_posegraph_num_poses(const icpgpu_posegraph* g);
long icpgpu_posegraph_num_keyframes(const icpgpu_posegraph* g);
int icpgpu_posegraph_get_pose(const icpgpu_posegraph* g, long i, icpgpu_pose* out);
int icpgpu_posegraph_get_keyframe(const icpgpu_posegraph* g, long i, icpgpu_pose* out, long* scan_index);
/* edge measurement between keyframe new_kf and new_kf - 1: new^-1 (+) prev (icpslam.cpp:82). */
int icpgpu_posegraph_get_edge(const icpgpu_posegraph* g, long new_kf, icpgpu_pose* out);
/* g2o text file: VERTEX_SE3:QUAT id x y z qx qy qz qw / EDGE_SE3:QUAT from to x y z qx qy qz qw + the 21
 * upper-triangular information entries -- what PoseGraphG2O::addSe3Node/addSe3Edge would have built. */
int icpgpu_posegraph_write_g2o(const icpgpu_posegraph* g, const char* path);

/* ---- measurement ---------------------------------------------------------------------------- */
/* time one correspondence sweep in `every` (default 13, coprime with the reference's 10 / 30 iterations; 1 = every sweep).
 * Average kernel durations are *_ms / *_timed. */
int icpgpu_profile_set_sampling(icpgpu_ctx* ctx, int every);
int icpgpu_profile_reset(icpgpu_ctx* ctx);
int icpgpu_profile_get(icpgpu_ctx* ctx, icpgpu_profile* out);
/* stream handle (hipStream_t as void*) so a host can order its own work against the context. */
int icpgpu_get_stream(icpgpu_ctx* ctx, void** out_stream);
int icpgpu_synchronize(icpgpu_ctx* ctx);
/* Counting runs (bench.py's useful-flop figure; process-wide, one context at a time): with enable != 0 every grid
 * correspondence sweep (nn_quad_kernel) adds the number of target points it evaluates to a device counter;
 * icpgpu_count_candidates_read waits for the stream and returns the count since it was enabled (or last read), then
 * zeroes it.  Not for production: one atomic per wave. */
int icpgpu_count_candidates(icpgpu_ctx* ctx, int enable);
int icpgpu_count_candidates_read(icpgpu_ctx* ctx, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ICPGPU_H */
