/*
 * ba.h — C-ABI of libmiba, the MI355X-native windowed bundle-adjustment solver.
 *
 * This is the drop-in boundary for the reference's hot path
 *
 *   bool windowOptimize(ceresGlobalProblem&, int kf_i, int kf_f,
 *                       vector<KeyFrame>&, Map3D&,
 *                       const Vector4d& intrinsics_initial,
 *                       Vector4d& intrinsics_optimized);
 *     declared  /root/reference/headers/OptimizationUtils.h:55
 *     defined   /root/reference/src/OptimizationUtils.cpp:215-313
 *
 * whose entire compute is `ceres::Solve(globalProblem.options, &problem, &summary)`
 * (src/OptimizationUtils.cpp:300) over the residual blocks built at :236-294.
 * The caller (a host adapter, see INTEGRATION.md and include/ba_window.hpp)
 * flattens the window into the SoA `ba_problem` below, calls ba_solve(), and
 * maps the results back (reference :303-310).
 *
 * Conventions
 *  - Plain C types only; every pointer is a caller-owned HOST buffer.
 *  - Poses use Sophus::SE3d storage order [qx,qy,qz,qw,tx,ty,tz]
 *    (reference headers/sophus/se3.hpp:469-479), T_w_c (camera -> window frame).
 *  - Updated in place: cams, points, intr (reference mutates T_w_c, map points
 *    and intrinsics_optimized in place, OptimizationUtils.cpp:248,274,236).
 *  - Return value: 0 = ok, <0 = error (see BA_E_*); ba_last_error() has text.
 *    The reference has no error convention (always returns true, :312); a
 *    Ceres-level failure (e.g. initial evaluation non-finite) is reported in
 *    ba_summary.termination_type exactly as Ceres would, with return 0.
 *  - One context per host thread; contexts cache device buffers across calls
 *    (the reference re-optimizes the same window repeatedly, main.cpp:163-168).
 */
#ifndef MIBA_BA_H
#define MIBA_BA_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version history:
 *   1  (rounds 1-5) ba_summary / ba_prepare_info without a size field; ba_prepare_info grew lin_path (r4),
 *      plan_device and tail (r5) under the same version.
 *   2  ba_summary and ba_prepare_info lead with `struct_size`: the caller sets it to sizeof() of ITS struct
 *      (BA_SUMMARY_INIT / BA_PREPARE_INFO_INIT), the library writes only that many bytes (fields a newer
 *      library added past the caller's size stay untouched) and rejects a size below the *_MIN_SIZE of this
 *      version with BA_E_INVALID.
 *   2, additive  ba_covariance with ba_cov_request / ba_cov_info (both sized structs); nothing else changed.
 *   2, additive  BA_LS_BLOCKED, a fourth value of ba_summary.linear_solver (wide co-visibility windows); no struct
 *                changed.
 *   2, additive  ba_residuals with ba_res_request / ba_res_info (both sized structs) and the BA_RES_* flags; nothing
 *                else changed.
 *   2, additive  ba_covisibility with ba_covis_request / ba_covis_info (both sized structs) and ba_solve_ordered;
 *                nothing else changed.
 *   2, additive  ba_set_constant_cameras (a set of constant poses beside fixed_cam), ba_local_window with
 *                ba_local_request / ba_local_info (both sized structs) and ba_solve_local; nothing else changed.
 *   2, additive  ba_localize with ba_loc_request / ba_loc_info (both sized structs): pose-only refinement of keyframes
 *                against a constant map; ba_options and everything else unchanged.
 *   2, additive  ba_refine_points with ba_pts_request / ba_pts_info (both sized structs): structure-only refinement of
 *                landmarks against constant keyframes; ba_options and everything else unchanged.
 *   2, additive  ba_pose_graph with ba_pg_problem, ba_pg_request / ba_pg_info (both sized structs): pose-graph
 *                optimisation of keyframe poses over relative-pose edges; ba_options and everything else unchanged.
 *   2, additive  ba_align with ba_align_problem, ba_align_request / ba_align_info (both sized structs): batched RANSAC
 *                relative pose from 3D-3D correspondences; ba_options and everything else unchanged.
 *   2, additive  ba_match with ba_match_problem, ba_match_request / ba_match_info (both sized structs): batched
 *                2-nearest-neighbour descriptor matching with the ratio test; everything else unchanged.
 *   2, additive  ba_guided_match with ba_gmatch_problem, ba_gmatch_request / ba_gmatch_info (both sized structs):
 *                descriptor search in a pixel window around projected landmarks; everything else unchanged. */
#define BA_API_VERSION 2

/* error codes */
#define BA_OK 0
#define BA_E_INVALID (-1)   /* bad argument / malformed problem */
#define BA_E_DEVICE (-2)    /* HIP runtime error / no device */
#define BA_E_NOMEM (-3)     /* allocation failed */
#define BA_E_COMM (-4)      /* RCCL / multi-device error */
#define BA_E_INTERNAL (-5)

/* Ceres 2.0 ceres::TerminationType values (types.h), mirrored numerically. */
#define BA_CONVERGENCE 0
#define BA_NO_CONVERGENCE 1
#define BA_FAILURE 2

/* Solver configuration.
 * Field-for-field mirror of ceresGlobalProblem
 * (/root/reference/headers/BundleAdjustmentConfig.h:44-69) plus the Ceres 2.0
 * Solver::Options defaults that the reference leaves untouched. */
typedef struct ba_options {
    /* ceresGlobalProblem constants, BundleAdjustmentConfig.h:47-50 */
    double hub_p_repr;         /* HUB_P_REPR = 1e-3: Huber a for reprojection blocks */
    double hub_p_unpr;         /* HUB_P_UNPR = 1e-3: Huber a for depth-prior blocks  */
    double weight_intrinsics;  /* WEIGHT_INTRINSICS = 1e-6 (IntrinsicsPrior weight)   */
    double weight_unpr;        /* WEIGHT_UNPR = 10 (depth prior weight numerator)     */
    /* Solver::Options set in initialize_options(), BundleAdjustmentConfig.h:61-67 */
    int32_t max_num_iterations;           /* 75 */
    int32_t minimizer_progress_to_stdout; /* 1 -> Ceres-style iteration table */
    double eta;                           /* 1e-6 (no effect on a direct Schur solve) */
    /* Ceres 2.0 defaults (not set by the reference) */
    double initial_trust_region_radius; /* 1e4  */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_relative_decrease;       /* 1e-3 */
    double min_lm_diagonal;             /* 1e-6 */
    double max_lm_diagonal;             /* 1e32 */
    int32_t max_num_consecutive_invalid_steps; /* 5 */
    int32_t jacobi_scaling;             /* 1 */
    double function_tolerance;          /* 1e-6 */
    double gradient_tolerance;          /* 1e-10 */
    double parameter_tolerance;         /* 1e-8 */
    /* MI355X execution knobs (no reference counterpart) */
    int32_t device;          /* HIP device ordinal for this context; -1 = current */
    int32_t deterministic;   /* 1 = fixed-order reductions only (no float atomics): bitwise-reproducible
                                solves (the Schur tiles write per-tile slabs summed in tile order; the
                                overflow Schur terms run in one workgroup), at some speed cost */
    int32_t profile_kernels; /* 1 = HIP-event timing of kernel launches (ba_kernel_stats) */
    int32_t profile_mask;    /* with profile_kernels: bit k selects kernel id k of ba_kernel_stats order; 0 = all */
    int32_t shard_min_obs;   /* landmark shards (ba_comm_init*): a window with fewer admissible observations
                                over all shards is gathered onto every rank at ba_prepare and solved there
                                alone (no per-iteration collectives, deterministic mode), each rank keeping
                                its own points; 0 = always run the sharded exchange. Default 262144 */
    int32_t small_window;    /* ignored: kept for layout compatibility (the round-2 single-workgroup small-window
                                kernel measured slower than the multi-launch path and was removed) */
    int32_t rebuild_plan;    /* 0 (default): ba_prepare / ba_solve reuse the context's host plan and device
                                structure when the window's structure is unchanged since the last prepare
                                (same sizes, fixed_cam, obs_cam, obs_pt, admissibility mask; the reference
                                re-optimises the same window every frame, main.cpp:163-168) and upload only the
                                parameters and the observation values that changed; 1 = rebuild every call.
                                Unsharded contexts only (landmark shards always rebuild) */
    int32_t reserved[1];
} ba_options;

/* One window, flattened. Mirrors what windowOptimize feeds to Ceres
 * (OptimizationUtils.cpp:236-294). Observations with depth <= 1e-15 are
 * skipped and excluded from the 1/N weight normaliser exactly like the
 * reference (countConstraints :184-213 and the skip at :265-268). */
typedef struct ba_problem {
    int32_t n_cams;
    int32_t n_points;
    int32_t n_obs;
    int32_t fixed_cam;        /* gauge: SetParameterBlockConstant(kf_i) (:299); -1 = none */
    double* cams;             /* [n_cams*7]  qx,qy,qz,qw,tx,ty,tz   (in/out) */
    double* points;           /* [n_points*3] (in/out) */
    double* intr;             /* [4] fx,fy,cx,cy (intrinsics_optimized, in/out) */
    const double* intr_prior; /* [4] intrinsics_initial (IntrinsicsPrior target, :238) */
    const int32_t* obs_cam;   /* [n_obs] camera index of each observation */
    const int32_t* obs_pt;    /* [n_obs] point index of each observation  */
    const double* obs_uv;     /* [n_obs*2] keypoint pixel (u,v)  (:262) */
    const double* obs_depth;  /* [n_obs] measured depth z (:261) */
} ba_problem;

/* Result summary (subset of ceres::Solver::Summary + per-phase device timings). */
/* ba_summary.linear_solver */
#define BA_LS_DENSE 0 /* dense-envelope LDS Cholesky */
#define BA_LS_BAND 1  /* banded LDS Cholesky (6x6 block band <= 6) */
#define BA_LS_BCR 2   /* block cyclic reduction over 64-dof camera blocks */
#define BA_LS_BLOCKED 3 /* multi-workgroup blocked Cholesky over 64-column blocks (wide co-visibility windows) */

typedef struct ba_summary {
    int32_t struct_size;            /* in: sizeof(ba_summary) of the caller's header (BA_SUMMARY_INIT) */
    int32_t reserved0;
    double initial_cost;
    double final_cost;
    int32_t num_successful_steps;   /* Ceres convention: includes iteration 0 */
    int32_t num_unsuccessful_steps;
    int32_t num_iterations;         /* LM steps computed = iterations after 0 */
    int32_t termination_type;       /* BA_CONVERGENCE / BA_NO_CONVERGENCE / BA_FAILURE */
    int32_t num_obs_admissible;     /* N of countConstraints */
    int32_t num_active_cams;
    int32_t num_active_points;
    int32_t reduced_system_size;    /* 6*active_cams + 4 */
    int32_t linear_solver;          /* reduced-system solver used: BA_LS_DENSE / _BAND / _BCR / _BLOCKED */
    int32_t camera_band;            /* max |cam_a - cam_b| over coupled active cameras */
    double time_setup_ms;           /* host prep + H2D + structure build */
    double time_lm_ms;              /* LM loop wall time (device work + host control) */
    double time_linearize_ms;       /* device: camera-side / point-side linearisation */
    double time_schur_ms;           /* device: Schur reduction over points */
    double time_factor_ms;          /* device: reduced camera system factor + solve */
    double time_update_ms;          /* device: back-substitution + candidate evaluation */
    double time_total_ms;
    char message[160];
} ba_summary;
/* the smallest struct_size ba_solve / ba_solve_prepared accept: every field before `message` */
#define BA_SUMMARY_MIN_SIZE ((int32_t)offsetof(ba_summary, message))
#define BA_SUMMARY_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))

/* Library / API identification. */
int32_t ba_api_version(void);
const char* ba_build_info(void);

/* Defaults = ceresGlobalProblem() + Ceres 2.0 defaults. */
void ba_default_options(ba_options* opts);

/* Context lifecycle. Returns NULL on failure (ba_last_error(NULL) explains). */
typedef struct ba_context ba_context;
ba_context* ba_create(const ba_options* opts);
void ba_destroy(ba_context* ctx);
/* Text of the context's last failed call; after a successful ba_solve / ba_solve_prepared it is empty, or a
 * note (e.g. LM iterations re-run with the per-level BCR launches after a resident-kernel hand-off timeout). */
const char* ba_last_error(const ba_context* ctx);
/* Replace the solver options of a live context (device buffers are kept;
 * opts->device must equal the context's device or be -1). */
int32_t ba_set_options(ba_context* ctx, const ba_options* opts);

/* Solve one window in place (the replacement of ceres::Solve at :300).
 * Equivalent to ba_prepare() followed by ba_solve_prepared(). summary->struct_size must be set
 * (BA_SUMMARY_INIT); min(struct_size, sizeof(ba_summary)) bytes are written. */
int32_t ba_solve(ba_context* ctx, ba_problem* prob, ba_summary* summary);

/* Split form of ba_solve for callers that re-solve a resident window:
 * ba_prepare() validates the window, builds the point-/camera-major orderings
 * and the reduced-system envelope on the host and uploads everything to HBM;
 * ba_solve_prepared() runs the LM loop on the resident window starting from the
 * parameters uploaded by the last ba_prepare() and writes the result into prob
 * (which must be the same window, same sizes). */
int32_t ba_prepare(ba_context* ctx, const ba_problem* prob);
int32_t ba_solve_prepared(ba_context* ctx, ba_problem* prob, ba_summary* summary);

/* What the last ba_prepare (or the prepare inside ba_solve / the debug hooks) did. */
typedef struct ba_prepare_info {
    int32_t struct_size;     /* in: sizeof(ba_prepare_info) of the caller's header (BA_PREPARE_INFO_INIT) */
    int32_t plan_reused;     /* 1: the window's structure matched the context's last plan (no plan rebuild) */
    int32_t obs_uploaded;    /* 1: observation values were uploaded (always on a rebuild; on a reuse only when
                                some pixel / depth value changed) */
    int32_t host_threads;    /* host plan threads (MIBA_HOST_THREADS, else min(16, OMP_NUM_THREADS, affinity)) */
    int32_t bcr_path;        /* reduced-solve path of the prepared window: 5 = narrow camera band (<= 3), the
                                whole system cyclic-reduced in one workgroup's LDS; 4 = one-block window, dense
                                single-workgroup solve; 3 / 2 = resident split kernel with two / one helper
                                workgroups per block, 1 = resident one-workgroup kernel, 0 = per-level launches,
                                -1 = not the block cyclic reduction (band / dense) */
    double compare_ms;       /* structure / value comparison against the last prepare (reuse check) */
    double plan_ms;          /* host plan build (0 on a reuse) */
    double upload_ms;        /* staging + enqueue of the uploads and the device gather */
    double total_ms;         /* the whole prepare, device work included */
    int32_t lin_path;        /* linearisation of the LM loop: 1 = small window, the point side inside the Schur
                                tiles and the camera side in the Schur launch (no separate linearisation launch);
                                0 = a linearisation launch before the Schur launch */
    int32_t plan_device;     /* 1: the window's plan passes ran on the device (MIBA_DEVICE_PLAN; 0 on a reuse) */
    int32_t tail;            /* 1: the band solve's launch also runs the point back-substitution and the LM
                                decision (bcr_path 5, small unsharded windows; MIBA_TAIL=0: separate launches) */
    int32_t bsfin;           /* 1: the point back-substitution and the LM decision run in one launch (larger
                                unsharded windows, k_backsub_final; opt-in, MIBA_BSFIN=1) — version 2 */
} ba_prepare_info;
/* the smallest struct_size ba_last_prepare accepts: the v2 layout through total_ms */
#define BA_PREPARE_INFO_MIN_SIZE ((int32_t)(offsetof(ba_prepare_info, total_ms) + sizeof(double)))
#define BA_PREPARE_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
/* Writes min(info->struct_size, sizeof(ba_prepare_info)) bytes; BA_E_INVALID below BA_PREPARE_INFO_MIN_SIZE. */
int32_t ba_last_prepare(const ba_context* ctx, ba_prepare_info* info);

/* Landmark sharding (one process per GPU). Every rank passes the SAME window
 * cameras, intrinsics, prior and fixed_cam to ba_solve / ba_prepare, and its OWN block of
 * landmarks (points with all their observations). Per LM iteration the ranks all-reduce
 * (RCCL over xGMI) the camera-side partials, the packed envelope of the reduced camera
 * system and the step scalars; every rank then runs the identical deterministic solve of
 * the reduced system, so poses and intrinsics stay bitwise identical across ranks and each
 * rank updates its own points. Rank 0 calls ba_comm_unique_id() and ships the id to the
 * other ranks (any host channel); then every rank calls ba_comm_init() collectively.
 * Sharding pays only when the per-rank point work exceeds the all-reduce time (a few
 * tens of us per iteration over xGMI): small windows should stay on one GPU. */
#define BA_COMM_ID_BYTES 128
int32_t ba_comm_unique_id(uint8_t id[BA_COMM_ID_BYTES]);
int32_t ba_comm_init(ba_context* ctx, int32_t nranks, int32_t rank, const uint8_t id[BA_COMM_ID_BYTES]);

/* The same landmark sharding over a caller-supplied host collective instead of RCCL (e.g. MPI,
 * or torch.distributed gloo in the multi-rank tests, where several ranks share one GPU and RCCL
 * refuses duplicate devices). fn reduces `count` elements of the host buffer `buf` in place across
 * the ranks and returns 0 on success (dtype BA_DTYPE_*, op BA_OP_*); libmiba calls it on the
 * thread running ba_solve, at the same points of the LM iteration as the RCCL collectives, with
 * the device data staged through pinned memory. Local (not collective): every rank calls it once. */
#define BA_DTYPE_F64 0
#define BA_DTYPE_I32 1
#define BA_OP_SUM 0
#define BA_OP_MAX 1
#define BA_OP_MIN 2
typedef int32_t (*ba_allreduce_fn)(void* buf, int64_t count, int32_t dtype, int32_t op, void* user);
int32_t ba_comm_init_host(ba_context* ctx, int32_t nranks, int32_t rank, ba_allreduce_fn fn, void* user);

/* Per-iteration log of the last solve, the rows Ceres prints with minimizer_progress_to_stdout
 * (iteration 0 .. num_iterations): cost, cost_change, |gradient|_inf, |step|, tr_ratio, tr_radius,
 * accepted (1 = successful step, 0 = unsuccessful / invalid, -1 = the step that met a tolerance),
 * 0. Returns the number of rows available (at most max_rows are written; rows may be NULL). */
#define BA_LOG_WIDTH 8
int32_t ba_iteration_log(const ba_context* ctx, double* rows, int32_t max_rows);

/* Per-kernel device timing (requires ba_options.profile_kernels = 1).
 * bytes_per_launch is the ALGORITHMIC traffic model of DESIGN.md §Roofline
 * for the last prepared window (compulsory bytes, each input/output once). */
typedef struct ba_kernel_stat {
    char name[32];
    int32_t launches;
    int32_t reserved;
    double total_ms;
    double bytes_per_launch;
    double flops_per_launch;
} ba_kernel_stat;
int32_t ba_kernel_stats(const ba_context* ctx, ba_kernel_stat* out, int32_t max_n); /* returns count */
void ba_reset_kernel_stats(ba_context* ctx);

/* ---- covariance of the estimate (the counterpart of ceres::Covariance) ----
 * Sigma = (J^T J)^-1 at prob's parameters, J the Jacobian the LM loop linearises with (sqrt(rho')-robustified, the
 * IntrinsicsPrior rows included, the gauge camera's columns and the cameras / points without an admissible
 * observation removed), in the tangent space of ba_debug_linearize: [upsilon(3), omega(3)] per camera applied as
 * T*exp(delta), 3 per point, 4 for fx, fy, cx, cy. No damping, no Jacobi scaling in the result. The residuals carry
 * the reference's 1/N weights, so Sigma is in the cost's units as Ceres' would be; ba_cov_info.variance_factor
 * reports 2 cost / (3 N + 4 - (6 nac + 3 nap + 4)) (0 when the denominator is <= 0) and is NOT applied.
 * Camera / intrinsics blocks are blocks of the inverse of the undamped reduced camera system (dense, on the device);
 * a point's 3x3 marginal is V^-1 + T^T Sigma[cols, cols] T, T = E V^-1, over the point's cameras and the intrinsics.
 * Behaves like the debug hooks: prepares the window (the plan cache applies) and evaluates at prob's parameters;
 * prob is not modified, and a following ba_solve / ba_solve_prepared behaves as if the call had not happened.
 * Blocks: a pair that involves the gauge camera is all zeros (a constant block); a camera or point without an
 * admissible observation is not estimable, its blocks are NaN (return code still 0); (a,b) and (b,a) are exact
 * transposes and a diagonal block is exactly symmetric. The system counts as rank deficient when a Cholesky pivot
 * is <= 0 or not finite or pivot_min / pivot_max < min_reciprocal_condition_number: the call returns 0 with
 * status = BA_COV_RANK_DEFICIENT and every requested output NaN. Contexts with landmark shards: BA_E_INVALID. */
#define BA_COV_INTR (-1)            /* the intrinsics block in pair_a / pair_b */
#define BA_COV_OK 0
#define BA_COV_RANK_DEFICIENT 1
typedef struct ba_cov_request {
    int32_t struct_size;            /* BA_COV_REQUEST_INIT */
    int32_t n_pairs;
    const int32_t* pair_a;          /* camera index of the window, or BA_COV_INTR */
    const int32_t* pair_b;
    double* pair_cov;               /* [n_pairs*36]: block k at 36*k, row-major dim(a) x dim(b), the rest 0 */
    int32_t n_points;               /* 0 = none */
    const int32_t* point_idx;       /* NULL with n_points == prob->n_points: every point, in order */
    double* point_cov;              /* [n_points*9] row-major 3x3 */
    double* full;                   /* optional [(6*nac+4)^2] row-major, ordered as ba_debug_reduced_system */
    double min_reciprocal_condition_number; /* <= 0: 1e-14, Ceres' Covariance::Options default */
} ba_cov_request;
typedef struct ba_cov_info {
    int32_t struct_size, status, n, nac;
    double pivot_min, pivot_max;    /* squared Cholesky diagonal of the Jacobi-scaled system */
    double cost, variance_factor;
    double time_build_ms, time_invert_ms, time_points_ms, time_total_ms;
} ba_cov_info;
#define BA_COV_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_cov_request))
#define BA_COV_INFO_MIN_SIZE ((int32_t)sizeof(ba_cov_info))
#define BA_COV_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_COV_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_covariance(ba_context* ctx, const ba_problem* prob, const ba_cov_request* req, ba_cov_info* info);

/* ---- residual report (the counterpart of ceres::Problem::Evaluate) ----
 * What every observation of the window is off by at prob's parameters, in physical units, which keyframes and
 * landmarks carry the error, and which observations are outliers against the caller's thresholds.
 * Per observation, in the caller's order: obs_err = du, dv [px] (projected minus measured pixel), depth - z and z (the
 * point's depth in the camera frame): the raw differences, without the 1/N weights and without the Huber corrector;
 * obs_cost = 0.5 rho_repr + 0.5 rho_unpr, the observation's share of the cost the LM loop minimises (weights and
 * Huber loss applied), the value the solver's candidate evaluation computes; obs_flags, the BA_RES_* bits. An
 * observation the solver skips (depth <= 1e-15) has NaN errors and cost and the flag BA_RES_INADMISSIBLE alone.
 * BA_RES_REPROJ compares sqrt(du^2 + dv^2), formed with IEEE multiply, add and square root, the value the maxima
 * report; BA_RES_DEPTH uses max(max_depth_abs, 0) + max(max_depth_rel, 0) * depth. Both tests are plain comparisons:
 * one with a NaN operand does not flag.
 * obs_depth_culled is prob->obs_depth with the BA_RES_OUTLIER observations set to 0: passed as obs_depth of the next
 * solve it makes the solver skip them (and N, the weights' normaliser, counts the rest).
 * Per block (cam_stats: every camera of the window, the gauge camera included; point_stats: every point), six values:
 *   [0] admissible observations   [1] of those, with a BA_RES_OUTLIER bit   [2] sum du^2 + dv^2
 *   [3] max sqrt(du^2 + dv^2)     [4] sum (depth - z)^2                       [5] sum obs_cost
 * [2], [3], [4] run over the block's projected observations (admissible and not BA_RES_BEHIND: a pixel that is not
 * finite stays out of the sums), [0], [1], [5] over all admissible ones. A block without an admissible observation is
 * all zeros. ba_res_info carries the same over the whole window: rms = sqrt(sum / projected count), 0 without a
 * projected observation; cost = sum obs_cost + prior_cost, the cost ba_debug_linearize reports.
 * Every sum has a fixed order (no floating-point atomics): the report is bitwise reproducible from call to call,
 * with ba_options.deterministic 0 or 1 and with the host or the device plan; the camera sums (and the totals formed
 * from them) follow the camera sub-segments (MIBA_SUBSEG), everything else does not depend on any setting.
 * Behaves like ba_covariance: prepares the window (the plan cache applies) and evaluates at prob's parameters; prob
 * is not modified, and a following ba_solve / ba_solve_prepared behaves as if the call had not happened. A window
 * without an admissible observation returns 0 with zero counts and cost = prior_cost. Contexts with landmark shards:
 * BA_E_INVALID. */
/* bits of obs_flags */
#define BA_RES_INADMISSIBLE 0x01 /* depth <= 1e-15: the solver skips it; its err / cost are NaN */
#define BA_RES_BEHIND       0x02 /* z <= 0 in the camera frame, or the projected pixel is not finite */
#define BA_RES_REPROJ       0x04 /* hypot(du, dv) > max_reproj_px */
#define BA_RES_DEPTH        0x08 /* |depth - z| > max_depth_abs + max_depth_rel * depth */
#define BA_RES_HUBER_REPR   0x10 /* reprojection block in Huber's linear zone (weighted s > a^2) */
#define BA_RES_HUBER_UNPR   0x20 /* depth-prior block in Huber's linear zone */
#define BA_RES_OUTLIER      (BA_RES_BEHIND | BA_RES_REPROJ | BA_RES_DEPTH)
#define BA_RES_ERR_N  4  /* du, dv [px] = projected - measured; depth - z; z (camera-frame depth) */
#define BA_RES_STAT_N 6  /* see above */
typedef struct ba_res_request {
    int32_t struct_size, reserved0;       /* BA_RES_REQUEST_INIT */
    double max_reproj_px;                 /* <= 0: no reprojection test */
    double max_depth_abs, max_depth_rel;  /* both <= 0: no depth test */
    double*  obs_err;          /* optional [n_obs * 4], original observation order */
    double*  obs_cost;         /* optional [n_obs]: 0.5 rho_repr + 0.5 rho_unpr, this observation's share of the cost */
    int32_t* obs_flags;        /* optional [n_obs] */
    double*  obs_depth_culled; /* optional [n_obs]: prob->obs_depth with the BA_RES_OUTLIER observations set to 0 */
    double*  cam_stats;        /* optional [n_cams * 6], every camera of the window, the gauge camera included */
    double*  point_stats;      /* optional [n_points * 6] */
} ba_res_request;
typedef struct ba_res_info {
    int32_t struct_size, n_admissible, n_outliers, n_behind, n_reproj, n_depth, n_huber_repr, n_huber_unpr;
    double cost, prior_cost;              /* cost = what ba_debug_linearize reports; prior_cost the IntrinsicsPrior share */
    double rms_reproj_px, max_reproj_px, rms_depth, max_depth;
    double time_eval_ms, time_total_ms;   /* the kernels (HIP events); the whole call, prepare and copies included */
} ba_res_info;
#define BA_RES_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_res_request))
#define BA_RES_INFO_MIN_SIZE ((int32_t)sizeof(ba_res_info))
#define BA_RES_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_RES_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_residuals(ba_context* ctx, const ba_problem* prob, const ba_res_request* req, ba_res_info* info);

/* ---- keyframe co-visibility and the camera ordering ----
 * The fast paths of the solver need co-visible cameras to be numbered close together, in active-camera index space:
 * the Schur tiles take a point whose cameras lie inside 12 consecutive active cameras, the block cyclic reduction a
 * camera_band below 10. A window numbered in time order that sees the scene more than once (global BA, a loop
 * closure, a hand-held sweep) falls off both although its co-visibility graph is as sparse as a sliding window's.
 * ba_covisibility reports that graph and an order of the cameras that narrows the band; ba_solve_ordered solves the
 * window in such an order.
 * weights: W[a][b] = the distinct points cameras a and b both see through admissible observations (depth > 1e-15),
 * W[a][a] = the distinct points a sees; an observation repeated for the same camera and point counts once; the gauge
 * camera is included. The input of a co-visibility-driven window selection.
 * order: order[k] = the camera of the window placed k-th. Reverse Cuthill-McKee over the active cameras (those with
 * an admissible observation, the gauge camera apart; an edge where W > 0): per connected component, from the
 * unvisited camera of lowest (degree, index) breadth-first, a camera's unvisited neighbours by (degree, index), the
 * component's list reversed; the components in the order they were started, then the gauge camera and the cameras
 * without an admissible observation in index order. The order is returned only if it narrows the band
 * (band_after < band_before) and sends no more points to the Schur stage's overflow path (wide_after <= wide_before);
 * otherwise the identity, order_changed = 0 and band_after / wide_after repeat the before values: a sliding window
 * keeps its numbering.
 * Stand-alone: validates the window as ba_prepare does, works on copies of obs_cam / obs_pt / obs_depth in device
 * buffers of its own and touches neither the context's plan nor its LM state: a ba_solve_prepared after it is bitwise
 * the solve without it. Integer arithmetic only: the report is bitwise reproducible. A window without an admissible
 * observation returns 0 with zero weights and the identity order. Contexts with landmark shards: BA_E_INVALID. */
typedef struct ba_covis_request {
    int32_t struct_size, reserved0;  /* BA_COVIS_REQUEST_INIT */
    int32_t* weights;                /* optional [n_cams * n_cams], row-major, symmetric */
    int32_t* order;                  /* optional [n_cams] */
} ba_covis_request;
typedef struct ba_covis_info {
    int32_t struct_size;
    int32_t n_active;                  /* cameras with an admissible observation, the gauge camera apart */
    int32_t n_edges;                   /* co-visible pairs of active cameras */
    int32_t n_components;              /* connected components of the active cameras' graph */
    int32_t band_before, band_after;   /* what ba_summary.camera_band is as given / would be in `order` */
    int32_t wide_before, wide_after;   /* points whose active cameras span more than 12 positions (overflow points) */
    int32_t order_changed;             /* 1: `order` is not the identity */
    int32_t reserved0;
    double time_count_ms;              /* the bit-matrix and weight kernels (HIP events) */
    double time_order_ms;              /* the ordering on the host and the span kernels */
    double time_total_ms;              /* the whole call, uploads and copies included */
} ba_covis_info;
#define BA_COVIS_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_covis_request))
#define BA_COVIS_INFO_MIN_SIZE ((int32_t)sizeof(ba_covis_info))
#define BA_COVIS_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_COVIS_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_covisibility(ba_context* ctx, const ba_problem* prob, const ba_covis_request* req, ba_covis_info* info);

/* ba_solve on the window with its cameras placed in `order` (a permutation of 0 .. n_cams-1, as ba_covisibility
 * returns it; NULL: computed by ba_covisibility first). The context keeps a shadow problem (the cameras permuted,
 * obs_cam and fixed_cam remapped; points, intrinsics and the other observation arrays are the caller's), runs
 * ba_solve on it and copies the cameras back to the caller's positions; points and intrinsics are updated in place
 * as usual. summary, ba_iteration_log, ba_last_prepare and the plan cache describe the ordered window: a repeat of
 * the same structure with the same order reuses the plan. Contexts with landmark shards: BA_E_INVALID. */
int32_t ba_solve_ordered(ba_context* ctx, ba_problem* prob, const int32_t* order, ba_summary* summary);

/* ---- constant cameras and the local window (local bundle adjustment) ----
 * is_constant[n_cams]: non-zero = the camera's pose is a constant parameter block in every later prepare on this
 * context (ba_prepare, ba_solve, ba_solve_ordered, the debug hooks, ba_covariance, ba_residuals), in addition to
 * prob->fixed_cam: ceres::Problem::SetParameterBlockConstant on several blocks. NULL or n_cams == 0 clears the set.
 * The mask is copied. A constant camera's observations stay admissible: they count in N, contribute to their points'
 * blocks and to the intrinsics and are part of the cost; its pose has no columns in the reduced system and comes back
 * bitwise as given; num_active_cams, reduced_system_size and camera_band describe the remaining cameras; a
 * ba_covariance pair that involves it is all zeros; ba_covisibility / ba_solve_ordered place it after the active
 * cameras as they place the gauge camera. Every camera constant is legal: the window is solved on its points and the
 * intrinsics. The mask is part of the plan-cache key (same mask: the plan is reused; changed mask: a new plan); the
 * host plan and the device plan (MIBA_DEVICE_PLAN) are built from it alike. A prepare whose n_cams differs from the
 * mask's returns BA_E_INVALID; so does one on a context with landmark shards while the set has a member. */
int32_t ba_set_constant_cameras(ba_context* ctx, const uint8_t* is_constant, int32_t n_cams);

/* ba_local_window selects, from a whole map given as a ba_problem, the window a local bundle adjustment around camera
 * `center` optimises (the local BA of ORB-SLAM-style back-ends). All of it is integer:
 *   w[a]  the distinct points cameras center and a both see through admissible observations (row `center` of
 *         ba_covisibility's weights, one and-popcount row of the camera x point bit matrix; w[center] = its points);
 *   L     the local cameras: center, plus every a with w[a] >= min_weight (<= 0: 1); if that exceeds max_local
 *         (<= 0: no cap), center and the max_local - 1 others of largest (w[a], -a): larger weight first, lower index
 *         on a tie;
 *   P     the local points: every point with an admissible observation in a camera of L;
 *   F     the fixed cameras: every camera outside L with an admissible observation of a point of P.
 * The sub-window: cameras L u F in increasing original index (cam_index; the map's numbering is kept, a sliding window
 * keeps its band), points P in increasing original index (pt_index), every admissible observation whose point is in
 * P, in the caller's order (obs_index; a stable compaction, inadmissible observations dropped), with its camera and
 * point renumbered (sub_obs_cam, sub_obs_pt). Constant in the sub-window (cam_constant): every camera of F, the map's
 * fixed_cam if it is in L u F, and the cameras of the context's constant set when one is set for the map's n_cams. If
 * that leaves nothing constant, the lowest camera of L is the sub-window's gauge (sub_fixed_cam, an index into
 * cam_index) and cam_constant is all zeros; otherwise sub_fixed_cam = -1.
 * Every output buffer is optional and sized by the caller for the worst case (n_cams, n_points, n_obs entries).
 * Stand-alone like ba_covisibility: validates the map as ba_prepare does, works on device buffers of its own and
 * touches neither the context's plan nor its LM state. The sort of at most n_cams weights runs on the host; bit rows,
 * popcounts, the points' ranks and the observations' compaction (flags, exclusive scan, scatter) are kernels. A
 * center without an admissible observation returns 0 with L = {center}, P, F and the observations empty and
 * sub_fixed_cam = 0. center out of range, contexts with landmark shards: BA_E_INVALID. */
typedef struct ba_local_request {
    int32_t struct_size, center;     /* BA_LOCAL_REQUEST_INIT */
    int32_t min_weight, max_local;
    int32_t* w;                      /* optional [n_cams] */
    int32_t* cam_index;              /* optional [n_local + n_fixed]: original indices of the sub-window's cameras */
    uint8_t* cam_constant;           /* optional [n_local + n_fixed] */
    uint8_t* cam_local;              /* optional [n_local + n_fixed]: 1 = the camera is in L */
    int32_t* pt_index;               /* optional [info.n_points] */
    int32_t* obs_index;              /* optional [info.n_obs]: original indices of the kept observations */
    int32_t* sub_obs_cam;            /* optional [info.n_obs] */
    int32_t* sub_obs_pt;             /* optional [info.n_obs] */
} ba_local_request;
typedef struct ba_local_info {
    int32_t struct_size;
    int32_t n_local, n_fixed;        /* |L|, |F| */
    int32_t n_points, n_obs;         /* of the sub-window */
    int32_t sub_fixed_cam;
    double time_select_ms;           /* the kernels (HIP events) */
    double time_total_ms;            /* the whole call, uploads, the host's sort and copies included */
} ba_local_info;
#define BA_LOCAL_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_local_request))
#define BA_LOCAL_INFO_MIN_SIZE ((int32_t)sizeof(ba_local_info))
#define BA_LOCAL_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_LOCAL_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_local_window(ba_context* ctx, const ba_problem* prob, const ba_local_request* req, ba_local_info* info);

/* ba_local_window, then ba_solve on the sub-window under its constant set. The context keeps the sub-window as a
 * shadow problem (cameras and points gathered, obs_uv / obs_depth gathered by obs_index; intrinsics and prior are the
 * caller's), solves it and copies L's cameras and P's points back to their places in prob. The intrinsics are
 * optimised against the prior as in every ba_solve (the reference's sliding windows do the same). Cameras outside L,
 * points outside P and constant cameras stay bitwise untouched, and the context's own constant set is back in force
 * afterwards. req's output buffers are filled as by ba_local_window. A sub-window without an observation: nothing is
 * solved and nothing in prob changes, summary is that of ba_solve on an empty window, the return value is 0.
 * summary, ba_iteration_log, ba_last_prepare and the plan cache describe the sub-window: a repeat with the same
 * selection reuses the plan. */
int32_t ba_solve_local(ba_context* ctx, ba_problem* prob, const ba_local_request* req, ba_local_info* info,
                       ba_summary* summary);

/* ---- localisation: pose-only refinement against a constant map ----
 * The optimiser a SLAM front-end calls per frame (ORB-SLAM's "track local map") or per pose hypothesis
 * (relocalisation): every selected camera's pose is refined with the points and the intrinsics held constant. With
 * those constant the cameras decouple, so a call is a batch of independent 6-parameter problems, one workgroup each,
 * the whole trust-region loop inside one kernel launch.
 * Cost. For every selected camera c with at least one admissible observation (depth > 1e-15) the call minimises over
 * c's pose alone the cost ba_solve has on the one-camera window made of c's observations: the sum over c's admissible
 * observations of 0.5 rho_repr + 0.5 rho_unpr with the weights 1 / N_c and weight_unpr / N_c, N_c being c's OWN
 * admissible count, and the Huber parameters of the context's options. The IntrinsicsPrior block has only constant
 * parameters and is not part of the cost (Ceres drops such a block from the program).
 * Loop. The LM loop of ba_solve restated per camera, every option taken from the context's ba_options: Jacobi scaling
 * 1 / (1 + sqrt(column norm^2)) taken at iteration 0; the LM diagonal clamp(diag, min_lm_diagonal, max_lm_diagonal) /
 * radius; the step delta = -scale * y applied as T * exp(delta); the model cost change from the unscaled Jacobian; rho
 * against min_relative_decrease; the radius update and the decrease factor; a non-positive or non-finite Cholesky
 * pivot or a model cost change that is not positive is an invalid step, max_num_consecutive_invalid_steps of them end
 * the camera with BA_FAILURE; the gradient, parameter and function tolerances, |x| being the ambient norm of the one
 * pose (7 values); max_num_iterations. log_rows receives camera log_cam's rows in ba_iteration_log's layout (the
 * gradient max-norm column is filled in every row).
 * cam_stats, BA_LOC_STAT_N values per camera of the window:
 *   [0] admissible observations N_c   [1] initial cost            [2] final cost (the lowest cost of any iteration)
 *   [3] LM iterations                 [4] successful steps (Ceres convention: includes iteration 0)
 *   [5] unsuccessful steps            [6] termination type (BA_CONVERGENCE / BA_NO_CONVERGENCE / BA_FAILURE), or -1 for
 *   a camera that was not selected or has no admissible observation   [7] the message kind of the LM loop (the msg of
 *   ba_debug_step_state). A camera with [6] = -1 has zeros elsewhere.
 *   [2] follows ceres::Solver::Summary::final_cost: the lowest cost any iteration evaluated, a rejected candidate's
 *   included, so it can lie below the cost at the returned pose (the cost of the last successful step in the log).
 * Inputs. prob->fixed_cam and the context's constant set (ba_set_constant_cameras) are not consulted: cam_mask alone
 * says which cameras are localised.
 * Outputs. Selected cameras are updated in place; points, intrinsics, the observation arrays and the unselected
 * cameras stay bitwise untouched, and so does a selected camera without an admissible observation. A camera whose
 * evaluation at the given pose is not finite ends with BA_FAILURE and keeps its pose.
 * Stand-alone like ba_covisibility: validates the window as ba_prepare does, works on device buffers of its own (the
 * context keeps them between calls) and touches neither the context's plan nor its LM state: a ba_solve_prepared
 * after it is bitwise the solve without it.
 * Reproducibility. No floating-point atomics; every sum has one fixed order, set by the observation's position among
 * its camera's admissible observations in the caller's order, and a camera's result does not depend on what else is
 * in the call: alone or beside hundreds of other cameras it gives the same bits.
 * ba_loc_info: n_selected cameras the mask names, n_solved of them with an admissible observation (the grid),
 * n_convergence + n_no_convergence + n_failure = n_solved, max_iterations the most LM iterations any camera took,
 * log_rows the rows camera log_cam's loop produced (iterations + 1, of which the first min(log_rows, log_max_rows) are
 * written and the rest of the buffer is left alone; 0 when log_cam was not solved or its evaluation at the given pose
 * failed).
 * log_cam >= n_cams, log_max_rows > 0 without log_rows, contexts with landmark shards: BA_E_INVALID. */
#define BA_LOC_STAT_N 8
typedef struct ba_loc_request {
    int32_t struct_size, reserved0;      /* BA_LOC_REQUEST_INIT */
    const uint8_t* cam_mask;             /* optional [n_cams]: non-zero = localise this camera; NULL = every camera */
    double* cam_stats;                   /* optional [n_cams * BA_LOC_STAT_N] */
    int32_t log_cam, log_max_rows;       /* log_cam < 0: no log */
    double* log_rows;                    /* [log_max_rows * BA_LOG_WIDTH], rows as ba_iteration_log, of camera log_cam */
} ba_loc_request;
typedef struct ba_loc_info {
    int32_t struct_size, n_selected, n_solved, n_convergence, n_no_convergence, n_failure, max_iterations, log_rows;
    double time_lm_ms, time_total_ms;    /* the kernel (HIP events); the whole call */
} ba_loc_info;
#define BA_LOC_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_loc_request))
#define BA_LOC_INFO_MIN_SIZE ((int32_t)sizeof(ba_loc_info))
/* (a zeroed request names camera 0 with log_max_rows = 0: no row is written, ba_loc_info.log_rows counts camera 0's) */
#define BA_LOC_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_LOC_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_localize(ba_context* ctx, ba_problem* prob, const ba_loc_request* req, ba_loc_info* info);

/* ---- point refinement: structure-only refinement against constant cameras ----
 * The other block of the alternation whose first block is ba_localize, and the optimiser an SfM or SLAM back-end
 * calls after triangulation or map-point insertion: every selected point's position is refined with the cameras and
 * the intrinsics held constant. With those constant the points decouple, so a call is a batch of independent
 * 3-parameter problems, one row of 16 lanes each (four points per wave), the whole trust-region loop inside one
 * kernel launch. The contract is ba_localize's with cameras and points swapped.
 * Cost. A point p is solved if it is selected and has at least min_obs (<= 0: 1) admissible observations (depth >
 * 1e-15). For each such point the call minimises over X_p alone the cost ba_solve has on the one-point window made
 * of p's observations with every camera constant: the sum over p's admissible observations of 0.5 rho_repr + 0.5
 * rho_unpr with the weights 1 / N_p and weight_unpr / N_p, N_p being p's OWN admissible count, and the Huber
 * parameters of the context's options. The IntrinsicsPrior block has only constant parameters and is not part of the
 * cost.
 * Loop. The LM loop of ba_solve restated for three Euclidean parameters, every option taken from the context's
 * ba_options: Jacobi scaling 1 / (1 + sqrt(column norm^2)) taken at iteration 0; the LM diagonal clamp(diag,
 * min_lm_diagonal, max_lm_diagonal) / radius; a 3x3 Cholesky with IEEE square root and division; the step delta =
 * -scale * y applied as X + delta; the model cost change from the unscaled Jacobian; rho against
 * min_relative_decrease; the radius update and the decrease factor; a non-positive or non-finite Cholesky pivot or a
 * model cost change that is not positive is an invalid step, max_num_consecutive_invalid_steps of them end the point
 * with BA_FAILURE; the gradient tolerance on max_i |X_i - (X_i + -g_i)|, the parameter tolerance with |X|_2 of the
 * three coordinates, the function tolerance; max_num_iterations. log_rows receives point log_pt's rows in
 * ba_iteration_log's layout (the gradient max-norm column is filled in every row).
 * pt_stats, BA_PTS_STAT_N values per point of the window:
 *   [0] admissible observations N_p   [1] initial cost            [2] final cost (the lowest cost of any iteration)
 *   [3] LM iterations                 [4] successful steps (Ceres convention: includes iteration 0)
 *   [5] unsuccessful steps            [6] termination type (BA_CONVERGENCE / BA_NO_CONVERGENCE / BA_FAILURE), or -1 for
 *   a point that was not selected or has fewer than min_obs admissible observations   [7] the message kind of the LM
 *   loop (the msg of ba_debug_step_state). A point with [6] = -1 has zeros elsewhere.
 *   [2] follows ceres::Solver::Summary::final_cost: the lowest cost any iteration evaluated, a rejected candidate's
 *   included, so it can lie below the cost at the returned position.
 * Inputs. prob->fixed_cam and the context's constant set (ba_set_constant_cameras) are not consulted: every camera is
 * constant here, and pt_mask alone says which points are refined.
 * Outputs. Solved points are updated in place; cameras, intrinsics, the observation arrays, the unselected points and
 * the selected points below min_obs stay bitwise untouched. A point whose evaluation at the given position is not
 * finite ends with BA_FAILURE (the evaluation-failed message), keeps its position and writes no log row.
 * Stand-alone like ba_localize: validates the window as ba_prepare does, works on device buffers of its own (the
 * context keeps them between calls; every call uploads the window) and touches neither the context's plan nor its LM
 * state nor the plan cache: a ba_solve_prepared after it is bitwise the solve without it.
 * Reproducibility. No floating-point atomics; every sum has one fixed order, set by the observation's position among
 * its point's admissible observations in the caller's order, and a point's result does not depend on what else is in
 * the call: alone or among 10^5 others it gives the same bits.
 * ba_pts_info: n_selected points the mask names, n_solved of them with min_obs admissible observations (the grid's
 * rows), n_convergence + n_no_convergence + n_failure = n_solved, max_iterations the most LM iterations any point
 * took, log_rows the rows point log_pt's loop produced (iterations + 1, of which the first min(log_rows,
 * log_max_rows) are written and the rest of the buffer is left alone; 0 when log_pt was not solved or its evaluation
 * at the given position failed).
 * log_pt >= n_points, log_max_rows > 0 without log_rows, contexts with landmark shards: BA_E_INVALID. */
#define BA_PTS_STAT_N 8
typedef struct ba_pts_request {
    int32_t struct_size, min_obs;        /* BA_PTS_REQUEST_INIT; min_obs <= 0: 1 */
    const uint8_t* pt_mask;              /* optional [n_points]: non-zero = refine this point; NULL = every point */
    double* pt_stats;                    /* optional [n_points * BA_PTS_STAT_N] */
    int32_t log_pt, log_max_rows;        /* log_pt < 0: no log */
    double* log_rows;                    /* [log_max_rows * BA_LOG_WIDTH], rows as ba_iteration_log, of point log_pt */
} ba_pts_request;
typedef struct ba_pts_info {
    int32_t struct_size, n_selected, n_solved, n_convergence, n_no_convergence, n_failure, max_iterations, log_rows;
    double time_lm_ms, time_total_ms;    /* the kernel (HIP events); the whole call */
} ba_pts_info;
#define BA_PTS_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_pts_request))
#define BA_PTS_INFO_MIN_SIZE ((int32_t)sizeof(ba_pts_info))
/* (a zeroed request names point 0 with log_max_rows = 0: no row is written, ba_pts_info.log_rows counts point 0's) */
#define BA_PTS_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_PTS_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_refine_points(ba_context* ctx, ba_problem* prob, const ba_pts_request* req, ba_pts_info* info);

/* ---- pose graph: keyframe poses over relative-pose edges ----
 * What a SLAM back-end runs when a loop closes, before any bundle adjustment: the accumulated drift is spread over the
 * keyframes by minimising the disagreement of the poses with a set of relative-pose measurements (sequential odometry,
 * strong co-visibility, the loop edges). Nodes are the poses of `cams` (ba_problem's layout: quaternion x, y, z, w, then
 * t, camera-to-world), solved in place; edge k joins edge_a[k] and edge_b[k] and carries the measured relative pose
 * Z_ab = T_a^-1 T_b in the same layout, with an optional pair (w_t, w_r) in edge_weight: the square roots of the
 * information of the translation part and of the rotation part (NULL: 1, 1).
 * Cost. Ceres' pose_graph_3d error term stated for this pose and retraction. For edge (a, b):
 *   t^ = R_a^T (t_b - t_a),  q^ = q_a^-1 q_b,  dq = q_meas q^^-1 taken on the hemisphere dq.w >= 0 (dq is negated
 *   when its w is negative: q and -q are one rotation, and the short way round is the one to minimise),
 *   r = [ w_t (t^ - t_meas) ; w_r 2 vec(dq) ], six values, one residual block per edge.
 * The cost is 1/2 sum rho(|r|^2): rho trivial for huber = 0, else Ceres' HuberLoss(huber) on the block, with the
 * sqrt(rho') corrector on residual and Jacobian as the LM kernels apply it to an observation block. Parameters move by
 * the Sophus right perturbation T exp(delta), delta = [upsilon, omega]; the Jacobians are the exact derivatives of r
 * with respect to delta_a and delta_b at 0 (no small-angle approximation of the residual).
 * A pose named by is_constant or fixed_cam is constant: it has no columns, and an edge between two constant poses
 * counts in the cost only.
 * Loop. The LM loop of ba_solve for 6 n_active unknowns, every option taken from the context's ba_options: Jacobi
 * scaling from iteration 0, the clamped LM diagonal over the radius, delta = -scale y, the model cost change
 * -(delta^T g + delta^T H delta / 2) from the unscaled quantities, rho against min_relative_decrease, the radius update,
 * invalid steps (a Cholesky pivot that is not positive, a model cost change that is not) with their limit, the three
 * tolerances with |x| the ambient norm of the active poses, max_num_iterations; the rows of `log` are
 * ba_iteration_log's.
 * Linear solve. The normal equations are dense-assembled (npad = 6 n_active rounded up to 16, squared, doubles) and
 * solved by the blocked multi-workgroup Cholesky of BA_LS_BLOCKED over the envelope the edges leave once the active
 * poses are placed in reverse Cuthill-McKee order (always: there is no Schur window to protect). A graph with
 * npad > BA_PG_MAX_NPAD (8192: 1365 active poses, 512 MB) is refused with BA_E_INVALID.
 * Legal inputs that return 0: no edge, or every pose constant (nothing is written, the costs are reported); an active
 * pose without an edge (it comes back bitwise as given: its block is the clamped diagonal alone and its step is zero);
 * a component without a constant pose (the damping keeps the system positive definite; where the poses of such a
 * component come to rest, the gauge, is then the caller's business).
 * Outputs. Only active poses are written back; constant poses and every other buffer stay bitwise untouched. No
 * floating-point atomics, every sum in one fixed order (an edge's position in the caller's arrays): two calls give
 * the same bits. Stand-alone like ba_localize: device buffers of its own, the context's plan and LM state untouched.
 * ba_pg_info: n_active poses with columns, n_edges_used edges with an active endpoint, n_components of the active
 * poses' graph, band_before / band_after (max position distance of two coupled active poses as given / as ordered),
 * reduced_system_size 6 n_active, the loop's counters, termination_type and message as ba_summary's, log_rows the rows
 * the loop produced (iterations + 1; the first min(log_rows, log_max_rows) are written), time_kernels_ms the device
 * time of the LM iterations' kernels and time_solve_ms the reduced solve's part of it (HIP events), time_order_ms the
 * host's ordering and envelope, time_total_ms the whole call.
 * Errors. A null argument, struct sizes below the minimum, contexts with landmark shards, negative sizes, a null
 * required buffer, an edge index out of range, a self edge, fixed_cam >= n_cams, a log without a buffer, the cap:
 * BA_E_INVALID. A pose, measurement or weight that is not finite: the call returns 0 with termination_type
 * BA_FAILURE and the evaluation-failed message, the poses kept, no log row (ba_localize's rule). */
#define BA_PG_MAX_NPAD 8192
typedef struct ba_pg_problem {
    int32_t n_cams, n_edges;
    double* cams;                 /* [n_cams*7] (in/out) */
    const int32_t* edge_a;        /* [n_edges] */
    const int32_t* edge_b;        /* [n_edges] */
    const double* edge_meas;      /* [n_edges*7] Z_ab = T_a^-1 T_b */
    const double* edge_weight;    /* optional [n_edges*2]: (w_t, w_r); NULL = 1, 1 */
    const uint8_t* is_constant;   /* optional [n_cams]: non-zero = a constant pose */
    int32_t fixed_cam, reserved0; /* a further constant pose; -1 = none */
} ba_pg_problem;
typedef struct ba_pg_request {
    int32_t struct_size, log_max_rows;   /* BA_PG_REQUEST_INIT */
    double huber;                        /* 0: trivial loss; > 0: HuberLoss(huber) on the edge's residual block */
    double* log;                         /* optional [log_max_rows * BA_LOG_WIDTH], rows as ba_iteration_log */
    int32_t* cam_order;                  /* optional [n_cams] out: the pose placed k-th (active ones first) */
    double* edge_cost;                   /* optional [n_edges] out: each edge's robustified cost at the result */
} ba_pg_request;
typedef struct ba_pg_info {
    int32_t struct_size, n_active, n_edges_used, n_components, band_before, band_after, reduced_system_size;
    int32_t iterations, n_successful, n_unsuccessful, termination_type, log_rows;
    double initial_cost, final_cost;
    double time_kernels_ms, time_solve_ms, time_order_ms, time_total_ms;
    char message[160];
} ba_pg_info;
#define BA_PG_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_pg_request))
#define BA_PG_INFO_MIN_SIZE ((int32_t)sizeof(ba_pg_info))
#define BA_PG_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_PG_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_pose_graph(ba_context* ctx, ba_pg_problem* g, const ba_pg_request* req, ba_pg_info* info);

/* ---- align: batched RANSAC relative pose from 3D-3D correspondences ----
 * What the tracker runs before anything can be refined (the reference's initializeRelativePose: OpenGV RANSAC over
 * the matched 3D points of two keyframes), and what measures a loop edge for ba_pose_graph or a start pose for
 * ba_localize. A call takes n_pairs independent pairs of point clouds: pair j owns the correspondences
 * [pair_begin[j], pair_begin[j+1]) of p1 / p2 (x, y, z per correspondence, f64); pair_begin is non-decreasing, starts
 * at 0 or above and ends at n_corr. The result of a pair is the pose Z with p1 ~ R p2 + t in ba_problem's layout
 * (quaternion x, y, z, w with w >= 0, then t): with p1 in keyframe a's frame and p2 in b's this is ba_pg_problem's
 * edge_meas Z_ab = T_a^-1 T_b, and the reference's T_1_2.
 * Hypotheses. Every pair evaluates n_hypotheses minimal samples (<= 0: 256; above BA_ALIGN_MAX_HYP: BA_E_INVALID), all
 * of them: nothing stops early. The sample of hypothesis h of pair j is integer arithmetic on uint64 alone:
 *   mix(x):  x += 0x9E3779B97F4A7C15; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB;
 *            x ^= x >> 31                                                     (the splitmix64 finaliser)
 *   key = mix(seed ^ mix((uint64)j << 32 | h)),  r_i = mix(key + i) for i = 1, 2, 3
 *   d0 = ((r_1 >> 32) * n) >> 32,  d1 = ((r_2 >> 32) * (n - 1)) >> 32,  d2 = ((r_3 >> 32) * (n - 2)) >> 32
 *   i0 = d0;  i1 = d1, plus 1 if i1 >= i0;  i2 = d2, plus 1 if i2 >= min(i0, i1), then plus 1 if i2 >= max(i0, i1)
 * with n the pair's size: three distinct indices of the pair, uniform over the ordered triples.
 * A sample (a, b, c) is degenerate when |(b - a) x (c - a)| <= min_cross (<= 0: 1e-6) in either cloud (compared on the
 * squares) or when one of its 18 coordinates is not finite; its count is -1. Otherwise its model is Arun's
 * least-squares fit of the three correspondences: c1, c2 the centroids, H = sum (p2 - c2)(p1 - c1)^T, R the rotation
 * (det +1) that maximises tr(R H), t = c1 - R c2. R comes from Horn's quaternion form: the eigenvector of the largest
 * eigenvalue of the symmetric 4x4 matrix built from H, by BA_ALIGN_SWEEPS cyclic Jacobi sweeps. A correspondence is
 * an inlier of a model when |p1 - (R p2 + t)|^2 < threshold^2 (threshold <= 0: 0.1, the reference's), compared in f64
 * on the squares; a correspondence with a coordinate that is not finite is never an inlier. hyp_count receives every
 * hypothesis's inlier count.
 * Selection. The hypothesis with the largest count wins, the smallest h among equals (OpenGV's strict > keeps the
 * first). A pair with n < 3 is BA_ALIGN_TOO_FEW (its hyp_count entries are -1), a pair whose every sample is degenerate
 * BA_ALIGN_NO_MODEL: both return the identity pose, 0 inliers and a zero mask, and the call still returns 0.
 * Refit, `refit` rounds (0: the reference's behaviour, the best minimal sample's model as it is): Arun's fit over the
 * current inlier set (the centroids first, then H about them), then the inlier set of the new pose. The round is taken
 * when its inlier count is >= the previous one, otherwise the rounds end and the previous pose stays; they also end
 * when a taken round left the set unchanged, when fewer than 3 inliers remain or when the fit is not finite.
 * pair_stats, BA_ALIGN_STAT_N values per pair:
 *   [0] status (BA_ALIGN_OK / BA_ALIGN_TOO_FEW / BA_ALIGN_NO_MODEL)   [1] n   [2] n_inliers of the returned pose
 *   [3] best_hyp (-1 without a model)   [4] n_degenerate samples   [5] the inliers' RMS distance |p1 - (R p2 + t)|
 *   [6] n_inliers of the best sample before any refit
 *   [7] k_needed = log(1 - probability) / log(1 - w^3), w = [6] / n (probability <= 0: 0.999): OpenGV's adaptive
 *   iteration count, computed on the host from the integers, so the caller can see whether n_hypotheses was enough
 *   (+inf for w = 0, 0 for w = 1 and for a pair without a model).
 * Reproducibility. No floating-point atomics; every decision is an integer comparison and every sum has one fixed
 * order set by the pair's size alone: two calls give the same bits, and the pair at index j gives the same bits
 * whatever the other pairs of the call are (its samples depend on the seed, j and its size alone).
 * Stand-alone like ba_localize: device buffers of its own, the context's plan and LM state untouched: a
 * ba_solve_prepared after it is bitwise the solve without it.
 * ba_align_info: n_pairs, the pairs per status, n_hypotheses as used, time_kernels_ms the two kernels (HIP events),
 * time_total_ms the whole call. BA_ALIGN_INFO_MIN_SIZE covers the counts; a caller's struct that ends before the
 * timings is served without them.
 * Errors, BA_E_INVALID: a null argument, struct sizes below the minimum, contexts with landmark shards, negative
 * sizes, a pair_begin that is missing, starts below 0, decreases or does not end at n_corr, a null required buffer
 * (p1 / p2 with n_corr > 0, poses with n_pairs > 0), n_hypotheses above BA_ALIGN_MAX_HYP. */
#define BA_ALIGN_STAT_N 8
#define BA_ALIGN_MAX_HYP 65536
#define BA_ALIGN_SWEEPS 6
#define BA_ALIGN_OK 0
#define BA_ALIGN_TOO_FEW 1
#define BA_ALIGN_NO_MODEL 2
typedef struct ba_align_problem {
    int32_t n_pairs, n_corr;
    const int32_t* pair_begin;    /* [n_pairs+1] */
    const double* p1;             /* [n_corr*3] */
    const double* p2;             /* [n_corr*3] */
} ba_align_problem;
typedef struct ba_align_request {
    int32_t struct_size, n_hypotheses;   /* BA_ALIGN_REQUEST_INIT; n_hypotheses <= 0: 256 */
    int32_t refit, reserved0;            /* refit rounds; 0 = the best sample's model */
    uint64_t seed;
    double threshold, min_cross, probability;  /* <= 0: 0.1, 1e-6, 0.999 */
    double* poses;                       /* [n_pairs*7] out */
    double* pair_stats;                  /* optional [n_pairs*BA_ALIGN_STAT_N] out */
    uint8_t* inlier;                     /* optional [n_corr] out: 1 = an inlier of its pair's pose */
    int32_t* hyp_count;                  /* optional [n_pairs*n_hypotheses] out: inlier counts, -1 = degenerate */
} ba_align_request;
typedef struct ba_align_info {
    int32_t struct_size, n_pairs, n_ok, n_too_few, n_no_model, n_hypotheses;
    double time_kernels_ms, time_total_ms;
} ba_align_info;
#define BA_ALIGN_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_align_request))
#define BA_ALIGN_INFO_MIN_SIZE ((int32_t)offsetof(ba_align_info, time_kernels_ms))
#define BA_ALIGN_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_ALIGN_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_align(ba_context* ctx, const ba_align_problem* prob, const ba_align_request* req, ba_align_info* info);

/* ---- match: batched 2-nearest-neighbour descriptor matching with the ratio test ----
 * What finds the correspondences ba_align starts from (the reference's matchKeypoints + filterMatchesLowe: OpenCV's
 * brute-force knnMatch with k = 2, then Lowe's ratio test). A call takes n_pairs independent pairs of descriptor
 * sets. A descriptor is desc_bytes bytes; kind says how two of them compare:
 *   BA_MATCH_HAMMING  the bytes as bit strings, distance = popcount(a xor b)                      (ORB, BRIEF)
 *   BA_MATCH_L2_U8    the bytes as the integers 0..255, distance = sum (a_k - b_k)^2, an exact int32: the SQUARE of
 *                     the Euclidean distance (byte SIFT)
 * Rows. Pair j's queries are query[q_begin..q_end) and its trains train[t_begin..t_end) (pair_range, four values per
 * pair; descriptor indices). Ranges of different pairs may overlap: one keyframe against many candidates is one copy
 * of its descriptors. Output row row_begin[j] + (q - q_begin) belongs to query q of pair j, with row_begin[j] the sum
 * of (q_end - q_begin) over the pairs before j; n_rows is that sum over all pairs.
 * Neighbours. The first and the second neighbour of a query are the two smallest trains of its pair under the
 * lexicographic order (distance, train index). The definition does not depend on any traversal order: a tile, a slice
 * and a merge of slices all give the same answer. Among equal distances the smaller index is first (OpenCV's
 * brute-force knnMatch with its strict <). nn_idx holds the two train indices inside the pair's range (t - t_begin),
 * nn_dist their distances; a pair with one train has no second neighbour, a pair with none has neither: -1 in both.
 * Acceptance. The conditions are checked in this order and a query is counted at the first one it fails:
 *   1. a second neighbour exists;
 *   2. the ratio test (ratio <= 0: 0.7, the reference's): HAMMING (float)d0 < ratio * (float)d1 evaluated in f32,
 *      which is filterMatchesLowe on OpenCV's float distances bit for bit; L2_U8 on the squares in f64,
 *      (double)s0 < ((double)ratio * (double)ratio) * (double)s1, which equals the reference's test on the square
 *      roots except where the two sides meet within rounding;
 *   3. d0 <= max_distance, if max_distance > 0 (for L2_U8 on the squared distance, as nn_dist holds it);
 *   4. with cross_check: the query is the smallest query of its pair, under (distance, query index), for the train
 *      it chose.
 * accept is 1 for a row that passes all of them. matches lists the accepted rows of each pair in query order as
 * (query, train), both local to the pair's ranges; pair j's are matches[2 match_begin[j] .. 2 match_begin[j+1]).
 * pair_counts, BA_MATCH_COUNT_N values per pair:
 *   [0] n_q   [1] n_t   [2] accepted   [3] no second neighbour   [4] failed the ratio   [5] failed max_distance
 *   [6] failed the cross-check                                                 ([2] + .. + [6] = [0])
 * Reproducibility. Only integer arithmetic and integer atomics are used (the ratio test is one product and one
 * comparison per row): two calls give the same bits, and a pair's rows give the same bits whatever the other pairs of
 * the call are and however the trains are sliced over workgroups.
 * Stand-alone like ba_align: device buffers of its own, the context's plan and LM state untouched: a
 * ba_solve_prepared after it is bitwise the solve without it.
 * ba_match_info: n_pairs, n_rows, n_matches (the accepted rows of all pairs), kind, time_kernels_ms the kernels (HIP
 * events), time_total_ms the whole call. BA_MATCH_INFO_MIN_SIZE covers the counts; a caller's struct that ends before
 * the timings is served without them.
 * Errors, BA_E_INVALID: a null argument, struct sizes below the minimum, contexts with landmark shards; then negative
 * sizes; a kind or desc_bytes outside the above; a range that is reversed or leaves [0, n_query) / [0, n_train);
 * n_rows that is not the sum of the pairs' query counts; a null required buffer (query / train with rows to read,
 * pair_range with pairs, nn_idx / nn_dist with rows, match_begin with matches); a grid above the launch limit of 2^32
 * threads (2^26 workgroups of 64 queries x train slices for HAMMING, 2^24 for L2_U8: some 10^9 rows). Empty pairs and
 * n_pairs = 0 return 0. */
#define BA_MATCH_HAMMING 0      /* bytes as bit strings: distance = popcount(a xor b)                    */
#define BA_MATCH_L2_U8   1      /* bytes as 0..255: distance = sum (a_k - b_k)^2, an exact int32         */
#define BA_MATCH_MAX_BYTES 256
#define BA_MATCH_COUNT_N 7
typedef struct ba_match_problem {
    int32_t kind, desc_bytes;          /* desc_bytes: a multiple of 4 in [4, BA_MATCH_MAX_BYTES]          */
    int32_t n_query, n_train;          /* descriptors in query / train                                    */
    int32_t n_pairs, n_rows;           /* n_rows = sum over pairs of (q_end - q_begin)                    */
    const uint8_t* query;              /* [n_query*desc_bytes]                                            */
    const uint8_t* train;              /* [n_train*desc_bytes]                                            */
    const int32_t* pair_range;         /* [n_pairs*4]: q_begin, q_end, t_begin, t_end                     */
} ba_match_problem;
typedef struct ba_match_request {
    int32_t struct_size, cross_check;  /* BA_MATCH_REQUEST_INIT; cross_check 0 = the reference            */
    float ratio; int32_t max_distance; /* ratio <= 0: 0.7f; max_distance <= 0: no limit                   */
    int32_t* nn_idx;                   /* [n_rows*2] out: train index inside the pair's range, -1 = none  */
    int32_t* nn_dist;                  /* [n_rows*2] out: the distances, -1 = none                        */
    uint8_t* accept;                   /* optional [n_rows] out                                           */
    int32_t* matches;                  /* optional [n_rows*2] out: accepted (query, train), both local to the pair */
    int32_t* match_begin;              /* optional [n_pairs+1] out (required with matches)                */
    int32_t* pair_counts;              /* optional [n_pairs*BA_MATCH_COUNT_N] out                         */
} ba_match_request;
typedef struct ba_match_info {
    int32_t struct_size, n_pairs, n_rows, n_matches, kind, reserved0;
    double time_kernels_ms, time_total_ms;
} ba_match_info;
#define BA_MATCH_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_match_request))
#define BA_MATCH_INFO_MIN_SIZE ((int32_t)offsetof(ba_match_info, time_kernels_ms))
#define BA_MATCH_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_MATCH_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_match(ba_context* ctx, const ba_match_problem* prob, const ba_match_request* req, ba_match_info* info);

/* ---- guided match: descriptor search in a pixel window around projected landmarks ----
 * What finds a landmark of the map in a frame whose pose is roughly known (ORB-SLAM's SearchByProjection / Fuse):
 * project the landmark with the pose as it stands, look only at the frame's keypoints within `radius` pixels of the
 * projection, take the best descriptor there. kind, desc_bytes and the two distances are ba_match's (BA_MATCH_HAMMING,
 * BA_MATCH_L2_U8, a multiple of 4 in [4, BA_MATCH_MAX_BYTES]). One camera model (intr, width x height) per call.
 * Rows. Frame entry f has the pose frame_pose[7 f ..] (T_w_c, Sophus order), the keypoints kp[begin..end)
 * (frame_range, two values per entry) and the candidates cand_pt[cand_begin[f] .. cand_begin[f+1]) (landmark indices
 * into points / pt_desc; cand_begin is non-decreasing from 0, n_rows = cand_begin[n_frames]). Output row r belongs to
 * candidate r. Ranges of different entries may overlap or be equal: many pose hypotheses of one image are one copy
 * of its keypoints (entries with equal ranges also share one binned grid on the device).
 * Projection. The LM loop's and ba_residuals' sequence of operations, bit for bit: R from the unit quaternion,
 * p = R^T (X - t), u = (cx z + fx x) (1/z), v = (cy z + fy y) (1/z). proj holds (u, v, z), u = v = 0 for status 1.
 * Window. Keypoint k of the entry's range is in the row's window when, evaluated in f64 in this order with no fused
 * multiply-add,
 *     du = kp_u - u;  dv = kp_v - v;  (du * du) + (dv * dv) <= radius * radius
 * and, when the depth gate is on (depth_tol > 0 and kp_depth given) and kp_depth[k] > 1e-15,
 *     |kp_depth[k] - z| <= depth_tol * z.
 * A keypoint without an admissible depth passes the gate. n_in_window counts the window's keypoints.
 * Neighbours. The first and the second neighbour are the two smallest keypoints of the window under the
 * lexicographic order (distance, keypoint index): independent of the binning and of any traversal order. nn_kp holds
 * their indices inside the entry's range (k - begin), nn_dist the distances; -1 in both where there is none.
 * Status. A row gets the first of these that applies:
 *   0 accepted
 *   1 z <= min_depth (or z is not a number)             (min_depth <= 0: 1e-15)
 *   2 the projection is outside [0, width) x [0, height)
 *   3 the window is empty
 *   4 a second neighbour exists and ba_match's ratio test fails (HAMMING (float)d0 < ratio * (float)d1 in f32; L2_U8
 *     (double)s0 < ((double)ratio * (double)ratio) * (double)s1 in f64; ratio <= 0: 0.7). A lone keypoint in the
 *     window passes: here, unlike in ba_match, that is the good case.
 *   5 max_distance > 0 and d0 > max_distance
 *   6 with one_to_one: another row of the same frame entry passed 1-5, chose the same keypoint and has the smaller
 *     key (d0, row)
 * matches lists the accepted rows of each entry in candidate order as (cand_pt value, keypoint index inside the
 * range); entry f's are matches[2 match_begin[f] .. 2 match_begin[f+1]). frame_counts, BA_GMATCH_COUNT_N per entry:
 *   [0] n_cand   [1] n_kp   [2 + s] rows of status s, s = 0..6                    ([2] + .. + [8] = [0])
 * cell_px is the side of the binning grid's cells (<= 0: the smallest power of two >= radius, at least 8, so that a
 * window touches at most 3 x 3 cells). It is a speed knob only.
 * Reproducibility. Floating point is used for the projection and the two gates alone, everything else is integer
 * work with integer atomics: two calls give the same bits, an entry's rows do not depend on the other entries of the
 * call nor on cell_px. Stand-alone like ba_match: device buffers of its own, a ba_solve_prepared after it is bitwise
 * the solve without it.
 * ba_gmatch_info: n_frames, n_rows, n_matches (status 0 over all entries), kind, n_grids (distinct keypoint ranges
 * binned), cell_px (as used), the timings as in ba_match_info (optional in the same way).
 * Errors, BA_E_INVALID, in this order: a null argument, struct sizes below the minimum, contexts with landmark
 * shards; negative sizes; kind; desc_bytes; width or height below 1; a radius that is not finite and positive; a
 * null frame_pose / frame_range / cand_begin with entries; a frame_range that is reversed or leaves [0, n_kp); a
 * cand_begin that does not start at 0, decreases, or does not end at n_rows; a null cand_pt with rows, a cand_pt
 * outside [0, n_points); a null required buffer (kp_uv / kp_desc with keypoints, points / pt_desc with rows, nn_kp /
 * nn_dist / status with rows, match_begin with matches); more than 2^31 - 1 grid cells, binned keypoints or
 * one-to-one slots over the call, or 2^24 or more entries (one workgroup of 256 threads each: the launch limit of
 * 2^32 threads). Empty ranges, empty candidate lists and n_frames = 0 return 0. */
#define BA_GMATCH_COUNT_N 9
typedef struct ba_gmatch_problem {
    int32_t kind, desc_bytes;          /* as ba_match_problem's                                           */
    int32_t width, height;             /* pixels                                                          */
    int32_t n_kp, n_points;            /* keypoints / landmarks                                           */
    int32_t n_frames, n_rows;          /* n_rows = cand_begin[n_frames]                                   */
    double intr[4];                    /* fx, fy, cx, cy                                                  */
    const double* kp_uv;               /* [n_kp*2]                                                        */
    const uint8_t* kp_desc;            /* [n_kp*desc_bytes]                                               */
    const double* kp_depth;            /* optional [n_kp]                                                 */
    const double* points;              /* [n_points*3] world frame                                        */
    const uint8_t* pt_desc;            /* [n_points*desc_bytes]                                           */
    const double* frame_pose;          /* [n_frames*7] T_w_c: qx qy qz qw tx ty tz                        */
    const int32_t* frame_range;        /* [n_frames*2] keypoint begin, end                                */
    const int32_t* cand_begin;         /* [n_frames+1]                                                    */
    const int32_t* cand_pt;            /* [n_rows] landmark indices                                       */
} ba_gmatch_problem;
typedef struct ba_gmatch_request {
    int32_t struct_size, one_to_one;   /* BA_GMATCH_REQUEST_INIT; one_to_one 0 / 1                        */
    double radius;                     /* pixels, > 0                                                     */
    float ratio; int32_t max_distance; /* ratio <= 0: 0.7f; max_distance <= 0: no limit                   */
    double min_depth, depth_tol;       /* min_depth <= 0: 1e-15; depth_tol <= 0: no depth gate            */
    int32_t cell_px, reserved0;        /* cell_px <= 0: the default                                       */
    int32_t* nn_kp;                    /* [n_rows*2] out: keypoint index inside the range, -1 = none      */
    int32_t* nn_dist;                  /* [n_rows*2] out: the distances, -1 = none                        */
    uint8_t* status;                   /* [n_rows] out                                                    */
    double* proj;                      /* optional [n_rows*3] out: u, v, z                                */
    int32_t* n_in_window;              /* optional [n_rows] out                                           */
    int32_t* matches;                  /* optional [n_rows*2] out: accepted (cand_pt value, keypoint in range) */
    int32_t* match_begin;              /* optional [n_frames+1] out (required with matches)               */
    int32_t* frame_counts;             /* optional [n_frames*BA_GMATCH_COUNT_N] out                       */
} ba_gmatch_request;
typedef struct ba_gmatch_info {
    int32_t struct_size, n_frames, n_rows, n_matches, kind, n_grids, cell_px, reserved0;
    double time_kernels_ms, time_total_ms;
} ba_gmatch_info;
#define BA_GMATCH_REQUEST_MIN_SIZE ((int32_t)sizeof(ba_gmatch_request))
#define BA_GMATCH_INFO_MIN_SIZE ((int32_t)offsetof(ba_gmatch_info, time_kernels_ms))
#define BA_GMATCH_REQUEST_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
#define BA_GMATCH_INFO_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (int32_t)sizeof(s))
int32_t ba_guided_match(ba_context* ctx, const ba_gmatch_problem* prob, const ba_gmatch_request* req, ba_gmatch_info* info);

/* ---- verification hooks (used by the parity tests; not on the hot path) ----
 * Evaluate per-observation robustified residuals and local Jacobians on the
 * device at the given parameters. Output layout per admissible observation k
 * in the ORIGINAL observation order (inadmissible rows are zero):
 *   res[k*3+{0,1,2}]   : sqrt(rho') * (reproj u, reproj v, depth) residual
 *   jcam[k*18 + r*6+d] : d res_r / d delta_d, delta = [upsilon(3), omega(3)]
 *   jpt [k*9  + r*3+i] : d res_r / d X_i
 *   jint[k*8  + r*4+i] : d res_r / d (fx,fy,cx,cy)_i  (rows 0,1; depth row is 0)
 * cost receives 0.5 * sum_blocks rho(|f_b|^2) including the intrinsics prior.
 * Any output pointer may be NULL. */
int32_t ba_debug_linearize(ba_context* ctx, const ba_problem* prob, double* cost,
                           double* res, double* jcam, double* jpt, double* jint);

/* Build the damped, Jacobi-scaled reduced camera system exactly as the first
 * LM iteration would (radius = initial_trust_region_radius unless radius > 0):
 * S [n*n] row-major dense (full symmetric), rhs [n], scale [6*n_cams + 3*n_points + 4]
 * where n = 6*active_cams + 4; active cameras in increasing index order. */
int32_t ba_debug_reduced_system(ba_context* ctx, const ba_problem* prob, double radius,
                                int32_t* n_out, double* S, double* rhs);

/* Test hook: the production camera-side pass (k_cam_side + k_cam_finalize, iteration-0 form) at the
 * problem's parameters. camdata[nac*51]: per active camera U upper-packed (21) | C 6x4 (24) | g (6);
 * lin[16]: cost, gradient max-norm of cameras + intrinsics, Ukk packed (10, + IntrinsicsPrior), gk (4,
 * + prior); ac_cam[nac]: the camera index of each active camera. With NULL outputs only *nac is set. */
int32_t ba_debug_camera_sums(ba_context* ctx, const ba_problem* prob, int32_t* nac, double* camdata,
                             double* lin, int32_t* ac_cam);

/* Test hook: the production LM step. Prepares the window and enqueues what ba_solve_prepared enqueues for
 * iteration zero and the first LM iteration (the same code), on the paths the prepare chose for the window
 * (reduced solve, band tail, fused / small-window linearisation, deterministic slabs, landmark shards);
 * radius replaces initial_trust_region_radius when > 0. prob is not modified. Outputs (all required):
 *   nac, ac_cam[n_cams]      active cameras, in increasing order (the first *nac entries are written)
 *   delta_cam[n_cams*6]      the parameter-space step -scale*y of active camera t at 6*t
 *   delta_intr[4]            the same for fx, fy, cx, cy
 *   delta_pts[n_points*3]    candidate point minus the point the step was computed from, in the caller's point
 *                            order; zero for points without an admissible observation; the same whether the
 *                            decision accepted or rejected the step
 *   log_row[BA_LOG_WIDTH]    row 1 of the iteration log (zeros if the solve ended before a step was taken)
 *   info[BA_STEP_INFO_N]     [0] the reduced-system factorisation flag of that iteration: bit 0 = not positive
 *                            definite, bit 1 = an inter-workgroup hand-off timed out; [1] retried: 1 = a
 *                            resident-kernel hand-off timed out and the iteration was re-run with the separate
 *                            launches, as ba_solve_prepared does (the context keeps them); [2] the window's
 *                            ba_summary.linear_solver and [3] camera_band; [4] with BA_LS_BAND the band width in
 *                            16x16 tiles (the banded Cholesky's instantiation), else 0; [5] LM iterations
 *                            counted (1 unless the solve ended before a step was taken); the rest 0 */
#define BA_STEP_INFO_N 8
int32_t ba_debug_step(ba_context* ctx, const ba_problem* prob, double radius, int32_t* nac, int32_t* ac_cam,
                      double* delta_cam, double* delta_intr, double* delta_pts, double* log_row, int32_t* info);

/* Test hook: what the last ba_debug_step left on the device, copied out without launching a kernel. Valid after a
 * successful ba_debug_step on the same context and until its next prepare / solve (BA_E_INVALID otherwise). All
 * outputs are required; cameras, intrinsics and points in the caller's order, as ba_debug_step was given them:
 *   cams_x, cams_cand[n_cams*7]   the parameter slot the step was computed from and the candidate slot
 *   intr_x, intr_cand[4]          (the gauge camera and blocks without an admissible observation hold the
 *   pts_x, pts_cand[n_points*3]    prepared value in both slots)
 *   scal[BA_STEP_SCAL_N]          the step scalars of that iteration: model cost change, candidate cost, ambient
 *                                 |x - x_cand|^2, gradient max-norm over the points, the bad-step code, |x_cand|^2,
 *                                 the rest 0
 *   lin[2]                        cost at x, gradient max-norm over cameras + intrinsics
 *   log_rows[2*BA_LOG_WIDTH]      rows 0 and 1 of the iteration log (row 0 carries the gradient max-norm at x)
 *   state[BA_STEP_STATE_N]        the LM state after the decision: radius, decrease_factor, xnorm2, x_cost,
 *                                 final_cost, cur (the slot of the accepted parameters), termination (-1 while
 *                                 the solve goes on), msg (the message kind), gmax_ci, initial_cost, iter, and
 *                                 the slot of x (so cur != that slot exactly when the step was accepted) */
#define BA_STEP_SCAL_N 8
#define BA_STEP_STATE_N 12
int32_t ba_debug_step_state(ba_context* ctx, double* cams_x, double* cams_cand, double* intr_x, double* intr_cand,
                            double* pts_x, double* pts_cand, double* scal, double* lin, double* log_rows,
                            double* state);

/* Test hook: FNV-1a digests of the last prepared window's plan arrays as the kernels read them from HBM (the
 * observation orderings, point order, tiles, chunks, segments, envelope), one per array, into out[max_n].
 * Returns the number of arrays. The host plan and the device plan (MIBA_DEVICE_PLAN) give the same digests. */
int32_t ba_debug_plan_digest(ba_context* ctx, uint64_t* out, int32_t max_n);

#ifdef __cplusplus
}
#endif
#endif /* MIBA_BA_H */
