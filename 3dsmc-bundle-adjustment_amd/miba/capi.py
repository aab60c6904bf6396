"""ctypes mirror of ``include/ba.h`` (the libmiba C-ABI).

The structures here are byte-for-byte the C structs; ``tests/test_capi.py``
checks their sizes against the compiled library. ``ProblemArrays`` keeps the
numpy buffers a ``ba_problem`` points into alive and contiguous.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

BA_OK = 0
BA_E_INVALID = -1
BA_E_DEVICE = -2
BA_E_NOMEM = -3
BA_E_COMM = -4
BA_E_INTERNAL = -5

BA_CONVERGENCE = 0
BA_NO_CONVERGENCE = 1
BA_FAILURE = 2

TERMINATION_NAMES = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE"}
# ba_summary.linear_solver (BA_LS_*): the reduced-solve path; the names are MIBA_SOLVER's values
LINEAR_SOLVER_NAMES = {0: "dense", 1: "band", 2: "bcr", 3: "blocked"}

# columns of an iteration-log row (ba_iteration_log, ba_debug_step), BA_LOG_WIDTH = 8 with the last one unused
LOG_FIELDS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "tr_ratio", "tr_radius", "accepted")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class BaOptions(C.Structure):
    """Mirror of ``ba_options`` (ceresGlobalProblem, BundleAdjustmentConfig.h:44-69)."""

    _fields_ = [
        ("hub_p_repr", C.c_double),
        ("hub_p_unpr", C.c_double),
        ("weight_intrinsics", C.c_double),
        ("weight_unpr", C.c_double),
        ("max_num_iterations", C.c_int32),
        ("minimizer_progress_to_stdout", C.c_int32),
        ("eta", C.c_double),
        ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("max_num_consecutive_invalid_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("device", C.c_int32),
        ("deterministic", C.c_int32),
        ("profile_kernels", C.c_int32),
        ("profile_mask", C.c_int32),
        ("shard_min_obs", C.c_int32),
        ("small_window", C.c_int32),
        ("rebuild_plan", C.c_int32),
        ("reserved", C.c_int32 * 1),
    ]


class BaProblem(C.Structure):
    """Mirror of ``ba_problem`` (the flattened window of windowOptimize)."""

    _fields_ = [
        ("n_cams", C.c_int32),
        ("n_points", C.c_int32),
        ("n_obs", C.c_int32),
        ("fixed_cam", C.c_int32),
        ("cams", _dp),
        ("points", _dp),
        ("intr", _dp),
        ("intr_prior", _dp),
        ("obs_cam", _ip),
        ("obs_pt", _ip),
        ("obs_uv", _dp),
        ("obs_depth", _dp),
    ]


class BaSummary(C.Structure):
    """Mirror of ``ba_summary`` (subset of ceres::Solver::Summary). BA_API_VERSION 2: ``struct_size`` is set to
    this mirror's size on construction (the library writes no more than that)."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("reserved0", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32),
        ("num_iterations", C.c_int32),
        ("termination_type", C.c_int32),
        ("num_obs_admissible", C.c_int32),
        ("num_active_cams", C.c_int32),
        ("num_active_points", C.c_int32),
        ("reduced_system_size", C.c_int32),
        ("linear_solver", C.c_int32),
        ("camera_band", C.c_int32),
        ("time_setup_ms", C.c_double),
        ("time_lm_ms", C.c_double),
        ("time_linearize_ms", C.c_double),
        ("time_schur_ms", C.c_double),
        ("time_factor_ms", C.c_double),
        ("time_update_ms", C.c_double),
        ("time_total_ms", C.c_double),
        ("message", C.c_char * 160),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_
             if name not in ("message", "struct_size", "reserved0")}
        d["message"] = self.message.decode(errors="replace")
        d["termination"] = TERMINATION_NAMES.get(self.termination_type, str(self.termination_type))
        d["linear_solver_name"] = LINEAR_SOLVER_NAMES.get(self.linear_solver, str(self.linear_solver))
        return d


class BaKernelStat(C.Structure):
    """Mirror of ``ba_kernel_stat``."""

    _fields_ = [
        ("name", C.c_char * 32),
        ("launches", C.c_int32),
        ("reserved", C.c_int32),
        ("total_ms", C.c_double),
        ("bytes_per_launch", C.c_double),
        ("flops_per_launch", C.c_double),
    ]


class BaPrepareInfo(C.Structure):
    """Mirror of ``ba_prepare_info`` (what the last prepare did; ba_last_prepare). ``struct_size`` is set to this
    mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("plan_reused", C.c_int32),
        ("obs_uploaded", C.c_int32),
        ("host_threads", C.c_int32),
        ("bcr_path", C.c_int32),
        ("compare_ms", C.c_double),
        ("plan_ms", C.c_double),
        ("upload_ms", C.c_double),
        ("total_ms", C.c_double),
        ("lin_path", C.c_int32),
        ("plan_device", C.c_int32),
        ("tail", C.c_int32),
        ("bsfin", C.c_int32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class BaCovRequest(C.Structure):
    """Mirror of ``ba_cov_request`` (ba_covariance). ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_pairs", C.c_int32),
        ("pair_a", _ip),
        ("pair_b", _ip),
        ("pair_cov", _dp),
        ("n_points", C.c_int32),
        ("point_idx", _ip),
        ("point_cov", _dp),
        ("full", _dp),
        ("min_reciprocal_condition_number", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaCovInfo(C.Structure):
    """Mirror of ``ba_cov_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("status", C.c_int32),
        ("n", C.c_int32),
        ("nac", C.c_int32),
        ("pivot_min", C.c_double),
        ("pivot_max", C.c_double),
        ("cost", C.c_double),
        ("variance_factor", C.c_double),
        ("time_build_ms", C.c_double),
        ("time_invert_ms", C.c_double),
        ("time_points_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


COV_INTR = -1  # BA_COV_INTR
COV_OK, COV_RANK_DEFICIENT = 0, 1


class BaResRequest(C.Structure):
    """Mirror of ``ba_res_request`` (ba_residuals). ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("reserved0", C.c_int32),
        ("max_reproj_px", C.c_double),
        ("max_depth_abs", C.c_double),
        ("max_depth_rel", C.c_double),
        ("obs_err", _dp),
        ("obs_cost", _dp),
        ("obs_flags", _ip),
        ("obs_depth_culled", _dp),
        ("cam_stats", _dp),
        ("point_stats", _dp),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaResInfo(C.Structure):
    """Mirror of ``ba_res_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_admissible", C.c_int32),
        ("n_outliers", C.c_int32),
        ("n_behind", C.c_int32),
        ("n_reproj", C.c_int32),
        ("n_depth", C.c_int32),
        ("n_huber_repr", C.c_int32),
        ("n_huber_unpr", C.c_int32),
        ("cost", C.c_double),
        ("prior_cost", C.c_double),
        ("rms_reproj_px", C.c_double),
        ("max_reproj_px", C.c_double),
        ("rms_depth", C.c_double),
        ("max_depth", C.c_double),
        ("time_eval_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


# bits of obs_flags (BA_RES_*)
RES_INADMISSIBLE, RES_BEHIND, RES_REPROJ, RES_DEPTH, RES_HUBER_REPR, RES_HUBER_UNPR = 1, 2, 4, 8, 16, 32
RES_OUTLIER = RES_BEHIND | RES_REPROJ | RES_DEPTH
RES_ERR_N, RES_STAT_N = 4, 6


class BaCovisRequest(C.Structure):
    """Mirror of ``ba_covis_request`` (ba_covisibility). ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("reserved0", C.c_int32),
        ("weights", _ip),
        ("order", _ip),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaCovisInfo(C.Structure):
    """Mirror of ``ba_covis_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_active", C.c_int32),
        ("n_edges", C.c_int32),
        ("n_components", C.c_int32),
        ("band_before", C.c_int32),
        ("band_after", C.c_int32),
        ("wide_before", C.c_int32),
        ("wide_after", C.c_int32),
        ("order_changed", C.c_int32),
        ("reserved0", C.c_int32),
        ("time_count_ms", C.c_double),
        ("time_order_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved0")}


_u8p = C.POINTER(C.c_uint8)


class BaLocalRequest(C.Structure):
    """Mirror of ``ba_local_request`` (ba_local_window / ba_solve_local). ``struct_size`` is set to this mirror's size
    on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("center", C.c_int32),
        ("min_weight", C.c_int32),
        ("max_local", C.c_int32),
        ("w", _ip),
        ("cam_index", _ip),
        ("cam_constant", _u8p),
        ("cam_local", _u8p),
        ("pt_index", _ip),
        ("obs_index", _ip),
        ("sub_obs_cam", _ip),
        ("sub_obs_pt", _ip),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaLocalInfo(C.Structure):
    """Mirror of ``ba_local_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_local", C.c_int32),
        ("n_fixed", C.c_int32),
        ("n_points", C.c_int32),
        ("n_obs", C.c_int32),
        ("sub_fixed_cam", C.c_int32),
        ("time_select_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


LOC_STAT_N = 8  # BA_LOC_STAT_N
LOC_STAT_FIELDS = ("n_obs", "initial_cost", "final_cost", "iterations", "successful_steps", "unsuccessful_steps",
                   "termination_type", "message_kind")


class BaLocRequest(C.Structure):
    """Mirror of ``ba_loc_request`` (ba_localize). ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("reserved0", C.c_int32),
        ("cam_mask", _u8p),
        ("cam_stats", _dp),
        ("log_cam", C.c_int32),
        ("log_max_rows", C.c_int32),
        ("log_rows", _dp),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaLocInfo(C.Structure):
    """Mirror of ``ba_loc_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_selected", C.c_int32),
        ("n_solved", C.c_int32),
        ("n_convergence", C.c_int32),
        ("n_no_convergence", C.c_int32),
        ("n_failure", C.c_int32),
        ("max_iterations", C.c_int32),
        ("log_rows", C.c_int32),
        ("time_lm_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


PTS_STAT_N = 8  # BA_PTS_STAT_N (the fields of LOC_STAT_FIELDS, per point)


class BaPtsRequest(C.Structure):
    """Mirror of ``ba_pts_request`` (ba_refine_points). ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("min_obs", C.c_int32),
        ("pt_mask", _u8p),
        ("pt_stats", _dp),
        ("log_pt", C.c_int32),
        ("log_max_rows", C.c_int32),
        ("log_rows", _dp),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaPtsInfo(C.Structure):
    """Mirror of ``ba_pts_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_selected", C.c_int32),
        ("n_solved", C.c_int32),
        ("n_convergence", C.c_int32),
        ("n_no_convergence", C.c_int32),
        ("n_failure", C.c_int32),
        ("max_iterations", C.c_int32),
        ("log_rows", C.c_int32),
        ("time_lm_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class BaPgProblem(C.Structure):
    """Mirror of ``ba_pg_problem`` (ba_pose_graph): a plain struct like ``ba_problem``."""

    _fields_ = [
        ("n_cams", C.c_int32),
        ("n_edges", C.c_int32),
        ("cams", _dp),
        ("edge_a", _ip),
        ("edge_b", _ip),
        ("edge_meas", _dp),
        ("edge_weight", _dp),
        ("is_constant", _u8p),
        ("fixed_cam", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class BaPgRequest(C.Structure):
    """Mirror of ``ba_pg_request``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("log_max_rows", C.c_int32),
        ("huber", C.c_double),
        ("log", _dp),
        ("cam_order", _ip),
        ("edge_cost", _dp),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaPgInfo(C.Structure):
    """Mirror of ``ba_pg_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_active", C.c_int32),
        ("n_edges_used", C.c_int32),
        ("n_components", C.c_int32),
        ("band_before", C.c_int32),
        ("band_after", C.c_int32),
        ("reduced_system_size", C.c_int32),
        ("iterations", C.c_int32),
        ("n_successful", C.c_int32),
        ("n_unsuccessful", C.c_int32),
        ("termination_type", C.c_int32),
        ("log_rows", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("time_kernels_ms", C.c_double),
        ("time_solve_ms", C.c_double),
        ("time_order_ms", C.c_double),
        ("time_total_ms", C.c_double),
        ("message", C.c_char * 160),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}
        d["message"] = self.message.decode(errors="replace")
        return d


PG_MAX_NPAD = 8192  # BA_PG_MAX_NPAD


class BaAlignProblem(C.Structure):
    """Mirror of ``ba_align_problem`` (ba_align): a plain struct like ``ba_problem``."""

    _fields_ = [
        ("n_pairs", C.c_int32),
        ("n_corr", C.c_int32),
        ("pair_begin", _ip),
        ("p1", _dp),
        ("p2", _dp),
    ]


class BaAlignRequest(C.Structure):
    """Mirror of ``ba_align_request``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_hypotheses", C.c_int32),
        ("refit", C.c_int32),
        ("reserved0", C.c_int32),
        ("seed", C.c_uint64),
        ("threshold", C.c_double),
        ("min_cross", C.c_double),
        ("probability", C.c_double),
        ("poses", _dp),
        ("pair_stats", _dp),
        ("inlier", _u8p),
        ("hyp_count", _ip),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaAlignInfo(C.Structure):
    """Mirror of ``ba_align_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_pairs", C.c_int32),
        ("n_ok", C.c_int32),
        ("n_too_few", C.c_int32),
        ("n_no_model", C.c_int32),
        ("n_hypotheses", C.c_int32),
        ("time_kernels_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


ALIGN_STAT_N = 8  # BA_ALIGN_STAT_N
ALIGN_MAX_HYP = 65536  # BA_ALIGN_MAX_HYP
ALIGN_OK, ALIGN_TOO_FEW, ALIGN_NO_MODEL = 0, 1, 2  # BA_ALIGN_OK / _TOO_FEW / _NO_MODEL


class BaMatchProblem(C.Structure):
    """Mirror of ``ba_match_problem`` (ba_match): a plain struct like ``ba_problem``."""

    _fields_ = [
        ("kind", C.c_int32),
        ("desc_bytes", C.c_int32),
        ("n_query", C.c_int32),
        ("n_train", C.c_int32),
        ("n_pairs", C.c_int32),
        ("n_rows", C.c_int32),
        ("query", _u8p),
        ("train", _u8p),
        ("pair_range", _ip),
    ]


class BaMatchRequest(C.Structure):
    """Mirror of ``ba_match_request``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("cross_check", C.c_int32),
        ("ratio", C.c_float),
        ("max_distance", C.c_int32),
        ("nn_idx", _ip),
        ("nn_dist", _ip),
        ("accept", _u8p),
        ("matches", _ip),
        ("match_begin", _ip),
        ("pair_counts", _ip),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaMatchInfo(C.Structure):
    """Mirror of ``ba_match_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_pairs", C.c_int32),
        ("n_rows", C.c_int32),
        ("n_matches", C.c_int32),
        ("kind", C.c_int32),
        ("reserved0", C.c_int32),
        ("time_kernels_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved0")}


MATCH_HAMMING, MATCH_L2_U8 = 0, 1  # BA_MATCH_HAMMING / BA_MATCH_L2_U8
MATCH_KINDS = {"hamming": MATCH_HAMMING, "l2_u8": MATCH_L2_U8}
MATCH_MAX_BYTES = 256  # BA_MATCH_MAX_BYTES
MATCH_COUNT_N = 7  # BA_MATCH_COUNT_N
# columns of a pair_counts row
MATCH_COUNT_FIELDS = ("n_q", "n_t", "accepted", "no_second", "ratio", "max_distance", "cross_check")


class BaGmatchProblem(C.Structure):
    """Mirror of ``ba_gmatch_problem`` (ba_guided_match): a plain struct like ``ba_match_problem``."""

    _fields_ = [
        ("kind", C.c_int32),
        ("desc_bytes", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_kp", C.c_int32),
        ("n_points", C.c_int32),
        ("n_frames", C.c_int32),
        ("n_rows", C.c_int32),
        ("intr", C.c_double * 4),
        ("kp_uv", _dp),
        ("kp_desc", _u8p),
        ("kp_depth", _dp),
        ("points", _dp),
        ("pt_desc", _u8p),
        ("frame_pose", _dp),
        ("frame_range", _ip),
        ("cand_begin", _ip),
        ("cand_pt", _ip),
    ]


class BaGmatchRequest(C.Structure):
    """Mirror of ``ba_gmatch_request``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("one_to_one", C.c_int32),
        ("radius", C.c_double),
        ("ratio", C.c_float),
        ("max_distance", C.c_int32),
        ("min_depth", C.c_double),
        ("depth_tol", C.c_double),
        ("cell_px", C.c_int32),
        ("reserved0", C.c_int32),
        ("nn_kp", _ip),
        ("nn_dist", _ip),
        ("status", _u8p),
        ("proj", _dp),
        ("n_in_window", _ip),
        ("matches", _ip),
        ("match_begin", _ip),
        ("frame_counts", _ip),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class BaGmatchInfo(C.Structure):
    """Mirror of ``ba_gmatch_info``. ``struct_size`` is set to this mirror's size on construction."""

    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_frames", C.c_int32),
        ("n_rows", C.c_int32),
        ("n_matches", C.c_int32),
        ("kind", C.c_int32),
        ("n_grids", C.c_int32),
        ("cell_px", C.c_int32),
        ("reserved0", C.c_int32),
        ("time_kernels_ms", C.c_double),
        ("time_total_ms", C.c_double),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved0")}


GMATCH_COUNT_N = 9  # BA_GMATCH_COUNT_N
# columns of a frame_counts row: the candidates, the keypoints of the range, then the rows of every status value
GMATCH_COUNT_FIELDS = ("n_cand", "n_kp", "accepted", "behind", "outside", "empty_window", "ratio", "max_distance",
                       "one_to_one")
# ba_guided_match's status values, by name
GMATCH_STATUS = {name: i for i, name in enumerate(GMATCH_COUNT_FIELDS[2:])}


def default_options_py() -> BaOptions:
    """Pure-Python defaults (used only where no compiled library is loaded)."""
    o = BaOptions()
    o.hub_p_repr = 1e-3
    o.hub_p_unpr = 1e-3
    o.weight_intrinsics = 1e-6
    o.weight_unpr = 10.0
    o.max_num_iterations = 75
    o.minimizer_progress_to_stdout = 1
    o.eta = 1e-6
    o.initial_trust_region_radius = 1e4
    o.max_trust_region_radius = 1e16
    o.min_trust_region_radius = 1e-32
    o.min_relative_decrease = 1e-3
    o.min_lm_diagonal = 1e-6
    o.max_lm_diagonal = 1e32
    o.max_num_consecutive_invalid_steps = 5
    o.jacobi_scaling = 1
    o.function_tolerance = 1e-6
    o.gradient_tolerance = 1e-10
    o.parameter_tolerance = 1e-8
    o.device = -1
    o.deterministic = 0  # = ba_default_options
    o.shard_min_obs = 262144
    o.small_window = 0
    o.rebuild_plan = 0  # reuse the host plan of an unchanged window structure
    return o


@dataclass
class ProblemArrays:
    """Owning numpy view of one window problem; ``.struct()`` gives a ``BaProblem``."""

    cams: np.ndarray  # (n_cams, 7) qx qy qz qw tx ty tz
    points: np.ndarray  # (n_points, 3)
    intr: np.ndarray  # (4,)
    intr_prior: np.ndarray  # (4,)
    obs_cam: np.ndarray  # (n_obs,) int32
    obs_pt: np.ndarray  # (n_obs,) int32
    obs_uv: np.ndarray  # (n_obs, 2)
    obs_depth: np.ndarray  # (n_obs,)
    fixed_cam: int = 0
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.cams = np.ascontiguousarray(self.cams, dtype=np.float64).reshape(-1, 7)
        self.points = np.ascontiguousarray(self.points, dtype=np.float64).reshape(-1, 3)
        self.intr = np.ascontiguousarray(self.intr, dtype=np.float64).reshape(4)
        self.intr_prior = np.ascontiguousarray(self.intr_prior, dtype=np.float64).reshape(4)
        self.obs_cam = np.ascontiguousarray(self.obs_cam, dtype=np.int32).reshape(-1)
        self.obs_pt = np.ascontiguousarray(self.obs_pt, dtype=np.int32).reshape(-1)
        self.obs_uv = np.ascontiguousarray(self.obs_uv, dtype=np.float64).reshape(-1, 2)
        self.obs_depth = np.ascontiguousarray(self.obs_depth, dtype=np.float64).reshape(-1)

    @property
    def n_cams(self) -> int:
        return self.cams.shape[0]

    @property
    def n_points(self) -> int:
        return self.points.shape[0]

    @property
    def n_obs(self) -> int:
        return self.obs_cam.shape[0]

    def copy(self) -> "ProblemArrays":
        return ProblemArrays(
            self.cams.copy(), self.points.copy(), self.intr.copy(), self.intr_prior.copy(),
            self.obs_cam.copy(), self.obs_pt.copy(), self.obs_uv.copy(), self.obs_depth.copy(),
            int(self.fixed_cam), dict(self.meta),
        )

    def struct(self) -> BaProblem:
        p = BaProblem()
        p.n_cams = self.n_cams
        p.n_points = self.n_points
        p.n_obs = self.n_obs
        p.fixed_cam = int(self.fixed_cam)
        p.cams = self.cams.ctypes.data_as(_dp)
        p.points = self.points.ctypes.data_as(_dp)
        p.intr = self.intr.ctypes.data_as(_dp)
        p.intr_prior = self.intr_prior.ctypes.data_as(_dp)
        p.obs_cam = self.obs_cam.ctypes.data_as(_ip)
        p.obs_pt = self.obs_pt.ctypes.data_as(_ip)
        p.obs_uv = self.obs_uv.ctypes.data_as(_dp)
        p.obs_depth = self.obs_depth.ctypes.data_as(_dp)
        return p

    def save_npz(self, path) -> None:
        np.savez(path, cams=self.cams, points=self.points, intr=self.intr, intr_prior=self.intr_prior,
                 obs_cam=self.obs_cam, obs_pt=self.obs_pt, obs_uv=self.obs_uv, obs_depth=self.obs_depth,
                 fixed_cam=np.int32(self.fixed_cam))

    @staticmethod
    def load_npz(path) -> "ProblemArrays":
        z = np.load(path, allow_pickle=False)
        return ProblemArrays(z["cams"], z["points"], z["intr"], z["intr_prior"], z["obs_cam"], z["obs_pt"],
                             z["obs_uv"], z["obs_depth"], int(z["fixed_cam"]))
