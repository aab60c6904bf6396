"""Python front-end of the libmiba C-ABI (include/ba.h).

``Solver`` owns one ``ba_context`` (device buffers cached across calls, like
the reference re-optimising the same window repeatedly, main.cpp:163-168).
``Solver.solve`` is the replacement of ``ceres::Solve`` inside
``windowOptimize`` (OptimizationUtils.cpp:300): it updates the problem's
poses, points and intrinsics in place and returns the summary.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .capi import (COV_INTR, LOG_FIELDS, RES_ERR_N, RES_OUTLIER, RES_STAT_N, BaCovInfo, BaCovRequest, BaCovisInfo,
                   BaCovisRequest, BaKernelStat, BaLocalInfo, BaLocalRequest, BaLocInfo, BaLocRequest, LOC_STAT_N,
                   BaPtsInfo, BaPtsRequest, PTS_STAT_N, BaPgInfo, BaPgProblem, BaPgRequest,
                   ALIGN_STAT_N, BaAlignInfo, BaAlignProblem, BaAlignRequest,
                   MATCH_COUNT_N, MATCH_KINDS, BaMatchInfo, BaMatchProblem, BaMatchRequest,
                   GMATCH_COUNT_N, BaGmatchInfo, BaGmatchProblem, BaGmatchRequest,
                   BaOptions, BaPrepareInfo, BaResInfo, BaResRequest, BaSummary, ProblemArrays)


def default_options(**overrides) -> BaOptions:
    o = BaOptions()
    _lib.lib().ba_default_options(C.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


class MibaError(RuntimeError):
    pass


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Solver:
    def __init__(self, options: BaOptions | None = None, **overrides):
        self._L = _lib.lib()
        self.options = options if options is not None else default_options()
        for k, v in overrides.items():
            setattr(self.options, k, v)
        h = self._L.ba_create(C.byref(self.options))
        if not h:
            raise MibaError("ba_create failed: " + (self._L.ba_last_error(None) or b"").decode())
        self._h = h
        self._cmask = None  # the constant cameras in force (set_constant_cameras), a bool array or None

    def close(self):
        if getattr(self, "_h", None):
            self._L.ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = (self._L.ba_last_error(self._h) or b"").decode()
            raise MibaError(f"{what} failed ({rc}): {msg}")

    def last_error(self) -> str:
        """ba_last_error() of this context: the error of the last failed call, or a note of the last solve."""
        return (self._L.ba_last_error(self._h) or b"").decode()

    def solve(self, prob: ProblemArrays, order=None) -> dict:
        """ba_solve; with ``order`` ba_solve_ordered: ``"auto"`` computes the camera order from the window's
        co-visibility first (ba_covisibility), an array is the order to use (order[k] = the camera placed k-th, as
        ``covisibility`` returns it). The cameras come back in the caller's numbering either way; the summary, the
        iteration log and ``last_prepare`` describe the ordered window."""
        s = BaSummary()
        ps = prob.struct()
        if order is None:
            self._check(self._L.ba_solve(self._h, C.byref(ps), C.byref(s)), "ba_solve")
            return s.as_dict()
        optr = None
        if not (isinstance(order, str) and order == "auto"):
            o = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
            if len(o) != prob.n_cams:
                raise ValueError("order must have one entry per camera")
            optr = o.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._L.ba_solve_ordered(self._h, C.byref(ps), optr, C.byref(s)), "ba_solve_ordered")
        return s.as_dict()

    def covisibility(self, prob: ProblemArrays, weights: bool = True, order: bool = True) -> dict:
        """The keyframe co-visibility graph of the window and the camera order that narrows its band
        (ba_covisibility; ``prob`` is not modified, the context's plan and LM state are not touched).

        ``weights`` (n_cams, n_cams) int32: distinct points two cameras both see through admissible observations, a
        camera's own count on the diagonal. ``order`` (n_cams,) int32: order[k] = the camera placed k-th (the
        identity unless the order narrows the band without widening any point past the Schur tile window). The dict
        also carries the fields of ``ba_covis_info``: n_active, n_edges, n_components, band_before / band_after,
        wide_before / wide_after, order_changed, time_*_ms."""
        i32p = C.POINTER(C.c_int32)
        req, info = BaCovisRequest(), BaCovisInfo()
        out = {}
        if weights:
            out["weights"] = np.zeros((prob.n_cams, prob.n_cams), dtype=np.int32)
            req.weights = out["weights"].ctypes.data_as(i32p)
        if order:
            out["order"] = np.zeros(prob.n_cams, dtype=np.int32)
            req.order = out["order"].ctypes.data_as(i32p)
        ps = prob.struct()
        self._check(self._L.ba_covisibility(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_covisibility")
        out.update(info.as_dict())
        return out

    def set_constant_cameras(self, mask) -> None:
        """ba_set_constant_cameras: ``mask`` (n_cams,) non-zero = the camera's pose is a constant parameter block in
        every later prepare on this solver, in addition to the problem's ``fixed_cam``; ``None`` (or an empty mask)
        clears the set. The mask is copied."""
        if mask is None or len(mask) == 0:
            self._check(self._L.ba_set_constant_cameras(self._h, None, 0), "ba_set_constant_cameras")
            self._cmask = None
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        self._check(self._L.ba_set_constant_cameras(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), len(m)),
                    "ba_set_constant_cameras")
        self._cmask = m.astype(bool)

    def _local_call(self, prob: ProblemArrays, center: int, min_weight: int, max_local: int, summary):
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        req, info = BaLocalRequest(), BaLocalInfo()
        req.center, req.min_weight, req.max_local = int(center), int(min_weight), int(max_local)
        nc, npt, no = max(prob.n_cams, 1), max(prob.n_points, 1), max(prob.n_obs, 1)
        w = np.zeros(nc, dtype=np.int32)
        cam_index = np.zeros(nc, dtype=np.int32)
        cam_constant, cam_local = np.zeros(nc, dtype=np.uint8), np.zeros(nc, dtype=np.uint8)
        pt_index = np.zeros(npt, dtype=np.int32)
        obs_index, sub_cam, sub_pt = (np.zeros(no, dtype=np.int32) for _ in range(3))
        req.w, req.cam_index, req.pt_index = (a.ctypes.data_as(i32p) for a in (w, cam_index, pt_index))
        req.cam_constant, req.cam_local = cam_constant.ctypes.data_as(u8p), cam_local.ctypes.data_as(u8p)
        req.obs_index, req.sub_obs_cam, req.sub_obs_pt = (a.ctypes.data_as(i32p) for a in (obs_index, sub_cam, sub_pt))
        ps = prob.struct()
        if summary is None:
            self._check(self._L.ba_local_window(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_local_window")
        else:
            self._check(self._L.ba_solve_local(self._h, C.byref(ps), C.byref(req), C.byref(info), C.byref(summary)),
                        "ba_solve_local")
        n = info.n_local + info.n_fixed
        out = dict(w=w[: prob.n_cams].copy(), cam_index=cam_index[:n].copy(), cam_constant=cam_constant[:n].astype(bool),
                   cam_local=cam_local[:n].astype(bool), pt_index=pt_index[: info.n_points].copy(),
                   obs_index=obs_index[: info.n_obs].copy(), sub_obs_cam=sub_cam[: info.n_obs].copy(),
                   sub_obs_pt=sub_pt[: info.n_obs].copy())
        out.update(info.as_dict())
        return out

    def local_window(self, prob: ProblemArrays, center: int, min_weight: int = 15, max_local: int = 0) -> dict:
        """The co-visibility-selected window around camera ``center`` of the map ``prob`` (ba_local_window; ``prob`` is
        not modified, the context's plan and LM state are not touched). ``w`` (n_cams,): points shared with the
        centre; ``cam_index``: the sub-window's cameras (local and fixed ones, increasing), ``cam_local`` /
        ``cam_constant`` flags per such camera; ``pt_index``; ``obs_index`` with the renumbered ``sub_obs_cam`` /
        ``sub_obs_pt``; and the fields of ``ba_local_info`` (n_local, n_fixed, n_points, n_obs, sub_fixed_cam,
        time_*_ms)."""
        return self._local_call(prob, center, min_weight, max_local, None)

    def solve_local(self, prob: ProblemArrays, center: int, min_weight: int = 15, max_local: int = 0) -> dict:
        """ba_solve_local: select the window around ``center`` and solve it with its fixed cameras constant; the
        local cameras, the local points and the intrinsics of ``prob`` are updated in place, everything else is
        untouched. Returns the summary of the sub-window's solve with the selection under ``"window"``."""
        s = BaSummary()
        win = self._local_call(prob, center, min_weight, max_local, s)
        d = s.as_dict()
        d["window"] = win
        return d

    def localize(self, prob: ProblemArrays, cams=None, log_cam=None) -> dict:
        """ba_localize: refine the poses of the cameras ``cams`` (indices or a boolean mask of n_cams entries; ``None``:
        every camera) against the points and intrinsics of ``prob`` as they stand, each camera on its own
        observations alone. ``prob.cams`` is updated in place; nothing else in ``prob`` changes and the context's plan
        and LM state are not touched. Returns the fields of ``ba_loc_info``, ``stats`` (n_cams, 8) (see
        ``capi.LOC_STAT_FIELDS``; a camera that was not selected or has no admissible observation has stats[6] = -1)
        and ``log``: camera ``log_cam``'s iteration rows (``iteration_log``'s layout), ``None`` without ``log_cam``."""
        req, info = BaLocRequest(), BaLocInfo()
        nc = prob.n_cams
        if cams is not None:
            c = np.asarray(cams)
            if c.dtype == bool:
                if c.shape != (nc,):
                    raise ValueError("a boolean camera mask must have one entry per camera")
                mask = np.ascontiguousarray(c, dtype=np.uint8)
            else:
                mask = np.zeros(nc, dtype=np.uint8)
                mask[np.asarray(c, dtype=np.int64).reshape(-1)] = 1
            if nc:
                req.cam_mask = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        stats = np.zeros((max(nc, 1), LOC_STAT_N))
        req.cam_stats = _dptr(stats)
        req.log_cam = -1
        log = None
        if log_cam is not None:
            log = np.zeros((max(int(self.options.max_num_iterations), 0) + 1, _lib.LOG_WIDTH))
            req.log_cam, req.log_max_rows, req.log_rows = int(log_cam), log.shape[0], _dptr(log)
        ps = prob.struct()
        self._check(self._L.ba_localize(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_localize")
        out = info.as_dict()
        out["stats"] = stats[:nc]
        out["log"] = None if log is None else log[: min(info.log_rows, log.shape[0])].copy()
        return out

    def refine_points(self, prob: ProblemArrays, points=None, log_pt=None, min_obs: int = 1) -> dict:
        """ba_refine_points: refine the positions of the points ``points`` (indices or a boolean mask of n_points
        entries; ``None``: every point) against the cameras and intrinsics of ``prob`` as they stand, each point on its
        own observations alone; a point with fewer than ``min_obs`` admissible observations is left as it is.
        ``prob.points`` is updated in place; nothing else in ``prob`` changes and the context's plan and LM state are
        not touched. Returns the fields of ``ba_pts_info``, ``stats`` (n_points, 8) (see ``capi.LOC_STAT_FIELDS``; a
        point that was not selected or has too few admissible observations has stats[6] = -1) and ``log``: point
        ``log_pt``'s iteration rows (``iteration_log``'s layout), ``None`` without ``log_pt``."""
        req, info = BaPtsRequest(), BaPtsInfo()
        npt = prob.n_points
        req.min_obs = int(min_obs)
        if points is not None:
            c = np.asarray(points)
            if c.dtype == bool:
                if c.shape != (npt,):
                    raise ValueError("a boolean point mask must have one entry per point")
                mask = np.ascontiguousarray(c, dtype=np.uint8)
            else:
                mask = np.zeros(npt, dtype=np.uint8)
                mask[np.asarray(c, dtype=np.int64).reshape(-1)] = 1
            if npt:
                req.pt_mask = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        stats = np.zeros((max(npt, 1), PTS_STAT_N))
        req.pt_stats = _dptr(stats)
        req.log_pt = -1
        log = None
        if log_pt is not None:
            log = np.zeros((max(int(self.options.max_num_iterations), 0) + 1, _lib.LOG_WIDTH))
            req.log_pt, req.log_max_rows, req.log_rows = int(log_pt), log.shape[0], _dptr(log)
        ps = prob.struct()
        self._check(self._L.ba_refine_points(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_refine_points")
        out = info.as_dict()
        out["stats"] = stats[:npt]
        out["log"] = None if log is None else log[: min(info.log_rows, log.shape[0])].copy()
        return out

    def pose_graph(self, cams, edge_a, edge_b, meas, weights=None, constant=None, fixed_cam: int = -1,
                   huber: float = 0.0, log: bool = False) -> dict:
        """ba_pose_graph: Levenberg-Marquardt over the poses ``cams`` (n, 7), updated in place (a float64
        C-contiguous array; anything else is solved on a copy, returned under ``"cams"``), against the relative-pose
        edges ``edge_a``, ``edge_b`` (m,), ``meas`` (m, 7) = T_a^-1 T_b, with optional ``weights`` (m, 2) = (w_t, w_r)
        and a Huber parameter. ``constant`` (indices or a boolean mask) and ``fixed_cam`` name the constant poses. The
        context's plan and LM state are not touched. Returns the fields of ``ba_pg_info``, ``cams``, ``cam_order``
        (n,), ``edge_cost`` (m,) and ``log`` (``iteration_log``'s layout; ``None`` unless ``log``)."""
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        x = cams if (isinstance(cams, np.ndarray) and cams.dtype == np.float64 and cams.flags.c_contiguous) else \
            np.ascontiguousarray(cams, dtype=np.float64)
        if x.size % 7:
            raise ValueError("cams must hold 7 values per pose")
        n = x.size // 7
        ea = np.ascontiguousarray(edge_a, dtype=np.int32).reshape(-1)
        eb = np.ascontiguousarray(edge_b, dtype=np.int32).reshape(-1)
        z = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 7)
        m = len(ea)
        if len(eb) != m or len(z) != m:
            raise ValueError("edge_a, edge_b and meas must have one entry per edge")
        g = BaPgProblem()
        g.n_cams, g.n_edges, g.fixed_cam = n, m, int(fixed_cam)
        g.cams = _dptr(x) if n else None
        if m:
            g.edge_a, g.edge_b, g.edge_meas = ea.ctypes.data_as(i32p), eb.ctypes.data_as(i32p), _dptr(z)
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, 2)
            if len(w) != m:
                raise ValueError("weights must have one (w_t, w_r) pair per edge")
            if m:
                g.edge_weight = _dptr(w)
        if constant is not None:
            c = np.asarray(constant)
            if c.dtype == bool:
                if c.shape != (n,):
                    raise ValueError("a boolean constant mask must have one entry per pose")
                mask = np.ascontiguousarray(c, dtype=np.uint8)
            else:
                mask = np.zeros(n, dtype=np.uint8)
                mask[np.asarray(c, dtype=np.int64).reshape(-1)] = 1
            if n:
                g.is_constant = mask.ctypes.data_as(u8p)
        req, info = BaPgRequest(), BaPgInfo()
        req.huber = float(huber)
        order = np.zeros(max(n, 1), dtype=np.int32)
        ecost = np.zeros(max(m, 1))
        req.cam_order, req.edge_cost = order.ctypes.data_as(i32p), _dptr(ecost)
        rows = None
        if log:
            rows = np.zeros((max(int(self.options.max_num_iterations), 0) + 1, _lib.LOG_WIDTH))
            req.log_max_rows, req.log = rows.shape[0], _dptr(rows)
        self._check(self._L.ba_pose_graph(self._h, C.byref(g), C.byref(req), C.byref(info)), "ba_pose_graph")
        out = info.as_dict()
        out["cams"] = x if x.ndim == 2 else x.reshape(-1, 7)
        out["cam_order"] = order[:n]
        out["edge_cost"] = ecost[:m]
        out["log"] = None if rows is None else rows[: min(info.log_rows, rows.shape[0])].copy()
        return out

    def align(self, p1, p2, pair_begin=None, threshold: float = 0.1, n_hypotheses: int = 256, seed: int = 0,
              refit: int = 0, min_cross: float = 0.0, probability: float = 0.0, masks: bool = True,
              counts: bool = False) -> dict:
        """ba_align: batched RANSAC relative pose from 3D-3D correspondences. ``p1``, ``p2`` (n, 3): matched points
        in the first and the second frame; ``pair_begin`` (P + 1,): pair j owns the rows [pair_begin[j],
        pair_begin[j + 1]) (``None``: one pair of all rows). Each pair's pose Z has ``p1 ~ R p2 + t``, which is
        ``pose_graph``'s ``meas`` Z_ab = T_a^-1 T_b for p1 in a's frame and p2 in b's. ``refit`` rounds re-estimate
        the best sample's model over its inliers (0: the best minimal sample's model as it is). The context's plan and
        LM state are not touched. Returns the fields of ``ba_align_info``, ``poses`` (P, 7), ``stats`` (P, 8: status,
        n, n_inliers, best_hyp, n_degenerate, the inliers' RMS distance, the best sample's n_inliers, k_needed),
        ``inlier`` (n,) uint8 (``None`` unless ``masks``) and ``hyp_count`` (P, n_hypotheses) int32 (``None`` unless
        ``counts``)."""
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        a = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
        if len(a) != len(b):
            raise ValueError("p1 and p2 must have one row per correspondence")
        n = len(a)
        begin = np.array([0, n], dtype=np.int32) if pair_begin is None else \
            np.ascontiguousarray(pair_begin, dtype=np.int32).reshape(-1)
        if len(begin) < 1:
            raise ValueError("pair_begin must have n_pairs + 1 entries")
        P = len(begin) - 1
        g = BaAlignProblem()
        g.n_pairs, g.n_corr = P, n
        g.pair_begin = begin.ctypes.data_as(i32p)
        if n:
            g.p1, g.p2 = _dptr(a), _dptr(b)
        req, info = BaAlignRequest(), BaAlignInfo()
        req.n_hypotheses, req.refit, req.seed = int(n_hypotheses), int(refit), int(seed) & 0xFFFFFFFFFFFFFFFF
        req.threshold, req.min_cross, req.probability = float(threshold), float(min_cross), float(probability)
        nh = int(n_hypotheses) if int(n_hypotheses) > 0 else 256
        poses = np.zeros((max(P, 1), 7))
        stats = np.zeros((max(P, 1), ALIGN_STAT_N))
        req.poses, req.pair_stats = _dptr(poses), _dptr(stats)
        mask = hyp = None
        if masks:
            mask = np.zeros(max(n, 1), dtype=np.uint8)
            req.inlier = mask.ctypes.data_as(u8p)
        if counts and nh <= _lib.ALIGN_MAX_HYP:
            hyp = np.zeros((max(P, 1), nh), dtype=np.int32)
            req.hyp_count = hyp.ctypes.data_as(i32p)
        self._check(self._L.ba_align(self._h, C.byref(g), C.byref(req), C.byref(info)), "ba_align")
        out = info.as_dict()
        out["poses"] = poses[:P]
        out["stats"] = stats[:P]
        out["inlier"] = None if mask is None else mask[:n]
        out["hyp_count"] = None if hyp is None else hyp[:P]
        return out

    def match(self, query, train, pair_range=None, kind: str = "hamming", ratio: float = 0.7, max_distance: int = 0,
              cross_check: bool = False, matches: bool = True, counts: bool = False) -> dict:
        """ba_match: batched 2-nearest-neighbour descriptor matching with Lowe's ratio test. ``query`` (n_query, B),
        ``train`` (n_train, B) uint8 descriptors of B bytes; ``kind`` ``"hamming"`` (the bytes as bit strings) or
        ``"l2_u8"`` (the bytes as 0..255, squared Euclidean distances). ``pair_range`` (P, 4): pair j matches the
        queries [q_begin, q_end) against the trains [t_begin, t_end) (``None``: one pair over everything); ranges may
        overlap. The context's plan and LM state are not touched. Returns the fields of ``ba_match_info``,
        ``row_begin`` (P + 1,), ``nn_idx`` / ``nn_dist`` (n_rows, 2) int32 (train indices inside the pair's range, -1 =
        none), ``accept`` (n_rows,) uint8, ``matches`` (n_matches, 2) int32 (query, train) local to the pair with
        ``match_begin`` (P + 1,) (``None`` unless ``matches``) and ``pair_counts`` (P, 7: n_q, n_t, accepted, no second
        neighbour, failed the ratio, failed max_distance, failed the cross-check; ``None`` unless ``counts``)."""
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        if kind not in MATCH_KINDS:
            raise ValueError(f"kind must be one of {sorted(MATCH_KINDS)}")
        q = np.ascontiguousarray(query, dtype=np.uint8)
        t = np.ascontiguousarray(train, dtype=np.uint8)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
            raise ValueError("query and train must be (n, desc_bytes) arrays of one descriptor size")
        rng = np.array([[0, len(q), 0, len(t)]], dtype=np.int32) if pair_range is None else \
            np.ascontiguousarray(pair_range, dtype=np.int32).reshape(-1, 4)
        P = len(rng)
        row_begin = np.concatenate([[0], np.cumsum(rng[:, 1].astype(np.int64) - rng[:, 0])])
        n_rows = int(row_begin[-1])
        g = BaMatchProblem()
        g.kind, g.desc_bytes = MATCH_KINDS[kind], q.shape[1]
        g.n_query, g.n_train, g.n_pairs, g.n_rows = len(q), len(t), P, n_rows
        if q.size:
            g.query = q.ctypes.data_as(u8p)
        if t.size:
            g.train = t.ctypes.data_as(u8p)
        if P:
            g.pair_range = rng.ctypes.data_as(i32p)
        req, info = BaMatchRequest(), BaMatchInfo()
        req.cross_check, req.ratio, req.max_distance = int(bool(cross_check)), float(ratio), int(max_distance)
        rows = max(n_rows, 1)
        nn_idx = np.zeros((rows, 2), dtype=np.int32)
        nn_dist = np.zeros((rows, 2), dtype=np.int32)
        accept = np.zeros(rows, dtype=np.uint8)
        req.nn_idx, req.nn_dist, req.accept = nn_idx.ctypes.data_as(i32p), nn_dist.ctypes.data_as(i32p), accept.ctypes.data_as(u8p)
        mlist = mbegin = pcounts = None
        if matches:
            mlist = np.zeros((rows, 2), dtype=np.int32)
            mbegin = np.zeros(P + 1, dtype=np.int32)
            req.matches, req.match_begin = mlist.ctypes.data_as(i32p), mbegin.ctypes.data_as(i32p)
        if counts:
            pcounts = np.zeros((max(P, 1), MATCH_COUNT_N), dtype=np.int32)
            req.pair_counts = pcounts.ctypes.data_as(i32p)
        self._check(self._L.ba_match(self._h, C.byref(g), C.byref(req), C.byref(info)), "ba_match")
        out = info.as_dict()
        out["row_begin"] = row_begin
        out["nn_idx"], out["nn_dist"], out["accept"] = nn_idx[:n_rows], nn_dist[:n_rows], accept[:n_rows]
        out["matches"] = None if mlist is None else mlist[: info.n_matches]
        out["match_begin"] = mbegin
        out["pair_counts"] = None if pcounts is None else pcounts[:P]
        return out

    def guided_match(self, points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width: int, height: int,
                     frame_range=None, cand=None, kp_depth=None, kind: str = "hamming", radius: float = 15.0,
                     ratio: float = 0.7, max_distance: int = 0, min_depth: float = 0.0, depth_tol: float = 0.0,
                     one_to_one: bool = True, cell_px: int = 0, matches: bool = True, counts: bool = False,
                     proj: bool = False) -> dict:
        """ba_guided_match: the descriptor search in a pixel window around projected landmarks. ``points`` (N, 3)
        world-frame landmarks with ``pt_desc`` (N, B) uint8; ``kp_uv`` (K, 2) keypoint pixels with ``kp_desc`` (K, B)
        and optionally ``kp_depth`` (K,); ``frame_pose`` (F, 7) ``T_w_c`` per frame entry; ``intr`` fx, fy, cx, cy of
        the ``width`` x ``height`` image. ``frame_range`` (F, 2): entry f searches the keypoints [begin, end)
        (``None``: all keypoints for every entry; equal ranges are binned once). ``cand``: per entry an array of
        landmark indices (``None``: every landmark for every entry). ``kind`` and the distances are ``match``'s. A
        landmark is matched to the nearest descriptor among the keypoints within ``radius`` pixels of its projection
        (and within ``depth_tol`` relative depth, when > 0 and ``kp_depth`` is given), subject to the ratio test
        against the window's second neighbour, ``max_distance`` and, with ``one_to_one``, to being the best row of
        its entry for that keypoint. The context's plan and LM state are not touched. Returns the fields of
        ``ba_gmatch_info``, ``cand_begin`` (F + 1,), ``cand_pt`` (n_rows,), ``nn_kp`` / ``nn_dist`` (n_rows, 2) int32
        (keypoint indices inside the entry's range, -1 = none), ``status`` (n_rows,) uint8 (``capi.GMATCH_STATUS``),
        ``n_in_window`` (n_rows,), ``matches`` (n_matches, 2) int32 (landmark index, keypoint inside the range) with
        ``match_begin`` (F + 1,) (``None`` unless ``matches``), ``frame_counts`` (F, 9; ``None`` unless ``counts``)
        and ``proj`` (n_rows, 3: u, v, z; ``None`` unless ``proj``)."""
        i32p, u8p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        if kind not in MATCH_KINDS:
            raise ValueError(f"kind must be one of {sorted(MATCH_KINDS)}")
        X = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(kp_uv, dtype=np.float64).reshape(-1, 2)
        pd = np.ascontiguousarray(pt_desc, dtype=np.uint8)
        kd = np.ascontiguousarray(kp_desc, dtype=np.uint8)
        if pd.ndim != 2 or kd.ndim != 2 or pd.shape[1] != kd.shape[1] or len(pd) != len(X) or len(kd) != len(uv):
            raise ValueError("pt_desc and kp_desc must be (n, desc_bytes) arrays of one descriptor size, one row per "
                             "landmark / keypoint")
        poses = np.ascontiguousarray(frame_pose, dtype=np.float64).reshape(-1, 7)
        F = len(poses)
        rng = np.tile(np.array([[0, len(uv)]], dtype=np.int32), (F, 1)) if frame_range is None else \
            np.ascontiguousarray(frame_range, dtype=np.int32).reshape(-1, 2)
        if len(rng) != F:
            raise ValueError("frame_range must have one (begin, end) per frame pose")
        if cand is None:
            cand = [np.arange(len(X), dtype=np.int32)] * F
        if len(cand) != F:
            raise ValueError("cand must have one index array per frame pose")
        cand = [np.asarray(c, dtype=np.int32).reshape(-1) for c in cand]
        cand_begin = np.zeros(F + 1, dtype=np.int32)
        if F:
            cand_begin[1:] = np.cumsum([len(c) for c in cand])
        cand_pt = np.ascontiguousarray(np.concatenate(cand) if F else np.zeros(0), dtype=np.int32)
        n_rows = int(cand_begin[-1])
        dep = None
        if kp_depth is not None:
            dep = np.ascontiguousarray(kp_depth, dtype=np.float64).reshape(-1)
            if len(dep) != len(uv):
                raise ValueError("kp_depth must have one value per keypoint")
        g = BaGmatchProblem()
        g.kind, g.desc_bytes, g.width, g.height = MATCH_KINDS[kind], kd.shape[1], int(width), int(height)
        g.n_kp, g.n_points, g.n_frames, g.n_rows = len(uv), len(X), F, n_rows
        g.intr[:] = [float(v) for v in np.asarray(intr, dtype=np.float64).reshape(4)]
        for name, arr, t in (("kp_uv", uv, f64p), ("kp_desc", kd, u8p), ("kp_depth", dep, f64p), ("points", X, f64p),
                             ("pt_desc", pd, u8p), ("frame_pose", poses, f64p), ("frame_range", rng, i32p),
                             ("cand_pt", cand_pt, i32p)):
            if arr is not None and arr.size:
                setattr(g, name, arr.ctypes.data_as(t))
        if F:
            g.cand_begin = cand_begin.ctypes.data_as(i32p)
        req, info = BaGmatchRequest(), BaGmatchInfo()
        req.one_to_one, req.radius, req.ratio, req.max_distance = int(bool(one_to_one)), float(radius), float(ratio), int(max_distance)
        req.min_depth, req.depth_tol, req.cell_px = float(min_depth), float(depth_tol), int(cell_px)
        rows = max(n_rows, 1)
        nn_kp = np.zeros((rows, 2), dtype=np.int32)
        nn_dist = np.zeros((rows, 2), dtype=np.int32)
        status = np.zeros(rows, dtype=np.uint8)
        n_win = np.zeros(rows, dtype=np.int32)
        req.nn_kp, req.nn_dist = nn_kp.ctypes.data_as(i32p), nn_dist.ctypes.data_as(i32p)
        req.status, req.n_in_window = status.ctypes.data_as(u8p), n_win.ctypes.data_as(i32p)
        mlist = mbegin = fcounts = pr = None
        if matches:
            mlist = np.zeros((rows, 2), dtype=np.int32)
            mbegin = np.zeros(F + 1, dtype=np.int32)
            req.matches, req.match_begin = mlist.ctypes.data_as(i32p), mbegin.ctypes.data_as(i32p)
        if counts:
            fcounts = np.zeros((max(F, 1), GMATCH_COUNT_N), dtype=np.int32)
            req.frame_counts = fcounts.ctypes.data_as(i32p)
        if proj:
            pr = np.zeros((rows, 3), dtype=np.float64)
            req.proj = pr.ctypes.data_as(f64p)
        self._check(self._L.ba_guided_match(self._h, C.byref(g), C.byref(req), C.byref(info)), "ba_guided_match")
        out = info.as_dict()
        out["cand_begin"], out["cand_pt"] = cand_begin, cand_pt
        out["nn_kp"], out["nn_dist"], out["status"], out["n_in_window"] = nn_kp[:n_rows], nn_dist[:n_rows], status[:n_rows], n_win[:n_rows]
        out["matches"] = None if mlist is None else mlist[: info.n_matches]
        out["match_begin"] = mbegin
        out["frame_counts"] = None if fcounts is None else fcounts[:F]
        out["proj"] = None if pr is None else pr[:n_rows]
        return out

    @staticmethod
    def comm_unique_id() -> bytes:
        """RCCL unique id for ba_comm_init (rank 0 creates it, ships it to the other ranks)."""
        L = _lib.lib()
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        rc = L.ba_comm_unique_id(buf)
        if rc != 0:
            raise MibaError(f"ba_comm_unique_id failed ({rc}): {(L.ba_last_error(None) or b'').decode()}")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        """Make this solver one landmark shard of an nranks-way sharded window (collective)."""
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("unique id must be BA_COMM_ID_BYTES long")
        self._check(self._L.ba_comm_init(self._h, nranks, rank, uid), "ba_comm_init")

    def comm_init_host(self, nranks: int, rank: int, allreduce) -> None:
        """Make this solver one landmark shard over a host collective instead of RCCL (ba_comm_init_host).
        ``allreduce(arr, op)`` reduces the numpy array ``arr`` (float64 or int32, a view of libmiba's
        pinned staging buffer) in place across the ranks; op is "sum", "max" or "min"."""
        ops = {0: "sum", 1: "max", 2: "min"}

        def fn(buf, count, dtype, op, user):
            try:
                ct = C.c_double if dtype == 0 else C.c_int32
                arr = np.ctypeslib.as_array((ct * int(count)).from_address(buf))
                allreduce(arr, ops[int(op)])
                return 0
            except Exception as e:  # reported through ba_last_error
                import sys
                print(f"miba host all-reduce failed: {e!r}", file=sys.stderr)
                return -1

        self._allreduce_cb = _lib.ALLREDUCE_FN(fn)  # kept alive as long as the context
        self._check(self._L.ba_comm_init_host(self._h, nranks, rank, self._allreduce_cb, None), "ba_comm_init_host")

    def iteration_log(self) -> np.ndarray:
        """Per-iteration log of the last solve (ba_iteration_log): rows 0..num_iterations of
        cost, cost_change, |gradient|, |step|, tr_ratio, tr_radius, accepted (1/0/-1), 0."""
        n = self._L.ba_iteration_log(self._h, None, 0)
        rows = np.zeros((max(n, 0), _lib.LOG_WIDTH))
        if n > 0:
            self._L.ba_iteration_log(self._h, _dptr(rows), n)
        return rows

    def set_options(self, **changes) -> None:
        for k, v in changes.items():
            setattr(self.options, k, v)
        self._check(self._L.ba_set_options(self._h, C.byref(self.options)), "ba_set_options")

    def prepare(self, prob: ProblemArrays) -> None:
        """Upload the window and build its device structure (ba_prepare)."""
        self._prepared = prob.struct()
        self._check(self._L.ba_prepare(self._h, C.byref(self._prepared)), "ba_prepare")

    def solve_prepared(self, prob: ProblemArrays) -> dict:
        """LM on the resident window from the parameters of the last prepare()."""
        s = BaSummary()
        ps = prob.struct()
        self._check(self._L.ba_solve_prepared(self._h, C.byref(ps), C.byref(s)), "ba_solve_prepared")
        return s.as_dict()

    def plan_digest(self) -> list:
        """ba_debug_plan_digest(): one FNV-1a digest per plan array of the last prepared window (as in HBM)."""
        buf = (C.c_uint64 * 64)()
        n = self._L.ba_debug_plan_digest(self._h, buf, 64)
        if n < 0:
            self._check(n, "ba_debug_plan_digest")
        return [int(buf[k]) for k in range(min(n, 64))]

    def last_prepare(self) -> dict:
        """ba_last_prepare(): whether the last prepare reused the plan, uploaded observations, its phase times and
        the reduced-solve path (bcr_path)."""
        info = BaPrepareInfo()
        self._check(self._L.ba_last_prepare(self._h, C.byref(info)), "ba_last_prepare")
        return info.as_dict()

    def kernel_stats(self) -> list:
        arr = (BaKernelStat * 32)()
        n = self._L.ba_kernel_stats(self._h, arr, 32)
        out = []
        for i in range(n):
            k = arr[i]
            out.append(dict(name=k.name.decode(), launches=k.launches, total_ms=k.total_ms,
                            bytes_per_launch=k.bytes_per_launch, flops_per_launch=k.flops_per_launch))
        return out

    def reset_kernel_stats(self) -> None:
        self._L.ba_reset_kernel_stats(self._h)

    def linearize(self, prob: ProblemArrays) -> dict:
        n = prob.n_obs
        res = np.zeros((n, 3)); jc = np.zeros((n, 3, 6)); jp = np.zeros((n, 3, 3)); jk = np.zeros((n, 2, 4))
        cost = np.zeros(1)
        ps = prob.struct()
        self._check(self._L.ba_debug_linearize(self._h, C.byref(ps), _dptr(cost), _dptr(res), _dptr(jc), _dptr(jp),
                                               _dptr(jk)), "ba_debug_linearize")
        return dict(cost=float(cost[0]), res=res, jcam=jc, jpt=jp, jint=jk)

    def lm_step(self, prob: ProblemArrays, radius: float = 0.0) -> dict:
        """The production LM step of the window's first iteration (ba_debug_step), on the paths the prepare
        chose: ac_cam (nac,), delta_cam (nac, 6), delta_intr (4,), delta_pts (n_points, 3) in parameter space,
        row 1 of the iteration log by name (LOG_FIELDS, ``accepted`` as int), the factorisation ``flag``,
        ``retried``, and the window's ``linear_solver`` (capi.LINEAR_SOLVER_NAMES: 0 dense, 1 band, 2 bcr, 3 blocked),
        ``camera_band``, ``band_tiles`` (banded Cholesky only) and ``num_iterations``. ``prob`` is not modified."""
        ps = prob.struct()
        nc = max(prob.n_cams, 1)
        ac = np.zeros(nc, dtype=np.int32); dc = np.zeros((nc, 6)); dk = np.zeros(4)
        dpt = np.zeros((prob.n_points, 3)); row = np.zeros(_lib.LOG_WIDTH)
        n = C.c_int32(0)
        info = np.zeros(8, dtype=np.int32)  # BA_STEP_INFO_N
        self._step_dims = None
        self._check(self._L.ba_debug_step(self._h, C.byref(ps), radius, C.byref(n),
                                          ac.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(dc), _dptr(dk), _dptr(dpt),
                                          _dptr(row), info.ctypes.data_as(C.POINTER(C.c_int32))), "ba_debug_step")
        self._step_dims = (prob.n_cams, prob.n_points)
        out = dict(ac_cam=ac[: n.value].copy(), delta_cam=dc[: n.value].copy(), delta_intr=dk, delta_pts=dpt,
                   flag=int(info[0]), retried=int(info[1]), linear_solver=int(info[2]), camera_band=int(info[3]),
                   band_tiles=int(info[4]), num_iterations=int(info[5]))
        out.update({k: float(v) for k, v in zip(LOG_FIELDS, row)})
        out["accepted"] = int(row[6])
        return out

    STEP_MSG_KINDS = ("none", "max_iter", "grad_tol", "min_radius", "param_tol", "func_tol", "invalid", "eval_fail",
                      "timeout")

    def lm_step_state(self) -> dict:
        """What the last ``lm_step`` left on the device (ba_debug_step_state; no kernel runs): the
        parameters the step was computed from and the candidate slot (``cams_x`` / ``cams_cand`` (n_cams, 7),
        ``intr_x`` / ``intr_cand`` (4,), ``pts_x`` / ``pts_cand`` (n_points, 3), in the caller's order), the step
        scalars ``mcc``, ``cand``, ``sn2``, ``gmax_pt``, ``bad``, ``xn2``, ``lin`` (cost at x, gradient max-norm of
        cameras + intrinsics), ``log`` (rows 0 and 1 of the iteration log) and the LM state after the decision:
        ``radius``, ``decrease_factor``, ``xnorm2``, ``x_cost``, ``final_cost``, ``cur``, ``termination``, ``msg``
        (one of STEP_MSG_KINDS), ``gmax_ci``, ``initial_cost``, ``iter`` and ``base`` (the slot of x)."""
        if getattr(self, "_step_dims", None) is None:
            raise MibaError("lm_step_state: no lm_step on this solver")
        n_cams, n_points = self._step_dims
        nc, npt = max(n_cams, 1), max(n_points, 1)
        cx = np.zeros((nc, 7)); cc = np.zeros((nc, 7)); kx = np.zeros(4); kc = np.zeros(4)
        px = np.zeros((npt, 3)); pc = np.zeros((npt, 3))
        scal = np.zeros(8); lin = np.zeros(2); log = np.zeros((2, _lib.LOG_WIDTH)); st = np.zeros(12)
        self._check(self._L.ba_debug_step_state(self._h, _dptr(cx), _dptr(cc), _dptr(kx), _dptr(kc), _dptr(px),
                                                _dptr(pc), _dptr(scal), _dptr(lin), _dptr(log), _dptr(st)),
                    "ba_debug_step_state")
        out = dict(cams_x=cx[:n_cams], cams_cand=cc[:n_cams], intr_x=kx, intr_cand=kc,
                   pts_x=px[:n_points], pts_cand=pc[:n_points], lin=lin, log=log)
        out.update({k: float(v) for k, v in zip(("mcc", "cand", "sn2", "gmax_pt", "bad", "xn2"), scal)})
        out.update({k: float(v) for k, v in zip(("radius", "decrease_factor", "xnorm2", "x_cost", "final_cost"), st)})
        out.update(cur=int(st[5]), termination=int(st[6]), msg=self.STEP_MSG_KINDS[int(st[7])], gmax_ci=float(st[8]),
                   initial_cost=float(st[9]), iter=int(st[10]), base=int(st[11]))
        return out

    def camera_sums(self, prob: ProblemArrays):
        """The production camera-side pass (ba_debug_camera_sums): per active camera U (6x6), C (6x4), g (6),
        the lin record (cost, gradient norm, intrinsics block + prior) and the active camera indices."""
        ps = prob.struct()
        n = C.c_int32(0)
        self._check(self._L.ba_debug_camera_sums(self._h, C.byref(ps), C.byref(n), None, None, None),
                    "ba_debug_camera_sums")
        cd = np.zeros((max(n.value, 1), 51)); lin = np.zeros(16); ac = np.zeros(max(n.value, 1), dtype=np.int32)
        self._check(self._L.ba_debug_camera_sums(self._h, C.byref(ps), C.byref(n), _dptr(cd), _dptr(lin),
                                                 ac.ctypes.data_as(C.POINTER(C.c_int32))), "ba_debug_camera_sums")
        cd, ac = cd[: n.value], ac[: n.value]
        U = np.zeros((n.value, 6, 6))
        iu = np.triu_indices(6)
        U[:, iu[0], iu[1]] = cd[:, :21]
        U[:, iu[1], iu[0]] = cd[:, :21]
        return dict(U=U, C=cd[:, 21:45].reshape(-1, 6, 4), g=cd[:, 45:51], lin=lin, ac_cam=ac)

    def reduced_system(self, prob: ProblemArrays, radius: float = 0.0):
        ps = prob.struct()
        n = C.c_int32(0)
        self._check(self._L.ba_debug_reduced_system(self._h, C.byref(ps), radius, C.byref(n), None, None),
                    "ba_debug_reduced_system")
        S = np.zeros((n.value, n.value)); rhs = np.zeros(n.value)
        self._check(self._L.ba_debug_reduced_system(self._h, C.byref(ps), radius, C.byref(n), _dptr(S), _dptr(rhs)),
                    "ba_debug_reduced_system")
        return S, rhs

    def covariance(self, prob: ProblemArrays, pairs=None, points=None, full: bool = False,
                   min_rcond: float = 0.0) -> dict:
        """Covariance of the estimate at ``prob``'s parameters (ba_covariance; ``prob`` is not modified).

        ``pairs``: (a, b) camera indices of the window, ``COV_INTR`` (-1) for the intrinsics; default every active
        camera's diagonal block plus the intrinsics block. ``points``: point indices, ``True`` / ``"all"`` for every
        point, default none. Returns ``pairs`` (the list), ``pair_cov`` (one dim(a) x dim(b) array per pair),
        ``point_idx`` / ``point_cov`` (k, 3, 3), ``full`` ((6 nac + 4)^2, ordered as ``reduced_system``) when asked,
        ``ac_cam`` and the fields of ``ba_cov_info`` (status, n, nac, pivot_min, pivot_max, cost, variance_factor,
        time_*_ms). Units: the cost's (the residuals carry the 1/N weights); the variance factor is not applied."""
        i32p = C.POINTER(C.c_int32)
        adm = np.asarray(prob.obs_depth) > 1e-15
        has = np.zeros(prob.n_cams, bool)
        has[np.asarray(prob.obs_cam)[adm]] = True
        if 0 <= prob.fixed_cam < prob.n_cams:
            has[prob.fixed_cam] = False
        if self._cmask is not None and len(self._cmask) == prob.n_cams:
            has[self._cmask] = False
        ac_cam = np.nonzero(has)[0].astype(np.int32)
        if pairs is None:
            pairs = [(int(c), int(c)) for c in ac_cam] + [(COV_INTR, COV_INTR)]
        pairs = [(int(a), int(b)) for a, b in pairs]
        pa = np.ascontiguousarray([a for a, _ in pairs], dtype=np.int32)
        pb = np.ascontiguousarray([b for _, b in pairs], dtype=np.int32)
        pc = np.zeros((len(pairs), 36))
        if points is None or points is False:
            pidx = np.zeros(0, dtype=np.int32)
        elif points is True or (isinstance(points, str) and points == "all"):
            pidx = np.arange(prob.n_points, dtype=np.int32)
        else:
            pidx = np.ascontiguousarray(points, dtype=np.int32)
        ptc = np.zeros((len(pidx), 3, 3))
        req, info = BaCovRequest(), BaCovInfo()
        req.n_pairs = len(pairs)
        if len(pairs):
            req.pair_a, req.pair_b, req.pair_cov = pa.ctypes.data_as(i32p), pb.ctypes.data_as(i32p), _dptr(pc)
        req.n_points = len(pidx)
        if len(pidx):
            req.point_idx, req.point_cov = pidx.ctypes.data_as(i32p), _dptr(ptc)
        nfull = 6 * len(ac_cam) + 4
        fm = np.zeros((nfull, nfull)) if full else None
        if full:
            req.full = _dptr(fm)
        req.min_reciprocal_condition_number = float(min_rcond)
        ps = prob.struct()
        self._check(self._L.ba_covariance(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_covariance")
        assert not full or info.n == nfull, (info.n, nfull)
        dim = lambda v: 4 if v == COV_INTR else 6
        out = dict(pairs=pairs, pair_cov=[pc[k, : dim(a) * dim(b)].reshape(dim(a), dim(b)).copy()
                                          for k, (a, b) in enumerate(pairs)],
                   point_idx=pidx, point_cov=ptc, ac_cam=ac_cam)
        if full:
            out["full"] = fm
        out.update(info.as_dict())
        return out

    def residuals(self, prob: ProblemArrays, max_reproj_px: float = 0.0, max_depth_abs: float = 0.0,
                  max_depth_rel: float = 0.0, per_obs: bool = True, per_block: bool = True) -> dict:
        """The residual report of the window at ``prob``'s parameters (ba_residuals; ``prob`` is not modified).

        ``per_obs``: ``err`` (n_obs, 4) = du, dv [px], depth - z, z; ``cost`` (n_obs,), the observation's share of
        the solver's cost; ``flags`` (n_obs,) int32, the capi.RES_* bits; ``depth_culled`` (n_obs,), ``obs_depth``
        with the RES_OUTLIER observations set to 0. ``per_block``: ``cam_stats`` (n_cams, 6) and ``point_stats``
        (n_points, 6): admissible, outliers, sum du^2 + dv^2, max sqrt(du^2 + dv^2), sum (depth - z)^2, sum cost.
        All in the caller's order; inadmissible observations are NaN with flag RES_INADMISSIBLE. The dict also
        carries the fields of ``ba_res_info`` (counts, prior_cost, rms / max errors, time_*_ms), its ``cost`` under
        the name ``total_cost``. Thresholds <= 0 switch a test off."""
        i32p = C.POINTER(C.c_int32)
        req, info = BaResRequest(), BaResInfo()
        req.max_reproj_px, req.max_depth_abs, req.max_depth_rel = float(max_reproj_px), float(max_depth_abs), float(max_depth_rel)
        out = {}
        n = prob.n_obs
        if per_obs:
            out.update(err=np.zeros((n, RES_ERR_N)), cost=np.zeros(n), flags=np.zeros(n, dtype=np.int32),
                       depth_culled=np.zeros(n))
            req.obs_err, req.obs_cost, req.obs_depth_culled = _dptr(out["err"]), _dptr(out["cost"]), _dptr(out["depth_culled"])
            req.obs_flags = out["flags"].ctypes.data_as(i32p)
        if per_block:
            out.update(cam_stats=np.zeros((prob.n_cams, RES_STAT_N)), point_stats=np.zeros((prob.n_points, RES_STAT_N)))
            req.cam_stats, req.point_stats = _dptr(out["cam_stats"]), _dptr(out["point_stats"])
        ps = prob.struct()
        self._check(self._L.ba_residuals(self._h, C.byref(ps), C.byref(req), C.byref(info)), "ba_residuals")
        d = info.as_dict()
        d["total_cost"] = d.pop("cost")  # (``cost`` is the per-observation array)
        out.update(d)
        return out

    def solve_culled(self, prob: ProblemArrays, max_reproj_px: float, max_depth_abs: float = 0.0,
                     max_depth_rel: float = 0.0, rounds: int = 2) -> dict:
        """Solve, drop the outliers, solve again (the loop of ORB-SLAM's local BA, on the host): after each solve
        the report at the solution (``residuals`` with the thresholds given); the loop ends when it flags no
        observation that is still in, or after ``rounds`` solves. Flagged observations get depth 0 in a working
        copy of the depths (the solver skips them and N, the normaliser of the weights, counts the rest); the next
        solve starts from the parameters already reached. The caller's observation arrays are never written;
        ``prob``'s cameras, points and intrinsics hold the last solution. Returns ``summaries`` (one per solve),
        ``report`` (the last one) and ``culled`` (n_obs,) bool."""
        work = ProblemArrays(prob.cams, prob.points, prob.intr, prob.intr_prior, prob.obs_cam, prob.obs_pt, prob.obs_uv,
                             prob.obs_depth.copy(), int(prob.fixed_cam))
        culled = np.zeros(prob.n_obs, dtype=bool)
        summaries, report = [], None
        for _ in range(max(int(rounds), 1)):
            summaries.append(self.solve(work))
            report = self.residuals(work, max_reproj_px, max_depth_abs, max_depth_rel, per_block=False)
            new = (report["flags"] & RES_OUTLIER) != 0
            if not new.any():
                break
            culled |= new
            work.obs_depth[new] = 0.0
        return dict(summaries=summaries, report=report, culled=culled)
