"""Reference of the residual report, ba_residuals (test infrastructure).

``evaluate`` restates the report from the formulas of include/ba.h and DESIGN §1 in numpy, in ``np.longdouble`` (the
reference) or in plain float64 (whose only purpose is to measure what rounding does to each quantity). It shares no
code with the device functions or with the oracle:

    R = R(q), q = (qx, qy, qz, qw) unnormalised as Eigen's toRotationMatrix;   p_c = R^T (X - t)
    u = fx x / z + cx,  v = fy y / z + cy;   du = u - u_o, dv = v - v_o, dd = depth - z
    s_r = (du^2 + dv^2) / N,  s_d = WEIGHT_UNPR dd^2 / N,  N = admissible observations (depth > 1e-15)
    rho(s, a) = s  if s <= a^2  else  2 a sqrt(s) - a^2;      cost_obs = rho(s_r, a_r) / 2 + rho(s_d, a_d) / 2
    prior_cost = WEIGHT_INTRINSICS |prior - K|^2 / 2

and the flags, block statistics and window totals as include/ba.h states them.

Tolerances. MEASURED_GAP is the largest difference between the float64 and the longdouble evaluation over every
window and both parameter sets of test_gpu_resid.py (test_refresid.py measures it again and asserts the constants
still cover it). The device gets 16 x that: its operation sequence is different but equally short (explicit FMAs, a
reciprocal refined by two Newton steps in place of a division). GAP = 1000 x the tolerance is the distance every
reference value keeps from every threshold the tests use (3 px, the depth test, both Huber boundaries, z = 0), so a
flag cannot flip within the tolerance.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import refschur
import refstep

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)

INADMISSIBLE, BEHIND, REPROJ, DEPTH, HUBER_REPR, HUBER_UNPR = 1, 2, 4, 8, 16, 32
OUTLIER = BEHIND | REPROJ | DEPTH

# the thresholds of the GPU tests
MAX_REPROJ_PX, MAX_DEPTH_ABS, MAX_DEPTH_REL = 3.0, 0.0, 0.05

STEP_WINDOWS = ("one1", "one2", "bcr21_messy", "inactive_mid21", "gauge_mid21", "nb37_b2_f32")
SCHUR_WINDOWS = ("spans_f32", "spans", "gauge_only", "obs256", "obs257", "bs_long", "short400")
WINDOWS = STEP_WINDOWS + SCHUR_WINDOWS
CULL_WINDOWS = ("bcr21_messy", "spans", "short400")
PARAM_SETS = ("start", "solved")

# max |float64 - longdouble| of du / dv [px], depth - z, z, and of obs_cost relative to itself, measured by
# test_refresid.py::test_rounding_constants over WINDOWS x PARAM_SETS
# (measured: uv 1.75e-13, spans start; dd = z 9.3e-16, gauge_mid21 start; cost 1.49e-3, gauge_only solved)
MEASURED_GAP = dict(uv=1.8e-13, dd=9.5e-16, z=9.5e-16, cost=1.5e-3)
TOL = {k: 16.0 * v for k, v in MEASURED_GAP.items()}
GAP = {k: 1000.0 * v for k, v in TOL.items()}
assert TOL["uv"] < 1e-9, "the du / dv tolerance must stay far below the nearest threshold gap (1.9e-5 px)"
# obs_cost relative to itself is ill-conditioned where a residual nearly vanishes (a point that hangs on one
# observation is fitted to 1e-7 px, and its cost carries the relative rounding of du twice: 1.5e-3 on gauge_only),
# so that tolerance says little. cost_bound is the bound that follows from the error tolerances themselves: the cost
# is rho(s_r) / 2 + rho(s_d) / 2 with 0 < rho' <= 1, so an error e_uv in du and dv and e_dd in dd moves it by at most
# ((|du| + |dv|) e_uv + e_uv^2 + WEIGHT_UNPR (|dd| e_dd + e_dd^2 / 2)) / N, plus COST_EPS roundings of the evaluation
# itself (a dozen operations from the residuals to the cost). The GPU test asserts both.
COST_EPS = 16


def cost_bound(ref, opts=None, e_uv=None, e_dd=None):
    """Per observation: how far an obs_cost may be from the reference's when its du / dv and depth - z are within
    e_uv / e_dd (default TOL) of the reference's."""
    opts = _options(opts)
    e_uv = LD(TOL["uv"] if e_uv is None else e_uv)
    e_dd = LD(TOL["dd"] if e_dd is None else e_dd)
    du, dv, dd = np.abs(ref.err[:, 0]), np.abs(ref.err[:, 1]), np.abs(ref.err[:, 2])
    w = LD(opts.weight_unpr)
    return ((du + dv) * e_uv + e_uv * e_uv + w * (dd * e_dd + e_dd * e_dd / 2)) / ref.N + COST_EPS * EPS64 * ref.cost

_cache = {}


def window(name):
    """The window ``name`` of refstep / refschur (cached there; callers must not modify it)."""
    return refstep.window(name) if name in refstep.WINDOWS else refschur.window(name)


def solved(name):
    """The window after oracle.solve (cached; callers must not modify it)."""
    from oracle import oracle
    if ("s", name) not in _cache:
        p = window(name).copy()
        s = oracle.solve(p)
        p.meta["oracle_summary"] = s
        _cache[("s", name)] = p
    return _cache[("s", name)]


def params(name, which):
    return window(name) if which == "start" else solved(name)


def _options(opts):
    if opts is None:
        from miba.capi import default_options_py
        opts = default_options_py()
    return opts


def evaluate(prob, opts=None, max_reproj_px=0.0, max_depth_abs=0.0, max_depth_rel=0.0, dtype=LD):
    """The report of ``prob`` at its parameters, every array in the caller's order: err (n_obs, 4), cost, flags,
    depth_culled, cam_stats (n_cams, 6), point_stats (n_points, 6), the window totals under ba_res_info's names,
    and s_r / s_d (the Huber arguments), hyp (sqrt(du^2 + dv^2)) for the gap conditions."""
    opts = _options(opts)
    T = dtype
    n = prob.n_obs
    depth64 = prob.obs_depth
    adm = depth64 > 1e-15
    N = T(max(int(adm.sum()), 1))
    cam = prob.obs_cam.astype(np.int64)
    pt = prob.obs_pt.astype(np.int64)
    q = prob.cams[cam].astype(T)
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    d = prob.points[pt].astype(T) - q[:, 4:7]
    two = T(2)
    one = T(1)
    # columns of R: p_c = R^T d
    r00 = one - two * (qy * qy + qz * qz); r10 = two * (qx * qy + qw * qz); r20 = two * (qx * qz - qw * qy)
    r01 = two * (qx * qy - qw * qz); r11 = one - two * (qx * qx + qz * qz); r21 = two * (qy * qz + qw * qx)
    r02 = two * (qx * qz + qw * qy); r12 = two * (qy * qz - qw * qx); r22 = one - two * (qx * qx + qy * qy)
    x = r00 * d[:, 0] + r10 * d[:, 1] + r20 * d[:, 2]
    y = r01 * d[:, 0] + r11 * d[:, 1] + r21 * d[:, 2]
    z = r02 * d[:, 0] + r12 * d[:, 1] + r22 * d[:, 2]
    fx, fy, cx, cy = (T(v) for v in prob.intr)
    depth = depth64.astype(T)
    with np.errstate(all="ignore"):
        u = fx * x / z + cx
        v = fy * y / z + cy
        du = u - prob.obs_uv[:, 0].astype(T)
        dv = v - prob.obs_uv[:, 1].astype(T)
        dd = depth - z
        s2 = du * du + dv * dv
        hyp = np.sqrt(s2)
        s_r = s2 / N
        s_d = T(opts.weight_unpr) * dd * dd / N
        a_r, a_d = T(opts.hub_p_repr), T(opts.hub_p_unpr)

        def rho(s, a):
            return np.where(s > a * a, two * a * np.sqrt(s) - a * a, s)

        cost = rho(s_r, a_r) / two + rho(s_d, a_d) / two
        flags = np.zeros(n, np.int32)
        flags[~(z > 0) | ~np.isfinite(u) | ~np.isfinite(v)] |= BEHIND
        if max_reproj_px > 0:
            flags[hyp > T(max_reproj_px)] |= REPROJ
        if max_depth_abs > 0 or max_depth_rel > 0:
            flags[np.abs(dd) > T(max(max_depth_abs, 0.0)) + T(max(max_depth_rel, 0.0)) * depth] |= DEPTH
        flags[s_r > a_r * a_r] |= HUBER_REPR
        flags[s_d > a_d * a_d] |= HUBER_UNPR
    nan = T(np.nan)
    err = np.stack([du, dv, dd, z], 1)
    err[~adm] = nan
    cost = np.where(adm, cost, nan)
    flags[~adm] = INADMISSIBLE
    proj = adm & ((flags & BEHIND) == 0)
    out_mask = adm & ((flags & OUTLIER) != 0)

    def stats(idx, nb):
        st = np.zeros((nb, 6), T)
        np.add.at(st[:, 0], idx[adm], one)
        np.add.at(st[:, 1], idx[out_mask], one)
        np.add.at(st[:, 2], idx[proj], s2[proj])
        np.maximum.at(st[:, 3], idx[proj], hyp[proj])
        np.add.at(st[:, 4], idx[proj], (dd * dd)[proj])
        np.add.at(st[:, 5], idx[adm], cost[adm])
        return st

    w = prob.intr_prior.astype(T) - prob.intr.astype(T)
    prior_cost = T(opts.weight_intrinsics) * (w * w).sum() / two
    n_proj = int(proj.sum())
    res = SimpleNamespace(
        err=err, cost=cost, flags=flags, adm=adm, proj=proj, hyp=hyp, s_r=s_r, s_d=s_d, N=N,
        depth_culled=np.where(out_mask, 0.0, depth64),
        cam_stats=stats(cam, prob.n_cams), point_stats=stats(pt, prob.n_points),
        n_admissible=int(adm.sum()), n_outliers=int(out_mask.sum()),
        n_behind=int((adm & ((flags & BEHIND) != 0)).sum()), n_reproj=int((adm & ((flags & REPROJ) != 0)).sum()),
        n_depth=int((adm & ((flags & DEPTH) != 0)).sum()),
        n_huber_repr=int((adm & ((flags & HUBER_REPR) != 0)).sum()),
        n_huber_unpr=int((adm & ((flags & HUBER_UNPR) != 0)).sum()),
        prior_cost=prior_cost, total_cost=cost[adm].sum() + prior_cost,
        rms_reproj_px=np.sqrt(s2[proj].sum() / n_proj) if n_proj else T(0),
        max_reproj_px=hyp[proj].max() if n_proj else T(0),
        rms_depth=np.sqrt((dd * dd)[proj].sum() / n_proj) if n_proj else T(0),
        max_depth=np.abs(dd)[proj].max() if n_proj else T(0),
    )
    return res


def reference(name, which, thresholds=True):
    """``evaluate`` of window ``name`` at the parameter set ``which`` with the GPU tests' thresholds (cached)."""
    key = ("e", name, which, thresholds)
    if key not in _cache:
        thr = (MAX_REPROJ_PX, MAX_DEPTH_ABS, MAX_DEPTH_REL) if thresholds else (0.0, 0.0, 0.0)
        _cache[key] = evaluate(params(name, which), None, *thr)
    return _cache[key]


def rounding_gap(prob, opts=None):
    """max |float64 - longdouble| over the admissible, projected observations: du / dv, depth - z, z, and obs_cost
    relative to itself."""
    a = evaluate(prob, opts, dtype=np.float64)
    b = evaluate(prob, opts, dtype=LD)
    m = b.proj
    e = np.abs(a.err[m].astype(LD) - b.err[m])
    rel = np.abs(a.cost[m].astype(LD) - b.cost[m]) / b.cost[m]
    return dict(uv=float(e[:, :2].max()), dd=float(e[:, 2].max()), z=float(e[:, 3].max()), cost=float(rel.max()))


def behind_case(kind):
    """one2 with the point of camera 1's first observation mirrored through that camera's centre (``mirror``: z < 0,
    the same pixel) or put on it (``on``: z = 0, the pixel is not finite): (window, that observation, its point),
    cached."""
    if ("b", kind) not in _cache:
        p = window("one2").copy()
        k = int(np.nonzero(p.obs_cam == 1)[0][0])
        pt = int(p.obs_pt[k])
        p.points[pt] = 2.0 * p.cams[1, 4:7] - p.points[pt] if kind == "mirror" else p.cams[1, 4:7]
        _cache[("b", kind)] = (p, k, pt)
    return _cache[("b", kind)]


def threshold_gaps(ref, prob, opts=None, max_reproj_px=MAX_REPROJ_PX, max_depth_abs=MAX_DEPTH_ABS,
                   max_depth_rel=MAX_DEPTH_REL, mask=None):
    """The smallest distance of a reference value to each threshold, in the units of the tolerances: reproj [px]
    (the 3 px test), depth (the depth test), huber_repr [px], huber_unpr (depth units), z (from 0); over the
    admissible observations (of ``mask``)."""
    opts = _options(opts)
    m = ref.adm if mask is None else ref.adm & mask
    hyp, dd, z = ref.hyp[m], ref.err[m, 2], ref.err[m, 3]
    depth = prob.obs_depth[m].astype(LD)
    sqN = np.sqrt(ref.N)
    with np.errstate(all="ignore"):
        g = dict(
            reproj=np.abs(hyp - LD(max_reproj_px)).min(),
            depth=np.abs(np.abs(dd) - (LD(max_depth_abs) + LD(max_depth_rel) * depth)).min(),
            huber_repr=np.abs(hyp - LD(opts.hub_p_repr) * sqN).min(),
            huber_unpr=np.abs(np.abs(dd) - LD(opts.hub_p_unpr) * sqN / np.sqrt(LD(opts.weight_unpr))).min(),
            z=np.abs(z).min(),
        )
    return {k: float(v) for k, v in g.items()}


def oracle_cull_loop(name, max_reproj_px=MAX_REPROJ_PX, rounds=2):
    """The cull loop of Solver.solve_culled on the CPU oracle (cached): solve, flag with this module's report at the
    solution, zero the flagged depths in a working copy, solve again from the parameters reached."""
    from oracle import oracle
    key = ("c", name, float(max_reproj_px), rounds)
    if key not in _cache:
        p = window(name).copy()
        culled = np.zeros(p.n_obs, bool)
        summaries, flagged = [], []
        for _ in range(rounds):
            summaries.append(oracle.solve(p))
            rep = evaluate(p, None, max_reproj_px)
            new = (rep.flags & OUTLIER) != 0
            flagged.append(int(new.sum()))
            if not new.any():
                break
            culled |= new
            p.obs_depth[new] = 0.0
        _cache[key] = SimpleNamespace(prob=p, culled=culled, summaries=summaries, flagged=flagged, report=rep)
    return _cache[key]
