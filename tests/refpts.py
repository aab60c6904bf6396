"""References of ba_refine_points (test infrastructure): structure-only Levenberg-Marquardt of one point against
constant cameras and intrinsics. refloc.py with cameras and points swapped.

A *track* is one point with its observations. Its residuals and point Jacobians come from ``oracle.linearize`` on the
one-point sub-problem (every camera kept, only the point's observations, so N is the point's own admissible count):
exactly the weighted, robustified residuals f (n, 3) and Jacobians Jp (n, 3, 3) of the cost ba_refine_points
minimises. The oracle's cost carries the IntrinsicsPrior block, which is constant here; its share is subtracted.

* ``step(lin, opts, radius)``  the first LM step in ``np.longdouble`` (as refloc.step): H = Jp^T Jp, g = Jp^T f, the
  Jacobi scaling s = 1 / (1 + sqrt(diag H)), D^2 = clip(diag(H) s^2, min_lm_diagonal, max_lm_diagonal) / radius, the
  damped scaled system (s H s + D^2) y = s g solved by f64 Cholesky with three refinement passes whose residuals are
  extended precision, delta = -s y; with the model cost change and cond_2 of the system.
* ``step64``  the same arithmetic in plain f64 with no refinement.
* ``lm(prob, p, opts, dtype)``  the whole loop, refloc.lm restated for the three Euclidean parameters of one point
  (the step applied as X + delta, the gradient max-norm max_i |X_i - (X_i + -g_i)|), with the margin of every decision.
* ``tracks_problem(counts, seed)``  a window whose point p has exactly ``counts[p]`` admissible observations.
"""
from __future__ import annotations

import numpy as np

from miba.capi import ProblemArrays
from oracle import oracle
from refloc import (MSG_EVAL_FAIL, MSG_FUNC_TOL, MSG_GRAD_TOL, MSG_INVALID, MSG_MAX_ITER, MSG_MIN_RADIUS,  # noqa: F401
                    MSG_NONE, MSG_PARAM_TOL, MARGIN_MIN, _chol_solve, _mcc, _rodrigues, _system, cached)
from refstep import EPS64, LD

# lanes of a point's group in the kernel (csrc/ba_pts.h PTS_LANES; test_pts_abi.py checks the two agree)
LANES = 16

# The largest f64 ratio |step64 - step|_inf / (cond eps |step|_inf) over every track of test_refpts.py's step cases
# (STEP_COUNTS x STEP_RADII on tracks_problem, and the loop tracks), as test_refpts.py::test_f64_ratio measured it on
# x86-64: 2.00, at 17 observations and radius 1e4 (it asserts that the stored value covers what it measures and is not
# stale by more than a factor two). The 3x3 systems are well conditioned (cond 1.4 .. 14), so the error is the
# rounding of the sums over the observations rather than cond * eps.
F64_RATIO = 2.1
# the step bound's factor: max(8, 4 x the f64 ratio), refloc.STEP_F's rule for refloc.STEP_F's reasons: the 4 for the
# device's own Jacobians (where the restatement uses the oracle's) and its tree-ordered sums
STEP_F = max(8.0, 4.0 * F64_RATIO)


def sub_problem(prob: ProblemArrays, p: int, X=None) -> ProblemArrays:
    """Point p's observations (admissible or not, in the caller's order) as a one-point window over every camera."""
    k = np.nonzero(prob.obs_pt == p)[0]
    pt = np.array(prob.points[p] if X is None else X, dtype=np.float64).reshape(1, 3)
    return ProblemArrays(prob.cams.copy(), pt, prob.intr.copy(), prob.intr_prior.copy(), prob.obs_cam[k].copy(),
                         np.zeros(len(k), dtype=np.int32), prob.obs_uv[k].copy(), prob.obs_depth[k].copy(), fixed_cam=-1)


def linearize(prob: ProblemArrays, p: int, opts=None, X=None):
    """dict(f (n, 3), J (n, 3, 3), cost, n, ok) of track p at ``X`` (default: the problem's)."""
    opts = opts or oracle.default_options()
    sp = sub_problem(prob, p, X)
    lin = oracle.linearize(sp, opts)
    adm = np.nonzero(sp.obs_depth > 1e-15)[0]
    fk = np.sqrt(opts.weight_intrinsics) * (sp.intr_prior - sp.intr)
    cost = lin["cost"] - 0.5 * float((fk * fk).sum())
    return dict(f=lin["res"][adm], J=lin["jpt"][adm], cost=cost, n=len(adm),
                ok=lin["rc"] == 0 and bool(np.isfinite(lin["cost"])))


def _sums(lin, dtype):
    J, f = lin["J"].astype(dtype).reshape(-1, 3), lin["f"].astype(dtype).reshape(-1)
    H = np.zeros((3, 3), dtype)
    g = np.zeros(3, dtype)
    for r in range(J.shape[0]):  # one fixed order: the observations in the caller's order
        H += np.outer(J[r], J[r])
        g += J[r] * f[r]
    return H, g


def _scale(H, opts, dtype):
    one = dtype(1)
    return one / (one + np.sqrt(np.diag(H))) if opts.jacobi_scaling else np.ones(3, dtype)


def step(lin, opts=None, radius: float = 0.0):
    """The longdouble step: dict(delta (3,) f64, delta_ld, mcc, cond, A, b, scale, d2)."""
    opts = opts or oracle.default_options()
    radius = radius if radius > 0 else opts.initial_trust_region_radius
    H, g = _sums(lin, LD)
    s = _scale(H, opts, LD)
    A, b = _system(H, g, s, opts, radius, LD)
    A64 = A.astype(np.float64)
    C = np.linalg.cholesky((A64 + A64.T) / 2)

    def solve(v):
        return np.linalg.solve(C.T, np.linalg.solve(C, v.astype(np.float64))).astype(LD)

    y = solve(b)
    for _ in range(3):
        y = y + solve(b - A @ y)
    delta = -s * y
    return dict(delta=delta.astype(np.float64), delta_ld=delta, mcc=float(_mcc(lin, delta, LD)),
                cond=float(np.linalg.cond(A64)), A=A, b=b, scale=s, d2=np.diag(A) - np.diag(H) * s * s)


def step64(lin, opts=None, radius: float = 0.0):
    """The f64 restatement's step (3,), no refinement."""
    opts = opts or oracle.default_options()
    radius = radius if radius > 0 else opts.initial_trust_region_radius
    H, g = _sums(lin, np.float64)
    s = _scale(H, opts, np.float64)
    A, b = _system(H, g, s, opts, radius, np.float64)
    y, ok = _chol_solve(A, b, np.float64)
    assert ok
    return -s * y


def f64_ratio(lin, opts=None, radius: float = 0.0) -> float:
    ref = step(lin, opts, radius)
    err = np.abs(step64(lin, opts, radius).astype(LD) - ref["delta_ld"]).max()
    return float(err / (ref["cond"] * EPS64 * np.abs(ref["delta_ld"]).max()))


def step_bound(ref) -> float:
    """STEP_F cond eps |step|_inf of a ``step`` result."""
    return STEP_F * ref["cond"] * EPS64 * float(np.abs(ref["delta"]).max())


def _gmax(x, g):
    g = np.asarray(g, dtype=np.float64)
    return float(np.abs(x - (x + -g)).max())


def lm(prob: ProblemArrays, p: int, opts=None, dtype=np.float64):
    """The LM loop of track p. Returns dict(accept [the log's accepted column, rows 1 ..], termination, msg, rows
    (iterations + 1, 8) f64, X (3,), iterations, n_succ, n_unsucc, initial_cost, final_cost, margin) as refloc.lm."""
    opts = opts or oracle.default_options()
    T = dtype
    x = np.array(prob.points[p], dtype=np.float64)
    rows, accept, margins = [], [], []

    def rel(v, thr):
        if thr > 0:
            margins.append(abs(float(v) - float(thr)) / float(thr))

    def out(term, msg):
        return dict(accept=accept, termination=term, msg=msg, rows=np.array(rows, dtype=np.float64), X=x,
                    iterations=it, n_succ=n_succ, n_unsucc=n_unsucc, initial_cost=float(initial), final_cost=float(final),
                    margin=min(margins) if margins else float("inf"))

    it, n_succ, n_unsucc, n_invalid, step_ok = 0, 1, 0, 0, True
    lin = linearize(prob, p, opts, x)
    if not (lin["ok"] and np.all(np.isfinite(x))):
        initial = final = float("nan")
        return out(2, MSG_EVAL_FAIL)
    H, g = _sums(lin, T)
    scale = _scale(H, opts, T)
    x_cost = T(lin["cost"])
    initial = final = x_cost
    gmax = _gmax(x, g)
    radius, decrease = T(opts.initial_trust_region_radius), T(2)
    xnorm = np.sqrt((x.astype(T) ** 2).sum())
    rows.append([x_cost, 0, gmax, 0, 0, radius, 1, 0])
    while True:
        if it >= opts.max_num_iterations:
            return out(1, MSG_MAX_ITER)
        if step_ok:
            rel(gmax, opts.gradient_tolerance)
            if gmax <= opts.gradient_tolerance:
                return out(0, MSG_GRAD_TOL)
        if radius <= opts.min_trust_region_radius:
            return out(0, MSG_MIN_RADIUS)
        it += 1
        A, b = _system(H, g, scale, opts, radius, T)
        y, ok = _chol_solve(A, b, T)
        mcc = T(0)
        if ok:
            delta = -scale * y
            mcc = _mcc(lin, delta, T)
            ok = bool(np.isfinite(mcc)) and mcc > 0
        if not ok:
            n_invalid += 1
            n_unsucc += 1
            if n_invalid >= opts.max_num_consecutive_invalid_steps:
                rows.append([x_cost, 0, gmax, 0, 0, radius, 0, 0])
                accept.append(0)
                return out(2, MSG_INVALID)
            radius, decrease, step_ok = radius / decrease, decrease * 2, False
            rows.append([x_cost, 0, gmax, 0, 0, radius, 0, 0])
            accept.append(0)
            continue
        n_invalid = 0
        xc = x + delta.astype(np.float64)
        lc = linearize(prob, p, opts, xc)
        cand = T(lc["cost"]) if lc["ok"] else T(np.finfo(np.float64).max)
        step_norm = np.sqrt(((x.astype(T) - xc.astype(T)) ** 2).sum())
        cost_change = x_cost - cand
        ptol = T(opts.parameter_tolerance)
        rel(step_norm, ptol * (xnorm + ptol))
        if step_norm <= ptol * (xnorm + ptol):
            rows.append([cand, cost_change, gmax, step_norm, 0, radius, -1, 0])
            accept.append(-1)
            return out(0, MSG_PARAM_TOL)
        rel(abs(cost_change), T(opts.function_tolerance) * x_cost)
        if abs(cost_change) <= T(opts.function_tolerance) * x_cost:
            rows.append([cand, cost_change, gmax, step_norm, 0, radius, -1, 0])
            accept.append(-1)
            return out(0, MSG_FUNC_TOL)
        rho = cost_change / mcc if lc["ok"] else -T(np.finfo(np.float64).max)
        margins.append(abs(float(rho) - opts.min_relative_decrease))
        if rho > opts.min_relative_decrease:
            x, lin = xc, lc
            H, g = _sums(lin, T)
            x_cost = cand
            gmax = _gmax(x, g)
            xnorm = np.sqrt((x.astype(T) ** 2).sum())
            t = 2 * rho - 1
            radius = min(radius / max(T(1) / T(3), 1 - t * t * t), T(opts.max_trust_region_radius))
            decrease, step_ok = T(2), True
            n_succ += 1
            final = min(final, x_cost)
            rows.append([x_cost, cost_change, gmax, step_norm, rho, radius, 1, 0])
            accept.append(1)
        else:
            radius, decrease, step_ok = radius / decrease, decrease * 2, False
            n_unsucc += 1
            final = min(final, cand)
            rows.append([cand, cost_change, gmax, step_norm, rho, radius, 0, 0])
            accept.append(0)


# ---------------------------------------------------------------------------------------------------- the tracks
def tracks_problem(counts, seed: int = 0, n_cams: int = 0, pixel_noise: float = 0.5, depth_noise: float = 0.01,
                   point_noise: float = 0.03, ray_noise: float = 0.0, bad_frac: float = 0.1,
                   shuffle: bool = True) -> ProblemArrays:
    """A window whose point p has exactly ``counts[p]`` admissible observations, each from a different camera of
    ``n_cams`` (default: max(counts)) cameras spread around the origin and looking down +z at a cloud 2.5 .. 5 in
    front of them. About ``bad_frac`` more observations per point (at least one) are inadmissible (depth 0 or -inf).
    The observation order is shuffled. The positions are the true ones perturbed by ``point_noise`` in every
    coordinate and, on top, by ``ray_noise`` x N(0, 1) x the point's depth along the ray from the origin;
    ``meta['truth']`` keeps the true positions."""
    from miba.synthetic import ROS_DEFAULT_INTRINSICS, quat_from_rotmat

    rng = np.random.default_rng(seed)
    K = ROS_DEFAULT_INTRINSICS.copy()
    npt = len(counts)
    nc = int(n_cams) if n_cams else (int(max(counts)) if npt else 0)
    X = np.stack([rng.uniform(-1.0, 1.0, npt), rng.uniform(-0.8, 0.8, npt), rng.uniform(2.5, 5.0, npt)], 1)
    R = np.stack([_rodrigues(rng.normal(0, 0.04, 3)) for _ in range(nc)]) if nc else np.zeros((0, 3, 3))
    t = rng.normal(0, 0.25, (nc, 3)) * np.array([1.0, 1.0, 0.3])
    obs_cam, obs_pt, uv, depth = [], [], [], []
    for p, n in enumerate(counts):
        n = int(n)
        n_bad = max(1, int(round(bad_frac * n)))
        cams = np.concatenate([rng.choice(nc, n, replace=False), rng.choice(nc, n_bad)]).astype(np.int64)
        pc = np.einsum("nji,nj->ni", R[cams], X[p] - t[cams])  # R^T (X - t)
        z = pc[:, 2]
        px = np.stack([K[0] * pc[:, 0] / z + K[2], K[1] * pc[:, 1] / z + K[3]], 1) + rng.normal(0, pixel_noise, (len(cams), 2))
        d = z * (1.0 + rng.normal(0, depth_noise, len(cams)))
        d[n:] = np.where(rng.random(n_bad) < 0.5, 0.0, -np.inf)
        obs_cam.append(cams)
        obs_pt.append(np.full(len(cams), p))
        uv.append(px)
        depth.append(d)
    cat = (lambda a, w: np.concatenate(a) if a else np.zeros((0,) + w))
    obs_cam, obs_pt, uv, depth = cat(obs_cam, ()), cat(obs_pt, ()), cat(uv, (2,)), cat(depth, ())
    if shuffle:
        perm = rng.permutation(len(obs_cam))
        obs_cam, obs_pt, uv, depth = obs_cam[perm], obs_pt[perm], uv[perm], depth[perm]
    X0 = X + rng.normal(0, point_noise, (npt, 3)) + X * (ray_noise * rng.normal(0, 1, (npt, 1)))
    cams = np.concatenate([quat_from_rotmat(R), t], 1) if nc else np.zeros((0, 7))
    return ProblemArrays(cams, X0, K, K.copy(), obs_cam.astype(np.int32), obs_pt.astype(np.int32), uv, depth, fixed_cam=-1,
                         meta=dict(truth=X, seed=seed))


# ------------------------------------------------------------------------------------------- the GPU tests' cases
L = LANES
STEP_COUNTS = (1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 4 * L + 1)
STEP_RADII = (1e4, 1e-2, 1e12)
# The loop tracks, 10 observations each (the map's mean track length). LOOP_EASY: all 16 points take only accepted
# steps (10 .. 41 iterations, ending on the function tolerance; smallest margin 1.4e-2). LOOP_HARD: the points start
# off by N(0, 1) x their depth along the viewing ray; searched over ray_noise 0.3, 0.5, 1.0 x seeds 3, 4 for tracks
# whose f64 and longdouble sequences agree, contain a rejected step and keep every margin >= MARGIN_MIN: none at 0.3,
# two at 0.5 / seed 4, two at 1.0 / seed 3, three at 1.0 / seed 4, which is taken: track 3 rejects three times in the
# middle, 4 four times from its second step, 14 twice (margins 8.8e-3, 2.0e-2, 5.4e-3).
LOOP_EASY = dict(counts=(10,) * 16, seed=3)
LOOP_EASY_TRACKS = tuple(range(16))
LOOP_HARD = dict(counts=(10,) * 16, seed=4, ray_noise=1.0)
LOOP_HARD_TRACKS = (3, 4, 14)
# noise-free tracks that start 1e-5 off the truth: two iterations, ending on the parameter tolerance
LOOP_QUICK = dict(counts=(10,) * 4, seed=5, pixel_noise=0.0, depth_noise=0.0, point_noise=1e-5)
# Huber parameters that put reprojection and depth blocks on both sides of the threshold on the chosen step track
HUBER_MIXED = dict(hub_p_repr=0.4, hub_p_unpr=0.012)
HUBER_TRACK = 8  # 65 observations: 52 / 13 reprojection and 45 / 20 depth blocks in the quadratic / linear zone


def step_tracks():
    return cached("pts_step_tracks", lambda: tracks_problem(STEP_COUNTS, seed=11))


def loop_problem(hard):
    """The loop tracks: False = LOOP_EASY, True = LOOP_HARD, "quick" = LOOP_QUICK (cached, read-only)."""
    kw = LOOP_QUICK if hard == "quick" else (LOOP_HARD if hard else LOOP_EASY)
    return cached(("pts_loop", hard), lambda: tracks_problem(**kw))


def merge(a: ProblemArrays, b: ProblemArrays) -> ProblemArrays:
    """a's points, then b's, each on its own cameras (the intrinsics are a's; the generators share them)."""
    return ProblemArrays(np.concatenate([a.cams, b.cams]), np.concatenate([a.points, b.points]), a.intr.copy(),
                         a.intr_prior.copy(), np.concatenate([a.obs_cam, b.obs_cam + a.n_cams]),
                         np.concatenate([a.obs_pt, b.obs_pt + a.n_points]), np.concatenate([a.obs_uv, b.obs_uv]),
                         np.concatenate([a.obs_depth, b.obs_depth]), fixed_cam=-1)


def tile(p: ProblemArrays, times: int) -> ProblemArrays:
    """The window repeated: point q + k n_points is point q again, seen by the same cameras."""
    n = p.n_points
    return ProblemArrays(p.cams.copy(), np.tile(p.points, (times, 1)), p.intr.copy(), p.intr_prior.copy(),
                         np.tile(p.obs_cam, times), np.concatenate([p.obs_pt + k * n for k in range(times)]),
                         np.tile(p.obs_uv, (times, 1)), np.tile(p.obs_depth, times), fixed_cam=-1)


def loop_refs(hard: bool, p: int, **okw):
    """(f64 loop, longdouble loop) of track p, cached."""
    def make():
        o = oracle.default_options(**okw)
        q = loop_problem(hard)
        return lm(q, p, o, np.float64), lm(q, p, o, LD)
    return cached(("pts_refs", hard, p, tuple(sorted(okw.items()))), make)


def huber_zones(prob: ProblemArrays, p: int, opts):
    """Blocks of track p in (reprojection quadratic, reprojection linear, depth quadratic, depth linear) zones."""
    lo = linearize(prob, p, opts)
    plain = linearize(prob, p, oracle.default_options(hub_p_repr=1e30, hub_p_unpr=1e30, weight_unpr=opts.weight_unpr))
    sr = (plain["f"][:, :2] ** 2).sum(1)
    sd = plain["f"][:, 2] ** 2
    br, bd = opts.hub_p_repr ** 2, opts.hub_p_unpr ** 2
    assert lo["n"] == plain["n"]
    return int((sr <= br).sum()), int((sr > br).sum()), int((sd <= bd).sum()), int((sd > bd).sum())
