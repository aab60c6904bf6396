"""References of ba_localize (test infrastructure): pose-only Levenberg-Marquardt of one camera against constant
points and intrinsics.

A *frame* is one camera with its observations. Its residuals and pose Jacobians come from ``oracle.linearize`` on the
one-camera sub-problem (``fixed_cam = -1``, so the camera is active and N is the camera's own admissible count): exactly
the weighted, robustified residuals f (n, 3) and Jacobians J (n, 3, 6) of the cost ba_localize minimises. The oracle's
cost carries the IntrinsicsPrior block, which is constant here; its share is subtracted.

* ``step(lin, opts, radius)``  the first LM step in ``np.longdouble`` (as refstep.py): H = J^T J, g = J^T f, the Jacobi
  scaling s = 1 / (1 + sqrt(diag H)), D^2 = clip(diag(H) s^2, min_lm_diagonal, max_lm_diagonal) / radius, the damped
  scaled system (s H s + D^2) y = s g solved by f64 Cholesky with three refinement passes whose residuals are extended
  precision, delta = -s y; with the model cost change -(J delta)^T (f + J delta / 2) and cond_2 of the system.
* ``step64``  the same arithmetic in plain f64 with no refinement (what a straightforward restatement gives): the
  f64 ratio |step64 - step|_inf / (cond eps |step|_inf) measures what factor of cond * eps such a solve really costs.
* ``lm(prob, c, opts, dtype)``  the whole loop, restated from oracle/ba_oracle.c's solve_impl for the one pose, with the
  sums, the solve and the decisions in ``dtype`` (f64 or longdouble) and the pose updated by ``oracle.se3_plus``. It
  records the margin of every decision it took, so a test can tell a frame whose accept / reject sequence is settled
  from one where a rounding could flip it.
* ``frames_problem(counts, seed)``  a window whose camera c has exactly ``counts[c]`` admissible observations.
"""
from __future__ import annotations

import numpy as np

from miba.capi import ProblemArrays
from oracle import oracle
from refstep import EPS64, LD

# the LM loop's message kinds (csrc/ba_kernels.h LmMsg), stats[7] of ba_localize
MSG_NONE, MSG_MAX_ITER, MSG_GRAD_TOL, MSG_MIN_RADIUS, MSG_PARAM_TOL, MSG_FUNC_TOL, MSG_INVALID, MSG_EVAL_FAIL = range(8)

# The largest f64 ratio |step64 - step|_inf / (cond eps |step|_inf) over every frame of test_refloc.py's step cases
# (STEP_COUNTS x STEP_RADII on frames_problem, and the loop frames), as test_refloc.py::test_f64_ratio measured it on
# x86-64: 8.62, at 256 observations and radius 1e4 (it asserts that the stored value covers what it measures and is
# not stale by more than a factor two). From 63 observations on the systems are well conditioned (cond 100 .. 180 at
# radius 1e4, below 2 at 1e-2), so the error is the rounding of sums over n observations rather than cond * eps, and
# the ratio passes refstep.step_tol's bare factor 8 on the larger frames.
F64_RATIO = 8.7
# the step bound's factor: max(8, 4 x the f64 ratio); the 4 for the device's own Jacobians (16 eps per pixel by
# refcand's bound where the restatement uses the oracle's) and its tree-ordered sums
STEP_F = max(8.0, 4.0 * F64_RATIO)


def sub_problem(prob: ProblemArrays, c: int, pose=None) -> ProblemArrays:
    """Camera c's observations (admissible or not, in the caller's order) as a one-camera window."""
    k = np.nonzero(prob.obs_cam == c)[0]
    cam = np.array(prob.cams[c] if pose is None else pose, dtype=np.float64).reshape(1, 7)
    return ProblemArrays(cam, prob.points.copy(), prob.intr.copy(), prob.intr_prior.copy(),
                         np.zeros(len(k), dtype=np.int32), prob.obs_pt[k].copy(), prob.obs_uv[k].copy(),
                         prob.obs_depth[k].copy(), fixed_cam=-1)


def linearize(prob: ProblemArrays, c: int, opts=None, pose=None):
    """dict(f (n, 3), J (n, 3, 6), cost, n, ok) of frame c at ``pose`` (default: the problem's)."""
    opts = opts or oracle.default_options()
    sp = sub_problem(prob, c, pose)
    lin = oracle.linearize(sp, opts)
    adm = np.nonzero(sp.obs_depth > 1e-15)[0]
    fk = np.sqrt(opts.weight_intrinsics) * (sp.intr_prior - sp.intr)
    cost = lin["cost"] - 0.5 * float((fk * fk).sum())
    return dict(f=lin["res"][adm], J=lin["jcam"][adm], cost=cost, n=len(adm),
                ok=lin["rc"] == 0 and bool(np.isfinite(lin["cost"])))


def _sums(lin, dtype):
    J, f = lin["J"].astype(dtype).reshape(-1, 6), lin["f"].astype(dtype).reshape(-1)
    H = np.zeros((6, 6), dtype)
    g = np.zeros(6, dtype)
    for r in range(J.shape[0]):  # one fixed order: the observations in the caller's order
        H += np.outer(J[r], J[r])
        g += J[r] * f[r]
    return H, g


def _system(H, g, scale, opts, radius, dtype):
    cn = np.diag(H)
    d2 = np.clip(cn * scale * scale, dtype(opts.min_lm_diagonal), dtype(opts.max_lm_diagonal)) / dtype(radius)
    A = H * scale[:, None] * scale[None, :] + np.diag(d2)
    return A, scale * g


def _chol_solve(A, b, dtype):
    """(y, ok) of A y = b by Cholesky in ``dtype``; ok False at a non-positive or non-finite pivot."""
    n = len(b)
    L = np.zeros((n, n), dtype)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (d > 0 and np.isfinite(d)):
            return None, False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(n, dtype)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - (L[i + 1:, i] * y[i + 1:]).sum()) / L[i, i]
    return y, bool(np.all(np.isfinite(y)))


def _scale(H, opts, dtype):
    one = dtype(1)
    return one / (one + np.sqrt(np.diag(H))) if opts.jacobi_scaling else np.ones(6, dtype)


def _mcc(lin, delta, dtype):
    J, f = lin["J"].astype(dtype), lin["f"].astype(dtype)
    jd = np.einsum("ord,d->or", J, delta)
    return -(jd * (f + jd / 2)).sum()


def step(lin, opts=None, radius: float = 0.0):
    """The longdouble step: dict(delta (6,) f64, delta_ld, mcc, cond, A, b, scale, d2)."""
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
    """The f64 restatement's step (6,), no refinement."""
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
    tp = oracle.se3_plus(x, -np.asarray(g, dtype=np.float64))
    return float(np.abs(x - tp).max())


def lm(prob: ProblemArrays, c: int, opts=None, dtype=np.float64):
    """The LM loop of frame c. Returns dict(accept [the log's accepted column, rows 1 ..], termination, msg, rows
    (iterations + 1, 8) f64, pose (7,), iterations, n_succ, n_unsucc, initial_cost, final_cost, margin): margin is
    the smallest of |rho - min_relative_decrease| and the relative distances of every tolerance test the loop made
    from its threshold (inf if it made none)."""
    opts = opts or oracle.default_options()
    T = dtype
    x = np.array(prob.cams[c], dtype=np.float64)
    rows, accept, margins = [], [], []

    def rel(v, thr):
        if thr > 0:
            margins.append(abs(float(v) - float(thr)) / float(thr))

    def out(term, msg):
        return dict(accept=accept, termination=term, msg=msg, rows=np.array(rows, dtype=np.float64), pose=x,
                    iterations=it, n_succ=n_succ, n_unsucc=n_unsucc, initial_cost=float(initial), final_cost=float(final),
                    margin=min(margins) if margins else float("inf"))

    it, n_succ, n_unsucc, n_invalid, step_ok = 0, 1, 0, 0, True
    lin = linearize(prob, c, opts, x)
    if not lin["ok"]:
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
        xc = oracle.se3_plus(x, delta.astype(np.float64))
        lc = linearize(prob, c, opts, xc)
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


# ---------------------------------------------------------------------------------------------------- the frames
def _rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def frames_problem(counts, seed: int = 0, n_cloud: int = 400, pixel_noise: float = 0.5, depth_noise: float = 0.01,
                   rot_noise: float = 0.01, trans_noise: float = 0.01, bad_frac: float = 0.05, dup_frac: float = 0.05,
                   shuffle: bool = True) -> ProblemArrays:
    """A window whose camera c has exactly ``counts[c]`` admissible observations of a shared cloud of ``n_cloud``
    points (distinct points while counts[c] <= n_cloud; about ``dup_frac`` of them observed a second time by the same
    camera, inside the count). About ``bad_frac`` more observations per camera (at least one) are inadmissible (depth
    0 or -inf). The observation order is shuffled. The poses are the true ones perturbed by ``rot_noise`` /
    ``trans_noise``; ``meta['truth']`` keeps the true poses."""
    from miba.synthetic import ROS_DEFAULT_INTRINSICS, quat_from_rotmat

    rng = np.random.default_rng(seed)
    K = ROS_DEFAULT_INTRINSICS.copy()
    nc = len(counts)
    X = np.stack([rng.uniform(-1.0, 1.0, n_cloud), rng.uniform(-0.8, 0.8, n_cloud), rng.uniform(2.5, 5.0, n_cloud)], 1)
    R_true = np.stack([_rodrigues(rng.normal(0, 0.03, 3)) for _ in range(nc)]) if nc else np.zeros((0, 3, 3))
    t_true = rng.normal(0, 0.08, (nc, 3))
    obs_cam, obs_pt, uv, depth = [], [], [], []
    for c, n in enumerate(counts):
        n = int(n)
        n_dup = int(round(dup_frac * n)) if n >= 4 else 0
        base = rng.choice(n_cloud, n - n_dup, replace=(n - n_dup) > n_cloud)
        pts = np.concatenate([base, rng.choice(base, n_dup)]) if n_dup else base
        n_bad = max(1, int(round(bad_frac * n)))
        pts = np.concatenate([pts, rng.choice(n_cloud, n_bad)]).astype(np.int64)
        pc = (X[pts] - t_true[c]) @ R_true[c]  # R^T (X - t)
        z = pc[:, 2]
        px = np.stack([K[0] * pc[:, 0] / z + K[2], K[1] * pc[:, 1] / z + K[3]], 1) + rng.normal(0, pixel_noise, (len(pts), 2))
        d = z * (1.0 + rng.normal(0, depth_noise, len(pts)))
        d[n:] = np.where(rng.random(n_bad) < 0.5, 0.0, -np.inf)
        obs_cam.append(np.full(len(pts), c))
        obs_pt.append(pts)
        uv.append(px)
        depth.append(d)
    cat = (lambda a, w: np.concatenate(a) if a else np.zeros((0,) + w))
    obs_cam, obs_pt, uv, depth = cat(obs_cam, ()), cat(obs_pt, ()), cat(uv, (2,)), cat(depth, ())
    if shuffle:
        perm = rng.permutation(len(obs_cam))
        obs_cam, obs_pt, uv, depth = obs_cam[perm], obs_pt[perm], uv[perm], depth[perm]
    R0 = np.stack([R_true[c] @ _rodrigues(rng.normal(0, rot_noise, 3)) for c in range(nc)]) if nc else R_true
    t0 = t_true + rng.normal(0, trans_noise, (nc, 3))
    cams = np.concatenate([quat_from_rotmat(R0), t0], 1) if nc else np.zeros((0, 7))
    truth = np.concatenate([quat_from_rotmat(R_true), t_true], 1) if nc else np.zeros((0, 7))
    return ProblemArrays(cams, X, K, K.copy(), obs_cam.astype(np.int32), obs_pt.astype(np.int32), uv, depth, fixed_cam=-1,
                         meta=dict(truth=truth, seed=seed))


# ------------------------------------------------------------------------------------------- the GPU tests' cases
B = 256  # the kernel's workgroup size (csrc/ba_loc.h LOC_TPB)
STEP_COUNTS = (1, 2, 63, 64, 65, B - 1, B, B + 1, 4 * B + 1)
STEP_RADII = (1e4, 1e-2, 1e12)
LOOP_EASY = dict(n_cams=12, n_points=144, obs_per_point=4, seed=3)
LOOP_HARD = dict(n_cams=8, n_points=96, obs_per_point=4, seed=3, rot_noise=0.6, trans_noise=1.0)
# frames of LOOP_HARD used by the sequence test: f64 and longdouble take the same sequence and the smallest decision
# margin is >= MARGIN_MIN (test_refloc.py asserts both): 3 runs into max_num_iterations with rejections on the way,
# 6 opens with two rejections and ends on the function tolerance, 7 has rejections too and also reaches the limit.
# Measured margins: 5.0e-3, 6.9e-2, 1.3e-3. (Frame 4 takes no rejection in this restatement.)
LOOP_HARD_FRAMES = (3, 6, 7)
MARGIN_MIN = 1e-3
# Huber parameters that put reprojection and depth blocks on both sides of the threshold on the step frames
HUBER_MIXED = dict(hub_p_repr=0.035, hub_p_unpr=0.012)
HUBER_FRAME = 4  # 65 observations: 8 / 57 reprojection and 32 / 33 depth blocks in the quadratic / linear zone

_cache = {}


def cached(key, make):
    """Shared, read-only test data (callers must not modify it)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def step_frames():
    return cached("step_frames", lambda: frames_problem(STEP_COUNTS, seed=11, n_cloud=4 * B + 1))


def loop_problem(hard: bool):
    from miba import synthetic
    return cached(("loop", hard), lambda: synthetic.make_problem(**(LOOP_HARD if hard else LOOP_EASY)))


def loop_refs(hard: bool, c: int, **okw):
    """(f64 loop, longdouble loop) of frame c, cached."""
    def make():
        o = oracle.default_options(**okw)
        p = loop_problem(hard)
        return lm(p, c, o, np.float64), lm(p, c, o, LD)
    return cached(("refs", hard, c, tuple(sorted(okw.items()))), make)


def huber_zones(lin_prob: ProblemArrays, c: int, opts):
    """Blocks of frame c in (reprojection quadratic, reprojection linear, depth quadratic, depth linear) zones."""
    lo = linearize(lin_prob, c, opts)
    # sqrt(rho') < 1 exactly in the linear zone: compare the robustified residual with the plain one
    plain = linearize(lin_prob, c, oracle.default_options(hub_p_repr=1e30, hub_p_unpr=1e30,
                                                          weight_unpr=opts.weight_unpr))
    sr = (plain["f"][:, :2] ** 2).sum(1)
    sd = plain["f"][:, 2] ** 2
    br, bd = opts.hub_p_repr ** 2, opts.hub_p_unpr ** 2
    assert lo["n"] == plain["n"]
    return int((sr <= br).sum()), int((sr > br).sum()), int((sd <= bd).sum()), int((sd > bd).sum())
