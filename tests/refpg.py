"""References of ba_pose_graph (test infrastructure): Levenberg-Marquardt over the poses of a pose graph.

A *graph* is a dict: ``cams`` (n, 7), ``ea`` / ``eb`` (m,), ``meas`` (m, 7), ``weights`` (m, 2) or None, ``constant``
(n,) bool, ``huber`` (0: trivial loss), plus ``truth`` (n, 7) where the generator knows it.

* ``linearize(g, cams, dtype)``  residuals f (m, 6), Jacobians Ja, Jb (m, 6, 6) (robustified by the Huber corrector),
  per-edge cost, in ``dtype``: the cost of include/ba.h's ba_pose_graph. For edge (a, b): t^ = R_a^T (t_b - t_a),
  q^ = conj(q_a) q_b, dq = q_meas conj(q^) on the hemisphere dq.w >= 0, r = [w_t (t^ - t_meas); w_r 2 vec(dq)]; with
  M = dq.w I + [dq.v]x the derivatives with respect to the right perturbations are
  J_a = [-w_t I, w_t [t^]x; 0, w_r M], J_b = [w_t R^, 0; 0, -w_r M R^], R^ = R_a^T R_b.
* ``step(g, opts, radius)``  the first LM step in ``np.longdouble``: H, g over the active poses (index order), Jacobi
  scaling, clamped LM diagonal, f64 Cholesky with three refinement passes whose residuals are extended precision,
  delta = -s y; cond_2 of the system over the poses that have an edge (an isolated active pose contributes a decoupled
  diagonal block whose step is exactly zero; the GPU test checks that pose bitwise instead).
* ``step64``  the same in plain f64 without refinement; ``f64_ratio`` = |step64 - step|_inf / (cond eps |step|_inf).
* ``lm(g, opts, dtype)``  the whole loop, restated from refloc.lm for 6 n_active unknowns, with the margin of every
  decision.
* seeded graph generators and the lists of cases the GPU tests use.
"""
from __future__ import annotations

import numpy as np

from miba import posegraph
from oracle import oracle
from refstep import EPS64, LD

MSG_NONE, MSG_MAX_ITER, MSG_GRAD_TOL, MSG_MIN_RADIUS, MSG_PARAM_TOL, MSG_FUNC_TOL, MSG_INVALID, MSG_EVAL_FAIL = range(8)

# The largest f64 ratio over every first-step graph (STEP_CASES x STEP_RADII and the Huber / weighted case), as
# test_refpg.py::test_f64_ratio measured it on x86-64: 5.44, on the loop of 22 poses at radius 1e-2 (it asserts that
# the stored value covers what it measures and is not stale by more than a factor two). The systems are well
# conditioned there (cond 2.2), so this is the rounding of the sums rather than cond * eps.
F64_RATIO = 5.5
# the step bound's factor: max(8, 4 x the f64 ratio); the 4 for the device's own Jacobians and its tree-ordered sums
# (DESIGN 4.13's rule)
STEP_F = max(8.0, 4.0 * F64_RATIO)


# ------------------------------------------------------------------------------------------------ the cost
def _quat_R(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), dtype=q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _skew(v):
    S = np.zeros((len(v), 3, 3), dtype=v.dtype)
    S[:, 0, 1], S[:, 0, 2] = -v[:, 2], v[:, 1]
    S[:, 1, 0], S[:, 1, 2] = v[:, 2], -v[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -v[:, 1], v[:, 0]
    return S


def weights_of(g):
    m = len(g["ea"])
    return np.ones((m, 2)) if g.get("weights") is None else np.asarray(g["weights"], dtype=np.float64).reshape(m, 2)


def residual(g, cams=None, dtype=LD, flipped=False):
    """Plain residuals r (m, 6) with the parts the Jacobians need: (r, t^, dq, R^). ``flipped``: also return the
    mask of edges whose dq was negated."""
    T = dtype
    x = np.asarray(g["cams"] if cams is None else cams, dtype=np.float64).astype(T)
    ea, eb = np.asarray(g["ea"]), np.asarray(g["eb"])
    z = np.asarray(g["meas"], dtype=np.float64).astype(T).reshape(-1, 7)
    w = weights_of(g).astype(T)
    xa, xb = x[ea], x[eb]
    Ra, Rb = _quat_R(xa[:, :4]), _quat_R(xb[:, :4])
    th = np.einsum("mki,mk->mi", Ra, xb[:, 4:] - xa[:, 4:])
    Rh = np.einsum("mki,mkj->mij", Ra, Rb)
    qh = posegraph.quat_mul(posegraph.quat_conj(xa[:, :4]), xb[:, :4])
    dq = posegraph.quat_mul(z[:, :4], posegraph.quat_conj(qh))
    neg = dq[:, 3] < 0
    dq = np.where(neg[:, None], -dq, dq)
    r = np.concatenate([w[:, :1] * (th - z[:, 4:]), w[:, 1:] * (2 * dq[:, :3])], axis=1)
    return (r, th, dq, Rh, neg) if flipped else (r, th, dq, Rh)


def linearize(g, cams=None, dtype=LD):
    """dict(f (m, 6), Ja, Jb (m, 6, 6), cost (m,), total, ok) in ``dtype``."""
    T = dtype
    r, th, dq, Rh = residual(g, cams, T)
    m = len(r)
    w = weights_of(g).astype(T)
    s = (r * r).sum(1)
    a = T(g.get("huber", 0.0) or 0.0)
    rho, sq = s.copy(), np.ones(m, dtype=T)
    if a > 0:
        lin = s > a * a
        rt = np.sqrt(np.where(lin, s, T(1)))
        rho = np.where(lin, 2 * a * rt - a * a, s)
        sq = np.where(lin, np.sqrt(a / rt), T(1))
    M = dq[:, 3, None, None] * np.eye(3, dtype=T)[None] + _skew(dq[:, :3])
    At, Ar = (sq * w[:, 0])[:, None, None], (sq * w[:, 1])[:, None, None]
    Ja = np.zeros((m, 6, 6), dtype=T)
    Jb = np.zeros((m, 6, 6), dtype=T)
    Ja[:, :3, :3] = -At * np.eye(3, dtype=T)[None]
    Ja[:, :3, 3:] = At * _skew(th)
    Ja[:, 3:, 3:] = Ar * M
    Jb[:, :3, :3] = At * Rh
    Jb[:, 3:, 3:] = -Ar * np.einsum("mik,mkj->mij", M, Rh)
    cost = rho / 2
    total = cost.sum() if m else T(0)
    return dict(f=sq[:, None] * r, Ja=Ja, Jb=Jb, cost=cost, total=total, ok=bool(np.all(np.isfinite(cost))))


def active(g):
    return np.nonzero(~np.asarray(g["constant"], dtype=bool))[0]


def _pos(g):
    act = active(g)
    pos = -np.ones(len(g["cams"]), dtype=np.int64)
    pos[act] = np.arange(len(act))
    return act, pos


def sums(g, lin, dtype):
    """H (6 na, 6 na) and g (6 na,) over the active poses in index order, the edges added in the caller's order."""
    act, pos = _pos(g)
    n = 6 * len(act)
    H, gr = np.zeros((n, n), dtype), np.zeros(n, dtype)
    Ja, Jb, f = lin["Ja"].astype(dtype), lin["Jb"].astype(dtype), lin["f"].astype(dtype)
    for k, (a, b) in enumerate(zip(g["ea"], g["eb"])):
        pa, pb = pos[a], pos[b]
        if pa >= 0:
            sa = slice(6 * pa, 6 * pa + 6)
            H[sa, sa] += Ja[k].T @ Ja[k]
            gr[sa] += Ja[k].T @ f[k]
        if pb >= 0:
            sb = slice(6 * pb, 6 * pb + 6)
            H[sb, sb] += Jb[k].T @ Jb[k]
            gr[sb] += Jb[k].T @ f[k]
        if pa >= 0 and pb >= 0:
            blk = Ja[k].T @ Jb[k]
            H[sa, sb] += blk
            H[sb, sa] += blk.T
    return H, gr


def _scale(H, opts, dtype):
    one = dtype(1)
    return one / (one + np.sqrt(np.diag(H))) if opts.jacobi_scaling else np.ones(len(H), dtype)


def _system(H, gr, scale, opts, radius, dtype):
    d2 = np.clip(np.diag(H) * scale * scale, dtype(opts.min_lm_diagonal), dtype(opts.max_lm_diagonal)) / dtype(radius)
    return H * scale[:, None] * scale[None, :] + np.diag(d2), scale * gr


def _solve(A, b, dtype):
    """(y, ok) of A y = b: f64 Cholesky; in longdouble three refinement passes with extended-precision residuals."""
    A64 = np.asarray(A, dtype=np.float64)
    if len(b) == 0:
        return np.zeros(0, dtype), True
    try:
        C = np.linalg.cholesky((A64 + A64.T) / 2)
    except np.linalg.LinAlgError:
        return None, False

    def sol(v):
        return np.linalg.solve(C.T, np.linalg.solve(C, np.asarray(v, dtype=np.float64)))

    y = sol(b).astype(dtype)
    if dtype is not np.float64:
        for _ in range(3):
            y = y + sol(b - A @ y).astype(dtype)
    return y, bool(np.all(np.isfinite(y)))


def _mcc(g, lin, delta, dtype):
    act, pos = _pos(g)
    d = np.concatenate([np.asarray(delta, dtype=dtype).reshape(-1, 6), np.zeros((1, 6), dtype)])  # [-1]: constant
    da, db = d[pos[np.asarray(g["ea"])]], d[pos[np.asarray(g["eb"])]]
    jd = np.einsum("mrd,md->mr", lin["Ja"].astype(dtype), da) + np.einsum("mrd,md->mr", lin["Jb"].astype(dtype), db)
    return -(jd * (lin["f"].astype(dtype) + jd / 2)).sum()


def _with_edge(g):
    """Mask over the active poses (index order): the pose has an edge."""
    act, pos = _pos(g)
    has = np.zeros(len(act), dtype=bool)
    for c in np.concatenate([np.asarray(g["ea"]), np.asarray(g["eb"])]).astype(np.int64):
        if pos[c] >= 0:
            has[pos[c]] = True
    return has


def step(g, opts=None, radius: float = 0.0):
    """The longdouble step: dict(delta (na, 6) f64, delta_ld, mcc, cond, A, b, scale, cost)."""
    opts = opts or oracle.default_options()
    radius = radius if radius > 0 else opts.initial_trust_region_radius
    lin = linearize(g, None, LD)
    H, gr = sums(g, lin, LD)
    s = _scale(H, opts, LD)
    A, b = _system(H, gr, s, opts, radius, LD)
    y, ok = _solve(A, b, LD)
    assert ok
    delta = -s * y
    dof = np.repeat(_with_edge(g), 6)
    A64 = A.astype(np.float64)[np.ix_(dof, dof)]
    cond = float(np.linalg.cond(A64)) if dof.any() else 1.0
    return dict(delta=delta.astype(np.float64).reshape(-1, 6), delta_ld=delta.reshape(-1, 6), mcc=float(_mcc(g, lin, delta, LD)),
                cond=cond, A=A, b=b, scale=s, cost=float(lin["total"]))


def step64(g, opts=None, radius: float = 0.0):
    """The plain f64 restatement's step (na, 6): no refinement."""
    opts = opts or oracle.default_options()
    radius = radius if radius > 0 else opts.initial_trust_region_radius
    lin = linearize(g, None, np.float64)
    H, gr = sums(g, lin, np.float64)
    s = _scale(H, opts, np.float64)
    A, b = _system(H, gr, s, opts, radius, np.float64)
    y, ok = _solve(A, b, np.float64)
    assert ok
    return (-s * y).reshape(-1, 6)


def f64_ratio(g, opts=None, radius: float = 0.0) -> float:
    ref = step(g, opts, radius)
    err = np.abs(step64(g, opts, radius).astype(LD) - ref["delta_ld"]).max()
    return float(err / (ref["cond"] * EPS64 * np.abs(ref["delta_ld"]).max()))


def step_bound(ref) -> float:
    """STEP_F cond eps |step|_inf of a ``step`` result."""
    return STEP_F * ref["cond"] * EPS64 * float(np.abs(ref["delta"]).max())


def _gmax(x, act, gr):
    gm = 0.0
    for k, c in enumerate(act):
        tp = oracle.se3_plus(x[c], -np.asarray(gr[6 * k:6 * k + 6], dtype=np.float64))
        gm = max(gm, float(np.abs(x[c] - tp).max()))
    return gm


def lm(g, opts=None, dtype=np.float64):
    """The LM loop. Returns dict(accept, termination, msg, rows, cams, iterations, n_succ, n_unsucc, initial_cost,
    final_cost, margin) as refloc.lm does."""
    opts = opts or oracle.default_options()
    T = dtype
    x = np.array(g["cams"], dtype=np.float64).reshape(-1, 7)
    act, _ = _pos(g)
    rows, accept, margins = [], [], []

    def rel(v, thr):
        if thr > 0:
            margins.append(abs(float(v) - float(thr)) / float(thr))

    def out(term, msg):
        return dict(accept=accept, termination=term, msg=msg, rows=np.array(rows, dtype=np.float64), cams=x,
                    iterations=it, n_succ=n_succ, n_unsucc=n_unsucc, initial_cost=float(initial), final_cost=float(final),
                    margin=min(margins) if margins else float("inf"))

    it, n_succ, n_unsucc, n_invalid, step_ok = 0, 1, 0, 0, True
    lin = linearize(g, x, T)
    if not lin["ok"]:
        initial = final = float("nan")
        return out(2, MSG_EVAL_FAIL)
    H, gr = sums(g, lin, T)
    scale = _scale(H, opts, T)
    x_cost = T(lin["total"])
    initial = final = x_cost
    gmax = _gmax(x, act, gr)
    radius, decrease = T(opts.initial_trust_region_radius), T(2)
    xnorm = np.sqrt((x[act].astype(T) ** 2).sum())
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
        A, b = _system(H, gr, scale, opts, radius, T)
        y, ok = _solve(A, b, T)
        mcc = T(0)
        if ok:
            delta = -scale * y
            mcc = _mcc(g, lin, delta, T)
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
        xc = x.copy()
        d64 = np.asarray(delta, dtype=np.float64).reshape(-1, 6)
        for k, c in enumerate(act):
            if np.any(d64[k] != 0):
                xc[c] = oracle.se3_plus(x[c], d64[k])
        lc = linearize(g, xc, T)
        cand = T(lc["total"]) if lc["ok"] else T(np.finfo(np.float64).max)
        step_norm = np.sqrt(((x[act].astype(T) - xc[act].astype(T)) ** 2).sum())
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
            H, gr = sums(g, lin, T)
            x_cost = cand
            gmax = _gmax(x, act, gr)
            xnorm = np.sqrt((x[act].astype(T) ** 2).sum())
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


# ---------------------------------------------------------------------------------------------------- the graphs
def _rodrigues_quat(w):
    th = np.linalg.norm(w)
    if th < 1e-14:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def perturb(cams, rng, rot, trans):
    """Every pose times exp of a random rotation (sigma ``rot`` rad per axis), plus translation noise."""
    out = np.array(cams, dtype=np.float64)
    for c in range(len(out)):
        out[c, :4] = posegraph.quat_mul(out[c, :4], _rodrigues_quat(rng.normal(0, rot, 3)))
        out[c, :4] /= np.linalg.norm(out[c, :4])
        out[c, 4:] += rng.normal(0, trans, 3)
    return out


def trajectory(n, rng, step=0.3, turn=0.15):
    """A smooth random walk of n poses."""
    cams = np.zeros((n, 7))
    T = np.array([0, 0, 0, 1.0, 0, 0, 0])
    for c in range(n):
        cams[c] = T
        Z = np.concatenate([_rodrigues_quat(rng.normal(0, turn, 3)), [step, 0, 0] + rng.normal(0, 0.05, 3)])
        T = posegraph.compose(T, Z)
    return cams


TOPOLOGIES = ("chain", "loop", "star", "two", "dup", "const_mid", "const_edge", "isolated")


def pairs_of(topology, n):
    """(pairs (m, 2) in the caller's order, constant mask) of a topology on n ACTIVE poses (constant ones are added:
    the returned mask has n + its count of constant poses entries)."""
    chain = [(i, i + 1) for i in range(n - 1)]
    if topology == "chain":  # pose n constant, at the end of the chain
        return chain + [(n - 1, n)], _mask(n + 1, [n])
    if topology == "loop":  # the loop edge from the last pose to the first: a wide band as given
        return chain + [(n - 1, n), (n - 1, 0)], _mask(n + 1, [n])
    if topology == "star":  # every pose hangs on the constant centre, given last, and on nothing else
        return [(n, i) if i % 2 else (i, n) for i in range(n)], _mask(n + 1, [n])
    if topology == "two":  # two components, each with a constant pose of its own
        h = (n + 1) // 2
        p = [(i, i + 1) for i in range(h - 1)] + [(h - 1, n)] + [(i, i + 1) for i in range(h, n - 1)]
        p += [(n - 1, n + 1)] if n > h else []
        return p, _mask(n + 2, [n, n + 1])
    if topology == "dup":  # duplicate and reversed edges of the same pairs
        p = chain + [(n - 1, n)]
        return p + [(b, a) for a, b in p[::2]] + p[:1], _mask(n + 1, [n])
    if topology == "const_mid":  # a constant pose in the middle of the index range
        k = n // 2
        idx = [i for i in range(n + 1)]
        return [(idx[i], idx[i + 1]) for i in range(n)], _mask(n + 1, [k])
    if topology == "const_edge":  # an edge between two constant poses: it counts in the cost only
        return chain + [(n - 1, n), (n, n + 1)], _mask(n + 2, [n, n + 1])
    if topology == "isolated":  # pose n - 1 has no edge at all (n >= 2), or the only active pose has none (n = 1)
        if n == 1:
            return [(1, 2)], _mask(3, [1, 2])
        return [(i, i + 1) for i in range(n - 2)] + [(n - 2, n)], _mask(n + 1, [n])
    raise ValueError(topology)


def _mask(n, const):
    m = np.zeros(n, dtype=bool)
    m[list(const)] = True
    return m


def make_graph(topology, n_active, seed=0, rot=0.05, trans=0.05, meas_rot=0.01, meas_trans=0.01, huber=0.0,
               weighted=False, flip_meas=False):
    """A seeded graph: a random-walk truth, measurements from the truth with noise, estimates = the truth perturbed.
    ``flip_meas``: every other measurement's quaternion negated (the same rotation; dq.w < 0 before the flip)."""
    rng = np.random.default_rng(1000 * seed + 17 * n_active + TOPOLOGIES.index(topology))
    pairs, const = pairs_of(topology, n_active)
    n = len(const)
    truth = trajectory(n, rng)
    pairs = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    ea, eb, meas = posegraph.edges_from_poses(truth, pairs)
    meas = perturb(meas, rng, meas_rot, meas_trans) if len(meas) else meas
    if flip_meas:
        meas[::2, :4] *= -1
    cams = perturb(truth, rng, rot, trans)
    weights = np.stack([rng.uniform(0.5, 3.0, len(ea)), rng.uniform(0.5, 3.0, len(ea))], 1) if weighted else None
    return dict(cams=cams, ea=ea, eb=eb, meas=meas, weights=weights, constant=const, huber=huber, truth=truth,
                topology=topology, n_active=n_active)


def loop_closure_graph(n=200, seed=5, drift_rot=0.004, drift_trans=0.01, n_loops=8):
    """Two sweeps of one circuit: n poses, the second sweep revisits the first. Estimates carry a random-walk drift
    (odometry edges are measured on the drifted estimates, so they are consistent with them); a handful of loop edges
    between the sweeps are measured on the truth. Pose 0 is constant."""
    rng = np.random.default_rng(seed)
    h = n // 2
    ang = 2 * np.pi * np.arange(n) / h
    truth = np.zeros((n, 7))
    for c in range(n):
        truth[c, :4] = _rodrigues_quat(np.array([0, 0, ang[c] + np.pi / 2]))
        truth[c, 4:] = [5 * np.cos(ang[c]), 5 * np.sin(ang[c]), 0.1 * np.sin(3 * ang[c]) + (0.05 if c >= h else 0.0)]
    odo = np.array([(i, i + 1) for i in range(n - 1)])
    _, _, z_true = posegraph.edges_from_poses(truth, odo)
    z_odo = perturb(z_true, rng, drift_rot, drift_trans)
    est = np.zeros((n, 7))
    est[0] = truth[0]
    for c in range(n - 1):
        est[c + 1] = posegraph.compose(est[c], z_odo[c])
    loops = np.array([(int(k), int(k) + h) for k in np.linspace(0, h - 1, n_loops).astype(int)])
    _, _, z_loop = posegraph.edges_from_poses(truth, loops)
    pairs = np.concatenate([odo, loops])
    const = _mask(n, [0])
    return dict(cams=est, ea=pairs[:, 0].astype(np.int32), eb=pairs[:, 1].astype(np.int32),
                meas=np.concatenate([z_odo, z_loop]), weights=None, constant=const, huber=0.0, truth=truth,
                topology="loop_closure", n_active=n - 1)


def pose_rms(cams, truth, mask=None):
    """RMS over the poses of the translation error (m)."""
    d = np.asarray(cams)[:, 4:] - np.asarray(truth)[:, 4:]
    if mask is not None:
        d = d[mask]
    return float(np.sqrt((d * d).sum(1).mean()))


# ------------------------------------------------------------------------------------------- the GPU tests' cases
# n_active on the layout's edges: 1, 2 (12 < 16), 3 (18 > 16), 10 (60), 11 (66: the second 64-block), 22 (three blocks),
# 43 (258: the envelope's fourth block)
STEP_SIZES = (1, 2, 3, 10, 11, 22, 43)
STEP_RADII = (1e4, 1e-2, 1e12)
# (topology, n_active): every size on a chain, every topology at sizes that put it on one and on several blocks
STEP_CASES = tuple(("chain", n) for n in STEP_SIZES) + tuple(
    (t, n) for t in TOPOLOGIES[1:] for n in ((2, 11, 22) if t != "isolated" else (1, 2, 11, 22)))
# Huber parameter that puts edges in both zones of the weighted graph below (test_refpg.py asserts it)
HUBER_CASE = dict(topology="dup", n_active=22, seed=3, huber=0.25, weighted=True, rot=0.08, trans=0.15)

# whole-loop cases: (name, make_graph keywords, option overrides). test_refpg.py asserts for each that the f64 and
# longdouble loops take the same accept / reject sequence with no decision closer than MARGIN_MIN to its threshold,
# and that the set has a rejected step, a function-tolerance end and an iteration-limit end.
MARGIN_MIN = 1e-3
LOOP_CASES = (
    ("easy_dup", dict(topology="dup", n_active=11, seed=1), {}),
    ("loop22", dict(topology="loop", n_active=22, seed=2, rot=0.2, trans=0.3), {}),
    ("wild", dict(topology="loop", n_active=11, seed=4, rot=1.2, trans=2.0), {}),
    ("limit", dict(topology="dup", n_active=22, seed=2, rot=0.3, trans=0.5, huber=0.5), dict(max_num_iterations=3)),
    ("dup_weighted", dict(topology="dup", n_active=43, seed=6, rot=0.3, trans=0.3, weighted=True, flip_meas=True), {}),
)

_cache = {}


def cached(key, make):
    """Shared, read-only test data (callers must not modify it)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def step_graph(topology, n):
    return cached(("g", topology, n), lambda: make_graph(topology, n, seed=1, flip_meas=(n % 2 == 0)))


def huber_graph():
    return cached("huber", lambda: make_graph(**HUBER_CASE))


def step_ref(key, g, radius, **okw):
    return cached(("step", key, radius, tuple(sorted(okw.items()))), lambda: step(g, oracle.default_options(**okw), radius))


def loop_case(name):
    for nm, kw, okw in LOOP_CASES:
        if nm == name:
            return cached(("lg", name), lambda: make_graph(**kw)), okw
    raise KeyError(name)


def loop_refs(name):
    """(f64 loop, longdouble loop) of a loop case, cached."""
    def make():
        g, okw = loop_case(name)
        o = oracle.default_options(**okw)
        return lm(g, o, np.float64), lm(g, o, LD)
    return cached(("lr", name), make)


def closure():
    return cached("closure", loop_closure_graph)


def closure_ref():
    return cached("closure_ref", lambda: lm(closure(), oracle.default_options(), np.float64))


def huber_zones(g):
    """(edges in the quadratic zone, edges in the linear zone) at the given poses."""
    r, _, _, _ = residual(g, None, np.float64)
    s = (r * r).sum(1)
    b = g["huber"] ** 2
    return int((s <= b).sum()), int((s > b).sum())
