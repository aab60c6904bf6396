"""The references of ba_refine_points (tests/refpts.py) checked on the CPU, and the conditions test_gpu_pts.py rests
on: the gradient and the step against finite differences of the cost, the longdouble step against an independent QR
solve, the f64 and longdouble loops on the tracks the GPU test uses, convergence of noise-free tracks to the true
position, the measured f64 ratio behind the step bound's factor, and the Huber case's four zones."""
import numpy as np
import pytest

import refloc
import refpts
from oracle import oracle
from refstep import EPS64, LD

STEP_CASES = [(p, r) for p in range(len(refpts.STEP_COUNTS)) for r in refpts.STEP_RADII]


def test_tracks_problem_counts():
    p = refpts.step_tracks()
    adm = p.obs_depth > 1e-15
    L = refpts.LANES
    assert refpts.STEP_COUNTS == (1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 4 * L + 1) == \
        (1, 2, 15, 16, 17, 31, 32, 33, 65)
    assert tuple(np.bincount(p.obs_pt[adm], minlength=p.n_points)) == refpts.STEP_COUNTS
    assert (~adm).sum() >= p.n_points  # inadmissible observations mixed in, for every point
    assert np.any(np.diff(p.obs_pt) < 0)  # shuffled
    pairs = np.stack([p.obs_cam[adm], p.obs_pt[adm]], 1)
    assert len(np.unique(pairs, axis=0)) == len(pairs)  # a point's admissible observations: distinct cameras


@pytest.mark.parametrize("p,radius", STEP_CASES)
def test_longdouble_step_matches_qr(p, radius):
    """[Jp s; D] y = -f by dense QR in f64, refined three times with the residual A^T (b - A y) in extended precision
    (R from the QR as the preconditioner): no normal equations are formed."""
    w, o = refpts.step_tracks(), oracle.default_options()
    lin = refpts.linearize(w, p, o)
    ref = refpts.step(lin, o, radius)
    A = np.concatenate([lin["J"].reshape(-1, 3).astype(LD) * ref["scale"], np.diag(np.sqrt(ref["d2"]))])
    b = np.concatenate([-lin["f"].reshape(-1).astype(LD), np.zeros(3, LD)])
    Q, R = np.linalg.qr(A.astype(np.float64))
    y = np.linalg.solve(R, Q.T @ b.astype(np.float64)).astype(LD)
    for _ in range(3):
        g = (A.T @ (b - A @ y)).astype(np.float64)
        y = y + np.linalg.solve(R, np.linalg.solve(R.T, g)).astype(LD)
    err = float(np.abs(ref["scale"] * y - ref["delta_ld"]).max())
    assert err <= 8 * ref["cond"] * EPS64 * np.abs(ref["delta"]).max()
    # the normal equations hold in extended precision
    r = ref["A"] @ (-(ref["delta_ld"] / ref["scale"])) - ref["b"]
    assert float(np.abs(r).max()) <= 64 * float(np.finfo(LD).eps) * ref["cond"] * float(np.abs(ref["b"]).max())


@pytest.mark.parametrize("p", [1, 4, 8])
def test_step_matches_finite_differences_of_the_cost(p):
    """The gradient Jp^T f the step is built from against central differences of the cost, and the step itself: the
    cost's slope along it is g . delta < 0, and at a huge radius (no damping) the step solves H delta = -g, so the
    finite-difference gradient vanishes to first order along it: H delta + g_fd = 0 within the differences' error."""
    w, o = refpts.step_tracks(), oracle.default_options(**refpts.HUBER_MIXED)
    lin = refpts.linearize(w, p, o)
    g = np.einsum("ord,or->d", lin["J"], lin["f"])
    H = np.einsum("ord,ore->de", lin["J"], lin["J"])
    h = 1e-6
    fd = np.zeros(3)
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        cp = refpts.linearize(w, p, o, w.points[p] + e)["cost"]
        cm = refpts.linearize(w, p, o, w.points[p] - e)["cost"]
        fd[d] = (cp - cm) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-5 * max(np.abs(g).max(), 1e-12), (fd, g)
    st = refpts.step(lin, o, 1e12)
    delta = st["delta"]
    assert g @ delta < 0 and fd @ delta < 0
    assert np.abs(H @ delta + fd).max() <= 1e-4 * np.abs(g).max()
    t = 1e-4  # the slope of the cost along the step
    cp = refpts.linearize(w, p, o, w.points[p] + t * delta)["cost"]
    cm = refpts.linearize(w, p, o, w.points[p] - t * delta)["cost"]
    assert (cp - cm) / (2 * t) == pytest.approx(g @ delta, rel=1e-4)
    assert st["mcc"] == pytest.approx(-(g @ delta + 0.5 * delta @ H @ delta), rel=1e-9)


@pytest.mark.parametrize("radius", refpts.STEP_RADII)
def test_first_steps_are_accepted(radius):
    """What test_gpu_pts.py's first-step test assumes of the counters: with one iteration and no tolerance every step
    track's first step is accepted, by a wide margin, in both references (also under the mixed Huber parameters)."""
    from refstep import NO_TOL
    w = refpts.step_tracks()
    for okw in ({}, refpts.HUBER_MIXED):
        o = oracle.default_options(max_num_iterations=1, initial_trust_region_radius=radius, **NO_TOL, **okw)
        for p in range(w.n_points):
            for T in (np.float64, LD):
                r = refpts.lm(w, p, o, T)
                assert r["accept"] == [1] and (r["n_succ"], r["n_unsucc"], r["termination"], r["msg"]) == \
                    (2, 0, 1, refpts.MSG_MAX_ITER)
                assert r["margin"] >= refloc.MARGIN_MIN


def test_noise_free_tracks_converge_to_the_truth():
    w = refpts.tracks_problem((2, 10, 40), seed=5, pixel_noise=0.0, depth_noise=0.0)
    o = oracle.default_options(function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-12)
    for p in range(w.n_points):
        r = refpts.lm(w, p, o)
        assert np.abs(r["X"] - w.meta["truth"][p]).max() < 1e-7
        assert r["final_cost"] < 1e-12 * r["initial_cost"]


def _all_tracks():
    yield from ((refpts.step_tracks(), p, r) for p, r in STEP_CASES)
    for hard in (False, True):
        w = refpts.loop_problem(hard)
        yield from ((w, p, 1e4) for p in range(w.n_points))


def test_f64_ratio():
    """The f64 restatement's step error in units of cond eps |step|, on every test track: the stored constant covers
    it, and is not stale by more than a factor two."""
    o = oracle.default_options()
    worst = 0.0
    for w, p, radius in _all_tracks():
        worst = max(worst, refpts.f64_ratio(refpts.linearize(w, p, o), o, radius))
    print(f"largest f64 ratio {worst:.3g}, stored {refpts.F64_RATIO}, F = {refpts.STEP_F}")
    assert worst <= refpts.F64_RATIO <= 2 * worst
    assert refpts.STEP_F == max(8.0, 4 * refpts.F64_RATIO)


@pytest.mark.parametrize("p", refpts.LOOP_EASY_TRACKS)
def test_easy_loop_tracks_qualify(p):
    a, b = refpts.loop_refs(False, p)
    assert a["accept"] == b["accept"] and a["termination"] == b["termination"] == 0
    assert a["msg"] == b["msg"] == refpts.MSG_FUNC_TOL
    assert a["accept"].count(0) == 0 and 10 <= a["iterations"] <= 41
    assert min(a["margin"], b["margin"]) >= refloc.MARGIN_MIN


def test_easy_loop_tracks_are_enough():
    assert len(refpts.LOOP_EASY_TRACKS) >= 12 and len(refpts.LOOP_HARD_TRACKS) >= 2
    w = refpts.loop_problem(False)
    adm = w.obs_depth > 1e-15
    assert np.all(np.bincount(w.obs_pt[adm], minlength=w.n_points) == 10)
    assert w.n_points == refpts.LANES  # one workgroup of points


@pytest.mark.parametrize("p", refpts.LOOP_HARD_TRACKS)
def test_hard_loop_tracks_qualify(p):
    a, b = refpts.loop_refs(True, p)
    assert a["accept"] == b["accept"] and a["termination"] == b["termination"] and a["msg"] == b["msg"]
    assert a["accept"].count(0) >= 1 and a["accept"].count(1) >= 1
    assert min(a["margin"], b["margin"]) >= refloc.MARGIN_MIN


@pytest.mark.parametrize("p", range(4))
def test_quick_tracks_take_two_iterations(p):
    a, b = refpts.loop_refs("quick", p)
    assert a["iterations"] == b["iterations"] == 2 and a["accept"] == b["accept"] == [1, -1]
    assert a["termination"] == b["termination"] == 0 and a["msg"] == b["msg"] == refpts.MSG_PARAM_TOL
    assert min(a["margin"], b["margin"]) >= refloc.MARGIN_MIN
    # and every easy track is still running after eight
    assert all(refpts.loop_refs(False, q)[0]["iterations"] > 8 for q in refpts.LOOP_EASY_TRACKS)


def test_loop_matches_the_oracle_at_the_start():
    """The restated loop against oracle.solve where the two problems coincide: the cost at the start and the
    admissible count (the oracle cannot hold cameras and intrinsics constant)."""
    w = refpts.loop_problem(False)
    r = refpts.lm(w, 5, oracle.default_options())
    sp = refpts.sub_problem(w, 5)
    s, tr = oracle.solve_trace(sp.copy(), oracle.default_options())
    assert r["rows"][0][0] == pytest.approx(tr[0][0], rel=1e-12)
    assert s["num_obs_admissible"] == refpts.linearize(w, 5)["n"] == 10


@pytest.mark.parametrize("hard,p", [(False, 2), (True, 4), (True, 14)])
def test_loop_first_iteration_matches_the_step_reference(hard, p):
    """Row 1 of the loop's log recomputed outside the loop from ``refpts.step``."""
    w, o = refpts.loop_problem(hard), oracle.default_options()
    row = refpts.loop_refs(hard, p)[1]["rows"][1]
    lin = refpts.linearize(w, p, o)
    st = refpts.step(lin, o)
    xc = w.points[p] + st["delta"]
    cand = refpts.linearize(w, p, o, xc)["cost"]
    change = lin["cost"] - cand
    rho = change / st["mcc"]
    assert row[1] == pytest.approx(change, rel=1e-9) and row[4] == pytest.approx(rho, rel=1e-9)
    assert row[3] == pytest.approx(float(np.linalg.norm(w.points[p] - xc)), rel=1e-9)
    assert row[6] == (1 if rho > o.min_relative_decrease else 0)
    assert row[0] == pytest.approx(cand, rel=1e-12)


@pytest.mark.parametrize("hard,p", [(False, 0), (True, 3), (True, 4), (True, 14)])
def test_loop_bookkeeping(hard, p):
    """The trust-region arithmetic of the log, row to row (refloc's test of the same name)."""
    o = oracle.default_options()
    r = refpts.loop_refs(hard, p)[0]
    rows = r["rows"]
    radius, dec, cost = o.initial_trust_region_radius, 2.0, rows[0][0]
    for row in rows[1:]:
        if row[6] == 1:
            assert row[4] > o.min_relative_decrease and row[0] < cost
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * row[4] - 1.0) ** 3), o.max_trust_region_radius)
            dec, cost = 2.0, row[0]
        elif row[6] == 0:
            assert row[4] <= o.min_relative_decrease
            radius, dec = radius / dec, 2.0 * dec
        assert row[5] == pytest.approx(radius, rel=1e-12)
    assert r["n_succ"] == 1 + r["accept"].count(1) and r["n_unsucc"] == r["accept"].count(0)
    assert r["iterations"] == len(rows) - 1 <= o.max_num_iterations
    assert r["final_cost"] <= cost


def test_evaluation_failure_of_a_nan_position():
    w = refpts.loop_problem(False).copy()
    w.points[2, 1] = np.nan
    r = refpts.lm(w, 2, oracle.default_options())
    assert (r["termination"], r["msg"], r["iterations"]) == (2, refpts.MSG_EVAL_FAIL, 0) and len(r["rows"]) == 0


def test_huber_case_has_every_zone():
    w, o = refpts.step_tracks(), oracle.default_options(**refpts.HUBER_MIXED)
    assert all(n >= 1 for n in refpts.huber_zones(w, refpts.HUBER_TRACK, o))
    # with the defaults nearly every block is linear
    z = refpts.huber_zones(w, refpts.HUBER_TRACK, oracle.default_options())
    assert z[1] + z[3] >= 0.9 * sum(z)
