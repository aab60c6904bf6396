"""The references of ba_localize (tests/refloc.py) checked on the CPU, and the conditions test_gpu_loc.py rests on:
the longdouble step against an independent QR solve, the gradient against finite differences of the cost, convergence
of noise-free frames to the true pose, the measured f64 ratio behind the step bound's factor, the margins of the loop
frames' decisions, and the Huber case's four zones."""
import numpy as np
import pytest

import refcand
import refloc
from oracle import oracle
from refstep import EPS64, LD

STEP_CASES = [(c, r) for c in range(len(refloc.STEP_COUNTS)) for r in refloc.STEP_RADII]


def test_frames_problem_counts():
    p = refloc.step_frames()
    adm = p.obs_depth > 1e-15
    assert tuple(np.bincount(p.obs_cam[adm], minlength=p.n_cams)) == refloc.STEP_COUNTS
    assert (~adm).sum() >= p.n_cams  # inadmissible observations mixed in, for every camera
    assert np.any(np.diff(p.obs_cam) < 0)  # shuffled
    pairs = np.stack([p.obs_cam[adm], p.obs_pt[adm]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)  # repeated observations
    assert refloc.B == 256


@pytest.mark.parametrize("c,radius", STEP_CASES)
def test_longdouble_step_matches_qr(c, radius):
    """[J s; D] y = -f by dense QR in f64, refined three times with the residual A^T (b - A y) in extended precision
    (R from the QR as the preconditioner): no normal equations are formed. Each pass gains a factor cond eps, so the
    result is far inside 8 cond eps |step|, the bound a single f64 solve of the normal equations would get."""
    p, o = refloc.step_frames(), oracle.default_options()
    lin = refloc.linearize(p, c, o)
    ref = refloc.step(lin, o, radius)
    A = np.concatenate([lin["J"].reshape(-1, 6).astype(LD) * ref["scale"], np.diag(np.sqrt(ref["d2"]))])
    b = np.concatenate([-lin["f"].reshape(-1).astype(LD), np.zeros(6, LD)])
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


@pytest.mark.parametrize("c", [2, 4, 8])
def test_gradient_matches_finite_differences(c):
    p, o = refloc.step_frames(), oracle.default_options(**refloc.HUBER_MIXED)
    lin = refloc.linearize(p, c, o)
    g = np.einsum("ord,or->d", lin["J"], lin["f"])
    h = 1e-6
    for d in range(6):
        e = np.zeros(6)
        e[d] = h
        cp = refloc.linearize(p, c, o, oracle.se3_plus(p.cams[c], e))["cost"]
        cm = refloc.linearize(p, c, o, oracle.se3_plus(p.cams[c], -e))["cost"]
        fd = (cp - cm) / (2 * h)
        assert abs(fd - g[d]) <= 1e-5 * max(abs(g).max(), 1e-12), (d, fd, g[d])


def test_noise_free_frames_converge_to_the_truth():
    p = refloc.frames_problem((6, 40, 300), seed=5, pixel_noise=0.0, depth_noise=0.0, dup_frac=0.0)
    o = oracle.default_options(function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-12)
    for c in range(p.n_cams):
        r = refloc.lm(p, c, o)
        truth = p.meta["truth"][c]
        sign = np.sign(truth[:4] @ r["pose"][:4])
        assert np.abs(r["pose"][:4] * sign - truth[:4]).max() < 1e-7
        assert np.abs(r["pose"][4:] - truth[4:]).max() < 1e-6
        assert r["final_cost"] < 1e-12 * r["initial_cost"]


def _all_frames():
    yield from ((refloc.step_frames(), c, r) for c, r in STEP_CASES)
    for hard in (False, True):
        p = refloc.loop_problem(hard)
        yield from ((p, c, 1e4) for c in range(p.n_cams))


def test_f64_ratio():
    """The f64 restatement's step error in units of cond eps |step|, on every test frame: the stored constant covers
    it, and is not stale by more than a factor two."""
    o = oracle.default_options()
    worst = 0.0
    for p, c, radius in _all_frames():
        worst = max(worst, refloc.f64_ratio(refloc.linearize(p, c, o), o, radius))
    print(f"largest f64 ratio {worst:.3g}, stored {refloc.F64_RATIO}, F = {refloc.STEP_F}")
    assert worst <= refloc.F64_RATIO <= 2 * worst
    assert refloc.STEP_F == max(8.0, 4 * refloc.F64_RATIO)


@pytest.mark.parametrize("c", range(12))
def test_easy_loop_frames_qualify(c):
    a, b = refloc.loop_refs(False, c)
    assert a["accept"] == b["accept"] and a["termination"] == b["termination"] == 0
    assert a["msg"] == b["msg"] == refloc.MSG_FUNC_TOL
    assert a["accept"].count(0) == 0 and 12 <= a["iterations"] <= 22
    assert min(a["margin"], b["margin"]) >= refloc.MARGIN_MIN


@pytest.mark.parametrize("c", refloc.LOOP_HARD_FRAMES)
def test_hard_loop_frames_qualify(c):
    a, b = refloc.loop_refs(True, c)
    assert a["accept"] == b["accept"] and a["termination"] == b["termination"] and a["msg"] == b["msg"]
    assert a["accept"].count(0) >= 1
    assert min(a["margin"], b["margin"]) >= refloc.MARGIN_MIN


def test_hard_loop_frames_cover_rejection_and_iteration_limit():
    refs = {c: refloc.loop_refs(True, c)[0] for c in refloc.LOOP_HARD_FRAMES}
    assert refs[6]["accept"][:2] == [0, 0] and refs[6]["msg"] == refloc.MSG_FUNC_TOL
    assert refs[3]["msg"] == refloc.MSG_MAX_ITER and refs[3]["termination"] == 1 and refs[3]["iterations"] == 75
    assert any(r["termination"] == 0 and r["accept"].count(0) for r in refs.values())


def test_loop_matches_the_oracle_on_a_one_camera_window():
    """The restated loop against oracle.solve where the two problems coincide. The oracle cannot hold points and
    intrinsics constant, so only the cost at the start and the admissible count can be compared: its gradient norm
    and its steps include the points' and the intrinsics' columns."""
    p = refloc.loop_problem(False)
    r = refloc.lm(p, 5, oracle.default_options())
    sp = refloc.sub_problem(p, 5)
    s, tr = oracle.solve_trace(sp.copy(), oracle.default_options())
    assert r["rows"][0][0] == pytest.approx(tr[0][0], rel=1e-14)
    assert s["num_obs_admissible"] == refloc.linearize(p, 5)["n"]


@pytest.mark.parametrize("hard,c", [(False, 2), (True, 6), (True, 3)])
def test_loop_first_iteration_matches_the_step_reference(hard, c):
    """Row 1 of the loop's log recomputed outside the loop: the step from ``refloc.step`` (checked against the QR solve
    above), the candidate by oracle.se3_plus, its cost by a fresh linearisation, rho against the step's own model
    cost change. Both sides are longdouble sums of the same f64 terms, so they agree far inside 1e-9."""
    p, o = refloc.loop_problem(hard), oracle.default_options()
    row = refloc.loop_refs(hard, c)[1]["rows"][1]
    lin = refloc.linearize(p, c, o)
    st = refloc.step(lin, o)
    xc = oracle.se3_plus(p.cams[c], st["delta"])
    cand = refloc.linearize(p, c, o, xc)["cost"]
    change = lin["cost"] - cand
    rho = change / st["mcc"]
    assert row[1] == pytest.approx(change, rel=1e-9) and row[4] == pytest.approx(rho, rel=1e-9)
    assert row[3] == pytest.approx(float(np.linalg.norm(p.cams[c] - xc)), rel=1e-9)
    assert row[6] == (1 if rho > o.min_relative_decrease else 0)
    assert row[0] == pytest.approx(cand, rel=1e-12)


@pytest.mark.parametrize("hard,c", [(False, 0), (True, 3), (True, 6), (True, 7)])
def test_loop_bookkeeping(hard, c):
    """The trust-region arithmetic of the log, row to row, as Ceres' LevenbergMarquardtStrategy states it: an accepted
    step divides the radius by max(1/3, 1 - (2 rho - 1)^3), the k-th rejection in a row divides it by 2^k; the cost
    column is the candidate's, accepted rows decrease, and the counters add up."""
    o = oracle.default_options()
    r = refloc.loop_refs(hard, c)[0]
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
        assert row[1] == pytest.approx(cost - row[0] if row[6] != 1 else row[1], rel=1e-9, abs=1e-18)
    assert r["n_succ"] == 1 + r["accept"].count(1) and r["n_unsucc"] == r["accept"].count(0)
    assert r["iterations"] == len(rows) - 1 <= o.max_num_iterations
    assert r["final_cost"] <= cost


def test_huber_case_has_every_zone():
    p, o = refloc.step_frames(), oracle.default_options(**refloc.HUBER_MIXED)
    assert all(n >= 1 for n in refloc.huber_zones(p, refloc.HUBER_FRAME, o))
    # with the defaults nearly every block is linear
    z = refloc.huber_zones(p, refloc.HUBER_FRAME, oracle.default_options())
    assert z[1] + z[3] >= 0.9 * sum(z)


def test_retraction_reference_is_refcand():
    T = refloc.step_frames().cams[3]
    d = np.array([0.01, -0.02, 0.005, 0.003, -0.004, 0.002])
    q, t = refcand.retract_quat(T, d)
    got = oracle.se3_plus(T, d)
    bq, bt = refcand.retraction_bound(T, d, cancelling_a=True)
    assert np.abs(got[:4] - q.astype(np.float64)).max() <= bq and np.abs(got[4:] - t.astype(np.float64)).max() <= bt
