"""The references of ba_pose_graph (tests/refpg.py) and the host helpers of miba/posegraph.py, on the CPU:

* the analytic Jacobians against central differences through refcand.retract_quat, including an edge with a rotation
  error near 90 degrees and edges whose dq has w < 0 before the flip;
* the longdouble step against a refined QR solve of the damped least-squares problem;
* the round trips of posegraph's helpers;
* test_f64_ratio, which sets the GPU's first-step tolerance;
* that every whole-loop graph of the GPU test qualifies, and that the set has the ends it must have."""
import numpy as np
import pytest

import refcand
import refpg
from miba import posegraph
from oracle import oracle
from refstep import EPS64, LD


def _retract(T, d):
    q, t = refcand.retract_quat(T, d)
    return np.concatenate([q, t])


def _residual_at(g, cams_ld):
    # refpg.residual converts its poses through f64; the differences need the longdouble poses themselves
    T = LD
    x = cams_ld
    ea, eb = np.asarray(g["ea"]), np.asarray(g["eb"])
    z = np.asarray(g["meas"], dtype=np.float64).astype(T).reshape(-1, 7)
    w = refpg.weights_of(g).astype(T)
    xa, xb = x[ea], x[eb]
    Ra, Rb = refpg._quat_R(xa[:, :4]), refpg._quat_R(xb[:, :4])
    th = np.einsum("mki,mk->mi", Ra, xb[:, 4:] - xa[:, 4:])
    qh = posegraph.quat_mul(posegraph.quat_conj(xa[:, :4]), xb[:, :4])
    dq = posegraph.quat_mul(z[:, :4], posegraph.quat_conj(qh))
    dq = np.where((dq[:, 3] < 0)[:, None], -dq, dq)
    return np.concatenate([w[:, :1] * (th - z[:, 4:]), w[:, 1:] * (2 * dq[:, :3])], axis=1), None, None, None


def _special_graph():
    """Three edges on four poses: a rotation error near 90 degrees, a measurement given on the other hemisphere
    (dq.w < 0 before the flip), and an ordinary weighted one."""
    rng = np.random.default_rng(7)
    truth = refpg.trajectory(4, rng)
    pairs = np.array([(0, 1), (1, 2), (3, 2)])
    ea, eb, meas = posegraph.edges_from_poses(truth, pairs)
    cams = refpg.perturb(truth, rng, 0.02, 0.05)
    # pose 1 turned by about 90 degrees: both of its edges see a large rotation error
    cams[1, :4] = posegraph.quat_mul(cams[1, :4], refpg._rodrigues_quat(np.array([0.3, -1.4, 0.5])))
    meas[1, :4] *= -1
    meas[2, :4] *= -1
    weights = np.array([[1.0, 1.0], [2.0, 0.5], [0.7, 3.0]])
    return dict(cams=cams, ea=ea, eb=eb, meas=meas, weights=weights, constant=np.zeros(4, dtype=bool), huber=0.0)


@pytest.mark.parametrize("huber", [0.0, 0.8])
def test_jacobians_against_central_differences(huber):
    g = _special_graph()
    g["huber"] = huber
    r, th, dq, Rh, neg = refpg.residual(g, None, LD, flipped=True)
    ang = 2 * np.degrees(np.arcsin(np.minimum(1, np.sqrt((dq[:, :3] ** 2).sum(1)).astype(np.float64))))
    assert ang[0] > 75 and ang[1] > 75  # the rotation errors near 90 degrees
    assert neg.any() and not neg.all()  # both hemispheres before the flip
    lin = refpg.linearize(g, None, LD)
    s = (r * r).sum(1)
    if huber:
        assert (s > huber * huber).any() and (s <= huber * huber).any()  # both zones
    x0 = np.asarray(g["cams"], dtype=np.float64).astype(LD)
    x0[:, :4] /= np.sqrt((x0[:, :4] ** 2).sum(1))[:, None]  # retract_quat normalises: differentiate at unit quaternions
    g0 = dict(g, cams=x0.astype(np.float64))
    h = LD(1e-7)
    sq = (lin["f"][:, 0] / r[:, 0])  # sqrt(rho') of every edge (constant to first order only in the quadratic zone)
    for k, (a, b) in enumerate(zip(g["ea"], g["eb"])):
        for side, c in (("Ja", a), ("Jb", b)):
            J = np.zeros((6, 6), dtype=LD)
            for d in range(6):
                e = np.zeros(6, dtype=LD)
                e[d] = h
                xp, xm = x0.copy(), x0.copy()
                xp[c], xm[c] = _retract(x0[c], e), _retract(x0[c], -e)
                rp, rm = _residual_at(g0, xp)[0][k], _residual_at(g0, xm)[0][k]
                J[:, d] = (rp - rm) / (2 * h)
            # the analytic Jacobian of the plain residual: the robustified one divided by the corrector's factor
            Jan = refpg.linearize(dict(g0, huber=0.0), None, LD)[side][k]
            assert np.abs(J - Jan).max() <= 1e-9 * max(1.0, np.abs(Jan).max()), (k, side)
            assert np.abs(lin[side][k] - sq[k] * refpg.linearize(dict(g, huber=0.0), None, LD)[side][k]).max() <= 1e-15


def test_step_against_qr():
    """The normal-equation step equals the least-squares solution of [J s; D] y = [f; 0] by QR, refined."""
    for topology, n in (("loop", 11), ("dup", 22), ("isolated", 11)):
        g = refpg.step_graph(topology, n)
        opts = oracle.default_options()
        for radius in refpg.STEP_RADII:
            ref = refpg.step(g, opts, radius)
            lin = refpg.linearize(g, None, LD)
            act, pos = refpg._pos(g)
            m, na = len(g["ea"]), len(act)
            J = np.zeros((6 * m, 6 * na), dtype=LD)
            for k, (a, b) in enumerate(zip(g["ea"], g["eb"])):
                if pos[a] >= 0:
                    J[6 * k:6 * k + 6, 6 * pos[a]:6 * pos[a] + 6] = lin["Ja"][k]
                if pos[b] >= 0:
                    J[6 * k:6 * k + 6, 6 * pos[b]:6 * pos[b] + 6] = lin["Jb"][k]
            s = ref["scale"]
            d2 = np.diag(ref["A"]) - (J * J).sum(0) * s * s
            Aug = np.concatenate([J * s[None, :], np.diag(np.sqrt(d2))])
            rhs = np.concatenate([lin["f"].reshape(-1), np.zeros(6 * na, dtype=LD)])
            Q, R = np.linalg.qr(Aug.astype(np.float64))
            y = np.zeros(6 * na, dtype=LD)
            for _ in range(4):  # refinement on the semi-normal equations with extended-precision residuals
                res = (Aug.T @ (rhs - Aug @ y)).astype(np.float64)
                y = y + np.linalg.solve(R, np.linalg.solve(R.T, res)).astype(LD)
            delta = (-s * y).reshape(-1, 6)
            err = float(np.abs(delta - ref["delta_ld"]).max())
            # the two extended-precision solves agree a thousand times finer than the unit of the GPU's bound
            assert err <= 1e-3 * ref["cond"] * EPS64 * float(np.abs(delta).max()) + 1e-30, (topology, n, radius, err)
            assert ref["mcc"] > 0


def test_f64_ratio():
    """The error of the plain-f64 restatement of the step against the longdouble step, in units of
    cond eps |step|_inf, on every first-step graph the GPU test uses. refpg.F64_RATIO must cover it and not be stale
    by more than a factor two; the GPU bound is F = max(8, 4 F64_RATIO)."""
    worst, where = 0.0, None
    graphs = [((t, n), refpg.step_graph(t, n)) for t, n in refpg.STEP_CASES] + [("huber", refpg.huber_graph())]
    for key, g in graphs:
        for radius in refpg.STEP_RADII:
            if not refpg._with_edge(g).any():
                continue  # the step is exactly zero
            fr = refpg.f64_ratio(g, None, radius)
            if fr > worst:
                worst, where = fr, (key, radius)
    print(f"f64 ratio: {worst:.3f} at {where}; stored {refpg.F64_RATIO}, F = {refpg.STEP_F}")
    assert worst <= refpg.F64_RATIO <= 2 * worst
    assert refpg.STEP_F == max(8.0, 4 * refpg.F64_RATIO)


def test_step_cases_cover_the_layout():
    sizes = {n for t, n in refpg.STEP_CASES if t == "chain"}
    assert sizes == {1, 2, 3, 10, 11, 22, 43}
    assert {t for t, _ in refpg.STEP_CASES} == set(refpg.TOPOLOGIES)
    for t, n in refpg.STEP_CASES:
        g = refpg.step_graph(t, n)
        assert len(refpg.active(g)) == n, (t, n)
    g = refpg.step_graph("dup", 11)
    pairs = {}
    for a, b in zip(g["ea"], g["eb"]):
        pairs.setdefault((min(a, b), max(a, b)), []).append((a, b))
    assert any(len(set(v)) == 2 for v in pairs.values())  # reversed edges of one pair
    assert any(len(v) > len(set(v)) for v in pairs.values())  # duplicate edges of one pair
    g = refpg.step_graph("const_edge", 11)
    c = np.asarray(g["constant"])
    assert any(c[a] and c[b] for a, b in zip(g["ea"], g["eb"]))
    g = refpg.step_graph("isolated", 11)
    assert (~refpg._with_edge(g)).sum() == 1
    quad, lin = refpg.huber_zones(refpg.huber_graph())
    assert quad >= 3 and lin >= 3 and refpg.huber_graph()["weights"] is not None


@pytest.mark.parametrize("name", [c[0] for c in refpg.LOOP_CASES])
def test_loop_cases_qualify(name):
    a, b = refpg.loop_refs(name)
    print(f"{name}: accept {a['accept']} msg {a['msg']} margin {a['margin']:.3g} / {b['margin']:.3g} "
          f"cost {a['initial_cost']:.4g} -> {a['final_cost']:.4g}")
    assert a["accept"] == b["accept"] and (a["termination"], a["msg"]) == (b["termination"], b["msg"])
    assert (a["iterations"], a["n_succ"], a["n_unsucc"]) == (b["iterations"], b["n_succ"], b["n_unsucc"])
    assert min(a["margin"], b["margin"]) >= refpg.MARGIN_MIN
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * b["final_cost"]
    assert b["final_cost"] > 1e-8  # well above the rounding floor: a relative bound on it means something


def test_loop_cases_have_the_required_ends():
    refs = {c[0]: refpg.loop_refs(c[0])[1] for c in refpg.LOOP_CASES}
    assert any(0 in r["accept"] for r in refs.values())  # a rejected step
    assert any(r["msg"] == refpg.MSG_FUNC_TOL for r in refs.values())
    assert any(r["msg"] == refpg.MSG_MAX_ITER for r in refs.values())


def test_loop_closure_reference():
    g, r = refpg.closure(), refpg.closure_ref()
    before, after = refpg.pose_rms(g["cams"], g["truth"]), refpg.pose_rms(r["cams"], g["truth"])
    assert len(refpg.active(g)) == 199 and r["termination"] == 0
    assert after < 0.25 * before


def test_posegraph_round_trips():
    rng = np.random.default_rng(3)
    cams = refpg.trajectory(12, rng)
    # relative_pose / compose, single and batched
    Z = posegraph.relative_pose(cams[2], cams[7])
    np.testing.assert_allclose(posegraph.compose(cams[2], Z), cams[7], atol=1e-14)
    pairs = np.array([(0, 1), (5, 2), (11, 3)])
    ea, eb, meas = posegraph.edges_from_poses(cams, pairs)
    assert ea.dtype == np.int32 and ea.tolist() == [0, 5, 11] and eb.tolist() == [1, 2, 3]
    np.testing.assert_allclose(posegraph.compose(cams[ea], meas), cams[eb], atol=1e-14)
    # edges measured on the poses themselves have zero residual there
    g = dict(cams=cams, ea=ea, eb=eb, meas=meas, weights=None, constant=np.zeros(12, dtype=bool), huber=0.0)
    assert float(refpg.linearize(g, None, np.float64)["total"]) < 1e-28
    ea0, eb0, m0 = posegraph.edges_from_poses(cams, np.zeros((0, 2)))
    assert len(ea0) == 0 and m0.shape == (0, 7)
    # transfer_points: a point seen from its reference keyframe keeps its camera-frame coordinates
    after = refpg.perturb(cams, rng, 0.2, 0.5)
    X = rng.normal(0, 2, (30, 3))
    ref = rng.integers(0, 12, 30)
    Y = posegraph.transfer_points(X, ref, cams, after)
    loc_b = posegraph.quat_rotate(posegraph.quat_conj(cams[ref, :4]), X - cams[ref, 4:])
    loc_a = posegraph.quat_rotate(posegraph.quat_conj(after[ref, :4]), Y - after[ref, 4:])
    np.testing.assert_allclose(loc_a, loc_b, atol=1e-13)
    np.testing.assert_allclose(posegraph.transfer_points(Y, ref, after, cams), X, atol=1e-13)
    np.testing.assert_array_equal(posegraph.transfer_points(X, ref, cams, cams).round(12), X.round(12))


def test_covis_edges():
    # two clusters joined by one weak link, an isolated camera
    W = np.zeros((7, 7), dtype=np.int32)
    for i, j, w in ((0, 1, 50), (1, 2, 40), (0, 2, 5), (3, 4, 60), (4, 5, 3), (3, 5, 2), (2, 3, 1)):
        W[i, j] = W[j, i] = w
    np.fill_diagonal(W, 100)
    e = posegraph.covis_edges(W, 30)
    got = {tuple(p) for p in e.tolist()}
    # the strong pairs, plus the spanning forest's weak links (4-5 beats 3-5; 2-3 joins the clusters); 0-2 and 3-5 not
    assert got == {(0, 1), (1, 2), (3, 4), (4, 5), (2, 3)}
    assert e.dtype == np.int32 and e.tolist() == sorted(e.tolist())
    assert all(6 not in p for p in got)
    # a threshold above every weight leaves the spanning forest alone: n - components edges
    assert len(posegraph.covis_edges(W, 1000)) == 5
    assert len(posegraph.covis_edges(W, 1)) == 7
