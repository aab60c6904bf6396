"""ba_refine_points on the GPU against tests/refpts.py (test_refpts.py checks the references and that the tracks used
here qualify).

* the first step (max_num_iterations = 1, from the generator's perturbed positions) against X + the longdouble step,
  within F cond eps |step|_inf + 2 eps |X|_inf, F = refpts.STEP_F, at three radii and at the group's observation-count
  boundaries (1, 2, L - 1, L, L + 1, 2 L - 1, 2 L, 2 L + 1, 4 L + 1 for L = PTS_LANES lanes per point); once more with
  Huber parameters that put blocks of both kinds in both zones;
* the whole loop on tracks whose accept / reject sequence is settled (the f64 and longdouble references agree and no
  decision is closer than 1e-3 to its threshold): the sequence, the counters, the termination, the final cost and the
  final position;
* bits and independence: two calls, alone against in the batch, batch sizes around the group / wave / workgroup
  boundaries, wave-mates that stop early, run long or fail, the mask, min_obs, inadmissible observations;
* no side effect on a prepared window; the errors; empty windows; the pipeline hook."""
import numpy as np
import pytest

import refpts
import refstep
from oracle import oracle
from refstep import EPS64, LD, NO_TOL

pytestmark = pytest.mark.gpu

L = refpts.LANES
ARRAYS = ("cams", "intr", "intr_prior", "obs_uv", "obs_depth", "obs_cam", "obs_pt")


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def _step_refs(okw_key):
    """The longdouble first steps of every step track at every radius (cached, shared)."""
    def make():
        w = refpts.step_tracks()
        out = {}
        for radius in refpts.STEP_RADII:
            o = oracle.default_options(**dict(okw_key))
            for p in range(w.n_points):
                out[p, radius] = refpts.step(refpts.linearize(w, p, o), o, radius)
        return out
    return refpts.cached(("gpu_pts_step_refs", okw_key), make)


def _check_first_step(radius, okw, tracks):
    w = refpts.step_tracks()
    refs = _step_refs(tuple(sorted(okw.items())))
    q = w.copy()
    with solver(max_num_iterations=1, initial_trust_region_radius=radius, **NO_TOL, **okw) as s:
        r = s.refine_points(q)
    assert r["n_selected"] == r["n_solved"] == w.n_points and r["max_iterations"] == 1
    for p in tracks:
        ref = refs[p, radius]
        st = r["stats"][p]
        n = refpts.STEP_COUNTS[p]
        want = w.points[p].astype(LD) + ref["delta_ld"]
        err = float(np.abs(q.points[p].astype(LD) - want).max())
        bound = refpts.step_bound(ref) + 2 * EPS64 * float(np.abs(w.points[p]).max())
        print(f"FIRST n={n} radius={radius:g} cond={ref['cond']:.3g} |step|={np.abs(ref['delta']).max():.2e} "
              f"err={err:.2e} bound={bound:.2e} stats={st[3:].tolist()}")
        assert st[0] == n and st[3] == 1
        assert (st[4], st[5], st[6], st[7]) == (2, 0, 1, refpts.MSG_MAX_ITER), st  # the step was accepted
        assert err <= bound, (n, radius, err, bound)
        lin = refpts.linearize(w, p, oracle.default_options(**okw))
        assert abs(st[1] - lin["cost"]) <= 1e-6 * lin["cost"]
    for k in ARRAYS:
        np.testing.assert_array_equal(getattr(q, k), getattr(w, k))
    return r


@pytest.mark.parametrize("radius", refpts.STEP_RADII)
def test_first_step(radius):
    _check_first_step(radius, {}, range(len(refpts.STEP_COUNTS)))


def test_first_step_huber_zones():
    _check_first_step(1e4, refpts.HUBER_MIXED, [refpts.HUBER_TRACK])


def _check_loop(hard, p):
    w = refpts.loop_problem(hard)
    a, b = refpts.loop_refs(hard, p)
    q = w.copy()
    with solver() as s:
        r = s.refine_points(q, points=[p], log_pt=p)
    st, log = r["stats"][p], r["log"]
    spread = float(np.abs(a["X"] - b["X"]).max())
    tol = 16 * max(spread, 64 * EPS64 * max(1.0, float(np.abs(b["X"]).max())))
    err = float(np.abs(q.points[p] - b["X"]).max())
    rel = abs(st[2] - b["final_cost"]) / b["final_cost"]
    print(f"LOOP hard={hard} p={p} iters={int(st[3])}/{b['iterations']} rej={b['accept'].count(0)} "
          f"cost rel={rel:.2e} X err={err:.2e} tol={tol:.2e} spread={spread:.2e}")
    assert r["log_rows"] == b["iterations"] + 1 == len(log)
    assert log[1:, 6].astype(int).tolist() == b["accept"]
    assert (st[3], st[4], st[5], st[6], st[7]) == (b["iterations"], b["n_succ"], b["n_unsucc"], b["termination"], b["msg"])
    assert rel <= 1e-6
    assert abs(st[1] - b["initial_cost"]) <= 1e-6 * b["initial_cost"]
    assert err <= tol
    # the log's own consistency: row 0 and the last accepted cost
    assert log[0, 0] == st[1] and log[0, 6] == 1 and np.all(log[:, 7] == 0)
    assert st[2] <= st[1]
    others = np.arange(w.n_points) != p
    np.testing.assert_array_equal(q.points[others], w.points[others])
    assert np.all(r["stats"][others, 6] == -1)


@pytest.mark.parametrize("p", refpts.LOOP_EASY_TRACKS)
def test_loop_all_steps_accepted(p):
    _check_loop(False, p)


@pytest.mark.parametrize("p", refpts.LOOP_HARD_TRACKS)
def test_loop_with_rejections(p):
    _check_loop(True, p)


@pytest.fixture(scope="module")
def base():
    """The easy loop window solved whole, once: (the solved copy, the result)."""
    w = refpts.loop_problem(False)
    a = w.copy()
    with solver() as s:
        ra = s.refine_points(a)
    assert ra["n_solved"] == w.n_points == L and np.all(ra["stats"][:, 6] == 0)
    assert not np.array_equal(a.points, w.points)
    return a, ra


def test_two_calls_give_the_same_bits(base):
    a, ra = base
    w = refpts.loop_problem(False)
    with solver() as s:
        for _ in range(2):
            b = w.copy()
            rb = s.refine_points(b)
            np.testing.assert_array_equal(b.points, a.points)
            np.testing.assert_array_equal(rb["stats"], ra["stats"])


def test_a_point_alone_against_in_the_batch(base):
    """One point from each of the four groups of a wave (and of two different waves), alone: row 0 of wave 0 then."""
    a, ra = base
    w = refpts.loop_problem(False)
    with solver() as s:
        for p in (0, 1, 2, 3, 6, 15):
            q = w.copy()
            rq = s.refine_points(q, points=[p], log_pt=p)
            np.testing.assert_array_equal(q.points[p], a.points[p])
            np.testing.assert_array_equal(rq["stats"][p], ra["stats"][p])
            assert rq["n_solved"] == 1 and rq["log_rows"] == ra["stats"][p, 3] + 1
            assert rq["log"][-1, 0] <= rq["log"][0, 0]


@pytest.mark.parametrize("n", [1, 3, 4, 5, L - 1, L, L + 1, L * 300 + 1])
def test_batch_sizes(base, n):
    """A partial group of a wave, a partial wave, a partial workgroup, and 301 workgroups: more than the device has
    compute units."""
    a, ra = base
    times = -(-n // L)
    big = refpts.cached(("pts_tile", times), lambda: refpts.tile(refpts.loop_problem(False), times))
    q = big.copy()
    with solver() as s:
        r = s.refine_points(q, points=np.arange(n))
    assert r["n_selected"] == r["n_solved"] == n
    np.testing.assert_array_equal(q.points[:n], np.tile(a.points, (times, 1))[:n])
    np.testing.assert_array_equal(r["stats"][:n], np.tile(ra["stats"], (times, 1))[:n])
    np.testing.assert_array_equal(q.points[n:], big.points[n:])
    assert np.all(r["stats"][n:, 6] == -1)


def test_quick_point_beside_points_that_run_to_the_limit():
    """Point 0 converges in two iterations; its three wave-mates and the twelve other points of the workgroup run
    into max_num_iterations = 8. Its bits are its bits alone, and theirs are theirs without it."""
    w = refpts.merge(refpts.loop_problem("quick"), refpts.loop_problem(False))
    slow = np.arange(4, w.n_points)
    with solver(max_num_iterations=8) as s:
        alone = w.copy()
        r1 = s.refine_points(alone, points=[0])
        assert r1["stats"][0, 3] == 2 and r1["stats"][0, 6] == 0 and r1["stats"][0, 7] == refpts.MSG_PARAM_TOL
        rest = w.copy()
        r2 = s.refine_points(rest, points=slow)
        assert np.all(r2["stats"][slow, 3] == 8) and np.all(r2["stats"][slow, 6] == 1)
        both = w.copy()
        sel = np.concatenate([[0], slow])  # the quick point is group 0 of the first wave, slow ones fill the rest
        r3 = s.refine_points(both, points=sel)
        assert r3["n_solved"] == len(sel) and r3["max_iterations"] == 8
        np.testing.assert_array_equal(both.points[0], alone.points[0])
        np.testing.assert_array_equal(r3["stats"][0], r1["stats"][0])
        np.testing.assert_array_equal(both.points[slow], rest.points[slow])
        np.testing.assert_array_equal(r3["stats"][slow], r2["stats"][slow])
        np.testing.assert_array_equal(both.points[1:4], w.points[1:4])
    ref = refpts.loop_refs("quick", 0)[1]
    assert np.abs(alone.points[0] - ref["X"]).max() <= 1e-12


def test_nan_point_beside_healthy_ones(base):
    """A position that is not finite: BA_FAILURE with the evaluation-failed message, the position kept, no log row;
    its wave-mates and the other points as without it."""
    a, ra = base
    w = refpts.loop_problem(False)
    q = w.copy()
    q.points[2, 1] = np.nan
    given = q.points[2].copy()
    with solver() as s:
        r = s.refine_points(q, log_pt=2)
    st = r["stats"][2]
    assert (st[0], st[3], st[6], st[7]) == (10, 0, 2, refpts.MSG_EVAL_FAIL) and np.isnan(st[1]) and np.isnan(st[2])
    assert r["log_rows"] == 0 and len(r["log"]) == 0 and r["n_failure"] == 1 and r["n_solved"] == w.n_points
    np.testing.assert_array_equal(q.points[2], given)
    keep = np.arange(w.n_points) != 2
    np.testing.assert_array_equal(q.points[keep], a.points[keep])
    np.testing.assert_array_equal(r["stats"][keep], ra["stats"][keep])


def test_mask_and_min_obs(base):
    a, ra = base
    w = refpts.loop_problem(False)
    with solver() as s:
        q = w.copy()
        mask = np.arange(w.n_points) % 3 == 1
        r = s.refine_points(q, points=mask)
        assert r["n_selected"] == r["n_solved"] == int(mask.sum())
        np.testing.assert_array_equal(q.points[mask], a.points[mask])
        np.testing.assert_array_equal(r["stats"][mask], ra["stats"][mask])
        np.testing.assert_array_equal(q.points[~mask], w.points[~mask])
        for k in ARRAYS:
            np.testing.assert_array_equal(getattr(q, k), getattr(w, k))
        assert np.all(r["stats"][~mask, 6] == -1) and np.all(np.delete(r["stats"][~mask], 6, axis=1) == 0)
        # min_obs: point 5 keeps 3 admissible observations, point 9 none; the threshold 4 leaves both alone
        q = w.copy()
        k5 = np.nonzero((q.obs_pt == 5) & (q.obs_depth > 1e-15))[0]
        q.obs_depth[k5[3:]] = 0.0
        q.obs_depth[q.obs_pt == 9] = -np.inf
        given = q.copy()
        r = s.refine_points(q, min_obs=4)
        keep = ~np.isin(np.arange(w.n_points), (5, 9))
        assert r["n_selected"] == w.n_points and r["n_solved"] == w.n_points - 2
        for p in (5, 9):
            np.testing.assert_array_equal(q.points[p], w.points[p])
            assert r["stats"][p].tolist() == [0, 0, 0, 0, 0, 0, -1, 0]
        np.testing.assert_array_equal(q.points[keep], a.points[keep])
        np.testing.assert_array_equal(r["stats"][keep], ra["stats"][keep])
        np.testing.assert_array_equal(q.obs_depth, given.obs_depth)
        # at the default threshold point 5 is solved on its three observations, point 9 still is not
        q = given.copy()
        r = s.refine_points(q)
        assert r["n_solved"] == w.n_points - 1 and r["stats"][5, 0] == 3 and r["stats"][5, 6] == 0
        assert r["stats"][9].tolist() == [0, 0, 0, 0, 0, 0, -1, 0]
        assert not np.array_equal(q.points[5], w.points[5])
        np.testing.assert_array_equal(q.points[9], w.points[9])


def test_inadmissible_observations_in_between(base):
    """Inadmissible observations inserted between the admissible ones: N_p does not count them, the same bits."""
    from miba.capi import ProblemArrays
    a, ra = base
    w = refpts.loop_problem(False)
    rng = np.random.default_rng(9)
    extra = rng.choice(w.n_obs, 40, replace=False)
    pos = np.sort(rng.choice(w.n_obs + 1, 40))
    bad_depth = np.where(rng.random(40) < 0.5, 0.0, -np.inf)
    q = ProblemArrays(w.cams.copy(), w.points.copy(), w.intr.copy(), w.intr_prior.copy(),
                      np.insert(w.obs_cam, pos, w.obs_cam[extra]), np.insert(w.obs_pt, pos, w.obs_pt[extra]),
                      np.insert(w.obs_uv, pos, w.obs_uv[extra] + 3.0, axis=0), np.insert(w.obs_depth, pos, bad_depth),
                      fixed_cam=-1)
    with solver() as s:
        r = s.refine_points(q)
    np.testing.assert_array_equal(q.points, a.points)
    np.testing.assert_array_equal(r["stats"], ra["stats"])


def test_no_side_effect_on_a_prepared_window():
    """prepare, refine_points (another window), solve_prepared: the bits of prepare, solve_prepared on a fresh context
    (deterministic = 1)."""
    w = refstep.window("bcr21")
    other = refpts.loop_problem(False)
    with solver(deterministic=1) as s:
        a = w.copy()
        s.prepare(a)
        sa = s.solve_prepared(a)
        la = s.iteration_log()
    with solver(deterministic=1) as s:
        b = w.copy()
        s.prepare(b)
        r = s.refine_points(other.copy(), log_pt=2)
        sb = s.solve_prepared(b)
        lb = s.iteration_log()
    assert r["n_solved"] == other.n_points
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(b, k), getattr(a, k))
    np.testing.assert_array_equal(lb, la)
    for k in ("final_cost", "initial_cost", "num_iterations", "num_successful_steps", "linear_solver", "camera_band"):
        assert sb[k] == sa[k], k


def test_errors():
    import ctypes as C

    from miba.capi import BaPtsInfo, BaPtsRequest
    from miba.solver import MibaError
    w = refpts.loop_problem(False)
    with solver() as s:
        for p in (w.n_points, w.n_points + 7):
            with pytest.raises(MibaError, match=r"\(-1\).*ba_refine_points.*log_pt"):
                s.refine_points(w.copy(), log_pt=p)
        bad = w.copy()
        bad.obs_pt[3] = w.n_points
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.refine_points(bad)
        bad = w.copy()
        bad.obs_cam[7] = -1
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.refine_points(bad)
        q = w.copy()
        ps = q.struct()
        # log_max_rows > 0 without a buffer
        req, info = BaPtsRequest(), BaPtsInfo()
        req.log_pt, req.log_max_rows = 1, 4
        assert s._L.ba_refine_points(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "log_rows" in s.last_error()
        # struct sizes below the minimum, through the C ABI
        for short_req in (True, False):
            req, info = BaPtsRequest(), BaPtsInfo()
            req.log_pt = -1
            if short_req:
                req.struct_size -= 8
            else:
                info.struct_size -= 8
            assert s._L.ba_refine_points(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
            assert "struct_size" in s.last_error()
        np.testing.assert_array_equal(q.points, w.points)
        # an info struct larger than the library's is legal: only the library's bytes are written
        class BigInfo(C.Structure):
            _fields_ = [("info", BaPtsInfo), ("tail", C.c_uint8 * 24)]
        big = BigInfo()
        big.info.struct_size = C.sizeof(BigInfo)
        for k in range(24):
            big.tail[k] = 0xA5
        req = BaPtsRequest()
        req.log_pt = -1
        assert s._L.ba_refine_points(s._h, C.byref(ps), C.byref(req), C.cast(C.pointer(big), C.POINTER(BaPtsInfo))) == 0
        assert big.info.struct_size == C.sizeof(BigInfo) and big.info.n_solved == w.n_points
        assert bytes(big.tail) == b"\xa5" * 24
        # log_pt named with no room for rows: nothing is written, the row count is still reported
        q = w.copy()
        ps = q.struct()
        req, info = BaPtsRequest(), BaPtsInfo()
        req.log_pt, req.log_max_rows = 2, 0
        assert s._L.ba_refine_points(s._h, C.byref(ps), C.byref(req), C.byref(info)) == 0
        assert info.log_rows >= 2
        r = s.refine_points(w.copy())  # the context still works
        assert r["n_solved"] == w.n_points
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.refine_points(w.copy())


def test_empty_window_and_empty_selection():
    import ctypes as C

    from miba.capi import BaPtsInfo, BaPtsRequest, ProblemArrays
    w = refpts.loop_problem(False)
    with solver() as s:
        q = w.copy()
        r = s.refine_points(q, points=[])
        assert (r["n_selected"], r["n_solved"], r["max_iterations"]) == (0, 0, 0)
        np.testing.assert_array_equal(q.points, w.points)
        assert np.all(r["stats"][:, 6] == -1)
        e = ProblemArrays(np.zeros((0, 7)), np.zeros((0, 3)), w.intr.copy(), w.intr.copy(), np.zeros(0, np.int32),
                          np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0), fixed_cam=-1)
        r = s.refine_points(e)
        assert (r["n_selected"], r["n_solved"]) == (0, 0)
        # a zeroed request (log_pt = 0) is legal on the empty window
        ps = e.struct()
        req, info = BaPtsRequest(), BaPtsInfo()
        assert s._L.ba_refine_points(s._h, C.byref(ps), C.byref(req), C.byref(info)) == 0 and info.log_rows == 0
        # cameras but no observation: nothing to solve
        e = ProblemArrays(w.cams.copy(), w.points.copy(), w.intr.copy(), w.intr.copy(), np.zeros(0, np.int32),
                          np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0), fixed_cam=-1)
        r = s.refine_points(e)
        assert (r["n_selected"], r["n_solved"]) == (w.n_points, 0)
        np.testing.assert_array_equal(e.points, w.points)


def test_pipeline_hook():
    """Keyframe 1's landmarks from the hook inside run_pipeline, from window.refine_landmarks called directly and from
    Solver.refine_points by hand on the same flattened frame are the same bits. (That run_pipeline without the hook
    writes what it wrote before is pinned on the CPU: test_pipeline_refine.py.)"""
    from miba import sequence, window
    kw = dict(n_keyframes=12, n_landmarks=400, seed=2)
    with solver(deterministic=1) as s:
        refine = lambda prob: s.refine_points(prob, min_obs=2)  # noqa: E731
        kfs, lms, K0, gt = sequence.make_tum_sequence(**kw)
        frame = window.refine_frame(1, kfs, lms, K0)
        assert frame is not None and frame.n_points > 20 and frame.n_cams == 2
        start = frame.points.copy()
        r = refine(frame)
        solved = r["stats"][:, 6] >= 0
        assert r["n_solved"] == solved.sum() > 20 and r["n_failure"] == 0
        assert np.any(frame.points[solved] != start[solved])
        np.testing.assert_array_equal(frame.points[~solved], start[~solved])
        # refine_landmarks writes the solved landmarks back, and only those
        lms0 = {k: v.copy() for k, v in lms.items()}
        poses = [kf.T_w_c.copy() for kf in kfs]
        out = window.refine_landmarks(1, kfs, lms, K0, refine)
        assert out["n_solved"] == r["n_solved"]
        ids = frame.meta["landmark_ids"]
        for q, lid in enumerate(ids):
            np.testing.assert_array_equal(lms[lid], frame.points[q] if solved[q] else lms0[lid])
        for lid in set(lms0) - set(ids):
            np.testing.assert_array_equal(lms[lid], lms0[lid])
        for k, kf in enumerate(kfs):
            np.testing.assert_array_equal(kf.T_w_c, poses[k])
        assert window.refine_landmarks(0, kfs, lms, K0, refine) is None
        # the hook in the loop
        kfs3, lms3, K0, gt = sequence.make_tum_sequence(**kw)
        seen = []

        def hook(prob):
            out = refine(prob)
            seen.append(prob.points.copy())
            return out

        sequence.run_pipeline(kfs3, lms3, K0, gt, s.solve, frame_frequency=4, window_size=4, refine_points=hook)
        assert len(seen) == 11  # never the first keyframe: it shares no landmark with an earlier one
        np.testing.assert_array_equal(seen[0], frame.points)
