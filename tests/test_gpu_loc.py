"""ba_localize on the GPU against tests/refloc.py (test_refloc.py checks the references and that the frames used here
qualify).

* the first step (max_num_iterations = 1, from the generator's perturbed poses) against refcand.retract_quat(x, the
  longdouble step), within refcand's retraction bound plus the step bound F cond eps |step|_inf, F = refloc.STEP_F,
  at three radii and at the workgroup's observation-count boundaries; once more with Huber parameters that put blocks
  of both kinds in both zones;
* the whole loop on frames whose accept / reject sequence is settled (the f64 and longdouble references agree and no
  decision is closer than 1e-3 to its threshold): the sequence, the counters, the termination, the final cost and the
  final pose;
* batch independence and bits, the mask, cameras without observations, inadmissible observations;
* no side effect on a prepared window; the errors; the pipeline hook."""
import numpy as np
import pytest

import refcand
import refloc
import refstep
from oracle import oracle
from refstep import EPS64, NO_TOL

pytestmark = pytest.mark.gpu


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def _step_refs(okw_key):
    """The longdouble first steps of every step frame at every radius (cached, shared)."""
    def make():
        p = refloc.step_frames()
        out = {}
        for radius in refloc.STEP_RADII:
            o = oracle.default_options(**dict(okw_key))
            for c in range(p.n_cams):
                out[c, radius] = refloc.step(refloc.linearize(p, c, o), o, radius)
        return out
    return refloc.cached(("gpu_step_refs", okw_key), make)


def _check_first_step(radius, okw, frames):
    p = refloc.step_frames()
    refs = _step_refs(tuple(sorted(okw.items())))
    q = p.copy()
    with solver(max_num_iterations=1, initial_trust_region_radius=radius, **NO_TOL, **okw) as s:
        r = s.localize(q)
    assert r["n_selected"] == r["n_solved"] == p.n_cams and r["max_iterations"] == 1
    for c in frames:
        ref = refs[c, radius]
        st = r["stats"][c]
        n = refloc.STEP_COUNTS[c]
        eq, et = refcand.retraction_error(q.cams[c], p.cams[c], ref["delta_ld"])
        bq, bt = refcand.retraction_bound(p.cams[c], ref["delta"])
        sb = refloc.step_bound(ref)
        print(f"FIRST n={n} radius={radius:g} cond={ref['cond']:.3g} |step|={np.abs(ref['delta']).max():.2e} "
              f"err q={eq:.2e} t={et:.2e} bound q={bq + sb:.2e} t={bt + sb:.2e} stats={st[3:].tolist()}")
        assert st[0] == n and st[3] == 1
        assert (st[4], st[5], st[6], st[7]) == (2, 0, 1, refloc.MSG_MAX_ITER), st  # the step was accepted
        assert eq <= bq + sb and et <= bt + sb, (n, radius, eq, et, bq, bt, sb)
        lin = refloc.linearize(p, c, oracle.default_options(**okw))
        assert abs(st[1] - lin["cost"]) <= 1e-6 * lin["cost"]
    return r


@pytest.mark.parametrize("radius", refloc.STEP_RADII)
def test_first_step(radius):
    _check_first_step(radius, {}, range(len(refloc.STEP_COUNTS)))


def test_first_step_huber_zones():
    _check_first_step(1e4, refloc.HUBER_MIXED, [refloc.HUBER_FRAME])


def _check_loop(hard, c):
    p = refloc.loop_problem(hard)
    a, b = refloc.loop_refs(hard, c)
    q = p.copy()
    with solver() as s:
        r = s.localize(q, cams=[c], log_cam=c)
    st, log = r["stats"][c], r["log"]
    spread = float(np.abs(a["pose"] - b["pose"]).max())
    tol = 16 * max(spread, 64 * EPS64 * max(1.0, float(np.abs(b["pose"][4:]).max())))
    err = float(np.abs(q.cams[c] - b["pose"]).max())
    rel = abs(st[2] - b["final_cost"]) / b["final_cost"]
    print(f"LOOP hard={hard} c={c} iters={int(st[3])}/{b['iterations']} rej={b['accept'].count(0)} "
          f"cost rel={rel:.2e} pose err={err:.2e} tol={tol:.2e} spread={spread:.2e}")
    assert r["log_rows"] == b["iterations"] + 1 == len(log)
    assert log[1:, 6].astype(int).tolist() == b["accept"]
    assert (st[3], st[4], st[5], st[6], st[7]) == (b["iterations"], b["n_succ"], b["n_unsucc"], b["termination"], b["msg"])
    assert rel <= 1e-6
    assert abs(st[1] - b["initial_cost"]) <= 1e-6 * b["initial_cost"]
    assert err <= tol
    # the log's own consistency: row 0 and the last accepted cost
    assert log[0, 0] == st[1] and log[0, 6] == 1 and np.all(log[:, 7] == 0)
    assert st[2] <= st[1]
    others = np.arange(p.n_cams) != c
    np.testing.assert_array_equal(q.cams[others], p.cams[others])
    assert np.all(r["stats"][others, 6] == -1)


@pytest.mark.parametrize("c", range(12))
def test_loop_all_steps_accepted(c):
    _check_loop(False, c)


@pytest.mark.parametrize("c", refloc.LOOP_HARD_FRAMES)
def test_loop_with_rejections(c):
    _check_loop(True, c)


def _tile(p, times):
    """The window repeated: camera c + k n_cams is camera c again, on the same points."""
    from miba.capi import ProblemArrays
    nc = p.n_cams
    return ProblemArrays(np.tile(p.cams, (times, 1)), p.points.copy(), p.intr.copy(), p.intr_prior.copy(),
                         np.concatenate([p.obs_cam + k * nc for k in range(times)]), np.tile(p.obs_pt, times),
                         np.tile(p.obs_uv, (times, 1)), np.tile(p.obs_depth, times), fixed_cam=-1)


def test_batch_independence_and_bits():
    p = refloc.loop_problem(False)
    nc = p.n_cams
    with solver() as s:
        a = p.copy()
        ra = s.localize(a)
        b = p.copy()
        rb = s.localize(b)
        np.testing.assert_array_equal(b.cams, a.cams)  # two calls, the same bits
        np.testing.assert_array_equal(rb["stats"], ra["stats"])
        assert ra["n_solved"] == nc and np.all(ra["stats"][:, 6] == 0)
        assert not np.array_equal(a.cams, p.cams)
        for c in (0, 5, 11):  # alone
            q = p.copy()
            rq = s.localize(q, cams=[c])
            np.testing.assert_array_equal(q.cams[c], a.cams[c])
            np.testing.assert_array_equal(rq["stats"][c], ra["stats"][c])
        big = _tile(p, 25)  # 300 workgroups, more than the device has compute units
        rbig = s.localize(big)
        assert rbig["n_solved"] == 300
        np.testing.assert_array_equal(big.cams, np.tile(a.cams, (25, 1)))
        np.testing.assert_array_equal(rbig["stats"], np.tile(ra["stats"], (25, 1)))
        # under a mask everything else is untouched, bitwise
        q = p.copy()
        mask = np.arange(nc) % 3 == 1
        rq = s.localize(q, cams=mask)
        assert rq["n_selected"] == rq["n_solved"] == int(mask.sum())
        np.testing.assert_array_equal(q.cams[mask], a.cams[mask])
        np.testing.assert_array_equal(q.cams[~mask], p.cams[~mask])
        for k in ("points", "intr", "intr_prior", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
            np.testing.assert_array_equal(getattr(q, k), getattr(p, k))
        assert np.all(rq["stats"][~mask, 6] == -1) and np.all(rq["stats"][~mask, :6] == 0)


def test_camera_without_observations_and_inadmissible_observations():
    p = refloc.loop_problem(False)
    with solver() as s:
        a = p.copy()
        ra = s.localize(a)
        # camera 5 loses every admissible observation: untouched, [6] = -1, the others as before
        q = p.copy()
        q.obs_depth[q.obs_cam == 5] = 0.0
        rq = s.localize(q)
        keep = np.arange(p.n_cams) != 5
        np.testing.assert_array_equal(q.cams[5], p.cams[5])
        assert rq["stats"][5].tolist() == [0, 0, 0, 0, 0, 0, -1, 0]
        assert rq["n_selected"] == p.n_cams and rq["n_solved"] == p.n_cams - 1
        np.testing.assert_array_equal(q.cams[keep], a.cams[keep])
        np.testing.assert_array_equal(rq["stats"][keep], ra["stats"][keep])
        # inadmissible observations added in between: N_c does not count them, the result is the same bits
        from miba.capi import ProblemArrays
        rng = np.random.default_rng(9)
        extra = rng.choice(p.n_obs, 40, replace=False)
        pos = np.sort(rng.choice(p.n_obs + 1, 40))
        bad_depth = np.where(rng.random(40) < 0.5, 0.0, -np.inf)
        w = ProblemArrays(p.cams.copy(), p.points.copy(), p.intr.copy(), p.intr_prior.copy(),
                          np.insert(p.obs_cam, pos, p.obs_cam[extra]), np.insert(p.obs_pt, pos, p.obs_pt[extra]),
                          np.insert(p.obs_uv, pos, p.obs_uv[extra] + 3.0, axis=0), np.insert(p.obs_depth, pos, bad_depth),
                          fixed_cam=-1)
        rw = s.localize(w)
        np.testing.assert_array_equal(w.cams, a.cams)
        np.testing.assert_array_equal(rw["stats"], ra["stats"])


def test_no_side_effect_on_a_prepared_window():
    """prepare, localize (another window), solve_prepared: the bits of prepare, solve_prepared on a fresh context
    (deterministic = 1)."""
    p = refstep.window("bcr21")
    other = refloc.loop_problem(False)
    with solver(deterministic=1) as s:
        a = p.copy()
        s.prepare(a)
        sa = s.solve_prepared(a)
        la = s.iteration_log()
    with solver(deterministic=1) as s:
        b = p.copy()
        s.prepare(b)
        r = s.localize(other.copy(), log_cam=2)
        sb = s.solve_prepared(b)
        lb = s.iteration_log()
    assert r["n_solved"] == other.n_cams
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(b, k), getattr(a, k))
    np.testing.assert_array_equal(lb, la)
    for k in ("final_cost", "initial_cost", "num_iterations", "num_successful_steps", "linear_solver", "camera_band"):
        assert sb[k] == sa[k], k


def test_errors():
    import ctypes as C

    from miba.capi import BaLocInfo, BaLocRequest
    from miba.solver import MibaError
    p = refloc.loop_problem(False)
    with solver() as s:
        for c in (p.n_cams, p.n_cams + 7):
            with pytest.raises(MibaError, match=r"\(-1\).*ba_localize.*log_cam"):
                s.localize(p.copy(), log_cam=c)
        bad = p.copy()
        bad.obs_pt[3] = p.n_points
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.localize(bad)
        bad = p.copy()
        bad.obs_cam[7] = -1
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.localize(bad)
        # struct sizes below the minimum, through the C ABI
        q = p.copy()
        ps = q.struct()
        for short_req in (True, False):
            req, info = BaLocRequest(), BaLocInfo()
            req.log_cam = -1
            if short_req:
                req.struct_size -= 8
            else:
                info.struct_size -= 8
            assert s._L.ba_localize(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
            assert "struct_size" in s.last_error()
        np.testing.assert_array_equal(q.cams, p.cams)
        # an info struct larger than the library's is legal: only the library's bytes are written
        class BigInfo(C.Structure):
            _fields_ = [("info", BaLocInfo), ("tail", C.c_uint8 * 24)]
        big = BigInfo()
        big.info.struct_size = C.sizeof(BigInfo)
        for k in range(24):
            big.tail[k] = 0xA5
        req = BaLocRequest()
        req.log_cam = -1
        assert s._L.ba_localize(s._h, C.byref(ps), C.byref(req), C.cast(C.pointer(big), C.POINTER(BaLocInfo))) == 0
        assert big.info.struct_size == C.sizeof(BigInfo) and big.info.n_solved == p.n_cams
        assert bytes(big.tail) == b"\xa5" * 24
        # log_cam named with no room for rows: nothing is written, the row count is still reported
        q = p.copy()
        ps = q.struct()
        req, info = BaLocRequest(), BaLocInfo()
        req.log_cam, req.log_max_rows = 2, 0
        assert s._L.ba_localize(s._h, C.byref(ps), C.byref(req), C.byref(info)) == 0
        assert info.log_rows >= 2
        r = s.localize(p.copy())  # the context still works
        assert r["n_solved"] == p.n_cams
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.localize(p.copy())


def test_evaluation_failure_at_the_given_pose():
    """A pose that is not finite: BA_FAILURE with the evaluation-failed message, the pose kept, no log row; the
    other cameras as without it."""
    p = refloc.loop_problem(False)
    with solver() as s:
        a = p.copy()
        ra = s.localize(a)
        q = p.copy()
        q.cams[3, 5] = np.nan
        given = q.cams[3].copy()
        r = s.localize(q, log_cam=3)
        st = r["stats"][3]
        assert (st[3], st[6], st[7]) == (0, 2, refloc.MSG_EVAL_FAIL) and np.isnan(st[1]) and np.isnan(st[2])
        assert r["log_rows"] == 0 and len(r["log"]) == 0 and r["n_failure"] == 1
        np.testing.assert_array_equal(q.cams[3], given)
        keep = np.arange(p.n_cams) != 3
        np.testing.assert_array_equal(q.cams[keep], a.cams[keep])
        np.testing.assert_array_equal(r["stats"][keep], ra["stats"][keep])


def test_empty_window_and_empty_selection():
    from miba.capi import ProblemArrays
    p = refloc.loop_problem(False)
    with solver() as s:
        q = p.copy()
        r = s.localize(q, cams=[])
        assert (r["n_selected"], r["n_solved"], r["max_iterations"]) == (0, 0, 0)
        np.testing.assert_array_equal(q.cams, p.cams)
        e = ProblemArrays(np.zeros((0, 7)), np.zeros((0, 3)), p.intr.copy(), p.intr.copy(), np.zeros(0, np.int32),
                          np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(0), fixed_cam=-1)
        r = s.localize(e)
        assert (r["n_selected"], r["n_solved"]) == (0, 0)


def test_pipeline_hook():
    """keyframe 1's pose from the hook inside run_pipeline, from window.localize_keyframe called directly and from
    Solver.localize by hand on the same flattened frame are the same bits. (That run_pipeline without the hook writes
    what it wrote before is pinned on the CPU, against a recorded trajectory: test_pipeline_localize.py.)"""
    from miba import sequence, window
    kw = dict(n_keyframes=12, n_landmarks=400, seed=2)
    with solver(deterministic=1) as s:
        kfs, lms, K0, gt = sequence.make_tum_sequence(**kw)
        frame = window.localize_frame(1, kfs, lms, K0)
        assert frame is not None and frame.n_obs > 20
        start = frame.cams[0].copy()
        r = s.localize(frame)
        assert r["n_solved"] == 1 and r["stats"][0, 6] == 0 and not np.array_equal(frame.cams[0], start)
        # localize_keyframe writes the pose back into the keyframe, and only there
        others = [kf.T_w_c.copy() for kf in kfs]
        out = window.localize_keyframe(1, kfs, lms, K0, s.localize)
        assert out["n_solved"] == 1
        np.testing.assert_array_equal(kfs[1].T_w_c, frame.cams[0])
        for k, kf in enumerate(kfs):
            if k != 1:
                np.testing.assert_array_equal(kf.T_w_c, others[k])
        assert window.localize_keyframe(0, kfs, lms, K0, s.localize) is None
        # the hook in the loop
        kfs3, lms3, K0, gt = sequence.make_tum_sequence(**kw)
        seen = []

        def hook(prob):
            out = s.localize(prob)
            seen.append(prob.cams[0].copy())
            return out

        sequence.run_pipeline(kfs3, lms3, K0, gt, s.solve, frame_frequency=4, window_size=4, localize=hook)
        assert len(seen) == 11  # never the first keyframe: it shares no landmark with an earlier one
        np.testing.assert_array_equal(seen[0], frame.cams[0])
