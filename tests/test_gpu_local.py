"""ba_local_window and ba_solve_local on the GPU.

Selection: every integer of ``Solver.local_window`` is compared exactly with tests/reflocal.py (sets and sorted lists
over the observation arrays). The maps (reflocal.make_map: repeated and inadmissible observations throughout) sit on
the kernels' boundaries: n_points 1, 63, 64, 65, 129 (the 64-bit words of a bit row) and 16385 (the 257th word: the
second workgroup of the scan over the words' popcounts, LOCAL_TPB = 256 words each); n_cams 1, 2, 15, 16, 17, 33 (the
tile of 16 of the co-visibility kernels; here one workgroup per camera); n_obs 0, 1, 255, 256, 257 (LOCAL_TPB = 256
observations per scanning workgroup) and 65537 = LOCAL_TPB^2 + 1 (the second round of the carry over the workgroups'
sums).

ba_solve_local on a two-sweep scene (refsweep's generator at 40 cameras, below G2's 50): bitwise against the same
done by hand on a fresh context (reflocal's sub-window, set_constant_cameras, solve, scatter back), deterministic = 1.
"""
import numpy as np
import pytest

import reflocal

pytestmark = pytest.mark.gpu


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def check(s, p, center, mask=None, **kw):
    got = s.local_window(p, center, **kw)
    ref = reflocal.select(p, center, mask=mask, **kw)
    reflocal.assert_same(got, ref, f"center={center} {kw}")
    return got


# (n_cams, n_points, n_obs)
SIZES = [(9, p, 300) for p in (1, 63, 64, 65, 129)] + [(c, 100, 400) for c in (1, 2, 15, 16, 17, 33)] + \
        [(9, 100, o) for o in (0, 1, 255, 256, 257)] + [(12, 16385, 3000), (33, 700, 65537)]


@pytest.mark.parametrize("nc,npt,no", SIZES)
def test_selection_on_the_kernels_boundaries(nc, npt, no):
    p = reflocal.make_map(nc, npt, no, seed=1000 + nc + npt + no, fixed_cam=min(1, nc - 1))
    with solver() as s:
        for center in sorted({0, nc // 2, nc - 1}):
            a = check(s, p, center, min_weight=1, max_local=0)
            b = check(s, p, center, min_weight=1, max_local=0)  # reproducible
            for k in reflocal.INT_KEYS:
                np.testing.assert_array_equal(a[k], b[k])
            check(s, p, center, min_weight=3, max_local=4)
        check(s, p, 0, min_weight=0, max_local=-1)  # <= 0: weight 1, no cap


def test_selection_contents():
    nc = 17
    p = reflocal.make_map(nc, 300, 2500, seed=5, span=5, fixed_cam=-1)
    # a camera and a point seen only through inadmissible observations; a centre without observations
    p.obs_depth[p.obs_cam == 6] = 0.0
    p.obs_depth[p.obs_pt == 11] = -np.inf
    p.obs_depth[p.obs_cam == 13] = 0.0
    with solver() as s:
        ref = check(s, p, 8, min_weight=1)
        assert ref["w"][6] == 0 and 6 not in ref["cam_index"] and 11 not in ref["pt_index"]
        e = check(s, p, 13, min_weight=1)  # the centre without an admissible observation
        assert (e["n_local"], e["n_fixed"], e["n_points"], e["n_obs"], e["sub_fixed_cam"]) == (1, 0, 0, 0, 0)
        top = int(ref["w"].max())
        lone = check(s, p, 8, min_weight=top + 1)  # above every weight: L = {centre}
        assert lone["n_local"] == 1 and lone["n_fixed"] > 0 and lone["sub_fixed_cam"] == -1
        one = check(s, p, 8, min_weight=1, max_local=1)
        assert one["n_local"] == 1
        two = check(s, p, 8, min_weight=1, max_local=2)
        assert two["n_local"] == 2
        for cap in range(3, 8):  # every cut through the ranking
            check(s, p, 8, min_weight=1, max_local=cap)
        check(s, p, 8, min_weight=1, max_local=0)
        # fixed_cam in L, in F and outside the window
        Lc = two["cam_index"][two["cam_local"]]
        Fc = two["cam_index"][~two["cam_local"]]
        outside = [a for a in range(nc) if a not in two["cam_index"]]
        for g in (int(Lc[0]), int(Fc[0]), int(outside[0])):
            p.fixed_cam = g
            r = check(s, p, 8, min_weight=1, max_local=2)
            if g == int(Lc[0]):
                assert r["cam_constant"][list(r["cam_index"]).index(g)]
        p.fixed_cam = -1
        # a context mask that intersects L
        mask = np.zeros(nc, bool)
        mask[[int(Lc[-1]), int(outside[0])]] = True
        s.set_constant_cameras(mask)
        r = check(s, p, 8, mask=mask, min_weight=1, max_local=2)
        assert r["cam_constant"][list(r["cam_index"]).index(int(Lc[-1]))] and r["sub_fixed_cam"] == -1
        # a mask set for another n_cams does not apply
        s.set_constant_cameras(np.ones(nc + 1, bool))
        check(s, p, 8, mask=None, min_weight=1, max_local=2)


def test_f_empty_and_a_tie_at_the_cut():
    p = reflocal.from_lists(5, 5, [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 2), (2, 3), (3, 0), (4, 4)])
    with solver() as s:
        r = check(s, p, 0, min_weight=1)
        assert r["n_local"] == 4 and r["n_fixed"] == 0 and r["sub_fixed_cam"] == 0 and not r["cam_constant"].any()
        assert r["cam_index"].tolist() == [0, 1, 2, 3]
        # a cut that falls on a tie: cameras 1 and 2 share two points with camera 0 each, the lower index stays
        t = check(s, p, 0, min_weight=1, max_local=2)
        assert t["w"].tolist() == [4, 2, 2, 1, 0] and t["cam_index"][t["cam_local"]].tolist() == [0, 1]
        assert t["cam_index"][~t["cam_local"]].tolist() == [2, 3] and t["sub_fixed_cam"] == -1


def test_stand_alone():
    """prepare, local_window (of another map and of the window itself), solve_prepared: the bits of prepare,
    solve_prepared on a context that never made the call (deterministic = 1)."""
    import refstep
    p = refstep.window("bcr21")
    other = reflocal.make_map(33, 700, 5000, seed=9)
    with solver(deterministic=1) as s:
        a = p.copy()
        s.prepare(a)
        sa = s.solve_prepared(a)
        la = s.iteration_log()
    with solver(deterministic=1) as s:
        b = p.copy()
        s.prepare(b)
        check(s, other, 16, min_weight=2, max_local=6)
        check(s, b, 10, min_weight=15)
        sb = s.solve_prepared(b)
        lb = s.iteration_log()
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(b, k), getattr(a, k))
    np.testing.assert_array_equal(lb, la)
    for k in ("final_cost", "initial_cost", "num_iterations", "num_successful_steps", "linear_solver", "camera_band"):
        assert sa[k] == sb[k], k


def test_errors():
    from miba.solver import MibaError
    p = reflocal.make_map(9, 100, 300, seed=2)
    with solver() as s:
        for c in (-1, 9):
            with pytest.raises(MibaError, match=r"\(-1\).*ba_local_window.*center"):
                s.local_window(p, c)
            with pytest.raises(MibaError, match=r"\(-1\).*ba_solve_local.*center"):
                s.solve_local(p, c)
        bad = p.copy()
        bad.obs_cam[3] = 9
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.local_window(bad, 0)
        check(s, p, 0, min_weight=1)  # the context still works
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.local_window(p, 0)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.solve_local(p, 0)


# ------------------------------------------------------------------------------------------------------- solve_local
N_SWEEP = 40  # two sweeps of 20 keyframes


def sweep_map():
    from miba import synthetic
    return synthetic.make_sweep_problem(N_SWEEP, 12 * N_SWEEP, 5, 2, seed=77, sensor_f32=True)


def test_solve_local_is_the_sub_window_solved_by_hand():
    base = sweep_map()
    center = N_SWEEP - 3  # a keyframe of the second sweep
    kw = dict(min_weight=15, max_local=8)
    own = np.zeros(N_SWEEP, bool)
    own[[center - 1, 3]] = True  # the context's own constant set: one camera inside L, one elsewhere
    p = base.copy()
    with solver(deterministic=1) as s:
        s.set_constant_cameras(own)
        sm = s.solve_local(p, center, **kw)
        first = s.last_prepare()["plan_reused"]
        win = sm["window"]
        q = base.copy()
        s.solve_local(q, center, **kw)  # a repeat of the same selection reuses the plan
        assert first == 0 and s.last_prepare()["plan_reused"] == 1
        # the context's own mask is still in force: a plain solve of the whole map keeps those cameras
        r = base.copy()
        sr = s.solve(r)
        np.testing.assert_array_equal(r.cams[own], base.cams[own])
        assert sr["num_active_cams"] == N_SWEEP - 1 - 2
    sel = reflocal.select(base, center, mask=own, **kw)
    reflocal.assert_same(win, sel, "solve_local's selection")
    L = sel["cam_index"][sel["cam_local"]]
    # the purpose: the window around a second-sweep keyframe holds keyframes of the first sweep; the last-k window
    # of the same size holds none
    assert (L < N_SWEEP // 2).any() and (L >= N_SWEEP // 2).any()
    assert not (np.arange(N_SWEEP - len(L), N_SWEEP) < N_SWEEP // 2).any()
    assert sel["n_fixed"] > 0 and sel["cam_constant"][list(sel["cam_index"]).index(center - 1)]
    # outside the window, and the constant cameras: bitwise unchanged
    const_cams = sel["cam_index"][sel["cam_constant"]]
    free = np.setdiff1d(L, const_cams)
    untouched = np.setdiff1d(np.arange(N_SWEEP), free)
    np.testing.assert_array_equal(p.cams[untouched], base.cams[untouched])
    outP = np.setdiff1d(np.arange(base.n_points), sel["pt_index"])
    assert len(outP) > 0
    np.testing.assert_array_equal(p.points[outP], base.points[outP])
    assert (np.abs(p.cams[free] - base.cams[free]).max(1) > 0).all()
    assert sm["num_active_cams"] == len(free) and sm["num_obs_admissible"] == sel["n_obs"]
    # inside: what a fresh context gives when it does the same by hand
    h = base.copy()
    sub = reflocal.sub_problem(h, sel)
    with solver(deterministic=1) as s:
        s.set_constant_cameras(sel["cam_constant"])
        sh = s.solve(sub)
    reflocal.scatter_back(h, sel, sub)
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(p, k), getattr(h, k), err_msg=k)
        np.testing.assert_array_equal(getattr(q, k), getattr(h, k), err_msg=k)
    for k in ("final_cost", "initial_cost", "num_iterations", "linear_solver", "camera_band"):
        assert sm[k] == sh[k], k
    assert sm["termination"] == "CONVERGENCE"


def test_solve_local_of_an_empty_sub_window():
    base = sweep_map()
    base.obs_depth[base.obs_cam == 7] = 0.0
    base.intr[:] = base.intr_prior + np.array([4.0, -3.0, 2.0, -1.0])
    p = base.copy()
    with solver() as s:
        sm = s.solve_local(p, 7)
    assert sm["window"]["n_obs"] == 0 and sm["window"]["sub_fixed_cam"] == 0
    assert sm["num_obs_admissible"] == 0 and sm["num_active_cams"] == 0 and sm["reduced_system_size"] == 4
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(p, k), getattr(base, k))


def test_pipeline_with_the_local_schedule():
    """sequence.run_pipeline(solve_local=...): whenever the schedule fires, the map so far is solved locally around
    its newest keyframe; without the switch the pipeline is the last-k schedule as before."""
    from miba import sequence

    def run(local):
        kfs, lms, K0, gt = sequence.make_tum_sequence(seed=0, n_keyframes=24, n_landmarks=600)
        with solver(deterministic=1) as s:
            kw = dict(solve_local=s.solve_local, min_weight=15, max_local=6) if local else {}
            txt, summ, K = sequence.run_pipeline(kfs, lms, K0, gt, s.solve, frame_frequency=10, window_size=10, **kw)
        return txt, summ, K

    txt_a, summ_a, _ = run(False)
    txt_b, summ_b, _ = run(True)
    assert len(summ_a) == len(summ_b) >= 2 and all("window" not in sm for _, _, sm in summ_a)
    for (a0, b0, _), (a1, b1, sm) in zip(summ_a, summ_b):
        assert (a0, b0) == (a1, b1)
        win = sm["window"]
        L = win["cam_index"][win["cam_local"]]
        assert b1 in L and 1 <= win["n_local"] <= 6 and sm["num_obs_admissible"] == win["n_obs"] > 0
        assert sm["final_cost"] < sm["initial_cost"]
    assert txt_a != txt_b and len(txt_a.splitlines()) == len(txt_b.splitlines())
