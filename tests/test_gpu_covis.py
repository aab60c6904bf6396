"""ba_covisibility and ba_solve_ordered (Solver.covisibility, Solver.solve(order=...)) against tests/reforder.py.

Everything ba_covisibility reports is an integer and is compared exactly: the weights against B B^T of the admissible
observations' incidence matrix, the order against the restated reverse Cuthill-McKee, the bands against
refstep.camera_band of the window as given and permuted, the overflow counts against reforder.wide.

The ordered solve is checked on the two sweep windows of the wide-window tests (camera band 14 / 25 as given, every point
an overflow point): in the computed order they are band-7 / band-9 windows on the block cyclic reduction without a
single overflow launch; the final cost meets the oracle's solve of the window AS GIVEN to 1e-6 relative (the project's
parity rule); the oracle's cost at the returned parameters, in the caller's numbering, is the reported final cost to
1e-9 relative (the cancellation in projected - measured pixel amplifies eps_f64 by |pixel| / |residual| <= about 1e3,
so 1e-13 is expected; a camera handed back at the wrong index moves the cost by orders of magnitude). Bitwise
comparisons run with deterministic = 1, the only mode that promises repeatable bits (the default mode sums the Schur
tiles with float atomics).

The LM step of the permuted windows against refstep.schur_step on the caller's numbering, at test_gpu_step.py's bound
8 cond(S) eps_f64.

Measured (MI355X): ordered sweep22 / sweep42 final cost against the oracle 2.6e-15 / 6.5e-16 relative with the oracle's
iteration counts (20 / 18), the oracle's cost at the returned parameters 1.1e-15 / 1.7e-15; the ordered step's largest
group error 7.6e-13 / 1.6e-12 (the intrinsics) against tol 2.5e-9 / 2.3e-9.
"""
import ctypes as C

import numpy as np
import pytest

import reforder
import refstep
import refsweep
from refstep import NO_TOL

pytestmark = pytest.mark.gpu

BCR, DENSE, BLOCKED = 2, 0, 3
INFO = ("n_active", "n_edges", "n_components", "band_before", "band_after", "wide_before", "wide_after", "order_changed")


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def unchanged(q, p):
    for a in ("cams", "points", "intr", "intr_prior", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"prob.{a} was modified")
    assert q.fixed_cam == p.fixed_cam


def check_report(got, p, ref):
    W = got["weights"]
    assert W.dtype == np.int32 and W.shape == (p.n_cams, p.n_cams)
    np.testing.assert_array_equal(W, ref["weights"])
    np.testing.assert_array_equal(W, W.T)
    adm = p.obs_depth > 1e-15
    for c in range(p.n_cams):
        assert W[c, c] == len(np.unique(p.obs_pt[adm & (p.obs_cam == c)]))
    for k in INFO:
        assert got[k] == ref[k], (k, got[k], ref[k])
    np.testing.assert_array_equal(got["order"], ref["order"])
    assert sorted(got["order"].tolist()) == list(range(p.n_cams))
    assert got["time_count_ms"] >= 0 and got["time_total_ms"] >= got["time_order_ms"] >= 0


def run_report(p, key=None):
    ref = reforder.ordering(p, key=key)
    q = p.copy()
    with solver() as s:
        got = s.covisibility(q)
    unchanged(q, p)
    check_report(got, p, ref)
    return got, ref


# --------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("n_points", [1, 63, 64, 65])
@pytest.mark.parametrize("n_cams", [1, 15, 16, 17, 33])
def test_weights(n_cams, n_points):
    """Camera counts around the 16-camera tile (one tile, a ragged second one, three) and point counts around the
    64-bit word; duplicated observations, bad depths, a shuffled order."""
    from miba import synthetic
    p = synthetic.make_problem(n_cams, n_points, obs_per_point=(2, 4), seed=100 * n_cams + n_points, dup_frac=0.1,
                               bad_depth_frac=0.1, shuffle_obs=True)
    run_report(p)


def test_weights_across_slices():
    """One word past a whole slice of a camera's row: two slices summed into W, the last one a single word."""
    from miba import synthetic
    n_points = 64 * reforder.COVIS_SLICE_WORDS + 1
    p = synthetic.make_problem(20, n_points, obs_per_point=2, seed=7, dup_frac=0.1, bad_depth_frac=0.1,
                               shuffle_obs=True)
    assert -(-n_points // 64) == reforder.COVIS_SLICE_WORDS + 1
    got, _ = run_report(p)
    # the last word's only point counts: the reference without it differs
    adm = (p.obs_depth > 1e-15) & (p.obs_pt == n_points - 1)
    assert adm.any() and got["weights"][p.obs_cam[adm][0], p.obs_cam[adm][0]] > 0


def test_weights_edge_cameras():
    """A camera without any observation, a camera whose depths are all zero, the gauge camera in the middle."""
    from miba import synthetic
    p = synthetic.make_problem(17, 65, obs_per_point=(2, 4), seed=3, fixed_cam=8, dup_frac=0.1, bad_depth_frac=0.1,
                               shuffle_obs=True)
    keep = p.obs_cam != 5
    p.obs_cam, p.obs_pt = p.obs_cam[keep].copy(), p.obs_pt[keep].copy()
    p.obs_uv, p.obs_depth = p.obs_uv[keep].copy(), p.obs_depth[keep].copy()
    p.obs_depth[p.obs_cam == 11] = 0.0
    got, _ = run_report(p)
    W = got["weights"]
    assert not W[5].any() and not W[11].any() and W[8, 8] > 0 and W[8].sum() > W[8, 8]
    assert got["n_active"] == 14


def test_no_admissible_observation():
    from miba import synthetic
    p = synthetic.make_problem(6, 40, obs_per_point=2, seed=1)
    p.obs_depth[:] = 0.0
    got, _ = run_report(p)
    assert not got["weights"].any() and np.array_equal(got["order"], np.arange(6))
    assert got["n_active"] == 0 and got["order_changed"] == 0


# ----------------------------------------------------------------------------------------------------------- order
ORDER_WINDOWS = ["sweep22", "sweep42", "sweep42_gauge17", "sweep50_relabelled", "two_scenes", "dense_wide30",
                 "gauge_mid21", "inactive_mid21"]


@pytest.mark.parametrize("name", ORDER_WINDOWS)
def test_order(name):
    p = reforder.window(name)
    got, ref = run_report(p, key=name)
    if name in reforder.TABLE:
        assert tuple(got[k] for k in ("band_before", "band_after", "wide_before", "wide_after", "order_changed")) == \
            reforder.TABLE[name]
    if name == "two_scenes":
        assert (got["n_components"], got["band_before"], got["band_after"]) == (2, 4, 2)
    if name == "dense_wide30":
        assert got["order_changed"] == 0 and np.array_equal(got["order"], np.arange(p.n_cams))


def test_optional_outputs_and_repeat():
    """Two calls give the same bits; outputs that are not asked for change nothing in the others."""
    p = reforder.window("sweep42")
    with solver() as s:
        a = s.covisibility(p.copy())
        b = s.covisibility(p.copy())
        c = s.covisibility(p.copy(), weights=False)
        d = s.covisibility(p.copy(), order=False)
        e = s.covisibility(p.copy(), weights=False, order=False)
    np.testing.assert_array_equal(a["weights"], b["weights"])
    np.testing.assert_array_equal(a["order"], b["order"])
    assert "weights" not in c and "order" not in d and "weights" not in e and "order" not in e
    np.testing.assert_array_equal(c["order"], a["order"])
    np.testing.assert_array_equal(d["weights"], a["weights"])
    for k in INFO:
        assert a[k] == b[k] == c[k] == d[k] == e[k], k


# ---------------------------------------------------------------------------------------------------- ordered solve
_oracle = {}


def oracle_solve(name):
    if name not in _oracle:
        from oracle import oracle
        _oracle[name] = oracle.solve(refsweep.window(name).copy())
    return _oracle[name]


def launches(stats, name):
    return sum(k["launches"] for k in stats if k["name"] == name)


@pytest.mark.parametrize("name,band_given,band_ordered", [("sweep22", 14, 7), ("sweep42", 25, 9)])
def test_ordered_solve(name, band_given, band_ordered):
    from oracle import oracle
    p = refsweep.window(name)
    ref = reforder.ordering(p, key=name)
    so = oracle_solve(name)
    with solver(profile_kernels=1) as s:
        q = p.copy()
        sg = s.solve(q, order="auto")
        stats = s.kernel_stats()
        log = s.iteration_log()
    rel = abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"]
    at = oracle.linearize(q)["cost"]
    rel_at = abs(at - sg["final_cost"]) / sg["final_cost"]
    print(f"ORDERED {name} ls={sg['linear_solver']} band={sg['camera_band']} iters={sg['num_iterations']} "
          f"oracle iters={so['num_iterations']} rel={rel:.2e} cost at the returned parameters rel={rel_at:.2e} "
          f"obs_pairs launches={launches(stats, 'obs_pairs')}")
    assert ref["band_after"] == band_ordered and sg["camera_band"] == ref["band_after"]
    assert sg["linear_solver"] == BCR, sg
    assert launches(stats, "obs_pairs") == 0, [k for k in stats if k["launches"]]
    assert sum(k["launches"] for k in stats) > 0
    assert sg["termination"] != "FAILURE" and len(log) == sg["num_iterations"] + 1
    assert rel <= 1e-6, rel
    # the cameras are back in the caller's numbering: the oracle's cost there is the reported one, the gauge camera
    # sits untouched at its index, every other camera moved
    assert rel_at <= 1e-9, rel_at
    np.testing.assert_array_equal(q.cams[p.fixed_cam], p.cams[p.fixed_cam])
    moved = np.any(q.cams != p.cams, axis=1)
    assert moved.sum() == p.n_cams - 1 and not moved[p.fixed_cam]
    for a in ("obs_cam", "obs_pt", "obs_uv", "obs_depth", "intr_prior"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a))
    # as given: the wide paths
    with solver(profile_kernels=1) as s:
        sw = s.solve(p.copy())
        stats_w = s.kernel_stats()
    assert sw["camera_band"] == band_given and sw["linear_solver"] in (DENSE, BLOCKED), sw
    assert launches(stats_w, "obs_pairs") > 0


@pytest.mark.parametrize("name", ["sweep22", "sweep42"])
def test_ordered_solve_equals_the_permuted_window(name):
    """solve(p, order) is solve(permute_cams(p, order)) mapped back, bit for bit (deterministic = 1); order="auto"
    and the saved order are the same solve."""
    from miba.order import permute_cams, restore_cams
    p = refsweep.window(name)
    order = reforder.ordering(p, key=name)["order"]
    with solver(deterministic=1) as s:
        a = p.copy()
        sa = s.solve(a, order=order)
    with solver(deterministic=1) as s:
        b = p.copy()
        sb = s.solve(b, order="auto")
    with solver(deterministic=1) as s:
        c = p.copy()
        cp = permute_cams(c, order)
        sc = s.solve(cp)
        restore_cams(c, cp, order)
    for x, sx in ((b, sb), (c, sc)):
        np.testing.assert_array_equal(x.cams, a.cams)
        np.testing.assert_array_equal(x.points, a.points)
        np.testing.assert_array_equal(x.intr, a.intr)
        for k in ("final_cost", "initial_cost", "num_iterations", "linear_solver", "camera_band"):
            assert sx[k] == sa[k], k
    assert sa["linear_solver"] == BCR


# ------------------------------------------------------------------------------------------------------------ step
@pytest.mark.parametrize("name", ["sweep22", "sweep42"])
def test_step_of_the_permuted_window(name):
    from miba.order import inverse_order, permute_cams
    p, ref, orc, accepted = refsweep.reference(name)
    order = reforder.ordering(p, key=name)["order"]
    q = p.copy()
    with solver(**NO_TOL) as s:
        g = s.lm_step(permute_cams(q, order), 1e4)
    unchanged(q, p)
    # position k of the permuted window is camera order[k]: the step's rows in the reference's camera order
    cams = order[g["ac_cam"]]
    rows = np.argsort(cams)
    mapped = dict(ac_cam=cams[rows].astype(np.int32), delta_cam=g["delta_cam"][rows], delta_intr=g["delta_intr"],
                  delta_pts=g["delta_pts"])
    assert np.array_equal(inverse_order(order)[mapped["ac_cam"]], g["ac_cam"][rows])
    tol = refstep.step_tol(ref.cond)
    err = refstep.rel_err(mapped, ref)
    rho_ref = g["cost_change"] / ref.model_cost_change
    e_rho = abs(g["tr_ratio"] - rho_ref) / abs(rho_ref)
    print(f"STEP ordered {name} ls={g['linear_solver']} band={g['camera_band']} cond={ref.cond:.3g} tol={tol:.2e} "
          f"cams={err['cams']:.1e} intr={err['intr']:.1e} pts={err['pts']:.1e} rho={e_rho:.1e}")
    assert g["linear_solver"] == BCR and g["camera_band"] == reforder.TABLE[name][1]
    assert g["retried"] == 0 and g["flag"] == 0 and g["num_iterations"] == 1, g
    assert max(err.values()) <= tol, (err, tol)
    assert e_rho <= tol, (g["tr_ratio"], rho_ref, tol)
    assert g["accepted"] == accepted


# -------------------------------------------------------------------------------------------------- no side effect
def test_no_side_effect_on_a_prepared_window():
    """prepare, covisibility (of another window), solve_prepared: the bits of prepare, solve_prepared on a fresh
    context (deterministic = 1)."""
    p = refstep.window("bcr21")
    other = reforder.window("sweep42")
    with solver(deterministic=1) as s:
        a = p.copy()
        s.prepare(a)
        sa = s.solve_prepared(a)
        la = s.iteration_log()
    with solver(deterministic=1) as s:
        b = p.copy()
        s.prepare(b)
        r1 = s.covisibility(other.copy())
        r2 = s.covisibility(b)
        sb = s.solve_prepared(b)
        lb = s.iteration_log()
    assert r1["order_changed"] == 1 and r2["order_changed"] == 0
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(b, k), getattr(a, k))
    np.testing.assert_array_equal(lb, la)
    for k in ("final_cost", "initial_cost", "num_iterations", "num_successful_steps", "linear_solver", "camera_band"):
        assert sa[k] == sb[k], k


# ------------------------------------------------------------------------------------------------------ plan cache
def test_plan_cache():
    p = refsweep.window("sweep22")
    order = reforder.ordering(p, key="sweep22")["order"]
    with solver() as s:
        s.solve(p.copy(), order=order)
        assert s.last_prepare()["plan_reused"] == 0
        s.solve(p.copy(), order=order)
        assert s.last_prepare()["plan_reused"] == 1
        s.solve(p.copy(), order="auto")
        assert s.last_prepare()["plan_reused"] == 1
        sg = s.solve(p.copy())  # the window as given is another structure
        assert s.last_prepare()["plan_reused"] == 0 and sg["camera_band"] == 14


# -------------------------------------------------------------------------------------------------------- adapters
def test_pipeline_with_the_order_switch():
    """sequence.run_pipeline(order="auto") on a sliding-window sequence: the windows are banded, so the order is the
    identity and every window's solve is the solve without the switch, bit for bit (deterministic = 1)."""
    from miba import sequence

    def run(**kw):
        kfs, lms, K0, gt = sequence.make_tum_sequence(seed=0, n_keyframes=24, n_landmarks=600)
        with solver(deterministic=1) as s:
            txt, summ, K = sequence.run_pipeline(kfs, lms, K0, gt, s.solve, frame_frequency=10, window_size=10, **kw)
        return txt, summ, K

    txt_a, summ_a, K_a = run()
    txt_b, summ_b, K_b = run(order="auto")
    assert txt_a == txt_b and len(summ_a) == len(summ_b) >= 2
    np.testing.assert_array_equal(K_a, K_b)
    for (a0, b0, sa), (a1, b1, sb) in zip(summ_a, summ_b):
        assert (a0, b0) == (a1, b1) and sa["final_cost"] == sb["final_cost"]
        assert sa["camera_band"] == sb["camera_band"] and sa["num_iterations"] == sb["num_iterations"]


# ---------------------------------------------------------------------------------------------------------- errors
def test_errors():
    from miba.capi import BaCovisInfo, BaCovisRequest, BaSummary
    from miba.solver import MibaError
    p = refsweep.window("sweep22")
    order = reforder.ordering(p, key="sweep22")["order"]
    with solver() as s:
        q = p.copy()
        rep, high, neg = order.copy(), order.copy(), order.copy()
        rep[3], high[3], neg[0] = rep[4], p.n_cams, -1
        with pytest.raises(MibaError, match=r"\(-1\).*ba_solve_ordered.*repeats"):
            s.solve(q, order=rep)
        for bad in (high, neg):
            with pytest.raises(MibaError, match=r"\(-1\).*ba_solve_ordered.*out of range"):
                s.solve(q, order=bad)
        unchanged(q, p)
        ps = q.struct()
        req, info = BaCovisRequest(), BaCovisInfo()
        req.struct_size -= 8
        assert s._L.ba_covisibility(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "BA_COVIS_REQUEST_MIN_SIZE" in s.last_error()
        req, info = BaCovisRequest(), BaCovisInfo()
        info.struct_size -= 8
        assert s._L.ba_covisibility(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "BA_COVIS_INFO_MIN_SIZE" in s.last_error()
        sm = BaSummary()
        sm.struct_size = 16
        o = np.ascontiguousarray(order, np.int32)
        assert s._L.ba_solve_ordered(s._h, C.byref(ps), o.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(sm)) == -1
        assert "BA_SUMMARY_MIN_SIZE" in s.last_error()
        bad_obs = p.copy()
        bad_obs.obs_pt[5] = p.n_points
        with pytest.raises(MibaError, match=r"\(-1\).*observation index out of range"):
            s.covisibility(bad_obs)
        got = s.covisibility(q)  # the context still works
        assert got["band_after"] == 7
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.covisibility(p.copy())
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.solve(p.copy(), order=order)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.solve(p.copy(), order="auto")
