"""The multi-workgroup blocked Cholesky (BA_LS_BLOCKED, csrc/ba_dense.hip) against the high-precision step reference.

``Solver.lm_step`` against ``refstep.schur_step`` with test_gpu_step.py's assertions at tol = 8 cond(S) eps_f64: per
group (cameras, intrinsics, points) max-norm error / max-norm of the reference <= tol, the GPU's tr_ratio against its
own cost change over the reference's model cost change, the oracle's decision, a zero factorisation flag; the oracle's
own step is asserted under the same tol. Every case asserts linear_solver == 3.

The forced windows (MIBA_SOLVER=blocked) reach every residue of npad mod 64 (16: one1 / bcr11 / bcr21 / bcr79,
32: dense_n160, 48: bcr81, 0: one10 / bcr20 / dense_wide30 / bcr41), one block (one1, one10), many blocks, and
block products skipped by the 64-block envelope (bcr41 .. bcr81: a narrow band plus the intrinsics border).

A failed factorisation has no test: a non-positive pivot needs a reduced system that is not positive definite, and
the LM diagonal (min_lm_diagonal > 0 over a finite radius) keeps the damped Schur complement of finite, valid input
positive definite; the flag path of the kernels is covered by reading only.
"""
import numpy as np
import pytest

import refstep
import refsweep
from refstep import NO_TOL

pytestmark = pytest.mark.gpu

BLOCKED = 3
FORCED = {"MIBA_SOLVER": "blocked"}


def run_step(monkeypatch, name, radius=1e4, env=None, opts=None, comm=False, tag="", want_ls=BLOCKED):
    """lm_step of window ``name`` (a refstep or a sweep window) under ``env`` / ``opts``, checked against the
    reference; returns (step, prepare info)."""
    from miba.solver import Solver
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    p, ref, orc, accepted = refsweep.reference(name, radius)
    q = p.copy()
    kw = dict(NO_TOL)
    kw.update(opts or {})
    with Solver(minimizer_progress_to_stdout=0, **kw) as s:
        if comm:
            s.comm_init(1, 0, Solver.comm_unique_id())
        g = s.lm_step(q, radius)
        info = s.last_prepare()
    for a in ("cams", "points", "intr", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"lm_step modified prob.{a}")
    tol = refstep.step_tol(ref.cond)
    e_orc = refstep.rel_err(orc, ref)
    e_gpu = refstep.rel_err(g, ref)
    rho_ref = g["cost_change"] / ref.model_cost_change
    e_rho = abs(g["tr_ratio"] - rho_ref) / abs(rho_ref)
    print(f"STEP {name} radius={radius:g} {tag} ls={g['linear_solver']} bcr_path={info['bcr_path']} "
          f"cond={ref.cond:.3g} tol={tol:.2e} oracle={max(e_orc.values()):.1e} gpu_cams={e_gpu['cams']:.1e} "
          f"gpu_intr={e_gpu['intr']:.1e} gpu_pts={e_gpu['pts']:.1e} rho={e_rho:.1e}")
    assert g["linear_solver"] == want_ls and info["bcr_path"] == -1, (g["linear_solver"], info)
    assert g["retried"] == 0 and g["flag"] == 0 and g["num_iterations"] == 1, g
    assert max(e_orc.values()) <= tol, (e_orc, tol)
    assert max(e_gpu.values()) <= tol, (e_gpu, tol)
    assert e_rho <= tol, (g["tr_ratio"], rho_ref, tol)
    assert g["accepted"] == accepted, g
    assert g["tr_radius"] > 0 and g["step_norm"] > 0
    return g, info


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ac_cam", "delta_cam", "delta_intr", "delta_pts"))


# ------------------------------------------------------------------------------------------- forced-path parity
FORCED_WINDOWS = ["one1", "one10", "bcr11", "bcr20", "bcr21", "dense_n160", "dense_wide30", "full31", "bcr41", "bcr79",
                  "bcr81", "gauge_mid21", "inactive_mid21", "bcr21_messy", "bcr21_f32"]
NPAD = {"one1": 16, "one10": 64, "bcr11": 80, "bcr20": 128, "bcr21": 144, "dense_n160": 160, "dense_wide30": 192,
        "full31": 192, "bcr41": 256, "bcr79": 480, "bcr81": 496}


@pytest.mark.parametrize("name", FORCED_WINDOWS)
def test_forced_step_parity(name, monkeypatch):
    g, _ = run_step(monkeypatch, name, env=FORCED, tag="forced")
    if name in NPAD:
        assert (6 * len(g["ac_cam"]) + 4 + 15) // 16 * 16 == NPAD[name]


@pytest.mark.parametrize("radius", [1e12, 1e-2])
@pytest.mark.parametrize("name", ["bcr21", "bcr81"])
def test_forced_radii(name, radius, monkeypatch):
    """Almost no damping (Gauss-Newton) and heavy damping."""
    run_step(monkeypatch, name, radius, env=FORCED, tag="forced")


# ------------------------------------------------------------------------------------------------ sweep windows
@pytest.mark.parametrize("how", ["forced", "selected"])
@pytest.mark.parametrize("name", sorted(refsweep.SWEEPS))
def test_sweep_windows(name, how, monkeypatch):
    """Wide co-visibility (camera band 14 / 25, every point an overflow point), forced and by the default rule with
    the threshold below the window's size."""
    run_step(monkeypatch, name, env=FORCED if how == "forced" else {"MIBA_BLOCKED_MIN": "64"}, tag=how)


def test_default_selection(monkeypatch):
    """Without any setting: k_chol below the threshold, the blocked path from it (sweep42: npad 256)."""
    for k in ("MIBA_SOLVER", "MIBA_DENSE_CHOL", "MIBA_BLOCKED_MIN"):
        monkeypatch.delenv(k, raising=False)
    g, _ = run_step(monkeypatch, "dense_wide30", tag="default", want_ls=0)
    assert g["camera_band"] >= 10
    assert refsweep.npad(refsweep.window("sweep42")) == 256
    run_step(monkeypatch, "sweep42", tag="default")
    # the explicit settings still mean k_chol
    run_step(monkeypatch, "sweep42", env={"MIBA_SOLVER": "dense"}, tag="dense", want_ls=0)
    monkeypatch.delenv("MIBA_SOLVER")
    run_step(monkeypatch, "sweep42", env={"MIBA_DENSE_CHOL": "1"}, tag="dense_chol", want_ls=0)


@pytest.mark.parametrize("name", ["dense_wide30", "sweep42"])
def test_agrees_with_k_chol(name, monkeypatch):
    """The blocked and the one-workgroup envelope Cholesky solve the same system: their steps agree to tol."""
    b, _ = run_step(monkeypatch, name, env=FORCED, tag="blocked")
    d, _ = run_step(monkeypatch, name, env={"MIBA_SOLVER": "dense"}, tag="dense", want_ls=0)
    tol = refstep.step_tol(refsweep.reference(name)[1].cond)
    err = refstep.rel_err(b, d)
    print(f"BLOCKED-DENSE {name} {err}")
    assert max(err.values()) <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------ deterministic
# The solve is bitwise reproducible GIVEN S and rhs (no atomics, fixed summation order), so these cases run on windows
# whose assembly is reproducible under deterministic = 1. The sweep windows' is not, whatever the reduced solve:
# ba_debug_reduced_system of sweep22 / sweep42 differs between two fresh deterministic contexts by 3e-16 .. 4e-16
# (absolute, MI355X), and their steps differ with MIBA_SOLVER=dense as they do with the blocked path, while
# dense_wide30's S and steps repeat bitwise on both paths. That is the overflow Schur's, not this path's.
@pytest.mark.parametrize("name", ["dense_wide30", "bcr81"])
def test_deterministic_step_repeats_bitwise(name, monkeypatch):
    a, _ = run_step(monkeypatch, name, env=FORCED, opts={"deterministic": 1}, tag="det")
    b, _ = run_step(monkeypatch, name, env=FORCED, opts={"deterministic": 1}, tag="det_repeat")
    assert same_bits(a, b)
    assert a["tr_ratio"] == b["tr_ratio"] and a["cost"] == b["cost"]


def test_no_residue_in_S_after_a_solve(monkeypatch):
    """deterministic = 1: after a full blocked solve the context builds the reduced system of a window, and its
    covariance, with the bits a fresh context builds them with: the solve leaves nothing behind in S."""
    from miba.solver import Solver
    monkeypatch.setenv("MIBA_SOLVER", "blocked")
    p = refstep.window("dense_wide30")
    with Solver(minimizer_progress_to_stdout=0, deterministic=1) as s:
        S0, r0 = s.reduced_system(p.copy(), 1e4)
        c0 = s.covariance(p.copy(), full=True)
    with Solver(minimizer_progress_to_stdout=0, deterministic=1) as s:
        q = p.copy()
        sm = s.solve(q)
        assert sm["linear_solver"] == BLOCKED and sm["termination"] != "FAILURE" and sm["num_iterations"] >= 2, sm
        S1, r1 = s.reduced_system(p.copy(), 1e4)
        c1 = s.covariance(p.copy(), full=True)
    assert S0.shape == (178, 178)
    np.testing.assert_array_equal(S1, S0)
    np.testing.assert_array_equal(r1, r0)
    assert c0["status"] == 0 and c1["status"] == 0
    np.testing.assert_array_equal(c1["full"], c0["full"])
    for a, b in zip(c0["pair_cov"], c1["pair_cov"]):
        np.testing.assert_array_equal(b, a)


# ---------------------------------------------------------------------------------------------------- sharding
def test_one_rank_communicator(monkeypatch):
    """The landmark-sharded launch list (envelope all-reduce before the solve) on a 1-rank communicator."""
    run_step(monkeypatch, "dense_wide30", env=FORCED, opts={"shard_min_obs": 0}, comm=True, tag="comm1")


# -------------------------------------------------------------------------------------------------- plan cache
def test_plan_cache(monkeypatch):
    """A second prepare of the same window reuses the plan (and the block lists) and repeats the bits; a window with
    changed obs_pt rebuilds them and still meets the reference."""
    from miba.solver import Solver
    monkeypatch.setenv("MIBA_SOLVER", "blocked")
    p, ref, _, _ = refstep.reference("dense_wide30")
    tol = refstep.step_tol(ref.cond)
    # the other structure: the last 20 points lose the two lowest cameras of their tracks (of 6 .. 16)
    lo = np.full(p.n_points, p.n_cams, np.int64)
    np.minimum.at(lo, p.obs_pt, p.obs_cam)
    keep = ~((p.obs_pt >= p.n_points - 20) & (p.obs_cam < lo[p.obs_pt] + 2))
    assert 0 < (~keep).sum() <= 40
    p2 = p.copy()
    p2.obs_cam, p2.obs_pt = p.obs_cam[keep].copy(), p.obs_pt[keep].copy()
    p2.obs_uv, p2.obs_depth = p.obs_uv[keep].copy(), p.obs_depth[keep].copy()
    ref2 = refstep.schur_step(p2, None, 1e4)
    with Solver(minimizer_progress_to_stdout=0, deterministic=1, **NO_TOL) as s:
        a = s.lm_step(p.copy(), 1e4)
        assert s.last_prepare()["plan_reused"] == 0
        b = s.lm_step(p.copy(), 1e4)
        assert s.last_prepare()["plan_reused"] == 1
        assert a["linear_solver"] == BLOCKED and b["linear_solver"] == BLOCKED
        assert same_bits(a, b) and a["tr_ratio"] == b["tr_ratio"]
        assert max(refstep.rel_err(b, ref).values()) <= tol
        c = s.lm_step(p2.copy(), 1e4)
        assert s.last_prepare()["plan_reused"] == 0
        e2 = refstep.rel_err(c, ref2)
        print(f"PLAN changed structure: {e2} tol={refstep.step_tol(ref2.cond):.2e}")
        assert c["linear_solver"] == BLOCKED and c["flag"] == 0
        assert max(e2.values()) <= refstep.step_tol(ref2.cond)
        d = s.lm_step(p.copy(), 1e4)  # and back
        assert s.last_prepare()["plan_reused"] == 0 and same_bits(a, d)


# ------------------------------------------------------------------------------------------------- whole solve
def test_whole_solve_against_the_oracle(monkeypatch):
    """sweep42 with default options on the default path: the oracle's termination, accept / reject sequence and
    iteration count; final cost within 1e-6 relative (the README's parity rule)."""
    from miba.solver import Solver
    from oracle import oracle
    for k in ("MIBA_SOLVER", "MIBA_DENSE_CHOL", "MIBA_BLOCKED_MIN"):
        monkeypatch.delenv(k, raising=False)
    p = refsweep.window("sweep42")
    so, tr = oracle.solve_trace(p.copy())
    with Solver(minimizer_progress_to_stdout=0) as s:
        sg = s.solve(p.copy())
        log = s.iteration_log()
    rel = abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"]
    print(f"SOLVE sweep42 ls={sg['linear_solver']} iters gpu={sg['num_iterations']} oracle={so['num_iterations']} "
          f"term gpu={sg['termination']} oracle={so['termination']} rel={rel:.2e}")
    assert sg["linear_solver"] == BLOCKED
    assert sg["termination"] == so["termination"] and sg["termination"] != "FAILURE"
    assert sg["num_iterations"] == so["num_iterations"]
    assert sg["num_successful_steps"] == so["num_successful_steps"]
    assert len(log) == len(tr)
    np.testing.assert_array_equal(log[:, 6], tr[:, 6])
    assert rel <= 1e-6, rel
