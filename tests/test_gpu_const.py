"""Constant cameras (ba_set_constant_cameras) on the GPU.

Step: ``Solver.lm_step`` under a mask against tests/refconst.py (refstep's extended-precision Schur route with the
masked cameras dropped), per group max-norm error / max-norm of the reference <= refstep.step_tol(cond) =
8 cond(S) eps_f64, the tolerance of tests/test_gpu_step.py; the reduced system (``Solver.reduced_system``) against the
reference's S and rhs in refschur.system_err's metric under the same bound. One window per reduced-solve path, each
the smallest of refstep's generator that takes it (refconst.window): 6 cameras for the one-block dense solve
(MIBA_BCR_BAND=0, bcr_path 4), the band solve with its tail (the default, bcr_path 5 / tail 1) and the blocked
Cholesky (MIBA_SOLVER=blocked, linear_solver 3); 24 cameras with tracks of 4..9 for the block cyclic reduction
(MIBA_BCR=launch, bcr_path 0; 12 active cameras are left when every second one is constant). The masks
(refconst.masks): first, middle, last, two adjacent, every second camera, all but one, a masked camera without
observations, a mask beside a different fixed_cam. Every case asserts the path it ran on.

Identity, digests (host plan against MIBA_DEVICE_PLAN=1), solves, the plan cache, covariance (tests/refcov.py driven
with the masked cameras dropped, test_gpu_cov.py's metric and tolerance), the ordered solve and the errors follow.
"""
import numpy as np
import pytest

import refconst
import refcov
import refschur
import refstep
from refstep import NO_TOL

pytestmark = pytest.mark.gpu

BCR, BLOCKED = 2, 3
# path -> (window, environment, (linear_solver, bcr_path, tail) by the active cameras left)
PATHS = {
    "dense1": ("small", {"MIBA_BCR_BAND": "0"}, lambda nac: (BCR, 4, 0)),
    "tail": ("small", {}, lambda nac: (BCR, 5, 1) if nac >= 2 else (BCR, 4, 0)),
    "bcr": ("bcr", {"MIBA_BCR": "launch"}, lambda nac: (BCR, 0, 0)),
    "blocked": ("small", {"MIBA_SOLVER": "blocked"}, lambda nac: (BLOCKED, -1, 0)),
}


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def cases():
    for path in PATHS:
        for name in refconst.MASK_NAMES:
            if path == "bcr" and name == "all_but_one":
                continue  # one active camera is a one-block window whatever the window's size: the small windows' case
            yield path, name


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ac_cam", "delta_cam", "delta_intr", "delta_pts"))


@pytest.mark.parametrize("path,name", list(cases()))
def test_step_under_a_mask(path, name, monkeypatch):
    kind, env, want = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, mask, ref = refconst.case(kind, name)
    q = p.copy()
    with solver(**NO_TOL) as s:
        s.set_constant_cameras(mask)
        g = s.lm_step(q, 1e4)
        info = s.last_prepare()
        S, rhs = s.reduced_system(q, 1e4)
    with solver(deterministic=1, **NO_TOL) as s:
        s.set_constant_cameras(mask)
        d = s.lm_step(q, 1e4)
        d2 = s.lm_step(q, 1e4)
    for a in ("cams", "points", "intr", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"lm_step modified prob.{a}")
    tol = refstep.step_tol(ref.cond)
    e_gpu, e_det = refstep.rel_err(g, ref), refstep.rel_err(d, ref)
    rho_ref = g["cost_change"] / ref.model_cost_change
    e_rho = abs(g["tr_ratio"] - rho_ref) / abs(rho_ref)
    S_ref, rhs_ref, _ = refconst.reduced_system(p, mask, None, 1e4)
    e_s, e_r = refschur.system_err(S, -rhs, S_ref, rhs_ref)
    nac = len(ref.ac_cam)
    print(f"CONST {path}/{name} nac={nac} ls={g['linear_solver']} bcr_path={info['bcr_path']} tail={info['tail']} "
          f"cond={ref.cond:.3g} tol={tol:.2e} cams={e_gpu['cams']:.1e} intr={e_gpu['intr']:.1e} pts={e_gpu['pts']:.1e} "
          f"det={max(e_det.values()):.1e} rho={e_rho:.1e} S={e_s:.1e} rhs={e_r:.1e}")
    assert (g["linear_solver"], info["bcr_path"], info["tail"]) == want(nac), (g["linear_solver"], info)
    assert g["retried"] == 0 and g["flag"] == 0 and g["num_iterations"] == 1, g
    assert S.shape == (6 * nac + 4,) * 2
    assert max(e_gpu.values()) <= tol, (e_gpu, tol)
    assert max(e_det.values()) <= tol, (e_det, tol)
    assert e_rho <= tol, (g["tr_ratio"], rho_ref, tol)
    assert max(e_s, e_r) <= tol, (e_s, e_r, tol)
    assert same_bits(d, d2)


# ---------------------------------------------------------------------------------------------------------- identity
def _solve(p, mask=None, clear=False, **kw):
    q = p.copy()
    with solver(deterministic=1, **kw) as s:
        if mask is not None:
            s.set_constant_cameras(mask)
        if clear:
            s.set_constant_cameras(None)
        sm = s.solve(q)
        log = s.iteration_log()
    return q, sm, log


def _assert_same_solve(a, b):
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(a[0], k), getattr(b[0], k))
    np.testing.assert_array_equal(a[2], b[2])
    for k in ("final_cost", "initial_cost", "num_iterations", "num_active_cams", "linear_solver", "camera_band"):
        assert a[1][k] == b[1][k], k


@pytest.mark.parametrize("kind", ["small", "bcr"])
def test_empty_mask_is_no_mask(kind):
    p = refconst.window(kind)
    fresh = _solve(p)
    _assert_same_solve(_solve(p, np.zeros(p.n_cams, bool)), fresh)
    _assert_same_solve(_solve(p, np.ones(p.n_cams, bool), clear=True), fresh)


@pytest.mark.parametrize("kind,g", [("small", 0), ("small", 3), ("bcr", 11), ("bcr", 23)])
def test_one_camera_mask_is_fixed_cam(kind, g):
    a = refconst.window(kind).copy()
    a.fixed_cam = g
    b = a.copy()
    b.fixed_cam = -1
    mask = np.zeros(a.n_cams, bool)
    mask[g] = True
    _assert_same_solve(_solve(b, mask), _solve(a))


# ----------------------------------------------------------------------------------------------------------- digests
@pytest.mark.parametrize("kind", ["small", "bcr"])
@pytest.mark.parametrize("name", refconst.MASK_NAMES)
def test_host_and_device_plan_digests_agree(kind, name, monkeypatch):
    p, mask, _ = refconst.case(kind, name) if (kind, name) != ("bcr", "all_but_one") else \
        (refconst.window("bcr"), refconst.masks(24, refconst.EMPTY_CAM)["all_but_one"][0], None)
    dig = {}
    for dev in ("0", "1"):
        monkeypatch.setenv("MIBA_DEVICE_PLAN", dev)
        with solver() as s:
            s.set_constant_cameras(mask)
            s.prepare(p.copy())
            assert s.last_prepare()["plan_device"] == int(dev)
            dig[dev] = s.plan_digest()
    assert dig["0"] == dig["1"] and len(dig["0"]) > 0
    if name in ("first", "middle", "last"):  # the digests of fixed_cam = g without a mask
        q = p.copy()
        q.fixed_cam = int(np.nonzero(mask)[0][0])
        with solver() as s:
            s.prepare(q)
            assert s.plan_digest() == dig["1"]


# ------------------------------------------------------------------------------------------------------------ solves
TOL_REASONS = ("Gradient tolerance reached", "Parameter tolerance reached", "Function tolerance reached")


@pytest.mark.parametrize("kind,name", [("small", "middle"), ("small", "every_second"), ("bcr", "adjacent"),
                                       ("bcr", "every_second"), ("bcr", "plus_fixed")])
def test_solve_under_a_mask(kind, name):
    p, mask, ref = refconst.case(kind, name)
    q = p.copy()
    with solver() as s:
        s.set_constant_cameras(mask)
        sm = s.solve(q)
        log = s.iteration_log()
        rep = s.residuals(q, per_obs=False, per_block=False)
    const = mask.copy()
    if p.fixed_cam >= 0:
        const[p.fixed_cam] = True
    np.testing.assert_array_equal(q.cams[const], p.cams[const])
    moved = np.abs(q.cams - p.cams).max(1) > 0
    assert moved[ref.ac_cam].all() and not moved[const].any()
    assert sm["num_active_cams"] == len(ref.ac_cam) and sm["reduced_system_size"] == 6 * len(ref.ac_cam) + 4
    print(f"SOLVE const {kind}/{name} {sm['termination']} it={sm['num_iterations']} cost {sm['initial_cost']:.6e} -> "
          f"{sm['final_cost']:.6e} |g|={log[-1, 2]:.2e} '{sm['message']}'")
    assert sm["final_cost"] < sm["initial_cost"]
    # the cost of the result is the cost the residual report evaluates there (different summation orders: the bound
    # test_gpu_covis.py holds the oracle's re-evaluation to)
    assert abs(rep["total_cost"] - sm["final_cost"]) <= 1e-9 * sm["final_cost"], (rep["total_cost"], sm["final_cost"])
    if sm["termination"] == "CONVERGENCE":
        assert log[-1, 2] <= s.options.gradient_tolerance or sm["message"].startswith(TOL_REASONS), sm["message"]
    else:  # the iteration limit, as ba_solve reports it
        assert sm["num_iterations"] == s.options.max_num_iterations and sm["message"].startswith("Maximum number")


def test_all_cameras_constant():
    p = refconst.window("small")
    q = p.copy()
    with solver() as s:
        s.set_constant_cameras(np.ones(p.n_cams, bool))
        sm = s.solve(q)
    assert sm["num_active_cams"] == 0 and sm["reduced_system_size"] == 4
    np.testing.assert_array_equal(q.cams, p.cams)
    assert sm["final_cost"] < sm["initial_cost"] and np.abs(q.points - p.points).max() > 0


# -------------------------------------------------------------------------------------------------------- plan cache
def test_plan_cache_keys_on_the_mask():
    p, mask, _ = refconst.case("bcr", "adjacent")
    other = refconst.masks(p.n_cams)["middle"][0]
    with solver() as s:
        s.set_constant_cameras(mask)
        s.solve(p.copy())
        assert s.last_prepare()["plan_reused"] == 0
        s.solve(p.copy())
        assert s.last_prepare()["plan_reused"] == 1
        s.set_constant_cameras(mask.copy())  # the same mask set again
        a = s.solve(p.copy())
        assert s.last_prepare()["plan_reused"] == 1
        s.set_constant_cameras(other)
        b = s.solve(p.copy())
        assert s.last_prepare()["plan_reused"] == 0 and b["num_active_cams"] == a["num_active_cams"] + 1
        s.set_constant_cameras(None)
        c = s.solve(p.copy())
        assert s.last_prepare()["plan_reused"] == 0 and c["num_active_cams"] == b["num_active_cams"] + 1


# -------------------------------------------------------------------------------------------------------- covariance
@pytest.mark.parametrize("kind,name", [("small", "middle"), ("bcr", "adjacent"), ("bcr", "plus_fixed")])
def test_covariance_under_a_mask(kind, name):
    p, mask, _ = refconst.case(kind, name)
    ref = refconst.schur_cov(p, mask)
    INTR = -1
    cams = list(range(p.n_cams))
    pairs = [(a, a) for a in cams] + [(a, INTR) for a in cams] + [(INTR, INTR)] + \
        [(int(np.nonzero(mask)[0][0]), int(ref.ac_cam[0])), (int(ref.ac_cam[0]), int(ref.ac_cam[-1]))]
    with solver() as s:
        s.set_constant_cameras(mask)
        g = s.covariance(p.copy(), pairs=pairs, points="all", full=True)
    assert g["status"] == 0 and list(g["ac_cam"]) == list(ref.ac_cam) and g["nac"] == len(ref.ac_cam)
    tol = refstep.step_tol(ref.cond)
    ep = refcov.pair_errors(g["full"], ref.red)
    ex = refcov.point_errors(g["point_cov"], ref.pts)
    print(f"COV const {kind}/{name} n={g['n']} cond={ref.cond:.3g} tol={tol:.2e} pairs={ep:.1e} points={ex:.1e}")
    assert ep <= tol and ex <= tol, (ep, ex, tol)
    ac_of = {int(c): t for t, c in enumerate(ref.ac_cam)}
    for (a, b), blk in zip(g["pairs"], g["pair_cov"]):
        const = [v for v in (a, b) if v != INTR and (mask[v] or v == p.fixed_cam)]
        if const:
            assert (blk == 0).all(), (a, b, "a pair with a constant camera is a zero block")
        elif any(v != INTR and v not in ac_of for v in (a, b)):
            assert np.isnan(blk).all(), (a, b)
        else:
            off = lambda v: 6 * len(ac_of) if v == INTR else 6 * ac_of[v]
            assert np.array_equal(blk, g["full"][off(a): off(a) + blk.shape[0], off(b): off(b) + blk.shape[1]])


# ------------------------------------------------------------------------------------------------------ ordered solve
def test_ordered_solve_under_a_mask():
    import reforder
    from miba.order import permute_cams, restore_cams
    p = reforder.window("sweep42").copy()
    mask = np.zeros(p.n_cams, bool)
    mask[[5, 20, 21, 40]] = True
    with solver(deterministic=1) as s:
        s.set_constant_cameras(mask)
        cv = s.covisibility(p)
        order = cv["order"]
        a = p.copy()
        sa = s.solve(a, order="auto")
        info = s.last_prepare()
        b = p.copy()
        sb = s.solve(b)  # the context's own mask is back in force: the same window unordered
    # constant cameras are not nodes of the ordering: they follow the active cameras, in index order
    n_active = cv["n_active"]
    assert cv["order_changed"] == 1 and n_active == p.n_cams - 1 - 4
    assert order[n_active:].tolist() == sorted([p.fixed_cam, 5, 20, 21, 40])
    np.testing.assert_array_equal(a.cams[mask], p.cams[mask])
    np.testing.assert_array_equal(b.cams[mask], p.cams[mask])
    assert sa["num_active_cams"] == sb["num_active_cams"] == n_active and sa["camera_band"] < sb["camera_band"]
    # the ordered solve is the solve of the permuted window under the permuted mask, bit for bit
    with solver(deterministic=1) as s:
        s.set_constant_cameras(mask[order])
        c = p.copy()
        cp = permute_cams(c, order)
        sc = s.solve(cp)
        restore_cams(c, cp, order)
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(a, k), getattr(c, k))
    assert sa["final_cost"] == sc["final_cost"] and sa["num_iterations"] == sc["num_iterations"]
    # and it meets the unordered solve as test_gpu_covis.py holds the ordered solve to the window as given: 1e-6
    rel = abs(sa["final_cost"] - sb["final_cost"]) / sb["final_cost"]
    print(f"ORDERED const band {sb['camera_band']} -> {sa['camera_band']} rel={rel:.1e} plan_device={info['plan_device']}")
    assert rel <= 1e-6, rel


# ------------------------------------------------------------------------------------------------------------ errors
def test_errors():
    from miba.solver import MibaError
    p = refconst.window("small")
    with solver() as s:
        s.set_constant_cameras(np.ones(p.n_cams + 1, bool))
        q = p.copy()
        with pytest.raises(MibaError, match=r"\(-1\).*constant-camera mask was set for 7"):
            s.solve(q)
        with pytest.raises(MibaError, match=r"\(-1\).*constant-camera mask"):
            s.prepare(q)
        for k in ("cams", "points", "intr"):
            np.testing.assert_array_equal(getattr(q, k), getattr(p, k))
        s.set_constant_cameras(None)
        assert s.solve(q)["termination"] == "CONVERGENCE"  # the context still works
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        s.set_constant_cameras(refconst.masks(p.n_cams)["middle"][0])
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.solve(p.copy())
        s.set_constant_cameras(None)
        assert s.solve(p.copy())["num_active_cams"] == 4
