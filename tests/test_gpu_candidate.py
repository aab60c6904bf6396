"""The second half of an LM iteration on every reduced-solve path against extended-precision references
(tests/refcand.py): the candidate x [+] delta, its cost, the scalars the decision reads and the decision's arithmetic.

``Solver.lm_step`` runs iteration zero and the first LM iteration with the production kernels, ``Solver.lm_step_state``
(ba_debug_step_state) then copies out what that left on the device: both parameter slots, the step scalars, lin[0..1],
rows 0 and 1 of the log and the LM state. Every case asserts the path it names (as test_gpu_step.py does) and

  1. retraction: the candidate pose of every active camera equals the extended-precision retraction of the GPU's own
     delta within 16 eps per quaternion component and 16 eps max(1, |t|, |upsilon|) per translation component;
     candidate K equals K + delta_K bitwise (the points' delta is the difference of the two slots by construction,
     asserted as such; test_gpu_step.py holds it to the reference step); the gauge camera, cameras and points without an admissible
     observation are bitwise unchanged in both slots, and the slot of x holds the window's parameters bitwise;
  2. the cost belongs to the stored candidate: the log's candidate cost (== SC_CAND) equals refcand.cost at the
     candidate the hook returned, x_cost and lin[0] that at x, each within cost_bound (16 eps A + N eps cost);
  3. cost_change within tol_cost(x) + tol_cost(cand); tr_ratio against reference cost change / reference model cost
     change within that over |cost_change| plus refstep.step_tol(cond), relative;
  4. step_norm^2 == SC_SN2 == |x - x_cand|^2 and SC_XN2 == |x_cand|^2 over the active blocks, recomputed from the
     returned slots, (N + 16) eps relative; the state's xnorm2 is SC_XN2 after an accepted step, |x|^2 otherwise;
  5. the log's |gradient| (row 0) == max(gmax_ci, SC_GMAX_PT), and equals the reference max-norm within its bound;
  6. the radius arithmetic from the GPU's own rho to 4 eps: min(max_radius, r / max(1/3, 1 - (2 rho - 1)^3)) and
     decrease_factor 2 on an accepted step, r / 2 and decrease_factor 4 on a rejected one;
  7. (deterministic = 1) a one-iteration Solver.solve returns bitwise the candidate slot when the step is accepted
     and bitwise its input when it is rejected.

Check 1 found intr_step's K + (-y s) contracted into one FMA while delta held the rounded product (the candidate K an
ulp off K + delta in a few percent of the steps, first seen on roll21 / split); ba_kernels.h's add_step rounds the sum
on its own, in intr_step and in the band tail's cand_compute.

The oracle's own float64 iteration is asserted under the same bounds in the same test (Ref.oracle_errors), with two
terms that belong to Sophus' formulas, which the oracle restates literally: the cancellation in (1 - cos theta) /
theta^2 (oracle only) and the small-angle branch's V = exp(omega) (both; refcand's docstring).

Windows beside refstep's: roll21 / roll_nb37 (two cameras rolled about their optical axes by 1.6 and 1.45 rad: first
steps of theta >= 1, the sincos branch, and 0.5 <= theta < 1, the polynomial branch near its end), bcr21 / nb37_b2 at
radius 1e-8 (theta on both sides of 1e-10) and 1e-9 (every camera on the small-angle branch), and the Huber windows
(thresholds = the median block norm, both zones half full at x, 39 % .. 43 % / 50 % linear at the candidate; the
_edge variants with two reprojection and two depth blocks 4e-13 relative above / below s = b). test_refcand.py asserts
those conditions on the CPU. At radius 1e-8 / 1e-9 the cost changes by 5e-9 / 5e-10 > 0, so with tolerances 0 no
function-tolerance termination ends the step: the oracle accepts it and so must the GPU.

Measured (MI355X; each entry the error as a fraction of its bound, the largest over the paths run on that window;
retract = max(quaternion, translation), cost = max(x, candidate, cost_change), norms = max(SN2, XN2); the oracle's
under its own bound, Sophus' terms included):

  window             radius   oracle: retract cost     gmax     gpu: retract cost     rho      norms    gmax     runs
  bcr21              10000    5.2e-02         6.9e-04  0.0e+00  2.9e-02      4.5e-04  1.0e-07  1.5e-03  0.0e+00  12
  roll21             10000    4.0e-02         2.7e-03  0.0e+00  3.3e-02      3.4e-04  1.0e-07  7.4e-04  0.0e+00  4
  one10              10000    3.3e-02         1.5e-03  0.0e+00  3.2e-02      8.4e-04  5.3e-07  1.6e-03  6.8e-02  3
  nb37_b2            10000    5.0e-02         4.0e-04  2.4e-02  3.0e-02      8.1e-04  1.2e-07  8.9e-04  1.2e-02  12
  roll_nb37          10000    5.0e-02         1.8e-03  2.3e-02  2.2e-02      3.2e-04  2.6e-07  9.5e-04  1.2e-02  4
  bc_L7              10000    4.8e-02         4.9e-04  2.0e-02  3.6e-02      1.2e-04  1.0e-07  0.0e+00  2.0e-02  1
  dense_wide30       10000    4.7e-02         6.1e-04  2.0e-02  3.0e-02      3.1e-04  2.9e-07  1.4e-03  6.1e-02  2
  bcr21_f32          10000    3.2e-02         5.5e-04  5.7e-02  3.6e-02      2.8e-04  5.1e-08  1.4e-03  0.0e+00  2
  nb37_b2_f32        10000    3.9e-02         1.6e-03  4.7e-02  2.8e-02      7.8e-04  0.0e+00  5.6e-04  0.0e+00  2
  bcr21_messy        10000    3.7e-02         8.9e-04  5.3e-02  3.1e-02      3.6e-04  0.0e+00  8.7e-04  0.0e+00  1
  nb37_b2_messy      10000    4.3e-02         4.0e-04  1.8e-02  3.8e-02      2.8e-04  2.4e-07  5.8e-04  2.3e-02  1
  bcr21              1e-08    3.7e-02         1.2e-03  0.0e+00  2.7e-02      1.4e-04  8.6e-05  7.7e-04  0.0e+00  1
  bcr21              1e-09    3.8e-02         6.9e-04  0.0e+00  1.5e-02      1.6e-04  1.6e-04  1.0e-03  0.0e+00  1
  nb37_b2            1e-08    4.3e-02         2.2e-03  2.4e-02  2.0e-02      4.0e-04  1.7e-04  0.0e+00  1.2e-02  2
  nb37_b2            1e-09    4.4e-02         4.1e-04  2.4e-02  2.7e-02      4.0e-04  2.6e-04  4.5e-04  1.2e-02  2
  huber_mixed21      0.1      4.0e-02         1.4e-03  5.2e-03  3.0e-02      3.4e-04  3.8e-04  7.7e-04  3.7e-02  1
  huber_edge21       0.1      3.3e-02         1.4e-03  5.2e-03  3.6e-02      3.3e-04  5.5e-05  0.0e+00  3.7e-02  1
  huber_mixed_nb37   0.1      5.2e-02         1.8e-03  6.6e-03  3.3e-02      4.6e-04  1.6e-04  4.5e-04  0.0e+00  1
  huber_edge_nb37    0.1      4.7e-02         1.8e-03  6.6e-03  3.6e-02      1.5e-04  6.5e-05  0.0e+00  0.0e+00  1
"""
import numpy as np
import pytest

import refcand
import refstep
from refstep import EPS64, NO_TOL

pytestmark = pytest.mark.gpu

LS = {"dense": 0, "band": 1, "bcr": 2, "blocked": 3}
BCR_MODES = {"launch": 0, "persist": 1, "split": 2, "split3": 3}
MAX_RADIUS = 1e16  # ba_default_options


def _frac(err, bound):
    return float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else np.inf)


def run_candidate(monkeypatch, name, radius=1e4, env=None, opts=None, comm=False, tag=""):
    """lm_step + lm_step_state of ``name`` under ``env`` / ``opts``, checked against refcand's references; returns
    (step, state, prepare info)."""
    from miba.solver import Solver
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = refcand.reference(name, radius)
    p, ref = r.prob, r.step
    q = p.copy()
    kw = dict(NO_TOL)
    kw.update(r.okw)
    kw.update(opts or {})
    with Solver(minimizer_progress_to_stdout=0, **kw) as s:
        if comm:
            s.comm_init(1, 0, Solver.comm_unique_id())
        g = s.lm_step(q, radius)
        st = s.lm_step_state()
        info = s.last_prepare()
    for a in ("cams", "points", "intr", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"lm_step modified prob.{a}")
    assert g["retried"] == 0 and g["flag"] == 0 and g["num_iterations"] == 1 and st["iter"] == 1, (g, st)
    assert st["bad"] == 0.0 and st["termination"] == -1 and st["msg"] == "none", st
    rejected = kw.get("min_relative_decrease", 0) >= 1e3
    assert g["accepted"] == (0 if rejected else r.accepted), g
    assert (st["cur"] != st["base"]) == (g["accepted"] == 1), st
    frac = {}

    # 1. the slots: x is the window, the candidate is x [+] the GPU's own delta
    _, ac, pt = refcand.active_blocks(p)
    assert np.array_equal(g["ac_cam"], ac)
    assert np.array_equal(st["cams_x"], p.cams) and np.array_equal(st["pts_x"], p.points)
    assert np.array_equal(st["intr_x"], p.intr)
    inactive = np.setdiff1d(np.arange(p.n_cams), ac)
    assert p.fixed_cam in inactive
    assert np.array_equal(st["cams_cand"][inactive], p.cams[inactive]), "an inactive camera's candidate slot moved"
    assert np.array_equal(st["pts_cand"][~pt], p.points[~pt]), "an inactive point's candidate slot moved"
    assert np.array_equal(st["intr_cand"], st["intr_x"] + g["delta_intr"])
    # (lm_step's delta_pts is the difference of the two slots: the points have no separate delta on the device)
    assert np.array_equal(g["delta_pts"], st["pts_cand"] - st["pts_x"])
    eq = et = 0.0
    theta = np.linalg.norm(g["delta_cam"][:, 3:], axis=1)
    for t, cam in enumerate(ac):
        e = refcand.retraction_error(st["cams_cand"][cam], p.cams[cam], g["delta_cam"][t])
        b = refcand.retraction_bound(p.cams[cam], g["delta_cam"][t])
        eq, et = max(eq, e[0] / b[0]), max(et, e[1] / b[1])
    frac["retract_q"], frac["retract_t"] = eq, et

    # 2. the costs, at the slots the hook returned
    cand = (st["cams_cand"], st["intr_cand"], st["pts_cand"])
    cost_c, tol_c = refcand.cost_bound(p, r.okw, *cand)
    assert g["cost"] == st["cand"], (g["cost"], st["cand"])
    frac["cost_cand"] = _frac(abs(g["cost"] - float(cost_c)), tol_c)
    frac["cost_x"] = max(_frac(abs(st["x_cost"] - float(r.cost_x)), r.tol_x),
                         _frac(abs(st["lin"][0] - float(r.cost_x)), r.tol_x),
                         _frac(abs(st["log"][0][0] - float(r.cost_x)), r.tol_x))
    assert st["initial_cost"] == st["log"][0][0]
    assert np.array_equal(st["log"][1][:7], [g[k] for k in ("cost", "cost_change", "gradient_max_norm", "step_norm",
                                                            "tr_ratio", "tr_radius")] + [float(g["accepted"])])

    # 3. cost_change and rho
    cc_ref = float(r.cost_x - cost_c)
    assert g["cost_change"] == st["x_cost"] - st["cand"]
    frac["cost_change"] = _frac(abs(g["cost_change"] - cc_ref), r.tol_x + tol_c)
    rho_ref = cc_ref / ref.model_cost_change
    tol_rho = (r.tol_x + tol_c) / abs(cc_ref) + refstep.step_tol(ref.cond)
    frac["rho"] = _frac(abs(g["tr_ratio"] - rho_ref) / abs(rho_ref), tol_rho)
    assert g["tr_ratio"] == g["cost_change"] / st["mcc"], (g["tr_ratio"], g["cost_change"], st["mcc"])

    # 4. the norms over the active blocks
    sn2, xn2, x2, rb = refcand.norms(p, st["cams_x"], st["intr_x"], st["pts_x"], *[cand[i] for i in (0, 1, 2)])
    assert abs(g["step_norm"] - np.sqrt(st["sn2"])) <= 2 * EPS64 * g["step_norm"] and g["step_norm"] > 0
    frac["sn2"] = _frac(abs(st["sn2"] - float(sn2)) / float(sn2), rb)
    frac["xn2"] = _frac(abs(st["xn2"] - float(xn2)) / float(xn2), rb)
    if g["accepted"] == 1:
        assert st["xnorm2"] == st["xn2"]
    else:
        frac["xn2"] = max(frac["xn2"], _frac(abs(st["xnorm2"] - float(x2)) / float(x2), rb))

    # 5. the gradient max-norm at x
    gm = st["log"][0][2]
    assert gm == max(st["gmax_ci"], st["gmax_pt"]), (gm, st["gmax_ci"], st["gmax_pt"])
    frac["gmax"] = max(_frac(abs(gm - r.gmax), r.gmax_tol),
                       _frac(abs(max(st["lin"][1], st["gmax_pt"]) - r.gmax), r.gmax_tol))

    # 6. the decision's arithmetic from the GPU's own rho
    assert st["radius"] == g["tr_radius"]
    if g["accepted"] == 1:
        rho = g["tr_ratio"]
        want = min(kw.get("max_trust_region_radius", MAX_RADIUS), radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
        assert abs(g["tr_radius"] - want) <= 4 * EPS64 * want and st["decrease_factor"] == 2.0, (g, want)
        assert st["final_cost"] == st["x_cost"]  # (the accepted point's cost is absorbed by the next iteration)
    else:
        assert g["tr_radius"] == radius / 2 and st["decrease_factor"] == 4.0, (g, st)
        assert st["final_cost"] == min(st["x_cost"], st["cand"])

    oe = r.oracle_errors()
    ofr = {k: _frac(e, b) for k, (e, b) in oe.items()}
    print(f"CAND {name} radius={radius:g} {tag} bcr_path={info['bcr_path']} ls={g['linear_solver']} tail={info['tail']} "
          f"lin_path={info['lin_path']} bsfin={info['bsfin']} theta_max={theta.max():.3g} theta_min={theta.min():.3g} "
          f"accepted={g['accepted']} tol_cost_rel={tol_c / float(cost_c):.1e} "
          + " ".join(f"gpu_{k}={v:.1e}" for k, v in frac.items()) + " "
          + " ".join(f"oracle_{k}={v:.1e}" for k, v in ofr.items()))
    for k, v in ofr.items():
        assert v <= 1.0, ("oracle", k, oe[k])
    for k, v in frac.items():
        assert v <= 1.0, ("gpu", k, v, frac)
    return g, st, info, theta


def _bcr(g, info, mode):
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == BCR_MODES[mode], (g["linear_solver"], info)


# ---------------------------------------------------------------------------------------- block cyclic reduction
@pytest.mark.parametrize("mode", sorted(BCR_MODES))
@pytest.mark.parametrize("name", ["bcr21", "roll21"])
def test_bcr(name, mode, monkeypatch):
    """k_update_cams / k_bcr_border / the resident kernels' camera step; roll21: theta >= 1 and 0.5 <= theta < 1."""
    g, st, info, theta = run_candidate(monkeypatch, name, env={"MIBA_BCR": mode}, tag=mode)
    _bcr(g, info, mode)
    if name == "roll21":
        assert (theta >= 1.0).sum() >= 1 and ((theta >= 0.5) & (theta < 1.0)).sum() >= 1, np.sort(theta)[-3:]


ONE_BLOCK_ENV = {"dense1": {"MIBA_BCR_BAND": "0"}, "split": {"MIBA_BCR_BAND": "0", "MIBA_BCR_DENSE1": "0"},
                 "band": {}}


@pytest.mark.parametrize("path", sorted(ONE_BLOCK_ENV))
def test_one_block(path, monkeypatch):
    g, st, info, _ = run_candidate(monkeypatch, "one10", env=ONE_BLOCK_ENV[path], tag=path)
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == {"dense1": 4, "split": 3, "band": 5}[path], info
    if path == "band":
        assert info["tail"] == 1 and info["lin_path"] == 1, info


# ---------------------------------------------------------------------------------------- narrow band, bcr_path 5
@pytest.mark.parametrize("sw", ["1", "0"])
@pytest.mark.parametrize("tail", ["1", "0"])
@pytest.mark.parametrize("name", ["nb37_b2", "roll_nb37"])
def test_narrow_band(name, tail, sw, monkeypatch):
    """The band tail (cand_compute's candidate table in LDS beside cam_step's stores) and the separate launches."""
    g, st, info, theta = run_candidate(monkeypatch, name, env={"MIBA_TAIL": tail, "MIBA_SW": sw},
                                       tag=f"tail{tail}_sw{sw}")
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == 5 and g["camera_band"] == 2, (g, info)
    assert info["tail"] == int(tail), info
    if sw == "0":
        assert info["lin_path"] == 0, info
    if name == "roll_nb37":
        assert (theta >= 1.0).sum() >= 1 and ((theta >= 0.5) & (theta < 1.0)).sum() >= 1, np.sort(theta)[-3:]


# ---------------------------------------------------------------------------------------- band / dense / blocked
def test_band_cholesky(monkeypatch):
    g, st, info, _ = run_candidate(monkeypatch, "bc_L7", env={"MIBA_SOLVER": "band"}, tag="bw3")
    assert g["linear_solver"] == LS["band"] and g["band_tiles"] == 3 and info["bcr_path"] == -1, (g, info)


@pytest.mark.parametrize("solver", ["dense", "blocked"])
def test_dense_and_blocked_cholesky(solver, monkeypatch):
    g, st, info, _ = run_candidate(monkeypatch, "dense_wide30", env={"MIBA_SOLVER": solver}, tag=solver)
    assert g["linear_solver"] == LS[solver] and info["bcr_path"] == -1, (g["linear_solver"], info)


# ---------------------------------------------------------------------------------------- variants
@pytest.mark.parametrize("variant", ["sw2", "fpl1", "fused0", "bsfin1", "comm1"])
@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_variants(name, variant, monkeypatch):
    """The linearisation / back-substitution variants of test_gpu_step.py (k_backsub_final, the unfused path) and the
    landmark-sharded k_final_shard + k_combine on a 1-rank communicator."""
    from test_gpu_step import VARIANTS
    e_bcr, e_band, opts, want = VARIANTS[variant]
    g, st, info, _ = run_candidate(monkeypatch, name, env=e_bcr if name == "bcr21" else e_band, opts=opts,
                                   comm=variant == "comm1", tag=variant)
    assert g["linear_solver"] == LS["bcr"] and (info["bcr_path"] == 5) == (name == "nb37_b2"), (g, info)
    for k, v in want.items():
        assert info[k] == v, (k, info)


@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_deterministic_commit(name, monkeypatch):
    """deterministic = 1: the checks hold, a rejected step leaves the same candidate behind, and a one-iteration
    Solver.solve commits bitwise the candidate slot (accepted) / returns bitwise its input (rejected)."""
    from miba.solver import Solver
    radius = 1e4
    a, sa, _, _ = run_candidate(monkeypatch, name, opts={"deterministic": 1}, tag="det")
    b, sb, _, _ = run_candidate(monkeypatch, name, opts={"deterministic": 1, "min_relative_decrease": 1e3},
                                tag="det_rejected")
    assert a["accepted"] == 1 and b["accepted"] == 0
    for k in ("cams_cand", "intr_cand", "pts_cand"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["cand"] == sb["cand"] and sa["sn2"] == sb["sn2"] and sa["mcc"] == sb["mcc"]
    p = refcand.reference(name, radius).prob
    for mrd, want in ((None, (sa["cams_cand"], sa["intr_cand"], sa["pts_cand"])), (1e3, (p.cams, p.intr, p.points))):
        kw = dict(NO_TOL, deterministic=1, max_num_iterations=1, initial_trust_region_radius=radius)
        if mrd is not None:
            kw["min_relative_decrease"] = mrd
        q = p.copy()
        with Solver(minimizer_progress_to_stdout=0, **kw) as s:
            sm = s.solve(q)
            log = s.iteration_log()
        assert sm["num_iterations"] == 1 and log[1][6] == (1.0 if mrd is None else 0.0)
        assert np.array_equal(q.cams, want[0]) and np.array_equal(q.intr, want[1]) and np.array_equal(q.points, want[2])
        assert log[1][1] == a["cost_change"] and log[1][4] == a["tr_ratio"] and log[1][3] == a["step_norm"]


@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_rejected_step(name, monkeypatch):
    """The default mode's rejected step: r / 2, decrease_factor 4, xnorm2 stays |x|^2, final_cost takes the candidate's
    cost."""
    g, st, _, _ = run_candidate(monkeypatch, name, opts={"min_relative_decrease": 1e3}, tag="rejected")
    assert g["accepted"] == 0


@pytest.mark.parametrize("layout", ["obs32", "f64"])
@pytest.mark.parametrize("name", ["bcr21_f32", "nb37_b2_f32"])
def test_observation_layouts(name, layout, monkeypatch):
    run_candidate(monkeypatch, name, env={} if layout == "obs32" else {"MIBA_OBS32": "0"}, tag=layout)


@pytest.mark.parametrize("name", ["bcr21_messy", "nb37_b2_messy"])
def test_duplicates_bad_depths_shuffled(name, monkeypatch):
    g, st, info, _ = run_candidate(monkeypatch, name, tag="default")
    assert (info["bcr_path"] == 5) == (name == "nb37_b2_messy"), info


# ---------------------------------------------------------------------------------------- the small-angle branch
@pytest.mark.parametrize("radius", refcand.SMALL_RADII)
@pytest.mark.parametrize("name,env", [("bcr21", {"MIBA_BCR": "persist"}), ("nb37_b2", {"MIBA_TAIL": "1"}),
                                      ("nb37_b2", {"MIBA_TAIL": "0"})])
def test_small_angle_branch(name, env, radius, monkeypatch):
    """radius 1e-8: theta on both sides of 1e-10; 1e-9: every camera below it (theta^2 < 1e-20 in se3_plus)."""
    g, st, info, theta = run_candidate(monkeypatch, name, radius, env=env, tag="_".join(env.values()))
    if name == "bcr21":
        _bcr(g, info, "persist")
    else:
        assert info["bcr_path"] == 5 and info["tail"] == int(env["MIBA_TAIL"]), info
    t2 = (g["delta_cam"][:, 3:] ** 2).sum(1)
    if radius == refcand.SMALL_RADII[0]:
        assert (t2 < 1e-20).sum() >= 1 and (t2 >= 1e-20).sum() >= 1, np.sort(theta)
    else:
        assert (t2 < 1e-20).all() and theta.min() >= 1e-12, np.sort(theta)
    # the step is visible in the stored quaternions
    ac = g["ac_cam"]
    assert np.abs(st["cams_cand"][ac, :4] - st["cams_x"][ac, :4]).max(1).min() >= 1e-13


# ---------------------------------------------------------------------------------------- both Huber zones
@pytest.mark.parametrize("name,env", [("huber_mixed21", {"MIBA_BCR": "persist"}), ("huber_edge21", {"MIBA_BCR": "persist"}),
                                      ("huber_mixed_nb37", {"MIBA_TAIL": "1"}), ("huber_edge_nb37", {"MIBA_TAIL": "1"})])
def test_huber_zones(name, env, monkeypatch):
    """Thresholds at the median block norm: both zones of eval_obs' Huber hold 25 % .. 75 % of the blocks at x and at
    the GPU's candidate; the _edge windows put blocks 4e-13 relative on either side of s = b."""
    g, st, info, _ = run_candidate(monkeypatch, name, refcand.HUBER_RADIUS, env=env, tag="_".join(env.values()))
    if name.endswith("21"):
        _bcr(g, info, "persist")
    else:
        assert info["bcr_path"] == 5 and info["tail"] == 1, info
    r = refcand.reference(name, refcand.HUBER_RADIUS)
    for par in ((), (st["cams_cand"], st["intr_cand"], st["pts_cand"])):
        fr, fd = refcand.zone_fractions(r.prob, r.okw, *par)
        assert 0.25 <= fr <= 0.75 and 0.25 <= fd <= 0.75, (fr, fd)


# ---------------------------------------------------------------------------------------- the hook's validity
def test_step_state_needs_a_step():
    from miba.solver import MibaError, Solver
    p = refstep.window("one2")
    with Solver(minimizer_progress_to_stdout=0) as s:
        s._step_dims = (p.n_cams, p.n_points)
        with pytest.raises(MibaError, match="ba_debug_step_state"):
            s.lm_step_state()
        s.lm_step(p.copy())
        a = s.lm_step_state()
        b = s.lm_step_state()  # read-only: a second call returns the same
        assert all(np.array_equal(a[k], b[k]) for k in a)
        s.solve(p.copy())
        s._step_dims = (p.n_cams, p.n_points)
        with pytest.raises(MibaError, match="ba_debug_step_state"):
            s.lm_step_state()
