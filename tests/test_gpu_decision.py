"""The LM decision state machine (lm_decide_local) against the oracle's trace, row by row: forced rejections, a
reject-reject-accept sequence, and every termination reason that finite, well-posed inputs reach, one option each.
(The invalid-step path needs a non-positive-definite system or a non-finite input; test_gpu_edge.py covers it.)

Costs and rho against the oracle use test_converged_parity.py's tolerances (cost 1e-6 relative, 1e-9 on the first
three rows, cost change / |gradient| / |step| / rho 1e-6); flags, counts and the termination are exact. A radius is
exact where it does not depend on rho's last bits: after a rejection (r / decrease_factor), under the
max_trust_region_radius clamp and where rho saturates the update at 3 r (1 - (2 rho - 1)^3 <= 1/3, rho >= 0.937: every
accepted step here); it is also recomputed from the GPU's own rho to 4 eps.

Measured (MI355X), relative to the oracle, the largest over a window's cases:

  window    cost (rows 0..2)  cost (all rows)  rho      where
  bcr21     5.5e-11           5.5e-11          2.5e-12  reject-reject-accept from radius 1e6 (the others <= 3.1e-15 / 3.3e-14)
  nb37_b2   4.6e-12           4.6e-12          2.3e-13  reject-reject-accept from radius 1e4; max_num_iterations = 2
(nb37_b2's reject-reject-accept sequence from radius 1e6 measured 9.1e-10 on row 1, too close to 1e-9 to keep: it
starts at 1e4.)
"""
import numpy as np
import pytest

import refstep
from oracle import oracle
from refstep import EPS64, NO_TOL

pytestmark = pytest.mark.gpu
WINDOWS = ["bcr21", "nb37_b2"]
PARAMS = ("cams", "intr", "points")


def run_sequence(name, **opts):
    """Solver.solve and oracle.solve_trace of window ``name`` under ``opts``, compared; returns (gpu summary, gpu
    log, solved gpu window, oracle summary, oracle trace, solved oracle window)."""
    from miba.solver import Solver
    p = refstep.window(name)
    kw = dict(NO_TOL)
    kw.update(opts)
    qo = p.copy()
    so, tr = oracle.solve_trace(qo, oracle.default_options(**kw))
    qg = p.copy()
    with Solver(minimizer_progress_to_stdout=0, **kw) as s:
        sg = s.solve(qg)
        log = s.iteration_log()
    kind = lambda m: m.split(".")[0].split(":")[0]
    assert sg["termination"] == so["termination"] and kind(sg["message"]) == kind(so["message"]), (sg, so["message"])
    for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps"):
        assert sg[k] == so[k], (k, sg[k], so[k])
    assert log.shape == tr.shape, (log.shape, tr.shape)
    np.testing.assert_array_equal(log[:, 6], tr[:, 6])
    np.testing.assert_allclose(log[:, 0], tr[:, 0], rtol=1e-6)
    np.testing.assert_allclose(log[:3, 0], tr[:3, 0], rtol=1e-9)
    scale = np.abs(tr[:, 0]).max()
    np.testing.assert_allclose(log[:, 1], tr[:, 1], rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(log[:-1, 2], tr[:-1, 2], rtol=1e-6)
    np.testing.assert_allclose(log[:, 3], tr[:, 3], rtol=1e-6)
    np.testing.assert_allclose(log[:, 4], tr[:, 4], rtol=1e-6, atol=1e-9)
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-12 * so["initial_cost"]
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-9 * so["final_cost"]
    # the radius sequence
    rmax = kw.get("max_trust_region_radius", 1e16)
    r, dec = log[0, 5], 2.0
    assert r == kw.get("initial_trust_region_radius", 1e4) == tr[0, 5]
    for i in range(1, log.shape[0]):
        acc, rho = log[i, 6], log[i, 4]
        if acc == 1:
            want = min(rmax, r / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            assert abs(log[i, 5] - want) <= 4 * EPS64 * want, (i, log[i], want)
            if want == rmax or min(rho, tr[i, 4]) >= 0.94:
                assert log[i, 5] == tr[i, 5], (i, log[i, 5], tr[i, 5])
            dec = 2.0
        elif acc == 0:
            assert log[i, 5] == r / dec == tr[i, 5], (i, log[i, 5], r, dec)
            dec *= 2.0
        else:  # a tolerance ended the solve inside the iteration: the radius is not updated
            assert log[i, 5] == r == tr[i, 5]
        r = log[i, 5]
    e_rows = np.abs(log[:, 0] - tr[:, 0]) / tr[:, 0]
    e_cost = float(e_rows.max())
    e_rho = float(np.max(np.abs(log[1:, 4] - tr[1:, 4]) / np.maximum(np.abs(tr[1:, 4]), 1e-300))) if len(log) > 1 else 0.0
    print(f"DECISION {name} {opts} rows={log.shape[0]} accepted={log[:, 6].tolist()} radius={log[:, 5].tolist()} "
          f"cost_err={e_cost:.1e} rows={[float(f'{v:.1e}') for v in e_rows]} rho_err={e_rho:.1e} {sg['message']!r}")
    return sg, log, qg, so, tr, qo


def unchanged(q, name):
    p = refstep.window(name)
    return all(np.array_equal(getattr(q, a), getattr(p, a)) for a in PARAMS)


@pytest.mark.parametrize("name", WINDOWS)
def test_forced_rejections(name):
    r0 = 1e4
    sg, log, qg, so, tr, qo = run_sequence(name, min_relative_decrease=1e3, max_num_iterations=4,
                                           initial_trust_region_radius=r0)
    assert log[1:, 6].tolist() == [0.0] * 4 and sg["num_iterations"] == 4 and sg["num_unsuccessful_steps"] == 4
    assert log[:, 5].tolist() == [r0, r0 / 2, r0 / 8, r0 / 64, r0 / 1024]
    assert unchanged(qg, name) and unchanged(qo, name)
    # Ceres keeps the minimum over the iterations' costs, the rejected candidates' included
    assert sg["final_cost"] == log[:, 0].min() < sg["initial_cost"]
    assert sg["termination"] == "NO_CONVERGENCE"


# quadratic loss (hub_p_* = 1e3: every block in Huber's quadratic zone) makes rho < 1 and growing towards 1 as the
# radius shrinks: at r, r / 2, r / 8 the oracle's rho is 0.99419, 0.99512, 0.99732 from r = 1e6 (bcr21) and 0.99519,
# 0.99673, 0.99876 from r = 1e4 (nb37_b2), so these thresholds reject twice and accept the third step, each rho at least
# 7e-4 from its threshold. window -> (initial radius, min_relative_decrease)
REJECT_THEN_ACCEPT = {"bcr21": (1e6, 0.996), "nb37_b2": (1e4, 0.998)}


@pytest.mark.parametrize("name", WINDOWS)
def test_reject_then_accept(name):
    r0, mrd = REJECT_THEN_ACCEPT[name]
    sg, log, qg, so, tr, qo = run_sequence(name, min_relative_decrease=mrd, max_num_iterations=3,
                                           initial_trust_region_radius=r0, hub_p_repr=1e3, hub_p_unpr=1e3)
    assert log[1:, 6].tolist() == [0.0, 0.0, 1.0], log[:, 6]
    assert log[:, 5].tolist() == [r0, r0 / 2, r0 / 8, 3 * r0 / 8]  # then 3 r with decrease_factor back at 2
    assert not unchanged(qg, name)
    for a in PARAMS:
        np.testing.assert_allclose(getattr(qg, a), getattr(qo, a), rtol=1e-8, atol=1e-8)


TERMINATIONS = {
    # option -> (termination, message kind, iterations, accepted flags of rows 1.., x unchanged)
    "max_iter0": (dict(max_num_iterations=0), "NO_CONVERGENCE", "Maximum number of iterations reached", 0, [], True),
    "max_iter1": (dict(max_num_iterations=1), "NO_CONVERGENCE", "Maximum number of iterations reached", 1, [1.0], False),
    "max_iter2": (dict(max_num_iterations=2), "NO_CONVERGENCE", "Maximum number of iterations reached", 2, [1.0, 1.0],
                  False),
    "gradient": (dict(gradient_tolerance=1e30), "CONVERGENCE", "Gradient tolerance reached", 0, [], True),
    "min_radius": (dict(min_trust_region_radius=1e5), "CONVERGENCE", "Minimum trust region radius reached", 0, [], True),
    "parameter": (dict(parameter_tolerance=1e30), "CONVERGENCE", "Parameter tolerance reached", 1, [-1.0], True),
    "function": (dict(function_tolerance=1e30), "CONVERGENCE", "Function tolerance reached", 1, [-1.0], True),
    "max_radius": (dict(max_trust_region_radius=2e4, max_num_iterations=2), "NO_CONVERGENCE",
                   "Maximum number of iterations reached", 2, [1.0, 1.0], False),
}


@pytest.mark.parametrize("reason", sorted(TERMINATIONS))
@pytest.mark.parametrize("name", WINDOWS)
def test_termination_reasons(name, reason):
    opts, term, kind, iters, flags, same = TERMINATIONS[reason]
    kw = dict(max_num_iterations=5, initial_trust_region_radius=1e4)
    kw.update(opts)
    sg, log, qg, so, tr, qo = run_sequence(name, **kw)
    assert sg["termination"] == term and sg["message"].startswith(kind), sg
    assert sg["num_iterations"] == iters and log[1:, 6].tolist() == flags, (sg, log[:, 6])
    assert unchanged(qg, name) == same and unchanged(qo, name) == same
    if reason == "max_radius":
        assert log[:, 5].tolist() == [1e4, 2e4, 2e4]  # 3 r clamped, then held at the clamp
    if reason == "max_iter1":
        assert log[:, 5].tolist() == [1e4, 3e4]
