"""tests/refresid.py, the reference of the residual report, checked on the CPU: its cost against the oracle's, its
rounding constants measured again, the gap condition that keeps every flag of the GPU tests decidable, and the cull
loop on the oracle.

Measured here: the reference's total cost and oracle.solve's initial / final cost agree to 4e-15 relative at worst;
float64 against longdouble: du / dv 1.75e-13 px, depth - z and z 9.3e-16, obs_cost 1.5e-3 of itself (a nearly
vanishing residual, see refresid.cost_bound); the nearest reference value to a threshold, against GAP: 3 px 4.9e-4
against 2.9e-9 (nb37_b2_f32 start), depth test 2.6e-5 against 1.5e-11 (spans start), Huber boundaries 5.9e-6 px against
2.9e-9 (gauge_only solved) and 8.4e-8 against 1.5e-11 (spans start), z 0.74 against 1.5e-11.
Cull loop (bcr21_messy, spans, short400): 28 / 37 / 26 observations flagged, then none; final cost 3.50e-2 -> 2.41e-2,
3.64e-2 -> 2.18e-2, 2.76e-2 -> 1.69e-2.
"""
import numpy as np
import pytest

import refresid
from refresid import LD

CASES = [(n, w) for n in refresid.WINDOWS for w in refresid.PARAM_SETS]


@pytest.mark.parametrize("name", refresid.WINDOWS)
def test_cost_equals_oracle(name):
    """Sum obs_cost + prior_cost is the oracle's cost at the start and at its solution, to 1e-12 relative."""
    s = refresid.solved(name).meta["oracle_summary"]
    for which, want in (("start", s["initial_cost"]), ("solved", s["final_cost"])):
        ref = refresid.reference(name, which)
        got = float(ref.total_cost)
        print(f"REFCOST {name} {which} ref={got:.15e} oracle={want:.15e} rel={abs(got - want) / want:.1e}")
        assert abs(got - want) <= 1e-12 * want
        # the block statistics and the totals are the same observations
        for st in (ref.cam_stats, ref.point_stats):
            assert st[:, 0].sum() == ref.n_admissible and st[:, 1].sum() == ref.n_outliers
            assert abs(st[:, 5].sum() + ref.prior_cost - ref.total_cost) <= 1e-17 * float(ref.total_cost) * len(st)


def test_rounding_constants():
    """MEASURED_GAP covers the float64 evaluation on every window and parameter set, without slack to spare (the
    constants are the measurement, rounded up), and the tolerances keep the condition of the issue."""
    worst = dict(uv=0.0, dd=0.0, z=0.0, cost=0.0)
    for name, which in CASES:
        g = refresid.rounding_gap(refresid.params(name, which))
        for k in worst:
            worst[k] = max(worst[k], g[k])
    print("ROUNDING", {k: f"{v:.3e}" for k, v in worst.items()}, "constants", refresid.MEASURED_GAP)
    for k, v in worst.items():
        assert v <= refresid.MEASURED_GAP[k], (k, v)
        assert refresid.MEASURED_GAP[k] <= 1.25 * v, (k, v, "the constant is no longer the measurement")
    assert refresid.TOL["uv"] < 1e-9
    assert all(refresid.TOL[k] == 16.0 * refresid.MEASURED_GAP[k] for k in worst)
    assert all(refresid.GAP[k] == 1000.0 * refresid.TOL[k] for k in worst)


@pytest.mark.parametrize("name,which", CASES)
def test_cost_bound_covers_f64(name, which):
    """cost_bound with the measured gaps in place of the tolerances covers the float64 evaluation's cost."""
    p = refresid.params(name, which)
    a = refresid.evaluate(p, dtype=np.float64)
    b = refresid.evaluate(p, dtype=LD)
    m = b.adm
    bound = refresid.cost_bound(b, e_uv=refresid.MEASURED_GAP["uv"], e_dd=refresid.MEASURED_GAP["dd"])
    assert (np.abs(a.cost[m].astype(LD) - b.cost[m]) <= bound[m]).all()


@pytest.mark.parametrize("name,which", CASES)
def test_gap_condition(name, which):
    """No reference value lies within GAP of a threshold the GPU tests use: 3 px, the depth test, both Huber
    boundaries, z = 0."""
    p = refresid.params(name, which)
    ref = refresid.reference(name, which)
    g = refresid.threshold_gaps(ref, p)
    print(f"GAPS {name} {which} " + " ".join(f"{k}={v:.2e}" for k, v in g.items()))
    assert g["reproj"] > refresid.GAP["uv"] and g["huber_repr"] > refresid.GAP["uv"]
    assert g["depth"] > refresid.GAP["dd"] and g["huber_unpr"] > refresid.GAP["dd"]
    assert g["z"] > refresid.GAP["z"]
    assert ref.n_behind == 0


def test_flags_and_nan_of_inadmissible():
    p = refresid.window("bcr21_messy")
    ref = refresid.reference("bcr21_messy", "start")
    bad = p.obs_depth <= 1e-15
    assert 0 < bad.sum() < p.n_obs and ref.n_admissible == int((~bad).sum())
    assert (ref.flags[bad] == refresid.INADMISSIBLE).all() and not (ref.flags[~bad] & refresid.INADMISSIBLE).any()
    assert np.isnan(ref.err[bad]).all() and np.isnan(ref.cost[bad]).all()
    assert np.array_equal(ref.depth_culled != p.obs_depth, (ref.flags & refresid.OUTLIER) != 0)
    # most observations of the perturbed start are beyond 3 px; about 2 % at the solution
    assert ref.n_reproj > 0.8 * ref.n_admissible
    assert 0 < refresid.reference("bcr21_messy", "solved").n_reproj < 0.04 * ref.n_admissible


def test_behind_camera_reference():
    """z < 0 (a point mirrored through a camera centre) and z = 0 (a point on it): BA_RES_BEHIND, counted, out of
    the sums."""
    thr = (refresid.MAX_REPROJ_PX, refresid.MAX_DEPTH_ABS, refresid.MAX_DEPTH_REL)
    base = refresid.evaluate(refresid.window("one2"), None, *thr)
    mir, k, pt = refresid.behind_case("mirror")
    r = refresid.evaluate(mir, None, *thr)
    assert r.flags[k] & refresid.BEHIND and r.err[k, 3] < 0 and r.n_behind >= 1
    # the mirrored point projects to the same pixel (x / z is unchanged)
    assert np.abs(r.err[k, :2] - base.err[k, :2]).max() < 1e-9
    on, k0, pt0 = refresid.behind_case("on")
    assert (k0, pt0) == (k, pt)
    r0 = refresid.evaluate(on, None, *thr)
    assert r0.flags[k] & refresid.BEHIND and r0.err[k, 3] == 0 and not np.isfinite(r0.err[k, 0])
    assert r0.cam_stats[1, 0] == base.cam_stats[1, 0] and np.isfinite(r0.cam_stats[1, 2:5].astype(np.float64)).all()
    # the gap condition of these two windows (the observation on the camera centre has no finite value to compare)
    for prob, ref, mask in ((mir, r, None), (on, r0, np.arange(on.n_obs) != k)):
        g = refresid.threshold_gaps(ref, prob, mask=mask)
        print("GAPS behind " + " ".join(f"{n}={v:.2e}" for n, v in g.items()))
        assert g["reproj"] > refresid.GAP["uv"] and g["huber_repr"] > refresid.GAP["uv"]
        assert g["depth"] > refresid.GAP["dd"] and g["huber_unpr"] > refresid.GAP["dd"]
        assert g["z"] > refresid.GAP["z"]


@pytest.mark.parametrize("name,flagged", zip(refresid.CULL_WINDOWS, (28, 37, 26)))
def test_cull_loop_on_oracle(name, flagged):
    c = refresid.oracle_cull_loop(name)
    print(f"CULL {name} flagged={c.flagged} final_cost={[s['final_cost'] for s in c.summaries]}")
    assert c.flagged == [flagged, 0]
    assert [s["termination_type"] for s in c.summaries] == [0, 0]  # BA_CONVERGENCE
    assert c.culled.sum() == flagged
    assert c.summaries[1]["final_cost"] < 0.75 * c.summaries[0]["final_cost"]
    assert c.report.n_outliers == 0 and float(c.report.max_reproj_px) < 3.0
    assert c.summaries[1]["num_obs_admissible"] == c.summaries[0]["num_obs_admissible"] - flagged
