"""The references of tests/refcand.py against each other and against the oracle, and the conditions of the windows
that test_gpu_candidate.py runs (CPU only): which branch of the retraction each camera's first step takes, which Huber
zone the blocks are in. Every bound that test_gpu_candidate.py asserts for the GPU is asserted here for the oracle's
own float64 result, so it is shown to hold for a correct implementation."""
import numpy as np
import pytest

import refcand
import refstep
from oracle import oracle
from refcand import LD

THETA_GRID = [0.0, 1e-12, 1e-10 * (1 - 1e-6), 1e-10 * (1 + 1e-6), 1e-5, 0.5, 1 - 1e-12, 1 + 1e-12, 2.0, np.pi - 1e-9,
              np.pi, 4.0]


def _poses(theta, n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        q = rng.normal(size=4)
        ax = rng.normal(size=3)
        yield (np.concatenate([q / np.linalg.norm(q), 3.0 * rng.normal(size=3)]),
               np.concatenate([rng.normal(size=3), ax / np.linalg.norm(ax) * theta]))


@pytest.mark.parametrize("theta", THETA_GRID)
def test_retractions_agree_and_oracle_within_bound(theta):
    worst = 0.0
    for T, d in _poses(theta, 25, 11):
        q, t = refcand.retract_quat(T, d)
        R, t2 = refcand.retract_mat(T, d)
        worst = max(worst, float(np.abs(refcand.quat_R(q) - R).max()), float(np.abs(t - t2).max()))
        eq, et = refcand.retraction_error(oracle.se3_plus(T, d), T, d)
        bq, bt = refcand.retraction_bound(T, d, cancelling_a=True)
        assert eq <= bq and et <= bt, (theta, eq, bq, et, bt)
    print(f"RETRACT theta={theta:g} two forms differ by {worst:.1e}")
    assert worst <= 1e-17


def test_series_threshold_is_continuous():
    """Just below / above theta^2 = 1e-8 the series and the closed forms give the same pose."""
    for T, d in _poses(1.0, 5, 3):
        w = d[3:] / np.linalg.norm(d[3:])
        lo = refcand.retract_quat(T, np.concatenate([d[:3], w * 1e-4 * (1 - 1e-9)]))
        hi = refcand.retract_quat(T, np.concatenate([d[:3], w * 1e-4 * (1 + 1e-9)]))
        assert float(np.abs(lo[0] - hi[0]).max()) <= 1e-12 and float(np.abs(lo[1] - hi[1]).max()) <= 1e-12


CASES = ([("bcr21", 1e4), ("nb37_b2", 1e4), ("one10", 1e4), ("bc_L7", 1e4), ("dense_wide30", 1e4), ("roll21", 1e4),
          ("roll_nb37", 1e4), ("bcr21_f32", 1e4), ("nb37_b2_f32", 1e4), ("bcr21_messy", 1e4), ("nb37_b2_messy", 1e4)]
         + [(n, r) for n in ("bcr21", "nb37_b2") for r in refcand.SMALL_RADII]
         + [(n, refcand.HUBER_RADIUS) for n in sorted(refcand.HUBER)])


@pytest.mark.parametrize("name,radius", CASES)
def test_oracle_within_every_bound(name, radius):
    """The oracle's cost at x, its candidate (retraction of its own step), the candidate's cost, cost_change, the
    norms and the gradient max-norm, each within the bound the GPU is held to."""
    r = refcand.reference(name, radius)
    p, tr = r.prob, r.trace
    assert r.accepted == 1 and r.summary["num_iterations"] == 1
    oe = r.oracle_errors()
    for k, (err, bound) in oe.items():
        assert err <= bound, (k, err, bound)
    q = r.orc_x  # accepted: the oracle's parameters are its candidate
    _, ac, pt = refcand.active_blocks(p)
    assert np.array_equal(ac, r.orc["ac_cam"])
    inactive = np.setdiff1d(np.arange(p.n_cams), ac)
    assert np.array_equal(q.cams[inactive], p.cams[inactive]) and np.array_equal(q.points[~pt], p.points[~pt])
    assert np.array_equal(q.intr, p.intr + r.orc["delta_intr"])
    assert np.array_equal(q.points, p.points + r.orc["delta_pts"])
    # the decision's arithmetic from the oracle's own rho
    rho = tr[1][4]
    assert abs(tr[1][5] - min(1e16, radius / max(1 / 3, 1 - (2 * rho - 1) ** 3))) <= 4 * refstep.EPS64 * tr[1][5]
    print(f"ORACLE {name} radius={radius:g} " + " ".join(f"{k}={e / b:.1e}" for k, (e, b) in oe.items())
          + " (fractions of the bound)")


@pytest.mark.parametrize("name", sorted(refcand.ROLLS))
def test_rolled_windows_reach_the_sincos_branch(name):
    r = refcand.reference(name, 1e4)
    assert (r.theta >= 1.0).sum() >= 1 and ((r.theta >= 0.5) & (r.theta < 1.0)).sum() >= 1, np.sort(r.theta)[-3:]
    d = refcand.cost(r.prob, r.okw, detail=True)
    assert float(d["z"].min()) > 0  # a roll about the optical axis keeps every depth positive
    assert (r.theta < 0.1).sum() >= len(r.theta) - 2  # the other cameras stay on the polynomial branch's usual range


@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_small_radii_reach_the_small_angle_branch(name):
    a, b = (refcand.reference(name, rad) for rad in refcand.SMALL_RADII)
    assert (a.theta < 1e-10).sum() >= 1 and (a.theta >= 1e-10).sum() >= 1, np.sort(a.theta)
    assert (b.theta < 1e-10).all() and b.theta.min() >= 1e-12, np.sort(b.theta)
    # the candidate quaternions move by >= 1e-13: the branch's result is visible in float64
    for r in (a, b):
        _, ac, _ = refcand.active_blocks(r.prob)
        move = np.abs(r.cand[0][ac, :4] - refcand._ld(r.prob.cams[ac, :4])).max(1)
        assert float(move.min()) >= 1e-13
        assert r.accepted == 1  # cost_change ~ 5e-9 .. 5e-10 > 0: no tolerance ends the step at tolerances 0


@pytest.mark.parametrize("name", sorted(refcand.HUBER))
def test_huber_windows_hold_both_zones(name):
    r = refcand.reference(name, refcand.HUBER_RADIUS)
    for where, par in (("x", ()), ("candidate", r.cand)):
        fr, fd = refcand.zone_fractions(r.prob, r.okw, *par)
        assert 0.25 <= fr <= 0.75 and 0.25 <= fd <= 0.75, (where, fr, fd)
    if "edge_r" in r.info:
        d = refcand.cost(r.prob, r.okw, detail=True)
        for key, norm, a in (("edge_r", d["nr"], r.okw["hub_p_repr"]), ("edge_d", d["nd"], r.okw["hub_p_unpr"])):
            above, below = (float(norm[j] / LD(a) - 1) for j in r.info[key])
            assert 0 < above <= 1e-12 and -1e-12 <= below < 0, (key, above, below)
