"""tests/refconst.py, the step reference under constant cameras: its two routes (dense QR of the stacked problem, the
Schur complement) against each other within step_tol, as tests/test_refstep.py holds refstep's, and a one-camera mask
against the same camera as ``fixed_cam``."""
import numpy as np
import pytest

import refconst
import refstep


@pytest.mark.parametrize("name", refconst.MASK_NAMES)
def test_qr_and_schur_routes_agree_under_a_mask(name):
    p, mask, sch = refconst.case("small", name)
    qr = refconst.qr_step(p, mask, None, 1e4)
    tol = refstep.step_tol(sch.cond)
    err = refstep.rel_err(qr, sch)
    print(f"REFCONST small/{name} nac={len(sch.ac_cam)} cond={sch.cond:.3g} tol={tol:.2e} err={err}")
    adm = p.obs_depth > 1e-15
    seen = np.zeros(p.n_cams, bool)
    seen[p.obs_cam[adm]] = True
    want = [c for c in range(p.n_cams) if seen[c] and not mask[c] and c != p.fixed_cam]
    assert sch.ac_cam.tolist() == want and sch.delta_cam.shape == (len(want), 6)
    assert max(err.values()) <= tol, (err, tol)
    assert abs(qr.model_cost_change - sch.model_cost_change) <= tol * abs(sch.model_cost_change)
    assert sch.model_cost_change > 0


@pytest.mark.parametrize("g", [0, 3, 5])
def test_one_camera_mask_is_fixed_cam(g):
    base = refconst.window("small")
    a = base.copy()
    a.fixed_cam = g
    ref = refstep.schur_step(a, None, 1e4)
    b = base.copy()
    b.fixed_cam = -1
    mask = np.zeros(base.n_cams, bool)
    mask[g] = True
    got = refconst.schur_step(b, mask, None, 1e4)
    tol = refstep.step_tol(ref.cond)
    assert max(refstep.rel_err(got, ref).values()) <= tol
    assert abs(got.cond - ref.cond) <= 1e-6 * ref.cond
    S0, r0, _ = refconst.reduced_system(a, np.zeros(base.n_cams, bool), None, 1e4)
    S1, r1, _ = refconst.reduced_system(b, mask, None, 1e4)
    np.testing.assert_allclose(S1, S0, rtol=0, atol=tol * np.abs(S0).max())
    np.testing.assert_allclose(r1, r0, rtol=0, atol=tol * np.abs(r0).max())


def test_covariance_of_the_masked_system_is_its_inverse():
    p, mask, _ = refconst.case("small", "middle")
    import refcov
    ref = refconst.schur_cov(p, mask)
    assert ref.red.shape == (6 * len(ref.ac_cam) + 4,) * 2 and not mask[ref.ac_cam].any()
    # against the inverse of refconst's own undamped reduced system, in parameter units
    S, _, L = refconst.reduced_system(p, mask, None, float("inf"))
    s = np.concatenate([L.s_c.ravel(), L.s_k]).astype(np.float64)
    inv = np.linalg.inv(S) * s[:, None] * s[None, :]
    assert refcov.pair_errors(inv, ref.red) <= refstep.step_tol(ref.cond)
