"""The step references (tests/refstep.py) against each other and against the oracle, on the CPU.

qr_step (dense QR of the stacked least-squares problem) and schur_step (point elimination in extended precision)
share only the oracle's per-observation Jacobians and the restated scaling / damping; where both can run they must
agree far below the tolerance the GPU tests use. oracle_lm_step (f64 Schur complement + Cholesky, what oracle.solve
steps with) must agree with the reference within tol = 8 cond(S) eps on EVERY window of the GPU matrix, so
test_gpu_step.py never runs against a window on which reference and oracle disagree."""
import numpy as np
import pytest

import refstep
from oracle import oracle

QR_WINDOWS = ["one1", "one2", "one10", "nb17_b3", "bcr11", "bcr21", "gauge_mid21", "inactive_mid21", "bcr21_messy"]


QR_CASES = [(n, 1e4) for n in QR_WINDOWS] + [(n, r) for n in ("bcr21", "one2", "bcr21_messy") for r in (1e-2, 1e12)]


@pytest.mark.parametrize("name,radius", QR_CASES)
def test_qr_and_schur_references_agree(name, radius):
    p = refstep.window(name)
    q = refstep.qr_step(p, None, radius)
    s = refstep.schur_step(p, None, radius)
    err = refstep.rel_err(q, s)
    print(f"REF {name} radius={radius:g} cond={s.cond:.3g} qr-schur {err}")
    # both are extended-precision refinements of f64 factorizations: they agree to ~eps_f64 * small, not to tol
    assert max(err.values()) <= 1e-12, err
    assert abs(q.model_cost_change - s.model_cost_change) <= 1e-13 * abs(s.model_cost_change)
    assert s.model_cost_change > 0


@pytest.mark.parametrize("name,radius", refstep.all_references())
def test_oracle_step_within_tol_of_reference(name, radius):
    p, ref, orc, accepted = refstep.reference(name, radius)
    tol = refstep.step_tol(ref.cond)
    err = refstep.rel_err(orc, ref)
    print(f"ORACLE {name} radius={radius:g} nac={len(ref.ac_cam)} cond={ref.cond:.3g} tol={tol:.2e} "
          f"err cams={err['cams']:.1e} intr={err['intr']:.1e} pts={err['pts']:.1e}")
    assert max(err.values()) <= tol, (err, tol)
    assert abs(orc["model_cost_change"] - ref.model_cost_change) <= tol * ref.model_cost_change
    assert accepted == 1
    # inactive points do not move
    adm_pts = np.unique(p.obs_pt[p.obs_depth > 1e-15])
    mask = np.ones(p.n_points, bool)
    mask[adm_pts] = False
    assert not orc["delta_pts"][mask].any() and not ref.delta_pts[mask].any()


def test_window_active_counts():
    """The windows reach the edges their names say: active cameras, camera band."""
    for n in refstep.BCR_COUNTS:
        assert len(refstep.reference(f"bcr{n}")[1].ac_cam) == n
    for n in refstep.ONE_BLOCK_COUNTS:
        assert len(refstep.reference(f"one{n}")[1].ac_cam) == n
    for n, b in refstep.NARROW:
        p, ref = refstep.reference(f"nb{n}_b{b}")[:2]
        assert len(ref.ac_cam) == n
        assert refstep.camera_band(p) == b
    assert refstep.camera_band(refstep.window("full31")) == 9
    p, ref = refstep.reference("inactive_mid21")[:2]
    assert len(ref.ac_cam) == 21 and 12 not in ref.ac_cam and 0 not in ref.ac_cam
    assert 11 not in refstep.reference("gauge_mid21")[1].ac_cam
    assert 21 not in refstep.reference("gauge_last21")[1].ac_cam
