"""synthetic.make_sweep_problem (windows whose co-visibility is not a narrow band) and, on the two sweep windows of the
wide-window GPU tests, the step references against each other and against the oracle: test_refstep.py's rule, so
test_gpu_blocked.py never runs against a window on which reference and oracle disagree."""
import numpy as np
import pytest

import refstep
import refsweep
from miba import synthetic


def _spans(p):
    hi = np.full(p.n_points, -1, np.int64)
    lo = np.full(p.n_points, p.n_cams, np.int64)
    np.maximum.at(hi, p.obs_pt, p.obs_cam)
    np.minimum.at(lo, p.obs_pt, p.obs_cam)
    return hi - lo


def test_seeded_and_repeatable():
    kw = dict(n_cams=24, n_points=200, obs_per_pass=4, passes=2)
    a = synthetic.make_sweep_problem(seed=5, **kw)
    b = synthetic.make_sweep_problem(seed=5, **kw)
    c = synthetic.make_sweep_problem(seed=6, **kw)
    for k in ("cams", "points", "intr", "intr_prior", "obs_cam", "obs_pt", "obs_uv", "obs_depth"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert not np.array_equal(a.obs_uv, c.obs_uv) and not np.array_equal(a.cams, c.cams)
    np.testing.assert_array_equal(a.obs_cam, c.obs_cam)  # the structure does not depend on the seed
    assert a.fixed_cam == 0 and len(a.obs_cam) == 200 * 2 * 4


def test_sensor_f32_values():
    p = synthetic.make_sweep_problem(24, 200, 4, 2, seed=5, sensor_f32=True)
    np.testing.assert_array_equal(p.obs_uv, p.obs_uv.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(p.obs_depth, p.obs_depth.astype(np.float32).astype(np.float64))


def test_n_cams_must_split_into_passes():
    with pytest.raises(ValueError):
        synthetic.make_sweep_problem(25, 100, 4, 2)


@pytest.mark.parametrize("n_cams,opp,passes", [(22, 4, 2), (42, 5, 2), (50, 5, 2), (200, 5, 2), (60, 4, 3)])
def test_wide_covisibility(n_cams, opp, passes):
    p = synthetic.make_sweep_problem(n_cams, 12 * n_cams, opp, passes, seed=n_cams)
    band = refstep.camera_band(p)
    m = n_cams // passes
    print(f"SWEEP {n_cams} cams, {passes} x {opp}: camera band {band}, min span {_spans(p).min()}")
    assert band >= 10
    # about n_cams (1 - 1 / passes): a run of opp cameras on the first and on the last sweep
    assert m * (passes - 1) <= band <= m * (passes - 1) + opp
    assert (_spans(p) > 12).all()  # every point is an overflow point of the Schur tiles
    assert (p.obs_depth > 0).all()
    cnt = np.bincount(p.obs_pt, minlength=p.n_points)
    assert (cnt == passes * opp).all()
    assert len(np.unique(p.obs_cam)) == n_cams
    assert len(np.unique(np.round(p.meta["truth"]["cams"], 12), axis=0)) == n_cams  # no two cameras coincide


@pytest.mark.parametrize("name", sorted(refsweep.SWEEPS))
def test_references_and_oracle_agree(name):
    p, ref, orc, accepted = refsweep.reference(name)
    assert refstep.camera_band(p) >= 10 and (_spans(p) > 12).all() and (p.obs_depth > 0).all()
    q = refstep.qr_step(p, None, 1e4)
    err = refstep.rel_err(q, ref)
    print(f"REF {name} cond={ref.cond:.3g} qr-schur {err}")
    assert max(err.values()) <= 1e-12, err
    assert abs(q.model_cost_change - ref.model_cost_change) <= 1e-13 * abs(ref.model_cost_change)
    tol = refstep.step_tol(ref.cond)
    e_orc = refstep.rel_err(orc, ref)
    print(f"ORACLE {name} nac={len(ref.ac_cam)} npad={refsweep.npad(p)} tol={tol:.2e} err {e_orc}")
    assert max(e_orc.values()) <= tol, (e_orc, tol)
    assert abs(orc["model_cost_change"] - ref.model_cost_change) <= tol * ref.model_cost_change
    assert accepted == 1


def test_sweep_window_sizes():
    assert refsweep.npad(refsweep.window("sweep22")) == 144
    assert refsweep.npad(refsweep.window("sweep42")) == 256
