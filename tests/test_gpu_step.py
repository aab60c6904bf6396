"""The LM step of every reduced-solve path against a high-precision reference (tests/refstep.py).

``Solver.lm_step`` (ba_debug_step) enqueues what ba_solve_prepared enqueues for iteration zero and the first LM
iteration and returns the step the production kernels computed: the Schur right-hand side and the reduced solve
(k_chol, k_chol_band<1..6>, the per-level BCR launches, k_bcr_persist, k_bcr_split with one or two helpers,
k_bcr_dense1, k_bcr_band / k_band_tail), the camera and intrinsics step (cam_step / intr_step in k_update_cams,
k_bcr_border and the resident kernels) and the point back-substitution (k_backsub_chunk, k_backsub_final, the tail's
chunks). Every case asserts

  * the path it names (last_prepare() and the hook's linear_solver / camera_band / band_tiles), retried == 0 and a
    zero factorisation flag, and that the window was not modified;
  * per group (cameras, intrinsics, points) max-norm error / max-norm of the reference <= tol;
  * the GPU's tr_ratio == its own cost_change / the reference's model cost change, to tol;
  * the decision (accepted) is the oracle's.

tol = 8 cond(S) eps_f64, cond(S) the 2-norm condition of the scaled, damped reduced system from the reference: the
forward-error bound of a backward-stable solve of that system, the 8 for the different summation order and the f64
atomics. The oracle's own step (oracle_lm_step) is asserted under the same tol in the same test, so the bound is
shown to hold for a correct solver.

Measured (MI355X; err = the largest of the three groups; gpu = the largest over the paths run on that window):

  window           radius  cond(S)   tol       oracle    gpu (max)  tr_ratio  runs
  bcr11            10000   1.46e+06  2.6e-09   1.4e-12   5.4e-12    5.9e-16   4
  bcr19            10000   1.41e+06  2.5e-09   1.1e-12   5.0e-12    1.2e-16   4
  bcr20            10000   1.33e+06  2.4e-09   2.6e-12   5.0e-12    2.9e-15   4
  bcr21            10000   1.33e+06  2.3e-09   6.1e-12   4.3e-12    3.6e-16   13
  bcr30            10000   1.29e+06  2.3e-09   2.5e-12   1.3e-11    2.4e-16   4
  bcr31            10000   1.30e+06  2.3e-09   3.2e-12   4.7e-11    3.6e-16   4
  bcr41            10000   1.27e+06  2.3e-09   8.6e-12   2.1e-11    5.9e-16   4
  bcr79            10000   1.16e+06  2.1e-09   1.5e-12   9.5e-12    1.2e-16   4
  bcr80            10000   1.13e+06  2.0e-09   4.0e-12   4.3e-11    1.4e-15   4
  bcr81            10000   1.15e+06  2.0e-09   1.2e-11   1.3e-11    3.6e-16   4
  bcr21            1e+12   1.58e+06  2.8e-09   9.7e-12   9.7e-12    1.2e-16   4
  bcr21            0.01    2.57e+03  4.6e-12   2.4e-15   2.4e-13    1.5e-15   4
  bcr81            1e+12   1.47e+06  2.6e-09   7.3e-12   1.2e-11    3.6e-16   4
  bcr81            0.01    1.69e+03  3.0e-12   3.1e-15   2.0e-13    8.8e-16   4
  full31           10000   1.32e+06  2.3e-09   3.3e-12   2.1e-11    8.3e-16   4
  gauge_mid21      10000   1.37e+06  2.4e-09   2.0e-11   1.9e-11    3.5e-16   4
  gauge_last21     10000   1.37e+06  2.4e-09   2.8e-12   2.2e-12    5.9e-16   4
  inactive_mid21   10000   1.32e+06  2.3e-09   5.5e-12   5.6e-12    3.5e-16   4
  one1             10000   1.06e+06  1.9e-09   5.7e-12   5.5e-12    3.5e-16   3
  one2             10000   1.29e+06  2.3e-09   8.5e-12   7.7e-12    3.6e-16   3
  one9             10000   1.27e+06  2.2e-09   6.5e-11   7.4e-12    2.4e-16   3
  one10            10000   1.27e+06  2.3e-09   2.4e-11   1.8e-11    9.5e-16   3
  nb2_b1           10000   1.03e+06  1.8e-09   3.8e-11   5.5e-12    6.0e-16   4
  nb9_b2           10000   1.24e+06  2.2e-09   2.5e-11   2.8e-11    4.7e-16   4
  nb10_b3          10000   1.30e+06  2.3e-09   3.2e-12   8.9e-12    1.4e-15   4
  nb17_b3          10000   1.27e+06  2.2e-09   8.5e-12   9.3e-12    5.9e-16   4
  nb37_b2          10000   1.06e+06  1.9e-09   2.3e-12   2.9e-12    2.4e-16   13
  nb49_b1          10000   1.06e+06  1.9e-09   4.3e-11   1.5e-11    2.3e-16   4
  nb49_b3          10000   1.11e+06  2.0e-09   4.3e-12   1.1e-11    8.3e-16   4
  nb51_b3          10000   1.11e+06  2.0e-09   6.8e-12   2.1e-12    2.4e-16   4
  nb64_b2          10000   1.11e+06  2.0e-09   1.8e-12   4.3e-12    2.4e-16   4
  nb99_b1          10000   1.03e+06  1.8e-09   5.9e-12   8.5e-12    4.7e-16   4
  bc_L2            10000   1.13e+06  2.0e-09   8.6e-12   6.7e-12    1.2e-16   1
  bc_L4            10000   1.20e+06  2.1e-09   2.5e-11   1.2e-10    1.1e-15   1
  bc_L7            10000   1.27e+06  2.2e-09   1.1e-11   1.3e-11    0.0e+00   1
  bc_L10           10000   1.31e+06  2.3e-09   1.0e-12   2.5e-12    1.2e-16   1
  bc_L13           10000   1.37e+06  2.4e-09   3.4e-12   3.1e-12    8.3e-16   1
  bc_L16           10000   1.36e+06  2.4e-09   4.8e-12   1.3e-11    7.1e-16   1
  dense_wide30     10000   1.37e+06  2.4e-09   2.8e-12   7.3e-12    8.4e-16   1
  dense_n160       10000   1.41e+06  2.5e-09   2.7e-12   2.2e-12    1.2e-16   1
  bcr21_f32        10000   1.33e+06  2.3e-09   1.0e-11   2.9e-12    2.4e-16   2
  nb37_b2_f32      10000   1.06e+06  1.9e-09   8.3e-13   2.0e-12    1.2e-16   2
  bcr21_messy      10000   1.33e+06  2.4e-09   2.8e-12   2.8e-12    1.2e-16   1
  nb37_b2_messy    10000   1.08e+06  1.9e-09   1.4e-11   3.0e-11    2.3e-16   1
"""
import os

import numpy as np
import pytest

import refstep
from refstep import NO_TOL

pytestmark = pytest.mark.gpu

LS = {"dense": 0, "band": 1, "bcr": 2}
BCR_MODES = {"launch": 0, "persist": 1, "split": 2, "split3": 3}


def run_step(monkeypatch, name, radius=1e4, env=None, opts=None, comm=False, tag=""):
    """lm_step of window ``name`` under ``env`` / ``opts``, checked against the reference; returns (step, prepare
    info)."""
    return run_prepared(monkeypatch, name, refstep.reference(name, radius), radius, env, opts, comm, tag)


def run_prepared(monkeypatch, name, prepared, radius=1e4, env=None, opts=None, comm=False, tag=""):
    """run_step on a prepared (window, schur_step, oracle.lm_step, the oracle's decision) — the tuple of
    refstep.reference; ``name`` labels the printed line. Without ``monkeypatch`` (a child process) ``env`` goes
    into os.environ."""
    from miba.solver import Solver
    for k, v in (env or {}).items():
        if monkeypatch is None:
            os.environ[k] = v
        else:
            monkeypatch.setenv(k, v)
    p, ref, orc, accepted = prepared
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
    print(f"STEP {name} radius={radius:g} {tag} bcr_path={info['bcr_path']} ls={g['linear_solver']} "
          f"tail={info['tail']} lin_path={info['lin_path']} bsfin={info['bsfin']} cond={ref.cond:.3g} tol={tol:.2e} "
          f"oracle={max(e_orc.values()):.1e} gpu_cams={e_gpu['cams']:.1e} gpu_intr={e_gpu['intr']:.1e} "
          f"gpu_pts={e_gpu['pts']:.1e} rho={e_rho:.1e}")
    assert g["retried"] == 0 and g["flag"] == 0 and g["num_iterations"] == 1, g
    assert max(e_orc.values()) <= tol, (e_orc, tol)
    assert max(e_gpu.values()) <= tol, (e_gpu, tol)
    assert e_rho <= tol, (g["tr_ratio"], rho_ref, tol)
    want = 0 if (opts or {}).get("min_relative_decrease", 0) >= 1e3 else accepted
    assert g["accepted"] == want, g
    assert g["tr_radius"] > 0 and g["step_norm"] > 0
    return g, info


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ac_cam", "delta_cam", "delta_intr", "delta_pts"))


# ---------------------------------------------------------------------------------------- block cyclic reduction
@pytest.mark.parametrize("mode", sorted(BCR_MODES))
@pytest.mark.parametrize("nac", refstep.BCR_COUNTS)
def test_bcr_block_boundaries(nac, mode, monkeypatch):
    """Blocks of 10 active cameras: partial last blocks of 1 and 9 cameras, full ones, non-power-of-two trees."""
    g, info = run_step(monkeypatch, f"bcr{nac}", env={"MIBA_BCR": mode}, tag=mode)
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == BCR_MODES[mode], (g, info)
    assert len(g["ac_cam"]) == nac


@pytest.mark.parametrize("mode", sorted(BCR_MODES))
@pytest.mark.parametrize("radius", [1e12, 1e-2])
@pytest.mark.parametrize("nac", [21, 81])
def test_bcr_radii(nac, radius, mode, monkeypatch):
    """Almost no damping (Gauss-Newton) and heavy damping."""
    g, info = run_step(monkeypatch, f"bcr{nac}", radius, env={"MIBA_BCR": mode}, tag=mode)
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == BCR_MODES[mode], (g, info)


@pytest.mark.parametrize("mode", sorted(BCR_MODES))
def test_bcr_full_width_coupling(mode, monkeypatch):
    """Tracks of exactly 10 cameras: camera band 9, every off-diagonal block dense."""
    g, info = run_step(monkeypatch, "full31", env={"MIBA_BCR": mode}, tag=mode)
    assert g["camera_band"] == 9 and g["linear_solver"] == LS["bcr"] and info["bcr_path"] == BCR_MODES[mode]


@pytest.mark.parametrize("mode", sorted(BCR_MODES))
@pytest.mark.parametrize("name", ["gauge_mid21", "gauge_last21", "inactive_mid21"])
def test_bcr_gauge_and_activity(name, mode, monkeypatch):
    """The gauge camera in the middle / last, and a middle camera without admissible observations: the active index
    map shifts."""
    g, info = run_step(monkeypatch, name, env={"MIBA_BCR": mode}, tag=mode)
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == BCR_MODES[mode]
    assert len(g["ac_cam"]) == 21


ONE_BLOCK_ENV = {"dense1": {"MIBA_BCR_BAND": "0"}, "split": {"MIBA_BCR_BAND": "0", "MIBA_BCR_DENSE1": "0"},
                 "band": {}}


@pytest.mark.parametrize("path", sorted(ONE_BLOCK_ENV))
@pytest.mark.parametrize("nac", refstep.ONE_BLOCK_COUNTS)
def test_one_block_windows(nac, path, monkeypatch):
    """One 64-dof block: k_bcr_dense1, the split kernel, the band solve with its tail (the default from 2 active
    cameras on; one active camera takes k_bcr_dense1)."""
    g, info = run_step(monkeypatch, f"one{nac}", env=ONE_BLOCK_ENV[path], tag=path)
    want = {"dense1": 4, "split": 3, "band": 5 if nac >= 2 else 4}[path]
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == want, (g, info)
    assert len(g["ac_cam"]) == nac
    if path == "band" and nac >= 2:
        assert info["tail"] == 1 and info["lin_path"] == 1, info


# ---------------------------------------------------------------------------------------- narrow band, bcr_path 5
@pytest.mark.parametrize("sw", ["1", "0"])
@pytest.mark.parametrize("tail", ["1", "0"])
@pytest.mark.parametrize("nac,band", refstep.NARROW)
def test_narrow_band(nac, band, tail, sw, monkeypatch):
    """The one-workgroup band solve (k_bcr_band / k_band_tail) at band 1, 2, 3, with and without the tail launch and
    the small-window Schur launch."""
    env = {"MIBA_TAIL": tail, "MIBA_SW": sw}
    if nac <= 10:
        env["MIBA_BCR_BAND"] = "2"  # one-block windows without the tail default to k_bcr_dense1
    g, info = run_step(monkeypatch, f"nb{nac}_b{band}", env=env, tag=f"tail{tail}_sw{sw}")
    assert g["linear_solver"] == LS["bcr"] and info["bcr_path"] == 5 and g["camera_band"] == band, (g, info)
    assert info["tail"] == int(tail), info
    if sw == "0":
        assert info["lin_path"] == 0, info
    elif nac <= 17 and (tail == "1" or nac <= 10):  # (these fit one resident round of the Schur launch by far)
        assert info["lin_path"] == 1, info


# ---------------------------------------------------------------------------------------- band / dense Cholesky
@pytest.mark.parametrize("tiles,track", list(enumerate(refstep.BANDCHOL_TRACKS, start=1)))
def test_band_cholesky(tiles, track, monkeypatch):
    """k_chol_band<BW> for BW = 1 .. 6 (tracks of 2, 4, 7, 10, 13, 16 cameras: every instantiation is reached)."""
    name = f"bc_L{track}"
    assert refstep.band_tiles(refstep.window(name)) == tiles
    g, info = run_step(monkeypatch, name, env={"MIBA_SOLVER": "band"}, tag=f"bw{tiles}")
    assert g["linear_solver"] == LS["band"] and g["band_tiles"] == tiles and info["bcr_path"] == -1, (g, info)


@pytest.mark.parametrize("name,n", [("dense_wide30", 178), ("dense_n160", 160)])
def test_dense_cholesky(name, n, monkeypatch):
    """k_chol on wide tracks (overflow points), n a multiple of 16 and not."""
    g, info = run_step(monkeypatch, name, env={"MIBA_SOLVER": "dense"}, tag="dense")
    assert g["linear_solver"] == LS["dense"] and info["bcr_path"] == -1 and 6 * len(g["ac_cam"]) + 4 == n


# ---------------------------------------------------------------------------------------- variants
VARIANTS = {
    # name: (env on the BCR window, env on the band window, options, expected prepare info)
    "sw2": ({"MIBA_SW": "2"}, {"MIBA_SW": "2"}, {}, {"lin_path": 1}),
    "fpl1": ({"MIBA_FPL": "1"}, {"MIBA_FPL": "1", "MIBA_SW": "0"}, {}, {"lin_path": 0}),
    "fused0": ({"MIBA_FUSED": "0"}, {"MIBA_FUSED": "0"}, {}, {"lin_path": 0, "tail": 0}),
    "bsfin1": ({"MIBA_BSFIN": "1"}, {"MIBA_BSFIN": "1", "MIBA_TAIL": "0"}, {}, {"bsfin": 1, "tail": 0}),
    "comm1": ({}, {}, {"shard_min_obs": 0}, {"tail": 0}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_variants(name, variant, monkeypatch):
    """The linearisation / back-substitution variants and the landmark-sharded path on a 1-rank communicator."""
    e_bcr, e_band, opts, want = VARIANTS[variant]
    g, info = run_step(monkeypatch, name, env=e_bcr if name == "bcr21" else e_band, opts=opts,
                       comm=variant == "comm1", tag=variant)
    assert g["linear_solver"] == LS["bcr"] and (info["bcr_path"] == 5) == (name == "nb37_b2"), (g, info)
    for k, v in want.items():
        assert info[k] == v, (k, info)


@pytest.mark.parametrize("name", ["bcr21", "nb37_b2"])
def test_deterministic_and_rejected_step(name, monkeypatch):
    """deterministic = 1 meets tol and repeats bitwise; a rejected step (min_relative_decrease = 1e3) is the same
    step, bitwise, with accepted = 0; the default mode's rejected step meets tol too."""
    a, _ = run_step(monkeypatch, name, opts={"deterministic": 1}, tag="det")
    b, _ = run_step(monkeypatch, name, opts={"deterministic": 1}, tag="det_repeat")
    assert same_bits(a, b)
    assert a["tr_ratio"] == b["tr_ratio"] and a["cost"] == b["cost"]
    r, _ = run_step(monkeypatch, name, opts={"deterministic": 1, "min_relative_decrease": 1e3}, tag="det_rejected")
    assert r["accepted"] == 0 and a["accepted"] == 1
    assert same_bits(a, r)
    assert r["tr_ratio"] == a["tr_ratio"] and r["cost_change"] == a["cost_change"]
    d, _ = run_step(monkeypatch, name, opts={"min_relative_decrease": 1e3}, tag="rejected")
    assert d["accepted"] == 0


@pytest.mark.parametrize("layout", ["obs32", "f64"])
@pytest.mark.parametrize("name", ["bcr21_f32", "nb37_b2_f32"])
def test_observation_layouts(name, layout, monkeypatch):
    """float32-valued pixels and depths take the 16-byte observation records; MIBA_OBS32=0 keeps the f64 arrays."""
    run_step(monkeypatch, name, env={} if layout == "obs32" else {"MIBA_OBS32": "0"}, tag=layout)


@pytest.mark.parametrize("name", ["bcr21_messy", "nb37_b2_messy"])
def test_duplicates_bad_depths_shuffled(name, monkeypatch):
    g, info = run_step(monkeypatch, name, tag="default")
    assert (info["bcr_path"] == 5) == (name == "nb37_b2_messy"), info
