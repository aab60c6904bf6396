"""The Schur reduction at its tile, chunk and overflow boundaries (windows and references: tests/refschur.py).

The step tests pin the reduced solve; these pin the stage before it — the plan's point classes, tiles and chunks and
the kernels that consume them (k_point_prep / k_lin_point, the Schur tiles in every variant, k_schur_gather,
k_obs_pairs, k_obs_pairs_det, k_backsub_chunk, the camera side) — on windows sculpted to sit on TILE_WIN = 12,
CHUNK_PTS = 32, CHUNK_OBS = 256, every used row-tile count of the 80-row M', K = 3 npts of the MFMA product not a
multiple of 4, BS_OBS = 1024 and n_tiles = 0. Every run sets MIBA_TILE_PTS (the plan's own value depends on the
device's resident slots), so refschur.geometry states the plan of the run exactly.

* Step runs: test_gpu_step.run_prepared with all its assertions (retried == 0, flag == 0, window unmodified, cameras /
  intrinsics / points / rho within tol = 8 cond(S) eps, the oracle's decision, the oracle under the same tol), at
  radius 1e4 and 1e-2 (tol about 6e-12: a wrong low-order term of the Schur update shows). Every window on the default
  path; the variant windows under MIBA_FUSED=0, MIBA_SW=0, MIBA_SW=2, MIBA_FPL=1 + MIBA_SW=0, MIBA_XCD_MAP=0,
  MIBA_SUBSEG=64, a one-rank communicator with shard_min_obs = 0, deterministic = 1, and MIBA_PP_LANES 1, 2, 4 (read
  once per process: one child process per value); short400 over the MIBA_TILE_PTS list; spans / holes / spans_f32 with
  one point per tile (every tile span 1 .. 12).
* Deterministic mode repeats bitwise and agrees with the atomic mode to tol.
* MIBA_DEVICE_PLAN=0 and =1 give equal plan digests on every window.
* The assembled system: Solver.reduced_system against refschur.schur_system in
  e = max_ij |S - S_ref|_ij / sqrt(S_ref,ii S_ref,jj) (rhs: / sqrt(S_ref,ii)), bound 8 max(e of the f64 oracle,
  m eps), m the longest camera sum of the window, computed from the oracle at run time.
* The camera side at MIBA_SUBSEG=64 with MIBA_XCD_MAP 0 and 1 against np.longdouble sums, 1e-11.

Measured (MI355X). Steps: err = the largest of the three groups, gpu = the largest over the runs of that window:

  window        radius  cond(S)   tol       oracle    gpu (max)  tr_ratio  runs
  spans         10000   1.43e+06  2.5e-09   3.2e-12   1.4e-12    4.8e-16   17
  spans         0.01    3.34e+03  5.9e-12   1.0e-15   1.9e-13    4.4e-16   17
  holes         10000   1.38e+06  2.5e-09   3.3e-12   2.6e-12    3.6e-16   14
  holes         0.01    3.71e+03  6.6e-12   1.6e-15   1.9e-13    6.6e-16   14
  dup_active    10000   1.43e+06  2.5e-09   4.1e-12   1.9e-12    2.4e-16   12
  dup_active    0.01    3.34e+03  5.9e-12   3.1e-15   1.0e-13    6.6e-16   12
  dup_gauge     10000   1.43e+06  2.5e-09   6.3e-12   1.5e-12    0.0e+00   1
  dup_gauge     0.01    3.34e+03  5.9e-12   2.5e-15   1.0e-13    4.4e-16   1
  obs256        10000   1.43e+06  2.5e-09   5.5e-12   3.9e-12    8.4e-16   12
  obs256        0.01    3.42e+03  6.1e-12   2.1e-15   1.7e-13    2.2e-16   12
  obs257        10000   1.43e+06  2.5e-09   7.8e-12   4.3e-12    1.1e-15   15
  obs257        0.01    3.42e+03  6.1e-12   2.4e-15   1.1e-13    2.2e-16   15
  chunk_cut     10000   1.42e+06  2.5e-09   6.9e-12   3.7e-12    6.0e-16   12
  chunk_cut     0.01    3.32e+03  5.9e-12   6.6e-16   1.2e-13    0.0e+00   12
  bs_long       10000   1.57e+06  2.8e-09   1.9e-11   9.2e-12    7.3e-16   12
  bs_long       0.01    4.31e+03  7.7e-12   8.4e-16   9.4e-14    2.6e-15   12
  all_overflow  10000   1.40e+06  2.5e-09   5.2e-12   4.5e-12    2.4e-16   1
  all_overflow  0.01    3.18e+03  5.7e-12   2.2e-15   9.9e-14    2.2e-16   1
  gauge_only    10000   1.44e+06  2.6e-09   5.6e-12   9.1e-13    0.0e+00   1
  gauge_only    0.01    3.77e+03  6.7e-12   3.1e-15   8.5e-14    2.2e-16   1
  short400      10000   1.30e+06  2.3e-09   1.1e-11   1.4e-11    3.5e-16   31
  short400      0.01    4.64e+03  8.3e-12   2.5e-15   2.4e-13    4.4e-16   31
  spans_f32     10000   1.43e+06  2.5e-09   4.9e-13   1.3e-12    2.4e-16   5
  spans_f32     0.01    3.34e+03  5.9e-12   2.6e-15   9.5e-14    6.6e-16   5

The assembled system (gpu = the larger of the atomic and the deterministic mode; bound = 8 max(oracle, m eps)):

  window        radius  m eps     S oracle  S bound   S gpu      rhs oracle  rhs bound  rhs gpu
  spans         10000   3.9e-14   3.9e-13   3.1e-12   3.4e-13    1.1e-15     3.1e-13    1.2e-15
  spans         3       3.9e-14   1.0e-15   3.1e-13   1.5e-14    7.5e-17     3.1e-13    7.8e-16
  holes         10000   3.4e-14   3.9e-13   3.1e-12   4.2e-13    2.4e-15     2.7e-13    1.4e-15
  holes         3       3.4e-14   1.1e-15   2.7e-13   1.8e-14    4.5e-17     2.7e-13    9.3e-16
  dup_active    10000   3.9e-14   5.0e-13   4.0e-12   2.2e-13    1.6e-15     3.1e-13    1.1e-15
  dup_active    3       3.9e-14   1.3e-15   3.1e-13   1.6e-14    9.0e-17     3.1e-13    7.7e-16
  dup_gauge     10000   3.9e-14   9.3e-13   7.4e-12   2.0e-13    2.6e-15     3.1e-13    1.1e-15
  dup_gauge     3       3.9e-14   1.3e-15   3.1e-13   1.6e-14    9.0e-17     3.1e-13    7.7e-16
  obs256        10000   3.9e-14   3.4e-13   2.7e-12   1.4e-13    4.5e-15     3.1e-13    1.1e-15
  obs256        3       3.9e-14   1.1e-15   3.1e-13   1.6e-14    9.9e-17     3.1e-13    7.8e-16
  obs257        10000   3.9e-14   5.7e-13   4.6e-12   2.6e-13    4.5e-15     3.1e-13    2.0e-15
  obs257        3       3.9e-14   1.6e-15   3.1e-13   1.6e-14    2.2e-16     3.1e-13    7.5e-16
  chunk_cut     10000   3.9e-14   5.1e-13   4.1e-12   3.9e-13    1.8e-15     3.1e-13    1.5e-15
  chunk_cut     3       3.9e-14   1.3e-15   3.1e-13   1.5e-14    1.5e-16     3.1e-13    7.5e-16
  bs_long       10000   5.7e-14   3.3e-12   2.6e-11   2.7e-12    1.9e-14     4.6e-13    3.2e-15
  bs_long       3       5.7e-14   6.7e-15   4.6e-13   1.5e-14    5.9e-16     4.6e-13    1.0e-15
  all_overflow  10000   4.2e-14   7.0e-13   5.6e-12   4.3e-13    1.6e-15     3.4e-13    1.1e-15
  all_overflow  3       4.2e-14   1.2e-15   3.4e-13   1.4e-14    1.2e-16     3.4e-13    7.3e-16
  gauge_only    10000   2.7e-14   9.2e-14   7.4e-13   3.5e-13    2.2e-15     2.2e-13    4.1e-16
  gauge_only    3       2.7e-14   6.5e-16   2.2e-13   6.2e-15    7.2e-17     2.2e-13    2.6e-16
  short400      10000   2.4e-14   3.3e-13   2.6e-12   3.9e-13    5.6e-16     1.9e-13    1.5e-15
  short400      3       2.4e-14   1.1e-15   1.9e-13   1.3e-15    8.4e-17     1.9e-13    2.2e-16
  spans_f32     10000   3.9e-14   2.5e-13   2.0e-12   2.7e-13    2.3e-15     3.1e-13    1.1e-15
  spans_f32     3       3.9e-14   1.6e-15   3.1e-13   1.5e-14    7.5e-17     3.1e-13    7.7e-16

What these tests found. With every kernel left to contract the residual's multiply-adds as its context suggested,
test_reduced_system missed its bound at radius 1e4 on spans (3.2e-12), holes (4.2e-12), obs256 (3.8e-12), spans_f32
(2.9e-12) and gauge_only (9.0e-13), in both modes, and the intrinsics step of the windows built from `spans` carried
2e-10 in every variant (inside tol). Observation 244 of `spans` (camera 6, point 35) has a residual of 0.0019 from
pixel coordinates near 220, so its Huber corrector amplifies the rounding of u - uo to about 2e-13; the camera-side
and the point-side kernels rounded it 2.3e-13 apart, and its two terms (U_cc, C_ck against W V^-1 W^T) nearly cancel
in S because the point hangs on that observation: S - S_ref in camera 6's blocks was that observation's camera-side
term times 2.3e-13 (cosine 0.96 and 0.99998). obs_project / obs_residual (ba_device.h) now fix the sequence of
operations for every kernel; the figures above are with them. The largest entry of the S metric sits in the
intrinsics block S_kk, which sums over all admissible observations and cancels about 2000-fold at radius 1e4: the
oracle itself is at 2 .. 60 m eps there.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import refschur
import refstep
from refstep import NO_TOL
from test_gpu_step import run_prepared, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(refschur.WINDOWS)
RADII = refschur.RADII


def tile_env(name, tile_pts=None):
    return {"MIBA_TILE_PTS": str(tile_pts or refschur.DEFAULT_TILE_PTS[name])}


def run(monkeypatch, name, radius, env=None, opts=None, comm=False, tag="", tile_pts=None):
    e = tile_env(name, tile_pts)
    e.update(env or {})
    return run_prepared(monkeypatch, name, refschur.reference(name, radius), radius, e, opts, comm,
                        f"{tag} tile_pts={e['MIBA_TILE_PTS']}")


# ---------------------------------------------------------------------------------------- the default path
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", ALL)
def test_default_path(name, radius, monkeypatch):
    g, info = run(monkeypatch, name, radius, tag="default")
    assert len(g["ac_cam"]) == refschur.window(name).n_cams - 1


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", ["spans", "holes", "spans_f32"])
def test_one_point_per_tile(name, radius, monkeypatch):
    """MIBA_TILE_PTS=1: every tile span from 1 to 12 — every used row-tile count of M' (they change at spans 1|2, 4|5,
    7|8, 9|10 and 12) — and K = 3."""
    geo = refschur.geometry(refschur.window(name), 1, 256)
    assert set(geo["tile_span"]) == set(range(1, 13)) and len(geo["tile_base"]) == geo["n_tiled"]
    run(monkeypatch, name, radius, tag="tile1", tile_pts=1)
    run(monkeypatch, name, radius, env={"MIBA_SW": "0"}, tag="tile1_sw0", tile_pts=1)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("sw", ["1", "0"])
@pytest.mark.parametrize("tile_pts", refschur.TILE_PTS)
def test_short400_tile_pts(tile_pts, sw, radius, monkeypatch):
    """Several chunks per tile and last chunks of 1, 2, 3, 5 points (K = 3, 6, 9, 15), in the small-window launch
    and in k_schur_tile."""
    run(monkeypatch, "short400", radius, env={"MIBA_SW": sw}, tag=f"sw{sw}", tile_pts=tile_pts)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("layout", ["obs32", "f64"])
def test_observation_layouts(layout, radius, monkeypatch):
    run(monkeypatch, "spans_f32", radius, env={} if layout == "obs32" else {"MIBA_OBS32": "0"}, tag=layout)


# ---------------------------------------------------------------------------------------- variants
VARIANTS = {
    # name: (env, options, communicator, expected prepare info)
    "fused0": ({"MIBA_FUSED": "0"}, {}, False, {"lin_path": 0, "tail": 0}),
    "sw0": ({"MIBA_SW": "0"}, {}, False, {"lin_path": 0}),
    "sw2": ({"MIBA_SW": "2"}, {}, False, {"lin_path": 1}),
    "fpl1": ({"MIBA_FPL": "1", "MIBA_SW": "0"}, {}, False, {"lin_path": 0}),
    "xcd0": ({"MIBA_XCD_MAP": "0"}, {}, False, {}),
    "subseg64": ({"MIBA_SUBSEG": "64"}, {}, False, {}),
    "comm1": ({}, {"shard_min_obs": 0}, True, {"tail": 0}),
    "det": ({}, {"deterministic": 1}, False, {"lin_path": 0, "tail": 0}),
}


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", refschur.VARIANT_WINDOWS)
def test_variants(name, variant, radius, monkeypatch):
    env, opts, comm, want = VARIANTS[variant]
    if variant == "sw2":  # the launch is taken wherever it fits one resident round, by the restated geometry
        geo = refschur.geometry(refschur.window(name), refschur.DEFAULT_TILE_PTS[name], 256)
        assert len(geo["tile_base"]) > 0 and refschur.sw_launch_blocks(geo) <= 256
    g, info = run(monkeypatch, name, radius, env=env, opts=opts, comm=comm, tag=variant)
    for k, v in want.items():
        assert info[k] == v, (k, info)


_PP_CHILD = r"""
import pickle, sys
root = sys.argv[1]
sys.path[:0] = [root, root + "/3dsmc-bundle-adjustment_amd", root + "/tests"]
import refschur
from test_gpu_step import run_prepared
with open(sys.argv[2], "rb") as f:
    refs = pickle.load(f)
for (name, radius), (ref, orc, accepted) in refs.items():
    env = {"MIBA_TILE_PTS": str(refschur.DEFAULT_TILE_PTS[name])}
    run_prepared(None, name, (refschur.window(name), ref, orc, accepted), radius, env, tag="pp_lanes=" + sys.argv[3])
print("pp_lanes child: ok")
"""


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_pp_lanes(lanes, tmp_path):
    """MIBA_PP_LANES (lanes per point of k_point_prep / k_lin_point: counts that no lane count divides) is read once
    per process, so each value runs the variant windows at both radii in a process of its own; the references go to
    it in a file."""
    refs = {(n, r): refschur.reference(n, r)[1:] for n in refschur.VARIANT_WINDOWS for r in RADII}
    path = str(tmp_path / "refs.pkl")
    with open(path, "wb") as f:
        pickle.dump(refs, f)
    r = subprocess.run([sys.executable, "-c", _PP_CHILD, ROOT, path, str(lanes)],
                       env=dict(os.environ, MIBA_PP_LANES=str(lanes)), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert r.stdout.count("STEP ") == len(refs) and "pp_lanes child: ok" in r.stdout


# ---------------------------------------------------------------------------------------- deterministic mode
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name,tile_pts", [("spans", 16), ("obs257", 16), ("short400", 3)])
def test_deterministic_repeats_and_agrees_with_atomic(name, tile_pts, radius, monkeypatch):
    """The per-tile slabs, k_schur_gather and k_obs_pairs_det (short400 at MIBA_TILE_PTS=3: many tiles whose windows
    overlap)."""
    a, _ = run(monkeypatch, name, radius, opts={"deterministic": 1}, tag="det", tile_pts=tile_pts)
    b, _ = run(monkeypatch, name, radius, opts={"deterministic": 1}, tag="det_repeat", tile_pts=tile_pts)
    assert same_bits(a, b)
    assert a["tr_ratio"] == b["tr_ratio"] and a["cost"] == b["cost"]
    c, _ = run(monkeypatch, name, radius, tag="atomic", tile_pts=tile_pts)
    tol = refstep.step_tol(refschur.reference(name, radius)[1].cond)
    assert max(refstep.rel_err(a, c).values()) <= tol


# ---------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("name", ALL)
def test_device_plan_matches_the_host_plan(name, monkeypatch):
    """bs_long's 1040-observation point takes the device plan's workgroup sort of long lists."""
    from miba.solver import Solver
    monkeypatch.setenv("MIBA_TILE_PTS", str(refschur.DEFAULT_TILE_PTS[name]))
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MIBA_DEVICE_PLAN", mode)
        with Solver(minimizer_progress_to_stdout=0, rebuild_plan=1, **NO_TOL) as s:
            s.prepare(refschur.window(name).copy())
            out[mode] = (s.plan_digest(), s.last_prepare()["plan_device"])
    print(f"PLAN {name} plan_device: MIBA_DEVICE_PLAN=0 -> {out['0'][1]}, =1 -> {out['1'][1]}")
    assert out["0"][1] == 0
    assert len(out["0"][0]) == len(out["1"][0]) > 0
    assert out["0"][0] == out["1"][0]


# ---------------------------------------------------------------------------------------- the assembled system
@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("mode", ["atomic", "det"])
@pytest.mark.parametrize("name", ALL)
def test_reduced_system(name, mode, radius, monkeypatch):
    """S and rhs of the scale + build launches against the extended-precision reference. The bound comes from the
    f64 oracle's own error in the same metric and the longest camera sum, never from the GPU's result. (Solver and
    oracle hold the gradient side: S y = -rhs.)"""
    from miba.solver import Solver
    from oracle import oracle
    p = refschur.window(name)
    monkeypatch.setenv("MIBA_TILE_PTS", str(refschur.DEFAULT_TILE_PTS[name]))
    S_ref, rhs_ref = refschur.schur_system(p, None, radius)
    So, ro = oracle.reduced_system(p, oracle.default_options(), radius)
    with Solver(minimizer_progress_to_stdout=0, deterministic=int(mode == "det")) as s:
        S, rhs = s.reduced_system(p.copy(), radius)
    assert S.shape == S_ref.shape
    o_s, o_r = refschur.system_err(So, -ro, S_ref, rhs_ref)
    g_s, g_r = refschur.system_err(S, -rhs, S_ref, rhs_ref)
    meps = refschur.longest_camera_sum(p) * refschur.EPS64
    print(f"SYS {name} radius={radius:g} {mode} m_eps={meps:.1e} oracle_S={o_s:.1e} gpu_S={g_s:.1e} "
          f"oracle_rhs={o_r:.1e} gpu_rhs={g_r:.1e}")
    assert g_s <= 8 * max(o_s, meps), (g_s, o_s, meps)
    assert g_r <= 8 * max(o_r, meps), (g_r, o_r, meps)


# ---------------------------------------------------------------------------------------- the camera side
def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("xcd", ["0", "1"])
@pytest.mark.parametrize("name", ["spans", "bs_long", "short400"])
def test_camera_side_sums(name, xcd, monkeypatch):
    """test_gpu_parity's camera-side sums at MIBA_SUBSEG=64 (several sub-segments per camera, near-equal cuts) with
    and without the XCD map, the reference accumulated in np.longdouble; 1e-11 (summation order only)."""
    from miba.solver import Solver
    from oracle import oracle
    LD = np.longdouble
    p = refschur.window(name)
    for k, v in {"MIBA_SUBSEG": "64", "MIBA_XCD_MAP": xcd, **tile_env(name)}.items():
        monkeypatch.setenv(k, v)
    with Solver(minimizer_progress_to_stdout=0) as s:
        g = s.camera_sums(p.copy())
    r = oracle.linearize(p)
    jc, jk, f = r["jcam"].astype(LD), r["jint"].astype(LD), r["res"].astype(LD)
    adm = p.obs_depth > 1e-15
    geo = refschur.geometry(p, refschur.DEFAULT_TILE_PTS[name], 64)
    assert list(g["ac_cam"]) == geo["ac_cam"]
    assert max(b - a for a, b in zip(geo["ac_seg"][0::2], geo["ac_seg"][1::2])) >= 2  # several sub-segments
    worst = 0.0
    for a, cam in enumerate(g["ac_cam"]):
        m = adm & (p.obs_cam == cam)
        U = np.einsum("nri,nrj->ij", jc[m], jc[m]).astype(np.float64)
        Cc = np.einsum("nri,nrm->im", jc[m, :2], jk[m]).astype(np.float64)
        gg = np.einsum("nri,nr->i", jc[m], f[m]).astype(np.float64)
        e = max(_rel(g["U"][a], U), _rel(g["C"][a], Cc), _rel(g["g"][a], gg))
        worst = max(worst, e)
        assert e <= 1e-11, (name, cam, e)
    w = LD(oracle.default_options().weight_intrinsics)
    Ukk = (np.einsum("nrm,nrl->ml", jk[adm], jk[adm]) + w * np.eye(4, dtype=LD)).astype(np.float64)
    gk = (np.einsum("nrm,nr->m", jk[adm], f[adm, :2]) - w * (p.intr_prior.astype(LD) - p.intr.astype(LD))).astype(np.float64)
    e_k = max(_rel(g["lin"][2:12], Ukk[np.triu_indices(4)]), _rel(g["lin"][12:16], gk))
    print(f"CAMSIDE {name} xcd={xcd} segs={len(geo['seg_cam'])} cams={worst:.1e} intr={e_k:.1e}")
    assert e_k <= 1e-11
    assert abs(g["lin"][0] - r["cost"]) <= 1e-12 * r["cost"]
