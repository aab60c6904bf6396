"""ba_covariance (Solver.covariance) against the extended-precision Schur reference of tests/refcov.py.

Every value case compares EVERY pair of blocks (cameras x cameras, cameras x intrinsics, intrinsics x intrinsics, the
gauge and inactive cameras included), the ``full`` matrix and EVERY point against refcov.schur_cov under

    pair (a, b):  max|delta| / sqrt(max|S_aa| max|S_bb|)  <=  tol        point:  max|delta| / max|S_pp|  <=  tol

tol = refstep.step_tol(cond) = 8 cond eps_f64, cond the 2-norm condition of the scaled, undamped reduced matrix (the
forward-error bound of a backward-stable inverse of that matrix; test_refcov.py shows the references themselves agree
four orders of magnitude below it).

The dense inverse works in blocks of 64 (ba_cov.hip); the windows are refstep.WINDOWS, each the smallest that reaches
its edge: one1 (n = 10, less than a 16-tile, one active camera, points seen by the gauge camera only), one2 (n = 16),
one10 (n = 64, exactly one block), bcr11 (n = 70, a second block of 6 rows), bcr21 (n = 130, the intrinsics rows
straddle 128), dense_n160 (a multiple of 16 but not of 64, tracks up to 16), full31 (dense coupling), nb37_b2_f32
(obs32 records, band path, n = 226), bcr81 (n = 490), gauge_mid21 / gauge_last21 (active-index mapping, zero blocks),
inactive_mid21 (camera 12 and the points only it sees are NaN), bcr21_messy (duplicates, bad depths) and cov200
(refcov.WINDOWS: n = 1204, the C4 benchmark's reduced size, 19 block columns).

Measured (MI355X): cond 1.1e6 .. 1.6e6, tol 2.0e-9 .. 2.9e-9; the largest error over all pairs / all points per window
is 1.4e-13 / 4.3e-13 (one1) .. 2.9e-11 / 4.2e-11 (full31, cov200); jacobi_scaling = 0 on bcr21: 6.5e-12 / 7.0e-12.
Free-gauge systems: smallest pivot -1.8e-16 (one2) and -1.8e-14 (bcr21) -> rank deficient; gauged: pivot ratio
2.1e-6 and 1.7e-6 -> OK at min_rcond = 1e-9.
"""
import ctypes as C

import numpy as np
import pytest

import refcov
import refstep

pytestmark = pytest.mark.gpu

INTR = -1
VALUE_WINDOWS = ["one1", "one2", "one10", "bcr11", "bcr21", "dense_n160", "full31", "nb37_b2_f32", "bcr81",
                 "gauge_mid21", "gauge_last21", "inactive_mid21", "bcr21_messy", "cov200"]


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def all_pairs(p):
    ids = list(range(p.n_cams)) + [INTR]
    return [(a, b) for a in ids for b in ids]


def unchanged(q, p):
    for a in ("cams", "points", "intr", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"covariance modified prob.{a}")


def check_values(name, g, p, ref, tol=None, tag=""):
    """Every pair, ``full`` and every point of the result ``g`` (all pairs, all points, full requested) against the
    reference; the exactness conditions."""
    tol = refstep.step_tol(ref.cond) if tol is None else tol
    assert g["status"] == 0, g["status"]
    assert list(g["ac_cam"]) == list(ref.ac_cam)
    nac = len(ref.ac_cam)
    assert g["nac"] == nac and g["n"] == 6 * nac + 4
    ac_of = {int(c): t for t, c in enumerate(ref.ac_cam)}
    blocks = dict(zip(g["pairs"], g["pair_cov"]))
    off = lambda v: 6 * nac if v == INTR else 6 * ac_of[v]
    dim = lambda v: 4 if v == INTR else 6
    assembled = np.full((6 * nac + 4, 6 * nac + 4), np.nan)
    for (a, b), blk in blocks.items():
        # (a, b) and (b, a) are exact transposes; a diagonal block is exactly symmetric
        assert np.array_equal(blk, blocks[(b, a)].T, equal_nan=True), (a, b)
        gauge = p.fixed_cam in (a, b) and p.fixed_cam >= 0
        inactive = any(v != INTR and v != p.fixed_cam and v not in ac_of for v in (a, b))
        if inactive:
            assert np.isnan(blk).all(), (a, b, "a camera without an admissible observation is NaN")
        elif gauge:
            assert (blk == 0).all(), (a, b, "a pair with the gauge camera is a zero block")
        else:
            assembled[off(a): off(a) + dim(a), off(b): off(b) + dim(b)] = blk
    # the blocks are the blocks of ``full``, bit for bit
    assert np.array_equal(assembled, g["full"]), "pair blocks differ from full"
    ep = refcov.pair_errors(g["full"], ref.red)
    ex = refcov.point_errors(g["point_cov"], ref.pts)
    print(f"COV {name} {tag} n={g['n']} cond={ref.cond:.3g} tol={tol:.2e} pairs={ep:.1e} points={ex:.1e} "
          f"pivots={g['pivot_min']:.2e}/{g['pivot_max']:.2e} build={g['time_build_ms']:.2f}ms "
          f"invert={g['time_invert_ms']:.2f}ms points={g['time_points_ms']:.2f}ms")
    assert ep <= tol, (ep, tol)
    assert ex <= tol, (ex, tol)
    pc = g["point_cov"]
    assert np.array_equal(pc, pc.transpose(0, 2, 1), equal_nan=True), "a point block is exactly symmetric"
    return ep, ex


def run_cov(name, monkeypatch=None, env=None, tag="", **opts):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    p, ref = refcov.reference(name)
    q = p.copy()
    with solver(**opts) as s:
        g = s.covariance(q, pairs=all_pairs(q), points=True, full=True)
        info = s.last_prepare()
    unchanged(q, p)
    check_values(name, g, p, ref, tag=tag)
    return g, info


@pytest.mark.parametrize("name", VALUE_WINDOWS)
def test_values(name):
    g, _ = run_cov(name)
    if name == "inactive_mid21":
        # (check_values asserted the NaN blocks of camera 12; the window's tracks of 4 to 9 cameras leave no point
        # that only camera 12 sees: test_inactive_point covers a point without an admissible observation)
        p = refcov.window(name)
        only12 = np.ones(p.n_points, bool)
        only12[p.obs_pt[(p.obs_cam != 12)]] = False
        assert np.isnan(g["point_cov"][only12]).all()
        assert not np.isnan(g["point_cov"][~only12]).any()
    if name == "one1":
        assert g["nac"] == 1


def test_inactive_point():
    """A point whose observations are all inadmissible is NaN; everything else matches the reference of that window."""
    p = refcov.window("one2").copy()
    p.obs_depth[p.obs_pt == 5] = 0.0
    ref = refcov.schur_cov(p)
    assert np.isnan(ref.pts[5]).all() and not np.isnan(np.delete(ref.pts, 5, 0)).any()
    q = p.copy()
    with solver(deterministic=1) as s:
        g = s.covariance(q, pairs=all_pairs(q), points=True, full=True)
        one = s.covariance(q, pairs=[], points=[5, 6])
    unchanged(q, p)
    check_values("one2", g, p, ref, tag="point 5 inactive")
    assert np.isnan(g["point_cov"][5]).all()
    assert np.isnan(one["point_cov"][0]).all() and np.array_equal(one["point_cov"][1], g["point_cov"][6])


def test_default_request():
    """Default pairs: every active camera's diagonal block plus the intrinsics block; no points."""
    p, ref = refcov.reference("gauge_mid21")
    with solver() as s:
        g = s.covariance(p.copy())
    nac = len(ref.ac_cam)
    assert g["pairs"] == [(int(c), int(c)) for c in ref.ac_cam] + [(INTR, INTR)]
    assert len(g["point_cov"]) == 0
    tol = refstep.step_tol(ref.cond)
    for t, blk in enumerate(g["pair_cov"]):
        o, d = (6 * nac, 4) if t == nac else (6 * t, 6)
        r = ref.red[o: o + d, o: o + d]
        assert np.abs(blk - r).max() / np.abs(r).max() <= tol


@pytest.mark.parametrize("name,env,path", [("bcr21", {"MIBA_BCR": "launch"}, 0), ("bcr21", {"MIBA_BCR": "persist"}, 1),
                                           ("bcr21", {"MIBA_BCR": "split"}, 2), ("nb10_b3", {}, 5)])
def test_every_path_s(name, env, path, monkeypatch):
    """The covariance does not depend on the reduced-solve path the window was prepared for."""
    g, info = run_cov(name, monkeypatch, env=env, tag=str(env))
    assert info["bcr_path"] == path, info


def _bits(g):
    return [g["full"], g["point_cov"]] + list(g["pair_cov"])


def test_deterministic_and_no_damping():
    p, ref = refcov.reference("bcr21")
    out = []
    for radius in (1e4, 1e4, 3.0):
        with solver(deterministic=1, initial_trust_region_radius=radius) as s:
            out.append(s.covariance(p.copy(), pairs=all_pairs(p), points=True, full=True))
    with solver(deterministic=1) as s:  # two calls on one context
        a = s.covariance(p.copy(), pairs=all_pairs(p), points=True, full=True)
        b = s.covariance(p.copy(), pairs=all_pairs(p), points=True, full=True)
    for g in (out[1], out[2], a, b):
        for x, y in zip(_bits(out[0]), _bits(g)):
            assert np.array_equal(x, y, equal_nan=True)
    check_values("bcr21", out[0], p, ref, tag="deterministic")


def test_no_jacobi_scaling():
    """jacobi_scaling = 0: the unscaled system is inverted; the covariance is the same."""
    p, ref = refcov.reference("bcr21")
    with solver(deterministic=1, jacobi_scaling=0) as s:
        g = s.covariance(p.copy(), pairs=all_pairs(p), points=True, full=True)
    check_values("bcr21", g, p, ref, tag="jacobi_scaling=0")


@pytest.mark.parametrize("name", ["bcr21", "one10"])
def test_no_side_effect(name):
    """solve on a fresh context == covariance followed by solve on another, bit for bit."""
    p = refcov.window(name)
    q0, q1 = p.copy(), p.copy()
    with solver(deterministic=1) as s:
        s0 = s.solve(q0)
        log0 = s.iteration_log()
    with solver(deterministic=1) as s:
        s.covariance(q1, points=True)
        unchanged(q1, p)
        s1 = s.solve(q1)
        log1 = s.iteration_log()
    for a in ("cams", "points", "intr"):
        assert np.array_equal(getattr(q0, a), getattr(q1, a)), a
    assert np.array_equal(log0, log1)
    for k, v in s0.items():
        if not k.startswith("time_"):
            assert s1[k] == v, (k, v, s1[k])
    assert s0["num_iterations"] >= 1


@pytest.mark.parametrize("name", ["one2", "bcr21"])
def test_rank_deficiency(name):
    p = refcov.window(name)
    free = p.copy()
    free.fixed_cam = -1
    with solver() as s:
        g = s.covariance(free, pairs=all_pairs(free), points=True, full=True, min_rcond=1e-9)
        ok = s.covariance(p.copy(), pairs=all_pairs(p), points=True, full=True, min_rcond=1e-9)
    print(f"RANK {name} free gauge: status={g['status']} pivots={g['pivot_min']:.3e}/{g['pivot_max']:.3e}; "
          f"gauged: status={ok['status']} ratio={ok['pivot_min'] / ok['pivot_max']:.2e}")
    assert g["status"] == 1
    assert np.isnan(g["full"]).all() and np.isnan(g["point_cov"]).all()
    assert all(np.isnan(b).all() for b in g["pair_cov"])
    assert ok["status"] == 0 and not np.isnan(ok["full"]).any()


def test_errors():
    from miba.capi import BaCovInfo, BaCovRequest
    from miba.solver import MibaError, Solver
    p = refcov.window("one2")
    with solver() as s:
        for kw in (dict(pairs=[(0, p.n_cams)]), dict(pairs=[(-2, 0)]), dict(points=[p.n_points]), dict(points=[-1])):
            with pytest.raises(MibaError, match=r"\(-1\).*out of range"):
                s.covariance(p.copy(), **kw)
        q = p.copy()  # (kept alive: the struct holds bare pointers into its arrays)
        ps = q.struct()
        req, info = BaCovRequest(), BaCovInfo()
        req.struct_size = 8
        assert s._L.ba_covariance(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "struct_size" in s.last_error()
        req, info = BaCovRequest(), BaCovInfo()
        info.struct_size = 16
        assert s._L.ba_covariance(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "struct_size" in s.last_error()
        assert s._L.ba_covariance(s._h, C.byref(ps), None, C.byref(info)) == -1
        assert s.last_error()
        g = s.covariance(p.copy(), points=True)  # the context still works
        assert g["status"] == 0
        # point_idx = NULL with n_points == prob->n_points: every point, in order; NULL with another count is refused
        pc = np.zeros((p.n_points, 3, 3))
        req, info = BaCovRequest(), BaCovInfo()
        req.n_points, req.point_cov = p.n_points, pc.ctypes.data_as(C.POINTER(C.c_double))
        assert s._L.ba_covariance(s._h, C.byref(ps), C.byref(req), C.byref(info)) == 0 and info.status == 0
        # (two assemblies of S with f64 atomics: equal to rounding times cond, not bitwise)
        assert (np.abs(pc - g["point_cov"]).max((1, 2)) <= 1e-9 * np.abs(g["point_cov"]).max((1, 2))).all()
        req.n_points = p.n_points - 1
        assert s._L.ba_covariance(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
    with solver() as s:
        s.comm_init(1, 0, Solver.comm_unique_id())
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.covariance(p.copy())


def test_variance_factor():
    p, ref = refcov.reference("bcr21_messy")
    with solver() as s:
        cost = s.linearize(p.copy())["cost"]
        g = s.covariance(p.copy())
    n_adm = int((p.obs_depth > 1e-15).sum())
    nap = len(np.unique(p.obs_pt[p.obs_depth > 1e-15]))
    dof = 3 * n_adm + 4 - (6 * len(ref.ac_cam) + 3 * nap + 4)
    assert dof > 0
    want = 2.0 * cost / dof
    assert abs(g["cost"] - cost) <= 1e-12 * cost
    assert abs(g["variance_factor"] - want) <= 1e-12 * want
