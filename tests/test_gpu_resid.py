"""ba_residuals (Solver.residuals, Solver.solve_culled) against the extended-precision reference of tests/refresid.py.

Values are checked on every window of refresid.WINDOWS at two parameter sets, the perturbed start (most observations
beyond 3 px) and the oracle's solution (about 2 %), with the thresholds 3 px / max_depth_rel = 0.05:

* obs_flags equal the reference's, exactly (test_refresid.py::test_gap_condition: no reference value is within
  1000 tolerances of a threshold);
* obs_err within refresid.TOL (16 x the float64-against-longdouble gap of the reference: du / dv 2.9e-12 px,
  depth - z and z 1.5e-14), obs_cost within TOL["cost"] of itself and within refresid.cost_bound;
* internal consistency against the device's OWN per-observation output: every count exact, every maximum equal to the
  maximum of sqrt(du^2 + dv^2) of the reported errors bit for bit, every sum within (n + 4) eps_f64, relative, of the
  longdouble sum of the reported terms (n terms; the any-order bound of a sum of non-negative terms, each formed with
  at most three roundings);
* cost within (n_admissible + 8) eps_f64, relative, of Solver.linearize's;
* obs_depth_culled is obs_depth with exactly the BA_RES_OUTLIER observations zeroed; prob is unchanged.

What the windows reach in the kernels: one1 / one2 less than a workgroup and points on the gauge camera only;
bcr21_messy duplicates, bad depths, a shuffled order (inadmissible slots, N below the observation count);
inactive_mid21 a camera whose observations are all inadmissible; gauge_mid21 a gauge that is not camera 0;
nb37_b2_f32 / spans_f32 the obs32 records; spans / gauge_only points of one observation; obs256 / obs257 a point of
256 / 257 observations and a camera over a 256-observation sub-segment; bs_long a point of 1040 observations; short400
many points per wave.

Measured (MI355X), the largest over all cases: du / dv 1.83e-13 px, depth - z and z 7.8e-16, obs_cost 1.8e-3 of itself
(gauge_only solved) and 4.4 % of refresid.cost_bound; the cull loop's final cost equals the oracle's to 2e-15.
"""
import ctypes as C

import numpy as np
import pytest

import refresid
from refresid import BEHIND, EPS64, INADMISSIBLE, LD, OUTLIER

pytestmark = pytest.mark.gpu

THR = dict(max_reproj_px=refresid.MAX_REPROJ_PX, max_depth_abs=refresid.MAX_DEPTH_ABS,
           max_depth_rel=refresid.MAX_DEPTH_REL)
ARRAYS = ("err", "cost", "flags", "depth_culled", "cam_stats", "point_stats")
INFO = ("n_admissible", "n_outliers", "n_behind", "n_reproj", "n_depth", "n_huber_repr", "n_huber_unpr", "total_cost",
        "prior_cost", "rms_reproj_px", "max_reproj_px", "rms_depth", "max_depth")


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def unchanged(q, p):
    for a in ("cams", "points", "intr", "intr_prior", "obs_uv", "obs_depth", "obs_cam", "obs_pt"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a), err_msg=f"residuals modified prob.{a}")


def same_report(a, b, skip=()):
    for k in ARRAYS:
        if k not in skip:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in INFO:
        if k not in skip:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


def _close(got, want, n):
    """|got - want| <= (n + 4) eps |want| elementwise (want: longdouble sums of n terms each); NaN matches NaN."""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    ok = np.abs(got - want) <= (np.asarray(n, LD) + 4) * EPS64 * np.abs(want)
    return bool((ok | nan).all())


def consistency(g, p):
    """The block statistics and the window totals against the report's own per-observation values."""
    f = g["flags"]
    adm = (f & INADMISSIBLE) == 0
    proj = adm & ((f & BEHIND) == 0)
    out = adm & ((f & OUTLIER) != 0)
    du, dv, dd = g["err"][:, 0], g["err"][:, 1], g["err"][:, 2]
    with np.errstate(all="ignore"):
        hyp = np.sqrt(du * du + dv * dv)  # float64, IEEE: the device's spelling
        s2 = du.astype(LD) ** 2 + dv.astype(LD) ** 2
        d2 = dd.astype(LD) ** 2
    cost = g["cost"].astype(LD)
    for idx, st, nb in ((p.obs_cam, g["cam_stats"], p.n_cams), (p.obs_pt, g["point_stats"], p.n_points)):
        n_adm = np.bincount(idx[adm], minlength=nb)
        n_proj = np.bincount(idx[proj], minlength=nb)
        assert np.array_equal(st[:, 0], n_adm) and np.array_equal(st[:, 1], np.bincount(idx[out], minlength=nb))
        mx = np.zeros(nb)
        np.maximum.at(mx, idx[proj], hyp[proj])
        assert np.array_equal(st[:, 3], mx)
        for slot, term, m, n in ((2, s2, proj, n_proj), (4, d2, proj, n_proj), (5, cost, adm, n_adm)):
            want = np.zeros(nb, LD)
            np.add.at(want, idx[m], term[m])
            assert _close(st[:, slot], want, n), slot
        assert (st[n_adm == 0] == 0).all()
    na, npj = int(adm.sum()), int(proj.sum())
    assert g["n_admissible"] == na and g["n_outliers"] == int(out.sum())
    for name, bit in (("n_behind", BEHIND), ("n_reproj", 4), ("n_depth", 8), ("n_huber_repr", 16), ("n_huber_unpr", 32)):
        assert g[name] == int((adm & ((f & bit) != 0)).sum()), name
    assert g["max_reproj_px"] == (hyp[proj].max() if npj else 0.0)
    assert g["max_depth"] == (np.abs(dd[proj]).max() if npj else 0.0)
    assert _close(g["total_cost"] - g["prior_cost"], cost[adm].sum(), na + 1)
    if npj:
        assert _close(g["rms_reproj_px"], np.sqrt(s2[proj].sum() / npj), npj + 2)
        assert _close(g["rms_depth"], np.sqrt(d2[proj].sum() / npj), npj + 2)
    else:
        assert g["rms_reproj_px"] == 0.0 and g["rms_depth"] == 0.0


def check_values(g, ref, mask=None, tag=""):
    """obs_err / obs_cost of the report against the reference, over the admissible observations (of ``mask``)."""
    m = ref.adm if mask is None else ref.adm & mask
    e = np.abs(g["err"][m].astype(LD) - ref.err[m])
    dc = np.abs(g["cost"][m].astype(LD) - ref.cost[m])
    fig = dict(uv=float(e[:, :2].max()), dd=float(e[:, 2].max()), z=float(e[:, 3].max()),
               cost=float((dc / ref.cost[m]).max()), cost_over_bound=float((dc / refresid.cost_bound(ref)[m]).max()))
    print(f"RESID {tag} " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["uv"] <= refresid.TOL["uv"] and fig["dd"] <= refresid.TOL["dd"] and fig["z"] <= refresid.TOL["z"], fig
    assert fig["cost"] <= refresid.TOL["cost"] and fig["cost_over_bound"] <= 1.0, fig
    return fig


def run_case(name, which, monkeypatch=None, env=None, **opts):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    p = refresid.params(name, which)
    ref = refresid.reference(name, which)
    q = p.copy()
    with solver(**opts) as s:
        g = s.residuals(q, **THR)
        info = s.last_prepare()  # (of the full prepare: the next call reuses the plan)
        lin = s.linearize(q)["cost"]
    unchanged(q, p)
    assert np.array_equal(g["flags"], ref.flags)
    assert np.isnan(g["err"][~ref.adm]).all() and np.isnan(g["cost"][~ref.adm]).all()
    check_values(g, ref, tag=f"{name} {which} {env or ''}")
    consistency(g, p)
    assert abs(g["total_cost"] - lin) <= (g["n_admissible"] + 8) * EPS64 * lin, (g["total_cost"], lin)
    assert g["prior_cost"] == pytest.approx(float(ref.prior_cost), rel=1e-14)
    assert np.array_equal(g["depth_culled"], np.where((g["flags"] & OUTLIER) != 0, 0.0, p.obs_depth))
    assert np.array_equal(g["depth_culled"], ref.depth_culled)
    for k in ("n_admissible", "n_outliers", "n_behind", "n_reproj", "n_depth", "n_huber_repr", "n_huber_unpr"):
        assert g[k] == getattr(ref, k), k
    return g, info


@pytest.mark.parametrize("which", refresid.PARAM_SETS)
@pytest.mark.parametrize("name", refresid.WINDOWS)
def test_values(name, which):
    g, _ = run_case(name, which)
    p = refresid.params(name, which)
    if name == "inactive_mid21":
        assert (g["cam_stats"][12] == 0).all() and (p.obs_cam == 12).any()
    if name == "gauge_mid21":
        assert p.fixed_cam == 11 and g["cam_stats"][11, 0] > 0 and g["cam_stats"][11, 2] > 0
    if name == "bcr21_messy":
        assert g["n_admissible"] < p.n_obs and (g["flags"] == INADMISSIBLE).sum() == p.n_obs - g["n_admissible"]
    if name in ("obs256", "obs257", "bs_long"):
        assert g["point_stats"][:, 0].max() == {"obs256": 256, "obs257": 257, "bs_long": 1040}[name]


@pytest.mark.parametrize("env", [{"MIBA_SUBSEG": "64"}, {"MIBA_DEVICE_PLAN": "0"}, {"MIBA_DEVICE_PLAN": "1"}],
                         ids=["subseg64", "hostplan", "devplan"])
@pytest.mark.parametrize("name", ["spans", "obs257", "bs_long"])
def test_variants(name, env, monkeypatch):
    """Active cameras over several sub-segments, the host plan and the device plan: the same checks, and the report
    of the default run bit for bit (under MIBA_SUBSEG all but the camera sums and the totals formed from them)."""
    base, _ = run_case(name, "solved")
    g, info = run_case(name, "solved", monkeypatch, env=env)
    if "MIBA_DEVICE_PLAN" in env:
        assert info["plan_device"] == int(env["MIBA_DEVICE_PLAN"])
        same_report(g, base)
    else:
        same_report(g, base, skip=("cam_stats", "total_cost", "rms_reproj_px", "rms_depth"))
        assert np.array_equal(g["cam_stats"][:, [0, 1, 3]], base["cam_stats"][:, [0, 1, 3]])


@pytest.mark.parametrize("kind", ["mirror", "on"])
def test_behind_the_camera(kind):
    p, k, pt = refresid.behind_case(kind)
    ref = refresid.evaluate(p, None, **THR)
    p0 = refresid.window("one2")
    with solver() as s:
        g = s.residuals(p.copy(), **THR)
        g0 = s.residuals(p0.copy(), **THR)
    assert np.array_equal(g["flags"], ref.flags) and g["flags"][k] & BEHIND
    assert g["n_behind"] == ref.n_behind >= 1
    # values: the observations of every other point (the moved point is far off in its other cameras)
    check_values(g, ref, mask=p.obs_pt != pt, tag=f"behind {kind}")
    consistency(g, p)  # (the sums of slots 2-4 leave the BEHIND observations out, the counts take them)
    if kind == "mirror":
        assert g["err"][k, 3] < 0 and np.isfinite(g["err"][k]).all()
    else:
        assert g["err"][k, 3] == 0 and not np.isfinite(g["err"][k, 0])
        assert np.isfinite(g["cam_stats"][1, 2:5]).all() and np.isfinite(g["point_stats"][pt, 2:5]).all()
    assert g["cam_stats"][1, 0] == g0["cam_stats"][1, 0] and g["cam_stats"][1, 1] >= 1
    assert g["point_stats"][pt, 0] == g0["point_stats"][pt, 0] and g["point_stats"][pt, 1] >= 1
    # every block without an observation of the moved point is unaffected, bit for bit
    other_pts = np.arange(p.n_points) != pt
    assert np.array_equal(g["point_stats"][other_pts], g0["point_stats"][other_pts])
    other_cams = np.ones(p.n_cams, bool)
    other_cams[p.obs_cam[p.obs_pt == pt]] = False
    assert other_cams.any() and np.array_equal(g["cam_stats"][other_cams], g0["cam_stats"][other_cams])


def test_empty_windows():
    from miba.capi import ProblemArrays
    p = refresid.window("one2").copy()
    p.obs_depth[:] = 0.0
    none = ProblemArrays(p.cams, p.points, p.intr * 1.001, p.intr_prior, np.zeros(0, np.int32), np.zeros(0, np.int32),
                         np.zeros((0, 2)), np.zeros(0), int(p.fixed_cam))
    with solver() as s:
        for q in (p, none):
            ref = refresid.evaluate(q, None, **THR)
            g = s.residuals(q.copy(), **THR)
            assert all(g[k] == 0 for k in INFO[:7])
            assert g["total_cost"] == g["prior_cost"] == pytest.approx(float(ref.prior_cost), rel=1e-14)
            assert g["rms_reproj_px"] == 0 and g["max_reproj_px"] == 0 and g["rms_depth"] == 0 and g["max_depth"] == 0
            assert (g["cam_stats"] == 0).all() and (g["point_stats"] == 0).all()
            assert (g["flags"] == INADMISSIBLE).all() and np.isnan(g["err"]).all() and np.isnan(g["cost"]).all()
            assert g["err"].shape == (q.n_obs, 4) and np.array_equal(g["depth_culled"], q.obs_depth)
        assert float(refresid.evaluate(none, None).prior_cost) > 0
        g = s.residuals(refresid.window("one2").copy(), **THR)  # the context goes on
        assert g["n_admissible"] == 86


def _raw(s, q, **want):
    """ba_residuals with only the request buffers named in ``want`` (name -> array)."""
    from miba.capi import BaResInfo, BaResRequest
    req, info = BaResRequest(), BaResInfo()
    req.max_reproj_px, req.max_depth_abs, req.max_depth_rel = THR["max_reproj_px"], THR["max_depth_abs"], THR["max_depth_rel"]
    for k, a in want.items():
        setattr(req, k, a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double)))
    ps = q.struct()
    assert s._L.ba_residuals(s._h, C.byref(ps), C.byref(req), C.byref(info)) == 0, s.last_error()
    return info.as_dict()


def test_bitwise(monkeypatch):
    p = refresid.params("bcr21_messy", "solved")
    with solver() as s:
        a = s.residuals(p.copy(), **THR)
        same_report(s.residuals(p.copy(), **THR), a)  # two calls on one context
        # each request buffer alone, and none
        names = dict(obs_err="err", obs_cost="cost", obs_flags="flags", obs_depth_culled="depth_culled",
                     cam_stats="cam_stats", point_stats="point_stats")
        q = p.copy()
        for field, key in names.items():
            buf = np.full_like(a[key], -1)
            info = _raw(s, q, **{field: buf})
            assert np.array_equal(buf, a[key], equal_nan=True), field
            assert all(info[k.replace("total_", "")] == a[k] for k in INFO), field
        assert all(_raw(s, q)[k.replace("total_", "")] == a[k] for k in INFO)
    with solver() as s:  # another context
        same_report(s.residuals(p.copy(), **THR), a)
    with solver(deterministic=1) as s:
        same_report(s.residuals(p.copy(), **THR), a)
    for plan in ("0", "1"):
        monkeypatch.setenv("MIBA_DEVICE_PLAN", plan)
        with solver() as s:
            same_report(s.residuals(p.copy(), **THR), a)
            assert s.last_prepare()["plan_device"] == int(plan)


@pytest.mark.parametrize("name", ["bcr21_messy", "one2"])
def test_no_side_effect(name):
    """solve on a fresh context == residuals followed by solve on another, bit for bit."""
    p = refresid.window(name)
    q0, q1 = p.copy(), p.copy()
    with solver(deterministic=1) as s:
        s0 = s.solve(q0)
        log0 = s.iteration_log()
    with solver(deterministic=1) as s:
        s.residuals(q1, **THR)
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


def test_errors():
    from miba.capi import BaResInfo, BaResRequest
    from miba.solver import MibaError, Solver
    p = refresid.window("one2")
    with solver() as s:
        q = p.copy()  # (kept alive: the struct holds bare pointers into its arrays)
        ps = q.struct()
        req, info = BaResRequest(), BaResInfo()
        req.struct_size = 8
        assert s._L.ba_residuals(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "struct_size" in s.last_error()
        req, info = BaResRequest(), BaResInfo()
        info.struct_size = 16
        assert s._L.ba_residuals(s._h, C.byref(ps), C.byref(req), C.byref(info)) == -1
        assert "struct_size" in s.last_error()
        assert s._L.ba_residuals(s._h, C.byref(ps), None, C.byref(info)) == -1
        assert s.last_error()
        assert s._L.ba_residuals(s._h, C.byref(ps), C.byref(BaResRequest()), None) == -1
        g = s.residuals(p.copy(), **THR)  # the context still works
        assert g["n_admissible"] == 86
    with solver() as s:
        s.comm_init(1, 0, Solver.comm_unique_id())
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            s.residuals(p.copy())


@pytest.mark.parametrize("name", refresid.CULL_WINDOWS)
def test_cull_loop(name):
    orc = refresid.oracle_cull_loop(name)
    p = refresid.window(name)
    q = p.copy()
    with solver() as s:
        r = s.solve_culled(q, refresid.MAX_REPROJ_PX, rounds=2)
    assert np.array_equal(r["culled"], orc.culled)
    assert [x["termination_type"] for x in r["summaries"]] == [0, 0]
    want = orc.summaries[-1]["final_cost"]
    got = r["summaries"][-1]["final_cost"]
    print(f"CULL {name} culled={int(r['culled'].sum())} final_cost gpu={got:.10e} oracle={want:.10e} "
          f"rel={abs(got - want) / want:.1e} first={r['summaries'][0]['final_cost']:.4e}")
    assert abs(got - want) <= 1e-6 * want
    assert r["report"]["n_outliers"] == 0 and not (r["report"]["flags"] & OUTLIER).any()
    assert r["report"]["n_admissible"] == int((p.obs_depth > 1e-15).sum()) - int(orc.culled.sum())
    for a in ("obs_depth", "obs_uv", "obs_cam", "obs_pt", "intr_prior"):
        np.testing.assert_array_equal(getattr(q, a), getattr(p, a))
    assert not np.array_equal(q.cams, p.cams)  # prob holds the solution
