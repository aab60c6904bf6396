"""ba_pose_graph on the GPU against tests/refpg.py (test_refpg.py checks the references and that the graphs used here
qualify).

* the first step (max_num_iterations = 1) against refcand.retract_quat(x, the longdouble step) within refcand's
  retraction bound plus F cond eps |step|_inf, F = refpg.STEP_F, at three radii, at the sizes on the layout's edges and
  on every topology; once more with a Huber parameter that puts edges in both zones and non-unit weights;
* the whole loop on graphs whose accept / reject sequence is settled: the sequence, the counters, the termination and
  message, the final cost and the poses;
* a loop closure of 200 poses (the one graph with a many-block envelope);
* bits and side effects; the errors."""
import ctypes as C

import numpy as np
import pytest

import refcand
import refpg
import refstep
from refstep import EPS64, NO_TOL

pytestmark = pytest.mark.gpu


def solver(**kw):
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0, **kw)


def run(s, g, cams=None, **kw):
    x = np.array(g["cams"] if cams is None else cams, dtype=np.float64)
    r = s.pose_graph(x, g["ea"], g["eb"], g["meas"], weights=g["weights"], constant=g["constant"], huber=g["huber"], **kw)
    assert r["cams"] is x
    return r


def _check_first_step(s, key, g, radius, okw):
    ref = refpg.step_ref(key, g, radius, **okw)
    act = refpg.active(g)
    r = run(s, g)
    x = r["cams"]
    has_edge = refpg._with_edge(g)
    sb = refpg.step_bound(ref)
    worst = 0.0
    for k, c in enumerate(act):
        if not has_edge[k]:
            np.testing.assert_array_equal(x[c], g["cams"][c])  # an isolated pose: bitwise as given
            assert np.all(ref["delta"][k] == 0)
            continue
        eq, et = refcand.retraction_error(x[c], g["cams"][c], ref["delta_ld"][k])
        bq, bt = refcand.retraction_bound(g["cams"][c], ref["delta"][k])
        worst = max(worst, eq / (bq + sb), et / (bt + sb))
        assert eq <= bq + sb and et <= bt + sb, (key, radius, c, eq, et, bq, bt, sb)
    const = np.asarray(g["constant"], dtype=bool)
    np.testing.assert_array_equal(x[const], g["cams"][const])
    print(f"FIRST {key} radius={radius:g} cond={ref['cond']:.3g} |step|={np.abs(ref['delta']).max():.2e} "
          f"worst err/bound={worst:.3f} band {r['band_before']}->{r['band_after']}")
    assert r["n_active"] == len(act) and r["reduced_system_size"] == 6 * len(act)
    assert abs(r["initial_cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    if has_edge.any():  # the step was taken and accepted
        assert (r["iterations"], r["n_successful"], r["n_unsuccessful"]) == (1, 2, 0), r
        assert r["termination_type"] == 1 and r["message"].startswith("Maximum number of iterations")
    return r


@pytest.mark.parametrize("radius", refpg.STEP_RADII)
def test_first_step(radius):
    with solver(max_num_iterations=1, initial_trust_region_radius=radius, **NO_TOL) as s:
        for topology, n in refpg.STEP_CASES:
            g = refpg.step_graph(topology, n)
            r = _check_first_step(s, (topology, n), g, radius, {})
            if topology == "loop" and n >= 11:
                assert r["band_after"] < r["band_before"] == n - 1
            if topology == "two":
                assert r["n_components"] == 2


def test_first_step_huber_zones_and_weights():
    g = refpg.huber_graph()
    quad, lin = refpg.huber_zones(g)
    assert quad >= 3 and lin >= 3
    with solver(max_num_iterations=1, **NO_TOL) as s:
        _check_first_step(s, "huber", g, 1e4, {})


@pytest.mark.parametrize("name", [c[0] for c in refpg.LOOP_CASES])
def test_loop(name):
    g, okw = refpg.loop_case(name)
    a, b = refpg.loop_refs(name)
    with solver(**okw) as s:
        r = run(s, g, log=True)
    x, log = r["cams"], r["log"]
    act = refpg.active(g)
    spread = float(np.abs(a["cams"] - b["cams"]).max())
    tol = 16 * max(spread, 64 * EPS64 * max(1.0, float(np.abs(b["cams"][:, 4:]).max())))
    err = float(np.abs(x - b["cams"]).max())
    rel = abs(r["final_cost"] - b["final_cost"]) / b["final_cost"]
    print(f"LOOP {name} iters={r['iterations']}/{b['iterations']} rej={b['accept'].count(0)} cost rel={rel:.2e} "
          f"pose err={err:.2e} tol={tol:.2e} spread={spread:.2e} msg={r['message']!r}")
    assert r["log_rows"] == b["iterations"] + 1 == len(log)
    assert log[1:, 6].astype(int).tolist() == b["accept"]
    assert (r["iterations"], r["n_successful"], r["n_unsuccessful"], r["termination_type"]) == \
        (b["iterations"], b["n_succ"], b["n_unsucc"], b["termination"])
    text = {refpg.MSG_MAX_ITER: "Maximum number of iterations", refpg.MSG_GRAD_TOL: "Gradient tolerance",
            refpg.MSG_FUNC_TOL: "Function tolerance", refpg.MSG_PARAM_TOL: "Parameter tolerance"}[b["msg"]]
    assert r["message"].startswith(text)
    assert rel <= 1e-6
    assert abs(r["initial_cost"] - b["initial_cost"]) <= 1e-6 * b["initial_cost"]
    assert err <= tol
    assert log[0, 0] == r["initial_cost"] and log[0, 6] == 1 and np.all(log[:, 7] == 0)
    const = np.asarray(g["constant"], dtype=bool)
    np.testing.assert_array_equal(x[const], g["cams"][const])
    assert len(act) == r["n_active"]


def test_loop_closure():
    g = refpg.closure()
    b = refpg.closure_ref()
    with solver() as s:
        r = run(s, g)
    before = refpg.pose_rms(g["cams"], g["truth"])
    ref_rms = refpg.pose_rms(b["cams"], g["truth"])
    rms = refpg.pose_rms(r["cams"], g["truth"])
    rel = abs(r["final_cost"] - b["final_cost"]) / b["final_cost"]
    print(f"CLOSURE rms {before:.4f} -> {rms:.4f} (reference {ref_rms:.4f}) cost rel={rel:.2e} iters={r['iterations']} "
          f"band {r['band_before']}->{r['band_after']} kernels {r['time_kernels_ms']:.2f} ms solve {r['time_solve_ms']:.2f} ms")
    assert r["reduced_system_size"] == 1194 and r["n_active"] == 199
    assert rms < before and rms <= 1.01 * ref_rms
    assert rel <= 1e-6
    assert r["band_after"] < r["band_before"]
    assert r["termination_type"] == 0


def test_bits_and_side_effects():
    g, okw = refpg.loop_case("dup_weighted")
    const = np.asarray(g["constant"], dtype=bool)
    with solver(**okw) as s:
        a = run(s, g, log=True)
        b = run(s, g, log=True)
        np.testing.assert_array_equal(a["cams"], b["cams"])  # two calls, the same bits
        np.testing.assert_array_equal(a["log"], b["log"])
        np.testing.assert_array_equal(a["edge_cost"], b["edge_cost"])
        assert a["final_cost"] == b["final_cost"] and not np.array_equal(a["cams"], g["cams"])
        n = len(g["cams"])
        assert sorted(a["cam_order"].tolist()) == list(range(n))  # a permutation, the active poses first
        assert not const[a["cam_order"][: a["n_active"]]].any() and const[a["cam_order"][a["n_active"]:]].all()
        np.testing.assert_array_equal(a["cams"][const], g["cams"][const])
        # the last decision of this graph is an accepted step or a tolerance on a candidate that was not taken: the
        # edge costs are those at the returned poses, whose sum is the cost of the last accepted row of the log
        last_acc = a["log"][a["log"][:, 6] == 1][-1, 0]
        assert abs(a["edge_cost"].sum() - last_acc) <= 1e-12 * last_acc
        assert a["final_cost"] <= last_acc
        # fixed_cam is constant in addition to the mask
        c = int(refpg.active(g)[3])
        x = np.array(g["cams"])
        r = s.pose_graph(x, g["ea"], g["eb"], g["meas"], weights=g["weights"], constant=g["constant"], fixed_cam=c)
        np.testing.assert_array_equal(x[c], g["cams"][c])
        assert r["n_active"] == a["n_active"] - 1
    # a graph whose final cost is the cost at the result
    g2, okw2 = refpg.loop_case("limit")
    with solver(**okw2) as s:
        r = run(s, g2, log=True)
        assert np.all(r["log"][1:, 6] == 1)
        assert abs(r["edge_cost"].sum() - r["final_cost"]) <= 1e-12 * r["final_cost"]


def test_no_side_effect_on_a_prepared_window():
    """prepare, pose_graph (another graph), solve_prepared: the bits of prepare, solve_prepared (deterministic = 1)."""
    p = refstep.window("bcr21")
    g, _ = refpg.loop_case("loop22")
    with solver(deterministic=1) as s:
        a = p.copy()
        s.prepare(a)
        sa = s.solve_prepared(a)
        la = s.iteration_log()
    with solver(deterministic=1) as s:
        b = p.copy()
        s.prepare(b)
        r = run(s, g)
        sb = s.solve_prepared(b)
        lb = s.iteration_log()
    assert r["iterations"] > 0
    for k in ("cams", "points", "intr"):
        np.testing.assert_array_equal(getattr(b, k), getattr(a, k))
    np.testing.assert_array_equal(lb, la)
    for k in ("final_cost", "initial_cost", "num_iterations", "num_successful_steps", "linear_solver", "camera_band"):
        assert sb[k] == sa[k], k


def test_legal_degenerate_inputs():
    g = refpg.step_graph("loop", 11)
    with solver() as s:
        # no edge: nothing is written, the costs are reported
        x = np.array(g["cams"])
        r = s.pose_graph(x, [], [], np.zeros((0, 7)), constant=g["constant"])
        np.testing.assert_array_equal(x, g["cams"])
        assert (r["iterations"], r["termination_type"], r["initial_cost"], r["final_cost"]) == (0, 0, 0.0, 0.0)
        assert r["n_active"] == 11 and r["n_edges_used"] == 0
        # every pose constant
        x = np.array(g["cams"])
        r = s.pose_graph(x, g["ea"], g["eb"], g["meas"], constant=np.ones(len(x), dtype=bool))
        np.testing.assert_array_equal(x, g["cams"])
        lin = refpg.linearize(g, None, np.float64)
        assert r["n_active"] == 0 and r["iterations"] == 0 and r["termination_type"] == 0
        assert abs(r["initial_cost"] - float(lin["total"])) <= 1e-12 * float(lin["total"]) and r["final_cost"] == r["initial_cost"]
        # no constant pose at all: legal, the damping keeps the system positive definite
        x = np.array(g["cams"])
        r = s.pose_graph(x, g["ea"], g["eb"], g["meas"])
        assert r["termination_type"] == 0 and r["n_active"] == len(x) and r["final_cost"] < r["initial_cost"]
        assert np.all(np.isfinite(x))
        # an empty graph
        r = s.pose_graph(np.zeros((0, 7)), [], [], np.zeros((0, 7)))
        assert r["n_active"] == 0 and r["iterations"] == 0


def test_errors_and_non_finite_inputs():
    from miba.capi import PG_MAX_NPAD, BaPgInfo, BaPgProblem, BaPgRequest
    from miba.solver import MibaError
    g = refpg.step_graph("loop", 11)
    n = len(g["cams"])

    def call(s, **over):
        kw = dict(cams=np.array(g["cams"]), edge_a=g["ea"].copy(), edge_b=g["eb"].copy(), meas=g["meas"].copy(),
                  constant=g["constant"])
        kw.update(over)
        return s.pose_graph(**kw), kw["cams"]

    with solver() as s:
        ea = g["ea"].copy(); ea[3] = n
        with pytest.raises(MibaError, match=r"\(-1\).*ba_pose_graph.*edge index out of range"):
            call(s, edge_a=ea)
        eb = g["eb"].copy(); eb[2] = -1
        with pytest.raises(MibaError, match=r"\(-1\).*edge index out of range"):
            call(s, edge_b=eb)
        eb = g["eb"].copy(); eb[4] = g["ea"][4]
        with pytest.raises(MibaError, match=r"\(-1\).*self edge"):
            call(s, edge_b=eb)
        with pytest.raises(MibaError, match=r"\(-1\).*fixed_cam"):
            call(s, fixed_cam=n)
        with pytest.raises(MibaError, match=r"\(-1\).*huber"):
            call(s, huber=-1.0)
        # through the C ABI: null arguments, sizes, null buffers, negative sizes, a log without a buffer
        x = np.array(g["cams"])
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def problem():
            p = BaPgProblem()
            p.n_cams, p.n_edges, p.fixed_cam = n, len(g["ea"]), -1
            p.cams, p.edge_meas = x.ctypes.data_as(dp), g["meas"].ctypes.data_as(dp)
            p.edge_a, p.edge_b = g["ea"].ctypes.data_as(ip), g["eb"].ctypes.data_as(ip)
            return p

        def raw(p, req, info):
            return s._L.ba_pose_graph(s._h, C.byref(p) if p is not None else None, C.byref(req) if req is not None else None,
                                      C.byref(info) if info is not None else None)

        for args in ((None, BaPgRequest(), BaPgInfo()), (problem(), None, BaPgInfo()), (problem(), BaPgRequest(), None)):
            assert raw(*args) == -1 and "null argument" in s.last_error()
        req = BaPgRequest(); req.struct_size -= 8
        assert raw(problem(), req, BaPgInfo()) == -1 and "request struct_size below BA_PG_REQUEST_MIN_SIZE" in s.last_error()
        info = BaPgInfo(); info.struct_size -= 8
        assert raw(problem(), BaPgRequest(), info) == -1 and "info struct_size below BA_PG_INFO_MIN_SIZE" in s.last_error()
        p = problem(); p.n_edges = -1
        assert raw(p, BaPgRequest(), BaPgInfo()) == -1 and "negative graph sizes" in s.last_error()
        p = problem(); p.edge_meas = None
        assert raw(p, BaPgRequest(), BaPgInfo()) == -1 and "null graph buffer" in s.last_error()
        p = problem(); p.cams = None
        assert raw(p, BaPgRequest(), BaPgInfo()) == -1 and "null graph buffer" in s.last_error()
        req = BaPgRequest(); req.log_max_rows = 4
        assert raw(problem(), req, BaPgInfo()) == -1 and "log buffer" in s.last_error()
        np.testing.assert_array_equal(x, g["cams"])
        # an info struct larger than the library's is legal: only the library's bytes are written
        class BigInfo(C.Structure):
            _fields_ = [("info", BaPgInfo), ("tail", C.c_uint8 * 24)]
        big = BigInfo()
        big.info.struct_size = C.sizeof(BigInfo)
        for k in range(24):
            big.tail[k] = 0xA5
        assert s._L.ba_pose_graph(s._h, C.byref(problem()), C.byref(BaPgRequest()), C.cast(C.pointer(big), C.POINTER(BaPgInfo))) == 0
        assert big.info.struct_size == C.sizeof(BigInfo) and big.info.n_active == 12 and bytes(big.tail) == b"\xa5" * 24
        # the cap: refused with the sizes in the text, before anything is allocated
        n_big = PG_MAX_NPAD // 6 + 1
        with pytest.raises(MibaError, match=rf"\(-1\).*{n_big} active poses.*above the cap of {PG_MAX_NPAD}"):
            s.pose_graph(np.tile(g["cams"][:1], (n_big, 1)), [0], [1], g["meas"][:1])
        # not finite: BA_FAILURE, the poses kept, no log row
        for what in ("pose", "meas", "weight"):
            kw = {}
            cams = np.array(g["cams"])
            if what == "pose":
                cams[3, 5] = np.nan
            elif what == "meas":
                m = g["meas"].copy(); m[2, 1] = np.inf; kw["meas"] = m
            else:
                w = np.ones((len(g["ea"]), 2)); w[5, 0] = np.nan; kw["weights"] = w
            given = cams.copy()
            r, out = call(s, cams=cams, log=True, **kw)
            assert r["termination_type"] == 2 and r["message"] == "Residual and Jacobian evaluation failed."
            assert r["iterations"] == 0 and r["log_rows"] == 0 and len(r["log"]) == 0
            assert np.isnan(r["initial_cost"]) and np.isnan(r["final_cost"])
            np.testing.assert_array_equal(out, given)
        r, _ = call(s)  # the context still works
        assert r["termination_type"] == 0
    with solver() as s:
        s.comm_init_host(1, 0, lambda arr, op: None)
        with pytest.raises(MibaError, match=r"\(-1\).*shard"):
            call(s)
