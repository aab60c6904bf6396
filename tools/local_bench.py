#!/usr/bin/env python3
"""Measure the local window (ba_local_window / ba_solve_local) on one GPU, in one process.

    python tools/local_bench.py --config G1 [--out profiles/local_g1.json]   200 cams / 100 k points, 2 sweeps x 5
    python tools/local_bench.py --config G2 [--out profiles/local_g2.json]   50 cams / 4 k points, 2 sweeps x 5
    python tools/local_bench.py --select C5 [--out profiles/local_c5.json]   the selection alone on a C5-sized map

Selection: ``Solver.local_window`` centred on a keyframe of the second sweep (the map's last keyframe but two), a warm
call and then --reps calls: time_select_ms (the kernels, HIP events) and time_total_ms (the whole call) of each, their
medians; beside them the wall time of the same selection by tests/reflocal.py's plain-Python sets (one run: it is the
reference the tests compare against, not an optimised host implementation).

Solve (--config): three legs in alternating runs, a fresh context per run, a warm call and then a timed call from the
same start: ``solve_local`` around the centre; ``solve`` of the whole map; ``solve`` of the last-k window, k = the
local window's |L|, cut out of the map as the reference's schedule does (the window's first keyframe its gauge). Per leg
the wall time of the call, the LM iterations, the sub-window's sizes and the reprojection RMS over the LOCAL window's
observations at the leg's result (``Solver.residuals`` on the local sub-window with the leg's parameters filled in; the
last-k leg leaves the first-sweep keyframes of the local window where they were). Prints one JSON line per map.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dsmc-bundle-adjustment_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def new_solver():
    from miba.solver import Solver
    return Solver(minimizer_progress_to_stdout=0)


def selection(prob, center, reps, min_weight, max_local, host=True):
    import reflocal
    with new_solver() as s:
        s.local_window(prob, center, min_weight, max_local)  # warm: code objects loaded, buffers grown
        runs = [s.local_window(prob, center, min_weight, max_local) for _ in range(reps)]
    rep = {k: int(runs[0][k]) for k in ("n_local", "n_fixed", "n_points", "n_obs", "sub_fixed_cam")}
    for k in ("time_select_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(r[k], 4) for r in runs]
        rep[k] = round(statistics.median(r[k] for r in runs), 4)
    if host:
        t0 = time.perf_counter()
        ref = reflocal.select(prob, center, min_weight, max_local)
        rep["reflocal_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        reflocal.assert_same(runs[0], ref, "local_bench")
    return rep, runs[0]


def last_k_window(prob, k):
    """The last k keyframes of the map as the reference's schedule cuts them: their observations, the points they see,
    the first of them the gauge. Returns (window, the map's camera indices, the map's point indices)."""
    from miba.capi import ProblemArrays
    cams = np.arange(prob.n_cams - k, prob.n_cams)
    keep = prob.obs_cam >= prob.n_cams - k
    pts = np.unique(prob.obs_pt[keep])
    pt_new = np.full(prob.n_points, -1, np.int32)
    pt_new[pts] = np.arange(len(pts), dtype=np.int32)
    w = ProblemArrays(prob.cams[cams].copy(), prob.points[pts].copy(), prob.intr.copy(), prob.intr_prior.copy(),
                      (prob.obs_cam[keep] - (prob.n_cams - k)).astype(np.int32), pt_new[prob.obs_pt[keep]],
                      prob.obs_uv[keep].copy(), prob.obs_depth[keep].copy(), 0)
    return w, cams, pts


def local_rms(prob, sel):
    """Reprojection RMS [px] over the local sub-window's observations at ``prob``'s parameters."""
    import reflocal
    with new_solver() as s:
        r = s.residuals(reflocal.sub_problem(prob, sel), per_obs=False, per_block=False)
    return r["rms_reproj_px"]


def one_leg(leg, prob, center, sel, min_weight, max_local):
    q = prob.copy()
    with new_solver() as s:
        if leg == "local":
            s.solve_local(prob.copy(), center, min_weight, max_local)  # warm
            t0 = time.perf_counter()
            sm = s.solve_local(q, center, min_weight, max_local)
            el = time.perf_counter() - t0
        elif leg == "whole":
            s.solve(prob.copy())
            t0 = time.perf_counter()
            sm = s.solve(q)
            el = time.perf_counter() - t0
        else:
            w, cams, pts = last_k_window(prob, int(sel["n_local"]))
            s.solve(w.copy())
            t0 = time.perf_counter()
            sm = s.solve(w)
            el = time.perf_counter() - t0
            q.cams[cams], q.points[pts], q.intr[:] = w.cams, w.points, w.intr
    return dict(ms=1e3 * el, iterations=sm["num_iterations"], active_cams=sm["num_active_cams"],
                obs=sm["num_obs_admissible"], points=sm["num_active_points"], linear_solver=sm["linear_solver_name"],
                camera_band=sm["camera_band"], termination=sm["termination"], final_cost=sm["final_cost"]), q


def measure(prob, reps, min_weight, max_local):
    center = prob.n_cams - 3
    res = {"cams": prob.n_cams, "points": prob.n_points, "obs": prob.n_obs, "center": center, "min_weight": min_weight,
           "max_local": max_local, "reps": reps}
    res["selection"], sel = selection(prob, center, reps, min_weight, max_local)
    L = sel["cam_index"][sel["cam_local"]]
    res["local_cams"] = [int(c) for c in L]
    res["first_sweep_in_L"] = int((L < prob.n_cams // 2).sum())
    res["rms_before_px"] = round(local_rms(prob, sel), 4)
    runs = {l: [] for l in ("local", "whole", "last_k")}
    last = {}
    for _ in range(reps):  # alternating
        for l in runs:
            r, q = one_leg(l, prob, center, sel, min_weight, max_local)
            runs[l].append(r["ms"])
            last[l] = (r, q)
    res["legs"] = {}
    for l, (r, q) in last.items():
        r = dict(r)
        r["ms_runs"] = [round(m, 3) for m in runs[l]]
        r["ms"] = round(statistics.median(runs[l]), 3)
        r["rms_local_window_px"] = round(local_rms(q, sel), 4)
        res["legs"][l] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["G1", "G2"], default=None)
    ap.add_argument("--select", default=None, help="a BASELINE config (C1 .. C5): the selection alone on it")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-weight", type=int, default=15)
    ap.add_argument("--max-local", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the plain-Python selection (slow on large maps)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from miba import synthetic
    out = []
    if a.select:
        prob = synthetic.make_config(a.select)
        rep, _ = selection(prob, prob.n_cams - 3, a.reps, a.min_weight, a.max_local, host=not a.no_host)
        r = {"config": a.select, "cams": prob.n_cams, "points": prob.n_points, "obs": prob.n_obs,
             "center": prob.n_cams - 3, "selection": rep}
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.config:
        prob = synthetic.make_sweep_config(a.config)
        r = measure(prob, a.reps, a.min_weight, a.max_local)
        r["config"] = a.config
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out if len(out) != 1 else out[0], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
