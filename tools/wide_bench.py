#!/usr/bin/env python3
"""Time the reduced-solve paths of wide co-visibility windows against each other, on one GPU and in one process.

    python tools/wide_bench.py --config G1 [--out profiles/wide_g1.json]    200 cams / 100 k points, 2 sweeps x 5
    python tools/wide_bench.py --config G2 [--out profiles/wide_g2.json]    50 cams / 4 k points, 2 sweeps x 5
    python tools/wide_bench.py --crossover [--out profiles/wide_crossover.json]
                                            sweep windows of npad 192 .. 1216, 12 points per camera
    python tools/wide_bench.py --ordered --config G1 [--out profiles/order_g1.json]
                                            the window as given against the window in its co-visibility order
    python tools/wide_bench.py --covis C5 [--out profiles/order_c5.json]    ba_covisibility's own times

Per window, MIBA_SOLVER=dense (the one-workgroup envelope Cholesky, k_chol) and MIBA_SOLVER=blocked (the
multi-workgroup blocked Cholesky) in alternating runs, a fresh context per run: a prepare, a warm solve, then a timed
solve of exactly --steps LM iterations (tolerances off) without HIP events -> LM it/s and ms per iteration; then one
profiled solve per path for the per-kernel table (ba_kernel_stats) and the reduced-solve time per iteration (the
sum of the path's kernels). Prints one JSON line per window.

--ordered: three legs in alternating runs, a fresh context per run, the default solver selection: Solver.solve(p) as
given, solve(p, order=o) with a saved order, solve(p, order="auto") (the co-visibility pass, the ordering and the
permutation inside the timed call). Per run a warm solve, then a timed solve of exactly --steps LM iterations: the whole
call (prepare with its plan cache, LM loop, copies) over the iterations -> ms per iteration and LM it/s, and the LM
loop's own time (ba_summary.time_lm_ms) beside it; the solver path, band and overflow launches of each leg, and
ba_covisibility's report and times.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dsmc-bundle-adjustment_amd"))
sys.path.insert(0, ROOT)

PATHS = ("dense", "blocked")
SOLVE_KERNELS = ("chol", "dense_copy", "dense_diag", "dense_panel", "dense_trail", "dense_back")
NO_TOL = dict(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
# npad -> cameras of the crossover's sweep windows (6 (cams - 1) + 4 padded to 16)
CROSSOVER = {192: 32, 256: 42, 384: 64, 512: 84, 768: 126, 1216: 202}


def one_run(prob, path, steps, profile):
    from miba.solver import Solver
    os.environ["MIBA_SOLVER"] = path
    with Solver(minimizer_progress_to_stdout=0, max_num_iterations=steps, profile_kernels=int(profile), profile_mask=0,
                **NO_TOL) as s:
        s.prepare(prob.copy())
        s.solve_prepared(prob.copy())  # warm: code objects loaded, buffers grown
        q = prob.copy()
        s.reset_kernel_stats()
        t0 = time.perf_counter()
        sm = s.solve_prepared(q)
        el = time.perf_counter() - t0
        stats = [k for k in s.kernel_stats() if k["launches"] > 0] if profile else []
    return sm, el, stats


def measure(prob, steps, reps):
    res = {"cams": prob.n_cams, "points": prob.n_points, "obs": prob.n_obs, "steps": steps, "reps": reps, "paths": {}}
    runs = {p: [] for p in PATHS}
    summ = {}
    for _ in range(reps):  # alternating
        for p in PATHS:
            sm, el, _ = one_run(prob, p, steps, False)
            runs[p].append(el)
            summ[p] = sm
    for p in PATHS:
        sm = summ[p]
        it = max(sm["num_iterations"], 1)
        ms = [1e3 * e / it for e in runs[p]]
        smp, _, stats = one_run(prob, p, steps, True)
        itp = max(smp["num_iterations"], 1)
        table = {k["name"]: {"launches_per_iter": round(k["launches"] / itp, 2),
                             "us_per_iter": round(1e3 * k["total_ms"] / itp, 2)} for k in stats}
        solve_us = sum(v["us_per_iter"] for n, v in table.items() if n in SOLVE_KERNELS)
        all_us = sum(v["us_per_iter"] for v in table.values())
        res["paths"][p] = {
            "linear_solver": sm["linear_solver"], "iterations": sm["num_iterations"], "final_cost": sm["final_cost"],
            "ms_per_iter_runs": [round(m, 4) for m in ms], "ms_per_iter": round(statistics.median(ms), 4),
            "lm_it_per_s": round(1e3 / statistics.median(ms), 1),
            "reduced_solve_us_per_iter": round(solve_us, 2), "kernels_us_per_iter": round(all_us, 2),
            "obs_pairs_share": round(table.get("obs_pairs", {}).get("us_per_iter", 0.0) / all_us, 4) if all_us else None,
            "kernels": table}
    res["npad"] = (summ["dense"]["reduced_system_size"] + 15) // 16 * 16
    res["camera_band"] = summ["dense"]["camera_band"]
    d, b = res["paths"]["dense"], res["paths"]["blocked"]
    res["speedup_lm"] = round(d["ms_per_iter"] / b["ms_per_iter"], 3)
    res["speedup_reduced_solve"] = round(d["reduced_solve_us_per_iter"] / max(b["reduced_solve_us_per_iter"], 1e-9), 3)
    return res


LEGS = ("given", "saved", "auto")


def ordered_run(prob, leg, order, steps, profile):
    from miba.solver import Solver
    os.environ.pop("MIBA_SOLVER", None)
    arg = {"given": None, "saved": order, "auto": "auto"}[leg]
    with Solver(minimizer_progress_to_stdout=0, max_num_iterations=steps, profile_kernels=int(profile), profile_mask=0,
                **NO_TOL) as s:
        s.solve(prob.copy(), order=arg)  # warm: code objects loaded, buffers grown, the plan cached
        q = prob.copy()
        s.reset_kernel_stats()
        t0 = time.perf_counter()
        sm = s.solve(q, order=arg)
        el = time.perf_counter() - t0
        stats = [k for k in s.kernel_stats() if k["launches"] > 0] if profile else []
        reused = s.last_prepare()["plan_reused"]
    return sm, el, stats, reused


def covis_report(prob, reps):
    from miba.solver import Solver
    with Solver(minimizer_progress_to_stdout=0) as s:
        s.covisibility(prob)  # warm
        runs = [s.covisibility(prob) for _ in range(reps)]
    rep = {k: v for k, v in runs[0].items() if k not in ("weights", "order") and not k.startswith("time_")}
    for k in ("time_count_ms", "time_order_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(r[k], 4) for r in runs]
        rep[k] = round(statistics.median(r[k] for r in runs), 4)
    return rep, runs[0]["order"]


def measure_ordered(prob, steps, reps):
    res = {"cams": prob.n_cams, "points": prob.n_points, "obs": prob.n_obs, "steps": steps, "reps": reps, "legs": {}}
    res["covisibility"], order = covis_report(prob, reps)
    runs = {l: [] for l in LEGS}
    lm = {l: [] for l in LEGS}
    summ, reused = {}, {}
    for _ in range(reps):  # alternating
        for l in LEGS:
            sm, el, _, ru = ordered_run(prob, l, order, steps, False)
            it = max(sm["num_iterations"], 1)
            runs[l].append(1e3 * el / it)
            lm[l].append(sm["time_lm_ms"] / it)
            summ[l], reused[l] = sm, ru
    for l in LEGS:
        sm = summ[l]
        smp, _, stats, _ = ordered_run(prob, l, order, steps, True)
        itp = max(smp["num_iterations"], 1)
        table = {k["name"]: {"launches_per_iter": round(k["launches"] / itp, 2),
                             "us_per_iter": round(1e3 * k["total_ms"] / itp, 2)} for k in stats}
        res["legs"][l] = {
            "linear_solver": sm["linear_solver"], "linear_solver_name": sm["linear_solver_name"],
            "camera_band": sm["camera_band"], "iterations": sm["num_iterations"], "final_cost": sm["final_cost"],
            "plan_reused": reused[l],
            "ms_per_iter_runs": [round(m, 4) for m in runs[l]], "ms_per_iter": round(statistics.median(runs[l]), 4),
            "lm_it_per_s": round(1e3 / statistics.median(runs[l]), 1),
            "lm_it_per_s_range": [round(1e3 / max(runs[l]), 1), round(1e3 / min(runs[l]), 1)],
            "lm_loop_ms_per_iter_runs": [round(m, 4) for m in lm[l]],
            "lm_loop_it_per_s": round(1e3 / statistics.median(lm[l]), 1),
            "obs_pairs_launches_per_iter": table.get("obs_pairs", {}).get("launches_per_iter", 0.0),
            "kernels": table}
    g = res["legs"]["given"]
    for l in ("saved", "auto"):
        res["legs"][l]["speedup_vs_given"] = round(g["ms_per_iter"] / res["legs"][l]["ms_per_iter"], 2)
        res["legs"][l]["range_above_given"] = bool(res["legs"][l]["lm_it_per_s_range"][0] > g["lm_it_per_s_range"][1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["G1", "G2"], default=None)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ordered", action="store_true", help="with --config: as given against the co-visibility order")
    ap.add_argument("--covis", default=None, help="a BASELINE config (C1 .. C5): ba_covisibility's times on it")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from miba import synthetic
    out = []
    if a.crossover:
        for npad, nc in CROSSOVER.items():
            prob = synthetic.make_sweep_problem(nc, 12 * nc, 5, 2, seed=900 + nc, sensor_f32=True)
            r = measure(prob, a.steps, a.reps)
            assert r["npad"] == npad, (r["npad"], npad)
            r["window"] = f"sweep {nc} cams x 12 points, 2 x 5"
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.covis:
        prob = synthetic.make_config(a.covis)
        rep, _ = covis_report(prob, a.reps)
        r = {"config": a.covis, "cams": prob.n_cams, "points": prob.n_points, "obs": prob.n_obs, "covisibility": rep}
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.config:
        prob = synthetic.make_sweep_config(a.config)
        r = measure_ordered(prob, a.steps, a.reps) if a.ordered else measure(prob, a.steps, a.reps)
        r["config"] = a.config
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out if len(out) != 1 else out[0], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
