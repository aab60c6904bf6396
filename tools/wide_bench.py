#!/usr/bin/env python3
"""Time the reduced-solve paths of wide co-visibility windows against each other, on one GPU and in one process.

    python tools/wide_bench.py --config G1 [--out profiles/wide_g1.json]    200 cams / 100 k points, 2 sweeps x 5
    python tools/wide_bench.py --config G2 [--out profiles/wide_g2.json]    50 cams / 4 k points, 2 sweeps x 5
    python tools/wide_bench.py --crossover [--out profiles/wide_crossover.json]
                                            sweep windows of npad 192 .. 1216, 12 points per camera

Per window, MIBA_SOLVER=dense (the one-workgroup envelope Cholesky, k_chol) and MIBA_SOLVER=blocked (the
multi-workgroup blocked Cholesky) in alternating runs, a fresh context per run: a prepare, a warm solve, then a timed
solve of exactly --steps LM iterations (tolerances off) without HIP events -> LM it/s and ms per iteration; then one
profiled solve per path for the per-kernel table (ba_kernel_stats) and the reduced-solve time per iteration (the
sum of the path's kernels). Prints one JSON line per window.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["G1", "G2"], default=None)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
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
    if a.config:
        prob = synthetic.make_sweep_config(a.config)
        r = measure(prob, a.steps, a.reps)
        r["config"] = a.config
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out if len(out) != 1 else out[0], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
