#!/usr/bin/env python3
"""Measure ba_refine_points (Solver.refine_points) on one GPU, in one process.

    python tools/refine_bench.py [--out-dir profiles] [--reps 7]

Runs: 1 and 4096 points of 10 admissible observations each (tests/refpts.tracks_problem: the positions perturbed as
the tests perturb them), refine_p1.json and refine_p4096.json; C4's map (synthetic.make_config("C4"): 200 cameras,
100 k points, 1 M observations) with every point perturbed by 3 cm per coordinate, refine_c4.json; and one point of
2000 observations, refine_o2000.json. Per run a warm call (code object loaded, buffers grown) and then --reps calls
from the same start positions: ``time_lm_ms`` (the kernel, HIP events) and ``time_total_ms`` (the whole call: grouping,
uploads, kernel, copies back), their medians and every value; the LM iterations (total, mean and the most any point
took); microseconds per point and per point-iteration from the kernel median, and the whole-call to kernel ratio. The
repeats must give the same bits (checked). For scale, the wall time of the plain-Python reference loop
(tests/refpts.lm, f64) on the first --ref-points points of the run: it is the reference the tests compare against,
not an optimised host implementation. Nothing here is a target; the numbers are reported as measured.
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

RUNS = ("p1", "p4096", "c4", "o2000")


def make(name):
    import refpts
    from miba import synthetic
    if name == "p1":
        return refpts.tracks_problem([10], seed=101, n_cams=64)
    if name == "p4096":
        return refpts.tracks_problem([10] * 4096, seed=102, n_cams=64)
    if name == "o2000":
        return refpts.tracks_problem([2000], seed=103)
    p = synthetic.make_config("C4")
    p.points += np.random.default_rng(104).normal(0, 0.03, p.points.shape)
    return p


def one_run(name, reps, ref_points):
    import refpts
    from miba.solver import Solver
    from oracle import oracle
    prob = make(name)
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = prob.copy()
        s.refine_points(warm)
        outs = []
        for _ in range(reps):
            q = prob.copy()
            r = s.refine_points(q)
            if not np.array_equal(q.points, warm.points):
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
    st = outs[0]["stats"]
    st = st[st[:, 6] >= 0]
    iters = st[:, 3]
    n = len(st)
    rep = dict(run=name, points=int(prob.n_points), cameras=int(prob.n_cams), n_obs_total=int(prob.n_obs),
               obs_per_point_mean=round(float(st[:, 0].mean()), 3), obs_per_point_max=int(st[:, 0].max()), reps=reps,
               n_solved=int(outs[0]["n_solved"]), n_convergence=int(outs[0]["n_convergence"]),
               n_no_convergence=int(outs[0]["n_no_convergence"]), n_failure=int(outs[0]["n_failure"]),
               iterations_total=int(iters.sum()), iterations_max=int(iters.max()),
               iterations_mean=round(float(iters.mean()), 3),
               cost_initial_mean=float(st[:, 1].mean()), cost_final_mean=float(st[:, 2].mean()))
    for k in ("time_lm_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(o[k], 4) for o in outs]
        rep[k] = round(statistics.median(o[k] for o in outs), 4)
    rep["us_per_point"] = round(1e3 * rep["time_lm_ms"] / n, 4)
    rep["us_per_point_iteration"] = round(1e3 * rep["time_lm_ms"] / max(rep["iterations_total"], 1), 4)
    rep["whole_call_over_kernel"] = round(rep["time_total_ms"] / max(rep["time_lm_ms"], 1e-9), 2)
    m = min(ref_points, n)
    o = oracle.default_options()
    solved = np.nonzero(outs[0]["stats"][:, 6] >= 0)[0][:m]
    t0 = time.perf_counter()
    ref_iters = sum(refpts.lm(prob, int(p), o)["iterations"] for p in solved)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    rep["python_reference"] = dict(points=m, iterations_total=int(ref_iters), wall_ms=round(ref_ms, 2),
                                   ms_per_point=round(ref_ms / m, 2))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-points", type=int, default=4)
    ap.add_argument("--runs", default=",".join(RUNS))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    for name in RUNS:
        if name not in want:
            continue
        rep = one_run(name, args.reps, args.ref_points)
        print(json.dumps(rep))
        with open(os.path.join(args.out_dir, f"refine_{name}.json"), "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
