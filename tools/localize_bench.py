#!/usr/bin/env python3
"""Measure ba_localize (Solver.localize) on one GPU, in one process.

    python tools/localize_bench.py [--out-dir profiles] [--reps 7]

Runs: batches of 1, 64, 256, 1024 and 4096 keyframes of 200 admissible observations each (a TUM keyframe; a shared
cloud, the poses perturbed as tests/refloc.frames_problem perturbs them), written to localize_b<N>.json, and one
keyframe of 2000 observations, localize_o2000.json. Per run a warm call (code object loaded, buffers grown) and then
--reps calls from the same start poses: ``time_lm_ms`` (the kernel, HIP events) and ``time_total_ms`` (the whole call:
grouping, uploads, kernel, copies back), their medians and every value; the LM iterations (total over the keyframes and
the most any keyframe took); microseconds per keyframe and per keyframe-iteration from the kernel median. The repeats
must give the same bits (checked). For scale, the wall time of the plain-Python reference loop (tests/refloc.lm, f64) on
the first --ref-frames keyframes of the run: it is the reference the tests compare against, not an optimised host
implementation. Nothing here is a target; the numbers are reported as measured.
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

RUNS = [("b1", 1, 200), ("b64", 64, 200), ("b256", 256, 200), ("b1024", 1024, 200), ("b4096", 4096, 200),
        ("o2000", 1, 2000)]


def one_run(name, n_frames, n_obs, reps, ref_frames):
    import refloc
    from miba.solver import Solver
    from oracle import oracle
    prob = refloc.frames_problem([n_obs] * n_frames, seed=100 + n_frames + n_obs, n_cloud=max(2000, n_obs))
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = prob.copy()
        s.localize(warm)
        outs = []
        for _ in range(reps):
            q = prob.copy()
            r = s.localize(q)
            if not np.array_equal(q.cams, warm.cams):
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
    st = outs[0]["stats"]
    iters = st[:, 3]
    rep = dict(run=name, keyframes=n_frames, obs_per_keyframe=n_obs, n_obs_total=int(prob.n_obs), reps=reps,
               n_solved=int(outs[0]["n_solved"]), n_convergence=int(outs[0]["n_convergence"]),
               n_no_convergence=int(outs[0]["n_no_convergence"]), n_failure=int(outs[0]["n_failure"]),
               iterations_total=int(iters.sum()), iterations_max=int(iters.max()),
               iterations_mean=round(float(iters.mean()), 3),
               cost_initial_mean=float(st[:, 1].mean()), cost_final_mean=float(st[:, 2].mean()))
    for k in ("time_lm_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(o[k], 4) for o in outs]
        rep[k] = round(statistics.median(o[k] for o in outs), 4)
    rep["us_per_keyframe"] = round(1e3 * rep["time_lm_ms"] / n_frames, 3)
    rep["us_per_keyframe_iteration"] = round(1e3 * rep["time_lm_ms"] / max(rep["iterations_total"], 1), 3)
    rep["us_per_keyframe_whole_call"] = round(1e3 * rep["time_total_ms"] / n_frames, 3)
    m = min(ref_frames, n_frames)
    o = oracle.default_options()
    t0 = time.perf_counter()
    ref_iters = sum(refloc.lm(prob, c, o)["iterations"] for c in range(m))
    ref_ms = 1e3 * (time.perf_counter() - t0)
    rep["python_reference"] = dict(keyframes=m, iterations_total=int(ref_iters), wall_ms=round(ref_ms, 2),
                                   ms_per_keyframe=round(ref_ms / m, 2))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-frames", type=int, default=4)
    ap.add_argument("--runs", default=",".join(r[0] for r in RUNS))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("localize_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    for name, n_frames, n_obs in RUNS:
        if name not in want:
            continue
        rep = one_run(name, n_frames, n_obs, args.reps, args.ref_frames)
        print(json.dumps(rep))
        with open(os.path.join(args.out_dir, f"localize_{name}.json"), "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
