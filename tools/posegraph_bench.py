#!/usr/bin/env python3
"""Measure ba_pose_graph (Solver.pose_graph) on one GPU, in one process.

    python tools/posegraph_bench.py [--out-dir profiles] [--reps 5] [--runs g2,g1,c5]

Runs: two-sweep trajectories (tests/refpg.loop_closure_graph) of G2 / G1 / C5 size, 50, 200 and 1000 keyframes. The
estimates carry a random-walk drift, the odometry edges are measured on the drifted estimates and a handful of loop
edges on the truth; keyframe 0 is constant. Written to posegraph_<run>.json. Per run a warm call and then --reps calls
from the same start: ``time_kernels_ms`` (the LM iterations' kernels, HIP events), ``time_solve_ms`` (the reduced
solve's part of it) and ``time_total_ms`` (the whole call: ordering, uploads, loop, copies back), their medians and
every value; the kernel time per LM iteration and the reduced solve's share; iterations; the translation RMS error
against the truth before and after; one more call with per-kernel events for the reduced solve's launches (the
stage's own six kernels carry no profiling ids; their launches are counted from the iterations). The
repeats must give the same bits (checked). For scale: the wall time of the plain-Python reference loop
(tests/refpg.lm, f64, dense numpy solves; the reference of the tests, not an optimised host implementation), and at
G2 / G1 the time of ``solve(order="auto")`` on a map built on the same drifted trajectory (landmarks above the
circuit, each placed through its first observer's drifted pose), as given and after the pose-graph pass with
``transfer_points``. Nothing here is a target; the numbers are reported as measured.
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

RUNS = [("g2", 50, 4), ("g1", 200, 8), ("c5", 1000, 16)]


def drifted_map(g, per_keyframe=20, seed=0):
    """A window on the graph's trajectory: landmarks in front of every keyframe (the cameras look along world z),
    observed by every keyframe whose image they fall into; the cameras are the drifted estimates and each landmark is
    placed through its first observer's drifted pose."""
    from miba import posegraph
    from miba.capi import ProblemArrays
    from miba.synthetic import IMAGE_H, IMAGE_W, ROS_DEFAULT_INTRINSICS
    rng = np.random.default_rng(seed)
    truth, est = g["truth"], g["cams"]
    n = len(truth)
    K = ROS_DEFAULT_INTRINSICS.copy()
    local = np.stack([rng.uniform(-1.0, 1.0, n * per_keyframe), rng.uniform(-0.8, 0.8, n * per_keyframe),
                      rng.uniform(2.5, 5.0, n * per_keyframe)], 1)
    owner = np.repeat(np.arange(n), per_keyframe)
    X = truth[owner, 4:] + posegraph.quat_rotate(truth[owner, :4], local)
    oc, op, uv, dep = [], [], [], []
    for c in range(n):
        pc = posegraph.quat_rotate(posegraph.quat_conj(truth[c, :4]), X - truth[c, 4:])
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = K[0] * pc[:, 0] / z + K[2], K[1] * pc[:, 1] / z + K[3]
        vis = np.nonzero((z > 0.5) & (u >= 0) & (u < IMAGE_W) & (v >= 0) & (v < IMAGE_H))[0]
        oc.append(np.full(len(vis), c)); op.append(vis)
        uv.append(np.stack([u[vis], v[vis]], 1) + rng.normal(0, 0.3, (len(vis), 2)))
        dep.append(z[vis] * (1 + rng.normal(0, 0.005, len(vis))))
    oc, op = np.concatenate(oc), np.concatenate(op)
    first = np.full(len(X), n, dtype=np.int64)
    np.minimum.at(first, op, oc)
    pts = posegraph.transfer_points(X, first, truth, est)
    prob = ProblemArrays(est.copy(), pts, K, K.copy(), oc.astype(np.int32), op.astype(np.int32), np.concatenate(uv),
                         np.concatenate(dep), fixed_cam=0)
    return prob, first


def one_run(name, n, n_loops, reps, with_ref, with_ba):
    import refpg
    from miba import posegraph
    from miba.solver import Solver
    from oracle import oracle
    g = refpg.loop_closure_graph(n=n, seed=5, n_loops=n_loops)
    args = (g["ea"], g["eb"], g["meas"])
    kw = dict(constant=g["constant"])
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = s.pose_graph(g["cams"].copy(), *args, **kw)
        outs = []
        for _ in range(reps):
            r = s.pose_graph(g["cams"].copy(), *args, **kw)
            if not np.array_equal(r["cams"], warm["cams"]):
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
    with Solver(minimizer_progress_to_stdout=0, profile_kernels=1) as s:
        s.pose_graph(g["cams"].copy(), *args, **kw)
        s.reset_kernel_stats()
        pr = s.pose_graph(g["cams"].copy(), *args, **kw)
        kstats = [k for k in s.kernel_stats() if k["launches"]]
    o0 = outs[0]
    it = max(int(o0["iterations"]), 1)
    rep = dict(run=name, keyframes=n, edges=int(len(g["ea"])), loop_edges=n_loops, reps=reps,
               n_active=int(o0["n_active"]), reduced_system_size=int(o0["reduced_system_size"]),
               band_before=int(o0["band_before"]), band_after=int(o0["band_after"]), iterations=int(o0["iterations"]),
               successful_steps=int(o0["n_successful"]), unsuccessful_steps=int(o0["n_unsuccessful"]),
               termination_type=int(o0["termination_type"]), message=o0["message"],
               cost_initial=float(o0["initial_cost"]), cost_final=float(o0["final_cost"]),
               rms_before_m=round(refpg.pose_rms(g["cams"], g["truth"]), 5),
               rms_after_m=round(refpg.pose_rms(o0["cams"], g["truth"]), 5))
    for k in ("time_kernels_ms", "time_solve_ms", "time_order_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(o[k], 4) for o in outs]
        rep[k] = round(statistics.median(o[k] for o in outs), 4)
    rep["kernel_ms_per_iteration"] = round(rep["time_kernels_ms"] / it, 4)
    rep["reduced_solve_share"] = round(rep["time_solve_ms"] / max(rep["time_kernels_ms"], 1e-9), 3)
    rep["kernels_profiled"] = [dict(name=k["name"], launches=int(k["launches"]), total_ms=round(k["total_ms"], 4),
                                    launches_per_iteration=round(k["launches"] / max(int(pr["iterations"]), 1), 1))
                               for k in kstats]
    # the stage's own kernels carry no profiling ids: 4 launches per iteration (assemble, step, candidate, decide) and
    # 2 more (edge records, gather) after every accepted step
    own = 4 * int(pr["iterations"]) + 2 * max(int(pr["n_successful"]) - 1, 0)
    rep["launches_per_iteration"] = round((sum(k["launches"] for k in kstats) + own) / max(int(pr["iterations"]), 1), 1)
    if with_ref:
        t0 = time.perf_counter()
        ref = refpg.lm(g, oracle.default_options(), np.float64)
        ref_ms = 1e3 * (time.perf_counter() - t0)
        rep["python_reference"] = dict(iterations=int(ref["iterations"]), wall_ms=round(ref_ms, 1),
                                       cost_final=float(ref["final_cost"]),
                                       rms_after_m=round(refpg.pose_rms(ref["cams"], g["truth"]), 5))
    if with_ba:
        prob, first = drifted_map(g)
        with Solver(minimizer_progress_to_stdout=0) as s:
            s.solve(prob.copy(), order="auto")  # warm
            a = prob.copy()
            sa = s.solve(a, order="auto")
            b = prob.copy()
            pg = s.pose_graph(b.cams, *args, **kw)
            b.points[:] = posegraph.transfer_points(prob.points, first, prob.cams, b.cams)
            sb = s.solve(b, order="auto")
        pick = ("initial_cost", "final_cost", "num_iterations", "termination_type", "time_total_ms", "time_lm_ms")
        rep["bundle_adjustment"] = dict(
            n_points=int(prob.n_points), n_obs=int(prob.n_obs),
            as_given=dict({k: sa[k] for k in pick}, rms_after_m=round(refpg.pose_rms(a.cams, g["truth"]), 5)),
            after_pose_graph=dict({k: sb[k] for k in pick}, rms_after_m=round(refpg.pose_rms(b.cams, g["truth"]), 5),
                                  pose_graph_total_ms=round(pg["time_total_ms"], 4)))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", default=",".join(r[0] for r in RUNS))
    ap.add_argument("--ref-max", type=int, default=1000, help="largest run that also times the Python reference")
    ap.add_argument("--device-note", default="", help="where the numbers were measured (recorded in the file)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("posegraph_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    for name, n, n_loops in RUNS:
        if name not in want:
            continue
        rep = one_run(name, n, n_loops, args.reps, n <= args.ref_max, n <= 200)
        rep["device"] = args.device_note or torch.cuda.get_device_name(0)
        print(json.dumps(rep))
        with open(os.path.join(args.out_dir, f"posegraph_{name}.json"), "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
