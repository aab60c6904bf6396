#!/usr/bin/env python3
"""Measure ba_align (Solver.align) on one GPU, in one process.

    python tools/align_bench.py [--out-dir profiles] [--reps 7] [--runs ...]

Runs (pairs x correspondences @ hypotheses), written to align_<run>.json: p1n200 (the tracker's call) and p1n2000 at
256 hypotheses; p64n500 and p1024n500 (loop candidates, relocalisation) at 256 and at 1024. Every pair is
tests/refalign.make_pair's: a rigid motion, 1 cm of noise, 40 % outliers. Per run a warm call (code object loaded,
buffers grown) and then --reps calls: ``time_kernels_ms`` (the two kernels, HIP events) and ``time_total_ms`` (the whole
call: uploads, kernels, copies back), their medians and every value. The repeats must give the same bits (checked).
Beside them:

* the same batch stated in torch f64 on the same GPU: the sample triples gathered, Arun's fit by a batched
  ``torch.linalg.svd``, the inlier counts by a broadcast distance and the argmax (chunked by pairs to bound the
  (pairs, hypotheses, correspondences) intermediate at --torch-gb), timed between synchronisations: median of --reps
  after a warm run. Its samples are torch's own random triples: the same work, not the same bits;
* ``tests/refalign.py``'s Python loop (the longdouble reference of the tests, not an optimised host implementation) on
  the first --ref-pairs pairs;
* pg200: tools/posegraph_bench.py's 200-keyframe graph with its 8 loop edges measured by
  ``posegraph.measured_edges`` on the drifted map instead of read off the truth: the translation RMS error against the
  truth before and after ``Solver.pose_graph``, beside the same graph with the loop edges from the truth.

``--table`` prints the README's table from the files written. Nothing here is a target; the numbers are reported as
measured.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# name, pairs, correspondences per pair, hypotheses
RUNS = [("p1n200", 1, 200, 256), ("p1n2000", 1, 2000, 256), ("p64n500", 64, 500, 256), ("p64n500h1024", 64, 500, 1024),
        ("p1024n500", 1024, 500, 256), ("p1024n500h1024", 1024, 500, 1024)]
THR = 0.1


def batch(n_pairs, n):
    import refalign
    # a few distinct pairs, repeated: the work per pair is what is measured
    base = [refalign.make_pair(n, 0.4, seed=500 + k)[:2] for k in range(min(n_pairs, 8))]
    p1 = np.concatenate([base[j % len(base)][0] for j in range(n_pairs)])
    p2 = np.concatenate([base[j % len(base)][1] for j in range(n_pairs)])
    return p1, p2, (np.arange(n_pairs + 1) * n).astype(np.int32)


def torch_statement(p1, p2, n_pairs, n, n_hyp, reps, max_gb):
    import torch
    dev = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    P1 = torch.from_numpy(p1).to(dev).reshape(n_pairs, n, 3)
    P2 = torch.from_numpy(p2).to(dev).reshape(n_pairs, n, 3)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d0, d1, d2 = (torch.randint(0, n - k, (n_pairs, n_hyp), device=dev, generator=gen) for k in range(3))
    i1 = d1 + (d1 >= d0)
    lo, hi = torch.minimum(d0, i1), torch.maximum(d0, i1)
    i2 = d2 + (d2 >= lo)
    i2 = i2 + (i2 >= hi)
    idx = torch.stack([d0, i1, i2], -1)  # distinct triples, uniform
    chunk = max(1, min(n_pairs, int(max_gb * 2**30 / (8.0 * 4 * n_hyp * n))))

    def once():
        best = torch.empty(n_pairs, dtype=torch.int64, device=dev)
        count = torch.empty(n_pairs, dtype=torch.int64, device=dev)
        for a in range(0, n_pairs, chunk):
            q1, q2, ix = P1[a:a + chunk], P2[a:a + chunk], idx[a:a + chunk]
            pi = torch.arange(len(q1), device=dev)[:, None, None]
            S1, S2 = q1[pi, ix], q2[pi, ix]  # (p, H, 3, 3)
            c1, c2 = S1.mean(2), S2.mean(2)
            Hm = (S2 - c2[:, :, None]).transpose(-1, -2) @ (S1 - c1[:, :, None])
            U, _, Vh = torch.linalg.svd(Hm)
            V, Ut = Vh.transpose(-1, -2), U.transpose(-1, -2)
            d = torch.sign(torch.linalg.det(V @ Ut))
            R = torch.cat([V[..., :2], V[..., 2:] * d[..., None, None]], -1) @ Ut
            t = c1 - torch.einsum("phik,phk->phi", R, c2)
            pred = torch.einsum("phik,pnk->phni", R, q2) + t[:, :, None, :]
            cnt = (((q1[:, None] - pred) ** 2).sum(-1) < THR * THR).sum(-1)
            count[a:a + chunk], best[a:a + chunk] = cnt.max(1)
        return best, count

    once()
    sync()
    ms = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        _, count = once()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(wall_ms_runs=[round(x, 4) for x in ms], wall_ms=round(statistics.median(ms), 4), pairs_per_chunk=chunk,
                best_count_mean=float(count.double().mean()))


def one_run(name, n_pairs, n, n_hyp, reps, ref_pairs, max_gb):
    import refalign
    from miba.solver import Solver
    p1, p2, begin = batch(n_pairs, n)
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = s.align(p1, p2, begin, n_hypotheses=n_hyp, seed=1, threshold=THR)
        outs = []
        for _ in range(reps):
            r = s.align(p1, p2, begin, n_hypotheses=n_hyp, seed=1, threshold=THR)
            if r["poses"].tobytes() != warm["poses"].tobytes() or r["inlier"].tobytes() != warm["inlier"].tobytes():
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
        refit = [s.align(p1, p2, begin, n_hypotheses=n_hyp, seed=1, threshold=THR, refit=3) for _ in range(3)][-1]
    st = outs[0]["stats"]
    rep = dict(run=name, pairs=n_pairs, correspondences_per_pair=n, hypotheses=n_hyp, reps=reps, n_ok=int(outs[0]["n_ok"]),
               inliers_mean=float(st[:, 2].mean()), k_needed_max=float(st[:, 7].max()))
    for k in ("time_kernels_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(o[k], 4) for o in outs]
        rep[k] = round(statistics.median(o[k] for o in outs), 4)
    rep["refit3_time_kernels_ms"] = round(refit["time_kernels_ms"], 4)
    rep["us_per_pair"] = round(1e3 * rep["time_kernels_ms"] / n_pairs, 3)
    # 15 f64 operations per hypothesis and correspondence, a fused multiply-add counted as two floating-point operations
    rep["gflops_scoring"] = round(27.0 * n_pairs * n_hyp * n / (rep["time_kernels_ms"] * 1e6), 2)
    rep["torch_f64"] = torch_statement(p1, p2, n_pairs, n, n_hyp, reps, max_gb)
    m = min(ref_pairs, n_pairs)
    t0 = time.perf_counter()
    refalign.align(p1[:begin[m]], p2[:begin[m]], begin[:m + 1], n_hypotheses=n_hyp, seed=1, threshold=THR)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    rep["python_reference"] = dict(pairs=m, wall_ms=round(ref_ms, 2), ms_per_pair=round(ref_ms / m, 2))
    return rep


def pose_graph_run():
    import refpg
    from miba import posegraph
    from miba.solver import Solver
    from posegraph_bench import drifted_map
    g = refpg.loop_closure_graph(n=200, seed=5, n_loops=8)
    n = len(g["truth"])
    prob, _ = drifted_map(g)
    loops = np.stack([g["ea"][n - 1:], g["eb"][n - 1:]], 1)
    with Solver(minimizer_progress_to_stdout=0) as s:
        ea, eb, meas, n_in = posegraph.measured_edges(prob, loops, s.align, seed=1, refit=3)
        truth_run = s.pose_graph(g["cams"].copy(), g["ea"], g["eb"], g["meas"], constant=g["constant"])
        kept = np.concatenate([np.arange(n - 1), n - 1 + np.nonzero([(a, b) in set(zip(ea.tolist(), eb.tolist()))
                                                                     for a, b in loops])[0]])
        z = g["meas"][kept].copy()
        z[n - 1:] = meas
        meas_run = s.pose_graph(g["cams"].copy(), g["ea"][kept], g["eb"][kept], z, constant=g["constant"])
    _, _, z_true = posegraph.edges_from_poses(g["truth"], np.stack([ea, eb], 1))
    return dict(run="pg200", keyframes=n, loop_edges=int(len(loops)), loop_edges_measured=int(len(ea)),
                inliers=n_in.tolist(), loop_edge_translation_error_m=[round(float(x), 5) for x in
                                                                      np.linalg.norm(meas[:, 4:] - z_true[:, 4:], axis=1)],
                rms_before_m=round(refpg.pose_rms(g["cams"], g["truth"]), 5),
                rms_after_truth_edges_m=round(refpg.pose_rms(truth_run["cams"], g["truth"]), 5),
                rms_after_measured_edges_m=round(refpg.pose_rms(meas_run["cams"], g["truth"]), 5),
                iterations_truth_edges=int(truth_run["iterations"]), iterations_measured_edges=int(meas_run["iterations"]))


def table(out_dir):
    print("| pairs x n @ hypotheses | kernels ms | whole call ms | refit 3 kernels ms | torch f64 ms | Python reference ms / pair |")
    print("|---|---|---|---|---|---|")
    for name, n_pairs, n, n_hyp in RUNS:
        path = os.path.join(out_dir, f"align_{name}.json")
        if not os.path.exists(path):
            continue
        r = json.load(open(path))
        print(f"| {n_pairs} x {n} @ {n_hyp} | {r['time_kernels_ms']:.3f} | {r['time_total_ms']:.3f} | "
              f"{r['refit3_time_kernels_ms']:.3f} | {r['torch_f64']['wall_ms']:.2f} | {r['python_reference']['ms_per_pair']:.0f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-pairs", type=int, default=2)
    ap.add_argument("--torch-gb", type=float, default=2.0)
    ap.add_argument("--runs", default=",".join([r[0] for r in RUNS] + ["pg200"]))
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return table(args.out_dir)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    reports = [one_run(*r, args.reps, args.ref_pairs, args.torch_gb) for r in RUNS if r[0] in want]
    if "pg200" in want:
        reports.append(pose_graph_run())
    for rep in reports:
        rep["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rep))
        with open(os.path.join(args.out_dir, f"align_{rep['run']}.json"), "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
