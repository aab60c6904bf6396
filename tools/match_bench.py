#!/usr/bin/env python3
"""Measure ba_match (Solver.match) on one GPU, in one process.

    python tools/match_bench.py [--out-dir profiles] [--reps 7] [--runs ...] [--kinds hamming,l2_u8]

Runs (pairs x (queries x trains)), written to match_<kind>_<run>.json for both kinds (HAMMING at 32 bytes, ORB's;
L2_U8 at 128, byte SIFT's): p1n500 (the tracker's call) and p1n2000; p64n500 (loop candidates, one descriptor set
per keyframe) and p256n2000 (relocalisation: one shared query set against 256 train sets). The trains are random
descriptors, the queries disturbed copies of half of them (miba.matching.disturb) and random ones. Per run a warm
call (code object loaded, buffers grown) and then --reps calls: ``time_kernels_ms`` (the launches, HIP events) and
``time_total_ms`` (the whole call: uploads, kernels, copies back), their medians and every value. The repeats must
give the same bits (checked). Beside them the same statement in torch on the same GPU, timed between
synchronisations, median of --reps after a warm run:

* HAMMING: a broadcast xor, a 256-entry popcount table, the sum over the bytes and ``topk(2, largest=False)``;
* L2_U8: ``torch.cdist`` on the values widened to f32, squared, and the same ``topk``;

both chunked over the queries to bound the intermediate at --torch-gb, on the first --torch-pairs pairs (the time of
all pairs is that times pairs / torch-pairs: ``wall_ms_scaled``). torch's neighbours are compared with ba_match's
where the distances are exact in its arithmetic (HAMMING).

For L2_U8 the achieved i8 multiply-accumulate rate is reported: pairs x queries x trains x the descriptor bytes padded
to the k-step, over the kernel time.

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
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# name, pairs, descriptors per set, one shared query set
RUNS = [("p1n500", 1, 500, False), ("p1n2000", 1, 2000, False), ("p64n500", 64, 500, False), ("p256n2000", 256, 2000, True)]
KINDS = ("hamming", "l2_u8")
BYTES = {"hamming": 32, "l2_u8": 128}
LEVEL = {"hamming": 0.06, "l2_u8": 10.0}
KSTEP = 64  # csrc/ba_match.h: MATCH_KSTEP


def batch(kind, n_pairs, n, shared):
    from miba import matching
    rng = np.random.default_rng(900 + n_pairs + n)
    nb = BYTES[kind]
    train = rng.integers(0, 256, size=(n_pairs * n, nb), dtype=np.uint8)
    n_sets = 1 if shared else n_pairs
    query = rng.integers(0, 256, size=(n_sets * n, nb), dtype=np.uint8)
    for j in range(n_sets):  # half of a query set: copies of its own train set's descriptors
        src = rng.permutation(n)[: n // 2]
        query[j * n: j * n + n // 2] = matching.disturb(rng, train[j * n + src], kind, LEVEL[kind])
    pr = np.array([[0 if shared else j * n, n if shared else (j + 1) * n, j * n, (j + 1) * n] for j in range(n_pairs)],
                  dtype=np.int32)
    return query, train, pr


def torch_statement(kind, query, train, pr, reps, max_gb, max_pairs):
    import torch
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    pairs = pr[:max_pairs]
    Q, T = torch.from_numpy(query).to(dev), torch.from_numpy(train).to(dev)
    pop = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.uint8, device=dev)
    nb = query.shape[1]
    nt_max = int((pairs[:, 3] - pairs[:, 2]).max())
    # HAMMING: the (chunk, n_t, B) xor as int32 indices and the looked-up bytes; L2_U8: the (chunk, n_t) f32 matrix
    per_query = nt_max * (nb * 6.0 if kind == "hamming" else 16.0)
    chunk = max(1, int(max_gb * 2**30 / per_query))

    def once():
        out = []
        for qb, qe, tb, te in pairs.tolist():
            t = T[tb:te]
            tf = t.float() if kind == "l2_u8" else None
            for a in range(qb, qe, chunk):
                q = Q[a:min(a + chunk, qe)]
                if kind == "hamming":
                    d = pop[(q[:, None, :] ^ t[None, :, :]).int()].sum(-1, dtype=torch.int32)
                else:
                    d = torch.cdist(q.float(), tf) ** 2
                out.append(torch.topk(d, 2, dim=1, largest=False))
        return out

    first = once()
    sync()
    ms = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        once()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    med = statistics.median(ms)
    nn_dist = torch.cat([v for v, _ in first]).cpu().numpy()
    return dict(wall_ms_runs=[round(x, 4) for x in ms], wall_ms=round(med, 4), pairs=int(len(pairs)), queries_per_chunk=chunk,
                wall_ms_scaled=round(med * len(pr) / len(pairs), 4)), nn_dist


def one_run(kind, name, n_pairs, n, shared, reps, max_gb, torch_pairs):
    from miba.solver import Solver
    query, train, pr = batch(kind, n_pairs, n, shared)
    keys = ("nn_idx", "nn_dist", "accept", "matches", "match_begin")
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = s.match(query, train, pr, kind=kind)
        outs = []
        for _ in range(reps):
            r = s.match(query, train, pr, kind=kind)
            if any(r[k].tobytes() != warm[k].tobytes() for k in keys):
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
        cross = [s.match(query, train, pr, kind=kind, cross_check=True) for _ in range(3)][-1]
    rep = dict(run=name, kind=kind, desc_bytes=BYTES[kind], pairs=n_pairs, queries_per_pair=n, trains_per_pair=n,
               shared_query_set=bool(shared), reps=reps, n_matches=int(warm["n_matches"]))
    for k in ("time_kernels_ms", "time_total_ms"):
        rep[k + "_runs"] = [round(o[k], 4) for o in outs]
        rep[k] = round(statistics.median(o[k] for o in outs), 4)
    rep["cross_check_time_kernels_ms"] = round(cross["time_kernels_ms"], 4)
    dist = float(n_pairs) * n * n
    rep["gdistances_per_s"] = round(dist / (rep["time_kernels_ms"] * 1e6), 2)
    if kind == "l2_u8":
        kpad = (BYTES[kind] + KSTEP - 1) // KSTEP * KSTEP
        rep["i8_tmac_per_s"] = round(dist * kpad / (rep["time_kernels_ms"] * 1e9), 3)
    rep["torch"], t_dist = torch_statement(kind, query, train, pr, reps, max_gb, torch_pairs)
    mine = warm["nn_dist"][: len(t_dist)]
    if kind == "hamming":  # exact in torch's integers too
        if not np.array_equal(mine, t_dist.astype(np.int32)):
            raise RuntimeError(f"{name}: torch's distances differ")
        rep["torch"]["same_distances"] = True
    else:  # cdist's f32 rounds: the relative difference is reported
        rep["torch"]["max_rel_distance_diff"] = float(np.abs(t_dist - mine).max() / max(1, mine.max()))
    return rep


def table(out_dir):
    print("| kind | pairs x (queries x trains) | kernels ms | whole call ms | cross-check kernels ms | torch ms | G distances / s |")
    print("|---|---|---|---|---|---|---|")
    for kind in KINDS:
        for name, n_pairs, n, shared in RUNS:
            path = os.path.join(out_dir, f"match_{kind}_{name}.json")
            if not os.path.exists(path):
                continue
            r = json.load(open(path))
            t = r["torch"]
            torch_ms = f"{t['wall_ms_scaled']:.2f}" + ("" if t["pairs"] == n_pairs else f" ({t['pairs']} pairs timed, scaled)")
            print(f"| {kind} {r['desc_bytes']} B | {n_pairs} x ({n} x {n}){', one query set' if shared else ''} | "
                  f"{r['time_kernels_ms']:.3f} | {r['time_total_ms']:.3f} | {r['cross_check_time_kernels_ms']:.3f} | {torch_ms} | "
                  f"{r['gdistances_per_s']:.1f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-gb", type=float, default=1.0)
    ap.add_argument("--torch-pairs", type=int, default=8)
    ap.add_argument("--runs", default=",".join(r[0] for r in RUNS))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return table(args.out_dir)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("match_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    for kind in args.kinds.split(","):
        for r in RUNS:
            if r[0] not in want:
                continue
            rep = one_run(kind, *r, args.reps, args.torch_gb, args.torch_pairs)
            rep["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(rep), flush=True)
            with open(os.path.join(args.out_dir, f"match_{kind}_{rep['run']}.json"), "w") as f:
                json.dump(rep, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
