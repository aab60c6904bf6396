#!/usr/bin/env python3
"""Measure ba_guided_match (Solver.guided_match) on one GPU, in one process.

    python tools/gmatch_bench.py [--out-dir profiles] [--reps 7] [--runs ...] [--kinds hamming,l2_u8] [--cells 8,16,32,64]

Runs, written to gmatch_<kind>_<run>.json for both kinds (HAMMING at 32 bytes, L2_U8 at 128), all at a radius of 15 px
on 640 x 480: f1 (1 frame x 2000 keypoints x 5000 landmarks: a keyframe against the local map), f64 (64 frames of
that, each with keypoints of its own: a window's keyframes in one call) and h1024 (1024 pose hypotheses sharing one
2000-keypoint range x 500 landmarks: one binned grid). The landmarks project into the image; three keypoints of four
are observations of a landmark (2 px of noise, a disturbed copy of its descriptor), the rest random. Per run a warm
call and then --reps calls: ``time_kernels_ms`` (the launches, HIP events) and ``time_total_ms`` (the whole call:
validation, layout, uploads, kernels, copies back), their medians and every value; the repeats must give the same
bits (checked). ``cell_sweep``: the kernels' median at every --cells value (the same bits, checked).

The comparison column is what the library could do before this stage, timed in the same process: ``Solver.match`` of
the same landmark descriptors against the same keypoints (one pair per distinct keypoint range: the hypotheses of
h1024 share one), then per frame the projection in numpy and the pixel-distance filter on the first neighbour
(``match_plus_filter``: the match call's kernels and whole call, the numpy part, their sum; median of --reps after a
warm run). It answers a different question (the nearest descriptor of the whole image, then whether it is near), so
its accepted count is reported beside the stage's, not compared.

``--table`` prints the README's table from the files written. Nothing here is a target; the numbers are as measured.
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

# name, frame entries, landmarks, one shared keypoint range
RUNS = [("f1", 1, 5000, False), ("f64", 64, 5000, False), ("h1024", 1024, 500, True)]
N_KP = 2000
KINDS = ("hamming", "l2_u8")
BYTES = {"hamming": 32, "l2_u8": 128}
LEVEL = {"hamming": 0.06, "l2_u8": 10.0}
W, H, RADIUS = 640, 480, 15.0
K = np.array([525.0, 525.0, 319.5, 239.5])
KEYS = ("nn_kp", "nn_dist", "status", "n_in_window", "matches", "match_begin")


def _pose(rng, scale):
    w = rng.normal(0, scale, 3)
    a = np.linalg.norm(w)
    q = np.concatenate([np.sin(a / 2) * w / a, [np.cos(a / 2)]])
    return np.concatenate([q, rng.normal(0, 2 * scale, 3)])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def project(X, pose):
    pc = (X - pose[4:]) @ _rot(pose[:4])
    return K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3], pc[:, 2]


def scene(kind, n_frames, n_lm, shared):
    from miba import matching
    rng = np.random.default_rng(700 + n_frames + n_lm)
    nb = BYTES[kind]
    px = np.stack([rng.uniform(20, W - 20, n_lm), rng.uniform(20, H - 20, n_lm)], axis=1)
    z = rng.uniform(2.0, 6.0, n_lm)
    X = np.stack([(px[:, 0] - K[2]) / K[0] * z, (px[:, 1] - K[3]) / K[1] * z, z], axis=1)  # the base camera is the world
    desc = rng.integers(0, 256, size=(n_lm, nb), dtype=np.uint8)
    poses = np.stack([_pose(rng, 0.004) for _ in range(n_frames)])
    uv, kd, kz = [], [], []
    for f in range(1 if shared else n_frames):
        u, v, zc = project(X, poses[f])
        seen = rng.permutation(n_lm)[: min(3 * N_KP // 4, n_lm)]
        obs = np.stack([u[seen], v[seen]], axis=1) + rng.normal(0, 2.0, (len(seen), 2))
        rest = N_KP - len(seen)
        uv.append(np.concatenate([obs, np.stack([rng.uniform(0, W, rest), rng.uniform(0, H, rest)], axis=1)]))
        kd.append(np.concatenate([matching.disturb(rng, desc[seen], kind, LEVEL[kind]),
                                  rng.integers(0, 256, size=(rest, nb), dtype=np.uint8)]))
        kz.append(np.concatenate([zc[seen], rng.uniform(2.0, 6.0, rest)]))
    rng_f = np.array([[0, N_KP] if shared else [f * N_KP, (f + 1) * N_KP] for f in range(n_frames)], dtype=np.int32)
    return dict(points=X, pt_desc=desc, kp_uv=np.concatenate(uv), kp_desc=np.concatenate(kd), kp_depth=np.concatenate(kz),
                frame_pose=poses, intr=K, width=W, height=H, frame_range=rng_f)


def match_plus_filter(s, sc, kind, reps):
    """Solver.match of the landmark descriptors against every distinct keypoint range, then numpy per frame."""
    ranges = np.unique(sc["frame_range"], axis=0)
    pr = np.array([[0, len(sc["pt_desc"]), b, e] for b, e in ranges], dtype=np.int32)
    pair_of = {(int(b), int(e)): j for j, (b, e) in enumerate(ranges)}

    def once():
        t0 = time.perf_counter()
        m = s.match(sc["pt_desc"], sc["kp_desc"], pr, kind=kind, matches=False)
        t1 = time.perf_counter()
        n_acc = 0
        for f, (b, e) in enumerate(sc["frame_range"].tolist()):
            j = pair_of[(b, e)]
            r0, r1 = m["row_begin"][j], m["row_begin"][j + 1]
            u, v, z = project(sc["points"], sc["frame_pose"][f])
            k = m["nn_idx"][r0:r1, 0]
            near = sc["kp_uv"][b + np.maximum(k, 0)]
            ok = (m["accept"][r0:r1] == 1) & (z > 1e-15) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & \
                 ((near[:, 0] - u) ** 2 + (near[:, 1] - v) ** 2 <= RADIUS * RADIUS)
            n_acc += int(ok.sum())
        t2 = time.perf_counter()
        return m["time_kernels_ms"], m["time_total_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), n_acc

    once()
    runs = [once() for _ in range(reps)]
    med = lambda i: round(statistics.median(r[i] for r in runs), 4)  # noqa: E731
    return dict(match_pairs=int(len(pr)), match_kernels_ms=med(0), match_total_ms=med(1), match_wall_ms=med(2), numpy_filter_ms=med(3),
                whole_ms=round(statistics.median(r[2] + r[3] for r in runs), 4), n_accepted=runs[0][4])


def one_run(kind, name, n_frames, n_lm, shared, reps, cells):
    from miba.solver import Solver
    sc = scene(kind, n_frames, n_lm, shared)
    kw = dict(kind=kind, radius=RADIUS)
    with Solver(minimizer_progress_to_stdout=0) as s:
        warm = s.guided_match(**sc, **kw)
        outs = []
        for _ in range(reps):
            r = s.guided_match(**sc, **kw)
            if any(r[k].tobytes() != warm[k].tobytes() for k in KEYS):
                raise RuntimeError(f"{name}: a repeat gave different bits")
            outs.append(r)
        sweep = {}
        for cell in cells:
            rs = [s.guided_match(**sc, cell_px=cell, **kw) for _ in range(reps + 1)][1:]
            if any(r[k].tobytes() != warm[k].tobytes() for r in rs for k in KEYS):
                raise RuntimeError(f"{name}: cell_px = {cell} gave different bits")
            sweep[str(cell)] = round(statistics.median(r["time_kernels_ms"] for r in rs), 4)
        rep = dict(run=name, kind=kind, desc_bytes=BYTES[kind], frames=n_frames, keypoints_per_range=N_KP, landmarks=n_lm,
                   shared_range=bool(shared), radius=RADIUS, width=W, height=H, reps=reps, n_rows=int(warm["n_rows"]),
                   n_matches=int(warm["n_matches"]), n_grids=int(warm["n_grids"]), cell_px=int(warm["cell_px"]),
                   mean_in_window=round(float(warm["n_in_window"].mean()), 2))
        for k in ("time_kernels_ms", "time_total_ms"):
            rep[k + "_runs"] = [round(o[k], 4) for o in outs]
            rep[k] = round(statistics.median(o[k] for o in outs), 4)
        rep["mrows_per_s"] = round(rep["n_rows"] / (rep["time_kernels_ms"] * 1e3), 2)
        rep["cell_sweep_kernels_ms"] = sweep
        rep["match_plus_filter"] = match_plus_filter(s, sc, kind, reps)
    return rep


def table(out_dir):
    print("| kind | frames x landmarks (keypoints per range) | kernels ms | whole call ms | accepted | match + numpy filter: kernels / whole ms |")
    print("|---|---|---|---|---|---|")
    for kind in KINDS:
        for name, n_frames, n_lm, shared in RUNS:
            path = os.path.join(out_dir, f"gmatch_{kind}_{name}.json")
            if not os.path.exists(path):
                continue
            r = json.load(open(path))
            m = r["match_plus_filter"]
            print(f"| {kind} {r['desc_bytes']} B | {n_frames} x {n_lm} ({N_KP}{', one shared range' if shared else ''}) | "
                  f"{r['time_kernels_ms']:.3f} | {r['time_total_ms']:.3f} | {r['n_matches']} | "
                  f"{m['match_kernels_ms']:.3f} / {m['whole_ms']:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", default=",".join(r[0] for r in RUNS))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--cells", default="8,16,32,64")
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    if args.table:
        return table(args.out_dir)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gmatch_bench needs a GPU")
    os.makedirs(args.out_dir, exist_ok=True)
    want = set(args.runs.split(","))
    cells = [int(c) for c in args.cells.split(",") if c]
    for kind in args.kinds.split(","):
        for r in RUNS:
            if r[0] not in want:
                continue
            rep = one_run(kind, *r, args.reps, cells)
            rep["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(rep), flush=True)
            with open(os.path.join(args.out_dir, f"gmatch_{kind}_{rep['run']}.json"), "w") as f:
                json.dump(rep, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
