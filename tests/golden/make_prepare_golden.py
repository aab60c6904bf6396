#!/usr/bin/env python3
"""Generate tests/golden/prepare_golden.json: what ba_prepare decides and uploads for the smallest windows that
reach each branch of the prepare (plan kind, reduced-system solver, BCR path, launch paths, traffic model).

Run on the GPU with the library whose prepare is the reference (the commit before a change that must leave the
prepare as it is):
    python tests/golden/make_prepare_golden.py [out.json]
Each case prepares its window on a fresh context, without a solve, and records from last_prepare() the chosen
paths, from plan_digest() one digest per plan array as it lies in HBM, and from kernel_stats() every kernel's
modelled bytes and flops per launch. tests/test_gpu_prepare_golden.py prepares the same cases and compares all of
it exactly. Only data is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "prepare_golden.json")

# (window, MIBA_* settings, solver options)
CASES = [
    ("C1", {}, {}),
    ("C1", {"MIBA_BCR_BAND": "0"}, {}),
    ("C1", {"MIBA_BCR": "launch"}, {}),
    ("C3", {}, {}),
    ("C3", {"MIBA_TAIL": "0"}, {}),
    ("C3", {"MIBA_FUSED": "0"}, {}),
    ("C3", {"MIBA_SW": "0"}, {}),
    ("C2", {}, {}),  # 50k observations: the device plan
    ("C2", {"MIBA_DEVICE_PLAN": "0"}, {}),
    ("C2", {"MIBA_BSFIN": "1"}, {}),
    ("C2", {"MIBA_OBS32": "0"}, {}),
    ("C2", {}, {"deterministic": 1}),
    ("bcr21", {"MIBA_DEVICE_PLAN": "1"}, {}),
    ("bcr21_messy", {}, {}),
    ("dense_wide30", {}, {}),
    ("dense_wide30", {"MIBA_BLOCKED_MIN": "64"}, {}),
    ("dense_wide30", {"MIBA_SOLVER": "blocked"}, {}),
    ("sweep42", {}, {}),
]
INFO_KEYS = ("plan_device", "bcr_path", "lin_path", "tail", "bsfin", "plan_reused")


def case_id(case):
    name, env, opts = case
    return "-".join([name] + [f"{k}={v}" for k, v in sorted({**env, **opts}.items())]) if env or opts else name


def window(name):
    for p in (ROOT, os.path.join(ROOT, "3dsmc-bundle-adjustment_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from miba import synthetic
    import refstep
    import refsweep
    if name in synthetic.CONFIGS:
        return synthetic.make_config(name)
    return refsweep.window(name) if name in refsweep.SWEEPS else refstep.window(name)


def record(case):
    """Prepare the case's window on a fresh context under its settings; what the prepare decided, as JSON data."""
    name, env, opts = case
    prob = window(name).copy()
    from miba.solver import Solver
    old = {k: os.environ.get(k) for k in os.environ if k.startswith("MIBA_") and k != "MIBA_LIB_PATH"}
    for k in old:
        del os.environ[k]
    os.environ.update(env)
    try:
        with Solver(device=0, minimizer_progress_to_stdout=0, **opts) as s:
            s.prepare(prob)
            info = s.last_prepare()
            digest = s.plan_digest()
            stats = s.kernel_stats()
    finally:
        for k in env:
            del os.environ[k]
        os.environ.update({k: v for k, v in old.items() if v is not None})
    return {"info": {k: int(info[k]) for k in INFO_KEYS}, "digest": digest,
            "kernels": [[k["name"], k["bytes_per_launch"], k["flops_per_launch"]] for k in stats]}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    cases = {case_id(c): record(c) for c in CASES}
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/make_prepare_golden.py", "cases": cases}, f, indent=0)
        f.write("\n")
    for k, v in cases.items():
        print(k, v["info"])
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
