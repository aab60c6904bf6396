"""The host ordering (csrc/ba_order.cpp) as a stand-alone program against its numpy restatement (reforder.py): the
candidate order, the graph's counts and the band before / after, exactly, on every window of the ordering table and
on the edge windows; once more under AddressSanitizer + UBSan (the stand-alone program only)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reforder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "order_main.cpp"), os.path.join(CSRC, "ba_order.cpp")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

WINDOWS = list(reforder.TABLE) + ["two_scenes"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("order") / "order_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC, *SRC, "-o", exe], check=True)
    return exe


def run(exe, W, fixed_cam, tmp_path, env=None):
    path = str(tmp_path / "weights.bin")
    with open(path, "wb") as f:
        np.array([W.shape[0], fixed_cam], np.int32).tofile(f)
        np.ascontiguousarray(W, np.int32).tofile(f)
    r = subprocess.run([exe, path], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    head, order = r.stdout.splitlines()[:2]
    return [int(v) for v in head.split()], np.array([int(v) for v in order.split()], np.int32), r.stderr


def expected(W, fixed_cam, prob=None):
    cand, ncomp, nact, nedge = reforder.rcm_order(W, fixed_cam)
    given = np.concatenate([np.nonzero(reforder.active(W, fixed_cam))[0], np.nonzero(~reforder.active(W, fixed_cam))[0]])

    def band(order):  # from W alone: the lowest co-visible position of every active position
        sub = W[np.ix_(order[:nact], order[:nact])] > 0
        return int(max((a - int(np.argmax(sub[a])) for a in range(nact)), default=0))

    return [nact, nedge, ncomp, band(given), band(cand)], cand


@pytest.mark.parametrize("name", WINDOWS)
def test_order_equals_the_restatement(name, harness, tmp_path):
    p = reforder.window(name)
    ref = reforder.ordering(p, key=name)
    head, order, _ = run(harness, ref["weights"], p.fixed_cam, tmp_path)
    want_head, want_order = expected(ref["weights"], p.fixed_cam)
    assert head == want_head
    assert np.array_equal(order, want_order) and np.array_equal(order, ref["candidate"])
    # the band from W is the band of the permuted problem (refstep.first_covisible)
    assert head[3] == ref["band_before"] and head[4] == ref["candidate_band"]
    assert head[:3] == [ref["n_active"], ref["n_edges"], ref["n_components"]]


def test_edge_graphs(harness, tmp_path):
    # no camera at all; one camera that is the gauge; cameras without observations; no gauge camera (-1)
    for W, fixed in ((np.zeros((0, 0), np.int32), 0), (np.array([[5]], np.int32), 0), (np.zeros((4, 4), np.int32), 0),
                     (np.array([[3, 0, 2], [0, 0, 0], [2, 0, 4]], np.int32), -1),
                     (np.array([[3, 0, 2], [0, 1, 0], [2, 0, 4]], np.int32), 2)):
        head, order, _ = run(harness, W, fixed, tmp_path)
        want_head, want_order = expected(W, fixed)
        assert head == want_head, (W, fixed)
        assert np.array_equal(order, want_order), (W, fixed)
        assert sorted(order.tolist()) == list(range(W.shape[0]))


def test_harness_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "order_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, *SRC, "-o", exe], check=True)
    for name in ("sweep42_gauge17", "two_scenes", "inactive_mid21"):
        p = reforder.window(name)
        ref = reforder.ordering(p, key=name)
        _, order, err = run(exe, ref["weights"], p.fixed_cam, tmp_path,
                            env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
        assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
        assert np.array_equal(order, ref["candidate"])
