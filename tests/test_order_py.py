"""miba.order (permute_cams / restore_cams) against reforder.permute, and the adapters' opt-in ``order`` switch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reforder
from miba import sequence, window
from miba.order import inverse_order, permute_cams, restore_cams


def test_permute_cams_equals_the_restatement():
    for name in ("sweep22", "sweep42_gauge17"):
        p = reforder.window(name)
        order = reforder.ordering(p, key=name)["order"]
        a, b = permute_cams(p, order), reforder.permute(p, order)
        for k in ("cams", "points", "intr", "intr_prior", "obs_cam", "obs_pt", "obs_uv", "obs_depth"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
        assert a.fixed_cam == b.fixed_cam == int(inverse_order(order)[p.fixed_cam])
        assert a.obs_cam.dtype == np.int32 and np.shares_memory(a.points, p.points)
        assert np.shares_memory(a.intr, p.intr) and not np.shares_memory(a.cams, p.cams)
        # camera order[k] sits at position k, and comes back
        np.testing.assert_array_equal(a.cams, p.cams[order])
        q = p.copy()
        a.cams += 1.0
        restore_cams(q, a, order)
        np.testing.assert_array_equal(q.cams, p.cams + 1.0)


def test_no_gauge_camera_stays_none():
    p = reforder.window("sweep22").copy()
    p.fixed_cam = -1
    assert permute_cams(p, np.arange(p.n_cams)[::-1]).fixed_cam == -1


def test_not_a_permutation():
    p = reforder.window("sweep22")
    for bad in (np.zeros(p.n_cams, int), np.arange(p.n_cams) + 1, np.arange(p.n_cams - 1)):
        with pytest.raises(ValueError):
            permute_cams(p, bad)


def test_adapters_pass_the_order_on_only_when_asked():
    calls = []

    def solve(prob, **kw):
        calls.append(kw)
        return dict(final_cost=0.0)

    kfs, lms, K0, gt = sequence.make_tum_sequence(n_keyframes=12, n_landmarks=60, seed=1)
    window.window_optimize(0, 5, kfs, lms, K0, K0.copy(), solve)
    window.window_optimize(0, 5, kfs, lms, K0, K0.copy(), solve, order="auto")
    assert calls == [{}, {"order": "auto"}]
    del calls[:]
    sequence.run_pipeline(list(kfs), lms, K0, gt, solve, frame_frequency=5, window_size=5, order="auto")
    assert calls and all(c == {"order": "auto"} for c in calls)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_window_solver_compiles(tmp_path):
    """include/ba_window.hpp's window_solver(ctx, ordered): both branches type-check against ba.h (no library is
    linked: the header stays usable with any solver)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "ws.cpp"
    src.write_text('#include "ba_window.hpp"\n'
                   "int32_t run(ba_context* ctx, ba_problem* p, ba_summary* s, bool ordered) {\n"
                   "    return miba::window_solver(ctx, ordered)(p, s);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(root, "include"), str(src)], check=True)
