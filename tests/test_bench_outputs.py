"""bench.py's timed-step loop and --dump-outputs, without a GPU: solve_steps() runs exactly the asked number of LM
iterations even when a solve ends early, and dump_outputs() writes float64 arrays within its size limit, a larger
array as the same seeded sample of rows on every call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from miba import synthetic  # noqa: E402

SUMM = dict(initial_cost=2.0, final_cost=0.5, num_iterations=3, num_successful_steps=4, num_unsuccessful_steps=0,
            termination_type=1)


class _Options:
    max_num_iterations = 0


class _FakeSolver:
    """ba_solve_prepared stand-in whose LM loop ends by itself after `ends_at` iterations; it writes the number of
    iterations it ran into the problem it is given (a list)."""

    def __init__(self, ends_at):
        self.options, self.ends_at, self.asked = _Options(), ends_at, []

    def set_options(self, **changes):
        self.options.max_num_iterations = changes["max_num_iterations"]

    def solve_prepared(self, prob):
        self.asked.append(self.options.max_num_iterations)
        prob[:] = [min(self.ends_at, self.options.max_num_iterations)]
        return dict(num_iterations=prob[0], message="stub")


@pytest.mark.parametrize("steps,ends_at,asked,kept", [
    (20, 100, [20], 20),                 # up to LAST_SOLVE_STEPS: one call
    (1, 100, [1], 1),
    (50, 100, [30, 20], 20),             # longer: what comes before, then a last solve of LAST_SOLVE_STEPS
    (100, 31, [80, 49, 18, 20], 20),     # the LM loop ends by itself after 31: the window again for what remains
    (21, 31, [1, 20], 20),
    (30, 7, [10, 3, 20, 13, 6], 7),      # even the last solve ends early: the count is made up after it
])
def test_solve_steps_runs_exactly_the_steps(steps, ends_at, asked, kept):
    assert bench.LAST_SOLVE_STEPS == 20
    s = _FakeSolver(ends_at)
    bufs = ([], [])
    summ, calls = bench.solve_steps(s, bufs, steps)
    assert s.asked == asked and calls == len(asked)
    assert sum(min(ends_at, a) for a in s.asked) == steps
    assert summ["num_iterations"] == kept and bufs[0] == [kept]  # the last solve's outputs are in bufs[0]


def test_solve_steps_refuses_a_loop_that_does_not_iterate():
    with pytest.raises(SystemExit):
        bench.solve_steps(_FakeSolver(0), ([], []), 5)


def test_dump_outputs_writes_the_window_and_summary(tmp_path):
    p = synthetic.make_problem(n_cams=6, n_points=200, obs_per_point=(2, 3), seed=1)
    bench.dump_outputs(str(tmp_path / "out"), p, SUMM)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["cams", "intr", "points", "summary"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["cams"], p.cams) and np.array_equal(got["points"], p.points)
    assert np.array_equal(got["intr"], p.intr)
    assert got["summary"].tolist() == [2.0, 0.5, 3.0, 4.0, 0.0, 1.0]


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    p = synthetic.make_problem(n_cams=6, n_points=200, obs_per_point=(2, 3), seed=1)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 50 * 24)  # a share of 50 point rows per array
    bench.dump_outputs(str(tmp_path / "a"), p, SUMM)
    bench.dump_outputs(str(tmp_path / "b"), p, SUMM)
    a, b = np.load(tmp_path / "a" / "points.npy"), np.load(tmp_path / "b" / "points.npy")
    assert a.shape == (50, 3) and np.array_equal(a, b)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4 * 50 * 24 + 4 * 128
    rows = {tuple(r) for r in p.points}
    assert all(tuple(r) in rows for r in a) and np.array_equal(np.load(tmp_path / "a" / "cams.npy"), p.cams)
