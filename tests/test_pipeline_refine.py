"""The pipeline's point-refinement hook on the CPU (tests/refpts.lm stands in for Solver.refine_points):

* ``run_pipeline`` without ``refine_points`` writes the trajectory it wrote before the hook existed:
  tests/golden/pipeline_default_k12.txt (12 keyframes, 400 landmarks, seed 2, frame_frequency = window_size = 4);
* ``window.refine_frame`` flattens the landmarks keyframe k shares with an earlier keyframe, with all their admissible
  observations in keyframes 0 .. k;
* ``window.refine_landmarks`` writes the solved landmarks back, and only those; with the hook ``run_pipeline`` refines
  after every keyframe but the first, right after the localisation hook."""
import os

import numpy as np

import refloc
import refpts
from miba import sequence, window
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_default_k12.txt")
SEQ = dict(n_keyframes=12, n_landmarks=400, seed=2)
SCHED = dict(frame_frequency=4, window_size=4)
# the hook's own runs: refpts.lm is plain Python, so a short sequence with a thin map
SMALL = dict(n_keyframes=5, n_landmarks=40, seed=2)
SMALL_SCHED = dict(frame_frequency=2, window_size=2)


def cpu_refine(prob, min_obs=2):
    """The contract of Solver.refine_points: the solved points refined in place, a dict with ``stats`` back."""
    adm = prob.obs_depth > 1e-15
    n = np.bincount(prob.obs_pt[adm], minlength=prob.n_points)
    stats = np.zeros((prob.n_points, 8))
    stats[:, 6] = -1
    for q in range(prob.n_points):
        if n[q] < min_obs:
            continue
        r = refpts.lm(prob, q, oracle.default_options())
        prob.points[q] = r["X"]
        stats[q] = [n[q], r["initial_cost"], r["final_cost"], r["iterations"], r["n_succ"], r["n_unsucc"],
                    r["termination"], r["msg"]]
    return dict(n_solved=int((stats[:, 6] >= 0).sum()), stats=stats)


def test_default_pipeline_is_what_it_was():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SEQ)
    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, **SCHED)
    assert len(summ) == 3
    assert txt == open(GOLDEN).read()


def test_refine_frame_contents():
    kfs, lms, K0, _ = sequence.make_tum_sequence(**SEQ)
    assert window.refine_frame(0, kfs, lms, K0) is None  # nothing is shared with an earlier keyframe
    for k in (1, 5, len(kfs) - 1):
        a = window.refine_frame(k, kfs, lms, K0)
        earlier = set().union(*(o.global_points_map.values() for o in kfs[:k]))
        ids = [lid for lid in dict.fromkeys(kfs[k].global_points_map.values()) if lid in earlier]
        assert a.meta["landmark_ids"] == ids and a.n_points == len(ids) > 0
        want = [(n, ids.index(lid), loc) for n in range(k + 1) for loc, lid in kfs[n].global_points_map.items()
                if kfs[n].points3d_local[loc][2] > 1e-15 and lid in set(ids)]
        assert a.n_cams == k + 1 and a.fixed_cam == -1 and a.n_obs == len(want)
        np.testing.assert_array_equal(a.cams, np.array([kf.T_w_c for kf in kfs[:k + 1]]))
        np.testing.assert_array_equal(a.points, np.array([lms[lid] for lid in ids]))
        np.testing.assert_array_equal(a.obs_cam, [n for n, _, _ in want])
        np.testing.assert_array_equal(a.obs_pt, [q for _, q, _ in want])
        np.testing.assert_array_equal(a.obs_depth, [kfs[n].points3d_local[loc][2] for n, _, loc in want])
        np.testing.assert_array_equal(a.obs_uv, np.array([kfs[n].keypoints[loc] for n, _, loc in want], dtype=np.float64))
        np.testing.assert_array_equal(a.intr, K0)
        # every point is seen by k and by an earlier keyframe (admissibly or not); most have two admissible observations
        n_adm = np.bincount(a.obs_pt, minlength=a.n_points)
        assert (n_adm >= 2).sum() >= 0.8 * a.n_points


def test_refine_landmarks_writes_the_solved_landmarks_back_and_only_those():
    kfs, lms, K0, _ = sequence.make_tum_sequence(**SMALL)
    poses = [kf.T_w_c.copy() for kf in kfs]
    lms0 = {k: v.copy() for k, v in lms.items()}
    assert window.refine_landmarks(0, kfs, lms, K0, cpu_refine) is None
    assert all(np.array_equal(lms[k], lms0[k]) for k in lms0)
    frame = window.refine_frame(2, kfs, lms, K0)
    ids = frame.meta["landmark_ids"]
    want = cpu_refine(frame.copy())

    def some(prob):  # a solver that leaves every third point unsolved and still scribbles on it
        out = cpu_refine(prob)
        out["stats"][::3, 6] = -1
        prob.points[::3] += 1.0
        return out

    out = window.refine_landmarks(2, kfs, lms, K0, some)
    solved = out["stats"][:, 6] >= 0
    assert 0 < solved.sum() < len(ids) and want["n_solved"] > 0
    moved = 0
    for q, lid in enumerate(ids):
        if solved[q]:
            ref = refpts.lm(frame, q, oracle.default_options())
            np.testing.assert_array_equal(lms[lid], ref["X"])
            moved += int(not np.array_equal(lms[lid], lms0[lid]))
        else:
            np.testing.assert_array_equal(lms[lid], lms0[lid])
    assert moved > 0
    for lid in set(lms0) - set(ids):  # nothing else moved: the other landmarks, the keyframes
        np.testing.assert_array_equal(lms[lid], lms0[lid])
    for k, kf in enumerate(kfs):
        np.testing.assert_array_equal(kf.T_w_c, poses[k])


def test_pipeline_with_the_hook():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SMALL)
    base = sequence.run_pipeline(*sequence.make_tum_sequence(**SMALL)[:2], K0, gt, oracle.solve, **SMALL_SCHED)[0]
    first = window.refine_frame(1, kfs[:2], lms, K0)
    want = cpu_refine(first.copy())
    order, calls = [], []

    def loc_hook(prob):
        order.append("localize")
        r = refloc.lm(prob, 0, oracle.default_options())
        prob.cams[0] = r["pose"]
        return dict(n_solved=1)

    def hook(prob):
        order.append("refine")
        before = prob.points.copy()
        out = cpu_refine(prob)
        calls.append((before, prob.points.copy(), prob.n_cams, out["n_solved"]))
        return out

    # the refinement alone: its first call is keyframe 1's frame, before any window has run
    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, refine_points=hook, **SMALL_SCHED)
    assert len(calls) == SMALL["n_keyframes"] - 1 and [c[2] for c in calls] == list(range(2, SMALL["n_keyframes"] + 1))
    np.testing.assert_array_equal(calls[0][0], first.points)
    assert all(n > 0 for _, _, _, n in calls) and want["n_solved"] == calls[0][3]
    np.testing.assert_array_equal(calls[0][1], _points_after(first))
    assert txt != base  # the hook is in the loop: the windows start from the refined landmarks
    # both hooks: the refinement runs right after the localisation of the same keyframe
    order.clear()
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SMALL)
    sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, localize=loc_hook, refine_points=hook, **SMALL_SCHED)
    assert order == ["localize", "refine"] * (SMALL["n_keyframes"] - 1)


def _points_after(frame):
    q = frame.copy()
    cpu_refine(q)
    return q.points
