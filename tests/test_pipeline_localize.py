"""The pipeline's localisation hook on the CPU (tests/refloc.lm stands in for Solver.localize):

* ``run_pipeline`` without ``localize`` writes the trajectory it wrote before the hook existed:
  tests/golden/pipeline_default_k12.txt, recorded from the commit before the hook with the CPU oracle as the solver
  (12 keyframes, 400 landmarks, seed 2, frame_frequency = window_size = 4);
* ``window.localize_frame`` flattens keyframe k's admissible observations of the landmarks an earlier keyframe also
  observes, the same with the running set ``run_pipeline`` keeps as without it;
* ``window.localize_keyframe`` writes the refined pose back into the keyframe, and does nothing where no landmark is
  shared; with the hook ``run_pipeline`` localises every keyframe but the first before the schedule looks at it."""
import os

import numpy as np

import refloc
from miba import sequence, window
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_default_k12.txt")
SEQ = dict(n_keyframes=12, n_landmarks=400, seed=2)
SCHED = dict(frame_frequency=4, window_size=4)


def cpu_localize(prob):
    """The contract of Solver.localize on a one-camera problem: the pose refined in place, a dict back."""
    r = refloc.lm(prob, 0, oracle.default_options())
    prob.cams[0] = r["pose"]
    return dict(n_solved=1, iterations=r["iterations"])


def test_default_pipeline_is_what_it_was():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SEQ)
    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, **SCHED)
    assert len(summ) == 3
    assert txt == open(GOLDEN).read()


def test_localize_frame_contents_and_running_set():
    kfs, lms, K0, _ = sequence.make_tum_sequence(**SEQ)
    assert window.localize_frame(0, kfs, lms, K0) is None  # nothing is shared with an earlier keyframe
    seen = set(kfs[0].global_points_map.values())
    for k in range(1, len(kfs)):
        kf = kfs[k]
        a = window.localize_frame(k, kfs, lms, K0)
        b = window.localize_frame(k, kfs, lms, K0, seen)
        for name in ("cams", "points", "intr", "intr_prior", "obs_cam", "obs_pt", "obs_uv", "obs_depth"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
        earlier = set().union(*(o.global_points_map.values() for o in kfs[:k]))
        want = [(lid, loc) for loc, lid in kf.global_points_map.items()
                if kf.points3d_local[loc][2] > 1e-15 and lid in earlier]
        assert a.n_cams == 1 and a.fixed_cam == -1 and a.n_obs == len(want) > 0
        np.testing.assert_array_equal(a.cams[0], kf.T_w_c)
        np.testing.assert_array_equal(a.obs_depth, [kf.points3d_local[loc][2] for _, loc in want])
        np.testing.assert_array_equal(a.obs_uv, np.array([kf.keypoints[loc] for _, loc in want], dtype=np.float64))
        np.testing.assert_array_equal(a.points[a.obs_pt], np.array([lms[lid] for lid, _ in want]))
        np.testing.assert_array_equal(a.intr, K0)
        seen.update(kf.global_points_map.values())


def test_localize_keyframe_writes_the_pose_back():
    kfs, lms, K0, _ = sequence.make_tum_sequence(**SEQ)
    start = [kf.T_w_c.copy() for kf in kfs]
    lms0 = {k: v.copy() for k, v in lms.items()}
    assert window.localize_keyframe(0, kfs, lms, K0, cpu_localize) is None
    np.testing.assert_array_equal(kfs[0].T_w_c, start[0])
    frame = window.localize_frame(3, kfs, lms, K0)
    want = refloc.lm(frame, 0, oracle.default_options())
    out = window.localize_keyframe(3, kfs, lms, K0, cpu_localize)
    assert out["n_solved"] == 1 and want["termination"] == 0 and want["final_cost"] < want["initial_cost"]
    np.testing.assert_array_equal(kfs[3].T_w_c, want["pose"])
    assert not np.array_equal(kfs[3].T_w_c, start[3])
    for k in range(len(kfs)):  # nothing else moved: the other keyframes, the landmarks
        if k != 3:
            np.testing.assert_array_equal(kfs[k].T_w_c, start[k])
    assert all(np.array_equal(lms[k], lms0[k]) for k in lms0)


def test_pipeline_with_the_hook():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SEQ)
    first = window.localize_frame(1, kfs[:2], lms, K0)
    want = refloc.lm(first, 0, oracle.default_options())["pose"]
    calls = []

    def hook(prob):
        before = prob.cams[0].copy()
        out = cpu_localize(prob)
        calls.append((before, prob.cams[0].copy(), prob.n_obs))
        return out

    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, localize=hook, **SCHED)
    assert len(calls) == SEQ["n_keyframes"] - 1 and len(summ) == 3
    np.testing.assert_array_equal(calls[0][1], want)  # keyframe 1, before any window has run
    assert all(n > 0 for _, _, n in calls)
    assert txt != open(GOLDEN).read()  # the hook is in the loop: the windows start from the localised poses
