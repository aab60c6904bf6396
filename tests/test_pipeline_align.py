"""The two consumers of ba_align on the CPU (tests/refalign.align stands in for Solver.align):

* ``posegraph.measured_edges`` on a two-sweep map returns the loop edges within the measurement noise of the truth,
  where ``posegraph.edges_from_poses`` on the drifted estimates returns the drift itself;
* ``window.track_matches`` / ``window.track_keyframe`` compose the tracked pose (main.cpp:49-78) and re-place the
  landmarks the keyframe is the first to observe; a keyframe with too few inliers keeps its pose;
* ``run_pipeline`` without ``align`` writes tests/golden/pipeline_default_k12.txt, and with it tracks every keyframe
  but the first before the schedule looks at it."""
import os

import numpy as np

import refalign
import refpg
from miba import posegraph, sequence, window
from miba.capi import ProblemArrays
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_default_k12.txt")
SEQ = dict(n_keyframes=12, n_landmarks=400, seed=2)
SCHED = dict(frame_frequency=4, window_size=4)
K = np.array([525.0, 525.0, 319.5, 239.5])


def cpu_align(p1, p2, pair_begin=None, **kw):
    out = refalign.align(p1, p2, pair_begin, **kw)
    return dict(poses=out["poses"], stats=out["stats"], inlier=out["inlier"])


def two_sweep_map(n=24, per_keyframe=40, seed=0, depth_noise=0.004, pixel_noise=0.3):
    """refpg.loop_closure_graph's circuit (the cameras look along world z) with landmarks above it, observed by every
    keyframe whose image they fall into; the cameras of the window are the drifted estimates."""
    g = refpg.loop_closure_graph(n=n, seed=5, n_loops=4)
    rng = np.random.default_rng(seed)
    truth = g["truth"]
    local = np.stack([rng.uniform(-1.0, 1.0, n * per_keyframe), rng.uniform(-0.8, 0.8, n * per_keyframe),
                      rng.uniform(2.5, 5.0, n * per_keyframe)], 1)
    owner = np.repeat(np.arange(n), per_keyframe)
    X = truth[owner, 4:] + posegraph.quat_rotate(truth[owner, :4], local)
    oc, op, uv, dep = [], [], [], []
    for c in range(n):
        pc = posegraph.quat_rotate(posegraph.quat_conj(truth[c, :4]), X - truth[c, 4:])
        z = pc[:, 2]
        u, v = K[0] * pc[:, 0] / z + K[2], K[1] * pc[:, 1] / z + K[3]
        vis = np.nonzero((z > 0.5) & (u >= 0) & (u < 640) & (v >= 0) & (v < 480))[0]
        oc.append(np.full(len(vis), c)); op.append(vis)
        uv.append(np.stack([u[vis], v[vis]], 1) + rng.normal(0, pixel_noise, (len(vis), 2)))
        dep.append(z[vis] * (1 + rng.normal(0, depth_noise, len(vis))))
    prob = ProblemArrays(g["cams"].copy(), X, K, K.copy(), np.concatenate(oc).astype(np.int32),
                         np.concatenate(op).astype(np.int32), np.concatenate(uv), np.concatenate(dep), fixed_cam=0)
    return g, prob


def _pose_gap(Z, Zt):
    """(translation distance, rotation angle) between poses (m, 7)."""
    dq = posegraph.quat_mul(posegraph.quat_conj(Z[:, :4]), Zt[:, :4])
    ang = 2 * np.arcsin(np.clip(np.linalg.norm(dq[:, :3], axis=1), 0, 1))
    return np.linalg.norm(Z[:, 4:] - Zt[:, 4:], axis=1), ang


def test_measured_edges_measure_the_loop_where_the_poses_give_the_drift():
    g, prob = two_sweep_map()
    n = len(g["truth"])
    loops = np.stack([g["ea"][n - 1:], g["eb"][n - 1:]], 1)
    assert len(loops) == 4 and (loops[:, 1] - loops[:, 0] == n // 2).all()
    # a pair that shares nothing (opposite sides of the circuit) is dropped; the others come back in order
    pairs = np.concatenate([loops, [[0, n // 4]]])
    ea, eb, meas, n_in = posegraph.measured_edges(prob, pairs, cpu_align, min_inliers=20, seed=3, refit=2)
    np.testing.assert_array_equal(np.stack([ea, eb], 1), loops)
    assert ea.dtype == eb.dtype == np.int32 and meas.shape == (4, 7) and (n_in >= 20).all()
    _, _, z_true = posegraph.edges_from_poses(g["truth"], loops)
    _, _, z_drift = posegraph.edges_from_poses(prob.cams, loops)
    dt, da = _pose_gap(meas, z_true)
    dt_d, da_d = _pose_gap(z_drift, z_true)
    print(f"measured: {dt.max():.4f} m {da.max():.5f} rad; read off the poses: {dt_d.max():.4f} m {da_d.max():.5f} rad; "
          f"inliers {n_in.tolist()}")
    # the noise of the truth: a point carries up to sigma = 2 cm (0.4 % of a depth of 5 m; 0.3 px there is 3 mm). A fit
    # over m inliers spread by s = 0.58 m (uniform on +-1 m) has a rotation sigma of sigma / (s sqrt(m)), which a
    # cloud L = 5 m from the camera turns into L times that of translation, beside sigma / sqrt(m) of the centroid;
    # four sigma of each, while the second sweep has drifted by decimetres
    sigma, spread, lever, m = 0.02, 0.58, 5.0, float(n_in.min())
    rot_sigma = sigma / (spread * np.sqrt(m))
    assert dt.max() < 4 * np.hypot(sigma / np.sqrt(m), lever * rot_sigma) and da.max() < 4 * np.sqrt(3) * rot_sigma
    assert dt_d[1:].min() > 5 * dt.max()
    # without a refit: the best minimal sample's model, still inside the inlier threshold's scale
    _, _, meas0, n0 = posegraph.measured_edges(prob, loops, cpu_align, seed=3)
    assert _pose_gap(meas0, z_true)[0].max() < 0.1 and (n0 >= 20).all()
    # the back-projection: the first loop pair's clouds are the landmarks both keyframes observe
    a, b = loops[0]
    shared = np.intersect1d(prob.obs_pt[prob.obs_cam == a], prob.obs_pt[prob.obs_cam == b])
    assert n_in[0] <= len(shared)
    empty = posegraph.measured_edges(prob, np.zeros((0, 2), dtype=int), cpu_align)
    assert [len(x) for x in empty] == [0, 0, 0, 0]


def test_track_keyframe_composes_the_pose_and_replaces_the_new_landmarks():
    kfs, lms, K0, _ = sequence.make_tum_sequence(**SEQ)
    k = 3
    p1, p2, ids = window.track_matches(k, kfs)
    prev_ids = set(kfs[k - 1].global_points_map.values())
    assert len(ids) > 20 and set(ids) == prev_ids & set(kfs[k].global_points_map.values())
    start = [kf.T_w_c.copy() for kf in kfs]
    lms0 = {i: v.copy() for i, v in lms.items()}
    assert window.track_keyframe(0, kfs, lms, cpu_align) is None
    out = window.track_keyframe(k, kfs, lms, cpu_align, seed=1)
    want = refalign.align(p1, p2, seed=1)
    assert out["tracked"] and want["stats"][0, 2] >= 20
    np.testing.assert_array_equal(kfs[k].T_w_c, window.se3_mul(start[k - 1], want["poses"][0]))
    # T_12 is the relative pose of the two frames: close to what the generator's estimates say, not equal to it
    rel = window.se3_mul(window.se3_inv(start[k - 1]), start[k])
    assert np.abs(want["poses"][0] - rel).max() < 0.05 and not np.array_equal(kfs[k].T_w_c, start[k])
    earlier = set().union(*(o.global_points_map.values() for o in kfs[:k]))
    new = [(loc, lid) for loc, lid in kfs[k].global_points_map.items() if lid not in earlier]
    assert new
    for loc, lid in new:
        np.testing.assert_array_equal(lms[lid], window.se3_act(kfs[k].T_w_c, kfs[k].points3d_local[loc]))
    moved = {lid for lid in lms if not np.array_equal(lms[lid], lms0[lid])}
    assert moved == {lid for _, lid in new}
    for i in range(len(kfs)):
        if i != k:
            np.testing.assert_array_equal(kfs[i].T_w_c, start[i])
    # tracking failed (too few inliers): the pose and the map stay
    before = kfs[5].T_w_c.copy()
    lms1 = {i: v.copy() for i, v in lms.items()}
    out = window.track_keyframe(5, kfs, lms, cpu_align, min_inliers=10**6)
    assert not out["tracked"]
    np.testing.assert_array_equal(kfs[5].T_w_c, before)
    assert all(np.array_equal(lms[i], lms1[i]) for i in lms1)


def test_default_pipeline_is_what_it_was():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SEQ)
    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, align=None, **SCHED)
    assert len(summ) == 3
    assert txt == open(GOLDEN).read()


def test_pipeline_with_the_hook():
    kfs, lms, K0, gt = sequence.make_tum_sequence(**SEQ)
    calls = []

    def hook(p1, p2, **kw):
        out = cpu_align(p1, p2, **kw)
        calls.append((len(p1), int(out["stats"][0, 2])))
        return out

    txt, summ, _ = sequence.run_pipeline(kfs, lms, K0, gt, oracle.solve, align=hook, **SCHED)
    assert len(calls) == SEQ["n_keyframes"] - 1 and len(summ) == 3
    assert all(n > 20 and m >= 20 for n, m in calls)
    assert txt != open(GOLDEN).read()  # the hook is in the loop: the windows start from the tracked poses
