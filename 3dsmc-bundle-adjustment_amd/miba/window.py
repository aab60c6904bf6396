"""Python mirror of the reference's window handling around ceres::Solve.

``window_optimize`` restates windowOptimize (/root/reference/src/OptimizationUtils.cpp:215-313)
over plain Python keyframe / landmark containers and any solver with the
``ba_solve`` contract (e.g. ``miba.solver.Solver().solve`` or the oracle).
``window_schedule`` restates the driver's window schedule (main.cpp:132-133,
163-183). ``include/ba_window.hpp`` is the C++ adapter with the same semantics;
tests/test_window_adapter.py checks the two against each other.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import matching
from .capi import ProblemArrays


# ---- SE(3) on Sophus storage [qx,qy,qz,qw,tx,ty,tz] (same operation order as ba_window.hpp)
def so3_rotate(q, v):
    qx, qy, qz, qw = q[0], q[1], q[2], q[3]
    uv0 = 2 * (qy * v[2] - qz * v[1])
    uv1 = 2 * (qz * v[0] - qx * v[2])
    uv2 = 2 * (qx * v[1] - qy * v[0])
    return np.array([v[0] + qw * uv0 + (qy * uv2 - qz * uv1),
                     v[1] + qw * uv1 + (qz * uv0 - qx * uv2),
                     v[2] + qw * uv2 + (qx * uv1 - qy * uv0)])


def se3_mul(a, b):
    t = so3_rotate(a, b[4:7])
    ax, ay, az, aw = a[0], a[1], a[2], a[3]
    bx, by, bz, bw = b[0], b[1], b[2], b[3]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    sq = x * x + y * y + z * z + w * w
    if sq != 1.0:
        f = 2.0 / (1.0 + sq)
        x, y, z, w = x * f, y * f, z * f, w * f
    return np.array([x, y, z, w, a[4] + t[0], a[5] + t[1], a[6] + t[2]])


def se3_inv(a):
    qi = np.array([-a[0], -a[1], -a[2], a[3]])
    t = so3_rotate(qi, -np.asarray(a[4:7]))
    return np.concatenate([qi, t])


def se3_act(T, p):
    return so3_rotate(T, p) + np.asarray(T[4:7])


@dataclass
class KeyFrame:
    """Mirror of CommonTypes.h:15-32 (the fields windowOptimize reads)."""

    T_w_c: np.ndarray  # (7,)
    keypoints: np.ndarray  # (K, 2) float32 pixel (cv::KeyPoint::pt)
    points3d_local: np.ndarray  # (K, 3)
    global_points_map: dict = field(default_factory=dict)  # localId -> LandmarkId (iteration order kept)
    timestamp: str = ""
    descriptors: np.ndarray | None = None  # (K, B) uint8, one row per keypoint (miba.matching.attach_descriptors)


def window_optimize(kf_i: int, kf_f: int, keyframes: list, landmarks: dict, intr_init, intr_opt: np.ndarray,
                    solve, order=None) -> dict:
    """windowOptimize (:215-313). ``landmarks``: LandmarkId -> (3,) point; ``intr_opt`` updated in place.
    ``order`` (opt-in, default off): passed on as ``solve(prob, order=order)``, for a ``miba.solver.Solver().solve``
    -- ``"auto"`` solves the window in its co-visibility order (ba_solve_ordered)."""
    T0 = np.array(keyframes[kf_i].T_w_c, dtype=np.float64)
    T0inv = se3_inv(T0)
    cams = []
    obs_cam, obs_pt, uv, depth = [], [], [], []
    pt_index, ids, pts = {}, [], []
    for kf_n in range(kf_i, kf_f + 1):
        kf = keyframes[kf_n]
        kf.T_w_c = se3_mul(T0inv, kf.T_w_c)  # :248
        cams.append(kf.T_w_c.copy())
        for local_id, landmark_id in kf.global_points_map.items():  # :257
            d = float(kf.points3d_local[local_id][2])
            px, py = float(kf.keypoints[local_id][0]), float(kf.keypoints[local_id][1])
            if d <= 1e-15:  # :265-268
                continue
            if landmark_id not in pt_index:  # :271-276
                landmarks[landmark_id] = se3_act(T0inv, landmarks[landmark_id])
                pt_index[landmark_id] = len(ids)
                ids.append(landmark_id)
                pts.append(landmarks[landmark_id].copy())
            obs_cam.append(kf_n - kf_i)
            obs_pt.append(pt_index[landmark_id])
            uv.append((px, py))
            depth.append(d)
    summary = None
    try:
        # :300 — solved even when no observation is admissible: the IntrinsicsPrior block (:236-241) is always
        # added, so Ceres still pulls intr_opt toward intr_init (the poses have no residual and stay put)
        prob = ProblemArrays(np.array(cams), np.array(pts, dtype=np.float64).reshape(-1, 3),
                             np.array(intr_opt, dtype=np.float64), np.array(intr_init, dtype=np.float64),
                             np.array(obs_cam, dtype=np.int32), np.array(obs_pt, dtype=np.int32),
                             np.array(uv, dtype=np.float64).reshape(-1, 2), np.array(depth, dtype=np.float64),
                             fixed_cam=0)
        summary = solve(prob) if order is None else solve(prob, order=order)
        intr_opt[:] = prob.intr
        for k, lid in enumerate(ids):
            landmarks[lid] = prob.points[k].copy()
        for kf_n in range(kf_i, kf_f + 1):
            keyframes[kf_n].T_w_c = prob.cams[kf_n - kf_i].copy()
    finally:
        # :303-310 map back — also when the solve raised, so the caller's window is never left re-anchored
        for kf_n in range(kf_i, kf_f + 1):
            keyframes[kf_n].T_w_c = se3_mul(T0, keyframes[kf_n].T_w_c)
        for lid in ids:
            landmarks[lid] = se3_act(T0, landmarks[lid])
    return summary


def local_optimize(kf_c: int, keyframes: list, landmarks: dict, intr_init, intr_opt: np.ndarray, solve_local,
                   min_weight: int = 15, max_local: int = 0) -> dict:
    """The opt-in local schedule: in place of the last-k window, the map so far (keyframes 0 .. kf_c, flattened as
    window_optimize flattens a window, keyframe 0 the map's gauge) handed to ``solve_local`` -- a
    ``miba.solver.Solver().solve_local`` -- centred on keyframe ``kf_c``: the keyframes co-visible with it are
    optimised with the landmarks they see, every other keyframe that sees those landmarks is held constant
    (ba_solve_local). The rest of the map is not touched."""
    return window_optimize(0, kf_c, keyframes, landmarks, intr_init, intr_opt,
                           lambda prob: solve_local(prob, kf_c, min_weight=min_weight, max_local=max_local))


def localize_frame(k: int, keyframes: list, landmarks: dict, intr, seen=None):
    """Keyframe ``k`` against the map as one-camera ``ProblemArrays`` (``None`` when nothing qualifies): its admissible
    observations of the landmarks an earlier keyframe (index < k) also observes, in the order of its
    global_points_map. A landmark first seen by ``k`` was created from k's own pose and says nothing about it.
    ``seen``: the landmark ids keyframes 0 .. k-1 observe, for a caller that keeps that set as the sequence grows
    (run_pipeline); ``None``: collected here."""
    kf = keyframes[k]
    if seen is None:
        seen = set()
        for other in keyframes[:k]:
            seen.update(other.global_points_map.values())
    obs_pt, uv, depth, pts, pt_index = [], [], [], [], {}
    for local_id, landmark_id in kf.global_points_map.items():
        d = float(kf.points3d_local[local_id][2])
        if d <= 1e-15 or landmark_id not in seen:
            continue
        if landmark_id not in pt_index:
            pt_index[landmark_id] = len(pts)
            pts.append(np.array(landmarks[landmark_id], dtype=np.float64))
        obs_pt.append(pt_index[landmark_id])
        uv.append((float(kf.keypoints[local_id][0]), float(kf.keypoints[local_id][1])))
        depth.append(d)
    if not obs_pt:
        return None
    K = np.array(intr, dtype=np.float64)
    return ProblemArrays(np.array(kf.T_w_c, dtype=np.float64).reshape(1, 7), np.array(pts).reshape(-1, 3), K, K.copy(),
                         np.zeros(len(obs_pt), dtype=np.int32), np.array(obs_pt, dtype=np.int32),
                         np.array(uv, dtype=np.float64).reshape(-1, 2), np.array(depth, dtype=np.float64), fixed_cam=-1)


def localize_keyframe(k: int, keyframes: list, landmarks: dict, intr, localize, seen=None):
    """Pose-only refinement of keyframe ``k`` against the map as it stands ("track local map"): ``localize_frame``
    handed to ``localize`` -- a ``miba.solver.Solver().localize`` -- and the pose written back. Landmarks and
    intrinsics are constant. With no landmark shared with an earlier keyframe it does nothing and returns ``None``."""
    prob = localize_frame(k, keyframes, landmarks, intr, seen)
    if prob is None:
        return None
    out = localize(prob)
    keyframes[k].T_w_c = prob.cams[0].copy()
    return out


def track_matches(k: int, keyframes: list):
    """The 3D-3D matches of keyframes ``k - 1`` and ``k`` (main.cpp:49-60): the local ids of the two that map to one
    landmark id with a depth in both, in the order of k's global_points_map; (p1, p2, ids) with p1 / p2 their ``points3d_local`` in frame
    k - 1 / k."""
    prev, kf = keyframes[k - 1], keyframes[k]
    by_landmark = {}
    for local_id, landmark_id in prev.global_points_map.items():
        if float(prev.points3d_local[local_id][2]) > 1e-15:
            by_landmark.setdefault(landmark_id, local_id)
    p1, p2, ids = [], [], []
    for local_id, landmark_id in kf.global_points_map.items():
        if landmark_id in by_landmark and float(kf.points3d_local[local_id][2]) > 1e-15:
            p1.append(prev.points3d_local[by_landmark[landmark_id]])
            p2.append(kf.points3d_local[local_id])
            ids.append(landmark_id)
    return (np.array(p1, dtype=np.float64).reshape(-1, 3), np.array(p2, dtype=np.float64).reshape(-1, 3), ids)


def track_keyframe(k: int, keyframes: list, landmarks: dict, align, seen=None, min_inliers: int = 20, match=None, **kw):
    """The reference tracker's pose of keyframe ``k`` (main.cpp:49-78, initializeRelativePose): ``align`` -- a
    ``miba.solver.Solver().align`` -- on ``track_matches`` gives T_12 with p1 ~ T_12 p2, and with ``min_inliers`` inliers
    or more ``T_w_c[k] = T_w_c[k-1] T_12``; with fewer (tracking failed) the pose is kept. The landmarks ``k`` is the
    first to observe were placed from k's earlier pose, so they are re-placed from the new one
    (``se3_act(T_new, points3d_local)``) and the map stays consistent with it. ``seen``: the landmark ids keyframes
    0 .. k-1 observe (``None``: collected here). ``match`` (opt-in, default off; a ``miba.solver.Solver().match``): when
    both keyframes carry descriptors the matches come from them as the reference's do (matchKeypoints +
    filterMatchesLowe, the previous keyframe's descriptors as the queries; ``matching.correspondences``) in place of
    ``track_matches``' landmark ids. Returns ``align``'s output with ``tracked`` (bool), or ``None`` for keyframe 0."""
    if k <= 0:
        return None
    prev, cur = keyframes[k - 1], keyframes[k]
    if match is not None and prev.descriptors is not None and cur.descriptors is not None:
        p1, p2 = matching.correspondences(match(prev.descriptors, cur.descriptors), 0, prev.points3d_local,
                                          cur.points3d_local)
    else:
        p1, p2, _ = track_matches(k, keyframes)
    out = dict(align(p1, p2, **kw))
    stats = np.asarray(out["stats"])[0]
    out["tracked"] = bool(stats[0] == 0 and stats[2] >= min_inliers)
    if not out["tracked"]:
        return out
    kf = keyframes[k]
    kf.T_w_c = se3_mul(np.array(keyframes[k - 1].T_w_c, dtype=np.float64), np.asarray(out["poses"], dtype=np.float64)[0])
    if seen is None:
        seen = set()
        for other in keyframes[:k]:
            seen.update(other.global_points_map.values())
    placed = set()
    for local_id, landmark_id in kf.global_points_map.items():
        if landmark_id not in seen and landmark_id not in placed and float(kf.points3d_local[local_id][2]) > 1e-15:
            landmarks[landmark_id] = se3_act(kf.T_w_c, kf.points3d_local[local_id])
            placed.add(landmark_id)
    return out


def search_local_map(k: int, keyframes: list, landmarks: dict, intr, width: int, height: int, guided_match,
                     n_recent: int = 5, **kw):
    """ORB-SLAM's SearchByProjection against the local map: the landmarks keyframes ``k - n_recent .. k - 1`` observe
    and keyframe ``k`` does not are projected into k with its pose as it stands and searched for among the keypoints
    of k that map to no landmark (that subset is the call's keypoint range; the indices are mapped back afterwards):
    ``guided_match(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, kp_depth=..., **kw)`` -- a
    ``miba.solver.Solver().guided_match``. A landmark's descriptor is that of its first observation
    (``matching.landmark_descriptors``). The accepted matches are added to ``global_points_map``. Returns the call's
    output with ``added``, the (local id, landmark id) pairs, or ``None`` when there is nothing to search (no
    descriptors, no such landmark, no free keypoint)."""
    kf = keyframes[k]
    first = max(0, k - n_recent)
    if k <= 0 or kf.descriptors is None:
        return None
    mine = set(kf.global_points_map.values())
    ids, desc = matching.landmark_descriptors(keyframes[:k])
    recent = set()
    for other in keyframes[first:k]:
        recent.update(other.global_points_map.values())
    sel = np.array([i for i, l in enumerate(ids.tolist()) if l in recent and l not in mine], dtype=np.int64)
    free = np.array([i for i in range(len(kf.keypoints)) if i not in kf.global_points_map], dtype=np.int64)
    if not len(sel) or not len(free):
        return None
    points = np.array([landmarks[int(l)] for l in ids[sel]], dtype=np.float64).reshape(-1, 3)
    loc = np.asarray(kf.points3d_local, dtype=np.float64).reshape(-1, 3)
    out = dict(guided_match(points, desc[sel], np.asarray(kf.keypoints, dtype=np.float64).reshape(-1, 2)[free],
                            np.asarray(kf.descriptors, dtype=np.uint8)[free], np.asarray(kf.T_w_c, dtype=np.float64).reshape(1, 7),
                            intr, width, height, kp_depth=loc[free, 2], **kw))
    out["added"] = [(int(free[kp]), int(ids[sel[pt]])) for pt, kp in np.asarray(out["matches"]).tolist()]
    for local_id, landmark_id in out["added"]:
        kf.global_points_map[local_id] = landmark_id
    return out


def refine_frame(k: int, keyframes: list, landmarks: dict, intr):
    """The landmarks keyframe ``k`` brings new evidence about, as ``ProblemArrays`` for a structure-only refinement
    (``None`` when nothing qualifies): the landmarks ``k`` observes that an earlier keyframe (index < k) also observes,
    in the order of k's global_points_map, with all their admissible observations in keyframes 0 .. k (keyframe by
    keyframe, each in the order of its global_points_map). The cameras are those k + 1 keyframes, constant to the
    refinement. ``meta['landmark_ids']`` names the landmark of every point."""
    kf = keyframes[k]
    earlier = set()
    for other in keyframes[:k]:
        earlier.update(other.global_points_map.values())
    pt_index, ids = {}, []
    for landmark_id in kf.global_points_map.values():
        if landmark_id in earlier and landmark_id not in pt_index:
            pt_index[landmark_id] = len(ids)
            ids.append(landmark_id)
    if not ids:
        return None
    obs_cam, obs_pt, uv, depth = [], [], [], []
    for n in range(k + 1):
        other = keyframes[n]
        for local_id, landmark_id in other.global_points_map.items():
            d = float(other.points3d_local[local_id][2])
            if d <= 1e-15 or landmark_id not in pt_index:
                continue
            obs_cam.append(n)
            obs_pt.append(pt_index[landmark_id])
            uv.append((float(other.keypoints[local_id][0]), float(other.keypoints[local_id][1])))
            depth.append(d)
    K = np.array(intr, dtype=np.float64)
    cams = np.array([np.array(o.T_w_c, dtype=np.float64) for o in keyframes[:k + 1]]).reshape(-1, 7)
    pts = np.array([np.array(landmarks[lid], dtype=np.float64) for lid in ids]).reshape(-1, 3)
    return ProblemArrays(cams, pts, K, K.copy(), np.array(obs_cam, dtype=np.int32), np.array(obs_pt, dtype=np.int32),
                         np.array(uv, dtype=np.float64).reshape(-1, 2), np.array(depth, dtype=np.float64), fixed_cam=-1,
                         meta=dict(landmark_ids=ids))


def refine_landmarks(k: int, keyframes: list, landmarks: dict, intr, refine_points):
    """Structure-only refinement of the landmarks keyframe ``k`` re-observes, against the keyframes as they stand:
    ``refine_frame`` handed to ``refine_points`` -- a ``miba.solver.Solver().refine_points`` -- and the solved landmarks
    (stats[:, 6] >= 0) written back, and only those. Keyframes and intrinsics are constant. With no landmark shared
    with an earlier keyframe it does nothing and returns ``None``."""
    prob = refine_frame(k, keyframes, landmarks, intr)
    if prob is None:
        return None
    out = refine_points(prob)
    for q, lid in enumerate(prob.meta["landmark_ids"]):
        if out["stats"][q][6] >= 0:
            landmarks[lid] = prob.points[q].copy()
    return out


def window_schedule(frame_frequency: int, window_size: int, n_keyframes: int, tracking_finished: bool,
                    optimization_finished: bool, tracked_this_frame: bool):
    """(run, kf_i, kf_f, finishes) for main.cpp:163-183."""
    if optimization_finished:
        return (False, 0, 0, False)
    n = n_keyframes
    if window_size > 0:
        if tracked_this_frame and n % frame_frequency == 0 and n >= window_size:
            return (True, n - window_size, n - 1, False)
        if tracking_finished and n % frame_frequency != 0:
            return (True, max(n - window_size, 0), n - 1, True)
    elif window_size < 0 and tracking_finished:
        return (True, 0, n - 1, True)
    return (False, 0, 0, False)
