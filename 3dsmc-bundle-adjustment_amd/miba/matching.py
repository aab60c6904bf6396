"""Descriptor matching around ``Solver.match`` (ba_match): the step between "two keyframes with features" and the 3D-3D
correspondences ``Solver.align`` starts from (the reference's matchKeypoints + filterMatchesLowe, main.cpp:50-62).

* ``attach_descriptors(keyframes, seed, kind, flip)``: descriptors for a synthetic sequence, which has none: every
  landmark id gets one random descriptor and every observation of it a disturbed copy.
* ``correspondences(out, j, pts_q, pts_t)``: the matched ``points3d_local`` of pair j of a ``Solver.match`` output,
  with the reference's depth filter.
* ``matched_edges(keyframes, pairs, match, align)``: relative-pose edges between keyframes from their descriptors
  alone, the counterpart of ``posegraph.measured_edges`` for keyframes that share no landmark id (a revisit the map
  does not know about: the loops that need closing).
* ``landmark_descriptors(keyframes)``: one descriptor per landmark id, for ``Solver.guided_match`` (ba_guided_match).
* ``fuse_landmarks(keyframes, landmarks, pairs, ...)``: after such a loop is closed, the landmarks keyframe a observes
  are searched for in keyframe b by projection; what is found adds an observation or merges two ids of one point."""
from __future__ import annotations

import numpy as np

# the descriptor sizes of the reference's detectors: ORB's 256 bits, byte SIFT's 128 values
DEFAULT_BYTES = {"hamming": 32, "l2_u8": 128}


def disturb(rng, desc, kind: str, flip: float):
    """A disturbed copy of uint8 descriptors (..., B): ``"hamming"`` flips every bit with probability ``flip``;
    ``"l2_u8"`` adds rounded Gaussian noise of sigma ``flip`` to every byte and clips to 0..255."""
    desc = np.asarray(desc, dtype=np.uint8)
    if kind == "hamming":
        return desc ^ np.packbits(rng.random(desc.shape[:-1] + (8 * desc.shape[-1],)) < flip, axis=-1)
    if kind == "l2_u8":
        return np.clip(desc.astype(np.int64) + np.rint(rng.normal(0.0, flip, desc.shape)).astype(np.int64), 0, 255).astype(np.uint8)
    raise ValueError("kind must be 'hamming' or 'l2_u8'")


def attach_descriptors(keyframes, seed: int, kind: str = "hamming", flip: float = 0.06, desc_bytes: int | None = None):
    """Give every keyframe a ``descriptors`` array (K, B) uint8, one row per keypoint: every landmark id of the
    sequence gets one random descriptor, every observation of it a copy disturbed by ``flip`` (``disturb``), and a
    keypoint that maps to no landmark a random descriptor of its own. The generator is this function's own, so the
    sequence's other outputs (``make_tum_sequence``) do not move. Returns ``keyframes``."""
    rng = np.random.default_rng(seed)
    nbytes = int(desc_bytes or DEFAULT_BYTES[kind])
    ids = sorted({lid for kf in keyframes for lid in kf.global_points_map.values()})
    row = {lid: i for i, lid in enumerate(ids)}
    base = rng.integers(0, 256, size=(len(ids), nbytes), dtype=np.uint8)
    for kf in keyframes:
        d = rng.integers(0, 256, size=(len(kf.keypoints), nbytes), dtype=np.uint8)
        local = np.array(list(kf.global_points_map.keys()), dtype=np.int64)
        if len(local):
            src = np.array([row[kf.global_points_map[int(i)]] for i in local], dtype=np.int64)
            d[local] = disturb(rng, base[src], kind, flip)
        kf.descriptors = d
    return keyframes


def correspondences(out: dict, j: int, pts_q, pts_t):
    """(p1, p2): the ``points3d_local`` of the accepted matches of pair ``j`` of a ``Solver.match`` output, p1 from the
    query keyframe's points and p2 from the train keyframe's, in the matches' order, without the matches whose depth
    is not above 1e-15 in either frame (main.cpp:58-62 hands exactly these to initializeRelativePose)."""
    m = np.asarray(out["matches"])[int(out["match_begin"][j]):int(out["match_begin"][j + 1])]
    pts_q = np.asarray(pts_q, dtype=np.float64).reshape(-1, 3)
    pts_t = np.asarray(pts_t, dtype=np.float64).reshape(-1, 3)
    p1, p2 = pts_q[m[:, 0]], pts_t[m[:, 1]]
    keep = (p1[:, 2] > 1e-15) & (p2[:, 2] > 1e-15)
    return np.ascontiguousarray(p1[keep]), np.ascontiguousarray(p2[keep])


def matched_edges(keyframes, pairs, match, align, min_inliers: int = 20, match_kw: dict | None = None, **kw):
    """(edge_a, edge_b, meas, n_inliers) of the pairs (m, 2) of keyframes, measured from their descriptors: one
    ``match(query, train, pair_range, **match_kw)`` call for all pairs (``match``: a ``miba.solver.Solver().match``;
    keyframe a's descriptors are the queries of pair (a, b), b's the trains; the call's one array holds every keyframe's
    descriptors once however many pairs it is part of, and is passed as the query set and as the train set, so the
    device holds two copies of it), ``correspondences`` of every pair, and one
    ``align(p1, p2, pair_begin, **kw)`` call for all of them. Its pose is ``Z_ab = T_a^-1 T_b``. A pair without a model
    or with fewer than ``min_inliers`` inliers is dropped. The keyframes' ``kind`` is ``match_kw``'s."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 7)), np.zeros(0, dtype=np.int64)
    used = sorted(set(pairs.ravel().tolist()))
    begin, at = {}, 0
    for c in used:
        begin[c] = at
        at += len(keyframes[c].descriptors)
    desc = np.concatenate([np.asarray(keyframes[c].descriptors, dtype=np.uint8) for c in used])
    rng = np.array([[begin[a], begin[a] + len(keyframes[a].descriptors), begin[b], begin[b] + len(keyframes[b].descriptors)]
                    for a, b in pairs.tolist()], dtype=np.int32)
    out = match(desc, desc, rng, **(match_kw or {}))
    p1, p2, pb = [], [], [0]
    for j, (a, b) in enumerate(pairs.tolist()):
        x, y = correspondences(out, j, keyframes[a].points3d_local, keyframes[b].points3d_local)
        p1.append(x); p2.append(y)
        pb.append(pb[-1] + len(x))
    res = align(np.concatenate(p1).reshape(-1, 3), np.concatenate(p2).reshape(-1, 3), np.array(pb, dtype=np.int32), **kw)
    stats = np.asarray(res["stats"])
    n_in = stats[:, 2].astype(np.int64)
    keep = (stats[:, 0] == 0) & (n_in >= min_inliers)
    return (pairs[keep, 0].astype(np.int32), pairs[keep, 1].astype(np.int32),
            np.asarray(res["poses"], dtype=np.float64)[keep], n_in[keep])


def landmark_descriptors(keyframes):
    """(ids, desc): every landmark id the keyframes observe, in the order of its first observation (keyframe order,
    then the order of ``global_points_map``), with the descriptor of that first observation. ids (n,) int64, desc
    (n, B) uint8. Keyframes without descriptors are passed over."""
    ids, desc, have = [], [], set()
    for kf in keyframes:
        if kf.descriptors is None:
            continue
        for local_id, landmark_id in kf.global_points_map.items():
            if landmark_id not in have:
                have.add(landmark_id)
                ids.append(landmark_id)
                desc.append(kf.descriptors[local_id])
    nbytes = next((kf.descriptors.shape[1] for kf in keyframes if kf.descriptors is not None), 0)
    return np.array(ids, dtype=np.int64), np.array(desc, dtype=np.uint8).reshape(-1, nbytes)


def fuse_landmarks(keyframes, landmarks, pairs, intr, width: int, height: int, guided_match, **kw):
    """ORB-SLAM's Fuse after a loop closure: for each (a, b) of ``pairs`` the landmarks keyframe a observes (and b does
    not) are projected into keyframe b with the poses and the map as they stand, and searched for among all of b's
    keypoints: one ``guided_match(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, frame_range=...,
    cand=..., kp_depth=..., **kw)`` call for all pairs (a ``miba.solver.Solver().guided_match``; every keyframe b's
    keypoints are in the call once). The accepted matches are applied in the order of the pairs: a match on a keypoint
    that maps to no landmark adds the observation to b's ``global_points_map`` (unless b observes that landmark by
    then); a match on a keypoint that maps to another id merges the two: the landmark with more observations is kept
    (on a tie the smaller id), every ``global_points_map`` entry of the other is rewritten to it and the other is
    dropped from ``landmarks``. Returns the merges as (kept id, dropped id) in the order they were made."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return []
    ids, desc = landmark_descriptors(keyframes)
    row = {int(l): i for i, l in enumerate(ids)}
    targets = sorted(set(pairs[:, 1].tolist()))
    begin, at = {}, 0
    for b in targets:
        begin[b] = at
        at += len(keyframes[b].keypoints)
    kp_uv = np.concatenate([np.asarray(keyframes[b].keypoints, dtype=np.float64).reshape(-1, 2) for b in targets])
    kp_desc = np.concatenate([np.asarray(keyframes[b].descriptors, dtype=np.uint8) for b in targets])
    kp_depth = np.concatenate([np.asarray(keyframes[b].points3d_local, dtype=np.float64).reshape(-1, 3)[:, 2] for b in targets])
    points = np.array([landmarks[int(l)] for l in ids], dtype=np.float64).reshape(-1, 3)
    cand, poses, ranges = [], [], []
    for a, b in pairs.tolist():
        in_b = set(keyframes[b].global_points_map.values())
        seen, c = set(), []
        for landmark_id in keyframes[a].global_points_map.values():
            if landmark_id not in in_b and landmark_id not in seen:
                seen.add(landmark_id)
                c.append(row[landmark_id])
        cand.append(np.array(c, dtype=np.int32))
        poses.append(np.asarray(keyframes[b].T_w_c, dtype=np.float64))
        ranges.append((begin[b], begin[b] + len(keyframes[b].keypoints)))
    out = guided_match(points, desc, kp_uv, kp_desc, np.array(poses).reshape(-1, 7), intr, width, height,
                       frame_range=np.array(ranges, dtype=np.int32), cand=cand, kp_depth=kp_depth, **kw)
    alias, merges = {}, []

    def current(landmark_id):
        while landmark_id in alias:
            landmark_id = alias[landmark_id]
        return landmark_id

    def n_obs(landmark_id):
        return sum(1 for kf in keyframes for g in kf.global_points_map.values() if g == landmark_id)

    for j, (a, b) in enumerate(pairs.tolist()):
        gpm = keyframes[b].global_points_map
        for pt, kp in np.asarray(out["matches"])[int(out["match_begin"][j]):int(out["match_begin"][j + 1])].tolist():
            found = current(int(ids[pt]))
            there = gpm.get(kp)
            if there is None:
                if found not in gpm.values():
                    gpm[kp] = found
                continue
            if there == found:
                continue
            na, nb = n_obs(found), n_obs(there)
            keep, drop = (found, there) if (na, -found) > (nb, -there) else (there, found)
            for kf in keyframes:
                for local_id, g in kf.global_points_map.items():
                    if g == drop:
                        kf.global_points_map[local_id] = keep
            landmarks.pop(drop, None)
            alias[drop] = keep
            merges.append((keep, drop))
    return merges
