"""Host-side helpers around ``Solver.pose_graph`` (numpy only): building the edges of a pose graph and carrying the
result over to the map.

Poses are ``ba_problem``'s: ``(qx, qy, qz, qw, tx, ty, tz)``, camera-to-world. An edge (a, b) carries the relative pose
``Z_ab = T_a^-1 T_b`` in the same layout.

* ``relative_pose(Ta, Tb)`` / ``compose(T, Z)``: ``T_a^-1 T_b`` and ``T Z`` (``compose(Ta, relative_pose(Ta, Tb))`` is
  ``Tb``).
* ``edges_from_poses(cams, pairs)``: the edge arrays ``Solver.pose_graph`` takes, measured on the poses ``cams``.
* ``measured_edges(prob, pairs, align)``: the same edge arrays measured from the data: for every pair the landmarks
  both keyframes observe, back-projected into the two camera frames and handed to ``align`` (a
  ``Solver().align``): the loop-edge measurement, which ``edges_from_poses`` can only read off the drifted poses.
* ``covis_edges(W, min_weight)``: ORB-SLAM's essential graph from ``Solver.covisibility``'s weights: every pair that
  shares at least ``min_weight`` points, plus a maximum-weight spanning forest of the co-visibility graph so that
  what is connected there stays connected.
* ``transfer_points(points, ref_cam, cams_before, cams_after)``: the map-point correction that follows a pose-graph
  pass: each landmark moves with its reference keyframe, ``X' = T_after T_before^-1 X``.
"""
from __future__ import annotations

import numpy as np


def quat_mul(p, q):
    """Hamilton product of quaternions (x y z w); broadcasts over leading axes."""
    p, q = np.asarray(p), np.asarray(q)
    px, py, pz, pw = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw,
                     pw * qw - px * qx - py * qy - pz * qz], axis=-1)


def quat_conj(q):
    q = np.asarray(q)
    return np.concatenate([-q[..., :3], q[..., 3:]], axis=-1)


def quat_rotate(q, v):
    """R(q) v for unit quaternions (x y z w)."""
    q, v = np.asarray(q), np.asarray(v)
    qv, qw = q[..., :3], q[..., 3:]
    uv = 2 * np.cross(qv, v)
    return v + qw * uv + np.cross(qv, uv)


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def relative_pose(Ta, Tb):
    """Z_ab = T_a^-1 T_b; (7,) or (n, 7)."""
    Ta, Tb = np.asarray(Ta, dtype=np.float64), np.asarray(Tb, dtype=np.float64)
    qa = _unit(Ta[..., :4])
    q = quat_mul(quat_conj(qa), _unit(Tb[..., :4]))
    t = quat_rotate(quat_conj(qa), Tb[..., 4:] - Ta[..., 4:])
    return np.concatenate([_unit(q), t], axis=-1)


def compose(T, Z):
    """T Z; (7,) or (n, 7)."""
    T, Z = np.asarray(T, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    qt = _unit(T[..., :4])
    q = quat_mul(qt, _unit(Z[..., :4]))
    t = T[..., 4:] + quat_rotate(qt, Z[..., 4:])
    return np.concatenate([_unit(q), t], axis=-1)


def edges_from_poses(cams, pairs):
    """(edge_a, edge_b, meas) of the pairs (m, 2), measured on ``cams`` (n, 7)."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ea, eb = pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)
    if len(pairs) == 0:
        return ea, eb, np.zeros((0, 7))
    return ea, eb, relative_pose(cams[ea], cams[eb])


def measured_edges(prob, pairs, align, min_inliers: int = 20, **kw):
    """(edge_a, edge_b, meas, n_inliers) of the pairs (m, 2) of keyframes of the window ``prob`` (a ``ProblemArrays``),
    measured from their shared observations: for a pair (a, b) the landmarks both keyframes observe with an admissible
    depth (the first such observation of a landmark in each keyframe), back-projected with ``prob.intr`` into a's and
    b's camera frames -- ``((u - cx) / fx d, (v - cy) / fy d, d)`` -- are the clouds p1 and p2 of one pair of a single
    ``align(p1, p2, pair_begin, **kw)`` call for all pairs (``align``: a ``miba.solver.Solver().align``). Its pose is
    ``Z_ab = T_a^-1 T_b``. A pair without a model or with fewer than ``min_inliers`` inliers is dropped."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    fx, fy, cx, cy = (float(v) for v in prob.intr)
    # per keyframe: landmark -> the back-projection of its first admissible observation
    local = {}
    for c in set(pairs.ravel().tolist()):
        rows = np.nonzero((prob.obs_cam == c) & (prob.obs_depth > 1e-15))[0]
        pts, first = np.unique(prob.obs_pt[rows], return_index=True)
        rows = rows[first]
        d = prob.obs_depth[rows]
        xyz = np.stack([(prob.obs_uv[rows, 0] - cx) / fx * d, (prob.obs_uv[rows, 1] - cy) / fy * d, d], 1)
        local[c] = (pts, xyz)
    p1, p2, begin = [], [], [0]
    for a, b in pairs:
        (pa, xa), (pb, xb) = local[int(a)], local[int(b)]
        _, ia, ib = np.intersect1d(pa, pb, assume_unique=True, return_indices=True)
        p1.append(xa[ia])
        p2.append(xb[ib])
        begin.append(begin[-1] + len(ia))
    if len(pairs) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 7)), np.zeros(0, dtype=np.int64)
    out = align(np.concatenate(p1).reshape(-1, 3), np.concatenate(p2).reshape(-1, 3), np.array(begin, dtype=np.int32), **kw)
    stats = np.asarray(out["stats"])
    n_in = stats[:, 2].astype(np.int64)
    keep = (stats[:, 0] == 0) & (n_in >= min_inliers)
    return (pairs[keep, 0].astype(np.int32), pairs[keep, 1].astype(np.int32),
            np.asarray(out["poses"], dtype=np.float64)[keep], n_in[keep])


def covis_edges(W, min_weight: int):
    """Pairs (m, 2), i < j, sorted: W[i, j] >= min_weight, plus a maximum-weight spanning forest of the graph W > 0
    (Kruskal; ties broken by the pair's indices, so the result is deterministic)."""
    W = np.asarray(W)
    n = W.shape[0]
    iu, ju = np.triu_indices(n, 1)
    w = W[iu, ju]
    pos = w > 0
    iu, ju, w = iu[pos], ju[pos], w[pos]
    keep = set(zip(iu[w >= min_weight].tolist(), ju[w >= min_weight].tolist()))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for k in np.lexsort((ju, iu, -w)):
        a, b = find(int(iu[k])), find(int(ju[k]))
        if a != b:
            parent[a] = b
            keep.add((int(iu[k]), int(ju[k])))
    return np.array(sorted(keep), dtype=np.int32).reshape(-1, 2)


def transfer_points(points, ref_cam, cams_before, cams_after):
    """X' = T_after T_before^-1 X with T the pose of each point's reference keyframe ``ref_cam`` (n_points,)."""
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ref = np.asarray(ref_cam, dtype=np.int64).reshape(-1)
    B = np.asarray(cams_before, dtype=np.float64).reshape(-1, 7)[ref]
    A = np.asarray(cams_after, dtype=np.float64).reshape(-1, 7)[ref]
    local = quat_rotate(quat_conj(_unit(B[:, :4])), X - B[:, 4:])
    return A[:, 4:] + quat_rotate(_unit(A[:, :4]), local)
