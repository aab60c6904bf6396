"""The co-visibility graph of a window and its camera ordering, restated in numpy (test infrastructure).

What ba_covisibility reports and ba_solve_ordered uses, from the problem arrays alone:

* ``weights``     W[a][b] = distinct points cameras a and b both see through admissible observations (depth > 1e-15),
                  W[a][a] = distinct points a sees; the gauge camera included.
* ``rcm_order``   the candidate order: reverse Cuthill-McKee over the active cameras (W[i][i] > 0, i != fixed_cam; an
                  edge where W[i][j] > 0). Per component: start at the unvisited node of lowest (degree, index),
                  breadth-first, each node's unvisited neighbours appended sorted by (degree, index), the component's
                  list reversed; components in the order they were started; then the gauge camera and the cameras
                  without an admissible observation, in index order.
* ``band``        refstep.camera_band: max a - fc[a] over the active cameras, in active-camera index space.
* ``wide``        points with an admissible active observation whose active cameras span more than TILE_WIN positions.
* ``ordering``    the report: the candidate is accepted only if band_after < band_before and wide_after <= wide_before,
                  otherwise the identity with order_changed = 0 and the before values repeated.
"""
from __future__ import annotations

import numpy as np

import refstep

TILE_WIN = 12          # ba_kernels.h: cameras per Schur tile window
COVIS_TILE = 16        # ba_covis.h: camera pairs per workgroup, 16 x 16
COVIS_SLICE_WORDS = 128  # ba_covis.h: 64-bit words of a camera's row one workgroup handles


def weights(prob) -> np.ndarray:
    adm = prob.obs_depth > 1e-15
    B = np.zeros((prob.n_cams, prob.n_points), np.int64)
    B[prob.obs_cam[adm], prob.obs_pt[adm]] = 1
    return (B @ B.T).astype(np.int32)


def active(W, fixed_cam) -> np.ndarray:
    a = np.diag(W) > 0
    if 0 <= fixed_cam < len(a):
        a[fixed_cam] = False
    return a


def rcm_order(W, fixed_cam):
    """(order, n_components, n_active, n_edges) of the candidate order."""
    n = W.shape[0]
    act = active(W, fixed_cam)
    adj = (W > 0) & act[:, None] & act[None, :]
    adj[np.arange(n), np.arange(n)] = False
    deg = adj.sum(1)
    visited = ~act
    order, ncomp = [], 0
    while not visited.all():
        cand = np.nonzero(~visited)[0]
        start = int(cand[np.lexsort((cand, deg[cand]))[0]])
        ncomp += 1
        comp = [start]
        visited[start] = True
        head = 0
        while head < len(comp):
            v = comp[head]
            head += 1
            nb = np.nonzero(adj[v] & ~visited)[0]
            nb = nb[np.lexsort((nb, deg[nb]))]
            visited[nb] = True
            comp.extend(int(x) for x in nb)
        order.extend(comp[::-1])
    order.extend(int(i) for i in np.nonzero(~act)[0])
    return np.asarray(order, np.int32), ncomp, int(act.sum()), int(adj.sum()) // 2


def permute(prob, order):
    """The window with the camera ``order[k]`` placed k-th (a copy; observations, points and intrinsics as given)."""
    order = np.asarray(order, np.int64)
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    q = prob.copy()
    q.cams = np.ascontiguousarray(prob.cams[order])
    q.obs_cam = inv[prob.obs_cam].astype(np.int32)
    if 0 <= prob.fixed_cam < prob.n_cams:
        q.fixed_cam = int(inv[prob.fixed_cam])
    return q


def band(prob) -> int:
    return refstep.camera_band(prob)


def wide(prob) -> int:
    adm = prob.obs_depth > 1e-15
    cam, pt = prob.obs_cam[adm].astype(np.int64), prob.obs_pt[adm].astype(np.int64)
    ac_cam, _ = refstep.first_covisible(prob)
    cam_ac = np.full(prob.n_cams, -1, np.int64)
    cam_ac[ac_cam] = np.arange(len(ac_cam))
    ac = cam_ac[cam]
    lo = np.full(prob.n_points, np.iinfo(np.int64).max)
    hi = np.full(prob.n_points, -1, np.int64)
    np.minimum.at(lo, pt[ac >= 0], ac[ac >= 0])
    np.maximum.at(hi, pt[ac >= 0], ac[ac >= 0])
    return int(((hi >= 0) & (hi - lo + 1 > TILE_WIN)).sum())


_cache = {}


def ordering(prob, key=None) -> dict:
    """The report of ba_covisibility on ``prob`` (cached under ``key`` when given)."""
    if key is not None and key in _cache:
        return _cache[key]
    W = weights(prob)
    cand, ncomp, nact, nedge = rcm_order(W, prob.fixed_cam)
    b0, w0 = band(prob), wide(prob)
    q = permute(prob, cand)
    b1, w1 = band(q), wide(q)
    ok = b1 < b0 and w1 <= w0
    out = dict(weights=W, candidate=cand, candidate_band=b1, candidate_wide=w1,
               order=cand if ok else np.arange(prob.n_cams, dtype=np.int32), n_active=nact, n_edges=nedge,
               n_components=ncomp, band_before=b0, band_after=b1 if ok else b0, wide_before=w0,
               wide_after=w1 if ok else w0, order_changed=int(ok))
    if key is not None:
        _cache[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the windows
def two_scenes():
    """Two disjoint scenes with the cameras interleaved: make_problem(8, 200, 3, seed=2) twice, scene s's camera c
    at 2 c + s, its points after the other scene's. 16 cameras, 400 points, band 4 as given and 2 ordered."""
    from miba import synthetic
    from miba.capi import ProblemArrays
    a = synthetic.make_problem(8, 200, obs_per_point=3, seed=2)
    cams = np.zeros((16, 7))
    cams[0::2], cams[1::2] = a.cams, a.cams
    return ProblemArrays(cams, np.concatenate([a.points, a.points]), a.intr.copy(), a.intr_prior.copy(),
                         np.concatenate([2 * a.obs_cam, 2 * a.obs_cam + 1]),
                         np.concatenate([a.obs_pt, a.obs_pt + a.n_points]), np.concatenate([a.obs_uv, a.obs_uv]),
                         np.concatenate([a.obs_depth, a.obs_depth]), 0)


def relabelled_sweep50():
    """G2's shape (make_sweep_problem(50, 4000, seed=12)) with the cameras randomly relabelled."""
    from miba import synthetic
    p = synthetic.make_sweep_problem(50, 4000, seed=12)
    return permute(p, np.random.default_rng(0).permutation(50))


def window(name):
    """The named windows of the ordering tests (cached; callers must not modify them)."""
    if ("w", name) in _cache:
        return _cache[("w", name)]
    import refsweep
    from miba import synthetic
    if name in refsweep.SWEEPS:
        p = refsweep.window(name)
    elif name == "sweep42_gauge17":
        p = refsweep.window("sweep42").copy()
        p.fixed_cam = 17
    elif name == "sweep50_relabelled":
        p = relabelled_sweep50()
    elif name == "two_scenes":
        p = two_scenes()
    elif name == "g2_shape":
        p = synthetic.make_sweep_problem(50, 4000, seed=12)
    elif name == "g1_cams":
        p = synthetic.make_sweep_problem(200, 20000, seed=3)
    elif name == "sweep60_3pass":
        p = synthetic.make_sweep_problem(60, 3000, passes=3, obs_per_pass=4, seed=4)
    elif name.startswith("mp_"):
        nc, npt, opp = (int(v) for v in name[3:].split("_"))
        p = synthetic.make_problem(nc, npt, opp)
    else:
        p = refstep.window(name)
    _cache[("w", name)] = p
    return p


# the issue's table: window -> (band as given, ordered, points wider than TILE_WIN as given, ordered, order_changed)
TABLE = {
    "sweep22": (14, 7, 264, 0, 1),
    "sweep42": (25, 9, 504, 0, 1),
    "g2_shape": (29, 9, 4000, 0, 1),
    "g1_cams": (104, 9, 20000, 0, 1),
    "sweep60_3pass": (43, 11, 3000, 0, 1),
    "sweep42_gauge17": (24, 9, 504, 0, 1),
    "sweep50_relabelled": (47, 9, 4000, 0, 1),
    "mp_10_800_2": (1, 1, 0, 0, 0),
    "mp_20_2000_10": (9, 9, 0, 0, 0),
    "mp_50_4000_2": (1, 1, 0, 0, 0),
    "gauge_mid21": (8, 8, 0, 0, 0),
    "inactive_mid21": (8, 8, 0, 0, 0),
    "full31": (9, 9, 0, 0, 0),
    "bcr21_messy": (8, 8, 0, 0, 0),
    "dense_wide30": (15, 15, 56, 56, 0),
}
# what the refused candidate of dense_wide30 would give
DENSE_WIDE30_CANDIDATE = (15, 64)
