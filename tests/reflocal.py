"""An independent restatement of ba_local_window's selection and of the sub-window's assembly (test infrastructure).

Plain Python sets and sorted lists over the observation arrays, no bit rows: ``select`` follows the definitions of
include/ba.h (w, L, P, F, the sub-window's cameras, points and observations, the constant cameras, the sub-window's
gauge) literally; ``sub_problem`` gathers the sub-window as a ``ProblemArrays``; ``scatter_back`` puts a solved
sub-window's local cameras and points back into the map. The window builders of the selection tests are here too.
"""
from __future__ import annotations

import numpy as np

from miba.capi import ProblemArrays


def select(prob, center, min_weight=15, max_local=0, mask=None) -> dict:
    """The selection around ``center``. ``mask``: the context's constant cameras (n_cams,) or None."""
    nc = prob.n_cams
    assert 0 <= center < nc
    if min_weight <= 0:
        min_weight = 1
    adm = [k for k in range(prob.n_obs) if prob.obs_depth[k] > 1e-15]
    sees = [set() for _ in range(nc)]  # the distinct points a camera sees through admissible observations
    for k in adm:
        sees[int(prob.obs_cam[k])].add(int(prob.obs_pt[k]))
    w = [len(sees[a] & sees[center]) for a in range(nc)]
    out = dict(w=np.array(w, dtype=np.int32))
    if not sees[center]:
        out.update(cam_index=np.array([center], np.int32), cam_constant=np.array([False]), cam_local=np.array([True]),
                   pt_index=np.zeros(0, np.int32), obs_index=np.zeros(0, np.int32), sub_obs_cam=np.zeros(0, np.int32),
                   sub_obs_pt=np.zeros(0, np.int32), n_local=1, n_fixed=0, n_points=0, n_obs=0, sub_fixed_cam=0)
        return out
    cand = [a for a in range(nc) if a != center and w[a] >= min_weight]
    if max_local > 0 and 1 + len(cand) > max_local:
        cand = sorted(cand, key=lambda a: (-w[a], a))[: max_local - 1]
    L = sorted([center] + cand)
    P = sorted(set().union(*(sees[a] for a in L)))
    Pset = set(P)
    F = [a for a in range(nc) if a not in L and sees[a] & Pset]
    cams = sorted(L + F)
    const = []
    for a in cams:
        c = a in F or a == prob.fixed_cam
        if mask is not None and len(mask) == nc and mask[a]:
            c = True
        const.append(bool(c))
    cam_new = {a: i for i, a in enumerate(cams)}
    pt_new = {p: i for i, p in enumerate(P)}
    obs = [k for k in adm if int(prob.obs_pt[k]) in Pset]
    out.update(cam_index=np.array(cams, np.int32), cam_constant=np.array(const, bool),
               cam_local=np.array([a in L for a in cams], bool), pt_index=np.array(P, np.int32),
               obs_index=np.array(obs, np.int32),
               sub_obs_cam=np.array([cam_new[int(prob.obs_cam[k])] for k in obs], np.int32),
               sub_obs_pt=np.array([pt_new[int(prob.obs_pt[k])] for k in obs], np.int32),
               n_local=len(L), n_fixed=len(F), n_points=len(P), n_obs=len(obs),
               sub_fixed_cam=-1 if any(const) else cam_new[L[0]])
    return out


INT_KEYS = ("w", "cam_index", "cam_constant", "cam_local", "pt_index", "obs_index", "sub_obs_cam", "sub_obs_pt")
INFO_KEYS = ("n_local", "n_fixed", "n_points", "n_obs", "sub_fixed_cam")


def assert_same(got: dict, ref: dict, what=""):
    """Every integer of a selection, exactly."""
    for k in INFO_KEYS:
        assert int(got[k]) == int(ref[k]), (what, k, got[k], ref[k])
    for k in INT_KEYS:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64),
                                      err_msg=f"{what} {k}")


def sub_problem(prob, sel) -> ProblemArrays:
    """The sub-window of a selection: cameras, points and observation values gathered (copies), intrinsics and prior
    copied, ``fixed_cam`` the sub-window's gauge. Its constant cameras are ``sel["cam_constant"]``."""
    oi = np.asarray(sel["obs_index"], dtype=np.int64)
    return ProblemArrays(prob.cams[sel["cam_index"]].copy(), prob.points[sel["pt_index"]].copy(), prob.intr.copy(),
                         prob.intr_prior.copy(), np.asarray(sel["sub_obs_cam"], np.int32).copy(),
                         np.asarray(sel["sub_obs_pt"], np.int32).copy(), prob.obs_uv[oi].copy(),
                         prob.obs_depth[oi].copy(), int(sel["sub_fixed_cam"]))


def scatter_back(prob, sel, sub) -> None:
    """The solved sub-window ``sub`` into the map: L's cameras that are not constant, P's points, the intrinsics."""
    for i, a in enumerate(sel["cam_index"]):
        if sel["cam_local"][i] and not sel["cam_constant"][i] and i != sel["sub_fixed_cam"]:
            prob.cams[a] = sub.cams[i]
    prob.points[sel["pt_index"]] = sub.points
    prob.intr[:] = sub.intr


# ------------------------------------------------------------------------------------------------ window builders
def make_map(n_cams, n_points, n_obs, seed, span=4, dup_frac=0.1, bad_frac=0.1, fixed_cam=0) -> ProblemArrays:
    """An integer-only map for the selection tests (the parameters are never evaluated): observation k sees a point
    and a camera within ``span`` of the point's home camera, a fraction repeated (the same camera and point again) and
    a fraction inadmissible (depth 0 or -inf). Exactly ``n_obs`` observations."""
    rng = np.random.default_rng(seed)
    home = rng.integers(0, max(n_cams, 1), max(n_points, 1))
    pt = rng.integers(0, max(n_points, 1), n_obs).astype(np.int32)
    cam = ((home[pt] + rng.integers(0, span, n_obs)) % max(n_cams, 1)).astype(np.int32)
    dup = np.nonzero(rng.random(n_obs) < dup_frac)[0]
    dup = dup[dup > 0]
    pt[dup], cam[dup] = pt[dup - 1], cam[dup - 1]
    depth = rng.uniform(0.5, 4.0, n_obs)
    bad = rng.random(n_obs) < bad_frac
    depth[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0.0, -np.inf)
    cams = np.zeros((n_cams, 7))
    cams[:, 3] = 1.0
    intr = np.array([525.0, 525.0, 319.5, 239.5])
    return ProblemArrays(cams, rng.normal(size=(n_points, 3)), intr, intr.copy(), cam, pt,
                         rng.uniform(0, 480, (n_obs, 2)), depth, fixed_cam)


def from_lists(n_cams, n_points, obs, fixed_cam=-1) -> ProblemArrays:
    """A hand-written map: ``obs`` is a list of (camera, point) or (camera, point, depth)."""
    cam = np.array([o[0] for o in obs], np.int32)
    pt = np.array([o[1] for o in obs], np.int32)
    depth = np.array([o[2] if len(o) > 2 else 1.0 for o in obs], np.float64)
    cams = np.zeros((n_cams, 7))
    cams[:, 3] = 1.0
    intr = np.array([525.0, 525.0, 319.5, 239.5])
    return ProblemArrays(cams, np.zeros((n_points, 3)), intr, intr.copy(), cam, pt, np.zeros((len(obs), 2)), depth,
                         fixed_cam)
