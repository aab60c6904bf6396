"""Two independent references of the covariance of a window's estimate (test infrastructure).

Both start from ``refstep._Lin(prob, opts, radius=inf)`` (the oracle's per-observation Jacobians, Jacobi-scaled, no
damping) and return Sigma = (J^T J)^-1 in the tangent space of ``ba_debug_linearize``, unscaled:

* ``qr_cov``     QR of the whole scaled Jacobian (the construction of ``refstep.qr_step`` without the D rows),
                 Sigma = R^-1 R^-T. No Schur complement, no normal equations. Dense: windows up to about 25 cameras.
* ``schur_cov``  the points eliminated in extended precision as ``refstep.schur_step`` does, the reduced matrix
                 inverted in f64 and (n <= 500, ``refine=True``) corrected by three Newton steps X += X (I - S X) in
                 extended precision; the points by Sigma_pp = V^-1 + T^T Sigma[cols, cols] T, T = E V^-1. Also
                 returns cond_2 of the scaled, undamped reduced matrix.

Both return ``Cov(ac_cam, red, pts, cond)``: the active cameras in increasing order, the (6 nac + 4)^2 covariance of
cameras and intrinsics ordered as ``ba_debug_reduced_system``, and a 3x3 block per point in the caller's order (NaN
for a point without an admissible observation).

Error metric (``pair_errors`` / ``point_errors``): for a pair of blocks (a, b) max|delta| / sqrt(max|S_aa| max|S_bb|),
for a point max|delta| / max|S_pp|; the tolerance is ``refstep.step_tol(cond)``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import refstep
from refstep import LD, _Lin, _inv3

REFINE_MAX_N = 500


class Cov(NamedTuple):
    ac_cam: np.ndarray
    red: np.ndarray
    pts: np.ndarray
    cond: Optional[float]


def _lin(prob, opts):
    return _Lin(prob, opts, float("inf"))


def _pts_out(L, blocks):
    pts = np.full((L.n_points, 3, 3), np.nan)
    if L.nap:
        pts[L.pt_idx] = blocks
    return pts


def qr_cov(prob, opts=None) -> Cov:
    L = _lin(prob, opts)
    n, no = L.n, L.no
    A = np.zeros((3 * no + 4, n))
    rows = 3 * np.arange(no)[:, None] + np.arange(3)[None, :]
    for k in range(6):
        A[rows, (6 * L.acz + k)[:, None]] += L.Jc[:, :, k].astype(np.float64)  # (zero for the gauge's observations)
    for k in range(3):
        A[rows, (L.o_p + 3 * L.ap + k)[:, None]] = L.Jp[:, :, k].astype(np.float64)
    for k in range(4):
        A[rows, L.o_k + k] = L.Jk[:, :, k].astype(np.float64)
    A[3 * no + np.arange(4), L.o_k + np.arange(4)] = L.Pk.astype(np.float64)
    R = np.linalg.qr(A, mode="r")
    Ri = np.linalg.solve(R, np.eye(n))
    s = np.concatenate([L.s_c.ravel(), L.s_p.ravel(), L.s_k]).astype(np.float64)
    full = (Ri @ Ri.T) * s[:, None] * s[None, :]
    red_idx = np.concatenate([np.arange(L.o_p), L.o_k + np.arange(4)])
    red = full[np.ix_(red_idx, red_idx)]
    blocks = np.zeros((L.nap, 3, 3))
    for p in range(L.nap):
        j = L.o_p + 3 * p
        blocks[p] = full[j: j + 3, j: j + 3]
    return Cov(L.ac_cam, red, _pts_out(L, blocks), None)


def schur_cov(prob, opts=None, refine: bool = True) -> Cov:
    L = _lin(prob, opts)
    nac, nr = L.nac, 6 * L.nac + 4
    kb = 6 * nac
    S = np.zeros((nr, nr), LD)
    Ucc = np.einsum("ora,orb->oab", L.Jc, L.Jc)
    Cck = np.einsum("ora,ork->oak", L.Jc, L.Jk)
    for o in np.nonzero(L.on)[0]:
        c0 = 6 * L.ac[o]
        S[c0: c0 + 6, c0: c0 + 6] += Ucc[o]
        S[c0: c0 + 6, kb:] += Cck[o]
        S[kb:, c0: c0 + 6] += Cck[o].T
    S[kb:, kb:] += np.einsum("ora,orb->ab", L.Jk, L.Jk) + np.diag(L.Pk * L.Pk)
    Vo = np.einsum("ora,orb->oab", L.Jp, L.Jp)
    Wo = np.einsum("ora,ori->oai", L.Jc, L.Jp)  # 6x3
    Ko = np.einsum("ork,ori->oki", L.Jk, L.Jp)  # 4x3
    order = np.argsort(L.ap, kind="stable")
    bounds = np.searchsorted(L.ap[order], np.arange(L.nap + 1))
    keep = []
    for p in range(L.nap):
        obs = order[bounds[p]: bounds[p + 1]]
        Vi = _inv3(Vo[obs].sum(0))  # no damping: d2_p = clip / inf = 0
        cams = np.unique(L.ac[obs][L.on[obs]])
        E = np.zeros((6 * len(cams) + 4, 3), LD)  # [W_p; K_p]
        for o in obs[L.on[obs]]:
            j = 6 * int(np.searchsorted(cams, L.ac[o]))
            E[j: j + 6] += Wo[o]
        E[6 * len(cams):] = Ko[obs].sum(0)
        cols = np.concatenate([(6 * cams[:, None] + np.arange(6)[None, :]).ravel(), kb + np.arange(4)]).astype(np.int64)
        T = E @ Vi
        S[np.ix_(cols, cols)] -= T @ E.T
        keep.append((cols, T, Vi))
    S64 = S.astype(np.float64)
    S64 = (S64 + S64.T) / 2
    X = np.linalg.inv(S64).astype(LD)
    if refine and nr <= REFINE_MAX_N:
        I = np.eye(nr, dtype=LD)
        for _ in range(3):
            X = X + X @ (I - S @ X)
    X = (X + X.T) / 2
    s = np.concatenate([L.s_c.ravel(), L.s_k])
    red = (X * s[:, None] * s[None, :]).astype(np.float64)
    blocks = np.zeros((L.nap, 3, 3))
    for p, (cols, T, Vi) in enumerate(keep):
        B = Vi + T.T @ X[np.ix_(cols, cols)] @ T
        blocks[p] = (B * L.s_p[p][:, None] * L.s_p[p][None, :]).astype(np.float64)
    return Cov(L.ac_cam, red, _pts_out(L, blocks), float(np.linalg.cond(S64)))


def _blocks(nac):
    return [(6 * a, 6) for a in range(nac)] + [(6 * nac, 4)]


def pair_errors(got, ref) -> float:
    """Max over all block pairs (cameras and intrinsics) of max|got - ref| / sqrt(max|ref_aa| max|ref_bb|)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nac = (ref.shape[0] - 4) // 6
    bl = _blocks(nac)
    dmax = np.array([np.abs(ref[o: o + d, o: o + d]).max() for o, d in bl])
    edges = [o for o, _ in bl] + [ref.shape[0]]
    diff = np.abs(got - ref)
    diff = np.where(np.isnan(diff), np.inf, diff)
    bmax = np.maximum.reduceat(np.maximum.reduceat(diff, edges[:-1], axis=0), edges[:-1], axis=1)
    return float((bmax / np.sqrt(dmax[:, None] * dmax[None, :])).max())


def point_errors(got, ref) -> float:
    """Max over the estimable points of max|got - ref| / max|ref_pp|; a point that is NaN in the reference must be
    NaN in ``got`` (else inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not len(ref):
        return 0.0
    nan_ref = np.isnan(ref).any((1, 2))
    if not np.isnan(got[nan_ref]).all() or np.isnan(got[~nan_ref]).any():
        return float("inf")
    g, r = got[~nan_ref], ref[~nan_ref]
    if not len(r):
        return 0.0
    return float((np.abs(g - r).max((1, 2)) / np.abs(r).max((1, 2))).max())


# ------------------------------------------------------------------------------------------------ the windows
# refstep.WINDOWS plus one: cov200, the reduced size of the C4 benchmark window (n = 1204, 19 block columns of 64)
WINDOWS = dict(refstep.WINDOWS)
WINDOWS["cov200"] = refstep._w(201, (4, 9), 901)

_cache = {}


def window(name):
    """The window ``name`` (cached; callers must not modify it)."""
    if name in refstep.WINDOWS:
        return refstep.window(name)
    if ("w", name) not in _cache:
        from miba import synthetic
        _cache[("w", name)] = synthetic.make_problem(**WINDOWS[name])
    return _cache[("w", name)]


def reference(name, jacobi_scaling=1):
    """(window, schur_cov) of ``name``, cached."""
    key = ("r", name, int(jacobi_scaling))
    if key not in _cache:
        from oracle import oracle
        opts = None if jacobi_scaling else oracle.default_options(jacobi_scaling=0)
        p = window(name)
        _cache[key] = (p, schur_cov(p, opts))
    return _cache[key]
