"""Reference for ba_align (no GPU, numpy only): the contract of include/ba.h restated in plain Python.

* ``mix`` / ``sample``: the minimal samples in Python integers (the header's text, bit for bit).
* ``arun_ref``: Arun's fit by an f64 SVD polished to ``np.longdouble``: Newton steps on "R H is symmetric" (the
  stationarity of tr(R H) over the rotations) with a Newton-Schulz step on R^T R = I between them.
* ``align``: the whole stage on the longdouble fit, with ``Solver.align``'s arguments and outputs. For every decision
  it records the *margin*: ``|d^2 - thr^2| / thr^2`` per hypothesis and correspondence (and per refit round), and
  ``|cross^2 - min_cross^2| / min_cross^2`` per sample. A case whose margins are far above the f64 rounding of the
  device has one right answer for every integer the stage returns.
* ``align64``: a plain f64 restatement of the kernel's own fit (Horn's 4x4 matrix, ``SWEEPS`` cyclic Jacobi sweeps,
  the operation order of csrc/ba_align_fit.h), whose distance to ``arun_ref`` sets the GPU test's pose bound.
* the seeded generators and the case lists the CPU and the GPU tests share.
"""
from __future__ import annotations

import functools
import math

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
M64 = (1 << 64) - 1

# the kernel's sizes (csrc/ba_align.h, include/ba.h); test_align_abi.py holds them to the headers
ALIGN_TPB = 256
ALIGN_TILE = 256
SWEEPS = 6
STAT_N = 8
MAX_HYP = 65536
OK, TOO_FEW, NO_MODEL = 0, 1, 2

# Every listed case clears this margin on every decision (test_refalign.py::test_margins measures 2.0e-5 as the
# smallest over all cases, on a threshold decision of "n-255"; every cross product is above 2e-2 against a min_cross of
# 1e-6, or far below it on the collinear pairs). The f64 rounding of a threshold decision is 2 F kappa eps max|p| / thr,
# about 2e-11 at kappa = 10, and test_margins also holds every hypothesis's own margin to 8 times its own rounding
# bound (the smallest quotient measured: 6e5).
MARGIN_MIN = 1e-5
# The largest f64 ratio: the pose action's error of align64 against arun_ref in units of kappa eps max|p|, over every
# fit (samples and refit rounds) of every case, as test_refalign.py::test_f64_ratio measured it on x86-64 (it asserts
# that the stored value covers what it measures and is not stale by more than a factor two): 4.41, on a sample of
# "n-513" with kappa = 8e4.
F64_RATIO = 4.5
# the pose bound's factor: max(8, 4 x the f64 ratio); the 4 for the device's own summation order (DESIGN 4.13's rule)
POSE_F = max(8.0, 4.0 * F64_RATIO)


# ------------------------------------------------------------------------------------------------ sampling
def mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def sample(seed: int, j: int, h: int, n: int):
    """The three distinct indices in [0, n) of hypothesis h of pair j (n >= 3)."""
    key = mix((seed & M64) ^ mix(((j << 32) | h) & M64))
    r1, r2, r3 = mix((key + 1) & M64), mix((key + 2) & M64), mix((key + 3) & M64)
    d0, d1, d2 = ((r1 >> 32) * n) >> 32, ((r2 >> 32) * (n - 1)) >> 32, ((r3 >> 32) * (n - 2)) >> 32
    i0 = d0
    i1 = d1 + (1 if d1 >= i0 else 0)
    lo, hi = min(i0, i1), max(i0, i1)
    i2 = d2
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


def samples(seed: int, j: int, n_hyp: int, n: int) -> np.ndarray:
    return np.array([sample(seed, j, h, n) for h in range(n_hyp)], dtype=np.int64).reshape(n_hyp, 3)


# ------------------------------------------------------------------------------------------------ poses
def quat_R(q):
    x, y, z, w = (q[..., k] for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def R_quat(R):
    """(x, y, z, w), w >= 0, of one rotation matrix (any float dtype), by the largest of the four squares."""
    R = np.asarray(R)
    m = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(m))
    s = np.sqrt(1 + m[k]) * 2
    if k == 0:
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    elif k == 1:
        q = [s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif k == 2:
        q = [(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q, dtype=R.dtype)
    q = q / np.sqrt((q * q).sum())
    return -q if q[3] < 0 else q


def act(pose, p2):
    """R p2 + t of a pose (7,) on points (n, 3), in the pose's dtype."""
    pose = np.asarray(pose)
    return np.asarray(p2, dtype=pose.dtype) @ quat_R(pose[:4]).T + pose[4:]


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------ the longdouble fit
def _axial(M):
    return np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)


def _skew(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def _solve3(J, b):
    r0, r1, r2 = J[..., 0, :], J[..., 1, :], J[..., 2, :]
    c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)
    det = (r0 * c0).sum(-1)
    return (c0 * b[..., 0:1] + c1 * b[..., 1:2] + c2 * b[..., 2:3]) / det[..., None]


def arun_ref(A1, A2):
    """Arun's fit of A1 ~ R A2 + t for point sets (..., m, 3), in longdouble. Returns (R, t, kappa, H): kappa =
    sigma1 / (sigma2 + d sigma3) of H = sum (p2 - c2)(p1 - c1)^T, d = +-1 the sign the det +1 constraint leaves on
    sigma3: the condition number of the rotation."""
    a1, a2 = np.asarray(A1).astype(LD), np.asarray(A2).astype(LD)
    m = a1.shape[-2]
    c1, c2 = a1.sum(-2) / LD(m), a2.sum(-2) / LD(m)
    H = np.einsum("...mi,...mk->...ik", a2 - c2[..., None, :], a1 - c1[..., None, :])
    U, S, Vt = np.linalg.svd(H.astype(np.float64))
    d = np.sign(np.linalg.det(np.swapaxes(Vt, -1, -2) @ np.swapaxes(U, -1, -2)))
    d = np.where(d == 0, 1.0, d)
    D = np.zeros(H.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    R = (np.swapaxes(Vt, -1, -2) @ D @ np.swapaxes(U, -1, -2)).astype(LD)
    I3 = np.eye(3, dtype=LD)
    E = np.eye(3, dtype=LD)
    for _ in range(4):
        R = R @ ((3 * I3 - np.swapaxes(R, -1, -2) @ R) / 2)
        M = R @ H
        g = _axial(M - np.swapaxes(M, -1, -2))
        cols = []
        for k in range(3):
            WM = _skew(np.broadcast_to(E[k], g.shape)) @ M
            cols.append(_axial(WM - np.swapaxes(WM, -1, -2)))
        J = np.stack(cols, -1)
        W = _skew(_solve3(J, -g))
        R = (I3 + W + W @ W / 2) @ R
    R = R @ ((3 * I3 - np.swapaxes(R, -1, -2) @ R) / 2)
    t = c1 - np.einsum("...ik,...k->...i", R, c2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = S[..., 0] / (S[..., 1] + d * S[..., 2])
    return R, t, kappa, H


def stationarity(R, H):
    """|axial(R H - (R H)^T)| / |H| and |R^T R - I|: both at the longdouble rounding for a polished fit."""
    M = R @ H
    g = np.abs(_axial(M - np.swapaxes(M, -1, -2))).max(-1) / np.abs(H).max((-1, -2))
    o = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3, dtype=LD)).max((-1, -2))
    return g, o


# ------------------------------------------------------------------------------------------------ the f64 restatement
def _jacobi4(A):
    """SWEEPS cyclic Jacobi sweeps on symmetric (B, 4, 4) f64, csrc/ba_align_fit.h's operations. Returns (A, V)."""
    A = A.copy()
    B = A.shape[0]
    V = np.broadcast_to(np.eye(4), (B, 4, 4)).copy()
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                apq = A[:, p, q].copy()
                on = apq != 0.0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                tt = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                tt = np.where(on, tt, 0.0)
                c = 1.0 / np.sqrt(tt * tt + 1.0)
                s = tt * c
                tap = np.where(on, tt * apq, 0.0)
                A[:, p, p] = A[:, p, p] - tap
                A[:, q, q] = A[:, q, q] + tap
                A[:, p, q] = A[:, q, p] = np.where(on, 0.0, apq)
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        A[:, r, p] = A[:, p, r] = np.where(on, c * arp - s * arq, arp)
                        A[:, r, q] = A[:, q, r] = np.where(on, s * arp + c * arq, arq)
                    vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p] = np.where(on, c * vrp - s * vrq, vrp)
                    V[:, r, q] = np.where(on, s * vrp + c * vrq, vrq)
    return A, V


def fit64_H(H, c1, c2):
    """align_fit_H in f64 on a batch: H (B, 3, 3), c1 / c2 (B, 3). Returns poses (B, 7) and the off-diagonal mass the
    sweeps left, relative to the diagonal's."""
    Sxx, Sxy, Sxz = H[:, 0, 0], H[:, 0, 1], H[:, 0, 2]
    Syx, Syy, Syz = H[:, 1, 0], H[:, 1, 1], H[:, 1, 2]
    Szx, Szy, Szz = H[:, 2, 0], H[:, 2, 1], H[:, 2, 2]
    A = np.empty((len(H), 4, 4))
    A[:, 0, 0] = (Sxx + Syy) + Szz
    A[:, 1, 1] = (Sxx - Syy) - Szz
    A[:, 2, 2] = (Syy - Sxx) - Szz
    A[:, 3, 3] = (Szz - Sxx) - Syy
    A[:, 0, 1] = A[:, 1, 0] = Syz - Szy
    A[:, 0, 2] = A[:, 2, 0] = Szx - Sxz
    A[:, 0, 3] = A[:, 3, 0] = Sxy - Syx
    A[:, 1, 2] = A[:, 2, 1] = Sxy + Syx
    A[:, 1, 3] = A[:, 3, 1] = Szx + Sxz
    A[:, 2, 3] = A[:, 3, 2] = Syz + Szy
    A, V = _jacobi4(A)
    diag = np.stack([A[:, k, k] for k in range(4)], -1)
    off = np.abs(A - diag[:, :, None] * np.eye(4)).max((1, 2)) / np.maximum(np.abs(diag).max(1), 1e-300)
    k = np.argmax(diag, axis=1)  # the first among equals
    q = V[np.arange(len(H)), :, k]
    nrm = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
    sg = np.where(q[:, 0] < 0.0, -1.0, 1.0)
    w, x, y, z = (sg * q[:, i] / nrm for i in range(4))
    quat = np.stack([x, y, z, w], -1)
    R = quat_R(quat)
    t = np.stack([c1[:, i] - ((R[:, i, 0] * c2[:, 0] + R[:, i, 1] * c2[:, 1]) + R[:, i, 2] * c2[:, 2]) for i in range(3)], -1)
    return np.concatenate([quat, t], -1), off


def fit64_samples(A1, A2):
    """align_fit3's model of the samples A1 / A2 (B, 3, 3) (sample point, coordinate) in f64."""
    c1 = ((A1[:, 0] + A1[:, 1]) + A1[:, 2]) / 3.0
    c2 = ((A2[:, 0] + A2[:, 1]) + A2[:, 2]) / 3.0
    a, b = A1 - c1[:, None, :], A2 - c2[:, None, :]
    H = (b[:, 0, :, None] * a[:, 0, None, :] + b[:, 1, :, None] * a[:, 1, None, :]) + b[:, 2, :, None] * a[:, 2, None, :]
    return fit64_H(H, c1, c2)


def fit64_set(P1, P2):
    """The refit's model of one inlier set P1 / P2 (m, 3) in f64: the centroids first, then H about them."""
    c1, c2 = P1.sum(0) / float(len(P1)), P2.sum(0) / float(len(P2))
    H = np.einsum("mi,mk->ik", P2 - c2, P1 - c1)
    pose, off = fit64_H(H[None], c1[None], c2[None])
    return pose[0], off[0]


# ------------------------------------------------------------------------------------------------ the stage
def _cross2(P):
    u, v = P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :]
    c = np.cross(u, v)
    return (c * c).sum(-1)


def _dist2(R, t, P1, P2):
    """(..., n) squared distances of the correspondences (n, 3) to the models R (..., 3, 3), t (..., 3), longdouble."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = P1.astype(LD) - (np.einsum("...ik,nk->...ni", R, P2.astype(LD)) + t[..., None, :])
        return (e * e).sum(-1)


def _margin(d2, thr2):
    with np.errstate(invalid="ignore"):
        m = np.abs(d2 - thr2) / thr2
    return np.where(np.isfinite(d2), m, np.inf).astype(np.float64)


def pair_hypotheses(P1, P2, j, n_hyp, seed, thr, min_cross):
    """The hypothesis stage of one pair: counts (n_hyp,) int32 with -1 for a degenerate sample, and per hypothesis the
    longdouble model, kappa, the smallest threshold margin, the cross margin; plus the f64 ratio of the samples."""
    n = len(P1)
    out = dict(n=n, hyp_count=np.full(n_hyp, -1, dtype=np.int32))
    if n < 3:
        return out
    idx = samples(seed, j, n_hyp, n)
    S1, S2 = P1[idx], P2[idx]  # (n_hyp, 3, 3)
    fin = np.isfinite(S1).all((1, 2)) & np.isfinite(S2).all((1, 2))
    mc2 = LD(min_cross * min_cross)
    with np.errstate(invalid="ignore", over="ignore"):
        cr1, cr2 = _cross2(S1.astype(LD)), _cross2(S2.astype(LD))
    good = fin.copy()
    good[fin] = (cr1[fin] > mc2) & (cr2[fin] > mc2)
    cross_margin = np.full(n_hyp, np.inf)
    cross_margin[fin] = np.minimum(np.abs(cr1[fin] - mc2), np.abs(cr2[fin] - mc2)).astype(np.float64) / float(mc2)
    out.update(idx=idx, good=good, cross_margin=cross_margin,
               cross_min=float(np.sqrt(np.minimum(cr1[good], cr2[good]).min())) if good.any() else np.inf)
    margin = np.full(n_hyp, np.inf)
    kappa = np.full(n_hyp, np.nan)
    R = np.zeros((n_hyp, 3, 3), dtype=LD)
    t = np.zeros((n_hyp, 3), dtype=LD)
    if good.any():
        Rg, tg, kg, _ = arun_ref(S1[good], S2[good])
        R[good], t[good], kappa[good] = Rg, tg, kg
        thr2 = LD(thr * thr)
        d2 = _dist2(Rg, tg, P1, P2)
        with np.errstate(invalid="ignore"):
            out["hyp_count"][good] = (d2 < thr2).sum(-1).astype(np.int32)
        margin[good] = _margin(d2, thr2).min(-1)
        # the f64 restatement of the same samples against the longdouble fit, in units of kappa eps max|p|
        pose64, off = fit64_samples(S1[good], S2[good])
        finite = np.isfinite(P1).all(1) & np.isfinite(P2).all(1)
        pmax = float(max(np.abs(P1[finite]).max(), np.abs(P2[finite]).max()))
        a64 = np.einsum("hik,nk->hni", quat_R(pose64[:, :4]), P2[finite]) + pose64[:, None, 4:]
        aref = np.einsum("hik,nk->hni", Rg, P2[finite].astype(LD)) + tg[:, None, :]
        err = np.abs(a64 - aref).max((1, 2)).astype(np.float64)
        out.update(f64_ratio=float((err / (kg * EPS64 * pmax)).max()), jacobi_off=float(off.max()), pose64=pose64)
    out.update(R=R, t=t, kappa=kappa, margin=margin)
    return out


def pair_finish(P1, P2, hyp, refit, thr, probability):
    """Selection, refit rounds and outputs of one pair from its hypothesis stage."""
    n = hyp["n"]
    res = dict(pose=IDENTITY.copy(), inlier=np.zeros(n, dtype=np.uint8), margin=np.inf, f64_ratio=0.0, kappa=np.nan,
               ties=0, rounds_taken=0)
    cnt = hyp["hyp_count"]
    if n < 3 or cnt.max() < 0:
        res["stats"] = np.array([TOO_FEW if n < 3 else NO_MODEL, n, 0, -1, 0 if n < 3 else int((cnt < 0).sum()), 0, 0, 0.0])
        return res
    best = int(np.argmax(cnt))  # the first among equals
    res["ties"] = int((cnt == cnt[best]).sum())
    thr2 = LD(thr * thr)
    R, t, kappa = hyp["R"][best], hyp["t"][best], float(hyp["kappa"][best])
    finite = np.isfinite(P1).all(1) & np.isfinite(P2).all(1)
    pmax = float(max(np.abs(P1[finite]).max(), np.abs(P2[finite]).max()))
    d2 = _dist2(R, t, P1, P2)
    with np.errstate(invalid="ignore"):
        cur = d2 < thr2
    m_sample = m_cur = int(cur.sum())
    assert m_sample == cnt[best]
    for _ in range(refit):
        if m_cur < 3:
            break
        Rn, tn, kn, _ = arun_ref(P1[cur], P2[cur])
        if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
            break
        d2n = _dist2(Rn, tn, P1, P2)
        res["margin"] = min(res["margin"], float(_margin(d2n, thr2).min()))
        pose64, _ = fit64_set(P1[cur], P2[cur])
        err = np.abs(act(pose64, P2[finite]) - (P2[finite].astype(LD) @ Rn.T + tn)).max()
        res["f64_ratio"] = max(res["f64_ratio"], float(err) / (float(kn) * EPS64 * pmax))
        with np.errstate(invalid="ignore"):
            new = d2n < thr2
        if int(new.sum()) < m_cur:
            break
        changed = bool((new != cur).any())
        R, t, kappa, d2, cur, m_cur = Rn, tn, float(kn), d2n, new, int(new.sum())
        res["rounds_taken"] += 1
        if not changed:
            break
    rms = float(np.sqrt(d2[cur].sum() / LD(m_cur))) if m_cur else 0.0
    w = m_sample / n
    w3 = w * w * w
    p = probability if probability > 0 else 0.999
    k_needed = math.inf if w3 <= 0.0 else 0.0 if w3 >= 1.0 else math.log(1.0 - p) / math.log(1.0 - w3)
    res.update(pose=np.concatenate([R_quat(R), t]), R=R, t=t, kappa=kappa, inlier=cur.astype(np.uint8), pmax=pmax,
               stats=np.array([OK, n, m_cur, best, int((cnt < 0).sum()), rms, m_sample, k_needed]))
    return res


def align(p1, p2, pair_begin=None, threshold=0.1, n_hypotheses=256, seed=0, refit=0, min_cross=0.0, probability=0.0,
          masks=True, counts=False, hyps=None):
    """``Solver.align`` on the longdouble reference: ``poses`` (P, 7) f64, ``stats`` (P, 8), ``inlier``, ``hyp_count``,
    and beside them ``pose_ld`` (the poses in longdouble), ``kappa`` (P,), ``pmax`` (P,), ``margin`` (the smallest
    threshold margin of any decision of the pair, refit rounds included), ``cross_margin``, ``ties``, ``f64_ratio``.
    ``hyps``: the pairs' hypothesis stages from an earlier call with the same inputs (``out["hyps"]``)."""
    P1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
    P2 = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
    begin = np.array([0, len(P1)]) if pair_begin is None else np.asarray(pair_begin, dtype=np.int64).reshape(-1)
    thr = threshold if threshold > 0 else 0.1
    mc = min_cross if min_cross > 0 else 1e-6
    nh = n_hypotheses if n_hypotheses > 0 else 256
    n_pairs = len(begin) - 1
    out = dict(poses=np.zeros((n_pairs, 7)), stats=np.zeros((n_pairs, STAT_N)), inlier=np.zeros(len(P1), dtype=np.uint8),
               hyp_count=np.zeros((n_pairs, nh), dtype=np.int32), pose_ld=np.zeros((n_pairs, 7), dtype=LD),
               kappa=np.full(n_pairs, np.nan), pmax=np.zeros(n_pairs), margin=np.full(n_pairs, np.inf),
               cross_margin=np.full(n_pairs, np.inf), ties=np.zeros(n_pairs, dtype=np.int64),
               f64_ratio=np.zeros(n_pairs), safety=np.full(n_pairs, np.inf), cross_min=np.full(n_pairs, np.inf),
               jacobi_off=np.zeros(n_pairs), hyps=[])
    for j in range(n_pairs):
        a, b = P1[begin[j]:begin[j + 1]], P2[begin[j]:begin[j + 1]]
        hyp = hyps[j] if hyps is not None else pair_hypotheses(a, b, j, nh, seed, thr, mc)
        fin = pair_finish(a, b, hyp, refit, thr, probability)
        out["hyps"].append(hyp)
        out["hyp_count"][j] = hyp["hyp_count"]
        out["poses"][j] = fin["pose"].astype(np.float64)
        out["pose_ld"][j] = fin["pose"]
        out["stats"][j] = fin["stats"]
        out["inlier"][begin[j]:begin[j + 1]] = fin["inlier"]
        out["kappa"][j], out["ties"][j] = fin["kappa"], fin["ties"]
        out["pmax"][j] = fin.get("pmax", 0.0)
        out["margin"][j] = min(fin["margin"], float(hyp["margin"].min()) if "margin" in hyp else np.inf)
        out["f64_ratio"][j] = max(fin["f64_ratio"], hyp.get("f64_ratio", 0.0))
        if "margin" in hyp:
            out["cross_margin"][j] = float(hyp["cross_margin"].min())
            out["cross_min"][j] = hyp["cross_min"]
            out["jacobi_off"][j] = hyp.get("jacobi_off", 0.0)
            good = hyp["good"]
            if good.any():
                # each hypothesis's own margin over its own rounding bound 2 F kappa eps max|p| / thr
                fnt = np.isfinite(a).all(1) & np.isfinite(b).all(1)
                pm = float(max(np.abs(a[fnt]).max(), np.abs(b[fnt]).max()))
                out["safety"][j] = float((hyp["margin"][good] / (2 * POSE_F * hyp["kappa"][good] * EPS64 * pm / thr)).min())
    if not masks:
        out["inlier"] = None
    if not counts:
        out["hyp_count"] = None
    return out


# ------------------------------------------------------------------------------------------------ generators
def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_pair(n, outliers=0.3, seed=0, noise=0.01, kind="rigid", nan_rows=0):
    """(p1, p2, truth): p1 = R p2 + t + noise (1 cm) with a share of outliers placed uniformly in the room; ``truth``
    the pose (7,). kind "collinear": both clouds on a line, exactly rigid (every sample is degenerate). ``nan_rows``:
    that many rows of p1 made NaN and one of p2 made inf."""
    rng = np.random.default_rng([seed, n, 7])
    lo, hi = np.array([-2.0, -1.5, 1.0]), np.array([2.0, 1.5, 5.0])
    R = _rodrigues(rng.normal(0, 0.3, 3))
    t = rng.normal(0, 0.5, 3)
    if kind == "collinear":
        p2 = lo + np.linspace(0.05, 0.95, n)[:, None] * (hi - lo)
        p1 = p2 @ R.T + t
    else:
        p2 = rng.uniform(lo, hi, (n, 3))
        p1 = p2 @ R.T + t + rng.normal(0, noise, (n, 3))
        k = int(round(outliers * n))
        if k:
            rows = rng.choice(n, k, replace=False)
            p1[rows] = rng.uniform(lo, hi, (k, 3)) @ R.T + t
    if nan_rows:
        rows = rng.choice(n, nan_rows + 1, replace=False)
        p1[rows[:-1]] = np.nan
        p2[rows[-1], 1] = np.inf
    return p1, p2, np.concatenate([R_quat(R), t])


def make_batch(specs, seed=0):
    """(p1, p2, pair_begin) of the pairs ``specs``: dicts of make_pair's arguments."""
    p1, p2, begin = [], [], [0]
    for k, s in enumerate(specs):
        a, b, _ = make_pair(seed=seed + 31 * k, **s) if s["n"] else (np.zeros((0, 3)), np.zeros((0, 3)), None)
        p1.append(a)
        p2.append(b)
        begin.append(begin[-1] + len(a))
    return np.concatenate(p1), np.concatenate(p2), np.array(begin, dtype=np.int32)


REFITS = (0, 1, 3)
# pair sizes at the kernels' boundaries: the minimum, the wave, the LDS tile
SIZES = (3, 4, 63, 64, 65, ALIGN_TILE - 1, ALIGN_TILE, ALIGN_TILE + 1, 2 * ALIGN_TILE + 1)
# hypothesis counts at the wave's and the workgroup's boundaries
HYPS = (1, 63, 64, 65, 255, 256, 257, 513)
_MIXED17 = [dict(n=200, outliers=0.4), dict(n=0), dict(n=64, outliers=0.3), dict(n=2), dict(n=40, kind="collinear"),
            dict(n=120, outliers=0.5, nan_rows=5), dict(n=3, outliers=0.0), dict(n=257, outliers=0.3), dict(n=65, outliers=0.6),
            dict(n=1, outliers=0.0), dict(n=100, outliers=0.0), dict(n=63, outliers=0.3), dict(n=256, outliers=0.5),
            dict(n=30, outliers=0.3), dict(n=0), dict(n=513, outliers=0.4), dict(n=90, outliers=0.2, nan_rows=2)]
# name -> (pair specs, n_hypotheses, seed[, align's further arguments])
CASES = {}
for _n in SIZES:
    CASES[f"n-{_n}"] = ([dict(n=_n, outliers=0.3 if _n >= 10 else 0.0)], 256, 11)
for _h in HYPS:
    CASES[f"hyp-{_h}"] = ([dict(n=200, outliers=0.4)], _h, 5)
CASES["n-1000"] = ([dict(n=1000, outliers=0.5)], 256, 3)
CASES["batch-1"] = ([dict(n=150, outliers=0.5, nan_rows=3)], 64, 2)
CASES["batch-2"] = ([dict(n=40, kind="collinear"), dict(n=130, outliers=0.3)], 128, 9)
CASES["batch-17"] = (_MIXED17, 96, 4)
# a threshold of three sigma of the noise: the refit rounds change the inlier set
CASES["tight-200"] = ([dict(n=200, outliers=0.3)], 256, 7, dict(threshold=0.03))
CASES["tight-batch"] = ([dict(n=300, outliers=0.4), dict(n=80, outliers=0.2)], 128, 8, dict(threshold=0.025))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    specs, n_hyp, seed = CASES[name][:3]
    p1, p2, begin = make_batch(specs, seed=seed)
    for a in (p1, p2, begin):
        a.setflags(write=False)
    return p1, p2, begin, n_hyp, seed, (CASES[name][3] if len(CASES[name]) > 3 else {})


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """{refit: align(...)} of a case, the hypothesis stage computed once; shared and left unchanged by the tests."""
    p1, p2, begin, n_hyp, seed, kw = case_inputs(name)
    out, hyps = {}, None
    for refit in REFITS:
        out[refit] = align(p1, p2, begin, n_hypotheses=n_hyp, seed=seed, refit=refit, counts=True, hyps=hyps, **kw)
        hyps = out[refit]["hyps"]
    return out
