"""Two independent high-precision references of one Levenberg-Marquardt step (test infrastructure).

Both start from the oracle's per-observation residuals and Jacobians (``oracle.linearize``, pinned by finite
differences in test_oracle.py) and restate, in ``np.longdouble``, what Ceres' TrustRegionMinimizer +
LevenbergMarquardtStrategy solve for the first step of a window:

    scale = 1 / (1 + sqrt(colnorm^2))                          (Jacobi scaling; 1 when jacobi_scaling = 0)
    D^2   = clip(colnorm^2 * scale^2, min_lm_diagonal, max_lm_diagonal) / radius
    y     = argmin |J scale y + f|^2 + |D y|^2,   delta = scale * y

over the admissible observations (depth > 1e-15), the IntrinsicsPrior rows (J = -sqrt(w) I, f = sqrt(w) (prior - K)),
without the gauge camera's columns and without cameras / points that have no admissible observation.

* ``qr_step``    the stacked least-squares problem [J s; D] y = -[f; 0] by dense QR, then three steps of the
                 augmented-system refinement (Bjorck) with the residuals in extended precision. No Schur complement,
                 no normal equations. Dense: windows up to about 25 cameras.
* ``schur_step`` the points eliminated one by one in extended precision (3x3 inverse from f64, Newton-corrected),
                 the reduced system solved by f64 Cholesky + extended-precision refinement, back-substitution.
                 Also returns cond_2 of the scaled, damped reduced matrix. ``schur_reduce`` is its elimination alone:
                 the reduced system in extended precision (refschur.schur_system rounds it to f64).

Both return ``Step(ac_cam, delta_cam, delta_intr, delta_pts, model_cost_change, cond)``: the active cameras in
increasing order, the parameter-space step of each (nac, 6), of the intrinsics (4,) and of every point in the caller's
order (n_points, 3; zero for a point without an admissible observation), and the model cost change
-sum_i (J_i delta)^T (f_i + J_i delta / 2), prior rows included (``cond`` is None for ``qr_step``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from oracle import oracle

LD = np.longdouble
# x86-64 extended precision (64-bit mantissa); the references' residuals need it
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not extended precision on this machine"
EPS64 = float(np.finfo(np.float64).eps)


class Step(NamedTuple):
    ac_cam: np.ndarray
    delta_cam: np.ndarray
    delta_intr: np.ndarray
    delta_pts: np.ndarray
    model_cost_change: float
    cond: Optional[float]


class _Lin:
    """The scaled Jacobian blocks of a window, in extended precision."""

    def __init__(self, prob, opts, radius):
        opts = opts or oracle.default_options()
        lin = oracle.linearize(prob, opts)
        assert lin["rc"] == 0, "oracle.linearize failed"
        radius = LD(radius if radius > 0 else opts.initial_trust_region_radius)
        adm = np.nonzero(prob.obs_depth > 1e-15)[0]
        cam, pt = prob.obs_cam[adm].astype(np.int64), prob.obs_pt[adm].astype(np.int64)
        cam_has = np.zeros(prob.n_cams, bool)
        cam_has[cam] = True
        if 0 <= prob.fixed_cam < prob.n_cams:
            cam_has[prob.fixed_cam] = False
        self.ac_cam = np.nonzero(cam_has)[0].astype(np.int32)
        cam_ac = np.full(prob.n_cams, -1, np.int64)
        cam_ac[self.ac_cam] = np.arange(len(self.ac_cam))
        self.pt_idx = np.unique(pt)
        pt_ap = np.full(prob.n_points, -1, np.int64)
        pt_ap[self.pt_idx] = np.arange(len(self.pt_idx))
        self.n_points = prob.n_points
        self.nac, self.nap, self.no = len(self.ac_cam), len(self.pt_idx), len(adm)
        self.ac, self.ap = cam_ac[cam], pt_ap[pt]
        self.on = self.ac >= 0  # observations of an active camera
        self.acz = np.where(self.on, self.ac, 0)
        self.f = lin["res"][adm].astype(LD)
        jc = lin["jcam"][adm].astype(LD) * self.on[:, None, None]
        jp = lin["jpt"][adm].astype(LD)
        jk = np.zeros((self.no, 3, 4), LD)
        jk[:, :2] = lin["jint"][adm]
        sw_k = np.sqrt(LD(opts.weight_intrinsics))
        self.fk = sw_k * (prob.intr_prior.astype(LD) - prob.intr.astype(LD))
        # squared column norms -> Jacobi scale and LM diagonal
        cn_c = np.zeros((self.nac, 6), LD)
        np.add.at(cn_c, self.acz, (jc * jc).sum(1))
        cn_p = np.zeros((self.nap, 3), LD)
        np.add.at(cn_p, self.ap, (jp * jp).sum(1))
        cn_k = (jk * jk).sum((0, 1)) + sw_k * sw_k
        one = LD(1)

        def scale_diag(cn):
            s = one / (one + np.sqrt(cn)) if opts.jacobi_scaling else np.ones_like(cn)
            d2 = np.clip(cn * s * s, LD(opts.min_lm_diagonal), LD(opts.max_lm_diagonal)) / radius
            return s, d2

        self.s_c, self.d2_c = scale_diag(cn_c)
        self.s_p, self.d2_p = scale_diag(cn_p)
        self.s_k, self.d2_k = scale_diag(cn_k)
        # unscaled (model cost change) and scaled blocks
        self.jc, self.jp, self.jk = jc, jp, jk
        self.Jc = jc * self.s_c[self.acz][:, None, :]
        self.Jp = jp * self.s_p[self.ap][:, None, :]
        self.Jk = jk * self.s_k[None, None, :]
        self.Pk = -sw_k * self.s_k  # the prior rows' diagonal
        self.sw_k = sw_k
        self.n = 6 * self.nac + 3 * self.nap + 4
        self.o_p, self.o_k = 6 * self.nac, 6 * self.nac + 3 * self.nap

    def split(self, y):
        return y[: self.o_p].reshape(self.nac, 6), y[self.o_p: self.o_k].reshape(self.nap, 3), y[self.o_k:]

    def finish(self, y, cond=None) -> Step:
        yc, yp, yk = self.split(y)
        dc, dp, dk = yc * self.s_c, yp * self.s_p, yk * self.s_k
        # model cost change with the unscaled Jacobians
        dcz = dc[self.acz] if self.nac else np.zeros((self.no, 6), LD)
        jd = (np.einsum("ord,od->or", self.jc, dcz) + np.einsum("ori,oi->or", self.jp, dp[self.ap])
              + np.einsum("ork,k->or", self.jk, dk))
        mcc = -(jd * (self.f + jd / 2)).sum()
        jdk = -self.sw_k * dk
        mcc += -(jdk * (self.fk + jdk / 2)).sum()
        pts = np.zeros((self.n_points, 3))
        pts[self.pt_idx] = dp.astype(np.float64)
        return Step(self.ac_cam, dc.astype(np.float64), dk.astype(np.float64), pts, float(mcc), cond)


def qr_step(prob, opts=None, radius: float = 0.0) -> Step:
    L = _Lin(prob, opts, radius)
    n, no = L.n, L.no
    m = 3 * no + 4 + n
    d = np.sqrt(np.concatenate([L.d2_c.ravel(), L.d2_p.ravel(), L.d2_k]))

    def A_mul(y):  # [J s; prior; D] y, extended precision, block by block
        yc, yp, yk = L.split(y)
        ycz = yc[L.acz] if L.nac else np.zeros((no, 6), LD)
        r = (np.einsum("ord,od->or", L.Jc, ycz) + np.einsum("ori,oi->or", L.Jp, yp[L.ap])
             + np.einsum("ork,k->or", L.Jk, yk))
        return np.concatenate([r.ravel(), L.Pk * yk, d * y])

    def At_mul(r):
        ro = r[: 3 * no].reshape(no, 3)
        gc = np.zeros((L.nac, 6), LD)
        np.add.at(gc, L.acz, np.einsum("ord,or->od", L.Jc, ro))
        gp = np.zeros((L.nap, 3), LD)
        np.add.at(gp, L.ap, np.einsum("ori,or->oi", L.Jp, ro))
        gk = np.einsum("ork,or->k", L.Jk, ro) + L.Pk * r[3 * no: 3 * no + 4]
        return np.concatenate([gc.ravel(), gp.ravel(), gk]) + d * r[3 * no + 4:]

    A = np.zeros((m, n))
    rows = 3 * np.arange(no)[:, None] + np.arange(3)[None, :]  # (no, 3)
    for k in range(6):
        A[rows, (6 * L.acz + k)[:, None]] += L.Jc[:, :, k].astype(np.float64)  # (zero for the gauge's observations)
    for k in range(3):
        A[rows, (L.o_p + 3 * L.ap + k)[:, None]] = L.Jp[:, :, k].astype(np.float64)
    for k in range(4):
        A[rows, L.o_k + k] = L.Jk[:, :, k].astype(np.float64)
    A[3 * no + np.arange(4), L.o_k + np.arange(4)] = L.Pk.astype(np.float64)
    A[3 * no + 4 + np.arange(n), np.arange(n)] = d.astype(np.float64)
    b = np.concatenate([-L.f.ravel(), -L.fk, np.zeros(n, LD)])
    Q, R = np.linalg.qr(A, mode="reduced")
    y = np.linalg.solve(R, Q.T @ b.astype(np.float64)).astype(LD)
    r = b - A_mul(y)
    for _ in range(3):  # [I A; A^T 0] [dr; dy] = [b - r - A y; -A^T r], residuals in extended precision
        f1 = (b - r - A_mul(y)).astype(np.float64)
        g1 = (-At_mul(r)).astype(np.float64)
        h = np.linalg.solve(R.T, g1)
        dy = np.linalg.solve(R, Q.T @ f1 - h).astype(LD)
        r = r + (f1.astype(LD) - A_mul(dy))
        y = y + dy
    return L.finish(y)


def _inv3(V):
    """3x3 inverse: f64, then two Newton corrections in extended precision."""
    X = np.linalg.inv(V.astype(np.float64)).astype(LD)
    I = np.eye(3, dtype=LD)
    for _ in range(2):
        X = X + X @ (I - V @ X)
    return X


def schur_reduce(L):
    """The scaled, damped reduced system of ``L`` in extended precision — active cameras in increasing order, six
    rows each, then the four intrinsics: (S, rhs, per active point (columns, [W_p; K_p], V_p^-1, g_p))."""
    nac, nr = L.nac, 6 * L.nac + 4
    kb = 6 * nac
    S = np.zeros((nr, nr), LD)
    rhs = np.zeros(nr, LD)
    # camera / intrinsics blocks, gradient
    Ucc = np.einsum("ora,orb->oab", L.Jc, L.Jc)
    Cck = np.einsum("ora,ork->oak", L.Jc, L.Jk)
    gc = np.einsum("ora,or->oa", L.Jc, L.f)
    for o in np.nonzero(L.on)[0]:
        c0 = 6 * L.ac[o]
        S[c0: c0 + 6, c0: c0 + 6] += Ucc[o]
        S[c0: c0 + 6, kb:] += Cck[o]
        S[kb:, c0: c0 + 6] += Cck[o].T
        rhs[c0: c0 + 6] -= gc[o]
    S[kb:, kb:] += np.einsum("ora,orb->ab", L.Jk, L.Jk) + np.diag(L.Pk * L.Pk)
    rhs[kb:] -= np.einsum("ork,or->k", L.Jk, L.f) + L.Pk * L.fk
    S[np.arange(nr), np.arange(nr)] += np.concatenate([L.d2_c.ravel(), L.d2_k])
    # the points, one by one
    Vo = np.einsum("ora,orb->oab", L.Jp, L.Jp)
    Wo = np.einsum("ora,ori->oai", L.Jc, L.Jp)  # 6x3
    Ko = np.einsum("ork,ori->oki", L.Jk, L.Jp)  # 4x3
    gpo = np.einsum("ori,or->oi", L.Jp, L.f)
    order = np.argsort(L.ap, kind="stable")
    bounds = np.searchsorted(L.ap[order], np.arange(L.nap + 1))
    keep = []
    for p in range(L.nap):
        obs = order[bounds[p]: bounds[p + 1]]
        V = Vo[obs].sum(0) + np.diag(L.d2_p[p])
        Vi = _inv3(V)
        gp = gpo[obs].sum(0)
        cams = np.unique(L.ac[obs][L.on[obs]])
        E = np.zeros((6 * len(cams) + 4, 3), LD)  # [W_p; K_p]
        for o in obs[L.on[obs]]:
            j = 6 * int(np.searchsorted(cams, L.ac[o]))
            E[j: j + 6] += Wo[o]
        E[6 * len(cams):] = Ko[obs].sum(0)
        cols = np.concatenate([(6 * cams[:, None] + np.arange(6)[None, :]).ravel(), kb + np.arange(4)])
        T = E @ Vi
        S[np.ix_(cols, cols)] -= T @ E.T
        rhs[cols] += T @ gp
        keep.append((cols, E, Vi, gp))
    return S, rhs, keep


def schur_step(prob, opts=None, radius: float = 0.0) -> Step:
    L = _Lin(prob, opts, radius)
    kb = 6 * L.nac
    S, rhs, keep = schur_reduce(L)
    S64 = S.astype(np.float64)
    S64 = (S64 + S64.T) / 2
    C = np.linalg.cholesky(S64)

    def solve(v):
        return np.linalg.solve(C.T, np.linalg.solve(C, v.astype(np.float64))).astype(LD)

    y = solve(rhs)
    for _ in range(3):
        y = y + solve(rhs - S @ y)
    yp = np.zeros((L.nap, 3), LD)
    for p, (cols, E, Vi, gp) in enumerate(keep):
        yp[p] = Vi @ (-gp - E.T @ y[cols])
    full = np.concatenate([y[:kb], yp.ravel(), y[kb:]])
    return L.finish(full, float(np.linalg.cond(S64)))


def rel_err(got, ref) -> dict:
    """Max-norm error over the max-norm of the reference, per group (cameras, intrinsics, points); ``got`` and
    ``ref`` are Steps or dicts with ac_cam / delta_cam / delta_intr / delta_pts."""
    g = got._asdict() if isinstance(got, tuple) else got
    r = ref._asdict() if isinstance(ref, tuple) else ref
    assert np.array_equal(np.asarray(g["ac_cam"]), np.asarray(r["ac_cam"])), "active cameras differ"
    out = {}
    for name, key in (("cams", "delta_cam"), ("intr", "delta_intr"), ("pts", "delta_pts")):
        a, b = np.asarray(g[key], dtype=np.float64), np.asarray(r[key], dtype=np.float64)
        assert a.shape == b.shape, (key, a.shape, b.shape)
        den = float(np.abs(b).max()) if b.size else 0.0
        out[name] = float(np.abs(a - b).max()) / den if den > 0 else 0.0
    return out


def step_tol(cond: float) -> float:
    """Forward-error bound of a backward-stable solve of the reduced system: 8 cond(S) eps_f64 (the factor 8 for a
    different summation order and f64 atomics)."""
    return 8.0 * cond * EPS64


# ------------------------------------------------------------------------------------------------ the windows
# The windows of the step tests (test_refstep.py checks the references and the oracle on every one of them,
# test_gpu_step.py runs the GPU paths on them): synthetic.make_problem, 12 points per camera, each the smallest
# that reaches its edge. Active cameras = cameras - 1 (the gauge) unless noted.
def _w(n_cams, tracks, seed, **kw):
    return dict(n_cams=n_cams, n_points=12 * n_cams, obs_per_point=tracks, seed=seed, **kw)


BCR_COUNTS = (11, 19, 20, 21, 30, 31, 41, 79, 80, 81)  # a BCR block is 10 active cameras
ONE_BLOCK_COUNTS = (1, 2, 9, 10)
# (active cameras, band) of the one-workgroup band solve, whose system must fit 160 KB of LDS: band 3 up to 51 active
# cameras, band 2 up to about 70, band 1 up to about 115
NARROW = ((2, 1), (9, 2), (10, 3), (17, 3), (37, 2), (49, 1), (49, 3), (51, 3), (64, 2), (99, 1))
NARROW_TRACKS = {1: 2, 2: (2, 3), 3: (2, 4)}
BANDCHOL_TRACKS = (2, 4, 7, 10, 13, 16)  # band widths of 1 .. 6 tiles: every k_chol_band<BW>
MESSY = dict(dup_frac=0.05, bad_depth_frac=0.05, shuffle_obs=True)

WINDOWS = {}
for _n in BCR_COUNTS:
    WINDOWS[f"bcr{_n}"] = _w(_n + 1, (4, 9), 200 + _n)
WINDOWS["full31"] = _w(32, 10, 301)  # tracks of exactly 10 cameras: camera band 9, every off-diagonal block dense
WINDOWS["gauge_mid21"] = _w(22, (4, 9), 311, fixed_cam=11)
WINDOWS["gauge_last21"] = _w(22, (4, 9), 312, fixed_cam=21)
WINDOWS["inactive_mid21"] = _w(23, (4, 9), 313)  # camera 12's depths zeroed below: 21 active cameras
for _n in ONE_BLOCK_COUNTS:
    WINDOWS[f"one{_n}"] = _w(_n + 1, (2, 4), 320 + _n)
for _n, _b in NARROW:
    WINDOWS[f"nb{_n}_b{_b}"] = _w(_n + 1, NARROW_TRACKS[_b], 400 + _n + _b)
for _l in BANDCHOL_TRACKS:
    WINDOWS[f"bc_L{_l}"] = _w(34, _l, 500 + _l)
WINDOWS["dense_wide30"] = dict(n_cams=30, n_points=150, obs_per_point=(6, 16), seed=5, rot_noise=0.005)  # n = 178
WINDOWS["dense_n160"] = _w(27, (6, 16), 601)  # n = 160, a multiple of 16
WINDOWS["bcr21_f32"] = _w(22, (4, 9), 221, sensor_f32=True)
WINDOWS["nb37_b2_f32"] = _w(38, (2, 3), 439, sensor_f32=True)
WINDOWS["bcr21_messy"] = _w(22, (4, 9), 701, **MESSY)
WINDOWS["nb37_b2_messy"] = _w(38, (2, 3), 702, **MESSY)
# radii beside the default 1e4
EXTRA_RADII = {"bcr21": (1e12, 1e-2), "bcr81": (1e12, 1e-2)}

_cache = {}


def window(name):
    """The window ``name`` (cached; callers must not modify it)."""
    if ("w", name) not in _cache:
        from miba import synthetic
        p = synthetic.make_problem(**WINDOWS[name])
        if name == "inactive_mid21":
            p.obs_depth[p.obs_cam == 12] = 0.0
        _cache[("w", name)] = p
    return _cache[("w", name)]


NO_TOL = dict(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)


def reference(name, radius=1e4):
    """(window, schur_step, oracle.lm_step, the oracle's own accept decision) of ``name`` at ``radius``, cached."""
    key = ("r", name, float(radius))
    if key not in _cache:
        p = window(name)
        ref = schur_step(p, None, radius)
        orc = oracle.lm_step(p, None, radius)
        _, tr = oracle.solve_trace(p.copy(), oracle.default_options(max_num_iterations=1,
                                                                    initial_trust_region_radius=radius, **NO_TOL))
        _cache[key] = (p, ref, orc, int(tr[1][6]))
    return _cache[key]


def all_references():
    return [(n, r) for n in WINDOWS for r in (1e4,) + EXTRA_RADII.get(n, ())]


def first_covisible(prob):
    """(active cameras, fc): fc[a] = the lowest active index among the cameras that share a point with active
    camera a through admissible observations (the reduced system's envelope)."""
    adm = prob.obs_depth > 1e-15
    cam, pt = prob.obs_cam[adm].astype(np.int64), prob.obs_pt[adm].astype(np.int64)
    has = np.zeros(prob.n_cams, bool)
    has[cam] = True
    if 0 <= prob.fixed_cam < prob.n_cams:
        has[prob.fixed_cam] = False
    ac_cam = np.nonzero(has)[0]
    cam_ac = np.full(prob.n_cams, -1, np.int64)
    cam_ac[ac_cam] = np.arange(len(ac_cam))
    ac = cam_ac[cam]
    lo = np.full(prob.n_points, len(ac_cam), np.int64)
    np.minimum.at(lo, pt[ac >= 0], ac[ac >= 0])
    fc = np.arange(len(ac_cam))
    np.minimum.at(fc, ac[ac >= 0], lo[pt[ac >= 0]])
    return ac_cam, fc


def camera_band(prob) -> int:
    _, fc = first_covisible(prob)
    return int((np.arange(len(fc)) - fc).max()) if len(fc) else 0


def band_tiles(prob) -> int:
    """16x16 tiles below the diagonal inside the camera band of the reduced system (its last block row, the
    intrinsics border, apart): the banded Cholesky runs for 1..6."""
    _, fc = first_covisible(prob)
    n = 6 * len(fc) + 4
    npad = (n + 15) // 16 * 16
    r = np.arange(npad)
    first = np.where(r < 6 * len(fc), 6 * fc[np.minimum(r // 6, len(fc) - 1)], 0) // 16
    fcol = np.array([first[16 * i: 16 * i + 16].min() for i in range(npad // 16)])
    return int(max([i - fcol[i] for i in range(npad // 16 - 1)], default=0))
