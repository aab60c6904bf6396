"""Extended-precision references of the second half of an LM iteration (test infrastructure): the retraction
x [+] delta, the cost of a parameter set, the ambient norms, the gradient max-norm, and first-order rounding bounds for
each. Everything is ``np.longdouble`` (x86-64 extended precision, as refstep.py) from the raw parameters; only the
gradient uses the oracle's per-observation Jacobians (``oracle.linearize``, pinned by finite differences in
test_oracle.py), accumulated in extended precision.

Poses are (qx qy qz qw tx ty tz), camera-to-world; delta = [upsilon, omega]; the retraction is Sophus' T exp(delta):

    q' = q (x) (omega sin(theta/2)/theta, cos(theta/2)),   t' = t + R(q) V upsilon,
    V  = I + a [omega]x + b [omega]x^2,   a = (1 - cos theta)/theta^2,   b = (theta - sin theta)/theta^3.

Two independent statements of it:

* ``retract_quat``  the quaternion product with the half-angle pair, V upsilon by cross products with
                    a = 2 sin^2(theta/2)/theta^2, the translation rotated by the quaternion sandwich;
* ``retract_mat``   R(q) Exp(omega) by Rodrigues' formula and V as 3x3 matrices, a = sin^2 theta / (theta^2 (1 + cos
                    theta)) while cos theta > 0 and (1 - cos theta)/theta^2 beyond.

Each uses the Taylor series (four terms) only below theta^2 = 1e-8, where the next term is below 1e-30. They are
compared as (R, t) (test_refcand.py), so the quaternion's sign does not matter.

Bounds (eps = 2^-52), each also asserted for the oracle's own f64 result wherever it is asserted for the GPU:

* retraction: 16 eps absolute per quaternion component, 16 eps max(1, |t|_inf, |upsilon|) per translation component
  (about a dozen roundings along the product / the rotated V upsilon; series truncation <= 3e-17 included). The
  oracle restates Sophus' V with a = (1 - cos theta)/theta^2 literally, whose cancellation costs eps/theta^2 in a,
  that is eps |upsilon| / theta in the translation: ``retraction_bound(..., cancelling_a=True)`` adds 2 eps |upsilon| /
  theta for it (zero-sized next to the rest for an LM step, where |upsilon| ~ theta). The device computes a from the
  half-angle pair / a series and is held to the bound without that term. Below theta = 1e-10 Sophus' small-angle
  branch takes V = exp(omega) (I + [omega]x + ...) where V = I + [omega]x / 2 + ...: a truncation of theta |upsilon| / 2
  + theta^2 |upsilon| / 3 that the oracle and the device both restate; the bound carries 0.51 theta |upsilon| for it
  (<= 5e-11 |upsilon|; below 1e-20 for an LM step small enough to take that branch).
* cost: ``cost_bound``: tol = 16 eps A + N_terms eps cost, A = sum_obs rho'_r sw_r^2 (|u - u_o| (|u| + |u_o|) + |v - v_o|
  (|v| + |v_o|)) + rho'_d sw_d^2 |d - z| (|d| + |z|), plus sw_k^2 |prior - K| (|prior| + |K|): d(rho/2) = rho' sw^2
  |r| d|r| with the pixel / depth known to 16 eps of its operands (rotate, divide, intrinsics), and N_terms eps for
  a sum of N_terms non-negative terms in any order.
* norms: (N_terms + 16) eps relative.
* gradient max-norm: 8 eps max_j sum_i |J_ij| |f_i| + the retraction bound.
"""
from __future__ import annotations

import numpy as np

import refstep
from oracle import oracle
from refstep import EPS64, LD, NO_TOL

_0, _1, _2 = LD(0), LD(1), LD(2)
SERIES_BELOW = LD(1e-8)  # theta^2


def _ld(a):
    return np.asarray(a, dtype=LD)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=LD)


def _series(t2, c):
    """c0 - c1 t2 + c2 t2^2 - c3 t2^3 with c = reciprocals' denominators."""
    return _1 / c[0] - t2 / c[1] + t2 * t2 / c[2] - t2 * t2 * t2 / c[3]


def quat_R(q):
    """Rotation matrix of the unit quaternion (x y z w)."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)


def _unit(q):
    return q / np.sqrt((q * q).sum())


def retract_quat(T, d):
    """T exp(d) in quaternion form; returns (q' normalised (x y z w), t')."""
    T, d = _ld(T), _ld(d)
    q, t, ups, om = _unit(T[:4]), T[4:], d[:3], d[3:]
    t2 = (om * om).sum()
    th = np.sqrt(t2)
    if t2 < SERIES_BELOW:
        imag = _series(t2, (2, 48, 3840, 645120))  # sin(theta/2)/theta
        real = _1 - t2 * _series(t2, (8, 384, 46080, 10321920))  # cos(theta/2)
        a = _series(t2, (2, 24, 720, 40320))
        b = _series(t2, (6, 120, 5040, 362880))
    else:
        sh, ch = np.sin(th / 2), np.cos(th / 2)
        imag, real = sh / th, ch
        a = 2 * sh * sh / t2
        b = (th - 2 * sh * ch) / (t2 * th)
    bx, by, bz, bw = imag * om[0], imag * om[1], imag * om[2], real
    qx, qy, qz, qw = q
    qn = np.array([qw * bx + qx * bw + qy * bz - qz * by,
                   qw * by + qy * bw + qz * bx - qx * bz,
                   qw * bz + qz * bw + qx * by - qy * bx,
                   qw * bw - qx * bx - qy * by - qz * bz], dtype=LD)
    wu = _cross(om, ups)
    vu = ups + a * wu + b * _cross(om, wu)
    qv = q[:3]
    uv = 2 * _cross(qv, vu)
    return _unit(qn), t + vu + qw * uv + _cross(qv, uv)


def retract_mat(T, d):
    """T exp(d) in rotation-matrix form; returns (R', t')."""
    T, d = _ld(T), _ld(d)
    R, t, ups, om = quat_R(_unit(T[:4])), T[4:], d[:3], d[3:]
    t2 = (om * om).sum()
    th = np.sqrt(t2)
    if t2 < SERIES_BELOW:
        s = _series(t2, (1, 6, 120, 5040))  # sin(theta)/theta
        a = _series(t2, (2, 24, 720, 40320))
        b = _series(t2, (6, 120, 5040, 362880))
    else:
        st, ct = np.sin(th), np.cos(th)
        s = st / th
        a = st * st / (t2 * (1 + ct)) if ct > 0 else (1 - ct) / t2
        b = (th - st) / (t2 * th)
    Om = np.array([[_0, -om[2], om[1]], [om[2], _0, -om[0]], [-om[1], om[0], _0]], dtype=LD)
    Om2 = Om @ Om
    I = np.eye(3, dtype=LD)
    return R @ (I + s * Om + a * Om2), t + R @ ((I + a * Om + b * Om2) @ ups)


def retraction_bound(T, d, cancelling_a=False):
    """(per quaternion component, per translation component)."""
    T, d = np.asarray(T, dtype=np.float64), np.asarray(d, dtype=np.float64)
    nu = float(np.linalg.norm(d[:3]))
    bt = 16 * EPS64 * max(1.0, float(np.abs(T[4:]).max()), nu)
    th = float(np.linalg.norm(d[3:]))
    if th < 1e-10:
        bt += 0.51 * th * nu
    elif cancelling_a:
        bt += 2 * EPS64 * nu / th
    return 16 * EPS64, bt


def retraction_error(got, T, d):
    """(max quaternion error, max translation error) of the pose ``got`` against retract_quat(T, d)."""
    q, t = retract_quat(T, d)
    g = _ld(got)
    return float(np.abs(g[:4] - q).max()), float(np.abs(g[4:] - t).max())


# --------------------------------------------------------------------------------------------------- the blocks
def active_blocks(prob):
    """(admissible observation indices, active camera indices, active point mask)."""
    adm = np.nonzero(prob.obs_depth > 1e-15)[0]
    has = np.zeros(prob.n_cams, bool)
    has[prob.obs_cam[adm]] = True
    if 0 <= prob.fixed_cam < prob.n_cams:
        has[prob.fixed_cam] = False
    pt = np.zeros(prob.n_points, bool)
    pt[prob.obs_pt[adm]] = True
    return adm, np.nonzero(has)[0], pt


def candidate(prob, step):
    """x [+] delta: (cams (n_cams, 7), intr (4,), points (n_points, 3)) in extended precision; ``step`` as
    Solver.lm_step / refstep.Step (ac_cam, delta_cam, delta_intr, delta_pts)."""
    s = step._asdict() if isinstance(step, tuple) else step
    cams = _ld(prob.cams).copy()
    for t, cam in enumerate(np.asarray(s["ac_cam"])):
        q, tr = retract_quat(prob.cams[cam], s["delta_cam"][t])
        cams[cam, :4], cams[cam, 4:] = q, tr
    return cams, _ld(prob.intr) + _ld(s["delta_intr"]), _ld(prob.points) + _ld(s["delta_pts"])


def _opts(opts):
    if opts is None or isinstance(opts, dict):
        return oracle.default_options(**(opts or {}))
    return opts


def cost(prob, opts=None, cams=None, intr=None, points=None, detail=False):
    """1/2 rho_r + 1/2 rho_d over the admissible observations plus the intrinsics prior, from the raw parameters
    (``cams`` / ``intr`` / ``points`` replace the window's). With ``detail`` a dict: cost, A (cost_bound's sum),
    n_terms, and per admissible observation the raw block norms nr, nd and the projection u, v, z."""
    o = _opts(opts)
    adm, _, _ = active_blocks(prob)
    C = _ld(prob.cams if cams is None else cams)
    K = _ld(prob.intr if intr is None else intr)
    X = _ld(prob.points if points is None else points)
    N = LD(len(adm))
    swr2, swd2, swk2 = _1 / N, LD(o.weight_unpr) / N, LD(o.weight_intrinsics)
    ar, ad = LD(o.hub_p_repr), LD(o.hub_p_unpr)
    c, p = prob.obs_cam[adm], prob.obs_pt[adm]
    q = C[c, :4]
    q = q / np.sqrt((q * q).sum(1))[:, None]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    dW = X[p] - C[c, 4:]
    # p_C = R^T (p_W - t)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)  # (3, 3, n)
    pc = np.einsum("jin,nj->ni", R, dW)
    u = K[0] * pc[:, 0] / pc[:, 2] + K[2]
    v = K[1] * pc[:, 1] / pc[:, 2] + K[3]
    uo, vo, dep = _ld(prob.obs_uv[adm, 0]), _ld(prob.obs_uv[adm, 1]), _ld(prob.obs_depth[adm])
    du, dv, dz = u - uo, v - vo, dep - pc[:, 2]
    sr, sd = swr2 * (du * du + dv * dv), swd2 * dz * dz
    nr, nd = np.sqrt(sr), np.sqrt(sd)
    lin_r, lin_d = nr > ar, nd > ad  # Huber's linear zone: s > b = a^2
    rho_r = np.where(lin_r, 2 * ar * nr - ar * ar, sr)
    rho_d = np.where(lin_d, 2 * ad * nd - ad * ad, sd)
    pk = _ld(prob.intr_prior) - K
    total = (rho_r.sum() + rho_d.sum()) / 2 + swk2 * (pk * pk).sum() / 2
    if not detail:
        return total
    d1r = np.where(lin_r, ar / np.where(lin_r, nr, _1), _1)
    d1d = np.where(lin_d, ad / np.where(lin_d, nd, _1), _1)
    A = (d1r * swr2 * (np.abs(du) * (np.abs(u) + np.abs(uo)) + np.abs(dv) * (np.abs(v) + np.abs(vo)))).sum()
    A += (d1d * swd2 * np.abs(dz) * (np.abs(dep) + np.abs(pc[:, 2]))).sum()
    A += (swk2 * np.abs(pk) * (np.abs(_ld(prob.intr_prior)) + np.abs(K))).sum()
    return dict(cost=total, A=A, n_terms=2 * len(adm) + 4, nr=nr, nd=nd, lin_r=lin_r, lin_d=lin_d, u=u, v=v,
                z=pc[:, 2], adm=adm, sw_r=np.sqrt(swr2), sw_d=np.sqrt(swd2))


def cost_bound(prob, opts=None, cams=None, intr=None, points=None):
    """(cost, tol) with tol = 16 eps A + N_terms eps cost (module docstring)."""
    d = cost(prob, opts, cams, intr, points, detail=True)
    return d["cost"], float(16 * EPS64 * d["A"] + d["n_terms"] * EPS64 * d["cost"])


def norms(prob, cams_x, intr_x, pts_x, cams_c, intr_c, pts_c):
    """(|x - x_cand|^2, |x_cand|^2, |x|^2, relative bound) over the active blocks, ambient, from the given slots."""
    _, ac, pt = active_blocks(prob)
    a = np.concatenate([_ld(cams_x)[ac].ravel(), _ld(pts_x)[pt].ravel(), _ld(intr_x)])
    b = np.concatenate([_ld(cams_c)[ac].ravel(), _ld(pts_c)[pt].ravel(), _ld(intr_c)])
    return ((a - b) ** 2).sum(), (b * b).sum(), (a * a).sum(), (a.size + 16) * EPS64


def gradient_max_norm(prob, opts=None):
    """(|x - Plus(x, -g)|_inf, bound), g = J^T f accumulated in extended precision from the oracle's
    per-observation Jacobians, the IntrinsicsPrior rows included."""
    o = _opts(opts)
    lin = oracle.linearize(prob, o)
    assert lin["rc"] == 0
    adm, ac, _ = active_blocks(prob)
    f = _ld(lin["res"][adm])
    jc, jp = _ld(lin["jcam"][adm]), _ld(lin["jpt"][adm])
    jk = np.zeros((len(adm), 3, 4), LD)
    jk[:, :2] = lin["jint"][adm]
    c, p = prob.obs_cam[adm], prob.obs_pt[adm]
    gc, gca = np.zeros((prob.n_cams, 6), LD), np.zeros((prob.n_cams, 6), LD)
    np.add.at(gc, c, np.einsum("ord,or->od", jc, f))
    np.add.at(gca, c, np.einsum("ord,or->od", np.abs(jc), np.abs(f)))
    gp, gpa = np.zeros((prob.n_points, 3), LD), np.zeros((prob.n_points, 3), LD)
    np.add.at(gp, p, np.einsum("ori,or->oi", jp, f))
    np.add.at(gpa, p, np.einsum("ori,or->oi", np.abs(jp), np.abs(f)))
    swk = np.sqrt(LD(o.weight_intrinsics))
    fk = swk * (_ld(prob.intr_prior) - _ld(prob.intr))
    gk = np.einsum("ork,or->k", jk, f) - swk * fk
    gka = np.einsum("ork,or->k", np.abs(jk), np.abs(f)) + swk * np.abs(fk)
    m, bret = _0, 0.0
    for cam in ac:
        q, t = retract_quat(prob.cams[cam], -gc[cam])
        m = max(m, np.abs(_ld(prob.cams[cam, :4]) - q).max(), np.abs(_ld(prob.cams[cam, 4:]) - t).max())
        bret = max(bret, *retraction_bound(prob.cams[cam], -gc[cam].astype(np.float64), cancelling_a=True))
    m = max(m, np.abs(gp).max(), np.abs(gk).max())
    bound = 8 * EPS64 * float(max(gca[ac].max() if len(ac) else 0, gpa.max(), gka.max())) + bret
    return float(m), bound


# --------------------------------------------------------------------------------------------------- the windows
# name -> (base window of refstep.WINDOWS, what is changed). The rolled cameras' initial quaternions are
# right-multiplied by a roll about the optical axis (the camera frame's z: depths are unchanged), so the first step
# must turn them back: theta >= 1 for the 1.6 rad roll, 0.5 <= theta < 1 for the second.
ROLLS = {"roll21": ("bcr21", ((7, 1.6), (15, 1.45))), "roll_nb37": ("nb37_b2", ((9, 1.6), (25, 1.45)))}
HUBER = {"huber_mixed21": ("bcr21", False), "huber_edge21": ("bcr21", True),
         "huber_mixed_nb37": ("nb37_b2", False), "huber_edge_nb37": ("nb37_b2", True)}
# Huber thresholds = the median raw block norm at x, so both zones hold half the blocks there; at radius 1e4 the step
# removes most of the reprojection error and 98 % of the candidate's reprojection blocks are quadratic, so these
# windows step at radius 0.1, where the candidate keeps 39 % .. 43 % of them in the linear zone
HUBER_RADIUS = 0.1
SMALL_RADII = (1e-8, 1e-9)  # theta on both sides of Sophus' 1e-10 / every camera below it (bcr21, nb37_b2)
EDGE_REL = 4e-13  # the boundary blocks' distance from s = b, relative, as constructed (asserted <= 1e-12)
_cache = {}


def _huber_case(name):
    base, edge = HUBER[name]
    p = refstep.window(base).copy()
    d = cost(p, None, detail=True)
    a_r, a_d = float(np.median(d["nr"])), float(np.median(d["nd"]))
    info = {}
    if edge:
        # observations 3 / 4: the reprojection block just above / below s = b (the pixel from the extended-precision
        # projection), 5 / 6: the depth block likewise
        k = d["adm"]
        for j, sgn in ((3, +1), (4, -1)):
            p.obs_uv[k[j], 0] = float(d["u"][j] - LD(a_r) * (1 + sgn * LD(EDGE_REL)) / d["sw_r"])
            p.obs_uv[k[j], 1] = float(d["v"][j])
        for j, sgn in ((5, +1), (6, -1)):
            p.obs_depth[k[j]] = float(d["z"][j] + LD(a_d) * (1 + sgn * LD(EDGE_REL)) / d["sw_d"])
        info = dict(edge_r=(3, 4), edge_d=(5, 6))
    return p, dict(hub_p_repr=a_r, hub_p_unpr=a_d), info


def case(name):
    """(window, option overrides, info) of ``name``: a refstep window, a rolled one or a Huber one (cached; callers
    must not modify the window)."""
    if ("c", name) not in _cache:
        if name in ROLLS:
            base, rolls = ROLLS[name]
            p = refstep.window(base).copy()
            for cam, phi in rolls:
                assert cam != p.fixed_cam
                x, y, z, w = p.cams[cam, :4]
                s, c = np.sin(phi / 2), np.cos(phi / 2)
                q = np.array([x * c + y * s, y * c - x * s, w * s + z * c, w * c - z * s])
                p.cams[cam, :4] = q / np.linalg.norm(q)
            _cache[("c", name)] = (p, {}, dict(rolled=[c for c, _ in rolls]))
        elif name in HUBER:
            _cache[("c", name)] = _huber_case(name)
        else:
            _cache[("c", name)] = (refstep.window(name), {}, {})
    return _cache[("c", name)]


class Ref:
    """The references of one (window, radius): the extended-precision step and its candidate, costs and bounds, the
    oracle's step and candidate, and the oracle's one-iteration trace."""

    def __init__(self, name, radius):
        self.name, self.radius = name, radius
        self.prob, self.okw, self.info = case(name)
        p = self.prob
        if not self.okw and name in refstep.WINDOWS:
            _, self.step, self.orc, _ = refstep.reference(name, radius)
        else:
            o = oracle.default_options(**self.okw)
            self.step = refstep.schur_step(p, o, radius)
            self.orc = oracle.lm_step(p, o, radius)
        q = p.copy()
        self.summary, self.trace = oracle.solve_trace(q, oracle.default_options(
            max_num_iterations=1, initial_trust_region_radius=radius, **NO_TOL, **self.okw))
        self.orc_x = q  # the oracle's parameters after its iteration (the candidate when accepted)
        self.accepted = int(self.trace[1][6])
        self.theta = np.linalg.norm(self.step.delta_cam[:, 3:], axis=1)
        self.cand = candidate(p, self.step)
        self.cost_x, self.tol_x = cost_bound(p, self.okw)
        self.cost_c, self.tol_c = cost_bound(p, self.okw, *self.cand)
        self.gmax, self.gmax_tol = gradient_max_norm(p, self.okw)


    def oracle_errors(self):
        """name -> (error, bound) of the oracle's own float64 iteration (accepted steps: its parameters after the
        iteration are its candidate): the checks test_gpu_candidate.py makes of the GPU, cached."""
        if getattr(self, "_oe", None) is None:
            p, q, tr = self.prob, self.orc_x, self.trace
            assert self.accepted == 1
            _, ac, _ = active_blocks(p)
            eq = et = 0.0
            for t, cam in enumerate(ac):
                e = retraction_error(q.cams[cam], p.cams[cam], self.orc["delta_cam"][t])
                b = retraction_bound(p.cams[cam], self.orc["delta_cam"][t], cancelling_a=True)
                eq, et = max(eq, e[0] / b[0]), max(et, e[1] / b[1])
            cc, tc = cost_bound(p, self.okw, q.cams, q.intr, q.points)
            sn2, _, _, rb = norms(p, p.cams, p.intr, p.points, q.cams, q.intr, q.points)
            self._oe = dict(
                retract_q=(eq, 1.0), retract_t=(et, 1.0),
                cost_x=(abs(tr[0][0] - float(self.cost_x)), self.tol_x),
                cost_cand=(abs(tr[1][0] - float(cc)), tc),
                cost_change=(abs(tr[1][1] - float(self.cost_x - cc)), self.tol_x + tc),
                sn2=(abs(tr[1][3] ** 2 - float(sn2)) / float(sn2), rb + 4 * EPS64),
                gmax=(abs(tr[0][2] - self.gmax), self.gmax_tol))
        return self._oe


def reference(name, radius=1e4) -> Ref:
    key = ("r", name, float(radius))
    if key not in _cache:
        _cache[key] = Ref(name, radius)
    return _cache[key]


def zone_fractions(prob, okw, cams=None, intr=None, points=None):
    """Fraction of the reprojection / depth blocks in Huber's linear zone."""
    d = cost(prob, okw, cams, intr, points, detail=True)
    return float(d["lin_r"].mean()), float(d["lin_d"].mean())
