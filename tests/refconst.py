"""The first-LM-step references of tests/refstep.py under a set of constant cameras (test infrastructure).

refstep's ``_Lin`` drops the gauge camera through ``cam_has``: its observations keep their rows, their point and
intrinsics columns, and lose their camera columns. ``restrict`` drops the masked cameras from a built ``_Lin`` the
same way — every per-camera quantity of ``_Lin`` (column norms, Jacobi scale, LM diagonal) belongs to one camera alone,
so removing a camera is removing its entries — and ``qr_step`` / ``schur_step`` / ``reduced_system`` run refstep's own
routines on the restricted blocks (refstep's routines build their ``_Lin`` through the module's name, which is pointed
at the restricting constructor for the duration of a call).
"""
from __future__ import annotations

import numpy as np

import refstep
from refstep import LD


def restrict(L, mask):
    """``L`` (a refstep._Lin) without the camera columns of the cameras in ``mask`` (n_cams,) bool."""
    mask = np.asarray(mask, bool)
    keep = ~mask[L.ac_cam]
    new = np.full(max(L.nac, 1), -1, np.int64)
    new[: L.nac][keep] = np.arange(int(keep.sum()))
    ac = np.where(L.ac >= 0, new[np.where(L.ac >= 0, L.ac, 0)], -1)
    L.ac_cam = L.ac_cam[keep]
    L.nac = len(L.ac_cam)
    L.ac, L.on = ac, ac >= 0
    L.acz = np.where(L.on, ac, 0)
    L.s_c, L.d2_c = L.s_c[keep], L.d2_c[keep]
    L.jc = L.jc * L.on[:, None, None]
    L.Jc = L.jc * L.s_c[L.acz][:, None, :] if L.nac else np.zeros_like(L.jc)
    L.n = 6 * L.nac + 3 * L.nap + 4
    L.o_p, L.o_k = 6 * L.nac, 6 * L.nac + 3 * L.nap
    return L


def _masked(fn, mask, *args):
    orig = refstep._Lin
    refstep._Lin = lambda prob, opts, radius: restrict(orig(prob, opts, radius), mask)
    try:
        return fn(*args)
    finally:
        refstep._Lin = orig


def qr_step(prob, mask, opts=None, radius: float = 0.0):
    return _masked(refstep.qr_step, mask, prob, opts, radius)


def schur_step(prob, mask, opts=None, radius: float = 0.0):
    return _masked(refstep.schur_step, mask, prob, opts, radius)


def reduced_system(prob, mask, opts=None, radius: float = 0.0):
    """(S, rhs) of the scaled, damped reduced system under the mask, rounded to f64 and symmetrised; an infinite
    radius gives the undamped system."""
    L = restrict(refstep._Lin(prob, opts, radius), mask)
    S, rhs, _ = refstep.schur_reduce(L)
    S = S.astype(np.float64)
    return (S + S.T) / 2, rhs.astype(np.float64), L


def schur_cov(prob, mask, opts=None):
    """tests/refcov.py's ``schur_cov`` (the covariance reference of test_gpu_cov.py) with the masked cameras dropped:
    refcov builds its ``_Lin`` through its own module's name, pointed at the restricting constructor for the call."""
    import refcov
    orig = refcov._Lin
    refcov._Lin = lambda p, o, radius: restrict(orig(p, o, radius), mask)
    try:
        return refcov.schur_cov(prob, opts)
    finally:
        refcov._Lin = orig


# ------------------------------------------------------------------------------------------------ masks and windows
def masks(n_cams, empty_cam=None):
    """name -> (mask, fixed_cam) of the constant-camera tests on a window of ``n_cams`` cameras."""
    def m(*idx):
        a = np.zeros(n_cams, bool)
        a[list(idx)] = True
        return a

    mid = n_cams // 2
    out = {
        "first": (m(0), -1),
        "middle": (m(mid), -1),
        "last": (m(n_cams - 1), -1),
        "adjacent": (m(mid, mid + 1), -1),
        "every_second": (m(*range(0, n_cams, 2)), -1),
        "all_but_one": (m(*[c for c in range(n_cams) if c != mid]), -1),
        "plus_fixed": (m(mid), 1),
    }
    if empty_cam is not None:
        out["unobserved"] = (m(empty_cam, 0), -1)
    return out


_cache = {}


def window(kind):
    """The windows of the constant-camera tests, built with refstep's generator (cached; not to be modified):
    ``small`` 6 cameras (one block: the dense one-block solve, the band tail, the blocked Cholesky when forced),
    ``bcr`` 24 cameras with tracks of 4..9 (12 active cameras under every second camera constant: two BCR blocks).
    Camera 2 has no admissible observation."""
    if kind not in _cache:
        from miba import synthetic
        cfg = {"small": refstep._w(6, (2, 4), 811), "bcr": refstep._w(24, (4, 9), 812)}[kind]
        p = synthetic.make_problem(**cfg)
        p.obs_depth[p.obs_cam == 2] = 0.0
        _cache[kind] = p
    return _cache[kind]


EMPTY_CAM = 2


def case(kind, name):
    """(window with the case's fixed_cam, mask, schur_step reference) of mask ``name`` on window ``kind``, cached."""
    key = (kind, name)
    if key not in _cache:
        base = window(kind)
        mask, fixed = masks(base.n_cams, EMPTY_CAM)[name]
        p = base.copy()
        p.fixed_cam = fixed
        _cache[key] = (p, mask, schur_step(p, mask, None, 1e4))
    return _cache[key]


MASK_NAMES = ("first", "middle", "last", "adjacent", "every_second", "all_but_one", "plus_fixed", "unobserved")
