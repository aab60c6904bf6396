"""The covariance references (tests/refcov.py) against each other, on the CPU.

qr_cov (dense QR of the whole scaled Jacobian, Sigma = R^-1 R^-T) and schur_cov (point elimination in extended
precision, the reduced inverse Newton-refined in extended precision) share only the oracle's per-observation
Jacobians and the restated Jacobi scaling; over ALL pairs of camera / intrinsics blocks and ALL points they must agree
within tol = refstep.step_tol(cond) = 8 cond eps, cond the 2-norm condition of the scaled, undamped reduced matrix,
the tolerance test_gpu_cov.py holds the device to. The Schur reference without the extended-precision refinement
(plain f64 LAPACK inversion, what windows of n > 500 use) must stay within the same tolerance of the refined one."""
import pytest

import refcov
import refstep

WINDOWS = ["one1", "one2", "one10", "bcr11", "bcr21", "gauge_mid21", "inactive_mid21", "bcr21_messy", "dense_n160"]


@pytest.mark.parametrize("name", WINDOWS)
def test_qr_and_schur_covariances_agree(name):
    p, s = refcov.reference(name)
    q = refcov.qr_cov(p)
    assert list(q.ac_cam) == list(s.ac_cam)
    tol = refstep.step_tol(s.cond)
    ep, ex = refcov.pair_errors(q.red, s.red), refcov.point_errors(q.pts, s.pts)
    print(f"REFCOV {name} n={s.red.shape[0]} cond={s.cond:.3g} tol={tol:.2e} qr-schur pairs={ep:.1e} points={ex:.1e}")
    assert ep <= tol and ex <= tol, (ep, ex, tol)


@pytest.mark.parametrize("name", WINDOWS)
def test_unrefined_schur_within_tol(name):
    p, s = refcov.reference(name)
    u = refcov.schur_cov(p, None, refine=False)
    tol = refstep.step_tol(s.cond)
    ep, ex = refcov.pair_errors(u.red, s.red), refcov.point_errors(u.pts, s.pts)
    print(f"REFCOV-F64 {name} tol={tol:.2e} pairs={ep:.1e} points={ex:.1e}")
    assert ep <= tol and ex <= tol, (ep, ex, tol)
