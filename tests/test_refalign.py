"""The reference of ba_align against itself (no GPU): the generator's truth is recovered, the samples are distinct and
uniform, the longdouble fit is stationary and orthogonal at the longdouble rounding, every listed case clears
MARGIN_MIN on every decision, the smallest-h rule is exercised by ties, and the stored f64 ratio is current."""
import numpy as np
import pytest

import refalign as ra


def test_generator_truth_is_recovered():
    for n, share, refit in ((64, 0.3, 0), (200, 0.5, 0), (200, 0.6, 3), (1000, 0.0, 1)):
        p1, p2, truth = ra.make_pair(n, share, seed=21)
        out = ra.align(p1, p2, refit=refit, n_hypotheses=512 if share > 0.5 else 256)
        err = float(np.abs(ra.act(out["poses"][0], p2) - ra.act(truth, p2)).max())
        n_in = int(out["stats"][0][2])
        print(f"n={n} outliers={share} refit={refit}: inliers {n_in}, action error {err:.2e}, k_needed {out['stats'][0][7]:.1f}")
        assert out["stats"][0][0] == ra.OK and n_in >= round((1 - share) * n) - 2
        # the noise is 1 cm per coordinate; a minimal sample extrapolates it over the room (a few cm), a refit averages it
        assert err < (0.01 if refit else 0.08)
        assert out["inlier"].sum() == n_in and out["poses"][0][3] >= 0


@pytest.mark.parametrize("n", [3, 4, 5, 2**31 - 1])
def test_samples_are_distinct_and_in_range(n):
    for seed in (0, 1, 2**64 - 1):
        for j in (0, 3, 2**31 - 1):
            for h in range(200):
                t = ra.sample(seed, j, h, n)
                assert len(set(t)) == 3 and min(t) >= 0 and max(t) < n


def test_samples_are_uniform_on_a_small_n():
    """n = 5: 60 ordered triples, 60000 hypotheses; each triple 1000 times on average (sigma 31, 6 sigma allowed)."""
    n, N = 5, 60000
    counts = {}
    for h in range(N):
        t = ra.sample(12345, h >> 14, h, n)
        counts[t] = counts.get(t, 0) + 1
    assert len(counts) == 60
    dev = max(abs(c - N / 60) for c in counts.values())
    print(f"largest deviation from {N / 60:.0f}: {dev:.0f}")
    assert dev < 6 * np.sqrt(N / 60)


def test_longdouble_fit_is_polished():
    rng = np.random.default_rng(3)
    A2 = rng.uniform(-2, 2, (500, 3, 3))
    R0 = np.stack([ra._rodrigues(w) for w in rng.normal(0, 0.5, (500, 3))])
    A1 = np.einsum("bik,bmk->bmi", R0, A2) + rng.normal(0, 0.3, (500, 1, 3)) + rng.normal(0, 0.02, (500, 3, 3))
    R, t, kappa, H = ra.arun_ref(A1, A2)
    ok = kappa < 1e4
    g, o = ra.stationarity(R[ok], H[ok])
    eps_ld = float(np.finfo(ra.LD).eps)
    print(f"{ok.sum()} fits: stationarity {float(g.max()):.2e}, orthogonality {float(o.max()):.2e}, longdouble eps {eps_ld:.2e}")
    assert float(g.max()) <= 64 * eps_ld and float(o.max()) <= 16 * eps_ld
    assert (np.linalg.det(R.astype(np.float64)) > 0.99).all()
    # the maximiser: no small rotation of R raises tr(R H)
    for w in np.eye(3) * 1e-4:
        for sgn in (1, -1):
            Rw = ra._rodrigues(sgn * w + 1e-300) @ R[ok].astype(np.float64)
            assert (np.trace(Rw @ H[ok].astype(np.float64), axis1=1, axis2=2) <=
                    np.trace((R[ok] @ H[ok]).astype(np.float64), axis1=1, axis2=2) + 1e-12).all()


@pytest.mark.parametrize("name", list(ra.CASES))
def test_margins(name):
    """Every decision of the case is far from its threshold: the integers of the stage have one right answer."""
    ref = ra.case_reference(name)
    margin = min(float(ref[r]["margin"].min()) for r in ra.REFITS)
    cross = float(ref[0]["cross_margin"].min())
    safety = float(ref[0]["safety"].min())
    print(f"{name}: threshold margin {margin:.2e}, cross margin {cross:.2e}, smallest cross product "
          f"{float(ref[0]['cross_min'].min()):.2e}, margin / rounding bound {safety:.2e}, off-diagonal left "
          f"{float(ref[0]['jacobi_off'].max()):.1e}")
    assert margin >= ra.MARGIN_MIN and cross >= ra.MARGIN_MIN
    assert safety >= 8.0
    assert float(ref[0]["jacobi_off"].max()) <= 4 * ra.EPS64  # SWEEPS sweeps have converged


def test_ties_exercise_the_smallest_h_rule():
    ties = {name: int(ra.case_reference(name)[0]["ties"].max()) for name in ra.CASES}
    print(ties)
    assert ties["n-64"] >= 20 and ties["hyp-513"] >= 20
    ref = ra.case_reference("n-64")[0]
    cnt = ref["hyp_count"][0]
    best = int(ref["stats"][0][3])
    assert cnt[best] == cnt.max() and (cnt[:best] < cnt.max()).all() and (cnt[best + 1:] == cnt.max()).any()


def test_refit_rounds_change_the_tight_cases():
    for name in ("tight-200", "tight-batch"):
        ref = ra.case_reference(name)
        n0, n3 = ref[0]["stats"][:, 2], ref[3]["stats"][:, 2]
        print(name, n0, ref[1]["stats"][:, 2], n3)
        assert (n3 >= n0).all() and (n3 > n0).any()
        assert (ref[3]["stats"][:, 6] == n0).all()  # the best sample's count is reported beside the refit's


def test_statuses_of_the_mixed_batch():
    ref = ra.case_reference("batch-17")[0]
    st = ref["stats"][:, 0].astype(int)
    n = ref["stats"][:, 1].astype(int)
    assert (st[n < 3] == ra.TOO_FEW).all() and st[4] == ra.NO_MODEL and (st == ra.OK).sum() == 12
    assert (ref["hyp_count"][n < 3] == -1).all() and (ref["hyp_count"][4] == -1).all()
    assert ref["stats"][5, 4] > 0  # samples that hit a NaN row are degenerate
    assert (ref["poses"][st != ra.OK] == ra.IDENTITY).all()


def test_f64_ratio():
    """align64 against the longdouble fit in units of kappa eps max|p|, over every fit of every case. F64_RATIO must
    cover it and not be stale by more than a factor two; the GPU bound is F = max(8, 4 F64_RATIO)."""
    worst, where = 0.0, None
    for name in ra.CASES:
        ref = ra.case_reference(name)
        fr = max(float(ref[r]["f64_ratio"].max()) for r in ra.REFITS)
        if fr > worst:
            worst, where = fr, name
    print(f"f64 ratio: {worst:.3f} at {where}; stored {ra.F64_RATIO}, F = {ra.POSE_F}")
    assert worst <= ra.F64_RATIO <= 2 * worst
    assert ra.POSE_F == max(8.0, 4 * ra.F64_RATIO)


def test_cases_cover_the_layout():
    T = ra.ALIGN_TILE
    assert set(ra.SIZES) == {3, 4, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1}
    assert set(ra.HYPS) == {1, 63, 64, 65, 255, 256, 257, 513}
    assert {len(ra.CASES[k][0]) for k in ("batch-1", "batch-2", "batch-17")} == {1, 2, 17}
    sizes = {s["n"] for s in ra.CASES["batch-17"][0]}
    assert {0, 2} <= sizes and any(s.get("kind") == "collinear" for s in ra.CASES["batch-17"][0])
    assert any(s.get("nan_rows") for s in ra.CASES["batch-17"][0])
