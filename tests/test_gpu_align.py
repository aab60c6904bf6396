"""ba_align on the GPU against tests/refalign.py: every integer the stage returns (hyp_count, best_hyp, n_inliers,
n_degenerate, the mask, the status) exactly, at refit 0, 1 and 3; the pose by its action within F kappa eps max|p|
(F = refalign.POSE_F, DESIGN 4.13's rule); reproducibility; independence of the neighbours in the batch; the stage
leaving the context's solve alone; the refusals in the scaffold's order; the sized structs.

The cases (refalign.CASES) are the smallest at which the kernels can go wrong: pair sizes around the minimum, the wave
and the LDS tile, hypothesis counts around the wave and the workgroup, batches of 1, 2 and 17 mixed pairs with empty,
two-point, collinear and NaN-carrying pairs. test_refalign.py shows every decision of them clear of its threshold by
MARGIN_MIN, so each integer has one right answer."""
import ctypes as C

import numpy as np
import pytest

import refalign as ra

pytestmark = pytest.mark.gpu

BA_E_INVALID = -1


@pytest.fixture(scope="module")
def solver():
    from miba.solver import Solver
    with Solver(minimizer_progress_to_stdout=0) as s:
        yield s


def run(solver, name, refit):
    p1, p2, begin, n_hyp, seed, kw = ra.case_inputs(name)
    return solver.align(p1, p2, begin, n_hypotheses=n_hyp, seed=seed, refit=refit, counts=True, **kw)


@pytest.mark.parametrize("refit", ra.REFITS)
@pytest.mark.parametrize("name", list(ra.CASES))
def test_against_reference(solver, name, refit):
    p1, p2, begin, n_hyp, seed, kw = ra.case_inputs(name)
    ref = ra.case_reference(name)[refit]
    out = run(solver, name, refit)
    np.testing.assert_array_equal(out["hyp_count"], ref["hyp_count"])
    for col, what in ((0, "status"), (1, "n"), (2, "n_inliers"), (3, "best_hyp"), (4, "n_degenerate"), (6, "n_inliers_sample")):
        np.testing.assert_array_equal(out["stats"][:, col], ref["stats"][:, col], err_msg=what)
    np.testing.assert_array_equal(out["inlier"], ref["inlier"])
    st = ref["stats"][:, 0].astype(int)
    assert (out["n_ok"], out["n_too_few"], out["n_no_model"]) == tuple(int((st == k).sum()) for k in (ra.OK, ra.TOO_FEW, ra.NO_MODEL))
    assert out["n_pairs"] == len(begin) - 1 and out["n_hypotheses"] == n_hyp
    thr = kw.get("threshold", 0.1)
    for j in range(len(begin) - 1):
        a, b = p1[begin[j]:begin[j + 1]], p2[begin[j]:begin[j + 1]]
        pose = out["poses"][j]
        if st[j] != ra.OK:
            np.testing.assert_array_equal(pose, ra.IDENTITY)
            continue
        fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
        err = float(np.abs(ra.act(pose.astype(ra.LD), b[fin]) - ra.act(ref["pose_ld"][j], b[fin])).max())
        bound = ra.POSE_F * ref["kappa"][j] * ra.EPS64 * ref["pmax"][j]
        print(f"{name} refit {refit} pair {j}: n {len(a)} inliers {int(out['stats'][j, 2])} action error {err:.2e} "
              f"bound {bound:.2e} (kappa {ref['kappa'][j]:.1f})")
        assert err <= bound
        assert pose[3] >= 0 and abs(float((pose[:4] ** 2).sum()) - 1) <= 8 * ra.EPS64
        # the RMS distance moves by at most the action's error; its sum of n squares rounds at n eps
        assert abs(out["stats"][j, 5] - ref["stats"][j, 5]) <= bound + 4 * len(a) * ra.EPS64 * thr
        k_ref = ref["stats"][j, 7]
        assert out["stats"][j, 7] == k_ref or abs(out["stats"][j, 7] - k_ref) <= 1e-12 * abs(k_ref)


def test_two_calls_give_the_same_bits(solver):
    for name, refit in (("batch-17", 3), ("n-513", 1)):
        a, b = run(solver, name, refit), run(solver, name, refit)
        for key in ("poses", "stats", "inlier", "hyp_count"):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_a_pair_does_not_depend_on_its_neighbours(solver):
    """Pair j = 2 of three: the same bits between small neighbours and between large, NaN-carrying ones."""
    mid1, mid2, _ = ra.make_pair(300, 0.4, seed=77)
    outs = []
    for specs in ([dict(n=5, outliers=0.0), dict(n=0)], [dict(n=513, outliers=0.5, nan_rows=4), dict(n=129, outliers=0.2)]):
        l1, l2, lb = ra.make_batch(specs, seed=5)
        r1, r2, _ = ra.make_pair(40 if specs[0]["n"] == 5 else 700, 0.3, seed=6)
        p1, p2 = np.concatenate([l1, mid1, r1]), np.concatenate([l2, mid2, r2])
        begin = np.concatenate([lb, [lb[-1] + 300, lb[-1] + 300 + len(r1)]]).astype(np.int32)
        o = solver.align(p1, p2, begin, n_hypotheses=257, seed=9, refit=3, threshold=0.03, counts=True)
        outs.append((o["poses"][2].tobytes(), o["stats"][2].tobytes(), o["hyp_count"][2].tobytes(),
                     o["inlier"][begin[2]:begin[3]].tobytes()))
        assert o["stats"][2, 0] == ra.OK and o["stats"][2, 2] > 100
    assert outs[0] == outs[1]


def test_a_solve_after_align_is_the_solve_without_it():
    """prepare, align, solve_prepared: the bits of prepare, solve_prepared on a fresh context (deterministic = 1, as
    the other stages' tests of this: the default solve is not reproducible by itself)."""
    from miba import synthetic
    from miba.solver import Solver
    p = synthetic.make_problem(n_cams=8, n_points=200, obs_per_point=(2, 4), seed=3)
    res = []
    for with_align in (False, True):
        q = p.copy()
        with Solver(minimizer_progress_to_stdout=0, deterministic=1) as s:
            s.prepare(q)
            if with_align:
                out = run(s, "batch-17", 3)
                assert out["n_ok"] == 12
            summ = s.solve_prepared(q)
            log = s.iteration_log()
        res.append((q.cams.tobytes(), q.points.tobytes(), q.intr.tobytes(), log.tobytes(), summ["final_cost"],
                    summ["initial_cost"], summ["num_iterations"], summ["num_successful_steps"]))
    assert res[0] == res[1]


def _raw(solver, prob, req, info):
    from miba.capi import BaAlignInfo, BaAlignProblem, BaAlignRequest
    ptr = lambda v, t: None if v is None else C.cast(C.pointer(v), C.POINTER(t))  # noqa: E731
    rc = solver._L.ba_align(solver._h, ptr(prob, BaAlignProblem), ptr(req, BaAlignRequest), ptr(info, BaAlignInfo))
    return rc, solver.last_error()


def _call(n_pairs=2, n_corr=8, begin=(0, 4, 8)):
    from miba.capi import BaAlignInfo, BaAlignProblem, BaAlignRequest
    keep = dict(begin=np.array(begin, dtype=np.int32), p1=np.arange(24.0), p2=np.arange(24.0) + 1, poses=np.zeros(14))
    g = BaAlignProblem()
    g.n_pairs, g.n_corr = n_pairs, n_corr
    g.pair_begin = keep["begin"].ctypes.data_as(C.POINTER(C.c_int32))
    g.p1 = keep["p1"].ctypes.data_as(C.POINTER(C.c_double))
    g.p2 = keep["p2"].ctypes.data_as(C.POINTER(C.c_double))
    req, info = BaAlignRequest(), BaAlignInfo()
    req.poses = keep["poses"].ctypes.data_as(C.POINTER(C.c_double))
    return g, req, info, keep


def test_refusals_in_the_scaffolds_order():
    from miba.solver import Solver
    below = lambda what: (f"{what} struct_size below BA_ALIGN_{what.upper()}_MIN_SIZE "  # noqa: E731
                          f"(set it with BA_ALIGN_{what.upper()}_INIT)")
    shards = "contexts with landmark shards (ba_comm_init*) are not supported"
    with Solver(minimizer_progress_to_stdout=0) as s, Solver(minimizer_progress_to_stdout=0) as sharded:
        sharded.comm_init(1, 0, Solver.comm_unique_id())

        def expect(solver, g, req, info, text):
            size = None if info is None else info.struct_size
            rc, msg = _raw(solver, g, req, info)
            print(f"rc={rc} error={msg!r}")
            assert rc == BA_E_INVALID and msg == f"ba_align: {text}"
            assert info is None or info.struct_size == size

        g, req, info, keep = _call()
        expect(s, None, req, info, "null argument")
        expect(s, g, None, info, "null argument")
        expect(s, g, req, None, "null argument")
        # each defect alone, then with every later one beside it: the earlier check of the fixed order wins
        g, req, info, keep = _call(); req.struct_size -= 8
        expect(s, g, req, info, below("request"))
        g, req, info, keep = _call(); req.struct_size -= 8; info.struct_size = 16; g.n_corr = -1
        expect(sharded, g, req, info, below("request"))
        g, req, info, keep = _call(); info.struct_size = 16
        expect(s, g, req, info, below("info"))
        g, req, info, keep = _call(); info.struct_size = 16; g.n_pairs = -1
        expect(sharded, g, req, info, below("info"))
        g, req, info, keep = _call()
        expect(sharded, g, req, info, shards)
        g, req, info, keep = _call(); g.n_corr = -1
        expect(sharded, g, req, info, shards)
        g, req, info, keep = _call(); g.n_corr = -1
        expect(s, g, req, info, "negative sizes")
        g, req, info, keep = _call(begin=(0, 5, 4)); g.n_pairs = -2
        expect(s, g, req, info, "negative sizes")
        g, req, info, keep = _call(begin=(0, 5, 4)); req.poses = None
        expect(s, g, req, info, "pair_begin decreases (pair 1)")
        g, req, info, keep = _call(begin=(-1, 4, 8))
        expect(s, g, req, info, "pair_begin starts below 0")
        g, req, info, keep = _call(begin=(0, 4, 7)); g.p1 = None
        expect(s, g, req, info, "pair_begin ends at 7, not at n_corr = 8")
        g, req, info, keep = _call(); g.pair_begin = None
        expect(s, g, req, info, "null required buffer (pair_begin)")
        g, req, info, keep = _call(); g.p2 = None; req.n_hypotheses = ra.MAX_HYP + 1
        expect(s, g, req, info, "null required buffer (p1 / p2)")
        g, req, info, keep = _call(); req.poses = None; req.n_hypotheses = ra.MAX_HYP + 1
        expect(s, g, req, info, "null required buffer (poses)")
        g, req, info, keep = _call(); req.n_hypotheses = ra.MAX_HYP + 1
        expect(s, g, req, info, f"n_hypotheses = {ra.MAX_HYP + 1} is above BA_ALIGN_MAX_HYP ({ra.MAX_HYP})")
        # and the same call without a defect goes through
        g, req, info, keep = _call()
        assert _raw(s, g, req, info) == (0, "") and info.n_pairs == 2


def test_sized_structs(solver):
    from miba.capi import BaAlignInfo
    p1, p2, begin, n_hyp, seed, kw = ra.case_inputs("batch-2")

    # an older caller: an info that ends before the timings is written no further than its size
    class Shell(C.Structure):
        _fields_ = [("info", BaAlignInfo), ("tail", C.c_uint8 * 24)]
    g, req, _, keep = _call()
    old = Shell()
    old.info.struct_size = BaAlignInfo.time_kernels_ms.offset
    C.memset(C.byref(old, old.info.struct_size), 0xA5, C.sizeof(Shell) - old.info.struct_size)
    assert _raw(solver, g, req, old.info) == (0, "")
    assert old.info.struct_size == BaAlignInfo.time_kernels_ms.offset and old.info.n_pairs == 2
    assert old.info.n_ok + old.info.n_too_few + old.info.n_no_model == 2 and old.info.n_hypotheses == 256
    assert bytes(old)[old.info.struct_size:] == b"\xa5" * (C.sizeof(Shell) - old.info.struct_size)
    # a newer caller: a larger struct keeps its tail and its size
    new = Shell()
    new.info.struct_size = C.sizeof(Shell)
    C.memset(new.tail, 0xA5, 24)
    assert _raw(solver, g, req, new.info) == (0, "")
    assert new.info.struct_size == C.sizeof(Shell) and new.info.n_pairs == 2 and bytes(new.tail) == b"\xa5" * 24
    assert new.info.time_total_ms > 0


def test_optional_outputs_and_defaults(solver):
    """Without masks and counts the poses are the same bits; the zeroed request's defaults are the named values."""
    p1, p2, begin, n_hyp, seed, kw = ra.case_inputs("batch-2")
    full = solver.align(p1, p2, begin, n_hypotheses=256, seed=seed, counts=True)
    bare = solver.align(p1, p2, begin, n_hypotheses=0, seed=seed, threshold=0.0, masks=False)
    assert bare["inlier"] is None and bare["hyp_count"] is None and bare["n_hypotheses"] == 256
    assert bare["poses"].tobytes() == full["poses"].tobytes() and bare["stats"].tobytes() == full["stats"].tobytes()
    one = solver.align(p1[begin[1]:], p2[begin[1]:], n_hypotheses=256, seed=seed)
    assert one["n_pairs"] == 1 and one["stats"][0, 0] == ra.OK
    empty = solver.align(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(1, dtype=np.int32))
    assert empty["n_pairs"] == 0 and empty["poses"].shape == (0, 7)
