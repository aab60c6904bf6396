"""ba_match on the GPU against tests/refmatch.py: every output array (nn_idx, nn_dist, accept, matches, match_begin,
pair_counts) and the info's counts with assert_array_equal, for both kinds. Every distance is an integer, so nothing
here has a tolerance.

The cases (refmatch.CASES) are the smallest at which the kernels can go wrong: n_q and n_t around every tile size, a
17 x 33 rectangle of random data at every descriptor size (a swapped operand map cannot pass), ties and the largest
distances, a pair the host slices, batches of 1, 2 and 9 with empty pairs and overlapping ranges, the acceptance
chain at three ratios with and without max_distance and cross_check. Then reproducibility, independence of the
neighbours in the batch, the stage leaving the context's solve alone, the refusals in the scaffold's order, the sized
structs, and the pipeline end to end (miba.matching, window.track_keyframe)."""
import ctypes as C

import numpy as np
import pytest

import refmatch as rm

pytestmark = pytest.mark.gpu

BA_E_INVALID = -1
ARRAYS = ("nn_idx", "nn_dist", "accept", "matches", "match_begin", "pair_counts")


@pytest.fixture(scope="module")
def solver():
    from miba.solver import Solver
    with Solver(minimizer_progress_to_stdout=0) as s:
        yield s


def run(solver, name, kind, nbytes=None, **over):
    q, t, pr, kw = rm.case_inputs(name, kind, nbytes)
    return solver.match(q, t, pr, kind=kind, counts=True, **{**kw, **over})


def check(out, ref):
    for key in ARRAYS:
        assert out[key].dtype == ref[key].dtype and out[key].shape == ref[key].shape, key
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    for key in ("n_matches", "n_pairs", "n_rows"):
        assert out[key] == ref[key], key
    np.testing.assert_array_equal(out["row_begin"], ref["row_begin"])


@pytest.mark.parametrize("kind,nbytes", [(k, b) for k in rm.KINDS for b in rm.DESC_BYTES[k]])
def test_rectangle_at_every_descriptor_size(solver, kind, nbytes):
    """First: 17 x 33 of random data pins which lane holds which row and column, and the padding of a k-step."""
    out = run(solver, "rect-17x33", kind, nbytes)
    check(out, rm.case_reference("rect-17x33", kind, nbytes))
    assert out["kind"] == rm.KIND_ID[kind]


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("name", [n for n in rm.CASES if n not in ("rect-17x33", "accept")])
def test_against_reference(solver, name, kind):
    check(run(solver, name, kind), rm.case_reference(name, kind))


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("ratio,md,cc", rm.ACCEPT_SETTINGS)
def test_acceptance_chain(solver, kind, ratio, md, cc):
    over = dict(ratio=ratio, max_distance=rm.MAX_DISTANCE[kind] if md else 0, cross_check=cc)
    out = run(solver, "accept", kind, **over)
    check(out, rm.case_reference("accept", kind, **over))
    c = out["pair_counts"]
    assert (c[:, 2:].sum(axis=1) == c[:, 0]).all() and out["n_matches"] == c[:, 2].sum()


@pytest.mark.parametrize("kind", rm.KINDS)
def test_forced_slicing_gives_the_same_bits(kind, monkeypatch):
    """The host slices the "slices" case's trains over several workgroups; MIBA_MATCH_SLICES = 1 forces one, and a
    count above the pair's tiles leaves empty slices (0 is "unset", 1000 is clamped): the same bits, the reference's."""
    from miba.solver import Solver
    ref = rm.case_reference("slices", kind, cross_check=True)
    outs = []
    for forced in (None, "1", "3", "64", "0", "1000"):
        if forced is None:
            monkeypatch.delenv("MIBA_MATCH_SLICES", raising=False)
        else:
            monkeypatch.setenv("MIBA_MATCH_SLICES", forced)
        with Solver(minimizer_progress_to_stdout=0) as s:
            out = run(s, "slices", kind, cross_check=True)
        check(out, ref)
        outs.append(b"".join(out[k].tobytes() for k in ARRAYS))
    assert len(set(outs)) == 1


@pytest.mark.parametrize("kind", rm.KINDS)
def test_two_calls_give_the_same_bits(solver, kind):
    a, b = (run(solver, "batch-9", kind, cross_check=True) for _ in range(2))
    for key in ARRAYS:
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("kind", rm.KINDS)
def test_a_pair_does_not_depend_on_its_neighbours(solver, kind):
    """Pair j = 1 of three: the same bits between small neighbours and between large ones."""
    nbytes = rm.DEFAULT_BYTES[kind]
    mq, mt, _ = rm.batch(kind, nbytes, [(70, 90)], 31)
    outs = []
    for shapes in ([(2, 3), (0, 5)], [(200, 300), (130, 65)]):
        q, t, pr = rm.batch(kind, nbytes, shapes, 32)
        q2, t2 = np.concatenate([q[: shapes[0][0]], mq, q[shapes[0][0]:]]), np.concatenate([t[: shapes[0][1]], mt, t[shapes[0][1]:]])
        a, b = shapes[0]
        rng = np.array([[0, a, 0, b], [a, a + 70, b, b + 90], [a + 70, len(q2), b + 90, len(t2)]], dtype=np.int32)
        o = solver.match(q2, t2, rng, kind=kind, cross_check=True, counts=True)
        r0, r1 = o["row_begin"][1], o["row_begin"][2]
        m0, m1 = o["match_begin"][1], o["match_begin"][2]
        outs.append((o["nn_idx"][r0:r1].tobytes(), o["nn_dist"][r0:r1].tobytes(), o["accept"][r0:r1].tobytes(),
                     o["matches"][m0:m1].tobytes(), o["pair_counts"][1].tobytes()))
        assert o["pair_counts"][1, 2] > 10
    assert outs[0] == outs[1]
    check1 = rm.match(mq, mt, [[0, 70, 0, 90]], kind, cross_check=True)
    assert outs[0][0] == check1["nn_idx"].tobytes() and outs[0][3] == check1["matches"].tobytes()


def test_a_solve_after_match_is_the_solve_without_it():
    """prepare, match, solve_prepared: the bits of prepare, solve_prepared on a fresh context (deterministic = 1, as
    the other stages' tests of this)."""
    from miba import synthetic
    from miba.solver import Solver
    p = synthetic.make_problem(n_cams=8, n_points=200, obs_per_point=(2, 4), seed=3)
    res = []
    for with_match in (False, True):
        q = p.copy()
        with Solver(minimizer_progress_to_stdout=0, deterministic=1) as s:
            s.prepare(q)
            if with_match:
                for kind in rm.KINDS:
                    assert run(s, "batch-9", kind, cross_check=True)["n_matches"] > 0
            summ = s.solve_prepared(q)
            log = s.iteration_log()
        res.append((q.cams.tobytes(), q.points.tobytes(), q.intr.tobytes(), log.tobytes(), summ["final_cost"],
                    summ["initial_cost"], summ["num_iterations"], summ["num_successful_steps"]))
    assert res[0] == res[1]


def _raw(solver, prob, req, info):
    from miba.capi import BaMatchInfo, BaMatchProblem, BaMatchRequest
    ptr = lambda v, t: None if v is None else C.cast(C.pointer(v), C.POINTER(t))  # noqa: E731
    rc = solver._L.ba_match(solver._h, ptr(prob, BaMatchProblem), ptr(req, BaMatchRequest), ptr(info, BaMatchInfo))
    return rc, solver.last_error()


def _call(ranges=((0, 3, 0, 5), (1, 4, 2, 6)), n_rows=6):
    from miba.capi import BaMatchInfo, BaMatchProblem, BaMatchRequest
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rng = np.random.default_rng(3)
    keep = dict(q=rm.random_desc(rng, 4, 32), t=rm.random_desc(rng, 6, 32), pr=np.array(ranges, dtype=np.int32),
                idx=np.zeros((8, 2), dtype=np.int32), dist=np.zeros((8, 2), dtype=np.int32),
                m=np.zeros((8, 2), dtype=np.int32), mb=np.zeros(3, dtype=np.int32))
    g = BaMatchProblem()
    g.kind, g.desc_bytes, g.n_query, g.n_train, g.n_pairs, g.n_rows = rm.HAMMING, 32, 4, 6, len(ranges), n_rows
    g.query, g.train = keep["q"].ctypes.data_as(u8p), keep["t"].ctypes.data_as(u8p)
    g.pair_range = keep["pr"].ctypes.data_as(i32p)
    req, info = BaMatchRequest(), BaMatchInfo()
    req.nn_idx, req.nn_dist = keep["idx"].ctypes.data_as(i32p), keep["dist"].ctypes.data_as(i32p)
    req.matches, req.match_begin = keep["m"].ctypes.data_as(i32p), keep["mb"].ctypes.data_as(i32p)
    return g, req, info, keep


def test_refusals_in_the_scaffolds_order():
    from miba.solver import Solver
    below = lambda what: (f"{what} struct_size below BA_MATCH_{what.upper()}_MIN_SIZE "  # noqa: E731
                          f"(set it with BA_MATCH_{what.upper()}_INIT)")
    shards = "contexts with landmark shards (ba_comm_init*) are not supported"
    with Solver(minimizer_progress_to_stdout=0) as s, Solver(minimizer_progress_to_stdout=0) as sharded:
        sharded.comm_init(1, 0, Solver.comm_unique_id())

        def expect(solver, g, req, info, text):
            size = None if info is None else info.struct_size
            rc, msg = _raw(solver, g, req, info)
            print(f"rc={rc} error={msg!r}")
            assert rc == BA_E_INVALID and msg == f"ba_match: {text}"
            assert info is None or info.struct_size == size

        g, req, info, keep = _call()
        expect(s, None, req, info, "null argument")
        expect(s, g, None, info, "null argument")
        expect(s, g, req, None, "null argument")
        # each defect alone, then with a later one beside it: the earlier check of the fixed order wins
        g, req, info, keep = _call(); req.struct_size -= 8
        expect(s, g, req, info, below("request"))
        g, req, info, keep = _call(); req.struct_size -= 8; info.struct_size = 16; g.n_rows = -1
        expect(sharded, g, req, info, below("request"))
        g, req, info, keep = _call(); info.struct_size = 16
        expect(s, g, req, info, below("info"))
        g, req, info, keep = _call(); info.struct_size = 16; g.n_pairs = -1
        expect(sharded, g, req, info, below("info"))
        g, req, info, keep = _call(); g.n_train = -1
        expect(sharded, g, req, info, shards)
        for field in ("n_query", "n_train", "n_pairs", "n_rows"):
            g, req, info, keep = _call(); setattr(g, field, -1); g.kind = 2
            expect(s, g, req, info, "negative sizes")
        g, req, info, keep = _call(); g.kind = 2; g.desc_bytes = 30
        expect(s, g, req, info, "kind = 2 is neither BA_MATCH_HAMMING nor BA_MATCH_L2_U8")
        for bad in (0, 30, 260):
            g, req, info, keep = _call(); g.desc_bytes = bad; g.pair_range = None
            expect(s, g, req, info, f"desc_bytes = {bad} is not a multiple of 4 in [4, 256]")
        g, req, info, keep = _call(); g.pair_range = None; g.n_rows = 5
        expect(s, g, req, info, "null required buffer (pair_range)")
        g, req, info, keep = _call(ranges=((0, 3, 0, 5), (3, 1, 2, 6))); g.n_rows = 5
        expect(s, g, req, info, "pair 1: the query range [3, 1) is reversed or leaves [0, n_query = 4)")
        g, req, info, keep = _call(ranges=((0, 5, 0, 5), (1, 4, 2, 6)))
        expect(s, g, req, info, "pair 0: the query range [0, 5) is reversed or leaves [0, n_query = 4)")
        g, req, info, keep = _call(ranges=((0, 3, -1, 5), (1, 4, 2, 6)))
        expect(s, g, req, info, "pair 0: the train range [-1, 5) is reversed or leaves [0, n_train = 6)")
        g, req, info, keep = _call(ranges=((0, 3, 0, 5), (1, 4, 2, 7))); g.query = None
        expect(s, g, req, info, "pair 1: the train range [2, 7) is reversed or leaves [0, n_train = 6)")
        g, req, info, keep = _call(n_rows=5); g.train = None
        expect(s, g, req, info, "n_rows = 5 is not the sum of the pairs' query counts (6)")
        g, req, info, keep = _call(); g.query = None; req.nn_idx = None
        expect(s, g, req, info, "null required buffer (query / train)")
        g, req, info, keep = _call(); g.train = None
        expect(s, g, req, info, "null required buffer (query / train)")
        g, req, info, keep = _call(); req.nn_dist = None; req.match_begin = None
        expect(s, g, req, info, "null required buffer (nn_idx / nn_dist)")
        g, req, info, keep = _call(); req.nn_idx = None
        expect(s, g, req, info, "null required buffer (nn_idx / nn_dist)")
        g, req, info, keep = _call(); req.match_begin = None
        expect(s, g, req, info, "null required buffer (match_begin with matches)")
        # and the same call without a defect goes through
        g, req, info, keep = _call()
        assert _raw(s, g, req, info) == (0, "") and info.n_pairs == 2 and info.n_rows == 6
        ref = rm.match(keep["q"], keep["t"], keep["pr"], "hamming")
        np.testing.assert_array_equal(keep["idx"][:6], ref["nn_idx"])
        np.testing.assert_array_equal(keep["mb"], ref["match_begin"])


def test_the_launch_limit_refusals_and_the_slices_setting(solver, monkeypatch):
    """A grid's threads must stay below 2^32. One pair of 2^31 - 1 queries and no train is 2^25 query tiles: refused
    by its size alone, before any buffer is read, written or allocated (the descriptors behind the pointer are a few
    rows). The text carries the slice count, so it also shows how MIBA_MATCH_SLICES parses: unset, 0 and negative
    values leave the host's choice (1 slice without a train), values above MATCH_MAX_SLICES are clamped to it."""
    big = 2 ** 31 - 1
    tiles = (big + rm.QTILE - 1) // rm.QTILE
    assert tiles == 2 ** 25
    for kind, tpb, setting, slices in (("l2_u8", 256, None, 1), ("l2_u8", 256, "0", 1), ("l2_u8", 256, "-3", 1),
                                       ("l2_u8", 256, "7", 7), ("l2_u8", 256, "1000", rm.MAX_SLICES),
                                       ("hamming", 64, "2", 2), ("hamming", 64, "64", 64), ("hamming", 64, "65", rm.MAX_SLICES)):
        if setting is None:
            monkeypatch.delenv("MIBA_MATCH_SLICES", raising=False)
        else:
            monkeypatch.setenv("MIBA_MATCH_SLICES", setting)
        assert tiles * slices * tpb > 2 ** 32 - 1
        g, req, info, keep = _call(ranges=((0, big, 0, 0),), n_rows=big)
        g.n_query, g.kind = big, rm.KIND_ID[kind]
        rc, msg = _raw(solver, g, req, info)
        print(f"rc={rc} error={msg!r}")
        assert rc == BA_E_INVALID and msg == (f"ba_match: the grid of {tiles} query tiles x {slices} train slices x {tpb} "
                                              "threads is above the launch limit of 2^32 threads")
    monkeypatch.delenv("MIBA_MATCH_SLICES", raising=False)
    # k_match_compact's grid is one workgroup of 256 threads per pair: 2^24 (empty) pairs are one too many
    n = 2 ** 24
    g, req, info, keep = _call(n_rows=0)
    ranges = np.zeros((n, 4), dtype=np.int32)
    g.n_pairs, g.pair_range = n, ranges.ctypes.data_as(C.POINTER(C.c_int32))
    rc, msg = _raw(solver, g, req, info)
    print(f"rc={rc} error={msg!r}")
    assert rc == BA_E_INVALID and msg == f"ba_match: the grid of {n} pairs x 256 threads is above the launch limit of 2^32 threads"


def test_sized_structs(solver):
    from miba.capi import BaMatchInfo

    # an older caller: an info that ends before the timings is written no further than its size
    class Shell(C.Structure):
        _fields_ = [("info", BaMatchInfo), ("tail", C.c_uint8 * 24)]
    g, req, _, keep = _call()
    old = Shell()
    old.info.struct_size = BaMatchInfo.time_kernels_ms.offset
    C.memset(C.byref(old, old.info.struct_size), 0xA5, C.sizeof(Shell) - old.info.struct_size)
    assert _raw(solver, g, req, old.info) == (0, "")
    assert old.info.struct_size == BaMatchInfo.time_kernels_ms.offset and old.info.n_pairs == 2 and old.info.n_rows == 6
    assert bytes(old)[old.info.struct_size:] == b"\xa5" * (C.sizeof(Shell) - old.info.struct_size)
    # a newer caller: a larger struct keeps its tail and its size
    new = Shell()
    new.info.struct_size = C.sizeof(Shell)
    C.memset(new.tail, 0xA5, 24)
    assert _raw(solver, g, req, new.info) == (0, "")
    assert new.info.struct_size == C.sizeof(Shell) and new.info.n_pairs == 2 and bytes(new.tail) == b"\xa5" * 24
    assert new.info.time_total_ms > 0


def test_optional_outputs_and_empty_calls(solver):
    q, t, pr, _ = rm.case_inputs("batch-2", "hamming")
    full = solver.match(q, t, pr, counts=True)
    bare = solver.match(q, t, pr, ratio=0.0, matches=False)  # ratio <= 0: the default
    assert bare["matches"] is None and bare["match_begin"] is None and bare["pair_counts"] is None
    for key in ("nn_idx", "nn_dist", "accept"):
        assert bare[key].tobytes() == full[key].tobytes()
    assert bare["n_matches"] == full["n_matches"] == len(full["matches"])
    one = solver.match(q[pr[1, 0]:pr[1, 1]], t[pr[1, 2]:pr[1, 3]])  # pair_range None: one pair over everything
    assert one["n_pairs"] == 1
    np.testing.assert_array_equal(one["matches"], full["matches"][full["match_begin"][1]:])
    none = solver.match(q, t, np.zeros((0, 4), dtype=np.int32), counts=True)
    assert none["n_pairs"] == 0 and none["n_rows"] == 0 and none["nn_idx"].shape == (0, 2)
    np.testing.assert_array_equal(none["match_begin"], [0])
    empty = solver.match(q[:0], t[:0], counts=True)
    assert empty["n_rows"] == 0 and empty["n_matches"] == 0
    np.testing.assert_array_equal(empty["pair_counts"], [[0] * 7])
    np.testing.assert_array_equal(empty["match_begin"], [0, 0])


# ---- end to end ----------------------------------------------------------------------------------------------------

def _pose(angle, t):
    """T_w_c as [qx, qy, qz, qw, t]: a rotation about y."""
    return np.array([0.0, np.sin(angle / 2), 0.0, np.cos(angle / 2), *t])


def _local(T, X):
    from miba import posegraph
    return posegraph.quat_rotate(posegraph.quat_conj(T[:4]), X - T[4:])


@pytest.fixture(scope="module")
def keyframe_pair():
    """Two synthetic keyframes of 500 features that share 350 landmarks (refmatch.two_keyframes: 256-bit descriptors,
    6 % of the bits flipped per observation), exact local points, a few of them without depth."""
    from miba import window
    da, db, ia, ib = rm.two_keyframes(0)
    rng = np.random.default_rng(5)
    X = rng.uniform(-2, 2, size=(int(max(ia.max(), ib.max())) + 1, 3)) + [0, 0, 6]
    Ta, Tb = _pose(0.0, [0, 0, 0]), _pose(0.1, [0.2, -0.1, 0.05])
    loc_a, loc_b = _local(Ta, X[ia]), _local(Tb, X[ib])
    loc_b[::17] = 0.0  # features without depth: the reference's filter drops their matches
    kf = lambda T, ids, loc, d: window.KeyFrame(T, np.zeros((500, 2), dtype=np.float32), loc,  # noqa: E731
                                                {i: int(g) for i, g in enumerate(ids)}, "", d)
    return kf(Ta, ia, loc_a, da), kf(Tb, ib, loc_b, db), ia, ib


def test_match_recovers_the_shared_landmarks(solver, keyframe_pair):
    a, b, ia, ib = keyframe_pair
    out = solver.match(a.descriptors, b.descriptors, counts=True)
    check(out, rm.match(a.descriptors, b.descriptors, [[0, 500, 0, 500]], "hamming"))
    m = out["matches"]
    assert out["n_matches"] == 350 and (ia[m[:, 0]] == ib[m[:, 1]]).all()  # all of them and no wrong pair


def test_correspondences_and_align(solver, keyframe_pair):
    from miba import matching
    a, b, _, _ = keyframe_pair
    out = solver.match(a.descriptors, b.descriptors)
    p1, p2 = matching.correspondences(out, 0, a.points3d_local, b.points3d_local)
    m = out["matches"]
    keep = (a.points3d_local[m[:, 0], 2] > 1e-15) & (b.points3d_local[m[:, 1], 2] > 1e-15)
    assert 0 < keep.sum() < len(m)
    h1, h2 = a.points3d_local[m[keep, 0]], b.points3d_local[m[keep, 1]]
    assert p1.tobytes() == h1.tobytes() and p2.tobytes() == h2.tobytes()
    x, y = solver.align(p1, p2, seed=4), solver.align(h1, h2, seed=4)
    assert x["poses"].tobytes() == y["poses"].tobytes() and x["stats"].tobytes() == y["stats"].tobytes()
    assert x["stats"][0, 2] == keep.sum()  # exact points: every correspondence is an inlier


def test_track_keyframe_with_a_matcher(solver, keyframe_pair):
    from miba import matching, window
    a, b, _, _ = keyframe_pair
    b.T_w_c = a.T_w_c.copy()  # the pose tracking starts from: the previous keyframe's
    out = window.track_keyframe(1, [a, b], {}, solver.align, match=solver.match, seed=4)
    p1, p2 = matching.correspondences(solver.match(a.descriptors, b.descriptors), 0, a.points3d_local, b.points3d_local)
    hand = solver.align(p1, p2, seed=4)
    assert out["tracked"] and out["poses"].tobytes() == hand["poses"].tobytes()
    assert out["stats"].tobytes() == hand["stats"].tobytes() and out["inlier"].tobytes() == hand["inlier"].tobytes()
    np.testing.assert_array_equal(b.T_w_c, window.se3_mul(a.T_w_c, hand["poses"][0]))
    np.testing.assert_allclose(b.T_w_c, _pose(0.1, [0.2, -0.1, 0.05]), atol=1e-9)
    # without descriptors the matcher is not asked: the landmark ids as before
    c = window.KeyFrame(b.T_w_c, b.keypoints, b.points3d_local, b.global_points_map)
    ids = window.track_keyframe(1, [a, c], {}, solver.align, match=solver.match, seed=4)
    q1, q2, _ = window.track_matches(1, [a, c])
    assert ids["stats"].tobytes() == solver.align(q1, q2, seed=4)["stats"].tobytes()


def test_matched_edges_between_keyframes_without_a_shared_id(solver):
    """Two sweeps past the same scene; the second sweep's landmarks got new ids (a revisit the map does not know
    about). measured_edges has nothing to measure the loop edges from; matched_edges finds them by the descriptors."""
    from miba import matching, posegraph, window
    from miba.capi import ProblemArrays
    rng = np.random.default_rng(8)
    n, n_lm, per_kf = 3, 260, 180
    X = rng.uniform(-2, 2, size=(n_lm, 3)) + [0, 0, 6]
    poses = [_pose(0.05 * k, [0.15 * k, 0.0, 0.02 * k]) for k in range(n)]
    poses += [_pose(0.05 * k + 0.02, [0.15 * k + 0.03, 0.04, 0.02 * k]) for k in range(n)]
    kfs = []
    for T in poses:
        seen = np.sort(rng.choice(n_lm, per_kf, replace=False))
        kfs.append(window.KeyFrame(T, np.zeros((per_kf, 2), dtype=np.float32), _local(T, X[seen]),
                                   {i: int(g) for i, g in enumerate(seen)}))
    matching.attach_descriptors(kfs, seed=7, kind="hamming", flip=0.06)
    assert all(kf.descriptors.shape == (per_kf, 32) and kf.descriptors.dtype == np.uint8 for kf in kfs)
    for kf in kfs[n:]:  # the revisit: new ids for the same landmarks
        kf.global_points_map = {i: g + n_lm for i, g in kf.global_points_map.items()}
    K = np.array([525.0, 525.0, 319.5, 239.5])
    oc = np.concatenate([np.full(per_kf, c) for c in range(2 * n)]).astype(np.int32)
    op = np.concatenate([list(kf.global_points_map.values()) for kf in kfs]).astype(np.int32)
    loc = np.concatenate([kf.points3d_local for kf in kfs])
    uv = np.stack([K[0] * loc[:, 0] / loc[:, 2] + K[2], K[1] * loc[:, 1] / loc[:, 2] + K[3]], 1)
    Xall = np.concatenate([X, X])
    prob = ProblemArrays(np.array(poses), Xall, K, K.copy(), oc, op, uv, loc[:, 2].copy(), fixed_cam=0)
    pairs = [(0, n), (1, n + 1), (0, 1)]
    ea, eb, _, _ = posegraph.measured_edges(prob, pairs, solver.align, seed=3)
    assert list(zip(ea.tolist(), eb.tolist())) == [(0, 1)]  # the loop pairs share no landmark id
    ma, mb, meas, n_in = matching.matched_edges(kfs, pairs, solver.match, solver.align, seed=3)
    assert list(zip(ma.tolist(), mb.tolist())) == pairs and (n_in >= 20).all()
    assert ma.dtype == mb.dtype == np.int32 and meas.shape == (3, 7)
    _, _, truth = posegraph.edges_from_poses(np.array(poses), pairs)
    dq = posegraph.quat_mul(posegraph.quat_conj(meas[:, :4]), truth[:, :4])
    # exact points: the edge is the true relative pose to rounding (ba_align's pose error is F kappa eps |p|, 1e-9 is
    # far above it and far below the 3 cm between the two sweeps)
    assert np.abs(meas[:, 4:] - truth[:, 4:]).max() < 1e-9 and np.linalg.norm(dq[:, :3], axis=1).max() < 1e-9
    empty = matching.matched_edges(kfs, np.zeros((0, 2), dtype=int), solver.match, solver.align)
    assert [len(x) for x in empty] == [0, 0, 0, 0]
