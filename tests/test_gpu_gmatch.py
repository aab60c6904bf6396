"""ba_guided_match on the GPU against tests/refgmatch.py: every integer output (nn_kp, nn_dist, status, n_in_window,
matches, match_begin, frame_counts) and the info's counts with assert_array_equal, for both kinds; proj within the
bound tests/test_gpu_resid.py holds the reprojection error to against its extended-precision reference
(refresid.TOL: u / v 2.9e-12 px, z 1.5e-14).

The comparison can be exact because no floating-point decision of a case is within 1e-6, relative, of its threshold
(test_refgmatch.py). The cases (refgmatch.CASES) are the smallest at which the kernels can go wrong: every descriptor
size class, candidate counts around the search kernel's wave and the scanning workgroup, entries without keypoints or
candidates, keypoints and projections on cell boundaries, a radius below one cell and one of several cells, windows
clipped at the borders of an image that is no multiple of the cell, keypoints outside the image, 300 keypoints on one
pixel, ties, the acceptance chain with every switch on and off. Then: cell_px and a second call change no bit, five
hypotheses over one range are five separate calls, an all-covering window gives Solver.match's neighbours, the stage
leaves the context's solve alone, the refusals in their order, the sized structs, and the pipeline
(window.search_local_map, matching.fuse_landmarks) end to end."""
import ctypes as C

import numpy as np
import pytest

import refgmatch as rg
import refmatch as rm
import refresid

pytestmark = pytest.mark.gpu

BA_E_INVALID = -1
LD = np.longdouble


@pytest.fixture(scope="module")
def solver():
    from miba.solver import Solver
    with Solver(minimizer_progress_to_stdout=0) as s:
        yield s


def run(solver, name, kind, nbytes=None, **over):
    args, kw = rg.case_inputs(name, kind, nbytes)
    return solver.guided_match(**args, kind=kind, counts=True, proj=True, **{**kw, **over})


def check(out, ref, tag=""):
    for key in rg.INT_ARRAYS:
        assert out[key].dtype == ref[key].dtype and out[key].shape == ref[key].shape, key
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    for key in ("n_matches", "n_frames", "n_rows"):
        assert out[key] == ref[key], key
    np.testing.assert_array_equal(out["cand_begin"], ref["cand_begin"])
    np.testing.assert_array_equal(out["cand_pt"], ref["cand_pt"])
    if len(ref["proj"]):
        e = np.abs(out["proj"].astype(LD) - ref["proj"])
        front = ref["status"] != rg.BEHIND  # (behind the camera u and v are 0 and z is all there is)
        uv = float(e[front, :2].max()) if front.any() else 0.0
        z = float(e[:, 2].max())
        print(f"GMATCH {tag} proj uv={uv:.2e} z={z:.2e}")
        assert uv <= refresid.TOL["uv"] and z <= refresid.TOL["z"]
        assert (out["proj"][~front, :2] == 0).all()


@pytest.mark.parametrize("kind,nbytes", [(k, b) for k in rm.KINDS for b in rg.DESC_BYTES[k]])
def test_every_descriptor_size(solver, kind, nbytes):
    out = run(solver, "small", kind, nbytes)
    check(out, rg.case_reference("small", kind, nbytes), f"small {kind} {nbytes}")
    assert out["kind"] == rm.KIND_ID[kind] and out["n_grids"] == 1 and out["cell_px"] == 16


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("name", [n for n in rg.CASES if n not in ("small", "accept")])
def test_against_reference(solver, name, kind):
    check(run(solver, name, kind), rg.case_reference(name, kind), f"{name} {kind}")


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("ratio,md,tol,one", rg.ACCEPT_SETTINGS)
def test_acceptance_chain(solver, kind, ratio, md, tol, one):
    over = rg.accept_kw(kind, ratio, md, tol, one)
    out = run(solver, "accept", kind, **over)
    check(out, rg.case_reference("accept", kind, **over), f"accept {kind}")
    c = out["frame_counts"]
    assert (c[:, 2:].sum(axis=1) == c[:, 0]).all() and out["n_matches"] == c[:, 2].sum()


def _bits(out):
    return b"".join(out[k].tobytes() for k in rg.INT_ARRAYS + ("proj",))


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("name", ["cand-counts", "boundaries", "borders", "crowd", "wide"])
def test_cell_px_gives_the_same_bits(solver, name, kind):
    ref = rg.case_reference(name, kind)
    outs = []
    for cell in rg.CELLS:
        out = run(solver, name, kind, cell_px=cell)
        assert out["cell_px"] == cell
        check(out, ref, f"{name} {kind} cell {cell}")
        outs.append(_bits(out))
    assert len(set(outs)) == 1


@pytest.mark.parametrize("kind", rm.KINDS)
def test_two_calls_give_the_same_bits(solver, kind):
    a, b = (run(solver, "cand-counts", kind) for _ in range(2))
    assert _bits(a) == _bits(b)


@pytest.mark.parametrize("kind", rm.KINDS)
def test_five_hypotheses_are_five_separate_calls(solver, kind):
    args, kw = rg.case_inputs("hypotheses", kind)
    all5 = run(solver, "hypotheses", kind)
    assert all5["n_grids"] == 1 and all5["n_frames"] == 5  # one binned grid for the shared range
    for f in range(5):
        one = solver.guided_match(**{**args, "frame_pose": args["frame_pose"][f:f + 1]}, kind=kind, counts=True, proj=True, **kw)
        a, b = all5["cand_begin"][f], all5["cand_begin"][f + 1]
        for key in ("nn_kp", "nn_dist", "status", "n_in_window", "proj"):
            assert one[key].tobytes() == all5[key][a:b].tobytes(), (f, key)
        m0, m1 = all5["match_begin"][f], all5["match_begin"][f + 1]
        assert one["matches"].tobytes() == all5["matches"][m0:m1].tobytes()
        assert one["frame_counts"][0].tobytes() == all5["frame_counts"][f].tobytes()


@pytest.mark.parametrize("kind", rm.KINDS)
def test_an_all_covering_window_gives_match_neighbours(solver, kind):
    args, kw = rg.case_inputs("all-in-view", kind)
    out = run(solver, "all-in-view", kind)
    assert (out["n_in_window"] == len(args["kp_uv"])).all()
    m = solver.match(args["pt_desc"], args["kp_desc"], kind=kind)
    np.testing.assert_array_equal(out["nn_kp"], m["nn_idx"])
    np.testing.assert_array_equal(out["nn_dist"], m["nn_dist"])


def test_a_solve_after_guided_match_is_the_solve_without_it():
    """prepare, guided_match, solve_prepared: the bits of prepare, solve_prepared on a fresh context (deterministic =
    1, as the other stages' tests of this)."""
    from miba import synthetic
    from miba.solver import Solver
    p = synthetic.make_problem(n_cams=8, n_points=200, obs_per_point=(2, 4), seed=3)
    res = []
    for with_stage in (False, True):
        q = p.copy()
        with Solver(minimizer_progress_to_stdout=0, deterministic=1) as s:
            s.prepare(q)
            if with_stage:
                for kind in rm.KINDS:
                    assert run(s, "cand-counts", kind)["n_matches"] > 0
            summ = s.solve_prepared(q)
            log = s.iteration_log()
        res.append((q.cams.tobytes(), q.points.tobytes(), q.intr.tobytes(), log.tobytes(), summ["final_cost"],
                    summ["initial_cost"], summ["num_iterations"], summ["num_successful_steps"]))
    assert res[0] == res[1]


# ---- the refusals, the sized structs, the optional outputs -----------------------------------------------------------

def _raw(solver, prob, req, info):
    from miba.capi import BaGmatchInfo, BaGmatchProblem, BaGmatchRequest
    ptr = lambda v, t: None if v is None else C.cast(C.pointer(v), C.POINTER(t))  # noqa: E731
    rc = solver._L.ba_guided_match(solver._h, ptr(prob, BaGmatchProblem), ptr(req, BaGmatchRequest), ptr(info, BaGmatchInfo))
    return rc, solver.last_error()


def _call():
    """Two frame entries over six keypoints and three landmarks, four rows."""
    from miba.capi import BaGmatchInfo, BaGmatchProblem, BaGmatchRequest
    i32p, u8p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    args, _ = rg.case_inputs("small", "hamming")
    keep = dict(uv=args["kp_uv"][:6].copy(), kd=args["kp_desc"][:6].copy(), pts=args["points"][:3].copy(),
                pd=args["pt_desc"][:3].copy(), pose=np.repeat(args["frame_pose"], 2, axis=0),
                rng=np.array([[0, 6], [2, 5]], dtype=np.int32), cb=np.array([0, 3, 4], dtype=np.int32),
                cp=np.array([0, 1, 2, 1], dtype=np.int32), nn=np.zeros((4, 2), dtype=np.int32), dist=np.zeros((4, 2), dtype=np.int32),
                st=np.zeros(4, dtype=np.uint8), m=np.zeros((4, 2), dtype=np.int32), mb=np.zeros(3, dtype=np.int32))
    g = BaGmatchProblem()
    g.kind, g.desc_bytes, g.width, g.height = rm.HAMMING, 32, rg.W0, rg.H0
    g.n_kp, g.n_points, g.n_frames, g.n_rows = 6, 3, 2, 4
    g.intr[:] = list(args["intr"])
    g.kp_uv, g.kp_desc = keep["uv"].ctypes.data_as(f64p), keep["kd"].ctypes.data_as(u8p)
    g.points, g.pt_desc = keep["pts"].ctypes.data_as(f64p), keep["pd"].ctypes.data_as(u8p)
    g.frame_pose, g.frame_range = keep["pose"].ctypes.data_as(f64p), keep["rng"].ctypes.data_as(i32p)
    g.cand_begin, g.cand_pt = keep["cb"].ctypes.data_as(i32p), keep["cp"].ctypes.data_as(i32p)
    req, info = BaGmatchRequest(), BaGmatchInfo()
    req.radius = 15.0
    req.nn_kp, req.nn_dist, req.status = keep["nn"].ctypes.data_as(i32p), keep["dist"].ctypes.data_as(i32p), keep["st"].ctypes.data_as(u8p)
    req.matches, req.match_begin = keep["m"].ctypes.data_as(i32p), keep["mb"].ctypes.data_as(i32p)
    return g, req, info, keep


def test_refusals_in_their_order():
    from miba.solver import Solver
    below = lambda what: (f"{what} struct_size below BA_GMATCH_{what.upper()}_MIN_SIZE "  # noqa: E731
                          f"(set it with BA_GMATCH_{what.upper()}_INIT)")
    shards = "contexts with landmark shards (ba_comm_init*) are not supported"
    null = "null required buffer "
    with Solver(minimizer_progress_to_stdout=0) as s, Solver(minimizer_progress_to_stdout=0) as sharded:
        sharded.comm_init(1, 0, Solver.comm_unique_id())

        def expect(solver, g, req, info, text):
            size = None if info is None else info.struct_size
            rc, msg = _raw(solver, g, req, info)
            print(f"rc={rc} error={msg!r}")
            assert rc == BA_E_INVALID and msg == f"ba_guided_match: {text}"
            assert info is None or info.struct_size == size

        g, req, info, keep = _call()
        expect(s, None, req, info, "null argument")
        expect(s, g, None, info, "null argument")
        expect(s, g, req, None, "null argument")
        # each defect alone or with a later one beside it: the earlier check of the fixed order wins
        g, req, info, keep = _call(); req.struct_size -= 8; info.struct_size = 16; g.n_rows = -1
        expect(sharded, g, req, info, below("request"))
        g, req, info, keep = _call(); info.struct_size = 16; g.n_frames = -1
        expect(sharded, g, req, info, below("info"))
        g, req, info, keep = _call(); g.n_kp = -1
        expect(sharded, g, req, info, shards)
        for field in ("n_kp", "n_points", "n_frames", "n_rows"):
            g, req, info, keep = _call(); setattr(g, field, -1); g.kind = 2
            expect(s, g, req, info, "negative sizes")
        g, req, info, keep = _call(); g.kind = 2; g.desc_bytes = 30
        expect(s, g, req, info, "kind = 2 is neither BA_MATCH_HAMMING nor BA_MATCH_L2_U8")
        for bad in (0, 30, 260):
            g, req, info, keep = _call(); g.desc_bytes = bad; g.width = 0
            expect(s, g, req, info, f"desc_bytes = {bad} is not a multiple of 4 in [4, 256]")
        g, req, info, keep = _call(); g.width = 0; req.radius = 0.0
        expect(s, g, req, info, "width = 0, height = 75: both must be positive")
        g, req, info, keep = _call(); g.height = -1
        expect(s, g, req, info, "width = 100, height = -1: both must be positive")
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            g, req, info, keep = _call(); req.radius = bad; g.frame_range = None
            expect(s, g, req, info, "radius is not a finite positive number")
        for field in ("frame_pose", "frame_range", "cand_begin"):
            g, req, info, keep = _call(); setattr(g, field, None); keep["rng"][0, 1] = 7
            expect(s, g, req, info, null + "(frame_pose / frame_range / cand_begin)")
        g, req, info, keep = _call(); keep["rng"][1] = (5, 2); keep["cb"][0] = 1
        expect(s, g, req, info, "frame 1: the keypoint range [5, 2) is reversed or leaves [0, n_kp = 6)")
        g, req, info, keep = _call(); keep["rng"][0] = (0, 7)
        expect(s, g, req, info, "frame 0: the keypoint range [0, 7) is reversed or leaves [0, n_kp = 6)")
        g, req, info, keep = _call(); keep["cb"][0] = 1; keep["cb"][2] = 0
        expect(s, g, req, info, "cand_begin[0] = 1 is not 0")
        g, req, info, keep = _call(); keep["cb"][1] = 5; g.n_rows = 7
        expect(s, g, req, info, "cand_begin decreases at frame 1")
        g, req, info, keep = _call(); g.n_rows = 5; g.cand_pt = None
        expect(s, g, req, info, "n_rows = 5 is not cand_begin[n_frames] (4)")
        g, req, info, keep = _call(); g.cand_pt = None; g.kp_uv = None
        expect(s, g, req, info, null + "(cand_pt)")
        g, req, info, keep = _call(); keep["cp"][2] = 3; g.kp_uv = None
        expect(s, g, req, info, "cand_pt[2] = 3 leaves [0, n_points = 3)")
        g, req, info, keep = _call(); keep["cp"][0] = -1
        expect(s, g, req, info, "cand_pt[0] = -1 leaves [0, n_points = 3)")
        g, req, info, keep = _call(); g.kp_desc = None; g.points = None
        expect(s, g, req, info, null + "(kp_uv / kp_desc)")
        g, req, info, keep = _call(); g.pt_desc = None; req.status = None
        expect(s, g, req, info, null + "(points / pt_desc)")
        for field in ("nn_kp", "nn_dist", "status"):
            g, req, info, keep = _call(); setattr(req, field, None); req.match_begin = None
            expect(s, g, req, info, null + "(nn_kp / nn_dist / status)")
        g, req, info, keep = _call(); req.match_begin = None
        expect(s, g, req, info, null + "(match_begin with matches)")
        # the launch limits, refused by the sizes alone before anything is allocated or read
        g, req, info, keep = _call(); g.width = g.height = 2 ** 31 - 1; req.cell_px = 8
        expect(s, g, req, info, "the grid of 268435456 x 268435456 cells x 2 keypoint ranges is above the limit of 2^31 - 1 cells")
        n = 2 ** 24
        g, req, info, keep = _call()
        zeros, many = np.zeros(n + 1, dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
        g.n_frames, g.n_rows = n, 0
        g.cand_begin, g.frame_range = zeros.ctypes.data_as(C.POINTER(C.c_int32)), many.ctypes.data_as(C.POINTER(C.c_int32))
        expect(s, g, req, info, f"the grid of {n} frames x 256 threads is above the launch limit of 2^32 threads")
        # and the same call without a defect goes through
        g, req, info, keep = _call()
        assert _raw(s, g, req, info) == (0, "") and info.n_frames == 2 and info.n_rows == 4 and info.n_grids == 2
        ref = rg.guided(keep["pts"], keep["pd"], keep["uv"], keep["kd"], keep["pose"], list(g.intr), rg.W0, rg.H0,
                        frame_range=keep["rng"], cand=[[0, 1, 2], [1]], kind="hamming")
        assert ref["margin"] >= rg.MIN_MARGIN
        np.testing.assert_array_equal(keep["nn"], ref["nn_kp"])
        np.testing.assert_array_equal(keep["st"], ref["status"])
        np.testing.assert_array_equal(keep["mb"], ref["match_begin"])


def test_sized_structs(solver):
    from miba.capi import BaGmatchInfo

    class Shell(C.Structure):
        _fields_ = [("info", BaGmatchInfo), ("tail", C.c_uint8 * 24)]
    g, req, _, keep = _call()
    old = Shell()  # an older caller: an info that ends before the timings is written no further than its size
    old.info.struct_size = BaGmatchInfo.time_kernels_ms.offset
    C.memset(C.byref(old, old.info.struct_size), 0xA5, C.sizeof(Shell) - old.info.struct_size)
    assert _raw(solver, g, req, old.info) == (0, "")
    assert old.info.struct_size == BaGmatchInfo.time_kernels_ms.offset and old.info.n_frames == 2 and old.info.n_rows == 4
    assert bytes(old)[old.info.struct_size:] == b"\xa5" * (C.sizeof(Shell) - old.info.struct_size)
    new = Shell()  # a newer caller: a larger struct keeps its tail and its size
    new.info.struct_size = C.sizeof(Shell)
    C.memset(new.tail, 0xA5, 24)
    assert _raw(solver, g, req, new.info) == (0, "")
    assert new.info.struct_size == C.sizeof(Shell) and new.info.n_frames == 2 and bytes(new.tail) == b"\xa5" * 24
    assert new.info.time_total_ms > 0


def test_optional_outputs_and_empty_calls(solver):
    args, kw = rg.case_inputs("empty", "hamming")
    full = solver.guided_match(**args, counts=True, proj=True)
    bare = solver.guided_match(**args, ratio=0.0, min_depth=-1.0, matches=False)  # <= 0: the defaults
    assert bare["matches"] is None and bare["match_begin"] is None and bare["frame_counts"] is None and bare["proj"] is None
    for key in ("nn_kp", "nn_dist", "status", "n_in_window"):
        assert bare[key].tobytes() == full[key].tobytes()
    assert bare["n_matches"] == full["n_matches"] == len(full["matches"])
    # frame_range None: every keypoint for every entry; cand None: every landmark
    one = solver.guided_match(**{**args, "frame_range": None, "cand": None, "frame_pose": args["frame_pose"][:1]}, counts=True)
    ref = rg.guided(**{**args, "frame_range": None, "cand": None, "frame_pose": args["frame_pose"][:1]})
    np.testing.assert_array_equal(one["matches"], ref["matches"])
    np.testing.assert_array_equal(one["frame_counts"], ref["frame_counts"])
    none = solver.guided_match(**{**args, "frame_pose": np.zeros((0, 7)), "frame_range": np.zeros((0, 2), dtype=np.int32), "cand": []},
                               counts=True)
    assert none["n_frames"] == 0 and none["n_rows"] == 0 and none["nn_kp"].shape == (0, 2) and none["n_grids"] == 0
    np.testing.assert_array_equal(none["match_begin"], [0])
    empty = solver.guided_match(**{**args, "cand": [[]] * 5}, counts=True)  # entries without a candidate: nothing is binned
    assert empty["n_rows"] == 0 and empty["n_matches"] == 0
    np.testing.assert_array_equal(empty["frame_counts"][:, 0], [0] * 5)
    np.testing.assert_array_equal(empty["frame_counts"][:, 1], full["frame_counts"][:, 1])
    np.testing.assert_array_equal(empty["match_begin"], [0] * 6)


# ---- end to end ------------------------------------------------------------------------------------------------------

PIPE_KW = dict(max_distance=64)  # test_refgmatch.py's


def test_search_local_map_restores_what_the_reference_restores(solver):
    from miba import sequence, window
    kfs, lms, K0, k, deleted = rg.hidden_links()
    ref_kfs, ref_lms, _, _, _ = rg.hidden_links()
    out = window.search_local_map(k, kfs, lms, K0, sequence.IMAGE_W, sequence.IMAGE_H, solver.guided_match, **PIPE_KW)
    ref = window.search_local_map(k, ref_kfs, ref_lms, K0, sequence.IMAGE_W, sequence.IMAGE_H, rg.cpu_guided, **PIPE_KW)
    assert out["added"] == ref["added"] and kfs[k].global_points_map == ref_kfs[k].global_points_map
    for key in ("nn_kp", "nn_dist", "status", "n_in_window", "matches"):
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    added = dict(out["added"])
    assert len(added) > 150 and all(deleted.get(i) == g for i, g in added.items())


def _problem(kfs, lms, K):
    from miba.capi import ProblemArrays
    ids = sorted(lms)
    row = {g: i for i, g in enumerate(ids)}
    oc = np.concatenate([np.full(len(kf.global_points_map), c) for c, kf in enumerate(kfs)]).astype(np.int32)
    op = np.array([row[g] for kf in kfs for g in kf.global_points_map.values()], dtype=np.int32)
    loc = np.concatenate([kf.points3d_local[list(kf.global_points_map)] for kf in kfs])
    uv = np.concatenate([np.asarray(kf.keypoints, dtype=np.float64)[list(kf.global_points_map)] for kf in kfs])
    return ProblemArrays(np.array([kf.T_w_c for kf in kfs]), np.array([lms[g] for g in ids]), K.copy(), K.copy(), oc, op, uv,
                         loc[:, 2].copy(), fixed_cam=0)


def test_fuse_landmarks_ties_the_two_sweeps_together(solver):
    from miba import matching
    kfs, lms, K, pairs = rg.two_sweeps()
    ref_kfs, ref_lms, _, _ = rg.two_sweeps()
    n_lm = rg.SWEEPS["n_lm"]
    w0 = solver.covisibility(_problem(kfs, lms, K), order=False)["weights"]
    assert all(w0[a, b] == 0 for a, b in pairs)
    merges = matching.fuse_landmarks(kfs, lms, pairs, K, 640, 480, solver.guided_match, **PIPE_KW)
    assert merges == matching.fuse_landmarks(ref_kfs, ref_lms, pairs, K, 640, 480, rg.cpu_guided, **PIPE_KW)
    assert len(merges) > 150 and all(keep % n_lm == drop % n_lm and keep != drop for keep, drop in merges)
    assert [kf.global_points_map for kf in kfs] == [kf.global_points_map for kf in ref_kfs] and set(lms) == set(ref_lms)
    w1 = solver.covisibility(_problem(kfs, lms, K), order=False)["weights"]
    assert all(w1[a, b] > 0 for a, b in pairs)
