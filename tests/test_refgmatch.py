"""tests/refgmatch.py checked on the CPU: the reference (every keypoint of the range, no grid) against its second
statement (the keypoints binned into cells, the window's cell rectangle, a running best two) at every cell size; that
no floating-point decision of any case is within 1e-6, relative, of its threshold, so the GPU comparison can be exact;
that the cases reach every status and every candidate count; that the counts add up; and that the two pipeline
fixtures (the hidden links, the two sweeps) meet their conditions under the reference alone."""
import numpy as np
import pytest

import refgmatch as rg
import refmatch as rm

SIMPLE = [n for n in rg.CASES if n != "accept"]


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("name", list(rg.CASES))
def test_margins_and_counts(name, kind):
    args, kw = rg.case_inputs(name, kind)
    ref = rg.case_reference(name, kind)
    print(f"GMATCH-REF {name} {kind} rows={ref['n_rows']} margin={ref['margin']:.3e}")
    assert ref["margin"] >= rg.MIN_MARGIN
    c = ref["frame_counts"]
    assert (c[:, 2:].sum(axis=1) == c[:, 0]).all() and ref["n_matches"] == c[:, 2].sum() == len(ref["matches"])
    assert (np.diff(ref["cand_begin"]) == c[:, 0]).all() and ref["match_begin"][-1] == ref["n_matches"]
    st = ref["status"]
    assert ((ref["nn_kp"][:, 0] >= 0) == (st >= rg.RATIO) | (st == rg.ACCEPTED)).all()
    assert ((ref["n_in_window"] == 0) == (ref["nn_kp"][:, 0] < 0)).all()
    assert ((ref["n_in_window"] >= 2) == (ref["nn_kp"][:, 1] >= 0)).all()
    assert (ref["proj"][st == rg.BEHIND, :2] == 0).all()


@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("name", list(rg.CASES))
def test_reference_agrees_with_the_grid_statement(name, kind):
    args, kw = rg.case_inputs(name, kind)
    ref = rg.case_reference(name, kind)
    for cell in (0,) + (rg.CELLS if name in ("small", "boundaries", "borders", "crowd") else ()):
        alt = rg.guided_grid(**args, kind=kind, **{**kw, **({"cell_px": cell} if cell else {})})
        for key in rg.INT_ARRAYS:
            np.testing.assert_array_equal(alt[key], ref[key], err_msg=f"{key} at cell {cell}")
        assert np.array_equal(alt["proj"], ref["proj"], equal_nan=True)


@pytest.mark.parametrize("kind", rm.KINDS)
def test_the_acceptance_settings_reach_every_status(kind):
    seen = set()
    args, kw = rg.case_inputs("accept", kind)
    for setting in rg.ACCEPT_SETTINGS:
        over = rg.accept_kw(kind, *setting)
        ref = rg.case_reference("accept", kind, **over)
        assert ref["margin"] >= rg.MIN_MARGIN
        c = ref["frame_counts"][0]
        seen |= set(ref["status"].tolist())
        assert (c[2 + rg.MAX_DISTANCE] > 0) == (over["max_distance"] > 0)
        assert over["one_to_one"] or c[2 + rg.ONE_TO_ONE] == 0
    assert seen == set(range(7))
    # each switch changes something
    base = rg.case_reference("accept", kind, **rg.accept_kw(kind, 0.7, False, 0.0, False))
    for setting in ((1.0, False, 0.0, False), (0.7, True, 0.0, False), (0.7, False, 0.1, False), (0.7, False, 0.0, True)):
        other = rg.case_reference("accept", kind, **rg.accept_kw(kind, *setting))
        assert other["status"].tobytes() != base["status"].tobytes(), setting
    gated = rg.case_reference("accept", kind, **rg.accept_kw(kind, 0.7, False, 0.1, False))
    assert (gated["n_in_window"] <= base["n_in_window"]).all() and (gated["n_in_window"] < base["n_in_window"]).any()


def test_the_cases_reach_their_limits():
    for kind in rm.KINDS:
        assert tuple(np.diff(rg.case_reference("cand-counts", kind)["cand_begin"])) == rg.CAND_COUNTS
        c = rg.case_reference("empty", kind)["frame_counts"]
        assert (c[:, 0] == 0).any() and (c[:, 1] == 0).any() and ((c[:, 0] > 0) & (c[:, 1] > 0)).any()
        assert (c[c[:, 1] == 0, 2 + rg.ACCEPTED] == 0).all()
        crowd = rg.case_reference("crowd", kind)
        assert crowd["n_in_window"][0] == 300 and list(crowd["nn_kp"][0]) == [117, 250] and crowd["nn_dist"][0, 0] == crowd["nn_dist"][0, 1]
        assert crowd["status"][0] == rg.RATIO
        ties = rg.case_reference("ties", kind)
        rows = {int(p): r for r, p in enumerate(ties["cand_pt"])}
        assert list(ties["nn_kp"][rows[0]]) == [0, 1] and ties["status"][rows[0]] == rg.RATIO
        assert ties["nn_kp"][rows[3], 0] == ties["nn_kp"][rows[4], 0] == ties["nn_kp"][rows[5], 0] == ties["nn_kp"][rows[6], 0] == 5
        assert ties["nn_dist"][rows[3], 0] == ties["nn_dist"][rows[5], 0] < ties["nn_dist"][rows[6], 0]
        # rows 1, 2, 3 hold landmarks 5, 3, 4: the smallest row wins the tie
        assert [ties["status"][rows[p]] for p in (5, 3, 4, 6)] == [rg.ACCEPTED, rg.ONE_TO_ONE, rg.ONE_TO_ONE, rg.ONE_TO_ONE]
        borders = rg.case_reference("borders", kind)
        assert (borders["n_in_window"] >= 2).all()  # a keypoint inside the image and one outside it, in every window
        wide = rg.case_reference("wide", kind)
        assert wide["n_in_window"].max() > 20
        args, kw = rg.case_inputs("boundaries", kind)
        assert kw["radius"] < rg.MIN_CELL and (args["kp_uv"][::4] % 8 == 0).all()
        hyp = rg.case_reference("hypotheses", kind)
        assert len(set(hyp["status"].reshape(5, -1).tobytes()[i * 80:(i + 1) * 80] for i in range(5))) > 1
        view = rg.case_reference("all-in-view", kind)
        args, kw = rg.case_inputs("all-in-view", kind)
        assert (view["n_in_window"] == len(args["kp_uv"])).all()
        m = rm.match(args["pt_desc"], args["kp_desc"], [[0, len(args["pt_desc"]), 0, len(args["kp_uv"])]], kind)
        np.testing.assert_array_equal(view["nn_kp"], m["nn_idx"])
        np.testing.assert_array_equal(view["nn_dist"], m["nn_dist"])
    assert W_NOT_A_MULTIPLE


W_NOT_A_MULTIPLE = all(rg.W0 % c and rg.H0 % c for c in rg.CELLS)


def test_a_frame_does_not_depend_on_the_other_frames():
    """Five hypotheses in one call are, row for row, the five separate calls."""
    args, kw = rg.case_inputs("hypotheses", "hamming")
    ref = rg.case_reference("hypotheses", "hamming")
    for f in range(5):
        one = rg.guided(**{**args, "frame_pose": args["frame_pose"][f:f + 1]}, kind="hamming", **kw)
        a, b = ref["cand_begin"][f], ref["cand_begin"][f + 1]
        for key in ("nn_kp", "nn_dist", "status", "n_in_window"):
            np.testing.assert_array_equal(one[key], ref[key][a:b])
        np.testing.assert_array_equal(one["matches"], ref["matches"][ref["match_begin"][f]:ref["match_begin"][f + 1]])


# ---- the pipeline fixtures under the reference alone ----------------------------------------------------------------

PIPE_KW = dict(max_distance=64)  # of 256 bits: a copy is some 30 bits off, a random descriptor some 128


def test_search_local_map_restores_the_hidden_links():
    from miba import sequence, window
    kfs, lms, K0, k, deleted = rg.hidden_links()
    before = dict(kfs[k].global_points_map)
    out = window.search_local_map(k, kfs, lms, K0, sequence.IMAGE_W, sequence.IMAGE_H, rg.cpu_guided, **PIPE_KW)
    assert out["margin"] >= rg.MIN_MARGIN
    added = dict(out["added"])
    assert len(deleted) > 150 and len(added) == out["n_matches"]
    assert all(deleted.get(i) == g for i, g in added.items())  # no restored link differs from the deleted truth
    assert kfs[k].global_points_map == {**before, **added}
    # of the deleted links whose landmark still projects into the image, at least 90 % come back
    u, v, z = rg.project(np.array([lms[g] for g in deleted.values()]), kfs[k].T_w_c, K0)
    in_image = int(((z > 1e-15) & (u >= 0) & (u < sequence.IMAGE_W) & (v >= 0) & (v < sequence.IMAGE_H)).sum())
    print(f"GMATCH-HIDDEN deleted={len(deleted)} in_image={in_image} restored={len(added)}")
    assert in_image > 150 and len(added) >= 0.9 * in_image
    # the range was the free keypoints alone
    assert out["frame_counts"][0, 1] == len(kfs[k].keypoints) - len(before) and out["n_rows"] >= len(deleted)
    assert window.search_local_map(0, kfs, lms, K0, sequence.IMAGE_W, sequence.IMAGE_H, rg.cpu_guided) is None


def test_fuse_landmarks_joins_the_two_sweeps():
    from miba import matching
    kfs, lms, K, pairs = rg.two_sweeps()
    n_lm = rg.SWEEPS["n_lm"]
    assert [rg.shared_ids(kfs, a, b) for a, b in pairs] == [0, 0, 0]
    merges = matching.fuse_landmarks(kfs, lms, pairs, K, 640, 480, rg.cpu_guided, **PIPE_KW)
    assert len(merges) > 150 and all(keep % n_lm == drop % n_lm and keep != drop for keep, drop in merges)
    assert all(drop not in lms and keep in lms for keep, drop in merges)
    ids = {g for kf in kfs for g in kf.global_points_map.values()}
    assert ids <= set(lms) and not ids & {drop for _, drop in merges}
    assert all(rg.shared_ids(kfs, a, b) > 50 for a, b in pairs)
    assert matching.fuse_landmarks(kfs, lms, np.zeros((0, 2), dtype=int), K, 640, 480, rg.cpu_guided) == []


def test_landmark_descriptors_and_the_pipeline_switch():
    import inspect
    from miba import matching, sequence
    kfs, lms, K0, k, deleted = rg.hidden_links()
    ids, desc = matching.landmark_descriptors(kfs)
    assert ids.dtype == np.int64 and desc.dtype == np.uint8 and desc.shape == (len(ids), 32) and len(set(ids.tolist())) == len(ids)
    assert set(ids.tolist()) == {g for kf in kfs for g in kf.global_points_map.values()}
    first = {}
    for kf in kfs:
        for i, g in kf.global_points_map.items():
            first.setdefault(g, kf.descriptors[i])
    assert all(np.array_equal(desc[j], first[int(g)]) for j, g in enumerate(ids))
    assert inspect.signature(sequence.run_pipeline).parameters["search"].default is None
