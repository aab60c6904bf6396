"""tests/reflocal.py, the selection reference of the local-window tests, on hand-written maps whose answers are
written out literally."""
import numpy as np

import reflocal


def _check(sel, **want):
    for k, v in want.items():
        got = sel[k]
        if isinstance(v, list):
            assert np.asarray(got).astype(int).tolist() == [int(x) for x in v], (k, got, v)
        else:
            assert int(got) == v, (k, got, v)


def test_tie_at_the_max_local_cut():
    # camera 0 sees points 0..3; cameras 1 and 2 share two of them each, camera 3 one, camera 4 none
    obs = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 2), (2, 3), (3, 0), (4, 4)]
    p = reflocal.from_lists(5, 5, obs)
    sel = reflocal.select(p, 0, min_weight=1, max_local=2)
    # the cut keeps one camera beside the centre: 1 and 2 tie at weight 2, the lower index wins
    _check(sel, w=[4, 2, 2, 1, 0], n_local=2, n_fixed=2, n_points=4, n_obs=9, sub_fixed_cam=-1,
           cam_index=[0, 1, 2, 3], cam_local=[1, 1, 0, 0], cam_constant=[0, 0, 1, 1], pt_index=[0, 1, 2, 3],
           obs_index=[0, 1, 2, 3, 4, 5, 6, 7, 8], sub_obs_cam=[0, 0, 0, 0, 1, 1, 2, 2, 3],
           sub_obs_pt=[0, 1, 2, 3, 0, 1, 2, 3, 0])
    # without the cap all three co-visible cameras are local, nothing is fixed and the lowest local camera is the gauge
    sel = reflocal.select(p, 0, min_weight=1, max_local=0)
    _check(sel, n_local=4, n_fixed=0, sub_fixed_cam=0, cam_index=[0, 1, 2, 3], cam_constant=[0, 0, 0, 0])
    # max_local = 3 takes both of the tie and leaves camera 3 fixed
    sel = reflocal.select(p, 0, min_weight=1, max_local=3)
    _check(sel, n_local=3, n_fixed=1, cam_index=[0, 1, 2, 3], cam_local=[1, 1, 1, 0], cam_constant=[0, 0, 0, 1])
    # min_weight = 2 leaves camera 3 out of L; it still sees point 0 of P
    sel = reflocal.select(p, 0, min_weight=2)
    _check(sel, n_local=3, n_fixed=1, cam_local=[1, 1, 1, 0])
    # the map's gauge inside the window is constant
    p.fixed_cam = 1
    sel = reflocal.select(p, 0, min_weight=1, max_local=0)
    _check(sel, sub_fixed_cam=-1, cam_constant=[0, 1, 0, 0])
    # a context mask that intersects L
    p.fixed_cam = -1
    sel = reflocal.select(p, 0, min_weight=1, max_local=0, mask=np.array([0, 0, 1, 0, 1], bool))
    _check(sel, sub_fixed_cam=-1, cam_constant=[0, 0, 1, 0])


def test_inadmissible_observation_does_not_make_a_fixed_camera():
    # camera 2 sees point 1 (a point of P) only at depth 0, and point 2 admissibly
    obs = [(0, 0), (0, 1), (1, 0), (2, 1, 0.0), (2, 2), (1, 1, -np.inf)]
    p = reflocal.from_lists(3, 3, obs)
    sel = reflocal.select(p, 0, min_weight=1)
    _check(sel, w=[2, 1, 0], n_local=2, n_fixed=0, n_points=2, n_obs=3, sub_fixed_cam=0, cam_index=[0, 1],
           cam_constant=[0, 0], pt_index=[0, 1], obs_index=[0, 1, 2], sub_obs_cam=[0, 0, 1], sub_obs_pt=[0, 1, 0])


def test_repeated_observation_counts_once():
    obs = [(0, 0), (0, 0), (1, 0), (1, 0), (1, 0), (1, 1)]
    p = reflocal.from_lists(2, 2, obs)
    sel = reflocal.select(p, 0, min_weight=1)
    # P is the OR of L's rows: camera 1 is local, so its point 1 is local too; every repeated observation is kept
    _check(sel, w=[1, 1], n_local=2, n_fixed=0, n_points=2, n_obs=6, obs_index=[0, 1, 2, 3, 4, 5],
           sub_obs_pt=[0, 0, 0, 0, 0, 1])
    sel = reflocal.select(p, 0, min_weight=2)  # above every weight: L = {centre}, camera 1 sees point 0: fixed
    _check(sel, n_local=1, n_fixed=1, n_points=1, n_obs=5, cam_constant=[0, 1], sub_fixed_cam=-1,
           obs_index=[0, 1, 2, 3, 4])


def test_centre_without_observations():
    p = reflocal.from_lists(3, 2, [(1, 0), (2, 0), (0, 1, 0.0)])
    sel = reflocal.select(p, 0)
    _check(sel, w=[0, 0, 0], n_local=1, n_fixed=0, n_points=0, n_obs=0, sub_fixed_cam=0, cam_index=[0],
           cam_constant=[0], pt_index=[], obs_index=[])


def test_sub_problem_and_scatter_back():
    p = reflocal.make_map(9, 40, 200, seed=3)
    p.cams[:, 4] = np.arange(9)
    sel = reflocal.select(p, 4, min_weight=1, max_local=3)
    sub = reflocal.sub_problem(p, sel)
    assert sub.n_cams == sel["n_local"] + sel["n_fixed"] and sub.n_points == sel["n_points"]
    np.testing.assert_array_equal(sub.cams[:, 4], sel["cam_index"])
    np.testing.assert_array_equal(sel["cam_index"][sub.obs_cam], p.obs_cam[sel["obs_index"]])
    np.testing.assert_array_equal(sel["pt_index"][sub.obs_pt], p.obs_pt[sel["obs_index"]])
    assert (sub.obs_depth > 1e-15).all()
    q = p.copy()
    sub.cams[:, 5] = 7.0
    sub.points[:] = 1.0
    reflocal.scatter_back(q, sel, sub)
    moved = np.zeros(9, bool)
    moved[sel["cam_index"][sel["cam_local"] & ~sel["cam_constant"]]] = True
    np.testing.assert_array_equal(q.cams[:, 5] == 7.0, moved)
    inP = np.zeros(40, bool)
    inP[sel["pt_index"]] = True
    np.testing.assert_array_equal((q.points == 1.0).all(1), inP)
