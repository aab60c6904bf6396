"""tests/refmatch.py checked without a GPU: the reference against a second formulation (popcount table; norms minus
twice the dot product in int64), the neighbours against a plain loop, and that each case family contains what it is
there for (ties of both sorts, every count of the acceptance chain, the largest distances)."""
import numpy as np
import pytest

import refmatch as rm

ALL = [(name, kind) for name in rm.CASES for kind in rm.KINDS]


@pytest.mark.parametrize("name,kind", ALL)
def test_two_formulations_agree(name, kind):
    q, t, pr, _ = rm.case_inputs(name, kind)
    for (a, b, c, d), D in zip(pr, rm.case_distances(name, kind)):
        assert D.dtype == np.int64 and D.shape == (b - a, d - c)
        np.testing.assert_array_equal(D, rm.distances_alt(q[a:b], t[c:d], kind))


@pytest.mark.parametrize("kind", rm.KINDS)
def test_rect_sizes_two_formulations(kind):
    for nbytes in rm.DESC_BYTES[kind]:
        q, t, pr, _ = rm.case_inputs("rect-17x33", kind, nbytes)
        assert q.shape == (17, nbytes) and t.shape == (33, nbytes)
        D = rm.case_distances("rect-17x33", kind, nbytes)[0]
        np.testing.assert_array_equal(D, rm.distances_alt(q, t, kind))
        assert not np.array_equal(D[:, :17], D[:, :17].T)  # a row / column swap cannot pass


def test_top2_is_the_lexicographic_order():
    rng = np.random.default_rng(1)
    D = rng.integers(0, 6, size=(40, 9)).astype(np.int64)  # many ties
    idx, dist = rm.top2(D)
    for q in range(len(D)):
        order = sorted(range(D.shape[1]), key=lambda t: (D[q, t], t))
        assert list(idx[q]) == order[:2] and list(dist[q]) == [D[q, order[0]], D[q, order[1]]]
    idx, dist = rm.top2(D[:, :1])
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all() and (dist[:, 1] == -1).all()
    idx, dist = rm.top2(D[:, :0])
    assert (idx == -1).all() and (dist == -1).all()


def test_the_ratio_tests_are_the_headers():
    # HAMMING in f32: 0.7f * 10 rounds to 7.0f, so 7 fails the strict test and 6 passes
    assert rm.match_pair(np.array([[7, 10]], dtype=np.int64), "hamming", 0.7)[2][0] == 4
    assert rm.match_pair(np.array([[6, 10]], dtype=np.int64), "hamming", 0.7)[2][0] == 2
    # ... and 0.3f is above 0.3, but 0.3f * 10 rounds to 3.0f: 3 fails in f32 where the exact product would let it pass
    assert rm.match_pair(np.array([[3, 10]], dtype=np.int64), "hamming", 0.3)[2][0] == 4
    # L2_U8 on the squares in f64 with the f32 ratio widened: (0.7f)^2 * 100 = 48.9999983..., (0.3f)^2 * 100 > 9
    assert rm.match_pair(np.array([[49, 100]], dtype=np.int64), "l2_u8", 0.7)[2][0] == 4
    assert rm.match_pair(np.array([[48, 100]], dtype=np.int64), "l2_u8", 0.7)[2][0] == 2
    assert rm.match_pair(np.array([[9, 100]], dtype=np.int64), "l2_u8", 0.3)[2][0] == 2
    # equal distances fail at ratio 1
    assert rm.match_pair(np.array([[5, 5]], dtype=np.int64), "hamming", 1.0)[2][0] == 4
    # the order of the chain: the first failed condition counts
    D = np.array([[9, 100], [8, 100]], dtype=np.int64)
    assert list(rm.match_pair(D, "hamming", 0.7, max_distance=5, cross_check=True)[2]) == [5, 5]
    assert list(rm.match_pair(D, "hamming", 0.7, cross_check=True)[2]) == [6, 2]


@pytest.mark.parametrize("kind", rm.KINDS)
def test_tie_cases_contain_ties(kind):
    ref = rm.case_reference("ties-train", kind)
    d, i = ref["nn_dist"], ref["nn_idx"]
    eq = d[:, 0] == d[:, 1]
    assert eq.sum() >= 3 and (i[eq, 0] < i[eq, 1]).all()  # equal (d0, d1): the smaller index first
    assert (ref["accept"][eq] == 0).all() and ref["pair_counts"][0, 4] >= eq.sum()  # ... and the ratio fails at 1.0
    D = rm.case_distances("ties-train", kind)[0]
    firsts = [(D[q] == D[q].min()).sum() for q in range(len(D))]
    assert max(firsts) >= 4  # equal first distances at different indices
    assert (d[:, 0] == 0).any()  # an identical descriptor
    ref = rm.case_reference("ties-query", kind)
    D = rm.case_distances("ties-query", kind)[0]
    assert np.array_equal(D[5], D[6]) and np.array_equal(D[5], D[20]) and np.array_equal(D[0], D[26])
    assert ref["accept"][5] == 1 and not ref["accept"][[6, 11, 20, 26]].any()  # only a group's smallest query can win
    assert ref["pair_counts"][0, 6] >= 4


def test_every_count_is_non_zero_somewhere():
    for kind in rm.KINDS:
        total = np.zeros(rm.COUNT_N, dtype=np.int64)
        per_setting = []
        for ratio, md, cc in rm.ACCEPT_SETTINGS:
            ref = rm.case_reference("accept", kind, ratio=ratio, max_distance=rm.MAX_DISTANCE[kind] if md else 0, cross_check=cc)
            c = ref["pair_counts"]
            assert (c[:, 2:].sum(axis=1) == c[:, 0]).all()
            assert ref["n_matches"] == c[:, 2].sum() == len(ref["matches"]) == ref["accept"].sum()
            total += c.sum(axis=0)
            per_setting.append(c.sum(axis=0))
        print(kind, total)
        assert (total > 0).all()
        full = per_setting[rm.ACCEPT_SETTINGS.index((0.7, True, True))]
        assert (full > 0).all()  # one call that reaches all seven
        # the settings differ in what they accept
        assert len({tuple(c) for c in per_setting}) >= 8


@pytest.mark.parametrize("kind", rm.KINDS)
def test_extremes_reach_the_largest_distances(kind):
    q, t, pr, _ = rm.case_inputs("extreme", kind)
    nbytes = q.shape[1]
    assert nbytes == rm.MAX_BYTES
    ref = rm.case_reference("extreme", kind)
    top = 8 * nbytes if kind == "hamming" else nbytes * 255 * 255
    assert ref["nn_dist"].max() == top and top < 2 ** 31
    assert (ref["nn_dist"][:, 0] == 0).any()
    assert rm.case_distances("extreme", kind)[0].max() == top


@pytest.mark.parametrize("kind", rm.KINDS)
def test_shapes_and_batches_are_what_they_say(kind):
    for name in ("shapes-q", "shapes-t", "shapes-square"):
        pr = rm.case_inputs(name, kind)[2]
        assert len(pr) == len(rm.EDGE_SIZES) == 10
    assert rm.EDGE_SIZES == [0, 1, 2, 3, 15, 16, 17, 63, 64, 65]
    assert {len(rm.case_inputs(n, kind)[2]) for n in ("batch-1", "batch-2", "batch-9")} == {1, 2, 9}
    pr = rm.case_inputs("batch-9", kind)[2]
    assert ((pr[:, 1] == pr[:, 0]).any() and (pr[:, 3] == pr[:, 2]).any())  # empty pairs
    assert pr[0, 1] > pr[1, 0] and pr[0, 3] > pr[1, 2]  # overlapping ranges
    pr = rm.case_inputs("one-vs-five", kind)[2]
    assert len(pr) == 5 and (pr[:, 0] == 0).all() and (pr[:, 1] == pr[0, 1]).all()
    pr = rm.case_inputs("slices", kind)[2]
    assert pr[0, 3] > 2 * rm.TTILE and pr[0, 1] > rm.QTILE


def test_the_matcher_recovers_the_shared_landmarks():
    """Two keyframes of 500 features with 350 shared landmarks, 256-bit descriptors, 6 % of the bits flipped per
    observation: the reference matcher finds all 350 and no wrong pair (a property of such inputs, on five seeds)."""
    for seed in range(5):
        da, db, ia, ib = rm.two_keyframes(seed)
        ref = rm.match(da, db, [[0, 500, 0, 500]], "hamming")
        m = ref["matches"]
        assert len(m) == 350 and (ia[m[:, 0]] == ib[m[:, 1]]).all()
