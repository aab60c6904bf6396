"""The ABI of ba_match (no GPU): the ctypes mirrors of ba_match_problem / ba_match_request / ba_match_info against the
header compiled by gcc, the *_INIT / *_MIN_SIZE macros and the constants, the declaration and the export, that the
addition left BA_API_VERSION at 2, that tests/refmatch.py's tile sizes are the kernels', and the Python side of the
stage that needs no device (miba.matching on plain arrays, the KeyFrame field, the settings table's row)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import refmatch as rm
from miba import _lib, capi, matching, sequence, window
from test_capi import ROOT, _c_layout
from test_loc_abi import _run_c

HEADER = os.path.join(ROOT, "include", "ba.h")
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")


@pytest.mark.parametrize("cls,cname", [("BaMatchProblem", "ba_match_problem"), ("BaMatchRequest", "ba_match_request"),
                                       ("BaMatchInfo", "ba_match_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    if cname != "ba_match_problem":  # the sized structs lead with their size
        assert names[0] == "struct_size" and cls().struct_size == size


def test_init_and_min_size_macros():
    out = _run_c("ba_match_request r; ba_match_info i; r.cross_check = 7; r.ratio = 3.0f; r.nn_idx = (int32_t*)&r; r.max_distance = 5;"
                 "i.n_matches = 3; BA_MATCH_REQUEST_INIT(r); BA_MATCH_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.cross_check, r.nn_idx == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_MATCH_REQUEST_MIN_SIZE, BA_MATCH_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d %d %d\\n", i.n_matches, BA_API_VERSION, BA_MATCH_COUNT_N, BA_MATCH_MAX_BYTES, r.ratio == 0.0f,'
                 "r.max_distance);"
                 'printf("%d %d %d\\n", BA_MATCH_HAMMING, BA_MATCH_L2_U8, (int)offsetof(ba_match_info, time_kernels_ms));')
    rs, rsz, cc, pnull, isz_set, isz, rmin, imin, nm, ver, ncount, maxb, ratio0, md, ham, l2, off = out
    assert rs == rsz == rmin == C.sizeof(capi.BaMatchRequest)
    assert isz_set == isz == C.sizeof(capi.BaMatchInfo)
    assert imin == off == capi.BaMatchInfo.time_kernels_ms.offset  # the counts; the timings are optional
    assert cc == 0 and pnull == 1 and nm == 0 and ratio0 == 1 and md == 0
    assert ver == 2
    assert ncount == capi.MATCH_COUNT_N == rm.COUNT_N == len(capi.MATCH_COUNT_FIELDS) == 7
    assert maxb == capi.MATCH_MAX_BYTES == rm.MAX_BYTES == 256
    assert (ham, l2) == (capi.MATCH_HAMMING, capi.MATCH_L2_U8) == (rm.HAMMING, rm.L2_U8) == (0, 1)
    assert capi.MATCH_KINDS == rm.KIND_ID and tuple(capi.MATCH_KINDS) == rm.KINDS


def test_declaration_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert ("int32_t ba_match(ba_context* ctx, const ba_match_problem* prob, const ba_match_request* req, "
            "ba_match_info* info);") in flat
    assert "ba_match" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_match" in text.split("#define BA_API_VERSION")[0]  # the history line
    assert flat.index("int32_t ba_align(") < flat.index("int32_t ba_match(") < flat.index("int32_t ba_debug_linearize(")


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_match$", out, flags=re.M)


def _constant(path, name):
    m = re.search(rf"static constexpr int {name} = (\d+);", open(os.path.join(CSRC, path)).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def test_reference_sizes_are_the_kernels():
    assert _constant("ba_match.h", "MATCH_QTILE") == rm.QTILE
    assert _constant("ba_match.h", "MATCH_TTILE") == rm.TTILE
    assert _constant("ba_match.h", "MATCH_MFMA") == rm.MFMA
    assert _constant("ba_match.h", "MATCH_KSTEP") == rm.KSTEP
    assert _constant("ba_match.h", "MATCH_MAX_SLICES") == rm.MAX_SLICES
    assert _constant("ba_match.h", "MATCH_COUNT") == rm.COUNT_N
    assert _constant("ba_match.h", "MATCH_TPB_HAMMING") == 64 and _constant("ba_match.h", "MATCH_SCAN_TPB") == 256
    # the sizes the GPU cases run at surround every one of them
    for t in (rm.QTILE, rm.TTILE, rm.MFMA):
        assert {t - 1, t, t + 1} <= set(rm.EDGE_SIZES)
    assert any(b % rm.KSTEP for b in rm.DESC_BYTES["l2_u8"]) and rm.MAX_BYTES % rm.KSTEP == 0


def test_the_slices_setting_is_in_the_table_and_the_sources_in_the_makefile():
    assert '"MIBA_MATCH_SLICES"' in open(os.path.join(CSRC, "ba_settings.cpp")).read()
    mk = open(os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    runtime = re.search(r"^RUNTIME := (.*)$", mk, flags=re.M).group(1).split()
    assert "ba_match" in kernels and "ba_match" in runtime


def test_solver_match_signature():
    from miba.solver import Solver
    sig = inspect.signature(Solver.match)
    want = dict(pair_range=None, kind="hamming", ratio=0.7, max_distance=0, cross_check=False, matches=True, counts=False)
    assert list(sig.parameters)[:3] == ["self", "query", "train"]
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want


# ---- miba.matching on plain arrays (the reference matcher stands in for Solver.match) ----

def cpu_match(query, train, pair_range=None, kind="hamming", **kw):
    pr = [[0, len(query), 0, len(train)]] if pair_range is None else pair_range
    return rm.match(np.asarray(query), np.asarray(train), pr, kind, **kw)


def test_keyframe_has_an_optional_trailing_descriptors_field():
    import dataclasses
    names = [f.name for f in dataclasses.fields(window.KeyFrame)]
    assert names[-1] == "descriptors" and names[:5] == ["T_w_c", "keypoints", "points3d_local", "global_points_map", "timestamp"]
    kf = window.KeyFrame(np.zeros(7), np.zeros((0, 2)), np.zeros((0, 3)))
    assert kf.descriptors is None
    assert inspect.signature(window.track_keyframe).parameters["match"].default is None
    assert inspect.signature(sequence.run_pipeline).parameters["match"].default is None


@pytest.mark.parametrize("kind", rm.KINDS)
def test_attach_descriptors_leaves_the_sequence_alone_and_matches_by_landmark(kind):
    seq = dict(n_keyframes=4, n_landmarks=300, seed=2)
    kfs, lms, K0, gt = sequence.make_tum_sequence(**seq)
    ref, ref_lms, _, ref_gt = sequence.make_tum_sequence(**seq)
    flip = 0.06 if kind == "hamming" else 8.0
    assert matching.attach_descriptors(kfs, seed=7, kind=kind, flip=flip) is kfs
    for a, b in zip(kfs, ref):  # an RNG of its own: nothing else of the sequence moved
        assert b.descriptors is None and a.descriptors.shape == (len(a.keypoints), matching.DEFAULT_BYTES[kind])
        assert a.descriptors.dtype == np.uint8 and a.keypoints.tobytes() == b.keypoints.tobytes()
        assert a.points3d_local.tobytes() == b.points3d_local.tobytes() and a.global_points_map == b.global_points_map
        assert a.T_w_c.tobytes() == b.T_w_c.tobytes()
    assert gt == ref_gt and all(np.array_equal(lms[i], ref_lms[i]) for i in lms)
    again, _, _, _ = sequence.make_tum_sequence(**seq)
    matching.attach_descriptors(again, seed=7, kind=kind, flip=flip)
    assert all(a.descriptors.tobytes() == b.descriptors.tobytes() for a, b in zip(kfs, again))
    # the matches of two consecutive keyframes are observations of one landmark, and most shared landmarks are found
    a, b = kfs[1], kfs[2]
    out = cpu_match(a.descriptors, b.descriptors, kind=kind)
    m = out["matches"]
    shared = set(a.global_points_map.values()) & set(b.global_points_map.values())
    assert len(m) >= 0.9 * len(shared) > 50
    assert all(a.global_points_map.get(int(q)) == b.global_points_map.get(int(t)) is not None for q, t in m)
    # correspondences: the matched local points, without those that have no depth
    p1, p2 = matching.correspondences(out, 0, a.points3d_local, b.points3d_local)
    keep = (a.points3d_local[m[:, 0], 2] > 1e-15) & (b.points3d_local[m[:, 1], 2] > 1e-15)
    np.testing.assert_array_equal(p1, a.points3d_local[m[keep, 0]])
    np.testing.assert_array_equal(p2, b.points3d_local[m[keep, 1]])
    # ... which are track_matches' pairs, found without the ids
    q1, q2, ids = window.track_matches(2, kfs)
    assert len(p1) >= 0.9 * len(q1)
    assert {tuple(r) for r in p2} <= {tuple(r) for r in q2}


def test_track_keyframe_takes_the_matcher_only_with_descriptors():
    import refalign
    align = lambda p1, p2, **kw: refalign.align(p1, p2, None, **kw)  # noqa: E731
    seq = dict(n_keyframes=4, n_landmarks=300, seed=2)
    kfs, lms, _, _ = sequence.make_tum_sequence(**seq)
    calls = []

    def hook(q, t, **kw):
        calls.append((len(q), len(t)))
        return cpu_match(q, t, **kw)

    plain = window.track_keyframe(2, kfs, dict(lms), align, seed=1)
    kfs2, lms2, _, _ = sequence.make_tum_sequence(**seq)
    same = window.track_keyframe(2, kfs2, lms2, align, match=hook, seed=1)  # no descriptors: the ids, as before
    assert not calls and same["poses"].tobytes() == plain["poses"].tobytes()
    kfs3, lms3, _, _ = sequence.make_tum_sequence(**seq)
    matching.attach_descriptors(kfs3, seed=7)
    out = window.track_keyframe(2, kfs3, lms3, align, match=hook, seed=1)
    assert calls == [(len(kfs3[1].keypoints), len(kfs3[2].keypoints))] and out["tracked"]
    p1, p2 = matching.correspondences(cpu_match(kfs3[1].descriptors, kfs3[2].descriptors), 0, kfs3[1].points3d_local,
                                      kfs3[2].points3d_local)
    assert out["poses"].tobytes() == refalign.align(p1, p2, None, seed=1)["poses"].tobytes()
