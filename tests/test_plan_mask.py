"""The host plan (csrc/ba_plan.cpp) under a set of constant cameras (PlanInput::cam_const, ba_set_constant_cameras).

tests/cpp/plan_mask_main.cpp (linked with ba_plan.cpp alone) prints the plan arrays of a window and a mask:
* without a mask and with an all-zero mask the plan is the same;
* the mask {g} with fixed_cam = -1 gives the plan of fixed_cam = g;
* for masks at the start, in the middle, at the end and on two adjacent cameras: the masked cameras have no active
  index, nac / ac_cam / cam_ac are what the definition says, every admissible observation of a masked camera is still
  in its point's list and in the camera-major order, no overflow slot and no tile window refers to one, and the points'
  first / last active cameras ignore them;
* 1 host thread and 16 give the same plan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from miba import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "plan_mask_main.cpp"), os.path.join(CSRC, "ba_plan.cpp")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

INT_MAX = 2 ** 31 - 1
NC = 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_mask") / "plan_mask_main")
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O2", "-I", CSRC, *SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def prob():
    # tracks of up to 14 cameras (wider than the tile window of 12: overflow points), repeated and inadmissible
    # observations, shuffled
    return synthetic.make_problem(NC, 600, (2, 14), seed=21, shuffle_obs=True, dup_frac=0.05, bad_depth_frac=0.05)


def plan(exe, prob, tmp_path, mask, fixed_cam, threads=4):
    path = str(tmp_path / "window.bin")
    with open(path, "wb") as f:
        np.array([prob.n_cams, prob.n_points, prob.n_obs, fixed_cam, 0 if mask is None else 1], np.int32).tofile(f)
        if mask is not None:
            np.ascontiguousarray(mask, np.uint8).tofile(f)
        np.ascontiguousarray(prob.obs_cam, np.int32).tofile(f)
        np.ascontiguousarray(prob.obs_pt, np.int32).tofile(f)
        np.ascontiguousarray(prob.obs_depth, np.float64).tofile(f)
    r = subprocess.run([exe, path], env=dict(os.environ, MIBA_HOST_THREADS=str(threads)), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "plan_mask_main: ok"
    out = {}
    for l in lines[:-1]:
        name, *vals = l.split(" ")
        out[name] = [int(v) for v in vals]
    return out


def _mask(*idx):
    m = np.zeros(NC, bool)
    m[list(idx)] = True
    return m


MASKS = {"start": _mask(0), "middle": _mask(NC // 2), "end": _mask(NC - 1), "adjacent": _mask(7, 8),
         "start_and_end": _mask(0, NC - 1)}


def test_empty_mask_is_the_plan_without_one(harness, prob, tmp_path):
    for fixed in (0, 9, -1):
        assert plan(harness, prob, tmp_path, None, fixed) == plan(harness, prob, tmp_path, np.zeros(NC, bool), fixed)


@pytest.mark.parametrize("g", [0, NC // 2, NC - 1])
def test_one_camera_mask_is_the_plan_of_fixed_cam(g, harness, prob, tmp_path):
    assert plan(harness, prob, tmp_path, _mask(g), -1) == plan(harness, prob, tmp_path, None, g)
    # the gauge inside the mask changes nothing either
    assert plan(harness, prob, tmp_path, _mask(g), g) == plan(harness, prob, tmp_path, None, g)


@pytest.mark.parametrize("fixed", [-1, 3])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_masked_cameras_are_point_side_only(name, fixed, harness, prob, tmp_path):
    mask = MASKS[name]
    pl = plan(harness, prob, tmp_path, mask, fixed)
    adm = prob.obs_depth > 1e-15
    seen = np.zeros(NC, bool)
    seen[prob.obs_cam[adm]] = True
    active = [c for c in range(NC) if seen[c] and not mask[c] and c != fixed]
    cam_ac = np.full(NC, -1)
    cam_ac[active] = np.arange(len(active))
    n_adm, nac, n_ap, n_tiled, n_ovf, n, cam_band, band_w = pl["scalars"]
    assert n_adm == int(adm.sum()) and nac == len(active) and n == 6 * nac + 4
    assert pl["ac_cam"] == active and pl["cam_ac"] == cam_ac.tolist()
    # the constant cameras' observations still count
    assert pl["cam_cnt"] == np.bincount(prob.obs_cam[adm], minlength=NC).tolist()
    assert pl["pt_cnt"] == np.bincount(prob.obs_pt[adm], minlength=prob.n_points).tolist()
    po, pt_ptr, pt_idx = np.array(pl["po_orig"]), pl["pt_ptr"], pl["pt_idx"]
    assert sorted(po.tolist()) == np.nonzero(adm)[0].tolist()  # every admissible observation, once
    assert sorted(pl["co_orig"]) == np.nonzero(adm)[0].tolist()
    masked_obs = np.nonzero(adm & mask[prob.obs_cam])[0]
    assert len(masked_obs) > 0
    slot_of = np.array(pl["po_dest"])
    for k in masked_obs:  # in its point's list
        a = pt_idx.index(int(prob.obs_pt[k]))
        assert pt_ptr[a] <= slot_of[k] < pt_ptr[a + 1] and po[slot_of[k]] == k
    # first / last active camera of every point over its active observations alone
    lo = np.full(prob.n_points, INT_MAX)
    hi = np.full(prob.n_points, -1)
    on = adm & (cam_ac[prob.obs_cam] >= 0)
    np.minimum.at(lo, prob.obs_pt[on], cam_ac[prob.obs_cam[on]])
    np.maximum.at(hi, prob.obs_pt[on], cam_ac[prob.obs_cam[on]])
    assert pl["pmin"] == lo.tolist() and pl["pmax"] == hi.tolist()
    # no overflow slot refers to a constant camera; every overflow point's active observation is there
    ovf_cams = prob.obs_cam[po[pl["ovf_obs"]]] if pl["ovf_obs"] else np.zeros(0, int)
    assert not mask[ovf_cams].any() and (fixed < 0 or not (ovf_cams == fixed).any())
    want_ovf = [q for q in range(pt_ptr[n_tiled], pt_ptr[n_ap]) if cam_ac[prob.obs_cam[po[q]]] >= 0]
    assert pl["ovf_obs"] == want_ovf and n_ovf == len(want_ovf) and n_ovf > 0
    # a tile's camera window [base, base + span) holds the active cameras of its points and nothing past nac
    tc, ca = pl["tile_chunk"], pl["chunk_ap"]
    assert n_tiled > 0 and ca[tc[-1]] == n_tiled
    for t in range(len(pl["tile_base"])):
        base, span = pl["tile_base"][t], pl["tile_span"][t]
        assert 0 <= base and base + span <= nac and 1 <= span <= 12
        for a in range(ca[tc[t]], ca[tc[t + 1]]):
            i = pt_idx[a]
            assert base <= lo[i] and hi[i] < base + span
            cams = cam_ac[prob.obs_cam[po[pt_ptr[a]: pt_ptr[a + 1]]]]
            assert all(c < 0 or base <= c < base + span for c in cams)
    # the sub-segments carry the constant cameras' observations with active index -1
    for c, a in zip(pl["seg_cam"], pl["seg_ac"]):
        assert a == cam_ac[c]
    assert set(pl["seg_cam"]) == set(np.nonzero(seen)[0].tolist())


def test_thread_count_does_not_change_the_masked_plan(harness, prob, tmp_path):
    for name in ("middle", "adjacent"):
        assert plan(harness, prob, tmp_path, MASKS[name], -1, threads=1) == \
            plan(harness, prob, tmp_path, MASKS[name], -1, threads=16)
