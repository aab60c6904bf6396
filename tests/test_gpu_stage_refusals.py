"""The refusals every stage beside the LM loop opens with, through the C ABI: ba_covariance, ba_residuals,
ba_covisibility, ba_local_window and ba_localize refuse a short request, a short info, a context with landmark shards
and (the three that never prepare) a window with bad sizes or an out-of-range index, each with BA_E_INVALID and one
exact ba_last_error text; with two defects at once the earlier check of the fixed order wins (null argument, request
struct_size, info struct_size, landmark shards, then the window).

The expected texts are written out here, not read from the library: they are the public wording of these calls."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BA_E_INVALID = -1
SHARDS = "contexts with landmark shards (ba_comm_init*) are not supported"

# entry point -> (request mirror, info mirror, the stem of its macros, checks the window itself before any prepare)
STAGES = {
    "ba_covariance": ("BaCovRequest", "BaCovInfo", "BA_COV", False),
    "ba_residuals": ("BaResRequest", "BaResInfo", "BA_RES", False),
    "ba_covisibility": ("BaCovisRequest", "BaCovisInfo", "BA_COVIS", True),
    "ba_local_window": ("BaLocalRequest", "BaLocalInfo", "BA_LOCAL", True),
    "ba_localize": ("BaLocRequest", "BaLocInfo", "BA_LOC", True),
}


def below(what, stem):
    macro = f"{stem}_{what.upper()}"
    return f"{what} struct_size below {macro}_MIN_SIZE (set it with {macro}_INIT)"


def window():
    """2 cameras, 3 points, 4 observations (every refusal comes before any of the values is read)."""
    from miba.capi import ProblemArrays
    cams = np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (2, 1))
    cams[1, 4] = 0.1
    pts = np.array([[0.0, 0.0, 2.0], [0.2, 0.1, 2.5], [-0.1, 0.2, 3.0]])
    K = np.array([500.0, 500.0, 320.0, 240.0])
    return ProblemArrays(cams, pts, K, K.copy(), [0, 0, 1, 1], [0, 1, 1, 2], np.full((4, 2), 300.0), np.full(4, 2.0))


def cases():
    """(id, entry point, the defects, the expected message without its prefix)"""
    out = []
    for name, (_, _, stem, own_checks) in STAGES.items():
        out.append((f"{name}-short-request", name, {"req": -1}, below("request", stem)))
        out.append((f"{name}-short-info", name, {"info": -1}, below("info", stem)))
        out.append((f"{name}-shards", name, {"shards": True}, SHARDS))
        if own_checks:
            out.append((f"{name}-negative-n_obs", name, {"n_obs": -1}, "invalid problem sizes"))
            out.append((f"{name}-obs_pt-past-the-end", name, {"bad_pt": True}, "observation index out of range"))
        # two defects: the info's size is judged before anything of the window is
        out.append((f"{name}-short-info-and-bad-index", name, {"info": -1, "bad_pt": True}, below("info", stem)))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def solvers():
    from miba.solver import Solver
    with Solver(minimizer_progress_to_stdout=0) as plain, Solver(minimizer_progress_to_stdout=0) as sharded:
        sharded.comm_init(1, 0, Solver.comm_unique_id())
        yield plain, sharded


@pytest.mark.parametrize("name,defects,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal(solvers, name, defects, expected):
    from miba import capi
    plain, sharded = solvers
    s = sharded if defects.get("shards") else plain
    req_t, info_t = getattr(capi, STAGES[name][0]), getattr(capi, STAGES[name][1])
    req, info = req_t(), info_t()
    if name == "ba_localize":
        req.log_cam = -1
    req.struct_size += defects.get("req", 0)
    info.struct_size += defects.get("info", 0)
    p = window()
    if defects.get("bad_pt"):
        p.obs_pt[2] = p.n_points
    ps = p.struct()
    if "n_obs" in defects:
        ps.n_obs = defects["n_obs"]
    info_size = info.struct_size
    rc = getattr(s._L, name)(s._h, C.byref(ps), C.byref(req), C.byref(info))
    msg = s.last_error()
    print(f"{name} {defects}: rc={rc} error={msg!r}")
    assert rc == BA_E_INVALID
    assert msg == f"{name}: {expected}"
    assert info.struct_size == info_size  # a refused call writes nothing into the info
