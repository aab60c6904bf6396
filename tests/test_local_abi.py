"""The ABI of the constant-camera and local-window entry points (no GPU): the ctypes mirrors of ba_local_request /
ba_local_info against the header compiled by gcc, the *_INIT / *_MIN_SIZE macros, the three declarations, and that the
addition left BA_API_VERSION at 2 and ba_options as it was."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from miba import _lib, capi
from test_capi import ROOT, _c_layout

HEADER = os.path.join(ROOT, "include", "ba.h")


@pytest.mark.parametrize("cls,cname", [(capi.BaLocalRequest, "ba_local_request"), (capi.BaLocalInfo, "ba_local_info")])
def test_struct_layout_matches_header(cls, cname):
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    assert names[0] == "struct_size" and cls().struct_size == size


def _run_c(body):
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"ba.h\"\nint main(void){" + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "m.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "m")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return [int(x) for x in subprocess.check_output([exe]).split()]


def test_init_and_min_size_macros():
    out = _run_c("ba_local_request r; ba_local_info i; r.center = 7; r.w = (int32_t*)&r; i.n_obs = 3;"
                 "BA_LOCAL_REQUEST_INIT(r); BA_LOCAL_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.center, r.w == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_LOCAL_REQUEST_MIN_SIZE, BA_LOCAL_INFO_MIN_SIZE);"
                 'printf("%d %d\\n", i.n_obs, BA_API_VERSION);')
    rs, rsz, center, wnull, isz_set, isz, rmin, imin, nobs, ver = out
    assert rs == rsz == rmin == C.sizeof(capi.BaLocalRequest)
    assert isz_set == isz == imin == C.sizeof(capi.BaLocalInfo)
    assert center == 0 and wnull == 1 and nobs == 0
    assert ver == 2


def test_declarations_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int32_t ba_set_constant_cameras(ba_context* ctx, const uint8_t* is_constant, int32_t n_cams);" in flat
    assert ("int32_t ba_local_window(ba_context* ctx, const ba_problem* prob, const ba_local_request* req, "
            "ba_local_info* info);") in flat
    assert ("int32_t ba_solve_local(ba_context* ctx, ba_problem* prob, const ba_local_request* req, "
            "ba_local_info* info, ba_summary* summary);") in flat
    for name in ("ba_set_constant_cameras", "ba_local_window", "ba_solve_local"):
        assert name in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_set_constant_cameras" in open(HEADER).read().split("#define BA_API_VERSION")[0]  # the history line


def test_ba_options_is_unchanged():
    names = [n for n, _ in capi.BaOptions._fields_]
    assert names == ["hub_p_repr", "hub_p_unpr", "weight_intrinsics", "weight_unpr", "max_num_iterations",
                     "minimizer_progress_to_stdout", "eta", "initial_trust_region_radius", "max_trust_region_radius",
                     "min_trust_region_radius", "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal",
                     "max_num_consecutive_invalid_steps", "jacobi_scaling", "function_tolerance", "gradient_tolerance",
                     "parameter_tolerance", "device", "deterministic", "profile_kernels", "profile_mask",
                     "shard_min_obs", "small_window", "rebuild_plan", "reserved"]
    size, offs = _c_layout("ba_options", names)
    assert size == 160 == C.sizeof(capi.BaOptions)
    assert offs[-1] == 156 and offs[names.index("device")] == 128
