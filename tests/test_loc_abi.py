"""The ABI of ba_localize (no GPU): the ctypes mirrors of ba_loc_request / ba_loc_info against the header compiled by
gcc, the *_INIT / *_MIN_SIZE macros, the declaration and the export, and that the addition left BA_API_VERSION at 2 and
ba_options as it was."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from miba import _lib, capi
from test_capi import ROOT, _c_layout

HEADER = os.path.join(ROOT, "include", "ba.h")


@pytest.mark.parametrize("cls,cname", [("BaLocRequest", "ba_loc_request"), ("BaLocInfo", "ba_loc_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
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
    out = _run_c("ba_loc_request r; ba_loc_info i; r.log_max_rows = 7; r.cam_stats = (double*)&r; i.n_solved = 3;"
                 "BA_LOC_REQUEST_INIT(r); BA_LOC_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.log_max_rows, r.cam_stats == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_LOC_REQUEST_MIN_SIZE, BA_LOC_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d\\n", i.n_solved, BA_API_VERSION, BA_LOC_STAT_N, BA_LOG_WIDTH);')
    rs, rsz, rows, snull, isz_set, isz, rmin, imin, nsolved, ver, nstat, logw = out
    assert rs == rsz == rmin == C.sizeof(capi.BaLocRequest)
    assert isz_set == isz == imin == C.sizeof(capi.BaLocInfo)
    assert rows == 0 and snull == 1 and nsolved == 0
    assert ver == 2
    assert nstat == capi.LOC_STAT_N == len(capi.LOC_STAT_FIELDS) == 8 and logw == _lib.LOG_WIDTH


def test_declaration_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert ("int32_t ba_localize(ba_context* ctx, ba_problem* prob, const ba_loc_request* req, "
            "ba_loc_info* info);") in flat
    assert "ba_localize" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_localize" in text.split("#define BA_API_VERSION")[0]  # the history line


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_localize$", out, flags=re.M)


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
