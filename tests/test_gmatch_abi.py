"""The ABI of ba_guided_match (no GPU): the ctypes mirrors of ba_gmatch_problem / ba_gmatch_request / ba_gmatch_info
against the header compiled by gcc, the *_INIT / *_MIN_SIZE macros and the constants, the declaration, its place in the
header and the export, that the addition left BA_API_VERSION at 2 and added no MIBA_* setting, that
tests/refgmatch.py's constants are the stage's, and the host side that needs no device: tests/cpp/gmatch_host_main.cpp
over csrc/ba_gmatch_host.h (the refusals in their order, the de-duplication of equal ranges, the cell rectangle against
a brute-force superset check), built with g++ plain and with -fsanitize=address,undefined and run as a program."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

import refgmatch as rg
from miba import _lib, capi
from test_capi import ROOT, _c_layout
from test_loc_abi import _run_c

HEADER = os.path.join(ROOT, "include", "ba.h")
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")
DECL = ("int32_t ba_guided_match(ba_context* ctx, const ba_gmatch_problem* prob, const ba_gmatch_request* req, "
        "ba_gmatch_info* info);")


@pytest.mark.parametrize("cls,cname", [("BaGmatchProblem", "ba_gmatch_problem"), ("BaGmatchRequest", "ba_gmatch_request"),
                                       ("BaGmatchInfo", "ba_gmatch_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    if cname != "ba_gmatch_problem":  # the sized structs lead with their size
        assert names[0] == "struct_size" and cls().struct_size == size


def test_init_and_min_size_macros():
    out = _run_c("ba_gmatch_request r; ba_gmatch_info i; r.one_to_one = 7; r.radius = 3.0; r.nn_kp = (int32_t*)&r; r.cell_px = 5;"
                 "i.n_matches = 3; BA_GMATCH_REQUEST_INIT(r); BA_GMATCH_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.one_to_one, r.nn_kp == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_GMATCH_REQUEST_MIN_SIZE, BA_GMATCH_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d %d %d\\n", i.n_matches, BA_API_VERSION, BA_GMATCH_COUNT_N, BA_MATCH_MAX_BYTES, r.radius == 0.0,'
                 "r.cell_px);"
                 'printf("%d\\n", (int)offsetof(ba_gmatch_info, time_kernels_ms));')
    rs, rsz, oo, pnull, isz_set, isz, rmin, imin, nm, ver, ncount, maxb, radius0, cell, off = out
    assert rs == rsz == rmin == C.sizeof(capi.BaGmatchRequest)
    assert isz_set == isz == C.sizeof(capi.BaGmatchInfo)
    assert imin == off == capi.BaGmatchInfo.time_kernels_ms.offset  # the counts; the timings are optional
    assert oo == 0 and pnull == 1 and nm == 0 and radius0 == 1 and cell == 0
    assert ver == 2 and maxb == 256
    assert ncount == capi.GMATCH_COUNT_N == rg.COUNT_N == len(capi.GMATCH_COUNT_FIELDS) == 9
    assert capi.GMATCH_STATUS == dict(accepted=rg.ACCEPTED, behind=rg.BEHIND, outside=rg.OUTSIDE, empty_window=rg.EMPTY,
                                      ratio=rg.RATIO, max_distance=rg.MAX_DISTANCE, one_to_one=rg.ONE_TO_ONE)


def test_declaration_order_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert DECL in flat
    assert "ba_guided_match" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_guided_match" in text.split("#define BA_API_VERSION")[0]  # the history line
    assert flat.index("int32_t ba_match(") < flat.index("int32_t ba_guided_match(") < flat.index("int32_t ba_debug_linearize(")


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_guided_match$", out, flags=re.M)


def _constant(path, name):
    m = re.search(rf"static constexpr int {name} = (\d+);", open(os.path.join(CSRC, path)).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def test_reference_constants_are_the_stages_and_no_setting_was_added():
    assert _constant("ba_gmatch_host.h", "GMATCH_COUNT") == rg.COUNT_N
    assert _constant("ba_gmatch_host.h", "GMATCH_MIN_CELL") == rg.MIN_CELL
    assert _constant("ba_gmatch_host.h", "GMATCH_TPB") == 256 and _constant("ba_gmatch.h", "GMATCH_SEARCH_TPB") == 64
    # the candidate counts of the GPU cases surround the search kernel's wave and the scanning workgroup
    assert {63, 64, 65, 255, 256, 257} <= set(rg.CAND_COUNTS)
    assert "GMATCH" not in open(os.path.join(CSRC, "ba_settings.cpp")).read().upper()
    mk = open(os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    runtime = re.search(r"^RUNTIME := (.*)$", mk, flags=re.M).group(1).split()
    assert "ba_gmatch" in kernels and "ba_gmatch" in runtime
    host = open(os.path.join(CSRC, "ba_gmatch_host.h")).read()
    assert "#include <hip" not in host and "ba_context.h" not in host  # plain C++: the stand-alone program builds it
    assert "ba_guided_match" in open(os.path.join(CSRC, "ba_stage.h")).read().split("#pragma once")[0]
    # the shared top-2 lives in one header that both matchers include
    for f in ("ba_match.hip", "ba_gmatch.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "ba_top2.h"' in text and "void top2_push" not in text


def test_solver_guided_match_signature():
    from miba.solver import Solver
    sig = inspect.signature(Solver.guided_match)
    assert list(sig.parameters)[:9] == ["self", "points", "pt_desc", "kp_uv", "kp_desc", "frame_pose", "intr", "width", "height"]
    want = dict(frame_range=None, cand=None, kp_depth=None, kind="hamming", radius=15.0, ratio=0.7, max_distance=0,
                min_depth=0.0, depth_tol=0.0, one_to_one=True, cell_px=0, matches=True, counts=False, proj=False)
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want
    assert list(sig.parameters)[9:] == list(want)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("gmatch_host")
    out = {}
    for name, flags in (("plain", ["-O2"]),
                        ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                  "-fno-sanitize-recover=all"])):
        out[name] = str(d / f"gmatch_host_{name}")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "gmatch_host_main.cpp"), "-o", out[name]], check=True)
    return out


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_host_side_as_a_stand_alone_program(exes, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exes[build]], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "ok refusals" and lines[1] == "ok layout and limits" and lines[-1] == "ok all"
    assert lines[2].startswith("ok superset admitted=") and "FAILED" not in r.stdout
