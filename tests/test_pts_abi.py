"""The ABI of ba_refine_points (no GPU): the ctypes mirrors of ba_pts_request / ba_pts_info against the header compiled
by gcc, the *_INIT / *_MIN_SIZE macros, the declaration and the export, that the addition left BA_API_VERSION at 2, and
that tests/refpts.py's group width is the kernel's."""
import ctypes as C
import os
import re
import subprocess

import pytest

import refpts
from miba import _lib, capi
from test_capi import ROOT, _c_layout
from test_loc_abi import HEADER, _run_c


@pytest.mark.parametrize("cls,cname", [("BaPtsRequest", "ba_pts_request"), ("BaPtsInfo", "ba_pts_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    assert names[0] == "struct_size" and cls().struct_size == size


def test_init_and_min_size_macros():
    out = _run_c("ba_pts_request r; ba_pts_info i; r.log_max_rows = 7; r.min_obs = 3; r.pt_stats = (double*)&r;"
                 "i.n_solved = 3; BA_PTS_REQUEST_INIT(r); BA_PTS_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.log_max_rows, r.pt_stats == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_PTS_REQUEST_MIN_SIZE, BA_PTS_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d %d\\n", i.n_solved, BA_API_VERSION, BA_PTS_STAT_N, BA_LOG_WIDTH, r.min_obs);')
    rs, rsz, rows, snull, isz_set, isz, rmin, imin, nsolved, ver, nstat, logw, min_obs = out
    assert rs == rsz == rmin == C.sizeof(capi.BaPtsRequest)
    assert isz_set == isz == imin == C.sizeof(capi.BaPtsInfo)
    assert rows == 0 and snull == 1 and nsolved == 0 and min_obs == 0
    assert ver == 2
    assert nstat == capi.PTS_STAT_N == len(capi.LOC_STAT_FIELDS) == 8 and logw == _lib.LOG_WIDTH


def test_declaration_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert ("int32_t ba_refine_points(ba_context* ctx, ba_problem* prob, const ba_pts_request* req, "
            "ba_pts_info* info);") in flat
    assert "ba_refine_points" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_refine_points" in text.split("#define BA_API_VERSION")[0]  # the history line


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_refine_points$", out, flags=re.M)


def test_reference_group_width_is_the_kernel_s():
    text = open(os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc", "ba_pts.h")).read()
    lanes = int(re.search(r"constexpr int PTS_LANES = (\d+);", text).group(1))
    tpb = int(re.search(r"constexpr int PTS_TPB = (\d+);", text).group(1))
    assert lanes == refpts.LANES and tpb == 256 and tpb // lanes == 16
