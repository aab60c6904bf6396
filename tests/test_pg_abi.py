"""The ABI of ba_pose_graph (no GPU): the ctypes mirrors of ba_pg_problem / ba_pg_request / ba_pg_info against the
header compiled by gcc, the *_INIT / *_MIN_SIZE macros, the declaration and the export, and that the addition left
BA_API_VERSION at 2."""
import ctypes as C
import os
import re
import subprocess

import pytest

from miba import _lib, capi
from test_capi import ROOT, _c_layout
from test_loc_abi import _run_c

HEADER = os.path.join(ROOT, "include", "ba.h")


@pytest.mark.parametrize("cls,cname", [("BaPgProblem", "ba_pg_problem"), ("BaPgRequest", "ba_pg_request"),
                                       ("BaPgInfo", "ba_pg_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    if cname != "ba_pg_problem":  # the sized structs lead with their size
        assert names[0] == "struct_size" and cls().struct_size == size


def test_init_and_min_size_macros():
    out = _run_c("ba_pg_request r; ba_pg_info i; r.log_max_rows = 7; r.huber = 3.0; r.edge_cost = (double*)&r; i.n_active = 3;"
                 "BA_PG_REQUEST_INIT(r); BA_PG_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.log_max_rows, r.edge_cost == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_PG_REQUEST_MIN_SIZE, BA_PG_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d %d\\n", i.n_active, BA_API_VERSION, BA_PG_MAX_NPAD, (int)sizeof(i.message), r.huber == 0.0);')
    rs, rsz, rows, enull, isz_set, isz, rmin, imin, nact, ver, cap, msg, hub0 = out
    assert rs == rsz == rmin == C.sizeof(capi.BaPgRequest)
    assert isz_set == isz == imin == C.sizeof(capi.BaPgInfo)
    assert rows == 0 and enull == 1 and nact == 0 and hub0 == 1
    assert ver == 2 and cap == capi.PG_MAX_NPAD == 8192 and msg == 160


def test_declaration_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert ("int32_t ba_pose_graph(ba_context* ctx, ba_pg_problem* g, const ba_pg_request* req, "
            "ba_pg_info* info);") in flat
    assert "ba_pose_graph" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_pose_graph" in text.split("#define BA_API_VERSION")[0]  # the history line


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_pose_graph$", out, flags=re.M)
