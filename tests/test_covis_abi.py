"""ba_covis_request / ba_covis_info: the ctypes mirrors have the header's layout (compiled by gcc, as test_capi.py does
for the other structs), and the header declares the additive entry points without touching the version or ba_options.
ba_covisibility / ba_solve_ordered themselves are covered by test_capi.py's export test."""
import ctypes as C
import os
import re

import pytest

from test_capi import ROOT, _c_layout


@pytest.mark.parametrize("cls,cname", [("BaCovisRequest", "ba_covis_request"), ("BaCovisInfo", "ba_covis_info")])
def test_covis_struct_layout_matches_header(cls, cname):
    from miba import capi
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    assert cls().struct_size == size


def test_covis_header():
    from miba import _lib, capi
    text = open(os.path.join(ROOT, "include", "ba.h")).read()
    assert "#define BA_API_VERSION 2" in text
    for macro in ("BA_COVIS_REQUEST_MIN_SIZE", "BA_COVIS_INFO_MIN_SIZE", "BA_COVIS_REQUEST_INIT", "BA_COVIS_INFO_INIT"):
        assert re.search(r"#define %s\b" % macro, text), macro
    assert re.search(r"int32_t ba_covisibility\(ba_context\* ctx, const ba_problem\* prob, const ba_covis_request\* req, "
                     r"ba_covis_info\* info\);", text)
    assert re.search(r"int32_t ba_solve_ordered\(ba_context\* ctx, ba_problem\* prob, const int32_t\* order, "
                     r"ba_summary\* summary\);", text)
    assert {"ba_covisibility", "ba_solve_ordered"} <= set(_lib.EXPORTS)
    # ba_options keeps its layout: the reserved field is still there
    assert ("reserved", C.c_int32 * 1) == capi.BaOptions._fields_[-1]
    assert "int32_t reserved[1];" in text
    # the info's fields, by name
    assert [n for n, _ in capi.BaCovisInfo._fields_] == [
        "struct_size", "n_active", "n_edges", "n_components", "band_before", "band_after", "wide_before", "wide_after",
        "order_changed", "reserved0", "time_count_ms", "time_order_ms", "time_total_ms"]
