"""ba_res_request / ba_res_info: the ctypes mirrors have the header's layout (compiled by gcc, as test_capi.py does
for the other structs), and the BA_RES_* constants of capi.py are the header's. ba_residuals itself is covered by
test_capi.py's export test."""
import ctypes as C
import os
import re

import pytest

from test_capi import ROOT, _c_layout


@pytest.mark.parametrize("cls,cname", [("BaResRequest", "ba_res_request"), ("BaResInfo", "ba_res_info")])
def test_res_struct_layout_matches_header(cls, cname):
    from miba import capi
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    assert cls().struct_size == size


def test_res_constants_match_header():
    from miba import capi
    text = open(os.path.join(ROOT, "include", "ba.h")).read()
    val = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (BA_RES_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)\b", text)}
    want = dict(BA_RES_INADMISSIBLE=capi.RES_INADMISSIBLE, BA_RES_BEHIND=capi.RES_BEHIND, BA_RES_REPROJ=capi.RES_REPROJ,
                BA_RES_DEPTH=capi.RES_DEPTH, BA_RES_HUBER_REPR=capi.RES_HUBER_REPR,
                BA_RES_HUBER_UNPR=capi.RES_HUBER_UNPR, BA_RES_ERR_N=capi.RES_ERR_N, BA_RES_STAT_N=capi.RES_STAT_N)
    for k, v in want.items():
        assert val[k] == v, k
    assert capi.RES_OUTLIER == capi.RES_BEHIND | capi.RES_REPROJ | capi.RES_DEPTH
    assert "BA_RES_OUTLIER      (BA_RES_BEHIND | BA_RES_REPROJ | BA_RES_DEPTH)" in text
    assert "ba_res_request" in text and "#define BA_API_VERSION 2" in text
