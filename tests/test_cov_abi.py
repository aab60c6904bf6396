"""ba_cov_request / ba_cov_info: the ctypes mirrors have the header's layout (compiled by gcc, as test_capi.py does
for the other structs). ba_covariance itself is covered by test_capi.py's export test."""
import ctypes as C

import pytest

from test_capi import _c_layout


@pytest.mark.parametrize("cls,cname", [("BaCovRequest", "ba_cov_request"), ("BaCovInfo", "ba_cov_info")])
def test_cov_struct_layout_matches_header(cls, cname):
    from miba import capi
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    assert cls().struct_size == size
