"""The ABI of ba_align (no GPU): the ctypes mirrors of ba_align_problem / ba_align_request / ba_align_info against the
header compiled by gcc, the *_INIT / *_MIN_SIZE macros and the constants, the declaration and the export, that the
addition left BA_API_VERSION at 2, and that tests/refalign.py's tile, block and sweep sizes are the kernel's."""
import ctypes as C
import os
import re
import subprocess

import pytest

import refalign as ra
from miba import _lib, capi
from test_capi import ROOT, _c_layout
from test_loc_abi import _run_c

HEADER = os.path.join(ROOT, "include", "ba.h")
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")


@pytest.mark.parametrize("cls,cname", [("BaAlignProblem", "ba_align_problem"), ("BaAlignRequest", "ba_align_request"),
                                       ("BaAlignInfo", "ba_align_info")])
def test_struct_layout_matches_header(cls, cname):
    cls = getattr(capi, cls)
    names = [n for n, _ in cls._fields_]
    size, offs = _c_layout(cname, names)
    assert C.sizeof(cls) == size
    assert [getattr(cls, n).offset for n in names] == offs
    if cname != "ba_align_problem":  # the sized structs lead with their size
        assert names[0] == "struct_size" and cls().struct_size == size


def test_init_and_min_size_macros():
    out = _run_c("ba_align_request r; ba_align_info i; r.n_hypotheses = 7; r.threshold = 3.0; r.poses = (double*)&r; r.seed = 5;"
                 "i.n_ok = 3; BA_ALIGN_REQUEST_INIT(r); BA_ALIGN_INFO_INIT(i);"
                 'printf("%d %d %d %d %d %d %d %d\\n", r.struct_size, (int)sizeof(r), r.n_hypotheses, r.poses == NULL,'
                 "i.struct_size, (int)sizeof(i), BA_ALIGN_REQUEST_MIN_SIZE, BA_ALIGN_INFO_MIN_SIZE);"
                 'printf("%d %d %d %d %d %d %d\\n", i.n_ok, BA_API_VERSION, BA_ALIGN_STAT_N, BA_ALIGN_MAX_HYP, r.threshold == 0.0,'
                 "r.seed == 0, BA_ALIGN_SWEEPS);"
                 'printf("%d %d %d %d\\n", BA_ALIGN_OK, BA_ALIGN_TOO_FEW, BA_ALIGN_NO_MODEL, (int)offsetof(ba_align_info, time_kernels_ms));')
    rs, rsz, nh, pnull, isz_set, isz, rmin, imin, nok, ver, nstat, cap, thr0, seed0, sweeps, ok, few, nomodel, off = out
    assert rs == rsz == rmin == C.sizeof(capi.BaAlignRequest)
    assert isz_set == isz == C.sizeof(capi.BaAlignInfo)
    assert imin == off == capi.BaAlignInfo.time_kernels_ms.offset  # the counts; the timings are optional
    assert nh == 0 and pnull == 1 and nok == 0 and thr0 == 1 and seed0 == 1
    assert ver == 2
    assert nstat == capi.ALIGN_STAT_N == ra.STAT_N == 8
    assert cap == capi.ALIGN_MAX_HYP == _lib.ALIGN_MAX_HYP == ra.MAX_HYP == 65536
    assert (ok, few, nomodel) == (capi.ALIGN_OK, capi.ALIGN_TOO_FEW, capi.ALIGN_NO_MODEL) == (ra.OK, ra.TOO_FEW, ra.NO_MODEL)
    assert sweeps == ra.SWEEPS


def test_declaration_and_export():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = " ".join(src.split())
    assert ("int32_t ba_align(ba_context* ctx, const ba_align_problem* prob, const ba_align_request* req, "
            "ba_align_info* info);") in flat
    assert "ba_align" in _lib.EXPORTS
    assert "#define BA_API_VERSION 2" in src
    assert "ba_align" in text.split("#define BA_API_VERSION")[0]  # the history line


def test_library_exports_the_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libmiba.so is not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT ba_align$", out, flags=re.M)


def _constant(path, name):
    m = re.search(rf"static constexpr int {name} = (\d+);", open(os.path.join(CSRC, path)).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def test_reference_sizes_are_the_kernels():
    assert _constant("ba_align.h", "ALIGN_TPB") == ra.ALIGN_TPB
    assert _constant("ba_align.h", "ALIGN_TILE") == ra.ALIGN_TILE
    assert _constant("ba_align.h", "ALIGN_STAT") == ra.STAT_N
    assert _constant("ba_align_fit.h", "ALIGN_SWEEPS") == ra.SWEEPS
    # the header's sampling text is the one the kernels compile
    text = open(os.path.join(CSRC, "ba_align_sample.h")).read()
    for word in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert word in text and word in open(HEADER).read()
