"""ba_prepare decides and uploads what it did before its host code was split into phases (csrc/ba_prepare.cpp).

tests/golden/prepare_golden.json was recorded by tests/golden/make_prepare_golden.py with the library of the commit
before the split, on the smallest windows that reach each branch of the prepare: host and device plan, every
reduced-system solver and BCR path, the launch paths (fused, tail, bsfin, small-window), obs32 and f64 layouts, the
deterministic slabs. Each case prepares its window on a fresh context, without a solve. Compared exactly: the paths
ba_last_prepare() reports, ba_debug_plan_digest()'s digest of every plan array as it lies in HBM, and every kernel's
modelled bytes and flops per launch (ba_kernel_stats(); the model moved verbatim, so the doubles are bitwise equal)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_prepare_golden",
                                               os.path.join(HERE, "golden", "make_prepare_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(HERE, "golden", "prepare_golden.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_the_golden_file_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(gen.case_id(c) for c in gen.CASES) and len(GOLDEN) == 18


@pytest.mark.parametrize("case", gen.CASES, ids=gen.case_id)
def test_prepare_matches_the_golden(case):
    want = GOLDEN[gen.case_id(case)]
    got = json.loads(json.dumps(gen.record(case)))  # as the file holds it (lists, exact float round trip)
    assert got["info"] == want["info"]
    assert got["digest"] == want["digest"]
    assert len(got["kernels"]) == len(want["kernels"])
    for g, w in zip(got["kernels"], want["kernels"]):
        assert g == w, (g, w)
