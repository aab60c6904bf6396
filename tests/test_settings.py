"""The MIBA_* settings of ba_prepare (csrc/ba_settings.cpp): one table names every prepare-time variable, how it
parses and whether it is part of the plan-cache key; read_settings() fills the struct and the key in one pass.

tests/cpp/settings_main.cpp prints the parsed struct and the key for the environment it is started in; it is built
from ba_settings.cpp alone. Checked: the defaults with every variable unset; every variable's parse, quirks included
(any MIBA_BCR value counts as "set", a non-numeric MIBA_BCR_BAND means off, an unknown MIBA_SOLVER string is
ignored); the key changes with every keyed variable, tells unset from the empty string, is equal for equal
environments and ignores the unkeyed variables; the same harness under AddressSanitizer + UndefinedBehaviorSanitizer
runs clean over the same environments and prints the same."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dsmc-bundle-adjustment_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "settings_main.cpp"), os.path.join(CSRC, "ba_settings.cpp")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

DEFAULTS = dict(obs32=1, fused=1, tail=1, xcd_map=1, bcr_dense1=1, device_plan=-1, sw=1, fpl=0, bsfin=0, bcr_xmap=0,
                dense_chol=0, solver=-1, bcr_set=0, bcr=-1, bcr_band=1, tile_pts=0, subseg=0, blocked_min_set=0,
                blocked_min=0, value_chunks=0, pp_lanes=1, plan_times=0, prep_times=0)

KEYED = ("MIBA_OBS32", "MIBA_TILE_PTS", "MIBA_SUBSEG", "MIBA_SOLVER", "MIBA_DENSE_CHOL", "MIBA_BCR", "MIBA_XCD_MAP",
         "MIBA_FUSED", "MIBA_SW", "MIBA_FPL", "MIBA_BCR_DENSE1", "MIBA_PP_LANES", "MIBA_DEVICE_PLAN", "MIBA_TAIL",
         "MIBA_BCR_BAND", "MIBA_BCR_XMAP", "MIBA_BLOCKED_MIN", "MIBA_BSFIN")
UNKEYED = ("MIBA_VALUE_CHUNKS", "MIBA_PLAN_TIMES", "MIBA_PREP_TIMES")

# (variable, value, the fields that differ from the defaults)
ROWS = []
for _var, _field in (("MIBA_OBS32", "obs32"), ("MIBA_FUSED", "fused"), ("MIBA_TAIL", "tail"),
                     ("MIBA_XCD_MAP", "xcd_map"), ("MIBA_BCR_DENSE1", "bcr_dense1")):
    # off iff the first character is '0'
    ROWS += [(_var, "0", {_field: 0}), (_var, "0x", {_field: 0}), (_var, "1", {}), (_var, "", {}), (_var, "off", {})]
for _var, _field in (("MIBA_FPL", "fpl"), ("MIBA_BSFIN", "bsfin"), ("MIBA_BCR_XMAP", "bcr_xmap"),
                     ("MIBA_DENSE_CHOL", "dense_chol")):
    # on iff the first character is '1'
    ROWS += [(_var, "1", {_field: 1}), (_var, "10", {_field: 1}), (_var, "0", {}), (_var, "", {}), (_var, "2", {}),
             (_var, "on", {})]
ROWS += [
    ("MIBA_DEVICE_PLAN", "0", {"device_plan": 0}), ("MIBA_DEVICE_PLAN", "1", {"device_plan": 1}),
    ("MIBA_DEVICE_PLAN", "auto", {}), ("MIBA_DEVICE_PLAN", "", {}), ("MIBA_DEVICE_PLAN", "2", {}),
    ("MIBA_SW", "0", {"sw": 0}), ("MIBA_SW", "2", {"sw": 2}), ("MIBA_SW", "1", {}), ("MIBA_SW", "", {}),
    ("MIBA_SW", "3", {}),
    ("MIBA_SOLVER", "dense", {"solver": 0}), ("MIBA_SOLVER", "band", {"solver": 1}), ("MIBA_SOLVER", "bcr", {"solver": 2}),
    ("MIBA_SOLVER", "blocked", {"solver": 3}), ("MIBA_SOLVER", "cholmod", {}), ("MIBA_SOLVER", "", {}),
    ("MIBA_SOLVER", "Dense", {}),
    # being set at all disables the dense1 and band paths; only three values override the path
    ("MIBA_BCR", "launch", {"bcr_set": 1, "bcr": 0}), ("MIBA_BCR", "persist", {"bcr_set": 1, "bcr": 1}),
    ("MIBA_BCR", "split", {"bcr_set": 1, "bcr": 2}), ("MIBA_BCR", "split3", {"bcr_set": 1}),
    ("MIBA_BCR", "", {"bcr_set": 1}), ("MIBA_BCR", "whatever", {"bcr_set": 1}),
    # atoi: a non-numeric string is 0, which is "off"
    ("MIBA_BCR_BAND", "0", {"bcr_band": 0}), ("MIBA_BCR_BAND", "2", {"bcr_band": 2}), ("MIBA_BCR_BAND", "1", {}),
    ("MIBA_BCR_BAND", "7", {"bcr_band": 7}), ("MIBA_BCR_BAND", "on", {"bcr_band": 0}), ("MIBA_BCR_BAND", "", {"bcr_band": 0}),
    ("MIBA_TILE_PTS", "96", {"tile_pts": 96}), ("MIBA_TILE_PTS", "0", {"tile_pts": 1}), ("MIBA_TILE_PTS", "-5", {"tile_pts": 1}),
    ("MIBA_TILE_PTS", "x", {"tile_pts": 1}),
    ("MIBA_SUBSEG", "512", {"subseg": 512}), ("MIBA_SUBSEG", "63", {"subseg": 64}), ("MIBA_SUBSEG", "", {"subseg": 64}),
    ("MIBA_BLOCKED_MIN", "64", {"blocked_min_set": 1, "blocked_min": 64}),
    ("MIBA_BLOCKED_MIN", "0", {"blocked_min_set": 1}), ("MIBA_BLOCKED_MIN", "-1", {"blocked_min_set": 1, "blocked_min": -1}),
    ("MIBA_BLOCKED_MIN", "5000000000", {"blocked_min_set": 1, "blocked_min": 5000000000}),
    ("MIBA_BLOCKED_MIN", "x", {"blocked_min_set": 1}),
    ("MIBA_VALUE_CHUNKS", "4", {"value_chunks": 4}), ("MIBA_VALUE_CHUNKS", "0", {"value_chunks": 1}),
    ("MIBA_VALUE_CHUNKS", "1000", {"value_chunks": 64}), ("MIBA_VALUE_CHUNKS", "", {"value_chunks": 1}),
    ("MIBA_PP_LANES", "2", {"pp_lanes": 2}), ("MIBA_PP_LANES", "4", {"pp_lanes": 4}), ("MIBA_PP_LANES", "1", {}),
    ("MIBA_PP_LANES", "3", {}), ("MIBA_PP_LANES", "8", {}), ("MIBA_PP_LANES", "", {}),
    ("MIBA_PLAN_TIMES", "1", {"plan_times": 1}), ("MIBA_PLAN_TIMES", "", {"plan_times": 1}),
    ("MIBA_PLAN_TIMES", "0", {"plan_times": 1}),
    ("MIBA_PREP_TIMES", "1", {"prep_times": 1}), ("MIBA_PREP_TIMES", "", {"prep_times": 1}),
]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("settings")
    out = {}
    for name, flags in (("plain", ["-O2"]),
                        ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                  "-fno-sanitize-recover=all"])):
        out[name] = str(d / f"settings_{name}")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", CSRC, *SRC, "-o", out[name]], check=True)
    return out


def _read(exe, env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("MIBA_")}
    base.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=dict(base, **env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return {k: int(v) for k, v in (line.split("=") for line in r.stdout.splitlines())}


def test_the_table_names_every_variable_once():
    assert len(set(KEYED)) == 18 and not set(KEYED) & set(UNKEYED)
    assert {v for v, _, _ in ROWS} == set(KEYED) | set(UNKEYED)


def test_defaults_with_every_variable_unset(exes):
    got = _read(exes["plain"], {})
    key = got.pop("key")
    assert got == DEFAULTS
    assert _read(exes["plain"], {})["key"] == key  # equal environments, equal keys (another process)


@pytest.mark.parametrize("var,value,diff", ROWS, ids=[f"{v}={x!r}" for v, x, _ in ROWS])
def test_every_row_parses_as_stated(exes, var, value, diff):
    got = _read(exes["plain"], {var: value})
    got.pop("key")
    assert got == dict(DEFAULTS, **diff)


def test_key_follows_the_keyed_variables_only(exes):
    unset = _read(exes["plain"], {})["key"]
    seen = {unset}
    for var in KEYED:
        value = next(x for v, x, _ in ROWS if v == var and x)
        k_val, k_empty = _read(exes["plain"], {var: value})["key"], _read(exes["plain"], {var: ""})["key"]
        assert k_val != unset, var
        assert k_empty != unset and k_empty != k_val, var  # unset is not the empty string
        assert _read(exes["plain"], {var: value})["key"] == k_val, var
        seen |= {k_val, k_empty}
    assert len(seen) == 1 + 2 * len(KEYED)  # no two of these environments share a key
    for var in UNKEYED:
        assert _read(exes["plain"], {var: "1"})["key"] == unset, var
        assert _read(exes["plain"], {var: ""})["key"] == unset, var
    # a keyed value is not confused with its neighbour's name: "A=x, B unset" differs from "A unset, B=x"
    assert _read(exes["plain"], {"MIBA_FPL": "1"})["key"] != _read(exes["plain"], {"MIBA_BSFIN": "1"})["key"]


def test_clean_under_asan_ubsan(exes):
    """The stand-alone harness with -fsanitize=address,undefined over the same environments: no report (stderr must
    be empty, the exit status 0) and the same output as the plain build."""
    envs = [{}] + [{v: x} for v, x, _ in ROWS] + [{v: "1" for v in KEYED + UNKEYED}]
    for env in envs:
        assert _read(exes["asan"], env) == _read(exes["plain"], env), env
