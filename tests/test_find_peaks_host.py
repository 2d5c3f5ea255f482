"""PeakFinding.find_peaks without a GPU: the numpy oracle (tests/find_peaks_oracle.py) against recorded SciPy 1.15.3 results
(tests/golden/find_peaks_vectors.json, tools/gen_find_peaks_golden.py), the library's tie rule against its statement, the argument
checks of the Python function, every argument error of the C entry point (it validates before it looks at the context, so a null context
reaches every message), the typed context pointer, the switch / sources / documents, and the host side under ASan / UBSan in a
stand-alone program (tests/san_find_peaks.cpp)."""
import base64
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import find_peaks_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib
from nx_signal_amd import peak_finding as PF
from nx_signal_amd._lib import ArgumentError

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "find_peaks_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_PEAKS) as f:
    ABI_GOLDEN = json.load(f)


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).copy()


ROW = dec(GOLDEN["row"])


def case_input(c):
    if "values" in c["x"]:
        return dec(c["x"]["values"])
    return {"f64": ROW, "f32": ROW.astype(np.float32), "halves": np.round(ROW * 2) / 2}[c["x"]["row"]]


def case_opts(c):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["opts"].items()}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# The oracle performs SciPy's operations in SciPy's order on doubles, so the gap of the four width arrays to the recorded values was
# MEASURED as 0.0 on every case (numpy 2.2, scipy 1.15.3; profiles/find_peaks/accuracy.txt) and the test asserts equality.
WIDTH_GAP = 0.0


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, opts = case_input(c), case_opts(c)
    peaks, props = O.line(x, **opts)
    assert np.array_equal(peaks, dec(c["peaks"])) and list(props) == list(c["props"]), c["name"]
    for name, rec in c["props"].items():
        want, got = dec(rec), props[name]
        if name in O.WIDTH_PROPS:
            with np.errstate(invalid="ignore"):
                gap = float(np.nanmax(np.abs(got - want), initial=0.0))
            print(f"find-peaks-oracle-gap {c['name']} {name}: {gap:.1e}")
            assert gap <= WIDTH_GAP and np.array_equal(np.isnan(got), np.isnan(want)), (c["name"], name, gap)
        else:   # indices, bases, edges, plateau sizes, heights, thresholds, prominences: exact
            assert np.array_equal(got.astype(want.dtype), want, equal_nan=want.dtype.kind == "f"), (c["name"], name)
            if want.dtype.kind == "f":
                assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)]), (c["name"], name)


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    cs = {c["name"]: c for c in GOLDEN["cases"]}
    assert GOLDEN["scipy"] == "1.15.3" and GOLDEN["n"] == 4096 == ROW.size and ROW.dtype == np.float64
    assert dec(cs["plateau_array"]["peaks"]).tolist() == [2, 5, 9] and cs["plateau_array"]["opts"] == {"plateau_size": 1}
    assert cs["nan_inf_array"]["opts"] == {"height": 0, "threshold": 0, "prominence": 0, "width": 0}
    assert np.isnan(case_input(cs["nan_inf_array"])[3]) and np.isinf(case_input(cs["nan_inf_array"])[7])
    assert cs["wlen_1p5"]["opts"]["wlen"] == 1.5 and case_input(cs["wlen_1p5"]).tolist() == [1, 2, 1]
    assert cs["flagship_f64"]["kept_of"] == [355, 1360]
    assert cs["flagship_f64"]["opts"] == {"distance": 7.5, "prominence": [0.3, None], "width": 1, "wlen": 101, "rel_height": 0.7}
    seeded = [c for c in GOLDEN["cases"] if "row" in c["x"]]
    assert len({c["name"].rsplit("_", 1)[0] for c in seeded}) >= 12 and {c["x"]["row"] for c in seeded} == {"f32", "f64", "halves"}
    for c in seeded:
        assert 10 <= c["kept_of"][0] < c["kept_of"][1], c["name"]
    used = {k: set() for k in ("distance", "rel_height", "wlen")}
    alone = set()
    for c in seeded:
        for k in used:
            if k in c["opts"]:
                used[k].add(c["opts"][k])
        conds = [k for k in c["opts"] if k not in ("wlen", "rel_height")]
        if len(conds) == 1:
            alone.add(conds[0])
    assert used["distance"] == {1, 2, 7.5, 300} and used["rel_height"] >= {0, 0.5, 0.7, 1.0} and used["wlen"] == {64, 33, 20.5, 101}
    assert alone == {"height", "threshold", "distance", "prominence", "width", "plateau_size"}
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f != "find_peaks_vectors.json")
    assert os.path.getsize(FIXTURE) <= largest


def test_the_tie_rule_is_the_librarys_own():
    """among equal heights the larger index is visited first: checked against the rule as stated, not against a recording"""
    x = np.array([0, 2, 0, 2, 0, 2, 0, 2, 0], np.float64)
    assert O.line(x, distance=3)[0].tolist() == [3, 7]
    assert O.line(x, distance=2)[0].tolist() == [1, 3, 5, 7] and O.line(x, distance=5)[0].tolist() == [1, 7] and O.line(x, distance=4.5)[0].tolist() == [1, 7]
    assert O.line(x, distance=7)[0].tolist() == [7]   # 7 is visited first and reaches 1
    x = np.array([0, 2, 0, 2, 0, 3, 0, 2, 0, 2, 0], np.float64)   # 5 first; then 9 (larger index) removes nothing left of 5; then 1
    assert O.line(x, distance=4)[0].tolist() == [1, 5, 9]
    x = np.array([0, 1, 0, 1, 0, 1, 0], np.float64)               # visited 5, 3, 1: 5 removes 3, 1 stays
    assert O.line(x, distance=3)[0].tolist() == [1, 5]


X8 = np.zeros(8, np.float32)
BAD = [
    ("distance below 1", dict(distance=0.5), "`distance` must be greater or equal to 1"),
    ("wlen 1", dict(prominence=0, wlen=1), "`wlen` must be larger than 1, was 1"),
    ("wlen below 1", dict(wlen=0.5), "`wlen` must be larger than 1, was 0.5"),
    ("rel_height", dict(width=0, rel_height=-0.1), "`rel_height` must be greater or equal to 0.0"),
    ("array border", dict(height=np.zeros(8)), "array-valued borders are not supported"),
    ("array border in a pair", dict(prominence=(np.zeros(8), None)), "array-valued borders are not supported"),
    ("three borders", dict(width=(1, 2, 3)), "array-valued borders are not supported"),
    ("border text", dict(height="high"), "height must be a number"),
    ("border nan", dict(threshold=float("nan")), "threshold is not a number"),
    ("complex", dict(x=np.zeros(8, np.complex64)), "complex tensors have no order"),
    ("rank 0", dict(x=np.float32(1.0)), "rank-0 tensor has no axis"),
    ("rank 9", dict(x=np.zeros((1,) * 8 + (4,), np.float32)), "rank must be at most 8"),
    ("empty dimension", dict(x=np.zeros((2, 0), np.float32)), "empty dimension"),
    ("axis", dict(axis=1), "axis 1 is out of range for rank 1"),
    ("axis type", dict(axis=0.0), "axis must be an integer"),
    ("max_peaks", dict(max_peaks=0), "max_peaks must be a positive integer"),
    ("unknown option", dict(order=2), "unknown keys"),
    ("text tensor", dict(x=np.array(["a", "b", "c"])), "unsupported type"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(case):
    _, change, pattern = case
    kw = dict(x=X8)
    kw.update(change)
    x = kw.pop("x")
    with pytest.raises(ArgumentError, match=re.escape(pattern)):
        PF.find_peaks(x, **kw)


def test_trim_takes_host_results_only():
    peaks = {"indices": np.array([[4], [9], [-1]], np.int32), "valid_indices": np.array(2, np.uint32)}
    idx, props = PF.trim(peaks, {"peak_heights": np.array([1.0, 2.0, np.nan])})
    assert idx.tolist() == [4, 9] and props["peak_heights"].tolist() == [1.0, 2.0]
    peaks = {"indices": np.array([[0, 4], [-1, -1]], np.int32), "valid_indices": np.array(5, np.uint32)}   # max_peaks was smaller
    idx, props = PF.trim(peaks, {})
    assert idx.tolist() == [[0, 4], [-1, -1]] and props == {}


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_find_peaks comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.PEAKS_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    rows = table["nxsig_find_peaks"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    for k, r in rows.items():
        if k != "valid":
            assert r["rc"] == _lib.ERR_INVALID_ARG and r["err"] != "null context", (k, r)
    assert rows["distance=0.5"]["err"] == "find_peaks: `distance` must be greater or equal to 1"
    assert rows["wlen=1"]["err"] == "find_peaks: `wlen` must be larger than 1, was 1"
    assert rows["rel_height=-1"]["err"] == "find_peaks: `rel_height` must be greater or equal to 0.0"
    assert _lib.SIGNATURES["nxsig_find_peaks"][1][0] is _lib._ctx_peaks and _lib._ctx_peaks not in (_lib._p, _lib._ctx, _lib._ctx_spectral, _lib._ctx_iir)
    assert _lib.TYPED_CTX[-1] is _lib._ctx_peaks and len(_lib.TYPED_CTX) == 4
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()
    assert ABI_GOLDEN["real_ctx"]["nxsig_find_peaks"].keys() == rows.keys()


def test_a_typed_context_pointer_that_is_not_null_reaches_the_library():
    """the argument checks come ahead of the context, so a made-up non-null context with distance = 0 is refused and never looked at"""
    lib, V = _lib.load(), C.c_void_p
    x, idx, valid = np.zeros(8, np.float32), np.zeros((3, 1), np.int32), np.zeros(1, np.uint32)
    fake = _lib.ctx_ptr(V(64), _lib._ctx_peaks)
    assert isinstance(fake, _lib._ctx_peaks) and _lib.ctx_ptr(None, _lib._ctx_peaks) is None
    p = lambda a: a.ctypes.data_as(V)   # noqa: E731
    sh = (C.c_int64 * 1)(8)
    assert lib.nxsig_find_peaks(fake, p(x), _lib.DT_F32, sh, 1, 0, None, 8, 0.0, -1, 0.5, 3, 0, p(idx), p(valid), None, None, _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "`distance` must be greater or equal to 1" in _lib.last_error()
    assert lib.nxsig_find_peaks_block() == 64 and lib.nxsig_find_peaks_rounds() >= 0


def test_the_switch_the_sources_and_the_documents_are_in_place():
    assert "X(DISABLE_FIND_PEAKS_TABLES)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    src = read("nx_signal_amd", "csrc", "kernels_find_peaks.hip")
    assert "tune(c, kT_DISABLE_FIND_PEAKS_TABLES, 0)" in src and '("kernels_find_peaks.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["nxsig_internal.h"] and "#pragma clang fp contract(off)" in src
    # the only atomics are integer or / and on mask words; no floating-point atomics, no fused multiply-add
    assert set(re.findall(r"\batomic[A-Z]\w*", src)) == {"atomicOr", "atomicAnd"} and "fma" not in src.lower().replace("no fma contraction", "")
    assert '"find_peaks.tables"' in src and '"find_peaks.generic"' in src
    plan = read("nx_signal_amd", "csrc", "find_peaks_plan.hpp")
    assert "kFindPeaksBlock = 64" in plan and "find_peaks_distance_rounds" in plan and "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_find_peaks.hip", "")
    assert "NXSIG_DISABLE_FIND_PEAKS_TABLES" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.14" in design and "find_peaks" in design and "larger index" in design and "array-valued" in design
    assert "find_peaks" in read("README.md")
    tools = read("tools", "README.md")
    assert "bench_find_peaks.py" in tools and "gen_find_peaks_golden.py" in tools
    header = read("include", "nxsig.h")
    for name in ("nxsig_find_peaks", "nxsig_find_peaks_block", "nxsig_find_peaks_rounds"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    # this change adds no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "find_peaks" not in nif and "find_peaks" not in read("elixir", "lib", "nx_signal_amd", "peak_finding.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.peak_finding.find_peaks is PF.find_peaks and callable(PF.trim)
    for f in ("bench.json", "accuracy.txt"):
        assert os.path.exists(os.path.join(ROOT, "profiles", "find_peaks", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_find_peaks.py"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks, the capacity and block arithmetic, every walk with the line summary against the walk element by element, and
    the rounds of the distance stage against the sequential rule (csrc/find_peaks_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_find_peaks")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_find_peaks.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized find_peaks host side ok" in r.stdout
