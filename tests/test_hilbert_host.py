"""Filters.hilbert without a GPU: the numpy oracle (tests/hilbert_oracle.py) against recorded SciPy 1.15.3 results
(tests/golden/hilbert_vectors.json, tools/gen_hilbert_golden.py), the multiplier rule and the tier choice of csrc/hilbert_plan.hpp, the
argument checks of the Python function, every argument error of the C entry point (it validates before it looks at the context, so a null
context reaches every message), the switch / sources / documents, and the host side under ASan / UBSan in a stand-alone program
(tests/san_hilbert.cpp)."""
import base64
import json
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import hilbert_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _hilbert, _lib, filters
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "hilbert_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_HILBERT) as f:
    ABI_GOLDEN = json.load(f)

# the oracle and SciPy differ by the rounding of two double transforms: measured <= 2.1e-15 absolute on N(0, 1) rows up to 4096 points
ORACLE_TOL = 1e-12


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).reshape(a["shape"]).copy()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def oracle_gap(c):
    x, y, at = dec(c["x"]), dec(c["y"]), dec(c["at"])
    got = np.moveaxis(O.hilbert(np.moveaxis(x, c["axis"], -1), c["N"]), -1, c["axis"])
    got = np.take(got, at, axis=c["axis"])
    assert got.shape == y.shape and y.dtype == np.complex128 and x.dtype == np.float32
    return float(np.abs(got - y).max()), float(np.abs(y).max())


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    gap, top = oracle_gap(c)
    print(f"hilbert-oracle-gap {c['name']}: {gap:.3e} absolute, {gap / top:.3e} of the row maximum")
    assert gap <= ORACLE_TOL * top, (c["name"], gap, top)
    for output, of in (("envelope", np.abs), ("quadrature", np.imag)):
        x = np.moveaxis(dec(c["x"]), c["axis"], -1)
        got = np.take(O.hilbert(x, c["N"], output), dec(c["at"]), axis=-1)
        assert np.abs(got - of(np.moveaxis(dec(c["y"]), c["axis"], -1))).max() <= ORACLE_TOL * top


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    cs = {c["name"]: c for c in GOLDEN["cases"]}
    assert GOLDEN["scipy"] == "1.15.3" and GOLDEN["lengths"] == [1, 2, 3, 7, 8, 1000, 1023, 1024, 2048, 4096]
    assert all(f"L{n}" in cs and cs[f"L{n}"]["N"] is None for n in GOLDEN["lengths"])
    resized = [tuple(r) for r in GOLDEN["resized"]]
    assert any(n > l for l, n in resized) and any(n < l for l, n in resized) and {n % 2 for _, n in resized} == {0, 1}
    assert all(f"L{l}_N{n}" in cs for l, n in resized)
    assert sum(c["axis"] == 0 and len(c["x"]["shape"]) == 2 for c in cs.values()) >= 2
    assert sum(c["name"].startswith("offset1000") and dec(c["x"]).mean() > 990 for c in cs.values()) == 2
    # SciPy leaves no finite component of a row that holds a NaN or an Inf: the non-finite rule of include/nxsig.h
    assert len(GOLDEN["nonfinite"]) == 9 and set(GOLDEN["nonfinite"].values()) == {0}
    assert os.path.getsize(FIXTURE) <= 128 << 10
    # the measured maximum that profiles/hilbert/accuracy.txt keeps
    kept = re.search(r"^hilbert-oracle-worst \(rows of N\(0, 1\) samples\): (\d\.\d{3}e-\d+) absolute \(bound 1e-12 of the row maximum\)$",
                     read("profiles", "hilbert", "accuracy.txt"), re.M)
    assert kept and float(kept.group(1)) <= 2.1e-15
    assert len(re.findall(r"^hilbert-oracle-gap \w+: ", read("profiles", "hilbert", "accuracy.txt"), re.M)) == len(GOLDEN["cases"])
    assert len(re.findall(r"^hilbert-accuracy (wave|generic|offset-1000) ", read("profiles", "hilbert", "accuracy.txt"), re.M)) >= 60
    with np.errstate(all="ignore"):
        for output in O.OUTPUTS:
            x = np.ones((3, 9), np.float32)
            x[1, 4] = np.inf
            y = O.hilbert(x, 8, output)
            assert not np.isfinite(y[1]).any() and np.isfinite(y[0]).all() and np.isfinite(y[2]).all()
            x[1, 4], x[1, 8] = 1.0, np.nan          # beyond min(L, N): not used
            assert np.isfinite(O.hilbert(x, 8, output)).all()


@pytest.fixture(scope="module")
def plan():
    """csrc/hilbert_plan.hpp behind three C functions, in a small shared library of its own (plain g++: the header has no HIP types)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    import ctypes as C
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    src, so = os.path.join(build, "hilbert_plan_c.cpp"), os.path.join(build, "hilbert_plan_c.so")
    with open(src, "w") as f:
        f.write('#include "hilbert_plan.hpp"\nextern "C" {\n'
                "int hb_gain(long long k, long long n) { return nxsig::hilbert_gain(k, n); }\n"
                "int hb_tier(long long n, int off) { return nxsig::hilbert_tier(n, off != 0); }\n"
                "int hb_wave_gain(int lane, int s, int p) { return nxsig::hilbert_wave_gain(lane, s, p); }\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    lib.hb_gain.argtypes, lib.hb_tier.argtypes, lib.hb_wave_gain.argtypes = [C.c_longlong] * 2, [C.c_longlong, C.c_int], [C.c_int] * 3
    return lib


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024])
def test_hilbert_gain_follows_the_rule_and_sums_to_n(plan, n):
    g = np.array([plan.hb_gain(k, n) for k in range(n)])
    assert np.array_equal(g, O.gain(n)) and g.sum() == n
    assert g[0] == 1 and (n % 2 or n == 1 or g[n // 2] == 1)
    if n in (1024,):
        assert all(plan.hb_wave_gain(lane, s, 16) == g[lane + 64 * s] for lane in range(64) for s in range(16))


def test_the_tier_choice(plan):
    for n in (1, 2, 3, 7, 8, 512, 1000, 1023, 1025, 2047, 2049, 4096, 6000, 1 << 15):
        assert plan.hb_tier(n, 0) == 1, n
    assert plan.hb_tier(1024, 0) == 0 and plan.hb_tier(2048, 0) == 0
    assert plan.hb_tier(1024, 1) == 1 and plan.hb_tier(2048, 1) == 1


X32 = np.zeros(32, np.float32)
BAD = [
    ("complex", dict(x=np.zeros(32, np.complex64)), ValueError, "x must be real."),
    ("complex list", dict(x=[1j, 2.0]), ValueError, "x must be real."),
    ("f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64"),
    ("output", dict(output="phase"), ArgumentError, "output must be 'analytic', 'envelope' or 'quadrature'"),
    ("output type", dict(output=1), ArgumentError, "output must be 'analytic', 'envelope' or 'quadrature'"),
    ("N 0", dict(N=0), ValueError, "N must be positive."),
    ("N -4", dict(N=-4), ValueError, "N must be positive."),
    ("N float", dict(N=32.0), ArgumentError, "N must be an integer"),
    ("N bool", dict(N=True), ArgumentError, "N must be an integer"),
    ("N 2^31", dict(N=1 << 31), NxSignalUnsupported, "unsupported N"),
    ("text", dict(x=np.array(["a"] * 32)), ArgumentError, "unsupported type"),
    ("rank 0", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("empty", dict(x=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
    ("axis", dict(axis=1), ArgumentError, "axis 1 is out of bounds"),
    ("unknown option", dict(order=2), ArgumentError, "unknown keys"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(case, monkeypatch):
    """every Python-side error comes before the library is loaded"""
    _, change, error, pattern = case

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    kw = dict(x=X32)
    kw.update(change)
    with pytest.raises(error, match=re.escape(pattern)):
        filters.hilbert(kw.pop("x"), **kw)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_hilbert_f32 comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.HILBERT_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    rows = table["nxsig_hilbert_f32"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    assert rows["batch=0"] == rows["valid"]        # batch = 0 passes every check and reaches the context
    unsupported = {"n_fft=2^31", "rows too large", "result too large"}
    for k, r in rows.items():
        if k not in ("valid", "batch=0"):
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
            assert r["err"].startswith("hilbert: ") or k == "mem=7", (k, r)
    assert {"null x", "null out", "length=0", "n_fft=0", "batch=-1", "batch_stride=length-1", "kind=3", "mem=7"} <= set(rows)
    assert _lib.SIGNATURES["nxsig_hilbert_f32"][1][0] is _lib._ctx_iir
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()
    assert set(ABI_GOLDEN["real_ctx"]["nxsig_hilbert_f32"]) == set(rows) - {"batch=0"}


def test_the_switch_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(DISABLE_HILBERT_WAVE)" in internal and "kScratchSlots = 32" in internal and '#include "hilbert_plan.hpp"' in internal
    src = read("nx_signal_amd", "csrc", "kernels_hilbert.hip")
    assert "tune(c, kT_DISABLE_HILBERT_WAVE, 0)" in src and '("kernels_hilbert.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["wave_stft.hpp"]
    assert not re.findall(r"\batomic[A-Z]\w*", src)
    assert 'dispatch_note("hilbert.wave")' in src and 'dispatch_note("hilbert.generic")' in src
    assert "wave_fft_core_T<K>" in src and "wave_fft_core<K, true, true>" in src and "hilbert_gain(k, N)" in src
    assert set(re.findall(r"kScratch\w+", src)) == {"kScratchFusedSpectrum", "kScratchIstftProduct"}
    plan = read("nx_signal_amd", "csrc", "hilbert_plan.hpp")
    assert "hilbert_gain" in plan and "hilbert_tier" in plan and "hilbert_check" in plan and "hilbert_pair_state" in plan
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_hilbert.hip", "")
    assert "hilbert_plan.hpp" in read("tests", "san_hilbert.cpp")
    assert "NXSIG_DISABLE_HILBERT_WAVE" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.16" in design and "hilbert.wave" in design and "kScratchFusedSpectrum" in design and "kScratchIstftProduct" in design
    assert "hilbert" in read("README.md")
    tools = read("tools", "README.md")
    assert "bench_hilbert.py" in tools and "gen_hilbert_golden.py" in tools
    header = read("include", "nxsig.h")
    assert re.search(r"\bnxsig_hilbert_f32\(", header) and "nxsig_hilbert_f32" in _lib.SIGNATURES
    assert "h[N / 2] = 1" in header and "NXSIG_HILBERT_QUADRATURE" in header and "no finite output element" in header
    # this change adds no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "hilbert" not in nif and "hilbert" not in read("elixir", "lib", "nx_signal_amd", "filters.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.filters.hilbert is filters.hilbert is _hilbert.hilbert and filters.hilbert.__module__ == "nx_signal_amd._hilbert"
    assert os.path.exists(os.path.join(ROOT, "profiles", "hilbert", "bench.json"))
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_hilbert.py"))


def test_the_private_module_can_be_imported_first():
    """filters imports _hilbert and _hilbert needs a helper of filters: either order of import must work, in a fresh interpreter"""
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._hilbert as m, nx_signal_amd.filters as f; assert f.hilbert is m.hilbert"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks over a sweep with the rejected ones, the multiplier rule against a naive DFT, the tier choice, and the fused
    kernel's row and lane arithmetic walked over exactly sized buffers (csrc/hilbert_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_hilbert")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_hilbert.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized hilbert host side ok" in r.stdout
