"""Filters.lfilter / lfilter_zi / filtfilt / lfiltic without a GPU: the f64 oracle (tests/lfilter_oracle.py) against recorded scipy
results (tests/golden/lfilter_vectors.json, tools/gen_lfilter_golden.py), lfilter_zi, lfiltic and the geometry queries of the library,
the argument checks of the Python functions, every argument error of the two C entry points (they validate before they look at the
context, so a null context reaches every message), the conditioning guard's verdict on the recorded filters, the guard case the GPU test
relies on, the switch / sources / documents, and the host side under ASan / UBSan in a stand-alone program (tests/san_lfilter.cpp)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lfilter_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "lfilter_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_LFILTER) as f:
    ABI_GOLDEN = json.load(f)
X = np.array(GOLDEN["x"], np.float32).astype(np.float64)   # f32 values, recorded in their shortest form
AT = GOLDEN["at"]   # the samples of every output that are recorded: every thirty-second and the last
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def gap(y, recorded):
    """largest error at the recorded samples over the largest recorded magnitude of the row"""
    return O.nerr(y[:, AT], np.array(recorded))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    """the recurrence bit for bit where scipy runs it (na > 1); within 1e-14 of the row maximum where scipy convolves instead (na == 1).
    The solves behind lfilter_zi and filtfilt go through LAPACK on both sides: a few eps x the condition of I - A"""
    b, a = np.array(c["b"]), np.array(c["a"])
    assert GOLDEN["scipy"] and max(len(b), len(a)) - 1 == c["order"]
    y, _ = O.lfilter(b, a, X)
    yz, zf = O.lfilter(b, a, X, np.array(c["zi"]))
    if len(a) > 1:
        assert np.array_equal(y[:, AT], np.array(c["y"])) and np.array_equal(yz[:, AT], np.array(c["y_zi"])) and np.array_equal(zf, np.array(c["zf"]))
    else:
        assert gap(y, c["y"]) <= 1e-14 and gap(yz, c["y_zi"]) <= 1e-14
        if c["order"]:
            assert np.abs(zf - np.array(c["zf"])).max() <= 1e-14 * np.abs(c["y_zi"]).max()
    assert np.array_equal(O.lfiltic(b, a, c["past_y"], c["past_x"]), np.array(c["lfiltic"]))   # the same sums in the same order
    if c["lfilter_zi"] is None:   # a pole at z = 1: scipy raised LinAlgError, and so does the oracle
        with pytest.raises(np.linalg.LinAlgError):
            O.lfilter_zi(b, a)
        assert "filtfilt" not in c
        return
    if not c["order"]:
        return
    ref = np.array(c["lfilter_zi"])
    bn, an, n = O.normalise(b, a)
    cond = np.linalg.cond(np.eye(n) - O.companion(an))
    tol = 8 * np.finfo(np.float64).eps * cond
    gaps = {"lfilter_zi": float(np.abs(O.lfilter_zi(b, a) - ref).max() / np.abs(ref).max())}
    assert O.default_padlen(b, a) == 3 * max(len(b), len(a))
    for padtype, ref in c["filtfilt"].items():
        gaps["filtfilt " + padtype] = gap(O.filtfilt(b, a, X, None if padtype == "None" else padtype), ref)
    gaps["filtfilt padlen"] = gap(O.filtfilt(b, a, X, "even", GOLDEN["padlen"]), c["filtfilt_padlen"])
    print(f"lfilter-oracle-gap {c['name']}: " + ", ".join(f"{k} {v:.1e}" for k, v in gaps.items()) + f" (tolerance {tol:.1e})")
    assert max(gaps.values()) <= max(tol, 1e-13), gaps


def test_the_recorded_filters_cover_every_padded_order_and_coefficient_shape():
    assert sorted({c["order"] for c in GOLDEN["cases"]}) == [0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 16]
    assert CASES["a0_is_2"]["a"][0] == 2.0 and len(CASES["nb_gt_na"]["b"]) > len(CASES["nb_gt_na"]["a"]) and len(CASES["na_gt_nb"]["a"]) > len(CASES["na_gt_nb"]["b"])
    assert CASES["integrator"]["lfilter_zi"] is None and CASES["preemph"]["a"] == [1.0] and CASES["gain"]["order"] == 0
    assert X.shape == (2, 96) and AT[-1] == X.shape[1] - 1 and GOLDEN["sampling_rate"] == 48000.0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lfilter_vectors.json")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "iir_vectors.json"))


def test_library_lfilter_zi_and_lfiltic_equal_scipy():
    for c in GOLDEN["cases"]:
        b, a = np.array(c["b"]), np.array(c["a"])
        ic = filters.lfiltic(b, a, c["past_y"], c["past_x"])
        assert ic.shape == (c["order"],) and np.array_equal(ic, np.array(c["lfiltic"]))   # the same sums in the same order
        if c["lfilter_zi"] is None:
            with pytest.raises(ArgumentError, match="singular"):
                filters.lfilter_zi(b, a)
            continue
        ref = np.array(c["lfilter_zi"])
        zi = filters.lfilter_zi(b, a)
        assert zi.shape == ref.shape == (c["order"],)
        if not c["order"]:
            continue
        # two backward-stable solves of one system agree within a few eps x its condition number
        bn, an, n = O.normalise(b, a)
        cond = np.linalg.cond(np.eye(n) - O.companion(an))
        g = np.abs(zi - ref).max() / np.abs(ref).max()
        print(f"lfilter-zi-gap {c['name']}: {g:.1e} (condition {cond:.1e})")
        assert g <= 8 * np.finfo(np.float64).eps * cond, c["name"]


def test_chunk_and_tile_depend_on_the_order_only():
    lib = _lib.load()
    for n in range(0, 17):
        c, t = lib.nxsig_lfilter_chunk(n), lib.nxsig_lfilter_tile(n)
        assert c >= 32 and c % 32 == 0 and t == 64 * c, (n, c, t)
    assert [lib.nxsig_lfilter_chunk(n) for n in (0, 1, 4, 5, 16)] == [32, 32, 32, 64, 64]
    for n in (-1, 17):
        assert lib.nxsig_lfilter_chunk(n) == _lib.ERR_INVALID_ARG and "order must be in [0, 16]" in _lib.last_error()
        assert lib.nxsig_lfilter_tile(n) == _lib.ERR_INVALID_ARG


XS = np.zeros((2, 100), np.float32)
LB, LA = [0.2, 0.3], [1.0, -0.5, 0.25]
BAD = [
    ("a0 zero", dict(a=[0.0, 1.0]), ArgumentError, r"a\[0\] must not be zero"),
    ("b 2-D", dict(b=[[0.2, 0.3]]), ArgumentError, "b must be a real 1-D array"),
    ("a empty", dict(a=[]), ArgumentError, "at least one coefficient"),
    ("b nan", dict(b=[np.nan, 0.3]), ArgumentError, "finite"),
    ("a text", dict(a=["x", "y"]), ArgumentError, "a must be a real 1-D array"),
    ("b complex", dict(b=[1j, 0.3]), ArgumentError, "b must be a real 1-D array"),
    ("order 17", dict(a=np.r_[1.0, np.full(17, 0.01)]), NxSignalUnsupported, "sosfilt"),
    ("fir of order 17", dict(b=np.full(18, 0.01), a=[1.0]), NxSignalUnsupported, "filters.fir"),
    ("f64 samples", dict(x=np.zeros((2, 100), np.float64)), NxSignalUnsupported, "f32"),
    ("c64 samples", dict(x=np.zeros((2, 100), np.complex64)), NxSignalUnsupported, "f32"),
    ("scalar", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("axis", dict(axis=2), ArgumentError, "axis 2 is out of bounds"),
    ("empty", dict(x=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
]


@pytest.mark.parametrize("fn", ["lfilter", "filtfilt"])
@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(fn, case):
    _, change, exc, pattern = case
    kw = dict(x=XS, b=LB, a=LA)
    kw.update(change)
    x, b, a = kw.pop("x"), kw.pop("b"), kw.pop("a")
    with pytest.raises(exc, match=pattern) as ei:
        getattr(filters, fn)(x, b, a, **kw)
    assert fn in str(ei.value)


def test_the_checks_of_each_function():
    with pytest.raises(ArgumentError, match=r"invalid zi shape.*must have shape \(2, 2\), got \(2,\)"):
        filters.lfilter(XS, LB, LA, zi=np.zeros(2))
    with pytest.raises(ArgumentError, match=r"must have shape \(2, 100\)"):   # axis 0: the order takes the axis' place
        filters.lfilter(XS, LB, LA, zi=np.zeros((2, 2)), axis=0)
    with pytest.raises(ArgumentError, match="direction must be 0 or 1"):
        filters.lfilter(XS, LB, LA, direction=2)
    with pytest.raises(ArgumentError, match="greater than padlen, which is 100"):
        filters.filtfilt(XS, LB, LA, padlen=100)
    with pytest.raises(ArgumentError, match="greater than padlen, which is 9"):   # scipy's default: 3 * max(2, 3)
        filters.filtfilt(XS[:, :9], LB, LA)
    with pytest.raises(ArgumentError, match="padtype must be 'even', 'odd', 'constant', or None"):
        filters.filtfilt(XS, LB, LA, padtype="reflect")
    for padlen in (-1, 2.5, True):
        with pytest.raises(ArgumentError, match="padlen must be a non-negative integer"):
            filters.filtfilt(XS, LB, LA, padlen=padlen)
    with pytest.raises(NxSignalUnsupported, match="gust"):
        filters.filtfilt(XS, LB, LA, method="gust")
    with pytest.raises(ArgumentError, match="method must be 'pad' or 'gust'"):
        filters.filtfilt(XS, LB, LA, method="fft")
    with pytest.raises(ArgumentError, match=r"a\[0\] must not be zero"):
        filters.lfilter_zi(LB, [0.0, 1.0])
    with pytest.raises(ArgumentError, match="b must be a real 1-D array"):
        filters.lfiltic([[1.0]], LA, [0.0])
    assert filters.lfilter_zi([0.5], [1.0]).shape == (0,)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_lfilter_f32 / nxsig_filtfilt_f32 comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.LFILTER_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    for name in ("nxsig_lfilter_f32", "nxsig_filtfilt_f32"):
        rows = table[name]
        assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
        unsupported = {"order 17, recursive", "order 17, fir", "rows too large"}
        for k, r in rows.items():
            if k != "valid":
                assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
        assert "sosfilt" in rows["order 17, recursive"]["err"] and "filters.fir" in rows["order 17, fir"]["err"]
        assert _lib.SIGNATURES[name][1][0] is _lib._ctx_iir
    assert "null zi" not in table["nxsig_lfilter_f32"] and "null zf_out" not in table["nxsig_lfilter_f32"]   # optional
    assert "which is 12" in table["nxsig_filtfilt_f32"]["default padlen >= length"]["err"]
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()


def test_a_typed_context_pointer_that_is_not_null_reaches_the_library():
    lib, V = _lib.load(), C.c_void_p
    x, y, b, a = np.zeros(100, np.float32), np.zeros(100, np.float32), np.array(LB), np.array(LA)
    fake = _lib.ctx_ptr(V(64), _lib._ctx_iir)
    p = lambda v: v.ctypes.data_as(V)   # noqa: E731
    assert lib.nxsig_lfilter_f32(fake, p(x), 100, 0, 100, p(b), 2, p(a), 3, None, 1, None, 0, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "lfilter: batch and length must be >= 1" in _lib.last_error()
    assert lib.nxsig_filtfilt_f32(fake, p(x), 100, 1, 100, p(b), 2, p(a), 3, 9, -1, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "filtfilt: padtype must be" in _lib.last_error()


# ---- the conditioning guard.  The plan's verdict is read from the stand-alone program, which evaluates lf_tables on the catalogue.
def _san_exe():
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_lfilter")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_lfilter.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def san_output():
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([_san_exe()], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_host_side_under_asan_ubsan(san_output):
    """the argument checks, the geometry, lfilter_zi, the tables and the whole scan scheme played on the host (csrc/lfilter_plan.hpp)
    in a stand-alone program with ASan / UBSan; every filter the guard lets onto the scan within 1e-7 of the long double recurrence"""
    assert "sanitized lfilter host side ok" in san_output and "FAILED" not in san_output


def test_the_plans_tier_choice_for_the_catalogue(san_output):
    verdict = {m.group(2).strip(): m.group(1) for m in re.finditer(r"^(scan|generic)\s+(.+?)\s+order", san_output, re.M)}
    want = {"butter(2, .2)": "scan", "butter(4, .1)": "scan", "butter(2, 20 Hz, hp)": "scan", "butter(4, 20 Hz, hp)": "generic",
            "cheby1(8, 1, 100 Hz)": "generic", "butter(4, [.2, .4], bp)": "scan", "ellip(6, .5, 60, .3)": "scan", "butter(12, .3)": "generic", "bessel(14, .2)": "generic", "15 clustered poles": "generic",
            "butter(16, .4)": "scan", "integrator": "scan", "pre-emphasis .97": "scan", "gain 0.5": "scan", "butter(4, 60 Hz, hp)": "generic",
            "butter(3, 20 Hz, hp)": "generic", "a[0] = 2": "scan", "butter(9, .3)": "scan"}
    assert {k: verdict.get(k) for k in want} == want
    # every line of a filter on the scan carries its emulated error: at most 1e-7
    for m in re.finditer(r"^scan\s+.+?kappa \S+ plain \S+ scan (\S+)$", san_output, re.M):
        assert float(m.group(1)) <= 1e-7


# The guard case of tests/test_gpu_lfilter.py: butter(4, 60 Hz, "hp", fs = 48 kHz) on 6 000 samples of seed-0 normal noise.
# Measured here (numpy 2.2): (a) double against long double 4.4e-9 of the row maximum, (b) the scan without the guard 6.1e-2.
# For the record, the neighbours looked at: butter(4, 20 Hz) 2.4e-7 / 1.6e-4 by a chunk-to-chunk emulation (misses (a): 1e-7 at most),
# butter(3, 20 Hz) 3.4e-10 / 3.0e-6 and butter(3, 40 Hz) 5.3e-11 / 6.3e-8 (miss (b)), butter(4, 100 Hz) 9.5e-10 / 7.4e-4 (meets both)
# by the whole scheme of tests/san_lfilter.cpp on its own noise.
def guard_case():
    c = CASES["butter4_hp60"]
    b, a = np.array(c["b"]), np.array(c["a"])
    x = np.random.default_rng(0).standard_normal(6000).astype(np.float32)
    return b, a, x


def test_the_guard_case_is_fine_in_double_and_lost_on_an_unguarded_scan():
    b, a, x = guard_case()
    assert c_order(b, a) == 4
    x64 = x.astype(np.float64)[None]
    ref, _ = O.lfilter(b, a, x64, dtype=np.longdouble)
    plain, _ = O.lfilter(b, a, x64)
    e_plain = O.nerr(plain, ref)
    with np.errstate(all="ignore"):
        e_scan = O.nerr(O.scan_emulated(b, a, x64[0], _lib.load().nxsig_lfilter_chunk(4))[None], ref)
    print(f"lfilter-guard-case: double vs long double {e_plain:.1e}, unguarded scan {e_scan:.1e}")
    assert e_plain <= 1e-7                      # condition (a)
    assert not (e_scan < 1e-5)                  # condition (b): 1e-5 or more, or not a number at all
    # ... and the 20 Hz high-pass of order 2, which has to stay on the scan, is as good there as in the plain recurrence
    c = CASES["butter2_hp20"]
    b2, a2 = np.array(c["b"]), np.array(c["a"])
    ref2, _ = O.lfilter(b2, a2, x64, dtype=np.longdouble)
    assert O.nerr(O.scan_emulated(b2, a2, x64[0], _lib.load().nxsig_lfilter_chunk(2))[None], ref2) <= 1e-7


def c_order(b, a):
    return max(len(b), len(a)) - 1


def test_the_switch_the_sources_and_the_documents_are_in_place():
    assert "X(DISABLE_LFILTER_SCAN)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    src = read("nx_signal_amd", "csrc", "kernels_lfilter.hip")
    assert "tune(c, kT_DISABLE_LFILTER_SCAN, 0)" in src
    assert '("kernels_lfilter.hip", [])' in read("nx_signal_amd", "build.py")
    # no atomics, no single-precision arithmetic on the recurrence (the shared kernels of recurrence_scan.hpp included), nothing included
    # but the internal header and those kernels
    shared = read("nx_signal_amd", "csrc", "recurrence_scan.hpp")
    assert "atomic" not in src.lower() and re.findall(r'#include "([^"]+)"', src) == ["nxsig_internal.h", "recurrence_scan.hpp"]
    assert "atomic" not in shared.lower() and re.findall(r'#include "([^"]+)"', shared) == ["nxsig_internal.h"]
    assert "fmaf" not in src and "fmaf" not in shared
    assert 'dispatch_note("lfilter.scan")' in src and 'dispatch_note("lfilter.generic")' in src
    plan = read("nx_signal_amd", "csrc", "lfilter_plan.hpp")
    assert "hip" not in plan.replace("free of HIP", "").lower() and '#include "iir_plan.hpp"' in plan and "kLfGuardMax" in plan
    assert "NXSIG_DISABLE_LFILTER_SCAN" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.18" in design and "lfilter.scan" in design and "kappa" in design
    assert "lfilter" in read("README.md") and "bench_lfilter.py" in read("tools", "README.md") and "gen_lfilter_golden.py" in read("tools", "README.md")
    header = read("include", "nxsig.h")
    for name in ("nxsig_lfilter_f32", "nxsig_filtfilt_f32", "nxsig_lfilter_chunk", "nxsig_lfilter_tile", "nxsig_lfilter_zi"):
        assert name in header and name in _lib.SIGNATURES
    assert "NOT SCIPY'S" in header   # the non-finite rule of an FIR filter is the recurrence's
    # this change adds no NIF: the shim's table keeps its 76 entries
    assert "lfilter" not in read("nif", "nxsig_nif.c")
    assert S.filters.lfilter is filters.lfilter and callable(filters.filtfilt) and callable(filters.lfilter_zi) and callable(filters.lfiltic)
