"""Filters.sosfilt / sosfilt_zi / sosfiltfilt without a GPU: the f64 oracle (tests/iir_oracle.py) against recorded scipy results
(tests/golden/iir_vectors.json, tools/gen_iir_golden.py), sosfilt_zi and the geometry queries of the library, the argument checks of the
Python functions, every argument error of the two C entry points (they validate before they look at the context, so a null context
reaches every message), the typed context pointer, the switch / sources / documents, and the host side under ASan / UBSan in a
stand-alone program (tests/san_iir.cpp)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import iir_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "iir_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_IIR) as f:
    ABI_GOLDEN = json.load(f)
X = np.array(GOLDEN["x"], np.float32).astype(np.float64)   # f32 values, recorded in their shortest form
AT = GOLDEN["at"]   # the samples of every output that are recorded: every sixteenth and the last


def gap(y, recorded):
    """largest error at the recorded samples over the largest recorded magnitude of the row"""
    return O.nerr(y[:, AT], np.array(recorded))

# The oracle runs scipy's recurrence in scipy's order of operations, so the gap to the recorded results was MEASURED as 0.0 on every
# cascade and function (numpy 2.2, scipy 1.15.3).  Ten times that is no bound another numpy build could meet (a fused multiply-add in
# either, another LAPACK in sosfilt_zi's 2 x 2 solve), so the bound is the round-off such a build may add: 160 samples of relative
# 1.1e-16 steps through poles of radius up to 0.999999 — the 1e-13 the issue expects.
ORACLE_TOL = 1e-13


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    sos = np.array(c["sos"])
    assert GOLDEN["scipy"] and sos.shape == (c["n_sections"], 6)
    y, _ = O.sosfilt(sos, X)
    gaps = {"y": gap(y, c["y"])}
    zi = np.array(c["zi"]).transpose(1, 0, 2)   # scipy: (n_sections, rows, 2)
    y, zf = O.sosfilt(sos, X, zi)
    zf_ref = np.array(c["zf"]).transpose(1, 0, 2)
    gaps["y_zi"] = gap(y, c["y_zi"])
    gaps["zf"] = float(np.abs(zf - zf_ref).max() / np.abs(zf_ref).max())
    if c["sosfilt_zi"] is None:   # a pole at z = 1: scipy raised LinAlgError, and so does the oracle
        with pytest.raises(np.linalg.LinAlgError):
            O.sosfilt_zi(sos)
        assert "sosfiltfilt" not in c
    else:
        ref = np.array(c["sosfilt_zi"])
        gaps["sosfilt_zi"] = float(np.abs(O.sosfilt_zi(sos) - ref).max() / np.abs(ref).max())
        assert O.default_padlen(sos) == c["default_padlen"]
        for padtype, ref in c["sosfiltfilt"].items():
            gaps["sosfiltfilt " + padtype] = gap(O.sosfiltfilt(sos, X, None if padtype == "None" else padtype), ref)
    print(f"iir-oracle-gap {c['name']}: " + ", ".join(f"{k} {v:.1e}" for k, v in gaps.items()))
    assert max(gaps.values()) <= ORACLE_TOL, gaps
    # the recurrence itself (no LAPACK in it) under the numpy that recorded the fixture: ten times the gap measured then, which was 0
    if np.__version__ == GOLDEN["numpy"]:
        assert max(gaps["y"], gaps["y_zi"], gaps["zf"]) <= 10 * c["oracle_gap"], (gaps, c["oracle_gap"])


def test_the_recorded_cascades_are_the_ones_the_issue_lists():
    cs = {c["name"]: c for c in GOLDEN["cases"]}
    assert [cs[n]["n_sections"] for n in ("butter4_lp4k", "butter2_hp20", "butter4_hp20", "ellip4_bp", "cheby1_8_lp100", "ellip16_bp",
                                          "ellip20_bp", "integrator", "unstable_r1001")] == [2, 1, 2, 4, 4, 16, 20, 1, 1]
    assert cs["integrator"]["sos"] == [[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]] and abs(cs["unstable_r1001"]["largest_pole"] - 1.001) < 1e-12
    assert abs(cs["cheby1_8_lp100"]["largest_pole"] - 0.99954) < 1e-5 and GOLDEN["sampling_rate"] == 48000.0
    assert X.shape[0] == 2 and 100 <= X.shape[1] <= 400 and len(cs) == 9 and AT[-1] == X.shape[1] - 1 and len(AT) >= 10


def test_library_sosfilt_zi_equals_scipy():
    for c in GOLDEN["cases"]:
        sos = np.array(c["sos"])
        if c["sosfilt_zi"] is None:
            with pytest.raises(ArgumentError, match="singular"):
                filters.sosfilt_zi(sos)
            continue
        ref = np.array(c["sosfilt_zi"])
        zi = filters.sosfilt_zi(sos)
        # two backward-stable solves of one 2 x 2 system agree within a few eps x its condition number (5.8e5 for the 20 Hz high-passes,
        # whose 1 + a1 + a2 is 3e-6); measured: at most 6.5e-13, on cheby1(8, 1 dB, 100 Hz)
        cond = max(np.linalg.cond(np.array([[1.0 + s[4], -1.0], [s[5], 1.0]])) for s in sos)
        gap = np.abs(zi - ref).max() / np.abs(ref).max()
        print(f"iir-zi-gap {c['name']}: {gap:.1e} (condition {cond:.1e})")
        assert zi.shape == ref.shape and gap <= 8 * np.finfo(np.float64).eps * cond, c["name"]


def test_chunk_and_tile_depend_on_the_section_count_only():
    lib = _lib.load()
    for s in range(1, 17):
        c, t = lib.nxsig_sosfilt_chunk(s), lib.nxsig_sosfilt_tile(s)
        assert c >= 32 and c % 32 == 0 and t == 64 * c, (s, c, t)
    assert [lib.nxsig_sosfilt_chunk(s) for s in (1, 2, 3, 16)] == [32, 32, 64, 64]
    for s in (0, -1, 17):
        assert lib.nxsig_sosfilt_chunk(s) == _lib.ERR_INVALID_ARG and "n_sections must be in [1, 16]" in _lib.last_error()
        assert lib.nxsig_sosfilt_tile(s) == _lib.ERR_INVALID_ARG


XS = np.zeros((2, 100), np.float32)
LP = np.array([[0.02, 0.04, 0.02, 1.0, -1.2, 0.4]])
BAD = [
    ("a0 != 1", dict(sos=[[0.02, 0.04, 0.02, 2.0, -1.2, 0.4]]), ArgumentError, r"sos\[:, 3\] should be all ones"),
    ("sos 1-D", dict(sos=[0.02, 0.04, 0.02, 1.0, -1.2, 0.4]), ArgumentError, "sos array must be 2D"),
    ("sos five columns", dict(sos=[[0.02, 0.04, 0.02, 1.0, -1.2]]), ArgumentError, r"sos array must be shape \(n_sections, 6\)"),
    ("sos empty", dict(sos=np.zeros((0, 6))), ArgumentError, r"shape \(n_sections, 6\)"),
    ("sos nan", dict(sos=[[np.nan, 0.04, 0.02, 1.0, -1.2, 0.4]]), ArgumentError, "finite"),
    ("sos text", dict(sos=[["a"] * 6]), ArgumentError, "real array"),
    ("f64 samples", dict(x=np.zeros((2, 100), np.float64)), NxSignalUnsupported, "f32"),
    ("c64 samples", dict(x=np.zeros((2, 100), np.complex64)), NxSignalUnsupported, "f32"),
    ("scalar", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("axis", dict(axis=2), ArgumentError, "axis 2 is out of bounds"),
    ("empty", dict(x=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
]


@pytest.mark.parametrize("fn", ["sosfilt", "sosfiltfilt"])
@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(fn, case):
    _, change, exc, pattern = case
    kw = dict(x=XS, sos=LP)
    kw.update(change)
    x, sos = kw.pop("x"), kw.pop("sos")
    with pytest.raises(exc, match=pattern) as ei:
        getattr(filters, fn)(x, sos, **kw)
    assert fn in str(ei.value)


def test_the_checks_of_each_function():
    with pytest.raises(ArgumentError, match=r"invalid zi shape.*must have shape \(1, 2, 2\), got \(1, 2\)"):
        filters.sosfilt(XS, LP, zi=np.zeros((1, 2)))
    with pytest.raises(ArgumentError, match=r"must have shape \(1, 2, 100\)"):   # axis 0: the 2 takes the axis' place
        filters.sosfilt(XS, LP, zi=np.zeros((1, 2, 2)), axis=0)
    with pytest.raises(ArgumentError, match="direction must be 0 or 1"):
        filters.sosfilt(XS, LP, direction=2)
    with pytest.raises(ArgumentError, match="greater than padlen, which is 100"):
        filters.sosfiltfilt(XS, LP, padlen=100)
    with pytest.raises(ArgumentError, match="greater than padlen, which is 9"):   # scipy's default: 3 * (2 + 1 - 0)
        filters.sosfiltfilt(XS[:, :9], LP)
    with pytest.raises(ArgumentError, match="padtype must be 'even', 'odd', 'constant', or None"):
        filters.sosfiltfilt(XS, LP, padtype="reflect")
    for padlen in (-1, 2.5, True):
        with pytest.raises(ArgumentError, match="padlen must be a non-negative integer"):
            filters.sosfiltfilt(XS, LP, padlen=padlen)
    with pytest.raises(NxSignalUnsupported, match="up to 16 sections"):
        filters.sosfiltfilt(XS, np.tile(LP, (17, 1)))
    with pytest.raises(ArgumentError, match="sos array must be 2D"):
        filters.sosfilt_zi([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_sosfilt_f32 / nxsig_sosfiltfilt_f32 comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.IIR_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    for name in ("nxsig_sosfilt_f32", "nxsig_sosfiltfilt_f32"):
        rows = table[name]
        assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
        unsupported = {"n_sections=17", "rows too large"}
        for k, r in rows.items():
            if k != "valid":
                assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
        assert _lib.SIGNATURES[name][1][0] is _lib._ctx_iir and _lib._ctx_iir not in (_lib._p, _lib._ctx, _lib._ctx_spectral)
    assert _lib._ctx_iir in _lib.TYPED_CTX
    assert "null zi" not in table["nxsig_sosfilt_f32"] and "null zf_out" not in table["nxsig_sosfilt_f32"]   # optional
    assert "which is 15" in table["nxsig_sosfiltfilt_f32"]["default padlen >= length"]["err"]
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()


def test_a_typed_context_pointer_that_is_not_null_reaches_the_library():
    """the argument checks come ahead of the context, so a made-up non-null context with batch = 0 is refused and never looked at; the
    conversion of the typed pointer itself is what runs here"""
    lib, V = _lib.load(), C.c_void_p
    x, y, sos = np.zeros(100, np.float32), np.zeros(100, np.float32), np.ascontiguousarray(LP)
    fake = _lib.ctx_ptr(V(64), _lib._ctx_iir)
    assert isinstance(fake, _lib._ctx_iir) and _lib.ctx_ptr(None, _lib._ctx_iir) is None
    p = lambda a: a.ctypes.data_as(V)   # noqa: E731
    assert lib.nxsig_sosfilt_f32(fake, p(x), 100, 0, 100, p(sos), 1, None, 1, None, 0, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "sosfilt: batch and length must be >= 1" in _lib.last_error()
    assert lib.nxsig_sosfiltfilt_f32(fake, p(x), 100, 1, 100, p(sos), 1, 9, -1, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "sosfiltfilt: padtype must be" in _lib.last_error()


def test_the_switch_the_sources_and_the_documents_are_in_place():
    assert "X(DISABLE_SOSFILT_SCAN)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    src = read("nx_signal_amd", "csrc", "kernels_iir.hip")
    assert "tune(c, kT_DISABLE_SOSFILT_SCAN, 0)" in src
    assert '("kernels_iir.hip", [])' in read("nx_signal_amd", "build.py")
    # no atomics, no single-precision arithmetic on the recurrence (the shared kernels of recurrence_scan.hpp included), nothing included
    # but the internal header and those kernels
    shared = read("nx_signal_amd", "csrc", "recurrence_scan.hpp")
    assert "atomic" not in src.lower() and re.findall(r'#include "([^"]+)"', src) == ["nxsig_internal.h", "recurrence_scan.hpp"]
    assert "atomic" not in shared.lower() and re.findall(r'#include "([^"]+)"', shared) == ["nxsig_internal.h"]
    assert "fmaf" not in src and "fmaf" not in shared
    assert 'dispatch_note("sosfilt.scan")' in src and 'dispatch_note("sosfilt.generic")' in src
    assert "NXSIG_DISABLE_SOSFILT_SCAN" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.13" in design and "NxSignalAMD.Filters.sosfilt" in design and "lfilter" in design
    assert "sosfilt" in read("README.md") and "bench_iir.py" in read("tools", "README.md") and "gen_iir_golden.py" in read("tools", "README.md")
    header = read("include", "nxsig.h")
    for name in ("nxsig_sosfilt_f32", "nxsig_sosfiltfilt_f32", "nxsig_sosfilt_chunk", "nxsig_sosfilt_tile", "nxsig_sosfilt_zi"):
        assert name in header and name in _lib.SIGNATURES
    # this change adds no NIF: the shim's table keeps its 76 entries
    assert "sosfilt" not in read("nif", "nxsig_nif.c")
    assert S.filters.sosfilt is filters.sosfilt and callable(filters.sosfiltfilt) and callable(filters.sosfilt_zi)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks, the geometry, sosfilt_zi, A^C against C steps of the recurrence and the whole scan scheme played on the host
    (csrc/iir_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_iir")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_iir.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized iir host side ok" in r.stdout
