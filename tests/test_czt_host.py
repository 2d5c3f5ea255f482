"""Transforms.czt / zoom_fft without a GPU: the numpy oracle (tests/czt_oracle.py) against recorded SciPy 1.15.3 results
(tests/golden/czt_vectors.json, tools/gen_czt_golden.py), the three tables of the C builder against exact rational phases, the tier
choice and the convolution length of csrc/czt_plan.hpp, a numpy single-precision emulation of the scheme built from the returned tables
(the project's 1e-5 bar on every recorded case, and the sweep the spiral gate is measured on), the argument checks of the Python
functions, every argument error of the C entry point (it validates before it looks at the context, so a null context reaches every
message), the switch / sources / documents, and the host side under ASan / UBSan in a stand-alone program (tests/san_czt.cpp)."""
import base64
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import czt_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _czt, _lib, transforms
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "czt_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_CZT) as f:
    ABI_GOLDEN = json.load(f)

SHAPES = [(1, 1), (3, 7), (600, 300), (512, 513), (513, 513), (1024, 1025), (1500, 549), (1025, 1025), (5000, 37), (100, 5000)]
# SciPy's general-w path is 1e-16 to 2e-11 of the row maximum from the direct sum at max(n, m) <= 1500 (3e-10 on the two longer shapes)
ORACLE_TOL = 1e-9
BAR = 1e-5        # the project's bar for a single-precision transform, of the row maximum
GATE = 32.0       # kCztSpreadGate of csrc/czt_plan.hpp


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).reshape(a["shape"]).copy()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def cplx(p):
    return None if p is None else complex(p[0], p[1])


def contour_of(c):
    if c["kind"] == "czt":
        return O.contour_czt(c["m"], cplx(c["w"]), cplx(c["a"]))
    return O.contour_zoom(c["fn"], c["m"], c["fs"], c["endpoint"])


def rows_of(c):
    """the samples of a case with the transformed axis last"""
    return np.moveaxis(dec(GOLDEN["inputs"][c["x"]]), c["axis"], -1)


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, y, at = rows_of(c), np.moveaxis(dec(c["y"]), c["axis"], -1), dec(c["at"])
    got = O.czt(x, c["m"], contour_of(c), at)
    assert got.shape == y.shape and y.dtype == np.complex128 and x.dtype in (np.float32, np.complex64)
    top = np.abs(y).max()
    gap = float(np.abs(got - y).max())
    print(f"czt-oracle-gap {c['name']}: {gap:.3e} absolute, {gap / top:.3e} of the row maximum")
    assert gap <= ORACLE_TOL * top, (c["name"], gap, top)


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    cs = {c["name"]: c for c in GOLDEN["cases"]}
    assert GOLDEN["scipy"] == "1.15.3" and [tuple(s) for s in GOLDEN["shapes"]] == SHAPES
    for n, m in SHAPES:
        for kind in ("czt", "czt_wa", "zoom", "zoom_scalar") + (("zoom_endpoint",) if m > 1 else ()):
            c = cs[f"n{n}_m{m}_{kind}"]
            assert dec(GOLDEN["inputs"][c["x"]]).shape == (n,) and c["m"] == m
    assert cs["n600_m300_czt"]["w"] is None and abs(abs(cplx(cs["n600_m300_czt_wa"]["w"])) - 1) < 1e-15
    assert cs["n600_m300_zoom_endpoint"]["endpoint"] is True and np.size(cs["n600_m300_zoom_scalar"]["fn"]) == 1
    spiral = cs["spiral_n64_m64"]
    assert abs(abs(cplx(spiral["w"])) - 1.0005) < 1e-12 and abs(abs(cplx(spiral["a"])) - 0.999) < 1e-12 and spiral["m"] == 64
    assert sum(c["axis"] == 0 for c in cs.values()) >= 2 and any(dec(GOLDEN["inputs"][c["x"]]).dtype == np.complex64 for c in cs.values())
    assert all(len(dec(c["at"])) <= 96 for c in cs.values())      # long results keep sampled places only
    assert {(s["n"], s["m"]) for s in GOLDEN["sweep"]} == {(64, 64), (600, 300)} and {s["spread"] for s in GOLDEN["sweep"]} == {4, 8, 16, 32, 64}
    assert os.path.getsize(FIXTURE) <= 256 << 10


@pytest.mark.parametrize("p", GOLDEN["points"], ids=lambda p: f"m{p['m']}")
def test_czt_points_equals_scipy(p):
    got = transforms.czt_points(p["m"], cplx(p["w"]), cplx(p["a"]))
    assert got.dtype == np.complex128 and np.array_equal(got, dec(p["y"]))
    with pytest.raises(ValueError, match="m must be positive and integer type"):
        transforms.czt_points(0)


# ---- the C builder of the tables
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def tables(lib, n, m, L, contour):
    A, F, W = np.empty(2 * n), np.empty(2 * L), np.empty(2 * m)
    spread = C.c_double()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rc = lib.nxsig_czt_tables(n, m, L, *contour, dp(A), dp(F), dp(W), C.byref(spread))
    return rc, A.view(np.complex128), F.view(np.complex128), W.view(np.complex128), spread.value


def exact_tables(n, m, L, contour):
    """A, v and W of include/nxsig.h in numpy double, the phases reduced by the oracle's integer arithmetic"""
    w_abs, w_step, w_den, a_abs, a_turns = contour
    half = O.turn_fraction(w_step, 2 * w_den)
    lw, la = math.log(w_abs), math.log(a_abs)

    def chirp(j):     # w^(j^2 / 2)
        j = j.astype(np.uint64)
        sq = j.astype(np.float64) ** 2
        return np.exp(0.5 * sq * lw) * np.exp(-2j * np.pi * O.reduced_turns(j * j, half))
    j, k = np.arange(n), np.arange(m)
    A = chirp(j) * np.exp(-j * la) * np.exp(-2j * np.pi * O.reduced_turns(j.astype(np.uint64), O.turn_fraction(a_turns)))
    v = np.zeros(L, np.complex128)
    v[:m] = 1.0 / chirp(k)
    if n > 1:
        v[L - n + 1:] = 1.0 / chirp(np.arange(n - 1, 0, -1))
    return A, v, chirp(k)


def turns_between(a, b):
    d = np.angle(a * np.conj(b)) / (2 * np.pi)
    return float(np.abs(d).max())


@pytest.mark.parametrize("n,m,contour", [
    (1 << 20, 1 << 20, O.contour_czt(1 << 20)),
    (1 << 20, 4096, O.contour_zoom([990.0, 1010.0], 4096, 48000.0)),
    (1000003, 777, O.contour_czt(777, np.exp(-0.37j), np.exp(0.2j))),
    (48000, 4096, O.contour_zoom([990.0, 1010.0], 4096, 48000.0, True)),
], ids=["dft-2^20", "zoom-2^20", "general-1000003", "zoom-48000-endpoint"])
def test_the_tables_against_exact_rational_phases(lib, n, m, contour):
    L = 1 << (n + m - 2).bit_length()
    rc, A, F, W, spread = tables(lib, n, m, L, contour)
    assert rc == 0 and spread == 1.0
    Ae, v, We = exact_tables(n, m, L, contour)
    ea, ew = turns_between(A, Ae), turns_between(W, We)
    Fe = np.fft.fft(v) / L
    ef = float(np.abs(F - Fe).max() / np.abs(Fe).max())
    print(f"czt-table-phase n={n} m={m} L={L}: A {ea:.2e} W {ew:.2e} of a turn, F {ef:.2e} of its maximum (f32 rounds at 6e-8)")
    # far under f32 rounding: the double sine of a 64-bit reduced phase, and one double transform against another
    assert ea <= 1e-15 and ew <= 1e-15 and ef <= 1e-12
    assert np.abs(np.abs(A) - 1).max() <= 4e-16 and np.abs(np.abs(W) - 1).max() <= 4e-16


def test_the_convolution_length_and_the_tier_at_their_edges(lib):
    for n, m, L in [(1, 1, 1024), (512, 513, 1024), (1024, 1, 1024), (513, 513, 2048), (1025, 1, 2048), (1024, 1025, 2048), (2048, 1, 2048),
                    (1025, 1025, 4096), (2049, 1, 4096), (1, 2049, 4096), (5000, 37, 8192), (100, 5000, 8192), (40000, 64, 65536)]:
        assert lib.nxsig_czt_conv_length(n, m) == L, (n, m)
    assert lib.nxsig_czt_conv_length(0, 1) == _lib.ERR_INVALID_ARG and lib.nxsig_czt_conv_length(1, 0) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_czt_conv_length(1 << 30, 2) == _lib.ERR_UNSUPPORTED
    # L must be a power of two that holds the convolution; a refused contour still reports its spread
    rc, *_ = tables(lib, 600, 300, 1000, O.contour_czt(300))
    assert rc == _lib.ERR_INVALID_ARG
    rc, *_ = tables(lib, 600, 300, 512, O.contour_czt(300))
    assert rc == _lib.ERR_INVALID_ARG
    rc, _, _, _, spread = tables(lib, 64, 64, 128, O.contour_czt(64, 1.01 * np.exp(-0.1j)))
    assert rc == _lib.ERR_UNSUPPORTED and spread > GATE and "the contour leaves single precision" in _lib.last_error()


@pytest.fixture(scope="module")
def plan():
    """csrc/czt_plan.hpp behind three C functions, in a small shared library of its own (plain g++: the header has no HIP types)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    src, so = os.path.join(build, "czt_plan_c.cpp"), os.path.join(build, "czt_plan_c.so")
    with open(src, "w") as f:
        f.write('#include "czt_plan.hpp"\nextern "C" {\n'
                "int cz_tier(long long n, long long m, int off) { return nxsig::czt_tier(n, m, off != 0); }\n"
                "long long cz_length(long long n, long long m, int off) { return nxsig::czt_conv_length(n, m, off != 0); }\n"
                "double cz_gate() { return nxsig::kCztSpreadGate; }\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    lib.cz_tier.argtypes, lib.cz_length.argtypes = [C.c_longlong, C.c_longlong, C.c_int], [C.c_longlong, C.c_longlong, C.c_int]
    lib.cz_length.restype, lib.cz_gate.restype = C.c_longlong, C.c_double
    return lib


def test_the_tier_choice(plan):
    for n, m in [(1, 1), (512, 513), (513, 513), (1024, 1025), (1500, 549), (2048, 1), (1, 2048), (1000, 25)]:
        assert plan.cz_tier(n, m, 0) == 0 and plan.cz_tier(n, m, 1) == 1, (n, m)
        assert plan.cz_length(n, m, 0) == (1024 if n + m - 1 <= 1024 else 2048)
        assert plan.cz_length(n, m, 1) == 1 << (n + m - 2).bit_length()
    for n, m in [(1025, 1025), (2049, 1), (1, 2049), (5000, 37), (100, 5000), (40000, 64)]:
        assert plan.cz_tier(n, m, 0) == 1 and plan.cz_length(n, m, 0) == plan.cz_length(n, m, 1) == 1 << (n + m - 2).bit_length()
    assert plan.cz_gate() == GATE


# ---- the scheme in numpy single precision, from the tables the device multiplies by
def emulate(x, m, L, A, F, W):
    A, F, W = A.astype(np.complex64), F.astype(np.complex64), W.astype(np.complex64)
    z = np.zeros(x.shape[:-1] + (L,), np.complex64)
    z[..., :x.shape[-1]] = x.astype(np.complex64) * A
    s = (np.fft.fft(z).astype(np.complex64) * F).astype(np.complex64)
    assert s.dtype == np.complex64
    y = (np.fft.ifft(s).astype(np.complex64) * np.float32(L)).astype(np.complex64)
    return (y[..., :m] * W).astype(np.complex64)


def worst_row(got, want):
    top = np.abs(want).max(axis=-1, keepdims=True)
    return float((np.abs(got - want) / top).max())


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_single_precision_emulation_meets_the_bar(lib, c):
    x, m, contour = rows_of(c), c["m"], contour_of(c)
    n = x.shape[-1]
    want = O.czt(x, m, contour)
    for L in sorted({lib.nxsig_czt_conv_length(n, m), 1 << (n + m - 2).bit_length()}):     # the wave tier's and the generic tier's
        rc, A, F, W, _ = tables(lib, n, m, L, contour)
        assert rc == 0, _lib.last_error()
        err = worst_row(emulate(x, m, L, A, F, W), want)
        print(f"czt-emulation {c['name']} L={L}: {err:.2e} of the row maximum")
        assert err <= BAR, (c["name"], L, err)


def test_the_spiral_gate_is_the_measured_one(lib):
    """the recorded sweep: the emulated error stays a decade under the bar at every spread up to the gate (the C builder serves those
    and refuses the rest, whose tables come from exact_tables); the figures beyond it are printed, and DESIGN.md keeps them"""
    inside = []
    for s in GOLDEN["sweep"]:
        n, m, contour = s["n"], s["m"], O.contour_czt(s["m"], cplx(s["w"]), cplx(s["a"]))
        x, L = dec(GOLDEN["inputs"][s["x"]]), lib.nxsig_czt_conv_length(s["n"], s["m"])
        rc, A, F, W, spread = tables(lib, n, m, L, contour)
        assert abs(spread - s["spread"]) <= 1e-6 * s["spread"]
        assert (rc == 0) == (s["spread"] <= GATE), (s, rc)
        if rc:
            A, v, W = exact_tables(n, m, L, contour)
            F = np.fft.fft(v) / L
        err = worst_row(emulate(x, m, L, A, F, W), O.czt(x, m, contour))
        side = "|w| > 1" if abs(cplx(s["w"])) > 1 else "|w| < 1"
        print(f"czt-spiral-sweep n={n} m={m} {side} spread {s['spread']}: {err:.2e} of the row maximum{'' if rc == 0 else ' (refused)'}")
        if rc == 0:
            inside.append(err)
    assert len(inside) == 16 and max(inside) <= BAR / 10, inside


# ---- the Python functions
X32 = np.zeros(32, np.float32)
BAD = [
    ("czt", "f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64"),
    ("czt", "c128", dict(x=np.zeros(32, np.complex128)), NxSignalUnsupported, "unsupported type complex128"),
    ("czt", "text", dict(x=np.array(["a"] * 32)), ArgumentError, "unsupported type"),
    ("czt", "rank 0", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("czt", "empty axis", dict(x=np.zeros((2, 0), np.float32)), ValueError, "Invalid number of CZT data points (0) specified. n must be positive and integer type."),
    ("czt", "empty dimension", dict(x=np.zeros((0, 4), np.float32)), ArgumentError, "empty dimension"),
    ("czt", "axis", dict(axis=1), ArgumentError, "axis 1 is out of bounds"),
    ("czt", "m 0", dict(m=0), ValueError, "Invalid number of CZT output points (0) specified. m must be positive and integer type."),
    ("czt", "m float", dict(m=8.0), ValueError, "Invalid number of CZT output points (8.0) specified. m must be positive and integer type."),
    ("czt", "w 0", dict(w=0.0), ArgumentError, "w must be finite and non-zero"),
    ("czt", "w nan", dict(w=complex("nan")), ArgumentError, "w must be finite and non-zero"),
    ("czt", "w text", dict(w="fast"), ArgumentError, "w must be a number"),
    ("czt", "a inf", dict(a=float("inf")), ArgumentError, "a must be finite and non-zero"),
    ("czt", "size", dict(m=1 << 30), NxSignalUnsupported, "n + m - 1 must be at most 2^30"),
    ("zoom_fft", "fn three", dict(fn=[0.1, 0.2, 0.3]), ValueError, "fn must be a scalar or 2-length sequence"),
    ("zoom_fft", "fn empty", dict(fn=[]), ValueError, "fn must be a scalar or 2-length sequence"),
    ("zoom_fft", "fn nan", dict(fn=[0.1, float("nan")]), ArgumentError, "must be finite"),
    ("zoom_fft", "fn text", dict(fn="low"), ArgumentError, "must be real numbers"),
    ("zoom_fft", "fs 0", dict(fs=0), ArgumentError, "fs non-zero"),
    ("zoom_fft", "endpoint", dict(endpoint=1), ArgumentError, "endpoint must be a boolean"),
    ("zoom_fft", "endpoint m 1", dict(m=1, endpoint=True), ValueError, "endpoint=True needs m >= 2"),
    ("zoom_fft", "m -3", dict(m=-3), ValueError, "Invalid number of CZT output points (-3) specified."),
    ("zoom_fft", "f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64"),
    ("zoom_fft", "axis", dict(axis=-2), ArgumentError, "axis -2 is out of bounds"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: f"{c[0]}-{c[1]}")
def test_arguments_are_checked_before_anything_runs(case, monkeypatch):
    """every Python-side error comes before the library is loaded"""
    fn, _, change, error, pattern = case

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    kw = dict(x=X32)
    if fn == "zoom_fft":
        kw["fn"] = [0.1, 0.3]
    kw.update(change)
    with pytest.raises(error, match=re.escape(pattern)):
        if fn == "czt":
            transforms.czt(kw.pop("x"), **kw)
        else:
            transforms.zoom_fft(kw.pop("x"), kw.pop("fn"), **kw)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_czt comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.CZT_TABLE_ENTRIES)
    rows, golden = table["nxsig_czt"], ABI_GOLDEN["null_ctx"]["nxsig_czt"]
    assert rows.keys() == golden.keys()
    for k in rows:
        assert rows[k] == golden[k], (k, rows[k], golden[k])
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    assert rows["batch=0"] == rows["valid"]        # batch = 0 passes every check and reaches the context
    unsupported = {"n+m-1=2^30+1", "m=2^31", "w_den=2^62", "spiral beyond the gate", "start beyond the gate", "rows too large", "result too large"}
    for k, r in rows.items():
        if k not in ("valid", "batch=0"):
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
            assert r["err"].startswith("czt: ") or k == "mem=7", (k, r)
    assert rows["spiral beyond the gate"]["err"] == "czt: the contour leaves single precision"
    assert {"null x", "null out", "length=0", "m=0", "batch=-1", "batch_stride=length-1", "w_den=0", "w_abs=0", "a_abs=0", "mem=7"} <= set(rows)
    assert _lib.SIGNATURES["nxsig_czt"][1][0] is _lib._ctx_iir
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and set(ABI_GOLDEN["real_ctx"]["nxsig_czt"]) == set(rows) - {"batch=0"}
    assert ABI_GOLDEN["real_ctx"]["nxsig_czt"]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}


def test_overlapping_operands_are_refused_ahead_of_the_context():
    lib = _lib.load()
    buf = np.zeros(64, np.complex64)
    x = buf[:24].view(np.float32)[:24]
    args = (0, 24, 1, 24, 13, 1.0, 0.4, 13, 1.0, 0.05)
    rc = lib.nxsig_czt(None, x.ctypes.data_as(C.c_void_p), *args, buf.ctypes.data_as(C.c_void_p), _lib.HOST)
    assert rc == _lib.ERR_INVALID_ARG and _lib.last_error() == "czt: x and out must not overlap"
    rc = lib.nxsig_czt(None, x.ctypes.data_as(C.c_void_p), *args, buf[12:].ctypes.data_as(C.c_void_p), _lib.HOST)   # 96 bytes on: disjoint
    assert rc == _lib.ERR_INVALID_ARG and _lib.last_error() == "null context"


def test_the_switch_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(CZT_WAVE)" in internal and "kScratchSlots = 32" in internal and '#include "czt_plan.hpp"' in internal
    src = read("nx_signal_amd", "csrc", "kernels_czt.hip")
    assert "tune(c, kT_CZT_WAVE, 1)" in src and "tune(c, kT_DISABLE_WAVE, 0)" in src and '("kernels_czt.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["wave_stft.hpp"]
    assert not re.findall(r"\batomic[A-Z]\w*", src)
    assert 'dispatch_note("czt.wave")' in src and 'dispatch_note("czt.generic")' in src
    assert "wave_fft_core_T<K>" in src and "wave_fft_core<K, true, true>" in src
    # the generic tier's two temporaries are its own buffers in the context
    assert src.count("own_buffer(c, c->czt_") == 2 and "} czt_rows, czt_spectra;" in internal and "hipStreamIsCapturing" not in src
    assert src.count("ctx_table(") == 3 and src.count("launch_fft(") == 2
    plan = read("nx_signal_amd", "csrc", "czt_plan.hpp")
    for name in ("czt_check", "czt_tier", "czt_conv_length", "czt_turn_fraction", "czt_tables", "czt_spread", "czt_pair_state", "czt_slot_sample",
                 "kCztSpreadGate"):
        assert name in plan, name
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_czt.hip", "")
    assert "czt_plan.hpp" in read("tests", "san_czt.cpp")
    assert "NXSIG_CZT_WAVE" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.20" in design and "czt.wave" in design and "czt.generic" in design and "kCztSpreadGate" in design
    readme = read("README.md")
    assert "transforms.czt" in readme and "zoom_fft" in readme and "_czt.py" in readme
    tools = read("tools", "README.md")
    assert "bench_czt.py" in tools and "gen_czt_golden.py" in tools and "--czt" in tools
    header = read("include", "nxsig.h")
    assert re.search(r"\bint nxsig_czt\(nxsig_ctx\* ctx, const void\* x, int32_t is_complex, int64_t length, int64_t batch, int64_t batch_stride, int64_t m,", header)
    assert re.search(r"\bint64_t nxsig_czt_conv_length\(int64_t n, int64_t m\);", header) and "nxsig_czt_tables(" in header
    for phrase in ("THE DEFINITION", "X[k] = sum_{j<n} x[j] a^(-j) w^(j k)", "czt.wave", "czt.generic", "NXSIG_CZT_WAVE", "no finite output element",
                   "the contour leaves single", "Not built", "Every argument check comes ahead of the context"):
        assert phrase in header[header.index("Transforms.czt"):], phrase
    for name in ("nxsig_czt", "nxsig_czt_conv_length", "nxsig_czt_tables"):
        assert name in _lib.SIGNATURES
    # no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "czt" not in nif and "czt" not in read("elixir", "lib", "nx_signal_amd", "transforms.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.transforms.czt is transforms.czt is _czt.czt and transforms.zoom_fft is _czt.zoom_fft and transforms.czt_points is _czt.czt_points
    assert transforms.czt.__module__ == "nx_signal_amd._czt"
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_czt.py"))


def test_the_private_module_can_be_imported_first():
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._czt as m, nx_signal_amd.transforms as t; "
                        "assert t.czt is m.czt and t.zoom_fft is m.zoom_fft"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks over a sweep with the rejected ones, the tier and the convolution length at their edges, the phase reduction
    against exact integers, the tables against the identity they serve, and the fused kernel's row and lane arithmetic walked over
    exactly sized buffers (csrc/czt_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_czt")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_czt.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized czt host side ok" in r.stdout
