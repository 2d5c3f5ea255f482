"""Transforms.cwt / Filters.fir_bank without a GPU: the numpy oracle (tests/cwt_oracle.py) against the recorded vectors and the two
spot checks of the definition (tests/golden/cwt_vectors.json, tools/gen_cwt_golden.py), its convolution against scipy.signal.convolve,
the two host helpers of the C ABI against the oracle, the class split and block step of csrc/cwt_plan.hpp at their edges, a numpy
single-precision restatement of the overlap-save scheme held to the GPU test's bar, the argument checks of the Python functions, every
argument error of the two C entry points (they validate before they look at the context, so a null context reaches every message), the
switch / sources / documents, and the host side under ASan / UBSan in a stand-alone program (tests/san_cwt.cpp)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft
import scipy.signal

import cwt_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _cwt, _lib, filters, transforms
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "cwt_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_CWT) as f:
    ABI_GOLDEN = json.load(f)

BAR = 1e-5   # the project's bar for a single-precision transform, of the (row, scale) maximum


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the oracle
@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_the_recorded_vectors(c):
    x = np.array(c["x"], np.float32)
    y = np.array(c["re"]) + 1j * np.array(c["im"])
    got = O.cwt(x, c["widths"], c["wavelet"], c["w"], kind="complex")
    assert got.shape == y.shape == (len(c["widths"]), c["L"]) and [O.support(a, c["L"]) for a in c["widths"]] == c["supports"]
    assert np.abs(got - y).max() <= 1e-13 * max(np.abs(y).max(), 1e-300)


def test_the_recorded_cases_cover_the_supports_the_issue_names():
    sup = {n for c in GOLDEN["cases"] for n in c["supports"]}
    assert 1 in sup and any(n % 2 == 0 for n in sup) and any(n % 2 == 1 and n > 1 for n in sup)
    assert any(n == c["L"] and O.support(a, 10 ** 9) > c["L"] for c in GOLDEN["cases"] for n, a in zip(c["supports"], c["widths"]))   # capped by L
    assert all(c["L"] <= 64 for c in GOLDEN["cases"]) and os.path.getsize(os.path.join(ROOT, "tests", "golden", "cwt_vectors.json")) < 64 * 1024


def test_the_two_spot_checks_of_the_definition():
    ramp = GOLDEN["spot_ramp"]
    got = O.cwt(np.arange(8.0), ramp["widths"], "ricker")[0]
    assert got.dtype == np.float64 and np.abs(got - np.array(ramp["y"])).max() <= 5e-9 * np.abs(got).max()   # nine recorded digits
    imp = GOLDEN["spot_impulse"]
    L, p = imp["L"], imp["p"]
    x = np.zeros(L)
    x[p] = 1.0
    y = O.cwt(x, imp["widths"], imp["wavelet"], imp["w"])
    for s, a in enumerate(imp["widths"]):
        h = O.taps(imp["wavelet"], a, L, imp["w"])
        N = len(h)
        want = np.zeros(L, np.complex128)
        for n in range(L):
            j = n - p + (N - 1) // 2
            if 0 <= j < N:
                want[n] = h[j]
        assert np.array_equal(y[s], want), (s, a)


def test_the_oracles_convolution_is_scipys_same():
    rng = np.random.Generator(np.random.PCG64(3))
    for L, N in [(1, 1), (2, 1), (2, 2), (37, 10), (37, 25), (37, 37), (64, 45), (10, 23), (10, 24)]:   # N > L: fir_bank takes such filters
        x = rng.standard_normal(L)
        h = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        ref = scipy.signal.convolve(x, h, "same", method="direct")
        assert ref.shape == (L,) and np.abs(O.same(x, h) - ref).max() <= 1e-13 * np.abs(ref).max()
    x = rng.standard_normal((2, 3, 16))
    bank = [rng.standard_normal(5), rng.standard_normal(8)]
    y = O.fir_bank(x, bank, "power")
    assert y.shape == (2, 3, 2, 16) and np.allclose(y[1, 2, 1], O.same(x[1, 2], bank[1]) ** 2)
    assert np.array_equal(O.sink(np.array([3 + 4j]), "magnitude"), [5.0]) and np.array_equal(O.sink(np.array([3 + 4j]), "real"), [3.0])


# ---- the host helpers of the C ABI
def test_support_and_wavelet_helpers_against_the_oracle():
    lib = _lib.load()
    for a, L in [(0.1, 100), (1.0, 100), (2.5, 100), (4.5, 100), (10.0, 37), (0.35, 9), (51.3, 5000), (51.4, 5000), (102.5, 5000), (102.6, 5000),
                 (1e-300, 3), (1e300, 3), (7.0, 1)]:
        assert lib.nxsig_cwt_support(a, L) == O.support(a, L), (a, L)
    assert lib.nxsig_cwt_support(0.0, 8) == _lib.ERR_INVALID_ARG and "width must be positive and finite" in _lib.last_error()
    assert lib.nxsig_cwt_support(float("nan"), 8) == _lib.ERR_INVALID_ARG and lib.nxsig_cwt_support(1.0, 0) == _lib.ERR_INVALID_ARG
    worst = 0.0
    for name, code in (("morlet2", 0), ("ricker", 1)):
        for a, L, w in [(0.1, 100, 5.0), (1.0, 100, 5.0), (2.5, 100, 5.0), (4.5, 100, 3.0), (10.0, 37, 5.0), (10.0, 36, 6.0), (51.3, 5000, 5.0), (0.7, 1, 5.0)]:
            N = O.support(a, L)       # N = 1, even and odd N, N capped by L
            out = np.zeros(2 * N)
            assert lib.nxsig_cwt_wavelet(code, a, w, N, out.ctypes.data_as(C.POINTER(C.c_double))) == 0, _lib.last_error()
            got, ref = out[0::2] + 1j * out[1::2], O.taps(name, a, L, w)
            assert ref.shape == (N,)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= 1e-15, (name, a, L, err)
            if name == "ricker":
                assert not out[1::2].any()
    print(f"cwt-wavelet-helper worst relative gap: {worst:.3e}")
    out = np.zeros(4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nxsig_cwt_wavelet(2, 1.0, 5.0, 2, p) == _lib.ERR_INVALID_ARG and lib.nxsig_cwt_wavelet(0, -1.0, 5.0, 2, p) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_cwt_wavelet(0, 1.0, 5.0, 0, p) == _lib.ERR_INVALID_ARG and lib.nxsig_cwt_wavelet(0, 1.0, 5.0, 2, None) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_cwt_wavelet(0, 1.0, float("inf"), 2, p) == _lib.ERR_INVALID_ARG and lib.nxsig_cwt_wavelet(1, 1.0, float("inf"), 2, p) == 0


def test_python_wavelets_are_the_oracles():
    for M, a in [(1, 0.3), (10, 1.0), (45, 4.5), (100, 7.7)]:
        assert np.array_equal(transforms.morlet2(M, a, 5.5), O.morlet2(M, a, 5.5)) and transforms.morlet2(M, a).dtype == np.complex128
        assert np.array_equal(transforms.ricker(M, a), O.ricker(M, a)) and transforms.ricker(M, a).dtype == np.float64
    for bad in (lambda: transforms.ricker(0, 1.0), lambda: transforms.ricker(4, 0.0), lambda: transforms.morlet2(4.0, 1.0),
                lambda: transforms.morlet2(4, float("nan")), lambda: transforms.morlet2(4, 1.0, float("inf"))):
        with pytest.raises(ArgumentError):
            bad()


# ---- the scheme in single precision (csrc/cwt_plan.hpp restated): blocks of K samples from base = b step - lead, the filter placed
# circularly at (j - c) mod K, one forward transform per block, per filter a product with H / K and an unscaled inverse, the run
# lead <= t < lead + step kept
def plan(N):
    return (1024 if N <= 513 else 2048) if N <= 1025 else None


def emulate(x, bank, K):
    L, Nmax = len(x), max(len(h) for h in bank)
    step, lead = K - Nmax + 1, Nmax - 1 - (Nmax - 1) // 2
    H = []
    for h in bank:
        g = np.zeros(K, np.complex128)
        np.add.at(g, (np.arange(len(h)) - (len(h) - 1) // 2) % K, h)
        H.append((np.fft.fft(g) / K).astype(np.complex64))
    out = np.zeros((len(bank), L), np.complex64)
    for b in range(-(-L // step)):
        base = b * step - lead
        blk = np.zeros(K, np.complex64)
        lo, hi = max(base, 0), min(base + K, L)
        blk[lo - base:hi - base] = x[lo:hi]
        X = scipy.fft.fft(blk)
        assert X.dtype == np.complex64
        for s in range(len(bank)):
            y = scipy.fft.ifft(X * H[s]) * np.float32(K)
            n0, n1 = base + lead, min(base + lead + step, L)
            out[s, n0:n1] = y[lead:lead + n1 - n0]
    return out


@pytest.mark.parametrize("K,widths", [(1024, [1.0, 4.5, 10.0, 51.2]), (2048, [51.4, 80.0, 102.4])], ids=["K1024", "K2048"])
def test_single_precision_restatement_meets_the_bar(K, widths):
    L = 5000
    rng = np.random.Generator(np.random.PCG64(K))
    t = np.arange(L)
    rows = {"noise": rng.standard_normal(L), "tone on an offset": 1000 + np.sin(2 * np.pi * 0.013 * t), "impulse": (t == 2345) * 1.0}
    for wavelet in ("morlet2", "ricker"):
        bank = [O.taps(wavelet, a, L).astype(np.complex64).astype(np.complex128) for a in widths]
        assert all(plan(len(h)) == K for h in bank)
        for name, x in rows.items():
            x = x.astype(np.float32)
            got, ref = emulate(x, bank, K), O.fir_bank(x, bank)
            for s, h in enumerate(bank):
                err = np.abs(got[s] - ref[s]).max()
                # the interior of a zero-mean wavelet's output cancels on the offset: that row is held to the convolution's size
                scale = np.abs(x).max() * np.abs(h).sum() if name == "tone on an offset" else np.abs(ref[s]).max()
                print(f"cwt-emulation K={K} {wavelet} a={widths[s]} {name}: {err / scale:.3e}")
                assert err <= BAR * scale, (K, wavelet, widths[s], name, err / scale)


# ---- the Python functions
X32 = np.zeros(32, np.float32)
H3 = [np.ones(3, np.float32)]
BAD = [
    ("cwt", "f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64: real f32 rows are built"),
    ("cwt", "c64", dict(x=np.zeros(32, np.complex64)), NxSignalUnsupported, "unsupported type complex64"),
    ("cwt", "text", dict(x=np.array(["a"] * 32)), ArgumentError, "unsupported type"),
    ("cwt", "rank 0", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("cwt", "empty dimension", dict(x=np.zeros((0, 4), np.float32)), ArgumentError, "empty dimension"),
    ("cwt", "empty axis", dict(x=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
    ("cwt", "axis", dict(axis=1), ArgumentError, "axis 1 is out of bounds"),
    ("cwt", "batch", dict(x=np.zeros((65536, 2), np.float32)), NxSignalUnsupported, "1 to 65535 rows"),
    ("cwt", "width 0", dict(widths=[1.0, 0.0]), ArgumentError, "every width must be positive and finite"),
    ("cwt", "width nan", dict(widths=[float("nan")]), ArgumentError, "every width must be positive and finite"),
    ("cwt", "width inf", dict(widths=[float("inf")]), ArgumentError, "every width must be positive and finite"),
    ("cwt", "no widths", dict(widths=[]), ArgumentError, "1-D sequence of 1 to 4096"),
    ("cwt", "too many widths", dict(widths=np.ones(4097)), ArgumentError, "1-D sequence of 1 to 4096"),
    ("cwt", "widths text", dict(widths="wide"), ArgumentError, "widths must be real numbers"),
    ("cwt", "wavelet", dict(wavelet="haar"), ArgumentError, "wavelet must be 'morlet2', 'ricker' or a callable"),
    ("cwt", "wavelet 3", dict(wavelet=3), ArgumentError, "wavelet must be 'morlet2', 'ricker' or a callable"),
    ("cwt", "w nan", dict(w=float("nan")), ArgumentError, "w must be finite"),
    ("cwt", "output", dict(output="phase"), ArgumentError, "output must be 'complex', 'real', 'magnitude' or 'power'"),
    ("cwt", "callable nan", dict(wavelet=lambda N, a: np.full(N, np.nan)), ArgumentError, "the taps must be finite"),
    ("cwt", "callable 2-D", dict(wavelet=lambda N, a: np.ones((N, 2))), ArgumentError, "every filter must be a 1-D numeric array"),
    ("fir_bank", "f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64: real f32 rows are built"),
    ("fir_bank", "no filters", dict(taps=[]), ArgumentError, "1 to 4096 filters"),
    ("fir_bank", "too many filters", dict(taps=[np.ones(1)] * 4097), ArgumentError, "1 to 4096 filters"),
    ("fir_bank", "empty filter", dict(taps=[np.ones(3), np.ones(0)]), ArgumentError, "at least one tap"),
    ("fir_bank", "2-D filter", dict(taps=[np.ones((2, 2))]), ArgumentError, "every filter must be a 1-D numeric array"),
    ("fir_bank", "text filter", dict(taps=[np.array(["a"])]), ArgumentError, "every filter must be a 1-D numeric array"),
    ("fir_bank", "taps inf", dict(taps=[np.array([1.0, np.inf])]), ArgumentError, "the taps must be finite"),
    ("fir_bank", "size", dict(taps=[np.zeros((1 << 24) - 30, np.float32)]), NxSignalUnsupported, "length + max taps - 1 must be at most 2^24"),
    ("fir_bank", "output", dict(output=3), ArgumentError, "output must be"),
    ("fir_bank", "axis", dict(axis=-2), ArgumentError, "axis -2 is out of bounds"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: f"{c[0]}-{c[1]}")
def test_arguments_are_checked_before_anything_runs(case, monkeypatch):
    """every Python-side error comes before the library is loaded and before a context exists"""
    fn, _, change, error, pattern = case

    def never(*a, **k):
        raise AssertionError("the library or a context was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "load", never)
    monkeypatch.setattr(S.device, "default_context", never)
    kw = dict(x=X32)
    kw.update(dict(widths=[1.0, 2.0]) if fn == "cwt" else dict(taps=H3))
    kw.update(change)
    with pytest.raises(error, match=re.escape(pattern)):
        if fn == "cwt":
            transforms.cwt(kw.pop("x"), kw.pop("widths"), **kw)
        else:
            filters.fir_bank(kw.pop("x"), kw.pop("taps"), **kw)


# ---- the C entry points
def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_fir_bank and nxsig_cwt comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.CWT_TABLE_ENTRIES)
    assert table.keys() == ABI_GOLDEN["null_ctx"].keys() == {"nxsig_fir_bank", "nxsig_cwt"}
    unsupported = {"length+taps-1=2^24+1", "tap count 2^40", "length=2^24+1", "length=2^24"}
    for name, prefix in (("nxsig_fir_bank", "fir_bank: "), ("nxsig_cwt", "cwt: ")):
        rows, golden = table[name], ABI_GOLDEN["null_ctx"][name]
        assert rows.keys() == golden.keys()
        for k in rows:
            assert rows[k] == golden[k], (k, rows[k], golden[k])
        assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
        for k, r in rows.items():
            if k != "valid":
                assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
                assert r["err"].startswith(prefix) or k == "mem=7", (k, r)
        assert _lib.SIGNATURES[name][1][0] is _lib._ctx_iir
    fb, cw = table["nxsig_fir_bank"], table["nxsig_cwt"]
    # the limits of the issue, each with a message of its own
    assert fb["batch=0"]["err"] == fb["batch=65536"]["err"] == "fir_bank: batch must be in [1, 65535]"
    assert fb["num_filters=0"]["err"] == fb["num_filters=4097"]["err"] == "fir_bank: num_filters must be in [1, 4096]"
    assert fb["tap count 0"]["err"] == "fir_bank: every tap count must be >= 1"
    assert fb["length+taps-1=2^24+1"]["err"] == "fir_bank: length + max taps - 1 must be at most 2^24"
    assert fb["taps nan"]["err"] == fb["taps inf"]["err"] == "fir_bank: the taps must be finite"
    assert cw["width 0"]["err"] == cw["width nan"]["err"] == cw["width inf"]["err"] == "cwt: every width must be positive and finite"
    assert len({fb["batch=0"]["err"], fb["num_filters=0"]["err"], fb["tap count 0"]["err"], fb["length+taps-1=2^24+1"]["err"], fb["taps nan"]["err"]}) == 5
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"}
    for name in ("nxsig_fir_bank", "nxsig_cwt"):
        assert set(ABI_GOLDEN["real_ctx"][name]) == set(table[name])
        assert ABI_GOLDEN["real_ctx"][name]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}


def test_overlapping_operands_are_refused_ahead_of_the_context():
    lib = _lib.load()
    buf = np.zeros(256, np.float32)
    x, taps, counts = buf[:24], np.ones(3, np.float32), np.array([3], np.int64)
    widths = np.array([1.0])
    pc, pw = counts.ctypes.data_as(C.POINTER(C.c_int64)), widths.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.nxsig_fir_bank(None, vp(x), 24, 1, 24, vp(taps), 0, pc, 1, 1, vp(buf[23:]), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert _lib.last_error() == "fir_bank: x and out must not overlap"
    assert lib.nxsig_fir_bank(None, vp(x), 24, 1, 24, vp(taps), 0, pc, 1, 1, vp(buf[24:]), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert _lib.last_error() == "null context"
    assert lib.nxsig_cwt(None, vp(x), 24, 1, 24, 0, pw, 1, 5.0, 0, vp(buf[20:]), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert _lib.last_error() == "cwt: x and out must not overlap"
    assert lib.nxsig_cwt(None, vp(buf[100:124]), 24, 1, 24, 0, pw, 1, 5.0, 0, vp(buf[:48]), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert _lib.last_error() == "null context"


def test_the_switch_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(CWT_WAVE)" in internal and "DISABLE_CWT" not in internal and "kScratchSlots = 32" in internal and '#include "cwt_plan.hpp"' in internal
    assert "OwnedBuffer cwt_flags, cwt_rows, cwt_spectra, cwt_conv;" in internal
    src = read("nx_signal_amd", "csrc", "kernels_cwt.hip")
    assert "tune(c, kT_CWT_WAVE, 1)" in src and "tune(c, kT_DISABLE_WAVE, 0)" in src and '("kernels_cwt.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["wave_stft.hpp"]
    assert not re.findall(r"\batomic[A-Z]\w*", src) and "ctx_scratch(" not in src and "fir_row_flags" not in src
    assert 'dispatch_note("cwt.wave")' in src and 'dispatch_note("cwt.generic")' in src
    assert "wave_fft_core_T<K>" in src and "wave_fft_core<K, true, true>" in src
    assert src.count("own_buffer(c, c->cwt_") == 4 and src.count("ctx_table(") == 2 and src.count("launch_fft(") == 2
    plan_src = read("nx_signal_amd", "csrc", "cwt_plan.hpp")
    for name in ("cwt_support", "cwt_wavelet", "cwt_class", "cwt_step", "cwt_lead", "cwt_split", "cwt_spectrum", "cwt_slot_pos", "cwt_bin", "cwt_pos_valid",
                 "cwt_bank_check", "cwt_widths_check"):
        assert name in plan_src, name
    assert "hip" not in plan_src.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_cwt.hip", "")
    assert "cwt_plan.hpp" in read("tests", "san_cwt.cpp")
    assert "NXSIG_CWT_WAVE" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.21" in design and "cwt.wave" in design and "cwt.generic" in design
    readme = read("README.md")
    assert "transforms.cwt" in readme and "fir_bank" in readme and "_cwt.py" in readme
    tools = read("tools", "README.md")
    assert "bench_cwt.py" in tools and "gen_cwt_golden.py" in tools and "--cwt" in tools
    header = read("include", "nxsig.h")
    assert re.search(r"\bint nxsig_fir_bank\(nxsig_ctx\* ctx, const void\* x, int64_t length, int64_t batch, int64_t batch_stride, const void\* taps, int32_t taps_complex,", header)
    assert re.search(r"\bint nxsig_cwt\(nxsig_ctx\* ctx, const void\* x, int64_t length, int64_t batch, int64_t batch_stride, int32_t wavelet, const double\* widths,", header)
    assert re.search(r"\bint64_t nxsig_cwt_support\(double width, int64_t length\);", header) and "nxsig_cwt_wavelet(" in header
    for phrase in ("THE DEFINITION", "out[s][n] = full[n + (N - 1) / 2]", "N   = min(ceil(10 a), L)", "conj(wavelet(N, a))[::-1]", "cwt.wave", "cwt.generic",
                   "NXSIG_CWT_WAVE", "no finite output element", "Not built"):
        assert phrase in header[header.index("Filters.fir_bank / Transforms.cwt"):], phrase
    for name in ("nxsig_fir_bank", "nxsig_cwt", "nxsig_cwt_support", "nxsig_cwt_wavelet"):
        assert name in _lib.SIGNATURES
    # no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "cwt" not in nif and "fir_bank" not in nif
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.transforms.cwt is transforms.cwt is _cwt.cwt and filters.fir_bank is _cwt.fir_bank
    assert transforms.morlet2 is _cwt.morlet2 and transforms.ricker is _cwt.ricker and transforms.cwt.__module__ == "nx_signal_amd._cwt"
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_cwt.py"))


def test_the_private_module_can_be_imported_first():
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._cwt as m, nx_signal_amd.transforms as t, nx_signal_amd.filters as f; "
                        "assert t.cwt is m.cwt and f.fir_bank is m.fir_bank"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the support rule, the wavelets, the argument checks, the class split and block geometry at their edges, and the fused kernel's
    block, lane and slot arithmetic walked over exactly sized buffers (csrc/cwt_plan.hpp) in a stand-alone program with ASan / UBSan;
    the edges it prints are the ones the issue names"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_cwt")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_cwt.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized cwt host side ok" in r.stdout
    edges = {int(m.group(1)): m.groups()[1:] for m in re.finditer(r"edge N=(\d+) class=(\d) K=(\d+) step=(\d+) lead=(\d+) name=(\S+)", r.stdout)}
    assert edges[513] == ("0", "1024", "512", "256", "cwt.wave") and edges[514] == ("1", "2048", "1535", "257", "cwt.wave")
    assert edges[1025] == ("1", "2048", "1024", "512", "cwt.wave") and edges[1026][0] == "2" and edges[1026][4] == "cwt.generic"
    assert edges[1] == ("0", "1024", "1024", "0", "cwt.wave")
    for N, e in edges.items():
        assert plan(N) == (int(e[1]) if e[4] == "cwt.wave" else None)
        if e[4] == "cwt.wave":
            assert int(e[2]) == int(e[1]) - N + 1 >= int(e[1]) // 2 - 1
