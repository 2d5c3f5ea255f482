"""Spectral.welch / csd / coherence without a GPU: the f64 oracle (tests/welch_oracle.py) against recorded scipy results
(tests/golden/welch_vectors.json, tools/gen_welch_golden.py), the option checks of the Python module, nxsig_welch_bins, every argument
error of the two C entry points (they validate before they look at the context, so a null context reaches every message), the NIF and
Elixir tables, and the host side under ASan / UBSan in a stand-alone program (tests/san_welch.cpp)."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import welch_oracle as W
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, spectral
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "welch_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_WELCH) as f:
    ABI_GOLDEN = json.load(f)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, w = (np.array(c[k], np.float32).astype(np.float64) for k in ("x", "window"))   # f32 values, recorded in their shortest form
    y = W.golden_y(x).astype(np.float64)
    o = dict(overlap_length=c["overlap_length"], fft_length=c["fft_length"], sampling_rate=c["sampling_rate"], detrend=c["detrend"],
             scaling=c["scaling"])
    f, pxx = W.welch(x, w, **o)
    _, pxy = W.csd(x, y, w, **o)
    ref, rxy = np.array(c["pxx"]), np.array(c["pxy_re"]) + 1j * np.array(c["pxy_im"])
    assert GOLDEN["scipy"] and pxx.shape == ref.shape == (2, c["fft_length"] // 2 + 1) and pxy.shape == rxy.shape
    assert float((np.abs(pxx - ref).max(-1) / ref.max(-1)).max()) <= 1e-12
    assert float((np.abs(pxy - rxy).max(-1) / np.abs(rxy).max(-1)).max()) <= 1e-12
    assert np.allclose(f, np.array(c["f"]), rtol=1e-15, atol=0.0)
    assert np.array_equal(spectral.frequencies(c["fft_length"], c["sampling_rate"]), np.array(c["f"]).astype(np.float32))
    _, coh = W.coherence(x, y, w, **o)
    assert coh.min() >= 0.0 and coh.max() <= 1.0 + 1e-12


def test_the_recorded_cases_cover_what_the_issue_lists():
    cs = GOLDEN["cases"]
    assert 5 <= len(cs) <= 8 and all(c["fft_length"] <= 512 and len(c["x"]) == 2 for c in cs)
    assert any(c["fft_length"] % 2 for c in cs) and any(c["fft_length"] % 2 == 0 for c in cs)
    assert any(c["fft_length"] > len(c["window"]) for c in cs)
    assert {c["scaling"] for c in cs} == {"density", "spectrum"} and {c["detrend"] for c in cs} == {"constant", False}


def test_welch_bins_for_even_and_odd_lengths():
    lib = _lib.load()
    for k in (1, 2, 3, 64, 255, 256, 1023, 1024, 2048, 2 ** 31 - 1):
        assert lib.nxsig_welch_bins(k) == k // 2 + 1 == len(np.fft.rfftfreq(min(k, 4096))) + (k // 2 - min(k, 4096) // 2)
    assert lib.nxsig_welch_bins(0) == _lib.ERR_INVALID_ARG and "fft_length must be >= 1" in _lib.last_error()
    assert lib.nxsig_welch_bins(-8) == _lib.ERR_INVALID_ARG


X, WIN = np.zeros((2, 100), np.float32), np.ones(16, np.float32)
BAD_OPTIONS = [
    ("detrend", dict(detrend="linear"), "unsupported"), ("detrend", dict(detrend="median"), "detrend"), ("detrend", dict(detrend=True), "detrend"),
    ("average", dict(average="median"), "unsupported"), ("scaling", dict(scaling="psd"), "scaling"), ("scaling", dict(scaling=None), "scaling"),
    ("overlap_length", dict(overlap_length=16), "overlap_length"), ("overlap_length", dict(overlap_length=-1), "overlap_length"),
    ("overlap_length", dict(overlap_length=7.5), "overlap_length"), ("fft_length", dict(fft_length=15), "fft_length"),
    ("fft_length", dict(fft_length="pow2"), "fft_length"), ("sampling_rate", dict(sampling_rate=0), "sampling_rate"),
    ("sampling_rate", dict(sampling_rate=float("nan")), "sampling_rate"), ("nfft", dict(nfft=32), "unknown keys"),
]


@pytest.mark.parametrize("fn", ["welch", "csd", "coherence"])
@pytest.mark.parametrize("case", BAD_OPTIONS, ids=lambda c: f"{c[0]}={list(c[1].values())[0]!r}")
def test_every_unsupported_option_is_named(fn, case):
    name, opts, word = case
    args = (X, WIN) if fn == "welch" else (X, X, WIN)
    with pytest.raises(ArgumentError) as ei:
        getattr(spectral, fn)(*args, **opts)
    assert fn in str(ei.value) and word in str(ei.value) and (name in str(ei.value) or word == "unknown keys")


@pytest.mark.parametrize("fn", ["welch", "csd", "coherence"])
def test_shapes_and_types_are_checked_before_anything_runs(fn):
    call = getattr(spectral, fn)
    two = (lambda x: (x,)) if fn == "welch" else (lambda x: (x, x))
    with pytest.raises(ArgumentError, match="does not fit"):      # L < N
        call(*two(np.zeros((2, 15), np.float32)), WIN)
    with pytest.raises(NxSignalUnsupported, match="f32"):
        call(*two(np.zeros((2, 100), np.float64)), WIN)
    with pytest.raises(ArgumentError, match="window"):
        call(*two(X), np.ones((2, 8), np.float32))
    with pytest.raises(ArgumentError, match="at least one axis"):
        call(*two(np.float32(1.0)), WIN)
    if fn != "welch":
        with pytest.raises(ArgumentError, match="same shape"):
            call(X, X[:, :50], WIN)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_welch_f32 / nxsig_csd_f32 comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.WELCH_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    for name in ("nxsig_welch_f32", "nxsig_csd_f32"):
        rows = table[name]
        assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
        assert all(r["rc"] == _lib.ERR_INVALID_ARG and r["err"] != "null context" for k, r in rows.items() if k != "valid"), rows
        assert _lib.SIGNATURES[name][1][0] is _lib._ctx_spectral and _lib._ctx_spectral is not _lib._p   # a typed context
    assert "null pxx_out" in table["nxsig_welch_f32"] and "null pxx_out" not in table["nxsig_csd_f32"]   # optional in csd
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()


def test_a_typed_context_pointer_that_is_not_null_reaches_the_library():
    """the argument checks come ahead of the context, so a made-up non-null context with batch = 0 is refused and never looked at; the
    conversion of the typed pointer itself is what runs here (a pointer type without its own _type_ crashed in it)"""
    import ctypes as C
    lib, V = _lib.load(), C.c_void_p
    x, w, out = np.zeros(100, np.float32), np.ones(16, np.float32), np.zeros(18, np.float32)
    fake = _lib.ctx_ptr(V(64), _lib._ctx_spectral)
    assert isinstance(fake, _lib._ctx_spectral) and _lib.ctx_ptr(None, _lib._ctx_spectral) is None
    p = lambda a: a.ctypes.data_as(V)   # noqa: E731
    assert lib.nxsig_welch_f32(fake, p(x), 100, 0, 100, p(w), 16, 8, 16, 1, 0, 1.0, p(out), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "welch: batch and length must be >= 1" in _lib.last_error()
    assert lib.nxsig_csd_f32(fake, p(x), p(x), 100, 1, 100, p(w), 16, 0, 16, 1, 0, 1.0, None, None, p(out), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "csd: hop must be in" in _lib.last_error()


def test_the_switch_the_sources_and_the_tables_are_in_place():
    assert "X(DISABLE_WELCH_WAVE)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "tune(c, kT_DISABLE_WELCH_WAVE, 0)" in read("nx_signal_amd", "csrc", "kernels_welch.hip")
    assert '("kernels_welch.hip", [])' in read("nx_signal_amd", "build.py")
    assert "NXSIG_DISABLE_WELCH_WAVE" in read("INTEGRATION.md") and "3.12" in read("DESIGN.md")
    # no atomics in the new kernels, and none of the existing kernel sources is included for more than wave_stft.hpp
    src = read("nx_signal_amd", "csrc", "kernels_welch.hip")
    assert "atomic" not in src.lower() and re.findall(r'#include "([^"]+)"', src) == ["wave_stft.hpp"]
    # the NIF table, the Elixir stubs and the wrapper agree: welch/10 and csd/11
    nif, stubs, ex = read("nif", "nxsig_nif.c"), read("elixir", "lib", "nx_signal_amd", "nif.ex"), read("elixir", "lib", "nx_signal_amd", "spectral.ex")
    assert '{"welch", 10, nif_welch, ERL_NIF_DIRTY_JOB_IO_BOUND}' in nif and '{"csd", 11, nif_csd, ERL_NIF_DIRTY_JOB_IO_BOUND}' in nif
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76   # (tests/test_elixir_sources.py holds the stubs of nif.ex to this table in both directions)
    for name, arity in (("welch", 10), ("csd", 11)):
        stub = re.search(rf"def {name}\(([^)]*)\)", stubs).group(1)
        assert len(stub.split(",")) == arity and f"NIF.{name}(" in ex, name   # the calls' arity: tests/test_elixir_sources.py
    assert "76 NIFs" in read("README.md") and "76 NIFs" in read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "elixir", "test", "spectral_test.exs"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks, the bin count and the run geometry (csrc/welch_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_welch")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_welch.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized welch host side ok" in r.stdout
