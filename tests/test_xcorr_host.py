"""Convolution.correlate_rows / convolve_rows without a GPU: the f64 oracle (tests/xcorr_oracle.py) against the recorded SciPy 1.15.3
results (tests/golden/xcorr_vectors.json, tools/gen_xcorr_golden.py), correlation_lags against SciPy's, csrc/xcorr_plan.hpp through a
small shared library of its own (the tier and the transform length at their edges, the index maps against the oracle, the mirror-bin
map of the packed split), the packed scheme in numpy single precision with and without its row scale, the argument errors of the
Python functions (before the library is loaded) and of the C entry point (ahead of the context, message by message), the switch /
sources / documents, and the host side under ASan / UBSan in a stand-alone program (tests/san_xcorr.cpp)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import xcorr_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, _xcorr, convolution
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

BAR = 1e-5
SHAPES = [(1, 1), (2, 1), (5, 3), (3, 5), (8, 8), (7, 10)]
with open(os.path.join(ROOT, "tests", "golden", "xcorr_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_XCORR) as f:
    ABI_GOLDEN = json.load(f)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def dec(v, is_complex):
    a = np.array(v, dtype=np.float64)
    return a[:, 0] + 1j * a[:, 1] if is_complex else a


# ---- the oracle and correlation_lags against SciPy
def test_the_recorded_cases_are_the_ones_the_issue_lists():
    assert GOLDEN["scipy"] == "1.15.3"
    assert {(c["n1"], c["n2"], c["complex"], c["kind"]) for c in GOLDEN["cases"]} == {(n1, n2, c, k) for n1, n2 in SHAPES for c in (False, True)
                                                                                      for k in ("integers", "noise")}
    for c in GOLDEN["cases"]:
        assert set(c["results"]) == {f"{op}.{mode}" for op in O.OPS for mode in O.MODES}


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: f"n{c['n1']}-n{c['n2']}-{'c' if c['complex'] else 'r'}-{c['kind']}")
def test_oracle_equals_scipy(c):
    x, y = dec(c["x"], c["complex"]), dec(c["y"], c["complex"])
    for key, recorded in c["results"].items():
        op, mode = key.split(".")
        want, got = dec(recorded, c["complex"]), O.pair(x, y, op, mode)
        assert got.shape == want.shape == (O.out_length(c["n1"], c["n2"], mode),), key
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), key
        assert np.array_equal(O.rows(x[None], y[None], op, mode)[0], got) and np.array_equal(O.rows(x[None], y, op, mode)[0], got)


def test_correlation_lags_equals_scipy():
    seen = set()
    for row in GOLDEN["lags"]:
        n1, n2, mode = row["n1"], row["n2"], row["mode"]
        got = convolution.correlation_lags(n1, n2, mode)
        assert got.dtype.kind == "i" and list(got) == row["lags"] == list(O.lags(n1, n2, mode)), (n1, n2, mode)
        assert len(row["lags"]) == O.out_length(n1, n2, mode)
        seen.add((n1 % 2, n2 % 2, n1 < n2, mode))
    assert len(seen) == 2 * 2 * 2 * 3      # odd and even lengths on either side of n1 = n2, in the three modes
    assert list(convolution.correlation_lags(5, 3)) == list(range(-2, 5))
    for bad in ((0, 3, "full"), (3, -1, "full"), (3.0, 3, "full"), (True, 3, "full"), (3, 3, "circular")):
        with pytest.raises(ArgumentError):
            convolution.correlation_lags(*bad)


# ---- csrc/xcorr_plan.hpp
@pytest.fixture(scope="module")
def plan():
    """csrc/xcorr_plan.hpp behind a few C functions, in a small shared library of its own (plain g++: the header has no HIP types)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    src, so = os.path.join(build, "xcorr_plan_c.cpp"), os.path.join(build, "xcorr_plan_c.so")
    with open(src, "w") as f:
        f.write('#include "xcorr_plan.hpp"\nextern "C" {\n'
                "int xc_tier(long long n1, long long n2, int cplx, int off) { return nxsig::xcorr_tier(n1, n2, cplx != 0, off != 0); }\n"
                "long long xc_length(long long n1, long long n2) { return nxsig::xcorr_fft_length(n1, n2); }\n"
                "long long xc_circ_start(long long n1, long long n2, int op, int mode, long long P) { return nxsig::xcorr_circ_start(n1, n2, op, mode, P); }\n"
                "long long xc_circ_index(long long cs, long long i, long long P) { return nxsig::xcorr_circ_index(cs, i, P); }\n"
                "long long xc_out_length(long long n1, long long n2, int mode) { return nxsig::xcorr_out_length(n1, n2, mode); }\n"
                "long long xc_first_lag(long long n1, long long n2, int mode) { return nxsig::xcorr_first_lag(n1, n2, mode); }\n"
                "int xc_mirror_lane(int lane) { return nxsig::xcorr_mirror_lane(lane); }\n"
                "int xc_mirror_reg(int lane, int s, int regs) { return nxsig::xcorr_mirror_reg(lane, s, regs); }\n"
                "int xc_mirror_bin(int k, int K) { return nxsig::xcorr_mirror_bin(k, K); }\n"
                "int xc_scale_exponent(unsigned bits) { return nxsig::xcorr_scale_exponent(bits); }\n"
                "long long xc_slab_rows(long long batch, long long P, long long forced) { return nxsig::xcorr_slab_rows(batch, P, forced); }\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    LL = C.c_longlong
    for name, args, res in (("xc_tier", [LL, LL, C.c_int, C.c_int], C.c_int), ("xc_length", [LL, LL], LL), ("xc_circ_start", [LL, LL, C.c_int, C.c_int, LL], LL),
                            ("xc_circ_index", [LL, LL, LL], LL), ("xc_out_length", [LL, LL, C.c_int], LL), ("xc_first_lag", [LL, LL, C.c_int], LL),
                            ("xc_mirror_lane", [C.c_int], C.c_int), ("xc_mirror_reg", [C.c_int] * 3, C.c_int), ("xc_mirror_bin", [C.c_int] * 2, C.c_int),
                            ("xc_scale_exponent", [C.c_uint], C.c_int), ("xc_slab_rows", [LL, LL, LL], LL)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


def test_the_tier_and_the_transform_length_at_their_edges(plan):
    lib = _lib.load()
    WAVE, GENERIC = 0, 1
    #            n1,   n2, need -> P, real tier, c64 tier
    for n1, n2, length, real, cplx in [(512, 513, 1024, WAVE, WAVE), (1024, 1, 1024, WAVE, WAVE), (513, 513, 2048, WAVE, GENERIC),
                                       (1025, 1, 2048, WAVE, GENERIC), (1024, 1025, 2048, WAVE, GENERIC), (2048, 1, 2048, WAVE, GENERIC),
                                       (1025, 1025, 4096, GENERIC, GENERIC), (2049, 1, 4096, GENERIC, GENERIC), (1, 1, 1024, WAVE, WAVE),
                                       (5000, 4000, 16384, GENERIC, GENERIC), (48000, 48000, 131072, GENERIC, GENERIC)]:
        assert plan.xc_length(n1, n2) == lib.nxsig_xcorr_fft_length(n1, n2) == O.fft_length(n1, n2) == length, (n1, n2)
        assert plan.xc_tier(n1, n2, 0, 0) == real and plan.xc_tier(n1, n2, 1, 0) == cplx, (n1, n2)
        assert plan.xc_tier(n1, n2, 0, 1) == plan.xc_tier(n1, n2, 1, 1) == GENERIC
    # need 600 under the switch: the generic tier at the contract's P = 1024, not at the next power of two
    assert plan.xc_tier(400, 201, 0, 1) == GENERIC and plan.xc_length(400, 201) == 1024
    assert lib.nxsig_xcorr_fft_length(0, 1) == _lib.ERR_INVALID_ARG and lib.nxsig_xcorr_fft_length(1, 0) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_xcorr_fft_length(1 << 30, 2) == _lib.ERR_UNSUPPORTED
    for mode_id, mode in enumerate(O.MODES):
        for n1, n2 in SHAPES + [(600, 300), (301, 600)]:
            assert plan.xc_out_length(n1, n2, mode_id) == lib.nxsig_conv_length(n1, n2, mode_id) == O.out_length(n1, n2, mode)
            assert plan.xc_first_lag(n1, n2, mode_id) == O.lags(n1, n2, mode)[0]
    assert plan.xc_slab_rows(5, 1024, 2) == 2 and plan.xc_slab_rows(5, 1024, 0) == 5 and plan.xc_slab_rows(10 ** 6, 1024, 0) == (256 << 20) // (4 * 1024 * 8)


def test_the_index_maps_against_the_oracle(plan):
    """the mode's window read out of the circular result at P through the plan's maps equals the oracle, for every op and mode"""
    for c in GOLDEN["cases"]:
        if c["kind"] != "integers":
            continue
        x, y, n1, n2 = dec(c["x"], c["complex"]), dec(c["y"], c["complex"]), c["n1"], c["n2"]
        Pn = plan.xc_length(n1, n2)
        X, Y = np.fft.fft(x, Pn), np.fft.fft(y, Pn)
        for op_id, op in ((0, "convolve"), (1, "correlate")):
            circ = np.fft.ifft(X * (np.conj(Y) if op == "correlate" else Y))
            for mode_id, mode in enumerate(O.MODES):
                cs = plan.xc_circ_start(n1, n2, op_id, mode_id, Pn)
                assert cs == O.circ_start(n1, n2, op, mode, Pn)
                idx = [plan.xc_circ_index(cs, i, Pn) for i in range(plan.xc_out_length(n1, n2, mode_id))]
                want = O.pair(x, y, op, mode)
                assert np.abs(circ[idx] - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0), (n1, n2, op, mode)


@pytest.mark.parametrize("K", [1024, 2048])
def test_the_mirror_bin_map_is_an_involution_over_every_lane_and_register(plan, K):
    regs = K // 64
    seen = np.zeros(K, int)
    for lane in range(64):
        for s in range(regs):
            k = lane + 64 * s
            ml, ms = plan.xc_mirror_lane(lane), plan.xc_mirror_reg(lane, s, regs)
            assert 0 <= ml < 64 and 0 <= ms < regs and ml + 64 * ms == plan.xc_mirror_bin(k, K) == (K - k) % K, (lane, s)
            assert (plan.xc_mirror_lane(ml), plan.xc_mirror_reg(ml, ms, regs)) == (lane, s)
            seen[ml + 64 * ms] += 1
    assert (seen == 1).all()


# ---- the packed scheme in numpy single precision: two real rows in one complex transform
def emulate_packed(plan, x, y, op, mode, normalise):
    n1, n2 = x.shape[-1], y.shape[-1]
    Pn = plan.xc_length(n1, n2)
    out = []
    for xr, yr in zip(x, y):
        ea = plan.xc_scale_exponent(int(np.abs(xr).max().view(np.uint32))) if normalise else 0
        eb = plan.xc_scale_exponent(int(np.abs(yr).max().view(np.uint32))) if normalise else 0
        if not xr.any() or not yr.any():     # an all-zero row: exact zeros, as the kernel has it
            out.append(np.zeros(O.out_length(n1, n2, mode), np.float32))
            continue
        z = np.zeros(Pn, np.complex64)
        z[:n1] += np.ldexp(xr, -ea).astype(np.float32)
        z[:n2] += 1j * np.ldexp(yr, -eb).astype(np.float32)
        Z = np.fft.fft(z).astype(np.complex64)
        Zm = np.conj(Z[(-np.arange(Pn)) % Pn])
        X, Y = ((Z + Zm) * np.float32(0.5)).astype(np.complex64), ((Z - Zm) * np.complex64(-0.5j)).astype(np.complex64)
        R = (X * (np.conj(Y) if op == "correlate" else Y)).astype(np.complex64)
        circ = np.fft.ifft(R).astype(np.complex64)
        idx = (O.circ_start(n1, n2, op, mode, Pn) + np.arange(O.out_length(n1, n2, mode))) % Pn
        out.append(np.ldexp(circ.real[idx].astype(np.float32), ea + eb))
    return np.stack(out)


def _noise(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)


DISPARITY = [(1.0, 1.0), (1e3, 1e-3), (1e4, 1e-4), (2.0 ** 13, 2.0 ** -13)]


@pytest.mark.parametrize("shape", [(600, 300), (1500, 549)], ids=lambda s: f"n{s[0]}-n{s[1]}")
def test_the_packed_emulation_meets_the_bar_with_its_row_scale_and_fails_it_without(plan, shape):
    n1, n2 = shape
    x0, y0 = _noise(11 + n1, (4, n1)), _noise(13 + n2, (4, n2))
    for sx, sy in DISPARITY:
        x, y = x0 * np.float32(sx), y0 * np.float32(sy)
        for op in O.OPS:
            want = O.rows(x, y, op, "full")
            top = np.abs(want).max(axis=-1)
            err = (np.abs(emulate_packed(plan, x, y, op, "full", True) - want).max(axis=-1) / top).max()
            bare = (np.abs(emulate_packed(plan, x, y, op, "full", False) - want).max(axis=-1) / top).max()
            print(f"xcorr-emulation {op} n1={n1} n2={n2} scales {sx:g} / {sy:g}: {err:.2e} of the row maximum with the row scale, {bare:.2e} without")
            assert err <= BAR / 10, (op, sx, sy, err)                 # a decade under the bar
            if sx >= 1e3:
                assert bare > BAR, (op, sx, sy, bare)                 # the test bites: the same scheme without the scale fails it
    # zero rows keep scale 1 and give exact zeros
    z = np.zeros((1, n1), np.float32)
    assert not emulate_packed(plan, z, y0[:1], "correlate", "full", True).any()


# ---- the Python functions
X32, Y32 = np.zeros((2, 32), np.float32), np.zeros((2, 8), np.float32)
BAD = [
    ("f64", dict(in1=np.zeros((2, 32))), NxSignalUnsupported, "unsupported type float64 of in1"),
    ("c128", dict(in2=np.zeros((2, 8), np.complex128)), NxSignalUnsupported, "unsupported type complex128 of in2"),
    ("mixed", dict(in2=np.zeros((2, 8), np.complex64)), ArgumentError, "both be real or both be complex"),
    ("text", dict(in1=np.array([["a"] * 32] * 2)), ArgumentError, "unsupported type"),
    ("rank 0", dict(in1=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("empty dimension", dict(in1=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
    ("axis", dict(axis=2), ArgumentError, "axis 2 is out of bounds"),
    ("leading shape", dict(in2=np.zeros((3, 8), np.float32)), ArgumentError, "in2 must have the shape of in1"),
    ("rank", dict(in2=np.zeros((1, 2, 8), np.float32)), ArgumentError, "in2 must have the shape of in1"),
    ("mode", dict(mode="circular"), ArgumentError, "expected mode to be one of"),
    ("weighting", dict(weighting="scot"), ArgumentError, "expected weighting to be None or 'phat'"),
    ("output", dict(output="argmax"), ArgumentError, "expected output to be 'rows' or 'peak'"),
    ("floor 1", dict(weighting="phat", phat_floor=1.0), ArgumentError, "phat_floor must be a number in [0, 1)"),
    ("floor nan", dict(weighting="phat", phat_floor=float("nan")), ArgumentError, "phat_floor must be a number in [0, 1)"),
    ("floor text", dict(phat_floor="low"), ArgumentError, "phat_floor must be a number in [0, 1)"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(case, monkeypatch):
    """every Python-side error comes before the library is loaded"""
    _, change, error, pattern = case

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    kw = dict(in1=X32, in2=Y32)
    kw.update(change)
    with pytest.raises(error, match=re.escape(pattern)):
        convolution.correlate_rows(kw.pop("in1"), kw.pop("in2"), **kw)
    if not set(change) & {"weighting", "output", "phat_floor"}:
        with pytest.raises(error, match=re.escape(pattern)):
            kw = dict(in1=X32, in2=Y32)
            kw.update(change)
            convolution.convolve_rows(kw.pop("in1"), kw.pop("in2"), **kw)
    with pytest.raises(TypeError):
        convolution.convolve_rows(X32, Y32, weighting="phat")


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_xcorr comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.XCORR_TABLE_ENTRIES)
    rows, golden = table["nxsig_xcorr"], ABI_GOLDEN["null_ctx"]["nxsig_xcorr"]
    assert rows.keys() == golden.keys()
    for k in rows:
        assert rows[k] == golden[k], (k, rows[k], golden[k])
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    assert rows["batch=0"] == rows["valid"]        # batch = 0 passes every check and reaches the context
    unsupported = {"n1+n2-1=2^30+1", "n1=2^31", "rows too large", "result too large"}
    for k, r in rows.items():
        if k not in ("valid", "batch=0"):
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
            assert r["err"].startswith("xcorr: ") or k == "mem=7", (k, r)
    assert {"null a", "null b", "null out", "null out_lags", "n1=0", "n2=0", "batch=-1", "a_stride=n1-1", "b_stride=n2-1", "op=2", "mode=3",
            "weighting=2", "sink=2", "phat with convolve", "peak with convolve", "phat_floor=1", "mem=7"} <= set(rows)
    assert _lib.SIGNATURES["nxsig_xcorr"][1][0] is _lib._ctx_iir
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and set(ABI_GOLDEN["real_ctx"]["nxsig_xcorr"]) == set(rows) - {"batch=0"}
    assert ABI_GOLDEN["real_ctx"]["nxsig_xcorr"]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}


def test_a_result_that_overlaps_an_operand_is_refused_and_in1_is_in2_accepted():
    lib = _lib.load()
    buf = np.zeros(256, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    a, b = buf[:24], buf[24:33]
    call = lambda a, b, out, lags=None, sink=0: lib.nxsig_xcorr(None, p(a), 24, 24, p(b), len(b), len(b), 1, 0, 1, 0, 0, 0.0, sink, p(out),  # noqa: E731
                                                                None if lags is None else p(lags), _lib.HOST)
    for out in (buf[0:], buf[20:], buf[30:]):          # over a, over both, over b
        assert call(a, b, out) == _lib.ERR_INVALID_ARG and _lib.last_error() == "xcorr: the result must not overlap an operand"
    assert call(a, b, buf[64:]) == _lib.ERR_INVALID_ARG and _lib.last_error() == "null context"          # disjoint: on to the context
    assert call(a, a, buf[64:]) == _lib.ERR_INVALID_ARG and _lib.last_error() == "null context"          # in1 is in2
    lags = buf[128:].view(np.int32)
    assert call(a, b, buf[64:], lags, 1) == _lib.ERR_INVALID_ARG and _lib.last_error() == "null context"
    for bad_lags in (buf[10:].view(np.int32), buf[64:].view(np.int32)):   # over an operand, over the values
        assert call(a, b, buf[64:], bad_lags, 1) == _lib.ERR_INVALID_ARG and _lib.last_error() == "xcorr: the result must not overlap an operand"


def test_the_switches_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(XCORR_WAVE)" in internal and "X(XCORR_SLAB_ROWS)" in internal and '#include "xcorr_plan.hpp"' in internal
    assert "DISABLE_XCORR" not in internal
    src = read("nx_signal_amd", "csrc", "kernels_xcorr.hip")
    assert "tune(c, kT_XCORR_WAVE, 1)" in src and "tune(c, kT_DISABLE_WAVE, 0)" in src and "tune(c, kT_XCORR_SLAB_ROWS, 0)" in src
    assert '("kernels_xcorr.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["wave_stft.hpp"]
    assert not re.findall(r"\batomic[A-Z]\w*", src) and "ctx_scratch(" not in src
    assert 'dispatch_note("xcorr.wave")' in src and 'dispatch_note("xcorr.generic")' in src
    assert "wave_fft_core_T<K>" in src and "wave_fft_core<K, true, true>" in src and "xcorr_scale_exponent" in src and "xcorr_mirror_bin" in src
    # the generic tier's four temporaries are its own buffers in the context
    assert src.count("own_buffer(c, c->xcorr_") == 4 and "OwnedBuffer xcorr_a, xcorr_b, xcorr_sa, xcorr_sb;" in internal
    assert "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE" in src and "c->stream" in src
    plan = read("nx_signal_amd", "csrc", "xcorr_plan.hpp")
    for name in ("xcorr_check", "xcorr_tier", "xcorr_fft_length", "xcorr_circ_start", "xcorr_circ_index", "xcorr_out_index", "xcorr_first_lag",
                 "xcorr_mirror_lane", "xcorr_mirror_reg", "xcorr_scale_exponent", "xcorr_slab_rows", "kXcorrSlabBytes", "xcorr_store_state"):
        assert name in plan, name
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_xcorr.hip", "")
    assert "xcorr_plan.hpp" in read("tests", "san_xcorr.cpp")
    integration = read("INTEGRATION.md")
    assert "NXSIG_XCORR_WAVE" in integration and "NXSIG_XCORR_SLAB_ROWS" in integration
    design = read("DESIGN.md")
    assert "3.22" in design and "xcorr.wave" in design and "xcorr.generic" in design and "kXcorrSlabBytes" in design
    readme = read("README.md")
    assert "correlate_rows" in readme and "convolve_rows" in readme and "_xcorr.py" in readme
    tools = read("tools", "README.md")
    assert "bench_xcorr.py" in tools and "gen_xcorr_golden.py" in tools and "--xcorr" in tools
    header = read("include", "nxsig.h")
    assert re.search(r"\bint nxsig_xcorr\(nxsig_ctx\* ctx, const void\* a, int64_t n1, int64_t a_stride, const void\* b, int64_t n2, int64_t b_stride, int64_t batch,", header)
    assert re.search(r"\bint64_t nxsig_xcorr_fft_length\(int64_t n1, int64_t n2\);", header)
    for phrase in ("THE DEFINITION", "full[k] = sum_l x[l] conj(y[l - k + n2 - 1])", "full[k] = sum_l x[l] y[k - l]", "xcorr.wave", "xcorr.generic",
                   "NXSIG_XCORR_WAVE", "NXSIG_XCORR_SLAB_ROWS", "256 MiB", "no finite output element", "max(1024, the next power of two", "Not built",
                   "f64 / c128", "n-D correlation", "max_lag", "\"coeff\"", "sharded", "NIF and Elixir", "Every argument check comes ahead of the context"):
        assert phrase in header[header.index("Convolution.correlate_rows"):], phrase
    for name in ("nxsig_xcorr", "nxsig_xcorr_fft_length"):
        assert name in _lib.SIGNATURES
    # no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "xcorr" not in nif and "correlate_rows" not in read("elixir", "lib", "nx_signal_amd", "convolution.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.convolution.correlate_rows is convolution.correlate_rows is _xcorr.correlate_rows and convolution.convolve_rows is _xcorr.convolve_rows
    assert convolution.correlation_lags is _xcorr.correlation_lags and convolution.correlate_rows.__module__ == "nx_signal_amd._xcorr"
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_xcorr.py")) and os.path.exists(os.path.join(ROOT, "tools", "gen_xcorr_golden.py"))


def test_the_private_module_can_be_imported_first():
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._xcorr as m, nx_signal_amd.convolution as t; "
                        "assert t.correlate_rows is m.correlate_rows and t.convolve_rows is m.convolve_rows"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks over a sweep with the rejected ones, the tier and the transform length at their edges, the index maps against
    directly summed circular results, the mirror-bin map, the row scale, the slabs, and the fused kernel's lane arithmetic walked over
    exactly sized buffers (csrc/xcorr_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_xcorr")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_xcorr.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized xcorr host side ok" in r.stdout
