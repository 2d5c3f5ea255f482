"""Transforms.dct / idct and mfcc without a GPU: the numpy oracle (tests/dct_oracle.py) against recorded SciPy 1.15.3 results
(tests/golden/dct_vectors.json, tools/gen_dct_golden.py), the tier choice, the tables and the geometry of csrc/dct_plan.hpp, the argument
checks of the Python functions, every argument error of the C entry point (it validates before it looks at the context, so a null
context reaches every message), the switch / sources / documents, the recorded GPU accuracy lines, and the host side under ASan / UBSan
in a stand-alone program (tests/san_dct.cpp)."""
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

import dct_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _dct, _lib, transforms
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dct_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_DCT) as f:
    ABI_GOLDEN = json.load(f)

# the oracle (a matrix product in double) and SciPy (pocketfft in double) each round at most n times 2^-53 of the row's magnitude: 9e-13
# for the longest row recorded (4099) and both together; 1e-11 of the row maximum leaves a factor of five
ORACLE_TOL = 1e-11
SIZES = [1, 2, 3, 8, 13, 80, 128, 255, 256, 257, 400, 1000, 1024, 4099]
NORM_KEYS = {None: "None", "ortho": "ortho", "forward": "forward"}


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).reshape(a["shape"]).copy()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, at = np.moveaxis(dec(c["x"]), c["axis"], -1), dec(c["at"])
    assert x.dtype == np.float32
    for fn in (O.dct, O.idct):
        for t in O.TYPES:
            for norm in O.NORMS:
                y = np.moveaxis(dec(c["y"][f"{fn.__name__}_{t}_{NORM_KEYS[norm]}"]), c["axis"], -1)
                got = np.take(fn(x, t, c["n"], norm), at, axis=-1)
                assert got.shape == y.shape and y.dtype == np.float64
                full = np.abs(fn(x, t, c["n"], norm)).max()
                gap = float(np.abs(got - y).max())
                assert gap <= ORACLE_TOL * full, (c["name"], fn.__name__, t, norm, gap, full)


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    cs = {c["name"]: c for c in GOLDEN["cases"]}
    assert GOLDEN["scipy"] == "1.15.3" and GOLDEN["lengths"] == SIZES
    assert all(f"L{n}" in cs and cs[f"L{n}"]["n"] is None for n in SIZES)
    assert sorted(tuple(r) for r in GOLDEN["resized"]) == sorted([(7, 16), (100, 257), (8, 5), (300, 128)])
    assert all(f"L{l}_n{n}" in cs for l, n in GOLDEN["resized"])
    assert sum(c["axis"] == 0 and len(c["x"]["shape"]) == 2 for c in cs.values()) >= 1
    assert all(len(c["y"]) == 12 for c in cs.values()) and GOLDEN["types"] == [2, 3] and GOLDEN["norms"] == [None, "ortho", "forward"]
    assert os.path.getsize(FIXTURE) <= 512 << 10


@pytest.mark.parametrize("n", [1, 2, 3, 8, 13, 80, 257])
def test_idct_of_dct_returns_the_row_in_the_oracle(n):
    x = np.random.Generator(np.random.PCG64(n)).standard_normal((3, n))
    for t in O.TYPES:
        for norm in O.NORMS + ("backward",):
            back = O.idct(O.dct(x, t, None, None if norm == "backward" else norm), t, None, norm)
            assert np.abs(back - x).max() <= 1e-12 * np.abs(x).max(), (n, t, norm)


@pytest.mark.parametrize("n", SIZES)
def test_the_oracles_fft_form_and_its_sampled_definition_equal_the_definition(n):
    """dct_fast (np.fft in double) and dct_at (the definition at a few coefficients) are what the GPU tests use on rows too long for the
    n x n matrix; here both are held to the matrix form on every recorded length, padding and truncation included"""
    x = np.random.Generator(np.random.PCG64(100 + n)).standard_normal((2, n + 3))
    for t in O.TYPES:
        for norm in O.NORMS:
            for nn in (n, n + 7):
                ref = O.dct(x, t, nn, norm)
                top = np.abs(ref).max()
                assert np.abs(O.dct_fast(x, t, nn, norm) - ref).max() <= ORACLE_TOL * top, (n, t, norm, nn)
                at = O.places(nn)
                assert np.abs(O.dct_at(x, at, t, nn, norm) - ref[..., at]).max() <= ORACLE_TOL * top, (n, t, norm, nn)
    assert np.array_equal(O.dct_fast(x, 2, n, "ortho", keep=1), O.dct_fast(x, 2, n, "ortho")[..., :1])


def test_keep_is_the_leading_slice_in_the_oracle():
    x = np.arange(24.0).reshape(2, 12) % 5
    assert np.array_equal(O.dct(x, 2, 16, "ortho", keep=5), O.dct(x, 2, 16, "ortho")[:, :5])


@pytest.fixture(scope="module")
def plan():
    """csrc/dct_plan.hpp behind a few C functions, in a small shared library of its own (plain g++: the header has no HIP types)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    src, so = os.path.join(build, "dct_plan_c.cpp"), os.path.join(build, "dct_plan_c.so")
    with open(src, "w") as f:
        f.write('#include <cstring>\n#include "dct_plan.hpp"\nextern "C" {\n'
                "int dp_tier(long long n, int off) { return nxsig::dct_tier(n, off != 0); }\n"
                "void dp_direct(long long n, long long keep, int type, int norm, float* out) {\n"
                "  const auto t = nxsig::dct_direct_table(n, keep, type, norm); std::memcpy(out, t.data(), t.size() * sizeof(float)); }\n"
                "void dp_fft(long long n, int type, int norm, float* out) {\n"
                "  const auto t = nxsig::dct_fft_table(n, type, norm); std::memcpy(out, t.data(), t.size() * sizeof(float)); }\n"
                "float dp_dc(long long n, int norm) { return nxsig::dct_dc_gain(n, norm); }\n"
                "void dp_geom(long long n, long long keep, long long batch, long long* out) {\n"
                "  const auto g = nxsig::dct_geom(n, keep, batch); out[0] = g.pitch; out[1] = g.groups; out[2] = g.tile_rows; out[3] = g.tiles; }\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    lib.dp_tier.argtypes = [C.c_longlong, C.c_int]
    lib.dp_direct.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    lib.dp_fft.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    lib.dp_dc.argtypes, lib.dp_dc.restype = [C.c_longlong, C.c_int], C.c_float
    lib.dp_geom.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]
    return lib


def direct_table(plan, n, keep, t, norm):
    out = np.empty((n, keep), np.float32)
    plan.dp_direct(n, keep, t, norm, out.ctypes.data_as(C.c_void_p))
    return out


def test_the_tier_choice(plan):
    for n in SIZES + [64, 2048, 65536]:
        assert plan.dp_tier(n, 0) == (0 if n <= 256 else 1), n
        assert plan.dp_tier(n, 1) == 1, n


@pytest.mark.parametrize("n", [1, 2, 3, 8, 13, 80, 128, 255, 256])
def test_the_direct_table(plan, n):
    """Tt[j][k] against the oracle's matrix to f32 rounding; exact zeros where k (2 j + 1) is an odd multiple of n; T[k][n - 1 - j] =
    (-1)^k T[k][j] to the bit; a table of `keep` coefficients is the leading part of the full one; the n = 1 and keep = 1 edges"""
    eye = np.eye(n)
    for code, norm in enumerate(O.NORMS):
        for t in O.TYPES:
            full = direct_table(plan, n, n, t, code)
            want = O.dct(eye, t, None, norm)          # row j: the transform of the unit impulse at j = column j of the matrix
            assert np.abs(full - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.0001, (n, t, norm)
            for keep in {1, max(1, n // 2), n}:
                assert np.array_equal(direct_table(plan, n, keep, t, code), full[:, :keep]), (n, keep, t, norm)
        t2 = direct_table(plan, n, n, 2, code)
        k, j = np.arange(n)[None, :], np.arange(n)[:, None]
        zero = (k * (2 * j + 1)) % (2 * n) == n
        assert np.all(t2[zero] == 0.0) and np.all(t2[~zero] != 0.0), (n, norm)
        assert np.array_equal(t2[::-1], t2 * np.where(np.arange(n) % 2, -1.0, 1.0).astype(np.float32)[None, :]), (n, norm)
        assert abs(float(t2[:, 0].astype(np.float64).sum()) - plan.dp_dc(n, code)) <= 1e-6 * plan.dp_dc(n, code)
    assert direct_table(plan, 1, 1, 2, 0)[0, 0] == 2.0 and direct_table(plan, 1, 1, 3, 0)[0, 0] == 1.0
    assert direct_table(plan, 1, 1, 2, 1)[0, 0] == 1.0 and direct_table(plan, 1, 1, 3, 1)[0, 0] == 1.0


@pytest.mark.parametrize("n", [1, 2, 13, 257, 1000, 4099])
def test_the_twiddle_table(plan, n):
    k = np.arange(n)
    for code, norm in enumerate(O.NORMS):
        tw = np.empty((n, 2), np.float32)
        plan.dp_fft(n, 2, code, tw.ctypes.data_as(C.c_void_p))
        g = np.full(n, 2.0)
        if norm == "ortho":
            g = np.where(k == 0, 2 * np.sqrt(1 / (4 * n)), 2 * np.sqrt(1 / (2 * n)))
        elif norm == "forward":
            g = g / (2 * n)
        want = np.stack([g * np.cos(np.pi * k / (2 * n)), g * np.sin(np.pi * k / (2 * n))], axis=1)
        assert np.abs(tw - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.0001 and tw[0, 1] == 0.0


def test_the_geometry_keeps_inside_the_lds_image(plan):
    for n in range(1, 257):
        for keep in {1, 13 if n >= 13 else n, n}:
            g = (C.c_longlong * 4)()
            plan.dp_geom(n, keep, 70000, g)
            pitch, groups, tile_rows, tiles = g
            assert pitch >= n + 1 and pitch % 4 == 0 and (pitch // 4) % 2 == 1
            assert groups >= 1 and groups * keep <= 256 and tile_rows == 8 * groups and tile_rows * pitch <= 8192
            assert (tiles - 1) * tile_rows < 70000 <= tiles * tile_rows


X32 = np.zeros(32, np.float32)
BAD = [
    ("type 1", dict(type=1), NxSignalUnsupported, "unsupported type 1"),
    ("type 4", dict(type=4), NxSignalUnsupported, "unsupported type 4"),
    ("type 5", dict(type=5), ArgumentError, "type must be 2 or 3"),
    ("type float", dict(type=2.0), ArgumentError, "type must be an integer"),
    ("keep 0", dict(keep=0), ArgumentError, "keep must be in [1, n]"),
    ("keep > n", dict(keep=33), ArgumentError, "keep must be in [1, n]"),
    ("keep > n given", dict(n=16, keep=17), ArgumentError, "keep must be in [1, n]"),
    ("n 0", dict(n=0), ArgumentError, "n must be positive"),
    ("n float", dict(n=32.0), ArgumentError, "n must be an integer"),
    ("n 2^31", dict(n=1 << 31), NxSignalUnsupported, "unsupported n"),
    ("norm", dict(norm="unitary"), ArgumentError, "norm must be None, 'backward', 'ortho' or 'forward'"),
    ("complex", dict(x=np.zeros(32, np.complex64)), ValueError, "x must be real."),
    ("f64", dict(x=np.zeros(32, np.float64)), NxSignalUnsupported, "unsupported type float64"),
    ("text", dict(x=np.array(["a"] * 32)), ArgumentError, "unsupported type"),
    ("rank 0", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("empty", dict(x=np.zeros((2, 0), np.float32)), ArgumentError, "empty dimension"),
    ("axis", dict(axis=1), ArgumentError, "axis 1 is out of bounds"),
    ("orthogonalize", dict(orthogonalize=True), ArgumentError, "unknown keys"),
    ("overwrite_x", dict(overwrite_x=True), ArgumentError, "unknown keys"),
    ("workers", dict(workers=2), ArgumentError, "unknown keys"),
]


@pytest.mark.parametrize("fn", ["dct", "idct"])
@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(case, fn, monkeypatch):
    """every Python-side error comes before the library is loaded"""
    _, change, error, pattern = case
    if fn == "idct" and "keep" in change:
        error, pattern = ArgumentError, "unknown keys"       # keep is dct's alone

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    kw = dict(x=X32)
    kw.update(change)
    with pytest.raises(error, match=re.escape(pattern)):
        getattr(transforms, fn)(kw.pop("x"), **kw)


class FakeDevice:
    """a device tensor as the package sees one (the CUDA array interface of device.py), without an allocation behind it: the refusals
    under test come before anything dereferences the address"""

    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"data": (4096, False), "shape": shape, "typestr": typestr, "strides": None, "version": 3}


def test_a_device_tensor_is_taken_along_its_last_axis_only(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    for fn in (transforms.dct, transforms.idct):
        with pytest.raises(NxSignalUnsupported, match="last axis"):
            fn(FakeDevice((4, 32), "<f4"), axis=0)
        with pytest.raises(NxSignalUnsupported, match="unsupported type float64"):
            fn(FakeDevice((4, 32), "<f8"))
        with pytest.raises(NxSignalUnsupported, match="device tensors must be f32"):
            fn(FakeDevice((4, 32), "<i4"))


MFCC_BAD = [
    ("n_mfcc > mel_bins", dict(n_mfcc=81, mel_bins=80), "n_mfcc must be in [1, mel_bins]"),
    ("n_mfcc > default mel_bins", dict(n_mfcc=129), "n_mfcc must be in [1, mel_bins]"),
    ("n_mfcc 0", dict(n_mfcc=0), "n_mfcc must be in [1, mel_bins]"),
    ("n_mfcc float", dict(n_mfcc=13.0), "n_mfcc must be an integer"),
    ("unknown key", dict(lifter=22), "unknown keys"),
    ("no sampling rate", dict(sampling_rate=None), "missing sampling_rate"),
]


@pytest.mark.parametrize("case", MFCC_BAD, ids=lambda c: c[0])
def test_mfcc_arguments_are_checked_before_anything_runs(case, monkeypatch):
    """... before a context is asked for (the option parsing of stft loads the library for nxsig_next_pow2, which needs no GPU)"""
    _, change, pattern = case

    def no_context(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")
    monkeypatch.setattr(S.device, "default_context", no_context)
    kw = dict(sampling_rate=16000, overlap_length=240)
    kw.update(change)
    with pytest.raises(ArgumentError, match=re.escape(pattern)):
        S.mfcc(np.zeros(4096, np.float32), np.hanning(400).astype(np.float32), **kw)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_dct_f32 comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.DCT_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    rows = table["nxsig_dct_f32"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    assert rows["batch=0"] == rows["valid"]        # batch = 0 passes every check and reaches the context
    unsupported = {"type=1", "type=4", "n=2^31", "rows too large", "result too large"}
    for k, r in rows.items():
        if k not in ("valid", "batch=0"):
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
            assert r["err"].startswith("dct: ") or k == "mem=7", (k, r)
    assert "type 1" in rows["type=1"]["err"] and "type 4" in rows["type=4"]["err"]
    assert {"null x", "null out", "length=0", "n=0", "batch=-1", "batch_stride=length-1", "type=5", "norm=3", "keep=0", "keep=n+1", "mem=7"} <= set(rows)
    assert _lib.SIGNATURES["nxsig_dct_f32"][1][0] is _lib._ctx_iir
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()
    assert set(ABI_GOLDEN["real_ctx"]["nxsig_dct_f32"]) == set(rows) - {"batch=0"}


def test_the_switch_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(DISABLE_DCT_DIRECT)" in internal and "kScratchSlots = 32" in internal and '#include "dct_plan.hpp"' in internal
    src = read("nx_signal_amd", "csrc", "kernels_dct.hip")
    assert "tune(c, kT_DISABLE_DCT_DIRECT, 0)" in src and '("kernels_dct.hip", [])' in read("nx_signal_amd", "build.py")
    assert not re.findall(r"\batomic[A-Z]\w*", src) and "sincosf" not in src
    assert 'dispatch_note("dct.direct")' in src and 'dispatch_note("dct.fft")' in src
    # every inner transform runs without the Nx.fft clean-up
    assert re.findall(r"launch_fft(?:_big)?\(c, [^;]*?, (\w+)\)\)\) return rc;", src) == ["false", "false"]
    assert set(re.findall(r"kScratch\w+", src)) == {"kScratchFusedSpectrum", "kScratchIstftProduct"}
    assert "gridDim.y" not in src and "blockIdx.y" not in src
    plan = read("nx_signal_amd", "csrc", "dct_plan.hpp")
    assert all(name in plan for name in ("dct_check", "dct_tier", "dct_direct_table", "dct_fft_table", "dct_geom", "dct_cos"))
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_dct.hip", "")
    assert "dct_plan.hpp" in read("tests", "san_dct.cpp")
    assert "NXSIG_DISABLE_DCT_DIRECT" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.17" in design and "dct.direct" in design and "dct.fft" in design
    readme = read("README.md")
    assert "transforms.dct" in readme and "mfcc" in readme
    tools = read("tools", "README.md")
    assert "bench_dct.py" in tools and "gen_dct_golden.py" in tools
    header = read("include", "nxsig.h")
    assert re.search(r"\bnxsig_dct_f32\(", header) and "nxsig_dct_f32" in _lib.SIGNATURES
    assert "cos(pi k (2 j + 1) / (2 n))" in header and "NXSIG_DCT_ORTHO" in header and "no finite output element" in header
    # this change adds no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "dct" not in nif and "mfcc" not in nif and "dct" not in read("elixir", "lib", "nx_signal_amd", "transforms.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.transforms.dct is transforms.dct is _dct.dct and transforms.idct is _dct.idct and S.mfcc is _dct.mfcc
    assert "stft_to_mel" in S.mfcc.__doc__ and "librosa" in S.mfcc.__doc__ and "(x + 4) / 4" in S.mfcc.__doc__
    assert os.path.exists(os.path.join(ROOT, "profiles", "dct", "bench.json"))
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_dct.py"))


def test_the_recorded_gpu_accuracy_stays_under_the_bound():
    """profiles/dct/accuracy.txt: the lines tests/test_gpu_dct.py printed on an MI355X, every figure under 1e-5"""
    text = read("profiles", "dct", "accuracy.txt")
    lines = re.findall(r"^dct-accuracy (\S+) (.*)$", text, re.M)
    # 10 direct + 7 fft + 3 forced lengths, 2 of 70 000 rows, 8 offset cases, 6 round trips, 2 mfcc framings
    assert len(lines) >= 38
    assert {fam for fam, _ in lines} >= {"direct", "fft", "fft-forced", "offset-1000-direct", "offset-1000-fft", "mfcc"}
    for fam, rest in lines:
        figures = [float(v) for v in re.findall(r"(\d\.\d{3}e[-+]\d+)", rest)]
        assert figures and max(figures) <= 1e-5, (fam, rest)


def test_the_private_module_can_be_imported_first():
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._dct as m, nx_signal_amd.transforms as t, nx_signal_amd as s; "
                        "assert t.dct is m.dct and s.mfcc is m.mfcc"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks, the reduced cosine, the tables and the direct kernel's tile / LDS / store arithmetic walked over exactly sized
    buffers (csrc/dct_plan.hpp) in a stand-alone program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_dct")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_dct.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized dct host side ok" in r.stdout
