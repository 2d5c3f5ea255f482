"""Filters.savgol_filter / savgol_coeffs without a GPU: the library's weights against the exact rational least-squares solution
(tests/savgol_oracle.py), the numpy oracle against recorded SciPy 1.15.3 results (tests/golden/savgol_vectors.json,
tools/gen_savgol_golden.py), the argument checks of the Python functions, every argument error of the C entry point (it validates before
it looks at the context, so a null context reaches every message), the switch / sources / documents, and the host side under ASan / UBSan
in a stand-alone program (tests/san_savgol.cpp)."""
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

import savgol_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "savgol_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_SAVGOL) as f:
    ABI_GOLDEN = json.load(f)

# every weight within 1e-12 max|k| of the rational solution: on a row whose offset is 1000 times its variation, with W <= 1025, the
# weights then contribute under a tenth of the suite's 1e-5 output bound
WEIGHT_TOL = 1e-12
# the oracle against SciPy where SciPy's own weights are sound to 1e-13 (the generator asserts it), relative to the row's largest output
ORACLE_TOL = 1e-12
DESIGNS = [(3, 1, 0), (4, 1, 0), (5, 2, 0), (5, 4, 3), (6, 3, 1), (16, 15, 0), (31, 3, 1), (101, 4, 2), (255, 5, 2), (512, 7, 3), (1025, 9, 4),
           (1025, 15, 4)]


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).copy()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def weight_gap(got, exact):
    want = np.array([float(v) for v in exact], np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_weights_are_the_exact_least_squares_weights():
    """every listed design at the default pos, one at pos = 2 with use="conv" and delta = 0.5: within 1e-12 max|k| of the rational
    solution; exact (anti)symmetry; an exactly zero centre for an odd derivative over an odd window; the figures are printed
    (profiles/savgol/accuracy.txt keeps a run's lines)"""
    worst, lines = 0.0, []
    for w, p, d in DESIGNS:
        k = filters.savgol_coeffs(w, p, deriv=d, use="dot")
        assert k.shape == (w,) and k.dtype == np.float64
        gap = weight_gap(k, O.exact_weights(w, p, d))
        lines.append(f"savgol-weights W={w} p={p} deriv={d}: {gap:.3e}")
        worst = max(worst, gap)
        assert gap <= WEIGHT_TOL, (w, p, d, gap)
        assert np.array_equal(k, -k[::-1] if d % 2 else k[::-1]), (w, p, d)
        assert np.array_equal(filters.savgol_coeffs(w, p, deriv=d), k[::-1])
        if w % 2 and d % 2:
            assert k[w // 2] == 0.0 and not np.signbit(k[w // 2])
    k = filters.savgol_coeffs(11, 3, deriv=1, delta=0.5, pos=2, use="conv")
    gap = weight_gap(k, O.exact_weights(11, 3, 1, 0.5, pos=2, use="conv"))
    lines.append(f"savgol-weights W=11 p=3 deriv=1 delta=0.5 pos=2 conv: {gap:.3e}")
    worst = max(worst, gap)
    assert gap <= WEIGHT_TOL
    assert not filters.savgol_coeffs(5, 2, deriv=3).any() and not filters.savgol_coeffs(7, 2, deriv=5, pos=1).any()   # deriv > polyorder
    assert filters.savgol_coeffs(1, 0).tolist() == [1.0]
    lines.append(f"savgol-weights-worst: {worst:.3e} (bound {WEIGHT_TOL:.0e})")
    print("\n".join(lines))


def test_the_oracles_edge_table_is_the_exact_fit():
    """the oracle forms E in double on the Legendre basis; a few rows against the rational solution"""
    for w, p, d in ((5, 2, 0), (31, 3, 1), (255, 5, 2), (1025, 9, 4)):
        E = O.edge_table(w, p, d)
        assert E.shape == (w // 2, w)
        for i in (0, 1, w // 2 - 1):
            assert weight_gap(E[i], O.exact_weights(w, p, d, pos=i)) <= 1e-11, (w, p, d, i)


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, y = dec(c["x"]), dec(c["y"])
    got = O.savgol_filter(x, c["window_length"], c["polyorder"], c["deriv"], c["delta"], c["mode"], c["cval"])
    assert got.shape == y.shape == (c["n"],)
    # SciPy rounds an f32 row once, from the same double sums: the oracle is rounded alike before the comparison
    gap = float(np.abs(got.astype(y.dtype).astype(np.float64) - y.astype(np.float64)).max() / np.abs(y).max())
    print(f"savgol-oracle-gap {c['name']}: {gap:.1e}")
    assert gap <= (ORACLE_TOL if y.dtype == np.float64 else 2.0 ** -23), (c["name"], gap)


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    cs = GOLDEN["cases"]
    assert GOLDEN["scipy"] == "1.15.3"
    assert [tuple(s) for s in GOLDEN["sets"]] == [(5, 2, 0), (5, 4, 3), (6, 3, 1), (7, 2, 1), (9, 4, 2), (11, 3, 0), (15, 5, 3), (31, 3, 1), (32, 3, 0),
                                                  (63, 4, 1), (101, 3, 1), (255, 3, 1)]
    assert {(c["window_length"], c["polyorder"], c["deriv"]) for c in cs} == {tuple(s) for s in GOLDEN["sets"]}
    assert max(GOLDEN["scipy_weight_gap"].values()) <= 1e-13
    assert {c["mode"] for c in cs} == set(O.MODES) and {c["delta"] for c in cs} == {0.5, 1.0}
    assert any(c["cval"] == 0.5 and c["mode"] == "constant" for c in cs)
    assert {c["x"]["dtype"] for c in cs} == {"<f4", "<f8"}
    ns = {c["n"] for c in cs}
    assert {1, 3, 64} <= ns and any(c["n"] == c["window_length"] for c in cs) and any(c["n"] == c["window_length"] + 1 for c in cs)
    assert {c["mode"] for c in cs if c["n"] < c["window_length"] // 2} == set(O.MODES) - {"interp"}
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f != "savgol_vectors.json")
    assert os.path.getsize(FIXTURE) <= largest


X32 = np.zeros(32, np.float32)
BAD = [
    ("polyorder", dict(polyorder=5), ArgumentError, "polyorder must be less than window_length."),
    ("mode", dict(mode="reflect"), ArgumentError, "mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'."),
    ("mode type", dict(mode=4), ArgumentError, "mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'."),
    ("interp length", dict(window_length=33, polyorder=2), ArgumentError, "If mode is 'interp', window_length must be less than or equal to the size of x."),
    ("window 0", dict(window_length=0, polyorder=0), ArgumentError, "window_length must be a positive integer"),
    ("window float", dict(window_length=5.0), ArgumentError, "window_length must be an integer"),
    ("window 1027", dict(window_length=1027, mode="mirror"), NxSignalUnsupported, "windows of up to 1025 samples are built"),
    ("polyorder 16", dict(window_length=31, polyorder=16), NxSignalUnsupported, "polynomials of up to degree 15 are built"),
    ("polyorder -1", dict(polyorder=-1), ArgumentError, "polyorder must be a nonnegative integer"),
    ("deriv -1", dict(deriv=-1), ArgumentError, "deriv must be a nonnegative integer"),
    ("deriv float", dict(deriv=1.0), ArgumentError, "deriv must be an integer"),
    ("delta 0", dict(delta=0.0), ArgumentError, "delta must be finite and non-zero"),
    ("delta nan", dict(delta=float("nan")), ArgumentError, "delta must be finite and non-zero"),
    ("cval inf", dict(mode="constant", cval=float("inf")), ArgumentError, "cval must be finite"),
    ("cval array", dict(mode="constant", cval=np.zeros(2)), ArgumentError, "cval must be a number"),
    ("complex", dict(x=np.zeros(32, np.complex64)), NxSignalUnsupported, "real f32 and f64 tensors are built"),
    ("text", dict(x=np.array(["a"] * 32)), ArgumentError, "unsupported type"),
    ("rank 0", dict(x=np.float32(1.0)), ArgumentError, "at least one axis"),
    ("empty", dict(x=np.zeros((2, 0), np.float32), mode="mirror"), ArgumentError, "empty dimension"),
    ("axis", dict(axis=1), ArgumentError, "axis 1 is out of bounds"),
    ("unknown option", dict(order=2), ArgumentError, "unknown keys"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_before_anything_runs(case):
    _, change, error, pattern = case
    kw = dict(x=X32, window_length=5, polyorder=2)
    kw.update(change)
    x, w, p = kw.pop("x"), kw.pop("window_length"), kw.pop("polyorder")
    with pytest.raises(error, match=re.escape(pattern)):
        filters.savgol_filter(x, w, p, **kw)


BAD_COEFFS = [
    (dict(polyorder=5), ArgumentError, "polyorder must be less than window_length."),
    (dict(pos=5), ArgumentError, "pos must be nonnegative and less than window_length."),
    (dict(pos=-1), ArgumentError, "pos must be nonnegative and less than window_length."),
    (dict(use="correlate"), ArgumentError, "`use` must be 'conv' or 'dot'."),
    (dict(delta=0), ArgumentError, "delta must be finite and non-zero"),
    (dict(window_length=1027), NxSignalUnsupported, "windows of up to 1025 samples are built"),
    (dict(mode="mirror"), ArgumentError, "unknown keys"),
]


@pytest.mark.parametrize("case", BAD_COEFFS, ids=lambda c: c[2][:24])
def test_coefficient_arguments_are_checked(case):
    change, error, pattern = case
    kw = dict(window_length=5, polyorder=2)
    kw.update(change)
    w, p = kw.pop("window_length"), kw.pop("polyorder")
    with pytest.raises(error, match=re.escape(pattern)):
        filters.savgol_coeffs(w, p, **kw)


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_savgol_filter comes ahead of the context: the recorded table, case by case"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.SAVGOL_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    rows = table["nxsig_savgol_filter"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    unsupported = {"window_length=1027", "polyorder=16", "rows too large"}
    for k, r in rows.items():
        if k != "valid":
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k in unsupported else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
    assert rows["polyorder=window_length"]["err"] == "savgol_filter: polyorder must be less than window_length."
    assert rows["mode=5"]["err"] == "savgol_filter: mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'."
    assert rows["interp window > length"]["err"] == "savgol_filter: If mode is 'interp', window_length must be less than or equal to the size of x."
    assert _lib.SIGNATURES["nxsig_savgol_filter"][1][0] is _lib._ctx_iir
    assert _lib.TYPED_CTX[-1] is _lib._ctx_peaks and len(_lib.TYPED_CTX) == 4
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()
    assert ABI_GOLDEN["real_ctx"]["nxsig_savgol_filter"].keys() == rows.keys()
    # the host-only entry point
    lib, out = _lib.load(), np.zeros(5, np.float64)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nxsig_savgol_coeffs(5, 2, 0, 1.0, -1.0, 1, po) == 0 and np.allclose(out, [-3 / 35, 12 / 35, 17 / 35, 12 / 35, -3 / 35], rtol=1e-15)
    for args, msg in (((5, 5, 0, 1.0, -1.0, 1, po), "polyorder must be less than window_length."),
                      ((5, 2, 0, 1.0, 5.0, 1, po), "pos must be nonnegative and less than window_length."),
                      ((5, 2, 0, 1.0, -0.5, 1, po), "pos must be nonnegative and less than window_length."),
                      ((5, 2, 0, 1.0, -1.0, 2, po), "`use` must be 'conv' or 'dot'."),
                      ((5, 2, 0, 1.0, -1.0, 1, None), "null pointer argument")):
        assert lib.nxsig_savgol_coeffs(*args) == _lib.ERR_INVALID_ARG and _lib.last_error() == "savgol_coeffs: " + msg


def test_a_typed_context_pointer_that_is_not_null_reaches_the_library():
    """the argument checks come ahead of the context, so a made-up non-null context with polyorder = window_length is refused and never
    looked at"""
    lib, V = _lib.load(), C.c_void_p
    x, y = np.zeros(16, np.float32), np.zeros(16, np.float32)
    fake = _lib.ctx_ptr(V(64), _lib._ctx_iir)
    assert isinstance(fake, _lib._ctx_iir)
    p = lambda a: a.ctypes.data_as(V)   # noqa: E731
    assert lib.nxsig_savgol_filter(fake, p(x), 0, 16, 1, 16, 5, 5, 0, 1.0, 4, 0.0, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "polyorder must be less than window_length." in _lib.last_error()
    assert lib.nxsig_savgol_filter(fake, p(x), 0, 16, 1, 16, 17, 2, 0, 1.0, 4, 0.0, p(y), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "window_length must be less than or equal to the size of x" in _lib.last_error()
    assert lib.nxsig_savgol_tile() == 2048


def test_the_switch_the_sources_and_the_documents_are_in_place():
    assert "X(DISABLE_SAVGOL_TILES)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    src = read("nx_signal_amd", "csrc", "kernels_savgol.hip")
    assert "tune(c, kT_DISABLE_SAVGOL_TILES, 0)" in src and '("kernels_savgol.hip", [])' in read("nx_signal_amd", "build.py")
    assert re.findall(r'#include "([^"]+)"', src) == ["nxsig_internal.h"]
    assert not re.findall(r"\batomic[A-Z]\w*", src) and "ctx_scratch" not in src
    assert '"savgol.tiles"' in src and '"savgol.generic"' in src
    plan = read("nx_signal_amd", "csrc", "savgol_plan.hpp")
    assert "kSavgolTile = 2048" in plan and "savgol_ext" in plan and "savgol_edge_table" in plan
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("no hip types", "").replace("kernels_savgol.hip", "")
    assert "kScratchSlots = 32" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "NXSIG_DISABLE_SAVGOL_TILES" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.15" in design and "savgol" in design and "not SciPy's" in design
    assert "savgol_filter" in read("README.md")
    tools = read("tools", "README.md")
    assert "bench_savgol.py" in tools and "gen_savgol_golden.py" in tools
    header = read("include", "nxsig.h")
    for name in ("nxsig_savgol_filter", "nxsig_savgol_coeffs", "nxsig_savgol_tile"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    assert "NOT SCIPY'S" in header and "ascending j" in header
    # this change adds no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "savgol" not in nif and "savgol" not in read("elixir", "lib", "nx_signal_amd", "filters.ex")
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.filters.savgol_filter is filters.savgol_filter and filters.savgol_filter.__module__ == "nx_signal_amd._savgol"
    assert os.path.exists(os.path.join(ROOT, "profiles", "savgol", "bench.json"))
    # the kept figures of one run: the weights against the rational solution, and every GPU case against the oracle
    kept = read("profiles", "savgol", "accuracy.txt")
    assert len(re.findall(r"^savgol-weights W=\d+ p=\d+ deriv=\d+: \d\.\d{3}e[-+]\d+$", kept, re.M)) == len(DESIGNS)
    assert re.search(r"^savgol-weights-worst: \d\.\d{3}e[-+]\d+ \(bound 1e-12\)$", kept, re.M)
    for w in (3, 4, 5, 6, 31, 32, 255, 1025):
        for t in ("float32", "float64"):
            assert re.search(r"^savgol-accuracy W=%d %s .*: \d\.\d{3}e[-+]\d+$" % (w, t), kept, re.M), (w, t)
    assert "savgol-accuracy offset-1000 deriv=2 W=1025" in kept and "savgol-accuracy scale=10000" in kept
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_savgol.py"))


def test_the_private_module_can_be_imported_first():
    """filters imports _savgol and _savgol needs a helper of filters: either order of import must work, in a fresh interpreter"""
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._savgol as m, nx_signal_amd.filters as f; assert f.savgol_filter is m.savgol_filter"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_side_under_asan_ubsan():
    """the argument checks, the weights against their moment conditions and a direct solve, E against the direct fit, the index rule
    against a brute-force extension for every mode and n = 1 .. 12, and the tile arithmetic (csrc/savgol_plan.hpp) in a stand-alone
    program with ASan / UBSan"""
    build = os.path.join(ROOT, "tests", "_san")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "san_savgol")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "nx_signal_amd", "csrc"), os.path.join(ROOT, "tests", "san_savgol.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitized savgol host side ok" in r.stdout
