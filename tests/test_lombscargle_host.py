"""Spectral.lombscargle without a GPU: the numpy oracle (tests/lombscargle_oracle.py) against recorded SciPy 1.15.3 results
(tests/golden/lombscargle_vectors.json, tools/gen_lombscargle_golden.py), the argument checks of the Python function (each ahead of the
context), every argument error of the C entry point with a null context, the symbol and its signature, the switch, the sources and the
documents, and the blocking sizes."""
import base64
import ctypes as C
import json
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lombscargle_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, _lombscargle, spectral
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lombscargle_vectors.json")
with open(FIXTURE) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_LOMBSCARGLE) as f:
    ABI_GOLDEN = json.load(f)

ORACLE_TOL = 1e-12   # of each row's largest magnitude
# "amplitude" is a ratio of the shifted sums: it is compared where the oracle's shifted CC and SS are both at least this (elsewhere SciPy
# itself divides rounding noise by the clamp: w = 0 always, and every frequency of the two-sample rows under floating_mean)
CONDITIONED = 1e-3


def dec(a):
    return np.frombuffer(zlib.decompress(base64.b64decode(a["z"])), np.dtype(a["dtype"])).reshape(a["shape"]).copy()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("c", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_scipy(c):
    x, freqs, weights, y = dec(c["x"]), dec(c["freqs"]), dec(c["weights"]), dec(c["y"])
    assert y.dtype == np.float32 and freqs[0] == 0.0
    for pre, fm, wts, norm in O.COMBOS:
        want = dec(c["pgram"][O.combo_name(pre, fm, wts, norm)])
        got, cc, ss = O.lombscargle(x, y, freqs, pre, norm, weights if wts else None, fm, parts=True)
        assert got.shape == want.shape == (y.shape[0], c["F"]) and got.dtype == want.dtype
        keep = np.ones(c["F"], bool)
        if norm == "amplitude":
            keep = (cc >= CONDITIONED) & (ss >= CONDITIONED)
            assert not keep[0]
            if c["n"] >= 63:
                assert keep[1:].all(), (c["name"], pre, fm, wts)
        if keep.any():
            err = O.row_error(got[:, keep], want[:, keep])
            assert (err <= ORACLE_TOL).all(), (c["name"], O.combo_name(pre, fm, wts, norm), err)


def test_the_recorded_cases_are_the_ones_the_issue_lists():
    assert GOLDEN["scipy"] == "1.15.3"
    assert [tuple(s) for s in GOLDEN["shapes"]] == [(1, 3), (2, 5), (63, 17), (257, 96)]
    assert len(O.COMBOS) == 24 and GOLDEN["combos"] == [O.combo_name(*c) for c in O.COMBOS] and len(set(GOLDEN["combos"])) == 24
    assert all(set(c["pgram"]) == set(GOLDEN["combos"]) for c in GOLDEN["cases"])
    assert os.path.getsize(FIXTURE) <= 256 << 10


def test_the_oracle_takes_scipys_spellings_of_normalize():
    rng = np.random.Generator(np.random.PCG64(5))
    x, y, f = rng.uniform(0, 10, 20), rng.standard_normal((2, 20)), np.linspace(0.1, 3, 7)
    assert np.array_equal(O.lombscargle(x, y, f, normalize=False), O.lombscargle(x, y, f, normalize="power"))
    assert np.array_equal(O.lombscargle(x, y, f, normalize=True), O.lombscargle(x, y, f, normalize="normalize"))
    assert O.lombscargle(x, y, f, normalize="amplitude").dtype == np.complex128
    # a row alone and in a batch: the same sums, through a matrix-vector and a matrix-matrix product of numpy's
    alone, batch = O.lombscargle(x, y[1], f, True, True, None, True), O.lombscargle(x, y, f, True, True, None, True)[1]
    assert alone.shape == (7,) and O.row_error(alone, batch).max() <= 1e-13


def test_the_parity_inputs_leave_no_frequency_out():
    """the seeded inputs of the GPU parity test: "amplitude" is conditioned (shifted CC and SS >= 1e-3) at every frequency, under all
    eight option sets and for the f32-rounded rows as well"""
    x, y, freqs, weights = O.parity_inputs()
    assert y.shape == (3, 257) and freqs.shape == (96,) and 0.01 < freqs.min() and freqs.max() < 20 and 0 <= x.min() and x.max() < 100
    for pre, fm, wts, norm in O.COMBOS:
        if norm == "amplitude":
            for rows in (y, y.astype(np.float32)):
                _, cc, ss = O.lombscargle(x, rows, freqs, pre, norm, weights if wts else None, fm, parts=True)
                assert O.conditioned(cc, ss).all(), (pre, fm, wts)


X8 = np.arange(8.0)
Y8 = np.zeros((2, 8), np.float32)
F3 = np.array([0.5, 1.0, 2.0])
BAD = [
    ("x rank 2", dict(x=np.zeros((2, 4))), ArgumentError, "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"),
    ("x empty", dict(x=np.zeros(0), y=np.zeros((2, 0), np.float32)), ArgumentError, "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"),
    ("y length", dict(y=np.zeros((2, 7), np.float32)), ArgumentError, "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"),
    ("y rank 0", dict(y=np.float32(1.0)), ArgumentError, "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"),
    ("weights length", dict(weights=np.ones(7)), ArgumentError, "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"),
    ("freqs rank 2", dict(freqs=np.ones((2, 2))), ArgumentError, "Parameter freqs must be a 1-D array of non-zero length!"),
    ("freqs empty", dict(freqs=np.zeros(0)), ArgumentError, "Parameter freqs must be a 1-D array of non-zero length!"),
    ("negative weight", dict(weights=np.r_[-1.0, np.ones(7)]), ArgumentError,
     "Parameter weights must have only non-negative entries which sum to a positive value!"),
    ("zero weights", dict(weights=np.zeros(8)), ArgumentError, "Parameter weights must have only non-negative entries which sum to a positive value!"),
    ("weights nan", dict(weights=np.r_[np.nan, np.ones(7)]), ArgumentError, "weights must be finite"),
    ("x inf", dict(x=np.r_[np.inf, np.ones(7)]), ArgumentError, "x must be finite"),
    ("freqs nan", dict(freqs=np.array([1.0, np.nan])), ArgumentError, "freqs must be finite"),
    ("normalize text", dict(normalize="psd"), ArgumentError, "Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'."),
    ("normalize number", dict(normalize=2), ArgumentError, "Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'."),
    ("precenter", dict(precenter=1), ArgumentError, "precenter must be True or False"),
    ("floating_mean", dict(floating_mean="yes"), ArgumentError, "floating_mean must be True or False"),
    ("complex rows", dict(y=np.zeros((2, 8), np.complex64)), NxSignalUnsupported, "real f32 and f64 rows are built"),
    ("text rows", dict(y=np.array([["a"] * 8])), ArgumentError, "unsupported type"),
    ("complex times", dict(x=np.zeros(8, np.complex128)), ArgumentError, "x must be a real host array"),
    ("text freqs", dict(freqs=["a"]), ArgumentError, "freqs must be a real host array"),
]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_arguments_are_checked_ahead_of_the_context(case, monkeypatch):
    """every Python-side error is raised while default_context raises, and before the library is loaded"""
    _, change, error, pattern = case

    def no_context(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(S.device, "default_context", no_context)
    monkeypatch.setattr(_lib, "load", no_load)
    kw = dict(x=X8, y=Y8, freqs=F3)
    kw.update(change)
    pos = [kw.pop("x"), kw.pop("y"), kw.pop("freqs")]
    with pytest.raises(error, match=re.escape(pattern)):
        spectral.lombscargle(*pos, **kw)


class FakeDevice:
    """a device tensor as the package sees one (the CUDA array interface of device.py), without an allocation behind it"""

    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"data": (4096, False), "shape": shape, "typestr": typestr, "strides": None, "version": 3}


def test_a_device_tensor_must_be_f32_or_f64(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(NxSignalUnsupported, match="device tensors must be f32 or f64"):
        spectral.lombscargle(X8, FakeDevice((2, 8), "<i4"), F3)
    with pytest.raises(ArgumentError, match="equal non-zero length"):
        spectral.lombscargle(X8, FakeDevice((2, 9), "<f4"), F3)


def test_weights_and_floating_mean_are_keyword_only():
    with pytest.raises(TypeError):
        spectral.lombscargle(X8, Y8, F3, False, False, np.ones(8))


def test_c_abi_errors_with_a_null_context():
    """every argument error of nxsig_lombscargle comes ahead of the context: the recorded table, case by case, one argument broken at
    a time"""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.LOMBSCARGLE_TABLE_ENTRIES)
    assert table == ABI_GOLDEN["null_ctx"]
    rows = table["nxsig_lombscargle"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    for k, r in rows.items():
        if k != "valid":
            assert r["rc"] == (_lib.ERR_UNSUPPORTED if k == "rows too large" else _lib.ERR_INVALID_ARG) and r["err"] != "null context", (k, r)
            assert r["err"].startswith("lombscargle: ") or k == "mem=7", (k, r)
    assert {"null y", "null x", "null freqs", "null out", "mem=7", "dtype=2", "n=0", "num_freqs=0", "batch=0", "batch_stride=n-1", "precenter=2",
            "normalize=3", "floating_mean=-1", "x not finite", "freqs not finite", "weights not finite", "negative weight", "zero weights"} <= set(rows)
    sentence = "Parameter weights must have only non-negative entries which sum to a positive value!"
    assert sentence in rows["negative weight"]["err"] and sentence in rows["zero weights"]["err"]
    assert "null weights" not in rows   # weights may be NULL
    assert set(ABI_GOLDEN) == {"null_ctx", "real_ctx"} and ABI_GOLDEN["real_ctx"].keys() == table.keys()
    assert set(ABI_GOLDEN["real_ctx"]["nxsig_lombscargle"]) == set(rows)
    assert not any(name == "nxsig_lombscargle" for name, _, _ in P.ENTRIES)   # no row in the probe's base table


def test_the_symbol_its_signature_and_its_pointer_type():
    res, args = _lib.SIGNATURES["nxsig_lombscargle"]
    assert res is C.c_int and len(args) == 15 and args[0] is _lib._ctx_iir
    assert list(_lib.TYPED_CTX)[-1] is _lib._ctx_peaks and len(_lib.TYPED_CTX) == 4
    assert args[1:] == [_lib._p, _lib._i32, _lib._i64, _lib._i32, _lib._i64, _lib._p, _lib._p, _lib._i64, _lib._p, _lib._i32, _lib._i32, _lib._i32,
                        _lib._p, _lib._i32]
    assert _lib.SIGNATURES["nxsig_lombscargle_block"] == (_lib._i32, [_lib._i32])
    lib = C.CDLL(_lib.LIB_PATH)
    assert lib.nxsig_lombscargle and lib.nxsig_lombscargle_block
    header = read("include", "nxsig.h")
    assert re.search(r"\bint nxsig_lombscargle\(nxsig_ctx\* ctx, const void\* y, int32_t dtype, int64_t n, int32_t batch, int64_t batch_stride,", header)
    assert re.search(r"\bint32_t nxsig_lombscargle_block\(int32_t which\);", header)
    for phrase in ("Non-finite rule", "Deterministic", "Dispatch", "lombscargle.tile", "lombscargle.generic", "NXSIG_LOMBSCARGLE_TILE", "epsneg",
                   "Every argument check comes ahead of the context"):
        assert phrase in header[header.index("Spectral.lombscargle"):], phrase


def test_the_blocking_sizes_are_positive():
    lib = _lib.load()
    sizes = [lib.nxsig_lombscargle_block(w) for w in range(3)]
    assert all(isinstance(v, int) and v > 0 for v in sizes), sizes
    assert lib.nxsig_lombscargle_block(3) < 0 and lib.nxsig_lombscargle_block(-1) < 0


def test_the_switch_the_sources_and_the_documents_are_in_place():
    internal = read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "X(LOMBSCARGLE_TILE)" in internal and '#include "lombscargle_plan.hpp"' in internal and "kScratchSlots = 32" in internal
    assert "DISABLE_LOMBSCARGLE" not in internal
    tunables = internal[internal.index("#define NXSIG_TUNABLES"):internal.index("enum TuneKey")]
    assert tunables.rstrip().splitlines()[-1].rstrip().endswith("X(LOMBSCARGLE_TILE)")   # on the last line of the list
    src = read("nx_signal_amd", "csrc", "kernels_lombscargle.hip")
    assert "ctx_scratch(" not in src and "kScratch" not in src
    assert "tune(c, kT_LOMBSCARGLE_TILE, 1)" in src and '("kernels_lombscargle.hip", [])' in read("nx_signal_amd", "build.py")
    assert not re.findall(r"\batomic[A-Z]\w*", src)
    # the double sincos only: no f32 phase, no fast or native sine
    assert not re.findall(r"sincosf|sinf\(|cosf\(|__sinf|__cosf|__sincosf|__ocml_native|__builtin_amdgcn_(?:sin|cos)", src)
    assert 'dispatch_note("lombscargle.tile")' in src and 'dispatch_note("lombscargle.generic")' in src
    assert src.count("ctx_table(") == 3
    plan = read("nx_signal_amd", "csrc", "lombscargle_plan.hpp")
    assert all(name in plan for name in ("ls_check_shape", "ls_check_arrays", "ls_weights", "ls_tier", "ls_block"))
    assert "hip" not in plan.lower().replace("no hip types", "").replace("kernels_lombscargle.hip", "")
    assert "NXSIG_LOMBSCARGLE_TILE" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "3.19" in design and "lombscargle.tile" in design and "lombscargle.generic" in design
    readme = read("README.md")
    assert "spectral.lombscargle" in readme and "_lombscargle.py" in readme
    tools = read("tools", "README.md")
    assert "bench_lombscargle.py" in tools and "gen_lombscargle_golden.py" in tools and "--lombscargle" in tools
    # no NIF and no Elixir function: the shim's table keeps its 76 entries
    nif = read("nif", "nxsig_nif.c")
    assert "lombscargle" not in nif
    assert len(re.findall(r'^\s*\{"\w+", \d+, nif_\w+', nif, re.M)) == 76
    assert S.spectral.lombscargle is spectral.lombscargle is _lombscargle.lombscargle
    assert spectral.lombscargle.__module__ == "nx_signal_amd._lombscargle"
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_lombscargle.py"))


def test_the_private_module_can_be_imported_first():
    r = subprocess.run([sys.executable, "-c", "import nx_signal_amd._lombscargle as m, nx_signal_amd.spectral as t; "
                        "assert t.lombscargle is m.lombscargle"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
