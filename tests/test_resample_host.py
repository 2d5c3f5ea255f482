"""Filters.resample_poly without a GPU: the length helper, the f64 oracle (tests/resample_oracle.py) against recorded
scipy.signal.resample_poly results (tests/golden/resample_vectors.json), the default anti-alias filter, and every argument error through
Python and through the C ABI (which validates before it looks at the context, so a null context and host arrays reach every message)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import resample_oracle as R
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "resample_vectors.json")) as f:
    GOLDEN = json.load(f)
with open(P.GOLDEN_OWN) as f:
    OWN_GOLDEN = json.load(f)

# measured on the CPU, see test_default_taps_against_scipy_s
TAPS_DIFF = {(1, 3): 4.63e-5, (147, 160): 5.38e-5}


def test_resample_length_is_the_ceiling_of_n_up_over_down():
    lib = _lib.load()
    for n in (0, 1, 2, 5, 199, 200, 48001, 2 ** 31 + 1):
        for up, down in ((1, 3), (3, 1), (2, 3), (4, 6), (160, 441), (147, 160), (5, 5), (48000, 16000), (7, 5), (2 ** 31 - 1, 3)):
            assert lib.nxsig_resample_length(n, up, down) == -((-n * up) // down) == R.length(n, up, down), (n, up, down)
    assert lib.nxsig_resample_length(-1, 1, 3) == _lib.ERR_INVALID_ARG and "length" in _lib.last_error()
    assert lib.nxsig_resample_length(8, 0, 3) == _lib.ERR_INVALID_ARG and lib.nxsig_resample_length(8, 1, -2) == _lib.ERR_INVALID_ARG
    assert "up and down must be >= 1" in _lib.last_error()
    assert lib.nxsig_resample_tile() >= 64


@pytest.mark.parametrize("e", GOLDEN["resample"], ids=lambda e: f"{e['up']}_{e['down']}")
def test_oracle_equals_scipy(e):
    h = R.design(e["up"], e["down"]) if e["h"] is None else np.array(e["h"])
    want = np.array(e["y"])
    got = R.resample_poly(np.array(e["x"]), e["up"], e["down"], h)
    assert got.shape == want.shape and e["scipy"] and "resample_poly" in e["call"]
    assert R.nmax_err(got, want) <= 1e-12


@pytest.mark.parametrize("up, down, L, n", [(1, 3, 61, 200), (3, 2, 61, 7), (160, 441, 8821, 130), (3, 4, 24, 90), (3, 4, 25, 2), (16, 1, 7, 9), (7, 5, 1, 33)])
def test_the_two_forms_of_the_oracle_agree(up, down, L, n):
    """the per-output sum and the per-tap passes (what the GPU tests run on long rows): the same values, the same non-finite outputs"""
    rng = np.random.Generator(np.random.PCG64(L + n))
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    h = rng.standard_normal(L)
    h[::5] = 0.0
    for xx in (x, x.real):
        a, b = R.resample_poly(xx, up, down, h), R.resample_poly_by_taps(xx, up, down, h)
        assert a.shape == b.shape == (2, R.length(n, up, down)) and R.nmax_err(b, a) <= 1e-15
    bad = x.real.copy()
    bad[1, n // 2], bad[1, 0] = np.inf, np.nan
    a, b = R.resample_poly(bad, up, down, h), R.resample_poly_by_taps(bad, up, down, h)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(a[0], b[0])


def test_the_golden_file_covers_what_it_should():
    assert sorted((e["up"], e["down"]) for e in GOLDEN["resample"]) == [(1, 3), (3, 2), (3, 4), (4, 6), (160, 441)]
    assert len([e for e in GOLDEN["resample"] if (e["up"], e["down"]) == (3, 4)][0]["h"]) == 24
    assert sorted((e["up"], e["down"]) for e in GOLDEN["taps"]) == [(1, 3), (147, 160)]


@pytest.mark.parametrize("ratio", [(1, 3), (160, 441), (147, 160), (4, 6)])
def test_default_taps_are_up_times_firwin_rounded_once(ratio):
    up, down = R.reduce(*ratio)
    big = max(up, down)
    want = (np.float64(up) * S.filters.firwin(20 * big + 1, [1.0 / big], window=("kaiser", 5.0), sampling_rate=2.0, type="f64")).astype(np.float32)
    got = S.filters.resample_poly_taps(*ratio)
    assert got.dtype == np.float32 and got.shape == (20 * big + 1,)
    assert got.tobytes() == want.tobytes() == R.design(*ratio).astype(np.float32).tobytes()
    hann = S.filters.resample_poly_taps(*ratio, window="hann")
    assert hann.tobytes() == (up * S.filters.firwin(20 * big + 1, [1.0 / big], window="hann", sampling_rate=2.0, type="f64")).astype(np.float32).tobytes()


@pytest.mark.parametrize("e", GOLDEN["taps"], ids=lambda e: f"{e['up']}_{e['down']}")
def test_default_taps_against_scipy_s(e):
    """max |ours - scipy's| / max |scipy's| of the f64 designs, measured on the CPU: 4.62e-5 at (1, 3), 5.37e-5 at (147, 160); the f32
    taps read the same.  That is the Kaiser window: Windows.kaiser evaluates I0 like the reference's (windows.ex:371-386: four terms of
    the power series below 3.75, a three-term asymptotic expansion above), scipy's i0 is exact to double.  Both figures exceed 1e-6; the bound is ten times the measured value (the margin is
    for another host's libm), not wider."""
    ours, theirs = R.design(e["up"], e["down"]), np.array(e["h"])
    assert ours.shape == theirs.shape
    d = float(np.abs(ours - theirs).max() / np.abs(theirs).max())
    d32 = float(np.abs(S.filters.resample_poly_taps(e["up"], e["down"]).astype(np.float64) - theirs).max() / np.abs(theirs).max())
    print(f"resample taps ({e['up']}, {e['down']}): f64 {d:.3e}, f32 {d32:.3e}")
    assert d <= 10 * TAPS_DIFF[(e["up"], e["down"])] and d32 <= 10 * TAPS_DIFF[(e["up"], e["down"])]
    assert abs(ours.sum() - e["up"]) < 1e-9 * e["up"]          # unit DC gain times up, like scipy's


X8 = np.linspace(-1, 1, 8, dtype=np.float32)


@pytest.mark.parametrize("args, kw, exc, text", [
    ((X8, 0, 1), {}, ArgumentError, "up and down must be >= 1"),
    ((X8, 1, 0), {}, ArgumentError, "up and down must be >= 1"),
    ((X8, -2, 3), {}, ArgumentError, "up and down must be >= 1"),
    ((X8, 1.5, 3), {}, ArgumentError, "must be an integer"),
    ((X8, 1, 2), {"taps": []}, ArgumentError, "tap vector is empty"),
    ((X8, 1, 2), {"taps": np.zeros((2, 2))}, ArgumentError, "1-D real"),
    ((X8, 1, 2), {"taps": np.zeros(3, np.complex64)}, ArgumentError, "1-D real"),
    ((X8, 1, 2), {"padtype": "line"}, ArgumentError, "padtype"),
    ((X8, 1, 2), {"padtype": "mean"}, ArgumentError, "padtype"),
    ((X8.astype(np.float64), 1, 2), {}, NxSignalUnsupported, "f32 and c64"),
    ((X8.astype(np.complex128), 1, 2), {}, NxSignalUnsupported, "f32 and c64"),
    ((np.arange(8), 1, 2), {}, NxSignalUnsupported, "f32 and c64"),
    ((X8, 1, 2), {"beta": 5.0}, ArgumentError, "unknown keys ['beta'] in resample_poly options"),
    ((X8, 1, 2), {"window": "boxcar"}, ArgumentError, "unknown window"),
    ((X8, 3, 3), {"window": "boxcar"}, ArgumentError, "unknown window"),
    ((X8, 1, 2), {"axis": 1}, ArgumentError, "axis"),
    ((np.zeros((2, 0), np.float32), 1, 2), {}, ArgumentError, "empty dimension"),
])
def test_python_argument_errors_need_no_gpu(args, kw, exc, text):
    with pytest.raises(exc) as ei:
        S.filters.resample_poly(*args, **kw)
    assert text in str(ei.value)


def test_c_abi_error_table_with_a_null_context():
    """tools/abi_error_probe.py, the probe behind tests/golden/abi_error_table.json, run over its OWN_TABLE_ENTRIES: valid arguments,
    then one argument broken at a time, ctx = NULL.  Codes and messages must be what tests/golden/abi_error_table_resample.json records
    (tests/test_gpu_resample.py compares the real-context half).  Every check of nxsig_resample_poly comes ahead of the context: each
    broken case answers with its own message, only the valid row says "null context"."""
    table = P.probe(_lib.LIB_PATH, real=False, entries=P.OWN_TABLE_ENTRIES)
    assert table == OWN_GOLDEN["null_ctx"]
    rows = OWN_GOLDEN["null_ctx"]["nxsig_resample_poly"]
    assert rows["valid"] == {"rc": _lib.ERR_INVALID_ARG, "err": "null context"}
    for label, rec in rows.items():
        assert label == "valid" or (rec["rc"] < 0 and rec["err"] and rec["err"] != "null context"), label
    assert rows["result too large"]["rc"] == _lib.ERR_UNSUPPORTED
    for label in ("null x", "null h", "null y", "mem=7", "batch=0", "length=0", "batch_stride=length-1", "up=0", "down=0", "num_taps=0"):
        assert label in rows
    assert set(OWN_GOLDEN["real_ctx"]["nxsig_resample_poly"]) == set(rows)


def test_every_entry_point_with_a_typed_context_has_its_own_table():
    """tests/test_abi_errors_host.py holds the entry points whose context is a plain void pointer to the recorded table, which predates
    this one; an entry point that declares nxsig_ctx* as the typed pointer _lib._ctx must be in the probe's OWN_TABLE_ENTRIES and in
    both halves of the golden file of its own — no compute entry point without a probed error table"""
    typed = {n for n, (_, args) in _lib.SIGNATURES.items() if args and args[0] is _lib._ctx}
    assert typed == {"nxsig_resample_poly"} == {name for name, _, _ in P.OWN_TABLE_ENTRIES}
    assert typed == set(OWN_GOLDEN["null_ctx"]) == set(OWN_GOLDEN["real_ctx"])
    assert not typed & {name for name, _, _ in P.ENTRIES}
    assert _lib.ctx_ptr(None) is None and isinstance(_lib.ctx_ptr(C.c_void_p(64)), _lib._ctx)


def test_every_layer_names_the_new_entry_points():
    """header, ctypes table, NIF table, Elixir stubs and the Elixir wrapper carry the new names (the cross-checks of
    tests/test_abi_and_host.py and tests/test_nif_shim.py compare the tables as wholes)"""
    read = lambda *p: open(os.path.join(ROOT, *p)).read()   # noqa: E731
    header = read("include", "nxsig.h")
    for name in ("nxsig_resample_length", "nxsig_resample_tile", "nxsig_resample_poly"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    shim, stubs, wrapper = read("nif", "nxsig_nif.c"), read("elixir", "lib", "nx_signal_amd", "nif.ex"), read("elixir", "lib", "nx_signal_amd", "filters.ex")
    for nif in ("resample_poly", "resample_poly_dev"):
        assert re.search(r'\{"%s", \d+, nif_%s, ERL_NIF_DIRTY_JOB_IO_BOUND\}' % (nif, nif), shim)
        assert re.search(r"def %s\(" % nif, stubs) and "NIF.%s(" % nif in wrapper
    assert re.search(r"def resample_poly\(", wrapper)
    assert "kernels_resample.hip" in read("nx_signal_amd", "build.py")
    assert "X(DISABLE_RESAMPLE_LDS)" in read("nx_signal_amd", "csrc", "nxsig_internal.h")
    assert "tune(c, kT_DISABLE_RESAMPLE_LDS, 0)" in read("nx_signal_amd", "csrc", "kernels_resample.hip")
