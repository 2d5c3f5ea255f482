"""PeakFinding without a GPU: the numpy oracle (tests/peaks_oracle.py) reproduces the reference's literals
(tests/golden/peak_finding_vectors.json) and scipy.signal.argrelextrema, the Python mirror raises its ArgumentErrors before it needs a
device, and the C ABI declares and exports both entry points."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import nx_signal_amd as S
import peaks_oracle as P
from nx_signal_amd import _lib
from nx_signal_amd._lib import ArgumentError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def custom_comparator(tag, x):
    """the two custom comparators of the reference's argrelextrema doctests, by their fixture tag"""
    if tag == "ge_double":
        return lambda a, b: np.greater_equal(a, np.multiply(b, 2))
    low = np.min(x)
    return lambda a, b: np.less(a, b) & np.not_equal(a, low) & np.not_equal(b, low)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "peak_finding_vectors.json")) as f:
        return json.load(f)["vectors"]


def check_literal(v, indices, valid):
    rows = np.array(v["expect_rows"], np.int32)
    x = np.array(v["input"])
    assert indices.dtype == np.int32 and indices.shape == (x.size, x.ndim), v["name"]
    assert int(valid) == v["expect_valid"], v["name"]
    assert np.array_equal(indices[: len(rows)], rows), v["name"]
    if v["rows_shown"] == "all":
        assert len(rows) == x.size, v["name"]


def test_oracle_reproduces_every_literal(vectors):
    assert len(vectors) == 10
    for v in vectors:
        x = np.array(v["input"])
        cmp = {"argrelmin": "less", "argrelmax": "greater"}.get(v["function"]) or custom_comparator(v["comparator"], x)
        indices, valid = P.argrelextrema(x, cmp, **v["options"])
        check_literal(v, indices, valid)


@pytest.mark.parametrize("seed", range(6))
def test_oracle_matches_scipy(seed):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(seed)
    rank = 1 + seed % 3
    shape = tuple(int(v) for v in rng.integers(1, 9, rank))
    x = rng.integers(0, 4, shape)
    for axis in range(rank):
        for order in (1, 2, 3, 5, 9):
            for name, fn in P.COMPARATORS.items():
                m = P.mask(x, name, axis, order)
                ref = signal.argrelextrema(x, fn, axis=axis, order=order, mode="clip")
                assert np.array_equal(np.argwhere(m).T, np.array(ref)), (shape, axis, order, name)


def test_oracle_quirks():
    x = np.array([3.0, 1.0, 2.0, np.nan, 1.0, 0.5, -0.0, 0.0, 2.0])
    # order <= 0 marks every element, NaN included
    for order in (0, -1, -0.5):
        assert P.mask(x, "less", 0, order).all()
    # a NaN is never marked and unmarks its neighbours; -0.0 == +0.0
    assert P.mask(x, "less", 0, 1).tolist() == [False, True, False, False, False, False, False, False, False]
    assert P.mask(x, "less_equal", 0, 1).tolist() == [False, True, False, False, False, False, True, True, False]
    # only the ends compare with themselves: less_equal marks a constant line everywhere, less nowhere
    assert P.mask(np.ones(5), "less_equal", 0, 7).all() and not P.mask(np.ones(5), "less", 0, 7).any()
    # fractional orders round up
    assert np.array_equal(P.mask(x, "greater", 0, 1.5), P.mask(x, "greater", 0, 2))


@pytest.mark.parametrize("fn", ["argrelmin", "argrelmax"])
def test_argument_errors(fn):
    f = getattr(S.peak_finding, fn)
    with pytest.raises(ArgumentError, match="unknown keys"):
        f(np.arange(5), ordre=2)
    with pytest.raises(ArgumentError, match="rank-0"):
        f(np.float32(1.0))
    with pytest.raises(ArgumentError, match="out of range"):
        f(np.zeros((3, 4)), axis=2)
    with pytest.raises(ArgumentError, match="out of range"):
        f(np.zeros((3, 4)), axis=-3)
    with pytest.raises(ArgumentError, match="complex"):
        f(np.zeros(4, np.complex64))
    with pytest.raises(ArgumentError, match="empty dimension"):
        f(np.zeros((3, 0)))
    with pytest.raises(ArgumentError, match="rank must be at most 8"):
        f(np.zeros((1,) * 9))
    with pytest.raises(ArgumentError, match="order"):
        f(np.zeros(4), order="2")
    with pytest.raises(ArgumentError, match="axis"):
        f(np.zeros(4), axis=0.0)


def test_argrelextrema_argument_errors():
    with pytest.raises(ArgumentError, match="unknown comparator"):
        S.peak_finding.argrelextrema(np.arange(5), "equal")
    with pytest.raises(ArgumentError, match="comparator must be"):
        S.peak_finding.argrelextrema(np.arange(5), 3)
    with pytest.raises(ArgumentError, match="unknown keys"):
        S.peak_finding.argrelextrema(np.arange(5), "less", kind=1)
    with pytest.raises(ArgumentError, match="complex"):
        S.peak_finding.argrelextrema(np.zeros(4, np.complex64), lambda a, b: a < b)


def test_peak_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nxsig.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nxsig_argrelextrema", "nxsig_nonzero"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name, value in (("NXSIG_DT_U64", 5), ("NXSIG_CMP_GREATER_EQUAL", 3)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
    assert S.peak_finding.argrelmin and S.peak_finding.argrelmax and S.peak_finding.argrelextrema


def test_peak_tiles_switch_is_a_context_tunable():
    src = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "nxsig_internal.h")).read()
    assert "X(DISABLE_PEAK_TILES)" in src
    kern = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "kernels_peaks.hip")).read()
    assert "tune(c, kT_DISABLE_PEAK_TILES, 0)" in kern
    # the ordered compaction takes no atomics and no inter-workgroup flags
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", kern)
