"""Filters.median / wiener without a GPU: the numpy oracle (tests/filters_oracle.py) reproduces the reference's literals
(tests/golden/filters_vectors.json) with ==, the Python mirror raises the reference's ArgumentErrors before it needs a device, and the
C ABI declares and exports both entry points."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import filters_oracle as F
import nx_signal_amd as S
from nx_signal_amd import _lib
from nx_signal_amd._lib import ArgumentError, NxSignalUnsupported

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "filters_vectors.json")) as f:
        return json.load(f)


def test_oracle_reproduces_the_median_literals(vectors):
    assert len(vectors["median"]) == 4
    for v in vectors["median"]:
        got = F.median(np.array(v["input"], np.int64), tuple(v["kernel_shape"]))
        assert got.dtype == np.float32
        assert np.array_equal(got, np.array(v["expect"], np.float32)), v["name"]


def test_oracle_reproduces_the_wiener_literals_bit_for_bit(vectors):
    assert len(vectors["wiener"]) == 7
    for v in vectors["wiener"]:
        dt = np.float64 if v["dtype"] == "f64" else np.float32
        ks = v["kernel_size"] if isinstance(v["kernel_size"], int) else tuple(v["kernel_size"])
        got = F.wiener(np.array(v["input"], dt), ks, v["noise"])
        exp = np.array(v["expect"], dt)
        assert got.dtype == dt and np.array_equal(got.view(np.uint8), exp.view(np.uint8)), v["name"]


def test_oracle_median_window_is_clamped_not_padded():
    # outputs 7, 8, 9 of the 1-D literal reuse the last full window [3, 2, 6]
    got = F.median(np.array([10, 9, 8, 7, 1, 4, 5, 3, 2, 6]), (3,))
    assert got[7] == got[8] == got[9] == 3.0
    # even windows: the mean of the two middle values; NaN sorts last
    assert F.median(np.array([1.0, 4.0, 2.0, 8.0], np.float32), (2,)).tolist() == [2.5, 3.0, 5.0, 5.0]
    got = F.median(np.array([np.nan, 1.0, 2.0], np.float32), (3,))
    assert got.tolist() == [2.0, 2.0, 2.0]


def test_oracle_wiener_zero_variance_is_nan():
    # l_var = 0 and noise 0: (t - l_mean) * (1 - 0 / 0) + l_mean.  The zero tensor's estimate is 0 too; a constant c != 0 has edge
    # windows that reach into the zero padding, so only its interior (constant windows) comes out NaN
    with np.errstate(invalid="ignore"):
        assert np.all(np.isnan(F.wiener(np.zeros((4, 5)), 3, None)))
        got = F.wiener(np.full((4, 5), 3.0), 3, 0)
        assert np.all(np.isnan(got[1:-1, 1:-1])) and not np.any(np.isnan(got[0]))


@pytest.mark.parametrize("shape,ks", [((10,), (5, 5)), ((5, 5), (5, 5, 5))])
def test_median_rank_mismatch_raises_the_reference_message(vectors, shape, ks):
    msg = vectors["median_errors"][0]["message"]
    with pytest.raises(ArgumentError, match=f"^{msg}$"):
        S.filters.median(np.arange(int(np.prod(shape))).reshape(shape), kernel_shape=ks)


def test_median_option_and_type_errors():
    with pytest.raises(ArgumentError, match="unknown keys"):
        S.filters.median(np.arange(10), kernel_shape=(3,), kernel_size=3)
    with pytest.raises(ArgumentError, match="kernel shape must be of the same rank"):
        S.filters.median(np.arange(10))
    with pytest.raises(ArgumentError):
        S.filters.median(np.arange(10), kernel_shape=(11,))
    with pytest.raises(ArgumentError):
        S.filters.median(np.arange(10), kernel_shape=(0,))
    with pytest.raises(ArgumentError):
        S.filters.median(np.ones(4, np.complex64), kernel_shape=(3,))


def test_wiener_option_errors(vectors):
    msg = vectors["wiener_errors"][0]["message"]
    for bad in ("3", 3.0, [3, 3], None):
        with pytest.raises(ArgumentError, match=f"^{msg}$"):
            S.filters.wiener(np.ones((4, 4)), kernel_size=bad)
    with pytest.raises(ArgumentError):
        S.filters.wiener(np.ones((4, 4)), kernel_size=(3,))
    with pytest.raises(ArgumentError, match="unknown keys"):
        S.filters.wiener(np.ones((4, 4)), kernel_shape=(3, 3))
    with pytest.raises(NxSignalUnsupported):
        S.filters.wiener(np.ones((4, 4), np.int64))
    with pytest.raises(NxSignalUnsupported):
        S.filters.wiener(np.ones((4, 4), np.complex64))


def test_filter_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nxsig.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nxsig_median_filter", "nxsig_wiener"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_filter_tiles_switch_is_a_context_tunable():
    src = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "nxsig_internal.h")).read()
    assert "X(DISABLE_FILTER_TILES)" in src
    kern = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "kernels_filters.hip")).read()
    assert "tune(c, kT_DISABLE_FILTER_TILES, 0)" in kern and "#pragma clang fp contract(off)" in kern
