"""istft_masked / spectrum_mask without a GPU: the declarations of the three layers agree, and every shape / type / placement /
option mistake raises ArgumentError before a context (and with it the GPU) is touched."""
import os
import re

import numpy as np
import pytest

import nif_harness as H
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib

NEW = ("nxsig_spectrum_mask_c64", "nxsig_istft_masked_c64")


def test_header_library_and_signatures_agree():
    header = open(os.path.join(ROOT, "include", "nxsig.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the parameter counts of the declarations and of the ctypes signatures
    for name in NEW:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "spectrum_mask" in S.__all__ and "istft_masked" in S.__all__
    for k, v in (("NXSIG_MASK_REAL", 0), ("NXSIG_MASK_ONESIDED", 1), ("NXSIG_MASK_COMPLEX", 2)):
        assert re.search(r"\b%s = %d\b" % (k, v), header), k


def test_the_switch_is_in_the_tuning_table():
    src = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "nxsig_internal.h")).read()
    assert "X(DISABLE_FUSED_MASK)" in src and "X(DISABLE_FUSED_FILTER)" in src


def test_nif_table_has_the_two_entries():
    H.build()
    table = H.funcs()
    assert ("spectrum_mask", 8) in table and ("istft_masked", 9) in table
    assert table[("spectrum_mask", 8)] in (1, 2) and table[("istft_masked", 9)] in (1, 2)   # dirty jobs
    nif_ex = open(os.path.join(ROOT, "elixir", "lib", "nx_signal_amd", "nif.ex")).read()
    assert re.search(r"def spectrum_mask\((\s*_\w+,){7}\s*_\w+\)", nif_ex) and re.search(r"def istft_masked\((\s*_\w+,){8}\s*_\w+\)", nif_ex)


class FakeDevice:
    """a device-resident operand as far as the placement checks can tell (never dereferenced: the checks come first)"""

    def __init__(self, shape, dtype):
        self.__cuda_array_interface__ = {"data": (4096, False), "shape": tuple(shape), "typestr": np.dtype(dtype).str,
                                         "strides": None, "version": 3}


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create or fetch a context fails the test"""
    def boom(*a, **k):
        raise AssertionError("a context was requested before the arguments were validated")
    monkeypatch.setattr(S, "default_context", boom)
    monkeypatch.setattr(S.device, "default_context", boom)
    monkeypatch.setattr(S.Context, "__init__", boom)


def _z(shape):
    return np.zeros(shape, np.complex64)


W = np.hanning(16).astype(np.float32)
W15 = np.hanning(15).astype(np.float32)

BAD_OPERANDS = [
    ("wrong M", _z((2, 5, 16)), np.ones((2, 4, 16), np.float32)),
    ("last axis neither K nor K/2 + 1", _z((2, 5, 16)), np.ones((2, 5, 8), np.float32)),
    ("last axis neither K nor K/2 + 1 (complex)", _z((2, 5, 16)), _z((2, 5, 10))),
    ("one-sided complex", _z((2, 5, 16)), _z((2, 5, 9))),
    ("one-sided with odd K", _z((2, 5, 15)), np.ones((2, 5, 8), np.float32)),
    ("Bz, Bm > 1 and different", _z((2, 5, 16)), np.ones((3, 5, 16), np.float32)),
    ("Bz, Bm > 1 and different (nested leading axes)", _z((2, 3, 5, 16)), np.ones((4, 5, 16), np.float32)),
    ("host spectrum, device mask", _z((2, 5, 16)), FakeDevice((2, 5, 16), np.float32)),
    ("device spectrum, host mask", FakeDevice((2, 5, 16), np.complex64), np.ones((2, 5, 16), np.float32)),
    ("c128 spectrum", np.zeros((2, 5, 16), np.complex128), np.ones((2, 5, 16), np.float32)),
    ("f64 mask", _z((2, 5, 16)), np.ones((2, 5, 16), np.float64)),
    ("c128 mask", _z((2, 5, 16)), np.zeros((2, 5, 16), np.complex128)),
    ("rank-1 mask", _z((5, 16)), np.ones(16, np.float32)),
    ("device spectrum that is not c64", FakeDevice((2, 5, 16), np.float32), FakeDevice((2, 5, 16), np.float32)),
]


@pytest.mark.parametrize("what,z,mask", BAD_OPERANDS, ids=[b[0] for b in BAD_OPERANDS])
def test_bad_operands_raise_before_any_context(no_context, what, z, mask):
    w = W15 if what == "one-sided with odd K" else W
    with pytest.raises(S.ArgumentError):
        S.istft_masked(z, mask, w)
    with pytest.raises(S.ArgumentError):
        S.spectrum_mask(z, mask)


def test_bad_options_raise_before_any_context(no_context):
    z, m = _z((2, 5, 16)), np.ones((2, 5, 16), np.float32)
    with pytest.raises(S.ArgumentError, match="unknown keys"):
        S.istft_masked(z, m, W, window_padding="valid")
    with pytest.raises(S.ArgumentError, match="sampling_rate is mandatory"):
        S.istft_masked(z, m, W, scaling="psd", sampling_rate=None)
    with pytest.raises(S.ArgumentError, match="invalid :scaling"):
        S.istft_masked(z, m, W, scaling="density")
    with pytest.raises(S.ArgumentError, match="overlap_length must be a number less than the window size"):
        S.istft_masked(z, m, W, overlap_length=16)
    with pytest.raises(S.ArgumentError):   # an f64 window belongs to the f64 tier
        S.istft_masked(z, m, W.astype(np.float64))
    with pytest.raises(S.ArgumentError):   # fft_length must equal the window length
        S.istft_masked(z, m, np.hanning(12).astype(np.float32))
    with pytest.raises(S.ArgumentError):
        S.istft_masked(z, m, W, fft_length=-3)


def test_the_neighbours_keep_their_errors(no_context):
    """spectrum_multiply and istft_filtered still take a rank-1 h only"""
    z = _z((2, 5, 16))
    with pytest.raises(S.ArgumentError, match="rank-1"):
        S.spectrum_multiply(z, _z((5, 16)))
    with pytest.raises(S.ArgumentError, match="rank-1"):
        S.istft_filtered(z, _z((5, 16)), W)
