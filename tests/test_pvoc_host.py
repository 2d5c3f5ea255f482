"""Transforms.phase_vocoder / time_stretch: what needs no GPU — the output frame count and the refused arguments."""
import ctypes as C

import numpy as np
import pytest

from nx_signal_amd import ArgumentError, NxSignalUnsupported, _lib, transforms as T


@pytest.mark.parametrize("rate", [0.1, 1 / 3, 0.7, 1.0, 1.3, 3.0, 1e6])
@pytest.mark.parametrize("M", [1, 5, 37, 11247])
def test_frame_count_is_numpy_aranges(M, rate):
    assert _lib.load().nxsig_pvoc_frames(M, rate) == len(np.arange(0, M, rate))


@pytest.mark.parametrize("rate", [0, -1.0, float("nan"), float("inf")])
def test_refused_rates(rate):
    z, lib = np.ones((2, 4, 3), np.complex64), _lib.load()
    with pytest.raises(ArgumentError, match="rate must be"):
        T.phase_vocoder(z, rate)
    with pytest.raises(ArgumentError, match="rate must be"):
        T.time_stretch(np.ones(64, np.float32), rate, np.ones(16, np.float32))
    assert lib.nxsig_pvoc_frames(4, rate) == _lib.ERR_INVALID_ARG
    out = np.empty((2, 4, 3), np.complex64)   # the checks come ahead of the context: a null one is never looked at
    assert lib.nxsig_phase_vocoder_c64(None, z.ctypes.data_as(C.c_void_p), 2, 4, 3, rate, out.ctypes.data_as(C.c_void_p), _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "rate must be" in _lib.last_error()


def test_refused_operands():
    with pytest.raises(ArgumentError, match="shape"):
        T.phase_vocoder(np.ones(8, np.complex64), 1.0)
    with pytest.raises(ArgumentError, match="complex64"):
        T.phase_vocoder(np.ones((4, 8), np.float32), 1.0)
    with pytest.raises(NxSignalUnsupported, match="complex128"):
        T.phase_vocoder(np.ones((4, 8), np.complex128), 1.0)
    z, lib = np.ones((4, 8), np.complex64), _lib.load()
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.nxsig_pvoc_frames(0, 1.0) == _lib.ERR_INVALID_ARG and lib.nxsig_pvoc_frames(4, 1e-300) == _lib.ERR_UNSUPPORTED
    for batch, frames, bins in [(-1, 4, 8), (1, 0, 8), (1, 4, 0)]:
        assert lib.nxsig_phase_vocoder_c64(None, p, batch, frames, bins, 1.0, p, _lib.HOST) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_phase_vocoder_c64(None, p, 1, 4, 8, 1.0, p, _lib.HOST) == _lib.ERR_INVALID_ARG and "overlap" in _lib.last_error()
