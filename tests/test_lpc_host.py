"""Spectral.lpc: what needs no GPU — the frame count and the refused arguments, through Python and through the C entry."""
import ctypes as C

import numpy as np
import pytest

from nx_signal_amd import ArgumentError, NxSignalUnsupported, _lib, spectral


@pytest.mark.parametrize("hop", [1, 3, 64, 1300])
@pytest.mark.parametrize("L", [2, 17, 1000])
@pytest.mark.parametrize("n", [1000, 1001, 4097])
def test_frame_count_is_librosas(n, L, hop):
    assert _lib.load().nxsig_lpc_frames(n, L, hop) == 1 + (n - L) // hop


def c_entry(x, L, hop, order, n=None, stride=None):
    """nxsig_lpc_f32 with a null context: the checks come ahead of it, so it is never looked at"""
    n = x.shape[-1] if n is None else n
    a = np.empty(4096, np.float32)
    return _lib.load().nxsig_lpc_f32(None, x.ctypes.data_as(C.c_void_p), 1, n, n if stride is None else stride, L, hop, order,
                                     a.ctypes.data_as(C.c_void_p), None, None, _lib.HOST)


@pytest.mark.parametrize("kwargs,what", [
    (dict(order=0), "order must be >= 1"),
    (dict(order=64, frame_length=64), "order must be < frame_length"),
    (dict(order=8, frame_length=64, hop=0), "hop must be >= 1"),
    (dict(order=8, frame_length=101), "frame_length must be <="),
])
def test_refused_values(kwargs, what):
    x = np.ones(100, np.float32)
    with pytest.raises(ArgumentError, match=what):
        spectral.lpc(x, **kwargs)
    L = kwargs.get("frame_length", 100)
    assert c_entry(x, L, kwargs.get("hop", 25), kwargs["order"]) == _lib.ERR_INVALID_ARG
    assert what in _lib.last_error()


def test_refused_operands():
    x = np.ones(400, np.float32)
    for bad in (dict(order=2.0), dict(order=True), dict(order=2, frame_length=8.0), dict(order=2, frame_length=8, hop="2")):
        with pytest.raises(ArgumentError, match="must be an integer"):
            spectral.lpc(x, **bad)
    with pytest.raises(NxSignalUnsupported, match="float64"):
        spectral.lpc(np.ones(400), 2)
    for dtype in (np.complex64, np.int32):
        with pytest.raises(ArgumentError, match="f32"):
            spectral.lpc(np.ones(400, dtype), 2)
    with pytest.raises(NxSignalUnsupported, match="orders up to 128 are built"):
        spectral.lpc(x, 129)
    assert c_entry(x, 400, 100, 129) == _lib.ERR_UNSUPPORTED and "orders up to 128 are built" in _lib.last_error()
    assert c_entry(x, 100, 25, 8, n=200, stride=199) == _lib.ERR_INVALID_ARG and "batch_stride" in _lib.last_error()
    lib = _lib.load()
    assert lib.nxsig_lpc_frames(10, 11, 1) == _lib.ERR_INVALID_ARG and lib.nxsig_lpc_frames(10, 4, 0) == _lib.ERR_INVALID_ARG
    assert lib.nxsig_lpc_f32(None, None, 1, 10, 10, 10, 2, 2, None, None, None, _lib.HOST) == _lib.ERR_INVALID_ARG
