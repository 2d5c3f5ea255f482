"""Spectral.yin without a GPU: the frame count, the refusals through Python and through the C entry, the wrapper's period arithmetic."""
import ctypes as C
import itertools

import numpy as np
import pytest

from nx_signal_amd import ArgumentError, NxSignalUnsupported, _lib, _yin, spectral


@pytest.mark.parametrize("n,L,hop,center", itertools.product([1000, 1001, 4097], [4, 17, 1000], [1, 3, 64, 1300], [0, 1]))
def test_frame_count(n, L, hop, center):
    assert _lib.load().nxsig_yin_frames(n, L, hop, center) == 1 + (n + (2 * (L // 2) if center else 0) - L) // hop


def c_entry(n=100, stride=None, L=64, hop=16, center=0, pmin=2, pmax=31, sr=16000.0, thr=0.1):
    """nxsig_yin_f32 with a null context: the checks come ahead of it, so it is never looked at"""
    x, f0 = np.ones(max(n, 1), np.float32), np.empty(4096, np.float32)
    return _lib.load().nxsig_yin_f32(None, x.ctypes.data_as(C.c_void_p), 1, n, n if stride is None else stride, L, hop, center, pmin, pmax,
                                     sr, thr, f0.ctypes.data_as(C.c_void_p), None, None, _lib.HOST)


@pytest.mark.parametrize("kwargs,what", [
    (dict(L=3, pmin=1, pmax=2), "frame_length must be >= 4"),
    (dict(hop=0), "hop must be >= 1"),
    (dict(L=101, pmax=50), "frame_length must be <= n without center"),
    (dict(stride=99), "batch_stride must be >= n"),
    (dict(pmin=0), "min_period must be >= 1"),
    (dict(pmin=31), "max_period must be > min_period"),
    (dict(pmax=32), "max_period must be <= frame_length - frame_length / 2 - 1"),
    (dict(sr=0.0), "sr must be finite and positive"),
    (dict(thr=float("nan")), "threshold must be finite and positive"),
    (dict(center=2), "center must be 0 or 1"),
])
def test_refused_by_the_c_entry(kwargs, what):
    assert c_entry(**kwargs) == _lib.ERR_INVALID_ARG and what in _lib.last_error()


def test_the_c_entry_accepts_the_limits_up_to_the_context():
    for ok in (dict(L=65, pmax=32), dict(L=64, n=10, center=1), dict(L=5, pmin=1, pmax=2)):   # every check passes: the null context is refused
        assert c_entry(**ok) == _lib.ERR_INVALID_ARG and "null context" in _lib.last_error()
    lib = _lib.load()
    assert c_entry(n=5000, L=4097, pmax=2048) == _lib.ERR_UNSUPPORTED and "frames of up to 4096 samples are built" in _lib.last_error()
    assert lib.nxsig_yin_frames(10, 11, 1, 0) == _lib.ERR_INVALID_ARG and lib.nxsig_yin_frames(10, 11, 1, 1) == 10
    assert lib.nxsig_yin_frames(10, 4, 0, 0) == _lib.ERR_INVALID_ARG and lib.nxsig_yin_frames(10, 4, 1, 3) == _lib.ERR_INVALID_ARG
    x = np.ones(100, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.nxsig_yin_f32(None, x, 1, 100, 100, 64, 16, 0, 2, 31, 16000.0, 0.1, None, x, None, _lib.HOST) == _lib.ERR_INVALID_ARG
    assert "null pointer" in _lib.last_error()


@pytest.mark.parametrize("kwargs,what", [
    (dict(frame_length=3), "frame_length must be >= 4"),
    (dict(hop=0), "hop must be >= 1"),
    (dict(frame_length=512, center=False), "frame_length must be <="),
    (dict(fmax=20000), "min_period"),
    (dict(frame_length=16), "max_period"),
    (dict(fmin=2000, fmax=50), "fmin must be < fmax"),
    (dict(fmin=0), "fmin must be a positive finite number"),
    (dict(sr=float("nan")), "sr must be a positive finite number"),
    (dict(trough_threshold=0), "trough_threshold must be a positive finite number"),
    (dict(frame_length=64.0), "must be an integer"),
    (dict(center=1), "center must be a boolean"),
])
def test_refused_by_python(kwargs, what):
    args = dict(fmin=50, fmax=2000, sr=16000, frame_length=64)
    args.update(kwargs)
    with pytest.raises(ArgumentError, match=what):
        spectral.yin(np.ones(400, np.float32), **args)


def test_refused_operands():
    with pytest.raises(NxSignalUnsupported, match="float64"):
        spectral.yin(np.ones(400), 50, 2000, 16000, 64)
    for dtype in (np.complex64, np.int32):
        with pytest.raises(ArgumentError, match="f32"):
            spectral.yin(np.ones(400, dtype), 50, 2000, 16000, 64)
    with pytest.raises(NxSignalUnsupported, match="frames of up to 4096 samples are built"):
        spectral.yin(np.ones(9000, np.float32), 50, 2000, 16000, 4098)


def test_period_arithmetic():
    assert _yin.periods(50, 2000, 16000, 512) == (8, 255)      # ceil(16000 / 50) = 320 is cut to 512 - 256 - 1
    assert _yin.periods(50, 2000, 16000, 1024) == (8, 320)
    assert _yin.periods(65, 2093, 48000, 2048) == (22, 739) and _yin.periods(200, 2000, 48000, 2048) == (24, 240)
    assert _yin.periods(70, 3000, 22050, 513) == (7, 256)      # an odd frame: 513 - 256 - 1
