"""Spectral.yin (an extension: the YIN fundamental-frequency estimate per frame, following librosa.yin), on the
kernels of csrc/kernels_yin.hip.  Reached as nx_signal_amd.spectral.yin."""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

MAX_FRAME = 4096


def _integer(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ArgumentError(f"yin: {what} must be an integer, got: {v!r}")
    return int(v)


def _positive(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not v > 0:
        raise ArgumentError(f"yin: {what} must be a positive finite number, got: {v!r}")
    return float(v)


def periods(fmin, fmax, sr, frame_length):
    """(min_period, max_period) in samples: floor(sr / fmax) and min(ceil(sr / fmin), L - L // 2 - 1)"""
    return int(math.floor(sr / fmax)), min(int(math.ceil(sr / fmin)), frame_length - frame_length // 2 - 1)


def yin(x, fmin, fmax, sr=22050, frame_length=2048, hop=None, *, trough_threshold=0.1, center=True, return_voicing=False,
        return_cmnd=False, ctx=None):
    """The YIN estimate of the fundamental frequency of every frame of every row, on the GPU, following librosa.yin (0.10): the difference
    function over a window of frame_length // 2 samples, its cumulative mean normalisation c, the first trough of c under
    trough_threshold (else the global minimum), a three-point parabolic shift, f0 = sr / period.  x: f32 host array or device tensor of
    rank >= 1, time on the last axis.  Lags run from min_period = floor(sr / fmax) to max_period = min(ceil(sr / fmin), frame_length -
    frame_length // 2 - 1).  center=True extends each row by frame_length // 2 zeros on both sides (pad_mode="constant"; the padded row is
    never written); frames start at multiples of hop (default frame_length // 4; hop may exceed frame_length).  Returns f0 = f32[..., F];
    return_voicing appends v = f32[..., F], the value of c at the chosen lag (small = voiced); return_cmnd appends c itself, f32[...,
    F, max_period - min_period + 1]; with either flag the result is a tuple.  Every sum is direct and in double (include/nxsig.h states
    the definition), where librosa uses a single-precision FFT autocorrelation and zeroes |acf| and |energy| below 1e-6: this follows
    librosa, it does not reproduce its rounding.  A frame whose used samples hold an Inf / NaN gets NaN in every output; every other
    frame keeps its bits.  Frames of up to 4096 samples are built; f64 rows are unsupported.  A host array gives numpy arrays; a device
    tensor DeviceBuffers, and the call does not wait."""
    L = _integer(frame_length, "frame_length")
    h = max(L // 4, 1) if hop is None else _integer(hop, "hop")
    lo, hi, rate = _positive(fmin, "fmin"), _positive(fmax, "fmax"), _positive(sr, "sr")
    thr = _positive(trough_threshold, "trough_threshold")
    if not lo < hi:
        raise ArgumentError(f"yin: fmin must be < fmax, got: {fmin!r}, {fmax!r}")
    if not isinstance(center, (bool, np.bool_)):
        raise ArgumentError(f"yin: center must be a boolean, got: {center!r}")
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype == np.dtype(np.float64):
        raise NxSignalUnsupported("yin: unsupported type float64: f32 rows are built")
    if xo.dtype != np.dtype(np.float32):
        raise ArgumentError(f"yin: expected real f32 rows, got {xo.dtype}")
    if len(xo.shape) < 1:
        raise ArgumentError("yin: expected a tensor of rank >= 1")
    xo.cast()
    batch, n = rows_last(xo.shape)
    if L < 4:
        raise ArgumentError(f"yin: frame_length must be >= 4, got: {L}")
    if h < 1:
        raise ArgumentError(f"yin: hop must be >= 1, got: {h}")
    if not center and L > n:
        raise ArgumentError(f"yin: frame_length must be <= the row length ({n}) without center, got: {L}")
    pmin, pmax = periods(lo, hi, rate, L)
    if pmin < 1:
        raise ArgumentError(f"yin: fmax must be <= sr: min_period = floor(sr / fmax) must be >= 1, got: {pmin}")
    if pmax <= pmin:
        raise ArgumentError(f"yin: max_period ({pmax}) must be > min_period ({pmin}): lower fmin, raise fmax or lengthen the frame")
    if L > MAX_FRAME:
        raise NxSignalUnsupported(f"yin: frames of up to {MAX_FRAME} samples are built, got: {L}")
    lib = _lib.load()
    frames = int(lib.nxsig_yin_frames(n, L, h, int(center)))
    if frames < 0:
        _lib.check(frames)
    lead = xo.shape[:-1] + (frames,)
    c = xo.context(ctx, caller_first=False)
    f0 = xo.result(lead, np.float32)
    v = xo.result(lead, np.float32) if return_voicing else None
    cm = xo.result(lead + (pmax - pmin + 1,), np.float32) if return_cmnd else None
    if batch:
        _lib.check(lib.nxsig_yin_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, batch, n, n, L, h, int(center), pmin, pmax, rate, thr,
                                     ptr(f0), ptr(v), ptr(cm), xo.mem))
    out = (f0,) + ((v,) if return_voicing else ()) + ((cm,) if return_cmnd else ())
    return out if len(out) > 1 else f0
