"""Spectral estimation (extension: the reference has no spectral estimator): Welch's averaged periodogram, the cross spectral density
and the magnitude-squared coherence of real f32 rows — scipy.signal.welch / csd / coherence with return_onesided=True and
average="mean", options spelled as in stft (include/nxsig.h: nxsig_welch_f32, nxsig_csd_f32)."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, ptr, rows_last, validate
from .device import DeviceBuffer

_KEYS = ("overlap_length", "fft_length", "sampling_rate", "detrend", "scaling", "average")
_SCALINGS = {"density": 0, "spectrum": 1}


def _parse(fn, n, opts):
    """(hop, fft_length, sampling_rate, detrend, scaling) of the validated options"""
    validate(opts, _KEYS, fn)
    overlap = opts.get("overlap_length", n // 2)
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)) or not 0 <= overlap < n:
        raise ArgumentError(f"{fn}: overlap_length must be an integer in [0, {n}), got: {overlap!r}")
    k = opts.get("fft_length", n)
    if k == "power_of_two":
        k = 1 << max(0, (n - 1).bit_length())
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < n:
        raise ArgumentError(f"{fn}: fft_length must be an integer >= the window length {n} or \"power_of_two\", got: {k!r}")
    fs = opts.get("sampling_rate", 1.0)
    if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)) or not 0 < float(fs) < float("inf"):
        raise ArgumentError(f"{fn}: sampling_rate must be a positive number, got: {fs!r}")
    detrend = opts.get("detrend", "constant")
    if detrend == "linear":
        raise ArgumentError(f"{fn}: detrend \"linear\" is unsupported, only \"constant\" and False are built")
    if not (detrend == "constant" or detrend is False):
        raise ArgumentError(f"{fn}: detrend must be \"constant\" or False, got: {detrend!r}")
    scaling = opts.get("scaling", "density")
    if not isinstance(scaling, str) or scaling not in _SCALINGS:
        raise ArgumentError(f"{fn}: scaling must be \"density\" or \"spectrum\", got: {scaling!r}")
    average = opts.get("average", "mean")
    if average != "mean":
        raise ArgumentError(f"{fn}: average {average!r} is unsupported, only \"mean\" is built")
    return n - int(overlap), int(k), float(fs), int(detrend == "constant"), _SCALINGS[scaling]


def _real_f32(fn, t) -> Operand:
    """a real f32 input with at least one axis and no empty one; a host array is made contiguous"""
    x = Operand(t)
    if x.dtype != np.float32:
        raise NxSignalUnsupported(f"{fn}: real f32 tensors are built, got {x.dtype}")
    x.shape = tuple(int(s) for s in x.shape)
    if len(x.shape) < 1 or any(s < 1 for s in x.shape):
        raise ArgumentError(f"{fn}: the tensor must have at least one axis and no empty dimension")
    return x.cast()


def _window(fn, window):
    w = np.ascontiguousarray(np.asarray(window), dtype=np.float32)
    if w.ndim != 1 or w.shape[0] < 1:
        raise ArgumentError(f"{fn}: the window must be a 1-D tensor of at least one sample")
    return w


def frequencies(fft_length, sampling_rate=1.0):
    """k * sampling_rate / fft_length for the bins k of a one-sided estimate, f32 (formed in double, rounded once)"""
    nb = _lib.check(_lib.load().nxsig_welch_bins(int(fft_length)))
    return (np.arange(nb, dtype=np.float64) * float(sampling_rate) / float(fft_length)).astype(np.float32)


def _estimate(fn, x, y, window, ctx, want_auto, opts):
    w = _window(fn, window)
    n = int(w.shape[0])
    hop, k, fs, detrend, scaling = _parse(fn, n, opts)
    x = _real_f32(fn, x)
    shape = x.shape
    if y is not None:
        y = _real_f32(fn, y)
        if y.shape != shape:
            raise ArgumentError(f"{fn}: x and y must have the same shape, got {shape} and {y.shape}")
        if x.device != y.device:
            raise ArgumentError(f"{fn}: x and y must both be host tensors or both be device tensors")
    batch, length = rows_last(shape)
    if length < n:
        raise ArgumentError(f"{fn}: the window of length {n} does not fit rows of length {length}")
    if batch >= 2 ** 31:
        raise ArgumentError(f"{fn}: 2^31 or more rows")
    lib = _lib.load()
    nb = _lib.check(lib.nxsig_welch_bins(k))
    oshape = shape[:-1] + (nb,)
    c = x.context(ctx, caller_first=False)
    cp = _lib.ctx_ptr(c.handle, _lib._ctx_spectral)
    if y is None:
        pxx = x.result(oshape, np.float32)
        _lib.check(lib.nxsig_welch_f32(cp, x.ptr, length, batch, length, ptr(w), n, hop, k, detrend, scaling, fs, ptr(pxx), x.mem))
        return frequencies(k, fs), pxx
    pxy = x.result(oshape, np.complex64)
    pxx = x.result(oshape, np.float32) if want_auto else None
    pyy = x.result(oshape, np.float32) if want_auto else None
    _lib.check(lib.nxsig_csd_f32(cp, x.ptr, y.ptr, length, batch, length, ptr(w), n, hop, k, detrend, scaling, fs, ptr(pxx), ptr(pyy), ptr(pxy),
                                 x.mem))
    return frequencies(k, fs), pxx, pyy, pxy, c


def welch(x, window, ctx=None, **opts):
    """(f, Pxx): Welch's estimate of the power spectral density (scaling="density", V^2 / Hz) or the power spectrum
    (scaling="spectrum", V^2) of the last axis of real f32 rows.  window: a 1-D tensor of N samples; overlap_length (default N // 2),
    fft_length (an integer >= N or "power_of_two", default N), sampling_rate (1.0), detrend ("constant" or False), scaling, average
    ("mean").  M = (L - N) // hop + 1 frames, no padding, a ragged tail is dropped.  f is f32[fft_length // 2 + 1]; Pxx is f32 of x's
    shape with the last axis replaced by the bins — a numpy array for a host tensor, a DeviceBuffer for a device tensor.  A row with an
    Inf / NaN inside the samples its frames cover is NaN in every bin."""
    return _estimate("welch", x, None, window, ctx, False, opts)


def csd(x, y, window, ctx=None, return_auto=False, **opts):
    """(f, Pxy): the cross spectral density mean_m conj(X_m) Y_m of two real f32 tensors of one shape, c64, options as welch.
    return_auto: (f, Pxy, Pxx, Pyy), the two auto-spectra of the same call.  A row with an Inf / NaN in the covered samples of x OR y is
    NaN in every bin of every result."""
    f, pxx, pyy, pxy, _ = _estimate("csd", x, y, window, ctx, bool(return_auto), opts)
    return (f, pxy, pxx, pyy) if return_auto else (f, pxy)


def coherence(x, y, window, ctx=None, **opts):
    """(f, Cxy): the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy), f32 in [0, 1], from ONE csd call that also returns both
    auto-spectra; the quotient of the fft_length // 2 + 1 numbers per row is formed on the host in double.  One frame gives 1."""
    f, pxx, pyy, pxy, c = _estimate("coherence", x, y, window, ctx, True, opts)
    device = isinstance(pxy, DeviceBuffer)
    if device:
        pxx, pyy, pxy = pxx.numpy(), pyy.numpy(), pxy.numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        num = pxy.real.astype(np.float64) ** 2 + pxy.imag.astype(np.float64) ** 2
        cxy = (num / (pxx.astype(np.float64) * pyy.astype(np.float64))).astype(np.float32)
    return f, (DeviceBuffer.from_numpy(c, cxy) if device else cxy)


# lombscargle lives in a module of its own (_lombscargle.py)
from ._lombscargle import lombscargle  # noqa: E402,F401
