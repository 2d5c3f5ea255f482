"""Spectral.lombscargle (an extension: scipy.signal 1.15's generalised Lomb-Scargle periodogram), on the kernels
of csrc/kernels_lombscargle.hip.  Reached as nx_signal_amd.spectral.lombscargle."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

_NORMALIZES = {"power": 0, "normalize": 1, "amplitude": 2}
_LENGTHS = "lombscargle: Parameters x, y, weights must be 1-D arrays of equal non-zero length!"
_WEIGHTS = "lombscargle: Parameter weights must have only non-negative entries which sum to a positive value!"


def _host_f64(v, what):
    """a host operand (times, frequencies, weights) as a C-contiguous f64 array of whatever rank it has"""
    try:
        a = np.asarray(v)
        if a.dtype.kind not in "fiub":
            raise TypeError
        return np.ascontiguousarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ArgumentError(f"lombscargle: {what} must be a real host array") from None


def _flag(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ArgumentError(f"lombscargle: {what} must be True or False, got: {v!r}")
    return int(bool(v))


def lombscargle(x, y, freqs, precenter=False, normalize=False, *, weights=None, floating_mean=False, ctx=None):
    """scipy.signal.lombscargle(x, y, freqs, precenter, normalize, weights=, floating_mean=) of SciPy 1.15 on the GPU, batched over rows
    that share one time base: x the sample times (n,), freqs the ANGULAR frequencies (F,), weights None or (n,) — host arrays, taken as
    f64 and finite — and y a real f32 or f64 tensor [..., n], a host array or a DeviceBuffer.  Returns [..., F]: f32 for f32 rows, f64
    for f64 rows, c64 / c128 under normalize="amplitude"; numpy out for a host tensor, a DeviceBuffer for a device tensor.  normalize is
    False / "power", True / "normalize" or "amplitude" as SciPy's.  Every sum is double on the device.  A row that holds an Inf / NaN is
    NaN at every frequency; the other rows keep their bits.  Host integer rows are computed as f64."""
    xs = _host_f64(x, "x")
    fs = _host_f64(freqs, "freqs")
    ws = None if weights is None else _host_f64(weights, "weights")
    yo = Operand(_as_tensor(y), any_dtype=True)
    if yo.dtype.kind == "c":
        raise NxSignalUnsupported(f"lombscargle: real f32 and f64 rows are built, got {yo.dtype}")
    if yo.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        if yo.device:
            raise NxSignalUnsupported(f"lombscargle: device tensors must be f32 or f64, got {yo.dtype}")
        if yo.dtype.kind not in "biuf":
            raise ArgumentError(f"lombscargle: unsupported type {yo.dtype}")
        yo.cast(np.float32 if yo.dtype.kind == "f" and yo.dtype.itemsize < 4 else np.float64)
    if not (xs.ndim == 1 and xs.size > 0 and len(yo.shape) >= 1 and yo.shape[-1] == xs.shape[0] and (ws is None or ws.shape == xs.shape)):
        raise ArgumentError(_LENGTHS)
    if not (fs.ndim == 1 and fs.size > 0):
        raise ArgumentError("lombscargle: Parameter freqs must be a 1-D array of non-zero length!")
    if not np.isfinite(xs).all():
        raise ArgumentError("lombscargle: x must be finite")
    if not np.isfinite(fs).all():
        raise ArgumentError("lombscargle: freqs must be finite")
    if ws is not None:
        if not np.isfinite(ws).all():
            raise ArgumentError("lombscargle: weights must be finite")
        if not (np.all(ws >= 0) and np.sum(ws) > 0):
            raise ArgumentError(_WEIGHTS)
    if isinstance(normalize, (bool, np.bool_)):
        normalize = "normalize" if normalize else "power"
    if not isinstance(normalize, str) or normalize not in _NORMALIZES:
        raise ArgumentError("lombscargle: Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'.")
    pre, fm = _flag(precenter, "precenter"), _flag(floating_mean, "floating_mean")
    yo.cast()
    batch, n = rows_last(yo.shape)
    f64 = yo.dtype == np.dtype(np.float64)
    if normalize == "amplitude":
        out_dtype = np.complex128 if f64 else np.complex64
    else:
        out_dtype = yo.dtype
    c = yo.context(ctx, caller_first=False)
    out = yo.result(yo.shape[:-1] + (fs.shape[0],), out_dtype)
    if batch:
        _lib.check(_lib.load().nxsig_lombscargle(_lib.ctx_ptr(c.handle, _lib._ctx_iir), yo.ptr, int(f64), n, batch, n, ptr(xs), ptr(fs), fs.shape[0],
                                                 ptr(ws), pre, _NORMALIZES[normalize], fm, ptr(out), yo.mem))
    return out
