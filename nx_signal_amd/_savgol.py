"""Filters.savgol_filter and savgol_coeffs (an extension: scipy.signal 1.15's Savitzky-Golay filter), on the
kernels of csrc/kernels_savgol.hip.  Both are reached as nx_signal_amd.filters.savgol_filter / .savgol_coeffs."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last, validate

# nxsig_savgol_mode / nxsig_savgol_use of include/nxsig.h
_MODES = {"mirror": 0, "constant": 1, "nearest": 2, "wrap": 3, "interp": 4}
_USES = {"conv": 0, "dot": 1}
_MAX_WINDOW, _MAX_ORDER = 1025, 15
_FILTER_KEYS = ("deriv", "delta", "axis", "mode", "cval", "ctx")
_COEFFS_KEYS = ("deriv", "delta", "pos", "use")


def _integer(v, what, fn):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ArgumentError(f"{fn}: {what} must be an integer, got: {v!r}")
    return int(v)


def _real(v, what, fn):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ArgumentError(f"{fn}: {what} must be a number, got: {v!r}")
    return float(v)


def _design(window_length, polyorder, deriv, delta, fn):
    """(W, p, deriv, delta), checked in scipy's order and words where scipy has them"""
    w, p, d = _integer(window_length, "window_length", fn), _integer(polyorder, "polyorder", fn), _integer(deriv, "deriv", fn)
    if w < 1:
        raise ArgumentError(f"{fn}: window_length must be a positive integer")
    if p < 0:
        raise ArgumentError(f"{fn}: polyorder must be a nonnegative integer")
    if p >= w:
        raise ArgumentError(f"{fn}: polyorder must be less than window_length.")
    if d < 0:
        raise ArgumentError(f"{fn}: deriv must be a nonnegative integer")
    dl = _real(delta, "delta", fn)
    if not math.isfinite(dl) or dl == 0.0:
        raise ArgumentError(f"{fn}: delta must be finite and non-zero")
    if w > _MAX_WINDOW:
        raise NxSignalUnsupported(f"{fn}: windows of up to {_MAX_WINDOW} samples are built, got {w}")
    if p > _MAX_ORDER:
        raise NxSignalUnsupported(f"{fn}: polynomials of up to degree {_MAX_ORDER} are built, got {p}")
    return w, p, d, dl


def savgol_coeffs(window_length, polyorder, deriv=0, delta=1.0, pos=None, use="conv", **opts):
    """scipy.signal.savgol_coeffs(window_length, polyorder, deriv=0, delta=1.0, pos=None, use="conv"): the f64 weights of a
    Savitzky-Golay filter.  THE EXACT LEAST-SQUARES WEIGHTS ROUNDED TO DOUBLE, NOT SCIPY'S: within 1e-12 of the rational solution at
    every window length up to 1025, where scipy's lstsq loses digits.  At the default pos (the centre) the
    weights are exactly symmetric (even deriv) or antisymmetric (odd deriv); deriv > polyorder gives zeros."""
    fn = "savgol_coeffs"
    validate(opts, _COEFFS_KEYS, fn)
    w, p, d, dl = _design(window_length, polyorder, deriv, delta, fn)
    at = -1.0
    if pos is not None:
        at = _real(pos, "pos", fn)
        if not 0 <= at < w:
            raise ArgumentError(f"{fn}: pos must be nonnegative and less than window_length.")
    if not isinstance(use, str) or use not in _USES:
        raise ArgumentError(f"{fn}: `use` must be 'conv' or 'dot'.")
    out = np.empty(w, np.float64)
    _lib.check(_lib.load().nxsig_savgol_coeffs(w, p, d, dl, at, _USES[use], out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def savgol_filter(x, window_length, polyorder, deriv=0, delta=1.0, axis=-1, mode="interp", cval=0.0, ctx=None, **opts):
    """scipy.signal.savgol_filter(x, window_length, polyorder, deriv=0, delta=1.0, axis=-1, mode="interp", cval=0.0) on the GPU:
    y[i] = sum_j k[j] ext(i - L + j) with the weights of savgol_coeffs(..., use="dot") and the row extended by `mode` ("mirror",
    "constant", "nearest", "wrap"), or — "interp", the default — the first and last window_length // 2 outputs taken from the polynomial
    fitted to the first / last window_length samples (include/nxsig.h states the definition).  Real f32 and f64 tensors, f32 in f32 out
    and f64 in f64 out, the sums in double either way; host integer arrays are computed as f64.  Host arrays: any axis, numpy out; a
    device tensor: the last axis only, a DeviceBuffer out, and the call does not wait.  An output is non-finite exactly when its
    (extended) window covers an Inf / NaN sample."""
    fn = "savgol_filter"
    validate(opts, _FILTER_KEYS, fn)
    w, p, d, dl = _design(window_length, polyorder, deriv, delta, fn)
    if not isinstance(mode, str) or mode not in _MODES:
        raise ArgumentError(f"{fn}: mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'.")
    cval = _real(cval, "cval", fn)
    if not math.isfinite(cval):
        raise ArgumentError(f"{fn}: cval must be finite")
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype.kind == "c":
        raise NxSignalUnsupported(f"{fn}: real f32 and f64 tensors are built, got {xo.dtype}")
    if xo.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        if xo.device:
            raise NxSignalUnsupported(f"{fn}: device tensors must be f32 or f64, got {xo.dtype}")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32 if xo.dtype.kind == "f" and xo.dtype.itemsize < 4 else np.float64)
    from .filters import _axis_last   # here, not at the top: filters imports this module, and either may be imported first
    axis = _axis_last(xo, axis, fn, NxSignalUnsupported(f"{fn}: device tensors are filtered along their last axis only"))
    batch, n = rows_last(xo.shape)
    if mode == "interp" and w > n:
        raise ArgumentError(f"{fn}: If mode is 'interp', window_length must be less than or equal to the size of x.")
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape, xo.dtype)
    _lib.check(_lib.load().nxsig_savgol_filter(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, int(xo.dtype == np.float64), n, batch, n, w, p, d,
                                               dl, _MODES[mode], cval, ptr(out), xo.mem))
    return out if xo.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))
