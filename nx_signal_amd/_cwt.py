"""Transforms.cwt / morlet2 / ricker and Filters.fir_bank (extensions: scipy.signal's continuous wavelet transform as SciPy <= 1.14 had
it, and the filter bank it is one instance of), on the kernels of csrc/kernels_cwt.hip.  Reached as
nx_signal_amd.transforms.cwt, morlet2, ricker and nx_signal_amd.filters.fir_bank."""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

# NXSIG_CWT_* of include/nxsig.h
_OUTPUTS = {"complex": 0, "real": 1, "magnitude": 2, "power": 3}
_WAVELETS = {"morlet2": 0, "ricker": 1}
_MAX_BATCH, _MAX_FILTERS, _MAX_EXTENT = 65535, 4096, 1 << 24


def _count(M, fn):
    if isinstance(M, (bool, np.bool_)) or not isinstance(M, numbers.Integral) or M < 1:
        raise ArgumentError(f"{fn}: the number of points must be a positive integer, got: {M!r}")
    return int(M)


def _positive(v, what, fn):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.number)) or not math.isfinite(v) or not v > 0:
        raise ArgumentError(f"{fn}: {what} must be positive and finite, got: {v!r}")
    return float(v)


def morlet2(M, s, w=5.0):
    """scipy.signal.morlet2(M, s, w) of SciPy <= 1.14: sqrt(1 / s) pi^(-1/4) exp(i w t) exp(-t^2 / 2) at t = (arange(M) - (M - 1) / 2) / s,
    complex128.  Host only."""
    M, s = _count(M, "morlet2"), _positive(s, "s", "morlet2")
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (numbers.Real, np.number)) or not math.isfinite(w):
        raise ArgumentError(f"morlet2: w must be finite, got: {w!r}")
    t = (np.arange(0, M) - (M - 1.0) / 2) / s
    return np.sqrt(1 / s) * np.pi ** (-0.25) * np.exp(1j * float(w) * t) * np.exp(-0.5 * t ** 2)


def ricker(M, a):
    """scipy.signal.ricker(M, a) of SciPy <= 1.14: 2 / (sqrt(3 a) pi^(1/4)) (1 - v^2 / a^2) exp(-v^2 / (2 a^2)) at v = arange(M) - (M - 1) / 2,
    float64.  Host only."""
    M, a = _count(M, "ricker"), _positive(a, "a", "ricker")
    v = np.arange(0, M) - (M - 1.0) / 2
    return 2 / (np.sqrt(3 * a) * np.pi ** 0.25) * (1 - v ** 2 / a ** 2) * np.exp(-v ** 2 / (2 * a ** 2))


def _support(width, length):
    """N = min(ceil(10 a), L), as nxsig_cwt_support"""
    n = math.ceil(10.0 * width)
    return length if not n < length else max(int(n), 1)


def _rows(fn, x, axis):
    """the operand with the axis last, every argument error of the tensor raised"""
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype.kind == "c":
        raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 rows are built")
    if xo.dtype != np.dtype(np.float32):
        if xo.dtype == np.dtype(np.float64):
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 rows are built")
        if xo.device:
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: device tensors must be f32")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32)
    rank = len(xo.shape)
    if rank < 1:
        raise ArgumentError(f"{fn}: the tensor must have at least one axis")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -rank <= axis < rank:
        raise ArgumentError(f"{fn}: axis {axis!r} is out of bounds for a tensor of rank {rank}")
    from .filters import _axis_last   # here, not at the top: the package imports either module first
    _axis_last(xo, axis, fn, NxSignalUnsupported(f"{fn}: unsupported axis: device tensors are transformed along their last axis only"))
    batch, length = rows_last(xo.shape)
    if length < 1:
        raise ArgumentError(f"{fn}: the axis must hold at least one sample")
    if not 1 <= batch <= _MAX_BATCH:
        raise NxSignalUnsupported(f"{fn}: unsupported batch: 1 to {_MAX_BATCH} rows are built, got {batch}")
    return xo, batch, length


def _output(output, fn, default):
    if output is None:
        return default
    if not isinstance(output, str) or output not in _OUTPUTS:
        raise ArgumentError(f"{fn}: output must be 'complex', 'real', 'magnitude' or 'power', got: {output!r}")
    return output


def _bank(fn, taps, length=None):
    """a list of 1-D tap arrays as (one f32 or c64 array, int64 counts, any complex); with `length` the extent limit is checked too"""
    if isinstance(taps, np.ndarray) and taps.ndim == 1 and taps.dtype != object:
        taps = [taps]
    try:
        hs = [np.asarray(h) for h in taps]
    except (TypeError, ValueError):
        raise ArgumentError(f"{fn}: taps must be a list of 1-D arrays") from None
    if not 1 <= len(hs) <= _MAX_FILTERS:
        raise ArgumentError(f"{fn}: 1 to {_MAX_FILTERS} filters are taken, got {len(hs)}")
    for h in hs:
        if h.ndim != 1 or h.dtype.kind not in "biufc":
            raise ArgumentError(f"{fn}: every filter must be a 1-D numeric array, got shape {h.shape}, type {h.dtype}")
        if h.size < 1:
            raise ArgumentError(f"{fn}: every filter must hold at least one tap")
    longest = max(h.size for h in hs)
    if length is not None and length + longest - 1 > _MAX_EXTENT:
        raise NxSignalUnsupported(f"{fn}: unsupported size: length + max taps - 1 must be at most 2^24, got {length + longest - 1}")
    cplx = any(h.dtype.kind == "c" for h in hs)
    flat = np.ascontiguousarray(np.concatenate(hs).astype(np.complex64 if cplx else np.float32))
    if not np.all(np.isfinite(flat)):
        raise ArgumentError(f"{fn}: the taps must be finite")
    return flat, np.array([h.size for h in hs], np.int64), cplx


def _run_bank(fn, xo, batch, length, flat, counts, cplx, output, ctx):
    c = xo.context(ctx, caller_first=False)
    S = int(counts.size)
    out = xo.result(xo.shape[:-1] + (S, length), np.complex64 if output == "complex" else np.float32)
    _lib.check(_lib.load().nxsig_fir_bank(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, length, batch, length, ptr(flat), int(cplx),
                                          counts.ctypes.data_as(C.POINTER(C.c_int64)), S, _OUTPUTS[output], ptr(out), xo.mem))
    return out


def fir_bank(x, taps, output="complex", ctx=None, axis=-1):
    """A bank of FIR filters on the GPU: out[..., s, :] = convolve(line, taps[s]) in "same" alignment, out[n] = full[n + (N_s - 1) // 2],
    for every line of x along `axis` (include/nxsig.h states the definition).  taps: a list of 1-D arrays of any lengths, all real or any
    complex.  Every block of a line is transformed once for the whole bank.  output: "complex" (c64), "real", "magnitude" or "power" (f32;
    the sink is fused, so a scalogram never passes through a complex tensor).  The result is [..., S, L] with the filtered axis moved last.
    Real f32 tensors; host integer and narrower float arrays are computed as f32; f64 rows are unsupported.  A device tensor: the last axis
    only, a DeviceBuffer out, and the call does not wait.  A line that holds an Inf / NaN has no finite output at any filter."""
    fn = "fir_bank"
    output = _output(output, fn, "complex")
    xo, batch, length = _rows(fn, x, axis)
    flat, counts, cplx = _bank(fn, taps, length)
    return _run_bank(fn, xo, batch, length, flat, counts, cplx, output, ctx)


def cwt(x, widths, wavelet="morlet2", w=5.0, output=None, ctx=None, axis=-1):
    """scipy.signal.cwt(x, wavelet, widths) of SciPy <= 1.14 on the GPU, for every line of x along `axis`: per width a the line is
    convolved ("same") with conj(wavelet(N, a))[::-1], N = min(ceil(10 a), L) (include/nxsig.h states the definition).  wavelet: "morlet2"
    (with w), "ricker", or a callable (N, width) -> array evaluated on the host and sent through the bank.  output: "complex", "real",
    "magnitude" or "power"; None means "real" for ricker and "complex" otherwise.  The result is [..., S, L] with the transformed axis moved
    last.  Operands as fir_bank's."""
    fn = "cwt"
    try:
        ws = np.atleast_1d(np.asarray(widths, dtype=np.float64))
    except (TypeError, ValueError):
        raise ArgumentError(f"{fn}: widths must be real numbers, got: {widths!r}") from None
    if ws.ndim != 1 or not 1 <= ws.size <= _MAX_FILTERS:
        raise ArgumentError(f"{fn}: widths must be a 1-D sequence of 1 to {_MAX_FILTERS} numbers, got shape {ws.shape}")
    if not np.all(np.isfinite(ws)) or not np.all(ws > 0):
        raise ArgumentError(f"{fn}: every width must be positive and finite, got: {widths!r}")
    named = isinstance(wavelet, str)
    if named and wavelet not in _WAVELETS:
        raise ArgumentError(f"{fn}: wavelet must be 'morlet2', 'ricker' or a callable, got: {wavelet!r}")
    if not named and not callable(wavelet):
        raise ArgumentError(f"{fn}: wavelet must be 'morlet2', 'ricker' or a callable, got: {wavelet!r}")
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (numbers.Real, np.number)) or not math.isfinite(w):
        raise ArgumentError(f"{fn}: w must be finite, got: {w!r}")
    output = _output(output, fn, "real" if wavelet == "ricker" else "complex")
    xo, batch, length = _rows(fn, x, axis)
    if not named:
        hs = [np.conj(np.asarray(wavelet(_support(a, length), a)))[::-1] for a in ws]
        flat, counts, cplx = _bank(fn, hs, length)
        return _run_bank(fn, xo, batch, length, flat, counts, cplx, output, ctx)
    if length + _support(float(ws.max()), length) - 1 > _MAX_EXTENT:
        raise NxSignalUnsupported(f"{fn}: unsupported size: length + max taps - 1 must be at most 2^24")
    c = xo.context(ctx, caller_first=False)
    ws = np.ascontiguousarray(ws)
    out = xo.result(xo.shape[:-1] + (int(ws.size), length), np.complex64 if output == "complex" else np.float32)
    _lib.check(_lib.load().nxsig_cwt(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, length, batch, length, _WAVELETS[wavelet],
                                     ws.ctypes.data_as(C.POINTER(C.c_double)), int(ws.size), float(w), _OUTPUTS[output], ptr(out), xo.mem))
    return out
