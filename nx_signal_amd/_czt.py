"""Transforms.czt / zoom_fft / czt_points (extensions: scipy.signal 1.15's chirp z-transform), on the kernels of
csrc/kernels_czt.hip.  Reached as nx_signal_amd.transforms.czt, zoom_fft and czt_points."""
from __future__ import annotations

import cmath
import math
import numbers

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last


def _validate_sizes(n, m):
    """scipy.signal._czt._validate_sizes, with its texts"""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"Invalid number of CZT data points ({n}) specified. n must be positive and integer type.")
    if m is None:
        m = n
    elif isinstance(m, (bool, np.bool_)) or not isinstance(m, numbers.Integral) or m < 1:
        raise ValueError(f"Invalid number of CZT output points ({m}) specified. m must be positive and integer type.")
    return int(m)


def _point(v, what, fn):
    """a finite non-zero complex number as (modulus, argument in turns)"""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Number, np.number)):
        raise ArgumentError(f"{fn}: {what} must be a number, got: {v!r}")
    v = complex(v)
    if not (cmath.isfinite(v) and abs(v) > 0.0 and math.isfinite(abs(v))):
        raise ArgumentError(f"{fn}: {what} must be finite and non-zero, got: {v!r}")
    return abs(v), cmath.phase(v) / (2.0 * math.pi)


def _run(fn, x, m, contour, axis, ctx):
    """contour: (w_abs, w_step, w_den, a_abs, a_turns) once m is known"""
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        if xo.dtype in (np.dtype(np.float64), np.dtype(np.complex128)):
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 and c64 rows are built")
        if xo.device:
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: device tensors must be f32 or c64")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32)
    rank = len(xo.shape)
    if rank < 1:
        raise ArgumentError(f"{fn}: the tensor must have at least one axis")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -rank <= axis < rank:
        raise ArgumentError(f"{fn}: axis {axis!r} is out of bounds for a tensor of rank {rank}")
    m = _validate_sizes(int(xo.shape[int(axis) % rank]), m)
    w_abs, w_step, w_den, a_abs, a_turns = contour(m)
    from .filters import _axis_last   # here, not at the top: the package imports either module first
    axis = _axis_last(xo, axis, fn, NxSignalUnsupported(f"{fn}: unsupported axis: device tensors are transformed along their last axis only"))
    batch, n = rows_last(xo.shape)
    if n + m - 1 > 1 << 30:
        raise NxSignalUnsupported(f"{fn}: unsupported size: n + m - 1 must be at most 2^30, got n = {n}, m = {m}")
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-1] + (m,), np.complex64)
    _lib.check(_lib.load().nxsig_czt(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, int(xo.dtype.kind == "c"), n, batch, n, m,
                                     w_abs, w_step, w_den, a_abs, a_turns, ptr(out), xo.mem))
    return out if xo.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))


def czt(x, m=None, w=None, a=1 + 0j, *, axis=-1, ctx=None):
    """scipy.signal.czt(x, m, w, a, axis=axis) on the GPU: X[k] = sum_j x[j] a^(-j) w^(j k) for k < m along `axis` (include/nxsig.h
    states the definition).  m defaults to the length of the axis and w to exp(-2 pi i / m), whose phases are then exact rationals; a
    given w or a is taken as modulus and argument, and a spiral (|w| or |a| off 1) is served while the chirps stay within single
    precision (else NxSignalUnsupported).  Real f32 or c64 tensors, c64 out; host integer and narrower float arrays are computed as f32;
    f64 / c128 rows are unsupported.  Host arrays: any axis, numpy out; a device tensor: the last axis only, a DeviceBuffer out, and the
    call does not wait.  A line that holds an Inf / NaN has no finite output; the other lines keep theirs."""
    fn = "czt"
    a_abs, a_turns = _point(a, "a", fn)
    if w is not None:
        w_abs, w_turns = _point(w, "w", fn)

    def contour(m):
        return (1.0, 1.0, m, a_abs, a_turns) if w is None else (w_abs, -w_turns, 1, a_abs, a_turns)
    return _run(fn, x, m, contour, axis, ctx)


def zoom_fft(x, fn, m=None, *, fs=2, endpoint=False, axis=-1, ctx=None):
    """scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint, axis=axis) on the GPU: m points of the DFT of every line, evenly spaced
    over the frequencies [f1, f2) (fn = [f1, f2], or a scalar f2 with f1 = 0) of a signal sampled at fs.  The step is carried as the
    rational scale / m of a turn, scale as SciPy computes it, so the phases of long rows are reduced exactly where SciPy's double
    loses them.  Operands as czt's."""
    name = "zoom_fft"
    size = np.size(fn)
    if size == 2:
        f1, f2 = fn
    elif size == 1:
        f1, f2 = 0.0, fn
    else:
        raise ValueError("fn must be a scalar or 2-length sequence")
    try:
        f1, f2, fs = (float(np.asarray(v).reshape(())) for v in (f1, f2, fs))
    except (TypeError, ValueError):
        raise ArgumentError(f"{name}: fn and fs must be real numbers, got: {fn!r}, {fs!r}") from None
    if not (math.isfinite(f1) and math.isfinite(f2) and math.isfinite(fs)) or fs == 0.0:
        raise ArgumentError(f"{name}: fn and fs must be finite and fs non-zero, got: {fn!r}, {fs!r}")
    if not isinstance(endpoint, (bool, np.bool_)):
        raise ArgumentError(f"{name}: endpoint must be a boolean, got: {endpoint!r}")

    def contour(m):
        if endpoint:
            if m < 2:
                raise ValueError(f"{name}: endpoint=True needs m >= 2")
            scale = ((f2 - f1) * m) / (fs * (m - 1))
        else:
            scale = (f2 - f1) / fs
        return 1.0, scale, m, 1.0, f1 / fs
    return _run(name, x, m, contour, axis, ctx)


def czt_points(m, w=None, a=1 + 0j):
    """scipy.signal.czt_points(m, w, a): the m points of the z-plane at which czt samples the z-transform, complex128, by SciPy's
    formula.  Host only."""
    m = _validate_sizes(1, m)
    k = np.arange(m)
    a = 1.0 * a
    if w is None:
        return a * np.exp(2j * np.pi * k / m)
    return a * (1.0 * w) ** -k
