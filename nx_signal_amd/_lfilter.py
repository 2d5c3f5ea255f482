"""Filters.lfilter / lfilter_zi / filtfilt / lfiltic (an extension: scipy.signal 1.15's transfer-function filter),
on the kernels of csrc/kernels_lfilter.hip.  Reached as nx_signal_amd.filters.lfilter and so on."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import ptr, rows_last

_MAX_ORDER = 16
_PD = C.POINTER(C.c_double)


def _ba(b, a, fn):
    """(b, a) as C-contiguous f64 vectors, validated as the library does (a[0] is divided out on the other side)"""
    out = []
    for name, v in (("b", b), ("a", a)):
        try:
            arr = np.atleast_1d(np.asarray(v))
            if arr.dtype.kind not in "fiub":
                raise TypeError
            arr = np.ascontiguousarray(arr, dtype=np.float64)
        except (TypeError, ValueError):
            raise ArgumentError(f"{fn}: {name} must be a real 1-D array") from None
        if arr.ndim != 1:
            raise ArgumentError(f"{fn}: {name} must be a real 1-D array, got shape {arr.shape}")
        if arr.shape[0] < 1:
            raise ArgumentError(f"{fn}: b and a must have at least one coefficient each")
        if not np.isfinite(arr).all():
            raise ArgumentError(f"{fn}: b and a must be finite")
        out.append(arr)
    b, a = out
    if a[0] == 0:
        raise ArgumentError(f"{fn}: a[0] must not be zero")
    if max(b.shape[0], a.shape[0]) - 1 > _MAX_ORDER:
        where = "filters.fir runs an FIR filter of any length" if a.shape[0] == 1 else "a recursive filter of this order belongs in second-order sections: sosfilt"
        raise NxSignalUnsupported(f"{fn}: orders up to {_MAX_ORDER} are built, got {max(b.shape[0], a.shape[0]) - 1} ({where})")
    return b, a


def lfilter_zi(b, a):
    """scipy.signal.lfilter_zi: the state (max(len(a), len(b)) - 1,) of the filter's settled step response."""
    b, a = _ba(b, a, "lfilter_zi")
    zi = np.empty(max(b.shape[0], a.shape[0]) - 1, np.float64)
    _lib.check(_lib.load().nxsig_lfilter_zi(C.cast(ptr(b), _PD), b.shape[0], C.cast(ptr(a), _PD), a.shape[0],
                                            C.cast(ptr(zi) if zi.size else ptr(np.empty(1)), _PD)))
    return zi


def lfiltic(b, a, y, x=None):
    """scipy.signal.lfiltic(b, a, y, x=None) on the host, in double: the state lfilter starts from so that its past outputs were
    y = {y[-1], y[-2], ...} and its past inputs x = {x[-1], x[-2], ...} (too short: filled up with zeros).  As scipy's, it takes b and
    a as they stand: divide both by a[0] first when a[0] != 1."""
    b, a = _ba(b, a, "lfiltic")
    N, M = a.shape[0] - 1, b.shape[0] - 1
    try:
        yv = np.asarray(y, np.float64).ravel()
        xv = np.zeros(M) if x is None else np.asarray(x, np.float64).ravel()
    except (TypeError, ValueError):
        raise ArgumentError("lfiltic: y and x must be real arrays") from None
    if xv.size < M:
        xv = np.r_[xv, np.zeros(M - xv.size)]
    if yv.size < N:
        yv = np.r_[yv, np.zeros(N - yv.size)]
    zi = np.zeros(max(M, N), np.float64)
    for m in range(M):
        zi[m] = np.sum(b[m + 1:] * xv[:M - m], axis=0)
    for m in range(N):
        zi[m] -= np.sum(a[m + 1:] * yv[:N - m], axis=0)
    return zi


def lfilter(x, b, a, zi=None, ctx=None, axis=-1, direction=0):
    """Extension (the reference has no recursive filter): scipy.signal.lfilter(b, a, x, axis, zi) on the GPU — the transfer function
    (b, a), both divided by a[0], in transposed direct form II over `axis` of real f32 rows, computed in double and rounded to f32
    once.  Orders max(len(b), len(a)) - 1 up to 16.  Returns y, or (y, zf) when `zi` (the shape of x with the order in place of `axis`)
    is given; zf is a numpy array.  Host arrays: any axis, numpy out; a device tensor: the last axis only, a DeviceBuffer out.
    direction=1 runs the filter from the end of each row towards its start.  Outputs ahead of a row's first Inf / NaN are untouched by
    it; every output from it on is non-finite (the recurrence's behaviour, also for an FIR filter)."""
    from .filters import _sos_operand   # here, not at the top: filters imports this module, and either may be imported first
    b, a = _ba(b, a, "lfilter")
    x, shape, axis = _sos_operand(x, axis, "lfilter")
    if direction not in (0, 1):
        raise ArgumentError(f"lfilter: direction must be 0 or 1, got: {direction!r}")
    (batch, n), order = rows_last(x.shape), max(b.shape[0], a.shape[0]) - 1
    zrows = zf = None
    if zi is not None:
        z = np.asarray(zi)
        want = shape[:axis] + (order,) + shape[axis + 1:]
        if z.shape != want or z.dtype.kind not in "fiu":
            raise ArgumentError(f"lfilter: invalid zi shape. With axis={axis - len(shape)}, an input with shape {shape}, and a filter of order "
                                f"{order}, zi must have shape {want}, got {z.shape}.")
        # [batch][order] for the C ABI
        zrows = np.ascontiguousarray(np.moveaxis(z.astype(np.float64), axis, -1).reshape(batch, order))
        zf = np.empty((batch, order), np.float64)
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, np.float32)
    some = order > 0   # a gain has no state: nothing to hand over
    _lib.check(_lib.load().nxsig_lfilter_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), x.ptr, n, batch, n, ptr(b), b.shape[0], ptr(a), a.shape[0],
                                             ptr(zrows) if some else None, batch, ptr(zf) if some else None, int(direction), ptr(out), x.mem))
    if not x.device:
        out = np.ascontiguousarray(np.moveaxis(out, -1, axis))
    if zi is None:
        return out
    zf = np.moveaxis(zf.reshape(shape[:axis] + shape[axis + 1:] + (order,)), -1, axis)
    return out, np.ascontiguousarray(zf)


_PADTYPES = {None: 0, "odd": 1, "even": 2, "constant": 3}


def filtfilt(x, b, a, ctx=None, axis=-1, padtype="odd", padlen=None, method="pad"):
    """Extension: scipy.signal.filtfilt(b, a, x, axis, padtype, padlen, method="pad") in one device-resident call — the rows extended by
    `padlen` samples per side (default: 3 * max(len(a), len(b))), filtered forward and backward from the states lfilter_zi scaled by the
    first sample each way, the middle kept.  padtype "odd" (default), "even", "constant" or None.  Real f32 rows; host arrays: any axis,
    numpy out; a device tensor: the last axis only, a DeviceBuffer out.  method="gust" is not built.  A row with an Inf / NaN is
    non-finite everywhere."""
    from .filters import _sos_operand
    if method != "pad":
        if method == "gust":
            raise NxSignalUnsupported("filtfilt: method 'gust' is not built; method='pad' is")
        raise ArgumentError("filtfilt: method must be 'pad' or 'gust'.")
    b, a = _ba(b, a, "filtfilt")
    if isinstance(padtype, (list, dict, set, np.ndarray)) or padtype not in _PADTYPES:
        raise ArgumentError(f"filtfilt: unknown value {padtype!r} given to padtype. padtype must be 'even', 'odd', 'constant', or None.")
    if padlen is not None and (isinstance(padlen, bool) or not isinstance(padlen, (int, np.integer)) or padlen < 0):
        raise ArgumentError(f"filtfilt: padlen must be a non-negative integer or None, got: {padlen!r}")
    x, shape, axis = _sos_operand(x, axis, "filtfilt")
    batch, n = rows_last(x.shape)
    edge = 0 if padtype is None else 3 * max(b.shape[0], a.shape[0]) if padlen is None else int(padlen)
    if n <= edge:   # scipy's _validate_pad
        raise ArgumentError(f"filtfilt: the length of the input vector x must be greater than padlen, which is {edge}.")
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, np.float32)
    _lib.check(_lib.load().nxsig_filtfilt_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), x.ptr, n, batch, n, ptr(b), b.shape[0], ptr(a), a.shape[0],
                                              _PADTYPES[padtype], edge, ptr(out), x.mem))
    return out if x.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))
