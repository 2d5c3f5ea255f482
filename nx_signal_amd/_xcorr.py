"""Convolution.correlate_rows / convolve_rows / correlation_lags (extensions: scipy.signal 1.15's correlate / convolve /
correlation_lags on row PAIRS), on the kernels of csrc/kernels_xcorr.hip.  Reached as
nx_signal_amd.convolution.correlate_rows, convolve_rows and correlation_lags."""
from __future__ import annotations

import numbers

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

_MODES = {"full": _lib.CONV_FULL, "same": _lib.CONV_SAME, "valid": _lib.CONV_VALID}
CONVOLVE, CORRELATE = 0, 1
PLAIN, PHAT = 0, 1
ROWS, PEAK = 0, 1
_F32, _C64 = np.dtype(np.float32), np.dtype(np.complex64)


def _length(v, what, fn):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or v < 1:
        raise ArgumentError(f"{fn}: {what} must be a positive integer, got: {v!r}")
    return int(v)


def correlation_lags(in1_len, in2_len, mode="full"):
    """scipy.signal.correlation_lags(in1_len, in2_len, mode): the lag of every element of correlate's result, by SciPy's formula (its
    "same" window of the lags included, which is one off the window of the values for odd in1_len with even in2_len).  Host only."""
    fn = "correlation_lags"
    n1, n2 = _length(in1_len, "in1_len", fn), _length(in2_len, "in2_len", fn)
    if mode not in _MODES:
        raise ArgumentError(f"{fn}: expected mode to be one of 'full', 'same', 'valid', got: {mode!r}")
    if mode == "full":
        return np.arange(-n2 + 1, n1)
    if mode == "same":
        lags = np.arange(-n2 + 1, n1)
        mid, bound = lags.size // 2, n1 // 2
        return lags[mid - bound:mid + bound + (n1 % 2)]
    bound = n1 - n2
    return np.arange(bound + 1) if bound >= 0 else np.arange(bound, 1)


def _operand(fn, name, t):
    o = Operand(_as_tensor(t), any_dtype=True)
    if o.dtype in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise NxSignalUnsupported(f"{fn}: unsupported type {o.dtype} of {name}: real f32 and c64 rows are built")
    if o.dtype not in (_F32, _C64):
        if o.device:
            raise NxSignalUnsupported(f"{fn}: unsupported type {o.dtype} of {name}: device tensors must be f32 or c64")
        if o.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {o.dtype} of {name}")
    return o


def _run(fn, op, in1, in2, mode, weighting, phat_floor, output, axis, ctx):
    if mode not in _MODES:
        raise ArgumentError(f"{fn}: expected mode to be one of 'full', 'same', 'valid', got: {mode!r}")
    if weighting not in (None, "phat"):
        raise ArgumentError(f"{fn}: expected weighting to be None or 'phat', got: {weighting!r}")
    if output not in ("rows", "peak"):
        raise ArgumentError(f"{fn}: expected output to be 'rows' or 'peak', got: {output!r}")
    if isinstance(phat_floor, (bool, np.bool_)) or not isinstance(phat_floor, numbers.Real) or not 0.0 <= float(phat_floor) < 1.0:
        raise ArgumentError(f"{fn}: phat_floor must be a number in [0, 1), got: {phat_floor!r}")
    same = in1 is in2
    a = _operand(fn, "in1", in1)
    b = a if same else _operand(fn, "in2", in2)
    if a.device != b.device:
        raise ArgumentError(f"{fn}: in1 and in2 must both be host arrays or both be device tensors")
    if (a.dtype == _C64) != (b.dtype == _C64):
        raise ArgumentError(f"{fn}: in1 and in2 must both be real or both be complex, got {a.dtype} and {b.dtype}")
    dtype = _C64 if a.dtype == _C64 else _F32
    if len(a.shape) < 1 or len(b.shape) < 1:
        raise ArgumentError(f"{fn}: the tensors must have at least one axis")
    from .filters import _axis_last   # here, not at the top: the package imports either module first
    device_error = NxSignalUnsupported(f"{fn}: unsupported axis: device tensors are taken along their last axis only")
    template = not same and len(b.shape) == 1 and len(a.shape) != 1
    if not a.device:
        a.cast(dtype)
        if not same:
            b.cast(dtype)
    rank = len(a.shape)
    axis = _axis_last(a, axis, fn, device_error)
    if not same:
        if template:
            _axis_last(b, -1, fn, device_error)
        else:
            if len(b.shape) != rank:
                raise ArgumentError(f"{fn}: in2 must have the shape of in1 up to the correlated axis, or one axis; got {a.shape} and {b.shape}")
            _axis_last(b, axis, fn, device_error)
            if b.shape[:-1] != a.shape[:-1]:
                raise ArgumentError(f"{fn}: in2 must have the shape of in1 up to the correlated axis, or one axis; got {a.shape} and {b.shape}")
    batch, n1 = rows_last(a.shape)
    n2 = int(b.shape[-1])
    if n1 + n2 - 1 > 1 << 30:
        raise NxSignalUnsupported(f"{fn}: unsupported size: n1 + n2 - 1 must be at most 2^30, got n1 = {n1}, n2 = {n2}")
    lib = _lib.load()
    n_out = _lib.check(lib.nxsig_conv_length(n1, n2, _MODES[mode]))
    c = a.context(ctx, caller_first=False)
    lead = a.shape[:-1]
    peak = output == "peak"
    out = a.result(lead if peak else lead + (n_out,), dtype)
    lags = a.result(lead, np.int32) if peak else None
    _lib.check(lib.nxsig_xcorr(_lib.ctx_ptr(c.handle, _lib._ctx_iir), a.ptr, n1, n1, b.ptr, n2, 0 if template else n2, batch, int(dtype == _C64), op,
                               _MODES[mode], PHAT if weighting == "phat" else PLAIN, float(phat_floor), PEAK if peak else ROWS, ptr(out), ptr(lags),
                               a.mem))
    if peak:
        return lags, out
    return out if a.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))


def correlate_rows(in1, in2, mode="full", *, weighting=None, phat_floor=0.0, output="rows", axis=-1, ctx=None):
    """scipy.signal.correlate(in1[r], in2[r], mode) for every row pair r on the GPU (include/nxsig.h states the definition).  in1 is
    [..., n1]; in2 is [..., n2] with the same leading shape, or 1-D: one template for every row.  `in1 is in2` is the autocorrelation.
    Both real f32 (f32 out) or both c64 (c64 out); host integer and narrower float arrays are computed as f32; f64 / c128 are
    unsupported and a mixed pair is an ArgumentError.  weighting="phat" whitens the cross spectrum (GCC-PHAT) at the contract's
    transform length, phat_floor in [0, 1) bounding the division.  output="peak" returns (lags s32[...], values[...]) instead of the
    rows: correlation_lags(n1, n2, mode)[argmax] and the value there, the first maximum of the values (real) or moduli (c64); the rows
    are never written.  Host arrays: any axis, numpy out; device tensors: the last axis only, DeviceBuffers out, and the call does not
    wait.  A pair that holds an Inf / NaN has no finite output (peak: NaN at lag 0); the other pairs keep theirs."""
    return _run("correlate_rows", CORRELATE, in1, in2, mode, weighting, phat_floor, output, axis, ctx)


def convolve_rows(in1, in2, mode="full", *, axis=-1, ctx=None):
    """scipy.signal.convolve(in1[r], in2[r], mode) for every row pair r on the GPU; operands and results as correlate_rows'."""
    return _run("convolve_rows", CONVOLVE, in1, in2, mode, None, 0.0, "rows", axis, ctx)
