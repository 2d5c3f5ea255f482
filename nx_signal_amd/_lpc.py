"""Spectral.lpc (an extension: librosa.lpc, Burg's linear prediction, per frame), on the kernels of
csrc/kernels_lpc.hip.  Reached as nx_signal_amd.spectral.lpc."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

MAX_ORDER = 128


def _integer(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ArgumentError(f"lpc: {what} must be an integer, got: {v!r}")
    return int(v)


def lpc(x, order, frame_length=None, hop=None, *, return_reflection=False, return_error=False, ctx=None):
    """librosa.lpc(y, order=order) on the GPU, of every frame of every row: Burg's method.  x: f32 host array or device tensor of rank
    >= 1, time on the last axis.  frame_length=None takes each row whole and returns a = f32[..., order + 1], the prediction
    polynomial with a[0] = 1; with frame_length the rows are framed as librosa.util.frame does (F = 1 + (n - frame_length) // hop frames
    at multiples of hop, default frame_length // 4; no padding; hop may exceed frame_length) and a is f32[..., F, order + 1].
    return_reflection appends the reflection coefficients k = f32[..., (F,) order], return_error the prediction error power
    e = f32[..., (F)] = mean(x^2) prod(1 - k^2); with either flag the result is a tuple.  Every sum is double on the device and the
    denominator is summed afresh at every stage (include/nxsig.h states the definition), where librosa updates it by a recurrence
    and computes in the type of y: for f32 rows the result is librosa's up to librosa's own single-precision rounding.  1 <= order <
    frame_length; orders up to 128 are built; f64 rows are unsupported.  An Inf / NaN sample makes the outputs of exactly the frames
    that contain it non-finite.  A host array gives numpy arrays; a device tensor DeviceBuffers, and the call does not wait."""
    p = _integer(order, "order")
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype == np.dtype(np.float64):
        raise NxSignalUnsupported("lpc: unsupported type float64: f32 rows are built")
    if xo.dtype != np.dtype(np.float32):
        raise ArgumentError(f"lpc: expected real f32 rows, got {xo.dtype}")
    if len(xo.shape) < 1:
        raise ArgumentError("lpc: expected a tensor of rank >= 1")
    xo.cast()
    batch, n = rows_last(xo.shape)
    whole = frame_length is None
    L = n if whole else _integer(frame_length, "frame_length")
    h = max(L // 4, 1) if hop is None else _integer(hop, "hop")
    if p < 1:
        raise ArgumentError(f"lpc: order must be >= 1, got: {p}")
    if p >= L:
        raise ArgumentError(f"lpc: order must be < frame_length ({L}), got: {p}")
    if h < 1:
        raise ArgumentError(f"lpc: hop must be >= 1, got: {h}")
    if L > n:
        raise ArgumentError(f"lpc: frame_length must be <= the row length ({n}), got: {L}")
    if p > MAX_ORDER:
        raise NxSignalUnsupported(f"lpc: orders up to {MAX_ORDER} are built, got: {p}")
    frames = int(_lib.load().nxsig_lpc_frames(n, L, h))
    if frames < 0:
        _lib.check(frames)
    lead = xo.shape[:-1] + (() if whole else (frames,))
    c = xo.context(ctx, caller_first=False)
    a = xo.result(lead + (p + 1,), np.float32)
    k = xo.result(lead + (p,), np.float32) if return_reflection else None
    e = xo.result(lead, np.float32) if return_error else None
    if batch:
        _lib.check(_lib.load().nxsig_lpc_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, batch, n, n, L, h, p, ptr(a), ptr(k), ptr(e), xo.mem))
    out = (a,) + ((k,) if return_reflection else ()) + ((e,) if return_error else ())
    return out if len(out) > 1 else a
