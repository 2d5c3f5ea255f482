"""Filters.hilbert (an extension: scipy.signal 1.15's analytic signal), on the kernels of
csrc/kernels_hilbert.hip.  Reached as nx_signal_amd.filters.hilbert."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last, validate

# nxsig_hilbert_kind of include/nxsig.h
_OUTPUTS = {"analytic": 0, "envelope": 1, "quadrature": 2}
_KEYS = ("N", "axis", "ctx", "output")


def hilbert(x, N=None, axis=-1, ctx=None, output="analytic", **opts):
    """scipy.signal.hilbert(x, N=None, axis=-1) on the GPU: every line of x along `axis` is truncated or zero-padded to N points
    (default: its length) and a = ifft(fft(line) * h) with h[0] = 1, h[N / 2] = 1 for an even N, 2 on the positive frequencies in between
    and 0 elsewhere (include/nxsig.h states the definition).  output="analytic" returns a (c64), "envelope" |a| and "quadrature" Im a, the
    Hilbert transform of the line (f32).  Real f32 tensors; host integer and narrower float arrays are computed as f32; f64 rows are
    unsupported.  Host arrays: any axis, numpy out; a device tensor: the last axis only, a DeviceBuffer out, and the call does not wait.
    A line that holds an Inf / NaN among the samples used has no finite output; the other lines keep theirs."""
    fn = "hilbert"
    validate(opts, _KEYS, fn)
    if not isinstance(output, str) or output not in _OUTPUTS:
        raise ArgumentError(f"{fn}: output must be 'analytic', 'envelope' or 'quadrature', got: {output!r}")
    if N is not None:
        if isinstance(N, (bool, np.bool_)) or not isinstance(N, (int, np.integer)):
            raise ArgumentError(f"{fn}: N must be an integer, got: {N!r}")
        if N <= 0:
            raise ValueError("N must be positive.")
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype.kind == "c":
        raise ValueError("x must be real.")
    if xo.dtype != np.dtype(np.float32):
        if xo.dtype == np.dtype(np.float64):
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 rows are built")
        if xo.device:
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: device tensors must be f32")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32)
    from .filters import _axis_last   # here, not at the top: filters imports this module, and either may be imported first
    axis = _axis_last(xo, axis, fn, NxSignalUnsupported(f"{fn}: unsupported axis: device tensors are transformed along their last axis only"))
    batch, length = rows_last(xo.shape)
    n_fft = length if N is None else int(N)
    if n_fft >= 1 << 31:
        raise NxSignalUnsupported(f"{fn}: unsupported N: rows of fewer than 2^31 points are built, got {n_fft}")
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-1] + (n_fft,), np.complex64 if output == "analytic" else np.float32)
    _lib.check(_lib.load().nxsig_hilbert_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, length, batch, length, n_fft, _OUTPUTS[output],
                                             ptr(out), xo.mem))
    return out if xo.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))
