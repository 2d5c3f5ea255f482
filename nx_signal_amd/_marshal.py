"""How a wrapper of this package hands a tensor to the C ABI: one operand type for host arrays and device-resident objects.

A wrapper is written once, for both placements:

    o = validate(opts, {...defaults...}, "fn")           # unknown option keys raise, defaults are filled in
    x = Operand(_as_tensor(t))                            # .device .shape .dtype .owner; nothing is copied yet
    ... the function's own dtype rule and argument checks, on x.dtype / x.shape ...
    x.cast(np.float32)                                    # host arrays: a contiguous copy in that type; device operands stay
    rows, n = rows_last(x.shape)
    c = x.context(ctx, caller_first=...)                  # as late as possible: argument errors need no GPU
    out = x.result(x.shape[:-1] + (m,), np.complex64)     # a DeviceBuffer of c, or np.empty: where the operand lives
    _lib.check(lib.nxsig_...(c.handle, x.ptr, n, rows, ..., ptr(w), ptr(out), x.mem))
    return out

`ptr(a)` is the c_void_p of a DeviceBuffer, an ndarray or None.  Which element types a function takes, and what it widens them to,
stays in the function: that is the API, not marshalling.  A function that works along one axis calls x.move_last(axis) (host arrays;
device tensors are taken along their last axis) and np.moveaxis(out, -1, axis) on the way back.  Operand(t, any_dtype=True) takes
torch tensors of integer types too (PeakFinding).  is_device() is left for refusals ("takes host tensors"), never to pick a branch
of a call.

Which context a call runs on.  `ctx=` is what the caller passed, the owner is the Context of a DeviceBuffer operand (any other device
object has none), the default is default_context().  Two rules exist and every function keeps the one it was written with:

    caller_first=True    ctx=, then the owner, then the default
        as_windowed, stft, stft_onesided, stft_packed, istft, istft_packed, istft_filtered, istft_masked, overlap_and_add,
        stft_to_mel, spectrum_multiply, spectrum_mask, mel_spectrogram, spectrogram, convolve, correlate, fftconvolve, fir,
        fft_nd, ifft_nd
    caller_first=False   the owner, then ctx=, then the default
        median, wiener, resample_poly, sosfilt, sosfiltfilt, welch, csd, coherence, sawtooth, square, gaussian_pulse, chirp,
        polynomial_sweep, argrelmin, argrelmax, argrelextrema

unit_impulse and nonzero allocate on `ctx=` or the default: they have no device operand.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib, device
from ._lib import ArgumentError
from .device import DeviceBuffer, device_view, is_device


def validate(opts: dict, allowed, fn: str) -> dict:
    """Keyword.validate!/keyword! — unknown keys raise ArgumentError; `allowed` as a dict gives the defaults"""
    unknown = [k for k in opts if k not in allowed]
    if unknown:
        raise ArgumentError(f"unknown keys {unknown} in {fn} options, the allowed keys are: {list(allowed)}")
    out = dict(allowed) if isinstance(allowed, dict) else {}
    out.update(opts)
    return out


def _as_tensor(x):
    """What Nx.tensor/1 would make of a host value: numpy arrays keep their dtype (np.float64 IS f64: the f64 tier); plain Python
    numbers and (nested) lists follow Nx's inference — floats become f32, complex numbers c64, integers stay integers."""
    if isinstance(x, np.ndarray) or is_device(x):
        return x
    a = np.asarray(x)
    if a.dtype == np.float64:
        return a.astype(np.float32)
    if a.dtype == np.complex128:
        return a.astype(np.complex64)
    return a


def rows_last(shape):
    """(product of the leading axes, last axis) of a shape of rank >= 1"""
    return int(math.prod(shape[:-1])), int(shape[-1])


def ptr(a):
    """the c_void_p of a DeviceBuffer, an ndarray or None"""
    if a is None:
        return None
    return C.c_void_p(a.ptr) if isinstance(a, DeviceBuffer) else a.ctypes.data_as(C.c_void_p)


class Operand:
    """A tensor argument as the C ABI takes it: a pointer, a shape, a dtype, where it lives and whose it is"""

    def __init__(self, t, any_dtype=False):
        self.device = is_device(t)
        if self.device:
            self._ptr, shape, dtype = device_view(t, any_dtype)
            self.host, self.owner = None, (t.ctx if isinstance(t, DeviceBuffer) else None)
        else:
            self.host, self.owner = np.asarray(t), None
            shape, dtype = self.host.shape, self.host.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.mem = _lib.DEVICE if self.device else _lib.HOST
        self.ctx = None

    def cast(self, dtype=None):
        """host arrays: a C-contiguous copy in `dtype` (default: their own) from here on; device operands are taken as they are"""
        if not self.device:
            self.host = np.ascontiguousarray(self.host if dtype is None else self.host.astype(dtype, copy=False))
            self.shape, self.dtype = self.host.shape, self.host.dtype
        return self

    def move_last(self, axis):
        """host arrays: `axis` goes to the back (a contiguous copy); np.moveaxis(result, -1, axis) brings a result's back"""
        if not self.device:
            self.host = np.ascontiguousarray(np.moveaxis(self.host, axis, -1))
            self.shape = self.host.shape
        return self

    @property
    def ptr(self):
        return C.c_void_p(self._ptr) if self.device else self.host.ctypes.data_as(C.c_void_p)

    def context(self, ctx, *, caller_first):
        """the context of the call, by one of the two rules of the module docstring; result() allocates on it"""
        first, second = (ctx, self.owner) if caller_first else (self.owner, ctx)
        self.ctx = first or second or device.default_context()
        return self.ctx

    def result(self, shape, dtype):
        """an uninitialised tensor where the operand lives: a DeviceBuffer of the call's context, or a numpy array"""
        return DeviceBuffer.empty(self.ctx, shape, dtype) if self.device else np.empty(shape, dtype)
