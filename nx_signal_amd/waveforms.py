"""NxSignal.Waveforms (lib/nx_signal/waveforms.ex): sawtooth/2, square/2, gaussian_pulse/2, chirp/5, polynomial_sweep/3, unit_impulse/2 on
the kernels of DESIGN.md section 3.10, and sinc/1 (:451-457, on the host: the FIR design path needs it).

t is a host array (numbers and lists as Nx.tensor reads them; integers become f32, np.float64 stays f64) or a device tensor of f32 /
f64, which gives device tensors back.  f32 results reproduce the reference's literals bit for bit; f64 is the same expression
evaluated in double.  Options are keyword arguments with the reference's names and defaults; an unknown one raises ArgumentError, as
do the reference's own checks, before any device is touched."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError
from .device import DeviceBuffer, default_context, device_view, is_device

_METHODS = {"linear": _lib.CHIRP_LINEAR, "quadratic": _lib.CHIRP_QUADRATIC, "logarithmic": _lib.CHIRP_LOGARITHMIC,
            "hyperbolic": _lib.CHIRP_HYPERBOLIC}
# unit_impulse's :type — the native element types of the kernel; narrower integer types are refused (an s8 result cannot be widened
# behind the caller's back the way a PeakFinding input can)
_TYPES = {"f32": np.float32, "f64": np.float64, "s32": np.int32, "s64": np.int64, "u32": np.uint32, "u64": np.uint64}
_DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64, np.dtype(np.int32): _lib.DT_S32,
       np.dtype(np.int64): _lib.DT_S64, np.dtype(np.uint32): _lib.DT_U32, np.dtype(np.uint64): _lib.DT_U64}


def sinc(t):
    a = t if isinstance(t, np.ndarray) else np.asarray(t, dtype=np.float32)   # Nx.tensor(number / list) is f32; an np.float64 array is f64
    if a.dtype == np.float64:   # f64 tensor: evaluated in double (the pi() of the reference's defn stays the f32 constant)
        a = np.ascontiguousarray(a)
        out = np.empty_like(a)
        _lib.check(_lib.load().nxsig_sinc_f64(a.ctypes.data_as(_lib.C.c_void_p), a.size, out.ctypes.data_as(_lib.C.c_void_p)))
        return out
    a = np.ascontiguousarray(np.asarray(t, dtype=np.float32))
    out = np.empty_like(a)
    _lib.check(_lib.load().nxsig_sinc_f32(a.ctypes.data_as(_lib.C.c_void_p), a.size, out.ctypes.data_as(_lib.C.c_void_p)))
    return out


def _options(opts, defaults, fn):
    unknown = [k for k in opts if k not in defaults]
    if unknown:   # keyword! / Keyword.validate!
        raise ArgumentError(f"unknown keys {unknown} in {fn} options, the allowed keys are: {list(defaults)}")
    o = dict(defaults)
    o.update(opts)
    return o


def _number(v, what, fn):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ArgumentError(f"{fn}: {what} must be a number, got: {v!r}")
    return float(v)


class _Tensor:
    """t (or a second stream of t's shape) as the C ABI takes it: a pointer, the tier and where it lives"""

    def __init__(self, t, fn, like=None):
        self.device = is_device(t)
        if self.device:
            ptr, shape, dtype = device_view(t)
            dtype = np.dtype(dtype)
            if dtype not in (np.float32, np.float64):
                raise ArgumentError(f"{fn}: device tensors must be f32 or f64, got {dtype}")
            self.ctx = t.ctx if isinstance(t, DeviceBuffer) else None
            self.host, self.ptr = None, C.c_void_p(ptr)
        else:
            from . import _as_tensor
            a = np.asarray(_as_tensor(t))
            if a.dtype.kind == "c":
                raise ArgumentError(f"{fn}: complex tensors are not supported")
            if a.dtype.kind not in "fiub":
                raise ArgumentError(f"{fn}: unsupported type {a.dtype}")
            want = like.dtype if like is not None else (np.float64 if a.dtype == np.float64 else np.float32)
            a = np.ascontiguousarray(a, dtype=want)   # integers become f32, as in an Nx binary op with the f32 pi()
            shape, dtype = a.shape, a.dtype
            self.ctx, self.host, self.ptr = None, a, a.ctypes.data_as(C.c_void_p)
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = math.prod(self.shape)
        self.is_f64 = int(self.dtype == np.float64)
        self.mem = _lib.DEVICE if self.device else _lib.HOST

    def context(self, ctx):
        return self.ctx or ctx or default_context()

    def result(self, c, dtype=None):
        dtype = dtype or self.dtype
        return DeviceBuffer.empty(c, self.shape, dtype) if self.device else np.empty(self.shape, dtype)


def _ptr(a):
    return C.c_void_p(a.ptr) if isinstance(a, DeviceBuffer) else a.ctypes.data_as(C.c_void_p)


def sawtooth(t, ctx=None, **opts):
    """Waveforms.sawtooth/2 — waveforms.ex:29-54.  Period 2 pi(), rising from -1 to 1 over [0, 2 pi() width] and falling back over
    the rest; width (default 1) in [0, 1].  Nx.remainder is C fmod: a negative t keeps its sign, as in the reference."""
    o = _options(opts, {"width": 1}, "sawtooth")
    width = _number(o["width"], "width", "sawtooth")
    if not 0 <= width <= 1:   # :34-36
        raise ArgumentError(f"width must be between 0 and 1, inclusive. Got: {o['width']!r}")
    x = _Tensor(t, "sawtooth")
    c = x.context(ctx)
    out = x.result(c)
    _lib.check(_lib.load().nxsig_sawtooth(c.handle, x.ptr, x.is_f64, x.n, width, _ptr(out), x.mem))
    return out


def square(t, ctx=None, **opts):
    """Waveforms.square/2 — waveforms.ex:96-104.  1 where fmod(t, 2 pi()) < duty * 2 * pi(), else -1, as int32.  duty (default 0.5)
    is a number or a tensor of t's shape that lives where t lives; it is read in t's type."""
    o = _options(opts, {"duty": 0.5}, "square")
    duty = o["duty"]
    x = _Tensor(t, "square")
    scalar, second = 0.0, None
    if is_device(duty) or isinstance(duty, (np.ndarray, list, tuple)):
        second = _Tensor(duty, "square", like=x)
        if second.device != x.device:
            raise ArgumentError("square: t and duty must both be host tensors or both be device tensors")
        if second.dtype != x.dtype:
            raise ArgumentError(f"square: duty must have t's type {x.dtype}, got {second.dtype}")
        if second.shape != x.shape:
            raise ArgumentError(f"square: duty must have t's shape {x.shape}, got {second.shape}")
    else:
        scalar = _number(duty, "duty", "square")
    c = x.context(ctx)
    out = x.result(c, np.int32)
    _lib.check(_lib.load().nxsig_square(c.handle, x.ptr, x.is_f64, x.n, scalar, second.ptr if second is not None else None, _ptr(out), x.mem))
    return out


def gaussian_pulse(t, ctx=None, **opts):
    """Waveforms.gaussian_pulse/2 — waveforms.ex:161-198.  {"envelope", "in_phase", "quadrature"}: exp(-a t^2) and its products with
    cos / sin(2 pi() fc t); options center_frequency (1000), bandwidth (0.5), bandwidth_reference_level (-6).  One pass over t writes
    the three tensors."""
    o = _options(opts, {"center_frequency": 1000, "bandwidth": 0.5, "bandwidth_reference_level": -6}, "gaussian_pulse")
    fc = _number(o["center_frequency"], "center_frequency", "gaussian_pulse")
    bw = _number(o["bandwidth"], "bandwidth", "gaussian_pulse")
    bwr = _number(o["bandwidth_reference_level"], "bandwidth_reference_level", "gaussian_pulse")
    if not fc >= 0:   # :173-186
        raise ArgumentError(f"Center frequency must be greater than or equal to 0, got: {o['center_frequency']!r}")
    if not bw > 0:
        raise ArgumentError(f"Bandwidth must be greater than 0, got: {o['bandwidth']!r}")
    if not bwr < 0:
        raise ArgumentError(f"Bandwidth reference level must be less than 0, got: {o['bandwidth_reference_level']!r}")
    x = _Tensor(t, "gaussian_pulse")
    c = x.context(ctx)
    env, yi, yq = x.result(c), x.result(c), x.result(c)
    _lib.check(_lib.load().nxsig_gaussian_pulse(c.handle, x.ptr, x.is_f64, x.n, fc, bw, bwr, _ptr(env), _ptr(yi), _ptr(yq), x.mem))
    return {"envelope": env, "in_phase": yi, "quadrature": yq}


def chirp(t, f0, t1, f1, ctx=None, **opts):
    """Waveforms.chirp/5 — waveforms.ex:249-300.  cos(phase(t) + phi) sweeping from f0 at 0 to f1 at t1; options phi (0), vertex_zero
    (True; :quadratic only), method "linear" (default), "quadratic", "logarithmic" or "hyperbolic".  :logarithmic with f0 f1 <= 0 is
    NaN everywhere, as in the reference."""
    o = _options(opts, {"phi": 0, "vertex_zero": True, "method": "linear"}, "chirp")
    method = o["method"]
    if not isinstance(method, str) or method not in _METHODS:   # :291-300
        raise ArgumentError(f"invalid method, must be one of [:linear, :quadratic, :logarithmic, :hyperbolic], got: {method!r}")
    f0, t1, f1 = _number(f0, "f0", "chirp"), _number(t1, "t1", "chirp"), _number(f1, "f1", "chirp")
    phi = _number(o["phi"], "phi", "chirp")
    x = _Tensor(t, "chirp")
    c = x.context(ctx)
    out = x.result(c)
    _lib.check(_lib.load().nxsig_chirp(c.handle, x.ptr, x.is_f64, x.n, f0, t1, f1, _METHODS[method], int(bool(o["vertex_zero"])), phi, _ptr(out),
                                       x.mem))
    return out


def polynomial_sweep(t, coefs, ctx=None, **opts):
    """Waveforms.polynomial_sweep/3 — waveforms.ex:343-361.  cos(2 pi() phase(t) + phi) with the instantaneous frequency the polynomial
    coefs (rank 1, highest power first, 1 to 32 entries, a host value); t is rank 1; options phi (0) and phi_unit "radians" (default)
    or "degrees".  The dot product of the integrated coefficients with the powers of t is summed in f64 and rounded once, which is what
    a BinaryBackend dot does; the reference's literals do not tell that from f32 sequential accumulation."""
    o = _options(opts, {"phi": 0, "phi_unit": "radians"}, "polynomial_sweep")
    if o["phi_unit"] not in ("radians", "degrees"):   # the case at :354-358 has no other clause
        raise ArgumentError(f"polynomial_sweep: phi_unit must be :radians or :degrees, got: {o['phi_unit']!r}")
    phi = _number(o["phi"], "phi", "polynomial_sweep")
    if is_device(coefs):
        raise ArgumentError("polynomial_sweep: coefs must be a host tensor")
    cf = np.asarray(coefs)
    if cf.ndim != 1 or cf.dtype.kind not in "fiub":   # {n} = Nx.shape(coefs)
        raise ArgumentError(f"polynomial_sweep: coefs must be a real tensor of rank 1, got shape {cf.shape}")
    if not 1 <= cf.size <= _lib.SWEEP_MAX_COEFS:
        raise ArgumentError(f"polynomial_sweep: coefs must have 1 to {_lib.SWEEP_MAX_COEFS} entries, got {cf.size}")
    x = _Tensor(t, "polynomial_sweep")
    if len(x.shape) != 1:   # ":assumes t is of shape {m}" (:346)
        raise ArgumentError(f"polynomial_sweep: t must have rank 1, got shape {x.shape}")
    cd = (C.c_double * cf.size)(*[float(v) for v in cf])
    c = x.context(ctx)
    out = x.result(c)
    _lib.check(_lib.load().nxsig_polynomial_sweep(c.handle, x.ptr, x.is_f64, x.n, cd, cf.size, phi, int(o["phi_unit"] == "degrees"), _ptr(out),
                                                  x.mem))
    return out


def unit_impulse(shape, ctx=None, device=False, **opts):
    """Waveforms.unit_impulse/2 — waveforms.ex:406-437.  Zeros of `shape` (a tuple, rank <= 8) with a one at `index`: a number (rank-1
    shapes), a list / tensor of rank entries (reshaped to {rank}), or "midpoint" (dim // 2 per axis); default 0.  type (default
    "f32") is "f32", "f64", "s32", "s64", "u32", "u64" or the matching numpy type; narrower types raise ArgumentError.  device=True
    returns a device tensor.  A shape with an empty dimension gives an empty tensor.  Deliberate deviation: an index outside the
    shape raises ArgumentError here; what the reference's Nx.indexed_put does with it is left to Nx."""
    o = _options(opts, {"index": 0, "type": "f32"}, "unit_impulse")
    if isinstance(shape, (int, np.integer)) and not isinstance(shape, bool):
        shape = (int(shape),)
    if not isinstance(shape, (tuple, list)) or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 for n in shape):
        raise ArgumentError(f"unit_impulse: shape must be a tuple of non-negative integers, got: {shape!r}")
    shape = tuple(int(n) for n in shape)
    rank = len(shape)
    if rank > 8:
        raise ArgumentError(f"unit_impulse: rank must be at most 8, got {rank}")
    ty = o["type"]
    try:
        dtype = np.dtype(_TYPES[ty] if isinstance(ty, str) else ty)
    except (KeyError, TypeError):
        raise ArgumentError(f"unit_impulse: unknown type {ty!r}") from None
    if dtype not in _DT:
        raise ArgumentError(f"unit_impulse: type must be one of {list(_TYPES)}, got {dtype}")
    index = o["index"]
    if isinstance(index, str):
        if index != "midpoint":
            raise ArgumentError(f"unit_impulse: index must be a number, a tensor of {rank} entries or :midpoint, got: {index!r}")
        idx = [n // 2 for n in shape]
    else:
        a = np.asarray(index)
        if a.dtype.kind not in "iu" or a.size != rank:   # Nx.reshape(index, {rank})
            raise ArgumentError(f"unit_impulse: index must hold {rank} integers for shape {shape}, got: {index!r}")
        idx = [int(v) for v in a.reshape(rank)]
    empty = 0 in shape
    if not empty:
        for d, (i, n) in enumerate(zip(idx, shape)):
            if not 0 <= i < n:
                raise ArgumentError(f"unit_impulse: index {i} is out of range for axis {d} of size {n}")
    if empty and not device:
        return np.zeros(shape, dtype)
    c = ctx or default_context()
    out = DeviceBuffer.empty(c, shape, dtype) if device else np.empty(shape, dtype)
    sh = (C.c_int64 * max(rank, 1))(*shape)
    ix = (C.c_int64 * max(rank, 1))(*idx)
    _lib.check(_lib.load().nxsig_unit_impulse(c.handle, _DT[dtype], sh, rank, ix, _ptr(out), _lib.DEVICE if device else _lib.HOST))
    return out
