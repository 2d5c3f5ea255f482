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
from . import device as _device
from ._marshal import Operand, _as_tensor, is_device, ptr, validate

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
        _lib.check(_lib.load().nxsig_sinc_f64(ptr(a), a.size, ptr(out)))
        return out
    a = np.ascontiguousarray(np.asarray(t, dtype=np.float32))
    out = np.empty_like(a)
    _lib.check(_lib.load().nxsig_sinc_f32(ptr(a), a.size, ptr(out)))
    return out


def _number(v, what, fn):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ArgumentError(f"{fn}: {what} must be a number, got: {v!r}")
    return float(v)


def _operand(t, fn, like=None):
    """t (or a second stream in the type of `like`) as the kernels take it: f32 or f64, integers as f32 -> (operand, elements, is_f64)"""
    x = Operand(_as_tensor(t))
    if x.device:
        if x.dtype not in (np.float32, np.float64):
            raise ArgumentError(f"{fn}: device tensors must be f32 or f64, got {x.dtype}")
    else:
        if x.dtype.kind == "c":
            raise ArgumentError(f"{fn}: complex tensors are not supported")
        if x.dtype.kind not in "fiub":
            raise ArgumentError(f"{fn}: unsupported type {x.dtype}")
        # integers become f32, as in an Nx binary op with the f32 pi()
        x.cast(like.dtype if like is not None else (np.float64 if x.dtype == np.float64 else np.float32))
    return x, math.prod(x.shape), int(x.dtype == np.float64)


def sawtooth(t, ctx=None, **opts):
    """Waveforms.sawtooth/2 — waveforms.ex:29-54.  Period 2 pi(), rising from -1 to 1 over [0, 2 pi() width] and falling back over
    the rest; width (default 1) in [0, 1].  Nx.remainder is C fmod: a negative t keeps its sign, as in the reference."""
    o = validate(opts, {"width": 1}, "sawtooth")
    width = _number(o["width"], "width", "sawtooth")
    if not 0 <= width <= 1:   # :34-36
        raise ArgumentError(f"width must be between 0 and 1, inclusive. Got: {o['width']!r}")
    x, n, is_f64 = _operand(t, "sawtooth")
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, x.dtype)
    _lib.check(_lib.load().nxsig_sawtooth(c.handle, x.ptr, is_f64, n, width, ptr(out), x.mem))
    return out


def square(t, ctx=None, **opts):
    """Waveforms.square/2 — waveforms.ex:96-104.  1 where fmod(t, 2 pi()) < duty * 2 * pi(), else -1, as int32.  duty (default 0.5)
    is a number or a tensor of t's shape that lives where t lives; it is read in t's type."""
    o = validate(opts, {"duty": 0.5}, "square")
    duty = o["duty"]
    x, n, is_f64 = _operand(t, "square")
    scalar, second = 0.0, None
    if is_device(duty) or isinstance(duty, (np.ndarray, list, tuple)):
        second = _operand(duty, "square", like=x)[0]
        if second.device != x.device:
            raise ArgumentError("square: t and duty must both be host tensors or both be device tensors")
        if second.dtype != x.dtype:
            raise ArgumentError(f"square: duty must have t's type {x.dtype}, got {second.dtype}")
        if second.shape != x.shape:
            raise ArgumentError(f"square: duty must have t's shape {x.shape}, got {second.shape}")
    else:
        scalar = _number(duty, "duty", "square")
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, np.int32)
    _lib.check(_lib.load().nxsig_square(c.handle, x.ptr, is_f64, n, scalar, second.ptr if second is not None else None, ptr(out), x.mem))
    return out


def gaussian_pulse(t, ctx=None, **opts):
    """Waveforms.gaussian_pulse/2 — waveforms.ex:161-198.  {"envelope", "in_phase", "quadrature"}: exp(-a t^2) and its products with
    cos / sin(2 pi() fc t); options center_frequency (1000), bandwidth (0.5), bandwidth_reference_level (-6).  One pass over t writes
    the three tensors."""
    o = validate(opts, {"center_frequency": 1000, "bandwidth": 0.5, "bandwidth_reference_level": -6}, "gaussian_pulse")
    fc = _number(o["center_frequency"], "center_frequency", "gaussian_pulse")
    bw = _number(o["bandwidth"], "bandwidth", "gaussian_pulse")
    bwr = _number(o["bandwidth_reference_level"], "bandwidth_reference_level", "gaussian_pulse")
    if not fc >= 0:   # :173-186
        raise ArgumentError(f"Center frequency must be greater than or equal to 0, got: {o['center_frequency']!r}")
    if not bw > 0:
        raise ArgumentError(f"Bandwidth must be greater than 0, got: {o['bandwidth']!r}")
    if not bwr < 0:
        raise ArgumentError(f"Bandwidth reference level must be less than 0, got: {o['bandwidth_reference_level']!r}")
    x, n, is_f64 = _operand(t, "gaussian_pulse")
    c = x.context(ctx, caller_first=False)
    env, yi, yq = (x.result(x.shape, x.dtype) for _ in range(3))
    _lib.check(_lib.load().nxsig_gaussian_pulse(c.handle, x.ptr, is_f64, n, fc, bw, bwr, ptr(env), ptr(yi), ptr(yq), x.mem))
    return {"envelope": env, "in_phase": yi, "quadrature": yq}


def chirp(t, f0, t1, f1, ctx=None, **opts):
    """Waveforms.chirp/5 — waveforms.ex:249-300.  cos(phase(t) + phi) sweeping from f0 at 0 to f1 at t1; options phi (0), vertex_zero
    (True; :quadratic only), method "linear" (default), "quadratic", "logarithmic" or "hyperbolic".  :logarithmic with f0 f1 <= 0 is
    NaN everywhere, as in the reference."""
    o = validate(opts, {"phi": 0, "vertex_zero": True, "method": "linear"}, "chirp")
    method = o["method"]
    if not isinstance(method, str) or method not in _METHODS:   # :291-300
        raise ArgumentError(f"invalid method, must be one of [:linear, :quadratic, :logarithmic, :hyperbolic], got: {method!r}")
    f0, t1, f1 = _number(f0, "f0", "chirp"), _number(t1, "t1", "chirp"), _number(f1, "f1", "chirp")
    phi = _number(o["phi"], "phi", "chirp")
    x, n, is_f64 = _operand(t, "chirp")
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, x.dtype)
    _lib.check(_lib.load().nxsig_chirp(c.handle, x.ptr, is_f64, n, f0, t1, f1, _METHODS[method], int(bool(o["vertex_zero"])), phi, ptr(out), x.mem))
    return out


def polynomial_sweep(t, coefs, ctx=None, **opts):
    """Waveforms.polynomial_sweep/3 — waveforms.ex:343-361.  cos(2 pi() phase(t) + phi) with the instantaneous frequency the polynomial
    coefs (rank 1, highest power first, 1 to 32 entries, a host value); t is rank 1; options phi (0) and phi_unit "radians" (default)
    or "degrees".  The dot product of the integrated coefficients with the powers of t is summed in f64 and rounded once, which is what
    a BinaryBackend dot does; the reference's literals do not tell that from f32 sequential accumulation."""
    o = validate(opts, {"phi": 0, "phi_unit": "radians"}, "polynomial_sweep")
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
    x, n, is_f64 = _operand(t, "polynomial_sweep")
    if len(x.shape) != 1:   # ":assumes t is of shape {m}" (:346)
        raise ArgumentError(f"polynomial_sweep: t must have rank 1, got shape {x.shape}")
    cd = (C.c_double * cf.size)(*[float(v) for v in cf])
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, x.dtype)
    _lib.check(_lib.load().nxsig_polynomial_sweep(c.handle, x.ptr, is_f64, n, cd, cf.size, phi, int(o["phi_unit"] == "degrees"), ptr(out), x.mem))
    return out


def unit_impulse(shape, ctx=None, device=False, **opts):
    """Waveforms.unit_impulse/2 — waveforms.ex:406-437.  Zeros of `shape` (a tuple, rank <= 8) with a one at `index`: a number (rank-1
    shapes), a list / tensor of rank entries (reshaped to {rank}), or "midpoint" (dim // 2 per axis); default 0.  type (default
    "f32") is "f32", "f64", "s32", "s64", "u32", "u64" or the matching numpy type; narrower types raise ArgumentError.  device=True
    returns a device tensor.  A shape with an empty dimension gives an empty tensor.  Deliberate deviation: an index outside the
    shape raises ArgumentError here; what the reference's Nx.indexed_put does with it is left to Nx."""
    o = validate(opts, {"index": 0, "type": "f32"}, "unit_impulse")
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
    c = ctx or _device.default_context()
    out = c.empty(shape, dtype) if device else np.empty(shape, dtype)
    sh = (C.c_int64 * max(rank, 1))(*shape)
    ix = (C.c_int64 * max(rank, 1))(*idx)
    _lib.check(_lib.load().nxsig_unit_impulse(c.handle, _DT[dtype], sh, rank, ix, ptr(out), _lib.DEVICE if device else _lib.HOST))
    return out
