"""NxSignal.PeakFinding: argrelmin/2, argrelmax/2, argrelextrema/3 (lib/nx_signal/peak_finding.ex) on the kernels of DESIGN.md
section 3.9.  Each returns {"indices": s32 (size, rank), "valid_indices": u32 scalar}: the coordinates of the marked elements in
row-major order, then -1 rows."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError
from .device import DeviceBuffer, default_context, is_device

# native element types of the kernels; narrower ones are widened exactly before the call
_DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64, np.dtype(np.int32): _lib.DT_S32,
       np.dtype(np.int64): _lib.DT_S64, np.dtype(np.uint32): _lib.DT_U32, np.dtype(np.uint64): _lib.DT_U64}
_WIDEN = {"b": np.int32, "i": np.int32, "u": np.int32, "f": np.float32}
_CMP = {"less": _lib.CMP_LESS, "greater": _lib.CMP_GREATER, "less_equal": _lib.CMP_LESS_EQUAL, "greater_equal": _lib.CMP_GREATER_EQUAL}
_UFUNC = {np.less: "less", np.greater: "greater", np.less_equal: "less_equal", np.greater_equal: "greater_equal"}


def _options(opts, fn):
    unknown = [k for k in opts if k not in ("axis", "order")]
    if unknown:   # keyword!
        raise ArgumentError(f"unknown keys {unknown} in {fn} options, the allowed keys are: ['axis', 'order']")
    axis, order = opts.get("axis", 0), opts.get("order", 1)
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
        raise ArgumentError(f"{fn}: axis must be an integer, got: {axis!r}")
    if isinstance(order, bool) or not isinstance(order, (int, float, np.integer, np.floating)) or math.isnan(order):
        raise ArgumentError(f"{fn}: order must be a number, got: {order!r}")
    return int(axis), order


def _shifts(order):
    """the number of shifts s = 1, 2, ... with s < order + 1"""
    return 0 if order <= 0 else (min(int(math.ceil(order)), 1 << 62) if math.isfinite(order) else 1 << 62)


def _check_shape(shape, axis, fn):
    rank = len(shape)
    if rank == 0:
        raise ArgumentError(f"{fn}: a rank-0 tensor has no axis")
    if rank > 8:
        raise ArgumentError(f"{fn}: rank must be at most 8, got {rank}")
    if not -rank <= axis < rank:
        raise ArgumentError(f"{fn}: axis {axis} is out of range for rank {rank}")
    if any(n < 1 for n in shape):
        raise ArgumentError(f"{fn}: empty dimension in shape {tuple(shape)}")
    if any(n >= 1 << 31 for n in shape):
        raise ArgumentError(f"{fn}: every dimension must be below 2^31")
    if math.prod(shape) >= 1 << 32:
        raise ArgumentError(f"{fn}: the tensor must have fewer than 2^32 elements")
    return axis % rank


def _device(t):
    """(ptr, shape, dtype, ctx or None) of a device input of any element type"""
    if isinstance(t, DeviceBuffer):
        return t.ptr, t.shape, t.dtype, t.ctx
    if hasattr(t, "__cuda_array_interface__"):
        cai = t.__cuda_array_interface__
        if cai.get("strides") is not None:
            raise ArgumentError("device inputs must be contiguous")
        return int(cai["data"][0]), tuple(cai["shape"]), np.dtype(cai["typestr"]), None
    if not t.is_contiguous():
        raise ArgumentError("device inputs must be contiguous")
    try:
        dt = np.dtype(str(t.dtype).replace("torch.", ""))
    except TypeError:
        raise ArgumentError(f"unsupported device dtype {t.dtype}") from None
    return int(t.data_ptr()), tuple(t.shape), dt, None


def _result(c, shape, dev):
    size, rank = math.prod(shape), len(shape)
    if dev:
        return DeviceBuffer.empty(c, (size, rank), np.int32), DeviceBuffer.empty(c, (), np.uint32)
    return np.empty((size, rank), np.int32), np.zeros((), np.uint32)


def _ptr(a):
    return C.c_void_p(a.ptr) if isinstance(a, DeviceBuffer) else a.ctypes.data_as(C.c_void_p)


def _fused(data, name, ctx, axis, order, fn):
    if is_device(data):
        ptr, shape, dtype, owner = _device(data)
        ax = _check_shape(shape, axis, fn)
        if dtype.kind == "c":
            raise ArgumentError(f"{fn}: complex tensors have no order")
        if dtype not in _DT:
            raise ArgumentError(f"{fn}: device tensors must be f32, f64, s32, s64, u32 or u64, got {dtype}")
        c = owner or ctx or default_context()
        mem, x = _lib.DEVICE, C.c_void_p(ptr)
    else:
        a = np.asarray(_as_tensor(data))
        shape = a.shape
        ax = _check_shape(shape, axis, fn)
        if a.dtype.kind == "c":
            raise ArgumentError(f"{fn}: complex tensors have no order")
        if a.dtype not in _DT:
            if a.dtype.kind not in _WIDEN:
                raise ArgumentError(f"{fn}: unsupported type {a.dtype}")
            a = a.astype(_WIDEN[a.dtype.kind])
        a = np.ascontiguousarray(a)
        dtype, c, mem, x = a.dtype, ctx or default_context(), _lib.HOST, a.ctypes.data_as(C.c_void_p)
    lib = _lib.load()
    indices, valid = _result(c, shape, mem == _lib.DEVICE)
    sh = (C.c_int64 * len(shape))(*shape)
    _lib.check(lib.nxsig_argrelextrema(c.handle, x, _DT[np.dtype(dtype)], sh, len(shape), ax, _shifts(order), _CMP[name], _ptr(indices),
                                       _ptr(valid), mem))
    return {"indices": indices, "valid_indices": valid}


def nonzero(mask, ctx=None):
    """The compaction step on its own: coordinates of the non-zero elements of a host mask (any rank 1 .. 8) in row-major order, then
    -1 rows, as argrelextrema returns them."""
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    _check_shape(m.shape, 0, "nonzero")
    c = ctx or default_context()
    indices, valid = _result(c, m.shape, False)
    sh = (C.c_int64 * m.ndim)(*m.shape)
    _lib.check(_lib.load().nxsig_nonzero(c.handle, m.ctypes.data_as(C.c_void_p), sh, m.ndim, _ptr(indices), _ptr(valid), _lib.HOST))
    return {"indices": indices, "valid_indices": valid}


def _custom(data, comparator, ctx, axis, order, fn):
    """A comparator that is not one of the four: the reference's loop on host arrays, comparator(data, shifted) and'ed into the mask,
    then nonzero on the device."""
    if is_device(data):
        raise ArgumentError(f"{fn}: a custom comparator needs a host tensor")
    a = np.asarray(_as_tensor(data))
    ax = _check_shape(a.shape, axis, fn)
    if a.dtype.kind == "c":
        raise ArgumentError(f"{fn}: complex tensors have no order")
    n = a.shape[ax]
    locs = np.arange(n)
    mask = np.ones(a.shape, bool)
    for s in range(1, min(_shifts(order), max(n - 1, 1)) + 1):
        plus = np.take(a, np.clip(locs + s, 0, n - 1), axis=ax)
        minus = np.take(a, np.clip(locs - s, 0, n - 1), axis=ax)
        mask &= np.asarray(comparator(a, plus)).astype(bool) & np.asarray(comparator(a, minus)).astype(bool)
        if not mask.any():
            break
    return nonzero(mask, ctx)


def argrelextrema(data, comparator, ctx=None, **opts):
    """PeakFinding.argrelextrema/3.  comparator: "less", "greater", "less_equal", "greater_equal" or the matching numpy ufunc (the
    fused kernels), or any callable comparator(x, y) -> boolean array (host tensors; the mask is compacted on the device).
    Options axis (default 0, negative counts from the end) and order (default 1; order <= 0 marks every element, as in the
    reference).  Host input gives numpy int32 (size, rank) and a 0-d uint32; device input gives DeviceBuffers."""
    axis, order = _options(opts, "argrelextrema")
    name = comparator if isinstance(comparator, str) else _UFUNC.get(comparator)
    if name is not None:
        if name not in _CMP:
            raise ArgumentError(f"argrelextrema: unknown comparator {comparator!r}")
        return _fused(data, name, ctx, axis, order, "argrelextrema")
    if not callable(comparator):
        raise ArgumentError(f"argrelextrema: comparator must be a name or a callable, got: {comparator!r}")
    return _custom(data, comparator, ctx, axis, order, "argrelextrema")


def argrelmin(data, ctx=None, **opts):
    """PeakFinding.argrelmin/2: argrelextrema(data, "less", ...)"""
    axis, order = _options(opts, "argrelmin")
    return _fused(data, "less", ctx, axis, order, "argrelmin")


def argrelmax(data, ctx=None, **opts):
    """PeakFinding.argrelmax/2: argrelextrema(data, "greater", ...)"""
    axis, order = _options(opts, "argrelmax")
    return _fused(data, "greater", ctx, axis, order, "argrelmax")


def _as_tensor(x):
    from . import _as_tensor as as_tensor
    return as_tensor(x)
