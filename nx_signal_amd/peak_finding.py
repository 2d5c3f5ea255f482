"""NxSignal.PeakFinding: argrelmin/2, argrelmax/2, argrelextrema/3 (lib/nx_signal/peak_finding.ex) on the kernels of DESIGN.md
section 3.9.  Each returns {"indices": s32 (size, rank), "valid_indices": u32 scalar}: the coordinates of the marked elements in
row-major order, then -1 rows.  find_peaks (an extension: scipy.signal.find_peaks on every line along an axis)
returns the same pair for the surviving peaks and a dict of their properties; trim cuts both to valid_indices on the host."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError
from ._marshal import Operand, _as_tensor, is_device, ptr, validate

# native element types of the kernels; narrower ones are widened exactly before the call
_DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64, np.dtype(np.int32): _lib.DT_S32,
       np.dtype(np.int64): _lib.DT_S64, np.dtype(np.uint32): _lib.DT_U32, np.dtype(np.uint64): _lib.DT_U64}
_WIDEN = {"b": np.int32, "i": np.int32, "u": np.int32, "f": np.float32}
_CMP = {"less": _lib.CMP_LESS, "greater": _lib.CMP_GREATER, "less_equal": _lib.CMP_LESS_EQUAL, "greater_equal": _lib.CMP_GREATER_EQUAL}
_UFUNC = {np.less: "less", np.greater: "greater", np.less_equal: "less_equal", np.greater_equal: "greater_equal"}


def _axis_order(opts, fn):
    validate(opts, ["axis", "order"], fn)   # keyword!
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


def _compact(c, x, call):
    """{"indices", "valid_indices"} where operand x lives, filled by call(indices pointer, valid pointer)"""
    indices, valid = x.result((math.prod(x.shape), len(x.shape)), np.int32), x.result((), np.uint32)
    if not x.device:
        valid[...] = 0
    _lib.check(call(ptr(indices), ptr(valid)))
    return {"indices": indices, "valid_indices": valid}


def _fused(data, name, ctx, axis, order, fn):
    x = Operand(_as_tensor(data), any_dtype=True)
    ax = _check_shape(x.shape, axis, fn)
    if x.dtype.kind == "c":
        raise ArgumentError(f"{fn}: complex tensors have no order")
    if x.dtype not in _DT:
        if x.device:
            raise ArgumentError(f"{fn}: device tensors must be f32, f64, s32, s64, u32 or u64, got {x.dtype}")
        if x.dtype.kind not in _WIDEN:
            raise ArgumentError(f"{fn}: unsupported type {x.dtype}")
    x.cast(x.dtype if x.dtype in _DT else _WIDEN[x.dtype.kind])
    c = x.context(ctx, caller_first=False)
    lib, shape = _lib.load(), x.shape
    sh = (C.c_int64 * len(shape))(*shape)
    return _compact(c, x, lambda ip, vp: lib.nxsig_argrelextrema(c.handle, x.ptr, _DT[x.dtype], sh, len(shape), ax, _shifts(order), _CMP[name],
                                                                 ip, vp, x.mem))


def nonzero(mask, ctx=None):
    """The compaction step on its own: coordinates of the non-zero elements of a host mask (any rank 1 .. 8) in row-major order, then
    -1 rows, as argrelextrema returns them."""
    x = Operand(np.asarray(mask) != 0).cast(np.uint8)
    _check_shape(x.shape, 0, "nonzero")
    c = x.context(ctx, caller_first=True)
    sh = (C.c_int64 * len(x.shape))(*x.shape)
    return _compact(c, x, lambda ip, vp: _lib.load().nxsig_nonzero(c.handle, x.ptr, sh, len(x.shape), ip, vp, x.mem))


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
    axis, order = _axis_order(opts, "argrelextrema")
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
    axis, order = _axis_order(opts, "argrelmin")
    return _fused(data, "less", ctx, axis, order, "argrelmin")


def argrelmax(data, ctx=None, **opts):
    """PeakFinding.argrelmax/2: argrelextrema(data, "greater", ...)"""
    axis, order = _axis_order(opts, "argrelmax")
    return _fused(data, "greater", ctx, axis, order, "argrelmax")


# find_peaks / trim live in a module of their own (_find_peaks.py) and are part of this one's interface
from ._find_peaks import find_peaks, trim  # noqa: E402,F401
