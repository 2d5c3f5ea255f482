"""PeakFinding.find_peaks and trim (an extension: scipy.signal.find_peaks 1.15 on every line along an axis), on
the kernels of csrc/kernels_find_peaks.hip.  Both are reached as nx_signal_amd.peak_finding.find_peaks / .trim."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError
from ._marshal import Operand, _as_tensor, is_device, ptr, validate
from .device import DeviceBuffer
from .peak_finding import _DT, _check_shape

# ---- find_peaks: the bits of include/nxsig.h
_CONDITIONS = ("plateau_size", "height", "threshold", "distance", "prominence", "width")   # bit k of `conditions`, SciPy's order
_BOUNDED = ("plateau_size", "height", "threshold", "prominence", "width")                   # rows of `bounds`
_F64_PROPS = ("peak_heights", "left_thresholds", "right_thresholds", "prominences", "width_heights", "left_ips", "right_ips", "widths")
_S32_PROPS = ("left_bases", "right_bases", "left_edges", "right_edges", "plateau_sizes")
_RETURNS = {"plateau_size": ("plateau_sizes", "left_edges", "right_edges"), "height": ("peak_heights",),
            "threshold": ("left_thresholds", "right_thresholds"), "distance": (),
            "prominence": ("prominences", "left_bases", "right_bases"),
            "width": ("prominences", "left_bases", "right_bases", "widths", "width_heights", "left_ips", "right_ips")}
_FIND_PEAKS_OPTS = {"axis": -1, "height": None, "threshold": None, "distance": None, "prominence": None, "width": None, "wlen": None,
                    "rel_height": 0.5, "plateau_size": None, "max_peaks": None}


def _number(v, what):
    """a real scalar as a float; anything with a shape is an array-valued border, which this port does not take"""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        if np.ndim(v) > 0:
            raise ArgumentError(f"find_peaks: array-valued borders are not supported ({what}); give a number or a (min, max) pair")
        raise ArgumentError(f"find_peaks: {what} must be a number, got: {v!r}")
    if math.isnan(v):
        raise ArgumentError(f"find_peaks: {what} is not a number")
    return float(v)


def _border(name, v):
    """(min, max) of a condition given as a number (the minimum) or a pair; an open side is -inf / +inf"""
    lo, hi = v, None
    if isinstance(v, (tuple, list, np.ndarray)):
        if (np.ndim(v) != 1 if isinstance(v, np.ndarray) else False) or len(v) != 2:
            raise ArgumentError(f"find_peaks: array-valued borders are not supported ({name}); give a number or a (min, max) pair")
        lo, hi = v
    return (-math.inf if lo is None else _number(lo, name), math.inf if hi is None else _number(hi, name))


def find_peaks(x, ctx=None, **opts):
    """scipy.signal.find_peaks 1.15 on every line of x along `axis` (default -1): options height, threshold, distance, prominence,
    width, wlen, rel_height (0.5), plateau_size as SciPy's — each condition None, a number (the minimum) or a (min, max) pair whose
    sides may be None; array-valued borders are not supported — and max_peaks, which lowers the capacity of the result.

    Returns (peaks, properties): peaks = {"indices": s32 (capacity, rank), "valid_indices": u32} as argrelmax returns it (row-major
    order, then -1 rows; valid_indices is the true count even when max_peaks is smaller); properties maps each name SciPy would return
    to `capacity` entries in the same order (f64, or s32 axis coordinates for bases, edges and plateau sizes; NaN / -1 at and past
    valid_indices).  capacity = lines * ((n - 1) // 2) unless max_peaks lowers it.  Among equal heights the distance condition visits
    the larger index first (SciPy leaves ties to an unstable sort).  f32 and f64 run natively; host integers are widened to f64, host
    f16 to f32; device tensors must be f32 or f64.  Host input gives numpy arrays, device input DeviceBuffers (a call with a distance
    waits for its rounds, any other returns at once).  trim(peaks, properties) cuts a host result to valid_indices."""
    fn = "find_peaks"
    o = validate(opts, _FIND_PEAKS_OPTS, fn)
    axis = o["axis"]
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
        raise ArgumentError(f"{fn}: axis must be an integer, got: {axis!r}")
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype.kind == "c":
        raise ArgumentError(f"{fn}: complex tensors have no order")
    ax = _check_shape(xo.shape, int(axis), fn)
    if xo.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        if xo.device:
            raise ArgumentError(f"{fn}: device tensors must be f32 or f64, got {xo.dtype}")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32 if xo.dtype.kind == "f" and xo.dtype.itemsize < 4 else np.float64)
    else:
        xo.cast()
    given = [k for k in _CONDITIONS if o[k] is not None]
    bounds = np.empty((len(_BOUNDED), 2), np.float64)
    bounds[:, 0], bounds[:, 1] = -np.inf, np.inf
    for k in given:
        if k != "distance":
            bounds[_BOUNDED.index(k)] = _border(k, o[k])
    distance = 1.0
    if o["distance"] is not None:
        distance = _number(o["distance"], "distance")
        if distance < 1:
            raise ArgumentError(f"{fn}: `distance` must be greater or equal to 1")
    wlen = -1
    if o["wlen"] is not None:
        w = _number(o["wlen"], "wlen")
        if not 1 < w:
            raise ArgumentError(f"{fn}: `wlen` must be larger than 1, was {o['wlen']}")
        wlen = int(min(math.ceil(w), 1 << 62))
    rel_height = _number(o["rel_height"], "rel_height")
    if rel_height < 0:
        raise ArgumentError(f"{fn}: `rel_height` must be greater or equal to 0.0")
    shape, n = xo.shape, xo.shape[ax]
    capacity = (math.prod(shape) // n) * max(0, (n - 1) // 2)
    if o["max_peaks"] is not None:
        k = o["max_peaks"]
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ArgumentError(f"{fn}: max_peaks must be a positive integer, got: {k!r}")
        capacity = min(capacity, int(k))
    names = [p for k in given for p in _RETURNS[k]]
    fnames, inames = [p for p in _F64_PROPS if p in names], [p for p in _S32_PROPS if p in names]
    want = sum(1 << i for i, p in enumerate(_F64_PROPS + _S32_PROPS) if p in names)
    conditions = sum(1 << i for i, k in enumerate(_CONDITIONS) if k in given)
    c = xo.context(ctx, caller_first=False)
    indices, valid = xo.result((capacity, len(shape)), np.int32), xo.result((), np.uint32)
    fblock = xo.result((max(len(fnames), 1), capacity), np.float64)
    iblock = xo.result((max(len(inames), 1), capacity), np.int32)
    if not xo.device:
        valid[...] = 0
    sh = (C.c_int64 * len(shape))(*shape)
    _lib.check(_lib.load().nxsig_find_peaks(_lib.ctx_ptr(c.handle, _lib._ctx_peaks), xo.ptr, _DT[xo.dtype], sh, len(shape), ax,
                                            bounds.ctypes.data_as(C.POINTER(C.c_double)), conditions, distance, wlen, rel_height, capacity,
                                            want, ptr(indices), ptr(valid), ptr(fblock), ptr(iblock), xo.mem))

    def row(block, r):
        if not xo.device:
            return block[r]
        view = DeviceBuffer(c, block.ptr + r * capacity * block.dtype.itemsize, (capacity,), block.dtype, owner=False)
        view._keep = block
        return view

    props = {p: row(fblock, r) for r, p in enumerate(fnames)}
    props.update({p: row(iblock, r) for r, p in enumerate(inames)})
    return {"indices": indices, "valid_indices": valid}, {p: props[p] for p in dict.fromkeys(names)}


def trim(peaks, properties):
    """A host result of find_peaks cut to valid_indices (or to the capacity, when max_peaks was smaller): (indices, properties).  For a
    1-D input the indices are SciPy's 1-D array; otherwise the (count, rank) coordinates."""
    indices, valid = peaks["indices"], peaks["valid_indices"]
    if is_device(indices) or any(is_device(v) for v in properties.values()):
        raise ArgumentError("trim: takes host tensors (call .numpy() on the DeviceBuffers first)")
    indices = np.asarray(indices)
    k = min(int(valid), indices.shape[0])
    idx = indices[:k, 0].copy() if indices.shape[1] == 1 else indices[:k].copy()
    return idx, {name: np.asarray(v)[:k].copy() for name, v in properties.items()}
