"""NxSignal.Transforms.fft_nd / ifft_nd — lib/nx_signal/transforms.ex:5-21: a fold of row FFTs over the listed axes
(the 1-axis case is how fftconvolve reaches Nx.fft; SURVEY §8f-4 for the multi-axis fold).  The whole fold runs in HBM
(nxsig_fft_nd: tiled transpose kernels bring an axis to the back and return it; four-step / Bluestein rows beyond the
LDS-resident sizes), for host tensors and for device-resident ones alike."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ArgumentError
from ._marshal import Operand, _as_tensor, ptr, rows_last, validate


def _run(tensor, inverse, opts, ctx):
    """Enum.zip_reduce(axes, lengths, tensor, &Nx.fft(&3, axis: &1, length: &2)) — transforms.ex:9-11 / :18-20"""
    validate(opts, ["axes", "lengths"], "fft_nd")
    axes = list(opts.get("axes", [-1]))
    lengths = opts.get("lengths") or [None] * len(axes)
    if len(lengths) != len(axes):
        raise ArgumentError("fft_nd: :axes and :lengths must have the same size")
    x = Operand(_as_tensor(tensor))   # Python numbers / lists follow Nx.tensor's inference (f32 / c64)
    if x.device:
        if x.dtype not in (np.float32, np.complex64):
            raise ArgumentError("fft_nd: device input must be float32 or complex64")
    else:
        if x.dtype in (np.float64, np.complex128):
            return _run_f64(x, inverse, axes, lengths, ctx)
        x.cast(np.complex64 if x.dtype.kind == "c" else np.float32)
    shape, is_real = x.shape, x.dtype == np.float32
    rank = len(shape)
    if rank == 0:
        raise ArgumentError("fft_nd: expected a tensor of rank >= 1")
    out_shape = list(shape)
    ax_n, len_n = [], []
    for axis, length in zip(axes, lengths):
        ax = int(axis)
        if ax < -rank or ax >= rank:
            raise ArgumentError(f"fft_nd: axis {axis} is out of bounds for a tensor of rank {rank}")
        ax %= rank
        K = int(length) if length is not None else out_shape[ax]
        if K < 1:
            raise ArgumentError("fft_nd: lengths must be positive")
        out_shape[ax] = K
        ax_n.append(ax)
        len_n.append(K)
    lib = _lib.load()
    sh = (C.c_int64 * rank)(*[int(s) for s in shape])
    axs = (C.c_int32 * max(len(ax_n), 1))(*ax_n)
    lns = (C.c_int64 * max(len(len_n), 1))(*len_n)
    c = x.context(ctx, caller_first=True)
    out = x.result(tuple(out_shape), np.complex64)
    _lib.check(lib.nxsig_fft_nd(c.handle, x.ptr, int(is_real), sh, rank, axs, lns, len(ax_n), int(inverse), ptr(out), x.mem))
    return out


def _run_f64(x, inverse, axes, lengths, ctx):
    """f64 tier (nxsig_fft_c128): Nx.fft / Nx.ifft in c128 over the LAST axis; other axes are not built in double"""
    rank = len(x.shape)
    if rank == 0:
        raise ArgumentError("fft_nd: expected a tensor of rank >= 1")
    if len(axes) != 1 or int(axes[0]) % rank != rank - 1:
        raise _lib.NxSignalUnsupported("fft_nd: f64 / c128 tensors are transformed over the last axis only")
    rows, n_in = rows_last(x.cast().shape)
    K = int(lengths[0]) if lengths[0] is not None else n_in
    if K < 1:
        raise ArgumentError("fft_nd: lengths must be positive")
    c = x.context(ctx, caller_first=True)
    out = x.result(x.shape[:-1] + (K,), np.complex128)
    _lib.check(_lib.load().nxsig_fft_c128(c.handle, x.ptr, int(x.dtype == np.float64), rows, n_in, K, int(inverse), ptr(out), x.mem))
    return out


def fft_nd(tensor, ctx=None, **opts):
    return _run(tensor, False, opts, ctx)


def ifft_nd(tensor, ctx=None, **opts):
    return _run(tensor, True, opts, ctx)


# dct / idct live in a module of their own (_dct.py) and are part of this one's interface
from ._dct import dct, idct  # noqa: E402,F401
# ... and so do czt / zoom_fft / czt_points (_czt.py)
from ._czt import czt, czt_points, zoom_fft  # noqa: E402,F401
# ... and so do cwt / morlet2 / ricker (_cwt.py)
from ._cwt import cwt, morlet2, ricker  # noqa: E402,F401
