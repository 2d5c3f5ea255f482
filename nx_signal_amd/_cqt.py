"""Spectral.cqt / vqt (an extension: constant-Q and variable-Q transforms, following librosa.cqt / librosa.vqt), on
the kernels of csrc/kernels_cqt.hip.  Reached as nx_signal_amd.spectral.cqt, vqt, cqt_frequencies and cqt_lengths."""
from __future__ import annotations

import functools
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last

KINDS = {"complex": 0, "magnitude": 1, "power": 2}


def _integer(v, what, least):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
        raise ArgumentError(f"cqt: {what} must be an integer >= {least}, got: {v!r}")
    return int(v)


def _number(v, what, positive=True):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or \
            (v <= 0 if positive else v < 0):
        raise ArgumentError(f"cqt: {what} must be a finite number {'> 0' if positive else '>= 0'}, got: {v!r}")
    return float(v)


def cqt_frequencies(n_bins, fmin, bins_per_octave=12):
    """f_k = fmin 2^(k / bins_per_octave), k = 0 ... n_bins - 1, f64"""
    n, B, f = _integer(n_bins, "n_bins", 1), _integer(bins_per_octave, "bins_per_octave", 1), _number(fmin, "fmin")
    return f * 2.0 ** (np.arange(n, dtype=np.float64) / B)


def cqt_lengths(sr, fmin, n_bins, bins_per_octave=12, filter_scale=1.0, gamma=0.0):
    """(l_k f64, lo_k s64, N_k s32) of the definition: l_k = filter_scale sr / (alpha f_k + gamma), alpha = 2^(1 / B) - 1; the kernel
    of bin k covers n = lo_k = floor(-l_k / 2) ... floor(l_k / 2) - 1, N_k samples.  f_k >= sr / 2 or N_k < 2 raise"""
    rate, q, gm = _number(sr, "sr"), _number(filter_scale, "filter_scale"), _number(gamma, "gamma", positive=False)
    f = cqt_frequencies(n_bins, fmin, bins_per_octave)
    if not f[-1] < rate / 2:
        raise ArgumentError(f"cqt: every bin must lie below sr / 2 = {rate / 2}, the last is at {f[-1]}")
    ell = q * rate / ((2.0 ** (1.0 / int(bins_per_octave)) - 1.0) * f + gm)
    lo, hi = np.floor(-ell / 2).astype(np.int64), np.floor(ell / 2).astype(np.int64) - 1
    count = hi - lo + 1
    if count.min() < 2:
        raise ArgumentError(f"cqt: every bin needs at least 2 samples, the shortest has {count.min()}: lower fmin + n_bins or raise filter_scale")
    if count.max() > 1 << 24:
        raise NxSignalUnsupported(f"cqt: a bin of at most 2^24 taps is built, got: {count.max()}")
    return ell, lo, count.astype(np.int32)


@functools.lru_cache(maxsize=8)
def _bank(sr, fmin, n_bins, bins_per_octave, filter_scale, norm, scale, gamma):
    """(lo s64, count s32, taps c64 concatenated): g_k conj(b_k), formed in double and rounded to f32 once"""
    ell, lo, count = cqt_lengths(sr, fmin, n_bins, bins_per_octave, filter_scale, gamma)
    f = cqt_frequencies(n_bins, fmin, bins_per_octave)
    taps = []
    for k in range(n_bins):
        N = int(count[k])
        b = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)) * np.exp(2j * np.pi * f[k] / sr * (lo[k] + np.arange(N, dtype=np.float64)))
        if norm == 1:
            b = b / np.abs(b).sum()
        elif norm == 2:
            b = b / math.sqrt((np.abs(b) ** 2).sum())
        taps.append(np.conj(b) * (math.sqrt(ell[k]) if scale else ell[k]))
    return lo, count, np.ascontiguousarray(np.concatenate(taps).astype(np.complex64))


def vqt(x, sr=22050, hop=512, fmin=32.703, n_bins=84, bins_per_octave=12, filter_scale=1.0, norm=1, scale=True, gamma=0.0,
        output="complex", ctx=None):
    """The variable-Q transform of every row, on the GPU, following librosa.vqt (window="hann", pad_mode="constant"): bin k is the
    correlation of the row with a Hann-windowed complex exponential at f_k = fmin 2^(k / bins_per_octave) of length l_k = filter_scale sr /
    (alpha f_k + gamma), centred at t hop, t = 0 ... len // hop (include/nxsig.h states the definition).  x: f32 host array or device
    tensor of rank >= 1, time on the last axis.  norm: 1, 2 or None; scale: multiply by sqrt(l_k) (else by l_k).  Returns c64[..., n_bins,
    F]; output="magnitude" / "power" give f32 |C| / |C|^2, formed before the one rounding.  The filters are evaluated directly, not by
    librosa's recursive downsampling: this follows librosa, it does not reproduce its approximation error.  An Inf / NaN sample makes
    exactly the outputs whose support holds it NaN.  f64 rows are unsupported.  A host array gives a numpy array; a device tensor a
    DeviceBuffer, and the call does not wait."""
    h, n_bins, B = _integer(hop, "hop", 1), _integer(n_bins, "n_bins", 1), _integer(bins_per_octave, "bins_per_octave", 1)
    if not (norm is None or (not isinstance(norm, (bool, np.bool_)) and isinstance(norm, (int, np.integer)) and norm in (1, 2))):
        raise ArgumentError(f"cqt: norm must be 1, 2 or None, got: {norm!r}")
    if not isinstance(scale, (bool, np.bool_)):
        raise ArgumentError(f"cqt: scale must be a boolean, got: {scale!r}")
    if not isinstance(output, str) or output not in KINDS:
        raise ArgumentError(f"cqt: output must be one of {list(KINDS)}, got: {output!r}")
    args = (_number(sr, "sr"), _number(fmin, "fmin"), n_bins, B, _number(filter_scale, "filter_scale"), None if norm is None else int(norm),
            bool(scale), _number(gamma, "gamma", positive=False))
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype == np.dtype(np.float64):
        raise NxSignalUnsupported("cqt: unsupported type float64: f32 rows are built")
    if xo.dtype != np.dtype(np.float32):
        raise ArgumentError(f"cqt: expected real f32 rows, got {xo.dtype}")
    if len(xo.shape) < 1 or xo.shape[-1] < 1:
        raise ArgumentError("cqt: expected a tensor of rank >= 1 with at least one sample per row")
    lo, count, taps = _bank(*args)
    xo.cast()
    batch, n = rows_last(xo.shape)
    lib = _lib.load()
    frames = int(lib.nxsig_cqt_frames(n, h))
    if frames < 0:
        _lib.check(frames)
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-1] + (n_bins, frames), np.complex64 if output == "complex" else np.float32)
    if batch:
        _lib.check(lib.nxsig_cqt_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, batch, n, n, h, n_bins, ptr(lo), ptr(count), ptr(taps),
                                     ptr(out), KINDS[output], xo.mem))
    return out


def cqt(x, sr=22050, hop=512, fmin=32.703, n_bins=84, bins_per_octave=12, filter_scale=1.0, norm=1, scale=True, output="complex", ctx=None):
    """The constant-Q transform of every row, following librosa.cqt: vqt with gamma = 0"""
    return vqt(x, sr, hop, fmin, n_bins, bins_per_octave, filter_scale, norm, scale, 0.0, output, ctx)
