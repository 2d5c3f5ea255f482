"""Transforms.mdct / imdct / mdct_window (extensions: the lapped cosine transform of audio coding), on the
kernels of csrc/kernels_mdct.hip.  Reached as nx_signal_amd.transforms.mdct, imdct and mdct_window."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last, validate

# NXSIG_MDCT_NORM_* of include/nxsig.h
_NORMS = {None: 0, "ortho": 1}


def _operand(x, fn, what):
    xo = Operand(_as_tensor(x), any_dtype=True)
    if xo.dtype.kind == "c":
        raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 rows are built")
    if xo.dtype != np.dtype(np.float32):
        if xo.dtype == np.dtype(np.float64):
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: real f32 rows are built")
        if xo.device:
            raise NxSignalUnsupported(f"{fn}: unsupported type {xo.dtype}: device tensors must be f32")
        if xo.dtype.kind not in "biuf":
            raise ArgumentError(f"{fn}: unsupported type {xo.dtype}")
        xo.cast(np.float32)
    else:
        xo.cast()
    if len(xo.shape) < what:
        raise ArgumentError(f"{fn}: expected a tensor of rank >= {what}, got shape {tuple(xo.shape)}")
    return xo


def _options(fn, window, pad_edges, norm):
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float32))
    if w.ndim != 1 or w.size < 4 or w.size % 4:
        raise ArgumentError(f"{fn}: window must be a vector whose length, the frame length, is a positive multiple of 4, got shape {w.shape}")
    if not isinstance(pad_edges, (bool, np.bool_)):
        raise ArgumentError(f"{fn}: pad_edges must be a boolean, got: {pad_edges!r}")
    if not (norm is None or isinstance(norm, str)) or norm not in _NORMS:
        raise ArgumentError(f"{fn}: norm must be None or 'ortho', got: {norm!r}")
    return w, int(pad_edges), _NORMS[norm]


def mdct(x, window, ctx=None, pad_edges=False, norm=None, **opts):
    """The MDCT of every row of x (last axis): frames of N = len(window) = 2 M samples, hop M, M real coefficients per frame, as
    f32[..., F, M] (include/nxsig.h states the definition).  pad_edges=False: F = (L - N) // M + 1, a ragged tail is dropped and L >= N;
    pad_edges=True: the row counts as M zeros, the row and zeros up to a whole frame, F = ceil(L / M) + 1, so that every sample lies
    under two frames.  norm None applies no factor, "ortho" sqrt(2 / M).  Real f32 tensors; host integer and narrower float arrays
    are computed as f32; f64 and complex rows are unsupported.  A host array gives a numpy array; a device tensor a DeviceBuffer, and
    the call does not wait.  An Inf / NaN sample makes exactly the frames that cover it non-finite."""
    fn = "mdct"
    validate(opts, ("ctx", "pad_edges", "norm"), fn)
    w, pad, nrm = _options(fn, window, pad_edges, norm)
    xo = _operand(x, fn, 1)
    batch, length = rows_last(xo.shape)
    N = w.size
    if length < 1 or (not pad and length < N):
        raise ArgumentError(f"{fn}: rows of {length} samples are shorter than the frame length {N}; pad_edges=True takes them")
    frames = int(_lib.load().nxsig_mdct_frames(length, N, pad))
    if frames < 0:
        _lib.check(frames)
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-1] + (frames, N // 2), np.float32)
    _lib.check(_lib.load().nxsig_mdct_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, length, batch, length, ptr(w), N, pad, nrm, ptr(out), xo.mem))
    return out


def imdct(X, window, ctx=None, pad_edges=False, norm=None, length=None, **opts):
    """The inverse MDCT of f32[..., F, M] coefficient frames: every frame's N = 2 M windowed samples overlap-added at hop M, as
    f32[..., samples].  pad_edges=False returns (F + 1) M samples; pad_edges=True the `length` (default (F - 1) M, at most F M)
    samples after the first M, so imdct(mdct(x, w, pad_edges=True), w, pad_edges=True, length=L) is x under a Princen-Bradley window
    (mdct_window).  norm None applies 2 / M, "ortho" sqrt(2 / M).  Operands as mdct's.  An Inf / NaN coefficient of frame m makes
    exactly the output samples [m M, m M + N) non-finite."""
    fn = "imdct"
    validate(opts, ("ctx", "pad_edges", "norm", "length"), fn)
    w, pad, nrm = _options(fn, window, pad_edges, norm)
    xo = _operand(X, fn, 2)
    N = w.size
    frames, M = int(xo.shape[-2]), int(xo.shape[-1])
    if 2 * M != N:
        raise ArgumentError(f"{fn}: frames of {M} coefficients need a window of {2 * M} samples, got {N}")
    if frames < 1:
        raise ArgumentError(f"{fn}: expected at least one frame, got shape {tuple(xo.shape)}")
    if length is not None:
        if isinstance(length, (bool, np.bool_)) or not isinstance(length, (int, np.integer)):
            raise ArgumentError(f"{fn}: length must be an integer, got: {length!r}")
        if not pad and int(length) != (frames + 1) * M:
            raise ArgumentError(f"{fn}: length is an option of pad_edges=True; without it the result has (F + 1) M = {(frames + 1) * M} samples")
        if not 1 <= int(length) <= frames * M:
            raise ArgumentError(f"{fn}: length must be in [1, F M = {frames * M}], got: {length!r}")
    n_out = int(length) if length is not None else ((frames - 1) * M if pad else (frames + 1) * M)
    if n_out < 1:
        raise ArgumentError(f"{fn}: pad_edges=True needs at least two frames, or a length")
    batch = int(np.prod(xo.shape[:-2], dtype=np.int64))
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-2] + (n_out,), np.float32)
    _lib.check(_lib.load().nxsig_imdct_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, frames, batch, ptr(w), N, pad, nrm, ptr(out), n_out, xo.mem))
    return out


def mdct_window(kind, frame_length, alpha=4.0):
    """A Princen-Bradley window of frame_length = 2 M samples (w[n]^2 + w[n + M]^2 = 1), formed in double and rounded once to f32:
    "sine" sin(pi (n + 1/2) / N); "vorbis" sin(pi / 2 sin^2(pi (n + 1/2) / N)); "kbd" the Kaiser-Bessel-derived window of
    scipy.signal.windows.kaiser_bessel_derived with beta = pi alpha."""
    fn = "mdct_window"
    if isinstance(frame_length, (bool, np.bool_)) or not isinstance(frame_length, (int, np.integer)) or frame_length < 4 or frame_length % 4:
        raise ArgumentError(f"{fn}: frame_length must be a positive multiple of 4, got: {frame_length!r}")
    N = int(frame_length)
    s = np.sin(np.pi * (np.arange(N, dtype=np.float64) + 0.5) / N)
    if kind == "sine":
        w = s
    elif kind == "vorbis":
        w = np.sin(0.5 * np.pi * s * s)
    elif kind == "kbd":
        if not np.isfinite(alpha) or alpha < 0:
            raise ArgumentError(f"{fn}: alpha must be finite and >= 0, got: {alpha!r}")
        k = np.kaiser(N // 2 + 1, np.pi * float(alpha))
        half = np.sqrt(np.cumsum(k[:-1]) / np.sum(k))
        w = np.concatenate([half, half[::-1]])
    else:
        raise ArgumentError(f"{fn}: kind must be 'sine', 'vorbis' or 'kbd', got: {kind!r}")
    return w.astype(np.float32)
