"""Transforms.dct / idct and mfcc (extensions: scipy.fft 1.15's cosine transforms of type 2 and 3), on the kernels
of csrc/kernels_dct.hip.  Reached as nx_signal_amd.transforms.dct / idct and nx_signal_amd.mfcc."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr, rows_last, validate

# nxsig_dct_norm of include/nxsig.h
_NORMS = {None: 0, "backward": 0, "ortho": 1, "forward": 2}
_INVERSE_NORM = {None: "forward", "backward": "forward", "ortho": "ortho", "forward": None}


def _integer(v, what, fn):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ArgumentError(f"{fn}: {what} must be an integer, got: {v!r}")
    return int(v)


def _run(fn, x, type, n, axis, norm, ctx, keep):
    type = _integer(type, "type", fn)
    if type in (1, 4):
        raise NxSignalUnsupported(f"{fn}: unsupported type {type}: the cosine transforms of type 2 and 3 are built")
    if type not in (2, 3):
        raise ArgumentError(f"{fn}: type must be 2 or 3 (1 and 4 are not built), got: {type!r}")
    if not (norm is None or isinstance(norm, str)) or norm not in _NORMS:
        raise ArgumentError(f"{fn}: norm must be None, 'backward', 'ortho' or 'forward', got: {norm!r}")
    if n is not None and _integer(n, "n", fn) < 1:
        raise ArgumentError(f"{fn}: n must be positive, got: {n!r}")
    if keep is not None and _integer(keep, "keep", fn) < 1:
        raise ArgumentError(f"{fn}: keep must be in [1, n], got: {keep!r}")
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
    from .filters import _axis_last   # here, not at the top: the package imports either module first
    axis = _axis_last(xo, axis, fn, NxSignalUnsupported(f"{fn}: unsupported axis: device tensors are transformed along their last axis only"))
    batch, length = rows_last(xo.shape)
    n = length if n is None else int(n)
    keep = n if keep is None else int(keep)
    if keep > n:
        raise ArgumentError(f"{fn}: keep must be in [1, n], got: {keep!r} with n = {n}")
    if n >= 1 << 31:
        raise NxSignalUnsupported(f"{fn}: unsupported n: rows of fewer than 2^31 points are built, got {n}")
    c = xo.context(ctx, caller_first=False)
    out = xo.result(xo.shape[:-1] + (keep,), np.float32)
    _lib.check(_lib.load().nxsig_dct_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), xo.ptr, length, batch, length, n, type, _NORMS[norm], keep,
                                         ptr(out), xo.mem))
    return out if xo.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))


def dct(x, type=2, n=None, axis=-1, norm=None, ctx=None, keep=None, **opts):
    """scipy.fft.dct(x, type, n, axis, norm) on the GPU, types 2 and 3: every line of x along `axis` is truncated or zero-padded to n
    points (default: its length) and transformed (include/nxsig.h states the definition; norm None / "backward", "ortho", "forward" as
    SciPy's).  keep=m (the one extension) computes and returns only the leading m coefficients, 1 <= m <= n, with the bits of the full
    result's leading slice.  Types 1 and 4 are unsupported; orthogonalize=, overwrite_x= and workers= are not offered.  Real f32
    tensors; host integer and narrower float arrays are computed as f32; f64 rows are unsupported.  Host arrays: any axis, numpy out; a
    device tensor: the last axis only, a DeviceBuffer out, and the call does not wait.  A line that holds an Inf / NaN among the samples
    used has no finite output; the other lines keep theirs."""
    validate(opts, ("type", "n", "axis", "norm", "ctx", "keep"), "dct")
    return _run("dct", x, type, n, axis, norm, ctx, keep)


def idct(x, type=2, n=None, axis=-1, norm=None, ctx=None, **opts):
    """scipy.fft.idct(x, type, n, axis, norm) on the GPU: the transform of the other type (2 <-> 3) with norm None / "backward" and
    "forward" exchanged and "ortho" kept, so idct(dct(x, type=t, norm=m), type=t, norm=m) returns x.  Operands as dct's."""
    validate(opts, ("type", "n", "axis", "norm", "ctx"), "idct")
    t = _integer(type, "type", "idct")
    if not (norm is None or isinstance(norm, str)) or norm not in _NORMS:
        raise ArgumentError(f"idct: norm must be None, 'backward', 'ortho' or 'forward', got: {norm!r}")
    return _run("idct", x, 5 - t if t in (2, 3) else t, n, axis, _INVERSE_NORM[norm], ctx, None)


def mfcc(data, window, ctx=None, n_mfcc=20, **opts):
    """Mel-frequency cepstral coefficients: transforms.dct(mel_spectrogram(data, window, ...), type=2, norm="ortho", keep=n_mfcc), to
    the bit, as f32[..., frames, n_mfcc].  Takes exactly the options of mel_spectrogram plus n_mfcc, 1 <= n_mfcc <= mel_bins.  The
    cepstrum is taken of the reference's stft_to_mel output — its log10 of the mel energies, the clamp 8 below the maximum and
    the (x + 4) / 4 rescaling — not of librosa's dB scale, so the numbers differ from librosa.feature.mfcc by more than a factor.  A host
    array is uploaded once and the result downloaded once; the log-mel tensor never visits the host."""
    from . import _resolve_stft_opts, mel_spectrogram
    from .device import default_context
    n_mfcc = _integer(n_mfcc, "n_mfcc", "mfcc")
    mel_bins = _integer(opts.get("mel_bins", 128), "mel_bins", "mfcc")
    if not 1 <= n_mfcc <= mel_bins:
        raise ArgumentError(f"mfcc: n_mfcc must be in [1, mel_bins], got: {n_mfcc!r} with mel_bins = {mel_bins}")
    # the option errors of mel_spectrogram, under this function's name and before anything is uploaded
    _resolve_stft_opts(window, {k: v for k, v in opts.items() if k not in ("mel_bins", "max_mel", "mel_frequency_spacing")}, "mfcc")
    op = Operand(data)
    if op.device:
        return dct(mel_spectrogram(data, window, ctx, **opts), type=2, norm="ortho", keep=n_mfcc)
    if op.dtype != np.float32 and op.dtype.kind not in "iub":   # mel_spectrogram's own refusal, before anything is uploaded
        return mel_spectrogram(data, window, ctx, **opts)
    c = ctx or default_context()
    mel = mel_spectrogram(c.to_device(op.cast(np.float32).host), window, c, **opts)
    return dct(mel, type=2, norm="ortho", keep=n_mfcc).numpy()
