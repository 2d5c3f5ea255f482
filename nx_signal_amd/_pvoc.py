"""Transforms.phase_vocoder / time_stretch (extensions: the time base of a spectrogram changed between stft and istft, DESIGN.md
section 3.24), on the kernels of csrc/kernels_pvoc.hip.  Reached as nx_signal_amd.transforms.phase_vocoder and time_stretch."""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, _as_tensor, ptr


def _rate(fn, rate):
    if isinstance(rate, (bool, np.bool_)) or not isinstance(rate, (int, float, np.integer, np.floating)) or not math.isfinite(rate) or not rate > 0:
        raise ArgumentError(f"{fn}: rate must be a finite real number > 0, got: {rate!r}")
    return float(rate)


def phase_vocoder(z, rate, ctx=None):
    """librosa.phase_vocoder / torchaudio.functional.phase_vocoder (transforms.TimeStretch) on a c64 spectrogram [..., M, K] as stft
    and stft_onesided return it: ceil(M / rate) frames c64[..., n_out, K] whose magnitudes are interpolated between the frames at
    t * rate and whose phases advance by the measured phase difference of those frames (include/nxsig.h states the definition;
    rate 2 plays twice as fast).  Bins are independent, so the full spectrum and K / 2 + 1 one-sided bins are served alike; the
    PACKED layout of stft_packed is not (its bin 0 carries two values).  There is no hop_length / phase_advance argument: the
    expected advance cancels modulo 2 pi, so the result is librosa's and torchaudio's for every hop.  c64 host arrays and device
    tensors of rank >= 2; c128 is unsupported.  A host array gives a numpy array; a device tensor a DeviceBuffer, and the call does
    not wait.  An Inf / NaN makes its bin non-finite from the first step that uses its frame."""
    fn = "phase_vocoder"
    r = _rate(fn, rate)
    zo = Operand(_as_tensor(z), any_dtype=True)
    if zo.dtype == np.dtype(np.complex128):
        raise NxSignalUnsupported(f"{fn}: unsupported type {zo.dtype}: c64 spectrograms are built")
    if zo.dtype != np.dtype(np.complex64):
        raise ArgumentError(f"{fn}: expected a complex64 spectrogram, got {zo.dtype}")
    zo.cast()
    if len(zo.shape) < 2 or zo.shape[-2] < 1 or zo.shape[-1] < 1:
        raise ArgumentError(f"{fn}: expected a tensor of shape (..., frames >= 1, bins >= 1), got shape {tuple(zo.shape)}")
    frames, bins = int(zo.shape[-2]), int(zo.shape[-1])
    batch = int(np.prod(zo.shape[:-2], dtype=np.int64))
    n_out = int(_lib.load().nxsig_pvoc_frames(frames, r))
    if n_out < 0:
        _lib.check(n_out)
    c = zo.context(ctx, caller_first=False)
    out = zo.result(zo.shape[:-2] + (n_out, bins), np.complex64)
    _lib.check(_lib.load().nxsig_phase_vocoder_c64(_lib.ctx_ptr(c.handle, _lib._ctx_iir), zo.ptr, batch, frames, bins, r, ptr(out), zo.mem))
    return out


def time_stretch(x, rate, window, ctx=None, **stft_opts):
    """librosa.effects.time_stretch: istft(phase_vocoder(stft(x, window, **stft_opts)[0], rate), window, **stft_opts) on one context
    (the options both stft and istft take: overlap_length, fft_length, scaling, sampling_rate).  For a device tensor every
    intermediate stays in HBM; the result is what istft returns."""
    from . import istft, stft
    _rate("time_stretch", rate)
    z = stft(x, window, ctx, **stft_opts)[0]
    ctx = ctx or getattr(z, "ctx", None)
    return istft(phase_vocoder(z, rate, ctx), window, ctx, **stft_opts)
