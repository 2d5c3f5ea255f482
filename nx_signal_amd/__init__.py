"""nx_signal_amd — MI355X-native STFT / iSTFT / FIR hot path behind the NxSignal API.

Python host mirror of the reference's function-level interface (elixir-nx/nx_signal v0.3.0):

    NxSignal.stft/3, istft/3, as_windowed/2, overlap_and_add/2, fft_frequencies/2   -> this module
    NxSignal.Windows.*            -> nx_signal_amd.windows
    NxSignal.Filters.firwin/3, median/2, wiener/2 -> nx_signal_amd.filters  (+ the new `fir`, `resample_poly`, `sosfilt`, `sosfilt_zi`, `sosfiltfilt`)
    NxSignal.PeakFinding.*        -> nx_signal_amd.peak_finding; (extension) welch / csd / coherence -> nx_signal_amd.spectral
    NxSignal.Convolution.*        -> nx_signal_amd.convolution (FFT method, 1-D)
    NxSignal.Waveforms.*          -> nx_signal_amd.waveforms (sinc/1 on the host)
    NxSignal.Transforms.fft_nd    -> nx_signal_amd.transforms (last axis)

Same option names, defaults, return shapes and failure cases (ArgumentError) as the reference; atoms
become strings ("valid", "reflect", "spectrum", ...), tensors become numpy arrays (host) or DeviceBuffers
(HBM-resident, returned when the input is device-resident).  All arithmetic runs in hand-written HIP
kernels behind the C ABI in include/nxsig.h; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import ArgumentError, NxSignalDeviceError, NxSignalLibraryError, NxSignalUnsupported, StftParams
from ._marshal import Operand, _as_tensor, is_device, ptr, rows_last, validate as _validate
from .device import Context, DeviceBuffer, default_context

__all__ = [
    "stft", "istft", "as_windowed", "overlap_and_add", "fft_frequencies", "mel_filters", "stft_to_mel", "mel_spectrogram", "mfcc",
    "spectrum_multiply", "istft_filtered", "spectrum_mask", "istft_masked", "stft_onesided", "spectrogram",
    "Context", "DeviceBuffer", "default_context", "ArgumentError",
    "NxSignalDeviceError", "NxSignalLibraryError", "NxSignalUnsupported",
]

_PAD_ATOMS = {"valid": _lib.PAD_VALID, "reflect": _lib.PAD_REFLECT, "same": _lib.PAD_SAME}
_SCALING = {None: _lib.SCALE_NONE, "spectrum": _lib.SCALE_SPECTRUM, "psd": _lib.SCALE_PSD}


def _host_f32(x: Operand, what: str) -> Operand:
    """the f32 entry points' rule for a host operand: f32 as it is, integers widened, anything else refused"""
    if x.dtype == np.float32 or x.dtype.kind in "iub":
        return x.cast(np.float32)
    if x.dtype == np.float64:
        raise ArgumentError(
            f"{what}: float64 input would produce an f64 / c128 result in the reference; this entry point computes f32 / c64 — "
            "cast to float32 explicitly (stft, istft, as_windowed, overlap_and_add, fft_nd over the last axis and 1-D fftconvolve "
            "take float64 / complex128 and compute in double)"
        )
    raise ArgumentError(f"{what}: unsupported dtype {x.dtype}")


def _window_host(window) -> np.ndarray:
    """the window as the host array handed to the library: f32, or f64 when the caller's is (the f64 tier, include/nxsig.h)"""
    w = np.asarray(window)
    if w.ndim != 1:
        raise ArgumentError(f"window must be a rank-1 tensor, got shape {w.shape}")
    if w.dtype == np.float64:
        return np.ascontiguousarray(w)
    return np.ascontiguousarray(w.astype(np.float32))


def _pad_args(padding, fn="as_windowed"):
    if isinstance(padding, str):
        if padding not in _PAD_ATOMS:  # lib/nx_signal.ex:325-329 (":zeros" and nil raise despite the docs, B2)
            raise ArgumentError(
                "invalid padding mode specified, padding must be one of :valid, :same, or a padding configuration, "
                f"got: {padding!r}"
            )
        return _PAD_ATOMS[padding], 0, 0
    if isinstance(padding, (list, tuple)):
        ok = len(padding) == 1 and len(padding[0]) == 2 and all(isinstance(v, (int, np.integer)) for v in padding[0])
        if not ok:  # :319-323
            raise ArgumentError(
                "padding must be a list of {high, low} tuples, where each element is an integer. " f"Got: {padding!r}"
            )
        return _lib.PAD_EXPLICIT, int(padding[0][0]), int(padding[0][1])
    raise ArgumentError(
        "invalid padding mode specified, padding must be one of :valid, :same, or a padding configuration, "
        f"got: {padding!r}"
    )


def _resolve_fft_length(fft_length, n: int) -> int:
    if fft_length in (None, "power_of_two"):
        return int(_lib.load().nxsig_next_pow2(int(n)))
    if isinstance(fft_length, (int, np.integer)) and fft_length >= 1:
        return int(fft_length)
    raise ArgumentError(f"expected :fft_length to be a positive integer or :power_of_two, got: {fft_length!r}")


# ------------------------------------------------------------------------------------------------
def fft_frequencies(sampling_rate, **opts):
    """NxSignal.fft_frequencies/2 — lib/nx_signal.ex:154-166."""
    o = _validate(opts, {"fft_length": None, "type": "f32", "name": "frequencies", "endpoint": False}, "fft_frequencies")
    if o["fft_length"] is None:
        raise ArgumentError("missing :fft_length option")
    K = int(o["fft_length"])
    f64 = o["type"] in ("f64", np.float64)
    if not f64 and o["type"] not in ("f32", np.float32):
        raise ArgumentError(f"fft_frequencies: type must be f32 or f64, got {o['type']!r}")
    out = np.empty(K, dtype=np.float64 if f64 else np.float32)
    entry = _lib.load().nxsig_fft_frequencies_f64 if f64 else _lib.load().nxsig_fft_frequencies_f32
    _lib.check(entry(float(sampling_rate), K, int(bool(o["endpoint"])), ptr(out)))
    return out


def as_windowed(tensor, ctx: Context | None = None, **opts):
    """NxSignal.as_windowed/2 — lib/nx_signal.ex:249-364.  (..., L) -> (..., M, window_length)."""
    o = _validate(opts, {"window_length": None, "padding": "valid", "stride": 1}, "as_windowed")
    if o["window_length"] is None:
        raise ArgumentError("missing :window_length option")
    stride = o["stride"]
    if not (isinstance(stride, (int, np.integer)) and stride >= 1):  # :282-284
        raise ArgumentError(f"expected an integer >= 1 or a list of integers, got: {stride!r}")
    mode, lo, hi = _pad_args(o["padding"])
    N = int(o["window_length"])
    lib = _lib.load()
    M = C.c_int64()
    x = Operand(_as_tensor(tensor))
    src_dtype = x.dtype
    ints = not x.device and x.dtype.kind in "iub"
    if x.device:
        if x.dtype not in (np.float32, np.float64):
            raise ArgumentError("as_windowed: device input must be float32 or float64")
    elif x.dtype == np.float64:   # f64 tier: 8-byte words through the same gather
        x.cast()
    elif ints:
        # framing is a pure gather (doctests :182-246 keep s64): 32-bit words travel through the kernel untouched, so integer
        # tensors stay EXACT (no rounding through f32); wider integers go through int32 when every value fits
        if x.host.size and (int(x.host.min()) < -2 ** 31 or int(x.host.max()) > 2 ** 31 - 1):
            raise ArgumentError("as_windowed: integer values beyond 32 bits are not supported by the MI355X path")
        x.cast(np.int32)
    else:
        _host_f32(x, "as_windowed")
    wide = x.dtype == np.float64
    c = x.context(ctx, caller_first=True)
    batch, L = rows_last(x.shape)
    m = _lib.check(lib.nxsig_num_frames(L, N, int(stride), mode, lo, hi))
    out = x.result(x.shape[:-1] + (m, N), np.float64 if wide else np.float32)
    entry = lib.nxsig_as_windowed_f64 if wide else lib.nxsig_as_windowed_f32
    _lib.check(entry(c.handle, x.ptr, L, batch, L, N, int(stride), mode, lo, hi, ptr(out), C.byref(M), x.mem))
    return out.view(np.int32).astype(src_dtype) if ints else out


_STFT_OPTS = {"overlap_length": None, "window": None, "scaling": None, "window_padding": "valid", "sampling_rate": 100,
              "fft_length": "power_of_two"}


def _resolve_stft_opts(window, opts, fn="stft"):
    """option parsing / defaults of NxSignal.stft/3 (lib/nx_signal.ex:71-85) -> (StftParams, N, hop, K); `fn` names the function in
    the unknown-key message (mel_spectrogram and spectrogram take the same options)"""
    o = _validate(opts, _STFT_OPTS, fn)
    w = _window_host(window)
    N = int(w.shape[0])
    if o["sampling_rate"] is None:
        raise ArgumentError("missing sampling_rate option")  # :81
    fs = float(o["sampling_rate"])
    overlap = N // 2 if o["overlap_length"] is None else int(o["overlap_length"])  # :83
    hop = N - overlap
    if o["scaling"] not in _SCALING:  # :124-126
        raise ArgumentError(f"invalid :scaling, expected one of :spectrum, :psd or nil, got: {o['scaling']!r}")
    mode, lo, hi = _pad_args(o["window_padding"])
    K = _resolve_fft_length(o["fft_length"], N)
    return StftParams(N, hop, K, mode, lo, hi, _SCALING[o["scaling"]], 0, fs), N, hop, K


def _frames(x: Operand, ctx, p):
    """what every framing call over the last axis of x needs -> (context, rows, row length, frames per row)"""
    c = x.context(ctx, caller_first=True)
    batch, L = rows_last(x.shape)
    m = _lib.check(_lib.load().nxsig_num_frames(L, p.frame_length, p.hop, p.pad_mode, p.pad_lo, p.pad_hi))
    return c, batch, L, m


def stft(data, window, ctx: Context | None = None, **opts):
    """NxSignal.stft/3 — lib/nx_signal.ex:68-130.  Returns (z c64[..., M, K], times f32[M], frequencies f32[K]).

    Defaults follow the code, not the doc: window_padding "valid", sampling_rate 100,
    fft_length "power_of_two", overlap_length div(N, 2); the :window key is accepted and ignored.

    Device-resident inputs (DeviceBuffer, torch tensors, __cuda_array_interface__ objects) return a DeviceBuffer and the call is
    ASYNCHRONOUS on the context's own HIP stream: it is ordered after earlier calls on the same context only.  Data produced
    on another stream (e.g. torch's current stream) must be complete before the call, and the result must not be consumed on
    another stream before `ctx.sync()` — or hand the library that stream with `ctx.set_stream(ptr)`.
    """
    return _stft(data, window, ctx, opts, False)


def stft_onesided(data, window, ctx: Context | None = None, **opts):
    """Extension (not in the reference API): `stft(data, window, **opts)` restricted to the bins 0 .. fft_length/2 - 1 — the slice
    the reference's own downstream code keeps for real signals (stft_to_mel, lib/nx_signal.ex:493-496; the spectrogram guide) —
    written straight from the transform (half the output traffic; the same bits as `stft(...)[0][..., :K // 2]`).
    Returns (z c64[..., M, K // 2], times f32[M], frequencies f32[K // 2])."""
    return _stft(data, window, ctx, opts, True)


def stft_packed(data, window, ctx: Context | None = None, **opts):
    """Extension (not in the reference API): the one-sided spectrum of `stft_onesided` with NOTHING of a real frame's spectrum
    lost — the imaginary part of bin 0 (zero for a real frame) carries Re X[fft_length / 2], the Nyquist bin.  The layout
    `istft_packed` inverts: together they run the reference's stft -> z * H -> istft chain (guides/filtering.livemd:137-159) at
    4 KB + 1 KB of HBM traffic per 1024-point frame instead of 8 + 2.  Returns (z c64[..., M, K // 2], times, frequencies[:K // 2])."""
    return _stft(data, window, ctx, opts, True, packed=True)


def istft_packed(data, window, ctx: Context | None = None, **opts):
    """Inverse of `stft_packed`: c64[..., M, K // 2] (packed) -> REAL f32[..., M * hop + overlap], equal to
    `istft(full Hermitian spectrum).real` to fp32 round-off.  Options as for `istft` (fft_length, if given, is the FULL length)."""
    return _istft(data, window, ctx, opts, None, packed=True)


def _stft(data, window, ctx, opts, onesided, packed=False):
    data, window = _as_tensor(data), _as_tensor(window)
    p, N, hop, K = _resolve_stft_opts(window, opts)
    w = _window_host(window)
    fs = float(p.sampling_rate)
    lib = _lib.load()
    M = C.c_int64()
    Kout = K // 2 if onesided else K
    if onesided and K < 2:
        raise ArgumentError("stft_onesided: fft_length >= 2 required")
    entry = lib.nxsig_stft_packed_f32 if packed else (lib.nxsig_stft_onesided_f32 if onesided else lib.nxsig_stft_f32)
    if packed and K % 2:
        raise ArgumentError("stft_packed: fft_length must be even")
    x = Operand(data)
    # f64 tier: f64 samples or an f64 window make the reference compute in f64 / c128 (Nx.multiply promotes, :101-102);
    # c128 samples, or c64 samples under an f64 window (the product of :101 promotes to c128): nxsig_stft_c128
    data_c128 = x.dtype == np.complex128 or (x.dtype == np.complex64 and w.dtype == np.float64)
    if x.dtype == np.float64 or data_c128 or w.dtype == np.float64:
        if onesided:
            raise ArgumentError("stft_onesided / stft_packed are f32 extensions; the f64 tier returns the full c128 spectrum")
        return _stft_f64(x, w, ctx, p, cplx=data_c128)
    # complex samples (c64 IQ data): the reference frames, multiplies and transforms whatever tensor it is given (lib/nx_signal.ex:94-102):
    # one transform per frame, nxsig_stft_c64
    data_c64 = x.dtype == np.complex64
    if data_c64:
        if onesided:
            raise ArgumentError("stft_onesided / stft_packed need real samples (a complex signal's spectrum is not Hermitian)")
        entry = lib.nxsig_stft_c64
    if x.device:
        if x.dtype != np.float32 and not data_c64:
            raise ArgumentError("stft: device input must be float32, float64 or complex64")
    elif data_c64:
        x.cast()
    else:
        _host_f32(x, "stft")
    c, batch, L, m = _frames(x, ctx, p)
    z = x.result(x.shape[:-1] + (m, Kout), np.complex64)
    _lib.check(entry(c.handle, x.ptr, L, batch, L, ptr(w), C.byref(p), ptr(z), C.byref(M), x.mem))
    freqs = fft_frequencies(fs, fft_length=K)
    return z, _stft_times(m, N, fs), (freqs[:Kout] if onesided else freqs)


def _stft_f64(x, w, ctx, p, cplx=False):
    """stft of f64 samples and / or with an f64 window: c128 spectrum (nxsig_stft_f64; complex samples: nxsig_stft_c128); times /
    frequencies stay f32 like the reference's (their linspace calls do not take the data type, lib/nx_signal.ex:106-111)"""
    lib = _lib.load()
    M = C.c_int64()
    fs = float(p.sampling_rate)
    entry = lib.nxsig_stft_c128 if cplx else lib.nxsig_stft_f64
    wide_t = np.complex128 if cplx else np.float64
    if x.device:
        if x.dtype != wide_t:
            raise NxSignalUnsupported("stft: an f64 window with device-resident f32 / c64 samples is not built; widen the samples first")
    else:
        if x.dtype.kind not in ("fiubc" if cplx else "fiub"):
            raise ArgumentError(f"stft: unsupported dtype {x.dtype}")
        x.cast(wide_t)   # f32 / c64 / integer samples widen exactly
    c, batch, L, m = _frames(x, ctx, p)
    z = x.result(x.shape[:-1] + (m, p.fft_length), np.complex128)
    _lib.check(entry(c.handle, x.ptr, L, batch, L, ptr(w), int(w.dtype == np.float64), C.byref(p), ptr(z), C.byref(M), x.mem))
    return z, _stft_times(m, p.frame_length, fs), fft_frequencies(fs, fft_length=p.fft_length)


def istft(data, window, ctx: Context | None = None, **opts):
    """NxSignal.istft/3 — lib/nx_signal.ex:582-638.  c64[..., M, K] -> c64[..., M*hop + overlap] (complex, B8)."""
    return _istft(data, window, ctx, opts, None)


def istft_filtered(data, h, window, ctx: Context | None = None, **opts):
    """Extension (not in the reference API): `istft(Nx.multiply(z, h), window, opts)` — the last two steps of the reference's
    STFT-domain filtering workflow (guides/filtering.livemd:141, :150-157) in one call.  Bit-identical to
    `istft(spectrum_multiply(z, h), window, **opts)`; for 1024-point frames the filter is applied inside the inverse-STFT
    kernel and the filtered spectrogram never exists in HBM.  h: c64[fft_length] (host)."""
    hh = np.ascontiguousarray(np.asarray(h).astype(np.complex64))
    if hh.ndim != 1:
        raise ArgumentError("istft_filtered: h must be a rank-1 tensor of fft_length bins")
    return _istft(data, window, ctx, opts, hh)


def _istft_options(window, opts):
    """the options of NxSignal.istft/3 with their defaults and errors, shared by istft, istft_filtered, istft_packed and istft_masked
    (needs no context) -> (options, host window, N, hop, sampling rate)"""
    o = _validate(opts, {"fft_length": None, "overlap_length": None, "scaling": None, "sampling_rate": 1000}, "istft")
    w = _window_host(window)
    N = int(w.shape[0])
    overlap = N // 2 if o["overlap_length"] is None else int(o["overlap_length"])  # :594-601
    if o["scaling"] not in _SCALING:  # :622-624
        raise ArgumentError(f"invalid :scaling, expected one of :spectrum, :psd or nil, got: {o['scaling']!r}")
    if o["scaling"] == "psd" and o["sampling_rate"] is None:  # :605
        raise ArgumentError(":sampling_rate is mandatory if scaling is :psd")
    fs = float(o["sampling_rate"]) if o["sampling_rate"] is not None else 0.0
    if overlap >= N:  # overlap_and_add check, :692-695
        raise ArgumentError(f"overlap_length must be a number less than the window size {N}, got: {N}")
    hop = N - overlap
    return o, w, N, hop, fs


def _istft_fft_length(o, Kin):
    """:fft_length against the spectrum's last axis (ifft pad / truncate is not built)"""
    K = _resolve_fft_length(o["fft_length"], Kin)
    if K != Kin:
        raise NxSignalUnsupported("istft: fft_length different from the spectrum's last axis (ifft pad/truncate) is not built")
    return K


def _istft(data, window, ctx, opts, hh, packed=False):
    data, window = _as_tensor(data), _as_tensor(window)
    o, w, N, hop, fs = _istft_options(window, opts)
    lib = _lib.load()
    x = Operand(data)
    if x.device:
        if x.dtype not in (np.complex64, np.complex128):
            raise ArgumentError("istft: device input must be complex64 or complex128")
        wide = x.dtype == np.complex128   # f64 tier: a c128 spectrum is inverted in c128 (Nx.ifft :609)
    else:
        wide = x.dtype in (np.complex128, np.float64)
        x.cast(np.complex128 if wide else np.complex64)
    if wide and (packed or hh is not None):
        raise ArgumentError("istft_packed / istft_filtered are f32 extensions; the f64 tier takes the full c128 spectrum")
    if w.dtype == np.float64 and not wide:
        # the reference would invert in c64 (Nx.ifft rounds to c64) and only then promote the frames to c128: not modelled
        raise NxSignalUnsupported("istft: a c64 spectrum with an f64 window is not built; pass the spectrum as complex128")
    if len(x.shape) < 2:
        raise ArgumentError("istft expects a tensor of shape {..., frames, frequencies}")
    (batch, Mf), Kin = rows_last(x.shape[:-1]), int(x.shape[-1])
    if packed:
        Kin *= 2   # the packed rows hold fft_length / 2 complex values
    K = _istft_fft_length(o, Kin)
    if hh is not None and int(hh.shape[0]) != K:
        raise ArgumentError("istft_filtered: h must have fft_length bins")
    p = StftParams(N, hop, K, 0, 0, 0, _SCALING[o["scaling"]], 0, fs)
    c = x.context(ctx, caller_first=True)
    out_len = _lib.check(lib.nxsig_ola_length(Mf, N, hop))
    y = x.result(x.shape[:-2] + (out_len,), np.complex128 if wide else (np.float32 if packed else np.complex64))
    head = (c.handle, x.ptr, Mf, batch, ptr(w))
    if wide:
        rc = lib.nxsig_istft_c128(*head, int(w.dtype == np.float64), C.byref(p), ptr(y), x.mem)
    elif packed:
        rc = lib.nxsig_istft_packed_f32(*head, C.byref(p), ptr(y), x.mem)
    elif hh is None:
        rc = lib.nxsig_istft_c64(*head, C.byref(p), ptr(y), x.mem)
    else:
        rc = lib.nxsig_istft_filtered_c64(*head, C.byref(p), ptr(hh), ptr(y), x.mem)
    _lib.check(rc)
    return y


def overlap_and_add(tensor, ctx: Context | None = None, **opts):
    """NxSignal.overlap_and_add/2 — lib/nx_signal.ex:684-736.  {..., M, N} -> {..., M*hop + overlap}."""
    o = _validate(opts, {"overlap_length": None, "type": None}, "overlap_and_add")
    if o["overlap_length"] is None:
        raise ArgumentError("missing :overlap_length option")
    overlap = int(o["overlap_length"])
    lib = _lib.load()
    x = Operand(_as_tensor(tensor))
    src = x.host
    src_dtype = x.dtype
    if x.device or x.dtype in (np.float64, np.complex128):
        x.cast()   # f64 tier
    elif x.dtype.kind == "c":
        x.cast(np.complex64)
    else:
        if src.dtype.kind in "iu" and src.size and src.ndim >= 2:
            # the reference adds integers exactly; here sums are formed in double and stored as f32, exact only below 2^24:
            # refuse loudly instead of returning rounded integers
            cover = -(-int(src.shape[-1]) // max(int(src.shape[-1]) - overlap, 1))
            if int(np.abs(src).max()) * cover >= 2 ** 24:
                raise ArgumentError("overlap_and_add: integer sums beyond 2^24 cannot be represented exactly by the f32 "
                                    "MI355X path; cast to a float type explicitly")
        _host_f32(x, "overlap_and_add")
    if len(x.shape) < 2:
        raise ArgumentError("overlap_and_add expects a tensor of shape {..., M, N}")
    (batch, Mf), N = rows_last(x.shape[:-1]), int(x.shape[-1])
    if overlap >= N:  # :692-695 — the message prints the window size twice (quirk B10)
        raise ArgumentError(f"overlap_length must be a number less than the window size {N}, got: {N}")
    c = x.context(ctx, caller_first=True)
    comps = 2 if x.dtype.kind == "c" else 1
    entry = lib.nxsig_overlap_and_add_f64 if x.dtype in (np.float64, np.complex128) else lib.nxsig_overlap_and_add
    out = x.result(x.shape[:-2] + (Mf * (N - overlap) + overlap,), x.dtype)
    _lib.check(entry(c.handle, x.ptr, Mf, batch, N, overlap, comps, ptr(out), x.mem))
    if x.device:
        return out
    target = o["type"] if o["type"] is not None else src_dtype  # code default: the input type (:685, B10)
    return out.astype(target) if np.dtype(target) != out.dtype else out


def mel_filters(fft_length, mel_bins, sampling_rate, **opts):
    """NxSignal.mel_filters/4 — lib/nx_signal.ex:397-445.  f32[mels: mel_bins][frequencies: fft_length]."""
    o = _validate(opts, {"max_mel": 3016, "mel_frequency_spacing": 200 / 3, "type": "f32"}, "mel_filters")
    if o["type"] not in ("f32", np.float32):
        raise ArgumentError("mel_filters: only type f32 is built")
    return _mel_filters_table(int(fft_length), int(mel_bins), float(sampling_rate), float(o["max_mel"]),
                              float(o["mel_frequency_spacing"])).copy()


@functools.lru_cache(maxsize=16)
def _mel_filters_table(fft_length: int, mel_bins: int, sampling_rate: float, max_mel: float, spacing: float) -> np.ndarray:
    """the filterbank is a pure function of its five parameters: generated once per combination (read-only copy)"""
    out = np.empty((mel_bins, fft_length), dtype=np.float32)
    _lib.check(_lib.load().nxsig_mel_filters_f32(fft_length, mel_bins, sampling_rate, max_mel, spacing, ptr(out)))
    out.setflags(write=False)
    return out


def _mel_filters_for(K, mb, fs, fopts):
    o = _validate(dict(fopts), {"max_mel": 3016, "mel_frequency_spacing": 200 / 3}, "mel_filters")
    return _mel_filters_table(int(K), int(mb), float(fs), float(o["max_mel"]), float(o["mel_frequency_spacing"]))


def stft_to_mel(z, sampling_rate, ctx: Context | None = None, **opts):
    """NxSignal.stft_to_mel/3 — lib/nx_signal.ex:486-513.  c64[..., frames, K] -> f32[..., frames, mel_bins]
    (the global maximum of the reference's `reduce_max` runs over the whole tensor)."""
    o = _validate(opts, {"fft_length": None, "mel_bins": 128, "max_mel": None, "mel_frequency_spacing": None, "type": "f32"},
                  "stft_to_mel")
    if o["fft_length"] is None:
        raise ArgumentError("missing :fft_length option")
    K, mb = int(o["fft_length"]), int(o["mel_bins"])
    fopts = {k: o[k] for k in ("max_mel", "mel_frequency_spacing") if o[k] is not None}
    filt = _mel_filters_for(K, mb, sampling_rate, fopts)
    x = Operand(z)
    if x.device and x.dtype != np.complex64:
        raise ArgumentError("stft_to_mel: device input must be complex64")
    x.cast(np.complex64)
    if x.shape[-1] != K:
        raise ArgumentError("stft_to_mel: the last axis must be fft_length")
    c = x.context(ctx, caller_first=True)
    out = x.result(x.shape[:-1] + (mb,), np.float32)
    _lib.check(_lib.load().nxsig_stft_to_mel(c.handle, x.ptr, rows_last(x.shape)[0], K, mb, ptr(filt), ptr(out), x.mem))
    return out


def spectrum_multiply(z, h, ctx: Context | None = None):
    """The `Nx.multiply(z, hfft)` step of the reference's STFT-domain filtering workflow (guides/filtering.livemd:137-159:
    stft -> z * H -> istft), kept on the device.  z c64[..., frames, K] (numpy or DeviceBuffer), h c64[K]
    (host) -> same kind and shape as z.  Components are computed in double and rounded once like Nx.BinaryBackend."""
    hh = np.ascontiguousarray(np.asarray(h).astype(np.complex64))
    if hh.ndim != 1:
        raise ArgumentError("spectrum_multiply: h must be a rank-1 tensor of fft_length bins")
    K = int(hh.shape[0])
    x = Operand(z)
    if x.device and (x.dtype != np.complex64 or x.shape[-1] != K):
        raise ArgumentError("spectrum_multiply: z must be complex64 with fft_length bins on the last axis")
    x.cast(np.complex64)
    if x.shape[-1] != K:
        raise ArgumentError("spectrum_multiply: z must have fft_length bins on the last axis")
    c = x.context(ctx, caller_first=True)
    out = x.result(x.shape, np.complex64)
    _lib.check(_lib.load().nxsig_spectrum_mul_c64(c.handle, x.ptr, rows_last(x.shape)[0], K, ptr(hh), ptr(out), x.mem))
    return out


_MASK_REAL, _MASK_ONESIDED, _MASK_COMPLEX = 0, 1, 2   # nxsig_mask_kind


def _mask_operands(z, mask, fn):
    """Shape / type / placement checks shared by spectrum_mask and istft_masked — all of them before a context exists.
    -> (z, mask, (M, K), kind, (Bz, Bm), lead): the two as Operands, host arrays contiguous in c64 and in f32 / c64."""
    z, mask = _as_tensor(z), _as_tensor(mask)
    if is_device(z) != is_device(mask):
        raise ArgumentError(f"{fn}: z and mask must both be host tensors or both be device-resident")
    z, mask = Operand(z), Operand(mask)
    dev = z.device
    if z.owner is not None and mask.owner is not None and z.owner is not mask.owner:
        raise ArgumentError(f"{fn}: z and mask live on different contexts")
    z.owner = z.owner or mask.owner   # the call runs where either operand lives
    zshape, zdt, mshape, mdt = z.shape, z.dtype, mask.shape, mask.dtype
    if zdt in (np.dtype(np.complex128), np.dtype(np.float64)) or mdt in (np.dtype(np.complex128), np.dtype(np.float64)):
        raise ArgumentError(f"{fn} is an f32 extension: f64 / c128 operands are not taken (cast to complex64 / float32)")
    if dev and zdt != np.dtype(np.complex64):
        raise ArgumentError(f"{fn}: device spectrum must be complex64")
    if mdt.kind == "c":
        cplx = True
    elif mdt.kind in "fiub":
        cplx = False
    else:
        raise ArgumentError(f"{fn}: unsupported mask dtype {mdt}")
    if dev and mdt not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise ArgumentError(f"{fn}: device mask must be float32 or complex64")
    if len(zshape) < 2 or len(mshape) < 2:
        raise ArgumentError(f"{fn} expects tensors of shape {{..., frames, frequencies}}")
    M, K = int(zshape[-2]), int(zshape[-1])
    if M < 1 or K < 1:
        raise ArgumentError(f"{fn}: the spectrum needs at least one frame and one bin")
    if int(mshape[-2]) != M:
        raise ArgumentError(f"{fn}: mask has {int(mshape[-2])} frames, the spectrum {M}")
    Km = int(mshape[-1])
    if Km == K:
        kind = _MASK_COMPLEX if cplx else _MASK_REAL
    elif Km == K // 2 + 1 and K % 2 == 0:
        if cplx:
            raise ArgumentError(f"{fn}: a one-sided mask must be real")
        kind = _MASK_ONESIDED
    elif K % 2 == 1 and Km == K // 2 + 1:
        raise ArgumentError(f"{fn}: a one-sided mask needs an even fft_length, got {K}")
    else:
        raise ArgumentError(f"{fn}: the mask's last axis must be fft_length ({K}) or fft_length / 2 + 1, got {Km}")
    Bz, Bm = rows_last(zshape[:-1])[0], rows_last(mshape[:-1])[0]
    if Bz != Bm and Bz != 1 and Bm != 1:
        raise ArgumentError(f"{fn}: z has {Bz} rows and mask {Bm}: they must be equal, or one of them 1")
    if max(Bz, Bm) < 1:
        raise ArgumentError(f"{fn}: empty leading axes")
    if max(Bz, Bm) > 65535:
        raise ArgumentError(f"{fn}: at most 65535 rows")
    # the leading shape of whichever operand carries the rows (the spectrum's when both do)
    lead = tuple(zshape[:-2]) if (Bz >= Bm and (Bz > 1 or len(zshape) >= len(mshape))) else tuple(mshape[:-2])
    z.cast(np.complex64)
    mask.cast(np.complex64 if cplx else np.float32)
    return z, mask, (M, K), kind, (Bz, Bm), tuple(int(d) for d in lead)


def spectrum_mask(z, mask, ctx: Context | None = None):
    """Extension: `Nx.multiply(z, mask)` for a time-frequency mask kept on the device.  z c64[..., M, K]; mask f32[..., M, K],
    c64[..., M, K] or the one-sided real f32[..., M, K/2 + 1] (bin k > K/2 takes mask[K - k]).  The flattened leading axes are equal
    or one of them is 1 (broadcast: one mixture and S masks).  Complex masks multiply like spectrum_multiply; a real gain
    multiplies each component on its own, in double with one rounding.  -> c64[lead..., M, K], host or DeviceBuffer like the inputs."""
    z, mask, (M, K), kind, (Bz, Bm), lead = _mask_operands(z, mask, "spectrum_mask")
    lib = _lib.load()
    c = z.context(ctx, caller_first=True)
    out = z.result(lead + (M, K), np.complex64)
    _lib.check(lib.nxsig_spectrum_mask_c64(c.handle, z.ptr, Bz, mask.ptr, kind, Bm, M, K, ptr(out), z.mem))
    return out


def istft_masked(z, mask, window, ctx: Context | None = None, **opts):
    """Extension: `istft(Nx.multiply(z, mask), window, opts)` in one call — the denoising / source-separation / spectral-gating step.
    Operands as in spectrum_mask, options, defaults and errors as in istft.  Bit-identical to
    `istft(spectrum_mask(z, mask), window, **opts)`; for 1024-point frames at hop 128 / 256 / 512 / 1024 the mask rows stream into
    the inverse-STFT kernel next to the spectrum and the masked spectrogram never exists in HBM."""
    window = _as_tensor(window)
    o, w, N, hop, fs = _istft_options(window, opts)
    if w.dtype == np.float64:
        raise ArgumentError("istft_masked is an f32 extension: an f64 window is not taken")
    z, mask, (M, K), kind, (Bz, Bm), lead = _mask_operands(z, mask, "istft_masked")
    K = _istft_fft_length(o, K)
    if K != N:
        raise ArgumentError("istft: fft_length must equal the window length (the reference broadcasts {M,K} x {N}, lib/nx_signal.ex:628)")
    lib = _lib.load()
    c = z.context(ctx, caller_first=True)
    p = StftParams(N, hop, K, 0, 0, 0, _SCALING[o["scaling"]], 0, fs)
    out_len = _lib.check(lib.nxsig_ola_length(M, N, hop))
    y = z.result(lead + (out_len,), np.complex64)
    _lib.check(lib.nxsig_istft_masked_c64(c.handle, z.ptr, Bz, M, ptr(w), C.byref(p), mask.ptr, kind, Bm, ptr(y), z.mem))
    return y


def mel_spectrogram(data, window, ctx: Context | None = None, **opts):
    """Extension (not in the reference API): `stft_to_mel(stft(data, window, ...)[0], sampling_rate, ...)` fused in one
    kernel — the spectrum never goes to HBM.  Takes the stft options plus :mel_bins (128), :max_mel,
    :mel_frequency_spacing.  Returns f32[..., frames, mel_bins], equal to the two-step result to fp32 rounding."""
    mel_keys = {"mel_bins": 128, "max_mel": None, "mel_frequency_spacing": None}
    mo = {k: opts.pop(k) for k in list(opts) if k in mel_keys}
    p, N, hop, K = _resolve_stft_opts(window, opts, "mel_spectrogram")
    w = _window_host(window)
    mb = int(mo.get("mel_bins", 128))
    fopts = {k: mo[k] for k in ("max_mel", "mel_frequency_spacing") if mo.get(k) is not None}
    filt = _mel_filters_for(K, mb, p.sampling_rate, fopts)
    M = C.c_int64()
    x = _real_f32(data, "mel_spectrogram")
    c, batch, L, m = _frames(x, ctx, p)
    out = x.result(x.shape[:-1] + (m, mb), np.float32)
    _lib.check(_lib.load().nxsig_stft_mel_f32(c.handle, x.ptr, L, batch, L, ptr(w), C.byref(p), mb, ptr(filt), ptr(out), C.byref(M), x.mem))
    return out


def _real_f32(data, fn) -> Operand:
    """the operand of the fused f32 extensions: a device tensor of f32, or a host array by the rule of _host_f32"""
    x = Operand(data)
    if not x.device:
        return _host_f32(x, fn)
    if x.dtype != np.float32:
        raise ArgumentError(f"{fn}: device input must be float32")
    return x


def _stft_times(m: int, N: int, fs: float) -> np.ndarray:
    times = np.empty(m, dtype=np.float32)
    _lib.check(_lib.load().nxsig_stft_times_f32(N, fs, m, ptr(times)))
    return times


_MAG_KINDS = {"magnitude": _lib.MAG_ABS, "power": _lib.MAG_POWER, "dbfs": _lib.MAG_DBFS}


def spectrogram(data, window, ctx: Context | None = None, **opts):
    """Extension (not in the reference API): the magnitude spectrogram guides/spectrogram.livemd:76-92
    derives from `NxSignal.stft/3` — `Nx.abs(s)` of the bins below fft_length / 2, optionally in dBFS
    (`20 * log(|s| / reduce_max(|s|)) / log(10)`) — fused with the STFT so the complex spectrum never goes to HBM.
    Takes the stft options plus :kind ("magnitude" (default), "power", "dbfs").
    Returns {spec f32[..., frames, fft_length/2], t, f[:fft_length/2]}."""
    kind = opts.pop("kind", "magnitude")
    if kind not in _MAG_KINDS:
        raise ArgumentError(f"invalid :kind, expected one of {list(_MAG_KINDS)}, got: {kind!r}")
    p, N, hop, K = _resolve_stft_opts(window, opts, "spectrogram")
    w = _window_host(window)
    half = K // 2
    M = C.c_int64()
    f = fft_frequencies(p.sampling_rate, fft_length=K)[:half]
    x = _real_f32(data, "spectrogram")
    c, batch, L, m = _frames(x, ctx, p)
    out = x.result(x.shape[:-1] + (m, half), np.float32)
    _lib.check(_lib.load().nxsig_stft_magnitude_f32(c.handle, x.ptr, L, batch, L, ptr(w), C.byref(p), _MAG_KINDS[kind], ptr(out), C.byref(M),
                                                    x.mem))
    return out, _stft_times(m, N, p.sampling_rate), f


from . import convolution, filters, peak_finding, spectral, transforms, waveforms, windows  # noqa: E402,F401
from ._dct import mfcc  # noqa: E402,F401  (mel_spectrogram, then transforms.dct: _dct.py)
