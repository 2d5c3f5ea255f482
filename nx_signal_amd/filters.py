"""NxSignal.Filters: median/2, wiener/2 (lib/nx_signal/filters.ex:17-110, :281-303), firwin/3 (:147-279) and the new `fir`
(BASELINE config 5), `resample_poly`, `sosfilt`, `sosfilt_zi` and `sosfiltfilt` (extensions in scipy.signal's spelling)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, convolution
from ._lib import ArgumentError, NxSignalUnsupported
from ._marshal import Operand, ptr, rows_last, validate

_WINDOWS = {
    "hamming": _lib.WIN_HAMMING, "hann": _lib.WIN_HANN, "blackman": _lib.WIN_BLACKMAN,
    "bartlett": _lib.WIN_BARTLETT, "rectangular": _lib.WIN_RECTANGULAR,
}


def firwin(num_taps, cutoff, **opts):
    """Window-method FIR design.  `cutoff` must be a list (quirk B13); window one of "hamming", "hann",
    "blackman", "bartlett", "rectangular" or ("kaiser", beta)."""
    o = validate(opts, {"window": "hamming", "pass_zero": True, "scale": True, "sampling_rate": 2.0, "type": "f32"}, "firwin")
    if not isinstance(cutoff, (list, tuple)):  # filters.ex:160-162
        raise ArgumentError(f"cutoff must be a list of frequencies, got: {cutoff!r}")
    win, beta = o["window"], 0.0
    if isinstance(win, (tuple, list)) and len(win) == 2 and win[0] == "kaiser":
        kind, beta = _lib.WIN_KAISER, float(win[1])
    elif isinstance(win, str) and win in _WINDOWS:
        kind = _WINDOWS[win]
    else:  # filters.ex:274-277
        raise ArgumentError(
            f"unknown window {win!r}, supported: :hamming, :hann, :blackman, :bartlett, :rectangular, {{:kaiser, beta}}"
        )
    f64 = o["type"] in ("f64", np.float64)
    if not f64 and o["type"] not in ("f32", np.float32):
        raise ArgumentError("firwin: type must be f32 or f64")
    cut = (C.c_double * len(cutoff))(*[float(c) for c in cutoff])
    out = np.empty(int(num_taps), dtype=np.float64 if f64 else np.float32)
    entry = _lib.load().nxsig_firwin_f64 if f64 else _lib.load().nxsig_firwin_f32
    _lib.check(entry(int(num_taps), cut, len(cutoff), kind, beta, int(bool(o["pass_zero"])), int(bool(o["scale"])), float(o["sampling_rate"]),
                     ptr(out)))
    return out


def fir(x, taps, mode="same", ctx=None):
    """FIR-filter a real stream (batched over leading axes) with real `taps` by overlap-save block FFT
    convolution on the GPU.  Equals Convolution.convolve(x, taps, method: :fft, mode:) of the reference
    (guides/filtering.livemd:126-128) to fp32 rounding; the reference has no streaming form."""
    return convolution.convolve(x, taps, mode=mode, method="fft", ctx=ctx)


def median(t, ctx=None, **opts):
    """Filters.median/2 — lib/nx_signal/filters.ex:17-55.  median(t, kernel_shape=(k_0, ..., k_{r-1})): the median of the window of
    kernel_shape that starts at min(i_d, n_d - k_d) on every axis (no padding), as f32 of t's shape.  Host arrays of any real type
    (integers are computed like f64) or a device tensor of f32 / f64, which gives a device tensor back.  Order like np.sort: NaN
    above +Inf, -0.0 == +0.0; even windows average the two middle values in the input's type."""
    validate(opts, ("kernel_shape",), "median")
    ks = opts.get("kernel_shape")
    x = Operand(t)
    shape, dtype = x.shape, x.dtype
    if not isinstance(ks, tuple) or len(ks) != len(shape):   # filters.ex:38-40
        raise ArgumentError("kernel shape must be of the same rank as the tensor")
    if dtype.kind == "c":
        raise ArgumentError("median: complex tensors have no order")
    if dtype.kind not in "fiub":
        raise ArgumentError(f"median: unsupported type {dtype}")
    if not 1 <= len(shape) <= 8:
        raise ArgumentError("median: rank must be in [1, 8]")
    ks = tuple(int(k) for k in ks)
    for d, (k, n) in enumerate(zip(ks, shape)):   # Nx.slice: the window must fit its axis
        if not 1 <= k <= n:
            raise ArgumentError(f"median: kernel_shape {k} is outside 1..{n} on axis {d}")
    is_f64 = dtype != np.float32
    sh = (C.c_int64 * len(shape))(*shape)
    kc = (C.c_int64 * len(shape))(*ks)
    if x.device and dtype not in (np.float32, np.float64):
        raise ArgumentError(f"median: device tensors must be f32 or f64, got {dtype}")
    x.cast(np.float64 if is_f64 else np.float32)
    c = x.context(ctx, caller_first=False)
    out = x.result(shape, np.float32)
    _lib.check(_lib.load().nxsig_median_filter(c.handle, x.ptr, int(is_f64), sh, len(shape), kc, ptr(out), x.mem))
    return out


def wiener(t, ctx=None, return_noise=False, **opts):
    """Filters.wiener/2 — lib/nx_signal/filters.ex:81-110, :281-303.  wiener(t, kernel_size=3, noise=None): local mean and variance
    over the :same-padded window in f64, then the Wiener formula; the result has t's type (f32 or f64, host or device).  noise=None
    estimates it as the mean local variance.  return_noise=True also returns the noise the formula used."""
    validate(opts, ("noise", "kernel_size"), "wiener")
    ks = opts.get("kernel_size", 3)
    noise = opts.get("noise")
    x = Operand(t)
    shape, dtype = x.shape, x.dtype
    rank = len(shape)
    if isinstance(ks, (int, np.integer)) and not isinstance(ks, bool):
        ks = (int(ks),) * rank
    elif not isinstance(ks, tuple):
        raise ArgumentError("kernel_size must be an integer or tuple")
    if len(ks) != rank:   # Nx.conv in the reference
        raise ArgumentError(f"wiener: kernel_size {ks} must have one length per axis of the rank-{rank} tensor")
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise ArgumentError(f"wiener: kernel_size {ks} must be >= 1 on every axis")
    if noise is not None and (isinstance(noise, bool) or not isinstance(noise, (int, float, np.integer, np.floating))):
        raise ArgumentError(f"wiener: noise must be a number or nil, got: {noise!r}")
    if dtype not in (np.float32, np.float64):
        raise NxSignalUnsupported(f"wiener: f32 and f64 tensors are built, got {dtype}")
    if not 1 <= rank <= 8:
        raise ArgumentError("wiener: rank must be in [1, 8]")
    sh = (C.c_int64 * rank)(*shape)
    kc = (C.c_int64 * rank)(*ks)
    used = C.c_double(0.0)
    x.cast()
    c = x.context(ctx, caller_first=False)
    out = x.result(shape, dtype)
    _lib.check(_lib.load().nxsig_wiener(c.handle, x.ptr, int(dtype == np.float64), sh, rank, kc, int(noise is not None),
                                        float(noise) if noise is not None else 0.0, ptr(out), C.byref(used) if return_noise else None, x.mem))
    return (out, used.value) if return_noise else out


def _axis_last(x, axis, fn, device_error):
    """`axis` of operand x, validated and counted from the front.  A host array gets that axis at the back; a device tensor is taken
    along its last axis only (else device_error)."""
    rank = len(x.shape)
    if rank < 1:
        raise ArgumentError(f"{fn}: the tensor must have at least one axis")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -rank <= axis < rank:
        raise ArgumentError(f"{fn}: axis {axis!r} is out of bounds for a tensor of rank {rank}")
    axis = int(axis) % rank
    if any(s < 1 for s in x.shape):
        raise ArgumentError(f"{fn}: empty dimension")
    if x.device and axis != rank - 1:
        raise device_error
    x.move_last(axis)
    return axis


_RESAMPLE_KEYS = ("ctx", "axis", "window", "taps", "padtype")


def resample_poly_taps(up, down, window=("kaiser", 5.0)):
    """The default anti-alias filter of resample_poly with its gain, f32: `up * firwin(20 * max(up, down) + 1, [1 / max(up, down)],
    window: w, sampling_rate: 2.0, type: f64)` of the REDUCED up / down, formed in f64 and rounded once (scipy.signal.resample_poly's
    design, on this project's firwin)."""
    up, down = _resample_ratio(up, down)
    big = max(up, down)
    h = firwin(20 * big + 1, [1.0 / big], window=window, sampling_rate=2.0, type="f64")
    return (np.float64(up) * h).astype(np.float32)


def _resample_ratio(up, down):
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ArgumentError(f"resample_poly: {name} must be an integer >= 1, got: {v!r}")
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ArgumentError(f"resample_poly: up and down must be >= 1, got: {up}, {down}")
    if up >= 2 ** 31 or down >= 2 ** 31:
        raise ArgumentError("resample_poly: up and down must fit 32 bits")
    g = int(np.gcd(up, down))
    return up // g, down // g


def resample_poly(x, up, down, ctx=None, axis=-1, window=("kaiser", 5.0), taps=None, padtype="constant", **opts):
    """Extension (the reference has no resampler): resample `axis` of real f32 or complex c64 rows by the rational factor up / down
    with a polyphase FIR on the GPU — scipy.signal.resample_poly(x, up, down, padtype="constant").  n samples give ceil(n up / down);
    with the reduced ratio, taps h (gain included) and half = (len(h) - 1) // 2:  y[m] = sum_j x[j] h[m down + half - j up] over the
    taps that exist (include/nxsig.h: nxsig_resample_poly).  window: any window firwin accepts, the default
    filter is resample_poly_taps(up, down, window); taps: a 1-D real array instead (scipy's array form of `window=`, WITHOUT the
    gain: h = up * taps).  up == down after reduction returns a copy.  Host arrays: any axis, numpy out; a device tensor: the last
    axis only, a DeviceBuffer out.  An Inf / NaN sample reaches the outputs whose taps cover it and nothing else."""
    validate(opts, _RESAMPLE_KEYS, "resample_poly")
    up, down = _resample_ratio(up, down)
    if padtype != "constant":
        raise ArgumentError(f"resample_poly: only padtype \"constant\" is built, got: {padtype!r}")
    if taps is not None:
        t = np.asarray(taps)
        if t.ndim != 1 or t.dtype.kind not in "fiu":
            raise ArgumentError("resample_poly: taps must be a 1-D real array")
        if t.shape[0] < 1:
            raise ArgumentError("resample_poly: the tap vector is empty")
        h = (np.float64(up) * t.astype(np.float64)).astype(np.float32)
    elif up != down:
        h = resample_poly_taps(up, down, window)
    else:
        firwin(3, [0.5], window=window)   # the window is validated although nothing is filtered
        h = np.ones(1, np.float32)
    x = Operand(x)
    if x.dtype not in (np.float32, np.complex64):
        raise NxSignalUnsupported(f"resample_poly: f32 and c64 tensors are built, got {x.dtype}")
    axis = _axis_last(x, axis, "resample_poly", ArgumentError("resample_poly: device tensors are resampled along their last axis only"))
    lib = _lib.load()
    batch, n = rows_last(x.shape)
    n_out = _lib.check(lib.nxsig_resample_length(n, up, down))
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape[:-1] + (n_out,), x.dtype)
    _lib.check(lib.nxsig_resample_poly(_lib.ctx_ptr(c.handle), x.ptr, int(x.dtype == np.complex64), n, batch, n, ptr(h), h.shape[0], up, down,
                                       ptr(out), x.mem))
    return out if x.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))


# ---- recursive filters: scipy.signal.sosfilt / sosfilt_zi / sosfiltfilt (include/nxsig.h)
_SOS_MAX = 16   # sections of one C call; longer cascades run as consecutive groups
_SOS_PADTYPES = {None: 0, "odd": 1, "even": 2, "constant": 3}


def _sos(sos, fn):
    """sos as a C-contiguous f64 [n_sections, 6] array, validated as scipy's _validate_sos does"""
    try:
        s = np.ascontiguousarray(np.asarray(sos), dtype=np.float64)
    except (TypeError, ValueError):
        raise ArgumentError(f"{fn}: sos must be a real array of shape (n_sections, 6)") from None
    if s.ndim != 2:
        raise ArgumentError(f"{fn}: sos array must be 2D")
    if s.shape[1] != 6 or s.shape[0] < 1:
        raise ArgumentError(f"{fn}: sos array must be shape (n_sections, 6)")
    if not (s[:, 3] == 1).all():
        raise ArgumentError(f"{fn}: sos[:, 3] should be all ones")
    if not np.isfinite(s).all():
        raise ArgumentError(f"{fn}: sos must be finite")
    return s


def _sos_operand(x, axis, fn):
    """(operand, its shape as given, axis) of the tensor a recursive filter runs over: real f32, the rows at the back"""
    x = Operand(x)
    if x.dtype != np.float32:
        raise NxSignalUnsupported(f"{fn}: real f32 tensors are built, got {x.dtype}")
    shape = x.shape
    axis = _axis_last(x, axis, fn, NxSignalUnsupported(f"{fn}: device tensors are filtered along their last axis only"))
    return x, shape, axis


def sosfilt_zi(sos):
    """scipy.signal.sosfilt_zi: the states (n_sections, 2) of the cascade's settled step response."""
    s = _sos(sos, "sosfilt_zi")
    zi = np.empty((s.shape[0], 2), np.float64)
    pd = C.POINTER(C.c_double)
    _lib.check(_lib.load().nxsig_sosfilt_zi(C.cast(ptr(s), pd), s.shape[0], C.cast(ptr(zi), pd)))
    return zi


def sosfilt(x, sos, zi=None, ctx=None, axis=-1, direction=0):
    """Extension (the reference has no recursive filter): scipy.signal.sosfilt(sos, x, axis, zi) on the GPU — a cascade of biquads
    `sos` (n_sections, 6), a0 == 1, in transposed direct form II over `axis` of real f32 rows, computed in double and rounded to f32
    once.  Returns y, or (y, zf) when `zi` (n_sections, ..., 2) is given, in scipy's layouts; zf is a numpy array.  Host arrays: any
    axis, numpy out; a device tensor: the last axis only, a DeviceBuffer out.  Cascades of more than 16 sections run as consecutive
    groups of 16 (f32 rows between the groups).  direction=1 runs the filter from the end of each row towards its start.  Outputs
    ahead of a row's first Inf / NaN are untouched by it; every output from it on is non-finite."""
    s = _sos(sos, "sosfilt")
    x, shape, axis = _sos_operand(x, axis, "sosfilt")
    if direction not in (0, 1):
        raise ArgumentError(f"sosfilt: direction must be 0 or 1, got: {direction!r}")
    (batch, n), ns = rows_last(x.shape), s.shape[0]
    zrows = None
    if zi is not None:
        z = np.asarray(zi)
        want = (ns,) + shape[:axis] + (2,) + shape[axis + 1:]
        if z.shape != want or z.dtype.kind not in "fiu":
            raise ArgumentError(f"sosfilt: invalid zi shape. With axis={axis - len(shape)}, an input with shape {shape}, and an sos array with "
                                f"{ns} sections, zi must have shape {want}, got {z.shape}.")
        # [batch][n_sections][2] for the C ABI
        zrows = np.ascontiguousarray(np.moveaxis(z.astype(np.float64), axis + 1, -1).reshape(ns, batch, 2).transpose(1, 0, 2))
    lib, c = _lib.load(), x.context(ctx, caller_first=False)
    zf = np.empty((batch, ns, 2), np.float64) if zi is not None else None
    src, out = x.ptr, None
    for g0 in range(0, ns, _SOS_MAX):
        sg = np.ascontiguousarray(s[g0:g0 + _SOS_MAX])
        k = sg.shape[0]
        zig = np.ascontiguousarray(zrows[:, g0:g0 + k]) if zrows is not None else None
        zfg = np.empty((batch, k, 2), np.float64) if zrows is not None else None
        nxt = x.result(x.shape, np.float32)
        _lib.check(lib.nxsig_sosfilt_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), src, n, batch, n, ptr(sg), k, ptr(zig), batch, ptr(zfg),
                                         int(direction), ptr(nxt), x.mem))
        out = nxt   # the previous group's result is let go only now, behind the call that read it
        src = ptr(out)
        if zfg is not None:
            zf[:, g0:g0 + k] = zfg
    if not x.device:
        out = np.ascontiguousarray(np.moveaxis(out, -1, axis))
    if zi is None:
        return out
    zf = np.moveaxis(zf.transpose(1, 0, 2).reshape((ns,) + shape[:axis] + shape[axis + 1:] + (2,)), -1, axis + 1)
    return out, np.ascontiguousarray(zf)


def sosfiltfilt(x, sos, ctx=None, axis=-1, padtype="odd", padlen=None):
    """Extension: scipy.signal.sosfiltfilt(sos, x, axis, padtype, padlen) in one device-resident call — the rows extended by `padlen`
    samples per side (default: scipy's), filtered forward and backward from the states sosfilt_zi scaled by the first sample each
    way, the middle kept.  padtype "odd" (default), "even", "constant" or None.  Real f32 rows; host arrays: any axis, numpy out; a
    device tensor: the last axis only, a DeviceBuffer out.  At most 16 sections.  A row with an Inf / NaN is non-finite everywhere."""
    s = _sos(sos, "sosfiltfilt")
    if isinstance(padtype, (list, dict, set, np.ndarray)) or padtype not in _SOS_PADTYPES:
        raise ArgumentError(f"sosfiltfilt: unknown value {padtype!r} given to padtype. padtype must be 'even', 'odd', 'constant', or None.")
    if padlen is not None and (isinstance(padlen, bool) or not isinstance(padlen, (int, np.integer)) or padlen < 0):
        raise ArgumentError(f"sosfiltfilt: padlen must be a non-negative integer or None, got: {padlen!r}")
    x, shape, axis = _sos_operand(x, axis, "sosfiltfilt")
    if s.shape[0] > _SOS_MAX:
        raise NxSignalUnsupported(f"sosfiltfilt: cascades of up to {_SOS_MAX} sections are built, got {s.shape[0]}")
    batch, n = rows_last(x.shape)
    if padtype is None:
        edge = 0
    elif padlen is None:
        edge = 3 * (2 * s.shape[0] + 1 - min(int((s[:, 2] == 0).sum()), int((s[:, 5] == 0).sum())))
    else:
        edge = int(padlen)
    if n <= edge:   # scipy's _validate_pad
        raise ArgumentError(f"sosfiltfilt: the length of the input vector x must be greater than padlen, which is {edge}.")
    c = x.context(ctx, caller_first=False)
    out = x.result(x.shape, np.float32)
    _lib.check(_lib.load().nxsig_sosfiltfilt_f32(_lib.ctx_ptr(c.handle, _lib._ctx_iir), x.ptr, n, batch, n, ptr(s), s.shape[0],
                                                 _SOS_PADTYPES[padtype], edge, ptr(out), x.mem))
    return out if x.device else np.ascontiguousarray(np.moveaxis(out, -1, axis))


# savgol_filter / savgol_coeffs live in a module of their own (_savgol.py) and are part of this one's interface
from ._savgol import savgol_coeffs, savgol_filter  # noqa: E402,F401
# ... and so does hilbert (_hilbert.py)
from ._hilbert import hilbert  # noqa: E402,F401
# ... and the transfer-function filters lfilter / lfilter_zi / filtfilt / lfiltic (_lfilter.py)
from ._lfilter import filtfilt, lfilter, lfilter_zi, lfiltic  # noqa: E402,F401
# ... and the filter bank fir_bank (_cwt.py)
from ._cwt import fir_bank  # noqa: E402,F401
