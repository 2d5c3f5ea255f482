"""What the Python mirror hands to the C ABI, call by call, without a GPU.

A recording stand-in takes the place of the loaded library (`_lib._lib`).  The entry points that take no context (length helpers,
windows, firwin, frequencies, times, mel_filters, sosfilt_zi, sinc) go to the real libnxsig.so; nxsig_alloc is answered with fake
addresses from a reserved range; every other call is written down and answered with 0: its name, the ctypes type of the context
argument and which of three fake contexts (caller, owner, default) stands behind it, every integer and float, the fields of a
StftParams passed by reference, the values of small ctypes arrays, for each pointer one of null / host / device#allocation+offset,
and the mem flag.  Of the result, the type, shape and dtype and the context a DeviceBuffer belongs to.  Tensor contents are not
recorded: the GPU suites cover them.

Every public function of the package's modules runs over a host tensor, a DeviceBuffer and a __cuda_array_interface__ object without
`.ctx`, each with and without `ctx=`, on the smallest shapes that reach the call; and once with an invalid argument while
default_context raises.  tests/golden/python_marshalling.json holds the transcript of the commit named inside it; the package must
reproduce it byte for byte.

    python tests/test_python_marshalling_host.py --write PATH --parent HASH    writes a transcript
    python tests/test_python_marshalling_host.py --time                       median wrapper time of stft, sosfilt, sawtooth
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import nx_signal_amd as S   # noqa: E402
from nx_signal_amd import _lib   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "python_marshalling.json")
FORWARDED = {
    "nxsig_abi_version", "nxsig_last_error", "nxsig_last_dispatch", "nxsig_next_pow2", "nxsig_num_frames", "nxsig_ola_length",
    "nxsig_conv_length", "nxsig_window_f32", "nxsig_window_f64", "nxsig_sinc_f32", "nxsig_sinc_f64", "nxsig_firwin_f32",
    "nxsig_firwin_f64", "nxsig_fft_frequencies_f32", "nxsig_fft_frequencies_f64", "nxsig_stft_times_f32", "nxsig_mel_filters_f32",
    "nxsig_resample_length", "nxsig_resample_tile", "nxsig_welch_bins", "nxsig_sosfilt_chunk", "nxsig_sosfilt_tile", "nxsig_sosfilt_zi",
}
BASE = 0x7E0000000000   # the reserved range of fake device addresses; nothing ever reads through one
HANDLES = {0x1000: "caller", 0x2000: "owner", 0x3000: "default"}
_INTS = (C.c_int32, C.c_int64, C.c_size_t)


class Recorder:
    """the stand-in for the loaded library"""

    def __init__(self, real):
        self.real = real
        self.reset()

    def reset(self):
        self.calls, self.allocs, self.next = [], [], BASE

    def alloc(self, nbytes):
        addr = self.next
        self.allocs.append((addr, max(int(nbytes), 1)))
        self.next += (max(int(nbytes), 1) + 255) // 256 * 256
        return addr

    def where(self, a):
        v = a.value if isinstance(a, C.c_void_p) else a
        if v is None:
            return "null"
        if isinstance(v, C._Pointer):
            v = C.cast(v, C.c_void_p).value
        for i, (addr, size) in enumerate(self.allocs):
            if addr <= v < addr + size:
                return f"device#{i}+{v - addr}"
        return "host"

    def describe(self, argtype, a):
        if argtype in _lib.TYPED_CTX or argtype is None:
            return f"{type(a).__name__}:{HANDLES.get(C.cast(a, C.c_void_p).value, '?') if a is not None else 'null'}"
        if argtype is C.c_void_p:
            return self.where(a)
        if argtype in _INTS:
            return int(a.value if hasattr(a, "value") else a)
        if argtype is C.c_double:
            return float(a)
        if a is None:
            return "null"
        if isinstance(a, C.Array):
            return [type(a)._type_.__name__] + list(a)
        obj = getattr(a, "_obj", None)
        if isinstance(obj, _lib.StftParams):
            return {"StftParams": [getattr(obj, f) for f, _ in obj._fields_]}
        return f"out:{type(obj).__name__}" if obj is not None else self.where(a)

    def __getattr__(self, name):
        if name in FORWARDED:
            return getattr(self.real, name)
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        if name == "nxsig_free":
            return lambda *a: 0   # runs when a buffer is collected: not part of a call's transcript

        def call(*args):
            argtypes = _lib.SIGNATURES[name][1]
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            row = [name] + [self.describe(None if i == 0 else t, a) for i, (t, a) in enumerate(zip(argtypes, args))]
            if name == "nxsig_alloc":
                args[2]._obj.value = self.alloc(args[1])
            self.calls.append(row)
            return 0

        return call


class Cai:
    """a device object that has __cuda_array_interface__ and no .ctx"""

    def __init__(self, ptr, shape, dtype):
        self.__cuda_array_interface__ = {"data": (ptr, False), "shape": tuple(shape), "typestr": np.dtype(dtype).str, "strides": None,
                                         "version": 3}


class World:
    """the recorder, the three contexts and the operand kinds of one run"""

    def __init__(self):
        self.saved = _lib._lib
        self.rec = _lib._lib = Recorder(_lib.load())
        self.ctx = {name: S.Context(_borrowed=h) for h, name in HANDLES.items()}
        self.names = {id(c): n for n, c in self.ctx.items()}
        self.patched = []
        self.patch_default(lambda device=0: self.ctx["default"])

    def patch_default(self, fn):
        for name, mod in list(sys.modules.items()):
            if name.split(".")[0] == "nx_signal_amd" and hasattr(mod, "default_context"):
                if not any(m is mod for m, _ in self.patched):
                    self.patched.append((mod, mod.default_context))
                mod.default_context = fn

    def close(self):
        for mod, fn in self.patched:
            mod.default_context = fn
        _lib._lib = self.saved

    def operand(self, kind):
        def make(a):
            a = np.asarray(a)
            if kind == "host":
                return a
            ptr = self.rec.alloc(a.nbytes)
            if kind == "buf":
                return S.DeviceBuffer(self.ctx["owner"], ptr, a.shape, a.dtype, owner=False)
            return Cai(ptr, a.shape, a.dtype)
        return make

    def result(self, r):
        if isinstance(r, np.ndarray):
            return ["ndarray", list(r.shape), str(r.dtype)]
        if isinstance(r, S.DeviceBuffer):
            return ["DeviceBuffer", list(r.shape), str(r.dtype), self.names.get(id(r.ctx), "?")]
        if isinstance(r, (tuple, list)):
            return [self.result(v) for v in r]
        if isinstance(r, dict):
            return {k: self.result(r[k]) for k in sorted(r)}
        return [type(r).__name__, r if isinstance(r, (int, float, str, type(None))) else repr(r)]

    def run(self, fn, kind, with_ctx):
        self.rec.reset()
        kw = {"ctx": self.ctx["caller"]} if with_ctx else {}
        try:
            with np.errstate(all="ignore"):   # results are never filled in: what numpy makes of their bytes says nothing
                out = {"result": self.result(fn(self.operand(kind), kw))}
        except Exception as e:   # the outcome of a case may be an error: it is part of the transcript
            out = {"raises": type(e).__name__, "message": str(e)}
        out["calls"] = self.rec.calls
        return out


# ---- the smallest operands that reach every call
def _ramp(shape, dtype=np.float32):
    return (np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) % 7 - 3).astype(dtype)


X, Y = _ramp((2, 64)), _ramp((2, 64))[:, ::-1].copy()   # 2 rows of 64 samples
W = np.hanning(18)[1:-1].astype(np.float32)                # N = 16, hop 4
ST = dict(overlap_length=12, fft_length=16, sampling_rate=100)
Z = (_ramp((2, 8, 16)) + 1j * _ramp((2, 8, 16))).astype(np.complex64)   # 2 x 8 frames of 16 bins
FR, MASK = _ramp((2, 8, 16)), np.abs(_ramp((2, 8, 16)))
H = np.ones(16, np.complex64)
ND = _ramp((4, 8))                                         # rank 2 for the n-D functions
TAPS = np.array([1, 2, 3, 2, 1], np.float32)
SOS = np.array([[0.2, 0.4, 0.2, 1.0, -0.3, 0.1]])
T1 = _ramp((64,))

F, Cv, Tr, Sp, Wv, Pk, Wi = S.filters, S.convolution, S.transforms, S.spectral, S.waveforms, S.peak_finding, S.windows

# id -> (call(T, kw), the same with an invalid argument or None); T makes the operand of the case's kind from an array
TENSOR_CASES = {
    "as_windowed": (lambda T, kw: S.as_windowed(T(X), window_length=16, stride=4, **kw),
                    lambda T, kw: S.as_windowed(T(X), window_length=16, stride=0, **kw)),
    "as_windowed.f64": (lambda T, kw: S.as_windowed(T(X.astype(np.float64)), window_length=16, stride=4, padding="reflect", **kw), None),
    "as_windowed.s32": (lambda T, kw: S.as_windowed(T(X.astype(np.int32)), window_length=16, padding=[(1, 2)], **kw), None),
    "stft": (lambda T, kw: S.stft(T(X), W, **ST, **kw), lambda T, kw: S.stft(T(X), W, scaling="bogus", **kw)),
    "stft.c64": (lambda T, kw: S.stft(T(X.astype(np.complex64)), W, **ST, **kw), None),
    "stft.f64": (lambda T, kw: S.stft(T(X.astype(np.float64)), W, **ST, **kw), None),
    "stft.c128": (lambda T, kw: S.stft(T(X.astype(np.complex128)), W.astype(np.float64), **ST, **kw), None),
    "stft.f64window": (lambda T, kw: S.stft(T(X), W.astype(np.float64), **ST, **kw), None),
    "stft.rank1": (lambda T, kw: S.stft(T(X[0]), W, window_padding="reflect", scaling="psd", **kw), None),
    "stft_onesided": (lambda T, kw: S.stft_onesided(T(X), W, **ST, **kw), lambda T, kw: S.stft_onesided(T(X), W, fft_length=1, **kw)),
    "stft_packed": (lambda T, kw: S.stft_packed(T(X), W, **ST, **kw), lambda T, kw: S.stft_packed(T(X), W, fft_length=17, **kw)),
    "istft": (lambda T, kw: S.istft(T(Z), W, overlap_length=12, **kw), lambda T, kw: S.istft(T(Z), W, overlap_length=16, **kw)),
    "istft.c128": (lambda T, kw: S.istft(T(Z.astype(np.complex128)), W.astype(np.float64), overlap_length=12, scaling="spectrum", **kw), None),
    "istft.rank1": (lambda T, kw: S.istft(T(Z[0, 0]), W, **kw), None),
    "istft_packed": (lambda T, kw: S.istft_packed(T(Z[..., :8].copy()), W, overlap_length=12, **kw),
                     lambda T, kw: S.istft_packed(T(Z[..., :8].copy()), W, bogus=1, **kw)),
    "istft_filtered": (lambda T, kw: S.istft_filtered(T(Z), H, W, overlap_length=12, **kw),
                       lambda T, kw: S.istft_filtered(T(Z), H.reshape(4, 4), W, overlap_length=12, **kw)),
    "overlap_and_add": (lambda T, kw: S.overlap_and_add(T(FR), overlap_length=12, **kw),
                        lambda T, kw: S.overlap_and_add(T(FR), overlap_length=16, **kw)),
    "overlap_and_add.c64": (lambda T, kw: S.overlap_and_add(T(Z), overlap_length=12, **kw), None),
    "overlap_and_add.f64": (lambda T, kw: S.overlap_and_add(T(FR.astype(np.float64)), overlap_length=12, type=np.float32, **kw), None),
    "overlap_and_add.s32": (lambda T, kw: S.overlap_and_add(T(FR.astype(np.int32)), overlap_length=12, **kw), None),
    "stft_to_mel": (lambda T, kw: S.stft_to_mel(T(Z), 100, fft_length=16, mel_bins=4, **kw),
                    lambda T, kw: S.stft_to_mel(T(Z), 100, fft_length=8, mel_bins=4, **kw)),
    "spectrum_multiply": (lambda T, kw: S.spectrum_multiply(T(Z), H, **kw), lambda T, kw: S.spectrum_multiply(T(Z), H[:8], **kw)),
    "spectrum_mask": (lambda T, kw: S.spectrum_mask(T(Z), T(MASK), **kw), lambda T, kw: S.spectrum_mask(T(Z), T(MASK[:, :4]), **kw)),
    "spectrum_mask.onesided": (lambda T, kw: S.spectrum_mask(T(Z[:1]), T(MASK[..., :9].copy()), **kw), None),
    "spectrum_mask.complex": (lambda T, kw: S.spectrum_mask(T(Z), T(Z[0]), **kw), None),
    "spectrum_mask.mixed": (lambda T, kw: S.spectrum_mask(T(Z), MASK, **kw), None),
    "istft_masked": (lambda T, kw: S.istft_masked(T(Z), T(MASK), W, overlap_length=12, **kw),
                     lambda T, kw: S.istft_masked(T(Z), T(MASK), W[:8], overlap_length=4, **kw)),
    "mel_spectrogram": (lambda T, kw: S.mel_spectrogram(T(X), W, mel_bins=4, **ST, **kw),
                        lambda T, kw: S.mel_spectrogram(T(X), W, mel_bins=4, bogus=1, **kw)),
    "spectrogram": (lambda T, kw: S.spectrogram(T(X), W, kind="dbfs", **ST, **kw), lambda T, kw: S.spectrogram(T(X), W, kind="bogus", **kw)),
    "spectrogram.defaults": (lambda T, kw: S.spectrogram(T(X), W, **kw), lambda T, kw: S.spectrogram(T(X), W, window_padding="zeros", **kw)),
    "convolve.direct": (lambda T, kw: Cv.convolve(T(ND), T(ND[:2, :3].copy()), mode="same", **kw),
                        lambda T, kw: Cv.convolve(T(ND), T(TAPS), **kw)),
    "convolve.scalar": (lambda T, kw: Cv.convolve(T(np.float32(2)), T(np.float32(3)), **kw), None),
    "convolve.fft": (lambda T, kw: Cv.convolve(T(X), TAPS, method="fft", mode="same", **kw), lambda T, kw: Cv.convolve(T(X), TAPS, mode="bogus", **kw)),
    "correlate": (lambda T, kw: Cv.correlate(T(ND), ND[:2, :3].astype(np.complex64), mode="valid", **kw),
                  lambda T, kw: Cv.correlate(T(ND), ND[:2, :3], method="bogus", **kw)),
    "fftconvolve": (lambda T, kw: Cv.fftconvolve(T(X), TAPS, **kw), lambda T, kw: Cv.fftconvolve(T(X), TAPS, bogus=1, **kw)),
    "fftconvolve.short": (lambda T, kw: Cv.fftconvolve(T(TAPS[:3].copy()), TAPS, mode="same", **kw), None),
    "fftconvolve.c64": (lambda T, kw: Cv.fftconvolve(T(T1.astype(np.complex64)), TAPS, mode="valid", **kw), None),
    "fftconvolve.nd": (lambda T, kw: Cv.fftconvolve(T(ND), ND[:2, :3], mode="same", **kw), lambda T, kw: Cv.fftconvolve(T(ND), Z, **kw)),
    "fftconvolve.f64": (lambda T, kw: Cv.fftconvolve(T(X.astype(np.float64)), TAPS, **kw), None),
    "fftconvolve.device_taps": (lambda T, kw: Cv.fftconvolve(X, T(TAPS), **kw), None),
    "fft_nd": (lambda T, kw: Tr.fft_nd(T(ND), **kw), lambda T, kw: Tr.fft_nd(T(ND), axes=[0, 1], lengths=[4], **kw)),
    "fft_nd.axes": (lambda T, kw: Tr.fft_nd(T(ND.astype(np.complex64)), axes=[0, -1], lengths=[None, 16], **kw),
                    None),
    "fft_nd.f64": (lambda T, kw: Tr.fft_nd(T(ND.astype(np.float64)), lengths=[16], **kw), None),
    "ifft_nd": (lambda T, kw: Tr.ifft_nd(T(ND), axes=[0, 1], **kw), lambda T, kw: Tr.ifft_nd(T(ND), bogus=1, **kw)),
    "fir": (lambda T, kw: F.fir(T(X), TAPS, **kw), lambda T, kw: F.fir(T(X), TAPS, mode="bogus", **kw)),
    "median": (lambda T, kw: F.median(T(ND), kernel_shape=(3, 3), **kw), lambda T, kw: F.median(T(ND), kernel_shape=(3,), **kw)),
    "median.f64": (lambda T, kw: F.median(T(ND.astype(np.float64)), kernel_shape=(1, 2), **kw), None),
    "median.s32": (lambda T, kw: F.median(T(ND.astype(np.int32)), kernel_shape=(1, 2), **kw), None),
    "wiener": (lambda T, kw: F.wiener(T(ND), **kw), lambda T, kw: F.wiener(T(ND), kernel_size=(3,), **kw)),
    "wiener.noise": (lambda T, kw: F.wiener(T(ND.astype(np.float64)), return_noise=True, noise=0.5, kernel_size=(3, 1), **kw),
                     lambda T, kw: F.wiener(T(ND), noise="x", **kw)),
    "resample_poly": (lambda T, kw: F.resample_poly(T(X), 3, 2, **kw), lambda T, kw: F.resample_poly(T(X), 3, 0, **kw)),
    "resample_poly.axis0": (lambda T, kw: F.resample_poly(T(X.astype(np.complex64)), 2, 4, axis=0, taps=TAPS, **kw),
                            lambda T, kw: F.resample_poly(T(X), 3, 2, padtype="line", **kw)),
    "resample_poly.copy": (lambda T, kw: F.resample_poly(T(X), 3, 3, window="hann", **kw), None),
    "sosfilt": (lambda T, kw: F.sosfilt(T(X), SOS, **kw), lambda T, kw: F.sosfilt(T(X), SOS, direction=2, **kw)),
    "sosfilt.zi": (lambda T, kw: F.sosfilt(T(X), SOS, zi=np.zeros((1, 2, 2)), direction=1, **kw),
                   lambda T, kw: F.sosfilt(T(X), SOS, zi=np.zeros((1, 2)), **kw)),
    "sosfilt.groups": (lambda T, kw: F.sosfilt(T(X), np.repeat(SOS, 17, 0), zi=np.zeros((17, 2, 2)), **kw), None),
    "sosfilt.axis0": (lambda T, kw: F.sosfilt(T(X), SOS, axis=0, **kw), lambda T, kw: F.sosfilt(T(X), SOS[:, :5], **kw)),
    "sosfiltfilt": (lambda T, kw: F.sosfiltfilt(T(X), SOS, **kw), lambda T, kw: F.sosfiltfilt(T(X), SOS, padtype="bogus", **kw)),
    "sosfiltfilt.padlen": (lambda T, kw: F.sosfiltfilt(T(X), np.repeat(SOS, 2, 0), padtype="even", padlen=5, axis=-1, **kw),
                           lambda T, kw: F.sosfiltfilt(T(X), SOS, padlen=64, **kw)),
    "welch": (lambda T, kw: Sp.welch(T(X), W, overlap_length=12, sampling_rate=100.0, **kw), lambda T, kw: Sp.welch(T(X), W, detrend="linear", **kw)),
    "welch.options": (lambda T, kw: Sp.welch(T(X), W, fft_length=32, detrend=False, scaling="spectrum", **kw),
                      lambda T, kw: Sp.welch(T(X.astype(np.float64)), W, **kw)),
    "csd": (lambda T, kw: Sp.csd(T(X), T(Y), W, overlap_length=12, **kw), lambda T, kw: Sp.csd(T(X), T(Y[:1]), W, **kw)),
    "csd.auto": (lambda T, kw: Sp.csd(T(X), T(Y), W, return_auto=True, **kw), lambda T, kw: Sp.csd(T(X), T(Y), W, bogus=1, **kw)),
    "csd.mixed": (lambda T, kw: Sp.csd(T(X), Y, W, **kw), None),
    "coherence": (lambda T, kw: Sp.coherence(T(X), T(Y), W, overlap_length=12, **kw), lambda T, kw: Sp.coherence(T(X), T(Y), W[:0], **kw)),
    "sawtooth": (lambda T, kw: Wv.sawtooth(T(X), width=0.5, **kw), lambda T, kw: Wv.sawtooth(T(X), width=2, **kw)),
    "sawtooth.f64": (lambda T, kw: Wv.sawtooth(T(X.astype(np.float64)), **kw), None),
    "sawtooth.s32": (lambda T, kw: Wv.sawtooth(T(X.astype(np.int32)), **kw), lambda T, kw: Wv.sawtooth(T(Z), **kw)),
    "square": (lambda T, kw: Wv.square(T(X), **kw), lambda T, kw: Wv.square(T(X), duty="x", **kw)),
    "square.duty": (lambda T, kw: Wv.square(T(X), duty=T(np.abs(X) / 4), **kw), lambda T, kw: Wv.square(T(X), duty=T(X[:1]), **kw)),
    "square.mixed": (lambda T, kw: Wv.square(T(X), duty=np.abs(X) / 4, **kw), None),
    "gaussian_pulse": (lambda T, kw: Wv.gaussian_pulse(T(X), center_frequency=5, **kw), lambda T, kw: Wv.gaussian_pulse(T(X), bandwidth=0, **kw)),
    "chirp": (lambda T, kw: Wv.chirp(T(X), 1, 10, 20, method="quadratic", vertex_zero=False, **kw),
              lambda T, kw: Wv.chirp(T(X), 1, 10, 20, method="bogus", **kw)),
    "polynomial_sweep": (lambda T, kw: Wv.polynomial_sweep(T(T1), [1, 2, 3], phi=90, phi_unit="degrees", **kw),
                         lambda T, kw: Wv.polynomial_sweep(T(X), [1, 2, 3], **kw)),
    "argrelmin": (lambda T, kw: Pk.argrelmin(T(ND), **kw), lambda T, kw: Pk.argrelmin(T(ND), axis=2, **kw)),
    "argrelmax": (lambda T, kw: Pk.argrelmax(T(ND.astype(np.int64)), axis=1, order=2, **kw), lambda T, kw: Pk.argrelmax(T(ND), order="x", **kw)),
    "argrelmax.s16": (lambda T, kw: Pk.argrelmax(T(ND.astype(np.int16)), axis=-1, order=0, **kw), None),
    "argrelextrema": (lambda T, kw: Pk.argrelextrema(T(ND), "greater_equal", order=2.5, **kw),
                      lambda T, kw: Pk.argrelextrema(T(ND), "bogus", **kw)),
    "argrelextrema.ufunc": (lambda T, kw: Pk.argrelextrema(T(ND.astype(np.float64)), np.less_equal, **kw),
                            lambda T, kw: Pk.argrelextrema(T(Z), np.less, **kw)),
    "argrelextrema.custom": (lambda T, kw: Pk.argrelextrema(T(ND), lambda a, b: a > b + 1, axis=1, **kw),
                             lambda T, kw: Pk.argrelextrema(T(ND), 3, **kw)),
    "nonzero": (lambda T, kw: Pk.nonzero(ND > 0, **kw), lambda T, kw: Pk.nonzero(np.ones((1,) * 9), **kw)),
    "unit_impulse": (lambda T, kw: Wv.unit_impulse((4, 8), index="midpoint", **kw), lambda T, kw: Wv.unit_impulse((4, 8), index=[4, 0], **kw)),
    "unit_impulse.device": (lambda T, kw: Wv.unit_impulse((4, 8), device=True, index=[1, 2], type="s64", **kw),
                            lambda T, kw: Wv.unit_impulse((4, 8), type="s8", **kw)),
    "unit_impulse.empty": (lambda T, kw: Wv.unit_impulse((4, 0), index=[0, 0], **kw), None),
}
_NO_TENSOR = {"nonzero", "unit_impulse", "unit_impulse.device", "unit_impulse.empty"}   # one operand kind is enough

# the functions that never see a context: one call each, and an invalid one
PLAIN_CASES = {
    "fft_frequencies": (lambda: S.fft_frequencies(100, fft_length=16), lambda: S.fft_frequencies(100)),
    "fft_frequencies.f64": (lambda: S.fft_frequencies(100, fft_length=16, type="f64", endpoint=True), lambda: S.fft_frequencies(100, fft_length=16, type="s8")),
    "mel_filters": (lambda: S.mel_filters(16, 4, 100), lambda: S.mel_filters(16, 4, 100, type="f64")),
    "firwin": (lambda: F.firwin(5, [0.25]), lambda: F.firwin(5, 0.25)),
    "firwin.kaiser": (lambda: F.firwin(5, [0.2, 0.4], window=("kaiser", 5.0), pass_zero=False, type="f64"), lambda: F.firwin(5, [0.25], bogus=1)),
    "resample_poly_taps": (lambda: F.resample_poly_taps(3, 2), lambda: F.resample_poly_taps(0, 2)),
    "sosfilt_zi": (lambda: F.sosfilt_zi(SOS), lambda: F.sosfilt_zi(SOS[0])),
    "spectral.frequencies": (lambda: Sp.frequencies(16, 100.0), None),
    "sinc": (lambda: Wv.sinc([0.0, 0.5]), None),
    "sinc.f64": (lambda: Wv.sinc(np.array([0.0, 0.5])), None),
    "windows.rectangular": (lambda: Wi.rectangular(16), lambda: Wi.rectangular(16, name="w")),
    "windows.bartlett": (lambda: Wi.bartlett(16), lambda: Wi.bartlett(16, name="w")),
    "windows.triangular": (lambda: Wi.triangular(16, type="f64"), lambda: Wi.triangular(1.5)),
    "windows.blackman": (lambda: Wi.blackman(16, is_periodic=False), lambda: Wi.blackman(16, type="s8")),
    "windows.hamming": (lambda: Wi.hamming(16), lambda: Wi.hamming(16, bogus=1)),
    "windows.hann": (lambda: Wi.hann(16), lambda: Wi.hann(16, bogus=1)),
    "windows.kaiser": (lambda: Wi.kaiser(16, beta=5.0), lambda: Wi.kaiser(16, bogus=1)),
}


def _boom(device=0):
    raise RuntimeError("default_context() reached before the argument error")


def transcript(parent):
    world = World()
    try:
        cases = {}
        for name, (ok, bad) in TENSOR_CASES.items():
            for kind in (("host",) if name in _NO_TENSOR else ("host", "buf", "cai")):
                for with_ctx in (False, True):
                    cases[f"{name}[{kind}{'+ctx' if with_ctx else ''}]"] = world.run(ok, kind, with_ctx)
        for name, (ok, bad) in PLAIN_CASES.items():
            cases[name] = world.run(lambda T, kw: ok(), "host", False)
        world.patch_default(_boom)
        for name, (ok, bad) in TENSOR_CASES.items():
            if bad is not None:
                cases[f"{name}[invalid]"] = world.run(bad, "host", False)
        for name, (ok, bad) in PLAIN_CASES.items():
            if bad is not None:
                cases[f"{name}[invalid]"] = world.run(lambda T, kw: bad(), "host", False)
    finally:
        world.close()
    rows = ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items())
    return f'{{"parent": {json.dumps(parent)}, "cases": {{\n{rows}\n}}}}\n'


def test_the_table_covers_every_public_function():
    import inspect

    mods = {"": S, "filters": F, "convolution": Cv, "transforms": Tr, "spectral": Sp, "waveforms": Wv, "peak_finding": Pk, "windows": Wi}
    skip = {"default_context"}   # hands out a context; the cases patch it
    have = {k.split(".")[0] for k in TENSOR_CASES} | {k.split(".")[-1] if k.startswith(("windows.", "spectral.")) else k.split(".")[0]
                                                     for k in PLAIN_CASES}
    missing = []
    for prefix, mod in mods.items():
        for name, fn in vars(mod).items():
            if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != mod.__name__ or name in skip:
                continue
            if name not in have:
                missing.append(f"{prefix}.{name}" if prefix else name)
    assert not missing, missing


def test_the_package_reproduces_the_recorded_transcript():
    with open(GOLDEN) as f:
        want = f.read()
    got = transcript(json.loads(want)["parent"])
    if got != want:
        a, b = json.loads(want)["cases"], json.loads(got)["cases"]
        diff = [k for k in a if a[k] != b.get(k)] + [k for k in b if k not in a]
        k = diff[0] if diff else None
        raise AssertionError(f"{len(diff)} cases differ from {GOLDEN}: {diff[:20]}\nfirst, recorded: {a.get(k)}\nfirst, now:      {b.get(k)}")


def _timing():
    world = World()
    try:
        c = world.ctx["caller"]
        sos = np.repeat(SOS, 1, 0)
        for name, fn in (("stft", lambda: S.stft(X, W, ctx=c, **ST)), ("filters.sosfilt", lambda: F.sosfilt(X, sos, ctx=c)),
                         ("waveforms.sawtooth", lambda: Wv.sawtooth(X, ctx=c))):
            for _ in range(200):
                fn()
            ts = []
            for _ in range(2000):
                world.rec.calls.clear()
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            print(f"{name}: median {np.median(ts) * 1e6:.2f} us over {len(ts)} calls")
    finally:
        world.close()


if __name__ == "__main__":
    if "--time" in sys.argv:
        _timing()
    else:
        path, parent = sys.argv[sys.argv.index("--write") + 1], sys.argv[sys.argv.index("--parent") + 1]
        with open(path, "w") as f:
            f.write(transcript(parent))
        print(f"wrote {path}")
