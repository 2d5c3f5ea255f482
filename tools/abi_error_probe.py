"""Error table of the C ABI: every compute entry point of include/nxsig.h is called with small valid arguments and then with ONE
argument broken at a time; the return code, nxsig_last_error() and what landed in *num_frames_out are recorded per case.

    python tools/abi_error_probe.py [--lib PATH] [--real] [--write tests/golden/abi_error_table.json]
    python tools/abi_error_probe.py --own [--real] [--write tests/golden/abi_error_table_resample.json]
    python tools/abi_error_probe.py --welch [--real] [--write tests/golden/abi_error_table_welch.json]
    python tools/abi_error_probe.py --iir [--real] [--write tests/golden/abi_error_table_iir.json]
    python tools/abi_error_probe.py --peaks [--real] [--write tests/golden/abi_error_table_find_peaks.json]
    python tools/abi_error_probe.py --savgol [--real] [--write tests/golden/abi_error_table_savgol.json]
    python tools/abi_error_probe.py --hilbert [--real] [--write tests/golden/abi_error_table_hilbert.json]
    python tools/abi_error_probe.py --dct [--real] [--write tests/golden/abi_error_table_dct.json]
    python tools/abi_error_probe.py --lfilter [--real] [--write tests/golden/abi_error_table_lfilter.json]
    python tools/abi_error_probe.py --lombscargle [--real] [--write tests/golden/abi_error_table_lombscargle.json]
    python tools/abi_error_probe.py --czt [--real] [--write tests/golden/abi_error_table_czt.json]
    python tools/abi_error_probe.py --cwt [--real] [--write tests/golden/abi_error_table_cwt.json]
    python tools/abi_error_probe.py --xcorr [--real] [--write tests/golden/abi_error_table_xcorr.json]

Without --real every call gets ctx = NULL (needs no GPU): entry points that look at the context first answer "null context", the ones
that validate first answer with the argument's own message.  With --real a context on device 0 is used: every broken case returns
before anything is launched (the probe refuses a broken case that returns 0), and the valid row of each entry point runs once with
NXSIG_HOST and once with NXSIG_DEVICE, the two results compared bit for bit.  The golden file holds both tables; regenerate it from
the build whose behaviour is the reference (tests/test_abi_errors_host.py and tests/test_gpu_abi_errors.py compare against it).

ENTRIES and that golden file are the recorded table of the entry points that existed when it was made.  An entry point added since
keeps its rows in OWN_TABLE_ENTRIES and a golden file of its own (--own; tests/test_resample_host.py and tests/test_gpu_resample.py
compare against it): the same probe, the same kinds of cases.  WELCH_TABLE_ENTRIES (--welch) does the same for nxsig_welch_f32 and
nxsig_csd_f32 (tests/test_welch_host.py, tests/test_gpu_welch.py), IIR_TABLE_ENTRIES (--iir) for nxsig_sosfilt_f32 and
nxsig_sosfiltfilt_f32 (tests/test_iir_host.py, tests/test_gpu_iir.py), PEAKS_TABLE_ENTRIES (--peaks) for nxsig_find_peaks
(tests/test_find_peaks_host.py, tests/test_gpu_find_peaks.py), SAVGOL_TABLE_ENTRIES (--savgol) for nxsig_savgol_filter
(tests/test_savgol_host.py, tests/test_gpu_savgol.py), HILBERT_TABLE_ENTRIES (--hilbert) for nxsig_hilbert_f32
(tests/test_hilbert_host.py, tests/test_gpu_hilbert.py), DCT_TABLE_ENTRIES (--dct) for nxsig_dct_f32 (tests/test_dct_host.py,
tests/test_gpu_dct.py), LFILTER_TABLE_ENTRIES (--lfilter) for nxsig_lfilter_f32 and nxsig_filtfilt_f32 (tests/test_lfilter_host.py,
tests/test_gpu_lfilter.py), LOMBSCARGLE_TABLE_ENTRIES (--lombscargle) for nxsig_lombscargle (tests/test_lombscargle_host.py,
tests/test_gpu_lombscargle.py), CZT_TABLE_ENTRIES (--czt) for nxsig_czt (tests/test_czt_host.py, tests/test_gpu_czt.py), CWT_TABLE_ENTRIES (--cwt) for nxsig_fir_bank
and nxsig_cwt (tests/test_cwt_host.py, tests/test_gpu_cwt.py), XCORR_TABLE_ENTRIES (--xcorr) for nxsig_xcorr (tests/test_xcorr_host.py,
tests/test_gpu_xcorr.py)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from nx_signal_amd import _lib  # noqa: E402  (signature table + structs only)

GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_error_table.json")
GOLDEN_OWN = os.path.join(ROOT, "tests", "golden", "abi_error_table_resample.json")
GOLDEN_WELCH = os.path.join(ROOT, "tests", "golden", "abi_error_table_welch.json")
GOLDEN_IIR = os.path.join(ROOT, "tests", "golden", "abi_error_table_iir.json")
GOLDEN_PEAKS = os.path.join(ROOT, "tests", "golden", "abi_error_table_find_peaks.json")
GOLDEN_SAVGOL = os.path.join(ROOT, "tests", "golden", "abi_error_table_savgol.json")
GOLDEN_HILBERT = os.path.join(ROOT, "tests", "golden", "abi_error_table_hilbert.json")
GOLDEN_DCT = os.path.join(ROOT, "tests", "golden", "abi_error_table_dct.json")
GOLDEN_LFILTER = os.path.join(ROOT, "tests", "golden", "abi_error_table_lfilter.json")
GOLDEN_LOMBSCARGLE = os.path.join(ROOT, "tests", "golden", "abi_error_table_lombscargle.json")
GOLDEN_CZT = os.path.join(ROOT, "tests", "golden", "abi_error_table_czt.json")
GOLDEN_CWT = os.path.join(ROOT, "tests", "golden", "abi_error_table_cwt.json")
GOLDEN_XCORR = os.path.join(ROOT, "tests", "golden", "abi_error_table_xcorr.json")
NF_SENTINEL = -7   # *num_frames_out before every call: a case that leaves it alone reports this value
NULL_ONLY = "null-ctx only"   # a broken value this entry point accepts: with a real context it would launch, so it runs with ctx = NULL alone

_rng = np.random.Generator(np.random.PCG64(7))


def _f32(*shape):
    return _rng.standard_normal(shape).astype(np.float32)


def _c64(*shape):
    return (_rng.standard_normal(shape) + 1j * _rng.standard_normal(shape)).astype(np.complex64)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            continue
        f.restype, f.argtypes = res, args
    return lib


# ---- the table.  An entry: (symbol, [(arg, kind, value)], [(label, {arg: broken value}[, NULL_ONLY])]).  Kinds:
#   in / out    tensor operand: a host array with NXSIG_HOST, a device copy with NXSIG_DEVICE        (+ "?": may be NULL)
#   host / hout array that is always read / written on the host (window, taps, shapes, noise_used)   (+ "?": may be NULL)
#   p           nxsig_stft_params as a dict; a case breaks one field as "p.<field>"
#   nf          int64_t* num_frames_out          v  scalar          mem  NXSIG_HOST / NXSIG_DEVICE
# Every required pointer gets a "null <arg>" case and every entry a "mem=7" case on top of the listed ones.
N, HOP, K, L, B, M = 8, 4, 8, 20, 2, 4
WIN = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)   # no zero sample: the OLA normaliser stays finite
PARAMS = dict(frame_length=N, hop=HOP, fft_length=K, pad_mode=_lib.PAD_VALID, pad_lo=0, pad_hi=0, scaling=_lib.SCALE_NONE, reserved=0,
              sampling_rate=48000.0)


def _stft_cases(bounded, min_fft, odd_ok=True):
    return [("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536}) + (() if bounded else (NULL_ONLY,)),
            ("batch_stride=length-1", {"batch_stride": L - 1}), ("fft_length=0", {"p.fft_length": 0}),
            ("fft_length=1", {"p.fft_length": 1}) + (() if min_fft >= 2 else (NULL_ONLY,)),
            ("fft_length=7", {"p.fft_length": 7}) + ((NULL_ONLY,) if odd_ok else ()),
            ("scaling=9", {"p.scaling": 9}), ("hop=0", {"p.hop": 0}), ("frame_length>length", {"p.frame_length": 32}),
            ("frame_length=0", {"p.frame_length": 0}), ("pad_mode=9", {"p.pad_mode": 9}), ("length=0", {"length": 0})]


def _stft(name, x, out, bounded, min_fft, odd_ok=True, extra=(), more=(), window=WIN, wflag=()):
    args = [("x", "in", x), ("length", "v", L), ("batch", "v", B), ("batch_stride", "v", L), ("window", "host", window), *wflag,
            ("p", "p", PARAMS), *extra, ("out", "out", out), ("nf", "nf", None), ("mem", "mem", None)]
    return (name, args, _stft_cases(bounded, min_fft, odd_ok) + list(more))


_ISTFT_CASES = [("batch=0", {"batch": 0}), ("num_frames=0", {"num_frames": 0}), ("scaling=9", {"p.scaling": 9}),
                ("frame_length=0", {"p.frame_length": 0}), ("hop=0", {"p.hop": 0}), ("hop>frame_length", {"p.hop": 9}),
                ("fft_length!=frame_length", {"p.fft_length": 16})]


def _istft(name, z, y, bounded, extra=(), more=(), window=WIN, wflag=()):
    args = [("z", "in", z), ("num_frames", "v", M), ("batch", "v", B), ("window", "host", window), *wflag, ("p", "p", PARAMS), *extra,
            ("y", "out", y), ("mem", "mem", None)]
    return (name, args, _ISTFT_CASES + [("batch=65536", {"batch": 65536}) + (() if bounded else (NULL_ONLY,))] + list(more))


_MASK_CASES = [("mask_kind=9", {"mask_kind": 9}), ("z_rows=0", {"z_rows": 0}), ("z_rows=2 mask_rows=3", {"mask_rows": 3}),
               ("z_rows=65536", {"z_rows": 65536, "mask_rows": 1})]
_OLA_CASES = [("components=3", {"components": 3}), ("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536}),
              ("num_frames=0", {"num_frames": 0}), ("frame_length=0", {"frame_length": 0}), ("overlap=frame_length", {"overlap_length": N}),
              ("overlap=-1", {"overlap_length": -1})]
_FRAMING_CASES = [("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536}), ("batch_stride=length-1", {"batch_stride": L - 1}),
                  ("window_length=0", {"window_length": 0}), ("stride=0", {"stride": 0}), ("window_length>length", {"window_length": 32}),
                  ("pad_mode=9", {"pad_mode": 9}), ("length=0", {"length": 0})]


def _framing(name, dt):
    return (name, [("x", "in", _f32(B, L).astype(dt)), ("length", "v", L), ("batch", "v", B), ("batch_stride", "v", L), ("window_length", "v", N),
                   ("stride", "v", HOP), ("pad_mode", "v", _lib.PAD_VALID), ("pad_lo", "v", 0), ("pad_hi", "v", 0),
                   ("out", "out", np.zeros((B, M, N), dt)), ("nf", "nf", None), ("mem", "mem", None)], _FRAMING_CASES)


def _ola(name, dt):
    return (name, [("frames", "in", _f32(B, M, N).astype(dt)), ("num_frames", "v", M), ("batch", "v", B), ("frame_length", "v", N),
                   ("overlap_length", "v", N - HOP), ("components", "v", 1), ("out", "out", np.zeros((B, M * HOP + N - HOP), dt)),
                   ("mem", "mem", None)], _OLA_CASES)


FL, TAPS = 16, 3


def _fir(name, dt, bounded, slice_):
    tail = [("out_start", "v", 1), ("out_len", "v", FL)] if slice_ else [("mode", "v", _lib.CONV_SAME)]
    cases = [("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536}) + (() if bounded else (NULL_ONLY,)),
             ("batch_stride=length-1", {"batch_stride": FL - 1}), ("length=0", {"length": 0}), ("num_taps=0", {"num_taps": 0})]
    cases += [("out_start=-1", {"out_start": -1}), ("out_len=0", {"out_len": 0}), ("slice past the end", {"out_start": 3})] if slice_ else [("mode=9", {"mode": 9})]
    return (name, [("x", "in", _f32(B, FL).astype(dt)), ("length", "v", FL), ("batch", "v", B), ("batch_stride", "v", FL),
                   ("h", "host", _f32(TAPS).astype(dt)), ("num_taps", "v", TAPS), *tail, ("y", "out", np.zeros((B, FL), dt)), ("mem", "mem", None)], cases)


def _fft(name, dt, cdt):
    return (name, [("in", "in", _f32(2, 8).astype(dt)), ("in_is_real", "v", 1), ("rows", "v", 2), ("n_in", "v", 8), ("fft_length", "v", 8),
                   ("inverse", "v", 0), ("out", "out", np.zeros((2, 8), cdt)), ("mem", "mem", None)],
            [("rows=0", {"rows": 0}), ("n_in=0", {"n_in": 0}), ("fft_length=0", {"fft_length": 0})])


def _conv_nd(name):
    return (name, [("a", "in", _f32(4, 4)), ("a_is_real", "v", 1), ("a_shape", "host", _i64(4, 4)), ("b", "in", _f32(2, 4)), ("b_is_real", "v", 1),   # (2, 2) of it
                   ("b_shape", "host", _i64(2, 2)), ("rank", "v", 2), ("mode", "v", _lib.CONV_FULL), ("out", "out", np.zeros((5, 5), np.float32)),
                   ("out_shape", "hout?", _i64(0, 0)), ("mem", "mem", None)],
            [("rank=0", {"rank": 0}), ("rank=9", {"rank": 9}), ("empty dimension", {"a_shape": _i64(4, 0)}), ("mode=9", {"mode": 9}),
             ("valid mode, neither contains the other", {"mode": _lib.CONV_VALID, "b_shape": _i64(1, 5)})])


def _wave(name, mid, cases, out=None):
    return (name, [("t", "in", np.linspace(0, 1, 8, dtype=np.float32)), ("is_f64", "v", 0), ("n", "v", 8), *mid,
                   ("out", "out", np.zeros(8, np.float32) if out is None else out), ("mem", "mem", None)], [("n=-1", {"n": -1})] + cases)


_PEAK_SHAPE_CASES = [("rank=0", {"rank": 0}), ("rank=9", {"rank": 9}), ("empty dimension", {"shape": _i64(0)}),
                     ("dimension 2^31", {"shape": _i64(1 << 31)}), ("2^32 elements", {"shape": _i64(1 << 30, 4), "rank": 2})]
_X8 = np.array([0, 2, 1, 3, 0, 5, 4, 4], np.float32)

ENTRIES = [
    _stft("nxsig_stft_f32", _f32(B, L), np.zeros((B, M, K), np.complex64), False, 1),
    _stft("nxsig_stft_c64", _c64(B, L), np.zeros((B, M, K), np.complex64), False, 1),
    _stft("nxsig_stft_onesided_f32", _f32(B, L), np.zeros((B, M, K // 2), np.complex64), True, 2),
    _stft("nxsig_stft_packed_f32", _f32(B, L), np.zeros((B, M, K // 2), np.complex64), True, 2, odd_ok=False),
    _stft("nxsig_stft_magnitude_f32", _f32(B, L), np.zeros((B, M, K // 2), np.float32), True, 2, extra=[("kind", "v", _lib.MAG_POWER)],
          more=[("kind=9", {"kind": 9})]),
    _stft("nxsig_stft_mel_f32", _f32(B, L), np.zeros((B, M, 4), np.float32), True, 2,
          extra=[("mel_bins", "v", 4), ("filters", "host", np.abs(_f32(K, 4)))], more=[("mel_bins=0", {"mel_bins": 0})]),
    _istft("nxsig_istft_c64", _c64(B, M, K), np.zeros((B, M * HOP + N - HOP), np.complex64), False),
    _istft("nxsig_istft_packed_f32", _c64(B, M, K // 2), np.zeros((B, M * HOP + N - HOP), np.float32), True,
           more=[("fft_length=7", {"p.fft_length": 7, "p.frame_length": 7})]),
    _istft("nxsig_istft_filtered_c64", _c64(B, M, K), np.zeros((B, M * HOP + N - HOP), np.complex64), True, extra=[("h", "host", _c64(K))]),
    ("nxsig_istft_masked_c64",
     [("z", "in", _c64(B, M, K)), ("z_rows", "v", B), ("num_frames", "v", M), ("window", "host", WIN), ("p", "p", PARAMS),
      ("mask", "in", np.abs(_f32(B, M, K))), ("mask_kind", "v", 0), ("mask_rows", "v", B), ("y", "out", np.zeros((B, M * HOP + N - HOP), np.complex64)),
      ("mem", "mem", None)],
     _MASK_CASES + [("one-sided mask, fft_length=7", {"mask_kind": 1, "p.fft_length": 7, "p.frame_length": 7})] +
     [c for c in _ISTFT_CASES if c[0] != "batch=0"]),
    ("nxsig_spectrum_mask_c64",
     [("z", "in", _c64(B, M, K)), ("z_rows", "v", B), ("mask", "in", np.abs(_f32(B, M, K))), ("mask_kind", "v", 0), ("mask_rows", "v", B),
      ("num_frames", "v", M), ("fft_length", "v", K), ("out", "out", np.zeros((B, M, K), np.complex64)), ("mem", "mem", None)],
     _MASK_CASES + [("one-sided mask, fft_length=7", {"mask_kind": 1, "fft_length": 7}), ("num_frames=0", {"num_frames": 0}),
                    ("fft_length=0", {"fft_length": 0})]),
    _framing("nxsig_as_windowed_f32", np.float32),
    _ola("nxsig_overlap_and_add", np.float32),
    _fft("nxsig_fft", np.float32, np.complex64),
    _fir("nxsig_fir_f32", np.float32, False, False),
    _fir("nxsig_fir_slice_f32", np.float32, False, True),
    ("nxsig_fftconvolve_c64",
     [("a", "in", _c64(8)), ("n1", "v", 8), ("b", "in", _c64(3)), ("n2", "v", 3), ("mode", "v", _lib.CONV_FULL), ("out", "out", np.zeros(10, np.complex64)),
      ("mem", "mem", None)], [("n1=0", {"n1": 0}), ("n2=0", {"n2": 0}), ("mode=9", {"mode": 9})]),
    ("nxsig_stft_to_mel",
     [("z", "in", _c64(M, K)), ("rows", "v", M), ("fft_length", "v", K), ("mel_bins", "v", 4), ("filters", "host", np.abs(_f32(K, 4))),
      ("out", "out", np.zeros((M, 4), np.float32)), ("mem", "mem", None)],
     [("rows=0", {"rows": 0}), ("fft_length=1", {"fft_length": 1}), ("mel_bins=0", {"mel_bins": 0}), ("fft_length=16386", {"fft_length": 16386})]),
    ("nxsig_spectrum_mul_c64",
     [("z", "in", _c64(M, K)), ("rows", "v", M), ("fft_length", "v", K), ("h", "host", _c64(K)), ("out", "out", np.zeros((M, K), np.complex64)),
      ("mem", "mem", None)], [("rows=-1", {"rows": -1}), ("fft_length=0", {"fft_length": 0})]),
    ("nxsig_fft_nd",
     [("in", "in", _f32(4, 4)), ("in_is_real", "v", 1), ("shape", "host", _i64(4, 4)), ("rank", "v", 2), ("axes", "host", np.array([0, 1], np.int32)),
      ("lengths", "host", _i64(4, 4)), ("n_axes", "v", 2), ("inverse", "v", 0), ("out", "out", np.zeros((4, 4), np.complex64)), ("mem", "mem", None)],
     [("rank=0", {"rank": 0}), ("rank=9", {"rank": 9}), ("n_axes=17", {"n_axes": 17}), ("empty dimension", {"shape": _i64(4, 0)}),
      ("axis=5", {"axes": np.array([0, 5], np.int32)}), ("lengths=0", {"lengths": _i64(4, 0)})]),
    _conv_nd("nxsig_fftconvolve_nd"),
    _conv_nd("nxsig_convolve_direct"),
    ("nxsig_median_filter",
     [("x", "in", _f32(4, 4)), ("is_f64", "v", 0), ("shape", "host", _i64(4, 4)), ("rank", "v", 2), ("kernel_shape", "host", _i64(3, 3)),
      ("out", "out", np.zeros((4, 4), np.float32)), ("mem", "mem", None)],
     [("rank=0", {"rank": 0}), ("rank=9", {"rank": 9}), ("empty dimension", {"shape": _i64(4, 0)}), ("kernel_shape=0", {"kernel_shape": _i64(3, 0)}),
      ("kernel_shape>dimension", {"kernel_shape": _i64(3, 5)})]),
    ("nxsig_wiener",
     [("x", "in", _f32(4, 4)), ("is_f64", "v", 0), ("shape", "host", _i64(4, 4)), ("rank", "v", 2), ("kernel_size", "host", _i64(3, 3)),
      ("has_noise", "v", 0), ("noise", "v", 0.0), ("out", "out", np.zeros((4, 4), np.float32)), ("noise_used", "hout?", np.zeros(1, np.float64)),
      ("mem", "mem", None)],
     [("rank=0", {"rank": 0}), ("rank=9", {"rank": 9}), ("empty dimension", {"shape": _i64(4, 0)}), ("kernel_size=0", {"kernel_size": _i64(3, 0)})]),
    ("nxsig_argrelextrema",
     [("x", "in", _X8), ("dtype", "v", _lib.DT_F32), ("shape", "host", _i64(8)), ("rank", "v", 1), ("axis", "v", 0), ("shifts", "v", 1),
      ("comparator", "v", _lib.CMP_GREATER), ("indices", "out", np.zeros((8, 1), np.int32)), ("valid", "out", np.zeros(1, np.uint32)), ("mem", "mem", None)],
     _PEAK_SHAPE_CASES + [("axis=1", {"axis": 1}), ("axis=-1", {"axis": -1}), ("dtype=9", {"dtype": 9}), ("comparator=9", {"comparator": 9})]),
    ("nxsig_nonzero",
     [("mask", "in", (_X8 > 2).astype(np.uint8)), ("shape", "host", _i64(8)), ("rank", "v", 1), ("indices", "out", np.zeros((8, 1), np.int32)),
      ("valid", "out", np.zeros(1, np.uint32)), ("mem", "mem", None)], _PEAK_SHAPE_CASES),
    _wave("nxsig_sawtooth", [("width", "v", 0.5)], [("width=2", {"width": 2.0}), ("width=nan", {"width": float("nan")})]),
    _wave("nxsig_square", [("duty", "v", 0.5), ("duty_tensor", "in?", None)], [], out=np.zeros(8, np.int32)),
    ("nxsig_gaussian_pulse",
     [("t", "in", np.linspace(-1, 1, 8, dtype=np.float32)), ("is_f64", "v", 0), ("n", "v", 8), ("center_frequency", "v", 1.0), ("bandwidth", "v", 0.5),
      ("bandwidth_reference_level", "v", -6.0), ("envelope", "out", np.zeros(8, np.float32)), ("in_phase", "out", np.zeros(8, np.float32)),
      ("quadrature", "out", np.zeros(8, np.float32)), ("mem", "mem", None)],
     [("n=-1", {"n": -1}), ("center_frequency=-1", {"center_frequency": -1.0}), ("bandwidth=0", {"bandwidth": 0.0}),
      ("bandwidth_reference_level=0", {"bandwidth_reference_level": 0.0})]),
    _wave("nxsig_chirp", [("f0", "v", 1.0), ("t1", "v", 1.0), ("f1", "v", 4.0), ("method", "v", _lib.CHIRP_LINEAR), ("vertex_zero", "v", 1), ("phi", "v", 0.0)],
          [("method=9", {"method": 9})]),
    _wave("nxsig_polynomial_sweep", [("coefs", "host", np.array([1.0, 2.0, 3.0])), ("ncoefs", "v", 3), ("phi", "v", 0.0), ("phi_degrees", "v", 0)],
          [("ncoefs=0", {"ncoefs": 0}), ("ncoefs=33", {"ncoefs": 33})]),
    ("nxsig_unit_impulse",
     [("dtype", "v", _lib.DT_F32), ("shape", "host?", _i64(8)), ("rank", "v", 1), ("index", "host?", _i64(3)), ("out", "out?", np.zeros(8, np.float32)),
      ("mem", "mem", None)],
     [("dtype=9", {"dtype": 9}), ("rank=-1", {"rank": -1}), ("rank=9", {"rank": 9}), ("null shape", {"shape": None}), ("null index", {"index": None}),
      ("negative dimension", {"shape": _i64(-8)}), ("shape too large", {"shape": _i64(1 << 40, 1 << 40), "rank": 2, "index": _i64(0, 0)}),
      ("null out", {"out": None}), ("index=8", {"index": _i64(8)})]),
    # f64 / c128 tier
    _stft("nxsig_stft_f64", _f32(B, L).astype(np.float64), np.zeros((B, M, K), np.complex128), True, 1, window=WIN.astype(np.float64),
          wflag=[("window_is_f64", "v", 1)]),
    _stft("nxsig_stft_c128", _c64(B, L).astype(np.complex128), np.zeros((B, M, K), np.complex128), True, 1, window=WIN.astype(np.float64),
          wflag=[("window_is_f64", "v", 1)]),
    _istft("nxsig_istft_c128", _c64(B, M, K).astype(np.complex128), np.zeros((B, M * HOP + N - HOP), np.complex128), True, window=WIN.astype(np.float64),
           wflag=[("window_is_f64", "v", 1)]),
    _fft("nxsig_fft_c128", np.float64, np.complex128),
    _framing("nxsig_as_windowed_f64", np.float64),
    _ola("nxsig_overlap_and_add_f64", np.float64),
    _fir("nxsig_fir_f64", np.float64, True, False),
    _fir("nxsig_fir_slice_f64", np.float64, True, True),
]


# entry points younger than the recorded table (their context is the typed pointer _lib._ctx)
OWN_TABLE_ENTRIES = [
    ("nxsig_resample_poly",
     [("x", "in", _f32(B, FL)), ("is_complex", "v", 0), ("length", "v", FL), ("batch", "v", B), ("batch_stride", "v", FL), ("h", "host", _f32(5)),
      ("num_taps", "v", 5), ("up", "v", 2), ("down", "v", 3), ("y", "out", np.zeros((B, 11), np.float32)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": FL - 1}), ("up=0", {"up": 0}),
      ("down=0", {"down": 0}), ("num_taps=0", {"num_taps": 0}),
      ("result past 64 bits", {"length": 1 << 62, "batch_stride": 1 << 62, "up": 1 << 20, "down": 1}),
      ("result too large", {"length": 1 << 58, "batch_stride": 1 << 58, "batch": 16, "up": 3, "down": 2})]),
]

# Spectral.welch / csd: 2 rows of 40 samples, 16-sample frames, hop 8, fft_length 32 (17 bins)
WL, WN, WK, WB = 40, 16, 32, 17
_WELCH_WIN = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(WN) / WN)).astype(np.float32)
_WELCH_CASES = [("batch=0", {"batch": 0}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": WL - 1}),
                ("frame_length=0", {"frame_length": 0}), ("hop=0", {"hop": 0}), ("hop>frame_length", {"hop": WN + 1}),
                ("fft_length<frame_length", {"fft_length": WN - 1}), ("fft_length past 2^24", {"fft_length": (1 << 24) + 1}),
                ("frame_length>length", {"frame_length": WL + 1, "fft_length": 64}), ("scaling=2", {"scaling": 2}),
                ("sampling_rate=0", {"sampling_rate": 0.0}), ("sampling_rate=nan", {"sampling_rate": float("nan")})]
_WELCH_COMMON = [("length", "v", WL), ("batch", "v", B), ("batch_stride", "v", WL), ("window", "host", _WELCH_WIN), ("frame_length", "v", WN),
                 ("hop", "v", 8), ("fft_length", "v", WK), ("detrend", "v", 1), ("scaling", "v", 0), ("sampling_rate", "v", 8000.0)]
WELCH_TABLE_ENTRIES = [
    ("nxsig_welch_f32", [("x", "in", _f32(B, WL)), *_WELCH_COMMON, ("pxx_out", "out", np.zeros((B, WB), np.float32)), ("mem", "mem", None)],
     _WELCH_CASES),
    ("nxsig_csd_f32",
     [("x", "in", _f32(B, WL)), ("y", "in", _f32(B, WL)), *_WELCH_COMMON, ("pxx_out", "out?", np.zeros((B, WB), np.float32)),
      ("pyy_out", "out?", np.zeros((B, WB), np.float32)), ("pxy_out", "out", np.zeros((B, WB), np.complex64)), ("mem", "mem", None)],
     _WELCH_CASES),
]

# Filters.sosfilt / sosfiltfilt: 2 rows of 40 samples through a two-section low-pass (sos, zi and zf are host arrays whatever `mem` says)
IL = 40
_IIR_SOS = np.array([[0.02, 0.04, 0.02, 1.0, -1.2, 0.4], [1.0, -0.5, 0.25, 1.0, -0.9, 0.5]], np.float64)
_IIR_BAD_A0 = _IIR_SOS.copy()
_IIR_BAD_A0[1, 3] = 2.0
_IIR_NAN = _IIR_SOS.copy()
_IIR_NAN[0, 1] = np.nan
_IIR_POLE1 = np.array([[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]] * 2, np.float64)
_IIR_CASES = [("batch=0", {"batch": 0}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": IL - 1}),
              ("n_sections=0", {"n_sections": 0}), ("n_sections=17", {"n_sections": 17}), ("a0=2", {"sos": _IIR_BAD_A0}),
              ("sos not finite", {"sos": _IIR_NAN}), ("rows too large", {"length": 1 << 59, "batch_stride": 1 << 59, "batch": 16})]
IIR_TABLE_ENTRIES = [
    ("nxsig_sosfilt_f32",
     [("x", "in", _f32(B, IL)), ("length", "v", IL), ("batch", "v", B), ("batch_stride", "v", IL), ("sos", "host", _IIR_SOS), ("n_sections", "v", 2),
      ("zi", "host?", 0.1 * _f32(B, 2, 2).astype(np.float64)), ("zi_rows", "v", B), ("zf_out", "hout?", np.zeros((B, 2, 2), np.float64)),
      ("direction", "v", 0), ("y", "out", np.zeros((B, IL), np.float32)), ("mem", "mem", None)],
     _IIR_CASES + [("zi_rows=3", {"zi_rows": 3}), ("direction=2", {"direction": 2})]),
    ("nxsig_sosfiltfilt_f32",
     [("x", "in", _f32(B, IL)), ("length", "v", IL), ("batch", "v", B), ("batch_stride", "v", IL), ("sos", "host", _IIR_SOS), ("n_sections", "v", 2),
      ("padtype", "v", 1), ("padlen", "v", -1), ("y", "out", np.zeros((B, IL), np.float32)), ("mem", "mem", None)],
     _IIR_CASES + [("padtype=4", {"padtype": 4}), ("padlen=length", {"padlen": IL}), ("default padlen >= length", {"length": 15, "batch_stride": 15}),
                   ("pole at z=1", {"sos": _IIR_POLE1})]),
]

# PeakFinding.find_peaks: the 8 samples of the argrelextrema row under height >= 1, distance 2, prominence >= 0.5 and width >= 0 (bounds is
# a host array whatever `mem` says); wanted are peak_heights, prominences, the four width arrays and the two bases: 6 f64 and 2 s32 rows
_FP_BOUNDS = np.array([[-np.inf, np.inf], [1.0, np.inf], [-np.inf, np.inf], [0.5, np.inf], [0.0, np.inf]], np.float64)
_FP_NAN_BOUNDS = _FP_BOUNDS.copy()
_FP_NAN_BOUNDS[3, 1] = np.nan
_FP_WANT = 0b1111111001
PEAKS_TABLE_ENTRIES = [
    ("nxsig_find_peaks",
     [("x", "in", _X8), ("dtype", "v", _lib.DT_F32), ("shape", "host", _i64(8)), ("rank", "v", 1), ("axis", "v", 0), ("bounds", "host", _FP_BOUNDS),
      ("conditions", "v", 2 | 8 | 16 | 32), ("distance", "v", 2.0), ("wlen", "v", -1), ("rel_height", "v", 0.5), ("capacity", "v", 3),
      ("want", "v", _FP_WANT), ("indices", "out", np.zeros((3, 1), np.int32)), ("valid", "out", np.zeros(1, np.uint32)),
      ("fprops", "out", np.zeros((6, 3), np.float64)), ("iprops", "out", np.zeros((2, 3), np.int32)), ("mem", "mem", None)],
     _PEAK_SHAPE_CASES + [("axis=1", {"axis": 1}), ("axis=-1", {"axis": -1}), ("dtype=2", {"dtype": _lib.DT_S32}), ("dtype=9", {"dtype": 9}),
                          ("distance=0.5", {"distance": 0.5}), ("distance=nan", {"distance": float("nan")}), ("wlen=1", {"wlen": 1}),
                          ("wlen=0", {"wlen": 0}), ("rel_height=-1", {"rel_height": -1.0}), ("rel_height=nan", {"rel_height": float("nan")}),
                          ("conditions=64", {"conditions": 64}), ("want=8192", {"want": 8192}), ("capacity=4", {"capacity": 4}),
                          ("capacity=-1", {"capacity": -1}), ("a border is nan", {"bounds": _FP_NAN_BOUNDS})]),
]

# Filters.savgol_filter: 2 rows of 24 samples, a window of 7 and a cubic, first derivative, mode interp (4)
SL = 24
SAVGOL_TABLE_ENTRIES = [
    ("nxsig_savgol_filter",
     [("x", "in", _f32(B, SL)), ("is_f64", "v", 0), ("length", "v", SL), ("batch", "v", B), ("batch_stride", "v", SL), ("window_length", "v", 7),
      ("polyorder", "v", 3), ("deriv", "v", 1), ("delta", "v", 0.5), ("mode", "v", 4), ("cval", "v", 0.0), ("y", "out", np.zeros((B, SL), np.float32)),
      ("mem", "mem", None)],
     [("batch=0", {"batch": 0}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": SL - 1}), ("is_f64=2", {"is_f64": 2}),
      ("window_length=0", {"window_length": 0}), ("window_length=1027", {"window_length": 1027, "polyorder": 3}),
      ("polyorder=window_length", {"polyorder": 7}), ("polyorder=-1", {"polyorder": -1}), ("polyorder=16", {"polyorder": 16, "window_length": 23}),
      ("deriv=-1", {"deriv": -1}), ("delta=0", {"delta": 0.0}), ("delta=nan", {"delta": float("nan")}), ("delta=inf", {"delta": float("inf")}),
      ("mode=5", {"mode": 5}), ("mode=-1", {"mode": -1}), ("cval=nan", {"cval": float("nan"), "mode": 1}), ("cval=inf", {"cval": float("inf")}),
      ("interp window > length", {"window_length": 25}), ("rows too large", {"length": 1 << 59, "batch_stride": 1 << 59, "batch": 16})]),
]

# Filters.hilbert: 2 rows of 24 samples, zero-padded to 32 points, the envelope (kind 1).  batch = 0 is valid and launches nothing, so it
# runs with ctx = NULL alone, where it shows that the argument checks let it through to the context
HL = 24
HILBERT_TABLE_ENTRIES = [
    ("nxsig_hilbert_f32",
     [("x", "in", _f32(B, HL)), ("length", "v", HL), ("batch", "v", B), ("batch_stride", "v", HL), ("n_fft", "v", 32), ("kind", "v", 1),
      ("out", "out", np.zeros((B, 32), np.float32)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}, NULL_ONLY), ("batch=-1", {"batch": -1}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": HL - 1}),
      ("n_fft=0", {"n_fft": 0}), ("n_fft=-1", {"n_fft": -1}), ("n_fft=2^31", {"n_fft": 1 << 31}), ("kind=3", {"kind": 3}), ("kind=-1", {"kind": -1}),
      ("rows too large", {"length": 1 << 59, "batch_stride": 1 << 59, "batch": 16}), ("result too large", {"n_fft": (1 << 31) - 1, "batch": 1 << 30})]),
]

# Transforms.dct: 2 rows of 24 samples, zero-padded to 32 points, type 2, norm "ortho" (1), the leading 13 coefficients.  batch = 0 is
# valid and launches nothing, so it runs with ctx = NULL alone, where it shows that the argument checks let it through to the context
DCT_TABLE_ENTRIES = [
    ("nxsig_dct_f32",
     [("x", "in", _f32(B, HL)), ("length", "v", HL), ("batch", "v", B), ("batch_stride", "v", HL), ("n", "v", 32), ("type", "v", 2), ("norm", "v", 1),
      ("keep", "v", 13), ("out", "out", np.zeros((B, 13), np.float32)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}, NULL_ONLY), ("batch=-1", {"batch": -1}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": HL - 1}),
      ("n=0", {"n": 0}), ("n=-1", {"n": -1}), ("n=2^31", {"n": 1 << 31}), ("type=1", {"type": 1}), ("type=4", {"type": 4}), ("type=5", {"type": 5}),
      ("type=0", {"type": 0}), ("norm=3", {"norm": 3}), ("norm=-1", {"norm": -1}), ("keep=0", {"keep": 0}), ("keep=n+1", {"keep": 33}),
      ("rows too large", {"length": 1 << 59, "batch_stride": 1 << 59, "batch": 16}), ("result too large", {"n": (1 << 31) - 1, "batch": 1 << 30})]),
]

# Filters.lfilter / filtfilt: 2 rows of 40 samples through a third-order filter with a[0] = 2 (b, a, zi and zf are host arrays whatever
# `mem` says)
_LF_B = np.array([0.2, 0.3, -0.1], np.float64)
_LF_A = np.array([2.0, -1.0, 0.5, -0.1], np.float64)
_LF_A0 = _LF_A.copy()
_LF_A0[0] = 0.0
_LF_NAN = _LF_B.copy()
_LF_NAN[1] = np.nan
_LF_LONG = np.r_[1.0, np.full(17, 0.01)]
_LF_CASES = [("batch=0", {"batch": 0}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": IL - 1}),
             ("nb=0", {"nb": 0}), ("na=0", {"na": 0}), ("a[0]=0", {"a": _LF_A0}), ("b not finite", {"b": _LF_NAN}),
             ("order 17, recursive", {"a": _LF_LONG, "na": 18}), ("order 17, fir", {"b": _LF_LONG, "nb": 18, "a": np.ones(1), "na": 1}),
             ("rows too large", {"length": 1 << 59, "batch_stride": 1 << 59, "batch": 16})]
LFILTER_TABLE_ENTRIES = [
    ("nxsig_lfilter_f32",
     [("x", "in", _f32(B, IL)), ("length", "v", IL), ("batch", "v", B), ("batch_stride", "v", IL), ("b", "host", _LF_B), ("nb", "v", 3),
      ("a", "host", _LF_A), ("na", "v", 4), ("zi", "host?", 0.1 * _f32(B, 3).astype(np.float64)), ("zi_rows", "v", B),
      ("zf_out", "hout?", np.zeros((B, 3), np.float64)), ("direction", "v", 0), ("y", "out", np.zeros((B, IL), np.float32)), ("mem", "mem", None)],
     _LF_CASES + [("zi_rows=3", {"zi_rows": 3}), ("direction=2", {"direction": 2})]),
    ("nxsig_filtfilt_f32",
     [("x", "in", _f32(B, IL)), ("length", "v", IL), ("batch", "v", B), ("batch_stride", "v", IL), ("b", "host", _LF_B), ("nb", "v", 3),
      ("a", "host", _LF_A), ("na", "v", 4), ("padtype", "v", 1), ("padlen", "v", -1), ("y", "out", np.zeros((B, IL), np.float32)), ("mem", "mem", None)],
     _LF_CASES + [("padtype=4", {"padtype": 4}), ("padlen=length", {"padlen": IL}), ("default padlen >= length", {"length": 12, "batch_stride": 12}),
                  ("pole at z=1", {"b": np.ones(1), "nb": 1, "a": np.array([1.0, -1.0]), "na": 2})]),
]

# Spectral.lombscargle: 2 rows of 40 samples at 5 angular frequencies, weighted, precentred (x, freqs and weights are host arrays whatever
# `mem` says; weights may be NULL)
_LS_X = np.sort(_rng.uniform(0.0, 10.0, IL))
_LS_F = np.array([0.0, 0.5, 1.0, 2.5, 7.0], np.float64)
_LS_W = _rng.uniform(0.5, 2.0, IL)


def _ls_broken(arr, at, value):
    out = arr.copy()
    out[at] = value
    return out


LOMBSCARGLE_TABLE_ENTRIES = [
    ("nxsig_lombscargle",
     [("y", "in", _f32(B, IL)), ("dtype", "v", 0), ("n", "v", IL), ("batch", "v", B), ("batch_stride", "v", IL), ("x", "host", _LS_X),
      ("freqs", "host", _LS_F), ("num_freqs", "v", 5), ("weights", "host?", _LS_W), ("precenter", "v", 1), ("normalize", "v", 0),
      ("floating_mean", "v", 0), ("out", "out", np.zeros((B, 5), np.float32)), ("mem", "mem", None)],
     [("dtype=2", {"dtype": 2}), ("n=0", {"n": 0}), ("num_freqs=0", {"num_freqs": 0}), ("batch=0", {"batch": 0}),
      ("batch_stride=n-1", {"batch_stride": IL - 1}), ("precenter=2", {"precenter": 2}), ("normalize=3", {"normalize": 3}),
      ("floating_mean=-1", {"floating_mean": -1}), ("rows too large", {"n": 1 << 59, "batch_stride": 1 << 59, "batch": 16}),
      ("x not finite", {"x": _ls_broken(_LS_X, 3, np.inf)}), ("freqs not finite", {"freqs": _ls_broken(_LS_F, 1, np.nan)}),
      ("weights not finite", {"weights": _ls_broken(_LS_W, 0, np.nan)}), ("negative weight", {"weights": _ls_broken(_LS_W, 2, -1.0)}),
      ("zero weights", {"weights": np.zeros(IL)})]),
]

# Transforms.czt: 2 rows of 24 real samples, 13 points of a zoom (w = exp(-2 pi i 0.4 / 13), a = exp(2 pi i 0.05)).  batch = 0 is valid
# and launches nothing, so it runs with ctx = NULL alone, where it shows that the argument checks let it through to the context
CZT_TABLE_ENTRIES = [
    ("nxsig_czt",
     [("x", "in", _f32(B, HL)), ("is_complex", "v", 0), ("length", "v", HL), ("batch", "v", B), ("batch_stride", "v", HL), ("m", "v", 13),
      ("w_abs", "v", 1.0), ("w_step", "v", 0.4), ("w_den", "v", 13), ("a_abs", "v", 1.0), ("a_turns", "v", 0.05),
      ("out", "out", np.zeros((B, 13), np.complex64)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}, NULL_ONLY), ("batch=-1", {"batch": -1}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": HL - 1}),
      ("m=0", {"m": 0}), ("m=-1", {"m": -1}), ("is_complex=2", {"is_complex": 2}), ("w_den=0", {"w_den": 0}), ("w_den=2^62", {"w_den": 1 << 62}),
      ("w_abs=0", {"w_abs": 0.0}), ("w_abs=-1", {"w_abs": -1.0}), ("w_abs=inf", {"w_abs": float("inf")}), ("w_abs=nan", {"w_abs": float("nan")}),
      ("a_abs=0", {"a_abs": 0.0}), ("a_abs=inf", {"a_abs": float("inf")}), ("w_step=nan", {"w_step": float("nan")}),
      ("a_turns=inf", {"a_turns": float("inf")}), ("n+m-1=2^30+1", {"m": (1 << 30) - HL + 2}), ("m=2^31", {"m": 1 << 31}),
      ("spiral beyond the gate", {"w_abs": 1.02}), ("start beyond the gate", {"a_abs": 1.2}),
      ("rows too large", {"length": 1 << 29, "batch_stride": 1 << 59, "batch": 16}), ("result too large", {"batch": 1 << 40})]),
]

# Filters.fir_bank / Transforms.cwt: 2 rows of 24 real samples; a bank of three real filters of 3, 4 and 1 taps, and three morlet2 widths
# (N = 5, 12 and 24, the last capped by the row).  Both refuse batch = 0
_CW_TAPS = np.array([0.25, 0.5, 0.25, 1.0, -1.0, 0.5, -0.5, 2.0], np.float32)
_CW_COUNTS = np.array([3, 4, 1], np.int64)
_CW_WIDTHS = np.array([0.5, 1.2, 4.0], np.float64)


def _cw_broken(arr, at, value):
    out = arr.copy()
    out[at] = value
    return out


CWT_TABLE_ENTRIES = [
    ("nxsig_fir_bank",
     [("x", "in", _f32(B, HL)), ("length", "v", HL), ("batch", "v", B), ("batch_stride", "v", HL), ("taps", "host", _CW_TAPS),
      ("taps_complex", "v", 0), ("tap_counts", "host", _CW_COUNTS), ("num_filters", "v", 3), ("kind", "v", 0),
      ("out", "out", np.zeros((B, 3, HL), np.complex64)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}), ("batch=-1", {"batch": -1}), ("batch=65536", {"batch": 65536}), ("length=0", {"length": 0}),
      ("batch_stride=length-1", {"batch_stride": HL - 1}), ("kind=4", {"kind": 4}), ("kind=-1", {"kind": -1}), ("taps_complex=2", {"taps_complex": 2}),
      ("num_filters=0", {"num_filters": 0}), ("num_filters=4097", {"num_filters": 4097}), ("tap count 0", {"tap_counts": _cw_broken(_CW_COUNTS, 1, 0)}),
      ("tap count -1", {"tap_counts": _cw_broken(_CW_COUNTS, 2, -1)}), ("length+taps-1=2^24+1", {"tap_counts": _cw_broken(_CW_COUNTS, 0, (1 << 24) - HL + 2)}),
      ("tap count 2^40", {"tap_counts": _cw_broken(_CW_COUNTS, 0, 1 << 40)}), ("length=2^24+1", {"length": (1 << 24) + 1, "batch_stride": (1 << 24) + 1}),
      ("taps nan", {"taps": _cw_broken(_CW_TAPS, 4, np.nan)}), ("taps inf", {"taps": _cw_broken(_CW_TAPS, 7, np.inf)})]),
    ("nxsig_cwt",
     [("x", "in", _f32(B, HL)), ("length", "v", HL), ("batch", "v", B), ("batch_stride", "v", HL), ("wavelet", "v", 0),
      ("widths", "host", _CW_WIDTHS), ("num_widths", "v", 3), ("w", "v", 5.0), ("kind", "v", 0),
      ("out", "out", np.zeros((B, 3, HL), np.complex64)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536}), ("length=0", {"length": 0}), ("batch_stride=length-1", {"batch_stride": HL - 1}),
      ("kind=4", {"kind": 4}), ("wavelet=2", {"wavelet": 2}), ("wavelet=-1", {"wavelet": -1}), ("num_widths=0", {"num_widths": 0}),
      ("num_widths=4097", {"num_widths": 4097}), ("width 0", {"widths": _cw_broken(_CW_WIDTHS, 0, 0.0)}), ("width -1", {"widths": _cw_broken(_CW_WIDTHS, 1, -1.0)}),
      ("width nan", {"widths": _cw_broken(_CW_WIDTHS, 2, np.nan)}), ("width inf", {"widths": _cw_broken(_CW_WIDTHS, 2, np.inf)}), ("w=nan", {"w": float("nan")}),
      ("length=2^24", {"length": 1 << 24, "batch_stride": 1 << 24})]),
]

# Convolution.correlate_rows: 2 pairs of 24 against 9 real samples, PHAT-weighted, under the peak sink (so that out_lags is a required
# pointer).  batch = 0 is valid and launches nothing, so it runs with ctx = NULL alone, where it shows that the argument checks let it
# through to the context
XL = 9
XCORR_TABLE_ENTRIES = [
    ("nxsig_xcorr",
     [("a", "in", _f32(B, HL)), ("n1", "v", HL), ("a_stride", "v", HL), ("b", "in", _f32(B, XL)), ("n2", "v", XL), ("b_stride", "v", XL), ("batch", "v", B),
      ("is_complex", "v", 0), ("op", "v", 1), ("mode", "v", 0), ("weighting", "v", 1), ("phat_floor", "v", 0.001), ("sink", "v", 1),
      ("out", "out", np.zeros(B, np.float32)), ("out_lags", "out", np.zeros(B, np.int32)), ("mem", "mem", None)],
     [("batch=0", {"batch": 0}, NULL_ONLY), ("batch=-1", {"batch": -1}), ("n1=0", {"n1": 0}), ("n2=0", {"n2": 0}), ("n2=-1", {"n2": -1}),
      ("a_stride=n1-1", {"a_stride": HL - 1}), ("b_stride=n2-1", {"b_stride": XL - 1}), ("b_stride=-1", {"b_stride": -1}),
      ("is_complex=2", {"is_complex": 2}), ("op=2", {"op": 2}), ("op=-1", {"op": -1}), ("mode=3", {"mode": 3}), ("weighting=2", {"weighting": 2}),
      ("sink=2", {"sink": 2}), ("phat with convolve", {"op": 0, "sink": 0}), ("peak with convolve", {"op": 0, "weighting": 0}),
      ("phat_floor=1", {"phat_floor": 1.0}), ("phat_floor=-0.1", {"phat_floor": -0.1}), ("phat_floor=nan", {"phat_floor": float("nan")}),
      ("n1+n2-1=2^30+1", {"n2": (1 << 30) - HL + 2, "b_stride": 0}), ("n1=2^31", {"n1": 1 << 31, "a_stride": 1 << 31}),
      ("rows too large", {"a_stride": 1 << 59, "batch": 16}), ("result too large", {"batch": 1 << 40})]),
]


def _cases(args, listed):
    out = [("valid", {})]
    out += [("null " + a, {a: None}) for a, kind, _ in args if kind in ("in", "out", "host", "hout", "p")]
    out.append(("mem=7", {"mem": 7}))
    return [c if len(c) == 3 else (*c, None) for c in out + list(listed)]


class Probe:
    def __init__(self, lib, ctx):
        self.lib, self.ctx = lib, ctx

    def _dev(self, arr):
        p = C.c_void_p()
        assert self.lib.nxsig_alloc(self.ctx, max(arr.nbytes, 4), C.byref(p)) == 0, self.lib.nxsig_last_error()
        assert self.lib.nxsig_upload(self.ctx, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0, self.lib.nxsig_last_error()
        return p

    def call(self, name, args, broken, mem):
        """one call; returns (record, {out arg: bytes})"""
        fn = getattr(self.lib, name)
        argtypes = _lib.SIGNATURES[name][1][1:]
        params = dict(PARAMS)
        for k, v in broken.items():
            if k.startswith("p."):
                params[k[2:]] = v
        nf = C.c_int64(NF_SENTINEL)
        keep, call, outs, devs = [], [], [], []
        for (a, kind, val), at in zip(args, argtypes):
            if a in broken:
                val = broken[a]
            if kind == "mem":
                call.append(val if val is not None else mem)
            elif kind == "v":
                call.append(val)
            elif kind == "nf":
                call.append(C.byref(nf))
            elif val is None:
                call.append(None)
            elif kind == "p":
                st = _lib.StftParams(*[params[f] for f, _ in _lib.StftParams._fields_])
                keep.append(st)
                call.append(C.byref(st))
            else:
                arr = np.array(val, copy=True)
                keep.append(arr)
                tensor = kind.rstrip("?") in ("in", "out")
                if tensor and mem == _lib.DEVICE:
                    d = self._dev(arr)
                    devs.append((d, arr, kind.startswith("out")))
                    call.append(d if at is C.c_void_p else C.cast(d, at))
                else:
                    call.append(arr.ctypes.data_as(at))
                if kind.rstrip("?") in ("out", "hout"):
                    outs.append((a, arr))
        ctx_type = _lib.SIGNATURES[name][1][0]
        rc = fn(_lib.ctx_ptr(self.ctx, ctx_type) if ctx_type in _lib.TYPED_CTX else self.ctx, *call)
        err = self.lib.nxsig_last_error().decode("utf-8", "replace") if rc != 0 else ""
        for d, arr, is_out in devs:
            if is_out and rc == 0:
                assert self.lib.nxsig_download(self.ctx, arr.ctypes.data_as(C.c_void_p), d, arr.nbytes) == 0, self.lib.nxsig_last_error()
            assert self.lib.nxsig_free(self.ctx, d) == 0
        if devs:
            assert self.lib.nxsig_sync(self.ctx) == 0
        rec = {"rc": rc, "err": err}
        if any(kind == "nf" for _, kind, _ in args):
            rec["num_frames_out"] = nf.value
        return rec, {a: arr.tobytes() for a, arr in outs}

    def run(self, entries=None):
        """{entry point: {case: record}}; with a context the valid row also carries "host_equals_device" """
        real = self.ctx is not None
        table = {}
        for name, args, listed in (ENTRIES if entries is None else entries):
            rows = {}
            for label, broken, only in _cases(args, listed):
                if real and only == NULL_ONLY:
                    continue
                rec, host_out = self.call(name, args, broken, _lib.HOST)
                if real and label == "valid":
                    assert rec["rc"] == 0, (name, rec)
                    rec_d, dev_out = self.call(name, args, broken, _lib.DEVICE)
                    assert rec_d == rec, (name, rec, rec_d)
                    rec["host_equals_device"] = host_out == dev_out
                elif real:
                    assert rec["rc"] != 0, f"{name} [{label}]: a broken argument was accepted (and something was launched)"
                rows[label] = rec
            table[name] = rows
        return table


def probe(lib_path, real, entries=None):
    lib = bind(lib_path)
    ctx = None
    if real:
        ctx = C.c_void_p()
        rc = lib.nxsig_ctx_create(0, C.byref(ctx))
        assert rc == 0, lib.nxsig_last_error()
    try:
        return Probe(lib, ctx).run(entries)
    finally:
        if real:
            lib.nxsig_ctx_destroy(ctx)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--real", action="store_true", help="use a context on device 0 (needs the GPU) instead of ctx = NULL")
    ap.add_argument("--write", metavar="JSON", default=None, help="merge the table into this golden file (default: print it)")
    ap.add_argument("--own", action="store_true", help="the entry points of OWN_TABLE_ENTRIES instead of the recorded table's")
    ap.add_argument("--welch", action="store_true", help="the entry points of WELCH_TABLE_ENTRIES (Spectral.welch / csd)")
    ap.add_argument("--iir", action="store_true", help="the entry points of IIR_TABLE_ENTRIES (Filters.sosfilt / sosfiltfilt)")
    ap.add_argument("--peaks", action="store_true", help="the entry point of PEAKS_TABLE_ENTRIES (PeakFinding.find_peaks)")
    ap.add_argument("--savgol", action="store_true", help="the entry point of SAVGOL_TABLE_ENTRIES (Filters.savgol_filter)")
    ap.add_argument("--hilbert", action="store_true", help="the entry point of HILBERT_TABLE_ENTRIES (Filters.hilbert)")
    ap.add_argument("--dct", action="store_true", help="the entry point of DCT_TABLE_ENTRIES (Transforms.dct / idct)")
    ap.add_argument("--lfilter", action="store_true", help="the entry points of LFILTER_TABLE_ENTRIES (Filters.lfilter / filtfilt)")
    ap.add_argument("--lombscargle", action="store_true", help="the entry point of LOMBSCARGLE_TABLE_ENTRIES (Spectral.lombscargle)")
    ap.add_argument("--czt", action="store_true", help="the entry point of CZT_TABLE_ENTRIES (Transforms.czt / zoom_fft)")
    ap.add_argument("--cwt", action="store_true", help="the entry points of CWT_TABLE_ENTRIES (Filters.fir_bank / Transforms.cwt)")
    ap.add_argument("--xcorr", action="store_true", help="the entry point of XCORR_TABLE_ENTRIES (Convolution.correlate_rows / convolve_rows)")
    a = ap.parse_args()
    key = "real_ctx" if a.real else "null_ctx"
    table = probe(a.lib, a.real, XCORR_TABLE_ENTRIES if a.xcorr else CWT_TABLE_ENTRIES if a.cwt else CZT_TABLE_ENTRIES if a.czt else LOMBSCARGLE_TABLE_ENTRIES if a.lombscargle else LFILTER_TABLE_ENTRIES if a.lfilter else DCT_TABLE_ENTRIES if a.dct else HILBERT_TABLE_ENTRIES if a.hilbert else SAVGOL_TABLE_ENTRIES if a.savgol else PEAKS_TABLE_ENTRIES if a.peaks else IIR_TABLE_ENTRIES if a.iir else WELCH_TABLE_ENTRIES if a.welch else OWN_TABLE_ENTRIES if a.own else None)
    if not a.write:
        print(json.dumps({key: table}, indent=1))
        return
    doc = {}
    if os.path.exists(a.write):
        with open(a.write) as f:
            doc = json.load(f)
    doc[key] = table
    with open(a.write, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.write}: {key}: {sum(len(v) for v in table.values())} cases of {len(table)} entry points")


if __name__ == "__main__":
    main()
