"""Where do the n-D, filter, peak and f64 entry points write, and what do they leave alone?

tests/test_gpu_output_extents.py puts the streaming families (stft, istft, fft rows, fir) into the arenas of tests/extents.py; this module
does the same for the entry points with the most index arithmetic per element, which had only ever run on exactly sized, freshly
allocated, 256-byte-aligned buffers: nxsig_argrelextrema / nxsig_nonzero (tile compaction, the -1 fill in 16-byte groups between a
scalar head and tail), nxsig_median_filter / nxsig_wiener (row, plane and generic tiles), nxsig_fft_nd / nxsig_fftconvolve_nd /
nxsig_fftconvolve_c64 / nxsig_convolve_direct (transposes, broadcast strides, centred slices), nxsig_overlap_and_add(_f64) /
nxsig_as_windowed_f32 / _f64 (16-byte paths chosen from pointer bits), nxsig_stft_to_mel (frame tiles), nxsig_spectrum_mul_c64 /
nxsig_spectrum_mask_c64 (in place, broadcast operands) and nxsig_istft_c128 / nxsig_fft_c128.

Every tensor of a call lies in an arena of its own — 4 KB of a NaN pattern on either side, a result pre-filled with it; the u8 mask of
nxsig_nonzero ends in a tail gap of pattern bytes, `valid` is a one-element u32 arena.  Host-side arguments (shapes, kernel shapes, the
filter of spectrum_mul, mel filters, windows, out_shape, noise_used) stay host arrays.  Every case asserts

* both guards of every result intact, no result element left unwritten,
* every input arena bit for bit as uploaded,
* the results bit-identical to the same call into plain nxsig_alloc buffers,
* the dispatch record pinned in RECORDS, led by the family the case is about,
* the result against the oracle at the bound the suite already holds that entry to (TOL_MAX, RTOL, exact bits, 1 ulp for the f32
  wiener estimate, the mel bound of tests/test_gpu_parity.py::test_stft_to_mel_is_bit_identical_to_the_oracle).

Shapes are the smallest that reach the mechanism: 4113 = kTile + 17 elements for the peak tiles (kernels_peaks.hip: kThreads x kItems =
4096), widths one past a multiple of the tile for the filters, 67 = 64 + 3 frames for the mel tile.  The argrelextrema inputs are seeded
on the CPU so that s0 = valid * rank, the first element of the -1 fill, takes every phase 0 .. 3 of a 16-byte group (PHASES, asserted
at import from tests/peaks_oracle.py alone).

NXSIG_DISPATCH_PROBE=1 prints the records instead of asserting them (how RECORDS and OFFSET_RECORDS were filled)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import extents as E
import filters_oracle as F
import peaks_oracle as P
import nx_signal_amd as S
import test_gpu_strided_rows as R
from nx_signal_amd import _lib
from oracle import nx_oracle as O

pytestmark = pytest.mark.gpu
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"
TOL_MAX = R.TOL_MAX      # 1e-5 normalised: tests/test_gpu_parity.py, tests/test_gpu_nd.py
RTOL = R.RTOL            # 1e-12: tests/test_gpu_f64.py, the f64 wiener estimate of tests/test_gpu_filters.py
FS = 16000.0
DEV = _lib.DEVICE
MODES = R.MODES
_vp = R._vp
KTILE = 256 * 16         # kernels_peaks.hip: kThreads * kItems flat elements per tile
HERE = os.path.dirname(os.path.abspath(__file__))


def _i64(v):
    return (C.c_int64 * len(v))(*[int(q) for q in v])


def _i32(v):
    return (C.c_int32 * len(v))(*[int(q) for q in v])


def _rows(shape):
    shape = tuple(int(s) for s in shape)
    return (int(np.prod(shape[:-1], dtype=np.int64)), shape[-1]) if len(shape) > 1 else (1, shape[0])


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _randn(rng, shape, dtype):
    dtype = np.dtype(dtype)
    x = rng.standard_normal(shape)
    if dtype.kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


class Case:
    """one call: `ins` [(name, array)] the device tensors, `outs` [(name, dtype, shape)] the results, `args(ins, outs, host)` the arguments
    behind the context (device pointers in; host-side outputs are left in the dict `host`), `judge(arenas, results, host)` the findings
    against the oracle"""

    def __init__(self, family, entry, ins, outs, args, judge, tuning=None, anywhere=False):
        self.family, self.entry, self.tuning, self.anywhere = family, entry, tuning or {}, anywhere
        self.ins = [(n, np.ascontiguousarray(a)) for n, a in ins]
        self.outs, self.args, self.judge = outs, args, judge

    def invoke(self, handle, ins, outs, host):
        return getattr(_lib.load(), self.entry)(handle, *self.args(ins, outs, host))


def _memo(fn):
    return functools.lru_cache(maxsize=1)(fn)


# ------------------------------------------------------------------------------- the bounds
def _exact(ref):
    return lambda outs, got, host: E.bit_findings(outs[0], got[0], np.asarray(ref()).astype(outs[0].dtype))


def _close(ref, tol):
    def judge(outs, got, host):
        r = np.asarray(ref())
        return E.finite_findings(outs[0], got[0], r) + E.value_findings(outs[0], got[0], r, tol)
    return judge


def _one_ulp(arena, got, ref):
    """tests/test_gpu_filters.py, _wiener_close: f32 results within one unit in the last place"""
    d = np.abs(got.view(np.int32).astype(np.int64) - np.asarray(ref, np.float32).reshape(got.shape).view(np.int32).astype(np.int64))
    return [f"{arena.name}: row {r}, index {i}: {int(d[r, i])} ulp from the oracle" for r, i in np.argwhere(d > 1)[:4].tolist()]


def _mel_bound(arena, got, ref):
    """tests/test_gpu_parity.py::test_stft_to_mel_is_bit_identical_to_the_oracle"""
    ref = np.asarray(ref, np.float32).reshape(got.shape)
    bad = np.argwhere(got != ref)
    out = []
    if len(bad) > max(1, got.size // 100_000):
        out.append(f"{arena.name}: {len(bad)} elements differ from the oracle, first at row {bad[0][0]}, index {bad[0][1]}")
    if not np.max(np.abs(got - ref)) < 2e-6:
        r, i = np.unravel_index(int(np.argmax(np.abs(got - ref))), got.shape)
        out.append(f"{arena.name}: row {r}, index {i}: error {float(np.abs(got - ref)[r, i]):.3e}, not below 2e-6")
    return out


# ------------------------------------------------------------------------------- argrelextrema, nonzero
DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64}
CMP = {"less": _lib.CMP_LESS, "greater_equal": _lib.CMP_GREATER_EQUAL}


def _peak_data(shape, dt, seed, const=False):
    """quarters: ties along every line, so greater_equal marks what greater does not"""
    if const:
        return np.full(shape, 1.5, dt)
    return (np.round(_rng(seed).standard_normal(shape) * 4) / 4).astype(dt)


def _table_judge(ref):
    return lambda outs, got, host: E.table_findings(outs[0], got[0], ref()[0]) + E.table_findings(outs[1], got[1], [int(ref()[1])])


def _table_outs(x):
    return [("indices", np.int32, (x.size, x.ndim)), ("valid", np.uint32, (1, 1))]


def peaks(family, shape, axis, shifts, cmp, dt, seed, tuning=None, const=False):
    x = _peak_data(shape, dt, seed, const)
    ref = _memo(lambda: P.argrelextrema(x, cmp, axis, shifts))
    args = lambda i, o, h: (i[0], DT[x.dtype], _i64(shape), x.ndim, axis, shifts, CMP[cmp], o[0], o[1], DEV)    # noqa: E731
    return Case(family, "nxsig_argrelextrema", [("x", x)], _table_outs(x), args, _table_judge(ref), tuning)


def _mask(shape, density):
    total = int(np.prod(shape))
    if density == "last-group":                     # every byte set but the last: valid = size - 1
        m = np.full(total, 255, np.uint8)
        m[-1] = 0
        return m.reshape(shape)
    rng = _rng(total, int(density * 8))
    return ((rng.random(total) < density) * rng.integers(1, 256, total)).astype(np.uint8).reshape(shape)


def nonzero(shape, density):
    m = _mask(shape, density)
    ref = _memo(lambda: P.nonzero(m))
    args = lambda i, o, h: (i[0], _i64(shape), m.ndim, o[0], o[1], DEV)    # noqa: E731
    return Case("nonzero", "nxsig_nonzero", [("mask", m)], _table_outs(m), args, _table_judge(ref))


# ------------------------------------------------------------------------------- median, wiener
def median(family, shape, ks, dt, tuning=None):
    x = _randn(_rng(sum(shape), sum(ks)), shape, dt)
    args = lambda i, o, h: (i[0], int(x.dtype == np.float64), _i64(shape), x.ndim, _i64(ks), o[0], DEV)    # noqa: E731
    return Case(family, "nxsig_median_filter", [("x", x)], [("out", np.float32, shape)], args, _exact(_memo(lambda: F.median(x, ks))), tuning)


def wiener(family, shape, ks, dt, noise):
    """noise None: the estimate (k_wiener_noise's partial sums), read back through noise_used"""
    x = _randn(_rng(sum(shape), 7), shape, dt) * 3 + np.linspace(0, 5, int(np.prod(shape))).reshape(shape).astype(dt)    # tests/test_gpu_filters.py
    ks = (ks,) * x.ndim if isinstance(ks, int) else ks
    ref = _memo(lambda: F.wiener(x, ks, noise, return_noise=True))

    def args(i, o, h):
        h["noise"] = C.c_double(float("nan"))
        return (i[0], int(x.dtype == np.float64), _i64(shape), x.ndim, _i64(ks), int(noise is not None), 0.0 if noise is None else noise, o[0],
                C.byref(h["noise"]), DEV)

    def judge(outs, got, host):
        exp, used = ref()
        if noise is not None:
            return E.bit_findings(outs[0], got[0], exp) + ([] if host["noise"].value == noise else [f"noise_used {host['noise'].value} is not the given {noise}"])
        found = [] if abs(host["noise"].value - used) <= 1e-12 * abs(used) else [f"noise_used {host['noise'].value!r}, the oracle's estimate {used!r}"]
        if x.dtype == np.float64:
            return found + E.finite_findings(outs[0], got[0], exp) + E.value_findings(outs[0], got[0], exp, RTOL)
        return found + _one_ulp(outs[0], got[0], exp)

    return Case(family, "nxsig_wiener", [("x", x)], [("out", x.dtype, shape)], args, judge)


# ------------------------------------------------------------------------------- fft_nd, the convolutions
def fft_nd(family, shape, axes, lengths, inverse, real=False):
    x = _randn(_rng(sum(shape), len(axes)), shape, np.float32 if real else np.complex64)
    oshape = list(shape)
    for ax, n in zip(axes, lengths):
        oshape[ax] = n
    ref = _memo(lambda: O.fft_nd(x, axes=axes, lengths=lengths, inverse=inverse) if axes else x.astype(np.complex64))
    args = lambda i, o, h: (i[0], int(real), _i64(shape), x.ndim, _i32(axes) if axes else None, _i64(lengths) if axes else None, len(axes),    # noqa: E731
                            int(inverse), o[0], DEV)
    return Case(family, "nxsig_fft_nd", [("in", x)], [("out", np.complex64, oshape)], args, _close(ref, TOL_MAX))


def conv_nd(family, entry, sa, sb, mode, a_dt=np.float32, b_dt=np.float32, tuning=None, anywhere=False):
    rng = _rng(sum(sa), sum(sb))
    a, b = _randn(rng, sa, a_dt), _randn(rng, sb, b_dt)
    direct = entry == "nxsig_convolve_direct"
    ref = _memo(lambda: (O.convolve_direct if direct else O.fftconvolve)(a, b, mode=mode))
    oshape = {"full": [x + y - 1 for x, y in zip(sa, sb)], "same": list(sa), "valid": [abs(x - y) + 1 for x, y in zip(sa, sb)]}[mode]    # nxsig.h
    odt = np.float32 if a.dtype == b.dtype == np.float32 else np.complex64

    def args(i, o, h):
        h["out_shape"] = _i64([-1] * a.ndim)
        return (i[0], int(a.dtype == np.float32), _i64(sa), i[1], int(b.dtype == np.float32), _i64(sb), a.ndim, MODES[mode], o[0], h["out_shape"], DEV)

    def judge(outs, got, host):
        r = ref()
        assert list(r.shape) == oshape and r.dtype == odt, (r.shape, oshape, r.dtype)
        found = [] if list(host["out_shape"]) == oshape else [f"out_shape {list(host['out_shape'])}, expected {oshape}"]
        return found + (E.bit_findings(outs[0], got[0], r) if direct else E.finite_findings(outs[0], got[0], r) + E.value_findings(outs[0], got[0], r, TOL_MAX))

    return Case(family, entry, [("a", a), ("b", b)], [("out", odt, oshape)], args, judge, tuning, anywhere)


def fftconvolve_c64(n1, n2, mode):
    rng = _rng(n1, n2)
    a, b = _randn(rng, (n1,), np.complex64), _randn(rng, (n2,), np.complex64)
    n_out = {"full": n1 + n2 - 1, "same": n1, "valid": abs(n1 - n2) + 1}[mode]
    ref = _memo(lambda: np.convolve(a.astype(np.complex128), b.astype(np.complex128), mode=mode))       # tests/test_gpu_nd.py
    args = lambda i, o, h: (i[0], n1, i[1], n2, MODES[mode], o[0], DEV)    # noqa: E731
    return Case("fft.rows_generic.pow2", "nxsig_fftconvolve_c64", [("a", a), ("b", b)], [("out", np.complex64, (n_out,))], args, _close(ref, TOL_MAX))


# ------------------------------------------------------------------------------- overlap_and_add, as_windowed
def ola(family, M, N, hop, comps, wide, rows=3):
    dt = np.dtype(np.float64 if wide else np.float32)
    fr = _randn(_rng(M, N, hop, comps), (rows, M, N * comps), dt)
    out_len = M * hop + N - hop

    def ref():
        t = fr.view(np.complex128 if wide else np.complex64) if comps == 2 else fr
        y = O.overlap_and_add_f64(t, N - hop) if wide else O.overlap_and_add(t, N - hop)
        return np.ascontiguousarray(y).view(dt)

    args = lambda i, o, h: (i[0], M, rows, N, N - hop, comps, o[0], DEV)    # noqa: E731
    return Case(family, "nxsig_overlap_and_add_f64" if wide else "nxsig_overlap_and_add", [("frames", fr.reshape(rows * M, N * comps))],
                [("out", dt, (rows, out_len * comps))], args, _close(_memo(ref), RTOL if wide else TOL_MAX))


PADS = {"valid": (_lib.PAD_VALID, 0, 0), "reflect": (_lib.PAD_REFLECT, 0, 0), "same": (_lib.PAD_SAME, 0, 0)}


def as_windowed(family, N, hop, L, pad, wide, rows=3):
    dt = np.dtype(np.float64 if wide else np.float32)
    x = _randn(_rng(N, hop, L), (rows, L), dt)
    mode, lo, hi = PADS[pad] if isinstance(pad, str) else (_lib.PAD_EXPLICIT, pad[0], pad[1])
    ref = _memo(lambda: O.as_windowed(x, N, hop, pad if isinstance(pad, str) else [pad]))
    M = O.num_frames(L, N, hop, pad if isinstance(pad, str) else [pad])

    def args(i, o, h):
        h["frames"] = C.c_int64(-1)
        return (i[0], L, rows, L, N, hop, mode, lo, hi, o[0], C.byref(h["frames"]), DEV)

    def judge(outs, got, host):
        return ([] if host["frames"].value == M else [f"num_frames_out {host['frames'].value}, expected {M}"]) + E.bit_findings(outs[0], got[0], ref().astype(dt))

    return Case(family, "nxsig_as_windowed_f64" if wide else "nxsig_as_windowed_f32", [("x", x)], [("out", dt, (rows, M * N))], args, judge)


# ------------------------------------------------------------------------------- stft_to_mel, spectrum_mul, spectrum_mask
def mel(family, rows, K, bands, tuning=None):
    rng = _rng(rows, K, bands)
    z = (_randn(rng, (rows, K), np.complex128) * 10.0 ** rng.uniform(-3, 3, (rows, 1))).astype(np.complex64)    # tests/test_gpu_parity.py
    filt = S.mel_filters(K, bands, FS)
    ref = _memo(lambda: O.stft_to_mel(z, FS, K, mel_bins=bands))
    args = lambda i, o, h: (i[0], rows, K, bands, _vp(filt), o[0], DEV)    # noqa: E731
    return Case(family, "nxsig_stft_to_mel", [("z", z)], [("out", np.float32, (rows, bands))], args,
                lambda outs, got, host: _mel_bound(outs[0], got[0], ref()), tuning)


def spectrum_mul(rows=5, K=30):
    rng = _rng(rows, K)
    z, hh = _randn(rng, (rows, K), np.complex64), _randn(rng, (K,), np.complex64)
    ref = _memo(lambda: (z.astype(np.complex128) * hh.astype(np.complex128)).astype(np.complex64))
    args = lambda i, o, h: (i[0], rows, K, _vp(hh), o[0], DEV)    # noqa: E731
    return Case("spectrum_mul", "nxsig_spectrum_mul_c64", [("z", z)], [("out", np.complex64, (rows, K))], args, _close(ref, TOL_MAX))


def spectrum_mask(kind, z_rows, mask_rows, M=5, K=30):
    rng = _rng(kind, z_rows, mask_rows)
    z = _randn(rng, (z_rows, M * K), np.complex64)
    per = {0: K, 1: K // 2 + 1, 2: K}[kind]           # nxsig_mask_kind: real, one-sided, complex
    mask = _randn(rng, (mask_rows, M * per), np.complex64) if kind == 2 else rng.random((mask_rows, M * per), dtype=np.float32)
    rows = max(z_rows, mask_rows)

    def ref():
        zz = np.broadcast_to(z.reshape(z_rows, M, K), (rows, M, K)).astype(np.complex128)
        m = np.broadcast_to(mask.reshape(mask_rows, M, per), (rows, M, per))
        if kind == 1:
            k = np.arange(K)
            m = m[..., np.where(k <= K // 2, k, K - k)]
        if kind == 2:
            return (zz * m.astype(np.complex128)).astype(np.complex64)
        m = m.astype(np.float64)
        return ((zz.real * m).astype(np.float32) + 1j * (zz.imag * m).astype(np.float32)).astype(np.complex64)

    args = lambda i, o, h: (i[0], z_rows, i[1], kind, mask_rows, M, K, o[0], DEV)    # noqa: E731
    return Case("spectrum_mask", "nxsig_spectrum_mask_c64", [("z", z), ("mask", mask)], [("out", np.complex64, (rows, M * K))], args,
                _close(_memo(ref), TOL_MAX))


# ------------------------------------------------------------------------------- the f64 tier
def istft_c128(N, hop, M, wide_window, rows=3):
    z = _randn(_rng(N, hop, M), (rows, M, N), np.complex128)
    w = S.windows.hann(N, type="f64") if wide_window else S.windows.hann(N)
    ref = _memo(lambda: O.istft_f64(z, w, overlap_length=N - hop))

    def args(i, o, h):
        h["p"] = _lib.StftParams(N, hop, N, 0, 0, 0, _lib.SCALE_NONE, 0, FS)
        return (i[0], M, rows, _vp(w), int(wide_window), C.byref(h["p"]), o[0], DEV)

    return Case("", "nxsig_istft_c128", [("z", z.reshape(rows, M * N))], [("y", np.complex128, (rows, M * hop + N - hop))], args, _close(ref, RTOL))


def fft_c128(K, inverse, real=False, rows=5):
    n_in = K
    x = _randn(_rng(K, int(inverse)), (rows, n_in), np.float64 if real else np.complex128)
    ref = _memo(lambda: O._eps_clean((np.fft.ifft if inverse else np.fft.fft)(x, n=K, axis=-1), O.FFT_EPS).astype(np.complex128))    # tests/test_gpu_f64.py
    args = lambda i, o, h: (i[0], int(real), rows, n_in, K, int(inverse), o[0], DEV)    # noqa: E731
    return Case("", "nxsig_fft_c128", [("in", x)], [("out", np.complex128, (rows, K))], args, _close(ref, RTOL))


# ------------------------------------------------------------------------------- the table: key -> (entry point, builder)
CASES = {}


def _add(key, builder, *a, **kw):
    assert key not in CASES, key
    CASES[key] = functools.partial(builder, *a, **kw)


ROWS2, ROWS3, COLS3 = (3, 1371), (3, 5, 275), (275, 5, 3)       # 4113 = KTILE + 17 and 4125 = KTILE + 29 elements: one full tile and a ragged one
assert ROWS2[0] * ROWS2[1] == KTILE + 17 and int(np.prod(ROWS3)) == int(np.prod(COLS3)) == KTILE + 29
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_PEAKS = [(f"rows:s{s}:{c}:{d.name}", "peaks.rows", ROWS2, 1, s, c, d, None) for s in (1, 9) for c in CMP for d in (_F32, _F64)] + \
         [(f"rows-rank3:{c}:{d.name}", "peaks.rows", ROWS3, 2, 1, c, d, None) for c in CMP for d in (_F32, _F64)] + \
         [(f"strided:s{s}:{c}:{d.name}", "peaks.strided", COLS3, 0, s, c, d, None) for s in (1, 9) for c in CMP for d in (_F32, _F64)] + \
         [("generic:rows-rank3:less:float32", "peaks.generic", ROWS3, 2, 9, "less", _F32, {"DISABLE_PEAK_TILES": 1}),
          ("generic:strided:greater_equal:float64", "peaks.generic", COLS3, 0, 1, "greater_equal", _F64, {"DISABLE_PEAK_TILES": 1})]


def _peak_seed(shape, axis, shifts, cmp, dt, want):
    """the first seed whose marks leave s0 = valid * rank `want` elements into a 16-byte group (the oracle alone decides)"""
    for seed in range(256):
        if int(P.argrelextrema(_peak_data(shape, dt, seed), cmp, axis, shifts)[1]) * len(shape) % 4 == want:
            return seed
    raise AssertionError((shape, axis, shifts, cmp, want))


PHASES = {}
for _n, (_key, _fam, _shape, _axis, _s, _c, _d, _tune) in enumerate(_PEAKS):
    _want = (_n + _n // 4) % 4 if len(_shape) % 2 else 2 * ((_n + _n // 2) % 2)           # an even rank leaves s0 even
    _seed = _peak_seed(_shape, _axis, _s, _c, _d, _want)
    PHASES[f"argrelextrema:{_key}"] = int(P.argrelextrema(_peak_data(_shape, _d, _seed), _c, _axis, _s)[1]) * len(_shape) % 4
    _add(f"argrelextrema:{_key}", peaks, _fam, _shape, _axis, _s, _c, _d, _seed, _tune)
# the condition of the fill's scalar head and tail: every phase of s0 = valid * rank within a 16-byte group occurs
assert set(PHASES.values()) == {0, 1, 2, 3}, PHASES
_add("argrelextrema:constant:less", peaks, "peaks.rows", ROWS2, 1, 1, "less", _F32, 0, None, True)        # valid = 0: every row -1
_add("argrelextrema:shifts0", peaks, "peaks.rows", ROWS2, 1, 0, "less", _F32, 0)                          # everything marked: no -1 row
for _shape in (ROWS2, (KTILE + 17,)):
    for _dens in (0, 0.5, 1):
        _add(f"nonzero:{'x'.join(map(str, _shape))}:{_dens}", nonzero, _shape, _dens)
# size 4115 = 3 mod 4, valid = 4114: s0 = 4114 and s1 = 4115 lie inside one 16-byte group, the fill's a0 > a1 branch
_add("nonzero:4115:last-group", nonzero, (KTILE + 19,), "last-group")

# median.rows: 512 outputs per workgroup, two per thread (1027 = 2 * 512 + 3; 31: the window is the row); median.plane: 128 x 4 tiles
_add("median:rows:3x1027:k9", median, "median.rows", (3, 2 * 512 + 3), (1, 9), _F32)
_add("median:rows:2x31:k31", median, "median.rows", (2, 31), (1, 31), _F32)
_add("median:rows:f64:3x515:k4", median, "median.rows", (3, 512 + 3), (1, 4), _F64)
_add("median:plane:2x7x131:k3x3", median, "median.plane", (2, 4 + 3, 128 + 3), (1, 3, 3), _F32)
_add("median:plane:2x9x129:k7x7", median, "median.plane", (2, 2 * 4 + 1, 128 + 1), (1, 7, 7), _F32)
_add("median:plane:f64:1x9x130:k2x7", median, "median.plane", (1, 2 * 4 + 1, 128 + 2), (1, 2, 7), _F64)
_add("median:generic:5x6x7", median, "median.generic", (5, 6, 7), (2, 3, 2), _F32)
_add("median:generic:3x4x5x6", median, "median.generic", (3, 4, 5, 6), (2, 2, 2, 2), _F32)
# wiener.plane: 64 x 4 tiles, kWMaxK 15
_add("wiener:plane:2x7x67:noise", wiener, "wiener.plane", (2, 4 + 3, 64 + 3), (1, 3, 5), _F32, 0.5)
_add("wiener:plane:2x7x67:estimated", wiener, "wiener.plane", (2, 4 + 3, 64 + 3), (1, 3, 5), _F32, None)
_add("wiener:plane:f64:1x17x65:k15", wiener, "wiener.plane", (1, 4 * 4 + 1, 64 + 1), (1, 15, 15), _F64, 0.5)
_add("wiener:generic:5x6x7:estimated", wiener, "wiener.generic", (5, 6, 7), 3, _F32, None)

# fft_nd: 64 x 64 transpose tiles; fft.tiled.columns takes powers of two 16 .. 1024 along an axis whose inner size is a multiple of 8
for _inv in (False, True):
    _t = "inverse" if _inv else "forward"
    _add(f"fft_nd:3x16x70:axis1:{_t}", fft_nd, "fft.transpose", (3, 16, 64 + 6), [1], [16], _inv)
    _add(f"fft_nd:2x12x5:axis1:{_t}", fft_nd, "fft.transpose", (2, 12, 5), [1], [12], _inv)
    _add(f"fft_nd:2x100x24:axis1:pad128:{_t}", fft_nd, "fft.tiled.columns", (2, 100, 24), [1], [128], _inv)
    _add(f"fft_nd:2x12x5:axis1:truncate8:{_t}", fft_nd, "fft.transpose", (2, 12, 5), [1], [8], _inv)
    _add(f"fft_nd:2x64x72:axes01:{_t}", fft_nd, "fft.transpose", (2, 64, 64 + 8), [0, 1], [4, 64], _inv)
_add("fft_nd:3x16x70:axis1:real", fft_nd, "fft.transpose", (3, 16, 70), [1], [16], False, True)
_add("fft_nd:3x16x70:no-axes", fft_nd, "", (3, 16, 70), [], [], False)
for _m in MODES:
    _add(f"fftconvolve_nd:12x17*5x4:{_m}", conv_nd, "fftconvolve_nd", "nxsig_fftconvolve_nd", (12, 17), (5, 4), _m, anywhere=True)
    if _m != "valid":       # neither operand is at least as large as the other in every dimension: test_a_refused_call_writes_nothing
        _add(f"fftconvolve_nd:6x1x9*3x7x2:c64:{_m}", conv_nd, "fftconvolve_nd", "nxsig_fftconvolve_nd", (6, 1, 9), (3, 7, 2), _m, np.complex64, anywhere=True)
    _add(f"fftconvolve_c64:300*41:{_m}", fftconvolve_c64, 300, 41, _m)
for _fam, _tune in (("convolve_direct.fast", None), ("convolve_direct.generic", {"DIRECT_FAST": 0})):     # the switch of tests/test_gpu_dispatch_switches.py
    for _m in MODES:
        _t = _fam.split(".")[1]
        _add(f"convolve_direct:{_t}:1000*7:{_m}", conv_nd, _fam, "nxsig_convolve_direct", (1000,), (7,), _m, tuning=_tune)
        _add(f"convolve_direct:{_t}:40x33*3x5:{_m}", conv_nd, _fam, "nxsig_convolve_direct", (40, 33), (3, 5), _m, tuning=_tune)
        _add(f"convolve_direct:{_t}:40x33*3x5:c64:{_m}", conv_nd, _fam, "nxsig_convolve_direct", (40, 33), (3, 5), _m, np.complex64, tuning=_tune)

for _wide in (False, True):
    _t = "f64" if _wide else "f32"
    # ola.v4: N % 4 == 0, hop % 4 == 0, one component, both pointers on a 16-byte boundary; the f64 entry has one kernel
    _add(f"ola:{_t}:M7:N8:hop4", ola, "" if _wide else "ola.v4", 7, 8, 4, 1, _wide)
    _add(f"ola:{_t}:M7:N10:hop3", ola, "" if _wide else "ola", 7, 10, 3, 1, _wide)
    _add(f"ola:{_t}:M7:N8:hop4:two-components", ola, "" if _wide else "ola", 7, 8, 4, 2, _wide)
    _add(f"ola:{_t}:M7:N8:hop8", ola, "" if _wide else "ola.v4", 7, 8, 8, 1, _wide)
    # as_windowed.v4: N % 4 == 0 and the result on a 16-byte boundary
    _add(f"as_windowed:{_t}:N6:hop4:reflect", as_windowed, "" if _wide else "as_windowed", 6, 4, 50, "reflect", _wide)
    for _pad in ("reflect", "same", (5, 3), (-2, -1)):
        _name = _pad if isinstance(_pad, str) else f"pads{_pad[0]},{_pad[1]}"
        _add(f"as_windowed:{_t}:N8:hop3:{_name}", as_windowed, "" if _wide else "as_windowed.v4", 8, 3, 50, _pad, _wide)

# mel.tile: up to 64 frames per tile, 67 = 64 + 3
for _fam, _tune in (("mel.tile", None), ("mel.pass1", {"MEL_TILE": 0})):
    _add(f"stft_to_mel:{_fam}:67xK64:8", mel, _fam, 64 + 3, 64, 8, _tune)
    _add(f"stft_to_mel:{_fam}:67xK512:40", mel, _fam, 64 + 3, 512, 40, _tune)
_add("spectrum_mul:5x30", spectrum_mul)
for _kind, _name in enumerate(("real", "onesided", "complex")):
    for _zr, _mr in ((3, 3), (1, 3), (3, 1)):
        _add(f"spectrum_mask:{_name}:z{_zr}:mask{_mr}", spectrum_mask, _kind, _zr, _mr)

for _ww in (True, False):
    _t = "f64-window" if _ww else "f32-window"
    _add(f"istft_c128:N64:hop16:M7:{_t}", istft_c128, 64, 16, 7, _ww)
    _add(f"istft_c128:N100:hop50:M7:{_t}", istft_c128, 100, 50, 7, _ww)
for _K in (64, 100, 1000):
    for _inv in (False, True):
        _add(f"fft_c128:K{_K}:{'inverse' if _inv else 'forward'}", fft_c128, _K, _inv)
_add("fft_c128:K100:real", fft_c128, 100, False, True)

KEYS = list(CASES)
# (key, which tensor lies 1 element off its 16-byte boundary)
OFFSET_KEYS = ["argrelextrema:rows:s1:less:float32", "argrelextrema:rows:s9:less:float32", "argrelextrema:rows:s1:greater_equal:float64",
               "argrelextrema:rows:s9:greater_equal:float64", "nonzero:3x1371:0.5", "ola:f32:M7:N8:hop4", "ola:f64:M7:N8:hop4",
               "as_windowed:f32:N8:hop3:reflect", "as_windowed:f64:N8:hop3:reflect", "median:rows:3x1027:k9", "median:rows:f64:3x515:k4",
               "spectrum_mul:5x30"]
assert set(OFFSET_KEYS) <= set(KEYS)

# the entry points of the issue's table: every one has a case, and include/nxsig.h declares every one the module calls
ENTRIES = ["nxsig_argrelextrema", "nxsig_nonzero", "nxsig_median_filter", "nxsig_wiener", "nxsig_fft_nd", "nxsig_fftconvolve_nd", "nxsig_fftconvolve_c64",
           "nxsig_convolve_direct", "nxsig_overlap_and_add", "nxsig_overlap_and_add_f64", "nxsig_as_windowed_f32", "nxsig_as_windowed_f64",
           "nxsig_stft_to_mel", "nxsig_spectrum_mul_c64", "nxsig_spectrum_mask_c64", "nxsig_istft_c128", "nxsig_fft_c128"]
ENTRY_OF = {"argrelextrema": "nxsig_argrelextrema", "nonzero": "nxsig_nonzero", "median": "nxsig_median_filter", "wiener": "nxsig_wiener",
            "fft_nd": "nxsig_fft_nd", "fftconvolve_nd": "nxsig_fftconvolve_nd", "fftconvolve_c64": "nxsig_fftconvolve_c64",
            "convolve_direct": "nxsig_convolve_direct", "ola:f32": "nxsig_overlap_and_add", "ola:f64": "nxsig_overlap_and_add_f64",
            "as_windowed:f32": "nxsig_as_windowed_f32", "as_windowed:f64": "nxsig_as_windowed_f64", "stft_to_mel": "nxsig_stft_to_mel",
            "spectrum_mul": "nxsig_spectrum_mul_c64", "spectrum_mask": "nxsig_spectrum_mask_c64", "istft_c128": "nxsig_istft_c128",
            "fft_c128": "nxsig_fft_c128"}


def _entry(key):
    return ENTRY_OF[next(p for p in sorted(ENTRY_OF, key=len, reverse=True) if key.startswith(p + ":"))]


with open(os.path.join(HERE, "..", "include", "nxsig.h")) as _f:
    assert sorted({_entry(k) for k in KEYS}) == sorted(ENTRIES) == sorted(set(re.findall(r"\bint (nxsig_\w+)\(", _f.read())) & set(ENTRIES))

# key -> dispatch record; filled from a probe run (NXSIG_DISPATCH_PROBE=1)
RECORDS = {
    "argrelextrema:rows:s1:less:float32": "peaks.rows", "argrelextrema:rows:s1:less:float64": "peaks.rows",
    "argrelextrema:rows:s1:greater_equal:float32": "peaks.rows", "argrelextrema:rows:s1:greater_equal:float64": "peaks.rows",
    "argrelextrema:rows:s9:less:float32": "peaks.rows", "argrelextrema:rows:s9:less:float64": "peaks.rows",
    "argrelextrema:rows:s9:greater_equal:float32": "peaks.rows", "argrelextrema:rows:s9:greater_equal:float64": "peaks.rows",
    "argrelextrema:rows-rank3:less:float32": "peaks.rows", "argrelextrema:rows-rank3:less:float64": "peaks.rows",
    "argrelextrema:rows-rank3:greater_equal:float32": "peaks.rows", "argrelextrema:rows-rank3:greater_equal:float64": "peaks.rows",
    "argrelextrema:strided:s1:less:float32": "peaks.strided", "argrelextrema:strided:s1:less:float64": "peaks.strided",
    "argrelextrema:strided:s1:greater_equal:float32": "peaks.strided", "argrelextrema:strided:s1:greater_equal:float64": "peaks.strided",
    "argrelextrema:strided:s9:less:float32": "peaks.strided", "argrelextrema:strided:s9:less:float64": "peaks.strided",
    "argrelextrema:strided:s9:greater_equal:float32": "peaks.strided", "argrelextrema:strided:s9:greater_equal:float64": "peaks.strided",
    "argrelextrema:generic:rows-rank3:less:float32": "peaks.generic", "argrelextrema:generic:strided:greater_equal:float64": "peaks.generic",
    "argrelextrema:constant:less": "peaks.rows", "argrelextrema:shifts0": "peaks.rows", "nonzero:3x1371:0": "nonzero",
    "nonzero:3x1371:0.5": "nonzero", "nonzero:3x1371:1": "nonzero", "nonzero:4113:0": "nonzero", "nonzero:4113:0.5": "nonzero",
    "nonzero:4113:1": "nonzero", "nonzero:4115:last-group": "nonzero", "median:rows:3x1027:k9": "median.rows",
    "median:rows:2x31:k31": "median.rows", "median:rows:f64:3x515:k4": "median.rows", "median:plane:2x7x131:k3x3": "median.plane",
    "median:plane:2x9x129:k7x7": "median.plane", "median:plane:f64:1x9x130:k2x7": "median.plane", "median:generic:5x6x7": "median.generic",
    "median:generic:3x4x5x6": "median.generic", "wiener:plane:2x7x67:noise": "wiener.plane", "wiener:plane:2x7x67:estimated": "wiener.plane",
    "wiener:plane:f64:1x17x65:k15": "wiener.plane", "wiener:generic:5x6x7:estimated": "wiener.generic",
    "fft_nd:3x16x70:axis1:forward": "fft.transpose+fft.rows_generic.pow2", "fft_nd:2x12x5:axis1:forward": "fft.transpose+fft.rows_generic.dft",
    "fft_nd:2x100x24:axis1:pad128:forward": "fft.tiled.columns", "fft_nd:2x12x5:axis1:truncate8:forward": "fft.transpose+fft.rows_generic.pow2",
    "fft_nd:2x64x72:axes01:forward": "fft.transpose+fft.rows_generic.pow2+fft.tiled.columns",
    "fft_nd:3x16x70:axis1:inverse": "fft.transpose+fft.rows_generic.pow2", "fft_nd:2x12x5:axis1:inverse": "fft.transpose+fft.rows_generic.dft",
    "fft_nd:2x100x24:axis1:pad128:inverse": "fft.tiled.columns", "fft_nd:2x12x5:axis1:truncate8:inverse": "fft.transpose+fft.rows_generic.pow2",
    "fft_nd:2x64x72:axes01:inverse": "fft.transpose+fft.rows_generic.pow2+fft.tiled.columns",
    "fft_nd:3x16x70:axis1:real": "fft.transpose+fft.rows_generic.pow2", "fft_nd:3x16x70:no-axes": "",
    "fftconvolve_nd:12x17*5x4:full": "fft.transpose+fft.rows_generic.pow2+fftconvolve_nd+fft.tiled.columns",
    "fftconvolve_nd:6x1x9*3x7x2:c64:full": "fft.transpose+fft.rows_generic.pow2+fftconvolve_nd",
    "fftconvolve_c64:300*41:full": "fft.rows_generic.pow2",
    "fftconvolve_nd:12x17*5x4:same": "fft.transpose+fft.rows_generic.pow2+fftconvolve_nd+fft.tiled.columns",
    "fftconvolve_nd:6x1x9*3x7x2:c64:same": "fft.transpose+fft.rows_generic.pow2+fftconvolve_nd",
    "fftconvolve_c64:300*41:same": "fft.rows_generic.pow2",
    "fftconvolve_nd:12x17*5x4:valid": "fft.transpose+fft.rows_generic.pow2+fftconvolve_nd+fft.tiled.columns",
    "fftconvolve_c64:300*41:valid": "fft.rows_generic.pow2", "convolve_direct:fast:1000*7:full": "convolve_direct.fast",
    "convolve_direct:fast:40x33*3x5:full": "convolve_direct.fast", "convolve_direct:fast:40x33*3x5:c64:full": "convolve_direct.fast",
    "convolve_direct:fast:1000*7:same": "convolve_direct.fast", "convolve_direct:fast:40x33*3x5:same": "convolve_direct.fast",
    "convolve_direct:fast:40x33*3x5:c64:same": "convolve_direct.fast", "convolve_direct:fast:1000*7:valid": "convolve_direct.fast",
    "convolve_direct:fast:40x33*3x5:valid": "convolve_direct.fast", "convolve_direct:fast:40x33*3x5:c64:valid": "convolve_direct.fast",
    "convolve_direct:generic:1000*7:full": "convolve_direct.generic", "convolve_direct:generic:40x33*3x5:full": "convolve_direct.generic",
    "convolve_direct:generic:40x33*3x5:c64:full": "convolve_direct.generic", "convolve_direct:generic:1000*7:same": "convolve_direct.generic",
    "convolve_direct:generic:40x33*3x5:same": "convolve_direct.generic", "convolve_direct:generic:40x33*3x5:c64:same": "convolve_direct.generic",
    "convolve_direct:generic:1000*7:valid": "convolve_direct.generic", "convolve_direct:generic:40x33*3x5:valid": "convolve_direct.generic",
    "convolve_direct:generic:40x33*3x5:c64:valid": "convolve_direct.generic", "ola:f32:M7:N8:hop4": "ola.v4", "ola:f32:M7:N10:hop3": "ola",
    "ola:f32:M7:N8:hop4:two-components": "ola", "ola:f32:M7:N8:hop8": "ola.v4", "as_windowed:f32:N6:hop4:reflect": "as_windowed",
    "as_windowed:f32:N8:hop3:reflect": "as_windowed.v4", "as_windowed:f32:N8:hop3:same": "as_windowed.v4",
    "as_windowed:f32:N8:hop3:pads5,3": "as_windowed.v4", "as_windowed:f32:N8:hop3:pads-2,-1": "as_windowed.v4", "ola:f64:M7:N8:hop4": "",
    "ola:f64:M7:N10:hop3": "", "ola:f64:M7:N8:hop4:two-components": "", "ola:f64:M7:N8:hop8": "", "as_windowed:f64:N6:hop4:reflect": "",
    "as_windowed:f64:N8:hop3:reflect": "", "as_windowed:f64:N8:hop3:same": "", "as_windowed:f64:N8:hop3:pads5,3": "",
    "as_windowed:f64:N8:hop3:pads-2,-1": "", "stft_to_mel:mel.tile:67xK64:8": "mel.tile", "stft_to_mel:mel.tile:67xK512:40": "mel.tile",
    "stft_to_mel:mel.pass1:67xK64:8": "mel.pass1", "stft_to_mel:mel.pass1:67xK512:40": "mel.pass1", "spectrum_mul:5x30": "spectrum_mul",
    "spectrum_mask:real:z3:mask3": "spectrum_mask", "spectrum_mask:real:z1:mask3": "spectrum_mask", "spectrum_mask:real:z3:mask1": "spectrum_mask",
    "spectrum_mask:onesided:z3:mask3": "spectrum_mask", "spectrum_mask:onesided:z1:mask3": "spectrum_mask",
    "spectrum_mask:onesided:z3:mask1": "spectrum_mask", "spectrum_mask:complex:z3:mask3": "spectrum_mask",
    "spectrum_mask:complex:z1:mask3": "spectrum_mask", "spectrum_mask:complex:z3:mask1": "spectrum_mask", "istft_c128:N64:hop16:M7:f64-window": "",
    "istft_c128:N100:hop50:M7:f64-window": "", "istft_c128:N64:hop16:M7:f32-window": "", "istft_c128:N100:hop50:M7:f32-window": "",
    "fft_c128:K64:forward": "", "fft_c128:K64:inverse": "", "fft_c128:K100:forward": "", "fft_c128:K100:inverse": "", "fft_c128:K1000:forward": "",
    "fft_c128:K1000:inverse": "", "fft_c128:K100:real": "",
}
assert set(RECORDS) == set(KEYS)
# (key, "result" | "input") -> dispatch record with that tensor 1 element off its 16-byte boundary: the 16-byte paths of ola.v4 and
# as_windowed.v4 decline (kernels_generic.hip: launch_overlap_and_add tests both pointers, launch_as_windowed the result's)
OFFSET_RECORDS = {
    ("argrelextrema:rows:s1:less:float32", "result"): "peaks.rows", ("argrelextrema:rows:s1:less:float32", "input"): "peaks.rows",
    ("argrelextrema:rows:s9:less:float32", "result"): "peaks.rows", ("argrelextrema:rows:s9:less:float32", "input"): "peaks.rows",
    ("argrelextrema:rows:s1:greater_equal:float64", "result"): "peaks.rows", ("argrelextrema:rows:s1:greater_equal:float64", "input"): "peaks.rows",
    ("argrelextrema:rows:s9:greater_equal:float64", "result"): "peaks.rows", ("argrelextrema:rows:s9:greater_equal:float64", "input"): "peaks.rows",
    ("nonzero:3x1371:0.5", "result"): "nonzero", ("nonzero:3x1371:0.5", "input"): "nonzero", ("ola:f32:M7:N8:hop4", "result"): "ola",
    ("ola:f32:M7:N8:hop4", "input"): "ola", ("ola:f64:M7:N8:hop4", "result"): "", ("ola:f64:M7:N8:hop4", "input"): "",
    ("as_windowed:f32:N8:hop3:reflect", "result"): "as_windowed", ("as_windowed:f32:N8:hop3:reflect", "input"): "as_windowed.v4",
    ("as_windowed:f64:N8:hop3:reflect", "result"): "", ("as_windowed:f64:N8:hop3:reflect", "input"): "",
    ("median:rows:3x1027:k9", "result"): "median.rows", ("median:rows:3x1027:k9", "input"): "median.rows",
    ("median:rows:f64:3x515:k4", "result"): "median.rows", ("median:rows:f64:3x515:k4", "input"): "median.rows",
    ("spectrum_mul:5x30", "result"): "spectrum_mul", ("spectrum_mul:5x30", "input"): "spectrum_mul",
}
assert set(OFFSET_RECORDS) == {(k, w) for k in OFFSET_KEYS for w in ("result", "input")}

_cache = {}


def _case(key):
    if key not in _cache:
        _cache[key] = CASES[key]()
        assert _cache[key].entry == _entry(key), key
    return _cache[key]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _call(ctx, *a):
    """E.call; a HIP error ends the session — nothing more is started on a device that has faulted"""
    try:
        return E.call(ctx, *a)
    except _lib.NxSignalDeviceError as e:
        pytest.exit(f"device error, the run ends here: {e}", returncode=3)


def _arena(name, a, off=0):
    rows, n = _rows(a.shape)
    return E.Arena(name, a.dtype, rows, n, offset_elems=off, data=a)


def _run(ctx, case, result_off=0, input_off=0):
    """the call through the arenas: (input arenas, result arenas, their images after the call, host-side outputs, dispatch record)"""
    ins = [_arena(n, a, input_off if q == 0 else 0).upload(ctx) for q, (n, a) in enumerate(case.ins)]
    outs = [E.Arena(n, dt, *_rows(sh), offset_elems=result_off if q == 0 else 0).upload(ctx) for q, (n, dt, sh) in enumerate(case.outs)]
    host = {}
    with R._Tuned(ctx, case):
        rec = _call(ctx, case.invoke, [a.ptr for a in ins], [o.ptr for o in outs], host)
    return ins, outs, [o.download() for o in outs], host, rec


def _plain(ctx, case):
    """the same call into plain nxsig_alloc buffers: (results, dispatch record)"""
    xs = [ctx.to_device(a) for _, a in case.ins]
    ys = [ctx.empty(_rows(sh), dt) for _, dt, sh in case.outs]
    with R._Tuned(ctx, case):
        rec = _call(ctx, case.invoke, [C.c_void_p(x.ptr) for x in xs], [C.c_void_p(y.ptr) for y in ys], {})
    return [y.numpy() for y in ys], rec


def _integer(arena):
    return arena.dtype.kind in "iu"


def _extent_findings(ins, outs, images, plain=None):
    found = []
    for a in ins:
        found += E.unchanged_findings(a, a.download())
    for q, (o, img) in enumerate(zip(outs, images)):
        found += E.guard_findings(o, img)
        if _integer(o):
            found += E.table_unwritten_findings(o, img)
            if plain is not None:
                found += [f"against the plain call — {f}" for f in E.table_findings(o, o.tensor(img), plain[q])]
        elif plain is not None:
            found += E.unwritten_findings(o, img, plain[q]) + E.bit_findings(o, o.tensor(img), plain[q])
    return found


def _leads(case, rec):
    if case.anywhere:               # the n-D convolution transforms its operands first: its own family follows theirs
        return case.family in rec.split("+")
    return rec == case.family or (case.family != "" and rec.startswith(case.family + "+"))


@pytest.mark.parametrize("key", KEYS)
def test_a_call_writes_its_result_and_nothing_else(ctx, key):
    case = _case(key)
    ins, outs, images, host, rec = _run(ctx, case)
    plain, rec_plain = _plain(ctx, case)
    for p, o in zip(plain, outs):
        assert _integer(o) or np.isfinite(E._components(p)).all(), key
    found = _extent_findings(ins, outs, images, plain) + case.judge(outs, [o.tensor(i) for o, i in zip(outs, images)], host)
    if found:
        raise E.ExtentError(f"{key}\n" + "\n".join(found))
    if PROBE:
        print(f'\nPROBE    "{key}": "{rec}",' + ("" if rec == rec_plain else f'   PLAIN "{rec_plain}"'))
        return
    assert rec == rec_plain == RECORDS[key], (key, rec, rec_plain)
    assert _leads(case, rec), (key, rec, case.family)


@pytest.mark.parametrize("which", ["result", "input"])
@pytest.mark.parametrize("key", OFFSET_KEYS)
def test_a_tensor_one_element_off_its_16_byte_boundary(ctx, key, which):
    """the first result, or the first input, one element into a 16-byte group (4 bytes of an f32 / s32 tensor, 8 of f64 / c64, 1 of the u8
    mask): the guards, every input unchanged, the values against the oracle (the family may differ from the aligned call's)"""
    case = _case(key)
    ins, outs, images, host, rec = _run(ctx, case, result_off=int(which == "result"), input_off=int(which == "input"))
    found = _extent_findings(ins, outs, images) + case.judge(outs, [o.tensor(i) for o, i in zip(outs, images)], host)
    for o, img in zip(outs, images):
        if not _integer(o):
            found += E.unwritten_findings(o, img, np.zeros((o.rows, o.row_len), o.dtype))
    if found:
        raise E.ExtentError(f"{key}, {which} off its boundary\n" + "\n".join(found))
    if PROBE:
        print(f'\nPROBE-OFFSET    ("{key}", "{which}"): "{rec}",')
        return
    assert rec == OFFSET_RECORDS[(key, which)], (key, which, rec)


def test_spectrum_mul_in_place(ctx):
    """include/nxsig.h: "out may alias z" — out = z in one arena: the bits of the out-of-place call, both guards intact"""
    case = _case("spectrum_mul:5x30")
    want, _ = _plain(ctx, case)
    z = _arena("z", case.ins[0][1]).upload(ctx)
    rec = _call(ctx, case.invoke, [z.ptr], [z.ptr], {})
    img = z.download()
    E.verify([], z, img, expected=want[0], same_bits_as=want[0])
    assert rec == "spectrum_mul"


def test_a_refused_call_writes_nothing(ctx):
    """:valid of (6, 1, 9) with (3, 7, 2), the third mode of the broadcast case: neither operand covers the other (convolution.ex:335-347),
    NXSIG_ERR_INVALID_ARG — and the result arena, out_shape and both operands stay as they were"""
    rng = _rng(6, 3)
    a, b = _randn(rng, (6, 1, 9), np.complex64), _randn(rng, (3, 7, 2), np.float32)
    ins = [_arena("a", a).upload(ctx), _arena("b", b).upload(ctx)]
    out = E.Arena("out", np.complex64, 1, 8 * 7 * 10).upload(ctx)          # room for the :full result
    osh = _i64([-1] * 3)
    rc = _lib.load().nxsig_fftconvolve_nd(ctx.handle, ins[0].ptr, 0, _i64(a.shape), ins[1].ptr, 1, _i64(b.shape), 3, MODES["valid"], out.ptr, osh, DEV)
    ctx.sync()
    assert rc == _lib.ERR_INVALID_ARG and "valid" in _lib.last_error() and list(osh) == [-1] * 3
    found = [f for x in ins + [out] for f in E.unchanged_findings(x, x.download())]
    assert found == [], found
