"""Rows `batch_stride` > length apart through every C ABI entry point that takes a row stride (include/nxsig.h), on every kernel family.

The Python mirror, the NIF and sharding.py pass batch_stride == length, so the rest of the suite runs dense rows; the launchers route on
the stride's low bits (stage_aligned, the 8-byte-load gates, fir rows2 / rows4, per-unit `mis`, per-pointer 16-byte tests, slab splits,
host uploads).  Here every family of FAMILIES runs with d = stride - length in {1, 2, 3, 4, 37, D256} through the arenas of
tests/extents.py: the gaps between the rows and 4 KB on either side of every tensor hold a NaN pattern, so

* a gap or guard element that reaches a result is a NaN the oracle does not have (the finite mask must equal the oracle's exactly),
* a store outside the result changes a guard, a result element nobody wrote still holds the pattern,
* an input arena that does not come back bit for bit was written to.

d = D256 (the smallest gap of a multiple of 256 bytes) keeps every row on the dense call's alignment: the same bits and the same
dispatch record as the dense call.  Every other d: the oracle at the suite's bounds (1e-5 normalised for f32 / c64, 1e-12 for f64 /
c128, the sinks at the bounds of their parity tests), and the dispatch record pinned in RECORDS.

NXSIG_DISPATCH_PROBE=1 prints the records instead of asserting them (how RECORDS was filled)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extents as E
import nx_signal_amd as S
from nx_signal_amd import _lib
from oracle import nx_oracle as O

pytestmark = pytest.mark.gpu
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"

TOL_MAX = 1e-5      # tests/test_gpu_parity.py
RTOL = 1.0e-12      # tests/test_gpu_f64.py
MEL_ATOL = 1e-4     # log-mel sinks: tests/test_gpu_tuned_kernels.py
DB_ATOL = 1e-2      # dBFS, bins above -80 dB: tests/test_gpu_parity.py::test_spectrogram_magnitude_power_dbfs
FS = 16000.0
MEL_BINS = 40
DS = (1, 2, 3, 4, 37, "D256")
VALID, REFLECT = _lib.PAD_VALID, _lib.PAD_REFLECT
MODES = {"full": _lib.CONV_FULL, "same": _lib.CONV_SAME, "valid": _lib.CONV_VALID}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Stft:
    """one framing + transform entry point: nxsig_stft_{f32,c64,f64,c128}, _onesided, _packed, _magnitude (abs / dbfs), _mel"""
    ENTRY = {"stft": "nxsig_stft_f32", "c64": "nxsig_stft_c64", "f64": "nxsig_stft_f64", "c128": "nxsig_stft_c128",
             "onesided": "nxsig_stft_onesided_f32", "packed": "nxsig_stft_packed_f32", "mag": "nxsig_stft_magnitude_f32",
             "dbfs": "nxsig_stft_magnitude_f32", "mel": "nxsig_stft_mel_f32"}
    IN = {"c64": np.complex64, "f64": np.float64, "c128": np.complex128}

    def __init__(self, family, N, hop, K, sink="stft", pad=VALID, tuning=None, rows=5, frames=None):
        self.family, self.N, self.hop, self.K, self.sink, self.pad, self.tuning = family, N, hop, K, sink, pad, tuning or {}
        self.B = rows
        frames = frames or (45 if K <= 1024 else 21)    # an odd, ragged unit count per row: workgroups straddle the row seams
        self.L = (frames - 1) * hop + N + 3          # three samples behind the last frame
        self.M = int(_lib.load().nxsig_num_frames(self.L, N, hop, pad, 0, 0))
        self.in_dtype = np.dtype(self.IN.get(sink, np.float32))
        self.wide = sink in ("f64", "c128")
        per = {"stft": K, "c64": K, "f64": K, "c128": K, "onesided": K // 2, "packed": K // 2, "mag": K // 2, "dbfs": K // 2, "mel": MEL_BINS}[sink]
        self.unit = per
        self.out_len = self.M * per
        self.out_dtype = np.dtype(np.complex128 if self.wide else (np.float32 if sink in ("mag", "dbfs", "mel") else np.complex64))
        self.window = S.windows.hann(N, type="f64") if self.wide else S.windows.hann(N)
        self.filters = S.mel_filters(K, MEL_BINS, FS) if sink == "mel" else None
        self.entry = self.ENTRY[sink]

    def data(self):
        rng = np.random.Generator(np.random.PCG64(self.N * 7 + self.K))
        x = rng.standard_normal((self.B, self.L))
        if self.in_dtype.kind == "c":
            x = x + 1j * rng.standard_normal((self.B, self.L))
        return x.astype(self.in_dtype)

    def invoke(self, handle, xptr, stride, outptr, mem):
        lib = _lib.load()
        p = _lib.StftParams(self.N, self.hop, self.K, self.pad, 0, 0, _lib.SCALE_NONE, 0, FS)
        head = (handle, xptr, self.L, self.B, stride, _vp(self.window))
        if self.wide:
            return getattr(lib, self.entry)(*head, 1, C.byref(p), outptr, None, mem)
        if self.sink in ("mag", "dbfs"):
            return getattr(lib, self.entry)(*head, C.byref(p), _lib.MAG_DBFS if self.sink == "dbfs" else _lib.MAG_ABS, outptr, None, mem)
        if self.sink == "mel":
            return getattr(lib, self.entry)(*head, C.byref(p), MEL_BINS, _vp(self.filters), outptr, None, mem)
        return getattr(lib, self.entry)(*head, C.byref(p), outptr, None, mem)

    def oracle(self, x):
        """(expected [B][out_len], bound, absolute?, where to compare values)"""
        pad = "reflect" if self.pad == REFLECT else "valid"
        opts = dict(overlap_length=self.N - self.hop, fft_length=self.K, window_padding=pad, sampling_rate=FS)
        if self.wide:
            return O.stft_f64(x, self.window, **opts)[0].reshape(self.B, -1), RTOL, False, None
        zo = O.stft(x, self.window, **opts)[0]
        half = self.K // 2
        if self.sink in ("stft", "c64"):
            return zo.reshape(self.B, -1), TOL_MAX, False, None
        if self.sink == "onesided":
            return zo[..., :half].reshape(self.B, -1), TOL_MAX, False, None
        if self.sink == "packed":       # the imaginary part of bin 0 carries Re X[K / 2]
            pk = zo[..., :half].copy()
            pk[..., 0] = zo[..., 0].real + 1j * zo[..., half].real
            return pk.reshape(self.B, -1), TOL_MAX, False, None
        mag = np.abs(zo[..., :half].astype(np.complex128)).astype(np.float32)
        if self.sink == "mag":
            return mag.reshape(self.B, -1), TOL_MAX, False, None
        if self.sink == "dbfs":
            # the maximum over the finite magnitudes: no reference defines the dBFS of a tensor that holds a NaN (the sink is not in the
            # reference API), so a non-finite sample is held to the stft rule — it reaches exactly its own frames
            with np.errstate(divide="ignore", invalid="ignore"):
                db = 20.0 * np.log10(mag.astype(np.float64) / float(np.nanmax(mag)))
            return db.reshape(self.B, -1), DB_ATOL, True, (db > -80.0).reshape(self.B, -1)   # below: the log amplifies fp32 round-off
        with np.errstate(invalid="ignore"):
            mel = O.stft_to_mel(zo.reshape(-1, self.K), FS, self.K, MEL_BINS)
        return mel.reshape(self.B, -1), MEL_ATOL, True, None


class AsWindowed:
    def __init__(self, family, wide=False):
        self.family, self.wide, self.tuning = family, wide, {}
        self.N, self.stride_w, self.B = 1024, 256, 5
        self.L = 44 * 256 + 1024 + 3
        self.M = (self.L - self.N) // self.stride_w + 1
        self.in_dtype = self.out_dtype = np.dtype(np.float64 if wide else np.float32)
        self.unit, self.out_len = self.N, self.M * self.N
        self.entry = "nxsig_as_windowed_f64" if wide else "nxsig_as_windowed_f32"

    def data(self):
        return np.random.Generator(np.random.PCG64(5)).standard_normal((self.B, self.L)).astype(self.in_dtype)

    def invoke(self, handle, xptr, stride, outptr, mem):
        return getattr(_lib.load(), self.entry)(handle, xptr, self.L, self.B, stride, self.N, self.stride_w, VALID, 0, 0, outptr, None, mem)

    def oracle(self, x):
        return O.as_windowed(x, self.N, self.stride_w).reshape(self.B, -1), 0.0, True, None     # index-only: exact


class Fir:
    """nxsig_fir_{f32,f64} in one mode, or nxsig_fir_slice_{f32,f64} (slice = (out_start, out_len) of the full convolution)"""

    def __init__(self, family, taps, mode=None, rows=37, L=9003, wide=False, slice_=None):
        self.family, self.taps, self.mode, self.B, self.L, self.wide, self.slice, self.tuning = family, taps, mode, rows, L, wide, slice_, {}
        full = L + taps - 1
        if slice_ is not None:
            self.start, self.out_len = slice_
        else:
            self.out_len = {"full": full, "same": L, "valid": L - taps + 1}[mode]
            self.start = {"full": 0, "same": (taps - 1) // 2, "valid": taps - 1}[mode]
        assert 0 <= self.start and self.start + self.out_len <= full
        self.unit = 1
        self.in_dtype = self.out_dtype = np.dtype(np.float64 if wide else np.float32)
        self.entry = ("nxsig_fir_slice_" if slice_ is not None else "nxsig_fir_") + ("f64" if wide else "f32")
        self.h = (np.random.Generator(np.random.PCG64(taps)).standard_normal(taps) / taps ** 0.5).astype(self.in_dtype)

    def data(self):
        return np.random.Generator(np.random.PCG64(self.taps + self.B)).standard_normal((self.B, self.L)).astype(self.in_dtype)

    def invoke(self, handle, xptr, stride, outptr, mem):
        head = (handle, xptr, self.L, self.B, stride, _vp(self.h), self.taps)
        if self.slice is not None:
            return getattr(_lib.load(), self.entry)(*head, self.start, self.out_len, outptr, mem)
        return getattr(_lib.load(), self.entry)(*head, MODES[self.mode], outptr, mem)

    def oracle(self, x):
        full = _full_convolution(self.taps, self.B, self.L, self.wide, x.tobytes(), self.h.tobytes())
        # the reference filters a row by ONE transform: a row that holds a NaN has no finite output (include/nxsig.h, nxsig_fir_slice_f32)
        bad = ~np.isfinite(x).all(axis=1)
        ref = full[:, self.start:self.start + self.out_len].copy()
        ref[bad] = np.nan
        return ref, (RTOL if self.wide else TOL_MAX), False, None


@functools.lru_cache(maxsize=4)
def _full_convolution(taps, B, L, wide, xbytes, hbytes):
    """the full convolution of every row in double: np.convolve, as the neighbouring FIR tests; the one-transform family (40 001 taps on
    70 001 samples, 2.8e9 products) through the oracle's fftconvolve; shared by the three modes of a tap count"""
    dt = np.float64 if wide else np.float32
    x, h = np.frombuffer(xbytes, dt).reshape(B, L), np.frombuffer(hbytes, dt)
    x = np.where(np.isfinite(x), x, 0.0)
    if taps > 5000:
        return np.stack([O.fftconvolve(r.astype(np.float32), h, "full").astype(np.float64) for r in x])
    return np.stack([np.convolve(r.astype(np.float64), h.astype(np.float64)) for r in x])


def _fir3(name, family, taps, **kw):
    return {f"{name}:{m}": Fir(family, taps, m, **kw) for m in MODES}


# key -> case.  `family`: what DESIGN.md section 3 / tests/test_gpu_dispatch_table.py name for the geometry; it must LEAD the dense record.
@functools.lru_cache(maxsize=1)
def families():
    t = {
        # ---- stft, f32 samples
        "stft1024": Stft("stft.pair.1r", 1024, 256, 1024),
        "stft1024-many-rounds": Stft("stft.pair", 1024, 256, 1024, tuning={"WAVE_SMALL_W": 0}),   # the geometry of launches beyond 24 pairs per CU
        "stft1024-reflect": Stft("stft.pair.1r+stft.pair.1r.edge", 1024, 256, 1024, pad=REFLECT),
        "stft512": Stft("stft.quad2", 512, 128, 512),
        "stft400-in-512": Stft("stft.quad2", 400, 160, 512),
        "stft256": Stft("stft.quad4", 256, 64, 256),
        "stft128": Stft("stft.quad8", 128, 32, 128),
        "stft2048": Stft("stft.real2x", 2048, 512, 2048),
        "stft4096": Stft("stft.real2x.4k", 4096, 1024, 4096),
        "stft8192": Stft("stft.8k", 8192, 2048, 8192),
        "stft400": Stft("stft.r20", 400, 160, 400),
        "stft320": Stft("stft.rab", 320, 80, 320),
        "stft882": Stft("stft.rab", 882, 220, 882),
        "stft441-odd": Stft("stft.rab", 441, 110, 441),
        "stft443": Stft("stft.blue", 443, 110, 443),
        "stft16": Stft("stft.generic.pow2", 16, 4, 16),
        "stft2310": Stft("stft.generic.blue", 2310, 577, 2310),
        # ---- stft, c64 samples
        "stft-c64-512": Stft("stft_c64.rab", 512, 128, 512, "c64"),
        "stft-c64-2048": Stft("stft_c64.rows", 2048, 512, 2048, "c64"),
        # ---- f64 / c128
        "stft-f64-512": Stft("", 512, 128, 512, "f64"),             # the f64 tier (kernels_f64.hip) notes no family: only nxsig_stft_c128 does (api.cpp:2270)
        "stft-c128-512": Stft("stft.f64.c128", 512, 128, 512, "c128"),
        # ---- as_windowed
        "as_windowed": AsWindowed("as_windowed.v4"),
        "as_windowed-f64": AsWindowed("", wide=True),
        # ---- fir_slice, f64
        "fir257-slice": Fir("fir.wave32", 257, slice_=(101, 9003 + 256 - 101)),          # out_start not a multiple of 4
        "fir257-f64:same": Fir("", 257, "same", wide=True),
        "fir257-f64-slice": Fir("", 257, wide=True, slice_=(101, 9003 + 256 - 101)),
    }
    for n, k in ((1024, 256), (512, 128)):     # ---- fused sinks
        # (the one-sided and packed layouts are sinks of the magnitude kernels; packed at 512 is the full transform + a packing pass)
        for sink, fam in (("onesided", "mag"), ("packed", "mag" if n == 1024 else "stft"), ("mag", "mag"), ("dbfs", "mag"), ("mel", "mel")):
            t[f"{sink}{n}"] = Stft(f"{fam}.{'pair' if n == 1024 else 'quad2'}", n, k, n, sink)
    t.update(_fir3("fir257", "fir.pair", 257))
    t.update(_fir3("fir100", "fir.wave32", 100))
    t.update(_fir3("fir513", "fir.r2k", 513))
    t.update(_fir3("fir1025", "fir.r2k", 1025))
    t.update(_fir3("fir4097", "fir.dline", 4097, rows=3, L=20011))
    t.update(_fir3("fir40001", "fir.long", 40001, rows=1, L=70001))
    return t


def _keys():
    return ["stft1024", "stft1024-many-rounds", "stft1024-reflect", "stft512", "stft400-in-512", "stft256", "stft128", "stft2048", "stft4096",
            "stft8192", "stft400", "stft320", "stft882", "stft441-odd", "stft443", "stft16", "stft2310", "stft-c64-512", "stft-c64-2048",
            "stft-f64-512", "stft-c128-512", "as_windowed", "as_windowed-f64", "fir257-slice", "fir257-f64:same", "fir257-f64-slice"] + \
           [f"{s}{n}" for n in (1024, 512) for s in ("onesided", "packed", "mag", "dbfs", "mel")] + \
           [f"fir{t}:{m}" for t in (257, 100, 513, 1025, 4097, 40001) for m in MODES]


KEYS = _keys()

# key -> (dense record, {d: record where it differs from the dense one}); filled from a probe run (NXSIG_DISPATCH_PROBE=1).
# The forward transforms keep their record at every d: a stride class only selects another instantiation of the same family
# (wave_stft.hpp, launch_wave: stage_aligned picks the padded / unpadded staged quad kernel, the (batch_stride & 1) gate the 8-byte or
# 4-byte loads of real2x; wave_rab.hpp / kernels_wave_r20.hip / kernels_wave_firlong.hip choose per unit from the pointer).  The
# tuned FIR launcher (kernels_wave.hip, launch_fir_wave_W) routes on it, with 37 rows under the per-row grid phase (row_mod != 0):
#   rows2 = (s.batch_stride - s.out_len) % 2 == 0, rows4 = (s.batch_stride - s.out_len) % 4 == 0
#   fast8 = (taps - 1) % 128 == 0 && rows2 && out_start % 2 == 0 && x, y 8-byte aligned      -> fir.pair / fir.pair2k (8-byte accesses)
#   use32 = K == 1024 && (taps - 1) % 32 == 0 && !fast8                                      -> fir.wave32 (4-byte accesses)
#   fir.r2k needs rows4 and 16-byte aligned x, y; the 2048-point blocks have no 4-byte kernel: without rows2 every block pair runs
#   on the bounds-checked fir.pair2k.edge
_PAIR, _W32 = "fir.pair+fir.pair.edge", "fir.wave32+fir.pair.edge"
_R2K, _P2K, _E2K = "fir.r2k+fir.pair2k.edge", "fir.pair2k+fir.pair2k.edge", "fir.pair2k.edge"
_ODD_TO = lambda rec: {1: rec, 3: rec, 37: rec}       # noqa: E731
_QUAD = lambda s, j: f"{s}.quad{j}+{s}.quad{j}.edge"   # noqa: E731  (the ragged last unit of a row and the units short of slack: the edge kernel)
RECORDS = {
    "stft1024": ("stft.pair.1r", {}),
    "stft1024-many-rounds": ("stft.pair+stft.pair.h4", {}),
    "stft1024-reflect": ("stft.pair.1r+stft.pair.1r.edge", {}),
    "stft512": (_QUAD("stft", 2), {}),
    "stft400-in-512": (_QUAD("stft", 2), {}),
    "stft256": (_QUAD("stft", 4), {}),
    "stft128": (_QUAD("stft", 8), {}),
    "stft2048": ("stft.real2x", {}),
    "stft4096": ("stft.real2x.4k", {}),
    "stft8192": ("stft.8k", {}),
    "stft400": ("stft.r20", {}),
    "stft320": ("stft.rab", {}),
    "stft882": ("stft.rab", {}),
    "stft441-odd": ("stft.rab", {}),
    "stft443": ("stft.blue", {}),
    "stft16": ("stft.generic.pow2", {}),
    "stft2310": ("stft.generic.blue", {}),
    "stft-c64-512": ("stft_c64.rab", {}),
    "stft-c64-2048": ("stft_c64.rows", {}),
    "stft-f64-512": ("", {}),
    "stft-c128-512": ("stft.f64.c128", {}),
    "as_windowed": ("as_windowed.v4", {}),
    "as_windowed-f64": ("", {}),
    "fir257-slice": (_W32, {}),                       # out_start 101: the grid phase 101 % 32 leaves x off an 8-byte boundary -> !fast8 at every d
    "fir257-f64:same": ("", {}),
    "fir257-f64-slice": ("", {}),
    "onesided1024": ("mag.pair", {}), "packed1024": ("mag.pair", {}), "mag1024": ("mag.pair", {}), "dbfs1024": ("mag.pair", {}),
    "mel1024": ("mel.pair", {}),
    "onesided512": (_QUAD("mag", 2), {}), "packed512": (_QUAD("stft", 2), {}), "mag512": (_QUAD("mag", 2), {}), "dbfs512": (_QUAD("mag", 2), {}),
    "mel512": (_QUAD("mel", 2), {}),
    # 257 taps, (taps - 1) % 128 == 0: an odd d fails rows2 -> the 4-byte kernel
    "fir257:full": (_PAIR, _ODD_TO(_W32)), "fir257:same": (_PAIR, _ODD_TO(_W32)), "fir257:valid": (_PAIR, _ODD_TO(_W32)),
    # 100 taps run as 129.  :full has out_len = length + 99: the DENSE stride fails rows2 ((9003 - 9102) % 2 != 0) and an odd d meets it;
    # :same / :valid start at out_start 49 / 99, whose grid phase (17 / 3) leaves x off an 8-byte boundary at every d
    "fir100:full": (_W32, _ODD_TO(_PAIR)), "fir100:same": (_W32, {}), "fir100:valid": (_W32, {}),
    # 513 / 1025 taps, 2048-point blocks: d = 2 keeps rows2 but not rows4 -> fir.pair2k; an odd d fails rows2 -> bounds-checked blocks only
    **{f"fir{t}:{m}": (_R2K, {2: _P2K, **_ODD_TO(_E2K)}) for t in (513, 1025) for m in ("full", "same", "valid")},
    **{f"fir4097:{m}": ("fir.dline+fir.dline.fused", {}) for m in ("full", "same", "valid")},
    **{f"fir40001:{m}": ("fir.long+fft.tiled+fftconvolve_nd", {}) for m in ("full", "same", "valid")},
}
assert set(RECORDS) == set(KEYS)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _d(case, d):
    return 256 // min(256, case.in_dtype.itemsize) if d == "D256" else d


class _Tuned:
    def __init__(self, ctx, case):
        self.ctx, self.t = ctx, case.tuning

    def __enter__(self):
        for k, v in self.t.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.t:
            self.ctx.clear_tuning(k)


_cache = {}


def _inputs(key):
    """(case, rows, oracle tuple) of a key: computed once and shared, never modified"""
    if ("in", key) not in _cache:
        case = families()[key]
        x = case.data()
        x.setflags(write=False)
        _cache[("in", key)] = (case, x, case.oracle(x))
    return _cache[("in", key)]


def _dense(ctx, key):
    """the dense device call of a key into a plain buffer: (result, dispatch record)"""
    if ("dense", key) not in _cache:
        case, x, _ = _inputs(key)
        xd = ctx.to_device(x)
        out = ctx.empty((case.B, case.out_len), case.out_dtype)
        with _Tuned(ctx, case):
            rec = E.call(ctx, case.invoke, C.c_void_p(xd.ptr), case.L, C.c_void_p(out.ptr), _lib.DEVICE)
        _cache[("dense", key)] = (out.numpy(), rec)
    return _cache[("dense", key)]


def _run(ctx, case, x, d, offset=0, mem=_lib.DEVICE):
    """one call through the arenas: (input arena, its image after the call, result arena, its image after the call, record)"""
    xin = E.Arena("x", case.in_dtype, case.B, case.L, case.L + d, offset_elems=offset, data=x)
    out = E.Arena("out", case.out_dtype, case.B, case.out_len)
    if mem == _lib.DEVICE:
        xin.upload(ctx), out.upload(ctx)
        with _Tuned(ctx, case):
            rec = E.call(ctx, case.invoke, xin.ptr, case.L + d, out.ptr, mem)
        return xin, xin.download(), out, out.download(), rec
    ximg, oimg = xin.image.copy(), out.image.copy()         # host memory: the arenas' images themselves
    with _Tuned(ctx, case):
        rec = E.call(ctx, case.invoke, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), case.L + d,
                     C.c_void_p(oimg.ctypes.data + out.offset_bytes), mem)
    return xin, ximg, out, oimg, rec


def _want(key, d):
    dense, other = RECORDS[key]
    return other.get(d, dense)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("key", KEYS)
def test_strided_rows(ctx, key, d):
    case, x, (ref, tol, absolute, where) = _inputs(key)
    xin, ximg, out, oimg, rec = _run(ctx, case, x, _d(case, d))
    if d == "D256":
        dense, dense_rec = _dense(ctx, key)
        # every row keeps the dense call's alignment: the same kernels on the same bits
        E.verify([(xin, ximg)], out, oimg, expected=ref, same_bits_as=dense, unit=case.unit)
        if PROBE:
            print(f'\nPROBE    "{key}" dense "{dense_rec}" D256 "{rec}"')
            return
        assert dense_rec == rec == _want(key, "dense"), (key, dense_rec, rec)
        assert rec == case.family or (case.family and rec.startswith(case.family + "+")), (key, rec, case.family)
        return
    E.verify([(xin, ximg)], out, oimg, expected=ref, tol=tol, absolute=absolute, where=where, unit=case.unit)
    if PROBE:
        print(f'\nPROBE    "{key}" {d} "{rec}"')
        return
    assert rec == _want(key, d), f"{key}, d = {d}: dispatched to [{rec}], pinned [{_want(key, d)}]"


def _with_nans(case, x):
    xn = x.copy()
    if case.B >= 4:
        xn[1, -1] = np.nan      # the last sample of row 1: the element in front of row 1's gap
        xn[3, 0] = np.nan       # the first sample of row 3: the element behind row 2's gap
    else:
        xn[case.B - 1, -1] = np.nan
        xn[case.B - 1, 0] = np.nan if case.B == 1 else xn[case.B - 1, 0]
    return xn


@pytest.mark.parametrize("key", KEYS)
def test_a_nan_next_to_a_gap_stays_where_the_reference_has_it(ctx, key):
    """d = 3, a real NaN in the last sample of row 1 and the first sample of row 3 (families of fewer rows: in their last row).  stft: the
    finite mask of the oracle, frame by frame; fir: exactly the rows that hold a NaN are non-finite, from end to end."""
    case, x, _ = _inputs(key)
    xn = _with_nans(case, x)
    ref, tol, absolute, where = case.oracle(xn)
    if where is not None:
        where = where & np.isfinite(ref)
    xin, ximg, out, oimg, _ = _run(ctx, case, xn, 3)
    E.verify([(xin, ximg)], out, oimg, expected=ref, tol=tol, absolute=absolute, where=where, unit=case.unit, by_frame=not isinstance(case, Fir))
    if isinstance(case, Fir):
        bad = ~np.isfinite(out.tensor(oimg)).all(axis=1)
        none = ~np.isfinite(out.tensor(oimg)).any(axis=1)
        want = ~np.isfinite(xn).all(axis=1)
        assert np.array_equal(bad, want) and np.array_equal(bad, none), (key, np.flatnonzero(bad), np.flatnonzero(want))


# one key per entry point that takes a row stride
HOST_KEYS = ["stft512", "stft-c64-512", "stft-f64-512", "stft-c128-512", "onesided1024", "packed512", "mag1024", "dbfs512", "mel1024", "mel512",
             "as_windowed", "as_windowed-f64", "fir257:same", "fir257-slice", "fir257-f64:same", "fir257-f64-slice", "stft1024", "stft441-odd",
             "fir1025:full", "fir4097:valid"]


@pytest.mark.parametrize("key", HOST_KEYS)
def test_host_rows_with_nan_gaps_give_the_device_call_s_bits(ctx, key):
    """NXSIG_HOST uploads (batch - 1) * batch_stride + length elements: a strided numpy array whose gaps hold NaN, d = 3"""
    case, x, (ref, _, _, _) = _inputs(key)
    _, _, out, oimg, _ = _run(ctx, case, x, 3)
    xin, ximg, hout, himg, _ = _run(ctx, case, x, 3, mem=_lib.HOST)
    E.verify([(xin, ximg)], hout, himg, expected=ref, same_bits_as=out.tensor(oimg), unit=case.unit)


SLICED = ["stft1024", "stft512", "stft2048", "stft320", "fir257:same", "fir513:same"]


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("key", SLICED)
def test_sliced_tensors(ctx, key, offset, d):
    """a tensor that starts 1 .. 3 elements off the 16-byte boundary (a slice of a larger device tensor), dense and with d = 1"""
    case, x, (ref, tol, absolute, where) = _inputs(key)
    xin, ximg, out, oimg, _ = _run(ctx, case, x, d, offset=offset)
    E.verify([(xin, ximg)], out, oimg, expected=ref, tol=tol, absolute=absolute, where=where, unit=case.unit)


# ------------------------------------------------------------------------------- the sharded entry points
SHARDED = {"stft": "stft1024", "fir": "fir257:same", "mel": "mel1024"}


def _sharded_call(group, what, case, xs, stride, outs, mem):
    lib = _lib.load()
    n = group.local_count
    xp = (C.c_void_p * n)(*xs)
    op = (C.c_void_p * n)(*outs)
    if what == "fir":
        return lib.nxsig_fir_sharded_f32(group.handle, xp, case.L, case.B, stride, _vp(case.h), case.taps, MODES[case.mode], _lib.SHARD_CHANNELS, 0, op, mem)
    p = _lib.StftParams(case.N, case.hop, case.K, VALID, 0, 0, _lib.SCALE_NONE, 0, FS)
    if what == "mel":
        return lib.nxsig_stft_mel_sharded_f32(group.handle, xp, case.L, case.B, stride, _vp(case.window), C.byref(p), MEL_BINS, _vp(case.filters),
                                              _lib.SHARD_CHANNELS, op, None, mem)
    return lib.nxsig_stft_sharded_f32(group.handle, xp, case.L, case.B, stride, _vp(case.window), C.byref(p), _lib.SHARD_CHANNELS, 0, op, mem)


def _unsharded(ctx, what, case, x, d, bounds):
    """the bits a sharded call must reproduce: the unsharded call at the same stride (d = None: the host form).  Two legitimate
    differences, both FIR's:
    * the tuned FIR kernels shift every row's block grid by its row index IN THE CALL (kernels_wave.hip, FirWaveArgs::row_mod /
      fir_row_shift(a.row_mod, rw)): row 3 of the tensor is row 0 of the second member, its blocks start elsewhere and round
      differently.  The reference is therefore the unsharded call on each member's rows alone.
    * the sharded HOST call uploads every row of a member's part densely (group.cpp, run_sharded: `din[i] + row * p.in_len` <- `xh +
      (p.row0 + row) * batch_stride + p.in0`): its kernels see dense rows (fir.pair), the unsharded call at stride length + 3 takes
      fir.wave32 (launch_fir_wave_W: rows2 declines the 8-byte kernel).  The host reference is the call on dense rows."""
    if what != "fir":
        _, _, out, oimg, _ = _run(ctx, case, x, 3)
        return out.tensor(oimg)
    parts = []
    for c0, c1 in bounds:
        _, _, out, oimg, _ = _run(ctx, Fir(case.family, case.taps, case.mode, rows=c1 - c0), x[c0:c1], 0 if d is None else d)
        parts.append(out.tensor(oimg))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def group():
    from nx_signal_amd import sharding
    g = sharding.Group.local(2, devices=[0, 0])
    yield g
    g.close()


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("what", list(SHARDED))
def test_sharded_calls_take_the_row_stride(ctx, group, what, mem):
    """two members on one GPU, the channels axis, 5 rows batch_stride = length + 3 apart: the bits of the unsharded call at that stride;
    0 < batch_stride < length is NXSIG_ERR_INVALID_ARG"""
    from nx_signal_amd import sharding
    case = families()[SHARDED[what]]
    if what == "fir":
        case = Fir(case.family, case.taps, case.mode, rows=5)
    x = case.data()
    ref = case.oracle(x)[0]
    d = 3
    bounds = [sharding.shard_channels(case.B, group.world, r) for r in group.ranks]
    want = _unsharded(ctx, what, case, x, d if mem == "device" else None, bounds)
    if mem == "device":
        ins = [E.Arena(f"x{i}", case.in_dtype, c1 - c0, case.L, case.L + d, data=x[c0:c1]).upload(c) for i, ((c0, c1), c) in enumerate(zip(bounds, group.contexts))]
        outs = [E.Arena(f"out{i}", case.out_dtype, c1 - c0, case.out_len).upload(c) for i, ((c0, c1), c) in enumerate(zip(bounds, group.contexts))]
        _lib.check(_sharded_call(group, what, case, [a.ptr for a in ins], case.L + d, [o.ptr for o in outs], _lib.DEVICE))
        group.sync()
        for (c0, c1), a, o in zip(bounds, ins, outs):
            E.verify([(a, a.download())], o, o.download(), expected=ref[c0:c1], same_bits_as=want[c0:c1], unit=case.unit)
        assert _sharded_call(group, what, case, [a.ptr for a in ins], case.L - 1, [o.ptr for o in outs], _lib.DEVICE) == _lib.ERR_INVALID_ARG
        return
    xin = E.Arena("x", case.in_dtype, case.B, case.L, case.L + d, data=x)
    out = E.Arena("out", case.out_dtype, case.B, case.out_len)
    ximg, oimg = xin.image.copy(), out.image.copy()
    null = [C.c_void_p(0)] * (group.local_count - 1)
    xs, os_ = [C.c_void_p(ximg.ctypes.data + xin.offset_bytes)] + null, [C.c_void_p(oimg.ctypes.data + out.offset_bytes)] + null
    _lib.check(_sharded_call(group, what, case, xs, case.L + d, os_, _lib.HOST))
    group.sync()
    E.verify([(xin, ximg)], out, oimg, expected=ref, same_bits_as=want, unit=case.unit)
    assert _sharded_call(group, what, case, xs, case.L - 1, os_, _lib.HOST) == _lib.ERR_INVALID_ARG
