"""Where does a call write, and what does it leave alone?  Dense inputs, every kernel family of tests/test_gpu_dispatch_table.py.

The kernels store by 16-byte streaming stores, per-row shifted grids (the FIR grid moves by up to 31 samples per row), run seams and edge
fix-ups patched by separate launches; a store a few floats past a result lands in the allocator's slack or a neighbouring tensor and
every parity test still passes.  Here the result lies in an arena of tests/extents.py — 4 KB of a NaN pattern on either side, the
result itself pre-filled with it — and so does every input.  Every case asserts

* both guards of the result intact, no result element left unwritten,
* the result bit-identical to the same call into a plain nxsig_alloc buffer,
* the input arenas bit-identical to what was uploaded,
* the dispatch record pinned in RECORDS, led by the family the geometry is documented for.

Geometries end in the middle of whatever the kernel stores by: odd frame counts (7, 15, 17, 45), 2 or 3 rows, 37 FIR rows of 9003 samples
(every row phase) in the three modes.  Five families run again with the result 8 bytes (2 floats: one c64 element, two f32 elements) off
its 16-byte boundary: guards, and the values against the oracle at 1e-5 — a launcher may route such a result elsewhere.

NXSIG_DISPATCH_PROBE=1 prints the records instead of asserting them (how RECORDS was filled)."""
import ctypes as C
import os

import numpy as np
import pytest

import extents as E
import nx_signal_amd as S
import test_gpu_strided_rows as R
from nx_signal_amd import _lib
from oracle import nx_oracle as O

pytestmark = pytest.mark.gpu
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"
TOL_MAX = 1e-5
_vp = R._vp


class Forward:
    """a case of tests/test_gpu_strided_rows.py (one input tensor x, rows dense)"""

    def __init__(self, case):
        self.case, self.family, self.tuning = case, case.family, case.tuning
        self.B, self.out_len, self.out_dtype, self.unit = case.B, case.out_len, case.out_dtype, case.unit

    def inputs(self):
        return [("x", self.case.in_dtype, self.case.B, self.case.L, self.case.data())]

    def invoke(self, handle, ptrs, outptr):
        return self.case.invoke(handle, ptrs[0], self.case.L, outptr, _lib.DEVICE)

    def oracle(self, data):
        return self.case.oracle(data[0])[0]


class Istft:
    """nxsig_istft_c64 / _filtered_c64 / _packed_f32 / _masked_c64: z [B][M][K] -> y [B][M hop + N - hop]"""

    def __init__(self, family, N, hop, M, rows=2, kind="plain"):
        self.family, self.N, self.hop, self.M, self.B, self.kind, self.tuning = family, N, hop, M, rows, kind, {}
        self.out_len, self.unit = M * hop + N - hop, 1
        self.out_dtype = np.dtype(np.float32 if kind == "packed" else np.complex64)
        self.window = S.windows.hann(N)
        self.h = (np.random.Generator(np.random.PCG64(N)).standard_normal(2 * N).astype(np.float32).view(np.complex64)) if kind == "filtered" else None

    def inputs(self):
        rng = np.random.Generator(np.random.PCG64(self.N + self.hop))
        Kz = self.N // 2 if self.kind == "packed" else self.N
        z = rng.standard_normal((self.B, self.M * Kz * 2), dtype=np.float32).view(np.complex64)
        ins = [("z", np.complex64, self.B, self.M * Kz, z)]
        if self.kind == "mask-real":
            ins.append(("mask", np.float32, self.B, self.M * self.N, rng.random((self.B, self.M * self.N), dtype=np.float32)))
        if self.kind == "mask-onesided":
            ins.append(("mask", np.float32, self.B, self.M * (self.N // 2 + 1), rng.random((self.B, self.M * (self.N // 2 + 1)), dtype=np.float32)))
        if self.kind == "mask-complex":
            ins.append(("mask", np.complex64, self.B, self.M * self.N, rng.standard_normal((self.B, self.M * self.N * 2), dtype=np.float32).view(np.complex64)))
        return ins

    def invoke(self, handle, ptrs, outptr):
        lib = _lib.load()
        p = _lib.StftParams(self.N, self.hop, self.N, 0, 0, 0, 0, 0, 48000.0)
        w = _vp(self.window)
        if self.kind == "filtered":
            return lib.nxsig_istft_filtered_c64(handle, ptrs[0], self.M, self.B, w, C.byref(p), _vp(self.h), outptr, _lib.DEVICE)
        if self.kind == "packed":
            return lib.nxsig_istft_packed_f32(handle, ptrs[0], self.M, self.B, w, C.byref(p), outptr, _lib.DEVICE)
        if self.kind.startswith("mask"):
            mk = {"mask-real": 0, "mask-onesided": 1, "mask-complex": 2}[self.kind]      # nxsig_mask_kind
            return lib.nxsig_istft_masked_c64(handle, ptrs[0], self.B, self.M, w, C.byref(p), ptrs[1], mk, self.B, outptr, _lib.DEVICE)
        return lib.nxsig_istft_c64(handle, ptrs[0], self.M, self.B, w, C.byref(p), outptr, _lib.DEVICE)

    def oracle(self, data):
        assert self.kind == "plain"
        return O.istft(data[0].reshape(self.B, self.M, self.N), self.window, overlap_length=self.N - self.hop, fft_length=self.N)


class Fft:
    def __init__(self, family, K, rows):
        self.family, self.K, self.B, self.tuning = family, K, rows, {}
        self.out_len, self.unit, self.out_dtype = K, 1, np.dtype(np.complex64)

    def inputs(self):
        a = np.random.Generator(np.random.PCG64(self.K)).standard_normal((self.B, 2 * self.K), dtype=np.float32).view(np.complex64)
        return [("in", np.complex64, self.B, self.K, a)]

    def invoke(self, handle, ptrs, outptr):
        return _lib.load().nxsig_fft(handle, ptrs[0], 0, self.B, self.K, self.K, 0, outptr, _lib.DEVICE)


def _cases():
    F, St, Fi = Forward, R.Stft, R.Fir
    t = {
        # ---- stft: 3 rows, 17 frames (7 from fft_length 2048 on)
        "stft1024": F(St("stft.pair.1r", 1024, 256, 1024, rows=3, frames=17)),
        "stft1024-many-rounds": F(St("stft.pair", 1024, 256, 1024, rows=3, frames=45, tuning={"WAVE_SMALL_W": 0})),
        "stft1024-reflect": F(St("stft.pair.1r+stft.pair.1r.edge", 1024, 256, 1024, pad=R.REFLECT, rows=2, frames=15)),
        "stft512": F(St("stft.quad2", 512, 128, 512, rows=3, frames=17)),
        "stft400-in-512": F(St("stft.quad2", 400, 160, 512, rows=3, frames=17)),
        "stft256": F(St("stft.quad4", 256, 64, 256, rows=3, frames=45)),
        "stft128": F(St("stft.quad8", 128, 32, 128, rows=3, frames=45)),
        "stft2048": F(St("stft.real2x", 2048, 512, 2048, rows=3, frames=7)),
        "stft4096": F(St("stft.real2x.4k", 4096, 1024, 4096, rows=3, frames=7)),
        "stft8192": F(St("stft.8k", 8192, 2048, 8192, rows=2, frames=7)),
        "stft400": F(St("stft.r20", 400, 160, 400, rows=3, frames=17)),
        "stft320": F(St("stft.rab", 320, 80, 320, rows=3, frames=17)),
        "stft882": F(St("stft.rab", 882, 220, 882, rows=3, frames=15)),
        "stft441-odd": F(St("stft.rab", 441, 110, 441, rows=3, frames=17)),
        "stft2205-odd": F(St("stft.rab", 2205, 441, 2205, rows=2, frames=7)),
        "stft443": F(St("stft.blue", 443, 110, 443, rows=3, frames=17)),
        "stft16": F(St("stft.generic.pow2", 16, 4, 16, rows=3, frames=17)),
        "stft2310": F(St("stft.generic.blue", 2310, 577, 2310, rows=2, frames=7)),
        "stft-c64-512": F(St("stft_c64.rab", 512, 128, 512, "c64", rows=3, frames=17)),
        "stft-c64-2048": F(St("stft_c64.rows", 2048, 512, 2048, "c64", rows=3, frames=7)),
        # ---- istft (3.2)
        "istft1024": Istft("istft.wave.deep", 1024, 256, 45),
        "istft1024-filtered": Istft("istft.wave.filt", 1024, 256, 17, kind="filtered"),
        "istft512": Istft("istft.half.deep", 512, 128, 45, rows=3),
        "istft256": Istft("istft.quad", 256, 64, 45, rows=3),
        "istft2048": Istft("istft.dbl", 2048, 512, 15),
        "istft4096": Istft("istft.4k", 4096, 1024, 7),
        "istft400": Istft("istft.r20", 400, 160, 17, rows=3),
        "istft960": Istft("istft.rab", 960, 240, 17, rows=3),
        "istft512-hop160": Istft("istft.rab", 512, 160, 17, rows=3),
        "istft441-odd": Istft("istft.rab", 441, 110, 45, rows=3),
        "istft2205-odd": Istft("istft.rab", 2205, 441, 15),        # (the A x B kernel needs M >= 2 ceil(N / hop) - 1 = 9 frames, wave_rab.hpp: launch_istft_rab_AB)
        "istft1600-quarter-hop": Istft("istft.rab.q", 1600, 400, 15),
        "istft443-generic": Istft("fft.rows_generic.blue+istft.generic", 443, 110, 17, rows=3),
        "istft-packed1024": Istft("istft.packed", 1024, 256, 17, kind="packed"),
        "istft-masked1024-real": Istft("istft.wave.mask", 1024, 256, 17, kind="mask-real"),
        "istft-masked1024-onesided": Istft("istft.wave.mask", 1024, 256, 17, kind="mask-onesided"),
        "istft-masked1024-complex": Istft("istft.wave.mask", 1024, 256, 17, kind="mask-complex"),
        # ---- Nx.fft rows
        "fft1024": Fft("fft.rows_wave", 1024, 5),
        "fft4096": Fft("fft.rows_wave", 4096, 3),
        "fft1000": Fft("fft.rows_generic.blue", 1000, 5),
        "fft-2^16": Fft("fft.tiled", 1 << 16, 2),
        # ---- fir: the delay-line and one-transform families (the tuned ones below)
        "fir4097:same": F(Fi("fir.dline", 4097, "same", rows=3, L=20011)),
        "fir4097:full": F(Fi("fir.dline", 4097, "full", rows=3, L=20011)),
        "fir4097:valid": F(Fi("fir.dline", 4097, "valid", rows=3, L=20011)),
        "fir40001:same": F(Fi("fir.long", 40001, "same", rows=1, L=70001)),
    }
    for taps, fam in ((100, "fir.wave32"), (257, "fir.pair"), (513, "fir.r2k"), (1025, "fir.r2k")):    # 37 rows of 9003: every row phase
        for m in R.MODES:
            t[f"fir{taps}:{m}"] = F(Fi(fam, taps, m))
    return t


KEYS = ["stft1024", "stft1024-many-rounds", "stft1024-reflect", "stft512", "stft400-in-512", "stft256", "stft128", "stft2048", "stft4096", "stft8192",
        "stft400", "stft320", "stft882", "stft441-odd", "stft2205-odd", "stft443", "stft16", "stft2310", "stft-c64-512", "stft-c64-2048",
        "istft1024", "istft1024-filtered", "istft512", "istft256", "istft2048", "istft4096", "istft400", "istft960", "istft512-hop160", "istft441-odd",
        "istft2205-odd", "istft1600-quarter-hop", "istft443-generic", "istft-packed1024", "istft-masked1024-real", "istft-masked1024-onesided",
        "istft-masked1024-complex", "fft1024", "fft4096", "fft1000", "fft-2^16", "fir4097:same", "fir4097:full", "fir4097:valid", "fir40001:same"] + \
       [f"fir{t}:{m}" for t in (100, 257, 513, 1025) for m in R.MODES]
OFFSET_KEYS = ["stft1024", "stft441-odd", "istft1024", "istft441-odd", "fir257:same"]

# key -> dispatch record; filled from a probe run (NXSIG_DISPATCH_PROBE=1)
_QUAD = R._QUAD
_CH, _FIX = "+istft.edge_chunks", "+istft.edge_fix"
RECORDS = {
    "stft1024": "stft.pair.1r", "stft1024-many-rounds": "stft.pair+stft.pair.h4", "stft1024-reflect": "stft.pair.1r+stft.pair.1r.edge",
    "stft512": _QUAD("stft", 2), "stft400-in-512": _QUAD("stft", 2), "stft256": _QUAD("stft", 4), "stft128": _QUAD("stft", 8),
    "stft2048": "stft.real2x", "stft4096": "stft.real2x.4k", "stft8192": "stft.8k", "stft400": "stft.r20", "stft320": "stft.rab",
    "stft882": "stft.rab", "stft441-odd": "stft.rab", "stft2205-odd": "stft.rab", "stft443": "stft.blue", "stft16": "stft.generic.pow2",
    "stft2310": "stft.generic.blue", "stft-c64-512": "stft_c64.rab", "stft-c64-2048": "stft_c64.rows",
    "istft1024": "istft.wave.deep" + _CH, "istft1024-filtered": "istft.wave.filt" + _CH, "istft512": "istft.half.deep" + _CH + _FIX,
    "istft256": "istft.quad" + _CH + _FIX, "istft2048": "istft.dbl" + _CH, "istft4096": "istft.4k" + _FIX, "istft400": "istft.r20" + _CH,
    "istft960": "istft.rab" + _CH, "istft512-hop160": "istft.rab" + _CH, "istft441-odd": "istft.rab" + _FIX, "istft2205-odd": "istft.rab" + _FIX,
    "istft1600-quarter-hop": "istft.rab.q" + _CH, "istft443-generic": "fft.rows_generic.blue+istft.generic" + _FIX,
    "istft-packed1024": "istft.packed" + _CH + _FIX, "istft-masked1024-real": "istft.wave.mask" + _CH,
    "istft-masked1024-onesided": "istft.wave.mask" + _CH, "istft-masked1024-complex": "istft.wave.mask" + _CH,
    "fft1024": "fft.rows_wave", "fft4096": "fft.rows_wave", "fft1000": "fft.rows_generic.blue", "fft-2^16": "fft.tiled",
    **{f"fir4097:{m}": "fir.dline+fir.dline.fused" for m in R.MODES}, "fir40001:same": "fir.long+fft.tiled+fftconvolve_nd",
    **{f"fir100:{m}": R._W32 for m in R.MODES}, **{f"fir257:{m}": R._PAIR for m in R.MODES},
    **{f"fir{t}:{m}": R._R2K for t in (513, 1025) for m in R.MODES},
}
assert set(RECORDS) == set(KEYS)

_cache = {}


def _case(key):
    if not _cache:
        _cache.update(_cases())
        assert list(_cache) == KEYS
    return _cache[key]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _run(ctx, case, offset_bytes=0):
    ins = [E.Arena(name, dt, rows, n, data=data).upload(ctx) for name, dt, rows, n, data in case.inputs()]
    out = E.Arena("out", case.out_dtype, case.B, case.out_len, offset_elems=offset_bytes // case.out_dtype.itemsize).upload(ctx)
    with R._Tuned(ctx, case):
        rec = E.call(ctx, case.invoke, [a.ptr for a in ins], out.ptr)
    return ins, [(a, a.download()) for a in ins], out, out.download(), rec


@pytest.mark.parametrize("key", KEYS)
def test_a_call_writes_its_result_and_nothing_else(ctx, key):
    case = _case(key)
    ins, after, out, oimg, rec = _run(ctx, case)
    plain = ctx.empty((case.B, case.out_len), case.out_dtype)
    xs = [ctx.to_device(a.tensor()) for a in ins]
    with R._Tuned(ctx, case):
        rec_plain = E.call(ctx, case.invoke, [C.c_void_p(x.ptr) for x in xs], C.c_void_p(plain.ptr))
    want = plain.numpy()
    assert np.isfinite(want.view(np.float32)).all(), key
    E.verify(after, out, oimg, expected=want, same_bits_as=want, unit=case.unit)
    if PROBE:
        print(f'\nPROBE    "{key}": "{rec}"' + ("" if rec == rec_plain else f'   PLAIN "{rec_plain}"'))
        return
    assert rec == rec_plain == RECORDS[key], (key, rec, rec_plain)
    assert rec == case.family or rec.startswith(case.family + "+"), (key, rec, case.family)


@pytest.mark.parametrize("key", OFFSET_KEYS)
def test_a_result_off_its_16_byte_boundary(ctx, key):
    """the result 8 bytes into a 16-byte group: the guards, and the values against the oracle (the family may differ from the aligned call's)"""
    case = _case(key)
    ins, after, out, oimg, rec = _run(ctx, case, offset_bytes=8)
    ref = case.oracle([a.tensor() for a in ins])
    E.verify(after, out, oimg, expected=np.asarray(ref).reshape(case.B, case.out_len), tol=TOL_MAX, unit=case.unit)
    if PROBE:
        print(f'\nPROBE-OFFSET    "{key}": "{rec}"')
