"""Transforms.cwt / Filters.fir_bank on the GPU against the f64 oracle of tests/cwt_oracle.py (the definition of include/nxsig.h through
np.convolve) run on the SAME samples.  The bar, per (row, scale): max |got - ref| <= 1e-5 max |ref|, the project's bar for a
single-precision transform (a numpy single-precision restatement of the scheme reads 1e-8 to 3e-7, tests/test_cwt_host.py).  One case
is a row of 1000 + N(0, 1): the interior of a zero-mean wavelet's output cancels there, so that case is held to
1e-5 max|x| sum|h_s|, the bound of the convolution's size.

Every run asserts its dispatch record: "cwt.wave" alone when every filter has N <= 1025, "cwt.wave+cwt.generic" followed by the row
transforms' families for a mixed bank, "cwt.generic..." without "cwt.wave" under NXSIG_CWT_WAVE=0.  Equal bits between the tiers are
not required.

Non-finite rule under test: a row that holds an Inf / NaN has no finite output element at any scale; every other row of the batch
keeps its bits.

Nothing here loads the library while pytest collects: the shapes come from csrc/cwt_plan.hpp's rule restated below (N <= 513: K = 1024,
514 <= N <= 1025: K = 2048, beyond: generic; block step K - Nmax + 1), and the reference of a (rows, bank) is formed once and shared."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import cwt_oracle as O
import extents as E
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters, transforms

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVE, GENERIC = "cwt.wave", "cwt.generic"
LENGTHS = [1, 2, 37, 511, 512, 513, 1024, 1025, 1537, 3000]
WIDTHS = [0.1, 1, 2.5, 4.5, 10]                      # N = 1, even, odd, and capped by L on the short rows
MIXED = [1, 51.3, 51.4, 102.5, 102.6]                # N = 10, 513 | 514, 1025 | 1026 on L = 5000: both wave classes and the generic one
KINDS = {"complex": 0, "real": 1, "magnitude": 2, "power": 3}
WAVELETS = {"morlet2": 0, "ricker": 1}


def klass(N):
    return "generic" if N > 1025 else (1024 if N <= 513 else 2048)


def step_of(K, Nmax):
    return K - Nmax + 1


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tuned:
    """one switch on one context for a block (None: left alone)"""

    def __init__(self, ctx, name, value):
        self.ctx, self.name, self.value = ctx, name, value

    def __enter__(self):
        if self.value is not None:
            self.ctx.set_tuning(self.name, self.value)

    def __exit__(self, *exc):
        if self.value is not None:
            self.ctx.clear_tuning(self.name)


def tier(ctx, generic):
    return Tuned(ctx, "CWT_WAVE", 0 if generic else None)


def rows_of(seed, batch, L):
    """seeded standard-normal rows, the last one a chirp from 0.001 to 0.25 cycles per sample"""
    x = np.random.Generator(np.random.PCG64(seed)).standard_normal((batch, L)).astype(np.float32)
    t = np.arange(L, dtype=np.float64)
    x[-1] = np.sin(2 * np.pi * (0.001 * t + 0.5 * (0.249 / max(L, 2)) * t * t)).astype(np.float32) if L > 1 else np.float32(0.75)
    return x


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def family(rec, supports, generic):
    classes = {klass(N) for N in supports}
    if generic or classes == {"generic"}:
        assert rec.split("+")[0] == GENERIC and WAVE not in rec.split("+"), (rec, supports, generic)
    elif "generic" in classes:
        assert rec.split("+")[:2] == [WAVE, GENERIC], (rec, supports)
    else:
        assert rec == WAVE, (rec, supports)
    return rec


_REFS = {}


def reference(key, x, wavelet, widths, w=5.0):
    """the definition on the rows x, complex128 [B, S, L], formed once per key"""
    if key not in _REFS:
        _REFS[key] = O.cwt(x, widths, wavelet, w, kind="complex")
    return _REFS[key]


def check(name, got, ref, kind, scale=None):
    """per (row, scale): max |got - ref| <= TOL max |ref| (or TOL scale[row, s]); ref is the oracle's own expression of `kind`"""
    want = O.sink(ref, kind)
    assert got.shape == want.shape and got.dtype == (np.complex64 if kind == "complex" else np.float32), (name, got.shape, got.dtype)
    assert np.isfinite(got).all(), name
    err = np.abs(got.astype(want.dtype) - want).max(axis=-1)
    top = np.abs(want).max(axis=-1) if scale is None else scale
    worst = float((err / top).max())
    print(f"cwt-accuracy {name} {kind}: {worst:.3e}")
    assert (err <= TOL * top).all(), (name, kind, worst)
    return worst


def dev(ctx, x, widths, wavelet, kind, generic=False, w=5.0):
    """one call on a device tensor: (numpy result, dispatch record)"""
    with tier(ctx, generic):
        out = transforms.cwt(ctx.to_device(x), widths, wavelet, w=w, output=kind, ctx=ctx)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert isinstance(out, S.DeviceBuffer)
    L = x.shape[-1]
    return out.numpy(), family(rec, [O.support(a, L) for a in widths], generic)


@pytest.mark.parametrize("generic", [False, True], ids=["default", "switched-off"])
@pytest.mark.parametrize("L", LENGTHS)
def test_parity_with_the_definition_on_both_tiers(ctx, L, generic):
    """every row length of the issue with the widths [0.1, 1, 2.5, 4.5, 10], both wavelets, all four kinds, two noise rows and a chirp"""
    x = rows_of(100 + L, 3, L)
    for wavelet in WAVELETS:
        ref = reference(("parity", L, wavelet), x, wavelet, WIDTHS)
        for kind in KINDS:
            got, rec = dev(ctx, x, WIDTHS, wavelet, kind, generic)
            check(f"{'generic' if generic else 'wave'} L={L} {wavelet} [{rec}]", got, ref, kind)


@pytest.mark.parametrize("generic", [False, True], ids=["default", "switched-off"])
def test_a_mixed_bank_runs_every_class_in_one_call(ctx, generic):
    """L = 5000, batch 3, widths [1, 51.3, 51.4, 102.5, 102.6]: N = 10, 513, 514, 1025, 1026, both wave classes at their boundaries and the
    generic class in one call"""
    L = 5000
    assert [O.support(a, L) for a in MIXED] == [10, 513, 514, 1025, 1026]
    assert [klass(O.support(a, L)) for a in MIXED] == [1024, 1024, 2048, 2048, "generic"]
    x = rows_of(77, 3, L)
    for wavelet, kinds in (("morlet2", ("complex", "power")), ("ricker", ("real", "magnitude"))):
        ref = reference(("mixed", wavelet), x, wavelet, MIXED)
        for kind in kinds:
            got, rec = dev(ctx, x, MIXED, wavelet, kind, generic)
            assert generic or rec.startswith(WAVE + "+" + GENERIC)
            check(f"mixed {'generic' if generic else 'default'} {wavelet} [{rec}]", got, ref, kind)


@pytest.mark.parametrize("generic", [False, True], ids=["default", "switched-off"])
def test_noise_on_an_offset_of_1000_is_held_to_the_size_of_the_convolution(ctx, generic):
    """a row of 1000 + N(0, 1): the interior of a zero-mean wavelet's output cancels, so the bound is 1e-5 max|x| sum|h_s|"""
    L = 3000
    x = (1000 + np.random.Generator(np.random.PCG64(9)).standard_normal((2, L))).astype(np.float32)
    for wavelet, widths in (("morlet2", WIDTHS), ("ricker", WIDTHS), ("morlet2", MIXED[:4])):
        ref = reference(("offset", wavelet, tuple(widths)), x, wavelet, widths)
        size = np.array([[np.abs(r).max() * np.abs(O.taps(wavelet, a, L)).sum() for a in widths] for r in x])
        for kind in ("complex", "real"):
            got, rec = dev(ctx, x, widths, wavelet, kind, generic)
            check(f"offset {'generic' if generic else 'default'} {wavelet} S={len(widths)} [{rec}]", got, ref, kind, scale=size)


@pytest.mark.parametrize("K,L,widths", [(1024, 3000, WIDTHS), (2048, 5000, [51.4, 80])], ids=["K1024", "K2048"])
def test_a_wave_that_walks_three_blocks_gives_the_bits_of_the_default_geometry(ctx, K, L, widths):
    """NXSIG_WAVE_UNITS_PER_WAVE = 3 with few enough blocks that every wave of the one workgroup walks 3 of them (the prefetched block,
    the reused LDS buffer; the heuristic gives this suite's launches one block per wave), then 2 (a ragged last workgroup)"""
    W = 4 if K == 1024 else 2
    Nmax = max(O.support(a, L) for a in widths)
    assert {klass(O.support(a, L)) for a in widths} == {K}
    units = 3 * -(-L // step_of(K, Nmax))
    assert units >= 3 * W, units    # every wave of the first workgroup walks 3 blocks
    x = rows_of(31 + K, 3, L)
    for wavelet, kind in (("morlet2", "complex"), ("ricker", "real"), ("morlet2", "power")):
        base, _ = dev(ctx, x, widths, wavelet, kind)
        check(f"default geometry K={K} {wavelet}", base, reference(("walk", K, wavelet), x, wavelet, widths), kind)
        for upw in (3, 2):
            with Tuned(ctx, "WAVE_UNITS_PER_WAVE", upw):
                got, rec = dev(ctx, x, widths, wavelet, kind)
            assert rec == WAVE and same_bits(got, base), (K, wavelet, kind, upw)


@pytest.mark.parametrize("generic", [False, True], ids=["default", "switched-off"])
def test_strided_rows_inside_poisoned_arenas(ctx, generic):
    """batch 3 with batch_stride = L + 3 through the two C entry points, the rows starting 4 bytes off a 16-byte boundary, the result at
    every 4-byte offset, inside poisoned arenas: the guards and gaps untouched, every result element written, the input unchanged"""
    lib = _lib.load()
    cwt_fn = lambda h, *a: lib.nxsig_cwt(_lib.ctx_ptr(h, _lib._ctx_iir), *a)            # noqa: E731
    bank_fn = lambda h, *a: lib.nxsig_fir_bank(_lib.ctx_ptr(h, _lib._ctx_iir), *a)      # noqa: E731
    for L, widths in [(37, WIDTHS), (1537, WIDTHS), (1301, [3, 51.4, 70])] + ([(1100, [3, 102.6])] if not generic else []):
        x = rows_of(5 * L, 3, L)
        ws = np.array(widths, np.float64)
        sup = [O.support(a, L) for a in widths]
        for wavelet, kind in (("morlet2", "complex"), ("ricker", "real"), ("morlet2", "magnitude")):
            ref = reference(("strided", L, wavelet, tuple(widths)), x, wavelet, widths)
            odt = np.complex64 if kind == "complex" else np.float32
            want = O.sink(ref, kind).astype(odt).reshape(3, -1)
            with tier(ctx, generic):
                for offset in range(4):
                    xin = E.Arena("x", np.float32, 3, L, L + 3, offset_elems=1, data=x).upload(ctx)
                    out = E.Arena("out", odt, 3, len(widths) * L, offset_elems=offset).upload(ctx)
                    rec = E.call(ctx, cwt_fn, xin.ptr, L, 3, L + 3, WAVELETS[wavelet], ws.ctypes.data_as(C.POINTER(C.c_double)), len(widths), 5.0,
                                 KINDS[kind], out.ptr, _lib.DEVICE)
                    family(rec, sup, generic)
                    E.verify([(xin, xin.download())], out, out.download(), expected=want, tol=TOL)
                    check(f"strided L={L} {wavelet} offset={offset}", out.tensor(out.download()).reshape(3, len(widths), L), ref, kind)
                # host memory: the staged copy keeps the row stride
                xin = E.Arena("x", np.float32, 3, L, L + 3, offset_elems=1, data=x)
                out = E.Arena("out", odt, 3, len(widths) * L)
                ximg, oimg = xin.image.copy(), out.image.copy()
                E.call(ctx, cwt_fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), L, 3, L + 3, WAVELETS[wavelet], ws.ctypes.data_as(C.POINTER(C.c_double)),
                       len(widths), 5.0, KINDS[kind], C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
                E.verify([(xin, ximg)], out, oimg, expected=want, tol=TOL)
        # the bank entry point on c64 taps: the same filters rounded to f32, the same result
        hs = [O.taps("morlet2", a, L).astype(np.complex64) for a in widths]
        flat, counts = np.ascontiguousarray(np.concatenate(hs)), np.array([len(h) for h in hs], np.int64)
        ref = reference(("strided", L, "morlet2", tuple(widths)), x, "morlet2", widths)
        with tier(ctx, generic):
            xin = E.Arena("x", np.float32, 3, L, L + 3, offset_elems=1, data=x).upload(ctx)
            out = E.Arena("out", np.float32, 3, len(widths) * L, offset_elems=3).upload(ctx)
            rec = E.call(ctx, bank_fn, xin.ptr, L, 3, L + 3, flat.ctypes.data_as(C.c_void_p), 1, counts.ctypes.data_as(C.POINTER(C.c_int64)), len(widths),
                         KINDS["power"], out.ptr, _lib.DEVICE)
            family(rec, sup, generic)
            E.verify([(xin, xin.download())], out, out.download(), expected=O.sink(ref, "power").astype(np.float32).reshape(3, -1), tol=TOL)
            check(f"strided bank L={L}", out.tensor(out.download()).reshape(3, len(widths), L), ref, "power")


@pytest.mark.parametrize("generic", [False, True], ids=["default", "switched-off"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_sample_takes_its_row_and_no_other(ctx, bad, generic):
    """3 rows, one bad sample in the middle row: no finite element at any scale there, the outer rows' bits as without it"""
    for L, widths, at in [(3000, WIDTHS, 1500), (5000, MIXED, 4999), (37, WIDTHS, 0), (1, [0.1, 3], 0)]:
        clean = rows_of(61 + L, 3, L)
        x = clean.copy()
        x[1, at] = bad
        for wavelet, kind in (("morlet2", "complex"), ("ricker", "real"), ("morlet2", "power")):
            y, _ = dev(ctx, x, widths, wavelet, kind, generic)
            finite = np.isfinite(y.real) | np.isfinite(y.imag) if kind == "complex" else np.isfinite(y)
            assert not finite[1].any() and finite[[0, 2]].all(), (L, wavelet, kind)
            again, _ = dev(ctx, clean, widths, wavelet, kind, generic)
            assert np.isfinite(again).all() and same_bits(y[[0, 2]], again[[0, 2]]), (L, wavelet, kind)


def test_bank_a_then_b_then_a_again_on_one_context():
    """the third result has the bits of the first and makes no new table request, in both tiers; host and device tensors agree"""
    c = S.Context(0)
    requests = lambda: c.get_tuning("TABLE_REQUESTS")[0]   # noqa: E731
    x = rows_of(401, 3, 5000)
    for generic in (False, True):
        first, _ = dev(c, x, MIXED, "morlet2", "complex", generic)
        other, _ = dev(c, x, [2, 60, 103], "ricker", "real", generic)
        before = requests()
        third, _ = dev(c, x, MIXED, "morlet2", "complex", generic)
        one, _ = dev(c, x[:1], MIXED, "morlet2", "complex", generic)
        assert requests() == before and same_bits(third, first) and same_bits(one, first[:1]), generic
        check(f"bank B generic={generic}", other, reference(("ctx-b",), x, "ricker", [2, 60, 103]), "real")
    host = transforms.cwt(x, MIXED, ctx=c)
    assert isinstance(host, np.ndarray) and same_bits(host, dev(c, x, MIXED, "morlet2", "complex")[0])


def test_the_python_surface(ctx):
    rng = np.random.Generator(np.random.PCG64(83))
    x = rng.standard_normal((2, 700, 3)).astype(np.float32)
    # fir_bank with real taps equals cwt with the same taps passed as a callable, bit for bit
    table = {N: rng.standard_normal(N).astype(np.float32) for N in (10, 25, 45)}
    widths = [1, 2.5, 4.5]
    rows = np.ascontiguousarray(np.moveaxis(x, 1, -1))
    for kind in KINDS:
        a = filters.fir_bank(rows, [table[10], table[25], table[45]], output=kind, ctx=ctx)
        assert ctx.last_dispatch() == WAVE
        b = transforms.cwt(rows, widths, wavelet=lambda N, a: table[N][::-1], output=kind, ctx=ctx)
        assert isinstance(a, np.ndarray) and a.shape == (2, 3, 3, 700) and same_bits(a, b), kind
        check(f"fir_bank {kind}", a.reshape(6, 3, 700), O.fir_bank(rows.reshape(6, 700), [table[10], table[25], table[45]]), kind)
    # axis= on a 3-D tensor: the axis goes last, the scales in front of it
    y = transforms.cwt(x, widths, "ricker", ctx=ctx, axis=1)
    assert y.shape == (2, 3, 3, 700) and y.dtype == np.float32 and y.flags.c_contiguous
    check("axis 1", y.reshape(6, 3, 700), O.cwt(rows.reshape(6, 700), widths, "ricker", kind="complex"), "real")
    assert transforms.cwt(x[0, :, 0], widths, ctx=ctx).dtype == np.complex64      # morlet2: complex by default
    # a complex bank, integers, one filter given as a bare array
    hs = [(rng.standard_normal(7) + 1j * rng.standard_normal(7)), rng.standard_normal(4)]
    ints = ((np.arange(64, dtype=np.int32) % 7) - 3).reshape(1, 64)
    check("integers", filters.fir_bank(ints, hs, ctx=ctx), O.fir_bank(ints, [h.astype(np.complex64) for h in hs]), "complex")
    check("one filter", filters.fir_bank(ints, table[10], output="real", ctx=ctx), O.fir_bank(ints, [table[10]]), "real")
    # device input gives device output
    d = filters.fir_bank(ctx.to_device(rows), [table[10], table[25], table[45]], output="magnitude", ctx=ctx)
    assert isinstance(d, S.DeviceBuffer) and same_bits(d.numpy(), filters.fir_bank(rows, [table[10], table[25], table[45]], output="magnitude", ctx=ctx))
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        transforms.cwt(ctx.to_device(x), widths, axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="unsupported"):
        transforms.cwt(ctx.to_device(x.astype(np.float64)), widths)


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its CWT_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_cwt.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_CWT) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.CWT_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    for name in ("nxsig_fir_bank", "nxsig_cwt"):
        rows = table[name]
        assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
        assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
        assert len(rows) == len(golden["null_ctx"][name])
