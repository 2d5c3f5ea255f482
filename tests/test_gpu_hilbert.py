"""Filters.hilbert on the GPU against the f64 oracle of tests/hilbert_oracle.py (the definition of include/nxsig.h on np.fft) run on the
SAME samples.  The error of a row is max |got - ref| / max |ref| over the row, bound 1e-5, for the analytic signal, the envelope and the
quadrature alike.  One exception that the formula forces: the quadrature of a row of one or two points is identically zero, so max |ref|
is zero (or what np.fft's rounding leaves of zero); such a row — max |Im a| below 1e-12 max |a| — is held to 1e-5 of max |a| instead.

Every run asserts its dispatch record: "hilbert.wave" alone for the fused tier, "hilbert.generic" followed by the row transforms'
families for the other.  The fused shapes run again under NXSIG_DISABLE_HILBERT_WAVE; equal bits between the tiers are not required.

Non-finite rule under test: a row that holds an Inf / NaN among the min(L, N) samples used has no finite output element; the other rows
of the batch stay in bound; a NaN beyond min(L, N) is never read."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import extents as E
import hilbert_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVE, GENERIC = "hilbert.wave", "hilbert.generic"
KIND = {"analytic": 0, "envelope": 1, "quadrature": 2}
FUSED = [(1024, None), (2048, None), (1000, 1024), (1, 1024), (1500, 1024), (2047, 2048), (3000, 2048)]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_DISABLE_HILBERT_WAVE on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_HILBERT_WAVE", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_HILBERT_WAVE")


def noise(seed, shape, offset=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(shape) + offset).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def family(rec, n_fft, generic):
    """the record names the tier first; the generic tier's row transforms follow"""
    fused = n_fft in (1024, 2048) and not generic
    assert (rec == WAVE) if fused else (rec.split("+")[0] == GENERIC and WAVE not in rec), (rec, n_fft, generic)
    return rec


def dev(ctx, x, N=None, output="analytic", generic=False):
    """hilbert on a device tensor: (numpy result, dispatch record)"""
    with Tier(ctx, generic):
        out = filters.hilbert(ctx.to_device(x), N=N, ctx=ctx, output=output)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), family(rec, x.shape[-1] if N is None else N, generic)


def row_errors(got, x, N, output):
    """per row: the error over the reference's magnitude; rows whose reference is not finite must hold no finite element"""
    ref = O.hilbert(x, N, output)
    assert got.shape == ref.shape and got.dtype == (np.complex64 if output == "analytic" else np.float32)
    got, ref = got.reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    whole = np.abs(O.hilbert(x, N, "analytic")).reshape(ref.shape).max(axis=-1)
    errs = []
    for r in range(ref.shape[0]):
        if not np.isfinite(ref[r]).all():
            assert not np.isfinite(got[r]).any(), f"row {r} holds a finite element"
            continue
        assert np.isfinite(got[r]).all(), f"row {r} holds a non-finite element"
        scale = np.abs(ref[r]).max()
        if scale <= 1e-12 * whole[r]:          # an identically zero quadrature (the module docstring)
            scale = whole[r]
        errs.append(float(np.abs(got[r].astype(ref.dtype) - ref[r]).max() / max(scale, 1e-300)))
    return errs


def check(name, got, x, N, output):
    errs = row_errors(got, x, N, output)
    worst = max(errs) if errs else 0.0
    assert worst <= TOL, (name, output, worst)
    return worst


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("batch", [1, 2, 3, 65])
def test_the_fused_shapes_on_both_tiers(ctx, batch, generic):
    """(L, N) around both fused lengths — full rows, zero padding from 1000, 1 and 2047 samples, truncation from 1500 and 3000 — at batch 1,
    2, 3 and 65, every output; (1023, 1024) at batch 3 puts the rows off a 16-byte boundary"""
    shapes = FUSED + ([(1023, 1024)] if batch == 3 else [])
    for L, N in shapes:
        x = noise(1000 * batch + L, (batch, L))
        worst = {o: check(f"L={L} N={N} batch={batch}", dev(ctx, x, N, o, generic)[0], x, N, o) for o in O.OUTPUTS}
        print(f"hilbert-accuracy {'generic' if generic else 'wave'} L={L} N={N} batch={batch}: " + " ".join(f"{o} {v:.3e}" for o, v in worst.items()))


class RowsPerWave:
    """NXSIG_WAVE_UNITS_PER_WAVE on one context for a block: the rows a wave of hilbert.wave walks (None: the launcher's heuristic, which
    gives every batch this suite can afford ONE row per wave, so the loop's second trip — the prefetched row, the reused LDS buffer —
    would never run)"""

    def __init__(self, ctx, rows):
        self.ctx, self.rows = ctx, rows

    def __enter__(self):
        if self.rows:
            self.ctx.set_tuning("WAVE_UNITS_PER_WAVE", self.rows)

    def __exit__(self, *exc):
        if self.rows:
            self.ctx.clear_tuning("WAVE_UNITS_PER_WAVE")


@pytest.mark.parametrize("rows_per_wave", [2, 4])
@pytest.mark.parametrize("shape", [(1024, None), (2048, None), (1000, 1024), (3000, 2048)], ids=lambda s: f"L{s[0]}-N{s[1]}")
def test_several_rows_per_wave_give_the_bits_of_one_row_per_wave(ctx, shape, rows_per_wave):
    """batch 65 with a wave walking 2 and 4 rows (workgroups of 8 / 16 rows at 1024 points, 4 / 8 at 2048; the last one ragged): every
    output in bound and the same uint32 words as the default geometry; then NaN and +Inf rows — one in the middle of a wave's walk with
    clean rows behind it on the same wave, one that a wave takes last, and the batch's last row — which take their own rows and leave
    every other row's bits alone"""
    L, N = shape
    x = noise(2000 + L, (65, L))
    for o in O.OUTPUTS:
        base, _ = dev(ctx, x, N, o)
        check(f"default geometry L={L} N={N}", base, x, N, o)
        with RowsPerWave(ctx, rows_per_wave):
            got, rec = dev(ctx, x, N, o)
        assert rec == WAVE and same_bits(got, base), (shape, o, rows_per_wave)
    used = min(L, N or L)
    bad_rows = [1, 10, 61, 64]
    keep = [r for r in range(65) if r not in bad_rows]
    for bad in (np.nan, np.inf):
        xb = x.copy()
        for i, r in enumerate(bad_rows):
            xb[r, (used // 5) * (i + 1)] = bad
        for o in O.OUTPUTS:
            base, _ = dev(ctx, x, N, o)
            with RowsPerWave(ctx, rows_per_wave):
                got, _ = dev(ctx, xb, N, o)
            check(f"{bad} rows, {rows_per_wave} rows per wave", got, xb, N, o)
            assert not np.isfinite(got[bad_rows]).any() and np.isfinite(got[keep]).all()
            assert same_bits(got[keep], base[keep]), (shape, o, rows_per_wave, bad)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 512, 1000, 1025, 4096, 6000])
def test_the_generic_tier_on_its_own_lengths(ctx, n):
    x = noise(7 + n, (3, n))
    worst = {o: check(f"N={n}", dev(ctx, x, None, o)[0], x, None, o) for o in O.OUTPUTS}
    print(f"hilbert-accuracy generic N={n}: " + " ".join(f"{o} {v:.3e}" for o, v in worst.items()))


def test_the_generic_tier_truncates_pads_and_takes_a_long_row(ctx):
    for L, N in ((1024, 1000), (100, 8192)):
        x = noise(L + N, (2, L))
        for o in O.OUTPUTS:
            check(f"L={L} N={N}", dev(ctx, x, N, o)[0], x, N, o)
    # one row of 2^15 points: a power of two at or above fft_tiled_min (8192), so launch_fft hands both transforms to the two-pass tiled
    # four-step of kernels_nd.hip — the record says so
    x = noise(15, (1, 1 << 15))
    for o in O.OUTPUTS:
        got, rec = dev(ctx, x, None, o)
        err = check("2^15", got, x, None, o)
        print(f"hilbert-accuracy generic N=32768 {o}: {err:.3e} [{rec}]")
    assert rec.split("+")[0] == GENERIC and "fft.tiled" in rec.split("+"), rec


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("output", O.OUTPUTS)
def test_strided_rows_inside_poisoned_arenas(ctx, generic, output):
    """batch 3 with batch_stride = L + 5 through the C entry point, rows and results 0 .. 3 elements off a 16-byte boundary, inside
    poisoned arenas: the guards and gaps untouched, every result element written, the input unchanged, the results in bound — full
    rows, zero-padded rows and truncated rows, and the generic tier's own lengths under `generic`"""
    lib = _lib.load()
    fn = lambda h, *a: lib.nxsig_hilbert_f32(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    odt = np.complex64 if output == "analytic" else np.float32
    shapes = [(1024, 1024), (1000, 1024), (1500, 1024), (2048, 2048), (2047, 2048)] + ([(1000, 1000), (777, 512), (300, 1025)] if generic else [])
    for L, N in shapes:
        x = noise(3 * L + N, (3, L))
        ref = O.hilbert(x, N, output).astype(odt)
        with Tier(ctx, generic):
            for gap, offset in ((5, 1), (5, 2), (5, 3), (0, 0)):
                xin = E.Arena("x", np.float32, 3, L, L + gap, offset_elems=offset, data=x).upload(ctx)
                out = E.Arena("out", odt, 3, N, offset_elems=(offset + 1) % 4).upload(ctx)
                rec = E.call(ctx, fn, xin.ptr, L, 3, L + gap, N, KIND[output], out.ptr, _lib.DEVICE)
                family(rec, N, generic)
                E.verify([(xin, xin.download())], out, out.download(), expected=ref, tol=TOL)
                check(f"strided L={L} N={N} gap={gap}", out.tensor(out.download()), x, N, output)
            # host memory: the staged copy keeps the row stride
            xin = E.Arena("x", np.float32, 3, L, L + 5, offset_elems=1, data=x)
            out = E.Arena("out", odt, 3, N)
            ximg, oimg = xin.image.copy(), out.image.copy()
            E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), L, 3, L + 5, N, KIND[output],
                   C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
            E.verify([(xin, ximg)], out, oimg, expected=ref, tol=TOL)


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_sample_takes_its_row_and_no_other(ctx, bad, generic):
    for L, N in [(1024, None), (2048, None), (1000, 1024), (1500, 1024)] + ([(1000, None), (6000, None), (100, 8192)] if generic else []):
        clean = noise(61 + L, (4, L))
        x = clean.copy()
        x[1, min(L, N or L) // 3] = bad
        for o in O.OUTPUTS:
            y, _ = dev(ctx, x, N, o, generic)
            check(f"{bad} in row 1, L={L} N={N}", y, x, N, o)
            assert not np.isfinite(y[1]).any() and np.isfinite(y[[0, 2, 3]]).all()
            assert same_bits(y[[0, 2, 3]], dev(ctx, clean, N, o, generic)[0][[0, 2, 3]])
    # beyond min(L, N) a NaN is not part of the row: the whole batch stays finite
    x = noise(67, (4, 1500))
    x[1, 1024:] = bad
    for o in O.OUTPUTS:
        y, _ = dev(ctx, x, 1024, o, generic)
        assert np.isfinite(y).all() and check("beyond min(L, N)", y, x, 1024, o) <= TOL


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_a_large_offset(ctx, generic):
    """1000 + N(0, 1): the quadrature is of the size of the noise, a thousandth of the samples"""
    for n in (1024, 2048) + ((1000,) if generic else ()):
        x = noise(71 + n, (3, n), offset=1000.0)
        worst = {o: check(f"offset 1000 N={n}", dev(ctx, x, None, o, generic)[0], x, None, o) for o in O.OUTPUTS}
        print(f"hilbert-accuracy offset-1000 {'generic' if generic else 'wave'} N={n}: " + " ".join(f"{o} {v:.3e}" for o, v in worst.items()))


def test_host_and_device_tensors_return_the_same_bits(ctx):
    for L, N in ((1500, 1024), (700, 1000)):
        x = noise(81 + L, (3, L))
        for o in O.OUTPUTS:
            d, _ = dev(ctx, x, N, o)
            h = filters.hilbert(x, N=N, ctx=ctx, output=o)
            family(ctx.last_dispatch(), N, False)
            assert isinstance(h, np.ndarray) and same_bits(h, d), (L, N, o)


def test_a_host_array_along_axis_0_and_integers(ctx):
    x = noise(83, (1024, 3))
    y = filters.hilbert(x, ctx=ctx, axis=0, output="envelope")
    assert isinstance(y, np.ndarray) and y.shape == (1024, 3) and y.flags.c_contiguous
    check("axis 0", np.ascontiguousarray(y.T), np.ascontiguousarray(x.T), None, "envelope")
    z = filters.hilbert(x, N=600, ctx=ctx, axis=0)
    assert z.shape == (600, 3) and check("axis 0, N=600", np.ascontiguousarray(z.T), np.ascontiguousarray(x.T), 600, "analytic") <= TOL
    ints = (np.arange(64, dtype=np.int32) % 7) - 3
    check("integers", filters.hilbert(ints, ctx=ctx), ints.astype(np.float32), None, "analytic")
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        filters.hilbert(ctx.to_device(x), axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="unsupported"):
        filters.hilbert(ctx.to_device(x.astype(np.float64)))


def test_a_repeated_call_asks_for_no_new_table():
    """the first call of a length forms the twiddle tables of its transforms; a second identical call makes no request"""
    c = S.Context(0)
    requests = lambda: c.get_tuning("TABLE_REQUESTS")[0]   # noqa: E731
    for n, generic in ((1024, False), (2048, False), (1024, True), (512, False), (1000, False)):
        x = noise(91 + n, (3, n))
        first, _ = dev(c, x, None, "analytic", generic)
        before = requests()
        again, _ = dev(c, x, None, "analytic", generic)
        assert requests() == before and same_bits(first, again), (n, generic)


def test_batch_0_launches_nothing(ctx):
    lib = _lib.load()
    x = ctx.to_device(noise(93, (1, 8)))
    out = ctx.empty((8,), np.float32)
    rc = lib.nxsig_hilbert_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(x.ptr), 8, 0, 8, 8, 1, C.c_void_p(out.ptr), _lib.DEVICE)
    assert rc == 0 and ctx.last_dispatch() == ""


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its HILBERT_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_hilbert.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_HILBERT) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.HILBERT_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_hilbert_f32"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
