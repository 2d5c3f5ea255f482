"""Convolution.correlate_rows / convolve_rows on the GPU against the f64 oracle of tests/xcorr_oracle.py (the definition of
include/nxsig.h as a direct sum in double; the PHAT weighting through np.fft in double at the contract's transform length) run on the
SAME samples.  The error of a row is max |got - ref| / max |ref| over the row, bound 1e-5: the project's bar for a single-precision
transform (the numpy single-precision restatement of the scheme reads 1e-7 on noise, tests/test_xcorr_host.py).

Every run asserts its dispatch record: "xcorr.wave" alone for the fused tier (n1 + n2 - 1 <= 1024, real pairs up to 2048),
"xcorr.generic" followed by the row transforms' families for the other.  The fused shapes run again under NXSIG_XCORR_WAVE=0; equal
bits between the tiers are not required.

Non-finite rule under test: a pair in which either row holds an Inf / NaN has no finite output element (peak sink: NaN at lag 0); every
other pair of the batch keeps its bits.

Nothing here loads the library while pytest collects, and the reference of a (shape, type, op) is formed once and shared.

profiles/xcorr/accuracy.txt is this file's own print-out: the "xcorr-accuracy" lines of `pytest tests/test_gpu_xcorr.py -m gpu -s`."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extents as E
import xcorr_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, convolution

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVE, GENERIC = "xcorr.wave", "xcorr.generic"
SHAPES = [(1, 1), (2, 1), (5, 3), (3, 5), (600, 300), (512, 513), (513, 513), (1024, 1025), (1025, 1025), (1500, 549), (3000, 70), (5000, 4000)]
BATCH = 37
MODE_ID = {"full": 0, "same": 1, "valid": 2}


def fused(n1, n2, complex_rows):
    need = n1 + n2 - 1
    return need <= 1024 or (need <= 2048 and not complex_rows)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tune:
    """a tuning key set on one context for a block (None: left alone)"""

    def __init__(self, ctx, key, value):
        self.ctx, self.key, self.value = ctx, key, value

    def __enter__(self):
        if self.value is not None:
            self.ctx.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        if self.value is not None:
            self.ctx.clear_tuning(self.key)


def Tier(ctx, generic):
    return Tune(ctx, "XCORR_WAVE", 0 if generic else None)


def noise(seed, shape, complex_rows=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(shape).astype(np.float32)
    return (x + 1j * rng.standard_normal(shape).astype(np.float32)).astype(np.complex64) if complex_rows else x


def finite_parts(y):
    """per element: some component is finite"""
    return (np.isfinite(y.real) | np.isfinite(y.imag)) if np.iscomplexobj(y) else np.isfinite(y)


def all_nan(v):
    return bool((np.isnan(v.real) & np.isnan(v.imag)).all() if np.iscomplexobj(v) else np.isnan(v).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def family(rec, n1, n2, complex_rows, generic):
    """the record names the tier first; the generic tier's row transforms follow"""
    wave = fused(n1, n2, complex_rows) and not generic
    assert (rec == WAVE) if wave else (rec.split("+")[0] == GENERIC and WAVE not in rec), (rec, n1, n2, complex_rows, generic)
    return rec


def dev(ctx, op, a, b, mode="full", generic=False, **kw):
    """one call on device tensors: (numpy result or (lags, values), dispatch record).  b may be `a` itself (autocorrelation)"""
    fn = convolution.correlate_rows if op == "correlate" else convolution.convolve_rows
    with Tier(ctx, generic):
        da = ctx.to_device(a)
        db = da if b is a else ctx.to_device(b)
        out = fn(da, db, mode, ctx=ctx, **kw)
        ctx.sync()
        rec = ctx.last_dispatch()
    family(rec, a.shape[-1], b.shape[-1], np.iscomplexobj(a), generic)
    if isinstance(out, tuple):
        assert all(isinstance(o, S.DeviceBuffer) for o in out)
        return tuple(o.numpy() for o in out), rec
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), rec


def row_errors(got, ref, scale=None):
    """per row: the error over the reference's largest magnitude (or over `scale`, one per row)"""
    assert got.shape == ref.shape and got.dtype == (np.complex64 if np.iscomplexobj(ref) else np.float32), (got.shape, ref.shape, got.dtype)
    assert np.isfinite(got).all()
    top = np.abs(ref).max(axis=-1) if scale is None else np.asarray(scale, np.float64)
    return np.abs(got.astype(ref.dtype) - ref).max(axis=-1) / top


def check(name, got, ref, scale=None):
    worst = float(row_errors(got, ref, scale).max())
    assert worst <= TOL, (name, worst)
    return worst


_INPUTS, _FULL = {}, {}


def inputs(shape, complex_rows):
    key = (shape, complex_rows)
    if key not in _INPUTS:
        n1, n2 = shape
        _INPUTS[key] = (noise(1000 + 7 * n1 + n2, (BATCH, n1), complex_rows), noise(2000 + 7 * n1 + n2, (BATCH, n2), complex_rows))
    return _INPUTS[key]


def reference(shape, complex_rows, op, mode):
    """the definition on the rows of inputs(): the full result of a (shape, type, op) is formed once, the modes are windows of it"""
    key = (shape, complex_rows, op)
    if key not in _FULL:
        a, b = inputs(shape, complex_rows)
        _FULL[key] = np.stack([O.full(a[r], b[r], op) for r in range(BATCH)])
    return O.window(_FULL[key], shape[0], shape[1], mode)


CASES = [(s, g, c) for s in SHAPES for c in (False, True) for g in (False, True) if g is False or fused(*s, c)]
CASE_IDS = [f"n{s[0]}-n{s[1]}-{'c64' if c else 'f32'}-{'switched-off' if g else 'default'}" for s, g, c in CASES]


@pytest.mark.parametrize("shape,generic,complex_rows", CASES, ids=CASE_IDS)
def test_parity_with_the_definition_on_both_tiers(ctx, shape, generic, complex_rows):
    """every shape, both ops, all three modes, at batch 37, 3 and 1 (the same pairs: a pair's bits do not depend on the batch).  The bar
    is 1e-5 of the row's maximum.  The "valid" windows at n1 = n2 or n1 = n2 - 1 with hundreds of samples — one element at (513, 513) and
    (1025, 1025), two at (512, 513) and (1024, 1025) — are sums over the whole overlap that cancel to anything between 0 and
    ||x|| ||y||, and their maximum is no scale: no single-precision sum is within 1e-5 of a value it cancelled to.  Those four windows
    are held to 1e-5 ||x||_2 ||y||_2 instead, the Cauchy-Schwarz bound of any output element (the scale of the cancelling-row test);
    "valid" keeps the row-maximum bar at every other shape, the short ones (sums of at most three products) included"""
    n1, n2 = shape
    tier = "generic" if generic or not fused(n1, n2, complex_rows) else "wave"
    a, b = inputs(shape, complex_rows)
    norms = np.linalg.norm(a.astype(np.complex128), axis=-1) * np.linalg.norm(b.astype(np.complex128), axis=-1)
    for op in O.OPS:
        for mode in O.MODES:
            ref = reference(shape, complex_rows, op, mode)
            cancelling = mode == "valid" and ref.shape[-1] <= 2 and min(n1, n2) >= 512
            whole = None
            for batch in (BATCH, 3, 1):
                got, rec = dev(ctx, op, a[:batch], b[:batch], mode, generic)
                errs = row_errors(got, ref[:batch], norms[:batch] if cancelling else None)
                print(f"xcorr-accuracy {tier} {op} {mode} {'c64' if complex_rows else 'f32'} n1={n1} n2={n2} batch={batch}: worst row {errs.max():.3e} "
                      f"median row {np.median(errs):.3e}{' of ||x|| ||y||' if cancelling else ''} [{rec}]")
                assert errs.max() <= TOL, (op, mode, batch, float(errs.max()))
                if whole is None:
                    whole = got
                assert same_bits(got, whole[:batch]), (op, mode, batch)
    if shape == (5000, 4000):
        assert any(f.startswith("fft.") for f in rec.split("+")[1:]), rec     # the long-row transforms of launch_fft


@pytest.mark.parametrize("shape,generic,complex_rows", CASES, ids=CASE_IDS)
def test_the_peak_sink_has_the_bits_of_the_rows(ctx, shape, generic, complex_rows):
    """lag and value of the fused sink against np.argmax / the value of the SAME tier's rows, bit for bit, in all three modes"""
    n1, n2 = shape
    a, b = inputs(shape, complex_rows)
    for mode in O.MODES:
        rows, _ = dev(ctx, "correlate", a, b, mode, generic)
        (lags, values), _ = dev(ctx, "correlate", a, b, mode, generic, output="peak")
        want_lags, want_values = O.peak(rows, n1, n2, mode)
        assert lags.dtype == np.int32 and lags.shape == (BATCH,) and values.shape == (BATCH,) and values.dtype == rows.dtype
        assert np.array_equal(lags, want_lags), (mode, lags[:5], want_lags[:5])
        assert same_bits(values, want_values), mode


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_a_cancelling_row_is_held_to_the_cauchy_schwarz_scale(ctx, generic):
    """ones(64) against alternating +-1: every lag is -1, 0 or +1, far below ||x|| ||y|| = 64, the bound of any output element; the
    error is held to 1e-5 of that"""
    x = np.ones((3, 64), np.float32)
    y = np.tile(np.where(np.arange(64) % 2 == 0, 1.0, -1.0).astype(np.float32), (3, 1))
    for op in O.OPS:
        for mode in O.MODES:
            got, _ = dev(ctx, op, x, y, mode, generic)
            ref = O.rows(x, y, op, mode)
            assert np.abs(ref).max() <= 1.0
            check(f"cancelling {op} {mode}", got, ref, scale=np.full(3, 64.0))


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("shape", [(1500, 549), (600, 300)], ids=lambda s: f"n{s[0]}-n{s[1]}")
def test_scale_disparity_and_zero_rows(ctx, shape, generic):
    """rows of in1 times 2^13 against rows of in2 times 2^-13 (the packed transform without its row scale fails this by decades), one
    all-zero row in each operand: the same bar, and exact zeros for the zero rows"""
    n1, n2 = shape
    for complex_rows in (False, True):
        a, b = noise(31 + n1, (6, n1), complex_rows) * np.float32(2.0 ** 13), noise(37 + n2, (6, n2), complex_rows) * np.float32(2.0 ** -13)
        a[1] = 0
        b[4] = 0
        for op in O.OPS:
            got, _ = dev(ctx, op, a, b, "full", generic)
            ref = O.rows(a, b, op, "full")
            keep = [0, 2, 3, 5]
            worst = check(f"disparity {op} {shape}", got[keep], ref[keep])
            print(f"xcorr-accuracy {'generic' if generic else 'wave'} {op} full {'c64' if complex_rows else 'f32'} n1={n1} n2={n2} scales 2^13 / 2^-13: worst row {worst:.3e}")
            assert not got[[1, 4]].any(), "a zero row gives exact zeros"


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_a_shared_template_and_the_autocorrelation(ctx, generic):
    for complex_rows in (False, True):
        for n1, n2 in [(600, 300), (1500, 400), (3000, 70)]:
            a, t = noise(41 + n1, (5, n1), complex_rows), noise(43 + n2, (n2,), complex_rows)
            tiled = np.ascontiguousarray(np.broadcast_to(t, (5, n2)))
            for op in O.OPS:
                shared, _ = dev(ctx, op, a, t, "same", generic)
                assert same_bits(shared, dev(ctx, op, a, tiled, "same", generic)[0]), (op, n1, n2)
                check(f"template {op}", shared, O.rows(a, t, op, "same"))
        x = noise(47, (5, 500), complex_rows)
        auto, _ = dev(ctx, "correlate", x, x, "full", generic)
        check("autocorrelation", auto, O.rows(x, x, "correlate", "full"))
        top = np.abs(auto).max(axis=-1)
        assert (np.abs(auto - np.conj(auto[:, ::-1])).max(axis=-1) <= TOL * top).all()          # Hermitian about lag 0
        energy = (np.abs(x.astype(np.complex128)) ** 2).sum(axis=-1)
        assert (np.abs(auto[:, 499] - energy) <= TOL * top).all()                                # lag 0 is sum |x|^2
        assert (np.argmax(np.abs(auto), axis=-1) == 499).all()


def delayed_pairs(seed, n1, n2, complex_rows, rows=16):
    """x: noise; y[j] = x[j - d] + 10 % noise (nothing but that noise where j < d), d seeded in [0, 40): in2 is in1 delayed by d, which
    SciPy's lag convention (the lag of full[k] is k - (n2 - 1)) reports as the lag -d.  The seeds in use are ones at which the f64
    oracle itself puts all sixteen rows of every case at the delay, plain and weighted (asserted where they are used): with n2 = 70 up
    to 39 of a template's samples carry no signal, and some seeds lose such a row in double already"""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.integers(0, 40, rows)
    x = noise(seed + 1, (rows, max(n1, n2)), complex_rows)
    y = np.zeros((rows, n2), x.dtype)
    for r in range(rows):
        y[r, d[r]:] = x[r, :n2 - d[r]]
    x = np.ascontiguousarray(x[:, :n1])
    y = (y + np.float32(0.1) * noise(seed + 3, (rows, n2), complex_rows)).astype(x.dtype)
    return x, y, d


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("shape", [(600, 300), (1000, 1000), (1024, 1025), (3000, 70)], ids=lambda s: f"n{s[0]}-n{s[1]}")
def test_phat_against_the_oracle_at_the_contract_length(ctx, shape, generic):
    """GCC-PHAT of a delayed copy: within 1e-5 of the row maximum of the oracle's PHAT at P = max(1024, next power of two), argmax at
    the delay on every one of the sixteen rows, and the fused peak sink reports the same lag"""
    n1, n2 = shape
    for complex_rows in (False, True):
        x, y, d = delayed_pairs(700 + n1 + n2, n1, n2, complex_rows)
        for floor in (0.0, 1e-3):
            got, rec = dev(ctx, "correlate", x, y, "full", generic, weighting="phat", phat_floor=floor)
            ref = O.phat_rows(x, y, "full", floor)
            worst = check(f"phat {shape} floor={floor}", got, ref)
            print(f"xcorr-accuracy {'generic' if generic or not fused(n1, n2, complex_rows) else 'wave'} phat floor={floor} {'c64' if complex_rows else 'f32'} "
                  f"n1={n1} n2={n2} batch=16: worst row {worst:.3e} [{rec}]")
            lags = O.lags(n1, n2, "full")
            assert np.array_equal(lags[np.argmax(np.abs(ref) if complex_rows else ref, axis=-1)], -d), "the oracle's own peak is at the delay"
            key = O.modulus32(got) if complex_rows else got
            assert np.array_equal(lags[np.argmax(key, axis=-1)], -d), (floor, lags[np.argmax(key, axis=-1)], -d)
            (plags, pvals), _ = dev(ctx, "correlate", x, y, "full", generic, weighting="phat", phat_floor=floor, output="peak")
            assert np.array_equal(plags, -d) and same_bits(pvals, O.peak(got, n1, n2, "full")[1])
        (plain, _), _ = dev(ctx, "correlate", x, y, "full", generic, output="peak")
        assert np.array_equal(plain, -d), "the unweighted peak is at the delay too"


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_phat_does_not_depend_on_the_scale_of_the_operands(ctx, generic):
    """operands of 1e12 and of 1e-12: the cross spectrum is near 1e27 / 1e-21 and its squared modulus leaves single precision, but G
    does not change with the scale, so the bar and the peak hold as they do at scale 1"""
    for complex_rows in (False, True):
        x, y, d = delayed_pairs(700 + 900, 600, 300, complex_rows)
        ref = O.phat_rows(x, y, "full", 1e-3)
        for scale in (1e12, 1e-12):
            xs, ys = x * np.float32(scale), y * np.float32(scale)
            got, _ = dev(ctx, "correlate", xs, ys, "full", generic, weighting="phat", phat_floor=1e-3)
            check(f"phat at scale {scale}", got, ref)
            (lags, _), _ = dev(ctx, "correlate", xs, ys, "full", generic, weighting="phat", phat_floor=1e-3, output="peak")
            assert np.array_equal(lags, -d), scale


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_a_pair_whose_product_overflows_is_nan_at_lag_0_under_the_peak_sink(ctx, generic):
    """c64 rows of 1e20: every bin of X conj(Y) overflows, the window is NaN throughout although no sample is; the peak sink writes NaN
    and lag 0 for that pair, as for a poisoned one, and the other pairs keep their bits"""
    a, b = noise(111, (3, 100), True), noise(112, (3, 50), True)
    (cl, cv), _ = dev(ctx, "correlate", a, b, "full", generic, output="peak")
    big_a, big_b = a.copy(), b.copy()
    big_a[1] *= np.float32(1e20)
    big_b[1] *= np.float32(1e20)
    rows, _ = dev(ctx, "correlate", big_a, big_b, "full", generic)
    assert np.isnan(rows[1].real).all() and np.isnan(rows[1].imag).all(), "the case is an all-NaN window"
    (pl, pv), _ = dev(ctx, "correlate", big_a, big_b, "full", generic, output="peak")
    assert all_nan(pv[[1]]) and pl[1] == 0
    assert np.array_equal(pl[[0, 2]], cl[[0, 2]]) and same_bits(pv[[0, 2]], cv[[0, 2]])


@pytest.mark.parametrize("rows_per_wave", [2, 4])
@pytest.mark.parametrize("shape", [(600, 300), (1500, 549)], ids=lambda s: f"n{s[0]}-n{s[1]}")
def test_several_rows_per_wave_give_the_bits_of_one_row_per_wave(ctx, shape, rows_per_wave):
    """batch 37 at P = 1024 and 2048 with a wave walking 2 and 4 pairs (the last workgroup ragged): the same uint32 words as the default
    geometry, under both sinks and with PHAT; then NaN and +Inf in either operand — in the middle of a wave's walk, at its end, in the
    batch's last pair — which take their own pairs and leave every other pair's bits alone"""
    n1, n2 = shape
    bad_rows = [1, 10, 33, 36]
    keep = [r for r in range(BATCH) if r not in bad_rows]
    for complex_rows in (False, True):
        if not fused(n1, n2, complex_rows):
            continue
        a, b = inputs(shape, complex_rows)
        for kw in ({}, {"weighting": "phat"}, {"output": "peak"}):
            base, _ = dev(ctx, "correlate", a, b, "same", **kw)
            with Tune(ctx, "WAVE_UNITS_PER_WAVE", rows_per_wave):
                got, rec = dev(ctx, "correlate", a, b, "same", **kw)
            assert rec == WAVE
            assert all(same_bits(g, w) for g, w in zip(got, base)) if isinstance(got, tuple) else same_bits(got, base), (shape, kw, rows_per_wave)
        base, _ = dev(ctx, "convolve", a, b, "full")
        for bad in (np.nan, np.inf):
            ab, bb = a.copy(), b.copy()
            for i, r in enumerate(bad_rows):
                (ab if i % 2 == 0 else bb)[r, ((n2 if i % 2 else n1) // 5) * (i + 1)] = bad
            with Tune(ctx, "WAVE_UNITS_PER_WAVE", rows_per_wave):
                got, _ = dev(ctx, "convolve", ab, bb, "full")
            finite = finite_parts(got)
            assert not finite[bad_rows].any() and np.isfinite(got[keep]).all(), (shape, rows_per_wave, bad)
            assert same_bits(got[keep], base[keep]), (shape, rows_per_wave, bad)


def test_several_slabs_give_the_bits_of_one_slab(ctx):
    """NXSIG_XCORR_SLAB_ROWS=2 on batch 5 (slabs of 2, 2 and 1 pairs): the generic tier's bits do not depend on the slab, under both sinks,
    with PHAT and with a shared template"""
    for complex_rows in (False, True):
        for n1, n2 in [(600, 300), (3000, 70)]:
            a, b = noise(71 + n1, (5, n1), complex_rows), noise(73 + n2, (5, n2), complex_rows)
            for second, kw in ((b, {}), (b, {"weighting": "phat", "phat_floor": 1e-3}), (b, {"output": "peak"}), (b[0], {})):
                one, _ = dev(ctx, "correlate", a, second, "full", True, **kw)
                with Tune(ctx, "XCORR_SLAB_ROWS", 2):
                    got, _ = dev(ctx, "correlate", a, second, "full", True, **kw)
                assert all(same_bits(g, w) for g, w in zip(got, one)) if isinstance(got, tuple) else same_bits(got, one), (n1, n2, kw)


def test_a_sequence_of_calls_on_one_context_then_the_first_again():
    """a seeded sequence of calls with different shapes, ops, modes and sinks on one context, both tiers and both types, then the first
    calls again: the same bits.  Host and device tensors give the same bits"""
    c = S.Context(0)
    rng = np.random.Generator(np.random.PCG64(5))
    a0, b0 = noise(401, (5, 700)), noise(402, (5, 300))
    first, _ = dev(c, "correlate", a0, b0, "same")
    first_generic, _ = dev(c, "correlate", a0, b0, "same", True)
    for step in range(8):
        n1, n2 = int(rng.integers(1, 3000)), int(rng.integers(1, 1500))
        cplx, generic = bool(step % 2), step % 3 == 0
        a, b = noise(500 + step, (int(rng.integers(1, 9)), n1), cplx), noise(600 + step, (1, n2), cplx)
        b = np.ascontiguousarray(np.broadcast_to(b, (a.shape[0], n2)))
        op, mode = O.OPS[step % 2], O.MODES[step % 3]
        got, _ = dev(c, op, a, b, mode, generic)
        check(f"step {step}: {op} {mode} n1={n1} n2={n2}", got, O.rows(a, b, op, mode), scale=np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    assert same_bits(dev(c, "correlate", a0, b0, "same")[0], first) and same_bits(dev(c, "correlate", a0, b0, "same", True)[0], first_generic)
    host = convolution.correlate_rows(a0, b0, "same", ctx=c)
    assert isinstance(host, np.ndarray) and same_bits(host, first)
    hl, hv = convolution.correlate_rows(a0, b0, "same", output="peak", ctx=c)
    assert hl.dtype == np.int32 and np.array_equal(hl, O.peak(first, 700, 300, "same")[0]) and same_bits(hv, O.peak(first, 700, 300, "same")[1])


def test_a_host_array_along_axis_0_and_integers(ctx):
    a, b = noise(83, (700, 3)), noise(84, (300, 3))
    y = convolution.correlate_rows(a, b, "valid", axis=0, ctx=ctx)
    assert isinstance(y, np.ndarray) and y.shape == (401, 3) and y.flags.c_contiguous and y.dtype == np.float32
    check("axis 0", np.ascontiguousarray(y.T), O.rows(np.ascontiguousarray(a.T), np.ascontiguousarray(b.T), "correlate", "valid"))
    ints = ((np.arange(64, dtype=np.int32) % 7) - 3).reshape(1, 64)
    check("integers", convolution.convolve_rows(ints, ints[0, :9], ctx=ctx), O.rows(ints, ints[0, :9], "convolve", "full"))
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        convolution.correlate_rows(ctx.to_device(a), ctx.to_device(b), axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="unsupported"):
        convolution.correlate_rows(ctx.to_device(a.astype(np.float64)), ctx.to_device(b.astype(np.float64)))


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_sample_takes_its_pair_and_no_other(ctx, bad, generic):
    for n1, n2 in [(600, 300), (1500, 549), (3, 5)] + ([(3000, 70)] if generic else []):
        for complex_rows in (False, True):
            a, b = noise(61 + n1, (5, n1), complex_rows), noise(62 + n2, (5, n2), complex_rows)
            ab, bb = a.copy(), b.copy()
            ab[1, n1 // 3] = bad
            bb[3, n2 // 2] = bad
            clean, _ = dev(ctx, "correlate", a, b, "full", generic)
            y, _ = dev(ctx, "correlate", ab, bb, "full", generic)
            finite = finite_parts(y)
            assert not finite[[1, 3]].any() and np.isfinite(y[[0, 2, 4]]).all(), (n1, n2, complex_rows)
            assert same_bits(y[[0, 2, 4]], clean[[0, 2, 4]])
            (cl, cv), _ = dev(ctx, "correlate", a, b, "full", generic, output="peak")
            (pl, pv), _ = dev(ctx, "correlate", ab, bb, "full", generic, output="peak")
            assert all_nan(pv[[1, 3]]) and (pl[[1, 3]] == 0).all(), (n1, n2, complex_rows)
            assert np.array_equal(pl[[0, 2, 4]], cl[[0, 2, 4]]) and same_bits(pv[[0, 2, 4]], cv[[0, 2, 4]])
            (wl, wv), _ = dev(ctx, "correlate", ab, bb, "full", generic, output="peak", weighting="phat")
            assert all_nan(wv[[1, 3]]) and (wl[[1, 3]] == 0).all() and np.isfinite(wv[[0, 2, 4]]).all()


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("complex_rows", [False, True], ids=["f32", "c64"])
def test_strided_rows_inside_poisoned_arenas(ctx, generic, complex_rows):
    """batch 3 with a_stride = n1 + 5 and b_stride = n2 + 3 through the C entry point, odd and even lengths, operands and results off
    their 8- / 16-byte boundaries, inside poisoned arenas: the guards and gaps untouched, every result element written, the operands
    unchanged, the results in bound; both sinks; host memory keeps the strides"""
    lib = _lib.load()
    fn = lambda h, *a: lib.nxsig_xcorr(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    dt = np.complex64 if complex_rows else np.float32
    for n1, n2 in [(601, 301), (600, 300), (1501, 547), (3, 5)] + ([(3001, 70)] if generic else []):
        a, b = noise(3 * n1 + n2, (3, n1), complex_rows), noise(5 * n1 + n2, (3, n2), complex_rows)
        for mode in ("full", "same"):
            ref = O.rows(a, b, "correlate", mode).astype(dt)
            n_out = ref.shape[-1]
            with Tier(ctx, generic):
                for gap, offset in ((5, 1), (5, 2), (0, 3), (0, 0)):
                    ain = E.Arena("a", dt, 3, n1, n1 + gap, offset_elems=offset, data=a).upload(ctx)
                    bin_ = E.Arena("b", dt, 3, n2, n2 + (3 if gap else 0), offset_elems=(offset + 2) % 4, data=b).upload(ctx)
                    out = E.Arena("out", dt, 3, n_out, offset_elems=(offset + 1) % 4).upload(ctx)
                    rec = E.call(ctx, fn, ain.ptr, n1, ain.row_stride, bin_.ptr, n2, bin_.row_stride, 3, int(complex_rows), 1, MODE_ID[mode], 0, 0.0, 0,
                                 out.ptr, None, _lib.DEVICE)
                    family(rec, n1, n2, complex_rows, generic)
                    E.verify([(ain, ain.download()), (bin_, bin_.download())], out, out.download(), expected=ref, tol=TOL)
                    rows = out.tensor(out.download())
                    pk = E.Arena("peak", dt, 1, 3, offset_elems=offset).upload(ctx)
                    lg = E.Arena("lags", np.int32, 1, 3, offset_elems=(offset + 1) % 4).upload(ctx)
                    E.call(ctx, fn, ain.ptr, n1, ain.row_stride, bin_.ptr, n2, bin_.row_stride, 3, int(complex_rows), 1, MODE_ID[mode], 0, 0.0, 1,
                           pk.ptr, lg.ptr, _lib.DEVICE)
                    E.verify([(ain, ain.download()), (bin_, bin_.download())], pk, pk.download(), same_bits_as=O.peak(rows, n1, n2, mode)[1])
                    E.verify([], lg, lg.download(), table=O.peak(rows, n1, n2, mode)[0])
                # host memory: the staged copies keep the row strides
                ain = E.Arena("a", dt, 3, n1, n1 + 5, offset_elems=1, data=a)
                bin_ = E.Arena("b", dt, 3, n2, n2 + 3, offset_elems=2, data=b)
                out = E.Arena("out", dt, 3, n_out)
                aimg, bimg, oimg = ain.image.copy(), bin_.image.copy(), out.image.copy()
                E.call(ctx, fn, C.c_void_p(aimg.ctypes.data + ain.offset_bytes), n1, n1 + 5, C.c_void_p(bimg.ctypes.data + bin_.offset_bytes), n2, n2 + 3, 3,
                       int(complex_rows), 1, MODE_ID[mode], 0, 0.0, 0, C.c_void_p(oimg.ctypes.data + out.offset_bytes), None, _lib.HOST)
                E.verify([(ain, aimg), (bin_, bimg)], out, oimg, expected=ref, tol=TOL)


def test_the_result_may_not_overlap_an_operand_but_the_operands_may_coincide(ctx):
    lib = _lib.load()
    x = ctx.to_device(noise(97, (2, 64)))
    out = ctx.empty((2, 127), np.float32)
    args = lambda a, b, o: (_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(a), 64, 64, C.c_void_p(b), 64, 64, 2, 0, 1, 0, 0, 0.0, 0, C.c_void_p(o), None,  # noqa: E731
                            _lib.DEVICE)
    assert lib.nxsig_xcorr(*args(x.ptr, x.ptr, out.ptr)) == 0                      # in1 is in2
    ctx.sync()
    check("autocorrelation through the C ABI", out.numpy(), O.rows(x.numpy(), x.numpy(), "correlate", "full"))
    for o in (x.ptr, x.ptr + 4 * 100):
        assert lib.nxsig_xcorr(*args(x.ptr, x.ptr, o)) != 0
        assert "must not overlap" in _lib.last_error()


def test_batch_0_launches_nothing(ctx):
    lib = _lib.load()
    x = ctx.to_device(noise(93, (1, 8)))
    out = ctx.empty((15,), np.float32)
    rc = lib.nxsig_xcorr(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(x.ptr), 8, 8, C.c_void_p(x.ptr), 8, 8, 0, 0, 1, 0, 0, 0.0, 0, C.c_void_p(out.ptr),
                         None, _lib.DEVICE)
    assert rc == 0 and ctx.last_dispatch() == ""


def test_the_switch_in_the_environment_of_a_fresh_process(tmp_path):
    """NXSIG_XCORR_WAVE=0 read at context creation by a child process: the generic tier, the same bound"""
    a, b = noise(95, (3, 600)), noise(96, (3, 300))
    np.save(tmp_path / "a.npy", a)
    np.save(tmp_path / "b.npy", b)
    code = (
        "import sys, numpy as np, nx_signal_amd as S\n"
        "from nx_signal_amd import convolution\n"
        "c = S.Context(0)\n"
        "y = convolution.correlate_rows(c.to_device(np.load(sys.argv[1])), c.to_device(np.load(sys.argv[2])), 'same', ctx=c); c.sync()\n"
        "print('DISPATCH', c.last_dispatch()); np.save(sys.argv[3], y.numpy())\n")
    env = dict(os.environ, NXSIG_XCORR_WAVE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "y.npy")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DISPATCH " + GENERIC in r.stdout
    check("NXSIG_XCORR_WAVE=0", np.load(tmp_path / "y.npy"), O.rows(a, b, "correlate", "same"))


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its XCORR_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_xcorr.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_XCORR) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.XCORR_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_xcorr"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
    assert len(rows) == len(golden["null_ctx"]["nxsig_xcorr"]) - 1     # batch = 0 runs with a null context alone
