"""Filters.sosfilt / sosfiltfilt on the GPU against the f64 oracle of tests/iir_oracle.py run on the SAME f32 samples.  The error of a
row is max |err| / max |ref| over the row, bound 1e-5 (the suite's own; measured: sosfilt <= 5.6e-8, the f32 rounding itself; sosfiltfilt, which rounds twice, <= 9.9e-8).  Chunk C and
tile T are read from the library, so the lengths sit on the seams of the scan: one chunk, one tile, several tiles, and more than 64 tiles
(the carry over the tiles of a row walks R = 2 tiles or more per lane there: its second level).

One reference serves every accuracy case: a causal filter's output over a prefix of a row is the prefix of its output, so ONE run of
the oracle over the longest row — every cascade at once, filled up to 20 sections with identity sections — gives the reference of
every shorter length.

Non-finite rule under test: outputs ahead of the first Inf / NaN sample of a row are bit for bit those of the row with that sample and
everything after it zeroed; every output from it on is non-finite; other rows are untouched; sosfiltfilt turns the whole row non-finite;
a zi row with a non-finite entry counts as a non-finite sample 0."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import extents as E
import iir_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters

pytestmark = pytest.mark.gpu

TOL = 1e-5
# states are doubles end to end: the scheme against the recurrence reads at most 1.7e-11 on the host (tests/san_iir.cpp); FMA contraction on the
# device and the oracle's own round-off (amplified by poles at radius 0.999) stay within a few 1e-11 as well; bound a decade above
ZF_TOL = 1e-9
SCAN, GENERIC = "sosfilt.scan", "sosfilt.generic"

with open(os.path.join(ROOT, "tests", "golden", "iir_vectors.json")) as f:
    GOLDEN = json.load(f)
SOS = {c["name"]: np.array(c["sos"], np.float64) for c in GOLDEN["cases"]}
GROWING = ("integrator", "unstable_r1001")   # a pole on and a pole pair outside the unit circle: 3000 samples
STABLE = [n for n in SOS if n not in GROWING]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_DISABLE_SOSFILT_SCAN on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_SOSFILT_SCAN", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_SOSFILT_SCAN")


def geometry(n_sections):
    lib = _lib.load()
    k = min(n_sections, 16)
    return lib.nxsig_sosfilt_chunk(k), lib.nxsig_sosfilt_tile(k)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def noise(seed, shape, offset=0.75):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(shape) + offset).astype(np.float32)


def dev(ctx, fn, x, sos, **kw):
    """a filter of nx_signal_amd.filters on a device tensor: (numpy result[, zf], dispatch record)"""
    out = fn(ctx.to_device(x), sos, ctx=ctx, **kw)
    ctx.sync()
    rec = ctx.last_dispatch()
    if isinstance(out, tuple):
        assert isinstance(out[0], S.DeviceBuffer)
        return out[0].numpy(), out[1], rec
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), rec


def c_sosfilt(ctx, x, sos, zi=None, want_zf=False, direction=0, mem=None):
    """nxsig_sosfilt_f32 itself on host memory (or device memory with mem = DEVICE): (y, zf or None)"""
    mem = _lib.HOST if mem is None else mem
    x = np.ascontiguousarray(x, np.float32)
    sos = np.ascontiguousarray(sos, np.float64)
    batch, n = x.shape
    y = np.empty_like(x)
    zf = np.empty((batch, sos.shape[0], 2), np.float64) if want_zf else None
    zi = None if zi is None else np.ascontiguousarray(zi, np.float64)
    zi_rows = 1 if zi is None or zi.ndim == 2 else zi.shape[0]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib = _lib.load()
    if mem == _lib.DEVICE:
        xd, yd = ctx.to_device(x), ctx.empty(x.shape, np.float32)
        _lib.check(lib.nxsig_sosfilt_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(xd.ptr), n, batch, n, p(sos), sos.shape[0], p(zi), zi_rows,
                                         p(zf), direction, C.c_void_p(yd.ptr), mem))
        ctx.sync()
        return yd.numpy(), zf
    _lib.check(lib.nxsig_sosfilt_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), p(x), n, batch, n, p(sos), sos.shape[0], p(zi), zi_rows, p(zf), direction,
                                     p(y), mem))
    return y, zf


def check(name, got, ref):
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), name
    err = O.nerr(got, ref)
    print(f"iir-accuracy {name}: {err:.3e}")
    assert err <= TOL, (name, err)
    return err


# ---- the shared reference
LONG_T = 4096   # the largest tile of any cascade here (asserted below): 65 tiles of it and a chunk and a sample
LONG = 65 * LONG_T + 64 + 1
SECTIONS = 20


@functools.lru_cache(maxsize=None)
def long_input():
    return noise(1, (1, LONG))


@functools.lru_cache(maxsize=None)
def long_reference():
    """{name: f64[LONG]}: every stable cascade over the one long row, in one run of the oracle"""
    stack = np.stack([O.pad_sections(SOS[n], SECTIONS) for n in STABLE])
    y, _ = O.sosfilt(stack, np.repeat(long_input().astype(np.float64), len(STABLE), axis=0))
    return {n: y[i] for i, n in enumerate(STABLE)}


@functools.lru_cache(maxsize=None)
def growing_reference(name):
    y, _ = O.sosfilt(SOS[name], long_input()[:, :3000].astype(np.float64))
    return y[0]


def lengths_of(name):
    c, t = geometry(SOS[name].shape[0])
    assert t <= LONG_T and c <= 64
    base = [1, 2, 3, c - 1, c, c + 1, t - 1, t, t + 1]
    return base + ([3000] if name in GROWING else [3 * t + c + 1, 65 * t + c + 1])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("name", list(SOS))
def test_accuracy_on_every_seam(ctx, name, generic):
    """every recorded cascade at 1, 2, 3, C - 1, C, C + 1, T - 1, T, T + 1, 3 T + C + 1 samples and at more than 64 tiles (the growing
    ones: 3000 samples), on both tiers; the 20 sections run through the Python split"""
    sos = SOS[name]
    ref = growing_reference(name) if name in GROWING else long_reference()[name]
    c, _ = geometry(sos.shape[0])
    worst = 0.0
    with Tier(ctx, generic):
        for n in lengths_of(name):
            y, rec = dev(ctx, filters.sosfilt, long_input()[:, :n], sos)
            assert rec.split("+") == [GENERIC if generic or n <= c else SCAN], (n, rec)
            worst = max(worst, check(f"{name} n={n} {'generic' if generic else 'scan'}", y, ref[None, :n]))
    print(f"iir-accuracy-worst {name} {'generic' if generic else 'scan'}: {worst:.3e}")


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_batches_of_1_3_and_65537_rows(ctx, generic):
    """65 537 rows of 40 samples: 251 distinct rows repeated — the small call is held to the oracle, every row of the large one to its bits"""
    sos = SOS["butter4_hp20"]
    assert 40 > geometry(2)[0]   # two chunks: the scan tier runs
    x = noise(7, (251, 40))
    ref, _ = O.sosfilt(sos, x)
    with Tier(ctx, generic):
        small, rec = dev(ctx, filters.sosfilt, x, sos)
        assert rec == (GENERIC if generic else SCAN)
        check("251 x 40", small, ref)
        for b in (1, 3):
            y, _ = dev(ctx, filters.sosfilt, x[:b], sos)
            assert same_bits(y, small[:b])
        reps = -(-65537 // 251)
        big, rec = dev(ctx, filters.sosfilt, np.tile(x, (reps, 1))[:65537], sos)
        assert rec == (GENERIC if generic else SCAN)
        assert same_bits(big, np.tile(small, (reps, 1))[:65537])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("direction", [0, 1])
def test_rows_that_are_not_on_a_16_byte_boundary(ctx, generic, direction):
    """odd lengths with batch_stride == length, then rows length + gap apart inside poisoned arenas: nothing of the pattern in a result,
    nothing written outside it, every output written, the inputs untouched, the bits of the dense call"""
    sos = SOS["ellip4_bp"]
    c, t = geometry(4)
    length = t + 2 * c + 5
    assert length % 2 == 1
    x = noise(11, (3, length))
    ref = (O.sosfilt_backward if direction else O.sosfilt)(sos, x)[0]
    lib = _lib.load()
    sp = sos.ctypes.data_as(C.c_void_p)
    fn = lambda h, *a: lib.nxsig_sosfilt_f32(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    with Tier(ctx, generic):
        dense, _ = c_sosfilt(ctx, x, sos, direction=direction, mem=_lib.DEVICE)
        check(f"odd rows dir={direction}", dense, ref)
        for gap, offset in ((0, 1), (3, 1), (5, 3), (64, 2)):
            xin = E.Arena("x", np.float32, 3, length, length + gap, offset_elems=offset, data=x).upload(ctx)
            out = E.Arena("y", np.float32, 3, length, offset_elems=(offset + 1) % 4).upload(ctx)
            rec = E.call(ctx, fn, xin.ptr, length, 3, length + gap, sp, 4, None, 1, None, direction, out.ptr, _lib.DEVICE)
            assert rec == (GENERIC if generic else SCAN)
            E.verify([(xin, xin.download())], out, out.download(), expected=ref.astype(np.float32), tol=TOL, same_bits_as=dense)
        # host memory: the staged copy keeps the row stride
        xin = E.Arena("x", np.float32, 3, length, length + 3, offset_elems=1, data=x)
        out = E.Arena("y", np.float32, 3, length)
        ximg, oimg = xin.image.copy(), out.image.copy()
        E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), length, 3, length + 3, sp, 4, None, 1, None, direction,
               C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
        E.verify([(xin, ximg)], out, oimg, expected=ref.astype(np.float32), tol=TOL, same_bits_as=dense)


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_states_in_and_out(ctx, generic):
    """zi for every row alike and per row, zf against the oracle, a row filtered in two pieces through zf -> zi, direction = 1"""
    for name in ("butter4_hp20", "ellip4_bp"):
        sos = SOS[name]
        ns = sos.shape[0]
        c, t = geometry(ns)
        n = 2 * t + c + 7
        x = noise(13, (3, n))
        rng = np.random.Generator(np.random.PCG64(14))
        zi_row = 0.3 * rng.standard_normal((3, ns, 2))
        with Tier(ctx, generic):
            for label, zi in (("one zi", zi_row[0]), ("zi per row", zi_row)):
                ref, zf_ref = O.sosfilt(sos, x, zi)
                y, zf = c_sosfilt(ctx, x, sos, zi=zi, want_zf=True)
                check(f"{name} {label}", y, ref)
                zerr = float((np.abs(zf - zf_ref).max(axis=(1, 2)) / np.abs(zf_ref).max(axis=(1, 2))).max())
                print(f"iir-accuracy {name} {label} zf: {zerr:.3e}")
                assert zerr <= ZF_TOL, (zerr, zf.tolist(), zf_ref.tolist())
            # scipy's layouts through the Python function: zi (n_sections, rows, 2)
            y, zf, _ = dev(ctx, filters.sosfilt, x, sos, zi=zi_row.transpose(1, 0, 2))
            ref, zf_ref = O.sosfilt(sos, x, zi_row)
            check(f"{name} python zi", y, ref)
            assert zf.shape == (ns, 3, 2) and np.abs(zf.transpose(1, 0, 2) - zf_ref).max() <= ZF_TOL * np.abs(zf_ref).max()
            # two pieces against one call: a seam off every chunk and tile boundary, and one on a tile boundary
            whole, zf_whole = c_sosfilt(ctx, x, sos, zi=zi_row, want_zf=True)
            for cut in (t + 5, t):
                a, zf_a = c_sosfilt(ctx, x[:, :cut], sos, zi=zi_row, want_zf=True)
                b, zf_b = c_sosfilt(ctx, x[:, cut:], sos, zi=zf_a, want_zf=True)
                check(f"{name} two pieces cut={cut}", np.concatenate([a, b], axis=1), O.sosfilt(sos, x, zi_row)[0])
                assert O.nerr(np.concatenate([a, b], axis=1), whole) <= TOL
                assert np.abs(zf_b - zf_whole).max() <= ZF_TOL * np.abs(zf_whole).max()
            # backwards: the flipped oracle, states included
            ref, zf_ref = O.sosfilt_backward(sos, x, zi_row)
            y, zf = c_sosfilt(ctx, x, sos, zi=zi_row, want_zf=True, direction=1)
            check(f"{name} backward", y, ref)
            assert np.abs(zf - zf_ref).max() <= ZF_TOL * np.abs(zf_ref).max()
            y, _ = dev(ctx, filters.sosfilt, x, sos, direction=1)
            check(f"{name} backward python", y, O.sosfilt_backward(sos, x)[0])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_the_same_bits_every_time(ctx, generic):
    """two calls; host against device memory; a row alone against the row inside a batch; the same row first and last of a large batch"""
    sos = SOS["cheby1_8_lp100"]
    c, t = geometry(4)
    n = 2 * t + c + 3
    x = noise(17, (5, n))
    with Tier(ctx, generic):
        a, _ = c_sosfilt(ctx, x, sos, mem=_lib.DEVICE)
        b, _ = c_sosfilt(ctx, x, sos, mem=_lib.DEVICE)
        h, _ = c_sosfilt(ctx, x, sos, mem=_lib.HOST)
        assert same_bits(a, b) and same_bits(a, h)
        for r in range(5):
            alone, _ = c_sosfilt(ctx, x[r:r + 1], sos, mem=_lib.DEVICE)
            assert same_bits(alone, a[r:r + 1]), r
        big = noise(18, (700, n))
        big[0] = big[-1] = x[2]
        y, _ = c_sosfilt(ctx, big, sos, mem=_lib.DEVICE)
        assert same_bits(y[0], a[2]) and same_bits(y[-1], a[2])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
def test_a_non_finite_sample_reaches_what_follows_it_and_nothing_else(ctx, generic, value):
    sos = SOS["ellip4_bp"]
    c, t = geometry(4)
    n = t + c + 9
    clean = noise(19, (3, n))
    with Tier(ctx, generic):
        base, _ = dev(ctx, filters.sosfilt, clean[[0, 2]], sos)
        for at in (0, c - 1, c, t, n - 1):
            x, twin = clean.copy(), clean.copy()
            x[1, at] = value
            twin[1, at:] = 0.0
            y, _ = dev(ctx, filters.sosfilt, x, sos)
            yt, _ = dev(ctx, filters.sosfilt, twin, sos)
            assert same_bits(y[1, :at], yt[1, :at]), at
            assert not np.isfinite(y[1, at:]).any(), at
            assert same_bits(y[[0, 2]], base), at
            ff, _ = dev(ctx, filters.sosfiltfilt, x, sos)
            assert not np.isfinite(ff[1]).any() and np.isfinite(ff[[0, 2]]).all(), at
        # a zi row with one non-finite entry (the last section's second state) counts as a non-finite sample 0
        zi = np.zeros((3, 4, 2))
        good, _ = c_sosfilt(ctx, clean, sos, zi=zi)
        zi[1, 3, 1] = value
        y, _ = c_sosfilt(ctx, clean, sos, zi=zi)
        assert not np.isfinite(y[1]).any() and same_bits(y[[0, 2]], good[[0, 2]])


def filtfilt_lengths(n_sections):
    c, t = geometry(n_sections)
    return [30, t + 1, 3 * t + c + 1]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["n=30", "n=T+1", "n=3T+C+1"])
@pytest.mark.parametrize("name", ["butter4_hp20", "ellip4_bp"])
def test_sosfiltfilt(ctx, name, which):
    """every padtype at scipy's default padlen, padlen 0 and padlen length - 1; 2 and 4 sections"""
    sos = SOS[name]
    n = filtfilt_lengths(sos.shape[0])[which]
    x = noise(23 + which, (2, n))
    cases = [(p, None) for p in ("odd", "even", "constant", None)] + [("odd", 0), ("even", n - 1), ("constant", n - 1), ("odd", n - 1)]
    for padtype, padlen in cases:
        ref = O.sosfiltfilt(sos, x, padtype, padlen)
        y, rec = dev(ctx, filters.sosfiltfilt, x, sos, padtype=padtype, padlen=padlen)
        assert set(rec.split("+")) <= {SCAN, GENERIC} and rec
        check(f"sosfiltfilt {name} n={n} {padtype} padlen={padlen}", y, ref)
    h = filters.sosfiltfilt(x, sos, ctx=ctx)
    assert isinstance(h, np.ndarray) and same_bits(h, dev(ctx, filters.sosfiltfilt, x, sos)[0])
    with Tier(ctx, True):
        y, rec = dev(ctx, filters.sosfiltfilt, x, sos)
        assert rec == GENERIC
        check(f"sosfiltfilt {name} n={n} generic", y, O.sosfiltfilt(sos, x))


def test_dispatch_names_and_the_switch(ctx):
    sos = SOS["butter4_lp4k"]
    c, t = geometry(2)
    x = noise(29, (2, t + 1))
    assert dev(ctx, filters.sosfilt, x, sos)[1] == SCAN
    assert dev(ctx, filters.sosfilt, x[:, :c], sos)[1] == GENERIC      # one chunk: nothing to run side by side
    assert dev(ctx, filters.sosfilt, x[:, :c + 1], sos)[1] == SCAN
    with Tier(ctx, True):
        assert dev(ctx, filters.sosfilt, x, sos)[1] == GENERIC
    assert dev(ctx, filters.sosfilt, x, sos)[1] == SCAN
    assert dev(ctx, filters.sosfiltfilt, x, sos)[1] == SCAN


def test_the_cached_matrices_follow_the_table_cache_and_a_stream_of_blocks_adds_no_table():
    """the powers of the state matrix are memoised per context beside the table cache and dropped with it: with room for two tables
    every call trims the cache, rebuilds the matrices and gives the same bits; a row streamed block by block through zf -> zi (every
    block another zi) matches the single call"""
    c = S.Context(0)
    sos = SOS["cheby1_8_lp100"]
    t = geometry(4)[1]
    x = noise(37, (1, 3 * t + 11))
    first, _ = dev(c, filters.sosfilt, x, sos)
    again, _ = dev(c, filters.sosfilt, x, sos)           # the memo's hit
    c.set_tuning("TABLE_CACHE_MAX", 2)
    for n in (x.shape[1], 70 * t, x.shape[1]):           # another R in between: another pair of tables, so the trim runs
        y, _ = dev(c, filters.sosfilt, noise(37, (1, 70 * t))[:, :n] if n != x.shape[1] else x, sos)
    c.clear_tuning("TABLE_CACHE_MAX")
    assert same_bits(first, again) and same_bits(first, y)
    zi, parts = np.zeros((1, 4, 2)), []
    for k in range(0, x.shape[1], t // 2 + 3):
        part, zi = c_sosfilt(c, x[:, k:k + t // 2 + 3], sos, zi=zi[0], want_zf=True)
        parts.append(part)
    check("streamed blocks", np.concatenate(parts, axis=1), O.sosfilt(sos, x)[0])


def test_twenty_sections_through_the_python_split(ctx):
    """16 + 4 sections, with states: zi and zf in scipy's layout over the whole cascade; host arrays and another axis"""
    sos = SOS["ellip20_bp"]
    assert sos.shape[0] == 20
    n = geometry(16)[1] + 70
    x = noise(31, (2, n))
    rng = np.random.Generator(np.random.PCG64(32))
    zi = 0.1 * rng.standard_normal((2, 20, 2))
    ref, zf_ref = O.sosfilt(sos, x, zi)
    y, zf, rec = dev(ctx, filters.sosfilt, x, sos, zi=zi.transpose(1, 0, 2))
    assert rec == SCAN
    check("20 sections with zi", y, ref)
    # the groups hand f32 rows on, so the second group's states see a rounded input: the output's bound, not the states' own
    assert np.abs(zf.transpose(1, 0, 2) - zf_ref).max() <= TOL * np.abs(zf_ref).max()
    host = filters.sosfilt(np.ascontiguousarray(x.T), sos, ctx=ctx, axis=0)
    assert isinstance(host, np.ndarray) and host.shape == (n, 2) and same_bits(np.ascontiguousarray(host.T), dev(ctx, filters.sosfilt, x, sos)[0])
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        filters.sosfilt(ctx.to_device(np.ascontiguousarray(x.T)), sos, axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="16 sections"):
        filters.sosfiltfilt(x, sos, ctx=ctx)


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its IIR_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_iir.json"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P

    with open(P.GOLDEN_IIR) as f:
        golden = json.load(f)["real_ctx"]
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.IIR_TABLE_ENTRIES)
    assert table == golden
    for name in ("nxsig_sosfilt_f32", "nxsig_sosfiltfilt_f32"):
        assert table[name]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
