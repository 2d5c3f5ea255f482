"""Filters.lfilter / filtfilt on the GPU against the f64 oracle of tests/lfilter_oracle.py run on the SAME f32 samples.  The error of a
row is max |err| / max |ref| over the row, bound 1e-5 (the suite's own; measured: <= 5.8e-8, the f32 rounding itself, on every filter but
butter(4, 20 Hz, "hp"), whose direct form reads 2.3e-7 in the plain recurrence); zf within 1e-9 (measured: <= 1.6e-14).  Chunk C and tile T are read from the
library, so the lengths sit on the seams of the scan: one chunk, one tile, several tiles, and one row of more than 64 tiles (the carry
over the tiles of a row walks R = 2 tiles per lane there: its second level).

One reference per filter serves every length: a causal filter's output over a prefix of a row is the prefix of its output.

Non-finite rule under test: outputs ahead of the first Inf / NaN sample of a row are bit for bit those of the row with that sample and
everything after it zeroed; every output from it on is non-finite; other rows are untouched; filtfilt turns the whole row non-finite; a
zi row with a non-finite entry counts as a non-finite sample 0.

The guard case: butter(4, 60 Hz, "hp") at 48 kHz is accurate in the plain double recurrence and lost on a scan (both figures are formed
on the host from the oracle, tests/test_lfilter_host.py); through the public call it must meet the bound and report lfilter.generic."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extents as E
import lfilter_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters

pytestmark = pytest.mark.gpu

TOL = 1e-5
# states are doubles end to end: the scheme against the long double recurrence reads at most 2.6e-11 on the host for the filters the guard
# lets onto the scan (tests/san_lfilter.cpp), and the oracle's own round-off is of that size; the bound sits two decades above
ZF_TOL = 1e-9
SCAN, GENERIC = "lfilter.scan", "lfilter.generic"

with open(os.path.join(ROOT, "tests", "golden", "lfilter_vectors.json")) as f:
    GOLDEN = json.load(f)
BA = {c["name"]: (np.array(c["b"], np.float64), np.array(c["a"], np.float64)) for c in GOLDEN["cases"]}
ON_SCAN = {c["name"]: c["on_scan"] for c in GOLDEN["cases"]}
R1001 = (np.array([1.0]), np.array([1.0, -2.0 * 1.001 * np.cos(0.3), 1.001 * 1.001]))   # a pole pair outside the unit circle
# one filter per padded-order boundary: orders 0, 1, 2, 3, 4, 5, 8, 9, 16
BY_ORDER = ["gain", "preemph", "butter2_lp02", "butter3_lp09", "butter4_lp01", "butter5_lp05", "butter4_bp", "butter9_lp03", "butter16_lp04"]


def order(name):
    b, a = BA[name]
    return max(len(b), len(a)) - 1


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_DISABLE_LFILTER_SCAN on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_LFILTER_SCAN", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_LFILTER_SCAN")


def geometry(n):
    lib = _lib.load()
    return lib.nxsig_lfilter_chunk(n), lib.nxsig_lfilter_tile(n)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def noise(seed, shape, offset=0.75):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(shape) + offset).astype(np.float32)


def dev(ctx, fn, x, ba, **kw):
    """a filter of nx_signal_amd.filters on a device tensor: (numpy result[, zf], dispatch record)"""
    out = fn(ctx.to_device(x), ba[0], ba[1], ctx=ctx, **kw)
    ctx.sync()
    rec = ctx.last_dispatch()
    if isinstance(out, tuple):
        assert isinstance(out[0], S.DeviceBuffer)
        return out[0].numpy(), out[1], rec
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), rec


def c_lfilter(ctx, x, ba, zi=None, want_zf=False, direction=0, mem=None):
    """nxsig_lfilter_f32 itself on host memory (or device memory with mem = DEVICE): (y, zf or None)"""
    mem = _lib.HOST if mem is None else mem
    x = np.ascontiguousarray(x, np.float32)
    b, a = (np.ascontiguousarray(v, np.float64) for v in ba)
    n_states = max(len(b), len(a)) - 1
    batch, n = x.shape
    y = np.empty_like(x)
    zf = np.empty((batch, n_states), np.float64) if want_zf else None
    zi = None if zi is None else np.ascontiguousarray(zi, np.float64)
    zi_rows = 1 if zi is None or zi.ndim == 1 else zi.shape[0]
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib, h = _lib.load(), _lib.ctx_ptr(ctx.handle, _lib._ctx_iir)
    if mem == _lib.DEVICE:
        xd, yd = ctx.to_device(x), ctx.empty(x.shape, np.float32)
        _lib.check(lib.nxsig_lfilter_f32(h, C.c_void_p(xd.ptr), n, batch, n, p(b), len(b), p(a), len(a), p(zi), zi_rows, p(zf), direction,
                                         C.c_void_p(yd.ptr), mem))
        ctx.sync()
        return yd.numpy(), zf
    _lib.check(lib.nxsig_lfilter_f32(h, p(x), n, batch, n, p(b), len(b), p(a), len(a), p(zi), zi_rows, p(zf), direction, p(y), mem))
    return y, zf


def check(name, got, ref):
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), name
    err = O.nerr(got, ref)
    print(f"lfilter-accuracy {name}: {err:.3e}")
    assert err <= TOL, (name, err)
    return err


def zf_gap(zf, ref):
    return float(np.abs(zf - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- the shared references: 3 rows of 2 T + 3 samples per filter (T at most 4096), one run of the oracle each
WIDE = 2 * 4096 + 3


@functools.lru_cache(maxsize=None)
def wide_input():
    return noise(1, (3, WIDE))


@functools.lru_cache(maxsize=None)
def wide_reference(name):
    return O.lfilter(*BA[name], wide_input().astype(np.float64))[0]


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("name", BY_ORDER)
def test_accuracy_on_every_seam_at_every_padded_order(ctx, name, generic):
    """orders 0, 1, 2, 3, 4, 5, 8, 9 and 16 at 1, C - 1, C, C + 1, T - 1, T, T + 1 and 2 T + 3 samples, 3 rows, on both tiers"""
    n_states = order(name)
    c, t = geometry(n_states)
    assert 2 * t + 3 <= WIDE and ON_SCAN[name]
    ref = wide_reference(name)
    worst = 0.0
    with Tier(ctx, generic):
        for n in (1, c - 1, c, c + 1, t - 1, t, t + 1, 2 * t + 3):
            y, rec = dev(ctx, filters.lfilter, wide_input()[:, :n], BA[name])
            assert rec == (GENERIC if generic or n <= c else SCAN), (n, rec)
            worst = max(worst, check(f"{name} order {n_states} n={n} {'generic' if generic else 'scan'}", y, ref[:, :n]))
    print(f"lfilter-accuracy-worst {name} {'generic' if generic else 'scan'}: {worst:.3e}")


@pytest.mark.parametrize("name", ["butter2_hp20", "ellip6", "a0_is_2", "nb_gt_na", "na_gt_nb", "integrator"])
def test_the_other_recorded_filters(ctx, name):
    """the 20 Hz high-pass of order 2 (clustered poles the guard still lets onto the scan), a[0] = 2, nb > na, na > nb, the integrator (3000 samples): scan and generic"""
    n = 3000
    assert n > geometry(order(name))[0] and ON_SCAN[name]
    x = wide_input()[:, :n]
    ref = O.lfilter(*BA[name], x.astype(np.float64))[0]
    y, rec = dev(ctx, filters.lfilter, x, BA[name])
    assert rec == SCAN
    check(f"{name} scan", y, ref)
    with Tier(ctx, True):
        y, rec = dev(ctx, filters.lfilter, x, BA[name])
        assert rec == GENERIC
        check(f"{name} generic", y, ref)


def test_a_pole_pair_at_radius_1001(ctx):
    """the response grows by e^3 over 3000 samples.  The carry's table A^(T R 32) of such a matrix is 1e29, so the guard sends the filter
    to the plain recurrence at every row length: this is lfilter.generic on a growing filter, NOT scan coverage — lfilter.scan never runs
    with a pole outside the unit circle (the integrator, a pole on it, does run there: test_the_other_recorded_filters)"""
    x = wide_input()[:1, :3000]
    ref = O.lfilter(*R1001, x.astype(np.float64))[0]
    y, rec = dev(ctx, filters.lfilter, x, R1001)
    assert rec == GENERIC
    check("radius 1.001", y, ref)


def test_one_row_across_the_second_level_of_the_carry(ctx):
    """64 T + 5 samples of the 20 Hz high-pass of order 2: 65 tiles, two per lane of the carry"""
    ba = BA["butter2_hp20"]
    t = geometry(2)[1]
    x = noise(3, (1, 64 * t + 5))
    ref = O.lfilter(*ba, x.astype(np.float64))[0]
    y, rec = dev(ctx, filters.lfilter, x, ba)
    assert rec == SCAN
    check("64 T + 5", y, ref)


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_batches_of_1_3_and_65_rows(ctx, generic):
    """65 rows of T + 9 samples against the oracle; the calls of 1 and 3 rows carry the bits of those rows in the large call"""
    ba = BA["butter4_bp"]
    n = geometry(8)[1] + 9
    x = noise(7, (65, n))
    ref = O.lfilter(*ba, x.astype(np.float64))[0]
    with Tier(ctx, generic):
        big, rec = dev(ctx, filters.lfilter, x, ba)
        assert rec == (GENERIC if generic else SCAN)
        check(f"65 rows {'generic' if generic else 'scan'}", big, ref)
        for b in (1, 3):
            y, _ = dev(ctx, filters.lfilter, x[:b], ba)
            assert same_bits(y, big[:b])
        alone, _ = dev(ctx, filters.lfilter, x[64:], ba)
        assert same_bits(alone, big[64:])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("direction", [0, 1])
def test_rows_that_are_not_on_a_16_byte_boundary(ctx, generic, direction):
    """an odd length with batch_stride == length, then rows length + gap apart inside poisoned arenas: nothing of the pattern in a result,
    nothing written outside it, every output written, the inputs untouched, the bits of the dense call"""
    ba = BA["butter5_lp05"]
    b, a = ba
    c, t = geometry(5)
    length = t + 2 * c + 5
    assert length % 2 == 1
    x = noise(11, (3, length))
    ref = (O.lfilter_backward if direction else O.lfilter)(b, a, x.astype(np.float64))[0]
    lib = _lib.load()
    bp, ap = b.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)
    fn = lambda h, *args: lib.nxsig_lfilter_f32(_lib.ctx_ptr(h, _lib._ctx_iir), *args)   # noqa: E731
    with Tier(ctx, generic):
        dense, _ = c_lfilter(ctx, x, ba, direction=direction, mem=_lib.DEVICE)
        check(f"odd rows dir={direction} {'generic' if generic else 'scan'}", dense, ref)
        for gap, offset in ((0, 1), (3, 1), (5, 3), (64, 2)):
            xin = E.Arena("x", np.float32, 3, length, length + gap, offset_elems=offset, data=x).upload(ctx)
            out = E.Arena("y", np.float32, 3, length, offset_elems=(offset + 1) % 4).upload(ctx)
            rec = E.call(ctx, fn, xin.ptr, length, 3, length + gap, bp, len(b), ap, len(a), None, 1, None, direction, out.ptr, _lib.DEVICE)
            assert rec == (GENERIC if generic else SCAN)
            E.verify([(xin, xin.download())], out, out.download(), expected=ref.astype(np.float32), tol=TOL, same_bits_as=dense)
        # host memory: the staged copy keeps the row stride
        xin = E.Arena("x", np.float32, 3, length, length + 3, offset_elems=1, data=x)
        out = E.Arena("y", np.float32, 3, length)
        ximg, oimg = xin.image.copy(), out.image.copy()
        E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), length, 3, length + 3, bp, len(b), ap, len(a), None, 1, None, direction,
               C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
        E.verify([(xin, ximg)], out, oimg, expected=ref.astype(np.float32), tol=TOL, same_bits_as=dense)


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_states_in_and_out(ctx, generic):
    """zi for every row alike and per row, zf against the oracle, direction = 1 equals filtering the flipped row, and a row filtered in
    three blocks through zf -> zi equals one call and asks for no table"""
    for name in ("butter3_lp09", "ellip6"):
        ba = BA[name]
        k = order(name)
        tier = "generic" if generic else "scan"
        c, t = geometry(k)
        n = 2 * t + c + 7
        x = noise(13, (3, n))
        x64 = x.astype(np.float64)
        rng = np.random.Generator(np.random.PCG64(14))
        zi_row = 0.3 * rng.standard_normal((3, k))
        with Tier(ctx, generic):
            for label, zi in (("one zi", zi_row[0]), ("zi per row", zi_row)):
                ref, zf_ref = O.lfilter(*ba, x64, zi)
                y, zf = c_lfilter(ctx, x, ba, zi=zi, want_zf=True)
                check(f"{name} {tier} {label}", y, ref)
                print(f"lfilter-accuracy {name} {tier} {label} zf: {zf_gap(zf, zf_ref):.3e}")
                assert zf_gap(zf, zf_ref) <= ZF_TOL
            # scipy's layout through the Python function: zi (rows, order) for axis -1
            y, zf, _ = dev(ctx, filters.lfilter, x, ba, zi=zi_row)
            ref, zf_ref = O.lfilter(*ba, x64, zi_row)
            check(f"{name} {tier} python zi", y, ref)
            assert zf.shape == (3, k) and zf_gap(zf, zf_ref) <= ZF_TOL
            # three blocks against one call: seams off and on a tile boundary; no table is requested on the way
            whole, zf_whole = c_lfilter(ctx, x, ba, zi=zi_row, want_zf=True)
            requests = ctx.get_tuning("TABLE_REQUESTS")[0]
            cuts = [0, t + 5, 2 * t, n]
            parts, zi = [], zi_row
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                part, zi = c_lfilter(ctx, x[:, lo:hi], ba, zi=zi, want_zf=True)
                parts.append(part)
            assert ctx.get_tuning("TABLE_REQUESTS")[0] == requests
            check(f"{name} {tier} three blocks", np.concatenate(parts, axis=1), ref)
            assert O.nerr(np.concatenate(parts, axis=1), whole) <= TOL and zf_gap(zi, zf_whole) <= ZF_TOL
            # backwards: the flipped oracle, states included, and the library's own forward run of the flipped row
            ref, zf_ref = O.lfilter_backward(*ba, x64, zi_row)
            y, zf = c_lfilter(ctx, x, ba, zi=zi_row, want_zf=True, direction=1)
            check(f"{name} {tier} backward", y, ref)
            assert zf_gap(zf, zf_ref) <= ZF_TOL
            flipped, _ = c_lfilter(ctx, np.ascontiguousarray(x[:, ::-1]), ba, zi=zi_row)
            assert O.nerr(y, flipped[:, ::-1]) <= TOL
            y, _ = dev(ctx, filters.lfilter, x, ba, direction=1)
            check(f"{name} {tier} backward python", y, O.lfilter_backward(*ba, x64)[0])


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
def test_the_same_bits_every_time(ctx, generic):
    """two calls; host against device memory; a row alone against the row inside a batch"""
    ba = BA["butter9_lp03"]
    c, t = geometry(9)
    n = 2 * t + c + 3
    x = noise(17, (5, n))
    with Tier(ctx, generic):
        a, _ = c_lfilter(ctx, x, ba, mem=_lib.DEVICE)
        b, _ = c_lfilter(ctx, x, ba, mem=_lib.DEVICE)
        h, _ = c_lfilter(ctx, x, ba, mem=_lib.HOST)
        assert same_bits(a, b) and same_bits(a, h)
        for r in range(5):
            alone, _ = c_lfilter(ctx, x[r:r + 1], ba, mem=_lib.DEVICE)
            assert same_bits(alone, a[r:r + 1]), r
        # host tensors equal device tensors through the Python function, on another axis too
        host = filters.lfilter(np.ascontiguousarray(x.T), *ba, ctx=ctx, axis=0)
        assert isinstance(host, np.ndarray) and host.shape == (n, 5) and same_bits(np.ascontiguousarray(host.T), a)
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        filters.lfilter(ctx.to_device(np.ascontiguousarray(x.T)), *ba, axis=0)


@pytest.mark.parametrize("generic", [False, True], ids=["scan", "generic"])
@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("name", ["gain", "preemph", "butter3_lp09"])
def test_a_non_finite_sample_reaches_what_follows_it_and_nothing_else(ctx, name, generic, value):
    """to the bit, on both tiers, for a gain (order 0: it runs as an order-1 filter with zero coefficients and keeps the rule), an FIR
    filter (na == 1: the recurrence's behaviour, not scipy's convolution) and a recursive one"""
    ba = BA[name]
    k = order(name)
    c, t = geometry(k)
    n = t + c + 9
    clean = noise(19, (3, n))
    with Tier(ctx, generic):
        base, _ = dev(ctx, filters.lfilter, clean[[0, 2]], ba)
        for at in (0, c - 1, c, t, n - 1):
            x, twin = clean.copy(), clean.copy()
            x[1, at] = value
            twin[1, at:] = 0.0
            y, rec = dev(ctx, filters.lfilter, x, ba)
            assert rec == (GENERIC if generic else SCAN)
            yt, _ = dev(ctx, filters.lfilter, twin, ba)
            assert same_bits(y[1, :at], yt[1, :at]), at
            assert not np.isfinite(y[1, at:]).any(), at
            assert same_bits(y[[0, 2]], base), at
            ff, _ = dev(ctx, filters.filtfilt, x, ba)
            assert not np.isfinite(ff[1]).any() and np.isfinite(ff[[0, 2]]).all(), at
        # a zi row with one non-finite entry (the last state) counts as a non-finite sample 0
        if k == 0:
            return
        zi = np.zeros((3, k))
        good, _ = c_lfilter(ctx, clean, ba, zi=zi)
        zi[1, k - 1] = value
        y, _ = c_lfilter(ctx, clean, ba, zi=zi)
        assert not np.isfinite(y[1]).any() and same_bits(y[[0, 2]], good[[0, 2]])


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["n=40", "n=T-1", "n=T", "n=T+1"])
@pytest.mark.parametrize("name", ["butter2_hp20", "butter4_lp01", "preemph"])
def test_filtfilt(ctx, name, which):
    """every padtype at scipy's default padlen, padlen 0 and an explicit padlen, lengths around T; orders 1, 2 and 4.  The oracle keeps
    the extension and the forward result as f32 rows, as the library does"""
    ba = BA[name]
    t = geometry(order(name))[1]
    n = [40, t - 1, t, t + 1][which]
    x = noise(23 + which, (2, n))
    cases = [(p, None) for p in ("odd", "even", "constant", None)] + [("odd", 0), ("even", 7), ("constant", n - 1), ("odd", n - 1)]
    for padtype, padlen in cases:
        ref = O.filtfilt(*ba, x, padtype, padlen, f32_rows=True)
        y, rec = dev(ctx, filters.filtfilt, x, ba, padtype=padtype, padlen=padlen)
        assert set(rec.split("+")) <= {SCAN, GENERIC} and rec
        check(f"filtfilt {name} n={n} {padtype} padlen={padlen}", y, ref)
    h = filters.filtfilt(x, *ba, ctx=ctx)
    assert isinstance(h, np.ndarray) and same_bits(h, dev(ctx, filters.filtfilt, x, ba)[0])
    with Tier(ctx, True):
        y, rec = dev(ctx, filters.filtfilt, x, ba)
        assert rec == GENERIC
        check(f"filtfilt {name} n={n} generic", y, O.filtfilt(*ba, x, f32_rows=True))


def test_the_recorded_scipy_results(ctx):
    """the library against scipy's own numbers on the two recorded rows (96 samples: two or three chunks)"""
    x = np.array(GOLDEN["x"], np.float32)
    at = GOLDEN["at"]
    for c in GOLDEN["cases"]:
        ba = BA[c["name"]]
        y, _ = dev(ctx, filters.lfilter, x, ba)
        assert O.nerr(y[:, at], np.array(c["y"])) <= TOL, c["name"]
        if "filtfilt" in c:
            for padtype, ref in c["filtfilt"].items():
                y, _ = dev(ctx, filters.filtfilt, x, ba, padtype=None if padtype == "None" else padtype)
                assert O.nerr(y[:, at], np.array(ref)) <= TOL, (c["name"], padtype)


def test_dispatch_names_the_guard_and_the_switch(ctx):
    """the guard case: accurate in the plain recurrence, lost on a scan (tests/test_lfilter_host.py forms both figures on the host from the
    oracle) — through the public call it meets the bound on lfilter.generic, while the 20 Hz high-pass of order 2 stays on lfilter.scan"""
    x = np.random.default_rng(0).standard_normal((1, 6000)).astype(np.float32)
    for name, tier in (("butter4_hp60", GENERIC), ("butter4_hp20", GENERIC), ("butter12_lp03", GENERIC), ("butter2_hp20", SCAN)):
        assert ON_SCAN[name] == (tier == SCAN)
        y, rec = dev(ctx, filters.lfilter, x, BA[name])
        assert rec == tier, (name, rec)
        check(f"guard {name} ({tier})", y, O.lfilter(*BA[name], x.astype(np.float64))[0])
    requests = ctx.get_tuning("TABLE_REQUESTS")[0]
    for name in ("butter4_hp60", "butter2_hp20"):            # the verdict and the tables are memoised: no request the second time
        dev(ctx, filters.lfilter, x, BA[name])
    assert ctx.get_tuning("TABLE_REQUESTS")[0] == requests
    ba = BA["butter2_lp02"]
    c, t = geometry(2)
    x = noise(29, (2, t + 1))
    assert dev(ctx, filters.lfilter, x, ba)[1] == SCAN
    assert dev(ctx, filters.lfilter, x[:, :c], ba)[1] == GENERIC      # one chunk: nothing to run side by side
    assert dev(ctx, filters.lfilter, x[:, :c + 1], ba)[1] == SCAN
    with Tier(ctx, True):
        assert dev(ctx, filters.lfilter, x, ba)[1] == GENERIC
    assert dev(ctx, filters.lfilter, x, ba)[1] == SCAN
    assert dev(ctx, filters.filtfilt, x, ba)[1] == SCAN


def test_the_switch_in_the_environment_of_a_fresh_process(tmp_path):
    """NXSIG_DISABLE_LFILTER_SCAN=1 read at context creation by a child process: the generic tier, the same bound"""
    ba = BA["ellip6"]
    x = noise(41, (2, geometry(6)[1] + 70))
    np.save(tmp_path / "x.npy", x)
    code = (
        "import sys, numpy as np, nx_signal_amd as S\n"
        "from nx_signal_amd import filters\n"
        "x = np.load(sys.argv[1]); b = np.array(%r); a = np.array(%r)\n"
        "c = S.Context(0)\n"
        "y = filters.lfilter(c.to_device(x), b, a, ctx=c); c.sync()\n"
        "print('DISPATCH', c.last_dispatch()); np.save(sys.argv[2], y.numpy())\n" % (ba[0].tolist(), ba[1].tolist()))
    env = dict(os.environ, NXSIG_DISABLE_LFILTER_SCAN="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "x.npy"), str(tmp_path / "y.npy")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DISPATCH " + GENERIC in r.stdout
    check("child process, generic", np.load(tmp_path / "y.npy"), O.lfilter(*ba, x.astype(np.float64))[0])


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its LFILTER_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_lfilter.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P

    with open(P.GOLDEN_LFILTER) as f:
        golden = json.load(f)["real_ctx"]
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.LFILTER_TABLE_ENTRIES)
    assert table == golden
    for name in ("nxsig_lfilter_f32", "nxsig_filtfilt_f32"):
        assert table[name]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
