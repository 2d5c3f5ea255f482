"""Filters.savgol_filter on the GPU against the f64 oracle of tests/savgol_oracle.py (the definition of include/nxsig.h in numpy, the
exact rational weights) run on the SAME samples.  The error of a row is max |err| / max |ref| over the row, bound 1e-5.  T, the outputs
of a tile, is read from csrc/savgol_plan.hpp — the library is not loaded while pytest collects — so the lengths sit on the seams: below
half a window, around a window, around a tile (rows shorter than a tile take savgol.generic), and two tiles and a bit.

The bound and the reference's own error.  The oracle is itself a double sum of W products: its result carries a rounding error of up to
W 2^-53 sum_j |k[j]| max|ext|.  Where the true result is far below the samples — the derivative of a row of one sample is exactly zero,
and what either side computes is what rounding leaves — 1e-5 of the reference's magnitude would be a bound on noise against noise.  So with
FLOOR that error of the reference, a row is held to the plain 1e-5 max|ref| wherever that is more than 1000 FLOOR — every row whose
result is of the samples' size, the 1000 + N(0, 1) rows under the second derivative included — and to 1e-5 max|ref| + FLOOR only where
the reference does not stand clear of its own rounding.

Every shape runs on savgol.tiles and on savgol.generic (NXSIG_DISABLE_SAVGOL_TILES) and the two are held to the same bits.

Non-finite rule under test: an output is non-finite exactly when its window, after extension, covers an Inf / NaN sample; under interp
all W // 2 edge outputs of a side are when the first / last W samples hold one; the finite outputs stay in bound."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import extents as E
import savgol_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, filters

pytestmark = pytest.mark.gpu

TOL = 1e-5
TILES, GENERIC = "savgol.tiles", "savgol.generic"
with open(os.path.join(ROOT, "nx_signal_amd", "csrc", "savgol_plan.hpp")) as f:
    T = int(re.search(r"kSavgolTile = (\d+);", f.read()).group(1))
WINDOWS = (3, 4, 5, 6, 31, 32, 255, 1025)
MODE_ID = {m: i for i, m in enumerate(("mirror", "constant", "nearest", "wrap", "interp"))}


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_DISABLE_SAVGOL_TILES on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_SAVGOL_TILES", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_SAVGOL_TILES")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def noise(seed, shape, dtype=np.float32, offset=0.75, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.standard_normal(shape) + offset) * scale).astype(dtype)


def order(w, deriv):
    """the polynomial of the accuracy cases: a cubic where the window holds one (deriv = 3 over three samples: deriv > polyorder, zeros)"""
    return min(3, w - 1)


def dev(ctx, x, w, p, generic=False, **kw):
    """savgol_filter on a device tensor: (numpy result, dispatch record)"""
    with Tier(ctx, generic):
        out = filters.savgol_filter(ctx.to_device(x), w, p, ctx=ctx, **kw)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), rec


def floor(x, w, p, deriv, delta, mode, cval):
    """the rounding error of the reference's own double sum: W 2^-53 sum|k| max|ext| (the module docstring)"""
    k = O.weights(w, p, deriv, float(delta))
    finite = np.abs(np.where(np.isfinite(x), x, 0.0)).max()
    top = max(float(finite), abs(cval) if mode == "constant" else 0.0)
    return w * 2.0 ** -53 * float(np.abs(k).sum()) * top


def check(name, got, x, w, p, deriv=0, delta=1.0, mode="interp", cval=0.0):
    """got against the oracle on the same samples: the finite pattern exactly, the finite outputs within the bound; returns the error"""
    ref = O.savgol_filter(x, w, p, deriv, delta, mode, cval)
    assert got.shape == ref.shape and got.dtype == x.dtype, name
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (name, np.argwhere(np.isfinite(got) != fin)[:4].tolist())
    d = np.where(fin, np.abs(np.where(fin, got, 0.0).astype(np.float64) - np.where(fin, ref, 0.0)), 0.0)
    scale = np.where(fin, np.abs(ref), 0.0).max(axis=-1)
    low = floor(x, w, p, deriv, delta, mode, cval)
    # a row whose reference stands clear of its own rounding error by a factor of 1000 against the bound is held to the plain 1e-5
    clear = TOL * scale > 1e3 * low
    bound = np.where(clear, TOL * scale, TOL * scale + low)
    assert (d.max(axis=-1) <= bound).all(), (name, (d.max(axis=-1) / np.maximum(scale, 1e-300)).tolist(), low)
    # the figure reported: the error over the reference's magnitude on those rows
    return float((d.max(axis=-1)[clear] / scale[clear]).max()) if clear.any() else 0.0


def lengths(w, mode):
    h = w // 2
    return [n for n in sorted({1, 2, h, w - 1, w, w + 1, T - 1, T, T + 1, 2 * T + h}) if n >= 1 and (mode != "interp" or n >= w)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("w", WINDOWS)
def test_accuracy_on_every_seam(ctx, w, dtype):
    """every mode x deriv 0 .. 3 at n = 1, 2, h, W - 1, W, W + 1, T - 1, T, T + 1, 2 T + h where the mode allows, three rows each, on
    device tensors through both tiers (same bits) and, for deriv 1, on host arrays as well"""
    worst = 0.0
    for mode in O.MODES:
        for deriv in range(4):
            p = order(w, deriv)
            for n in lengths(w, mode):
                x = noise(w * 131 + deriv * 17 + n, (3, n), dtype)
                kw = dict(deriv=deriv, delta=0.5, mode=mode, cval=0.5)
                y, rec = dev(ctx, x, w, p, **kw)
                assert rec == (TILES if n >= T else GENERIC), (mode, deriv, n, rec)
                worst = max(worst, check(f"W={w} {mode} deriv={deriv} n={n}", y, x, w, p, **kw))
                yg, rec = dev(ctx, x, w, p, generic=True, **kw)
                assert rec == GENERIC and same_bits(y, yg), (mode, deriv, n)
                if deriv == 1:
                    host = filters.savgol_filter(x, w, p, ctx=ctx, **kw)
                    assert isinstance(host, np.ndarray) and same_bits(host, y), (mode, n)
    print(f"savgol-accuracy W={w} {np.dtype(dtype).name} every mode, deriv 0..3, every seam: {worst:.3e}")


@pytest.mark.parametrize("generic", [False, True], ids=["tiles", "generic"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_strided_rows_inside_poisoned_arenas(ctx, generic, dtype):
    """batch 3 with batch_stride > length, rows starting 1, 2 and 3 elements off a 16-byte boundary, inside poisoned arenas: nothing of
    the pattern in a result, nothing written outside it, every output written, the inputs untouched, the bits of the dense call"""
    w, p, deriv, length = 31, 3, 1, T + 2 * 31 + 5
    assert length % 2 == 1
    x = noise(11, (3, length), dtype)
    lib = _lib.load()
    is64 = int(dtype == np.float64)
    fn = lambda h, *a: lib.nxsig_savgol_filter(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    for mode in ("interp", "mirror", "wrap"):
        dense, _ = dev(ctx, x, w, p, generic=generic, deriv=deriv, mode=mode)
        check(f"dense {mode}", dense, x, w, p, deriv, 1.0, mode)
        ref = O.savgol_filter(x, w, p, deriv, 1.0, mode).astype(dtype)
        with Tier(ctx, generic):
            for gap, offset in ((1, 1), (3, 2), (5, 3), (64, 0)):
                xin = E.Arena("x", dtype, 3, length, length + gap, offset_elems=offset, data=x).upload(ctx)
                out = E.Arena("y", dtype, 3, length, offset_elems=(offset + 1) % 4).upload(ctx)
                rec = E.call(ctx, fn, xin.ptr, is64, length, 3, length + gap, w, p, deriv, 1.0, MODE_ID[mode], 0.0, out.ptr, _lib.DEVICE)
                assert rec == (GENERIC if generic else TILES)
                E.verify([(xin, xin.download())], out, out.download(), expected=ref, tol=TOL, same_bits_as=dense)
            # host memory: the staged copy keeps the row stride
            xin = E.Arena("x", dtype, 3, length, length + 3, offset_elems=1, data=x)
            out = E.Arena("y", dtype, 3, length)
            ximg, oimg = xin.image.copy(), out.image.copy()
            E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), is64, length, 3, length + 3, w, p, deriv, 1.0, MODE_ID[mode], 0.0,
                   C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
            E.verify([(xin, ximg)], out, oimg, expected=ref, tol=TOL, same_bits_as=dense)


@pytest.mark.parametrize("generic", [False, True], ids=["tiles", "generic"])
def test_a_large_offset_and_rows_of_every_scale(ctx, generic):
    """a 1000 + N(0, 1) f32 row under the second derivative — the case an f32 accumulation misses by two decades — and rows scaled
    1e-4, 1 and 1e4"""
    n = 2 * T + 77
    x = noise(21, (2, n), offset=1000.0)
    for w, p in ((5, 2), (31, 3), (255, 5), (1025, 9)):
        for mode in ("interp", "nearest"):
            y, _ = dev(ctx, x, w, p, generic=generic, deriv=2, mode=mode)
            err = check(f"offset 1000 W={w} {mode}", y, x, w, p, 2, 1.0, mode)
            print(f"savgol-accuracy offset-1000 deriv=2 W={w} {mode} {'generic' if generic else 'tiles'}: {err:.3e}")
    for scale in (1e-4, 1.0, 1e4):
        x = noise(22, (2, n), scale=scale)
        for deriv in (0, 1):
            y, _ = dev(ctx, x, 31, 3, generic=generic, deriv=deriv, mode="mirror")
            err = check(f"scale {scale} deriv={deriv}", y, x, 31, 3, deriv, 1.0, "mirror")
            print(f"savgol-accuracy scale={scale:g} deriv={deriv} {'generic' if generic else 'tiles'}: {err:.3e}")


def test_a_host_array_along_axis_0_and_integers(ctx):
    n = T + 9
    x = noise(23, (n, 3))
    y = filters.savgol_filter(x, 9, 2, ctx=ctx, axis=0, mode="wrap")
    assert isinstance(y, np.ndarray) and y.shape == (n, 3) and y.flags.c_contiguous
    check("axis 0", np.ascontiguousarray(y.T), np.ascontiguousarray(x.T), 9, 2, 0, 1.0, "wrap")
    assert same_bits(np.ascontiguousarray(y.T), dev(ctx, np.ascontiguousarray(x.T), 9, 2, mode="wrap")[0])
    ints = np.arange(40, dtype=np.int32) ** 2
    yi = filters.savgol_filter(ints, 7, 2, ctx=ctx, deriv=1)
    assert yi.dtype == np.float64 and np.abs(yi - 2.0 * np.arange(40)).max() <= 1e-9     # a parabola's slope, edges included
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        filters.savgol_filter(ctx.to_device(x), 9, 2, axis=0)


@pytest.mark.parametrize("generic", [False, True], ids=["tiles", "generic"])
def test_two_calls_give_the_same_bits_and_a_row_does_not_depend_on_its_neighbours(ctx, generic):
    n = T + 300
    x = noise(25, (3, n))
    for mode in ("interp", "constant"):
        a, _ = dev(ctx, x, 32, 4, generic=generic, deriv=1, mode=mode, cval=2.0)
        b, _ = dev(ctx, x, 32, 4, generic=generic, deriv=1, mode=mode, cval=2.0)
        assert same_bits(a, b)
        for r in range(3):
            alone, _ = dev(ctx, x[r:r + 1], 32, 4, generic=generic, deriv=1, mode=mode, cval=2.0)
            assert same_bits(alone[0], a[r])
        others = x.copy()
        others[0], others[2] = 7.0, np.nan
        c, _ = dev(ctx, others, 32, 4, generic=generic, deriv=1, mode=mode, cval=2.0)
        assert same_bits(c[1], a[1])


@pytest.mark.parametrize("generic", [False, True], ids=["tiles", "generic"])
def test_65537_rows(ctx, generic):
    """the row index does not live on gridDim.y: 251 distinct rows repeated to 65 537 — the small call is held to the oracle, every row
    of the large one to its bits"""
    x = noise(27, (251, 40))
    small, _ = dev(ctx, x, 7, 3, generic=generic, deriv=1)
    check("251 x 40", small, x, 7, 3, 1)
    reps = -(-65537 // 251)
    big, rec = dev(ctx, np.tile(x, (reps, 1))[:65537], 7, 3, generic=generic, deriv=1)
    assert rec == GENERIC and same_bits(big, np.tile(small, (reps, 1))[:65537])
    # and as tiles: 65 537 rows of one tile each is too much for a test; 2 tiles x 300 rows runs the same row arithmetic
    y = noise(28, (3, 2 * T))
    tall, rec = dev(ctx, np.tile(y, (100, 1)), 7, 3, generic=generic, deriv=1)
    assert rec == (GENERIC if generic else TILES) and same_bits(tall, np.tile(dev(ctx, y, 7, 3, generic=generic, deriv=1)[0], (100, 1)))


@pytest.mark.parametrize("generic", [False, True], ids=["tiles", "generic"])
@pytest.mark.parametrize("w", [7, 32])
def test_non_finite_samples_reach_exactly_the_outputs_whose_window_covers_them(ctx, w, generic):
    """NaN / +Inf / -Inf in the middle, within W // 2 of each end for every mode, and in a neighbouring row: the finite / non-finite
    pattern equals the oracle's and the finite outputs stay in bound; other rows keep their bits"""
    h, p = w // 2, 3
    for n in (T + 3 * w, 3 * w):
        clean = noise(31 + n, (3, n))
        for mode in O.MODES:
            ref_clean, _ = dev(ctx, clean, w, p, generic=generic, deriv=1, mode=mode, cval=0.5)
            for bad, places in ((np.nan, (n // 2,)), (np.inf, (h - 1,)), (-np.inf, (n - h,)), (np.nan, (0, n - 1)), (np.inf, (1, n // 2, n - 2))):
                x = clean.copy()
                for q in places:
                    x[1, q] = bad
                y, _ = dev(ctx, x, w, p, generic=generic, deriv=1, mode=mode, cval=0.5)
                check(f"W={w} n={n} {mode} {bad} at {places}", y, x, w, p, 1, 1.0, mode, 0.5)
                assert same_bits(y[0], ref_clean[0]) and same_bits(y[2], ref_clean[2]), (mode, places)
                assert not np.isfinite(y[1, list(places)]).any()
    # zero weights do not hide a sample: deriv > polyorder gives all-zero weights and still a non-finite window
    x = noise(33, (1, 64))
    x[0, 30] = np.inf
    y, _ = dev(ctx, x, 5, 2, generic=generic, deriv=3, mode="mirror")
    assert np.array_equal(np.isfinite(y[0]), np.abs(np.arange(64) - 30) > 2) and not y[0][np.isfinite(y[0])].any()


def test_the_tables_of_a_parameter_set_are_formed_once_and_follow_the_table_cache():
    """the weights and the edge table are memoised per context beside the table cache and dropped with it.  The context counts how often
    it is asked for a cached table ("TABLE_REQUESTS"): the first call of a parameter set asks twice (weights, edge table; once without
    interp), every later call with the same parameters not at all — the memo hands the two pointers back, so nothing is formed again and
    no table is added.  With room for two tables every other parameter set trims the cache; the tables are rebuilt and the bits stay"""
    c = S.Context(0)
    requests = lambda: c.get_tuning("TABLE_REQUESTS")[0]   # noqa: E731
    x = noise(41, (1, T + 1100))
    before = requests()
    first, rec = dev(c, x, 1025, 15, deriv=1)
    assert rec == TILES and requests() == before + 2
    for generic in (False, True, False):
        y, _ = dev(c, x, 1025, 15, generic=generic, deriv=1)
        assert same_bits(first, y) and requests() == before + 2
    dev(c, x, 1025, 15, deriv=1, mode="mirror")            # another parameter set: the weights alone
    assert requests() == before + 3
    dev(c, x, 1025, 15, deriv=1, mode="nearest", cval=3.0)   # neither the mode (but for interp) nor cval is part of the set
    assert requests() == before + 3
    c.set_tuning("TABLE_CACHE_MAX", 2)
    for w in (1025, 31, 1025):           # another parameter set in between: another pair of tables, so the trim runs
        y, _ = dev(c, x, w, 15, deriv=1)
    c.clear_tuning("TABLE_CACHE_MAX")
    assert same_bits(first, y) and requests() > before + 5
    assert c.get_tuning("TABLE_REQUESTS")[1] is False
    with pytest.raises(Exception, match="no such switch"):
        c.set_tuning("TABLE_REQUESTS", 1)


def test_the_dispatch_record_names_the_tier(ctx):
    x = noise(43, (2, T))
    assert dev(ctx, x, 5, 2)[1] == TILES and dev(ctx, x, 5, 2, generic=True)[1] == GENERIC
    assert dev(ctx, x[:, :T - 1], 5, 2)[1] == GENERIC        # a row shorter than one tile
    assert _lib.load().nxsig_savgol_tile() == T


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its SAVGOL_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_savgol.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_SAVGOL) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.SAVGOL_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_savgol_filter"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
