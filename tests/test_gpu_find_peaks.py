"""PeakFinding.find_peaks on the GPU against tests/find_peaks_oracle.py (the rules in numpy, sequential distance rule, the library's tie
rule).  Every comparison is bit for bit: the integer arrays, peak_heights, the thresholds and the prominences by the issue's own demand,
and the four width arrays as well, because the gap to the oracle MEASURED on the MI355X is 0.0 on every case of this file (the kernels
do the oracle's operations in the oracle's order, no fused multiply-add; profiles/find_peaks/accuracy.txt).  Only a NaN's payload is
not compared (x86 and the GPU disagree on the sign of the default NaN).

Every shape runs four ways: host and device tensors, on find_peaks.tables (the line summary) and on find_peaks.generic
(NXSIG_DISABLE_FIND_PEAKS_TABLES) — so the two tiers are held to the same bits through the oracle.  B is the summary's block, read from
the library; TILE the 4096 flat elements of a compaction tile.  The inputs are quantised noise unless a case builds its own: equal
heights, equal minima and plateaus are the rule in them, not the exception."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import extents as E
import find_peaks_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib
from nx_signal_amd import peak_finding as PF

sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

# The summary's block, as csrc/find_peaks_plan.hpp states it.  The parametrised shapes need it when this module is imported, and
# importing a test module must not load libnxsig.so: pytest imports every module before the first test runs, and a process that maps
# the library (and the HIP runtime it links) ahead of a test that imports torch ends up with torch's own copy of the runtime beside it,
# which then answers ctypes.CDLL("libamdhip64.so") in the graph-capture tests of test_gpu_parity.py and knows no device.
# test_the_block_is_the_librarys holds nxsig_find_peaks_block() to this value.
with open(os.path.join(ROOT, "nx_signal_amd", "csrc", "find_peaks_plan.hpp")) as _f:
    B = int(re.search(r"constexpr int kFindPeaksBlock = (\d+);", _f.read()).group(1))
TILE = 4096
TABLES, GENERIC = "find_peaks.tables", "find_peaks.generic"
OPEN = (None, None)
# every condition given with both sides open: nothing is removed, every property comes back
ALL = dict(plateau_size=OPEN, height=OPEN, threshold=OPEN, prominence=OPEN, width=OPEN)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_DISABLE_FIND_PEAKS_TABLES on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_FIND_PEAKS_TABLES", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_FIND_PEAKS_TABLES")


def noise(seed, shape, dtype=np.float32, step=0.25):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.round(rng.standard_normal(shape) / step) * step).astype(dtype)


def same(a, b):
    """bit for bit, a NaN's payload aside"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def call(ctx, x, device, **opts):
    """(peaks, properties) as numpy arrays, and the dispatch record"""
    peaks, props = PF.find_peaks(ctx.to_device(x) if device else x, ctx=ctx, **opts)
    if device:
        ctx.sync()
        assert all(isinstance(v, S.DeviceBuffer) for v in [*peaks.values(), *props.values()])
        peaks = {k: v.numpy() for k, v in peaks.items()}
        props = {k: v.numpy() for k, v in props.items()}
    return peaks, props, ctx.last_dispatch()


def compare(tag, peaks, props, coords, ref, capacity):
    idx, valid = peaks["indices"], int(peaks["valid_indices"])
    assert idx.shape == (capacity, coords.shape[1]) and idx.dtype == np.int32 and peaks["valid_indices"].dtype == np.uint32, tag
    assert valid == len(coords), (tag, valid, len(coords))
    k = min(valid, capacity)
    assert np.array_equal(idx[:k], coords[:k]) and (idx[k:] == -1).all(), tag
    assert list(props) == list(ref), (tag, list(props), list(ref))
    for name, want in ref.items():
        got = props[name]
        assert got.shape == (capacity,) and got.dtype == want.dtype, (tag, name)
        if name in O.WIDTH_PROPS and k:
            with np.errstate(invalid="ignore"):
                gap = np.nanmax(np.abs(got[:k] - want[:k]), initial=0.0)
            if gap:
                print(f"find-peaks-width-gap {tag} {name}: {gap:.3e}")
        assert same(got[:k], want[:k]), (tag, name, got[:k][:8], want[:k][:8])
        assert (got[k:] == -1).all() if want.dtype.kind == "i" else np.isnan(got[k:]).all(), (tag, name)


def check(ctx, x, tag, axis=-1, ways=((False, False), (False, True), (True, False), (True, True)), **opts):
    """x along axis under opts, every way (generic tier?, device tensor?), against the oracle; returns the oracle's count"""
    oracle_opts = {k: v for k, v in opts.items() if k != "max_peaks"}
    coords, ref = O.tensor(x, axis, **oracle_opts)
    n = x.shape[axis]
    capacity = (x.size // n) * max(0, (n - 1) // 2)
    if opts.get("max_peaks") is not None:
        capacity = min(capacity, opts["max_peaks"])
    for generic, device in ways:
        with Tier(ctx, generic):
            peaks, props, rec = call(ctx, x, device, axis=axis, **opts)
        assert rec == (GENERIC if generic else TABLES), (tag, rec)
        compare(f"{tag} {'generic' if generic else 'tables'} {'device' if device else 'host'}", peaks, props, coords, ref, capacity)
    return len(coords)


def test_the_block_is_the_librarys():
    assert _lib.load().nxsig_find_peaks_block() == B == 64


# ---- line lengths around the block, 1 / 3 / 70 rows, both types
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rows", [1, 3, 70])
def test_line_lengths_on_the_block_boundaries(ctx, dtype, rows):
    found = 0
    for n in (1, 2, 3, 4, B - 1, B, B + 1, 3 * B + 5):
        x = noise(100 + n, (rows, n), dtype)
        found += check(ctx, x, f"{rows}x{n}", distance=3, **ALL)
        found += check(ctx, x, f"{rows}x{n} filtered", ways=((False, True), (True, True)), height=-0.5, threshold=(None, 2.0), prominence=0.5,
                       width=(0.5, None), wlen=B + 1.5, rel_height=0.7)
    assert found > 20 * rows


def test_one_dimension_and_scipy_shapes_after_trim(ctx):
    x = noise(7, (3 * B + 5,))
    peaks, props, _ = call(ctx, x, False, height=0.0, prominence=OPEN)
    idx, cut = PF.trim(peaks, props)
    ref, rprops = O.line(x, height=0.0, prominence=OPEN)
    assert idx.ndim == 1 and np.array_equal(idx, ref) and list(cut) == list(rprops)
    assert all(same(cut[k], rprops[k].astype(cut[k].dtype)) for k in cut)


@pytest.mark.parametrize("shape", [(3, 257, 5), (2, B + 3, 3)], ids=str)
def test_an_axis_that_is_not_the_last(ctx, shape):
    for dtype in (np.float32, np.float64):
        x = noise(11, shape, dtype)
        assert check(ctx, x, f"{shape} axis 1", axis=1, distance=4, **ALL) > 20
        assert check(ctx, x, f"{shape} axis 0", axis=0, ways=((False, True), (True, True)), **ALL) >= 0
        assert check(ctx, x, f"{shape} axis 1 filtered", axis=1, ways=((False, True), (True, True)), prominence=0.75, width=1.0, wlen=9) > 5


def test_plateaus(ctx):
    n = 5 * B
    x = np.zeros((6, n), np.float32)
    x[0, B // 2:2 * B + B // 2 + 3] = 1.0       # starts in one block, ends two blocks later
    x[1, B:3 * B] = 1.0                          # covers whole blocks exactly
    x[2, 2 * B + 5:] = 1.0                       # ends at n - 1: no peak
    x[3, 7] = -1.0
    x[3, 8:8 + 2 * B] = 1.0                      # 2 B long right after a rising edge ...
    x[3, 8 + 2 * B] = 2.0                        # ... with a higher sample after it: no peak there, the single sample is one
    x[4, :] = 3.0                                # constant
    x[5, 1:n - 1] = 1.0                          # the whole interior
    count = check(ctx, x, "plateaus", **ALL)
    coords, ref = O.tensor(x, -1, **ALL)
    assert count == 4 and coords.tolist() == [[0, (B // 2 + 2 * B + B // 2 + 2) // 2], [1, (B + 3 * B - 1) // 2], [3, 8 + 2 * B], [5, (n - 1) // 2]]
    assert ref["plateau_sizes"].tolist() == [2 * B + 3, 2 * B, 1, n - 2]
    check(ctx, x.astype(np.float64), "plateaus f64", plateau_size=(2, 2 * B), width=OPEN)


def test_prominence_and_width_walks(ctx):
    n = 4 * B
    x = np.ones((4, n), np.float32)
    x[:, 5::3] = 1.5
    x[0, 2 * B] = 9.0                            # the tallest peak: bases in the first and the last block
    x[0, 3], x[0, n - 2] = 0.0, 0.5
    x[1, 2 * B] = 9.0                            # equal minima on both sides: the nearer one is the base
    x[1, [10, 40, B + 9]] = 0.25
    x[1, [3 * B + 1, 3 * B + 30, n - 4]] = 0.25
    x[2] = noise(5, (n,)) + 3
    x[3] = np.abs(np.arange(n) - 2 * B) * -0.125 + 20   # one triangle: the width walk crosses whole blocks
    x[3, 2 * B - B // 2] += 0.0625
    coords, ref = O.tensor(x, -1, **ALL)
    k = coords.tolist().index([0, 2 * B])
    assert (ref["left_bases"][k], ref["right_bases"][k], ref["prominences"][k]) == (3, n - 2, 8.5)
    k = coords.tolist().index([1, 2 * B])
    assert (ref["left_bases"][k], ref["right_bases"][k]) == (B + 9, 3 * B + 1)
    for rel in (0.0, 0.5, 1.0):
        check(ctx, x, f"walks rel {rel}", rel_height=rel, **ALL)
        check(ctx, x.astype(np.float64), f"walks f64 rel {rel}", ways=((False, True), (True, True)), rel_height=rel, **ALL)
    # wlen cuts the walk inside a block (peak 2 B, half 20 and 21) and on a block boundary (half B: the window ends at 3 B, starts at B)
    for wlen in (40, 41.5, 2 * B, 2 * B + 1, 2 * B - 2, 2, 3):
        check(ctx, x, f"walks wlen {wlen}", ways=((False, True), (True, True)), wlen=wlen, rel_height=1.0, **ALL)


def test_lines_longer_than_a_super_block(ctx):
    """the summary's second level holds 64 blocks per entry: walks that cross whole super-blocks, end inside one, or meet a NaN there"""
    S = 64 * B
    n = 2 * S + 70
    x = np.zeros((5, n), np.float32)
    x[0] = noise(71, (n,)) + 1e-3 * np.arange(n)          # noise on a slow slope: every right walk is long, every left one short
    x[1, ::1000] = -1.0
    x[1, 100:2 * S + 20] = 2.0                             # a plateau over two whole super-blocks
    x[2] = noise(72, (n,))
    x[2, n // 2], x[2, 7], x[2, n - 9] = 50.0, -30.0, -30.0   # the tallest peak: bases near both ends, super-blocks crossed on both sides
    x[3] = x[2]
    x[3, S + 5], x[3, 3] = np.nan, np.inf                  # a NaN inside the super-block the left walk would cross
    x[4] = -np.abs(np.arange(n) - S - 33) * 0.015625       # one triangle: the width walk crosses super-blocks
    coords, ref = O.tensor(x, -1, **ALL)
    k = coords.tolist().index([2, n // 2])
    assert (ref["left_bases"][k], ref["right_bases"][k]) == (7, n - 9)
    k = coords.tolist().index([1, (100 + 2 * S + 19) // 2])
    assert ref["plateau_sizes"][k] == 2 * S - 80
    assert check(ctx, x, "super-blocks", rel_height=0.9, **ALL) > 2000
    check(ctx, x.astype(np.float64), "super-blocks f64 wlen", ways=((False, True), (True, True)), wlen=2 * S + 1, rel_height=1.0, prominence=0.5, width=OPEN)
    y = np.ascontiguousarray(x[:, :S + 3].T)               # the same along axis 0: [S + 3, 5]
    check(ctx, y, "super-blocks axis 0", axis=0, ways=((False, True), (True, True)), **ALL)


def test_distance(ctx):
    lib = _lib.load()
    # a cluster across a tile boundary: two lines of TILE - 30 and the peaks of the second straddle flat element TILE
    x = noise(21, (2, TILE - 30), step=0.5)
    assert check(ctx, x, "tile boundary d 9", distance=9, height=OPEN) > 100
    assert check(ctx, x, "tile boundary d 2.5", ways=((False, True),), distance=2.5) > 100
    # d larger than n: one survivor per line
    x = noise(22, (5, 300))
    assert check(ctx, x, "d > n", distance=1000.0, height=OPEN) == 5
    # distance = 1 removes nothing
    assert check(ctx, x, "d 1", distance=1) == len(O.tensor(x, -1)[0])
    # all heights equal: the larger index is visited first
    x = np.zeros((2, 9), np.float32)
    x[:, 1::2] = 2.0
    check(ctx, x, "ties", distance=3)
    peaks, _, _ = call(ctx, x[0], True, distance=3)
    assert peaks["indices"][:2, 0].tolist() == [3, 7] and int(peaks["valid_indices"]) == 2
    x = np.zeros((3, 2 * B + 1), np.float64)
    x[:, 1::2] = 1.0
    check(ctx, x, "ties long", distance=B - 1.5)
    # the many-round case: 2000 peaks at spacing 2, descending and ascending, d = 3: about one round per two peaks
    n = 4002
    for name, heights in (("descending", np.arange(2000, 0, -1)), ("ascending", np.arange(1, 2001))):
        x = np.zeros((1, n), np.float32)
        x[0, 1:n - 1:2] = heights
        assert check(ctx, x, f"chain {name}", distance=3, height=OPEN) == 1000
        rounds = lib.nxsig_find_peaks_rounds()
        print(f"find-peaks-rounds chain {name}: {rounds}")
        assert 1000 <= rounds <= 1001
    x = noise(23, (4, 3000), step=1e-3)
    check(ctx, x, "noise d 48", ways=((False, True),), distance=48)
    print(f"find-peaks-rounds noise 4 x 3000, d 48: {lib.nxsig_find_peaks_rounds()}")
    assert 1 <= lib.nxsig_find_peaks_rounds() <= 40


def test_the_nan_inf_row_of_the_fixture_on_the_device(ctx):
    x = np.array([0, 1, 0, np.nan, 0, 3, 0, np.inf, 0, 1, 0.5, 2, 0], np.float64)
    for dtype in (np.float64, np.float32):
        assert check(ctx, x.astype(dtype)[None, :], "nan inf", height=0, threshold=0, prominence=0, width=0) == 5
    rows = noise(31, (3, 3 * B + 5), np.float64)
    rows[0, ::17], rows[1, 5::40], rows[2, B] = np.nan, np.inf, -np.inf
    check(ctx, rows, "nan inf rows", distance=2, **ALL)


def test_max_peaks(ctx):
    x = noise(41, (3, 3 * B + 5))
    total = len(O.tensor(x, -1)[0])
    assert total > 40
    for k in (1, 7, total - 1, total, total + 5):
        assert check(ctx, x, f"max_peaks {k}", max_peaks=k, distance=2, **ALL) <= total


def test_two_runs_and_two_tiers_give_the_same_bits(ctx):
    x = noise(51, (8, 5 * TILE + 77), step=1e-2)
    opts = dict(distance=7.5, prominence=(0.3, None), width=1, wlen=101, rel_height=0.7, max_peaks=20000)
    runs = []
    for generic in (False, False, True):
        with Tier(ctx, generic):
            runs.append(call(ctx, x, True, **opts))
    assert [r[2] for r in runs] == [TABLES, TABLES, GENERIC]
    valid = int(runs[0][0]["valid_indices"])
    assert 1000 < valid < 20000
    for peaks, props, _ in runs[1:]:
        assert int(peaks["valid_indices"]) == valid and np.array_equal(peaks["indices"], runs[0][0]["indices"])
        assert all(same(props[k], runs[0][1][k]) for k in props) and list(props) == list(runs[0][1])
    # and the oracle, one row of it
    ref, rprops = O.line(x[3], **{k: v for k, v in opts.items() if k != "max_peaks"})
    idx = runs[0][0]["indices"][:valid]
    mine = idx[:, 0] == 3
    assert np.array_equal(idx[mine, 1], ref) and all(same(runs[0][1][k][:valid][mine], rprops[k].astype(runs[0][1][k].dtype)) for k in rprops)


def test_real_context_error_table(ctx):
    with open(P.GOLDEN_PEAKS) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.PEAKS_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_find_peaks"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] == _lib.ERR_INVALID_ARG for k, r in rows.items() if k != "valid")


def arena_call(ctx, x, capacity, want, conditions, bounds, distance=1.0, wlen=-1, rel_height=0.5):
    """nxsig_find_peaks itself on device arenas with guard words: (indices, valid, fprops, iprops) images checked, tensors returned"""
    lib = _lib.load()
    nf, ni = bin(want & 0xFF).count("1"), bin(want >> 8).count("1")
    xin = E.Arena("x", x.dtype, 1, x.size, data=x).upload(ctx)
    idx = E.Arena("indices", np.int32, capacity, x.ndim).upload(ctx)
    val = E.Arena("valid", np.uint32, 1, 1).upload(ctx)
    fp = E.Arena("fprops", np.float64, nf, capacity).upload(ctx)
    ip = E.Arena("iprops", np.int32, ni, capacity).upload(ctx)
    sh = (C.c_int64 * x.ndim)(*x.shape)
    b = np.ascontiguousarray(bounds, np.float64)
    fn = lambda h, *a: lib.nxsig_find_peaks(_lib.ctx_ptr(h, _lib._ctx_peaks), *a)   # noqa: E731
    E.call(ctx, fn, xin.ptr, _lib.DT_F64 if x.dtype == np.float64 else _lib.DT_F32, sh, x.ndim, x.ndim - 1, b.ctypes.data_as(C.POINTER(C.c_double)),
           conditions, distance, wlen, rel_height, capacity, want, idx.ptr, val.ptr, fp.ptr, ip.ptr, _lib.DEVICE)
    found = E.unchanged_findings(xin, xin.download())
    images = {a.name: a.download() for a in (idx, val, fp, ip)}
    for a in (idx, val, fp, ip):
        found += E.guard_findings(a, images[a.name])
    assert not found, "\n".join(found)
    return idx.tensor(images["indices"]), int(val.tensor(images["valid"])[0, 0]), fp.tensor(images["fprops"]), ip.tensor(images["iprops"])


def test_extents_of_every_result(ctx):
    x = noise(61, (3, 3 * B + 5))
    bounds = np.array([[-np.inf, np.inf]] * 5)
    coords, ref = O.tensor(x, -1, distance=2, **ALL)
    total, most = len(coords), 3 * ((3 * B + 4) // 2)
    want, cond = (1 << 13) - 1, 63
    for generic in (False, True):
        with Tier(ctx, generic):
            for capacity in (most, total, 5, 1):
                idx, valid, fp, ip = arena_call(ctx, x, capacity, want, cond, bounds, distance=2.0)
                k = min(total, capacity)
                assert valid == total and np.array_equal(idx[:k], coords[:k]) and (idx[k:] == -1).all()
                for r, name in enumerate(O.F64_PROPS):
                    assert same(fp[r, :k], ref[name][:k]) and np.isnan(fp[r, k:]).all(), (name, capacity)
                for r, name in enumerate(O.S32_PROPS):
                    assert np.array_equal(ip[r, :k], ref[name][:k]) and (ip[r, k:] == -1).all(), (name, capacity)
    # a single wanted row of each kind: the rows are packed in bit order
    idx, valid, fp, ip = arena_call(ctx, x, most, (1 << 3) | (1 << 12), 1 | 16, bounds)
    coords, ref = O.tensor(x, -1, plateau_size=OPEN, prominence=OPEN)
    assert valid == len(coords) and same(fp[0, :valid], ref["prominences"]) and np.array_equal(ip[0, :valid], ref["plateau_sizes"])
