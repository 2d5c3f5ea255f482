"""PeakFinding on the MI355X: the reference's literals (custom comparators through nonzero), random parity with
tests/peaks_oracle.py over dtypes, ranks, axes, orders, comparators and special values, every tuned family against peaks.generic, the
dispatch record, device-resident calls, run-to-run identity, the all / none marked edges, one indices buffer over 2^31 bytes, the NIF
shim, and one throughput floor per family.  Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nx_signal_amd as S
import peaks_oracle as P
from nx_signal_amd import _lib
from test_peaks_host import check_literal, custom_comparator

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"
CMPS = ("less", "greater", "less_equal", "greater_equal")
FLOOR_ROWS, FLOOR_ROWS64, FLOOR_STRIDED, FLOOR_GENERIC, FLOOR_NONZERO = 0.22, 0.125, 0.22, 0.21, 0.24   # 0.7 x 0.312, 0.179, 0.319, 0.304, 0.347


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def run(ctx, x, cmp="less", axis=0, order=1):
    r = S.peak_finding.argrelextrema(x, cmp, ctx=ctx, axis=axis, order=order)
    return r["indices"], r["valid_indices"]


def same(got, exp):
    gi, gv = got
    ei, ev = exp
    assert gi.dtype == np.int32 and gi.shape == ei.shape
    assert np.asarray(gv).dtype == np.uint32 and np.asarray(gv).shape == ()
    assert int(gv) == int(ev)
    assert np.array_equal(gi, ei)


def special(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, shape).astype(dtype)
    if np.dtype(dtype).kind == "f":
        flat = x.reshape(-1)
        pick = rng.random(flat.size)
        flat[pick < 0.03] = np.nan
        flat[(pick >= 0.03) & (pick < 0.05)] = np.inf
        flat[(pick >= 0.05) & (pick < 0.07)] = -np.inf
        flat[(pick >= 0.07) & (pick < 0.12)] = -0.0
    return x


# ---- the reference's literals ----
def test_literals(ctx):
    with open(os.path.join(HERE, "golden", "peak_finding_vectors.json")) as f:
        vectors = json.load(f)["vectors"]
    for v in vectors:
        x = Nx_tensor(v["input"])
        if v["function"] == "argrelextrema":
            r = S.peak_finding.argrelextrema(x, custom_comparator(v["comparator"], x), ctx=ctx, **v["options"])
            assert ctx.last_dispatch() == "nonzero"
        else:
            r = getattr(S.peak_finding, v["function"])(x, ctx=ctx, **v["options"])
        check_literal(v, r["indices"], r["valid_indices"])


def Nx_tensor(values):
    return np.array(values)   # Nx.tensor of integer literals: s64


# ---- random parity with the oracle ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64, np.uint64, np.uint8, np.float16])
def test_parity_dtypes_ranks_axes(ctx, dtype):
    rng = np.random.default_rng(np.dtype(dtype).num)
    for rank in (1, 2, 3, 4):
        shape = tuple(int(v) for v in rng.integers(1, 12, rank))
        x = special(shape, dtype, rank) if np.dtype(dtype).kind == "f" else rng.integers(0, 5, shape).astype(dtype)
        for axis in list(range(rank)) + [-1, -rank]:
            for order in (0, 1, 2, 3, 7):
                for cmp in CMPS:
                    same(run(ctx, x, cmp, axis, order), P.argrelextrema(x, cmp, axis, order))


@pytest.mark.parametrize("order", [0, 1, 2, 3, 7, 8, 9, 64, 1000, 5000, 300000])
@pytest.mark.parametrize("shape,axis", [((4, 9000), 1), ((9000,), 0), ((3, 1500, 17), 1), ((2, 300, 40), 0), ((3, 5, 2001), -1)])
def test_parity_orders(ctx, order, shape, axis):
    x = special(shape, np.float32, order + len(shape))
    for cmp in CMPS:
        same(run(ctx, x, cmp, axis, order), P.argrelextrema(x, cmp, axis, order))


@pytest.mark.parametrize("dtype", [np.float64, np.int64, np.uint32])
@pytest.mark.parametrize("order", [1, 5, 40, 3000])
def test_parity_wide_types(ctx, dtype, order):
    rng = np.random.default_rng(order)
    for shape, axis in (((3, 20000), 1), ((2, 900, 40), 1)):
        x = rng.integers(0, 50, shape).astype(dtype)
        if dtype == np.int64:
            x = x + np.int64(1 << 60)   # differences below a double's resolution
        for cmp in ("less", "greater_equal"):
            same(run(ctx, x, cmp, axis, order), P.argrelextrema(x, cmp, axis, order))


# ---- tuned families against peaks.generic ----
FAMILIES = [((8, 50000), 1, "peaks.rows"), ((100000,), 0, "peaks.rows"), ((4, 2000, 96), 1, "peaks.strided"),
            ((300, 7, 5), 0, "peaks.strided")]


@pytest.mark.parametrize("shape,axis,family", FAMILIES)
@pytest.mark.parametrize("order", [1, 4, 8, 9, 50, 600])
def test_families_equal_generic(ctx, shape, axis, family, order):
    x = special(shape, np.float32, order)
    for cmp in CMPS:
        tuned = run(ctx, x, cmp, axis, order)
        assert ctx.last_dispatch() == family
        ctx.set_tuning("DISABLE_PEAK_TILES", 1)
        try:
            generic = run(ctx, x, cmp, axis, order)
            assert ctx.last_dispatch() == "peaks.generic"
        finally:
            ctx.clear_tuning("DISABLE_PEAK_TILES")
        same(tuned, generic)


def test_dispatch_of_each_shape(ctx):
    x = np.zeros((4, 5, 6), np.float32)
    for axis, family in ((2, "peaks.rows"), (-1, "peaks.rows"), (1, "peaks.strided"), (0, "peaks.strided")):
        run(ctx, x, "less", axis)
        assert ctx.last_dispatch() == family
    S.peak_finding.nonzero(np.ones(3), ctx=ctx)
    assert ctx.last_dispatch() == "nonzero"


# ---- device-resident calls ----
def test_device_resident(ctx):
    x = special((6, 10000), np.float64, 3)
    dx = S.DeviceBuffer.from_numpy(ctx, x)
    for fn, cmp in ((S.peak_finding.argrelmin, "less"), (S.peak_finding.argrelmax, "greater")):
        r = fn(dx, axis=1, order=5)
        assert isinstance(r["indices"], S.DeviceBuffer) and isinstance(r["valid_indices"], S.DeviceBuffer)
        assert r["valid_indices"].shape == () and r["valid_indices"].dtype == np.uint32
        same((r["indices"].numpy(), r["valid_indices"].numpy()), P.argrelextrema(x, cmp, 1, 5))
    with pytest.raises(_lib.ArgumentError):
        S.peak_finding.argrelextrema(dx, lambda a, b: a < b)


# ---- determinism and edges ----
def test_run_to_run_identity(ctx):
    x = special((16, 100000), np.float32, 4)
    first = run(ctx, x, "greater", 1, 3)
    for _ in range(3):
        same(run(ctx, x, "greater", 1, 3), first)


def test_none_and_all_marked(ctx):
    x = np.ones((7, 1000), np.float32)
    idx, valid = run(ctx, x, "less", 1, 2)
    assert int(valid) == 0 and np.all(idx == -1)
    idx, valid = run(ctx, x, "less_equal", 1, 2)
    assert int(valid) == x.size and not np.any(idx == -1)
    assert np.array_equal(idx, np.argwhere(np.ones(x.shape, bool)))
    idx, valid = run(ctx, np.arange(5000.0).reshape(50, 100), "greater", 0, 0)   # order 0 marks everything
    assert int(valid) == 5000 and np.array_equal(idx, np.argwhere(np.ones((50, 100), bool)))


def test_indices_over_2_gib(ctx):
    # 2^28 + 12345 elements of rank 2: an indices buffer of 2^31 + 98760 bytes
    rows, cols = 8, (1 << 25) + 12345 // 8 + 1
    x = np.zeros((rows, cols), np.uint8)
    x[:, 1::3] = 1   # every third column is a strict maximum: a third of the rows are marked
    dx = S.DeviceBuffer.from_numpy(ctx, x.astype(np.int32))
    del x
    r = S.peak_finding.argrelmax(dx, axis=1)
    assert r["indices"].nbytes > (1 << 31)
    expect = rows * len(range(1, cols - 1, 3))
    assert int(r["valid_indices"].numpy()) == expect
    idx = r["indices"].numpy()
    per_row = expect // rows
    for k in (0, 1, per_row - 1, per_row, expect // 2, expect - 1):
        assert idx[k].tolist() == [k // per_row, 1 + 3 * (k % per_row)]
    assert np.all(idx[expect:] == -1)


# ---- the NIF shim ----
def test_nif_shim(ctx):
    import nif_harness as N

    ok, nctx = N.call("ctx_create", 0)
    assert ok == "ok"
    x = special((5, 3000), np.float32, 11)
    ok, idx, valid = N.call("argrelextrema", nctx, x.tobytes(), _lib.DT_F32, list(x.shape), 1, 4, _lib.CMP_GREATER)
    assert ok == "ok"
    ei, ev = P.argrelextrema(x, "greater", 1, 4)
    assert valid == int(ev) and np.array_equal(np.frombuffer(idx, np.int32).reshape(ei.shape), ei)
    m = (x > 1).astype(np.uint8)
    ok, idx, valid = N.call("nonzero", nctx, m.tobytes(), list(m.shape))
    ei, ev = P.nonzero(m)
    assert ok == "ok" and valid == int(ev) and np.array_equal(np.frombuffer(idx, np.int32).reshape(ei.shape), ei)
    del nctx
    N.release_all()


# ---- one throughput floor per family: algorithmic bytes (input + 4 * rank * size + 4) / time over 8 TB/s, ~0.7 x the fraction measured
# on an MI355X (NXSIG_DISPATCH_PROBE=1 prints it: profiles/peaks/floors_probe.txt), scaled by this box's copy rate like
# test_gpu_filters.py
FLOORS = {
    "peaks.rows 8 x 60 s order 1": ((8, 48000 * 60), 1, 1, np.float32, "peaks.rows", FLOOR_ROWS),
    "peaks.rows 8 x 60 s order 64": ((8, 48000 * 60), 1, 64, np.float32, "peaks.rows", FLOOR_ROWS64),
    "peaks.strided [8, 11247, 512] axis 1 order 1": ((8, 11247, 512), 1, 1, np.float32, "peaks.strided", FLOOR_STRIDED),
    "peaks.generic 8 x 60 s order 1": ((8, 48000 * 60), 1, 1, np.float32, "peaks.generic", FLOOR_GENERIC),
    "nonzero 8 x 60 s": ((8, 48000 * 60), None, None, np.uint8, "nonzero", FLOOR_NONZERO),
}
HEALTHY_COPY = 0.70


@pytest.fixture(scope="module")
def box_scale(ctx):
    import time
    hip = C.CDLL("libamdhip64.so")
    n = 1 << 30
    a, b = ctx.empty((n,), np.uint8), ctx.empty((n,), np.uint8)
    for _ in range(3):
        hip.hipMemcpyDtoD(C.c_void_p(b.ptr), C.c_void_p(a.ptr), C.c_size_t(n))
    hip.hipDeviceSynchronize()
    best = 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(8):
            hip.hipMemcpyDtoD(C.c_void_p(b.ptr), C.c_void_p(a.ptr), C.c_size_t(n))
        hip.hipDeviceSynchronize()
        best = max(best, 8 * 2 * n / (time.perf_counter() - t0) / 8.0e12)
    del a, b
    return min(1.0, best / HEALTHY_COPY), best


@pytest.mark.parametrize("key", list(FLOORS))
def test_throughput_floor(ctx, box_scale, key):
    shape, axis, order, dt, family, floor = FLOORS[key]
    lib = _lib.load()
    rng = np.random.default_rng(2)
    x = rng.standard_normal(shape).astype(np.float32) if dt == np.float32 else (rng.random(shape) < 0.3).astype(np.uint8)
    xd = ctx.to_device(x)
    r, size = len(shape), int(np.prod(shape))
    sh = (C.c_int64 * r)(*shape)
    idx, valid = ctx.empty((size, r), np.int32), ctx.empty((), np.uint32)
    if family == "nonzero":
        fn = lambda: _lib.check(lib.nxsig_nonzero(ctx.handle, C.c_void_p(xd.ptr), sh, r, C.c_void_p(idx.ptr), C.c_void_p(valid.ptr), _lib.DEVICE))
    else:
        fn = lambda: _lib.check(lib.nxsig_argrelextrema(ctx.handle, C.c_void_p(xd.ptr), _lib.DT_F32, sh, r, axis, order, _lib.CMP_GREATER,
                                                        C.c_void_p(idx.ptr), C.c_void_p(valid.ptr), _lib.DEVICE))
    if family == "peaks.generic":
        ctx.set_tuning("DISABLE_PEAK_TILES", 1)
    try:
        for _ in range(3):
            fn()
        ctx.sync()
        assert ctx.last_dispatch() == family
        best = float("inf")
        for _ in range(2):
            ctx.timer_start()
            for _ in range(5):
                fn()
            best = min(best, ctx.timer_stop() / 5)
    finally:
        ctx.clear_tuning("DISABLE_PEAK_TILES")
    frac = (size * np.dtype(dt).itemsize + 4 * r * size + 4) / (best * 1e-3) / 8.0e12
    if PROBE:
        print(f"\nPROBE floor {key}: {frac:.4f} of 8 TB/s ({best:.4f} ms), copy {box_scale[1]:.3f}")
        return
    assert frac >= floor * box_scale[0], f"{key}: {frac:.3f} of 8 TB/s, floor {floor * box_scale[0]:.3f}"
