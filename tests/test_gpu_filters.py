"""Filters.median / wiener on the MI355X: the reference's literals, random parity with tests/filters_oracle.py
on every tier, tier equivalence against the generic kernels, special values, device-resident calls, the dispatch record, run-to-run
determinism of the estimated noise, one input over 2^31 bytes, and one throughput floor per tier.

Median is exact (==).  Wiener with a given noise is bit-identical to the oracle; with noise: nil the estimate's sum runs in a fixed
order that differs from the oracle's sequential one, so its outputs are held to 1e-12 (f64, normalised) / 1 ulp (f32)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import filters_oracle as F
import nx_signal_amd as S
from nx_signal_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "filters_vectors.json")) as f:
        return json.load(f)


def _rand(shape, dtype, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


def _median_eq(got, exp):
    """exact, NaN where the oracle has NaN, and no -0.0"""
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got, exp, equal_nan=True)
    assert not np.any(np.signbit(got) & (got == 0))


# ---- the reference's literals ----
def test_median_literals(ctx, vectors):
    for v in vectors["median"]:
        got = S.filters.median(np.array(v["input"], np.int64), ctx=ctx, kernel_shape=tuple(v["kernel_shape"]))
        assert got.dtype == np.float32
        assert np.array_equal(got, np.array(v["expect"], np.float32)), v["name"]


def test_wiener_literals(ctx, vectors):
    for v in vectors["wiener"]:
        dt = np.float64 if v["dtype"] == "f64" else np.float32
        ks = v["kernel_size"] if isinstance(v["kernel_size"], int) else tuple(v["kernel_size"])
        got = S.filters.wiener(np.array(v["input"], dt), ctx=ctx, kernel_size=ks, noise=v["noise"])
        assert _same_bits(got, np.array(v["expect"], dt)), v["name"]


# ---- random parity, every tier ----
ROWS_SHAPE = (8, 48000 * 10)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 9, 15, 31])
def test_median_rows_parity(ctx, k):
    x = _rand(ROWS_SHAPE, np.float32, k)
    got = S.filters.median(x, ctx=ctx, kernel_shape=(1, k))
    assert ctx.last_dispatch() == "median.rows"
    _median_eq(got, F.median(x, (1, k)))


@pytest.mark.parametrize("k", [4, 9, 31])
def test_median_rows_parity_f64_and_rank1(ctx, k):
    x = _rand((3, 50001), np.float64, 100 + k)
    _median_eq(S.filters.median(x, ctx=ctx, kernel_shape=(1, k)), F.median(x, (1, k)))
    y = _rand((77777,), np.float32, 200 + k)
    got = S.filters.median(y, ctx=ctx, kernel_shape=(k,))
    assert ctx.last_dispatch() == "median.rows"
    _median_eq(got, F.median(y, (k,)))


@pytest.mark.parametrize("kh,kw", [(3, 3), (4, 4), (5, 5), (7, 7), (2, 7), (7, 1)])
def test_median_plane_parity(ctx, kh, kw):
    x = _rand((4, 512, 700), np.float32, kh * 10 + kw)
    got = S.filters.median(x, ctx=ctx, kernel_shape=(1, kh, kw))
    assert ctx.last_dispatch() == "median.plane"
    _median_eq(got, F.median(x, (1, kh, kw)))


@pytest.mark.parametrize("kh,kw", [(3, 3), (6, 5), (7, 7)])
def test_median_plane_parity_f64(ctx, kh, kw):
    x = _rand((2, 133, 301), np.float64, kh * 10 + kw)
    _median_eq(S.filters.median(x, ctx=ctx, kernel_shape=(1, kh, kw)), F.median(x, (1, kh, kw)))


@pytest.mark.parametrize("shape,ks", [((20, 30, 40), (3, 3, 3)), ((16, 9, 33), (2, 1, 5)), ((5, 6, 7), (5, 6, 7)), ((1001,), (1001,)),
                                      ((64, 40), (32, 2)), ((3, 4, 5, 6), (2, 2, 2, 2))])
def test_median_generic_parity(ctx, shape, ks):
    for dt in (np.float32, np.float64):
        x = _rand(shape, dt, len(shape))
        got = S.filters.median(x, ctx=ctx, kernel_shape=ks)
        assert ctx.last_dispatch() == "median.generic"
        _median_eq(got, F.median(x, ks))


def test_median_integer_input(ctx):
    x = np.random.default_rng(5).integers(-1000, 1000, (37, 41))
    _median_eq(S.filters.median(x, ctx=ctx, kernel_shape=(4, 3)), F.median(x, (4, 3)))


WIENER = [((3, 200, 300), 3), ((3, 200, 300), 5), ((3, 200, 300), (1, 2, 3)), ((200, 300), (2, 3)), ((10000,), 7), ((12, 20, 30), 3),
          ((6, 7, 8, 9), (2, 3, 1, 2))]


def _wiener_close(got, exp, dt):
    if dt == np.float64:
        err = np.max(np.abs(got - exp)) / max(1e-300, np.max(np.abs(exp)))
        assert err <= 1e-12, err
    else:
        ulp = np.abs(got.view(np.int32).astype(np.int64) - exp.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()


@pytest.mark.parametrize("case", range(len(WIENER)))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_wiener_parity(ctx, case, dt):
    shape, ks = WIENER[case]
    x = _rand(shape, dt, case) * 3 + np.linspace(0, 5, int(np.prod(shape))).reshape(shape).astype(dt)
    for noise in (0.5, 2, 0):
        got = S.filters.wiener(x, ctx=ctx, kernel_size=ks, noise=noise)
        assert _same_bits(got, F.wiener(x, ks, noise)), (shape, ks, noise)
    got, used = S.filters.wiener(x, ctx=ctx, kernel_size=ks, return_noise=True)
    exp, noise = F.wiener(x, ks, None, return_noise=True)
    assert abs(used - noise) <= 1e-12 * abs(noise)
    _wiener_close(got, exp, dt)


# ---- tier equivalence: the fast tiers and the switched-off generic tier give the same bits ----
@pytest.mark.parametrize("kind,shape,ks,dt", [
    ("median", (4, 20011), (1, 9), np.float32), ("median", (2, 5003), (1, 30), np.float64), ("median", (3, 97, 211), (1, 5, 5), np.float32),
    ("median", (2, 61, 83), (1, 7, 6), np.float64), ("wiener", (3, 97, 211), (1, 5, 5), np.float32), ("wiener", (2, 61, 83), (1, 3, 4), np.float64),
])
def test_tier_equivalence(ctx, kind, shape, ks, dt):
    x = _rand(shape, dt, 7)
    x[0, 0, ...] = np.nan
    x.reshape(-1)[5::97] = -0.0
    fn = (lambda: S.filters.median(x, ctx=ctx, kernel_shape=ks)) if kind == "median" else (lambda: S.filters.wiener(x, ctx=ctx, kernel_size=ks))
    fast = fn()
    assert ctx.last_dispatch() != f"{kind}.generic"
    ctx.set_tuning("DISABLE_FILTER_TILES", 1)
    try:
        slow = fn()
        assert ctx.last_dispatch() == f"{kind}.generic"
    finally:
        ctx.clear_tuning("DISABLE_FILTER_TILES")
    assert _same_bits(fast, slow)


# ---- special values ----
@pytest.mark.parametrize("ks", [(1, 3), (1, 4), (3, 3), (2, 2), (2, 3, 2)])
def test_median_special_values(ctx, ks):
    rng = np.random.default_rng(11)
    x = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 2.5], np.float32), size=(4, 30, 40))
    x.reshape(-1)[::7] = rng.standard_normal(x.size // 7 + 1).astype(np.float32)[: x.reshape(-1)[::7].size]
    ks3 = (1,) * (3 - len(ks)) + ks
    for dt in (np.float32, np.float64):
        _median_eq(S.filters.median(x.astype(dt), ctx=ctx, kernel_shape=ks3), F.median(x.astype(dt), ks3))


def test_median_nan_only_at_the_middle_rank(ctx):
    x = np.array([1.0, np.nan, 3.0, np.nan, np.nan, 2.0, 5.0], np.float32)
    got = S.filters.median(x, ctx=ctx, kernel_shape=(3,))
    # windows from 0, 1, 2, 3, 4, 4, 4: [1 N 3] -> 3, [N 3 N] -> N, [3 N N] -> N, [N N 2] -> N, [N 2 5] -> 5
    assert np.array_equal(got, np.array([3.0, np.nan, np.nan, np.nan, 5.0, 5.0, 5.0], np.float32), equal_nan=True)
    even = S.filters.median(np.array([-0.0, 0.0, np.inf, -np.inf], np.float32), ctx=ctx, kernel_shape=(2,))
    # [-0 0] -> +0, [0 Inf] -> Inf, [Inf -Inf] -> NaN (the mean), the last window is the one before
    assert np.array_equal(even, np.array([0.0, np.inf, np.nan, np.nan], np.float32), equal_nan=True) and not np.signbit(even[0])


def test_wiener_zero_variance_is_nan(ctx):
    """a constant window gives l_var = 0; with noise 0 (given, or the estimate of the zero tensor) the formula is 0 / 0"""
    for dt in (np.float32, np.float64):
        assert np.all(np.isnan(S.filters.wiener(np.zeros((5, 6), dt), ctx=ctx)))
        got = S.filters.wiener(np.full((6, 7), -1.5, dt), ctx=ctx, kernel_size=3, noise=0)
        assert np.all(np.isnan(got[1:-1, 1:-1])) and not np.any(np.isnan(got[0]))
        assert np.all(np.isnan(S.filters.wiener(np.full((40,), 2.0, dt), ctx=ctx, kernel_size=1)))


# ---- device-resident ----
def test_device_resident(ctx):
    x = _rand((3, 129, 257), np.float32, 3)
    xd = ctx.to_device(x)
    m = S.filters.median(xd, kernel_shape=(1, 3, 3))
    assert isinstance(m, S.DeviceBuffer) and m.dtype == np.float32 and m.shape == x.shape
    _median_eq(m.numpy(), F.median(x, (1, 3, 3)))
    for dt in (np.float32, np.float64):
        xd = ctx.to_device(x.astype(dt))
        w = S.filters.wiener(xd, kernel_size=(1, 3, 5), noise=0.25)
        assert isinstance(w, S.DeviceBuffer) and w.dtype == dt
        assert _same_bits(w.numpy(), F.wiener(x.astype(dt), (1, 3, 5), 0.25))
        w, used = S.filters.wiener(xd, kernel_size=(1, 3, 5), return_noise=True)
        exp, noise = F.wiener(x.astype(dt), (1, 3, 5), None, return_noise=True)
        assert abs(used - noise) <= 1e-12 * abs(noise)
        _wiener_close(w.numpy(), exp, dt)


# ---- dispatch ----
@pytest.mark.parametrize("kind,shape,ks,family", [
    ("median", (4, 1000), (1, 31), "median.rows"), ("median", (4, 1000), (1, 32), "median.generic"), ("median", (1000,), (5,), "median.rows"),
    ("median", (2, 3, 50, 60), (1, 1, 7, 7), "median.plane"), ("median", (50, 60), (8, 3), "median.generic"),
    ("median", (5, 50, 60), (2, 3, 3), "median.generic"), ("median", (50, 60), (3, 1), "median.plane"),
    ("wiener", (50, 60), (3, 3), "wiener.plane"), ("wiener", (1000,), (9,), "wiener.plane"), ("wiener", (5, 50, 60), (1, 15, 15), "wiener.plane"),
    ("wiener", (50, 60), (16, 3), "wiener.generic"), ("wiener", (5, 50, 60), (3, 3, 3), "wiener.generic"),
])
def test_dispatch_family(ctx, kind, shape, ks, family):
    x = _rand(shape, np.float32, 1)
    if kind == "median":
        S.filters.median(x, ctx=ctx, kernel_shape=ks)
    else:
        S.filters.wiener(x, ctx=ctx, kernel_size=ks, noise=0.1)
    assert ctx.last_dispatch() == family


# ---- determinism of the estimated noise ----
def test_wiener_estimate_is_deterministic(ctx):
    x = _rand((16, 1024, 1024), np.float32, 9)
    xd = ctx.to_device(x)
    a, na = S.filters.wiener(xd, kernel_size=(1, 3, 3), return_noise=True)
    b, nb = S.filters.wiener(xd, kernel_size=(1, 3, 3), return_noise=True)
    assert na == nb and _same_bits(a.numpy(), b.numpy())
    _, noise = F.wiener(x, (1, 3, 3), None, return_noise=True)
    assert abs(na - noise) <= 1e-12 * abs(noise)


# ---- one input over 2^31 bytes (64-bit indexing), spot-checked ----
def test_median_rows_over_2gib(ctx):
    n = (1 << 29) + 4099           # f32 elements: 2 GiB + 16 KiB in and out
    base = _rand((1 << 20,), np.float32, 21)
    xd = S.DeviceBuffer.empty(ctx, (n,), np.float32)
    lib = _lib.load()
    for off in range(0, n, 1 << 20):   # the input is the base row repeated
        m = min(1 << 20, n - off)
        _lib.check(lib.nxsig_upload(ctx.handle, C.c_void_p(xd.ptr + 4 * off), base.ctypes.data_as(C.c_void_p), 4 * m))
    k = 9
    yd = S.filters.median(xd, kernel_shape=(k,))
    assert ctx.last_dispatch() == "median.rows"
    for pos in (0, 12345, (1 << 29) - 3, (1 << 29) + 17, n - 64):
        got = np.empty(64, np.float32)
        _lib.check(lib.nxsig_download(ctx.handle, got.ctypes.data_as(C.c_void_p), C.c_void_p(yd.ptr + 4 * pos), 4 * 64))
        exp = np.empty(64, np.float32)
        for q in range(64):
            s = min(pos + q, n - k)
            w = base[np.arange(s, s + k) % (1 << 20)]
            exp[q] = np.sort(w)[k // 2]
        assert np.array_equal(got, exp), pos
    del xd, yd


# ---- throughput floors: (input + output bytes) / time over 8 TB/s, ~0.7 x the fraction measured on an MI355X
# (profiles/filters/floors_probe.txt: 0.381, 0.296, 0.0003, 0.135, 0.0078 with the box's copy at 0.65), scaled by this box's copy rate like
# test_gpu_dispatch_table.py
FLOORS = {
    "median.rows 8 x 60 s {1, 9}": ("median", (8, 48000 * 60), (1, 9), np.float32, "median.rows", 0.27),
    "median.plane 16 x 1024^2 3x3": ("median", (16, 1024, 1024), (1, 3, 3), np.float32, "median.plane", 0.21),
    "median.generic 64^3 {3,3,3}": ("median", (64, 64, 64), (3, 3, 3), np.float32, "median.generic", 0.0002),
    "wiener.plane 16 x 1024^2 3x3 f32 noise": ("wiener", (16, 1024, 1024), (1, 3, 3), np.float32, "wiener.plane", 0.094),
    "wiener.generic 64^3 {3,3,3} f64 noise": ("wiener", (64, 64, 64), (3, 3, 3), np.float64, "wiener.generic", 0.0055),
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
    kind, shape, ks, dt, family, floor = FLOORS[key]
    lib = _lib.load()
    xd = ctx.to_device(_rand(shape, dt, 2))
    r = len(shape)
    sh, kc = (C.c_int64 * r)(*shape), (C.c_int64 * r)(*ks)
    if kind == "median":
        yd = ctx.empty(shape, np.float32)
        fn = lambda: _lib.check(lib.nxsig_median_filter(ctx.handle, C.c_void_p(xd.ptr), int(dt == np.float64), sh, r, kc, C.c_void_p(yd.ptr), _lib.DEVICE))
    else:
        yd = ctx.empty(shape, dt)
        fn = lambda: _lib.check(lib.nxsig_wiener(ctx.handle, C.c_void_p(xd.ptr), int(dt == np.float64), sh, r, kc, 1, 0.5, C.c_void_p(yd.ptr), None,
                                                 _lib.DEVICE))
    for _ in range(5):
        fn()
    ctx.sync()
    assert ctx.last_dispatch() == family
    best = float("inf")
    for _ in range(2):
        ctx.timer_start()
        for _ in range(5):
            fn()
        best = min(best, ctx.timer_stop() / 5)
    frac = int(np.prod(shape)) * (np.dtype(dt).itemsize + yd.dtype.itemsize) / (best * 1e-3) / 8.0e12
    if PROBE:
        print(f"\nPROBE floor {key}: {frac:.4f} of 8 TB/s ({best:.4f} ms), copy {box_scale[1]:.3f}")
        return
    assert frac >= floor * box_scale[0], f"{key}: {frac:.3f} of 8 TB/s, floor {floor * box_scale[0]:.3f}"
