"""Waveforms on the MI355X: the reference's literals bit for bit, parity with tests/waveforms_oracle.py for every
function and chirp method in both tiers from host arrays, device buffers and a device view offset by one element, special values,
unit_impulse, determinism and the dispatch record, the NIF path, and one throughput floor per function.

Acceptance against the oracle.
  f32   equal bits are expected.  The device's double math library and the host's may differ in the last f64 bit, which can flip an f32
        rounding: an element may differ by at most 4 * 2^-23 * max(1, |phase|) (phase: the oracle's argument of the final cos / sin /
        exp; sawtooth: 4 f32 ulps of the output), and at most 1e-3 of a case's elements may differ in bits at all.
  f64   |got - oracle| <= K * 2^-52 * max(1, |phase|).  Kernel and oracle run the same IEEE operations (+ - * / fmod are exact to the
        last bit on both sides, no FMA contraction on either), so they can only part at a transcendental, by the two libraries' last
        bits.  K allows one unit for every rounded op of the function's longest chain and two for every transcendental in it:
          sawtooth 3 (fmod, the subtraction, the division), square exact,
          gaussian_pulse 8 (t t, (-a) x, exp 2 | w t, cos 2 | the product),
          chirp linear 9 (f0 t, pow 2, x 0.5 beta, +, x 2pi, + phi, cos 2), quadratic 10 (one more: / 3),
          quadratic vertex_zero: false 12 (t1 - t, pow 2, - t1^3, x beta, / 3, f1 t, +, x 2pi, + phi, cos 2),
          logarithmic 9 (t / t1, pow 2, - 1, x beta f0, x 2pi, + phi, cos 2), hyperbolic 9 (t / sp, 1 - x, log 2, x k, x 2pi, + phi, cos 2),
          polynomial_sweep of 3 coefficients 16 (3 pow 6, 3 products, 3 sums, x 2pi, + phi, cos 2).
        The parameters below keep the sums free of cancellation over [-50, 50] (their terms share a sign, or vanish together at 0) and
        the constant that multiplies a difference of a transcendental ((f1/f0)^(t/t1) - 1, (t1 - t)^3 - t1^3) below 2, so that one
        unit of a transcendental stays within one unit of max(1, |phase|)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nx_signal_amd as S
import waveforms_oracle as O
from nx_signal_amd import _lib
from nx_signal_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.environ.get("NXSIG_DISPATCH_PROBE") == "1"
W = S.waveforms
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 70001)

# name -> (function, positional arguments, options, K of the f64 bound, dispatch family)
CASES = {
    "sawtooth": ("sawtooth", (), {"width": 0.25}, 3, "waveform.sawtooth"),
    "sawtooth.width1": ("sawtooth", (), {}, 3, "waveform.sawtooth"),
    "sawtooth.width0": ("sawtooth", (), {"width": 0}, 3, "waveform.sawtooth"),
    "square": ("square", (), {"duty": 0.3}, 0, "waveform.square"),
    "gaussian_pulse": ("gaussian_pulse", (), {"center_frequency": 0.05, "bandwidth": 0.5}, 8, "waveform.gaussian_pulse"),
    "chirp.linear": ("chirp", (2.0, 40.0, 3.0), {"method": "linear", "phi": 0.3}, 9, "waveform.chirp.linear"),
    "chirp.quadratic": ("chirp", (1.0, 40.0, 3.0), {"method": "quadratic"}, 10, "waveform.chirp.quadratic"),
    "chirp.quadratic.t1": ("chirp", (-0.5, 2.0, 0.0), {"method": "quadratic", "vertex_zero": False}, 12, "waveform.chirp.quadratic"),
    "chirp.logarithmic": ("chirp", (0.05, 25.0, 4.75), {"method": "logarithmic"}, 9, "waveform.chirp.logarithmic"),
    "chirp.hyperbolic": ("chirp", (1.0, 40.0, 2.0), {"method": "hyperbolic", "phi": -1.0}, 9, "waveform.chirp.hyperbolic"),
    "polynomial_sweep": ("polynomial_sweep", ([0.002, 0.0, 0.5],), {"phi": 30, "phi_unit": "degrees"}, 16, "waveform.polynomial_sweep"),
}


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(HERE, "golden", "waveforms_vectors.json")) as f:
        return json.load(f)["cases"]


def draw(n, dtype, seed=0, around=0.0):
    """t from [-50, 50] (or around + [0, 50]); the same values for every case of a size"""
    rng = np.random.default_rng(1000 * seed + n)
    t = rng.uniform(-50.0, 50.0, n) if around == 0.0 else around + rng.uniform(0.0, 50.0, n)
    return t.astype(dtype)


def keep_off_the_square_threshold(t, duty):
    """square must be equal everywhere: move the elements whose tmod lies within a few ulps of the threshold (checked on the CPU)"""
    tmod, thr = O.square_parts(t, duty)
    near = np.abs(tmod - thr) <= 8 * np.spacing(np.abs(thr).astype(t.dtype)).astype(np.float64)
    t = t.copy()
    t[near] = 0.25
    tmod, thr = O.square_parts(t, duty)
    assert not np.any(np.abs(tmod - thr) <= 8 * np.spacing(np.abs(thr).astype(t.dtype)).astype(np.float64))
    return t


def to_host(a):
    if isinstance(a, dict):
        return {k: to_host(v) for k, v in a.items()}
    return a.numpy() if isinstance(a, DeviceBuffer) else a


def run(name, t, ctx, **more):
    fn, args, opts, _, _ = CASES[name]
    return getattr(W, fn)(t, *args, ctx=ctx, **{**opts, **more})


def oracle(name, t, **more):
    fn, args, opts, _, _ = CASES[name]
    return getattr(O, fn)(t, *args, **{**opts, **more})


def accept(name, got, want, phase, label):
    """the acceptance rule of the module docstring for one output tensor"""
    fn, _, _, K, _ = CASES[name]
    assert got.dtype == want.dtype and got.shape == want.shape, label
    if got.size == 0:
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    if got.dtype == np.int32:
        assert np.array_equal(got, want), label
        return
    g, w = got[~nan].astype(np.float64), want[~nan].astype(np.float64)
    scale = np.maximum(1.0, np.abs(np.where(np.isfinite(phase[~nan]), phase[~nan], 1.0))) if phase is not None else 1.0
    with np.errstate(invalid="ignore"):
        err = np.where(g == w, 0.0, np.abs(g - w))   # equal infinities are equal
    if got.dtype == np.float32:
        differ = got[~nan].view(np.uint32) != want[~nan].view(np.uint32)
        assert differ.mean() <= 1e-3 if differ.size else True, (label, float(differ.mean()))
        bound = 4 * np.spacing(np.abs(want[~nan])).astype(np.float64) if fn == "sawtooth" else 4 * 2.0 ** -23 * scale
    else:
        bound = K * 2.0 ** -52 * scale
    assert np.all(err <= bound), (label, float(np.max(err / bound)))


def accept_all(name, got, want, phase, label):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for k in want:
            accept(name, got[k], want[k], phase[k], f"{label} {k}")
    else:
        accept(name, got, want, phase, label)


# ---- the reference's literals ----
def test_literals_bit_for_bit(ctx, cases):
    from test_waveforms_host import check_case
    for c in cases:
        if c["fn"] == "unit_impulse":
            opts = dict(c["opts"])
            check_case(c, W.unit_impulse(tuple(c["shape"]), ctx=ctx, **opts))
            check_case(c, W.unit_impulse(tuple(c["shape"]), ctx=ctx, device=True, **opts).numpy())
            continue
        opts = dict(c["opts"])
        if isinstance(opts.get("duty"), list):
            opts["duty"] = np.asarray(opts["duty"], np.float32)
        args = [np.asarray(a) if isinstance(a, list) else a for a in c.get("args", [])]
        t = O.fixture_t(c["t"])
        check_case(c, getattr(W, c["fn"])(t, *args, ctx=ctx, **opts))
        if "duty" in opts and isinstance(opts["duty"], np.ndarray):
            opts["duty"] = ctx.to_device(opts["duty"])
        check_case(c, to_host(getattr(W, c["fn"])(ctx.to_device(t), *args, ctx=ctx, **opts)))


# ---- parity with the oracle ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_oracle(ctx, name, dtype):
    for n in SIZES:
        t = draw(n, dtype)
        if name == "square":
            t = keep_off_the_square_threshold(t, CASES[name][2]["duty"])
        want, phase = oracle(name, t)
        accept_all(name, run(name, t, ctx), want, phase, f"{name} host n={n}")
        assert ctx.last_dispatch() == (CASES[name][4] if n else "")
        accept_all(name, to_host(run(name, ctx.to_device(t), ctx)), want, phase, f"{name} device n={n}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_parity_around_1e6(ctx, dtype):
    t = draw(4099, dtype, seed=1, around=1.0e6)
    for name in CASES:
        tt = keep_off_the_square_threshold(t, CASES[name][2]["duty"]) if name == "square" else t
        want, phase = oracle(name, tt)
        accept_all(name, to_host(run(name, ctx.to_device(tt), ctx)), want, phase, f"{name} 1e6")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_device_view_offset_by_one_element(ctx, dtype):
    """input (and a tensor duty) start one element past a 16-byte boundary: the element-by-element loads give the same bits as the
    aligned call"""
    n = 4099
    t = draw(n + 1, dtype, seed=2)
    base = ctx.to_device(t)
    view = DeviceBuffer(ctx, base.ptr + t.itemsize, (n,), dtype, owner=False)
    assert view.ptr % 16 != 0
    for name in CASES:
        aligned = to_host(run(name, ctx.to_device(t[1:]), ctx))
        got = to_host(run(name, view, ctx))
        for k in (aligned if isinstance(aligned, dict) else {"": None}):
            a, g = (aligned[k], got[k]) if k else (aligned, got)
            assert a.tobytes() == g.tobytes(), (name, k)
    duty = np.random.default_rng(3).uniform(0.05, 0.95, n + 1).astype(dtype)
    dbase = ctx.to_device(duty)
    dview = DeviceBuffer(ctx, dbase.ptr + duty.itemsize, (n,), dtype, owner=False)
    got = W.square(view, ctx=ctx, duty=dview).numpy()
    assert np.array_equal(got, W.square(t[1:], ctx=ctx, duty=duty[1:]))
    del base, dbase


# ---- special values ----
SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -2.5, -1000.0, 3.0, 6.2831855, -6.2831855]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_special_values(ctx, dtype):
    t = np.array(SPECIAL, dtype)
    for name in CASES:
        want, phase = oracle(name, t)
        got = run(name, t, ctx)
        for k in (want if isinstance(want, dict) else {"": None}):
            w, g = (want[k], got[k]) if k else (want, got)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (name, k)
            if dtype == np.float32 or g.dtype == np.int32:
                assert g[~np.isnan(w)].tobytes() == w[~np.isnan(w)].tobytes(), (name, k, g, w)
            else:
                accept(name, g, w, phase[k] if k else phase, f"{name} special {k}")
    # sawtooth(-1.0) lies below -1: Nx.remainder keeps the dividend's sign
    assert W.sawtooth(np.array([-1.0], dtype), ctx=ctx)[0] < -1


def test_options_and_branches(ctx, cases):
    t = draw(257, np.float32, seed=4)
    # f0 == f1 of both special-cased methods, and f0 f1 <= 0 with :logarithmic
    for method in ("logarithmic", "hyperbolic"):
        want, _ = O.chirp(t, 3.0, 7.0, 3.0, method=method, phi=0.5)
        got = W.chirp(t, 3.0, 7.0, 3.0, ctx=ctx, method=method, phi=0.5)
        assert (got.view(np.uint32) != want.view(np.uint32)).mean() <= 1e-3 and np.max(np.abs(got - want)) < 1e-3
        assert ctx.last_dispatch() == f"waveform.chirp.{method}"
    for f0, f1 in ((-1.0, 2.0), (0.0, 2.0), (2.0, 0.0)):
        got = W.chirp(t, f0, 7.0, f1, ctx=ctx, method="logarithmic")
        assert got.dtype == np.float32 and np.isnan(got).all()
    # phi in degrees and in radians
    a = W.polynomial_sweep(t, [1, 0], ctx=ctx, phi=180, phi_unit="degrees")
    want, _ = O.polynomial_sweep(t, [1, 0], phi=180, phi_unit="degrees")
    assert (a.view(np.uint32) != want.view(np.uint32)).mean() <= 1e-3
    assert not np.array_equal(a, W.polynomial_sweep(t, [1, 0], ctx=ctx, phi=180))
    # 32 coefficients are accepted
    c32 = np.zeros(32)
    c32[-2:] = (1.0, 0.5)
    want, arg = O.polynomial_sweep(t[:16] / 50, c32)
    got = W.polynomial_sweep(t[:16] / 50, c32, ctx=ctx)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 4 * 2.0 ** -23 * np.maximum(1, np.abs(arg)))
    # integer t is read as f32; a duty tensor of t's shape (the reference's fourth square doctest is among the literals)
    assert W.sawtooth(np.arange(7), ctx=ctx).dtype == np.float32
    assert np.array_equal(W.sawtooth(np.arange(7), ctx=ctx), W.sawtooth(np.arange(7, dtype=np.float32), ctx=ctx))
    duty = np.random.default_rng(5).uniform(0.05, 0.95, t.size).astype(np.float32)
    tmod, thr = O.square_parts(t, duty)
    ok = np.abs(tmod - thr) > 1e-5
    assert np.array_equal(W.square(t, ctx=ctx, duty=duty)[ok], O.square(t, duty)[0][ok])
    x2 = W.square(t.reshape(1, 257), ctx=ctx, duty=0.5)
    assert x2.shape == (1, 257) and x2.dtype == np.int32


# ---- unit_impulse ----
@pytest.mark.parametrize("ty", ["f32", "f64", "s32", "s64", "u32", "u64"])
def test_unit_impulse(ctx, ty):
    dt = {"f32": np.float32, "f64": np.float64, "s32": np.int32, "s64": np.int64, "u32": np.uint32, "u64": np.uint64}[ty]
    checks = [((7,), 0), ((7,), 6), ((7,), 3), ((1,), 0), ((70001,), 70000), ((70001,), "midpoint"), ((3, 5), "midpoint"), ((3, 5), [2, 3]),
              ((3, 5), [[2, 4]]), ((3, 5), [0, 0]), ((2, 1, 3, 1, 2, 2, 1, 3), "midpoint"), ((2, 1, 3, 1, 2, 2, 1, 3), [1, 0, 2, 0, 1, 1, 0, 2]),
              ((2, 1, 3, 1, 2, 2, 1, 3), [0] * 8)]
    for shape, index in checks:
        want, _ = O.unit_impulse(shape, index, dt)
        got = W.unit_impulse(shape, ctx=ctx, index=index, type=ty)
        assert got.dtype == dt and got.shape == shape and got.tobytes() == want.tobytes(), (shape, index)
        assert got.sum() == 1
        dev = W.unit_impulse(shape, ctx=ctx, device=True, index=np.asarray(index) if not isinstance(index, str) else index, type=dt)
        assert isinstance(dev, DeviceBuffer) and dev.numpy().tobytes() == want.tobytes(), (shape, index)
    assert ctx.last_dispatch() == "waveform.unit_impulse"
    for shape in ((0,), (3, 0), (0, 4)):
        e = W.unit_impulse(shape, ctx=ctx, type=ty, index="midpoint")
        assert e.shape == shape and e.dtype == dt and e.size == 0
        assert W.unit_impulse(shape, ctx=ctx, type=ty, device=True, index="midpoint").shape == shape


def test_unit_impulse_into_an_offset_view(ctx):
    """the C entry point on a device pointer that is only element-aligned: head, body and tail, nothing outside"""
    lib = _lib.load()
    for dt, code in ((np.float32, _lib.DT_F32), (np.int64, _lib.DT_S64)):
        n = 1031
        buf = ctx.to_device(np.full(n + 4, 7, dt))
        sh, ix = (C.c_int64 * 1)(n), (C.c_int64 * 1)(n - 1)
        _lib.check(lib.nxsig_unit_impulse(ctx.handle, code, sh, 1, ix, C.c_void_p(buf.ptr + np.dtype(dt).itemsize), _lib.DEVICE))
        got = buf.numpy()
        want = np.full(n + 4, 7, dt)
        want[1:n + 1] = 0
        want[n] = 1
        assert np.array_equal(got, want)


# ---- determinism, dispatch, aliasing ----
def test_determinism_dispatch_and_outputs_do_not_alias(ctx):
    t = draw(70001, np.float32, seed=6)
    td = ctx.to_device(t)
    for name, (_, _, _, _, family) in CASES.items():
        a = to_host(run(name, td, ctx))
        assert ctx.last_dispatch() == family
        b = to_host(run(name, td, ctx))
        for k in (a if isinstance(a, dict) else {"": None}):
            assert (a[k] if k else a).tobytes() == (b[k] if k else b).tobytes(), name
    g = W.gaussian_pulse(td, ctx=ctx, center_frequency=0.05)
    spans = sorted((v.ptr, v.ptr + v.nbytes) for v in g.values())
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(2))
    h = W.gaussian_pulse(t, ctx=ctx, center_frequency=0.05)
    assert not any(np.shares_memory(h[a], h[b]) for a in h for b in h if a != b)
    assert not np.array_equal(h["in_phase"], h["quadrature"]) and np.array_equal(h["envelope"], g["envelope"].numpy())


# ---- through the NIF ----
def test_through_the_nif(ctx):
    import nif_harness as H
    t = draw(1027, np.float32, seed=7)
    t64 = draw(515, np.float64, seed=8)
    ok, nctx = H.call("ctx_create", 0)
    assert ok == "ok"
    f32 = lambda b: np.frombuffer(b, np.float32)
    ok, b = H.call("sawtooth", nctx, t, 0, 0.25)
    assert ok == "ok" and f32(b).tobytes() == W.sawtooth(t, ctx=ctx, width=0.25).tobytes()
    ok, b = H.call("sawtooth", nctx, t64, 1, 1)
    assert np.frombuffer(b, np.float64).tobytes() == W.sawtooth(t64, ctx=ctx).tobytes()
    ok, b = H.call("square", nctx, t, 0, 0.3, b"")
    assert np.array_equal(np.frombuffer(b, np.int32), W.square(t, ctx=ctx, duty=0.3))
    duty = np.random.default_rng(9).uniform(0, 1, t.size).astype(np.float32)
    ok, b = H.call("square", nctx, t, 0, 0.0, duty)
    assert np.array_equal(np.frombuffer(b, np.int32), W.square(t, ctx=ctx, duty=duty))
    ok, e, yi, yq = H.call("gaussian_pulse", nctx, t, 0, 0.05, 0.5, -6)
    want = W.gaussian_pulse(t, ctx=ctx, center_frequency=0.05)
    assert [f32(x).tobytes() for x in (e, yi, yq)] == [want[k].tobytes() for k in ("envelope", "in_phase", "quadrature")]
    for code, method in enumerate(("linear", "quadratic", "logarithmic", "hyperbolic")):
        ok, b = H.call("chirp", nctx, t, 0, (0.05, 25.0, 4.75), code, 0, 0.25)
        assert f32(b).tobytes() == W.chirp(t, 0.05, 25.0, 4.75, ctx=ctx, method=method, vertex_zero=False, phi=0.25).tobytes(), method
    ok, b = H.call("polynomial_sweep", nctx, t, 0, np.array([0.002, 0.0, 0.5]), 30, 1)
    assert f32(b).tobytes() == W.polynomial_sweep(t, [0.002, 0.0, 0.5], ctx=ctx, phi=30, phi_unit="degrees").tobytes()
    ok, b = H.call("unit_impulse", nctx, 2, [3, 5], [1, 2])
    assert np.array_equal(np.frombuffer(b, np.int32).reshape(3, 5), W.unit_impulse((3, 5), ctx=ctx, type="s32", index="midpoint"))
    ok, b = H.call("unit_impulse", nctx, 1, [3, 0], [0, 0])
    assert ok == "ok" and b == b""
    # the library's ArgumentErrors arrive as {:error, {-1, message}}
    for args in (("sawtooth", nctx, t, 0, 1.5), ("gaussian_pulse", nctx, t, 0, -1.0, 0.5, -6), ("chirp", nctx, t, 0, (1.0, 1.0, 2.0), 4, 1, 0),
                 ("polynomial_sweep", nctx, t, 0, b"", 0, 0), ("polynomial_sweep", nctx, t, 0, np.zeros(33), 0, 0), ("unit_impulse", nctx, 0, [3], [3])):
        with pytest.raises(H.NifError) as err:
            H.call(*args)
        assert err.value.code == -1, args[0]
    with pytest.raises(H.BadArg):
        H.call("sawtooth", nctx, b"abc", 0, 1)
    with pytest.raises(H.BadArg):
        H.call("square", nctx, t, 0, 0.5, duty[:5])


# ---- throughput floors: (input + output bytes) / time over 8 TB/s for 2^26 f32 elements on device buffers, half of the fraction
# measured on an MI355X (profiles/waveforms/floors_probe.txt: 0.415, 0.642, 0.339, 0.120, 0.117, 0.054, 0.609 with the box's copy at
# 0.69), scaled by this box's copy rate like test_gpu_filters.py
FLOORS = {
    "sawtooth": 0.21,
    "square": 0.32,
    "gaussian_pulse": 0.17,
    "chirp.linear": 0.06,
    "chirp.logarithmic": 0.058,
    "polynomial_sweep": 0.027,
    "unit_impulse": 0.3,
}
HEALTHY_COPY = 0.70
FLOOR_N = 1 << 26


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


@pytest.fixture(scope="module")
def floor_t(ctx):
    return ctx.to_device(np.random.default_rng(10).uniform(-50.0, 50.0, FLOOR_N).astype(np.float32))


@pytest.mark.parametrize("key", list(FLOORS))
def test_throughput_floor(ctx, box_scale, floor_t, key):
    if key == "unit_impulse":
        fn = lambda: W.unit_impulse((FLOOR_N,), ctx=ctx, device=True, index="midpoint")
        nbytes, family = 4 * FLOOR_N, "waveform.unit_impulse"
    else:
        fn = lambda: run(key, floor_t, ctx)
        nbytes, family = 4 * FLOOR_N * (4 if key == "gaussian_pulse" else 2), CASES[key][4]
    for _ in range(3):
        fn()
    ctx.sync()
    assert ctx.last_dispatch() == family
    best = float("inf")
    for _ in range(2):
        ctx.timer_start()
        for _ in range(3):
            fn()
        best = min(best, ctx.timer_stop() / 3)
    frac = nbytes / (best * 1e-3) / 8.0e12
    if PROBE:
        print(f"\nPROBE floor waveform.{key} 2^26 f32: {frac:.4f} of 8 TB/s ({best:.4f} ms), copy {box_scale[1]:.3f}")
        return
    assert frac >= FLOORS[key] * box_scale[0], f"{key}: {frac:.4f} of 8 TB/s, floor {FLOORS[key] * box_scale[0]:.4f}"
