"""NumPy restatement of NxSignal.Waveforms (lib/nx_signal/waveforms.ex) under the numeric contract of DESIGN.md section 3.10.

f32 tier: every Nx op is evaluated in double on f32-rounded operands and rounded back to f32 (the BinaryBackend rule of SURVEY
Appendix A).  f64 tier (t is float64): the same expressions with no rounding.  pi() is the f32 constant in both tiers and 2 * pi() its
exact double.  Orderings that the reference's literals pin and a plain left-to-right reading does not:
  chirp :hyperbolic / :logarithmic   the factor 2 pi() multiplies last
  sawtooth                           width is an Elixir number: width + 1 and 1 - width are double arithmetic, and pi() * (that) is one
                                     op on the unrounded number (the width: 0.2 regression vector pins it)
  gaussian_pulse                     a = -f32((pi64 fc bw)^2) / (4 log(ref)) with the pi-only product folded in double;
                                     envelope = exp((-a) (t t))
Every function returns (values, phase): phase is the argument of the final cos / sin / exp (None where there is none), which the GPU
tests scale their bound by."""
import math

import numpy as np

PI = float(np.float32(math.pi))
TWO_PI = 2.0 * PI
CHIRP_METHODS = ("linear", "quadratic", "logarithmic", "hyperbolic")


def _tier(t):
    """(t as float64 values, rounding function, result dtype)"""
    a = np.asarray(t)
    if a.dtype == np.float64:
        return a, (lambda x: np.asarray(x, np.float64)), np.float64
    a = a.astype(np.float32).astype(np.float64)
    return a, (lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)), np.float32


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


@_quiet
def sawtooth(t, width=1):
    t, R, dt = _tier(t)
    w = float(width)   # an Elixir number: width + 1 and 1 - width are plain double arithmetic, and the number meets pi() unrounded
    tmod = R(np.fmod(t, TWO_PI))
    if width == 1:
        out = R(R(tmod / R(PI * w)) - 1.0)
    elif width == 0:
        out = R(R(R(PI * (w + 1.0)) - tmod) / R(PI * (1.0 - w)))
    else:
        rise = R(R(tmod / R(PI * w)) - 1.0)
        fall = R(R(R(PI * (w + 1.0)) - tmod) / R(PI * (1.0 - w)))
        out = np.where(tmod < R(TWO_PI * w), rise, fall)
    return out.astype(dt), None


@_quiet
def square_parts(t, duty=0.5):
    """(tmod, threshold) of square/2, as float64 values"""
    t, R, _ = _tier(t)
    d = R(np.asarray(duty, np.float64))
    return R(np.fmod(t, TWO_PI)), R(R(d * 2.0) * PI)


def square(t, duty=0.5):
    tmod, thr = square_parts(t, duty)
    return np.where(tmod < thr, 1, -1).astype(np.int32), None


def gaussian_scalars(R, fc, bw, bwr):
    """(-a, 2 pi() fc) as the kernels receive them"""
    ref = R(10.0 ** (bwr / 20.0))
    a = R(-R((math.pi * fc * bw) ** 2) / R(4.0 * R(math.log(ref))))
    return float(R(-a)), float(R(TWO_PI * R(fc)))


@_quiet
def gaussian_pulse(t, center_frequency=1000, bandwidth=0.5, bandwidth_reference_level=-6):
    t, R, dt = _tier(t)
    na, w = gaussian_scalars(R, center_frequency, bandwidth, bandwidth_reference_level)
    earg = R(na * R(t * t))
    env = R(np.exp(earg))
    yarg = R(w * t)
    out = {"envelope": env.astype(dt), "in_phase": R(env * R(np.cos(yarg))).astype(dt), "quadrature": R(env * R(np.sin(yarg))).astype(dt)}
    return out, {"envelope": earg, "in_phase": yarg, "quadrature": yarg}


@_quiet
def chirp_phase(t, f0, t1, f1, method="linear", vertex_zero=True):
    t, R, _ = _tier(t)
    f0, t1, f1 = float(R(f0)), float(R(t1)), float(R(f1))
    if method == "linear":
        beta = R(R(f1 - f0) / t1)
        return R(TWO_PI * R(R(f0 * t) + R(R(0.5 * beta) * R(np.power(t, 2.0)))))
    if method == "quadratic" and vertex_zero:
        beta = R(R(f1 - f0) / R(t1 ** 2))
        return R(TWO_PI * R(R(f0 * t) + R(R(beta * R(np.power(t, 3.0))) / 3.0)))
    if method == "quadratic":
        beta = R(R(f1 - f0) / R(t1 ** 2))
        return R(TWO_PI * R(R(f1 * t) + R(R(beta * R(R(np.power(R(t1 - t), 3.0)) - R(t1 ** 3))) / 3.0)))
    if method == "logarithmic":
        if f0 * f1 <= 0:
            return np.full(t.shape, np.nan)
        if f0 == f1:
            return R(R(TWO_PI * f0) * t)
        ratio = R(f1 / f0)
        beta = R(t1 / R(math.log(ratio)))
        return R(TWO_PI * R(R(beta * f0) * R(R(np.power(ratio, R(t / t1))) - 1.0)))
    if method == "hyperbolic":
        if f0 == f1:
            return R(R(TWO_PI * f0) * t)
        sp = R(R(R(-f1) * t1) / R(f0 - f1))
        return R(TWO_PI * R(R(R(-sp) * f0) * R(np.log(R(np.abs(R(1.0 - R(t / sp))))))))
    raise ValueError(method)


@_quiet
def chirp(t, f0, t1, f1, phi=0, vertex_zero=True, method="linear"):
    _, R, dt = _tier(t)
    arg = R(chirp_phase(t, f0, t1, f1, method, vertex_zero) + R(phi))
    return R(np.cos(arg)).astype(dt), arg


@_quiet
def polynomial_sweep(t, coefs, phi=0, phi_unit="radians"):
    """The dot product is summed in f64 and rounded once (a BinaryBackend dot); the reference's literals do not tell that from f32
    sequential accumulation."""
    t, R, dt = _tier(t)
    c = R(np.asarray(coefs, np.float64))
    n = len(c)
    acc = np.zeros(t.shape, np.float64)
    for k in range(n):
        acc = acc + R(c[k] / (n - k)) * R(np.power(t, float(n - k)))
    phase = R(acc)
    p = R(phi) if phi_unit == "radians" else R(float(phi) * PI / 180.0)   # constants fold in double
    arg = R(R(TWO_PI * phase) + p)
    return R(np.cos(arg)).astype(dt), arg


def unit_impulse(shape, index=0, dtype=np.float32):
    shape = tuple(shape)
    idx = tuple(n // 2 for n in shape) if isinstance(index, str) and index == "midpoint" else tuple(int(i) for i in np.asarray(index).reshape(len(shape)))
    out = np.zeros(shape, dtype)
    if out.size:
        out[idx] = 1
    return out, None


# ---- the fixture tests/golden/waveforms_vectors.json ----
def fixture_t(recipe):
    """the f32 tensor a fixture recipe stands for, as the reference builds it"""
    f32 = np.float32
    if "linspace" in recipe:   # Nx.linspace: iota * step + start in f32
        start, stop, n = recipe["linspace"]
        step = f32((stop - start) / (n - 1))
        return (np.arange(n, dtype=f32) * step).astype(f32) + f32(start)
    if "iota_times" in recipe:
        n, c = recipe["iota_times"]
        return (np.arange(n, dtype=np.float64) * float(f32(c))).astype(f32)
    return np.asarray(recipe["values"], f32)


def run_case(impl, case):
    """one fixture case through impl (this module or nx_signal_amd.waveforms, whose functions return the values alone)"""
    opts = dict(case.get("opts", {}))
    if case["fn"] == "unit_impulse":
        if "type" in opts:
            opts["dtype" if impl.__name__.endswith("oracle") else "type"] = {"s32": np.int32}[opts.pop("type")]
        out = impl.unit_impulse(tuple(case["shape"]), **opts)
    else:
        if isinstance(opts.get("duty"), list):
            opts["duty"] = np.asarray(opts["duty"], np.float32)
        args = [np.asarray(a) if isinstance(a, list) else a for a in case.get("args", [])]
        out = getattr(impl, case["fn"])(fixture_t(case["t"]), *args, **opts)
    return out[0] if impl.__name__.endswith("oracle") else out
