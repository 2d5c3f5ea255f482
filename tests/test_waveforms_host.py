"""Waveforms without a GPU: the numpy oracle (tests/waveforms_oracle.py) reproduces every literal of the reference
(tests/golden/waveforms_vectors.json) bit for bit and agrees with scipy.signal on t >= 0, the Python mirror raises its ArgumentErrors
before it needs a device, and the C ABI declares and exports the six entry points."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import nx_signal_amd as S
import waveforms_oracle as O
from nx_signal_amd import _lib
from nx_signal_amd._lib import ArgumentError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W = S.waveforms
ENTRY_POINTS = ("nxsig_sawtooth", "nxsig_square", "nxsig_gaussian_pulse", "nxsig_chirp", "nxsig_polynomial_sweep", "nxsig_unit_impulse")


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(HERE, "golden", "waveforms_vectors.json")) as f:
        return json.load(f)["cases"]


def literal_matches(case, got, expected):
    """bit equality, or the reference's own atol = rtol = 1e-4 for a literal the fixture marks as such"""
    exp = np.asarray(expected, got.dtype)
    assert got.shape == exp.shape, case["source"]
    if case["compare"] == "bits":
        return got.tobytes() == exp.tobytes()
    return bool(np.all(np.abs(got - exp) <= 1e-4 + 1e-4 * np.abs(exp)))


def check_case(case, got):
    exp = case["expected"]
    if isinstance(exp, dict):
        assert sorted(got) == sorted(exp) == ["envelope", "in_phase", "quadrature"]
        for k in exp:
            assert got[k].dtype == np.float32
            assert literal_matches(case, np.asarray(got[k]), exp[k]), (case["source"], k, got[k], exp[k])
    else:
        want = {"square": np.int32, "unit_impulse": np.dtype(case.get("dtype", "float32"))}.get(case["fn"], np.float32)
        assert got.dtype == want, case["source"]
        assert literal_matches(case, np.asarray(got), exp), (case["source"], got, exp)


def test_oracle_reproduces_every_literal(cases):
    assert len(cases) == 22
    assert {c["fn"] for c in cases} == {"sawtooth", "square", "gaussian_pulse", "chirp", "polynomial_sweep", "unit_impulse"}
    assert all(c["compare"] == "bits" for c in cases)   # no literal needed the 1e-4 fallback
    for c in cases:
        check_case(c, O.run_case(O, c))


def test_oracle_f64_matches_scipy_for_nonnegative_t():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    # the oracle's period is 2 * f32(pi): scale t so that both see the same position in the period
    u = rng.uniform(0.0, 8.0, 4000)
    for width in (0, 0.25, 0.5, 1):
        got, _ = O.sawtooth(u * O.TWO_PI, width=width)
        assert got.dtype == np.float64
        # away from the jumps, where a last-bit difference in the remainder would flip the branch
        pos = np.mod(u, 1.0)
        keep = (np.abs(pos - width) > 1e-9) & (pos > 1e-9) & (pos < 1 - 1e-9)
        assert np.max(np.abs(got[keep] - signal.sawtooth(u[keep] * 2 * np.pi, width))) <= 1e-12, width
    for duty in (0.1, 0.5, 0.9):
        got, _ = O.square(u * O.TWO_PI, duty=duty)
        pos = np.mod(u, 1.0)
        keep = (np.abs(pos - duty) > 1e-9) & (pos > 1e-9) & (pos < 1 - 1e-9)
        assert np.array_equal(got[keep], signal.square(u[keep] * 2 * np.pi, duty).astype(np.int32)), duty


def test_oracle_tiers_and_quirks():
    t = np.linspace(-3, 3, 7)
    assert O.sawtooth(t)[0].dtype == np.float64 and O.sawtooth(t.astype(np.float32))[0].dtype == np.float32
    assert O.sawtooth(np.arange(4))[0].dtype == np.float32   # integers are read as f32
    # Nx.remainder is C fmod: the sign of the dividend, so sawtooth(-1.0) lies below -1 as in the reference
    assert O.sawtooth(np.float32([-1.0]))[0][0] < -1
    assert np.isnan(O.chirp(np.float32([0.5, 1.0]), -1, 1, 2, method="logarithmic")[0]).all()
    for m in ("logarithmic", "hyperbolic"):   # f0 == f1
        got, arg = O.chirp(np.float32([0.25, 0.5]), 3, 1, 3, method=m)
        assert np.array_equal(arg, (np.float32(O.TWO_PI * 3) * np.float32([0.25, 0.5])).astype(np.float64)), m


def test_argument_errors_fire_before_a_device_is_needed():
    t = np.linspace(0, 1, 5, dtype=np.float32)
    for width in (-0.1, 1.5, float("nan")):
        with pytest.raises(ArgumentError, match="width must be between 0 and 1, inclusive"):
            W.sawtooth(t, width=width)
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.sawtooth(t, widht=1)
    with pytest.raises(ArgumentError, match="complex"):
        W.sawtooth(np.zeros(3, np.complex64))
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.square(t, width=1)
    with pytest.raises(ArgumentError, match="duty must have t's shape"):
        W.square(t, duty=np.zeros(4, np.float32))
    with pytest.raises(ArgumentError, match="duty must be a number"):
        W.square(t, duty="half")
    with pytest.raises(ArgumentError, match="Center frequency must be greater than or equal to 0"):
        W.gaussian_pulse(t, center_frequency=-1)
    for bw in (0, -2):
        with pytest.raises(ArgumentError, match="Bandwidth must be greater than 0"):
            W.gaussian_pulse(t, bandwidth=bw)
    for bwr in (0, 3):
        with pytest.raises(ArgumentError, match="Bandwidth reference level must be less than 0"):
            W.gaussian_pulse(t, bandwidth_reference_level=bwr)
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.gaussian_pulse(t, fc=4)
    with pytest.raises(ArgumentError, match="invalid method, must be one of"):
        W.chirp(t, 1, 1, 2, method="cubic")
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.chirp(t, 1, 1, 2, vertex=True)
    with pytest.raises(ArgumentError, match="f0 must be a number"):
        W.chirp(t, "1", 1, 2)
    with pytest.raises(ArgumentError, match="1 to 32 entries"):
        W.polynomial_sweep(t, [])
    with pytest.raises(ArgumentError, match="1 to 32 entries"):
        W.polynomial_sweep(t, np.ones(33))
    with pytest.raises(ArgumentError, match="rank 1"):
        W.polynomial_sweep(t, np.ones((2, 2)))
    with pytest.raises(ArgumentError, match="t must have rank 1"):
        W.polynomial_sweep(np.zeros((2, 3), np.float32), [1, 0])
    with pytest.raises(ArgumentError, match="phi_unit"):
        W.polynomial_sweep(t, [1, 0], phi_unit="turns")
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.polynomial_sweep(t, [1, 0], unit="degrees")
    for shape, index in (((3,), 3), ((3,), -1), ((3, 5), [3, 0]), ((3, 5), [0, 5])):
        with pytest.raises(ArgumentError, match="out of range"):
            W.unit_impulse(shape, index=index)
    with pytest.raises(ArgumentError, match="index must hold 2 integers"):
        W.unit_impulse((3, 5), index=1)
    with pytest.raises(ArgumentError, match="index must hold"):
        W.unit_impulse((3,), index=0.5)
    with pytest.raises(ArgumentError, match="type must be one of"):
        W.unit_impulse((3,), type=np.int8)
    with pytest.raises(ArgumentError, match="unknown type"):
        W.unit_impulse((3,), type="s8")
    with pytest.raises(ArgumentError, match="rank must be at most 8"):
        W.unit_impulse((1,) * 9)
    with pytest.raises(ArgumentError, match="unknown keys"):
        W.unit_impulse((3,), dtype="f32")
    # an empty dimension gives an empty tensor, without a device
    assert W.unit_impulse((3, 0), type="s32", index="midpoint").shape == (3, 0)


def test_waveform_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nxsig.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name, value in (("NXSIG_CHIRP_LINEAR", 0), ("NXSIG_CHIRP_QUADRATIC", 1), ("NXSIG_CHIRP_LOGARITHMIC", 2), ("NXSIG_CHIRP_HYPERBOLIC", 3)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
        assert getattr(_lib, name[6:]) == value
    assert re.search(r"#define NXSIG_SWEEP_MAX_COEFS 32\b", hdr) and _lib.SWEEP_MAX_COEFS == 32
    for fn in ("sawtooth", "square", "gaussian_pulse", "chirp", "polynomial_sweep", "unit_impulse", "sinc"):
        assert callable(getattr(W, fn)), fn


def test_waveform_kernels_keep_the_rounding_contract():
    kern = open(os.path.join(ROOT, "nx_signal_amd", "csrc", "kernels_waveforms.hip")).read()
    code = re.sub(r"//.*", "", kern)
    assert "#pragma clang fp contract(off)" in code
    # the double functions only, no atomics
    assert not re.search(r"\b(cosf|sinf|expf|powf|logf|fmodf|__cosf|__sinf|__expf)\s*\(", code)
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", code)
    from nx_signal_amd import build
    assert any(src == "kernels_waveforms.hip" for src, _ in build.UNITS)
