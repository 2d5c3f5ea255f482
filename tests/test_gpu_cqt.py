"""Spectral.cqt / vqt on the GPU against the definition of include/nxsig.h restated in numpy long double.  Every comparison is against 1e-5
of the row maximum of |C_ref| (of |C_ref|^2 for the power output).  NXSIG_CQT_MFMA=0 forces cqt.direct."""
import ctypes as C
import functools

import numpy as np
import pytest

import nx_signal_amd as S
from nx_signal_amd import _cqt, _lib, spectral

pytestmark = pytest.mark.gpu

TOL, LD = 1e-5, np.longdouble
PI = np.arccos(LD(-1))


def reference(x, sr, fmin, n_bins, B, hop, filter_scale=1.0, norm=1, scale=True, gamma=0.0):
    """C[row, k, t] of the definition in long double, and (lo_k, N_k)"""
    n, alpha = x.shape[-1], LD(2) ** (LD(1) / B) - 1
    frames, spans = 1 + n // hop, []
    out = np.zeros((len(x), n_bins, frames), np.clongdouble)
    for k in range(n_bins):
        f = LD(fmin) * LD(2) ** (LD(k) / B)
        ell = LD(filter_scale) * sr / (alpha * f + LD(gamma))
        lo, hi = int(np.floor(-ell / 2)), int(np.floor(ell / 2)) - 1
        N, nn = hi - lo + 1, np.arange(lo, hi + 1).astype(LD)
        b = (LD(0.5) - LD(0.5) * np.cos(2 * PI * np.arange(N).astype(LD) / N)) * np.exp(2j * PI * f * nn / sr)
        b = b / np.abs(b).sum() if norm == 1 else b / np.sqrt((np.abs(b) ** 2).sum()) if norm == 2 else b
        a = np.conj(b) * (np.sqrt(ell) if scale else ell)
        xp = np.pad(x.astype(LD), ((0, 0), (N, N)))
        for t in range(frames):
            out[:, k, t] = xp[:, N + t * hop + lo:N + t * hop + hi + 1] @ a
        spans.append((lo, N))
    return out, spans


def signal(kind, sr, fmin, n_bins, B, n):
    """two f32 rows: tones at bins 5 and n_bins - 2 with different phases per row, or white noise"""
    if kind == "noise":
        return np.random.default_rng(n + n_bins).standard_normal((2, n)).astype(np.float32)
    t, f = np.arange(n) / sr, fmin * 2.0 ** (np.array([5, n_bins - 2]) / B)
    return np.stack([np.sin(2 * np.pi * f[0] * t + 0.3 + r) + 0.5 * np.cos(2 * np.pi * f[1] * t + 1.1 * r) for r in range(2)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, kind, opts=()):
    sr, fmin, n_bins, B, hop, n = shape
    x = signal(kind, sr, fmin, n_bins, B, n)
    return x, reference(x, sr, fmin, n_bins, B, hop, **{k: v for k, v in opts if k != "output"})


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def run(ctx, x, shape, tier, **opts):
    sr, fmin, n_bins, B, hop, _ = shape
    if tier == "direct":
        ctx.set_tuning("CQT_MFMA", 0)
    try:
        got = spectral.vqt(x, sr, hop, fmin, n_bins, B, ctx=ctx, **opts)
        assert ctx.last_dispatch() == "cqt." + tier, ctx.last_dispatch()
    finally:
        if tier == "direct":
            ctx.clear_tuning("CQT_MFMA")
    return got


def worst(got, ref):
    return float((np.abs(got.astype(ref.dtype) - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))).max())


# the issue's four shapes, F = 1 (len < hop) and F = 33 (one frame past a wave's 32 frames); then the other boundaries of the plan:
# F = 16 | 17 (a frame tile), 128 | 129 (a workgroup's frames).  The n range of a bin tile crosses a panel (512) in the second shape
SECOND = (8000, 100, 40, 12, 64, 1500)
SHAPES = [(8000, 500, 12, 12, 16, 200), SECOND, (16000, 110, 70, 24, 37, 900), (22050, 32.7, 24, 12, 512, 6000),
          (8000, 500, 12, 12, 64, 40), (8000, 500, 12, 12, 16, 520), (8000, 500, 12, 12, 16, 250), (8000, 500, 12, 12, 16, 260),
          (8000, 500, 12, 12, 16, 2040), (8000, 500, 12, 12, 16, 2050)]
TIERS = ["mfma", "direct"]


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("kind", ["tones", "noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_against_the_definition(ctx, shape, kind, tier):
    x, (ref, _) = case(shape, kind)
    got = run(ctx, x, shape, tier)
    assert got.shape == ref.shape and got.dtype == np.complex64
    err = worst(got, ref)
    print(f"cqt-accuracy {shape} {kind} {tier}: {err:.3g} of the row maximum {float(np.abs(ref).max()):.3g}")
    assert err <= TOL, err


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("opts", [dict(gamma=20.0), dict(norm=2), dict(norm=None), dict(scale=False), dict(filter_scale=0.5),
                                  dict(output="magnitude"), dict(output="power"), dict(gamma=5.0, norm=2, scale=False, output="power")], ids=str)
def test_vqt_and_the_options(ctx, opts, tier):
    x, (ref, _) = case(SECOND, "tones", tuple(sorted(opts.items())))
    kind = opts.get("output", "complex")
    ref = np.abs(ref) if kind == "magnitude" else np.abs(ref) ** 2 if kind == "power" else ref
    got = run(ctx, x, SECOND, tier, **opts)
    assert got.dtype == (np.complex64 if kind == "complex" else np.float32)
    err = worst(got, ref)
    print(f"cqt-options {opts} {tier}: {err:.3g}")
    assert err <= TOL, err


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("output", ["complex", "power"])
@pytest.mark.parametrize("tier", TIERS)
def test_non_finite_samples_stay_in_their_supports(ctx, tier, output):
    sr, fmin, n_bins, B, hop, n = SECOND
    x, (_, spans) = case(SECOND, "noise")
    at = (300, 1100)
    lo, N = (np.array(v)[:, None] for v in zip(*spans))
    start = np.arange(1 + n // hop)[None, :] * hop + lo
    hit = np.logical_or.reduce([(start <= p) & (p < start + N) for p in at])
    assert hit.any() and not hit.all()
    order = np.argsort(-N[:, 0], kind="stable")
    groups = [order[i:i + 16] for i in range(0, n_bins, 16)]   # the bin tiles: sorted by length, 16 each
    assert any((hit[g].any(axis=0) & ~hit[g].all(axis=0)).any() for g in groups)   # a padded tile multiplies 0 by NaN there
    bad, zero = x.copy(), x.copy()
    bad[1, at[0]], bad[1, at[1]], zero[1, at] = np.inf, np.nan, 0
    clean, got, want = (run(ctx, v, SECOND, tier, output=output) for v in (x, bad, zero))
    parts = got[1].view(np.float32).reshape(hit.shape + (-1,))   # both parts of a complex output
    assert np.array_equal(np.isnan(parts), np.broadcast_to(hit[..., None], parts.shape))
    assert np.array_equal(bits(got[1][~hit]), bits(want[1][~hit])) and np.array_equal(bits(got[0]), bits(clean[0]))


@pytest.mark.parametrize("tier", TIERS)
def test_strided_rows_through_the_c_entry(ctx, tier):
    sr, fmin, n_bins, B, hop, n = SECOND
    x, _ = case(SECOND, "noise")
    dense = run(ctx, x, SECOND, tier)
    wide = np.full((2, n + 31), np.nan, np.float32)
    wide[:, :n] = x
    lo, count, taps = _cqt._bank(float(sr), float(fmin), n_bins, B, 1.0, 1, True, 0.0)
    dx, out = ctx.to_device(wide), ctx.empty(dense.shape, np.complex64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if tier == "direct":
        ctx.set_tuning("CQT_MFMA", 0)
    try:
        _lib.check(_lib.load().nxsig_cqt_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(dx.ptr), 2, n, n + 31, hop, n_bins, p(lo), p(count),
                                             p(taps), C.c_void_p(out.ptr), 0, _lib.DEVICE))
    finally:
        if tier == "direct":
            ctx.clear_tuning("CQT_MFMA")
    assert np.array_equal(bits(out.numpy()), bits(dense))


def test_device_tensor_gives_the_same_bits(ctx):
    shape = (16000, 110, 70, 24, 37, 900)
    x, _ = case(shape, "tones")
    host = run(ctx, x, shape, "mfma", output="magnitude")
    got = run(ctx, ctx.to_device(x.reshape(2, 1, -1)), shape, "mfma", output="magnitude")
    assert isinstance(got, S.DeviceBuffer) and got.shape == (2, 1) + host.shape[1:]
    assert np.array_equal(bits(got.numpy().reshape(host.shape)), bits(host))
