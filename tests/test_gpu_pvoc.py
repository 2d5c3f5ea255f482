"""Transforms.phase_vocoder / time_stretch on the GPU against the definition of include/nxsig.h written wrap-free in numpy: the phase of
step t is angle(z[0]) + sum_{s<t} (angle(z[i_s + 1]) - angle(z[i_s])) accumulated in long double and reduced mod 2 pi, times the
interpolated double magnitude, with angle(0) = 0.  The bar is the project's: per row of the batch, max |got - ref| <= 1e-5 max |ref|.
pvoc.scan is forced with the value switch NXSIG_PVOC_CHUNK (a context switch: no child process is needed)."""
import functools

import numpy as np
import pytest

import nx_signal_amd as S
from nx_signal_amd import transforms as T

pytestmark = pytest.mark.gpu

TOL = 1e-5


def steps(M, rate):
    s = np.arange(len(np.arange(0, M, rate)), dtype=np.float64) * rate
    i = np.floor(s).astype(np.int64)
    return i, (s - i)[:, None]


def reference(z, rate):
    M = z.shape[1]
    i, al = steps(M, rate)
    zp = np.concatenate([z, np.zeros_like(z[:, :2])], axis=1).astype(np.complex128)   # frames M and M + 1 count as zeros
    ang = np.where(zp == 0, 0, np.arctan2(zp.imag.astype(np.longdouble), zp.real.astype(np.longdouble)))
    acc = ang[:, :1] + np.cumsum(ang[:, i + 1] - ang[:, i], axis=1) - (ang[:, i + 1] - ang[:, i])   # exclusive: the sum over s < t
    phase = np.fmod(acc, 2 * np.pi * np.longdouble(1)).astype(np.float64)
    return ((1 - al) * np.abs(zp[:, i]) + al * np.abs(zp[:, i + 1])) * np.exp(1j * phase)


def spectrogram(seed, *shape):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def case(shape, rate):
    z = spectrogram(sum(shape), *shape)
    return z, reference(z, rate)


def check(what, got, ref, tol=TOL):
    got, ref = np.asarray(got, np.complex128).reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    worst = np.abs(got - ref).max(axis=1)
    print(f"{what}: worst row {np.max(worst / np.maximum(np.abs(ref).max(axis=1), 1e-300)):.3g}")
    assert np.all(worst <= tol * np.abs(ref).max(axis=1)), (what, worst)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def run(ctx, z, rate, chunk=0):
    """phase_vocoder on the context, under NXSIG_PVOC_CHUNK=chunk when given, with the dispatch record checked against the plan"""
    if chunk:
        ctx.set_tuning("PVOC_CHUNK", chunk)
    try:
        got = T.phase_vocoder(z, rate, ctx)
        n_out = got.shape[-2]
        assert ctx.last_dispatch() == ("pvoc.scan" if chunk and n_out > chunk else "pvoc.walk"), (ctx.last_dispatch(), n_out)
    finally:
        if chunk:
            ctx.clear_tuning("PVOC_CHUNK")
    return got


# [2, 37, 9]: odd K, the 8-byte path; [3, 200, 64]: the 16-byte path, one tile; [1, 50, 130]: two tiles and a tail; [2, 40, 513]:
# one-sided with Nyquist; [1, 5, 6] at rate 7 has a single output frame.  Chunks of 8 give several chunks and a ragged last one
@pytest.mark.parametrize("chunk", [0, 8])
@pytest.mark.parametrize("rate", [0.37, 0.5, 1.0, 1.3, 2.5, 7.0])
@pytest.mark.parametrize("shape", [(2, 37, 9), (3, 200, 64), (1, 50, 130), (2, 40, 513), (1, 5, 6)])
def test_against_the_definition(ctx, shape, rate, chunk):
    z, ref = case(shape, rate)
    got = run(ctx, z, rate, chunk)
    assert got.dtype == np.complex64 and got.shape == ref.shape
    check(f"pvoc {shape} rate {rate} chunk {chunk}", got, ref)


def test_long_scan_keeps_its_phase(ctx):
    """391 chunks of 64 frames: where a product carried in f32 has drifted to 4e-6, the double carry stays at rounding"""
    z, ref = case((1, 20000, 4), 0.8)
    check("pvoc long scan", run(ctx, z, 0.8, 64), ref)


@pytest.mark.parametrize("chunk", [0, 8])
def test_rate_one_is_the_identity(ctx, chunk):
    z = spectrogram(3, 3, 40, 10)
    z[0, 5:9, 2] = 0
    z[0, 0, 3] = 0            # a bin that starts at zero: u(0) = 1
    z[1] = 0                  # an all-zero row comes back as zeros
    z[2, 7, 4] = complex(-0.0, 1.5)
    z[2, 9, 4] = complex(-0.0, 0.0)
    check("identity", run(ctx, z, 1.0, chunk), z.astype(np.complex128), tol=1e-6)


@pytest.mark.parametrize("hop", [64, 100])
def test_equals_librosas_loop_for_every_hop(ctx, hop):
    """librosa.phase_vocoder restated (atan2, wrap, phase_acc) in double: the expected advance it needs cancels, so both hops agree"""
    z, rate = spectrogram(9, 1, 60, 129), 1.3
    zp = np.concatenate([z[0], np.zeros_like(z[0, :2])]).astype(np.complex128)
    phi = np.linspace(0, np.pi * hop, zp.shape[1])
    acc, out = np.angle(zp[0]), []
    for s in np.arange(0, z.shape[1], rate):
        c0, c1, al = zp[int(s)], zp[int(s) + 1], np.mod(s, 1.0)
        out.append(((1 - al) * np.abs(c0) + al * np.abs(c1)) * np.exp(1j * acc))
        d = np.angle(c1) - np.angle(c0) - phi
        acc = acc + phi + d - 2 * np.pi * np.round(d / (2 * np.pi))
    check(f"librosa hop {hop}", run(ctx, z, rate), np.array(out)[None])


@pytest.mark.parametrize("chunk", [0, 8])
def test_non_finite_stays_in_its_bin_from_its_step_on(ctx, chunk):
    rate, (row, k) = 1.3, (1, 2)
    z = spectrogram(5, 2, 30, 6)
    clean = run(ctx, z, rate, chunk)
    bad = z.copy()
    bad[row, 10, k], bad[row, 20, k] = np.inf, np.nan
    got = run(ctx, bad, rate, chunk)
    i, _ = steps(30, rate)
    first = np.flatnonzero((i == 9) | (i == 10))[0]   # the first step whose pair holds frame 10
    hit = np.zeros(got.shape, bool)
    hit[row, first:, k] = True
    assert np.array_equal(~np.isfinite(got), hit)
    assert np.array_equal(got[~hit].view(np.uint32), clean[~hit].view(np.uint32))


def test_device_tensor_gives_the_same_bits(ctx):
    z, _ = case((2, 37, 9), 1.3)
    got = run(ctx, ctx.to_device(z), 1.3, 8)
    assert isinstance(got, S.DeviceBuffer)
    assert np.array_equal(got.numpy().view(np.uint32), run(ctx, z, 1.3, 8).view(np.uint32))


def test_time_stretch(ctx):
    x = np.random.default_rng(2).standard_normal((2, 4096)).astype(np.float32)
    w, o = S.windows.hann(256), {"overlap_length": 192}
    got = T.time_stretch(ctx.to_device(x), 0.8, w, ctx, **o)
    want = S.istft(T.phase_vocoder(S.stft(ctx.to_device(x), w, ctx, **o)[0], 0.8, ctx), w, ctx, **o)
    assert got.shape == want.shape and np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    same = T.time_stretch(x, 1.0, w, ctx, **o)
    assert same.shape == x.shape and np.abs(same[:, 256:-256] - x[:, 256:-256]).max() <= 1e-5 * np.abs(x).max()
