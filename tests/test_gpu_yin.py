"""Spectral.yin on the GPU against the definition of include/nxsig.h restated in numpy long double.  Per frame: cmnd within 1e-5 max |c_ref|,
v within 1e-5 |v_ref|, f0 within 1e-5 f0_ref.  The pick of the lag is discrete, so every case first shows ON THE REFERENCE ALONE that each
comparison which decides it is >= 1e-6 (relatively) from flipping: a condition on the inputs.  NXSIG_YIN_LAGS forces the lags per thread."""
import ctypes as C
import functools

import numpy as np
import pytest

import nx_signal_amd as S
from nx_signal_amd import _lib, spectral

pytestmark = pytest.mark.gpu

TOL, MARGIN, SR, THR, LD = 1e-5, 1e-6, 16000, 0.1, np.longdouble


def yin_frame(x, pmin, pmax, thr=THR, sr=SR):
    """the definition on one frame: (f0, v, c, the smallest relative margin of the comparisons that decide the pick)"""
    x, W, rel = x.astype(LD), len(x) // 2, lambda a, b: abs(a - b) / max(abs(a), abs(b))
    d = np.array([np.sum((x[1:W + 1] - x[1 + t:W + 1 + t]) ** 2) for t in range(pmax + 1)])
    tau = np.arange(pmin, pmax + 1)
    c = d[tau] / (np.cumsum(d[1:])[tau - 1] / tau + LD(np.finfo(np.float64).tiny))
    m = len(c)
    trough = np.r_[c[0] < c[1], (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:]), c[-1] < c[-2]]
    hits = np.flatnonzero(trough & (c < thr))
    i = int(hits[0]) if len(hits) else int(np.argmin(c))
    margins = [] if len(hits) else [rel(*np.sort(c)[:2])]
    for k in range(i + 1 if len(hits) else m):
        near = [c[j] for j in (k - 1, k + 1) if 0 <= j < m]
        if min(near + [c[k]]) < 1.001 * thr:
            margins += [rel(c[k], q) for q in near] + [rel(c[k], LD(thr))]
    shift = LD(0)
    if 0 < i < m - 1:
        a, b = c[i + 1] + c[i - 1] - 2 * c[i], (c[i + 1] - c[i - 1]) / 2
        margins.append(rel(abs(a), abs(b)))
        if abs(b) < abs(a):
            shift = -b / a
    return sr / (pmin + i + shift), c[i], c, min(margins)


def reference(x, L, hop, pmin, pmax, center):
    """(f0 [rows, F], v [rows, F], c [rows, F, m], the smallest margin) in long double"""
    lead = L // 2 if center else 0
    xp = np.pad(x, ((0, 0), (lead, lead)))
    out = [[yin_frame(row[s:s + L], pmin, pmax) for s in range(0, xp.shape[1] - L + 1, hop)] for row in xp]
    return tuple(np.array([[fr[i] for fr in row] for row in out], LD) for i in range(3)) + (min(fr[3] for row in out for fr in row),)


def signal(kind, n, seed):
    """two f32 rows: five harmonics of 110 Hz 2^(row / 3) with 2 % vibrato at 5 Hz, that plus 5 % noise, or white noise"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal((2, n)).astype(np.float32)
    t = np.arange(n) / SR
    f = 110.0 * 2.0 ** (np.arange(2)[:, None] / 3)
    phase = 2 * np.pi * f * t - 0.02 * f / 5 * np.cos(2 * np.pi * 5 * t)
    y = sum(np.sin(k * phase) / k for k in range(1, 6))
    if kind == "tone+noise":
        y = y + 0.05 * y.std() * rng.standard_normal(y.shape)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(kind, L, hop, pmin, pmax, center):
    n = L + 2 * hop + min(hop, 3)   # three frames and a ragged tail
    x = signal(kind, n, L + hop + pmax)
    return x, reference(x, L, hop, pmin, pmax, center)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def run(ctx, x, L, hop, pmin, pmax, center, lags=0):   # all three results for the lags pmin ... pmax, under NXSIG_YIN_LAGS=lags if given
    if lags:
        ctx.set_tuning("YIN_LAGS", lags)
    try:
        got = spectral.yin(x, SR / (pmax - 0.5), SR / (pmin + 0.5), SR, L, hop, center=center, return_voicing=True, return_cmnd=True, ctx=ctx)
        assert ctx.last_dispatch() == "yin.tile", ctx.last_dispatch()
    finally:
        if lags:
            ctx.clear_tuning("YIN_LAGS")
    return got


# the issue's shapes, then one on each side of every boundary of the plan that they leave out: 128 | 129 lags (2 | 4 per thread), 257
# (4 | 8), 512 | 513 (64 | 256 threads), 1025 (4 | 8 on 256 threads); 64 | 65, 256 and 1024 are among the first ten
SHAPES = [(8, 2, 1, 3), (64, 16, 2, 31), (128, 32, 1, 63), (130, 33, 3, 64), (256, 64, 8, 65), (512, 100, 16, 255), (1024, 256, 32, 400),
          (2048, 512, 32, 1023), (2048, 2500, 40, 230), (4096, 1024, 20, 2047),
          (256, 64, 8, 127), (258, 64, 8, 128), (514, 100, 16, 256), (1024, 256, 32, 511), (1026, 256, 32, 512), (2050, 512, 32, 1024)]


@pytest.mark.parametrize("lags", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("center", [False, True], ids=["frame", "center"])
@pytest.mark.parametrize("kind", ["tone", "tone+noise", "noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_against_the_definition(ctx, shape, kind, center, lags):
    L, hop, pmin, pmax = shape
    x, (f0, v, c, margin) = case(kind, L, hop, pmin, pmax, center)
    assert margin >= MARGIN, margin   # the precondition, on the reference alone
    g0, gv, gc = (np.asarray(g, LD) for g in run(ctx, x, L, hop, pmin, pmax, center, lags))
    assert (g0.shape, gv.shape, gc.shape) == (f0.shape, v.shape, c.shape)
    err = [np.abs(gc - c).max(axis=2) / np.abs(c).max(axis=2), np.abs(gv - v) / np.abs(v), np.abs(g0 - f0) / f0]
    print(f"yin-accuracy {shape} {kind} center={center} lags={lags}: cmnd, v, f0 {[float(f'{float(e.max()):.3g}') for e in err]}")
    assert all(np.all(e <= TOL) for e in err), err


@pytest.mark.parametrize("center", [0, 1])
def test_strided_rows_through_the_c_entry(ctx, center):
    L, hop, pmin, pmax, n, stride = 64, 16, 2, 31, 100, 131   # an odd stride: every row and frame start is misaligned differently
    x = signal("tone+noise", 3 * stride, 11)[0].reshape(3, stride)
    frames = int(_lib.load().nxsig_yin_frames(n, L, hop, center))
    dx, d0, dc = ctx.to_device(x), ctx.empty((3, frames), np.float32), ctx.empty((3, frames, pmax - pmin + 1), np.float32)
    _lib.check(_lib.load().nxsig_yin_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(dx.ptr), 3, n, stride, L, hop, center, pmin, pmax,
                                         float(SR), THR, C.c_void_p(d0.ptr), None, C.c_void_p(dc.ptr), _lib.DEVICE))
    f0, _, c, margin = reference(x[:, :n], L, hop, pmin, pmax, bool(center))
    assert margin >= MARGIN and f0.shape == (3, frames)
    assert np.all(np.abs(d0.numpy() - f0) <= TOL * f0) and np.all(np.abs(dc.numpy() - c).max(axis=2) <= TOL * np.abs(c).max(axis=2))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_an_all_zero_frame(ctx):
    L, pmin, pmax = 64, 2, 31
    x = signal("tone+noise", 3 * L, 3)[:1]
    clean = run(ctx, x, L, L, pmin, pmax, False)
    x[0, L:2 * L] = 0
    got = run(ctx, x, L, L, pmin, pmax, False)
    assert got[0][0, 1] == np.float32(SR / pmin) and got[1][0, 1] == 0 and not got[2][0, 1].any()
    for g, c in zip(got, clean):
        assert np.array_equal(bits(g[0, [0, 2]]), bits(c[0, [0, 2]]))


def test_a_frame_of_exact_integer_period(ctx):
    """a square wave of period 16: c is exactly 0 at lags 16, 32 and 48, and lag 16 is picked.  c(15) = 15 / 64 and c(17) = 17 / 65 differ
    (the cumulative mean), so the definition's f0 is sr / (16 + shift) with shift = -0.0274, not sr / 16"""
    L, pmin, pmax = 128, 2, 63
    x = np.where(np.arange(L) % 16 < 8, 1.0, -1.0).astype(np.float32)[None]
    f0, v, c = run(ctx, x, L, L, pmin, pmax, False)
    assert not c[0, 0, [16 - pmin, 32 - pmin, 48 - pmin]].any() and np.count_nonzero(c[0, 0] == 0) == 3 and v[0, 0] == 0
    r0 = yin_frame(x[0], pmin, pmax)[0]
    assert abs(f0[0, 0] - r0) <= TOL * r0 and abs(r0 - SR / (16 - (17 / 65 - 15 / 64) / 2 / (17 / 65 + 15 / 64))) < 1e-9 * r0


def test_non_finite_samples_stay_in_their_frames(ctx):
    L, hop, pmin, pmax, n = 64, 16, 2, 31, 400
    x = signal("tone+noise", n, 5)
    clean = run(ctx, x, L, hop, pmin, pmax, True)
    bad = x.copy()
    bad[1, 32], bad[1, 301] = np.inf, np.nan   # 32 is sample 0 of the frame that starts there: that frame stays finite
    got = run(ctx, bad, L, hop, pmin, pmax, True)
    s = np.arange(0, n + 1, hop) - L // 2   # the frames' starts
    hit = np.zeros((2, len(s)), bool)
    hit[1] = ((s + 1 <= 32) & (32 <= s + L // 2 + pmax)) | ((s + 1 <= 301) & (301 <= s + L // 2 + pmax))
    assert hit[1, 0] == False and 32 in s and not hit[1, list(s).index(32)] and hit.sum() == 7   # noqa: E712
    for g, c in zip(got, clean):
        g2, c2 = g.reshape(hit.shape + (-1,)), c.reshape(hit.shape + (-1,))
        assert np.array_equal(np.isnan(g2), np.broadcast_to(hit[..., None], g2.shape))
        assert np.array_equal(bits(g2[~hit]), bits(c2[~hit]))


def test_device_tensor_gives_the_same_bits(ctx):
    shape = (130, 33, 3, 64)
    x, _ = case("tone+noise", *shape, True)
    got = run(ctx, ctx.to_device(x.reshape(2, 1, -1)), *shape, True)
    host = run(ctx, x, *shape, True)
    assert got[0].shape == (2, 1) + host[0].shape[1:] and got[2].shape == (2, 1) + host[2].shape[1:]
    for g, h in zip(got, host):
        assert isinstance(g, S.DeviceBuffer) and np.array_equal(bits(g.numpy().reshape(h.shape)), bits(h))
    only = spectral.yin(x, SR / 63.5, SR / 3.5, SR, 130, 33, ctx=ctx)
    assert np.array_equal(bits(only), bits(host[0]))
