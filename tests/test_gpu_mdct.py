"""Transforms.mdct / imdct on the GPU against the definition of include/nxsig.h as a dense cosine matrix in numpy double.  The bar is
the project's for a single-precision transform: per row of the batch, max |got - ref| <= 1e-5 max |ref| of that row (inputs are seeded
standard normal, so no row cancels).  RUN and SHARE restate kMdMinRun and kMdWaves * kMdMinRun of csrc/mdct_plan.hpp: the frames of a
wave's run and of a workgroup's share at the smallest launch, so that F = RUN + 1 and SHARE + 1 put a seam inside a row.  The generic
tier is forced with the value switch NXSIG_MDCT_WAVE=0 (a context switch: no child process is needed)."""
import ctypes as C

import numpy as np
import pytest

import nx_signal_amd as S
from nx_signal_amd import _lib, transforms as T

pytestmark = pytest.mark.gpu

TOL, RUN, SHARE = 1e-5, 8, 32


def scale(M, norm, inverse):
    return np.sqrt(2.0 / M) if norm == "ortho" else (2.0 / M if inverse else 1.0)


def cosines(M):
    return np.cos(np.pi / M * (np.arange(2 * M) + 0.5 + M / 2) * (np.arange(M)[:, None] + 0.5))   # [k, n]


def ref_mdct(x, w, pad=False, norm=None):
    M, (rows, L) = len(w) // 2, x.shape
    F = -(-L // M) + 1 if pad else (L - 2 * M) // M + 1
    xp, lo = np.zeros((rows, (F + 1) * M)), M if pad else 0
    n = min(L, (F + 1) * M - lo)                       # a ragged tail is dropped
    xp[:, lo:lo + n] = x[:, :n]
    frames = np.stack([xp[:, m * M:m * M + 2 * M] for m in range(F)], axis=1) * w.astype(np.float64)
    return scale(M, norm, False) * frames @ cosines(M).T


def ref_imdct(X, w, pad=False, norm=None, length=None):
    rows, F, M = X.shape
    y, Cm = np.zeros((rows, (F + 1) * M)), cosines(M)
    for m in range(F):
        y[:, m * M:m * M + 2 * M] += scale(M, norm, True) * w.astype(np.float64) * (X[:, m].astype(np.float64) @ Cm)
    return y[:, M:M + ((F - 1) * M if length is None else length)] if pad else y


def check(what, got, ref):
    got = np.asarray(got, np.float64).reshape(ref.shape[0], -1)
    ref = ref.reshape(ref.shape[0], -1)
    err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"{what}: worst row {err.max():.3g}")
    assert np.all(err <= TOL), (what, err)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def rows_of(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def both(ctx, x, X, w, tier, pad=False, norm=None):
    """forward of x and inverse of X on device tensors, each against the definition, with the dispatch record"""
    opts = {"pad": pad, "norm": norm}
    got = T.mdct(ctx.to_device(x), w, ctx, pad_edges=pad, norm=norm)
    assert ctx.last_dispatch().startswith("mdct." + tier), ctx.last_dispatch()
    check(f"mdct {x.shape} M={len(w) // 2} {opts}", got.numpy(), ref_mdct(x.astype(np.float64), w, **opts))
    got = T.imdct(ctx.to_device(X), w, ctx, pad_edges=pad, norm=norm)
    assert ctx.last_dispatch().startswith("imdct." + tier), ctx.last_dispatch()
    check(f"imdct {X.shape} {opts}", got.numpy(), ref_imdct(X, w, **opts))


@pytest.mark.parametrize("F", [1, 2, RUN + 1, SHARE + 1])
@pytest.mark.parametrize("M", [256, 512, 1024])
def test_wave_frame_counts(ctx, M, F):
    w = T.mdct_window("sine", 2 * M)
    both(ctx, rows_of(M + F, 1, (F + 1) * M), rows_of(F, 1, F, M), w, "wave")


@pytest.mark.parametrize("rows", [1, 5])
def test_wave_rows_and_ragged_tail(ctx, rows):
    M, F = 256, SHARE + 1
    both(ctx, rows_of(rows, rows, 2 * M + (F - 1) * M + 3), rows_of(rows + 7, rows, F, M), T.mdct_window("sine", 2 * M), "wave")


@pytest.mark.parametrize("norm", [None, "ortho"])
@pytest.mark.parametrize("pad", [False, True])
def test_wave_pad_edges_and_norm(ctx, pad, norm):
    M = 512
    both(ctx, rows_of(3, 2, 9 * M + 3), rows_of(4, 2, 11, M), T.mdct_window("vorbis", 2 * M), "wave", pad=pad, norm=norm)


@pytest.mark.parametrize("pad", [False, True])
def test_wave_offset_view_and_row_stride(ctx, pad):
    """rows that start one float past a 16-byte boundary and lie L + 5 apart, through the C entry points"""
    M, rows, L = 256, 3, 10 * 256 + 3
    w, lib, h = T.mdct_window("sine", 2 * M), _lib.load(), _lib.ctx_ptr(ctx.handle, _lib._ctx_iir)
    x = rows_of(11, rows, L)
    arena = np.zeros(1 + rows * (L + 5), np.float32)
    for r in range(rows):
        arena[1 + r * (L + 5):1 + r * (L + 5) + L] = x[r]
    F = int(lib.nxsig_mdct_frames(L, 2 * M, int(pad)))
    dx, out = ctx.to_device(arena), ctx.empty((rows, F, M), np.float32)
    _lib.check(lib.nxsig_mdct_f32(h, C.c_void_p(dx.ptr + 4), L, rows, L + 5, w.ctypes.data_as(C.c_void_p), 2 * M, int(pad), 0, C.c_void_p(out.ptr), _lib.DEVICE))
    assert ctx.last_dispatch() == "mdct.wave"
    check("mdct view", out.numpy(), ref_mdct(x.astype(np.float64), w, pad=pad))
    X = rows_of(12, rows, F, M)
    n_out = (F - 1) * M - 3 if pad else (F + 1) * M
    dX, y = ctx.to_device(np.concatenate([np.zeros(1, np.float32), X.ravel()])), ctx.empty((1 + rows * n_out,), np.float32)
    _lib.check(lib.nxsig_imdct_f32(h, C.c_void_p(dX.ptr + 4), F, rows, w.ctypes.data_as(C.c_void_p), 2 * M, int(pad), 0, C.c_void_p(y.ptr + 4), n_out, _lib.DEVICE))
    assert ctx.last_dispatch() == "imdct.wave"
    check("imdct view", y.numpy()[1:], ref_imdct(X, w, pad=pad, length=n_out))


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", [2, 6, 18, 480])
def test_generic_lengths(ctx, M, F):
    both(ctx, rows_of(M, 2, (F + 1) * M), rows_of(M + 1, 2, F, M), T.mdct_window("sine", 2 * M), "generic")


def test_generic_under_the_switch(ctx):
    ctx.set_tuning("MDCT_WAVE", 0)
    try:
        both(ctx, rows_of(5, 2, 4 * 512), rows_of(6, 2, 3, 512), T.mdct_window("sine", 1024), "generic")
    finally:
        ctx.clear_tuning("MDCT_WAVE")


@pytest.mark.parametrize("kind", ["sine", "vorbis", "kbd"])
@pytest.mark.parametrize("M", [256, 18])
def test_round_trip(ctx, M, kind):
    w, x = T.mdct_window(kind, 2 * M), rows_of(M, 2, 9 * M + 5)
    X = T.mdct(ctx.to_device(x), w, ctx, pad_edges=True)
    y = T.imdct(X, w, ctx, pad_edges=True, length=x.shape[1])
    assert ctx.last_dispatch().startswith("imdct.wave" if M == 256 else "imdct.generic")
    check(f"round trip M={M} {kind}", y.numpy(), x.astype(np.float64))


@pytest.mark.parametrize("M", [256, 18])
def test_non_finite_stays_in_its_frames(ctx, M):
    w, F = T.mdct_window("sine", 2 * M), 6
    x = rows_of(M + 2, 1, (F + 1) * M)
    x[0, 3 * M + M // 2] = np.nan                      # block 3: frames 2 and 3 cover it
    got, hit = T.mdct(ctx.to_device(x), w, ctx).numpy(), [2, 3]
    keep = [m for m in range(F) if m not in hit]
    assert not np.isfinite(got[0, hit]).any()
    check("frames beside a NaN sample", got[:, keep], ref_mdct(np.nan_to_num(x).astype(np.float64), w)[:, keep])
    X = rows_of(M + 3, 1, F, M)
    X[0, 2, M // 3] = np.nan
    y, ref = T.imdct(ctx.to_device(X), w, ctx).numpy(), ref_imdct(np.nan_to_num(X), w)
    assert not np.isfinite(y[0, 2 * M:4 * M]).any()
    check("samples beside a NaN coefficient", np.delete(y, np.s_[2 * M:4 * M], axis=1), np.delete(ref, np.s_[2 * M:4 * M], axis=1))


@pytest.mark.parametrize("M", [256, 18])
def test_host_and_device_operands_give_the_same_bits(ctx, M):
    w, x, X = T.mdct_window("kbd", 2 * M), rows_of(1, 3, 5 * M + 1), rows_of(2, 3, 4, M)
    assert np.array_equal(T.mdct(x, w, ctx), T.mdct(ctx.to_device(x), w, ctx).numpy())
    assert np.array_equal(T.imdct(X, w, ctx), T.imdct(ctx.to_device(X), w, ctx).numpy())
