"""Spectral.lpc on the GPU against the definition of include/nxsig.h restated in numpy long double.  The bar is the project's: per frame,
max |a - ref| <= 1e-5 max |ref|, k against max |k| and e against e_ref alike.  lpc.rows is forced with the value switch NXSIG_LPC_WAVE=0
(a context switch: no child process is needed)."""
import ctypes as C
import functools

import numpy as np
import pytest

import nx_signal_amd as S
from nx_signal_amd import _lib, spectral

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVE_LIMIT = 2048
LD = np.longdouble


def burg(x, p):
    """the definition on one frame: (a[0 ... p], k[0 ... p-1], e)"""
    x = x.astype(LD)
    f, b, a, ks = x[1:], x[:-1], np.ones(1, LD), []
    for _ in range(p):
        k = -2 * np.sum(f * b) / (np.sum(f * f) + np.sum(b * b) + LD(np.finfo(np.float64).tiny))
        a = np.append(a, 0)
        a = a + k * a[::-1]
        f, b = (f + k * b)[1:], (b + k * f)[:-1]
        ks.append(k)
    ks = np.array(ks)
    return a, ks, np.sum(x * x) / len(x) * np.prod(1 - ks * ks)


def reference(x, p, L, hop):
    out = [[burg(row[s:s + L], p) for s in range(0, len(row) - L + 1, hop)] for row in x]
    return tuple(np.array([[fr[i] for fr in row] for row in out], LD) for i in range(3))


def signal(kind, rows, n, seed):
    """f32 rows: white noise, the AR(4) process of pole radii 0.885 and 0.714, or that process plus 5 % noise"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((rows, n + 64))
    if kind == "noise":
        return e[:, 64:].astype(np.float32)
    y = np.zeros_like(e)
    for i in range(4, n + 64):
        y[:, i] = 2.2 * y[:, i - 1] - 2.3 * y[:, i - 2] + 1.3 * y[:, i - 3] - 0.4 * y[:, i - 4] + e[:, i]
    y = y[:, 64:]
    if kind == "ar4+noise":
        y = y + 0.05 * y.std() * rng.standard_normal(y.shape)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(kind, L, hop, p):
    n = L + 2 * hop + min(hop, 3)   # three frames and a ragged tail
    x = signal(kind, 2, n, L + hop + p)
    return x, reference(x, p, L, hop)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def run(ctx, x, p, L=None, hop=None, rows=False):
    """lpc with all three results on the context, on lpc.rows when asked, with the dispatch record checked against the plan"""
    if rows:
        ctx.set_tuning("LPC_WAVE", 0)
    try:
        got = spectral.lpc(x, p, L, hop, return_reflection=True, return_error=True, ctx=ctx)
        frame = x.shape[-1] if L is None else L
        assert ctx.last_dispatch() == ("lpc.rows" if rows or frame > WAVE_LIMIT else "lpc.wave"), ctx.last_dispatch()
    finally:
        if rows:
            ctx.clear_tuning("LPC_WAVE")
    return got


def check(what, got, ref):
    for name, g, r in zip("ake", got, ref):
        g = np.asarray(g.numpy() if isinstance(g, S.DeviceBuffer) else g, LD).reshape(r.shape)
        g, r = g.reshape(r.shape[0] * r.shape[1], -1), r.reshape(r.shape[0] * r.shape[1], -1)
        scale = np.abs(r).max(axis=1)
        worst = np.abs(g - r).max(axis=1)
        print(f"lpc-accuracy {what} {name}: {float(np.max(worst / np.maximum(scale, LD(1e-300)))):.3g}")
        assert np.all(worst <= TOL * scale), (what, name, worst / scale)


# (2, 1, 1): a single pair; (17, 5, 16): order L - 1, the pairs run down to one; 63 / 64 / 65: around a lane count; (129, 129, 128):
# the largest order, one sample past two slots per lane, no overlap; (1000, 250, 16): no multiple of anything; (1000, 1300, 16): hop
# beyond the frame; 2048 / 2049: the last frame of lpc.wave and the first of lpc.rows
SHAPES = [(2, 1, 1), (17, 5, 16), (63, 16, 8), (64, 16, 8), (65, 16, 8), (129, 129, 128), (1000, 250, 16), (1000, 1300, 16),
          (WAVE_LIMIT, 700, 32), (WAVE_LIMIT + 1, 700, 32)]


@pytest.mark.parametrize("rows", [False, True], ids=["default", "rows"])
@pytest.mark.parametrize("kind", ["ar4", "noise", "ar4+noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_against_the_definition(ctx, shape, kind, rows):
    L, hop, p = shape
    x, ref = case(kind, L, hop, p)
    got = run(ctx, x, p, L, hop, rows)
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape and got[2].shape == ref[2].shape[:2]
    check(f"{shape} {kind} {'rows' if rows else 'default'}", got, ref)


def test_whole_rows_of_many_chunks(ctx):
    """frame_length=None: 49 chunks of 4096 pairs and a ragged last one per row on lpc.rows"""
    x = signal("ar4+noise", 3, 200_000, 7)
    got = run(ctx, x, 64)
    assert got[0].shape == (3, 65) and got[1].shape == (3, 64) and got[2].shape == (3,)
    ref = tuple(np.array([burg(row, 64)[i] for row in x], LD)[:, None] for i in range(3))
    check("whole rows", got, ref)


def test_strided_rows_through_the_c_entry(ctx):
    """batch_stride > n: the Python mirror takes dense tensors only"""
    L, hop, p, n, stride = 65, 16, 8, 100, 131   # an odd stride: every row and frame start is misaligned differently
    x = signal("ar4", 3, stride, 11)
    frames = 1 + (n - L) // hop
    dx, da = ctx.to_device(x), ctx.empty((3, frames, p + 1), np.float32)
    _lib.check(_lib.load().nxsig_lpc_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(dx.ptr), 3, n, stride, L, hop, p,
                                         C.c_void_p(da.ptr), None, None, _lib.DEVICE))
    ref = reference(x[:, :n], p, L, hop)[0]
    assert frames == ref.shape[1]
    got = da.numpy().astype(LD)
    assert np.all(np.abs(got - ref).max(axis=2) <= TOL * np.abs(ref).max(axis=2))


@pytest.mark.parametrize("rows", [False, True], ids=["wave", "rows"])
def test_an_all_zero_frame(ctx, rows):
    L, hop, p = 64, 64, 8
    x = signal("ar4", 1, 3 * L, 3)
    clean = run(ctx, x, p, L, hop, rows)
    x[0, L:2 * L] = 0
    a, k, e = run(ctx, x, p, L, hop, rows)
    assert np.array_equal(a[0, 1], np.eye(1, p + 1, dtype=np.float32)[0]) and not k[0, 1].any() and e[0, 1] == 0
    for g, c in zip((a, k, e), clean):
        assert np.array_equal(g[0, [0, 2]].view(np.uint32), c[0, [0, 2]].view(np.uint32))


@pytest.mark.parametrize("rows", [False, True], ids=["wave", "rows"])
def test_non_finite_samples_stay_in_their_frames(ctx, rows):
    L, hop, p, n = 100, 30, 12, 700
    x = signal("ar4+noise", 2, n, 5)
    clean = run(ctx, x, p, L, hop, rows)
    bad = x.copy()
    bad[1, 215], bad[1, 480] = np.inf, np.nan
    got = run(ctx, bad, p, L, hop, rows)
    starts = np.arange(0, n - L + 1, hop)
    hit = np.zeros((2, len(starts)), bool)
    hit[1] = ((starts <= 215) & (215 < starts + L)) | ((starts <= 480) & (480 < starts + L))
    assert hit.any() and not hit.all()
    for g, c in zip(got, clean):
        g2, c2 = g.reshape(hit.shape + (-1,)), c.reshape(hit.shape + (-1,))
        assert np.array_equal(~np.isfinite(g2), np.broadcast_to(hit[..., None], g2.shape))
        assert np.array_equal(g2[~hit].view(np.uint32), c2[~hit].view(np.uint32))


@pytest.mark.parametrize("rows", [False, True], ids=["wave", "rows"])
def test_device_tensor_gives_the_same_bits(ctx, rows):
    x, _ = case("ar4", 65, 16, 8)
    got = run(ctx, ctx.to_device(x.reshape(2, 1, -1)), 8, 65, 16, rows)
    host = run(ctx, x, 8, 65, 16, rows)
    assert got[0].shape == (2, 1, 3, 9)
    for g, h in zip(got, host):
        assert isinstance(g, S.DeviceBuffer) and np.array_equal(g.numpy().reshape(h.shape).view(np.uint32), h.view(np.uint32))
    only_a = spectral.lpc(x, 8, 65, 16, ctx=ctx)
    assert np.array_equal(only_a.view(np.uint32), run(ctx, x, 8, 65, 16)[0].view(np.uint32))
