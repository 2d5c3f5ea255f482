"""istft_masked / spectrum_mask on the GPU: time-frequency masks fused into the inverse STFT (N = 1024) or applied by the two-step
form, for the three mask kinds, with broadcast rows, from host and device operands, and through the NIF.

The product is Nx.BinaryBackend's: formed in double, one rounding per component; a real gain multiplies each component on its own.
Bounds: bit identity between the fused and the two-step form and with the numpy product; against the oracle's istft of that
product the project's bound for this chain, nerr < 2e-4 on the interior (test_istft_filtered_is_bit_identical_to_multiply_then_istft)."""
import numpy as np
import pytest

import nif_harness as H
from oracle import nx_oracle as O

import nx_signal_amd as S

pytestmark = pytest.mark.gpu

BOUND = 2e-4
KIND_ID = {"real": 0, "onesided": 1, "complex": 2}


def nerr(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got.astype(np.complex128) - ref.astype(np.complex128))
    return float(d.max()) / max(float(np.max(np.abs(ref))), 1e-30)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_z(rng, lead, M, N):
    shape = tuple(lead) + (M, N)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def make_mask(rng, lead, M, N, kind):
    if kind == "complex":
        return make_z(rng, lead, M, N)
    return rng.standard_normal(tuple(lead) + (M, N if kind == "real" else N // 2 + 1)).astype(np.float32)


def mirrored(mask, N):
    """the full mask a one-sided one stands for: m_full[k] = m[k] for k <= N/2, else m[N - k]"""
    k = np.arange(N)
    return np.ascontiguousarray(mask[..., np.where(k <= N // 2, k, N - k)])


def product(z, mask, kind, N):
    """Nx.multiply on the BinaryBackend model: double, one rounding per component (componentwise for a real gain)"""
    zr, zi = z.real.astype(np.float64), z.imag.astype(np.float64)
    if kind == "complex":
        mr, mi = mask.real.astype(np.float64), mask.imag.astype(np.float64)
        re, im = zr * mr - zi * mi, zr * mi + zi * mr
    else:
        g = (mirrored(mask, N) if kind == "onesided" else mask).astype(np.float64)
        re, im = zr * g, zi * g
    out = np.empty(np.broadcast(zr, re).shape, np.complex64)
    out.real, out.imag = re.astype(np.float32), im.astype(np.float32)
    return out


def opts_of(N, hop, scaling):
    return dict(overlap_length=N - hop, fft_length=N, sampling_rate=16000, scaling=scaling)


@pytest.fixture(scope="module")
def ctx():
    return S.default_context()


def check_case(ctx, N, hop, scaling, rows, M, kind, expect_fused):
    rng = np.random.default_rng(1000 * N + hop + 7 * KIND_ID[kind] + M)
    z = make_z(rng, (rows,), M, N)
    mask = make_mask(rng, (rows,), M, N, kind)
    z0, m0 = z.copy(), mask.copy()
    w = S.windows.hann(N)
    opts = opts_of(N, hop, scaling)
    # the two-step form and its first step against the rule
    zm = S.spectrum_mask(z, mask)
    want_zm = product(z, mask, kind, N)
    assert zm.dtype == np.complex64 and zm.shape == want_zm.shape and np.array_equal(bits(zm), bits(want_zm))
    want = S.istft(zm, w, **opts)
    # host operands
    got = S.istft_masked(z, mask, w, **opts)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(z), bits(z0)) and np.array_equal(bits(mask), bits(m0))
    # device operands
    zd, md = ctx.to_device(z), ctx.to_device(mask)
    gd = S.istft_masked(zd, md, w, **opts)
    disp = ctx.last_dispatch()
    assert ("istft.wave.mask" in disp) == expect_fused, disp
    assert S.device.is_device(gd) and gd.shape == want.shape and np.array_equal(bits(gd.numpy()), bits(want))
    zmd = S.spectrum_mask(zd, md)
    assert S.device.is_device(zmd) and np.array_equal(bits(zmd.numpy()), bits(want_zm))
    assert np.array_equal(bits(zd.numpy()), bits(z0)) and np.array_equal(bits(md.numpy()), bits(m0))
    # the oracle's chain on the same product
    yo = O.istft(want_zm, w, **opts)
    inner = slice(N, -N) if yo.shape[-1] > 3 * N else slice(None)
    e = nerr(got[..., inner], yo[..., inner])
    print(f"N={N} hop={hop} scaling={scaling} rows={rows} M={M} {kind}: nerr {e:.3e} dispatch {disp}")
    assert e < BOUND


FUSED = [(1024, 256, None, 3, 41), (1024, 128, "spectrum", 2, 30), (1024, 512, "psd", 1, 9), (1024, 1024, None, 2, 5),
         (1024, 1024, None, 1, 1)]
DECLINED = [(1024, 256, None, 1, 6), (1024, 300, None, 2, 12), (512, 128, "spectrum", 2, 25), (2048, 512, None, 1, 11),
            (400, 160, None, 2, 14), (96, 24, None, 2, 20)]


@pytest.mark.parametrize("kind", ["real", "onesided", "complex"])
@pytest.mark.parametrize("N,hop,scaling,rows,M", FUSED)
def test_fused_geometries_are_bit_identical_to_mask_then_istft(ctx, N, hop, scaling, rows, M, kind):
    """N = 1024, hop 128 ... 1024, M >= 2R - 1: the mask rides in the inverse kernel.  hop == N runs the double-precision fix-up on
    every sample; (1024, 256, M = 41) is several kernel runs per row, so halo frames pick up their masks too."""
    check_case(ctx, N, hop, scaling, rows, M, kind, expect_fused=True)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("N,hop,scaling,rows,M", DECLINED)
def test_declined_geometries_take_the_two_step_form(ctx, N, hop, scaling, rows, M, kind):
    """too few frames, a hop or a length the fused kernel does not take: the product is materialised once, then the size's own inverse"""
    check_case(ctx, N, hop, scaling, rows, M, kind, expect_fused=False)


@pytest.mark.parametrize("N,hop,M", [(1024, 256, 41), (512, 128, 25)])
def test_onesided_mask_equals_its_mirrored_full_mask(ctx, N, hop, M):
    rng = np.random.default_rng(N + M)
    z = make_z(rng, (2,), M, N)
    m1 = make_mask(rng, (2,), M, N, "onesided")
    mf = mirrored(m1, N)
    assert mf.shape == (2, M, N) and np.array_equal(mf[..., N // 2 + 1:], m1[..., 1:N // 2][..., ::-1])
    w = S.windows.hann(N)
    opts = opts_of(N, hop, None)
    assert np.array_equal(bits(S.istft_masked(z, m1, w, **opts)), bits(S.istft_masked(z, mf, w, **opts)))
    assert np.array_equal(bits(S.spectrum_mask(z, m1)), bits(S.spectrum_mask(z, mf)))
    zd = ctx.to_device(z)
    a = S.istft_masked(zd, ctx.to_device(m1), w, **opts).numpy()
    b = S.istft_masked(zd, ctx.to_device(mf), w, **opts).numpy()
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", ["real", "onesided", "complex"])
@pytest.mark.parametrize("N,hop,M", [(1024, 256, 41), (512, 128, 25)])
def test_broadcast_rows_equal_the_tiled_call(ctx, N, hop, M, kind):
    """one mixture and S masks (the spectrum is read through a zero row stride), and one mask for S spectra"""
    rng = np.random.default_rng(3 * N + M + KIND_ID[kind])
    w = S.windows.hann(N)
    opts = opts_of(N, hop, None)
    z1, z3 = make_z(rng, (), M, N), make_z(rng, (3, 1), M, N)
    m1, m3 = make_mask(rng, (1,), M, N, kind), make_mask(rng, (3,), M, N, kind)
    # Bz = 1, Bm = 3: the result takes the mask's leading shape
    want = S.istft_masked(np.ascontiguousarray(np.broadcast_to(z1, (3,) + z1.shape)), m3, w, **opts)
    got = S.istft_masked(z1, m3, w, **opts)
    assert got.shape == want.shape == (3, want.shape[-1]) and np.array_equal(bits(got), bits(want))
    gd = S.istft_masked(ctx.to_device(z1), ctx.to_device(m3), w, **opts)
    assert gd.shape == want.shape and np.array_equal(bits(gd.numpy()), bits(want))
    sm = S.spectrum_mask(z1, m3)
    assert sm.shape == (3, M, N) and np.array_equal(bits(sm), bits(product(z1[None], m3, kind, N)))
    # Bz = 3, Bm = 1: the result takes the spectrum's leading shape
    want = S.istft_masked(z3, np.ascontiguousarray(np.broadcast_to(m1[0], (3, 1) + m1.shape[1:])), w, **opts)
    got = S.istft_masked(z3, m1, w, **opts)
    assert got.shape == want.shape == (3, 1, want.shape[-1]) and np.array_equal(bits(got), bits(want))
    gd = S.istft_masked(ctx.to_device(z3), ctx.to_device(m1), w, **opts)
    assert gd.shape == want.shape and np.array_equal(bits(gd.numpy()), bits(want))
    smd = S.spectrum_mask(ctx.to_device(z3), ctx.to_device(m1))
    assert smd.shape == (3, 1, M, N) and np.array_equal(bits(smd.numpy()), bits(product(z3, m1[0], kind, N)))


@pytest.mark.parametrize("kind", ["real", "onesided", "complex"])
def test_switch_sends_the_fused_cases_to_the_two_step_form(ctx, kind):
    N, hop, M = 1024, 256, 41
    rng = np.random.default_rng(99 + KIND_ID[kind])
    zd, md = ctx.to_device(make_z(rng, (2,), M, N)), ctx.to_device(make_mask(rng, (2,), M, N, kind))
    w = S.windows.hann(N)
    opts = opts_of(N, hop, "spectrum")
    fused = S.istft_masked(zd, md, w, **opts).numpy()
    assert "istft.wave.mask" in ctx.last_dispatch()
    ctx.set_tuning("NXSIG_DISABLE_FUSED_MASK", 1)
    try:
        two = S.istft_masked(zd, md, w, **opts).numpy()
        disp = ctx.last_dispatch()
    finally:
        ctx.clear_tuning("DISABLE_FUSED_MASK")
    assert "istft.wave.mask" not in disp and "spectrum_mask" in disp, disp
    assert np.array_equal(bits(fused), bits(two))


@pytest.mark.parametrize("frame", [7, 19])
@pytest.mark.parametrize("kind", ["real", "onesided", "complex"])
def test_a_nan_in_the_mask_reaches_exactly_the_reference_samples(ctx, kind, frame):
    """one NaN at a single (row, frame, bin): the non-finite output samples are those of the two-step form and of the oracle on the
    same product; frame 19 is the last one, whose mask row must not leak into the tail-flush frames"""
    N, hop, rows, M = 1024, 256, 2, 20
    rng = np.random.default_rng(4242 + KIND_ID[kind] + frame)
    z = make_z(rng, (rows,), M, N)
    mask = make_mask(rng, (rows,), M, N, kind)
    mask[1, frame, 37] = np.nan
    w = S.windows.hann(N)
    opts = opts_of(N, hop, None)
    zd, md = ctx.to_device(z), ctx.to_device(mask)
    fused = S.istft_masked(zd, md, w, **opts).numpy()
    assert "istft.wave.mask" in ctx.last_dispatch()
    zm = S.spectrum_mask(z, mask)
    two = S.istft(zm, w, **opts)
    yo = O.istft(product(z, mask, kind, N), w, **opts)
    bad = ~np.isfinite(yo)
    assert bad.any() and not bad[0].any()
    assert np.array_equal(~np.isfinite(fused), bad) and np.array_equal(~np.isfinite(two), bad)
    assert np.array_equal(~np.isfinite(S.istft_masked(z, mask, w, **opts)), bad)
    ok = ~bad
    ok[..., :N] = False
    ok[..., -N:] = False
    d = np.abs(fused.astype(np.complex128) - yo.astype(np.complex128))[ok]
    e = float(d.max()) / float(np.max(np.abs(yo[ok])))
    print(f"{kind} frame {frame}: {int(bad.sum())} non-finite samples, nerr of the finite interior {e:.3e}")
    assert e < BOUND
    assert np.array_equal(bits(fused[~bad]), bits(two[~bad]))


@pytest.fixture(scope="module")
def nctx():
    ok, c = H.call("ctx_create", 0)
    assert ok == "ok"
    yield c
    H.release_all()


@pytest.mark.parametrize("N,hop,M,rows", [(1024, 256, 12, 2), (512, 128, 9, 2)])
def test_through_the_nif_equals_the_ctypes_path(nctx, N, hop, M, rows):
    """one fused and one declined shape, host binaries and device buffers, the three mask kinds; and a broadcast spectrum"""
    params = (N, hop, N, 0, 0, 0, 0, 16000.0)
    w = S.windows.hann(N)
    opts = opts_of(N, hop, None)
    rng = np.random.default_rng(N + 5)
    z = make_z(rng, (rows,), M, N)
    for kind in ("real", "onesided", "complex"):
        mask = make_mask(rng, (rows,), M, N, kind)
        want, want_zm = S.istft_masked(z, mask, w, **opts), S.spectrum_mask(z, mask)
        ok, yb = H.call("istft_masked", nctx, z, rows, M, w, params, mask, KIND_ID[kind], rows)
        assert ok == "ok" and np.array_equal(np.frombuffer(yb, np.uint32), bits(want).reshape(-1))
        ok, ob = H.call("spectrum_mask", nctx, z, rows, mask, KIND_ID[kind], rows, M, N)
        assert ok == "ok" and np.array_equal(np.frombuffer(ob, np.uint32), bits(want_zm).reshape(-1))
        ok, zb = H.call("to_device", nctx, z)
        ok, mb = H.call("to_device", nctx, mask)
        ok, ybuf = H.call("istft_masked", nctx, zb, rows, M, w, params, mb, KIND_ID[kind], rows)
        ok, ydev = H.call("from_device", ybuf)
        assert np.array_equal(np.frombuffer(ydev, np.uint32), bits(want).reshape(-1))
        ok, obuf = H.call("spectrum_mask", nctx, zb, rows, mb, KIND_ID[kind], rows, M, N)
        ok, odev = H.call("from_device", obuf)
        assert np.array_equal(np.frombuffer(odev, np.uint32), bits(want_zm).reshape(-1))
        ok, zkeep = H.call("from_device", zb)
        assert np.array_equal(np.frombuffer(zkeep, np.uint32), bits(z).reshape(-1))
        with pytest.raises(H.BadArg):   # host spectrum with a device mask
            H.call("istft_masked", nctx, z, rows, M, w, params, mb, KIND_ID[kind], rows)
        with pytest.raises(H.BadArg):   # mask binary of the wrong size
            H.call("istft_masked", nctx, z, rows, M, w, params, mask[:, :-1], KIND_ID[kind], rows)
    mask = make_mask(rng, (rows,), M, N, "real")
    ok, yb = H.call("istft_masked", nctx, z[:1], 1, M, w, params, mask, 0, rows)
    assert np.array_equal(np.frombuffer(yb, np.uint32), bits(S.istft_masked(z[0], mask, w, **opts)).reshape(-1))
    with pytest.raises(H.BadArg):       # 2 spectra and 3 masks
        H.call("istft_masked", nctx, z, rows, M, w, params, np.concatenate([mask, mask[:1]]), 0, rows + 1)
