"""Filters.resample_poly on the GPU against the f64 oracle of tests/resample_oracle.py run on the SAME f32 taps: normalised max error
<= 1e-5 per row (the project's bound; a sequential-f32 model of these sums reads 0.3 ... 2.4e-7), no case or element left out.  Bit
equalities: batched rows against single-row calls, the two tiers, a non-reduced ratio against the reduced one, c64 against its planes,
host against device memory, clean rows next to a row that holds an Inf / NaN.  Dispatch families through ctx.last_dispatch().

Where no n gives exactly the wanted number of outputs (up > down skips lengths) the smallest n that gives at least that many is used."""
import ctypes as C

import numpy as np
import pytest

import extents as E
import resample_oracle as R

import nx_signal_amd as S
from nx_signal_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-5
LDS, GENERIC, COPY = "resample.poly.lds", "resample.poly.generic", "resample.copy"
RATIOS = [(1, 3), (3, 1), (1, 2), (2, 1), (2, 3), (3, 2), (7, 5), (147, 160), (160, 441)]
ZERO_TAPS = np.array([0.5, 0.0, 0.25, 0.0, 0.0, 1.0, 0.0, -0.5], np.float32)   # explicit taps with exact zeros in them


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(scope="module")
def tile():
    return int(_lib.load().nxsig_resample_tile())


class Generic:
    """NXSIG_DISABLE_RESAMPLE_LDS on one context for a block"""

    def __init__(self, ctx, on=True):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_RESAMPLE_LDS", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_RESAMPLE_LDS")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(ctx, x, up, down, **kw):
    """device in, device out: (result as numpy, dispatch record)"""
    y = S.filters.resample_poly(ctx.to_device(x), up, down, **kw)
    assert isinstance(y, S.DeviceBuffer)
    ctx.sync()
    return y.numpy(), ctx.last_dispatch()


def signal(seed, shape, dtype=np.float32):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def n_for(n_out, up, down):
    n = max(1, (n_out * down) // up - 2)
    while R.length(n, up, down) < n_out:
        n += 1
    return n


def taps_of(up, down, taps=None):
    """the f32 taps (gain included) a call uses"""
    up, down = R.reduce(up, down)
    return S.filters.resample_poly_taps(up, down) if taps is None else (np.float64(up) * np.asarray(taps, np.float64)).astype(np.float32)


def check(y, x, up, down, h):
    want = R.resample_poly_by_taps(x, up, down, h)
    assert y.shape == want.shape, (y.shape, want.shape)
    assert np.array_equal(np.isfinite(y), np.isfinite(want))
    err = R.nmax_err(y, want)
    print(f"resample {up}/{down} n={x.shape[-1]} rows={x.reshape(-1, x.shape[-1]).shape[0]} taps={h.shape[0]}: {err:.3e}")
    assert err <= TOL, (up, down, x.shape, err)


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_ratios_lengths_and_batches(ctx, tile, ratio):
    up, down = ratio
    h = taps_of(up, down)
    for n in [1, 2, 5] + [n_for(t, up, down) for t in (tile - 1, tile, tile + 1, 2 * tile + 1)]:
        x = signal(n * 31 + up, (3, n))
        y, rec = dev(ctx, x, up, down)
        assert rec == LDS and y.shape == (3, R.length(n, up, down))
        check(y, x, up, down, h)
        for k in range(3):
            y1, rec = dev(ctx, x[k:k + 1], up, down)
            assert rec == LDS and same_bits(y1[0], y[k]), (n, k)
    x = signal(48001 + up, (1, 48001))
    y, rec = dev(ctx, x, up, down)
    assert rec == LDS
    check(y, x, up, down, h)


def test_a_ratio_that_is_not_reduced_and_the_identity(ctx, tile):
    x = signal(46, (3, n_for(tile + 1, 2, 3)))
    a, rec_a = dev(ctx, x, 4, 6)
    b, rec_b = dev(ctx, x, 2, 3)
    assert rec_a == rec_b == LDS and same_bits(a, b)
    for xx in (x, signal(55, (2, 777), np.complex64)):
        y, rec = dev(ctx, xx, 5, 5)
        assert rec == COPY and same_bits(y, xx)
        y, rec = dev(ctx, xx, 5, 5, taps=[0.25, 0.5])          # scipy applies no filter either
        assert rec == COPY and same_bits(y, xx)
    yh = S.filters.resample_poly(x, 5, 5, ctx=ctx)
    assert isinstance(yh, np.ndarray) and same_bits(yh, x)


def test_explicit_taps(ctx, tile):
    x = signal(1, (3, 2 * tile + 7))
    y, rec = dev(ctx, x, 1, 2, taps=[1.0])                     # y[m] = x[2 m] exactly
    assert rec == LDS and same_bits(y, x[:, ::2])
    rng = np.random.Generator(np.random.PCG64(24))
    for L in (24, 25):
        t = rng.standard_normal(L).astype(np.float32)
        y, rec = dev(ctx, x, 3, 4, taps=t)
        assert rec == LDS
        check(y, x, 3, 4, taps_of(3, 4, t))
    # 7 taps at up = 16 (h = 16 * t is exact): branches r >= 7 are empty, the others hold one tap
    t = rng.standard_normal(7).astype(np.float32)
    h = taps_of(16, 1, t)
    for n in (5, tile // 16 + 3):
        xs = signal(n, (2, n))
        y, rec = dev(ctx, xs, 16, 1, taps=t)
        assert rec == LDS and y.shape == (2, 16 * n)
        m = np.arange(16 * n)
        q, r = (m + 3) // 16, (m + 3) % 16
        live = (r < 7) & (q < n)
        want = np.where(live, xs[:, np.minimum(q, n - 1)] * h[np.minimum(r, 6)], np.float32(0.0)).astype(np.float32)
        assert np.array_equal(y, want)                         # the single product, or zero
        assert np.all(bits(y[:, ~live]) == 0)                  # +0.0 exactly
        with Generic(ctx):
            yg, rec = dev(ctx, xs, 16, 1, taps=t)
        assert rec == GENERIC and same_bits(yg, y)
    # 20 001 taps: an 80 KB phase table is past the LDS tier
    t = (rng.standard_normal(20001) / 100).astype(np.float32)
    xs = signal(9, (2, 3001))
    y, rec = dev(ctx, xs, 3, 2, taps=t)
    assert rec == GENERIC
    check(y, xs, 3, 2, taps_of(3, 2, t))


@pytest.mark.parametrize("ratio", [(1, 3), (160, 441), (3, 2)], ids=lambda r: f"{r[0]}_{r[1]}")
def test_the_two_tiers_return_the_same_bits(ctx, tile, ratio):
    up, down = ratio
    for dtype in (np.float32, np.complex64):
        for n in (5, n_for(tile, up, down), n_for(3 * tile + 5, up, down)):
            x = signal(n + down, (3, n), dtype)
            a, rec_a = dev(ctx, x, up, down)
            with Generic(ctx):
                b, rec_b = dev(ctx, x, up, down)
            assert (rec_a, rec_b) == (LDS, GENERIC) and same_bits(a, b), (n, dtype)
    assert ctx.get_tuning("DISABLE_RESAMPLE_LDS")[1] is False


@pytest.mark.parametrize("ratio", [(1, 3), (3, 2)], ids=lambda r: f"{r[0]}_{r[1]}")
def test_complex_rows_are_their_two_planes(ctx, tile, ratio):
    up, down = ratio
    x = signal(64 + up, (3, n_for(tile + 1, up, down)), np.complex64)
    y, rec = dev(ctx, x, up, down)
    re, _ = dev(ctx, np.ascontiguousarray(x.real), up, down)
    im, _ = dev(ctx, np.ascontiguousarray(x.imag), up, down)
    assert rec == LDS and y.dtype == np.complex64
    assert same_bits(np.ascontiguousarray(y.real), re) and same_bits(np.ascontiguousarray(y.imag), im)
    check(y, x, up, down, taps_of(up, down))


@pytest.mark.parametrize("generic", [False, True], ids=["lds", "generic"])
def test_host_memory_equals_device_memory_and_any_host_axis(ctx, tile, generic):
    with Generic(ctx, generic):
        for dtype in (np.float32, np.complex64):
            x = signal(7, (2, 3, tile // 2 + 9), dtype)
            d, rec = dev(ctx, x, 2, 3)
            h = S.filters.resample_poly(x, 2, 3, ctx=ctx)
            assert isinstance(h, np.ndarray) and rec == ctx.last_dispatch() == (GENERIC if generic else LDS) and same_bits(h, d)
            xt = np.ascontiguousarray(np.moveaxis(x, -1, 0))
            for axis in (0, -3):
                ht = S.filters.resample_poly(xt, 2, 3, ctx=ctx, axis=axis)
                assert same_bits(ht, np.ascontiguousarray(np.moveaxis(d, -1, 0)))
    with pytest.raises(_lib.ArgumentError):
        S.filters.resample_poly(ctx.to_device(x), 2, 3, axis=0)


@pytest.mark.parametrize("dtype", [np.float32, np.complex64], ids=["f32", "c64"])
@pytest.mark.parametrize("generic", [False, True], ids=["lds", "generic"])
@pytest.mark.parametrize("ratio", [(1, 3), (3, 2)], ids=lambda r: f"{r[0]}_{r[1]}")
def test_extents_of_strided_and_offset_rows(ctx, tile, ratio, generic, dtype):
    """rows length + 5 elements apart that start 1 ... 3 elements off the allocation's alignment, NaN pattern in the gaps and in 4 KB on
    either side of both tensors: nothing of it in a result, nothing written outside y, every element of y written, x unchanged"""
    up, down = ratio
    h = taps_of(up, down)
    fn = lambda handle, *a: _lib.load().nxsig_resample_poly(_lib.ctx_ptr(handle), *a)   # noqa: E731
    n = n_for(tile + 1, up, down)
    n_out = R.length(n, up, down)
    x = signal(n + 3 * up, (3, n), dtype)
    want = R.resample_poly_by_taps(x, up, down, h)
    dense, _ = dev(ctx, x, up, down)
    for offset in (1, 2, 3):
        xin = E.Arena("x", dtype, 3, n, n + 5, offset_elems=offset, data=x).upload(ctx)
        out = E.Arena("y", dtype, 3, n_out).upload(ctx)
        with Generic(ctx, generic):
            rec = E.call(ctx, fn, xin.ptr, int(np.dtype(dtype).kind == "c"), n, 3, n + 5, h.ctypes.data_as(C.c_void_p), h.shape[0], up, down,
                         out.ptr, _lib.DEVICE)
        assert rec == (GENERIC if generic else LDS)
        E.verify([(xin, xin.download())], out, out.download(), expected=want.astype(dtype), tol=TOL, same_bits_as=dense)
        # host memory: the arenas' images themselves
        ximg, oimg = xin.image.copy(), out.image.copy()
        with Generic(ctx, generic):
            E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), int(np.dtype(dtype).kind == "c"), n, 3, n + 5,
                   h.ctypes.data_as(C.c_void_p), h.shape[0], up, down, C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
        E.verify([(xin, ximg)], out, oimg, expected=want.astype(dtype), tol=TOL, same_bits_as=dense)


@pytest.mark.parametrize("generic", [False, True], ids=["lds", "generic"])
@pytest.mark.parametrize("case", [(1, 3, None), (3, 2, None), (160, 441, None), (2, 3, ZERO_TAPS), (1, 2, ZERO_TAPS)],
                         ids=lambda c: f"{c[0]}_{c[1]}" + ("" if c[2] is None else "_zero_taps"))
def test_non_finite_samples_reach_the_outputs_of_the_definition_only(ctx, tile, case, generic):
    up, down, taps = case
    h = taps_of(up, down, taps)
    kw = {} if taps is None else {"taps": taps}
    n = max(n_for(tile + 1, up, down), 400)
    x = signal(100 + up, (3, n))
    with Generic(ctx, generic):
        clean, _ = dev(ctx, x, up, down, **kw)
        bad = x.copy()
        bad[1, 100], bad[1, 0] = np.inf, np.nan
        y, rec = dev(ctx, bad, up, down, **kw)
    assert rec == (GENERIC if generic else LDS)
    want = R.resample_poly_by_taps(bad, up, down, h)
    assert not np.isfinite(want[1]).all() and np.isfinite(want[1]).any()
    assert np.array_equal(np.isfinite(y), np.isfinite(want))                  # the set of non-finite outputs, exactly
    assert same_bits(y[0], clean[0]) and same_bits(y[2], clean[2])
    ok = np.isfinite(want[1])
    assert same_bits(y[1][ok], clean[1][ok])                                  # and what it does not reach is untouched
    assert float(np.abs(y[1][ok] - want[1][ok]).max() / np.abs(want[1][ok]).max()) <= TOL


def test_48k_to_16k_into_the_log_mel_front_end_stays_on_the_device(ctx):
    """3 x 1 s at 48 kHz -> resample_poly(., 1, 3) -> mel_spectrogram (400-sample frames, hop 160, 80 bands), all on DeviceBuffers: the
    bits of the same two calls with a host round trip in between"""
    x = signal(48, (3, 48000))
    w = S.windows.hann(400)
    opts = dict(overlap_length=240, fft_length=400, window_padding="reflect", sampling_rate=16000, mel_bins=80)
    y = S.filters.resample_poly(ctx.to_device(x), 1, 3)
    assert isinstance(y, S.DeviceBuffer) and y.shape == (3, 16000) and ctx.last_dispatch() == LDS
    mel = S.mel_spectrogram(y, w, **opts)
    assert isinstance(mel, S.DeviceBuffer)
    yh = S.filters.resample_poly(x, 1, 3, ctx=ctx)
    melh = S.mel_spectrogram(yh, w, ctx=ctx, **opts)
    assert isinstance(yh, np.ndarray) and same_bits(yh, y.numpy())
    assert melh.shape == (3, 101, 80) and same_bits(melh, mel.numpy()) and np.isfinite(melh).all()


def test_through_the_nif_equals_the_ctypes_path(ctx):
    """resample_poly/8 and resample_poly_dev/8 of nif/nxsig_nif.c with the terms elixir/lib/nx_signal_amd/filters.ex builds: the bits of
    the Python call; badarg for a binary of the wrong size or a buffer that is too short"""
    import nif_harness as H

    _, nctx = H.call("ctx_create", 0)
    for dtype, is_c in ((np.float32, 0), (np.complex64, 1)):
        x = signal(77 + is_c, (3, 2500), dtype)
        for up, down in ((1, 3), (3, 2)):
            h = taps_of(up, down)
            want, _ = dev(ctx, x, up, down)
            ok, yb, n_out = H.call("resample_poly", nctx, x, is_c, 2500, 3, h, up, down)
            assert ok == "ok" and n_out == want.shape[1] and yb == want.tobytes()
            _, xb = H.call("to_device", nctx, x)
            ok, ybuf, n_out = H.call("resample_poly_dev", nctx, xb, is_c, 2500, 3, h, up, down)
            assert ok == "ok" and n_out == want.shape[1] and H.call("from_device", ybuf)[1] == want.tobytes()
            assert H.call("last_dispatch", nctx)[1] in (LDS, LDS.encode())
            assert H.call("from_device", xb)[1] == x.tobytes()
            with pytest.raises(H.BadArg):
                H.call("resample_poly", nctx, x[:, :-1], is_c, 2500, 3, h, up, down)
            with pytest.raises(H.BadArg):   # one element too many
                H.call("resample_poly", nctx, np.concatenate([x.ravel(), x.ravel()[:1]]), is_c, 2500, 3, h, up, down)
            with pytest.raises(H.BadArg):
                H.call("resample_poly_dev", nctx, xb, is_c, 2501, 3, h, up, down)
    with pytest.raises(H.NifError) as ei:
        H.call("resample_poly", nctx, x, 1, 2500, 3, h, 0, 2)
    assert "up and down must be >= 1" in str(ei.value)


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its OWN_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_resample.json: every
    broken argument is refused with the recorded code and message (the probe refuses a broken case that returns 0, i.e. launches), and
    the valid row runs once with NXSIG_HOST and once with NXSIG_DEVICE, the two results equal bit for bit"""
    import json
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import abi_error_probe as P

    with open(P.GOLDEN_OWN) as f:
        golden = json.load(f)["real_ctx"]
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.OWN_TABLE_ENTRIES)
    assert table == golden
    assert table["nxsig_resample_poly"]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
