"""Spectral.welch / csd / coherence on the GPU against the f64 definition of tests/welch_oracle.py run on the SAME f32 samples and window.
The error of a row is max |err| / max |ref| over its bins (csd: ref = sqrt(Pxx Pyy)), bound 1e-5 (the suite's own; an f32 emulation of
these sums reads 2.3e-7 ... 3.0e-7).  Bit equalities: two calls, host against device memory, batched rows against single-row calls,
strided rows against plain buffers, clean rows next to a row that holds an Inf / NaN.  Dispatch families through ctx.last_dispatch().

Non-finite rule under test: a row (csd: the PAIR x_r, y_r) with an Inf / NaN inside the samples its frames cover is NaN in every bin of
EVERY result of that row — Pxx of a row whose y holds the NaN included; the dropped tail, the gap between rows and other rows reach
nothing."""
import ctypes as C

import numpy as np
import pytest

import extents as E
import welch_oracle as W

import nx_signal_amd as S
from nx_signal_amd import _lib, spectral

pytestmark = pytest.mark.gpu

TOL = 1e-5
WP, WG, CP, CG = "welch.pair", "welch.generic", "csd.pair", "csd.generic"


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Generic:
    """NXSIG_DISABLE_WELCH_WAVE on one context for a block"""

    def __init__(self, ctx, on=True):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_WELCH_WAVE", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_WELCH_WAVE")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def noise(seed, shape, offset=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(shape) + offset).astype(np.float32)


def hann(n):
    return S.windows.hann(n)


def dev_welch(ctx, x, w, **o):
    f, p = spectral.welch(ctx.to_device(x), w, **o)
    assert isinstance(p, S.DeviceBuffer) and f.dtype == np.float32
    ctx.sync()
    return p.numpy(), ctx.last_dispatch()


def dev_csd(ctx, x, y, w, **o):
    f, p = spectral.csd(ctx.to_device(x), ctx.to_device(y), w, **o)
    assert isinstance(p, S.DeviceBuffer) and p.dtype == np.complex64
    ctx.sync()
    return p.numpy(), ctx.last_dispatch()


def row_err(got, ref, scale=None):
    """largest per-row max |err| / max |scale| (scale: the reference itself unless given)"""
    got, ref = np.asarray(got), np.asarray(ref)
    scale = np.abs(ref) if scale is None else scale
    return float((np.abs(got - ref).max(-1) / scale.max(-1)).max())


def check_welch(name, p, x, w, **o):
    _, ref = W.welch(x, w, **o)
    assert p.shape == ref.shape and p.dtype == np.float32 and np.isfinite(p).all(), name
    err = row_err(p, ref)
    print(f"welch-accuracy {name}: {err:.3e}")
    assert err <= TOL, (name, err)


def check_csd(name, p, x, y, w, **o):
    _, ref = W.csd(x, y, w, **o)
    scale = np.sqrt(W.welch(x, w, **o)[1] * W.welch(y, w, **o)[1])
    assert p.shape == ref.shape and np.isfinite(p.view(np.float32)).all(), name
    err = row_err(p, ref, scale)
    print(f"welch-accuracy {name}: {err:.3e}")
    assert err <= TOL, (name, err)


# name, rows, length, N, overlap, K, family
FUSED = [
    ("1024-hop256-M37-tail", 3, 1024 + 36 * 256 + 100, 1024, 768, 1024),
    ("1024-hop256-M1", 3, 1024 + 100, 1024, 768, 1024),
    ("1024-hop256-M2", 3, 1024 + 256, 1024, 768, 1024),
    ("1024-hop1-M9", 3, 1032, 1024, 1023, 1024),
    ("1024-hop160", 3, 1024 + 20 * 160 + 7, 1024, 1024 - 160, 1024),
    ("1024-hop1024", 3, 5 * 1024 + 3, 1024, 0, 1024),
    ("400-in-1024", 3, 400 + 30 * 160, 400, 240, 1024),
    ("2048-hop512", 3, 2048 + 13 * 512 + 5, 2048, 1536, 2048),
]
GENERIC = [
    ("400-in-512", 3, 400 + 30 * 160, 400, 240, 512),
    ("255-odd", 3, 255 * 9 + 11, 255, 127, 255),
    ("64", 3, 64 * 70, 64, 32, 64),
]


# every fused shape on its own tier and again with the wave tier switched off; the generic shapes once
SHAPES = [(c, False) for c in FUSED + GENERIC] + [(c, True) for c in FUSED]


@pytest.mark.parametrize("case,forced", SHAPES, ids=[c[0] + ("-wave-off" if f else "") for c, f in SHAPES])
def test_welch_and_csd_shapes(ctx, case, forced):
    name, rows, length, n, overlap, k = case
    fused = case in FUSED and not forced
    x, y, w = noise(length + n, (rows, length)), noise(length + n + 1, (rows, length)), hann(n)
    o = dict(overlap_length=overlap, fft_length=k, sampling_rate=48000.0)
    with Generic(ctx, forced):
        p, rec = dev_welch(ctx, x, w, **o)
        assert (WP if fused else WG) in rec.split("+"), rec
        check_welch(f"welch {name} {'pair' if fused else 'generic'}", p, x, w, **o)
        q, rec = dev_csd(ctx, x, y, w, **o)
        assert (CP if fused else CG) in rec.split("+"), rec
        check_csd(f"csd {name} {'pair' if fused else 'generic'}", q, x, y, w, **o)


def test_one_long_row_is_split_over_many_runs(ctx):
    n = 20 * 48000
    x, w = noise(5, (1, n)), hann(1024)
    assert (n - 1024) // 256 + 1 == 3747
    o = dict(overlap_length=768, sampling_rate=48000.0)
    p, rec = dev_welch(ctx, x, w, **o)
    assert rec == WP
    check_welch("welch 1024 one row M=3747", p, x, w, **o)
    y = noise(6, (1, n))
    q, rec = dev_csd(ctx, x, y, w, **o)
    assert rec == CP
    check_csd("csd 1024 one row M=3747", q, x, y, w, **o)


@pytest.mark.parametrize("tier", ["generic", "pair"])
def test_rows_past_the_grid_limit(ctx, tier):
    """65 537 rows: 251 distinct rows repeated — the small call is held to the oracle, every row of the large one to the small call's bits
    (with one frame, or a row's own frame count below a run, the run geometry of a row does not depend on the batch; where it does —
    welch.pair / csd.pair with runs longer than four units — the bits change with the batch and the contract is tolerance:
    tests/test_gpu_call_size.py test_welch_and_csd_runs_longer_than_four_units)"""
    n, k, length, overlap = (64, 64, 96, 32) if tier == "generic" else (1024, 1024, 1024, 512)
    base, w = noise(65537, (251, length)), hann(n)
    o = dict(overlap_length=overlap, fft_length=k)
    small, rec = dev_welch(ctx, base, w, **o)
    assert (WG if tier == "generic" else WP) in rec.split("+")
    check_welch(f"welch {tier} 251 rows", small, base, w, **o)
    idx = np.arange(65537) % 251
    big, rec = dev_welch(ctx, base[idx], w, **o)
    assert (WG if tier == "generic" else WP) in rec.split("+") and big.shape == (65537, k // 2 + 1)
    assert same_bits(big, small[idx])


@pytest.mark.parametrize("tier", ["generic", "pair"])
@pytest.mark.parametrize("gap", [1, 3, 37])
def test_rows_that_are_not_on_a_16_byte_boundary(ctx, tier, gap):
    """rows length + gap elements apart, NaN pattern in the gaps and in the guards: nothing of it in a result, nothing written outside the
    result, every element written, the inputs unchanged, and the bits of the same call on plain buffers"""
    n, k, length, overlap = (100, 128, 100 + 7 * 40 + 9, 60) if tier == "generic" else (1024, 1024, 1024 + 6 * 256 + 31, 768)
    x, y, w = noise(gap, (3, length)), noise(gap + 50, (3, length)), hann(n)
    nb = k // 2 + 1
    o = dict(overlap_length=overlap, fft_length=k, sampling_rate=8000.0)
    dense, _ = dev_welch(ctx, x, w, **o)
    dense_xy, _ = dev_csd(ctx, x, y, w, **o)
    _, want = W.welch(x, w, **o)
    _, want_xy = W.csd(x, y, w, **o)
    lib = _lib.load()
    wp = w.ctypes.data_as(C.c_void_p)
    fw = lambda h, *a: lib.nxsig_welch_f32(_lib.ctx_ptr(h, _lib._ctx_spectral), *a)   # noqa: E731
    fc = lambda h, *a: lib.nxsig_csd_f32(_lib.ctx_ptr(h, _lib._ctx_spectral), *a)     # noqa: E731
    for offset in (1, 3):
        xin = E.Arena("x", np.float32, 3, length, length + gap, offset_elems=offset, data=x).upload(ctx)
        yin = E.Arena("y", np.float32, 3, length, length + gap, offset_elems=offset, data=y).upload(ctx)
        out = E.Arena("pxx", np.float32, 3, nb).upload(ctx)
        rec = E.call(ctx, fw, xin.ptr, length, 3, length + gap, wp, n, n - overlap, k, 1, 0, 8000.0, out.ptr, _lib.DEVICE)
        assert (WG if tier == "generic" else WP) in rec.split("+")
        E.verify([(xin, xin.download())], out, out.download(), expected=want.astype(np.float32), tol=TOL, same_bits_as=dense)
        oxy = E.Arena("pxy", np.complex64, 3, nb).upload(ctx)
        rec = E.call(ctx, fc, xin.ptr, yin.ptr, length, 3, length + gap, wp, n, n - overlap, k, 1, 0, 8000.0, None, None, oxy.ptr, _lib.DEVICE)
        assert (CG if tier == "generic" else CP) in rec.split("+")
        E.verify([(xin, xin.download()), (yin, yin.download())], oxy, oxy.download(), same_bits_as=dense_xy)
        assert row_err(oxy.tensor(oxy.download()), want_xy, np.sqrt(want * W.welch(y, w, **o)[1])) <= TOL
        # host memory: the arenas' images themselves
        ximg, oimg = xin.image.copy(), out.image.copy()
        E.call(ctx, fw, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), length, 3, length + gap, wp, n, n - overlap, k, 1, 0, 8000.0,
               C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
        E.verify([(xin, ximg)], out, oimg, expected=want.astype(np.float32), tol=TOL, same_bits_as=dense)


@pytest.mark.parametrize("forced", [False, True], ids=["pair", "generic"])
def test_detrend_of_a_large_offset(ctx, forced):
    """rows of 1000 + N(0, 1): one f32 pass over the mean leaves 3.9e-4 of the row maximum at the lowest bins, the bound is 1e-5"""
    x, w = noise(1000, (3, 1024 + 36 * 256), offset=1000.0), hann(1024)
    with Generic(ctx, forced):
        for detrend in ("constant", False):
            o = dict(overlap_length=768, detrend=detrend)
            p, rec = dev_welch(ctx, x, w, **o)
            assert (WG if forced else WP) in rec.split("+")
            check_welch(f"welch offset 1000 detrend={detrend} {'generic' if forced else 'pair'}", p, x, w, **o)
        y = noise(1001, x.shape, offset=-500.0)
        q, _ = dev_csd(ctx, x, y, w, overlap_length=768)
        check_csd(f"csd offsets 1000 / -500 {'generic' if forced else 'pair'}", q, x, y, w, overlap_length=768)


@pytest.mark.parametrize("forced", [False, True], ids=["pair", "generic"])
def test_rows_of_very_different_level_are_judged_on_their_own(ctx, forced):
    x, w = noise(3, (3, 1024 + 36 * 256)), hann(1024)
    x *= np.array([[1e-4], [1.0], [1e4]], np.float32)
    with Generic(ctx, forced):
        for scaling in ("density", "spectrum"):
            p, _ = dev_welch(ctx, x, w, overlap_length=768, scaling=scaling)
            check_welch(f"welch levels 1e-4 / 1 / 1e4 {scaling} {'generic' if forced else 'pair'}", p, x, w, overlap_length=768, scaling=scaling)


@pytest.mark.parametrize("forced", [False, True], ids=["pair", "generic"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_sample_poisons_its_row_and_nothing_else(ctx, forced, value):
    length = 1024 + 36 * 256 + 100   # M = 37, the last 100 samples are dropped
    x, y, w = noise(11, (3, length)), noise(12, (3, length)), hann(1024)
    o = dict(overlap_length=768)
    with Generic(ctx, forced):
        clean, _ = dev_welch(ctx, x, w, **o)
        clean_xy, _ = dev_csd(ctx, x, y, w, **o)
        for at in (0, 5000, 1024 + 36 * 256 - 1):          # first, some, and the last covered sample
            bad = x.copy()
            bad[1, at] = value
            p, _ = dev_welch(ctx, bad, w, **o)
            assert np.isnan(p[1]).all() and same_bits(p[0], clean[0]) and same_bits(p[2], clean[2]), at
        tail = x.copy()
        tail[1, length - 100:] = value                      # the dropped tail reaches nothing
        p, _ = dev_welch(ctx, tail, w, **o)
        assert same_bits(p, clean)
        # csd: the pair rule — a NaN in y poisons Pxy, Pyy, the coherence AND Pxx of that row
        bad_y = y.copy()
        bad_y[1, 777] = value
        _, pxy, pxx, pyy = spectral.csd(ctx.to_device(x), ctx.to_device(bad_y), w, return_auto=True, **o)
        pxx, pyy, pxy = pxx.numpy(), pyy.numpy(), pxy.numpy()
        assert np.isnan(pxy[1].view(np.float32)).all() and np.isnan(pyy[1]).all() and np.isnan(pxx[1]).all()
        assert same_bits(pxy[0], clean_xy[0]) and same_bits(pxy[2], clean_xy[2])
        assert np.isfinite(pxx[[0, 2]]).all() and np.isfinite(pyy[[0, 2]]).all()
        _, coh = spectral.coherence(ctx.to_device(x), ctx.to_device(bad_y), w, **o)
        coh = coh.numpy()
        assert np.isnan(coh[1]).all() and np.isfinite(coh[[0, 2]]).all()
        tail_y = y.copy()
        tail_y[1, length - 1] = value
        q, _ = dev_csd(ctx, x, tail_y, w, **o)
        assert same_bits(q, clean_xy)


@pytest.mark.parametrize("forced", [False, True], ids=["pair", "generic"])
def test_the_same_bits_every_time_from_host_and_device_batched_and_row_by_row(ctx, forced):
    x, y, w = noise(21, (4, 1024 + 36 * 256 + 100)), noise(22, (4, 1024 + 36 * 256 + 100)), hann(1024)
    o = dict(overlap_length=768, sampling_rate=16000.0)
    with Generic(ctx, forced):
        a, rec = dev_welch(ctx, x, w, **o)
        b, _ = dev_welch(ctx, x, w, **o)
        assert same_bits(a, b)
        f, h = spectral.welch(x, w, ctx=ctx, **o)
        assert isinstance(h, np.ndarray) and ctx.last_dispatch() == rec and same_bits(h, a)
        assert np.array_equal(f, (np.arange(513) * 16000.0 / 1024).astype(np.float32))
        qa, rec = dev_csd(ctx, x, y, w, **o)
        qb, _ = dev_csd(ctx, x, y, w, **o)
        _, qh = spectral.csd(x, y, w, ctx=ctx, **o)
        assert same_bits(qa, qb) and same_bits(qh, qa) and ctx.last_dispatch() == rec
        for r in range(4):
            p1, _ = dev_welch(ctx, x[r:r + 1], w, **o)
            q1, _ = dev_csd(ctx, x[r:r + 1], y[r:r + 1], w, **o)
            assert same_bits(p1[0], a[r]) and same_bits(q1[0], qa[r]), r
    assert ctx.get_tuning("DISABLE_WELCH_WAVE")[1] is False


@pytest.mark.parametrize("forced", [False, True], ids=["pair", "generic"])
def test_csd_of_a_filtered_copy_and_coherence(ctx, forced):
    rng = np.random.Generator(np.random.PCG64(31))
    length = 1024 + 60 * 256
    x = noise(31, (3, length))
    h = S.filters.firwin(65, [0.2])
    y = np.stack([np.convolve(r, h, mode="same") for r in x.astype(np.float64)])
    y = (y + 0.3 * rng.standard_normal(y.shape)).astype(np.float32)
    w = hann(1024)
    tag = "generic" if forced else "pair"
    with Generic(ctx, forced):
        for scaling in ("density", "spectrum"):
            o = dict(overlap_length=768, sampling_rate=48000.0, scaling=scaling)
            q, _ = dev_csd(ctx, x, y, w, **o)
            check_csd(f"csd y=fir(x)+noise {scaling} {tag}", q, x, y, w, **o)
            # csd(x, x) is welch(x): real within the bound
            p, _ = dev_welch(ctx, x, w, **o)
            qq, _ = dev_csd(ctx, x, x, w, **o)
            _, ref = W.welch(x, w, **o)
            assert row_err(qq.real, ref) <= TOL and row_err(p, ref) <= TOL
            assert float((np.abs(qq.imag).max(-1) / ref.max(-1)).max()) <= TOL
            _, coh = spectral.coherence(ctx.to_device(x), ctx.to_device(y), w, **o)
            coh = coh.numpy()
            _, cref = W.coherence(x, y, w, **o)
            print(f"welch-accuracy coherence {scaling} {tag}: {float(np.abs(coh - cref).max()):.3e}")
            assert coh.dtype == np.float32 and coh.min() >= 0.0 and coh.max() <= 1.0 + 1e-5
            _, one = spectral.coherence(x, x, w, ctx=ctx, **o)
            assert isinstance(one, np.ndarray) and float(np.abs(one - 1.0).max()) <= 1e-5
        # one frame: |conj(X) Y|^2 = |X|^2 |Y|^2
        _, c1 = spectral.coherence(x[:, :1024], y[:, :1024], w, ctx=ctx)
        assert float(np.abs(c1 - 1.0).max()) <= 1e-5


def test_through_the_nif_equals_the_ctypes_path(ctx):
    """welch/10 and csd/11 of nif/nxsig_nif.c with the terms elixir/lib/nx_signal_amd/spectral.ex builds: the bits of the Python call;
    badarg for a binary of the wrong size"""
    import nif_harness as H

    _, nctx = H.call("ctx_create", 0)
    x, y, w = noise(71, (3, 1024 + 9 * 256 + 5)), noise(72, (3, 1024 + 9 * 256 + 5)), hann(1024)
    length = x.shape[1]
    for k, fam in ((1024, "pair"), (1536, "generic")):
        o = dict(overlap_length=768, fft_length=k, sampling_rate=8000.0, scaling="spectrum")
        _, want = spectral.welch(x, w, ctx=ctx, **o)
        ok, pb, bins = H.call("welch", nctx, x, length, 3, w, 256, k, 1, 1, 8000.0)
        assert ok == "ok" and bins == k // 2 + 1 and pb == want.tobytes()
        assert H.call("last_dispatch", nctx)[1] in ("welch." + fam, ("welch." + fam).encode()) or fam == "generic"
        _, wxy, wxx, wyy = spectral.csd(x, y, w, ctx=ctx, return_auto=True, **o)
        ok, pxy, pxx, pyy, bins = H.call("csd", nctx, x, y, length, 3, w, 256, k, 1, 1, 8000.0)
        assert ok == "ok" and bins == k // 2 + 1 and pxy == wxy.tobytes() and pxx == wxx.tobytes() and pyy == wyy.tobytes()
    with pytest.raises(H.BadArg):
        H.call("welch", nctx, x[:, :-1], length, 3, w, 256, 1024, 1, 1, 8000.0)
    with pytest.raises(H.BadArg):
        H.call("csd", nctx, x, y[:, :-1], length, 3, w, 256, 1024, 1, 1, 8000.0)
    with pytest.raises(H.NifError) as ei:
        H.call("welch", nctx, x, length, 3, w, 0, 1024, 1, 1, 8000.0)
    assert "hop must be in" in str(ei.value)


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its WELCH_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_welch.json"""
    import json
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import abi_error_probe as P

    with open(P.GOLDEN_WELCH) as f:
        golden = json.load(f)["real_ctx"]
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.WELCH_TABLE_ENTRIES)
    assert table == golden
    for name in ("nxsig_welch_f32", "nxsig_csd_f32"):
        assert table[name]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
