"""Is every kernel family as accurate as single precision allows?  (third rule: the measured coefficient.)

The suite's value tests bound `max |got - ref| / max |ref|` over a whole tensor of white noise by 1e-5: about 70 x above what the
kernels deliver, so a transform with twiddles from an f32 angle (2 x the error) or from a recurrence (100 x) passes all of them.
Here every family of the dispatch table — the shapes of tests/test_gpu_frame_isolation.py, two rows at equal level — is measured
PER FRAME (per hop-segment for the inverses) against a double-precision reference, in the max norm and the l2 norm, and bounded by
3 x what a native single-precision transform (scipy on complex64, accuracy_model.stft_model / istft_model) reaches on the same data
with the same statistic.  Own-frame metrics: reach 1 for the families that transform a frame alone, the family's reach
(accuracy_model.REACH) for the packed ones.

Inputs: white noise; an impulse per frame (rectangular window, hop = K — 420 in 441 for the 21 x 21 kernel, accuracy_model.FORWARD —, positions 0, 1, K/2 - 1, K/2, K - 1 and seeded random ones:
every output bin is one twiddle chain of magnitude 1, so the max norm is a per-bin figure); a bin-centred tone plus an off-bin tone at
1e-3 of it.  The inverses get the spectrum of an impulse (rectangular window too) and a one-bin spectrum instead, and are asserted
twice: over every hop-segment, and over the interior ones against the model's interior (accuracy_model.interior_segments says why).

The transforms beyond the LDS-resident kernels (kernels_nd.hip: the two-pass and the five-pass four-step, column transforms, the
chained Bluestein, and stft / istft / FIR / n-D fftconvolve built on them) are measured per row, column, frame or call in the same way,
on the smallest shapes that reach each piece of their arithmetic (accuracy_model.FFT_ROWS_LONG and the tables beside it): the pass-A
twiddle of the four-step is an f32 recurrence re-seeded from a table every eighth element, and tests/test_accuracy_model_host.py shows
that a re-seed period of 64 — inside the suite's 1e-5 — fails this bound.  For the chained Bluestein the model is the larger of the direct
transform and a single-precision chirp-z chain (accuracy_model.bluestein_f32).

NXSIG_ACCURACY_PROBE=1 prints every figure and asserts nothing (how profiles/accuracy/per_frame_accuracy.txt was filled)."""
import numpy as np
import pytest

import accuracy_model as A

import nx_signal_amd as S

pytestmark = pytest.mark.gpu

ROWS = 2


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(geometry=None, switches=None):
        key = geometry if not switches else tuple(sorted(switches.items()))
        if key not in made:
            made[key] = A.context(switches if switches else (A.PAIR_GEOMETRIES[geometry] if geometry else None))
        return made[key]
    return get


def forward_input(kind, K, hop, M, cplx, seed, impulse_n=None):
    """-> (x [ROWS, L], window, hop)"""
    if kind == "impulse":
        n = impulse_n or K
        x, w, hop = A.impulse_signal(K, M, ROWS, seed, n), np.ones(n, np.float32), n
    elif kind == "tone":
        x, w = A.tone_signal(K, hop, M, ROWS, seed), S.windows.hann(K)
    else:
        x, w = np.random.default_rng(seed).standard_normal((ROWS, (M - 1) * hop + K)).astype(np.float32), S.windows.hann(K)
    if cplx:
        x = (x + 1j * np.roll(x, 7, axis=-1)).astype(np.complex64)
    return x, w, hop


@pytest.mark.parametrize("kind", ["noise", "impulse", "tone"])
@pytest.mark.parametrize("key", list(A.FORWARD))
def test_forward_families_reach_single_precision(contexts, key, kind):
    K, hop, family, opts = A.FORWARD[key]
    M = A.forward_frames(K, hop, family, opts)
    x, w, hop = forward_input(kind, K, hop, M, opts.get("cplx", False), seed=3 * K + len(kind), impulse_n=opts.get("impulse_N"))
    z, rec = A.run_stft(contexts(opts.get("geometry")), x, w, hop, K)
    A.assert_family(rec, family)
    ref, model = A.stft_reference(x, w, hop, K), A.stft_model(x, w, hop, K)
    assert z.shape == ref.shape == (ROWS, M, K) and np.isfinite(z).all()
    reach = A.reach_of(family)
    m = A.worst(A.frame_errors(model, ref, reach))
    e = A.worst(A.frame_errors(z, ref, reach))
    A.check(family, f"K={K} hop={hop} M={M}", kind + ":" + key, m, e)


def inverse_input(kind, N, M, seed):
    if kind == "impulse":
        return A.impulse_spectra(N, M, ROWS, seed)
    if kind == "one-bin":
        return A.one_bin_spectra(N, M, ROWS, seed)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((ROWS, M, N)) + 1j * rng.standard_normal((ROWS, M, N))).astype(np.complex64)


@pytest.mark.parametrize("kind", ["noise", "impulse", "one-bin"])
@pytest.mark.parametrize("key", list(A.INVERSE))
def test_inverse_families_reach_single_precision(contexts, key, kind):
    N, hop, family, M, opts = A.INVERSE[key]
    z = inverse_input(kind, N, M, seed=5 * N + hop + len(kind))
    # the impulse spectra go through a RECTANGULAR window, like the forward impulses: under a Hann window the impulses at 0, 1 and
    # N - 1 are multiplied by 0 ... 1e-5, the first and last segments of a row hold nothing but round-off over a normaliser of 1e-9, and
    # a relative figure there measures the input, not the transform (profiles/accuracy/per_frame_accuracy.txt has the figures: k_istft_r20
    # read 1.8e-4 that way, an absolute error of 1.4e-8 over a neighbourhood whose loudest sample is 7.5e-5)
    w = np.ones(N, np.float32) if kind == "impulse" else S.windows.hann(N)
    y, rec = A.run_istft(contexts(), z, w, hop, mask=opts.get("mask", False))
    A.assert_family(rec, family, opts.get("lead"))
    ref, model = A.istft_reference(z, w, hop), A.istft_model(z, w, hop)
    assert y.shape == ref.shape and np.isfinite(y).all()
    reach = A.reach_of(family, N)
    A.inverse_check(family, f"N={N} hop={hop} M={M}", kind + ":" + key, A.segment_errors(model, ref, hop, N, reach),
                    A.segment_errors(y, ref, hop, N, reach), N, hop, M)


@pytest.mark.parametrize("taps", list(A.FIR))
def test_fir_rows_reach_single_precision(contexts, taps):
    x = np.random.default_rng(taps).standard_normal((ROWS, A.FIR_L)).astype(np.float32)
    h = S.filters.firwin(taps, [4000.0], sampling_rate=48000)
    ctx = contexts()
    y = np.asarray(S.filters.fir(x, h, mode="same", ctx=ctx))
    rec = ctx.last_dispatch()
    if A.PROBE:
        print(f"\nDISPATCH {A.FIR[taps]:<18} [{rec}]")
    else:
        assert rec.split("+")[0] == A.FIR[taps], rec
    ref = A.fir_reference(x, h)
    m = A.worst(A.row_errors(A.fir_model(x, h), ref))
    e = A.worst(A.row_errors(y, ref))
    A.check(A.FIR[taps], f"taps={taps} L={A.FIR_L}", "noise", m, e)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", list(A.FFT_ROWS))
def test_fft_rows_reach_single_precision(contexts, K, inverse):
    rng = np.random.default_rng(K + inverse)
    x = (rng.standard_normal((ROWS, K)) + 1j * rng.standard_normal((ROWS, K))).astype(np.complex64)
    ctx = contexts()
    fn = S.transforms.ifft_nd if inverse else S.transforms.fft_nd
    z = np.asarray(fn(x, ctx=ctx, axes=[-1]))
    A.assert_family(ctx.last_dispatch(), A.FFT_ROWS[K])
    xd = x.astype(np.complex128)
    ref = A.clean(np.fft.ifft(xd, axis=-1) if inverse else np.fft.fft(xd, axis=-1))
    model = A.clean(A.scipy.fft.ifft(x, axis=-1) if inverse else A.scipy.fft.fft(x, axis=-1))
    m = A.worst(A.row_errors(model, ref))
    e = A.worst(A.row_errors(z, ref))
    A.check(A.FFT_ROWS[K], f"K={K} rows={ROWS}", "noise:" + ("ifft" if inverse else "fft"), m, e)


@pytest.mark.parametrize("key", list(A.FORWARD_SINKS))
def test_forward_sinks_reach_single_precision(contexts, key):
    """the magnitude / one-sided sinks of the r20, rab and Bluestein front-ends on noise, measured like the FORWARD cases"""
    K, hop, family, opts = A.FORWARD_EXTRA[key]
    M = A.forward_frames(K, hop, family, opts)
    x, w, hop = forward_input("noise", K, hop, M, False, seed=3 * K + 5)
    z, rec = A.run_stft(contexts(), x, w, hop, K, sink=opts["sink"])
    A.assert_family(rec, family)
    ref = A.through_sink(A.stft_reference(x, w, hop, K), opts["sink"])
    model = A.through_sink(A.stft_model(x, w, hop, K), opts["sink"])
    assert z.shape == ref.shape == (ROWS, M, K // 2) and np.isfinite(z).all()
    reach = A.reach_of(family)
    A.check(family, f"K={K} hop={hop} M={M}", "noise:" + key, A.worst(A.frame_errors(model, ref, reach)), A.worst(A.frame_errors(z, ref, reach)))


def _noise_c64(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("kind", ["noise", "noise-padded", "impulse"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fft", "ifft"])
@pytest.mark.parametrize("key", list(A.FFT_ROWS_LONG))
def test_long_fft_rows_reach_single_precision(contexts, key, inverse, kind):
    """rows beyond the LDS-resident kernels: both four-step forms at every tile geometry that changes how pass A's twiddle recurrence
    walks, and the chained Bluestein.  noise-padded: n_in = K - 5, the padding is applied on load inside pass A.  impulse: one row per
    position of accuracy_model.long_impulse_positions; the inverse gets an impulse of height K, so that its output has magnitude 1
    like the forward one's — at height 1 the samples of a 2^21-point inverse are 5e-7, and one whose component lies within round-off of
    Nx.ifft's 1e-10 clean-up moves by 2e-4 of that, in the kernel or in the model as chance has it"""
    K, family, switches, rows = A.FFT_ROWS_LONG[key]
    if kind == "impulse":
        x = A.long_impulse_rows(K, A.LONG_IMPULSES, seed=K) * np.complex64(K if inverse else 1)
    else:
        x = _noise_c64(np.random.default_rng(K + inverse), (rows, K - 5 if kind == "noise-padded" else K))
    ctx = contexts(switches=switches)
    fn = S.transforms.ifft_nd if inverse else S.transforms.fft_nd
    z = np.asarray(fn(x, ctx=ctx, axes=[-1], lengths=[K]))
    A.assert_family(ctx.last_dispatch(), family)
    ref = A.fft_rows_reference(x, K, inverse)
    assert z.shape == ref.shape and np.isfinite(z).all()
    m = A.fft_rows_model_errors(x, K, inverse, ref, family)
    e = A.worst(A.row_errors(z, ref))
    A.check(family, f"K={K} rows={x.shape[0]}", f"{kind}:{'ifft' if inverse else 'fft'}:{key}", m, e)


@pytest.mark.parametrize("inverse", [False, True], ids=["fft", "ifft"])
@pytest.mark.parametrize("key", list(A.COLUMNS))
def test_column_transforms_reach_single_precision(contexts, key, inverse):
    """a transform along an axis that is not the fastest one, per column: the last listed axis is moved to the back and every
    (outer, inner) column measured as a row.  Reference and model fold over the axes like O.fft_nd, the clean-up after each"""
    shape, axes, lengths, family = A.COLUMNS[key]
    x = _noise_c64(np.random.default_rng(sum(shape) + inverse), shape)
    lengths = lengths or [shape[a] for a in axes]
    ctx = contexts()
    fn = S.transforms.ifft_nd if inverse else S.transforms.fft_nd
    z = np.asarray(fn(x, ctx=ctx, axes=axes, lengths=lengths))
    rec = ctx.last_dispatch()
    A.assert_family(rec, family)
    A.assert_noted(rec, "fft.tiled.columns")
    ref, model = x.astype(np.complex128), x
    for ax, n in zip(axes, lengths):
        ref = A.clean(np.fft.ifft(ref, n=n, axis=ax) if inverse else np.fft.fft(ref, n=n, axis=ax))
        model = A.clean(A.scipy.fft.ifft(model, n=n, axis=ax) if inverse else A.scipy.fft.fft(model, n=n, axis=ax))
    assert model.dtype == np.complex64 and z.shape == ref.shape and np.isfinite(z).all()

    def columns(t):
        return np.moveaxis(t, axes[-1], -1).reshape(-1, lengths[-1])
    m = A.worst(A.row_errors(columns(model), columns(ref)))
    e = A.worst(A.row_errors(columns(z), columns(ref)))
    label = "x".join(map(str, shape)) + " ax" + ",".join(map(str, axes)) + " K=" + ",".join(map(str, lengths))
    A.check("fft.tiled.columns", label, "noise:" + ("ifft" if inverse else "fft"), m, e)


@pytest.mark.parametrize("direction", ["stft", "istft"])
@pytest.mark.parametrize("key", list(A.LONG_FRAMES))
def test_long_frames_reach_single_precision(contexts, key, direction):
    """frames longer than the wave kernels take: every frame is a row of the long-row transforms (reach 1)"""
    N, K, hop, forward, inverse = A.LONG_FRAMES[key]
    M = A.LONG_FRAMES_M
    rng = np.random.default_rng(N + hop)
    w = S.windows.hann(N)
    if direction == "stft":
        x = rng.standard_normal((ROWS, (M - 1) * hop + N)).astype(np.float32)
        z, rec = A.run_stft(contexts(), x, w, hop, K)
        A.assert_family(rec, forward)
        ref, model = A.stft_reference(x, w, hop, K), A.stft_model(x, w, hop, K)
        assert z.shape == ref.shape == (ROWS, M, K) and np.isfinite(z).all()
        A.check(forward, f"K={K} hop={hop} M={M}", "noise:" + key, A.worst(A.frame_errors(model, ref, 1)), A.worst(A.frame_errors(z, ref, 1)))
    else:
        z = _noise_c64(rng, (ROWS, M, N))
        y, rec = A.run_istft(contexts(), z, w, hop)
        A.assert_family(rec, inverse)
        ref, model = A.istft_reference(z, w, hop), A.istft_model(z, w, hop)
        assert y.shape == ref.shape and np.isfinite(y).all()
        A.inverse_check(inverse, f"N={N} hop={hop} M={M}", "noise:istft-" + key, A.segment_errors(model, ref, hop, N, 1),
                        A.segment_errors(y, ref, hop, N, 1), N, hop, M)


@pytest.mark.parametrize("key", list(A.FIR_LONG))
def test_fir_long_rows_reach_single_precision(contexts, key):
    """more taps than the overlap-save kernels take: one transform of next_pow2(L + taps - 1) points per row"""
    taps, L, switches = A.FIR_LONG[key]
    x = np.random.default_rng(taps).standard_normal((ROWS, L)).astype(np.float32)
    h = S.filters.firwin(taps, [4000.0], sampling_rate=48000)
    ctx = contexts(switches=switches)
    y = np.asarray(S.filters.fir(x, h, mode="same", ctx=ctx))
    A.assert_family(ctx.last_dispatch(), "fir.long", "fir.long")
    if taps <= 4097:
        ref = A.fir_reference(x, h)
    else:
        # a direct sum of 1e9 products per row has no place in a test of seconds: a double-precision FFT convolution instead, whose
        # own error (~1e-15) is eight orders below what is measured here (~1e-7)
        s = (taps - 1) // 2
        ref = np.stack([A.scipy.signal.fftconvolve(r.astype(np.float64), h.astype(np.float64), mode="full")[s: s + L] for r in x])
    assert y.shape == ref.shape and np.isfinite(y).all()
    A.check("fir.long", f"taps={taps} L={L}", "noise:" + key, A.worst(A.row_errors(A.fir_model(x, h), ref)), A.worst(A.row_errors(y, ref)))


def _centered(full, shape):
    """apply_mode :same of the reference (convolution.ex:300-347): the middle `shape` of the full result, start div(full - new, 2)"""
    return full[tuple(slice((f - n) // 2, (f - n) // 2 + n) for f, n in zip(full.shape, shape))]


@pytest.mark.parametrize("mode", ["full", "same"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("shapes", A.CONV_ND, ids=lambda s: "x".join(map(str, s[0])) + "*" + "x".join(map(str, s[1])))
def test_fftconvolve_nd_reaches_single_precision(contexts, shapes, cplx, mode):
    """n-D fftconvolve against a direct double-precision convolution; max and l2 over the whole result of one call"""
    s1, s2 = shapes
    rng = np.random.default_rng(sum(s1) + cplx)
    a = _noise_c64(rng, s1) if cplx else rng.standard_normal(s1).astype(np.float32)
    b = rng.standard_normal(s2).astype(np.float32)
    ctx = contexts()
    got = np.asarray(S.convolution.fftconvolve(a, b, mode=mode, ctx=ctx))
    A.assert_noted(ctx.last_dispatch(), "fftconvolve_nd")
    ref = A.scipy.signal.convolve(a.astype(np.complex128 if cplx else np.float64), b.astype(np.float64), mode="full", method="direct")
    model = A.scipy.signal.fftconvolve(a, b, mode="full")
    assert model.dtype == (np.complex64 if cplx else np.float32)
    if mode == "same":
        ref, model = _centered(ref, s1), _centered(model, s1)
    assert got.shape == ref.shape and got.dtype == model.dtype and np.isfinite(got).all()

    def flat(t):
        return np.asarray(t).reshape(1, -1)
    m = A.worst(A.row_errors(flat(model), flat(ref)))
    e = A.worst(A.row_errors(flat(got), flat(ref)))
    A.check("fftconvolve_nd", "x".join(map(str, s1)) + "*" + "x".join(map(str, s2)), f"noise:{'c64' if cplx else 'f32'}:{mode}", m, e)
