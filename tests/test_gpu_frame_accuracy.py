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

    def get(geometry=None):
        if geometry not in made:
            made[geometry] = A.context(A.PAIR_GEOMETRIES[geometry] if geometry else None)
        return made[geometry]
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
