"""How far does one frame's energy reach?  (third rule.)

The reference transforms frame by frame, so a frame's error is relative to that frame.  Most tuned kernels pack frames into a shared
complex transform (pair, quad, r20, rab, Bluestein, the half / quad inverses), and a quiet frame then carries the round-off of its
partners at the partners' level.  That is the documented limit of a packed unit; what these tests pin is that it STOPS there — at the
unit named in `accuracy_model.REACH` (read off the kernels, file:line beside every entry), never at a carried register, a neighbouring
unit or the first frame of the next row (rows are channels).

Signal (accuracy_model.mixed_signal): four rows — quiet noise (1e-4), the same noise with two one-hop bursts at level 1 (one at an
even hop index, one at an odd one: both unit alignments; 4 * reach frames apart and that far from the ends), a loud row, a quiet row
behind it (the row seam).  M is odd, so the last unit of every packing is ragged.  Hann window, `valid` padding, scaling nil.

Assertion: `frame_errors(z, ref, REACH[family])` — per frame, max norm and l2 norm, the denominator the loudest frame of the SAME row
within the family's reach — maximised over every frame of every row, is at most 3 x what the single-precision model (scipy on
complex64) reaches on the same frames against its OWN frame (reach 1).  No frame and no bin is left out.  The reference is double
precision (accuracy_model.stft_reference).  tests/test_accuracy_model_host.py shows on the CPU that a packing one frame wider than
documented, or one across the row seam, fails this.

NXSIG_ACCURACY_PROBE=1 prints every figure and asserts nothing (how profiles/accuracy/per_frame_accuracy.txt was filled)."""
import numpy as np
import pytest

import accuracy_model as A

import nx_signal_amd as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(geometry=None):
        if geometry not in made:
            made[geometry] = A.context(A.PAIR_GEOMETRIES[geometry] if geometry else None)
        return made[geometry]
    return get


def forward_case(contexts, key, table):
    K, hop, family, opts = table[key]
    padding, sink, cplx = opts.get("padding", "valid"), opts.get("sink", "spectrum"), opts.get("cplx", False)
    reach = A.reach_of(family)
    x, M = A.mixed_signal(K, hop, reach, padding, opts.get("M"), seed=K + hop, cplx=cplx)
    w = S.windows.hann(K)
    z, rec = A.run_stft(contexts(opts.get("geometry")), x, w, hop, K, padding, sink)
    A.assert_family(rec, family)
    ref = A.through_sink(A.stft_reference(x, w, hop, K, padding), sink)
    model = A.through_sink(A.stft_model(x, w, hop, K, padding), sink)
    assert z.shape == ref.shape and ref.shape[:2] == (4, M), (z.shape, ref.shape, M)
    assert np.isfinite(z).all()
    return z, ref, model, reach, f"K={K} hop={hop} M={M}" + ("" if padding == "valid" else " " + padding)


@pytest.mark.parametrize("key", list(A.FORWARD) + list(A.FORWARD_EXTRA))
def test_a_frame_is_bounded_at_the_level_of_its_unit(contexts, key):
    table = A.FORWARD if key in A.FORWARD else A.FORWARD_EXTRA
    z, ref, model, reach, shape = forward_case(contexts, key, table)
    m = A.worst(A.frame_errors(model, ref, 1))
    e = A.worst(A.frame_errors(z, ref, reach))
    A.check(table[key][2], shape, "mixed:" + key, m, e)


def test_the_pair_kernel_fails_at_reach_one(contexts):
    """the same data against every frame's OWN level: a quiet frame beside a burst carries the burst's round-off (a level ratio of
    1e4), so the test measures what it says.  This is the documented limit of the packed unit, not a defect."""
    z, ref, model, _, shape = forward_case(contexts, "pair-headline", A.FORWARD)
    m = A.worst(A.frame_errors(model, ref, 1))
    em, e2 = A.frame_errors(z, ref, 1)
    A.record([], "stft.pair", shape, "mixed:reach=1", m, (float(em.max()), float(e2.max())))
    if A.PROBE:
        return
    assert em.max() > A.MARGIN * m[0] and e2.max() > A.MARGIN * m[1]
    # ... and only in row 1, next to the bursts: rows 0, 2 and 3 are at one level each and stay at the model's
    for r in (0, 2, 3):
        assert em[r].max() <= A.MARGIN * m[0] and e2[r].max() <= A.MARGIN * m[1], r


@pytest.mark.parametrize("key", list(A.INVERSE))
def test_a_segment_is_bounded_at_the_level_of_its_frames_units(contexts, key):
    """spectra of noise at 1e-4, frames 13 and 30 of row 1 and all of row 2 at level 1 (M = 41 at N = 1024: several runs per row, so a
    loud frame sits in a run's recomputed halo)"""
    N, hop, family, M, opts = A.INVERSE[key]
    z = A.mixed_spectra(N, M, seed=N + hop + M)
    w = S.windows.hann(N)
    y, rec = A.run_istft(contexts(), z, w, hop, mask=opts.get("mask", False))
    A.assert_family(rec, family, opts.get("lead"))
    ref, model = A.istft_reference(z, w, hop), A.istft_model(z, w, hop)
    assert y.shape == ref.shape and np.isfinite(y).all()
    reach = A.reach_of(family, N)
    A.inverse_check(family, f"N={N} hop={hop} M={M}", "mixed:" + key, A.segment_errors(model, ref, hop, N, 1),
                    A.segment_errors(y, ref, hop, N, reach), N, hop, M)


@pytest.fixture(scope="module")
def fir_rows():
    x = A.mixed_rows(A.FIR_L, A.FIR_BURST, seed=60)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("taps", list(A.FIR))
def test_fir_rows_do_not_share_a_transform(contexts, fir_rows, taps):
    """the reference transforms a FIR row once, so only ROWS are separate: each row's error over its own row's peak.  The kernels
    filter two blocks as re / im of one transform — two rows in one transform would put row 2's round-off into rows 1 and 3."""
    h = S.filters.firwin(taps, [4000.0], sampling_rate=48000)
    ctx = contexts()
    y = np.asarray(S.filters.fir(fir_rows, h, mode="same", ctx=ctx))
    rec = ctx.last_dispatch()
    if A.PROBE:
        print(f"\nDISPATCH {A.FIR[taps]:<18} [{rec}]")
    else:
        assert rec.split("+")[0] == A.FIR[taps], rec
    ref = A.fir_reference(fir_rows, h)
    mm, m2 = A.row_errors(A.fir_model(fir_rows, h), ref)
    em, e2 = A.row_errors(y, ref)
    for r in range(4):
        A.check(A.FIR[taps], f"taps={taps} L={A.FIR_L}", f"mixed:row{r}", (float(mm[r]), float(m2[r])), (float(em[r]), float(e2[r])))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", list(A.FFT_ROWS))
def test_fft_rows_do_not_share_a_transform(contexts, K, inverse):
    """four c64 rows, rows 0 and 3 at 1e-4, rows 1 and 2 at 1: every row against its own level"""
    x = A.mixed_rows(K, K, seed=K, cplx=True)
    ctx = contexts()
    fn = S.transforms.ifft_nd if inverse else S.transforms.fft_nd
    z = np.asarray(fn(x, ctx=ctx, axes=[-1]))
    A.assert_family(ctx.last_dispatch(), A.FFT_ROWS[K])
    xd = x.astype(np.complex128)
    ref = A.clean(np.fft.ifft(xd, axis=-1) if inverse else np.fft.fft(xd, axis=-1))
    model = A.clean(A.scipy.fft.ifft(x, axis=-1) if inverse else A.scipy.fft.fft(x, axis=-1))
    assert model.dtype == np.complex64 and z.shape == ref.shape
    m = A.worst(A.row_errors(model, ref))
    e = A.worst(A.row_errors(z, ref))
    A.check(A.FFT_ROWS[K], f"K={K} rows=4", "mixed:" + ("ifft" if inverse else "fft"), m, e)
