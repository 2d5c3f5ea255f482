"""The per-frame accuracy metric of tests/accuracy_model.py bites before anyone trusts it on a GPU: numpy stand-ins for a kernel (a
textbook f32 radix-2 FFT, its pair-packed form, and degraded variants of both) are measured exactly as
tests/test_gpu_frame_isolation.py and tests/test_gpu_frame_accuracy.py measure the HIP kernels — MARGIN x the single-precision model
on the same frames and the same statistic.  No GPU."""
import numpy as np
import pytest

import accuracy_model as A
from oracle import nx_oracle as O

HOP_DIV = 4


def _noise_case(K, M=9, rows=2, seed=5):
    x = np.random.default_rng(seed + K).standard_normal((rows, (M - 1) * (K // HOP_DIV) + K)).astype(np.float32)
    w = O.hann(K)
    return x, w, K // HOP_DIV


@pytest.fixture(scope="module")
def mixed():
    """the mixed-level signal of the isolation tests at the pair kernel's shape, with its reference and its model"""
    K, hop = 1024, 256
    x, M = A.mixed_signal(K, hop, reach=2, seed=11)
    w = O.hann(K)
    d = dict(K=K, hop=hop, M=M, fr=A.windowed_frames(x, w, hop), ref=A.stft_reference(x, w, hop, K), model=A.stft_model(x, w, hop, K))
    d["model_err"] = A.worst(A.frame_errors(d["model"], d["ref"], 1))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _within(err, model):
    return err[0] <= A.MARGIN * model[0] and err[1] <= A.MARGIN * model[1]


@pytest.mark.parametrize("K", [1024, 4096])
def test_a_textbook_f32_radix2_passes(K):
    x, w, hop = _noise_case(K)
    ref, model = A.stft_reference(x, w, hop, K), A.stft_model(x, w, hop, K)
    m = A.worst(A.frame_errors(model, ref, 1))
    e = A.worst(A.frame_errors(A.fft_radix2_f32(A.windowed_frames(x, w, hop)), ref, 1))
    print(f"K={K}: model {m}, radix-2 {e}")
    assert 5e-8 < m[1] < 3e-7          # the model is single precision, not double and not worse
    assert _within(e, m), (e, m)


def test_the_model_figures_are_those_of_single_precision():
    """scipy on complex64 input must not silently run in double: its per-frame l2 error is ~1.1e-7 at K = 1024"""
    x, w, hop = _noise_case(1024)
    z = A.stft_model(x, w, hop, 1024)
    assert z.dtype == np.complex64
    m = A.worst(A.frame_errors(z, A.stft_reference(x, w, hop, 1024), 1))
    assert 5e-8 < m[1] < 2.5e-7 and 5e-8 < m[0] < 1e-6, m


@pytest.mark.parametrize("K,least", [(1024, 6.0), (4096, 30.0)])
def test_recurrence_twiddles_fail(K, least):
    """w^(k+1) = w^k w in c64: 1.2e-5 at K = 1024 and 9e-5 at 4096 per frame (100 x and 760 x the model)"""
    x, w, hop = _noise_case(K)
    ref = A.stft_reference(x, w, hop, K)
    m = A.worst(A.frame_errors(A.stft_model(x, w, hop, K), ref, 1))
    e = A.worst(A.frame_errors(A.fft_radix2_f32(A.windowed_frames(x, w, hop), twiddles="recurrence"), ref, 1))
    print(f"K={K}: model {m}, recurrence {e}, ratio {e[1] / m[1]:.1f}")
    assert e[1] > A.MARGIN * m[1] and e[0] > A.MARGIN * m[0]
    assert e[1] > least * m[1]


def test_twiddles_from_an_f32_angle_are_measurably_worse():
    """cos / sin of an angle rounded to f32: about 2 x the model at K = 1024 — the figure the probe file is read against (a ratio
    above 1.5 is reported); recorded, not asserted against the margin (the issue measured 2.2 x: under the 3 x bound)"""
    x, w, hop = _noise_case(1024)
    ref = A.stft_reference(x, w, hop, 1024)
    m = A.worst(A.frame_errors(A.stft_model(x, w, hop, 1024), ref, 1))
    e = A.worst(A.frame_errors(A.fft_radix2_f32(A.windowed_frames(x, w, hop), twiddles="f32angle"), ref, 1))
    print(f"model {m}, f32-angle {e}, ratio {e[1] / m[1]:.2f}")
    assert e[1] > 1.5 * m[1]


def test_pair_packing_passes_at_reach_two_and_fails_at_reach_one(mixed):
    z = A.stft_pair_packed_f32(mixed["fr"])
    e2 = A.worst(A.frame_errors(z, mixed["ref"], 2))
    e1 = A.worst(A.frame_errors(z, mixed["ref"], 1))
    print(f"model {mixed['model_err']}, pair-packed reach 2 {e2}, reach 1 {e1}")
    assert _within(e2, mixed["model_err"]), (e2, mixed["model_err"])
    assert e1[0] > 100 * A.MARGIN * mixed["model_err"][0] and e1[1] > 100 * A.MARGIN * mixed["model_err"][1]   # a level ratio of 1e4


def test_the_unpacked_transform_passes_at_reach_one(mixed):
    e = A.worst(A.frame_errors(A.fft_radix2_f32(mixed["fr"]), mixed["ref"], 1))
    assert _within(e, mixed["model_err"]), (e, mixed["model_err"])


def test_a_packing_one_frame_wider_than_documented_fails(mixed):
    """frame f rides with frame f + 2: fails at reach 2, passes at reach 3"""
    z = A.stft_pair_packed_f32(mixed["fr"], stride=2)
    e2 = A.worst(A.frame_errors(z, mixed["ref"], 2))
    e3 = A.worst(A.frame_errors(z, mixed["ref"], 3))
    print(f"model {mixed['model_err']}, stride-2 packing reach 2 {e2}, reach 3 {e3}")
    assert not _within(e2, mixed["model_err"]) and e2[1] > 100 * mixed["model_err"][1]
    assert _within(e3, mixed["model_err"]), (e3, mixed["model_err"])


@pytest.mark.parametrize("reach", [2, 3, 16, 1000])
def test_a_packing_across_the_row_seam_fails_at_any_reach(mixed, reach):
    """M is odd: the last frame of row r rides with the first frame of row r + 1; row 3 (quiet) sits behind row 2 (loud)"""
    assert mixed["M"] % 2 == 1
    z = A.stft_pair_packed_f32(mixed["fr"], across_rows=True)
    em, e2 = A.frame_errors(z, mixed["ref"], reach)
    m = mixed["model_err"]
    assert not _within((em.max(), e2.max()), m)
    bad = np.argwhere(e2 > A.MARGIN * m[1])
    # rows 0 / 1 are paired straight (row 0 has an even start); what fails is a quiet frame that shared a transform with row 2
    assert {int(r) for r, _ in bad} <= {1, 2, 3} and any(int(r) == 3 for r, _ in bad), bad[:8]


def test_frame_errors_never_looks_at_another_row():
    ref = np.ones((3, 5, 8), np.complex128)
    ref[1] *= 1e6
    got = ref.copy()
    got[0, 2, 3] += 1e-3
    em, e2 = A.frame_errors(got, ref, 1000)
    assert em[0, 2] == pytest.approx(1e-3) and em[1].max() == 0 and em[2].max() == 0
    assert e2[0, 2] == pytest.approx(1e-3 / np.sqrt(8))


def test_neighbourhood_is_symmetric_and_strict():
    ref = np.full((1, 9, 4), 1e-4, np.complex128)
    ref[0, 4] = 1.0
    got = ref + 1e-8
    em, _ = A.frame_errors(got, ref, 1)
    assert em[0, 3] == pytest.approx(1e-4) and em[0, 4] == pytest.approx(1e-8)
    em, _ = A.frame_errors(got, ref, 3)          # |g - f| < 3: frames 2 .. 6 see frame 4
    assert np.allclose(em[0, 2:7], 1e-8) and np.allclose(em[0, [0, 1, 7, 8]], 1e-4)


def test_segment_errors_neighbourhood():
    """N / hop = 4, reach 1: segment s is covered by frames s - 3 .. s, which touch segments s - 3 .. s + 3"""
    hop, N, M = 8, 32, 12
    ref = np.full((1, M * hop + N - hop), 1e-4, np.complex128)
    ref[0, 7 * hop: 8 * hop] = 1.0
    got = ref + 1e-8
    em, _ = A.segment_errors(got, ref, hop, N, 1)
    assert em.shape == (1, M + 3)
    assert np.allclose(em[0, 4:11], 1e-8) and np.allclose(em[0, [0, 1, 2, 3, 11, 12]], 1e-4)
    em, _ = A.segment_errors(got, ref, hop, N, 2)
    assert np.allclose(em[0, 3:12], 1e-8) and np.allclose(em[0, [2, 12]], 1e-4)


def test_istft_model_is_the_oracle_chain_and_the_reference_is_close():
    rng = np.random.default_rng(2)
    N, hop, M = 256, 64, 11
    z = (rng.standard_normal((2, M, N)) + 1j * rng.standard_normal((2, M, N))).astype(np.complex64)
    w = O.hann(N)
    yo = O.istft(z, w, overlap_length=N - hop)
    ym = A.istft_model(z, w, hop)
    yr = A.istft_reference(z, w, hop)
    assert ym.shape == yo.shape == yr.shape
    assert np.max(np.abs(ym - yo)) / np.max(np.abs(yo)) < 1e-6           # the same chain, another single-precision transform
    m = A.worst(A.segment_errors(ym, yr, hop, N, 1))
    o = A.worst(A.segment_errors(yo, yr, hop, N, 1))
    assert o[1] < m[1] < 1e-6, (o, m)                                     # the oracle (double transform) is the closer of the two


def test_fir_model_and_reference():
    x = A.mixed_rows(6000, 500, seed=4)
    h = O.firwin(33, [0.25])
    m = A.row_errors(A.fir_model(x, h), A.fir_reference(x, h))
    assert m[0].shape == (4,) and 1e-8 < m[1].max() < 1e-6, m


@pytest.fixture(scope="module", params=[14, 17])
def long_rows(request):
    """rows of 2^lg points as the long-row GPU tests measure them: white noise and the impulse set (the five named positions and three
    seeded random ones), each with its double reference and the model's (max, l2)"""
    lg = request.param
    K = 1 << lg
    rng = np.random.default_rng(lg)
    inputs = {"noise": (rng.standard_normal((2, K)) + 1j * rng.standard_normal((2, K))).astype(np.complex64),
              "impulse": A.long_impulse_rows(K, 8, seed=lg)}
    d = {"lg": lg}
    for name, x in inputs.items():
        ref = A.fft_rows_reference(x, K, False)
        for v in (x, ref):
            v.setflags(write=False)
        d[name] = (x, ref, A.fft_rows_model_errors(x, K, False, ref, "fft.tiled"))
    return d


def _fourstep_errors(long_rows, kind, **form):
    x, ref, m = long_rows[kind]
    e = A.worst(A.row_errors(A.clean(A.fourstep_f32(x, long_rows["lg"], **form)), ref))
    print(f"2^{long_rows['lg']} {kind} {form}: model {m}, four-step {e}, ratio max {e[0] / m[0]:.2f} l2 {e[1] / m[1]:.2f}")
    return e, m


@pytest.mark.parametrize("kind", ["noise", "impulse"])
@pytest.mark.parametrize("form", [dict(twiddles="table"), dict(twiddles="recurrence", reseed=8)], ids=["table", "every-8"])
def test_a_fourstep_with_the_kernels_twiddles_passes(long_rows, kind, form):
    """the two-level table product at every element, and the recurrence re-seeded every eighth element (what k_fft_tile does)"""
    e, m = _fourstep_errors(long_rows, kind, **form)
    assert _within(e, m), (e, m)


@pytest.mark.parametrize("reseed", [64, None], ids=["every-64", "never"])
def test_a_fourstep_with_a_longer_twiddle_recurrence_fails(long_rows, reseed):
    """a re-seed period of 64, or none: both pass the suite's whole-tensor 1e-5 and must not pass here.  On noise both norms exceed the
    margin; on the impulse set the max norm (a per-bin figure) does"""
    e, m = _fourstep_errors(long_rows, "noise", twiddles="recurrence", reseed=reseed)
    assert e[0] > A.MARGIN * m[0] and e[1] > A.MARGIN * m[1], (e, m)
    e, m = _fourstep_errors(long_rows, "impulse", twiddles="recurrence", reseed=reseed)
    assert not _within(e, m) and e[0] > A.MARGIN * m[0], (e, m)


def test_a_fourstep_twiddle_from_an_f32_angle_stays_inside_the_margin(long_rows):
    """what the bound does NOT separate: one twiddle per element from an angle rounded to f32 reads 1.1 - 1.5 x the model here (the
    per-frame radix-2 form of it, with a rounded angle in every stage, about 2 x) — recorded, like the f32-angle case above"""
    for kind in ("noise", "impulse"):
        e, m = _fourstep_errors(long_rows, kind, twiddles="f32angle")
        assert _within(e, m), (e, m)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K", [5000, 10007])
def test_a_single_precision_bluestein_stays_near_the_direct_transform(K, inverse):
    """bluestein_f32 is the floor of fft.big.blue's algorithm: within the margin of the direct complex64 transform, under 2.5 x of it
    in both norms, and (trivially, being part of it) within its own model"""
    rng = np.random.default_rng(K)
    for name, x in (("noise", (rng.standard_normal((2, K - 5)) + 1j * rng.standard_normal((2, K - 5))).astype(np.complex64)),
                    ("impulse", A.long_impulse_rows(K, 8, seed=K))):
        ref = A.fft_rows_reference(x, K, inverse)
        direct = A.fft_rows_model_errors(x, K, inverse, ref, "fft.tiled")
        own = A.fft_rows_model_errors(x, K, inverse, ref, "fft.big.blue")
        e = A.worst(A.row_errors(A.clean(A.bluestein_f32(x, K, inverse)), ref))
        print(f"K={K} {name} inverse={inverse}: direct {direct}, bluestein {e}, ratio max {e[0] / direct[0]:.2f} l2 {e[1] / direct[1]:.2f}")
        assert 5e-8 < direct[1] < 3e-7, direct
        assert _within(e, direct) and _within(e, own), (e, direct, own)
        assert e[0] < 2.5 * direct[0] and e[1] < 2.5 * direct[1], (e, direct)
        assert own[0] >= direct[0] and own[1] >= direct[1]


def test_long_impulse_positions_are_the_named_ones():
    p = A.long_impulse_positions(1 << 15, 8, seed=1)
    assert list(p[:5]) == [1, 127, 129, (1 << 14) + 1, (1 << 15) - 1] and len(p) == 8 and (p < (1 << 15)).all()
    x = A.long_impulse_rows(1 << 15, 8, seed=1)
    assert x.shape == (8, 1 << 15) and (np.abs(x).sum(axis=-1) == 1).all() and (np.argmax(np.abs(x), axis=-1) == p).all()


def test_every_long_case_names_a_family_with_a_reach():
    for K, family, switches, rows in A.FFT_ROWS_LONG.values():
        assert A.reach_of(family) == 1 and rows == 2 and K >= 4097
    for key in A.FORWARD_SINKS:
        K, hop, family, opts = A.FORWARD_EXTRA[key]
        assert A.reach_of(family) == A.reach_of("stft." + family.split(".")[1]) and opts["sink"] in ("magnitude", "onesided")


def test_family_of_reads_dispatch_records():
    assert A.family_of("stft.pair.1r+stft.pair.1r.edge") == "stft.pair"
    assert A.family_of("stft.pair+stft.pair.h4") == "stft.pair"
    assert A.family_of("stft.real2x.4k") == "stft.real2x.4k" and A.family_of("stft.real2x") == "stft.real2x"
    assert A.family_of("istft.wave.deep+istft.edge_chunks") == "istft.wave"
    assert A.family_of("istft.wave.mask+istft.edge_chunks") == "istft.wave.mask"
    assert A.family_of("istft.rab.q") == "istft.rab.q" and A.family_of("istft.rab+istft.edge_chunks") == "istft.rab"
    assert A.family_of("fft.rows_generic.blue+istft.generic+istft.edge_fix") == "fft.rows_generic"
    assert A.family_of("stft.big+fft.tiled+fft.tiled") == "stft.big" and A.family_of("fft.tiled+fft.tiled") == "fft.tiled"
    assert A.family_of("fft.tiled.columns") == "fft.tiled.columns" and A.family_of("fft.transpose+fft.rows_wave") == "fft.transpose"
    assert A.family_of("mag.rab") == "mag.rab" and A.family_of("mel.rab") is None
    assert A.reach_of("istft.quad", 256) == 4 and A.reach_of("stft.quad8") == 16


def test_every_reach_entry_cites_its_kernel():
    """REACH is read off the kernels: every entry carries a file:line of its own"""
    import inspect
    import re
    src = inspect.getsource(A)
    body = src[src.index("REACH = {"): src.index("\n}\n", src.index("REACH = {"))]
    entries = [ln for ln in body.splitlines() if re.match(r'\s*"[a-z_0-9.]+":', ln)]
    assert len(entries) == len(A.REACH)
    for ln in entries:
        assert re.search(r"[\w/]+\.(hip|hpp):\d+", ln), ln
