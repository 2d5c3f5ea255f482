"""A result does not depend on the launch geometry: every streaming kernel at every geometry its switches can force,
on shapes of a few dozen frames, bit for bit against the default geometry.

At the shapes of the other correctness modules `fill_units_per_wave` gives every wave ONE unit and `istft_min_run` every run TWO frames
(tests/test_launch_geometry_host.py shows it from the launcher arithmetic), so the software-pipelined parts of the kernels — the next
unit's loads under this unit's butterflies, the peeled last unit, `load_direct` under the stores, the carry strip and the pending sums
at a run seam — run at production sizes only.  Here `NXSIG_WAVE_UNITS_PER_WAVE`, `NXSIG_FIR_UNITS_PER_WAVE`, `NXSIG_WAVE_SMALL_CHUNK` /
`NXSIG_WAVE_SMALL_W`, `NXSIG_ISTFT_MIN_RUN` and `NXSIG_ISTFT_RUNS_PER_CU` force them on the cases of tests/launch_geometry.py:

* BASELINE: a fresh context without geometry switches.  The dispatch record must name the case's family and the result is checked
  against the reference the way that family is checked elsewhere — per frame (per hop-segment) at accuracy_model.MARGIN x the
  single-precision model where the family is in accuracy_model.REACH, the suite's global bounds otherwise (1e-5 of the largest
  reference value; 1e-4 absolute for log-mel).  The inverses get both: the global bound says little under a Hann window (the largest
  reference value is an edge sample over a normaliser of 1e-9), so the packed and filtered inverses are held to the per-segment bound
  as well, at the reach read off their kernels, and so are the short rows.
* EVERY GEOMETRY, finite data: the same leading family (the suffixes .1r / .h4 / .deep the geometry itself selects aside) and the same
  uint32 words as the baseline.  Because of that, the one accuracy check covers all of them.
* EVERY GEOMETRY, non-finite twin: a NaN in the middle of row 1, an Inf in the last frame of row 0 and in the first frame of row 2
  (bins of those frames for the inverses): the same set of non-finite outputs and the same words in every finite one.

* FIR: that twin poisons all three rows (a non-finite sample leaves no finite output in its row), so a second twin holds the NaN of row 1
  alone and the words of rows 0 and 2 are compared beside a poisoned row.
* NXSIG_ISTFT_RUNS_PER_CU cannot change the launch of a 3-row call (fewer units than compute units): its `-1cu` twins above launch the
  runs of their partners.  One case per launcher form that reads it runs on 17 - 65 rows as well, where 1, 2 and 4096 waves per CU
  give runs of 5, 3 and 1 units.

A difference is reported with its first (row, frame, bin) or (row, sample) and the unit, wave and chunk — or the run — that owns it
under that geometry.  No family needed an exception: bit equality holds for all of them."""
import numpy as np
import pytest

import accuracy_model as A
import launch_geometry as G
from oracle import nx_oracle as O

import nx_signal_amd as S

pytestmark = pytest.mark.gpu

f32, c64 = np.float32, np.complex64
GLOBAL_BOUND = 1.0e-5        # max |got - ref| / max |ref|: the bound of tests/test_gpu_tuned_kernels.py and tests/test_gpu_parity.py
MEL_BOUND = 1.0e-4           # absolute, log10 units: test_composite_lengths_fused_sinks
MEL_BINS, MEL_FS = 80, 16000


@pytest.fixture(scope="module")
def contexts():
    """one context per distinct switch setting, shared by every case of the module"""
    made = {}

    def get(knobs):
        key = tuple(sorted(knobs.items()))
        if key not in made:
            ctx = S.Context(0)
            ctx.clear_tuning()                  # whatever the environment set: a case names its switches itself
            for name, v in key:
                ctx.set_tuning(name, v)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def stem(record):
    """leading entry of a dispatch record without the suffixes a geometry selects"""
    first = record.split("+")[0]
    again = True
    while again:
        again = False
        for suffix in (".1r", ".h4", ".deep"):
            if first.endswith(suffix):
                first, again = first[: -len(suffix)], True
    return first


def elementwise_finite(a):
    return np.isfinite(a)          # a complex element is finite when both components are


def first_difference(got, base):
    """None when `got` has the baseline's non-finite elements and the baseline's words in every finite one, else (index, what)"""
    assert got.shape == base.shape and got.dtype == base.dtype, (got.shape, base.shape, got.dtype, base.dtype)
    fg, fb = elementwise_finite(got), elementwise_finite(base)
    if not np.array_equal(fg, fb):
        idx = tuple(int(i) for i in np.argwhere(fg != fb)[0])
        return idx, f"finite in one, not in the other (got {got[idx]!r}, baseline {base[idx]!r})"
    wg = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape + (-1,))
    wb = np.ascontiguousarray(base).view(np.uint32).reshape(base.shape + (-1,))
    differ = (wg != wb).any(axis=-1) & fb
    if differ.any():
        idx = tuple(int(i) for i in np.argwhere(differ)[0])
        return idx, f"got {got[idx]!r}, baseline {base[idx]!r}; {int(differ.sum())} of {differ.size} elements differ"
    return None


def assert_same_bits(got, base, label, owner):
    d = first_difference(got, base)
    assert d is None, f"{label}: first difference at {d[0]}: {d[1]}; owner under this geometry: {owner(d[0])}"


# ------------------------------------------------------------------------------------------------------------------------- forward
def forward_input(case, twin):
    rng = np.random.default_rng(1000 + sum(map(ord, case.key)))
    if case.kind == "rows":
        x = (rng.standard_normal((case.rows, case.K)) + 1j * rng.standard_normal((case.rows, case.K))).astype(c64)
    else:
        x = rng.standard_normal((case.rows, case.L)).astype(f32)
        if case.entry == "stft_c64":
            x = (x + 1j * np.roll(x, 7, axis=-1)).astype(c64)
    if twin:
        n = x.shape[-1]
        x[1, n // 2] = np.nan          # the middle of row 1: R frames hold it
        x[0, n - 1] = np.inf           # the last frame of row 0 only
        x[2, 0] = -np.inf              # the first frame of row 2 only
    return x


def forward_window(case):
    return S.windows.hann(case.K)


def run_forward(ctx, case, x):
    opts = dict(overlap_length=case.K - case.hop, fft_length=case.K)
    if case.entry in ("stft", "stft_c64"):
        out = S.stft(x, forward_window(case), ctx=ctx, **opts)[0]
    elif case.entry == "magnitude":
        out = S.spectrogram(x, forward_window(case), ctx=ctx, kind="magnitude", **opts)[0]
    elif case.entry == "mel":
        out = S.mel_spectrogram(x, forward_window(case), ctx=ctx, mel_bins=MEL_BINS, sampling_rate=MEL_FS, **opts)
    else:
        out = S.transforms.fft_nd(x, ctx=ctx, axes=[-1])
    return np.asarray(out), ctx.last_dispatch()


def assert_forward_family(case, record):
    if case.family in A.REACH:
        A.assert_family(record, case.family)
    else:
        assert stem(record) == case.family, f"dispatched to [{record}], the case is about [{case.family}]"


def check_forward_baseline(case, x, got):
    w = forward_window(case)
    shape = f"K={case.K} hop={case.hop} M={case.M} rows={case.rows}"
    if case.entry == "fft_nd":
        ref = A.clean(np.fft.fft(x.astype(np.complex128), axis=-1))
        model = A.clean(A.scipy.fft.fft(x, axis=-1))
        assert got.shape == ref.shape and np.isfinite(got).all()
        A.check(case.family, shape, "noise", A.worst(A.row_errors(model, ref)), A.worst(A.row_errors(got, ref)))
        return
    ref = A.stft_reference(x, w, case.hop, case.K)
    assert ref.shape == (case.rows, case.M, case.K)
    if case.entry == "mel":
        zo = np.stack([O.stft(r, w, overlap_length=case.K - case.hop, fft_length=case.K, sampling_rate=MEL_FS)[0] for r in x])
        melo = O.stft_to_mel(zo.reshape(-1, case.K), MEL_FS, case.K, MEL_BINS).reshape(case.rows, case.M, MEL_BINS)
        assert got.shape == melo.shape and np.isfinite(got).all()
        err = float(np.max(np.abs(got - melo)))
        print(f"\nBASELINE {case.key}: log-mel max abs error {err:.3e}")
        assert err < MEL_BOUND, (case.key, err)
        return
    sink = "magnitude" if case.entry == "magnitude" else "spectrum"
    ref = A.through_sink(ref, sink)
    assert got.shape == ref.shape and np.isfinite(got).all()
    if case.family in A.REACH:
        model = A.through_sink(A.stft_model(x, w, case.hop, case.K), sink)
        reach = A.reach_of(case.family)
        A.check(case.family, shape, "noise", A.worst(A.frame_errors(model, ref, reach)), A.worst(A.frame_errors(got, ref, reach)))
    else:
        err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        print(f"\nBASELINE {case.key}: max error / max reference {err:.3e}")
        assert err < GLOBAL_BOUND, (case.key, err)


@pytest.mark.parametrize("key", list(G.FORWARD))
def test_forward_kernels_give_the_same_bits_at_every_geometry(contexts, key):
    case = G.FORWARD[key]
    base_knobs = dict(case.base)
    geometries = G.forward_geometries(case)
    for twin in (False, True):
        x = forward_input(case, twin)
        base, rec0 = run_forward(contexts(base_knobs), case, x)
        assert_forward_family(case, rec0)
        if not twin:
            check_forward_baseline(case, x, base)
        else:
            bad = ~np.isfinite(base)
            assert bad.any() and (case.entry == "mel" or not bad.all())       # (log-mel: one non-finite frame makes the whole result NaN)
        for name, knobs in geometries.items():
            got, rec = run_forward(contexts({**base_knobs, **knobs}), case, x)
            assert stem(rec) == stem(rec0), f"{key} {name}: dispatched to [{rec}], the baseline to [{rec0}]"
            launch = G.forward_launch(case, knobs)
            assert_same_bits(got, base, f"{key} {name} {knobs}{' non-finite twin' if twin else ''}",
                             lambda idx: (launch, launch.owner(idx[0], idx[1] if case.kind != "rows" else 0)))


def test_a_forced_chunk_is_taken_as_it_is_and_never_changes_the_spectrum(contexts):
    """NXSIG_WAVE_SMALL_CHUNK is neither rounded nor refused.  The heuristic rounds its own chunk to a multiple of four pairs
    (kernels_wave.hip:1155) for balance only: the pair kernel walks any chunk with `for (pr = p_begin + wave; pr + W < p_end; pr += W)`
    plus the peeled last unit (wave_stft.hpp:1048-1067), a wave without a unit loads an existing unit and uses nothing of it (:749), so
    a chunk of 1, 3, 5 or 18 pairs on 12 waves is as correct as one of 16.  Pinned: the switch accepts the values, the launch reports the
    one-round kernel, and the spectrum — under a scaling too, with a non-finite sample too — has the bits of the default geometry."""
    case = G.FORWARD["pair-hop256"]
    w = forward_window(case)
    for twin in (False, True):
        x = forward_input(case, twin)
        opts = dict(overlap_length=case.K - case.hop, fft_length=case.K, scaling="spectrum", sampling_rate=48000)
        ctx0 = contexts({})
        base = np.asarray(S.stft(x, w, ctx=ctx0, **opts)[0])
        assert ctx0.last_dispatch().split("+")[0] == "stft.pair.1r"
        for ch in G.SMALL_CHUNKS:
            for small_w in (None, 0):
                knobs = {G.SMALL_CHUNK: ch, **({} if small_w is None else {G.SMALL_W: 0})}
                ctx = contexts(knobs)
                assert ctx.get_tuning(G.SMALL_CHUNK) == (ch, True)
                got = np.asarray(S.stft(x, w, ctx=ctx, **opts)[0])
                assert ctx.last_dispatch().split("+")[0] == "stft.pair.1r", ctx.last_dispatch()
                launch = G.forward_launch(case, knobs)
                assert_same_bits(got, base, f"forced chunk {knobs}", lambda idx: (launch, launch.owner(idx[0], idx[1])))


# ----------------------------------------------------------------------------------------------------------------------------- FIR
def fir_taps(case):
    return S.filters.firwin(case.taps, [4000.0], sampling_rate=48000)


@pytest.fixture(scope="module")
def fir_references():
    """direct double-precision convolution per (taps, mode, row length): computed once, shared, never written to"""
    made = {}

    def get(case, x):
        key = (case.taps, case.mode, case.L)
        if key not in made:
            h = fir_taps(case).astype(np.float64)
            ref = np.stack([np.convolve(r.astype(np.float64), h, mode=case.mode) for r in x])
            ref.setflags(write=False)
            made[key] = ref
        return made[key]
    return get


@pytest.mark.parametrize("key", list(G.FIR))
def test_fir_streams_give_the_same_bits_at_every_geometry(contexts, fir_references, key):
    case = G.FIR[key]
    h = fir_taps(case)
    # twins: none; the placement of every other family (a non-finite sample poisons its whole row, like the reference's one transform per
    # row, so ALL THREE rows are non-finite and only the set is compared); the NaN of row 1 alone (rows 0 and 2 stay finite: their words
    # are compared, beside a poisoned row whose flag and poison pass ran)
    for twin in ("", "every-row", "row-1"):
        x = np.random.default_rng(case.taps).standard_normal((case.rows, case.L)).astype(f32)     # (one signal per tap count: the modes share it)
        if twin:
            x[1, case.L // 2] = np.nan
        if twin == "every-row":
            x[0, case.L - 1] = np.inf
            x[2, 0] = -np.inf
        ctx0 = contexts({})
        base = np.asarray(S.filters.fir(x, h, mode=case.mode, ctx=ctx0))
        rec0 = ctx0.last_dispatch()
        assert rec0.split("+")[0] == case.family, f"dispatched to [{rec0}], the case is about [{case.family}]"
        if not twin:
            ref = fir_references(case, x)
            assert base.shape == ref.shape and np.isfinite(base).all()
            err = float(np.max(np.abs(base - ref)) / np.max(np.abs(ref)))
            print(f"\nBASELINE {key}: max error / max reference {err:.3e}")
            assert err < GLOBAL_BOUND, (key, err)
        elif twin == "every-row":
            assert not np.isfinite(base).any()
        else:
            assert not np.isfinite(base[1]).any() and np.isfinite(base[0]).all() and np.isfinite(base[2]).all()
            ref = fir_references(case, x)        # (of the finite signal: rows 0 and 2 are the same samples)
            assert float(np.max(np.abs(base[[0, 2]] - ref[[0, 2]])) / np.max(np.abs(ref))) < GLOBAL_BOUND
        for name, knobs in G.fir_geometries(case).items():
            ctx = contexts(knobs)
            got = np.asarray(S.filters.fir(x, h, mode=case.mode, ctx=ctx))
            assert ctx.last_dispatch() == rec0, f"{key} {name}: dispatched to [{ctx.last_dispatch()}], the baseline to [{rec0}]"
            launch, first = G.fir_launch(case, knobs)
            assert_same_bits(got, base, f"{key} {name}{' non-finite twin ' + twin if twin else ''}",
                             lambda idx: (launch, f"first sample of the stream launch {first} (a row's grid moves by up to 31 samples)",
                                          launch.owner(idx[0], idx[1] - first)))


# ------------------------------------------------------------------------------------------------------------------------ inverses
def inverse_input(case, M, twin, rows=G.ROWS):
    rng = np.random.default_rng(7 * case.N + case.hop + M + rows)
    N = case.N
    if case.entry == "istft_packed":      # the packed half of a Hermitian spectrum: Re X[N/2] rides in the imaginary part of bin 0
        half = np.fft.rfft(rng.standard_normal((rows, M, N)), axis=-1)
        z = half[..., : N // 2].astype(c64)
        z[..., 0] = half[..., 0].real + 1j * half[..., N // 2].real
    else:
        z = (rng.standard_normal((rows, M, N)) + 1j * rng.standard_normal((rows, M, N))).astype(c64)
    extra = None
    if case.entry == "istft_filtered":
        extra = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(c64)
    elif case.entry == "istft_masked":
        extra = rng.uniform(0.1, 1.0, (rows, M, N if case.mask == "real" else N // 2 + 1)).astype(f32)
    if twin:
        z[1, M // 2, 7] = np.nan
        z[0, M - 1, 5] = np.inf
        z[2, 0, 3] = -np.inf
    return z, extra


def run_inverse(ctx, case, z, extra):
    w = S.windows.hann(case.N)
    opts = dict(overlap_length=case.N - case.hop, fft_length=case.N)
    if case.entry == "istft":
        y = S.istft(z, w, ctx=ctx, **opts)
    elif case.entry == "istft_filtered":
        y = S.istft_filtered(z, extra, w, ctx=ctx, **opts)
    elif case.entry == "istft_masked":
        y = S.istft_masked(z, extra, w, ctx=ctx, **opts)
    else:
        y = S.istft_packed(z, w, ctx=ctx, **opts)
    return np.asarray(y), ctx.last_dispatch()


def full_gain(case, mask):
    """a one-sided mask row g[0 .. N/2] as the N gains it stands for (bin k > N/2 takes g[N - k], nxsig_internal.h spectrum_mask_apply)"""
    if case.mask == "real":
        return mask
    return np.concatenate([mask, mask[..., -2:0:-1]], axis=-1)


# consecutive frames that share one transform in the two inverse families accuracy_model.REACH does not list
EXTRA_REACH = {
    "istft.packed": 2,        # kernels_wave_packed.hip:14-15 (two frames share the 1024-point core exactly as in k_istft_wave_half)
    "istft.wave.filt": 1,     # kernels_wave.hip:1321 (k_istft_wave with the filter multiplied in: one frame per transform)
}


def check_inverse_baseline(case, M, z, extra, got):
    """the global bound against the oracle (every case), and per hop-segment at MARGIN x the single-precision model (every case too:
    the global figure is taken against the largest reference value, which under a Hann window is an edge sample over a normaliser of
    1e-9 — it reads 1e-10 whatever the kernel does inside the row)"""
    w, N, hop = S.windows.hann(case.N), case.N, case.hop
    shape = f"N={N} hop={hop} M={M}"
    opts = dict(overlap_length=N - hop, fft_length=N)
    assert np.isfinite(got).all()
    zin, real = z, False
    if case.entry == "istft_packed":
        half = np.concatenate([z, np.zeros(z.shape[:-1] + (1,), c64)], axis=-1)
        half[..., N // 2] = z[..., 0].imag
        half[..., 0] = z[..., 0].real
        zin, real = np.concatenate([half, np.conj(half[..., -2:0:-1])], axis=-1).astype(c64), True
    elif case.entry == "istft_filtered":     # the product rounded to c64 first, like Nx.multiply
        zin = (z.astype(np.complex128) * extra.astype(np.complex128)).astype(c64)
    elif case.entry == "istft_masked":       # each component times the gain in double, one rounding (spectrum_mask_apply)
        g = full_gain(case, extra).astype(np.float64)
        zin = ((z.real.astype(np.float64) * g).astype(f32) + 1j * (z.imag.astype(np.float64) * g).astype(f32)).astype(c64)
    oracle = np.stack([O.istft(r, w, **opts) for r in zin])
    oracle = oracle.real if real else oracle
    assert got.shape == oracle.shape
    err = float(np.max(np.abs(got - oracle)) / np.max(np.abs(oracle)))
    print(f"\nBASELINE {case.key} M={M}: max error / max reference {err:.3e}")
    assert err < GLOBAL_BOUND, (case.key, M, err)
    ref, model = A.istft_reference(zin, w, hop), A.istft_model(zin, w, hop)
    if real:
        ref, model = ref.real, model.real
    reach = A.reach_of(case.family, N) if case.family in A.REACH else EXTRA_REACH[case.family]
    A.inverse_check(case.family, shape, "noise:" + case.key, A.segment_errors(model, ref, hop, N, reach),
                    A.segment_errors(got, ref, hop, N, reach), N, hop, M)


INVERSE_PARAMS = [(key, which) for key in G.INVERSE for which in (0, 1)]


@pytest.mark.parametrize("key,which", INVERSE_PARAMS, ids=[f"{k}-{'M61' if w == 0 else 'short'}" for k, w in INVERSE_PARAMS])
def test_inverse_kernels_give_the_same_bits_at_every_run_length(contexts, key, which):
    case = G.INVERSE[key]
    M = G.inverse_frames(case)[which]
    base_knobs = dict(case.base)
    for twin in (False, True):
        z, extra = inverse_input(case, M, twin)
        base, rec0 = run_inverse(contexts(base_knobs), case, z, extra)
        assert rec0.split("+")[0] == case.lead, f"dispatched to [{rec0}], the case is about [{case.lead}]"
        if not twin:
            check_inverse_baseline(case, M, z, extra, base)
        else:
            bad = ~np.isfinite(base)
            assert bad.any() and (not bad.all() or M < 2 * case.R)
        for name, knobs in G.inverse_geometries(case, M).items():
            got, rec = run_inverse(contexts({**base_knobs, **knobs}), case, z, extra)
            assert stem(rec) == stem(rec0), f"{key} {name}: dispatched to [{rec}], the baseline to [{rec0}]"
            runs = G.inverse_launch(case, M, knobs)
            assert_same_bits(got, base, f"{key} M={M} {name} {knobs}{' non-finite twin' if twin else ''}",
                             lambda idx: (runs, f"segment {idx[1] // case.hop}", runs.owner(idx[1] // case.hop)))


@pytest.mark.parametrize("key", G.MANY_ROWS_KEYS)
def test_runs_per_cu_changes_the_runs_and_not_the_bits(contexts, key):
    """NXSIG_ISTFT_RUNS_PER_CU cannot change a launch of 3 rows (fewer units than compute units: the run length is NXSIG_ISTFT_MIN_RUN's,
    tests/launch_geometry.py inverse_geometries).  Here one case per form of launcher that reads it, with enough rows of 61 frames that
    the run length is the switch's — runs of 5, 3 and 1 units (6, 4, 2 for the pair kernels) at 1, 2 and 4096 waves per CU
    (tests/test_launch_geometry_host.py asserts those figures) — against the default geometry, finite and non-finite twin"""
    case = G.INVERSE[key]
    M, rows = G.INVERSE_M, G.many_rows(case)
    base_knobs = dict(case.base)
    for twin in (False, True):
        z, extra = inverse_input(case, M, twin, rows)
        base, rec0 = run_inverse(contexts(base_knobs), case, z, extra)
        assert rec0.split("+")[0] == case.lead, f"dispatched to [{rec0}], the case is about [{case.lead}]"
        if not twin:
            check_inverse_baseline(case, M, z, extra, base)
        else:
            bad = ~np.isfinite(base)
            assert bad[:3].any() and not bad[:3].all() and not bad[3:].any()
        for name, knobs in G.MANY_ROWS_GEOMETRIES.items():
            got, rec = run_inverse(contexts({**base_knobs, **knobs}), case, z, extra)
            assert stem(rec) == stem(rec0), f"{key} {name}: dispatched to [{rec}], the baseline to [{rec0}]"
            runs = G.inverse_launch(case, M, knobs, rows=rows)
            assert_same_bits(got, base, f"{key} rows={rows} {name} {knobs}{' non-finite twin' if twin else ''}",
                             lambda idx: (runs, f"segment {idx[1] // case.hop}", runs.owner(idx[1] // case.hop)))
