"""The pair front-end's streaming loop (fft_length 1024) keeps its cold routes out of the loop: a unit (frame pair)
that holds a non-finite sample runs the paired route like every other and is REDONE frame by frame after the wave's loop; the last
unit of a wave is a peeled copy of the body; frame B reuses frame A's registers.  That kernel (HOP4) takes hop = fft_length / 4 calls
in the four-wave geometry; `NXSIG_NO_HOP4=1`, the 12-wave one-round geometry and every other hop keep the general kernel.  The reference's rule is unchanged — a non-finite sample
reaches exactly the frames that contain it (lib/nx_signal.ex:94-102), DESIGN.md 3.0 — and is checked here against
`oracle/nx_oracle.py` with the tolerances and the per-frame placement checks of tests/test_gpu_reference_numerics.py, for every
position a redone unit can take in a wave and a workgroup.

Geometry of a launch (launch_wave): unit u = row * units_per_row + unit-in-row; workgroup u // chunk; inside the chunk wave
(u % chunk) % W takes the units (u % chunk) // W = 0, 1, ... in turn.  `NXSIG_WAVE_SMALL_W=0` + `NXSIG_WAVE_UNITS_PER_WAVE=2` give the
headline geometry (W = 4, chunk = 8: two units per wave) whatever the size of the call; the default for calls this small is one
12-wave workgroup per CU, and three units per wave with NXSIG_WAVE_SMALL_W=0 alone."""
import numpy as np
import pytest

from oracle import nx_oracle as O

import nx_signal_amd as S

pytestmark = pytest.mark.gpu

K, HOP, M, ROWS = 1024, 256, 45, 3          # odd M: the last unit of a row is ragged (frame A only)
L = HOP * (M - 1) + K
UPR = (M + 1) // 2                           # 23 units per row: workgroups of 8 units straddle the row seams
W, CHUNK = 4, 8

GEOMETRIES = {
    "headline": {"NXSIG_WAVE_SMALL_W": 0, "NXSIG_WAVE_UNITS_PER_WAVE": 2},
    "three-per-wave": {"NXSIG_WAVE_SMALL_W": 0},
    "one-round": {},
}


def nerr(got, ref):
    d = np.abs(np.asarray(got).astype(np.complex128) - np.asarray(ref).astype(np.complex128))
    return float(d.max()) / max(float(np.max(np.abs(ref))), 1e-30)


def context(switches):
    ctx = S.Context(0)
    for name, v in switches.items():
        ctx.set_tuning(name, v)
    return ctx


def signal(seed):
    return np.random.default_rng(seed).standard_normal((ROWS, L)).astype(np.float32)


def poisoned_units(x, hop=HOP):
    """launch-wide unit numbers of the frame pairs that hold a non-finite sample"""
    out = set()
    m_of = (x.shape[1] - K) // hop + 1
    for r, i in np.argwhere(~np.isfinite(x)):
        for m in range(max(0, (i - K) // hop + 1), min(m_of - 1, i // hop) + 1):
            out.add(int(r) * ((m_of + 1) // 2) + m // 2)
    return out


def place(x, unit, value, where="last"):
    """a non-finite sample inside launch-wide unit `unit`: the last sample of its frame A (frames 2u .. 2u + 3 of the row hold it: units u
    and u + 1), or the first sample of the row / the last of the row where only one frame holds it"""
    r, u = divmod(unit, UPR)
    x[r, {"last": 2 * u * HOP + K - 1, "row-start": 0, "row-end": L - 1}[where]] = value


def scenario(name):
    x = signal(len(name))
    if name == "first-unit-of-a-wave":          # slots 0 .. 3 of a chunk are the waves' first units
        place(x, 8 * 1 + 1, np.nan); place(x, 8 * 4 + 0, np.inf)
        want_slots = {0, 1, 2}
    elif name == "last-unit-of-a-wave":          # slots 4 .. 7: the waves' second (last) units
        place(x, 8 * 1 + 5, np.nan); place(x, 8 * 5 + 4, -np.inf)
        want_slots = {4, 5, 6}
    elif name == "both-units-of-a-wave":         # slots s and s + 4 belong to one wave
        place(x, 8 * 2 + 1, np.nan); place(x, 8 * 2 + 5, np.inf)
        want_slots = {1, 2, 5, 6}
    elif name == "every-unit-of-a-workgroup":
        for s in range(8):
            place(x, 8 * 3 + s, np.nan if s % 2 else np.inf)
        want_slots = set(range(8))
    elif name == "ragged-last-pair":             # frame M - 1 alone: the unit's frame B does not exist
        place(x, UPR - 1, np.nan, "row-end"); place(x, 3 * UPR - 1, np.inf, "row-end")
        want_slots = None
    elif name == "row-seam":                     # last unit of row 0 and first unit of row 1: neighbours in one workgroup
        place(x, UPR - 1, np.inf, "row-end"); place(x, UPR, np.nan, "row-start")
        want_slots = None
        assert (UPR - 1) // CHUNK == UPR // CHUNK
    else:
        raise KeyError(name)
    units = poisoned_units(x)
    if want_slots is not None:
        assert {u % CHUNK for u in units} == want_slots, sorted(units)      # the placement does what its name says (headline geometry)
    return x


def check_against_oracle(z, x, w, hop=HOP, scaling=None):
    zo, _, _ = O.stft(x, w, overlap_length=K - hop, fft_length=K, scaling=scaling)
    fin, fino = np.isfinite(z).all(axis=-1), np.isfinite(zo).all(axis=-1)
    assert np.array_equal(fin, fino), np.argwhere(fin != fino)[:8]
    assert 0 < (~fin).sum() < fin.size
    assert nerr(z[fin], zo[fin]) < 1e-5
    return zo


SCENARIOS = ["first-unit-of-a-wave", "last-unit-of-a-wave", "both-units-of-a-wave", "every-unit-of-a-workgroup", "ragged-last-pair", "row-seam"]


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("name", SCENARIOS)
def test_non_finite_units_are_redone_wherever_they_sit(name, geometry):
    x = scenario(name)
    w = S.windows.hann(K)
    ctx = context(GEOMETRIES[geometry])
    for scaling in (None, "spectrum"):
        z = S.stft(ctx.to_device(x), w, ctx=ctx, overlap_length=K - HOP, fft_length=K, scaling=scaling)[0].numpy()
        check_against_oracle(z, x, w, scaling=scaling)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_non_finite_unit_with_a_silent_frame(geometry):
    """the solo route and the eps clean-up meet: frame A of a unit holds a NaN, its frame B is digital silence (every component +0 in the
    reference, and here: the redone frame is cleaned eagerly); further on a silent unit (the speculative drain's re-drain) and a silent
    frame beside an ordinary one (its bins are the round-off of the shared transform, far above the 1e-10 threshold and inside the
    tolerance: the paired route's limit — DESIGN.md 3.0, third rule: a frame is bounded at the level of the loudest frame of its
    unit — which tests/test_gpu_frame_isolation.py bounds and pins to the unit; here only the tolerance is asked of it)"""
    x = signal(77)
    w = S.windows.hann(K)
    for r, u in ((0, 9), (1, 12), (2, 6)):                        # chunk slots 1, 3 (first units) and 4 (a last unit) in the headline geometry
        x[r, (2 * u + 1) * HOP: (2 * u + 1) * HOP + K] = 0.0      # frame 2u + 1 is silent ...
        x[r, 2 * u * HOP] = np.nan                                 # ... and frame 2u (not 2u + 1) holds a NaN
    x[0, 31 * HOP: 31 * HOP + K] = 0.0                            # frame 31 of row 0 silent beside an ordinary frame 30, no NaN near
    x[0, 36 * HOP: 37 * HOP + K] = 0.0                            # frames 36, 37: a silent unit
    ctx = context(GEOMETRIES[geometry])
    z = S.stft(ctx.to_device(x), w, ctx=ctx, overlap_length=K - HOP, fft_length=K)[0].numpy()
    zo = check_against_oracle(z, x, w)
    silent = np.all(zo == 0, axis=-1)
    assert silent.sum() == 6 and silent[0, 19] and silent[1, 25] and silent[2, 13] and silent[0, 31] and silent[0, 36] and silent[0, 37]
    for r, m in np.argwhere(silent):
        print("silent frame", (r, m), "max |z|", float(np.max(np.abs(z[r, m]))))
    silent[0, 31] = False
    assert np.array_equal(z[silent].view(np.uint32), zo[silent].astype(np.complex64).view(np.uint32))   # bit pattern: +0.0


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_hop_specialisation_is_bit_identical_with_the_general_kernel(geometry):
    """hop = fft_length / 4 with NXSIG_NO_HOP4 off and on: the same bits, finite units, redone units and the ragged tail alike"""
    w = S.windows.hann(K)
    opts = dict(overlap_length=K - HOP, fft_length=K)
    for x in (signal(1), scenario("both-units-of-a-wave"), scenario("ragged-last-pair"), np.ascontiguousarray(signal(2)[:, : L - HOP])):   # the last: even M
        ctx = context(GEOMETRIES[geometry])
        for scaling in (None, "psd"):
            z_spec = S.stft(ctx.to_device(x), w, ctx=ctx, scaling=scaling, sampling_rate=48000, **opts)[0].numpy()
            rec = ctx.last_dispatch().split("+")
            assert rec[0].startswith("stft.pair") and ("stft.pair.h4" in rec) == (geometry != "one-round"), rec   # HOP4 really ran ...
            ctx.set_tuning("NXSIG_NO_HOP4", 1)
            z_gen = S.stft(ctx.to_device(x), w, ctx=ctx, scaling=scaling, sampling_rate=48000, **opts)[0].numpy()
            rec = ctx.last_dispatch().split("+")
            assert rec[0].startswith("stft.pair") and "stft.pair.h4" not in rec, rec  # ... and the switch takes the call off it
            ctx.clear_tuning("NO_HOP4")
            assert z_spec.shape == z_gen.shape
            assert np.array_equal(z_spec.view(np.uint32), z_gen.view(np.uint32))
        zo, _, _ = O.stft(x, w, **opts)
        fin = np.isfinite(zo).all(axis=-1)
        z = S.stft(ctx.to_device(x), w, ctx=ctx, **opts)[0].numpy()
        assert np.array_equal(np.isfinite(z).all(axis=-1), fin) and nerr(z[fin], zo[fin]) < 1e-5


@pytest.mark.parametrize("hop", [128, 255, 257, 512])
@pytest.mark.parametrize("geometry", ["headline", "one-round"])
def test_hops_that_do_not_take_the_specialisation(hop, geometry):
    rng = np.random.default_rng(hop)
    Lh = hop * 60 + K + (3 if hop % 2 else 0)     # 61 frames (odd): a ragged last unit; rows of odd length at the odd hops
    x = rng.standard_normal((ROWS, Lh)).astype(np.float32)
    x[0, 5 * hop + 100] = np.nan
    x[1, Lh - 1] = np.inf
    x[2, 0] = -np.inf
    x[2, 31 * hop + K - 1] = np.nan
    w = S.windows.hann(K)
    ctx = context(GEOMETRIES[geometry])
    for scaling in (None, "spectrum"):
        z = S.stft(ctx.to_device(x), w, ctx=ctx, overlap_length=K - hop, fft_length=K, scaling=scaling)[0].numpy()
        check_against_oracle(z, x, w, hop=hop, scaling=scaling)
        rec = ctx.last_dispatch().split("+")
        assert rec[0].startswith("stft.pair") and "stft.pair.h4" not in rec, rec
    ctx.set_tuning("NXSIG_NO_HOP4", 1)            # no effect on a hop the specialisation does not take
    z2 = S.stft(ctx.to_device(x), w, ctx=ctx, overlap_length=K - hop, fft_length=K, scaling="spectrum")[0].numpy()
    assert np.array_equal(z.view(np.uint32), z2.view(np.uint32))
