"""A result does not depend on the size of the call: the ten newer kernel families on the branch of their launcher that only a LARGE
call takes, against a small call of the same rows.

resample_poly, welch / csd, find_peaks, hilbert, dct, lfilter, lombscargle and czt pick their launch geometry from the total work of the
call (tests/call_size.py restates the arithmetic; tests/test_call_size_host.py shows that the shapes of the families' own modules stay
on the first branch).  Here every case of tests/call_size.py, built for the compute-unit count of the device:

1. the SMALL call — at most 251 distinct rows (17 lines for find_peaks), on the first branch — against the family's own oracle at the
   family's own bound: `check` / `TOL` of tests/test_gpu_<family>.py, imported, none new;
2. the LARGE call — the same rows repeated, `small_rows[arange(rows) % distinct]`, on the branch the case names — must report the
   same dispatch family, and
3. give every row the bits of that row in the small call (hilbert, dct, czt, lombscargle, lfilter with zf, resample, welch.generic /
   csd.generic; find_peaks: the per-line results of the small call concatenated in row-major order);
4. welch.pair / csd.pair regroup their f32 partial sums with the batch (run_len is a function of rows x units): every row within TOL
   of the oracle, rows of equal content inside the one call with equal bits, and the number of words that differ from the small call
   PRINTED (`call-size ... words`), not asserted;
5. a non-finite twin: a NaN in one row that the second trip, the last slab or chunk, or a later tile of a multi-tile workgroup owns;
   the non-finite outputs are the ones the family's rule in include/nxsig.h gives, every other row keeps its bits.

A difference is reported with its row and element and the workgroup, trip, slab or chunk that owns it.  Each test prints one
`call-size <case>: cus=... <geometry> wall=...s` line."""
import ctypes as C
import time

import numpy as np
import pytest

import call_size as Z
from test_gpu_launch_geometry import assert_same_bits

import nx_signal_amd as S

pytestmark = pytest.mark.gpu

HIP_ATTR_MULTIPROCESSOR_COUNT = 63      # hipDeviceAttributeMultiprocessorCount of hip_runtime_api.h


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """the catalogue at the compute-unit count of the device, read once"""
    hip = C.CDLL("libamdhip64.so")
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0 and v.value > 0
    by = {c.key: c for c in Z.all_cases(v.value)}
    for c in by.values():        # what tests/test_call_size_host.py asserts for 256, 64 and 32 units, for this device
        assert all(g.first_branch() for g in c.small) and all(c.large[i].reached() for i in c.claims), (v.value, c.key, c.describe())
        assert c.device_bytes < Z.MEMORY_CAP
    by["cus"] = v.value
    return by


class Report:
    """the line of a case: geometry reached and wall time"""

    def __init__(self, cases, key):
        self.case, self.cus, self.extra = cases[key], cases["cus"], ""

    def __enter__(self):
        self.t0 = time.perf_counter()
        return self.case

    def __exit__(self, kind, *exc):
        if kind is None:
            print(f"\ncall-size {self.case.key}: cus={self.cus} rows={self.case.rows} distinct={self.case.distinct} [{self.case.describe()}]"
                  f"{self.extra} wall={time.perf_counter() - self.t0:.2f}s")


def repeat_index(case):
    return np.arange(case.rows) % case.distinct


def same_rows(case, got, want, label, elem=lambda idx: idx[1] if len(idx) > 1 else 0):
    assert_same_bits(got, want, f"{case.key} {label}", lambda idx: (f"row {idx[0]} = distinct row {idx[0] % case.distinct}", case.owner(idx[0], elem(idx))))


def leading(rec):
    return rec.split("+")[0]


def no_finite_component(a):
    """no finite element; of a complex array: no finite component of any element"""
    return not (np.isfinite(a.real) | np.isfinite(a.imag)).any() if a.dtype.kind == "c" else not np.isfinite(a).any()


# ------------------------------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("key", [k for k in Z.case_keys() if k.startswith("resample")])
def test_resample_workgroups_of_several_tiles(ctx, cases, key):
    import resample_oracle as R
    import test_gpu_resample as T

    with Report(cases, key) as case:
        p = case.params
        up, down, n = p["up"], p["down"], p["n"]
        h = T.taps_of(up, down)
        x = T.signal(n + 7 * up, (case.distinct, n), np.complex64 if p["complex"] else np.float32)
        small, rec = T.dev(ctx, x, up, down)
        assert rec == case.family and small.shape == (case.distinct, p["n_out"])
        T.check(small, x, up, down, h)
        idx = repeat_index(case)
        xb = x[idx]
        big, rec = T.dev(ctx, xb, up, down)
        assert rec == case.family
        want = small[idx]
        same_rows(case, big, want, "large call against the small one")
        # a NaN among the samples of the SECOND tile of the row's first workgroup (a later trip of its loop in every geometry here)
        bad = case.bad_row()
        at = min(n - 1, (3 * p["tile"] // 2) * down // up)
        xb[bad, at] = np.nan
        got, _ = T.dev(ctx, xb, up, down)
        rule = R.resample_poly_by_taps(xb[bad:bad + 1], up, down, h)[0]
        hit = ~np.isfinite(rule)
        assert hit.any() and not hit.all() and np.array_equal(~np.isfinite(got[bad]), hit)
        assert {case.large[0].owner(bad, int(m))["trip"] for m in np.flatnonzero(hit)} - {0}, "the NaN reaches no later tile of a workgroup"
        got[bad][hit] = want[bad][hit]
        same_rows(case, got, want, "non-finite twin")
        del xb, big, got, want


# ------------------------------------------------------------------------------------------------------------------------ welch / csd
def welch_inputs(case, seed):
    import test_gpu_welch as T

    p = case.params
    x, y = T.noise(seed, (case.distinct, p["length"])), T.noise(seed + 1, (case.distinct, p["length"]))
    return T, x, y, T.hann(p["N"]), dict(overlap_length=p["N"] - p["hop"], fft_length=p["K"], sampling_rate=48000.0)


def csd_all(ctx, x, y, w, o):
    """csd with both auto-spectra: ({name: numpy}, dispatch record)"""
    from nx_signal_amd import spectral

    _, pxy, pxx, pyy = spectral.csd(ctx.to_device(x), ctx.to_device(y), w, return_auto=True, **o)
    ctx.sync()
    return {"pxy": pxy.numpy(), "pxx": pxx.numpy(), "pyy": pyy.numpy()}, ctx.last_dispatch()


def csd_reference(T, x, y, w, o):
    import welch_oracle as W

    pxx, pyy = W.welch(x, w, **o)[1], W.welch(y, w, **o)[1]
    return {"pxy": W.csd(x, y, w, **o)[1], "pxx": pxx, "pyy": pyy}, {"pxy": np.sqrt(pxx * pyy), "pxx": pxx, "pyy": pyy}


def words_that_differ(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("key", ["welch-1024-run7", "csd-1024-run7", "csd-2048-run6"])
def test_welch_and_csd_runs_longer_than_four_units(ctx, cases, key):
    """the fused tier regroups a row's f32 sums with the batch: in tolerance, equal rows equal, the differing words counted"""
    report = Report(cases, key)
    with report as case:
        T, x, y, w, o = welch_inputs(case, 7000 + case.params["M"])
        import welch_oracle as W

        idx = repeat_index(case)
        if case.params["csd"]:
            small, rec = T.dev_csd(ctx, x, y, w, **o)
            assert leading(rec) == case.family
            T.check_csd(f"{key} small", small, x, y, w, **o)
            ref, scale = W.csd(x, y, w, **o)[1], np.sqrt(W.welch(x, w, **o)[1] * W.welch(y, w, **o)[1])
            run = lambda rows: T.dev_csd(ctx, rows, y[idx], w, **o)     # noqa: E731
        else:
            small, rec = T.dev_welch(ctx, x, w, **o)
            assert leading(rec) == case.family
            T.check_welch(f"{key} small", small, x, w, **o)
            ref = W.welch(x, w, **o)[1]
            scale = ref
            run = lambda rows: T.dev_welch(ctx, rows, w, **o)          # noqa: E731
        xb = x[idx]
        big, rec = run(xb)
        assert leading(rec) == case.family and big.shape == (case.rows,) + small.shape[1:]
        assert np.isfinite(big.view(np.float32)).all()
        err = T.row_err(big, ref[idx], scale[idx])
        print(f"\nwelch-accuracy {key} large call: {err:.3e}")
        assert err <= T.TOL, (key, err)
        same_rows(case, big, big[:case.distinct][idx], "rows of equal content inside the large call")
        differ = words_that_differ(big, small[idx])
        report.extra = f" words that differ from the small call: {differ} of {big.view(np.uint32).size}"
        # a NaN in the last frame of a row — the ragged last run's — takes every bin of that row and no other row's bits
        bad = case.bad_row()
        xb[bad, case.params["length"] - 10] = np.nan
        got, _ = run(xb)
        assert np.isnan(got[bad].view(np.float32)).all()
        got[bad] = big[bad]
        same_rows(case, got, big, "non-finite twin")
        del xb, big, got


@pytest.mark.parametrize("key", ["csd-pair-slabs", "csd-generic-chunks"])
def test_csd_over_several_slabs_and_chunks(ctx, cases, key):
    report = Report(cases, key)
    with report as case:
        T, x, y, w, o = welch_inputs(case, 7100 + case.params["N"])
        small, rec = csd_all(ctx, x, y, w, o)
        assert leading(rec) == case.family
        ref, scale = csd_reference(T, x, y, w, o)
        for name in ("pxy", "pxx", "pyy"):
            assert np.isfinite(small[name].view(np.float32)).all()
            err = T.row_err(small[name], ref[name], scale[name])
            print(f"\nwelch-accuracy {key} small {name}: {err:.3e}")
            assert err <= T.TOL, (key, name, err)
        idx = repeat_index(case)
        xb, yb = x[idx], y[idx]
        big, rec = csd_all(ctx, xb, yb, w, o)
        assert leading(rec) == case.family
        differ = 0
        for name in ("pxy", "pxx", "pyy"):
            if case.params["fused"]:
                assert T.row_err(big[name], ref[name][idx], scale[name][idx]) <= T.TOL, (key, name)
                same_rows(case, big[name], big[name][:case.distinct][idx], f"{name}: rows of equal content inside the large call")
                differ += words_that_differ(big[name], small[name][idx])
            else:
                same_rows(case, big[name], small[name][idx], f"{name}: large call against the small one")
        if case.params["fused"]:
            report.extra = f" words that differ from the small call: {differ}"
        # the pair rule in the last slab / chunk: a NaN in y takes Pxy, Pyy AND Pxx of its row, and nothing else
        bad = case.bad_row()
        assert case.large[0].owner(bad, 0)["slab" if case.params["fused"] else "chunk"] == 2
        yb[bad, case.params["length"] // 2] = np.nan
        got, _ = csd_all(ctx, xb, yb, w, o)
        for name in ("pxy", "pxx", "pyy"):
            assert np.isnan(got[name][bad].view(np.float32)).all(), (key, name)
            got[name][bad] = big[name][bad]
            same_rows(case, got[name], big[name], f"{name}: non-finite twin")
        del xb, yb, big, got


# ------------------------------------------------------------------------------------------------------------- grid-stride passes
def test_hilbert_generic_on_a_second_trip(ctx, cases):
    import hilbert_oracle as O
    import test_gpu_hilbert as T
    from nx_signal_amd import filters

    with Report(cases, "hilbert-1000") as case:
        N = case.params["N"]
        x = T.noise(4001, (case.distinct, N))
        idx = repeat_index(case)
        xb = x[idx]
        bad = case.bad_row()
        xt = xb.copy()
        xt[bad, N // 3] = np.nan
        xd, xtd = ctx.to_device(xb), ctx.to_device(xt)
        for o in O.OUTPUTS:
            small, rec = T.dev(ctx, x, None, o)
            assert leading(rec) == case.family
            T.check(f"{case.key} small", small, x, None, o)
            big = filters.hilbert(xd, ctx=ctx, output=o).numpy()
            assert leading(ctx.last_dispatch()) == case.family
            want = small[idx]
            same_rows(case, big, want, f"{o}: large call against the small one")
            got = filters.hilbert(xtd, ctx=ctx, output=o).numpy()
            assert no_finite_component(got[bad]), o
            got[bad] = want[bad]
            same_rows(case, got, want, f"{o}: non-finite twin")
        del xd, xtd


@pytest.mark.parametrize("key", ["czt-1500-700-f32", "czt-1500-700-c64"])
def test_czt_generic_on_a_second_trip(ctx, cases, key):
    import test_gpu_czt as T

    with Report(cases, key) as case:
        p = case.params
        kind = "czt_wa" if p["complex"] else "zoom"
        x = T.noise(4100 + p["n"], (case.distinct, p["n"]), p["complex"])
        small, rec = T.dev(ctx, x, p["m"], kind)
        assert leading(rec) == case.family
        T.check(f"{key} small", small, T.reference(x, p["m"], kind))
        idx = repeat_index(case)
        xb = x[idx]
        big, rec = T.dev(ctx, xb, p["m"], kind)
        assert leading(rec) == case.family
        want = small[idx]
        same_rows(case, big, want, "large call against the small one")
        bad = case.bad_row()
        xb[bad, p["n"] // 3] = np.nan
        got, _ = T.dev(ctx, xb, p["m"], kind)
        assert no_finite_component(got[bad])
        got[bad] = want[bad]
        same_rows(case, got, want, "non-finite twin")
        del xb, big, got, want


@pytest.mark.parametrize("key", [k for k in Z.case_keys() if k.startswith("dct")])
def test_dct_fft_on_a_second_trip(ctx, cases, key):
    import test_gpu_dct as T

    with Report(cases, key) as case:
        p = case.params
        n, keep, t, forced = p["n"], p["keep"], p["type"], p["forced"]
        norm = "ortho" if t == 2 else None
        x = T.noise(4200 + n + t, (case.distinct, n))
        small, fam = T.dev(ctx, x, t, None, norm, keep, forced)
        assert fam.startswith("fft") and small.shape == (case.distinct, keep)
        T.check(f"{key} small", small, T.reference(x, t, None, norm))
        idx = repeat_index(case)
        xb = x[idx]
        big, fam = T.dev(ctx, xb, t, None, norm, keep, forced)
        assert fam.startswith("fft")
        want = small[idx]
        same_rows(case, big, want, "large call against the small one")
        bad = case.bad_row()
        xb[bad, n // 3] = np.nan
        got, _ = T.dev(ctx, xb, t, None, norm, keep, forced)
        assert not np.isfinite(got[bad]).any()
        got[bad] = want[bad]
        same_rows(case, got, want, "non-finite twin")
        del xb, big, got, want


def test_lombscargle_generic_on_a_second_trip(ctx, cases):
    import lombscargle_oracle as O
    import test_gpu_lombscargle as T

    with Report(cases, "lombscargle-16-1000") as case:
        p = case.params
        x, y64, freqs, weights = T.inputs(4300, case.distinct, p["n"], p["F"])
        y = y64.astype(np.float32)
        kw = dict(precenter=True, normalize="power", weights=weights)
        small = T.run(ctx, x, y, freqs, True, **kw)            # (asserts lombscargle.generic)
        want = O.lombscargle(x, y.astype(np.float64), freqs, True, "power", weights, False)
        err = float(O.row_error(small.astype(np.float64), want).max())
        print(f"\nlombscargle-accuracy {case.key} small: {err:.3e}")
        assert err <= T.TOL[np.dtype(np.float32)], err
        idx = repeat_index(case)
        yb = y[idx]
        big = T.run(ctx, x, yb, freqs, True, **kw)
        same_rows(case, big, small[idx], "large call against the small one")
        bad = case.bad_row()
        yb[bad, 5] = np.nan
        got = T.run(ctx, x, yb, freqs, True, **kw)
        assert np.isnan(got[bad]).all()
        got[bad] = big[bad]
        same_rows(case, got, big, "non-finite twin")


# ------------------------------------------------------------------------------------------------------------------------ find_peaks
def lines_repeated(peaks, props, idx):
    """the results of a call on lines[idx], formed from the results of the call on the lines: the per-line results concatenated in
    row-major order.  -> (coords [valid][2], {name: values [valid]})"""
    valid = int(peaks["valid_indices"])
    coords = peaks["indices"][:valid]
    assert (np.diff(coords[:, 0]) >= 0).all()
    lines = int(idx.max()) + 1
    start, stop = np.searchsorted(coords[:, 0], np.arange(lines)), np.searchsorted(coords[:, 0], np.arange(lines), side="right")
    counts = (stop - start)[idx]
    first = np.repeat(start[idx] - np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
    sel = first + np.arange(int(counts.sum()))
    rows = np.repeat(np.arange(len(idx)), counts)
    return np.stack([rows, coords[sel, 1]], axis=1).astype(np.int32), {k: v[:valid][sel] for k, v in props.items()}


@pytest.mark.parametrize("key", ["find_peaks-tables", "find_peaks-generic"])
def test_find_peaks_past_the_grid_and_the_scan(ctx, cases, key):
    import find_peaks_oracle as O
    import test_gpu_find_peaks as T

    with Report(cases, key) as case:
        n, generic = case.params["n"], case.params["generic"]
        opts = dict(distance=3, **T.ALL)
        x = T.noise(4400, (case.distinct + 1, n))
        x[case.distinct, 2000], x[case.distinct, 100] = np.nan, np.inf      # the line of the twin
        coords, ref = O.tensor(x, -1, **opts)
        with T.Tier(ctx, generic):
            peaks, props, rec = T.call(ctx, x, True, **opts)
            assert rec == case.family
            T.compare(f"{key} small", peaks, props, coords, ref, x.shape[0] * ((n - 1) // 2))
            for twin in (False, True):
                idx = repeat_index(case)
                if twin:
                    idx[case.bad_row()] = case.distinct
                want_coords, want = lines_repeated(peaks, props, idx)
                xd = ctx.to_device(x[idx])
                big_peaks, big_props, rec = call_on_device(ctx, xd, opts)
                assert rec == case.family
                capacity = case.large[0].capacity
                assert len(want_coords) < capacity
                T.compare(f"{key} large{' non-finite twin' if twin else ''}", big_peaks, big_props, want_coords, want, capacity)
                del xd, big_peaks, big_props


def call_on_device(ctx, xd, opts):
    """find_peaks on a tensor that is on the device already"""
    from nx_signal_amd import peak_finding as PF

    peaks, props = PF.find_peaks(xd, ctx=ctx, **opts)
    ctx.sync()
    rec = ctx.last_dispatch()
    return {k: v.numpy() for k, v in peaks.items()}, {k: v.numpy() for k, v in props.items()}, rec


# --------------------------------------------------------------------------------------------------------------------------- lfilter
@pytest.mark.parametrize("key", [k for k in Z.case_keys() if k.startswith("lfilter")])
def test_lfilter_65537_rows(ctx, cases, key):
    """zi per row, zf returned, both directions; the mirror of test_batches_of_1_3_and_65537_rows in tests/test_gpu_iir.py"""
    import lfilter_oracle as O
    import test_gpu_lfilter as T
    from nx_signal_amd import _lib

    with Report(cases, key) as case:
        p = case.params
        ba, order, n, direction = T.BA[p["name"]], p["order"], p["n"], p["direction"]
        assert T.order(p["name"]) == order and T.ON_SCAN[p["name"]]
        x = T.noise(4500 + order, (case.distinct, n))
        zi = 0.3 * np.random.Generator(np.random.PCG64(4501)).standard_normal((case.distinct, order))
        oracle = O.lfilter_backward if direction else O.lfilter
        with T.Tier(ctx, p["generic"]):
            small, zf = T.c_lfilter(ctx, x, ba, zi=zi, want_zf=True, direction=direction, mem=_lib.DEVICE)
            assert ctx.last_dispatch() == case.family
            ref, zf_ref = oracle(*ba, x.astype(np.float64), zi)
            T.check(f"{key} small", small, ref)
            assert T.zf_gap(zf, zf_ref) <= T.ZF_TOL
            idx = repeat_index(case)
            xb, zb = x[idx], zi[idx]
            big, big_zf = T.c_lfilter(ctx, xb, ba, zi=zb, want_zf=True, direction=direction, mem=_lib.DEVICE)
            assert ctx.last_dispatch() == case.family
            want, want_zf = small[idx], zf[idx]
            same_rows(case, big, want, "large call against the small one")
            same_rows(case, big_zf, want_zf, "zf of the large call against the small one", elem=lambda i: 0)
            # a NaN in the middle chunk of a row of the last workgroups: what is filtered before it keeps the bits of the row with the
            # NaN and everything behind it zeroed (one row, alone: a row's bits do not depend on the batch), the rest is not finite
            bad, at = case.bad_row(), case.large[0].chunk + 5
            zeroed = xb[bad:bad + 1].copy()
            if direction:
                zeroed[0, :at + 1] = 0.0
            else:
                zeroed[0, at:] = 0.0
            alone, _ = T.c_lfilter(ctx, zeroed, ba, zi=zb[bad:bad + 1], direction=direction, mem=_lib.DEVICE)
            xb[bad, at] = np.nan
            got, got_zf = T.c_lfilter(ctx, xb, ba, zi=zb, want_zf=True, direction=direction, mem=_lib.DEVICE)
            before, behind = (slice(at + 1, n), slice(0, at + 1)) if direction else (slice(0, at), slice(at, n))
            assert not np.isfinite(got[bad, behind]).any()
            assert T.same_bits(got[bad, before], alone[0, before])
            got[bad], got_zf[bad] = want[bad], want_zf[bad]
            same_rows(case, got, want, "non-finite twin")
            same_rows(case, got_zf, want_zf, "zf of the non-finite twin", elem=lambda i: 0)
        del xb, big, got, want
