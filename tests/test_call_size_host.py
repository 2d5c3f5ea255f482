"""What tests/test_gpu_call_size.py is worth, shown without a GPU from the launcher arithmetic restated in tests/call_size.py.

The GPU module compares a large call, row by row, with a small call of the same rows.  That says something only if the two calls take
different branches of their launcher, so for 256, 64 and 32 compute units this module asserts of every case: the small call is on the
first branch (one tile per workgroup, runs of four units or of the whole row, one slab, one chunk, one trip, one tile per scan thread)
and the large call on the branch the case names — `tiles_per_wg` of 2, 3 and 16, a run longer than four units with a ragged last run,
three slabs, three chunks, a partial second trip, two tiles per scan thread — within the memory cap.  It also shows WHY the GPU module
exists: the shapes the families' own modules run today are on the first branch (two calls are not, and are named) — and that every
`file:line` the catalogue cites still holds the text it is cited for."""
import os

import pytest

import call_size as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lines_of(path, _cache={}):
    if path not in _cache:
        with open(os.path.join(ROOT, path)) as f:
            _cache[path] = f.read().split("\n")
    return _cache[path]


def holds(path, ref, text):
    line = int(ref.split(":")[1])
    found = [i + 1 for i, s in enumerate(lines_of(path)) if text in s]
    assert line in found, f"{ref} no longer holds [{text}]; it is on line(s) {found}"


@pytest.mark.parametrize("ref,text", Z.all_citations(), ids=[c[0] for c in Z.all_citations()])
def test_every_citation_points_at_its_constant_or_call(ref, text):
    holds(Z.CSRC + ref.split(":")[0], ref, text)


EXISTING = Z.existing_shapes() + Z.existing_shapes_past_the_cap()


@pytest.mark.parametrize("family,cite,geometry", EXISTING, ids=[f"{e[0]}@{e[1][0]}" for e in EXISTING])
def test_every_citation_into_the_families_own_modules_holds(family, cite, geometry):
    holds("tests/" + cite[0].split(":")[0], cite[0], cite[1])


def test_the_restated_constants_are_the_library_s():
    k = Z.lib_constants()
    assert k["resample_tile"] == 1024 and k["find_peaks_block"] == 64 and k["lombscargle_block"] == (64, 8, 128)
    assert k["lfilter"] == {2: (32, 32 * 64), 8: (64, 64 * 64)}
    assert Z.THREADS == 256 and Z.FP_TILE == Z.THREADS * 16
    assert (Z.WELCH_PART_BYTES, Z.WELCH_CHUNK_BYTES, Z.WELCH_GENERIC_RUN) == (64 << 20, 32 << 20, 64)


def test_the_case_keys_need_no_library_and_match_the_cases():
    for cus in Z.CU_COUNTS:
        assert [c.key for c in Z.all_cases(cus)] == Z.case_keys()
    assert len(set(Z.case_keys())) == len(Z.case_keys())


CASES = [(cus, key) for cus in Z.CU_COUNTS for key in Z.case_keys()]


def case_of(cus, key, _cache={}):
    if cus not in _cache:
        _cache[cus] = {c.key: c for c in Z.all_cases(cus)}
    return _cache[cus][key]


@pytest.mark.parametrize("cus,key", CASES, ids=[f"{c}cu-{k}" for c, k in CASES])
def test_the_small_call_is_on_the_first_branch_and_the_large_one_is_not(cus, key):
    case = case_of(cus, key)
    assert 1 <= case.distinct <= (Z.FP_DISTINCT if key.startswith("find_peaks") else Z.DISTINCT) and case.rows > case.distinct
    assert len(case.small) == len(case.large) and case.claims
    for g in case.small:
        assert g.first_branch(), (key, cus, g.describe())
    for i in case.claims:
        assert case.large[i].reached() and not case.large[i].first_branch(), (key, cus, case.large[i].describe())
    assert case.device_bytes < Z.MEMORY_CAP, (key, cus, case.device_bytes)
    assert case.distinct <= case.bad_row() < case.rows
    assert all(ref.split(":")[0].endswith((".hip", ".hpp", ".h")) and text for ref, text in case.cites) and case.cites


@pytest.mark.parametrize("cus", Z.CU_COUNTS)
def test_the_named_branches(cus):
    """said plainly, per family"""
    by = {c.key: c for c in Z.all_cases(cus)}
    for up, down in Z.RESAMPLE_RATIOS:
        for d in ("f32", "c64"):
            geos = [by[f"resample-{up}_{down}-{d}-tpw{t}"].large[0] for t in (2, 3, 16)]
            assert [g.tiles for g in geos] == [5, 5, 5] and geos[0].n_out % geos[0].tile == 37
            assert [g.tiles_per_wg for g in geos] == [2, 3, 16]
            assert [g.wg_tiles() for g in geos] == [[2, 2, 1], [3, 2], [5]]     # a ragged last workgroup, and one that holds the row
    flags = {(c.params["pad"], c.params["up1"]) for c in by.values() if c.key.startswith("resample")}
    # an even whole-number decimation is padded AND reads its taps by scalar loads (a reduced ratio with down % up == 0 has up == 1),
    # the other two ratios are neither
    assert flags == {(True, True), (False, False)}
    for key, run_len, units in (("welch-1024-run7", 7, [7, 7, 5]), ("csd-1024-run7", 7, [7, 7, 7, 7, 7, 2]), ("csd-2048-run6", 6, [6, 6, 2])):
        g = by[key].large[0]
        assert g.run_len == run_len and g.run_units() == units and g.slabs == 1, g.describe()
        assert by[key].small[0].run_len == 4
    g = by["csd-pair-slabs"].large[0]
    assert g.slabs == 3 and g.slab_rows == 6553 and g.rows - 2 * g.slab_rows == 6553 // 2 and g.run_len == g.units_per_row == 2
    g = by["csd-generic-chunks"].large[0]
    assert g.slabs == 1 and g.chunks_per_slab == 3 and g.chunk_runs == 16384 and g.runs_per_row == 1 and g.rows == 40960
    for key in ("hilbert-1000", "czt-1500-700-f32", "czt-1500-700-c64", "dct-type2-n1000-keep1000", "dct-type3-n1000-keep1000",
                "dct-type2-n64-keep13", "dct-type3-n64-keep13", "lombscargle-16-1000"):
        case = by[key]
        for i in case.claims:
            g = case.large[i]
            assert g.trips == 2 and g.total % (g.blocks * Z.THREADS) != 0 and g.blocks == cus * 32
            assert g.total % g.per_row == 0
            if g.per_row & (g.per_row - 1):      # rows that are no power of two: one row lies across the seam of the two trips
                assert (g.blocks * Z.THREADS) % g.per_row != 0
            assert g.first_row_of_the_last_trip() <= case.bad_row()
    assert by["czt-1500-700-f32"].large[2].first_branch()                     # rows * m stays under the cap: the case is about rows * L
    assert by["dct-type3-n64-keep13"].large[0].trips > 2                       # rows * n of the pre-pass: many whole trips
    for tier in ("tables", "generic"):
        g = by[f"find_peaks-{tier}"].large[0]
        assert g.ntiles > 1024 and g.scan_run == 2 and g.total > Z.stream_cap(cus) and g.capacity > Z.stream_cap(cus)
    for key in Z.case_keys():
        if key.startswith("lfilter"):
            g = by[key].large[0]
            assert g.batch == 65537 and g.generic_blocks == 1025 and g.chunks == 3 and g.tiles == 1


def test_sizes_at_256_compute_units():
    """the figures the catalogue's docstrings quote"""
    by = {c.key: c for c in Z.all_cases(256)}
    assert [by[f"resample-3_2-f32-tpw{t}"].rows for t in (2, 3, 16)] == [512, 640, 4096]
    assert 970 < by["welch-1024-run7"].rows <= 1131 and 498 < by["csd-1024-run7"].rows <= 581 and 365 < by["csd-2048-run6"].rows <= 438
    assert by["csd-pair-slabs"].rows == 16382 and by["csd-generic-chunks"].rows == 40960
    assert by["hilbert-1000"].rows == 2412 and by["czt-1500-700-f32"].rows == 589 and by["lombscargle-16-1000"].rows == 2412
    assert by["dct-type2-n64-keep13"].rows == 185518 and by["find_peaks-tables"].rows == 1100
    assert all(c.distinct == Z.DISTINCT for c in by.values() if not c.key.startswith("find_peaks"))
    assert max(c.device_bytes for c in by.values()) < 1 << 30


@pytest.mark.parametrize("family,cite,geometry", Z.existing_shapes(), ids=[f"{e[0]}@{e[1][0]}" for e in Z.existing_shapes()])
def test_the_shapes_of_today_s_modules_are_on_the_first_branch(family, cite, geometry):
    """why tests/test_gpu_call_size.py exists"""
    assert geometry.first_branch(), (family, cite[0], geometry.describe())
    if isinstance(geometry, Z.FindPeaks):
        assert geometry.total <= Z.stream_cap() and geometry.ntiles <= 1024


def test_two_calls_of_today_s_modules_pass_the_cap_on_row_boundaries_only():
    """65 rows of 65536 points (czt.generic at L = 65536, dct.fft with keep = n) take three trips — of whole rows: every trip boundary is
    a row boundary and every trip is a full one.  The cases here end on a partial trip, and rows of 1000, 700 or 13 elements put a row
    across the seam of two trips"""
    for family, cite, g in Z.existing_shapes_past_the_cap():
        assert not g.first_branch() and g.trips == 3 and not g.reached()
        assert (g.blocks * Z.THREADS) % g.per_row == 0, (family, cite)


def test_owner_arithmetic():
    g = Z.GridStride("x", rows=2412, per_row=1000)
    assert g.blocks == 8192 and g.trips == 2 and g.first_row_of_the_last_trip() == 2098
    assert g.owner(2097, 151)["trip"] == 0 and g.owner(2097, 152) == dict(launch="x", trip=1, block=0, of_trips=2)
    r = Z.ResampleLds(4133, 640, 1024, 256, 3)
    assert r.owner(7, 3072)["trip"] == 0 and r.owner(7, 3071) == dict(workgroup=14, trip=2, tile=2, tiles_of_the_row_s_workgroups=[3, 2])
    w = Z.WelchPlan(2, 16382, 1024, True, True, 256, ("slabs", 3))
    assert w.owner(6553, 0)["slab"] == 1 and w.owner(16381, 0)["slab"] == 2
    c = Z.WelchPlan(2, 40960, 64, True, False, 256, ("chunks", 3))
    assert c.owner(16383, 0)["chunk"] == 0 and c.owner(16384, 0)["chunk"] == 1 and c.owner(40959, 0)["chunk"] == 2
    lf = Z.Lfilter(8, 189, 65537, 64, 4096)
    assert lf.owner(65536, 130) == dict(scan_workgroup=65536, chunk=2, generic_workgroup=1024, lane=0, of_generic_workgroups=1025)


def test_a_difference_is_attributed_to_the_trip_and_row_that_own_it():
    """the comparison of the GPU module on arrays made here: the message names the distinct row and the owner under the large geometry"""
    import numpy as np

    import test_gpu_call_size as T

    case = case_of(256, "hilbert-1000")
    want = np.zeros((case.rows, 1000), np.float32)
    got = want.copy()
    T.same_rows(case, got, want, "equal")
    got[2097, 152] = 1.0
    with pytest.raises(AssertionError, match=r"first difference at \(2097, 152\).*row 2097 = distinct row 89.*'trip': 1, 'block': 0"):
        T.same_rows(case, got, want, "large call against the small one")
    assert T.no_finite_component(np.array([complex(np.nan, np.inf)])) and not T.no_finite_component(np.array([complex(np.nan, 1.0)]))
    assert T.no_finite_component(np.array([np.nan, np.inf], np.float32)) and not T.no_finite_component(np.array([np.nan, 0.0], np.float32))
    assert T.words_that_differ(np.array([0.0, -0.0, 1.0], np.float32), np.array([0.0, 0.0, 1.0], np.float32)) == 1


def test_the_expected_peaks_of_repeated_lines_are_the_oracle_s():
    """lines_repeated of the GPU module — the per-line results of a call concatenated in row-major order — against the oracle run on the
    repeated lines themselves, a line without a peak and a line with a NaN among them"""
    import numpy as np

    import find_peaks_oracle as O
    import test_gpu_call_size as T

    rng = np.random.Generator(np.random.PCG64(5))
    x = (np.round(rng.standard_normal((6, 300)) / 0.25) * 0.25).astype(np.float32)
    x[2] = 1.0
    x[5, 150] = np.nan
    opts = dict(distance=3, plateau_size=(None, None), height=(None, None), threshold=(None, None), prominence=(None, None), width=(None, None))
    coords, ref = O.tensor(x, -1, **opts)
    pad = 7       # the tail of a device result: -1 / NaN beyond valid_indices
    peaks = {"indices": np.concatenate([coords, -np.ones((pad, 2), coords.dtype)]).astype(np.int32), "valid_indices": np.uint32(len(coords))}
    props = {k: np.concatenate([v, v[:pad]]) for k, v in ref.items()}
    idx = np.arange(23) % 5
    idx[21] = 5
    want_coords, want = T.lines_repeated(peaks, props, idx)
    again, ref2 = O.tensor(x[idx], -1, **opts)
    assert np.array_equal(want_coords, again) and list(want) == list(ref2)
    assert all(np.array_equal(want[k], ref2[k], equal_nan=True) for k in ref2) and len(again) > 500
