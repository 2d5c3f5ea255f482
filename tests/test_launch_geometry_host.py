"""What tests/test_gpu_launch_geometry.py is worth, shown without a GPU from the launcher arithmetic restated in tests/launch_geometry.py.

The GPU module compares every geometry of a call bit for bit with the default one.  That says something only if the geometries differ
where the kernels' pipelines differ, so for every case this module asserts: some geometry hands a wave two units and some three (the
prefetch, the peeled last unit, a steady-state trip between them), some chunk holds units of two rows (the row advance of the
prefetch), the last chunk is ragged, and one geometry puts the whole launch into one workgroup; for the inverses that the forced run
lengths reach 1, an odd value, one that does not divide a row, one run per row and a run longer than the row.  It also shows WHY the
GPU module exists: the default geometry of every case is one unit per wave, or runs of two frames — and that every `file:line` the
catalogue cites still holds the constant or call it is cited for."""
import os
import re

import pytest

import launch_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_lines(name, _cache={}):
    if name not in _cache:
        with open(os.path.join(ROOT, G.CSRC, name)) as f:
            _cache[name] = f.read().split("\n")
    return _cache[name]


@pytest.mark.parametrize("ref,text", G.all_citations(), ids=[c[0] for c in G.all_citations()])
def test_every_citation_points_at_its_constant_or_call(ref, text):
    name, line = ref.split(":")
    lines = source_lines(name)
    found = [i + 1 for i, s in enumerate(lines) if text in s]
    assert int(line) in found, f"{ref} no longer holds [{text}]; it is on line(s) {found}"


def test_the_factor_table_is_the_header_s():
    """RAB_FACTORS / RAB_INVERSE_ONLY against the X(K, A, B) lists of wave_rab.hpp; the lengths against the suite's own RAB_LENGTHS"""
    forward, inverse_only = {}, {}
    for s in source_lines("wave_rab.hpp"):
        m = re.match(r"#define NXSIG_RAB_(PART\d|INVERSE_ONLY)\(X\)(.*)", s)
        if m:
            for K, A, B in re.findall(r"X\((\d+), *(\d+), *(\d+)\)", m.group(2)):
                (inverse_only if m.group(1) == "INVERSE_ONLY" else forward)[int(K)] = (int(A), int(B))
    assert forward == G.RAB_FACTORS and inverse_only == G.RAB_INVERSE_ONLY
    assert all(A * B == K for K, (A, B) in {**forward, **inverse_only}.items())
    with open(os.path.join(ROOT, "tests", "test_gpu_tuned_kernels.py")) as f:
        src = f.read()
    listed = re.search(r"^RAB_LENGTHS = \[(.*?)\]", src, re.S | re.M).group(1)
    listed = [int(v) for v in re.findall(r"\b\d+\b", re.sub(r"#.*", "", listed))]
    assert listed == G.RAB_LENGTHS and set(listed) == set(G.RAB_FACTORS)


def test_the_catalogue_holds_the_cases_the_families_need():
    fams = {c.family for c in G.FORWARD.values()}
    assert {"stft.pair", "stft.quad2", "stft.quad4", "stft.quad8", "stft.real2x", "stft.real2x.4k", "stft.8k", "stft.r20", "stft.rab", "stft.blue",
            "stft_c64.rab", "fft.rows_wave"} <= fams
    assert {f"{s}.{fe}" for s in ("mag", "mel") for fe in ("pair", "quad2", "real2x", "r20", "rab")} <= fams
    assert {c.K for c in G.FORWARD.values() if c.family == "stft.rab"} == set(G.RAB_LENGTHS)
    assert {(c.K, c.K <= 512) for c in G.FORWARD.values() if c.family == "stft.blue"} == {(443, True), (1000, False)}
    assert {c.K for c in G.FORWARD.values() if c.kind == "rows"} == {1024, 2048, 4096}
    assert {(c.taps, c.mode, c.family) for c in G.FIR.values()} == {(t, m, f) for t, f in ((33, "fir.wave32"), (257, "fir.pair"), (513, "fir.r2k"))
                                                                    for m in ("same", "full")}
    inv = {(c.family, c.N, c.hop) for c in G.INVERSE.values()}
    assert {("istft.wave", 1024, h) for h in (128, 256, 512, 1024)} <= inv
    assert {("istft.half", 512, 128), ("istft.half", 512, 256), ("istft.quad", 256, 64), ("istft.quad", 128, 32), ("istft.dbl", 2048, 512),
            ("istft.4k", 4096, 1024), ("istft.packed", 1024, 256), ("istft.r20", 400, 160), ("istft.rab", 960, 240), ("istft.rab", 512, 160),
            ("istft.rab.q", 1152, 288), ("istft.rab.q", 2880, 720), ("istft.wave.filt", 1024, 256), ("istft.wave.mask", 1024, 256)} <= inv
    assert {c.lead for c in G.INVERSE.values() if c.family == "istft.wave"} == {"istft.wave", "istft.wave.deep"}
    assert {c.mask for c in G.INVERSE.values() if c.family == "istft.wave.mask"} == {"real", "onesided"}


# -------------------------------------------------------------------------------------------------------------- forward, FIR and rows
def chunked_cases():
    for key, c in G.FORWARD.items():
        yield key, c, G.forward_geometries(c), lambda knobs, c=c: G.forward_launch(c, knobs)
    for key, c in G.FIR.items():
        yield key, c, G.fir_geometries(c), lambda knobs, c=c: G.fir_launch(c, knobs)[0]


CHUNKED = list(chunked_cases())


@pytest.mark.parametrize("key,case,geometries,launch", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_shapes_are_small_odd_and_off_the_workgroup_grid(key, case, geometries, launch):
    base = launch({})
    assert base.units_per_row % base.W != 0 or case.__class__ is G.Forward and case.kind == "rows", (key, base)
    if isinstance(case, G.Forward) and case.kind == "rows":
        assert case.rows == 50 and case.rows % base.W != 0
    elif isinstance(case, G.Forward):
        assert case.rows == 3 and case.M % 2 == 1 and (case.M == 25 if case.kind == "8k" else 40 <= case.M <= 70)
        assert case.M % case.launcher.per_unit != 0 or case.launcher.per_unit == 1     # the last unit of a row is ragged
    else:
        assert case.rows == 3 and case.L % 32 != 0 and 40 <= base.units_per_row <= 60


@pytest.mark.parametrize("key,case,geometries,launch", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_the_default_geometry_is_one_unit_per_wave(key, case, geometries, launch):
    """the reason tests/test_gpu_launch_geometry.py exists: at a shape the suite can afford no wave sees a second unit"""
    base = launch({})
    assert base.max_units_per_wave() == 1, (key, base)
    assert case.launcher.dflt >= 2            # ... while production runs 2 .. 16


@pytest.mark.parametrize("key,case,geometries,launch", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_the_geometries_reach_the_pipelined_parts(key, case, geometries, launch):
    launches = {g: launch(knobs) for g, knobs in geometries.items()}
    upw = {g: la.max_units_per_wave() for g, la in launches.items()}
    assert any(v == 2 for v in upw.values()), upw                          # a first and a (peeled) last unit, nothing between
    assert any(v >= 3 for v in upw.values()), upw                          # a steady-state trip between them
    assert any(la.a_chunk_straddles_rows() and la.max_units_per_wave() >= 2 for la in launches.values())   # the prefetch crosses a row seam
    assert any(la.last_chunk_is_ragged() and la.max_units_per_wave() >= 2 for la in launches.values())
    assert any(la.one_workgroup() for la in launches.values())
    assert launches[f"upw{G.UPW_MAX}"].one_workgroup()                      # "more than the launch holds"
    assert all(1 <= v <= 4096 for knobs in geometries.values() for k, v in knobs.items() if k in (G.WAVE_UPW, G.FIR_UPW))   # tuning_in_range
    wanted = {1, 2, 3, case.launcher.dflt, case.launcher.dflt + 1, G.UPW_MAX} if isinstance(case, G.Forward) else {1, 2, 3, 8, 9, G.UPW_MAX}
    assert {knobs[case.launcher.knob] for knobs in geometries.values() if case.launcher.knob in knobs} == wanted
    # the launch names the family: every geometry of a case runs the same kernel family
    assert {la.name.replace(".1r", "") for la in launches.values()} == {case.family}


def test_forced_chunks_of_the_pair_kernel():
    """NXSIG_WAVE_SMALL_CHUNK reaches both workgroup sizes, with chunks that are no multiple of four pairs, of the 12 (or 4) waves, or of a row"""
    for key in G.PAIR_SPECTRUM:
        case = G.FORWARD[key]
        geos = G.forward_geometries(case)
        for ch in G.SMALL_CHUNKS:
            big, small = G.forward_launch(case, geos[f"chunk{ch}"]), G.forward_launch(case, geos[f"chunk{ch}-w0"])
            assert (big.W, big.chunk, small.W, small.chunk) == (12, ch, 4, ch)
        assert {ch % 4 for ch in G.SMALL_CHUNKS} == {0, 1, 2, 3} and any(ch < 12 for ch in G.SMALL_CHUNKS) and any(ch % 12 for ch in G.SMALL_CHUNKS if ch > 12)
        base = G.forward_launch(case, {})
        assert (base.W, base.chunk, base.name) == (12, 1, "stft.pair.1r")       # the default: one-round geometry, one pair per workgroup
        w0 = G.forward_launch(case, geos["small-w0"])
        assert (w0.W, w0.chunk) == (4, 4)


def test_the_switch_alone_does_not_reach_the_one_round_pair_launch():
    """why the pair cases set NXSIG_WAVE_SMALL_W=0 beside NXSIG_WAVE_UNITS_PER_WAVE"""
    case = G.FORWARD["pair-hop256"]
    assert G.forward_launch(case, {G.WAVE_UPW: 3}) == G.forward_launch(case, {})
    assert G.forward_launch(case, {G.WAVE_UPW: 3, G.SMALL_W: 0}).chunk == 12


def test_production_sizes_take_the_production_geometry():
    """the restated heuristic at a production size: 32 streams of 60 s at 48 kHz on the pair kernel run two pairs per wave"""
    M = (60 * 48000 - 1024) // 256 + 1
    total = 32 * G.cdiv(M, 2)
    assert G.fill_units_per_wave(total, 4, 2) == 2 and G.fill_units_per_wave(93, 4, 2) == 1
    assert G.istft_min_run({}, 32 * (M + 3), G.NUM_CUS * 8, 4) == 4 and G.istft_min_run({}, 3 * 64, G.NUM_CUS * 8, 4) == 2


# ---------------------------------------------------------------------------------------------------------------------------- inverses
INVERSES = [(key, c) for key, c in G.INVERSE.items()]


@pytest.mark.parametrize("key,case", INVERSES, ids=[c[0] for c in INVERSES])
def test_the_default_runs_are_two_frames(key, case):
    for M in G.inverse_frames(case):
        assert M >= 2 * case.R - 1                                           # a valid call of the tuned kernel
        base = G.inverse_launch(case, M, {})
        # (the packed inverse has no small-launch rule: it keeps its production floor of 8, kernels_wave_packed.hip:210)
        assert base.run_len == (2 if case.small_rule else case.dflt_run), (key, M, base)
        assert case.dflt_run >= 4
    assert G.inverse_frames(case)[0] == 61


@pytest.mark.parametrize("key,case", INVERSES, ids=[c[0] for c in INVERSES])
def test_the_forced_runs_reach_every_regime(key, case):
    M = G.INVERSE_M
    geos = G.inverse_geometries(case, M)
    asked = {knobs[G.MIN_RUN] for knobs in geos.values()}
    assert asked == {1, 2, 3, 5, 8, 17, M, M + case.R + 5}
    assert all(1 <= v <= (1 << 20) for v in asked)                            # tuning_in_range
    assert {knobs.get(G.RUNS_PER_CU) for knobs in geos.values()} == {None, 1}
    runs = {g: G.inverse_launch(case, M, knobs) for g, knobs in geos.items()}
    lens = {r.run_len for r in runs.values()}
    upr = next(iter(runs.values())).units_per_row
    assert len(lens) >= 4, lens                                               # after the kernel's own rounding (frame pairs: even)
    if not case.even:
        assert 1 in lens and any(v % 2 == 1 and v > 1 for v in lens)
    assert min(lens) == (2 if case.even else 1)
    assert any(upr % v != 0 and v < upr for v in lens)                        # the last run of a row is short
    assert any(r.runs_per_row == 1 for r in runs.values())                    # one run per row ...
    assert any(r.run_len > upr for r in runs.values())                        # ... and a run longer than the row
    assert any(r.runs_per_row >= 3 and r.run_len >= 3 for r in runs.values())  # several runs of several units: seams between long runs
    # the short row: the same switches, a row of 2R - 1 frames
    Ms = G.inverse_frames(case)[1]
    short = {G.inverse_launch(case, Ms, knobs).run_len for knobs in G.inverse_geometries(case, Ms).values()}
    assert len(short) >= 4


@pytest.mark.parametrize("key,case", INVERSES, ids=[c[0] for c in INVERSES])
def test_runs_per_cu_cannot_change_a_launch_of_three_rows(key, case):
    """said plainly: the `-1cu` twins of the 3-row shapes launch the SAME runs as their partners — 3 rows hold fewer units than there
    are compute units, so the run length is NXSIG_ISTFT_MIN_RUN's whatever NXSIG_ISTFT_RUNS_PER_CU says.  They are run because a call
    must not care, and they add no geometry: the switch is tested on the shapes of MANY_ROWS_KEYS (next test)"""
    for M in G.inverse_frames(case):
        geos = G.inverse_geometries(case, M)
        assert G.inverse_launch(case, M, {}).units_per_row * G.ROWS < G.NUM_CUS
        for name, knobs in geos.items():
            if name.endswith("-1cu"):
                assert G.inverse_launch(case, M, knobs) == G.inverse_launch(case, M, geos[name[:-4]]), (key, M, name)


def test_every_launcher_form_that_reads_runs_per_cu_has_a_many_rows_case():
    reads = {c.cites[0] for c in G.INVERSE.values() if c.runs_per_cu_knob}          # one launcher form per first citation
    assert reads == {G.INVERSE[k].cites[0] for k in G.MANY_ROWS_KEYS}
    assert [k for k, c in G.INVERSE.items() if not c.runs_per_cu_knob] == ["4k"]     # kernels_wave.hip:1417: a constant 4 waves per CU
    assert {G.INVERSE[k].family for k in G.MANY_ROWS_KEYS} == {c.family for c in G.INVERSE.values()} - {"istft.4k"}


@pytest.mark.parametrize("key", G.MANY_ROWS_KEYS)
def test_runs_per_cu_decides_the_runs_of_the_many_rows_shapes(key):
    case = G.INVERSE[key]
    rows = G.many_rows(case)
    runs = {g: G.inverse_launch(case, G.INVERSE_M, knobs, rows=rows) for g, knobs in G.MANY_ROWS_GEOMETRIES.items()}
    upr = runs["1cu"].units_per_row
    assert upr * rows > 4 * G.NUM_CUS and rows >= 13
    assert [runs[g].run_len for g in ("1cu", "2cu", "4096cu")] == ([6, 4, 2] if case.even else [5, 3, 1])
    assert len({r.runs_per_row for r in runs.values()}) == 3                        # three different launches
    assert upr % runs["1cu"].run_len != 0 or upr % runs["2cu"].run_len != 0         # a short last run in a row
    assert all(1 <= knobs[G.RUNS_PER_CU] <= 4096 for knobs in G.MANY_ROWS_GEOMETRIES.values())   # tuning_in_range
    if case.waves is not None:   # the default geometry of such a call is none of them for the forms whose waves per CU are known here
        assert G.inverse_launch(case, G.INVERSE_M, dict(case.base), rows=rows).run_len in (2, 8)


def test_run_owner_arithmetic():
    r = G.Runs(run_len=3, units_per_row=16, runs_per_row=6, segs_per_unit=4)
    assert r.owner(0) == dict(unit=0, run=0, first_unit_of_run=0)
    assert r.owner(47) == dict(unit=11, run=3, first_unit_of_run=9)


def test_chunk_owner_arithmetic():
    la = G.Chunked("x", W=4, chunk=12, units_per_row=31, rows=3, elems_per_unit=2)
    assert la.owner(0, 0) == dict(unit=0, chunk=0, wave=0, kth=0)
    assert la.owner(1, 5) == dict(unit=33, chunk=2, wave=1, kth=2)           # unit 33 = slot 9 of chunk 2: wave 1's third unit
    assert la.max_units_per_wave() == 3 and la.a_chunk_straddles_rows() and la.last_chunk_is_ragged() and not la.one_workgroup()
    assert G.Chunked("x", 4, 4, 15, 3, 4, u_lo=0).owner(0, 60) is None      # the ragged 16th unit of a quad row: the edge launch's


def test_a_difference_is_found_located_and_attributed():
    """the comparison of the GPU module on arrays made here: NaN payloads and non-finite elements are compared as a set, finite elements
    as words (-0.0 is not +0.0), and the message names the owner under the geometry"""
    import numpy as np

    import test_gpu_launch_geometry as T

    base = (np.arange(2 * 6 * 4, dtype=np.float32).reshape(2, 6, 4) + 1j).astype(np.complex64)
    base[1, 2, 3] = np.nan
    assert T.first_difference(base.copy(), base) is None
    other = base.copy()
    other[1, 2, 3] = complex(np.inf, np.nan)                    # another non-finite value in the same element: the same set
    assert T.first_difference(other, base) is None
    other = base.copy()
    other[1, 4, 1] = np.nextafter(other[1, 4, 1].real, np.float32(1e9)) + 1j * other[1, 4, 1].imag
    idx, what = T.first_difference(other, base)
    assert idx == (1, 4, 1) and "1 of 48 elements differ" in what
    other = base.copy()
    other[0, 5, 0] = np.inf
    assert T.first_difference(other, base)[0] == (0, 5, 0)
    zeros = np.zeros((1, 3), np.float32)
    assert T.first_difference(-zeros, zeros)[0] == (0, 0)
    launch = G.Chunked("stft.x", W=4, chunk=12, units_per_row=3, rows=2, elems_per_unit=2)
    other = base.copy()
    other[1, 4, 1] += 1
    with pytest.raises(AssertionError, match=r"first difference at \(1, 4, 1\).*'unit': 5, 'chunk': 0, 'wave': 1, 'kth': 1"):
        T.assert_same_bits(other, base, "case geometry", lambda i: launch.owner(i[0], i[1]))
    assert T.stem("stft.pair.1r+stft.pair.1r.edge") == "stft.pair" and T.stem("istft.half.deep") == "istft.half" and T.stem("stft.pair.h4") == "stft.pair"
