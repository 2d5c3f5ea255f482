"""Launch geometries of the streaming kernels, restated in Python (no GPU needed).

Every tuned kernel is a loop over units (frame pairs, quads, block pairs, rows; runs of hop-segments for the inverses) and its launcher
hands each wave a share of that loop.  The software-pipelined part of a kernel — the next unit's loads under this unit's butterflies,
the peeled last unit, the carry strip and the pending sums of a run — only runs when a wave gets TWO OR MORE units, and at the shapes a
correctness suite can afford the launchers' small-launch rules (`fill_units_per_wave`, `istft_min_run`) give every wave one unit, every
run two frames.  The design promises that a result does not depend on that geometry: forward units are independent,
FIR blocks sit on a grid fixed by the output offset, the inverses add in ascending frame order.  So the same call under every geometry
the switches can force must give the same BITS as the default one, and one accuracy check of the default covers them all.

This module holds what tests/test_launch_geometry_host.py (CPU) and tests/test_gpu_launch_geometry.py share:

* the CASES: entry point, a small shape, the dispatch family the call must report, and for its launcher the waves per workgroup `W`, the
  production units per wave (or shortest run) and the frames per unit, each with a `file:line` citation and the text that line holds;
* the GEOMETRIES of a case: the switch settings to run it under;
* the LAUNCHER ARITHMETIC: chunk -> workgroup -> wave -> units for the forward / FIR / row kernels (`forward_launch`, `fir_launch`),
  run length -> runs per row for the inverses (`inverse_launch`), so that each (case, geometry) can be classified without a GPU and a
  differing output element can be reported with the unit, wave and chunk — or the run — that owns it.

Geometry of a chunked launch: launch-wide unit u = row * units_per_row + unit-in-row; workgroup u // chunk; inside the chunk wave
(u % chunk) % W takes the units (u % chunk) // W = 0, 1, ... in turn (`for (u = begin + wave; u < end; u += W)` in every kernel).
Geometry of a run launch: unit-in-row j belongs to run j // run_len of its row; every run recomputes its halo."""
from dataclasses import dataclass

CSRC = "nx_signal_amd/csrc/"
NUM_CUS = 256      # compute units of an MI355X.  The GPU module uses this figure too: it only names the owner of a differing element
                   # in a failure message, the comparison itself does not depend on it
ROWS = 3
UPW_MAX = 64       # "more than the launch holds" for every case here (the host test checks it), and the most the pair kernel's
                   # non-finite mask tells apart (wave_stft.hpp: bit 63 saturates; above it DESIGN promises round-off only)

WAVE_UPW = "NXSIG_WAVE_UNITS_PER_WAVE"
FIR_UPW = "NXSIG_FIR_UNITS_PER_WAVE"
MIN_RUN = "NXSIG_ISTFT_MIN_RUN"
RUNS_PER_CU = "NXSIG_ISTFT_RUNS_PER_CU"
SMALL_W = "NXSIG_WAVE_SMALL_W"
SMALL_CHUNK = "NXSIG_WAVE_SMALL_CHUNK"

# the heuristics every launcher shares: (file:line, text the line must hold)
CITE_FILL = ("nxsig_internal.h:222", "static inline int fill_units_per_wave(")
CITE_TUNED = ("nxsig_internal.h:230", "static inline int tuned_units_per_wave(")
CITE_MIN_RUN = ("nxsig_internal.h:238", "static inline int istft_min_run(")
CITE_BALANCED = ("wave_stft.hpp:88", "inline int64_t istft_balanced_run_len(")


def cdiv(a, b):
    return -(-a // b)


def fill_units_per_wave(total_units, W, dflt, num_cus=NUM_CUS):
    """nxsig_internal.h, fill_units_per_wave: one unit per wave until the launch holds more than num_cus * 3 * W units"""
    fill = cdiv(total_units, num_cus * 3 * W)
    return max(1, fill) if fill < dflt else dflt


def tuned_units_per_wave(knobs, key, total_units, W, dflt, num_cus=NUM_CUS):
    """nxsig_internal.h, tuned_units_per_wave: the switch when it is set, else the heuristic"""
    return int(knobs[key]) if key in knobs else fill_units_per_wave(total_units, W, dflt, num_cus)


def istft_min_run(knobs, total_units, slots, dflt):
    """nxsig_internal.h, istft_min_run"""
    if MIN_RUN in knobs:
        return int(knobs[MIN_RUN])
    return 2 if total_units <= 2 * slots else dflt


def istft_balanced_run_len(units_per_row, rows, slots, halo, min_run):
    """wave_stft.hpp, istft_balanced_run_len"""
    def cost(length):
        return cdiv(cdiv(units_per_row, length) * rows, slots) * (min(length, units_per_row) + halo)
    best = max(cdiv(units_per_row * rows, slots), min_run)
    best_cost = cost(best)
    for r in range(1, 9):
        length = max(cdiv(units_per_row, r), min_run)
        c = cost(length)
        if c < best_cost or (c == best_cost and length > best):
            best, best_cost = length, c
    return best


# ------------------------------------------------------------------------------------------------------------------- chunked launches
@dataclass(frozen=True)
class Chunked:
    """one chunked launch: `rows` x `units_per_row` units dealt out `chunk` at a time to workgroups of `W` waves.  The launch covers the
    units u_lo .. u_lo + units_per_row - 1 of every row (the interior ones; the bounds-checked edge launch keeps one unit per wave)"""
    name: str
    W: int
    chunk: int
    units_per_row: int
    rows: int
    elems_per_unit: int      # frames (forward), output samples (FIR), rows (row kernels) one unit produces
    u_lo: int = 0

    @property
    def total(self):
        return self.units_per_row * self.rows

    @property
    def workgroups(self):
        return cdiv(self.total, self.chunk)

    def max_units_per_wave(self):
        return cdiv(min(self.chunk, self.total), self.W)

    def a_chunk_straddles_rows(self):
        return any((b * self.chunk) // self.units_per_row != (min((b + 1) * self.chunk, self.total) - 1) // self.units_per_row
                   for b in range(self.workgroups))

    def last_chunk_is_ragged(self):
        return self.total % self.chunk != 0

    def one_workgroup(self):
        return self.chunk >= self.total

    def owner(self, row, elem):
        """(unit, wave, k-th unit of that wave, workgroup) of element `elem` (frame / sample / 0) of `row`, None when the edge launch owns it"""
        u_in = elem // self.elems_per_unit - self.u_lo
        if not 0 <= u_in < self.units_per_row:
            return None
        u = row * self.units_per_row + u_in
        return dict(unit=u, chunk=u // self.chunk, wave=(u % self.chunk) % self.W, kth=(u % self.chunk) // self.W)


# A x B factors of the composite lengths (wave_rab.hpp:23-34, NXSIG_RAB_PART0 .. 7 and NXSIG_RAB_INVERSE_ONLY)
RAB_FACTORS = {
    320: (16, 20), 480: (24, 20), 640: (32, 20), 960: (32, 30),
    32: (8, 4), 64: (8, 8), 100: (10, 10), 120: (12, 10), 160: (16, 10), 200: (20, 10), 240: (16, 15), 300: (20, 15), 360: (24, 15), 384: (24, 16),
    500: (25, 20), 600: (30, 20), 720: (30, 24), 768: (32, 24), 800: (32, 25), 900: (30, 30),
    1000: (40, 25), 1200: (40, 30), 1280: (40, 32), 1600: (40, 40),
    192: (16, 12), 288: (24, 12), 576: (24, 24), 1152: (48, 24), 1440: (48, 30), 1536: (48, 32), 1920: (48, 40),
    441: (21, 21), 882: (42, 21), 1764: (42, 42), 2205: (35, 63),
    2400: (50, 48), 2880: (60, 48), 3840: (64, 60),
}
RAB_INVERSE_ONLY = {128: (16, 8), 256: (16, 16), 512: (32, 16), 1024: (32, 32)}
# the list tests/test_gpu_tuned_kernels.py runs (its RAB_LENGTHS): every fft length with a native forward A x B kernel
RAB_LENGTHS = [441, 882, 1764, 2205, 2400, 2880, 3840, 192, 288, 576, 1152, 1440, 1536, 1920, 32, 64, 100, 120, 160, 200, 240, 300, 360, 384,
               320, 480, 640, 960, 500, 600, 720, 768, 800, 900, 1000, 1200, 1280, 1600]


def rab_bp(B):
    return B + (2 if B & 1 else 1)


def rab_tab_bytes(K):
    return 4 * ((K + 3) & ~3) + 8 * ((K + 1) & ~1)


def rab_buf(A, B):
    """(T, BUF): frame pairs per wave iteration and complex cells of a wave's exchange buffer (wave_rab.hpp:446-448)"""
    KB, LT = A * B, max(A, B)
    T = 64 // LT
    TRS = A * rab_bp(B)
    return T, ((T * max(TRS, KB) + 15) & ~15) + 16


def rab_wg(A, B):
    """wave_rab.hpp:56-64: the window stays in global memory when that buys another wave"""
    KB = A * B
    _, BUF = rab_buf(A, B)
    w12 = min(8, (160 * 1024 - KB * 12) // (BUF * 8))
    w8 = min(8, (160 * 1024 - KB * 8) // (BUF * 8))
    return (A > 48 or B > 48) and w8 > w12 and w8 <= 4


def rab_forward_waves(A, B):
    """waves per workgroup of launch_rab (wave_rab.hpp:451-453)"""
    KB = A * B
    _, BUF = rab_buf(A, B)
    tabs = KB * 8 if rab_wg(A, B) else rab_tab_bytes(KB)
    w_fit = (160 * 1024 - tabs) // (BUF * 8)
    return min(w_fit, 8) if KB * 12 + 4 * BUF * 8 > 80 * 1024 else 4


def rab_c64_waves(A, B):
    """waves per workgroup of launch_rab_c64 (wave_rab.hpp:717)"""
    _, BUF = rab_buf(A, B)
    return min(4, (160 * 1024 - rab_tab_bytes(A * B)) // (BUF * 8))


@dataclass(frozen=True)
class Launcher:
    """what the launcher of a forward / FIR / row family does with its units: waves per workgroup, production units per wave, frames
    (rows, output samples) per unit — each with its citation — and the switch that sets the units per wave"""
    W: int
    dflt: int
    per_unit: int
    cites: tuple
    knob: str = WAVE_UPW


def _wave_launcher(mode, J, sink, C=1024):
    """launch_wave (wave_stft.hpp): pair / quad / real-2x front-ends, W = 4 (the call sites of kernels_wave.hip, _mel.hip, _mag.hip)"""
    per_unit = {"pair": 2, "quad": 2 * J, "real2x": 1}[mode]
    if sink == "spectrum":
        dflt = {"pair": 2, "quad": 8 if J == 8 else 4, "real2x": 8}[mode]
        cite = ("wave_stft.hpp:1514", "MODE == kModePair ? 2 : (MODE == kModeQuad ? (J == 8 ? 8 : 4) : 8)")
    else:
        dflt = 16 if mode == "pair" else 8
        cite = ("wave_stft.hpp:1512" if sink == "magnitude" else "wave_stft.hpp:1513", "tune(c, kT_WAVE_UNITS_PER_WAVE, MODE == kModePair ? 16 : 8)")
    site = {"spectrum": {"pair": ("kernels_wave.hip:1160", "launch_wave<1024, kModePair, 4>(c, s)"),
                         "quad": (f"kernels_wave.hip:{1162 + {2: 0, 4: 1, 8: 2}[J]}", f"launch_wave<1024, kModeQuad, 4, {J}>(c, s)"),
                         "real2x": (f"kernels_wave.hip:{1165 + (C == 2048)}", f"launch_wave<{C}, kModeReal2x, 4>(c, s)")},
            "magnitude": {"pair": ("kernels_wave_mag.hip:18", "launch_wave<1024, kModePair, 4, 2, kSinkMag>"),
                          "quad": ("kernels_wave_mag.hip:19", "launch_wave<1024, kModeQuad, 4, 2, kSinkMag>"),
                          "real2x": ("kernels_wave_mag.hip:22", "launch_wave<1024, kModeReal2x, 4, 2, kSinkMag>")},
            "mel": {"pair": ("kernels_wave_mel.hip:17", "launch_wave<1024, kModePair, 4, 2, kSinkMel>"),
                    "quad": ("kernels_wave_mel.hip:18", "launch_wave<1024, kModeQuad, 4, 2, kSinkMel>"),
                    "real2x": ("kernels_wave_mel.hip:21", "launch_wave<1024, kModeReal2x, 4, 2, kSinkMel>")}}[sink][mode]
    return Launcher(4, dflt, per_unit, (site, cite, ("wave_stft.hpp:1530", "constexpr int F = MODE == kModePair ? 2 : (MODE == kModeQuad ? 2 * J : 1)"),
                                        ("wave_stft.hpp:1517", "c->tuning.set[kT_WAVE_UNITS_PER_WAVE] ? units_per_wave : fill_units_per_wave(")))


def _r20_launcher(sink):
    return Launcher(4, 8 if sink == "mel" else 2, 6,
                    (("kernels_wave_r20.hip:303", "constexpr int W = 4, KB = 400"),
                     ("kernels_wave_r20.hip:354", "b.units_per_row = (a.pairs_per_row + 2) / 3"),
                     ("kernels_wave_r20.hip:368", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, b.total_units, W, sink == kSinkMel ? 8 : 2)")))


def _rab_launcher(K, sink):
    A, B = RAB_FACTORS[K]
    T, _ = rab_buf(A, B)
    return Launcher(rab_forward_waves(A, B), 8 if sink == "mel" else 4, 2 * T,
                    (("wave_rab.hpp:453", "constexpr int W = (KB * 12 + 4 * BUF * 8 > 80 * 1024) ? (W_FIT < 8 ? W_FIT : 8) : 4"),
                     ("wave_rab.hpp:509", "b.units_per_row = (a.pairs_per_row + T - 1) / T"),
                     ("wave_rab.hpp:529", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, b.total_units, w, sink == kSinkMel ? 8 : 4)")))


def _rab_c64_launcher(K):
    A, B = {**RAB_FACTORS, **RAB_INVERSE_ONLY}[K]
    T, _ = rab_buf(A, B)
    return Launcher(rab_c64_waves(A, B), 4, T,
                    (("wave_rab.hpp:717", "W = W_FIT < 4 ? W_FIT : 4"),
                     ("wave_rab.hpp:726", "a.units_per_row = (s.fr.M + T - 1) / T"),
                     ("wave_rab.hpp:744", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, a.total_units, W, 4)")))


LAUNCHER_BLUE = Launcher(4, 4, 2, (("wave_stft.hpp:1750", "constexpr int W = 4, R3 = C / 256"),
                                   ("wave_stft.hpp:1810", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, a.total_pairs, W, 4)")))
LAUNCHER_8K = Launcher(8, 2, 1, (("kernels_wave_8k.hip:140", "constexpr int W = 8, K = 1024"),
                                 ("kernels_wave_8k.hip:205", "const int fpw = 2;"),
                                 ("kernels_wave_8k.hip:196", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, a.total_frames, W, fpw < 1 ? 1 : fpw)")))


def _rows_launcher(K):
    return Launcher(4, 2 if K == 4096 else 4, 1,
                    (("kernels_wave_rows.hip:267", "constexpr int W = 4;"),
                     ("kernels_wave_rows.hip:268", "tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, rows, W, K == 4096 ? 2 : 4)")))


@dataclass(frozen=True)
class Forward:
    """a forward case.  entry: "stft" (f32 samples), "stft_c64", "magnitude" (spectrogram kind), "mel" (mel_spectrogram), "fft_nd"
    (rows x K, c64).  base: switches of every context of the case, the baseline included (what sends the call to the family)"""
    key: str
    entry: str
    K: int
    hop: int
    M: int
    family: str
    kind: str                 # "pair", "quad", "real2x", "8k", "r20", "rab", "blue", "rab_c64", "rows"
    launcher: Launcher
    rows: int = ROWS
    base: tuple = ()
    J: int = 0

    @property
    def L(self):
        return (self.M - 1) * self.hop + self.K


def frames_for(units_of, W):
    """an odd frame count in 40 .. 70 whose units per row are no multiple of W: chunks then straddle row seams and the last one is ragged"""
    for M in (61, 63, 59, 65, 57, 67, 55, 69, 53, 51, 49, 47, 45, 43, 41):
        if units_of(M) % W != 0:
            return M
    raise ValueError("no frame count fits")


def _forward_cases():
    out = {}

    def add(key, entry, K, hop, family, kind, launcher, rows=ROWS, base=(), J=0, M=None):
        per = launcher.per_unit
        if M is None:
            # (quad: the staged interior launch takes complete units only, interior_units below)
            M = frames_for((lambda m: (m - 1) // per) if kind == "quad" else (lambda m: cdiv(m, per)), launcher.W)
        out[key] = Forward(key, entry, K, hop, M, family, kind, launcher, rows, tuple(base), J)

    # ---- spectrum sink
    add("pair-hop256", "stft", 1024, 256, "stft.pair", "pair", _wave_launcher("pair", 2, "spectrum"))
    add("pair-hop320", "stft", 1024, 320, "stft.pair", "pair", _wave_launcher("pair", 2, "spectrum"))
    add("quad2", "stft", 512, 128, "stft.quad2", "quad", _wave_launcher("quad", 2, "spectrum"), J=2)
    add("quad4", "stft", 256, 64, "stft.quad4", "quad", _wave_launcher("quad", 4, "spectrum"), J=4)
    add("quad8", "stft", 128, 32, "stft.quad8", "quad", _wave_launcher("quad", 8, "spectrum"), J=8)
    add("real2x", "stft", 2048, 512, "stft.real2x", "real2x", _wave_launcher("real2x", 2, "spectrum"))
    add("real2x-4k", "stft", 4096, 1024, "stft.real2x.4k", "real2x", _wave_launcher("real2x", 2, "spectrum", C=2048))
    add("8k", "stft", 8192, 2048, "stft.8k", "8k", LAUNCHER_8K, M=25)
    add("r20", "stft", 400, 100, "stft.r20", "r20", _r20_launcher("spectrum"))
    for K in RAB_LENGTHS:
        add(f"rab{K}", "stft", K, K // 4, "stft.rab", "rab", _rab_launcher(K, "spectrum"))
    add("blue443", "stft", 443, 110, "stft.blue", "blue", LAUNCHER_BLUE, base=(("NXSIG_DISABLE_RAB", 1),))
    add("blue1000", "stft", 1000, 250, "stft.blue", "blue", LAUNCHER_BLUE, base=(("NXSIG_DISABLE_RAB", 1),))
    add("c64-rab512", "stft_c64", 512, 128, "stft_c64.rab", "rab_c64", _rab_c64_launcher(512))
    for K in (1024, 2048, 4096):
        add(f"rows{K}", "fft_nd", K, K, "fft.rows_wave", "rows", _rows_launcher(K), rows=50, M=1)
    # ---- magnitude and log-mel sinks
    for sink, entry in (("mag", "magnitude"), ("mel", "mel")):
        add(f"{sink}-pair", entry, 1024, 256, f"{sink}.pair", "pair", _wave_launcher("pair", 2, entry))
        add(f"{sink}-quad2", entry, 512, 128, f"{sink}.quad2", "quad", _wave_launcher("quad", 2, entry), J=2)
        add(f"{sink}-real2x", entry, 2048, 512, f"{sink}.real2x", "real2x", _wave_launcher("real2x", 2, entry))
        add(f"{sink}-r20", entry, 400, 100, f"{sink}.r20", "r20", _r20_launcher(entry))
        add(f"{sink}-rab960", entry, 960, 240, f"{sink}.rab", "rab", _rab_launcher(960, entry))
    return out


FORWARD = _forward_cases()
PAIR_SPECTRUM = ("pair-hop256", "pair-hop320")
SMALL_CHUNKS = (1, 3, 5, 16, 18, 64)


def forward_geometries(case):
    """name -> switches (on top of case.base).  The pair kernel's spectrum launch of a call this small is the one-round geometry, which
    sizes its chunk itself (kernels_wave.hip:1149-1157): NXSIG_WAVE_UNITS_PER_WAVE reaches it with NXSIG_WAVE_SMALL_W=0 only"""
    d = case.launcher.dflt
    extra = {SMALL_W: 0} if case.key in PAIR_SPECTRUM else {}
    out = {}
    for v in sorted({1, 2, 3, d, d + 1, UPW_MAX}):
        out[f"upw{v}"] = {case.launcher.knob: v, **extra}
    if case.key in PAIR_SPECTRUM:
        out["small-w0"] = {SMALL_W: 0}
        for ch in SMALL_CHUNKS:
            out[f"chunk{ch}"] = {SMALL_CHUNK: ch}
            out[f"chunk{ch}-w0"] = {SMALL_CHUNK: ch, SMALL_W: 0}
    return out


def interior_units(case):
    """(u_lo, u_hi) of the streaming launch under :valid padding with L = (M - 1) hop + K: every frame lies inside the signal, so every
    unit is interior — except on the quad front-ends, whose staged 16-byte loads need complete units with 7 floats of slack behind the
    span (wave_stft.hpp:1546-1555): the ragged last unit of a row goes to the bounds-checked edge launch (one unit per wave)"""
    per = case.launcher.per_unit
    if case.kind == "quad":
        mh = min(case.M, (case.L - (case.K + 7)) // case.hop + 1)
        return 0, mh // per
    return 0, cdiv(case.M, per)


def forward_launch(case, knobs, num_cus=NUM_CUS):
    """the streaming launch of `case` under the switches `knobs` (case.base included or not: only geometry switches are read)"""
    la = case.launcher
    u_lo, u_hi = interior_units(case)
    upr, rows = (1, case.rows) if case.kind == "rows" else (u_hi - u_lo, case.rows)
    total = upr * rows
    W = la.W
    if case.key in PAIR_SPECTRUM:    # launch_stft_wave, case 1024 (kernels_wave.hip:1148-1160)
        pairs = rows * cdiv(case.M, 2)
        chunk = int(knobs.get(SMALL_CHUNK, 0))
        forced = chunk > 0
        if int(knobs.get(SMALL_W, 12)) >= 12 and (forced or pairs <= num_cus * 24):
            if not forced:
                wgs = (num_cus * 11) // 16
                chunk = cdiv(pairs, wgs)
                if chunk >= 16:
                    chunk = (chunk + 3) & ~3
            return Chunked("stft.pair.1r", 12, chunk, upr, rows, la.per_unit, u_lo)
        if forced and pairs <= num_cus * 24:
            return Chunked("stft.pair.1r", 4, chunk, upr, rows, la.per_unit, u_lo)
        upw = tuned_units_per_wave(knobs, WAVE_UPW, total, W, la.dflt, num_cus)
        chunk = W * max(1, upw)
        if upw == 2 and WAVE_UPW not in knobs and cdiv(total, 2 * W) <= num_cus * 3:     # wave_stft.hpp:1522-1524
            chunk = W * 3
        return Chunked(case.family, W, chunk, upr, rows, la.per_unit, u_lo)
    upw = tuned_units_per_wave(knobs, la.knob, total, W, la.dflt, num_cus)
    return Chunked(case.family, W, W * max(1, upw), upr, rows, la.per_unit, u_lo)


# --------------------------------------------------------------------------------------------------------------------------------- FIR
@dataclass(frozen=True)
class Fir:
    key: str
    taps: int
    mode: str
    L: int
    family: str
    launcher: Launcher
    rows: int = ROWS


FIR_LAUNCHERS = {
    "fir.wave32": Launcher(4, 4, 0, (("kernels_wave_fir32.hip:210", "constexpr int W = 4;"),
                                      ("kernels_wave_fir32.hip:233", "tuned_units_per_wave(c, kT_FIR_UNITS_PER_WAVE, a.total_dp, W, 4)"),
                                      ("kernels_wave.hip:1766", "(a.pb_hi - a.pb_lo) / 2")), FIR_UPW),
    "fir.pair": Launcher(4, 8, 0, (("kernels_wave.hip:1784", "return launch_fir_wave_W<4>(c, s, handled);"),
                                    ("kernels_wave.hip:1691", "c->tuning.set[kT_FIR_UNITS_PER_WAVE] ? tune(c, kT_FIR_UNITS_PER_WAVE, 8) : fill_units_per_wave(c, a.total_units, W, 8)"),
                                    ("kernels_wave.hip:1769", "rc = launch(true, a.pb_hi - a.pb_lo);")), FIR_UPW),
    "fir.r2k": Launcher(4, 8, 0, (("kernels_wave.hip:1746", "constexpr int W4 = 4;"),
                                   ("kernels_wave.hip:1749", "c->tuning.set[kT_FIR_UNITS_PER_WAVE] ? tune(c, kT_FIR_UNITS_PER_WAVE, 8) : fill_units_per_wave(c, b.total_units, W4, 8)"),
                                   ("kernels_wave.hip:1747", "b.units_per_row = 2 * (a.pb_hi - a.pb_lo);")), FIR_UPW),
}
# samples per unit: a double block pair (4 V), a block pair (2 V), one real block (V); V = block length - (taps - 1)
_FIR_SHAPES = {33: ("fir.wave32", 4 * (1024 - 32)), 257: ("fir.pair", 2 * (1024 - 256)), 513: ("fir.r2k", 2048 - 512)}
# about 50 units per row; + 20: rows no multiple of 32 samples (every row then has a grid phase of its own, FirWaveArgs::row_mod); one
# unit more where the stream launch would otherwise hold a multiple of W units per row (the host test checks what comes out)
_FIR_UNITS = {"fir257-same": 51, "fir513-full": 52}
FIR = {f"fir{taps}-{mode}": Fir(f"fir{taps}-{mode}", taps, mode, _FIR_UNITS.get(f"fir{taps}-{mode}", 50) * per + 20, fam, FIR_LAUNCHERS[fam])
       for taps, (fam, per) in _FIR_SHAPES.items() for mode in ("same", "full")}


def fir_geometries(case):
    return {f"upw{v}": {FIR_UPW: v} for v in (1, 2, 3, 8, 9, UPW_MAX)}


def fir_launch(case, knobs, num_cus=NUM_CUS):
    """launch_fir_wave_W (kernels_wave.hip:1563-1773) for contiguous, 16-byte aligned rows: the stream launch of the case's family"""
    taps, L, rows = case.taps, case.L, case.rows
    out_start = {"full": 0, "same": (taps - 1) // 2, "valid": taps - 1}[case.mode]
    out_len = {"full": L + taps - 1, "same": L, "valid": L - taps + 1}[case.mode]
    r2k = taps > 385
    K = 2048 if taps > 385 else 1024
    if K == 2048:     # leading zero taps make out_start a multiple of 4 (:1579-1588)
        lead = (4 - out_start % 4) % 4
        if cdiv(taps + lead - 1, 256) * 256 + 1 > K // 2 + 1:
            lead = 0
        taps, out_start = taps + lead, out_start + lead
    q = 256 if r2k else 32
    eff = cdiv(taps - 1, q) * q + 1
    if eff <= K // 2 + 1:
        taps = eff
    V = K - (taps - 1)
    phase = out_start % 32
    out_start -= phase
    xlo, xhi = -phase, L - phase
    row_mod = out_len % 32 if rows > 1 else 0
    margin = 31 if row_mod else 0
    first_block = (out_start - margin) // V if out_start - margin >= 0 else -1
    nblocks = (out_start + out_len - 1) // V - first_block + 1
    pairs_per_row = (nblocks + 1) // 2
    lo = 0
    while lo < pairs_per_row:
        b1 = first_block + 2 * lo
        if b1 * V - (taps - 1) >= xlo and b1 * V - out_start >= 0:
            break
        lo += 1
    hi = pairs_per_row
    while hi > lo:
        b1 = first_block + 2 * (hi - 1)
        if (b1 + 1 - first_block) < nblocks and b1 * V - (taps - 1) + V + K <= xhi - margin and b1 * V - out_start + 2 * V + margin <= out_len:
            break
        hi -= 1
    la = case.launcher
    if case.family == "fir.r2k":
        upr, per = 2 * (hi - lo), V
    elif case.family == "fir.wave32":
        hi -= (hi - lo) & 1
        upr, per = (hi - lo) // 2, 4 * V
    else:
        upr, per = hi - lo, 2 * V
    upw = tuned_units_per_wave(knobs, FIR_UPW, upr * rows, la.W, la.dflt, num_cus)
    launch = Chunked(case.family, la.W, la.W * max(1, upw), upr, rows, per)
    # first output sample (of the shifted grid of row 0; a row's grid moves by up to 31 samples) the stream launch writes
    return launch, (first_block + 2 * lo) * V - out_start


# ---------------------------------------------------------------------------------------------------------------------------- inverses
@dataclass(frozen=True)
class Inverse:
    """an inverse case.  entry: "istft", "istft_filtered", "istft_masked" (mask: "real" / "onesided"), "istft_packed".
    segs_per_unit: hop-segments one unit of a run covers; even: run lengths are rounded up to an even number (frame pairs);
    waves: resident waves per CU the run length derives from (None: = W of an LDS-sized workgroup, which drops out at these sizes,
    see inverse_launch); dflt_run: production shortest run; small_rule: the launcher takes runs of 2 for a small launch"""
    key: str
    entry: str
    N: int
    hop: int
    family: str
    lead: str                  # leading dispatch entry of the baseline
    segs_per_unit: int
    dflt_run: int
    waves: object
    cites: tuple
    even: bool = False
    small_rule: bool = True
    balanced_halo: object = None   # units of halo of istft_balanced_run_len's cost model, None: the plain max(ceil, min_run) rule
    base: tuple = ()
    mask: str = ""
    runs_per_cu_knob: bool = True

    @property
    def R(self):
        return cdiv(self.N, self.hop)


def _inverse_cases():
    out = {}

    def add(key, entry, N, hop, family, lead, spu, dflt_run, waves, cites, **kw):
        out[key] = Inverse(key, entry, N, hop, family, lead, spu, dflt_run, waves, tuple(cites) + (CITE_MIN_RUN,), **kw)

    wave_cites = (("kernels_wave.hip:1255", "tune(c, kT_ISTFT_RUNS_PER_CU, (DBL || s.filt || deep || half_deep) ? 8 : 12)"),
                  ("kernels_wave.hip:1259", "istft_min_run(c, total_segs, (int64_t)c->num_cus * waves_per_cu, (!HALF && !DBL) ? 4 : 8)"),
                  ("kernels_wave.hip:1261", "if (HALF) run_len = (run_len + 1) & ~(int64_t)1;"))
    for hop in (128, 256, 512, 1024):
        add(f"wave-deep-hop{hop}", "istft", 1024, hop, "istft.wave", "istft.wave.deep", 1, 4, 8, wave_cites)
        add(f"wave-hop{hop}", "istft", 1024, hop, "istft.wave", "istft.wave", 1, 4, 12, wave_cites, base=(("NXSIG_ISTFT_DEEP", 0),))
    add("wave-filt", "istft_filtered", 1024, 256, "istft.wave.filt", "istft.wave.filt", 1, 4, 8, wave_cites)
    mask_cites = (("kernels_wave_mask.hip:199", "tune(c, kT_ISTFT_RUNS_PER_CU, 8)"),
                  ("kernels_wave_mask.hip:201", "istft_min_run(c, total_segs, (int64_t)c->num_cus * waves_per_cu, 4)"))
    add("mask-real", "istft_masked", 1024, 256, "istft.wave.mask", "istft.wave.mask", 1, 4, 8, mask_cites, mask="real")
    add("mask-onesided", "istft_masked", 1024, 256, "istft.wave.mask", "istft.wave.mask", 1, 4, 8, mask_cites, mask="onesided")
    add("half-hop128", "istft", 512, 128, "istft.half", "istft.half.deep", 1, 8, 8, wave_cites + (("kernels_wave.hip:1254", "HALF && tune(c, kT_ISTFT_HALF_DEEP, R == 4 ? 1 : 0)"),), even=True)
    add("half-hop256", "istft", 512, 256, "istft.half", "istft.half", 1, 8, 12, wave_cites, even=True)
    quad_cites = (("kernels_wave.hip:1353", "const int64_t units_per_row = (a.segs_per_row + J - 1) / J;"),
                  ("kernels_wave.hip:1355", "tune(c, kT_ISTFT_RUNS_PER_CU, 12)"),
                  ("kernels_wave.hip:1359", "istft_min_run(c, total_units, (int64_t)c->num_cus * waves_per_cu, 8)"))
    add("quad-256", "istft", 256, 64, "istft.quad", "istft.quad", 4, 8, 12, quad_cites)
    add("quad-128", "istft", 128, 32, "istft.quad", "istft.quad", 8, 8, 12, quad_cites)
    add("dbl", "istft", 2048, 512, "istft.dbl", "istft.dbl", 1, 8, 8, wave_cites)
    add("4k", "istft", 4096, 1024, "istft.4k", "istft.4k", 1, 8, 4,
        (("kernels_wave.hip:1417", "const int waves_per_cu = 4;"), ("kernels_wave.hip:1419", "istft_min_run(c, total_segs, (int64_t)c->num_cus * waves_per_cu, 8)")),
        runs_per_cu_knob=False)
    add("packed", "istft_packed", 1024, 256, "istft.packed", "istft.packed", 1, 8, 12,
        (("kernels_wave_packed.hip:208", "tune(c, kT_ISTFT_RUNS_PER_CU, 12)"), ("kernels_wave_packed.hip:210", "tune(c, kT_ISTFT_MIN_RUN, 8)"),
         ("kernels_wave_packed.hip:212", "run_len = (run_len + 1) & ~(int64_t)1;")), even=True, small_rule=False)
    add("r20", "istft", 400, 160, "istft.r20", "istft.r20", 3, 8, None,
        (("kernels_wave_r20.hip:610", "a.units_per_row = (segs + 2) / 3;"), ("kernels_wave_r20.hip:612", "istft_balanced_run_len(a.units_per_row, s.batch, (int64_t)c->num_cus * waves_per_cu, (RP - 1 + 2) / 3,"),
         ("kernels_wave_r20.hip:613", "istft_min_run(c, a.units_per_row * s.batch, (int64_t)c->num_cus * waves_per_cu, 8)"), CITE_BALANCED),
        balanced_halo=lambda RP, T: cdiv(RP - 1, 3))
    rab_cites = (("wave_rab.hpp:1198", "a.units_per_row = (segs + T - 1) / T;"),
                 ("wave_rab.hpp:1231", "istft_balanced_run_len(a.units_per_row, s.batch, (int64_t)c->num_cus * waves_per_cu, (RP - 1 + T - 1) / T,"),
                 ("wave_rab.hpp:1232", "istft_min_run(c, a.units_per_row * s.batch, (int64_t)c->num_cus * waves_per_cu, 8)"), CITE_BALANCED)
    for N, hop in ((960, 240), (512, 160)):
        T = 64 // max({**RAB_FACTORS, **RAB_INVERSE_ONLY}[N])
        add(f"rab{N}-hop{hop}", "istft", N, hop, "istft.rab", "istft.rab", T, 8, None, rab_cites, balanced_halo=lambda RP, T: cdiv(RP - 1, T))
    rabq_cites = (("wave_rab.hpp:1200", "if (hop * 4 == KB && tune(c, kT_ISTFT_REGOLA, 1))"),
                  ("wave_rab.hpp:1208", "istft_balanced_run_len(a.units_per_row, s.batch, (int64_t)c->num_cus * waves_per_cu, RP - 1,"),
                  ("wave_rab.hpp:1209", "istft_min_run(c, a.units_per_row * s.batch, (int64_t)c->num_cus * waves_per_cu, 8)"), CITE_BALANCED)
    for N in (1152, 2880):
        add(f"rabq{N}", "istft", N, N // 4, "istft.rab.q", "istft.rab.q", 1, 8, None, rabq_cites, balanced_halo=lambda RP, T: RP - 1)
    return out


INVERSE = _inverse_cases()
INVERSE_M = 61


def inverse_frames(case):
    """the two frame counts of a case: 61, and the shortest row the kernel takes (2R - 1: head and tail rows of the normaliser touch)"""
    return (INVERSE_M, 2 * case.R - 1)


def inverse_geometries(case, M):
    """the forced run lengths of the 3-row shapes.  The `-1cu` twins (NXSIG_ISTFT_RUNS_PER_CU=1) are run because a launch must not care,
    but at these sizes they CANNOT change a launch: 3 rows hold at most 231 units, fewer than the 256 wave slots of one wave per CU, so
    cdiv(total, slots) is 1 and the run length is what NXSIG_ISTFT_MIN_RUN says (the host test asserts exactly that).  The shapes on
    which the switch does change the runs are those of INVERSE_MANY_ROWS below"""
    out = {}
    for v in (1, 2, 3, 5, 8, 17, M, M + case.R + 5):
        out[f"run{v}"] = {MIN_RUN: v}
        out[f"run{v}-1cu"] = {MIN_RUN: v, RUNS_PER_CU: 1}
    return out


# One case per form of inverse launcher that reads NXSIG_ISTFT_RUNS_PER_CU (`istft.4k` derives its runs from a constant 4 waves per CU,
# kernels_wave.hip:1417), with enough rows of 61 frames that the switch decides the run length: more than four units per compute unit,
# so that run_len = cdiv(total_units, num_cus * RUNS_PER_CU) is 5 at one wave per CU, 3 at two, and falls back to
# NXSIG_ISTFT_MIN_RUN = 1 at 4096.  The non-finite twin keeps its placement in rows 0, 1 and 2.
MANY_ROWS_KEYS = ("wave-deep-hop256", "wave-hop256", "wave-filt", "mask-real", "half-hop128", "half-hop256", "quad-256", "dbl", "packed", "r20",
                  "rab960-hop240", "rabq1152")
MANY_ROWS_GEOMETRIES = {"1cu": {MIN_RUN: 1, RUNS_PER_CU: 1}, "2cu": {MIN_RUN: 1, RUNS_PER_CU: 2}, "4096cu": {MIN_RUN: 1, RUNS_PER_CU: 4096}}


def many_rows(case, num_cus=NUM_CUS):
    """rows of INVERSE_M frames that put more than 4 * num_cus units into the launch (runs of 5 and 3 units, 6 and 4 for the pair kernels)"""
    upr = inverse_launch(case, INVERSE_M, MANY_ROWS_GEOMETRIES["4096cu"], rows=1, num_cus=num_cus).units_per_row
    return cdiv(4 * num_cus + 1, upr)


@dataclass(frozen=True)
class Runs:
    run_len: int           # units
    units_per_row: int
    runs_per_row: int
    segs_per_unit: int

    def owner(self, segment):
        u = segment // self.segs_per_unit
        return dict(unit=u, run=u // self.run_len, first_unit_of_run=(u // self.run_len) * self.run_len)


def inverse_launch(case, M, knobs, rows=ROWS, num_cus=NUM_CUS):
    """run length -> runs per row of the case's launcher under `knobs`"""
    R = case.R
    if case.balanced_halo is None:
        segs = M + R - 1
    else:
        segs = cdiv((M - 1) * case.hop + case.N, case.hop)          # the last segment may be partial
    upr = cdiv(segs, case.segs_per_unit)
    total = upr * rows
    if case.waves is None:
        # one LDS-sized workgroup per CU: waves_per_cu = its W (1 ... 12).  At these sizes the launch is one partial round for any W >= 1
        # (asserted here), so W drops out of the run length — unless the switch names the waves per CU itself
        waves = int(knobs.get(RUNS_PER_CU, 1))
        assert RUNS_PER_CU in knobs or total <= num_cus, (case.key, total)
    else:
        waves = int(knobs.get(RUNS_PER_CU, case.waves)) if case.runs_per_cu_knob else case.waves
    slots = num_cus * waves
    if case.small_rule:
        min_run = istft_min_run(knobs, total, slots, case.dflt_run)
    else:
        min_run = int(knobs.get(MIN_RUN, case.dflt_run))
    if case.balanced_halo is not None:
        run_len = istft_balanced_run_len(upr, rows, slots, case.balanced_halo(R, case.segs_per_unit), min_run)
    else:
        run_len = max(cdiv(total, slots), min_run)
        if case.even:
            run_len = (run_len + 1) & ~1
    return Runs(run_len, upr, cdiv(upr, run_len), case.segs_per_unit)


def all_citations():
    """every (file:line, text) of the catalogue, once"""
    seen = {CITE_FILL, CITE_TUNED, CITE_MIN_RUN, CITE_BALANCED,
            ("kernels_wave.hip:1149", "int64_t chunk = tune(c, kT_WAVE_SMALL_CHUNK, 0);"),
            ("kernels_wave.hip:1157", "return launch_wave<1024, kModePair, 12>(c, s, nullptr, chunk);"),
            ("kernels_wave.hip:1159", "return launch_wave<1024, kModePair, 4>(c, s, nullptr, chunk);"),
            ("wave_stft.hpp:1524", "a.chunk = (int64_t)W * 3;"),
            ("wave_stft.hpp:1564", "a.chunk = (split < ((int64_t)1 << 61)) ? W : chunk_main;"),
            ("wave_stft.hpp:1554", "u_hi = mh / F;  // complete units only"),
            ("wave_rab.hpp:23", "#define NXSIG_RAB_PART0(X) X(320, 16, 20) X(480, 24, 20) X(640, 32, 20) X(960, 32, 30)"),
            ("wave_rab.hpp:34", "#define NXSIG_RAB_INVERSE_ONLY(X) X(128, 16, 8) X(256, 16, 16) X(512, 32, 16) X(1024, 32, 32)")}
    for c in list(FORWARD.values()) + list(FIR.values()):
        seen.update(c.launcher.cites)
    for c in INVERSE.values():
        seen.update(c.cites)
    return sorted(seen)
