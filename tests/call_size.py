"""Launch geometries that depend on the SIZE of a call, restated in Python (no GPU needed).

The ten kernel families after the streaming ones — resample_poly, welch / csd, sosfilt, find_peaks, savgol, hilbert, dct, lfilter,
lombscargle, czt — have no geometry switch: their launchers pick the geometry from the total work of the call, set against the
compute-unit count or a byte budget.  At 3 rows and a few tiles every such choice lands on its first branch: one tile per workgroup,
runs of four units, one slab, one chunk, one trip of a grid-stride loop, one tile per lane of the offset scan.  The other branch — a loop
trip, a seam, a pointer offset — only runs when the call is large.

This module holds what tests/test_call_size_host.py (CPU) and tests/test_gpu_call_size.py share:

* the LAUNCHER ARITHMETIC of every such choice as a function of the shape and `num_cus`, each with `(file:line, text that line holds)`;
* the CASES: functions of `num_cus` that return the small call (at most 251 distinct rows, on the first branch), the large call (the
  same rows repeated, `idx = arange(rows) % distinct`, on the branch the case names), the dispatch family, and the geometry of both;
* EXISTING: the largest shapes the families' own GPU modules run today, with citations into those modules, so that the host test can
  show which branch they take.

A geometry object answers `first_branch()`, `reached()` (the case's claim about the large call) and `owner(row, elem)` (the workgroup,
trip, slab or chunk that owns an output element: only named in a failure message)."""
from dataclasses import dataclass, field

import resample_oracle as R

CSRC = "nx_signal_amd/csrc/"
NUM_CUS = 256            # compute units of an MI355X; the GPU module reads the device's own count
DISTINCT = 251           # distinct rows of a small call (a prime: the repetition lines up with no power-of-two geometry)
FP_DISTINCT = 17         # find_peaks: its oracle is a Python loop
MEMORY_CAP = 2 << 30     # device bytes a large call may need
THREADS = 256
FP_TILE = 4096
CU_COUNTS = (256, 64, 32)

CITE = {
    # resample.poly.lds
    "resample.tile": ("nxsig_internal.h:388", "constexpr int kResampleTile = 1024;"),
    "resample.want": ("kernels_resample.hip:222", "const int64_t want = (tiles * a.batch) / ((int64_t)c->num_cus * 4);"),
    "resample.tpw": ("kernels_resample.hip:223", "const int64_t tpw = want < 1 ? 1 : (want > 16 ? 16 : want);"),
    "resample.wg_per_row": ("kernels_resample.hip:224", "const int64_t wg_per_row = (tiles + tpw - 1) / tpw;"),
    "resample.tile_first": ("kernels_resample.hip:58", "const int tile_first = (blockIdx.x % wg_per_row) * p.tiles_per_wg;"),
    "resample.loop": ("kernels_resample.hip:65", "for (int tile = tile_first; tile < tile_end; ++tile) {"),
    "resample.sync": ("kernels_resample.hip:79", "__syncthreads();   // the previous tile's reads are done"),
    "resample.pad": ("kernels_resample.hip:215", "const bool pad = a.down % a.up == 0 && (a.down / a.up) % 2 == 0;"),
    "resample.up1": ("kernels_resample.hip:180", "if (p.up == 1) return pad ?"),
    # welch / csd
    "welch.part_bytes": ("welch_plan.hpp:10", "constexpr int64_t kWelchPartBytes = (int64_t)64 << 20;"),
    "welch.chunk_bytes": ("welch_plan.hpp:11", "constexpr int64_t kWelchChunkBytes = (int64_t)32 << 20;"),
    "welch.generic_run": ("welch_plan.hpp:12", "constexpr int32_t kWelchGenericRun = 64;"),
    "welch.units": ("welch_plan.hpp:52", "p.units_per_row = csd ? M : (M + 1) / 2;"),
    "welch.len": ("welch_plan.hpp:55", "int64_t len = (total + wave_slots - 1) / wave_slots;"),
    "welch.len_min": ("welch_plan.hpp:56", "if (len < 4) len = 4;"),
    "welch.len_max": ("welch_plan.hpp:57", "if (len > p.units_per_row) len = p.units_per_row;"),
    "welch.plane_fused": ("welch_plan.hpp:59", "p.plane_floats = csd ? K / 2 + 128 : K;"),
    "welch.run_generic": ("welch_plan.hpp:62", "p.run_len = M < kWelchGenericRun ? M : kWelchGenericRun;"),
    "welch.plane_generic": ("welch_plan.hpp:63", "p.plane_floats = K / 2 + 1;"),
    "welch.slab_rows": ("welch_plan.hpp:67", "p.slab_rows = kWelchPartBytes / row_bytes;"),
    "welch.slots_max": ("welch_plan.hpp:71", "int64_t slots_max = kWelchChunkBytes / ((int64_t)K * 8);"),
    "welch.slots_cap": ("welch_plan.hpp:72", "if (slots_max > 32768) slots_max = 32768;"),
    "welch.chunk_runs": ("welch_plan.hpp:73", "p.chunk_runs = slots_max / p.run_len;"),
    "welch.slots": ("kernels_welch.hip:395", "(a.K == 1024 ? 12 : csd ? 4 : 6);"),
    "welch.slab_loop": ("kernels_welch.hip:407", "for (int64_t r0 = 0; r0 < a.batch; r0 += p.slab_rows) {"),
    "welch.slab_y": ("kernels_welch.hip:411", "s.y = csd ? a.y + (size_t)r0 * a.batch_stride : nullptr;"),
    "welch.slab_pyy": ("kernels_welch.hip:427", "f.pyy = a.pyy ? a.pyy + (size_t)r0 * nb : nullptr;"),
    "welch.slab_pxy": ("kernels_welch.hip:428", "f.pxy = a.pxy ? a.pxy + (size_t)r0 * nb : nullptr;"),
    "welch.chunk_loop": ("kernels_welch.hip:362", "for (int64_t r0 = 0; r0 < total_runs; r0 += p.chunk_runs) {"),
    "welch.chunk_fy": ("kernels_welch.hip:354", "float* fy = fx + (size_t)slots_max * a.N;"),
    "welch.chunk_sy": ("kernels_welch.hip:356", "float2* sy = sx + (size_t)slots_max * a.K;"),
    # the grid-stride passes
    "hilbert.threads": ("kernels_hilbert.hip:24", "constexpr int kThreads = 256;"),
    "hilbert.cap": ("kernels_hilbert.hip:206", "cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;"),
    "hilbert.gain_loop": ("kernels_hilbert.hip:182", "i < total; i += (int64_t)gridDim.x * kThreads) {"),
    "hilbert.gain": ("kernels_hilbert.hip:232", "hipLaunchKernelGGL(k_hilbert_gain, dim3(stream_blocks(c, rows * N))"),
    "hilbert.sink": ("kernels_hilbert.hip:237", "hipLaunchKernelGGL(k_hilbert_sink, dim3(stream_blocks(c, rows * N))"),
    "czt.threads": ("kernels_czt.hip:24", "constexpr int kThreads = 256;"),
    "czt.cap": ("kernels_czt.hip:249", "cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;"),
    "czt.pre": ("kernels_czt.hip:257", "hipLaunchKernelGGL(k_czt_pre<false>, dim3(stream_blocks(c, rows * L))"),
    "czt.mul": ("kernels_czt.hip:260", "hipLaunchKernelGGL(k_czt_mul, dim3(stream_blocks(c, rows * L))"),
    "czt.post": ("kernels_czt.hip:263", "hipLaunchKernelGGL(k_czt_post, dim3(stream_blocks(c, rows * m))"),
    "dct.cap": ("kernels_dct.hip:205", "cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;"),
    "dct.gather_cap": ("kernels_dct.hip:268", "const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 64;"),
    "dct.gather_loop": ("kernels_dct.hip:143", "for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {"),
    "dct.post": ("kernels_dct.hip:273", "hipLaunchKernelGGL(k_dct2_post, dim3(stream_blocks(c, rows * a.keep))"),
    "dct.pre": ("kernels_dct.hip:278", "hipLaunchKernelGGL(k_dct3_pre, dim3(stream_blocks(c, rows * n))"),
    "dct.sink": ("kernels_dct.hip:282", "hipLaunchKernelGGL(k_dct3_sink, dim3(stream_blocks(c, rows * a.keep))"),
    "lombscargle.threads": ("lombscargle_plan.hpp:19", "constexpr int kLsGenericThreads = 256;"),
    "lombscargle.need": ("kernels_lombscargle.hip:267", "const int64_t total = (int64_t)l.batch * l.num_freqs, need = (total + kLsGenericThreads - 1) / kLsGenericThreads;"),
    "lombscargle.cap": ("kernels_lombscargle.hip:268", "const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;"),
    "lombscargle.loop": ("kernels_lombscargle.hip:181", "idx < total; idx += (int64_t)gridDim.x * kLsGenericThreads) {"),
    # find_peaks
    "find_peaks.tile": ("kernels_find_peaks.hip:25", "constexpr int kThreads = 256, kItems = 16, kTile = kThreads * kItems;"),
    "find_peaks.grid_for": ("kernels_find_peaks.hip:411", "most = (uint64_t)c->num_cus * 32;"),
    "find_peaks.scan_run": ("kernels_find_peaks.hip:295", "const uint64_t run = (ntiles + 1023) / 1024,"),
    "find_peaks.ntiles": ("kernels_find_peaks.hip:418", "const uint64_t ntiles = (G.total + kTile - 1) / kTile,"),
    "find_peaks.keep_grid": ("kernels_find_peaks.hip:465", "const unsigned grid = grid_for(c, G.total);"),
    "find_peaks.properties": ("kernels_find_peaks.hip:493", "dim3(grid_for(c, (uint64_t)a.capacity))"),
    "find_peaks.summary": ("kernels_find_peaks.hip:450", "const uint64_t groups = (nsum + 15) / 16, most = (uint64_t)c->num_cus * 32;"),
    # lfilter
    "lfilter.lanes": ("iir_plan.hpp:15", "constexpr int32_t kIirLanes = 64;"),
    "lfilter.chunk": ("lfilter_plan.hpp:23", "inline int32_t lf_chunk(int32_t n)"),
    "lfilter.tile": ("lfilter_plan.hpp:24", "inline int32_t lf_tile(int32_t n) { return lf_chunk(n) * kIirLanes; }"),
    "lfilter.generic_row": ("recurrence_scan.hpp:235", "const int64_t row = (int64_t)blockIdx.x * kLanes + threadIdx.x;"),
    "lfilter.generic_grid": ("recurrence_scan.hpp:326", "dim3((unsigned)(((int64_t)a.batch + kLanes - 1) / kLanes))"),
    "lfilter.scan_grid": ("recurrence_scan.hpp:329", "const unsigned blocks = (unsigned)(g.tiles * a.batch);"),
    "lfilter.carry_grid": ("recurrence_scan.hpp:333", "hipLaunchKernelGGL(k_scan_carry<F>, dim3((unsigned)a.batch)"),
    "lfilter.p_elems": ("recurrence_scan.hpp:291", "const size_t p_elems = scan ? (size_t)a.batch * g.tiles * NP * kLanes : 0;"),
    "lfilter.tile_start": ("recurrence_scan.hpp:221", "double* ts = tile_start + (row * g.tiles + t) * NP;"),
}


def cdiv(a, b):
    return -(-a // b)


_LIB = {}


def lib_constants():
    """the blocking sizes the library exports, read from it (loading the library needs no GPU)"""
    if not _LIB:
        from nx_signal_amd import _lib

        lib = _lib.load()
        _LIB.update(resample_tile=int(lib.nxsig_resample_tile()), find_peaks_block=int(lib.nxsig_find_peaks_block()),
                    lombscargle_block=tuple(int(lib.nxsig_lombscargle_block(w)) for w in range(3)),
                    lfilter={n: (int(lib.nxsig_lfilter_chunk(n)), int(lib.nxsig_lfilter_tile(n))) for n in (2, 8)})
    return _LIB


# ------------------------------------------------------------------------------------------------------------------- grid-stride passes
def stream_blocks(total, num_cus=NUM_CUS):
    """stream_blocks of kernels_hilbert.hip / _czt.hip / _dct.hip, grid_for of kernels_find_peaks.hip, the block count of
    lombscargle.generic: one block of 256 threads per 256 elements, at most num_cus * 32 of them"""
    return min(max(cdiv(total, THREADS), 1), max(num_cus, 1) * 32)


def stream_cap(num_cus=NUM_CUS):
    """elements one trip of such a launch covers at most"""
    return max(num_cus, 1) * 32 * THREADS


@dataclass(frozen=True)
class GridStride:
    """one element-wise pass: `rows` x `per_row` elements on stream_blocks(total) blocks, element i on trip i // (blocks * 256)"""
    name: str
    rows: int
    per_row: int
    num_cus: int = NUM_CUS

    @property
    def total(self):
        return self.rows * self.per_row

    @property
    def blocks(self):
        return stream_blocks(self.total, self.num_cus)

    @property
    def trips(self):
        return cdiv(self.total, self.blocks * THREADS)

    def first_branch(self):
        return self.trips == 1

    def reached(self):
        """a second trip, and a partial one: 1.05 to 1.3 times the cap"""
        return self.trips == 2 and 1.05 * stream_cap(self.num_cus) <= self.total <= 1.3 * stream_cap(self.num_cus)

    def first_row_of_the_last_trip(self):
        """the first row that lies wholly in the last trip"""
        return cdiv((self.trips - 1) * self.blocks * THREADS, self.per_row)

    def owner(self, row, elem):
        i = row * self.per_row + elem
        return dict(launch=self.name, trip=i // (self.blocks * THREADS), block=(i // THREADS) % self.blocks, of_trips=self.trips)

    def describe(self):
        return f"{self.name}: {self.total} elements on {self.blocks} blocks, {self.trips} trip(s)"


def rows_past_the_cap(per_row, num_cus, factor=1.15):
    """rows that put rows * per_row at `factor` times the cap of one trip"""
    return cdiv(int(factor * stream_cap(num_cus)), per_row)


def rows_under_the_cap(per_row, num_cus, most=DISTINCT):
    return max(1, min(most, stream_cap(num_cus) // per_row))


# ------------------------------------------------------------------------------------------------------------------- resample.poly.lds
@dataclass(frozen=True)
class ResampleLds:
    """launch_resample_poly's LDS tier: a workgroup runs tiles_per_wg consecutive tiles of one row"""
    n_out: int
    batch: int
    tile: int
    num_cus: int = NUM_CUS
    want_tpw: int = 1

    @property
    def tiles(self):
        return cdiv(self.n_out, self.tile)

    @property
    def tiles_per_wg(self):
        return min(max((self.tiles * self.batch) // (self.num_cus * 4), 1), 16)

    @property
    def wg_per_row(self):
        return cdiv(self.tiles, self.tiles_per_wg)

    def wg_tiles(self):
        """tiles of each workgroup of a row"""
        t = self.tiles_per_wg
        return [min(t, self.tiles - w * t) for w in range(self.wg_per_row)]

    def first_branch(self):
        return self.tiles_per_wg == 1

    def reached(self):
        return self.tiles_per_wg == self.want_tpw and max(self.wg_tiles()) >= 2

    def owner(self, row, elem):
        tile = elem // self.tile
        return dict(workgroup=row * self.wg_per_row + tile // self.tiles_per_wg, trip=tile % self.tiles_per_wg, tile=tile,
                    tiles_of_the_row_s_workgroups=self.wg_tiles())

    def describe(self):
        return f"resample.poly.lds: {self.tiles} tiles x {self.batch} rows, tiles_per_wg {self.tiles_per_wg}, workgroups of {self.wg_tiles()} tiles"


def n_for(n_out, up, down):
    """the smallest input length that gives at least n_out outputs (tests/test_gpu_resample.py n_for)"""
    n = max(1, (n_out * down) // up - 2)
    while R.length(n, up, down) < n_out:
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------------- welch / csd
WELCH_PART_BYTES = 64 << 20
WELCH_CHUNK_BYTES = 32 << 20
WELCH_GENERIC_RUN = 64


def welch_slots(K, csd, num_cus=NUM_CUS):
    """kernels_welch.hip:395: resident waves of the fused tier"""
    return max(num_cus, 1) * (12 if K == 1024 else 4 if csd else 6)


@dataclass(frozen=True)
class WelchPlan:
    """welch_plan of welch_plan.hpp"""
    M: int
    rows: int
    K: int
    csd: bool
    fused: bool
    num_cus: int = NUM_CUS
    want: tuple = ()          # the case's claim: ("run_len", v) | ("slabs", n) | ("chunks", n)

    @property
    def planes(self):
        return 4 if self.csd else 1

    @property
    def units_per_row(self):
        return self.M if (self.csd or not self.fused) else (self.M + 1) // 2

    @property
    def run_len(self):
        if not self.fused:
            return min(self.M, WELCH_GENERIC_RUN)
        length = cdiv(self.units_per_row * self.rows, welch_slots(self.K, self.csd, self.num_cus))
        return min(max(length, 4), self.units_per_row)

    @property
    def plane_floats(self):
        return (self.K // 2 + 128 if self.csd else self.K) if self.fused else self.K // 2 + 1

    @property
    def runs_per_row(self):
        return cdiv(self.units_per_row, self.run_len)

    @property
    def slab_rows(self):
        return min(max(WELCH_PART_BYTES // (self.runs_per_row * self.planes * self.plane_floats * 4), 1), self.rows)

    @property
    def slabs(self):
        return cdiv(self.rows, self.slab_rows)

    @property
    def chunk_runs(self):
        return max(min(WELCH_CHUNK_BYTES // (self.K * 8), 32768) // self.run_len, 1)

    @property
    def chunks_per_slab(self):
        """generic tier: launches of the frame / transform / reduce trio for the first slab"""
        return cdiv(self.runs_per_row * self.slab_rows, self.chunk_runs)

    def run_units(self):
        """units of each run of a row"""
        return [min(self.run_len, self.units_per_row - r * self.run_len) for r in range(self.runs_per_row)]

    def first_branch(self):
        one = self.slabs == 1 and (self.fused or self.chunks_per_slab == 1)
        return one and (not self.fused or self.run_len == 4 or self.run_len == self.units_per_row)

    def reached(self):
        what, v = self.want
        if what == "run_len":
            return self.fused and self.run_len == v > 4 and self.run_units()[-1] < v and self.runs_per_row >= 2
        if what == "slabs":
            return self.slabs >= v and self.rows % self.slab_rows != 0
        return not self.fused and self.chunks_per_slab >= v and (self.runs_per_row * self.slab_rows) % self.chunk_runs != 0

    def owner(self, row, elem):
        in_slab = row % self.slab_rows
        return dict(slab=row // self.slab_rows, of_slabs=self.slabs, chunk=None if self.fused else (in_slab * self.runs_per_row) // self.chunk_runs,
                    run_len=self.run_len, runs_per_row=self.runs_per_row)

    def describe(self):
        tier = ("csd" if self.csd else "welch") + (".pair" if self.fused else ".generic")
        return (f"{tier}: M {self.M}, {self.rows} rows, run_len {self.run_len}, runs of {self.run_units()} units, {self.slabs} slab(s) of "
                f"{self.slab_rows} rows" + ("" if self.fused else f", {self.chunks_per_slab} chunk(s) of {self.chunk_runs} runs"))


def rows_for_run_len(units_per_row, slots, run_len):
    """rows that make ceil(units_per_row * rows / slots) == run_len (the middle of the interval)"""
    return cdiv(int((run_len - 0.5) * slots), units_per_row)


# -------------------------------------------------------------------------------------------------------------------------- find_peaks
@dataclass(frozen=True)
class FindPeaks:
    """kernels_find_peaks.hip run(): the passes on grid_for(...) blocks and the one-workgroup scan of the tile counts"""
    lines: int
    n: int
    num_cus: int = NUM_CUS

    @property
    def total(self):
        return self.lines * self.n

    @property
    def capacity(self):
        return self.lines * max(0, (self.n - 1) // 2)

    @property
    def ntiles(self):
        return cdiv(self.total, FP_TILE)

    @property
    def scan_run(self):
        return cdiv(self.ntiles, 1024)

    def passes(self):
        return (GridStride("k_fp_keep / k_fp_remove", self.lines, self.n, self.num_cus),
                GridStride("k_fp_properties", self.lines, max(1, (self.n - 1) // 2), self.num_cus))

    def first_branch(self):
        return self.scan_run == 1 and all(p.first_branch() for p in self.passes())

    def reached(self):
        return self.scan_run >= 2 and self.ntiles % 1024 != 0 and all(p.trips >= 2 for p in self.passes())

    def owner(self, slot, _elem=0):
        return dict(properties=self.passes()[1].owner(0, slot), scan_run=self.scan_run, ntiles=self.ntiles)

    def describe(self):
        return (f"find_peaks: {self.lines} lines of {self.n}, {self.ntiles} tiles, {self.scan_run} tile(s) per scan thread, "
                + "; ".join(p.describe() for p in self.passes()))


# ----------------------------------------------------------------------------------------------------------------------------- lfilter
@dataclass(frozen=True)
class Lfilter:
    """recurrence_scan.hpp run<F> for kernels_lfilter.hip: scan passes on tiles * batch workgroups and one carry workgroup per row; the plain recurrence on
    ceil(batch / 64) workgroups of 64 rows"""
    order: int
    n: int
    batch: int
    chunk: int
    tile: int

    @property
    def tiles(self):
        return cdiv(self.n, self.tile)

    @property
    def chunks(self):
        return cdiv(self.n, self.chunk)

    @property
    def generic_blocks(self):
        return cdiv(self.batch, 64)

    def first_branch(self):
        return self.batch <= 65535      # every row count the suite has run: no grid dimension of the launches is past 16 bits

    def reached(self):
        return self.batch > 65535 and self.batch % 64 != 0 and self.chunks == 3 and self.n % self.chunk != 0

    def owner(self, row, elem):
        return dict(scan_workgroup=row * self.tiles + elem // self.tile, chunk=(elem % self.tile) // self.chunk, generic_workgroup=row // 64,
                    lane=row % 64, of_generic_workgroups=self.generic_blocks)

    def describe(self):
        return (f"lfilter order {self.order}: {self.batch} rows of {self.n} ({self.chunks} chunks of {self.chunk}), scan grid "
                f"{self.tiles * self.batch}, generic grid {self.generic_blocks} (last of {self.batch - 64 * (self.generic_blocks - 1)} rows)")


# ------------------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    key: str
    family: str               # the dispatch family both calls must report
    params: dict              # what the GPU module needs to build the call
    distinct: int             # rows of the small call
    rows: int                 # rows of the large call: small[arange(rows) % distinct]
    small: tuple              # geometry objects of the small call
    large: tuple              # ... of the large call, the same passes
    claims: tuple             # indices into `large` of the geometries that must be on the other branch
    device_bytes: int         # operands, results and scratch of the large call
    cites: tuple = field(default=())

    def bad_row(self):
        """a row of the large call that the other branch owns: the last but one"""
        return self.rows - 2

    def owner(self, row, elem):
        return [self.large[i].owner(row, elem) for i in self.claims]

    def describe(self):
        return " | ".join(g.describe() for g in self.large)


RESAMPLE_RATIOS = ((3, 2), (1, 2), (160, 441))      # neither padded nor pure decimation; both (an even decimation: PAD and UP1); neither


def resample_is_pad(up, down):
    return down % up == 0 and (down // up) % 2 == 0


def resample_cases(num_cus=NUM_CUS):
    """rows of 5 tiles (n_out = 4 tile + 37), batches of 2, 2.5 and 16 rows per compute unit: tiles_per_wg 2 (workgroups of 2, 2, 1
    tiles), 3 (3, 2) and 16 (one workgroup, 5 tiles)"""
    tile = lib_constants()["resample_tile"]
    n_out_want = 4 * tile + 37
    out = []
    for up, down in RESAMPLE_RATIOS:
        n = n_for(n_out_want, up, down)
        n_out = R.length(n, up, down)
        for complex_rows in (False, True):
            elem = 8 if complex_rows else 4
            for tpw, batch in ((2, 2 * num_cus), (3, (5 * num_cus) // 2), (16, 16 * num_cus)):
                distinct = min(DISTINCT, (2 * num_cus * 4 - 1) // cdiv(n_out, tile))
                out.append(Case(f"resample-{up}_{down}-{'c64' if complex_rows else 'f32'}-tpw{tpw}", "resample.poly.lds",
                                dict(up=up, down=down, n=n, n_out=n_out, complex=complex_rows, tile=tile, pad=resample_is_pad(up, down), up1=up == 1),
                                distinct, batch, (ResampleLds(n_out, distinct, tile, num_cus),), (ResampleLds(n_out, batch, tile, num_cus, tpw),), (0,),
                                batch * (n + n_out) * elem,
                                tuple(CITE[k] for k in CITE if k.startswith("resample."))))
    return out


def welch_run_cases(num_cus=NUM_CUS):
    """welch.pair / csd.pair with run_len > 4 and a ragged last run"""
    out = []
    for key, csd, N, hop, M, run_len in (("welch-1024-run7", False, 1024, 256, 37, 7), ("csd-1024-run7", True, 1024, 256, 37, 7),
                                         ("csd-2048-run6", True, 2048, 512, 14, 6)):
        upr = M if csd else (M + 1) // 2
        slots = welch_slots(N, csd, num_cus)
        rows = rows_for_run_len(upr, slots, run_len)
        distinct = min(DISTINCT, (4 * slots) // upr)
        length = N + (M - 1) * hop
        nb = N // 2 + 1
        large = WelchPlan(M, rows, N, csd, True, num_cus, ("run_len", run_len))
        part = large.slab_rows * large.runs_per_row * large.planes * large.plane_floats * 4
        out.append(Case(key, "csd.pair" if csd else "welch.pair", dict(N=N, K=N, hop=hop, M=M, length=length, csd=csd, fused=True), distinct, rows,
                        (WelchPlan(M, distinct, N, csd, True, num_cus),), (large,), (0,),
                        rows * length * 4 * (2 if csd else 1) + rows * nb * 4 * (4 if csd else 1) + part,
                        tuple(CITE[k] for k in ("welch.units", "welch.len", "welch.len_min", "welch.len_max", "welch.slots", "welch.plane_fused"))))
    return out


def csd_offset_cases(num_cus=NUM_CUS):
    """csd with several slabs (csd.pair) and several chunks (csd.generic); pxx, pyy and pxy are all asked for"""
    out = []
    # csd.pair 1024, M = 2: a row's partial sums are 4 planes of 640 floats, 6553 rows share the 64 MiB buffer
    N, hop, M = 1024, 512, 2
    probe = WelchPlan(M, 1 << 30, N, True, True, num_cus)
    rows = 2 * probe.slab_rows + probe.slab_rows // 2
    length, nb = N + (M - 1) * hop, N // 2 + 1
    large = WelchPlan(M, rows, N, True, True, num_cus, ("slabs", 3))
    out.append(Case("csd-pair-slabs", "csd.pair", dict(N=N, K=N, hop=hop, M=M, length=length, csd=True, fused=True), DISTINCT, rows,
                    (WelchPlan(M, DISTINCT, N, True, True, num_cus),), (large,), (0,),
                    2 * rows * length * 4 + rows * nb * 16 + WELCH_PART_BYTES,
                    tuple(CITE[k] for k in ("welch.part_bytes", "welch.slab_rows", "welch.slab_loop", "welch.slab_y", "welch.slab_pyy", "welch.slab_pxy"))))
    # csd.generic N = K = 64, rows of 96 samples (M = 2, one run per row): 16384 runs per chunk
    N, hop, M = 64, 32, 2
    probe = WelchPlan(M, 1 << 30, N, True, False, num_cus)
    rows = 2 * probe.chunk_runs + probe.chunk_runs // 2
    length, nb = N + (M - 1) * hop, N // 2 + 1
    large = WelchPlan(M, rows, N, True, False, num_cus, ("chunks", 3))
    slots = large.chunk_runs * large.run_len
    out.append(Case("csd-generic-chunks", "csd.generic", dict(N=N, K=N, hop=hop, M=M, length=length, csd=True, fused=False), DISTINCT, rows,
                    (WelchPlan(M, DISTINCT, N, True, False, num_cus),), (large,), (0,),
                    2 * rows * length * 4 + rows * nb * 16 + rows * 4 * nb * 4 + slots * N * 4 * 2 + slots * N * 8 * 2,
                    tuple(CITE[k] for k in ("welch.chunk_bytes", "welch.generic_run", "welch.run_generic", "welch.plane_generic", "welch.slots_max",
                                            "welch.slots_cap", "welch.chunk_runs", "welch.chunk_loop", "welch.chunk_fy", "welch.chunk_sy"))))
    return out


def _stride_case(key, family, params, per_row_of, claims, bytes_per_row, cites, num_cus, sized_by):
    """a case whose passes are GridStride launches: rows from the pass `sized_by` (1.15 times its cap)"""
    rows = rows_past_the_cap(per_row_of[sized_by][1], num_cus)
    distinct = min(rows_under_the_cap(per, num_cus) for _, per in per_row_of)
    return Case(key, family, params, distinct, rows, tuple(GridStride(n, distinct, per, num_cus) for n, per in per_row_of),
                tuple(GridStride(n, rows, per, num_cus) for n, per in per_row_of), claims, rows * bytes_per_row, tuple(CITE[k] for k in cites))


DCT_SHORT_N = 64         # dct.fft takes it under NXSIG_DISABLE_DCT_DIRECT (tests/test_gpu_dct.py FORCED_N, test_70000_rows_of_8)


def grid_stride_cases(num_cus=NUM_CUS):
    """the second, partial trip of the element-wise passes of hilbert.generic, czt.generic, dct.fft and lombscargle.generic"""
    out = []
    N = 1000
    out.append(_stride_case("hilbert-1000", "hilbert.generic", dict(N=N), (("k_hilbert_gain", N), ("k_hilbert_sink", N)), (0, 1),
                            N * (4 + 4 + 8 + 8 + 8), ("hilbert.threads", "hilbert.cap", "hilbert.gain_loop", "hilbert.gain", "hilbert.sink"), num_cus, 0))
    n, m, L = 1500, 700, 4096
    for complex_rows in (False, True):
        out.append(_stride_case(f"czt-1500-700-{'c64' if complex_rows else 'f32'}", "czt.generic", dict(n=n, m=m, L=L, complex=complex_rows),
                                (("k_czt_pre", L), ("k_czt_mul", L), ("k_czt_post", m)), (0, 1),
                                n * (8 if complex_rows else 4) + m * 8 + 2 * L * 8, ("czt.threads", "czt.cap", "czt.pre", "czt.mul", "czt.post"), num_cus, 0))
    # keep = 13 needs 77 times the rows of keep = n: at n = 1000 its spectra and temporaries alone are 3 GB, beyond the memory cap.
    # The row count is what reaches the branch, so it stays and the rows shrink: 64 points, on dct.fft with dct.direct switched off
    for t in (2, 3):
        for n, keep in ((1000, 1000), (DCT_SHORT_N, 13)):
            passes = (("k_dct2_post", keep),) if t == 2 else (("k_dct3_pre", n), ("k_dct3_sink", keep))
            sized_by = 0 if t == 2 else 1
            claims = (0,) if t == 2 else ((0, 1) if keep == n else (1,))
            out.append(_stride_case(f"dct-type{t}-n{n}-keep{keep}", "dct.fft", dict(n=n, keep=keep, type=t, forced=n <= 256), passes, claims,
                                    n * 4 + keep * 4 + n * 8 + n * (4 if t == 2 else 8) + 4,
                                    ("dct.cap", "dct.post", "dct.pre", "dct.sink", "dct.gather_cap", "dct.gather_loop"), num_cus, sized_by))
    n, F = 16, 1000
    out.append(_stride_case("lombscargle-16-1000", "lombscargle.generic", dict(n=n, F=F), (("k_ls_generic", F),), (0,), n * 4 + F * 4,
                            ("lombscargle.threads", "lombscargle.need", "lombscargle.cap", "lombscargle.loop"), num_cus, 0))
    return out


def find_peaks_cases(num_cus=NUM_CUS):
    """lines of 4096 along the last axis, more than 1024 tiles: k_fp_scan walks two tiles per thread, and every grid_for pass takes
    another trip"""
    n = FP_TILE
    lines = max(1024 + 76, cdiv(int(1.05 * stream_cap(num_cus)), (n - 1) // 2))
    large = FindPeaks(lines, n, num_cus)
    cites = tuple(CITE[k] for k in CITE if k.startswith("find_peaks."))
    return [Case(f"find_peaks-{tier}", f"find_peaks.{tier}", dict(n=n, generic=tier == "generic"), FP_DISTINCT, lines,
                 (FindPeaks(FP_DISTINCT, n, num_cus),), (large,), (0,),
                 large.total * 4 + large.total // 4 + large.capacity * (8 * 8 + 4 * 7 + 4 + 8) + large.capacity * 4, cites) for tier in ("tables", "generic")]


LFILTER_ROWS = 65537


def lfilter_cases(num_cus=NUM_CUS):
    """65 537 rows of three chunks (the last one ragged): past 65 535 workgroups in a grid dimension, and a last workgroup of one row on
    the plain recurrence.  The geometry does not depend on the compute-unit count"""
    out = []
    for order, name in ((2, "butter2_lp02"), (8, "butter4_bp")):
        chunk, tile = lib_constants()["lfilter"][order]
        n = 3 * chunk - 3
        for generic in (False, True):
            if generic and order == 2:
                continue
            for direction in (0, 1):
                np_pad = order
                scratch = 0 if generic else LFILTER_ROWS * cdiv(n, tile) * np_pad * 65 * 8
                out.append(Case(f"lfilter-order{order}-{'generic' if generic else 'scan'}-dir{direction}", "lfilter.generic" if generic else "lfilter.scan",
                                dict(order=order, name=name, n=n, generic=generic, direction=direction), DISTINCT, LFILTER_ROWS,
                                (Lfilter(order, n, DISTINCT, chunk, tile),), (Lfilter(order, n, LFILTER_ROWS, chunk, tile),), (0,),
                                LFILTER_ROWS * (2 * n * 4 + 2 * np_pad * 8) + scratch,
                                tuple(CITE[k] for k in CITE if k.startswith("lfilter."))))
    return out


def all_cases(num_cus=NUM_CUS):
    return (resample_cases(num_cus) + welch_run_cases(num_cus) + csd_offset_cases(num_cus) + grid_stride_cases(num_cus) + find_peaks_cases(num_cus)
            + lfilter_cases(num_cus))


def case_keys():
    """the keys of every case; they do not depend on the compute-unit count, and forming them loads nothing"""
    keys = [f"resample-{up}_{down}-{d}-tpw{t}" for up, down in RESAMPLE_RATIOS for d in ("f32", "c64") for t in (2, 3, 16)]
    keys += ["welch-1024-run7", "csd-1024-run7", "csd-2048-run6", "csd-pair-slabs", "csd-generic-chunks", "hilbert-1000",
             "czt-1500-700-f32", "czt-1500-700-c64"]
    keys += [f"dct-type{t}-n{n}-keep{k}" for t in (2, 3) for n, k in ((1000, 1000), (DCT_SHORT_N, 13))]
    keys += ["lombscargle-16-1000", "find_peaks-tables", "find_peaks-generic"]
    keys += [f"lfilter-order{o}-{tier}-dir{d}" for o, tier in ((2, "scan"), (8, "scan"), (8, "generic")) for d in (0, 1)]
    return keys


def all_citations():
    return sorted(set(CITE.values()))


# ---------------------------------------------------------------------------------------------- what the families' own modules run today
# (family, (test file:line, text of that line), geometry at 256 compute units).  The largest call of every test of the modules
# tests/test_gpu_{resample,welch,hilbert,czt,dct,lombscargle,find_peaks,lfilter}.py that reaches the launcher in question.
def existing_shapes(num_cus=NUM_CUS):
    tile = 1024
    rs = lambda n_out, batch: ResampleLds(n_out, batch, tile, num_cus)    # noqa: E731
    wp = lambda M, rows, K, csd, fused: WelchPlan(M, rows, K, csd, fused, num_cus)   # noqa: E731
    gs = lambda name, rows, per: GridStride(name, rows, per, num_cus)     # noqa: E731
    return [
        # resample: 3 rows of up to 2 tile + 1 outputs, one row of 48001 samples at every ratio (3/1 gives the most outputs: 144003)
        ("resample.poly.lds", ("test_gpu_resample.py:101", "for n in [1, 2, 5] + [n_for(t, up, down) for t in (tile - 1, tile, tile + 1, 2 * tile + 1)]:"), rs(2 * tile + 1, 3)),
        ("resample.poly.lds", ("test_gpu_resample.py:109", "x = signal(48001 + up, (1, 48001))"), rs(3 * 48001, 1)),
        ("resample.poly.lds", ("test_gpu_resample.py:167", "for n in (5, n_for(tile, up, down), n_for(3 * tile + 5, up, down)):"), rs(3 * tile + 5, 3)),
        ("resample.poly.lds", ("test_gpu_resample.py:261", "x = signal(48, (3, 48000))"), rs(16000, 3)),
        # welch / csd: 3 or 4 rows of up to 61 frames, one row of 3747 frames, 65537 rows of one frame (welch only)
        ("welch.pair", ("test_gpu_welch.py:103", '("1024-hop256-M37-tail", 3, 1024 + 36 * 256 + 100, 1024, 768, 1024),'), wp(37, 3, 1024, False, True)),
        ("csd.pair", ("test_gpu_welch.py:103", '("1024-hop256-M37-tail", 3, 1024 + 36 * 256 + 100, 1024, 768, 1024),'), wp(37, 3, 1024, True, True)),
        ("csd.pair", ("test_gpu_welch.py:110", '("2048-hop512", 3, 2048 + 13 * 512 + 5, 2048, 1536, 2048),'), wp(14, 3, 2048, True, True)),
        ("welch.pair", ("test_gpu_welch.py:141", "assert (n - 1024) // 256 + 1 == 3747"), wp(3747, 1, 1024, False, True)),
        ("csd.pair", ("test_gpu_welch.py:141", "assert (n - 1024) // 256 + 1 == 3747"), wp(3747, 1, 1024, True, True)),
        ("csd.pair", ("test_gpu_welch.py:291", "length = 1024 + 60 * 256"), wp(61, 3, 1024, True, True)),
        ("csd.generic", ("test_gpu_welch.py:115", '("64", 3, 64 * 70, 64, 32, 64),'), wp(139, 3, 64, True, False)),
        ("csd.generic", ("test_gpu_welch.py:291", "length = 1024 + 60 * 256"), wp(61, 3, 1024, True, False)),
        # hilbert.generic: 65 rows of 2048 under the switch, 3 rows of 6000, one row of 32768
        ("hilbert.generic", ("test_gpu_hilbert.py:108", '@pytest.mark.parametrize("batch", [1, 2, 3, 65])'), gs("k_hilbert_gain", 65, 2048)),
        ("hilbert.generic", ("test_gpu_hilbert.py:167", '@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 512, 1000, 1025, 4096, 6000])'), gs("k_hilbert_gain", 3, 6000)),
        ("hilbert.generic", ("test_gpu_hilbert.py:181", "x = noise(15, (1, 1 << 15))"), gs("k_hilbert_gain", 1, 1 << 15)),
        # lombscargle.generic: at most 2 RB + 3 rows of 96 frequencies
        ("lombscargle.generic", ("test_gpu_lombscargle.py:190", "rows, n, F = 2 * RB + 3, x.shape[0], freqs.shape[0]"), gs("k_ls_generic", 19, 96)),
        ("lombscargle.generic", ("test_gpu_lombscargle.py:245", "x, y64, freqs, weights = inputs(77, 3, 300, 70, tmax=1e5, wmax=1e2)"), gs("k_ls_generic", 3, 70)),
        # find_peaks: 8 lines of 5 tiles + 77, 70 lines of 3 B + 5, 5 lines of two super-blocks
        ("find_peaks", ("test_gpu_find_peaks.py:285", "x = noise(51, (8, 5 * TILE + 77), step=1e-2)"), FindPeaks(8, 5 * FP_TILE + 77, num_cus)),
        ("find_peaks", ("test_gpu_find_peaks.py:136", '@pytest.mark.parametrize("rows", [1, 3, 70])'), FindPeaks(70, 3 * 64 + 5, num_cus)),
        ("find_peaks", ("test_gpu_find_peaks.py:211", "n = 2 * S + 70"), FindPeaks(5, 2 * 64 * 64 + 70, num_cus)),
        # czt.generic and dct.fft at 3 to 65 rows of up to 2048 / 8192 points
        ("czt.generic", ("test_gpu_czt.py:36", "SHAPES = [(1, 1), (3, 7), (600, 300), (512, 513), (513, 513), (1024, 1025), (1500, 549), (1025, 1025), (5000, 37), (100, 5000),"), gs("k_czt_pre", 65, 8192)),
        ("dct.fft", ("test_gpu_dct.py:39", "FFT_N = [257, 400, 1000, 1024, 2048, 4099, 65536]"), gs("k_dct2_post", 65, 2048)),
        ("dct.fft", ("test_gpu_dct.py:39", "FFT_N = [257, 400, 1000, 1024, 2048, 4099, 65536]"), gs("k_dct2_post", 3, 65536)),
        ("dct.fft", ("test_gpu_dct.py:172", "x = noise(70, (70000, 8))"), gs("k_dct2_post", 70000, 8)),
        # lfilter: 1, 3, 5 and 65 rows
        ("lfilter", ("test_gpu_lfilter.py:213", "x = noise(7, (65, n))"), Lfilter(8, 4096 + 9, 65, 64, 4096)),
    ]


# Two calls of today's suite are NOT on the first branch, and the catalogue says so instead of leaving them out: 65 rows of 65536 points.
# Their rows are a power of two and their passes run whole rows (keep = n, m < L), so every trip boundary of theirs falls on a row
# boundary and every trip is a full one: `i / N` and `i - r * N` never see a row that two trips share, nor a last trip that ends
# inside the grid, which the cases above (N = 1000, keep = 13: a row across the seam; all of them: a partial second trip) do.
def existing_shapes_past_the_cap(num_cus=NUM_CUS):
    gs = lambda name, rows, per: GridStride(name, rows, per, num_cus)     # noqa: E731
    return [
        ("czt.generic", ("test_gpu_czt.py:37", "(1000, 25), (2048, 1), (40000, 64)]"), gs("k_czt_pre", 65, 65536)),
        ("dct.fft", ("test_gpu_dct.py:145", "if n > 2048 and batch != 3 and (norm is not None or scale != 1.0):"), gs("k_dct2_post", 65, 65536)),
    ]
