// TEST INFRASTRUCTURE: AddressSanitizer / UndefinedBehaviorSanitizer run of the host side of Spectral.welch / csd that needs no GPU
// (nx_signal_amd/csrc/welch_plan.hpp): the argument checks, the bin count and the run geometry.  Built and run by
// tests/test_welch_host.py with g++ -fsanitize=address,undefined -fno-sanitize-recover.  For every plan the program plays the launch
// on the host: each unit of each row is marked by the run that owns it, each partial-sum cell by the run that stores it, through plain
// vectors, so that an index outside the buffers of the plan's own sizes aborts the process and a unit left out or taken twice fails it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "welch_plan.hpp"

using namespace nxsig;

static int fail(const char* what, long a, long b, long c) {
  std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static int play(int64_t M, int64_t rows, int32_t K, bool csd, bool fused, int32_t cus) {
  const WelchPlan p = welch_plan(M, rows, K, csd, fused, (int64_t)cus * (K == 1024 ? 12 : 6));
  if (p.run_len < 1 || p.runs_per_row < 1 || p.slab_rows < 1 || p.slab_rows > rows || p.chunk_runs < 1) return fail("plan", M, rows, K);
  if ((p.runs_per_row - 1) * p.run_len >= p.units_per_row || p.runs_per_row * p.run_len < p.units_per_row) return fail("runs", M, rows, K);
  const int32_t nb = welch_bins(K);
  if (nb > p.plane_floats) return fail("plane", M, rows, K);
  const int64_t frames_per_unit = fused && !csd ? 2 : 1;
  for (int64_t r0 = 0; r0 < rows; r0 += p.slab_rows) {
    const int64_t srows = rows - r0 < p.slab_rows ? rows - r0 : p.slab_rows;
    std::vector<unsigned char> frame((size_t)(srows * M), 0);
    std::vector<unsigned char> cell((size_t)(srows * p.runs_per_row * p.planes * p.plane_floats), 0);
    const int64_t total_runs = srows * p.runs_per_row;
    const int64_t step = fused ? total_runs : p.chunk_runs;
    for (int64_t c0 = 0; c0 < total_runs; c0 += step) {
      const int64_t c1 = c0 + step < total_runs ? c0 + step : total_runs;
      if (!fused && (c1 - c0) * p.run_len > 32768 && p.chunk_runs > 1) return fail("chunk", M, rows, K);
      for (int64_t run = c0; run < c1; ++run) {
        const int64_t row = run / p.runs_per_row, u0 = (run - row * p.runs_per_row) * p.run_len;
        const int64_t u1 = u0 + p.run_len < p.units_per_row ? u0 + p.run_len : p.units_per_row;
        for (int64_t u = u0; u < u1; ++u)
          for (int64_t j = 0; j < frames_per_unit; ++j) {
            const int64_t m = u * frames_per_unit + j;
            if (m < M) frame.at((size_t)(row * M + m)) += 1;
          }
        // what the run stores: welch.pair all K bins of one plane; csd.pair bins 0 .. K / 2 + 127 of four; generic nb of each
        const int64_t stored = fused ? (csd ? K / 2 + 128 : K) : nb;
        for (int32_t pl = 0; pl < p.planes; ++pl)
          for (int64_t k = 0; k < stored; ++k) cell.at((size_t)((run * p.planes + pl) * p.plane_floats + k)) += 1;
      }
    }
    for (unsigned char f : frame) if (f != 1) return fail("frame coverage", M, rows, K);
    // what the finishing kernel reads was stored once
    for (int64_t row = 0; row < srows; ++row)
      for (int64_t run = 0; run < p.runs_per_row; ++run)
        for (int32_t pl = 0; pl < p.planes; ++pl)
          for (int32_t k = 0; k < nb; ++k) {
            const size_t at = (size_t)(((row * p.runs_per_row + run) * p.planes + pl) * p.plane_floats);
            if (cell.at(at + k) != 1) return fail("cell", M, rows, k);
            if (fused && !csd && cell.at(at + (K - k) % K) != 1) return fail("mirror cell", M, rows, k);
          }
  }
  return 0;
}

int main() {
  int bad = 0;
  // the argument checks: every message once, and the valid call
  struct { int64_t L; int32_t b; int64_t bs; int32_t n, hop, k, sc; double fs; bool ok; } cases[] = {
      {40, 2, 40, 16, 8, 32, 0, 8000.0, true},   {0, 2, 40, 16, 8, 32, 0, 1.0, false},  {40, 0, 40, 16, 8, 32, 0, 1.0, false},
      {40, 2, 39, 16, 8, 32, 0, 1.0, false},     {40, 2, 40, 0, 8, 32, 0, 1.0, false},  {40, 2, 40, 16, 0, 32, 0, 1.0, false},
      {40, 2, 40, 16, 17, 32, 0, 1.0, false},    {40, 2, 40, 16, 8, 15, 0, 1.0, false}, {40, 2, 40, 16, 8, (1 << 24) + 1, 0, 1.0, false},
      {40, 2, 40, 41, 8, 64, 0, 1.0, false},     {40, 2, 40, 16, 8, 32, 2, 1.0, false}, {40, 2, 40, 16, 8, 32, -1, 1.0, false},
      {40, 2, 40, 16, 8, 32, 0, 0.0, false},     {40, 2, 40, 16, 8, 32, 1, -1.0, false},
      {INT64_MAX, 1, INT64_MAX, INT32_MAX, 1, INT32_MAX, 1, 1.0, false}, {INT64_MAX, INT32_MAX, INT64_MAX, 1, 1, 1, 1, 1e300, true}};
  for (const auto& c : cases)
    if ((welch_check_args(c.L, c.b, c.bs, c.n, c.hop, c.k, c.sc, c.fs) == nullptr) != c.ok) bad += fail("check_args", (long)c.L, c.n, c.k);
  if (welch_bins(0) != -1 || welch_bins(-5) != -1 || welch_bins(1) != 1 || welch_bins(255) != 128 || welch_bins(256) != 129 ||
      welch_bins(INT32_MAX) != INT32_MAX / 2 + 1)
    bad += fail("bins", 0, 0, 0);
  if (welch_frames(1023, 1024, 256) != 0 || welch_frames(1024, 1024, 256) != 1 || welch_frames(1279, 1024, 256) != 1 ||
      welch_frames(1280, 1024, 256) != 2 || welch_frames(INT64_MAX, 1, 1) != INT64_MAX || welch_frames(10, 0, 1) != 0 ||
      welch_frames(10, 4, 0) != 0)
    bad += fail("frames", 0, 0, 0);
  long plans = 0;
  for (int64_t M : {1, 2, 3, 5, 9, 37, 64, 65, 129, 3747})
    for (int64_t rows : {1, 3, 67})
      for (int32_t cus : {1, 256})
        for (int csd = 0; csd <= 1; ++csd) {
          for (int32_t K : {1024, 2048}) { bad += play(M, rows, K, csd != 0, true, cus); ++plans; }
          for (int32_t K : {1, 3, 64, 255, 512}) { bad += play(M, rows, K, csd != 0, false, cus); ++plans; }
        }
  // the row counts past the grid limit, and sizes whose partial sums need slabs or whose spectra need one-run chunks
  bad += play(1, 65537, 1024, false, true, 256) + play(2, 65537, 64, false, false, 256) + play(1, 20000, 2048, true, true, 256);
  bad += play(40, 3, 1 << 20, false, false, 256) + play(3, 2, 1 << 20, true, false, 256);
  if (bad) return 1;
  std::printf("sanitized welch host side ok: %ld plans\n", plans + 5);
  return 0;
}
