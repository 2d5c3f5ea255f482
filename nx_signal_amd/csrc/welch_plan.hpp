// Spectral.welch / csd: the host-side argument checks and the run geometry, free of HIP so that a stand-alone program can drive them
// under a sanitizer (tests/san_welch.cpp).  The geometry depends on shapes and the compute-unit count only: the same call gives the same
// partial sums, added in the same order, every time.
#pragma once

#include <cstdint>

namespace nxsig {

constexpr int64_t kWelchPartBytes = (int64_t)64 << 20;    // partial sums of one slab of rows
constexpr int64_t kWelchChunkBytes = (int64_t)32 << 20;   // spectra of one chunk of the generic tier
constexpr int32_t kWelchGenericRun = 64;                  // frames per run of the generic tier (fewer when a row has fewer)

// M = (L - N) / hop + 1 frames, no padding; 0 when the row is shorter than a frame
inline int64_t welch_frames(int64_t L, int32_t N, int32_t hop) { return L < N || N < 1 || hop < 1 ? 0 : (L - N) / hop + 1; }

// bins of a one-sided estimate, even and odd fft lengths alike (rfft); -1 when fft_length < 1
inline int32_t welch_bins(int32_t fft_length) { return fft_length < 1 ? -1 : fft_length / 2 + 1; }

// nullptr, or what is wrong with the arguments (the part of the message after the entry point's name)
inline const char* welch_check_args(int64_t length, int32_t batch, int64_t batch_stride, int32_t frame_length, int32_t hop, int32_t fft_length,
                                    int32_t scaling, double sampling_rate) {
  if (batch < 1 || length < 1) return "batch and length must be >= 1";
  if (batch_stride < length) return "batch_stride < length";
  if (frame_length < 1) return "frame_length must be >= 1";
  if (hop < 1 || hop > frame_length) return "hop must be in [1, frame_length] (0 <= overlap_length < frame_length)";
  if (fft_length < frame_length) return "fft_length must be >= frame_length";
  if (fft_length > (1 << 24)) return "fft_length beyond 2^24";
  if (length < frame_length) return "the rows are shorter than one frame (length < frame_length)";
  if (scaling != 0 && scaling != 1) return "scaling must be NXSIG_WELCH_DENSITY or NXSIG_WELCH_SPECTRUM";
  if (!(sampling_rate > 0.0) || sampling_rate > 1.0e300) return "sampling_rate must be a positive finite number";
  return nullptr;
}

struct WelchPlan {
  int64_t M;                // frames per row
  int64_t units_per_row;    // fused welch: pairs of frames, ceil(M / 2); fused csd and the generic tier: M
  int64_t run_len;          // units a run covers (the last run of a row may be shorter); runs never straddle a row
  int64_t runs_per_row;
  int32_t planes;           // sums per bin: 1 (welch), 4 (csd: Pxx, Pyy, Re Pxy, Im Pxy)
  int64_t plane_floats;     // floats of one plane of one run
  int64_t slab_rows;        // rows whose partial sums share the buffer at one time (>= 1)
  int64_t chunk_runs;       // generic tier: runs whose frames are transformed at one time (>= 1)
};

// fused: the wave tier (K = 1024 / 2048); wave_slots > 0: the waves of that tier the device holds at one time.
inline WelchPlan welch_plan(int64_t M, int64_t rows, int32_t K, bool csd, bool fused, int64_t wave_slots) {
  WelchPlan p;
  p.M = M;
  p.planes = csd ? 4 : 1;
  if (fused) {
    p.units_per_row = csd ? M : (M + 1) / 2;
    // one run per resident wave over the whole call, at least four units each (a run's start-up is its window and tables)
    const int64_t total = p.units_per_row * rows;
    int64_t len = (total + wave_slots - 1) / wave_slots;
    if (len < 4) len = 4;
    if (len > p.units_per_row) len = p.units_per_row;
    p.run_len = len;
    p.plane_floats = csd ? K / 2 + 128 : K;
  } else {
    p.units_per_row = M;
    p.run_len = M < kWelchGenericRun ? M : kWelchGenericRun;
    p.plane_floats = K / 2 + 1;
  }
  p.runs_per_row = (p.units_per_row + p.run_len - 1) / p.run_len;
  const int64_t row_bytes = p.runs_per_row * p.planes * p.plane_floats * 4;
  p.slab_rows = kWelchPartBytes / row_bytes;
  if (p.slab_rows < 1) p.slab_rows = 1;
  if (p.slab_rows > rows) p.slab_rows = rows;
  // a chunk: at most 32 768 frame slots (run_len per run), spectra within kWelchChunkBytes
  int64_t slots_max = kWelchChunkBytes / ((int64_t)K * 8);
  if (slots_max > 32768) slots_max = 32768;
  p.chunk_runs = slots_max / p.run_len;
  if (p.chunk_runs < 1) p.chunk_runs = 1;
  return p;
}

}  // namespace nxsig
