// Spectral.yin: everything of it that is plain C++ — the argument checks, the frame count and the geometry of
// yin.tile (lags per thread, threads per frame, frames per workgroup, the LDS layout).  The C entry points and the kernels of
// kernels_yin.hip share this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace nxsig {

constexpr int64_t kYinMaxFrame = 4096;                    // the staged samples of a frame stay within 40 KB of LDS
constexpr int64_t kYinMaxFrames = (int64_t)1 << 40;       // frames of one call

// ---- the definition.  center = 0: librosa.util.frame, F = 1 + (n - L) / hop frames at multiples of hop.  center = 1: the row is
// extended by L / 2 zeros on both sides first, so frame f starts at f hop - L / 2 of the row
inline int64_t yin_frames(int64_t n, int64_t frame_length, int64_t hop, int32_t center) {
  return 1 + (n + (center ? 2 * (frame_length / 2) : 0) - frame_length) / hop;
}
inline int64_t yin_window(int64_t frame_length) { return frame_length / 2; }                        // W
inline int64_t yin_max_period(int64_t frame_length) { return frame_length - frame_length / 2 - 1; }  // the largest lag

// the errors of (n, frame_length, hop, center) alone; nullptr when all is well
inline const char* yin_check_framing(int64_t n, int64_t frame_length, int64_t hop, int32_t center, bool* unsupported) {
  *unsupported = false;
  if (center != 0 && center != 1) return "center must be 0 or 1";
  if (frame_length < 4) return "frame_length must be >= 4";
  if (hop < 1) return "hop must be >= 1";
  if (n < 1) return "n must be >= 1";
  if (!center && frame_length > n) return "frame_length must be <= n without center";
  if (frame_length > kYinMaxFrame) { *unsupported = true; return "frames of up to 4096 samples are built"; }
  return nullptr;
}
inline const char* yin_check(int64_t batch, int64_t n, int64_t batch_stride, int64_t frame_length, int64_t hop, int32_t center,
                             int64_t min_period, int64_t max_period, double sr, double threshold, bool* unsupported) {
  // a frame that is too long is reported after the values that are wrong at any length
  const char* too_long = yin_check_framing(n, frame_length, hop, center, unsupported);
  if (too_long && !*unsupported) return too_long;
  *unsupported = false;
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < n) return "batch_stride must be >= n";
  if (min_period < 1) return "min_period must be >= 1";
  if (max_period <= min_period) return "max_period must be > min_period";
  if (max_period > yin_max_period(frame_length)) return "max_period must be <= frame_length - frame_length / 2 - 1";
  if (!(sr > 0) || !std::isfinite(sr)) return "sr must be finite and positive";
  if (!(threshold > 0) || !std::isfinite(threshold)) return "threshold must be finite and positive";
  *unsupported = true;
  if (too_long) return too_long;
  if (batch > ((int64_t)1 << 31) || batch_stride > INT64_MAX / 8 / (batch < 1 ? 1 : batch)) return "the rows are too large";
  if (batch * yin_frames(n, frame_length, hop, center) > kYinMaxFrames) return "at most 2^40 frames per call are built";
  *unsupported = false;
  return nullptr;
}

// ---- yin.tile.  A thread owns R consecutive lags (R double accumulators); kYinThreads[0] threads serve a frame when R of kYinLags
// covers its T + 1 lags with them, kYinThreads[1] otherwise.  A rule of max_period and the switch alone, never of the batch
constexpr int kYinLags[4] = {1, 2, 4, 8};
constexpr int kYinThreads[2] = {64, 256};
constexpr int kYinWaves = 4;                              // a workgroup of one-wave frames takes up to four consecutive frames
constexpr size_t kYinLdsBytes = 64 << 10;                 // a workgroup's staged frames stay within this

struct YinGeometry {
  int lags;           // R
  int threads;        // per frame: 64 or 256
  int block;          // B: template values per step of the walk over j, a multiple of R
  int frames;         // per workgroup: 1 for 256 threads, up to kYinWaves for 64 (fewer where LDS runs out)
  int64_t groups;     // groups of R staged samples per frame, each padded to yin_group_stride(R) doubles
  size_t frame_bytes; // LDS per frame
};
inline int yin_block(int lags) { return lags < 4 ? 4 : lags; }
// doubles between two groups of R samples: one more than R for even R, so that neighbouring lanes' window reads (R samples apart)
// fall into different banks
inline int yin_group_stride(int lags) { return lags == 1 ? 1 : lags + 1; }
// `forced` (NXSIG_YIN_LAGS) is taken when it is one of kYinLags and 256 threads of it cover the lags; 0 = automatic: the smallest R that
// covers the lags with one wave, else 4 or 8 lags on 256 threads
inline YinGeometry yin_geometry(int64_t frame_length, int64_t max_period, int forced) {
  const int64_t lags = max_period + 1, W = yin_window(frame_length);
  YinGeometry g = {};
  bool found = false;
  for (int r : kYinLags)
    if (r == forced && lags <= (int64_t)r * kYinThreads[1]) {
      g.lags = r; g.threads = lags <= (int64_t)r * kYinThreads[0] ? kYinThreads[0] : kYinThreads[1];
      found = true;
    }
  for (int t = 0; t < 2 && !found; ++t)
    for (int r : kYinLags)
      if (!found && (t == 0 || r >= 4) && lags <= (int64_t)r * kYinThreads[t]) { g.lags = r; g.threads = kYinThreads[t]; found = true; }
  g.block = yin_block(g.lags);
  // the staged samples x[1 ... W + T] and zeros up to the last one any lane reads: the walk's last block starts below W rounded up to
  // B, the last lane's window ends 2 B past its first lag
  const int64_t reach = (W + g.block - 1) / g.block * g.block + (int64_t)g.threads * g.lags + 2 * g.block;
  g.groups = (reach + g.lags - 1) / g.lags;
  g.frame_bytes = (size_t)g.groups * yin_group_stride(g.lags) * sizeof(double);
  g.frames = 1;
  if (g.threads == kYinThreads[0]) {
    g.frames = (int)(kYinLdsBytes / g.frame_bytes);
    if (g.frames > kYinWaves) g.frames = kYinWaves;
    if (g.frames < 1) g.frames = 1;
  }
  return g;
}

}  // namespace nxsig
