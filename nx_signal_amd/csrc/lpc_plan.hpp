// Spectral.lpc: everything of it that is plain C++ — the argument checks, the frame count, the tier choice and
// the geometry of both tiers.  The C entry points and the kernels of kernels_lpc.hip share this one copy.  No HIP types.
#pragma once

#include <cstddef>
#include <cstdint>

namespace nxsig {

enum LpcTier : int32_t { kLpcWave = 0, kLpcRows = 1 };

constexpr int kLpcMaxOrder = 128;                         // a[0 ... 128]: three coefficients per lane of the wave that steps them up
constexpr int64_t kLpcMaxFrame = (int64_t)1 << 28;        // lpc.rows keeps 32 bytes per sample of a frame: 8 GiB at this length
constexpr int64_t kLpcMaxFrames = (int64_t)1 << 40;       // frames of one call

// ---- the definition.  librosa.util.frame: F = 1 + (n - L) // hop frames that start at multiples of hop, no padding
inline int64_t lpc_frames(int64_t n, int64_t frame_length, int64_t hop) { return 1 + (n - frame_length) / hop; }

// the errors of (n, frame_length, hop) alone; nullptr when all is well
inline const char* lpc_check_framing(int64_t n, int64_t frame_length, int64_t hop, bool* unsupported) {
  *unsupported = false;
  if (frame_length < 2) return "frame_length must be >= 2";
  if (hop < 1) return "hop must be >= 1";
  if (frame_length > n) return "frame_length must be <= n";
  if (frame_length > kLpcMaxFrame) { *unsupported = true; return "frames of up to 2^28 samples are built"; }
  return nullptr;
}
inline const char* lpc_check(int64_t batch, int64_t n, int64_t batch_stride, int64_t frame_length, int64_t hop, int64_t order, bool* unsupported) {
  if (const char* what = lpc_check_framing(n, frame_length, hop, unsupported)) return what;
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < n) return "batch_stride must be >= n";
  if (order < 1) return "order must be >= 1";
  if (order >= frame_length) return "order must be < frame_length";
  *unsupported = true;
  if (order > kLpcMaxOrder) return "orders up to 128 are built";
  if (batch > ((int64_t)1 << 31) || batch_stride > INT64_MAX / 8 / (batch < 1 ? 1 : batch)) return "the rows are too large";
  if (batch * lpc_frames(n, frame_length, hop) > kLpcMaxFrames) return "at most 2^40 frames per call are built";
  *unsupported = false;
  return nullptr;
}

// ---- lpc.wave: one wave owns a frame.  Its L - 1 (f, b) pairs lie BLOCKED over the lanes, lane l holding pairs l R ... l R + R - 1 in
// 2 R double registers; R is one of kLpcSlots, the smallest with 64 R >= L - 1
constexpr int kLpcWaves = 4;                              // waves of a workgroup: consecutive frames (of one row, mostly: they overlap)
constexpr int64_t kLpcWaveLimit = 2048;                   // the longest frame of lpc.wave: 2047 pairs in 64 x 32 slots
constexpr int kLpcSlots[4] = {2, 8, 16, 32};
inline int lpc_slots(int64_t frame_length) {
  for (int r : kLpcSlots)
    if (frame_length - 1 <= 64 * (int64_t)r) return r;
  return 0;
}
// a rule of the frame length and the switch alone (NXSIG_LPC_WAVE=0, or NXSIG_DISABLE_WAVE), never of the batch
inline int lpc_tier(int64_t frame_length, bool wave_on) { return wave_on && frame_length <= kLpcWaveLimit ? kLpcWave : kLpcRows; }

// ---- lpc.rows: one launch per stage over (frame, chunk) units; a chunk is kLpcChunk pairs, a CONSTANT, so the partial sums of a frame
// and the order they are added in depend on the frame length alone, never on the grid or the batch
constexpr int kLpcRowsThreads = 256;
constexpr int64_t kLpcChunk = 4096;                       // pairs per workgroup: 16 per thread
constexpr size_t kLpcSlabBytes = (size_t)256 << 20;       // the frames of a call are walked in slabs whose temporary stays within this
inline int64_t lpc_chunks(int64_t frame_length) { return (frame_length - 1 + kLpcChunk - 1) / kLpcChunk; }
// doubles of the temporary per frame: f and b of L - 1 pairs, twice (a stage reads one copy and writes the other), two partial sums
// per chunk and stage parity, the chunks' sums of x^2, and the reflection coefficients so far
inline size_t lpc_frame_doubles(int64_t frame_length, int64_t order) {
  return 4 * (size_t)(frame_length - 1) + 5 * (size_t)lpc_chunks(frame_length) + (size_t)order;
}
// frames per slab: as many as stay within kLpcSlabBytes and one launch's grid, at least one (a single longer frame takes what it needs)
inline int64_t lpc_slab_frames(int64_t frames_total, int64_t frame_length, int64_t order) {
  int64_t f = (int64_t)(kLpcSlabBytes / (lpc_frame_doubles(frame_length, order) * sizeof(double)));
  const int64_t grid = 0x7fffffffLL / lpc_chunks(frame_length);
  if (f > grid) f = grid;
  if (f < 1) f = 1;
  return f < frames_total ? f : frames_total;
}

}  // namespace nxsig
