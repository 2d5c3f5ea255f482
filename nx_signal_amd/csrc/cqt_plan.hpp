// Spectral.cqt / vqt: everything of it that is plain C++ — the argument checks, the frame count, the bin tiles
// of cqt.mfma and the cell of its table that a tap lands in.  The C entry points and the kernels of kernels_cqt.hip share this one
// copy.  No HIP types.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nxsig {

constexpr int64_t kCqtMaxBins = 4096;                     // bins of one bank
constexpr int64_t kCqtMaxCount = (int64_t)1 << 24;        // taps of one bin
constexpr int64_t kCqtMaxTaps = (int64_t)1 << 22;         // taps of one bank (the padded table of cqt.mfma is at most 16 times this)
constexpr int64_t kCqtMaxLo = (int64_t)1 << 40;           // |lo| and the row length
enum : int32_t { kCqComplex = 0, kCqMagnitude = 1, kCqPower = 2 };

// ---- the definition: frames are centred at t hop, t = 0 ... length / hop
inline int64_t cqt_frames(int64_t length, int64_t hop) { return 1 + length / hop; }

inline const char* cqt_check_framing(int64_t length, int64_t hop, bool* unsupported) {
  *unsupported = false;
  if (length < 1) return "length must be >= 1";
  if (hop < 1) return "hop must be >= 1";
  if (length > kCqtMaxLo || hop > kCqtMaxLo) { *unsupported = true; return "length and hop must be at most 2^40"; }
  return nullptr;
}
// lo and count are read only once n_bins is known to be sane; *total: the taps of the bank
inline const char* cqt_check(int64_t batch, int64_t length, int64_t batch_stride, int64_t hop, int64_t n_bins, const int64_t* lo,
                             const int32_t* count, int32_t kind, bool* unsupported, int64_t* total) {
  if (const char* what = cqt_check_framing(length, hop, unsupported)) return what;
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < length) return "batch_stride must be >= length";
  if (n_bins < 1) return "n_bins must be >= 1";
  if (kind != kCqComplex && kind != kCqMagnitude && kind != kCqPower) return "output_kind must be 0 (complex), 1 (magnitude) or 2 (power)";
  if (n_bins > kCqtMaxBins) { *unsupported = true; return "at most 4096 bins are built"; }
  int64_t sum = 0;
  bool big = false;
  for (int64_t k = 0; k < n_bins; ++k) {
    if (count[k] < 2) return "every bin must have at least 2 taps";
    big = big || count[k] > kCqtMaxCount || lo[k] > kCqtMaxLo || lo[k] < -kCqtMaxLo;
    sum += count[k];
  }
  *unsupported = true;
  if (big || sum > kCqtMaxTaps) return "a bin of at most 2^24 taps, |lo| <= 2^40 and a bank of at most 2^22 taps are built";
  if (batch > ((int64_t)1 << 24) || batch_stride > INT64_MAX / 8 / (batch < 1 ? 1 : batch)) return "the rows are too large";
  if (batch * n_bins > ((int64_t)1 << 40) / cqt_frames(length, hop)) return "at most 2^40 outputs per call are built";
  *unsupported = false;
  *total = sum;
  return nullptr;
}

// ---- cqt.mfma: D[bin, frame] = sum_n A[bin, n] X[n, frame] on v_mfma_f32_16x16x4_f32, bins on M, frames on N, samples on K.
// Bins are sorted by length (longest first, ties by index) and cut into tiles of kCqtTileBins; a tile walks the n range of all its
// bins in sub-panels of kCqtSub samples, kCqtPanelSubs of which form a panel whose f32 sums are added to the double sums.
constexpr int kCqtTileBins = 16;      // M of the matrix instruction: 16 bins at 12 per octave span 2.4 x in length, about 67 % of the products useful
constexpr int kCqtTileFrames = 16;    // N
constexpr int kCqtSub = 64;           // samples staged per step of the walk: 16 matrix steps of K = 4
constexpr int kCqtPanelSubs = 8;      // a panel is 512 samples
constexpr int kCqtWaves = 4;          // per workgroup
constexpr int kCqtWaveTiles = 2;      // frame tiles per wave: the A operand of a step serves both
constexpr int kCqtBlockFrames = kCqtWaves * kCqtWaveTiles * kCqtTileFrames;   // 128 frames share a staged basis sub-panel
constexpr int kCqtPitch = kCqtSub + 4;                                        // words between two frames' staged samples
constexpr size_t kCqtLdsBytes = (size_t)kCqtBlockFrames * kCqtPitch * 4 + (size_t)kCqtSub / 4 * 64 * 8;   // signal + basis: 43 008

struct CqtTile {
  int64_t first, bins;   // its bins are order[first ... first + bins)
  int64_t n_lo;          // the smallest n of its bins
  int64_t subs;          // sub-panels that cover [n_lo, the largest n of its bins]
  int64_t sub_off;       // sub-panels of the tiles before it: its part of the table starts at sub_off * 1024 cells
};
struct CqtPlan {
  std::vector<int32_t> order;   // bins, longest first
  std::vector<CqtTile> tiles;
  int64_t subs_total = 0;       // the table holds subs_total * 1024 complex cells
};
inline void cqt_plan(int64_t n_bins, const int64_t* lo, const int32_t* count, CqtPlan* p) {
  p->order.resize((size_t)n_bins);
  for (int64_t k = 0; k < n_bins; ++k) p->order[(size_t)k] = (int32_t)k;
  std::stable_sort(p->order.begin(), p->order.end(), [&](int32_t a, int32_t b) { return count[a] > count[b]; });
  p->tiles.clear();
  p->subs_total = 0;
  for (int64_t first = 0; first < n_bins; first += kCqtTileBins) {
    CqtTile t;
    t.first = first; t.bins = std::min<int64_t>(kCqtTileBins, n_bins - first);
    int64_t n_lo = INT64_MAX, n_hi = INT64_MIN;
    for (int64_t m = 0; m < t.bins; ++m) {
      const int32_t k = p->order[(size_t)(first + m)];
      n_lo = std::min(n_lo, lo[k]); n_hi = std::max(n_hi, lo[k] + count[k] - 1);
    }
    t.n_lo = n_lo; t.subs = (n_hi - n_lo + kCqtSub) / kCqtSub; t.sub_off = p->subs_total;
    p->subs_total += t.subs;
    p->tiles.push_back(t);
  }
}
// the cell of the table (in complex elements) that tap n of the tile's m-th bin lands in.  Within a sub-panel, sample w = 16 g + s is
// the K index g of matrix step s: lane 16 g + m of step s holds it, so a lane's 16 samples of a sub-panel are consecutive (one frame's
// staged samples are read 16 bytes at a time) and a step's 64 cells are one 512-byte line
inline int64_t cqt_cell(const CqtTile& t, int64_t m, int64_t n) {
  const int64_t i = n - t.n_lo, u = i / kCqtSub, w = i % kCqtSub, g = w / 16, s = w % 16;
  return ((t.sub_off + u) * 16 + s) * 64 + g * 16 + m;
}

// ---- cqt.direct: one wave per (bin, kCqtDirectFrames frames), the taps walked in chunks of kCqtDirectChunk (8 KB of LDS)
constexpr int kCqtDirectFrames = 8;
constexpr int kCqtDirectChunk = 256;

}  // namespace nxsig
