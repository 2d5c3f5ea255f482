// PeakFinding.find_peaks: everything of it that is plain C++ — the argument checks, the capacity and block
// arithmetic, the walks along a line (plateau, prominence, width) with and without the line summary, and the round rule of the distance
// stage.  The kernels of kernels_find_peaks.hip call the walks as they stand here, so the stand-alone program tests/san_find_peaks.cpp
// runs the same code on the host under ASan / UBSan: the summary walks against the element-by-element ones, the rounds against the
// sequential rule.  No HIP types, no allocation in the walks.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define NXSIG_FP_HD __host__ __device__ __forceinline__
#else
#define NXSIG_FP_HD inline
#endif

namespace nxsig {

// axis positions per entry of the line summary (nxsig_find_peaks_block): one 16-lane group of the summary pass loads a block as
// 16-byte vectors, and a walk pays at most one block of single steps at either end
constexpr int kFindPeaksBlock = 64;
// blocks per entry of the summary's second level: a walk of w positions takes about w / 4096 + 2 * 64 + 2 * 64 steps
constexpr int kFindPeaksFan = 64;
constexpr int64_t kFindPeaksSuper = (int64_t)kFindPeaksBlock * kFindPeaksFan;

// bits of `conditions`, in SciPy's order of application; bounds holds a (min, max) pair for each but the distance
enum FindPeaksCondition : uint32_t {
  kFpPlateauSize = 1u << 0, kFpHeight = 1u << 1, kFpThreshold = 1u << 2, kFpDistance = 1u << 3, kFpProminence = 1u << 4, kFpWidth = 1u << 5,
  kFpConditionMask = (1u << 6) - 1
};
enum { kFpBoundPlateau = 0, kFpBoundHeight = 1, kFpBoundThreshold = 2, kFpBoundProminence = 3, kFpBoundWidth = 4, kFpBounds = 5 };
// bits of `want`: the f64 properties (rows of fprops, in this order), then the s32 ones (rows of iprops)
enum FindPeaksProperty : uint32_t {
  kFpPeakHeights = 0, kFpLeftThresholds, kFpRightThresholds, kFpProminences, kFpWidthHeights, kFpLeftIps, kFpRightIps, kFpWidths,
  kFpLeftBases, kFpRightBases, kFpLeftEdges, kFpRightEdges, kFpPlateauSizes, kFpProperties
};
constexpr int kFpF64Properties = 8, kFpS32Properties = 5;
constexpr uint32_t kFpWantMask = (1u << kFpProperties) - 1;

inline int fp_popcount(uint32_t v) {
  int c = 0;
  for (; v; v &= v - 1) ++c;
  return c;
}
inline int find_peaks_f64_rows(uint32_t want) { return fp_popcount(want & ((1u << kFpF64Properties) - 1)); }
inline int find_peaks_s32_rows(uint32_t want) { return fp_popcount((want & kFpWantMask) >> kFpF64Properties); }

// the most peaks `lines` lines of n samples hold: a peak needs a lower sample on either side
inline int64_t find_peaks_capacity(int64_t lines, int64_t n) { return n < 3 ? 0 : lines * ((n - 1) / 2); }
inline int64_t find_peaks_blocks(int64_t n) { return (n + kFindPeaksBlock - 1) / kFindPeaksBlock; }
inline int64_t find_peaks_supers(int64_t n) { return (n + kFindPeaksSuper - 1) / kFindPeaksSuper; }
// d = ceil(distance), at most n: two positions of a line are always less than n apart
inline int64_t find_peaks_d(double distance, int64_t n) {
  const double c = std::ceil(distance);
  return c >= (double)n ? n : (int64_t)c;
}

// the argument errors that need neither the tensor nor a context; nullptr when all is well.  wlen: ceil of the caller's value, or -1
// when none was given.  msg: room for the one message that carries a number
inline const char* find_peaks_check(uint32_t conditions, const double* bounds, double distance, int64_t wlen, double rel_height, uint32_t want,
                                    int64_t capacity, int64_t most, char* msg, size_t msg_len) {
  if (conditions & ~kFpConditionMask) return "unknown bits in conditions";
  if (want & ~kFpWantMask) return "unknown bits in want";
  if ((conditions & (kFpConditionMask & ~kFpDistance)) && !bounds) return "null pointer argument";
  if (bounds)
    for (int k = 0; k < 2 * kFpBounds; ++k)
      if (bounds[k] != bounds[k]) return "a border is not a number";
  if ((conditions & kFpDistance) && !(distance >= 1.0)) return "`distance` must be greater or equal to 1";
  if (wlen != -1 && wlen < 2) {
    std::snprintf(msg, msg_len, "`wlen` must be larger than 1, was %lld", (long long)wlen);
    return msg;
  }
  if (!(rel_height >= 0.0)) return "`rel_height` must be greater or equal to 0.0";
  if (capacity < 0 || capacity > most) return "capacity must be in [0, lines * ((n - 1) / 2)]";
  return nullptr;
}

// one side of a condition: open when the border is the infinity of that side
NXSIG_FP_HD bool fp_within(double p, double lo, double hi) {
  if (lo != -INFINITY && !(lo <= p)) return false;
  if (hi != INFINITY && !(p <= hi)) return false;
  return true;
}

// ---- a line of the [outer][n][inner] view and its summary: element i at x[i * st], block b at smin / smax[b * sst], super-block s (the
// kFindPeaksFan blocks from s * kFindPeaksFan on) at tmin / tmax[s * sst].  An entry over a NaN holds NaN in both, which fails every
// skip test below, so such a stretch is always walked one level down
template <typename T>
struct FpLine {
  const T* x;
  int64_t st, n;
  const T* smin;
  const T* smax;
  const T* tmin;
  const T* tmax;
  int64_t sst;
  NXSIG_FP_HD T at(int64_t i) const { return x[i * st]; }
  NXSIG_FP_HD T bmin(int64_t b) const { return smin[b * sst]; }
  NXSIG_FP_HD T bmax(int64_t b) const { return smax[b * sst]; }
  NXSIG_FP_HD T smin2(int64_t s) const { return tmin[s * sst]; }
  NXSIG_FP_HD T smax2(int64_t s) const { return tmax[s * sst]; }
  NXSIG_FP_HD int64_t block_end(int64_t i) const { return (i + kFindPeaksBlock < n ? i + kFindPeaksBlock : n) - 1; }   // i a block's start
  NXSIG_FP_HD int64_t super_end(int64_t i) const { return (i + kFindPeaksSuper < n ? i + kFindPeaksSuper : n) - 1; }   // i a super-block's start
};

// min and max of super-block s from the first level (st: the stride of the first level's entries), NaN in both when an entry is NaN
template <typename T>
NXSIG_FP_HD void fp_super_summary(const T* smin, const T* smax, int64_t st, int64_t nblk, int64_t s, T* mn, T* mx) {
  const int64_t b0 = s * kFindPeaksFan, b1 = b0 + kFindPeaksFan < nblk ? b0 + kFindPeaksFan : nblk;
  T lo = smin[b0 * st], hi = smax[b0 * st];
  bool nan = lo != lo;
  for (int64_t b = b0 + 1; b < b1; ++b) {
    const T l = smin[b * st], h = smax[b * st];
    nan = nan || l != l;
    lo = l < lo ? l : lo;
    hi = h > hi ? h : hi;
  }
  *mn = nan ? (T)NAN : lo;
  *mx = nan ? (T)NAN : hi;
}

// min and max of block b of a line, written the way every producer of the summary must: NaN in both when the block holds one
template <typename T>
NXSIG_FP_HD void fp_block_summary(const T* x, int64_t st, int64_t n, int64_t b, T* mn, T* mx) {
  const int64_t q0 = b * kFindPeaksBlock, q1 = q0 + kFindPeaksBlock < n ? q0 + kFindPeaksBlock : n;
  T lo = x[q0 * st], hi = lo;
  bool nan = lo != lo;
  for (int64_t q = q0 + 1; q < q1; ++q) {
    const T v = x[q * st];
    nan = nan || v != v;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  *mn = nan ? (T)NAN : lo;
  *mx = nan ? (T)NAN : hi;
}

// rule 1: the first j > i with x[j] != x[i], or n - 1.  TAB: whole blocks of the value are crossed in one step
template <typename T, bool TAB>
NXSIG_FP_HD int64_t fp_plateau_end(const FpLine<T>& L, int64_t i, T v) {
  const int64_t last = L.n - 1;
  int64_t j = i + 1;
  while (j < last) {
    if (TAB && (j & (kFindPeaksSuper - 1)) == 0 && j + kFindPeaksSuper <= last) {
      const int64_t s = j / kFindPeaksSuper;
      if (L.smin2(s) == v && L.smax2(s) == v) {
        j += kFindPeaksSuper;
        continue;
      }
    }
    if (TAB && (j & (kFindPeaksBlock - 1)) == 0 && j + kFindPeaksBlock <= last) {
      const int64_t b = j / kFindPeaksBlock;
      if (L.bmin(b) == v && L.bmax(b) == v) {
        j += kFindPeaksBlock;
        continue;
      }
    }
    if (!(L.at(j) == v)) break;
    ++j;
  }
  return j;
}

// the left edge of the plateau whose middle is the peak p (a sample below v lies left of it, so the walk ends above 0)
template <typename T, bool TAB>
NXSIG_FP_HD int64_t fp_plateau_start(const FpLine<T>& L, int64_t p, T v) {
  int64_t j = p;
  while (j > 0) {
    if (TAB && (j & (kFindPeaksSuper - 1)) == 0) {
      const int64_t s = j / kFindPeaksSuper - 1;
      if (L.smin2(s) == v && L.smax2(s) == v) {
        j -= kFindPeaksSuper;
        continue;
      }
    }
    if (TAB && (j & (kFindPeaksBlock - 1)) == 0) {
      const int64_t b = j / kFindPeaksBlock - 1;
      if (L.bmin(b) == v && L.bmax(b) == v) {
        j -= kFindPeaksBlock;
        continue;
      }
    }
    if (!(L.at(j - 1) == v)) break;
    --j;
  }
  return j;
}

// is a peak's plateau starting at i (1 <= i <= n - 2)?  *right: its right edge
template <typename T, bool TAB>
NXSIG_FP_HD bool fp_peak_at(const FpLine<T>& L, int64_t i, int64_t* right) {
  const T v = L.at(i);
  if (!(L.at(i - 1) < v)) return false;
  const int64_t j = fp_plateau_end<T, TAB>(L, i, v);
  if (!(L.at(j) < v)) return false;
  *right = j - 1;
  return true;
}

struct FpProminence {
  double prominence;
  int64_t left_base, right_base;
};

// rule 4.  half: wlen // 2, or -1 for the whole line.  TAB: a block or super-block inside the window whose max is <= x[p] gives its min
// in one step; when the side's minimum came out of one, that one stretch is scanned again for the position nearest to the peak
template <typename T, bool TAB>
NXSIG_FP_HD FpProminence fp_prominence(const FpLine<T>& L, int64_t p, int64_t half) {
  constexpr int64_t B = kFindPeaksBlock;
  const T v = L.at(p);
  int64_t i_min = 0, i_max = L.n - 1;
  if (half >= 0) {
    i_min = p - half > 0 ? p - half : 0;
    i_max = p + half < L.n - 1 ? p + half : L.n - 1;
  }
  FpProminence r;
  T lmin = v, rmin = v;
  constexpr int64_t S = kFindPeaksSuper;
  // where a side's minimum so far came from: an element (pos), a block (blk >= 0) or a super-block (sup >= 0)
  int64_t pos = p, blk = -1, sup = -1, i = p;
  while (i >= i_min) {
    if (TAB && (i & (S - 1)) == S - 1 && i - (S - 1) >= i_min) {
      const int64_t s = i / S;
      if (L.smax2(s) <= v) {
        const T sm = L.smin2(s);
        if (sm < lmin) {
          lmin = sm;
          sup = s;
          blk = -1;
        }
        i -= S;
        continue;
      }
    }
    if (TAB && (i & (B - 1)) == B - 1 && i - (B - 1) >= i_min) {
      const int64_t b = i / B;
      if (L.bmax(b) <= v) {
        const T bm = L.bmin(b);
        if (bm < lmin) {
          lmin = bm;
          blk = b;
          sup = -1;
        }
        i -= B;
        continue;
      }
    }
    const T xi = L.at(i);
    if (!(xi <= v)) break;
    if (xi < lmin) {
      lmin = xi;
      pos = i;
      blk = sup = -1;
    }
    --i;
  }
  if (sup >= 0)   // the block of the super-block nearest to the peak that holds the minimum
    for (blk = sup * kFindPeaksFan + kFindPeaksFan - 1; !(L.bmin(blk) == lmin); --blk) {
    }
  if (blk >= 0)
    for (int64_t q = blk * B + B - 1;; --q)
      if (L.at(q) == lmin) {
        pos = q;
        lmin = L.at(q);
        break;
      }
  r.left_base = pos;
  pos = p;
  blk = sup = -1;
  i = p;
  while (i <= i_max) {
    if (TAB && (i & (S - 1)) == 0 && L.super_end(i) <= i_max) {
      const int64_t s = i / S;
      if (L.smax2(s) <= v) {
        const T sm = L.smin2(s);
        if (sm < rmin) {
          rmin = sm;
          sup = s;
          blk = -1;
        }
        i = L.super_end(i) + 1;
        continue;
      }
    }
    if (TAB && (i & (B - 1)) == 0 && L.block_end(i) <= i_max) {
      const int64_t b = i / B;
      if (L.bmax(b) <= v) {
        const T bm = L.bmin(b);
        if (bm < rmin) {
          rmin = bm;
          blk = b;
          sup = -1;
        }
        i = L.block_end(i) + 1;
        continue;
      }
    }
    const T xi = L.at(i);
    if (!(xi <= v)) break;
    if (xi < rmin) {
      rmin = xi;
      pos = i;
      blk = sup = -1;
    }
    ++i;
  }
  if (sup >= 0)
    for (blk = sup * kFindPeaksFan; !(L.bmin(blk) == rmin); ++blk) {
    }
  if (blk >= 0)
    for (int64_t q = blk * B;; ++q)
      if (L.at(q) == rmin) {
        pos = q;
        rmin = L.at(q);
        break;
      }
  r.right_base = pos;
  const double lm = (double)lmin, rm = (double)rmin;
  r.prominence = (double)v - (lm > rm ? lm : rm);
  return r;
}

struct FpWidth {
  double width, width_height, left_ip, right_ip;
};

// rule 5, in double on the widened samples.  No product here may be fused into the sum after it: contraction is off inside the
// function (a pragma of the including file that comes after this header would not reach it), and host builds pass -ffp-contract=off.  TAB: a block strictly inside (base, p) whose min is above h is crossed in one step
template <typename T, bool TAB>
NXSIG_FP_HD FpWidth fp_width(const FpLine<T>& L, int64_t p, const FpProminence& pr, double rel_height) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int64_t B = kFindPeaksBlock, S = kFindPeaksSuper;
  FpWidth w;
  const double scaled = pr.prominence * rel_height;
  const double h = (double)L.at(p) - scaled;
  w.width_height = h;
  int64_t i = p;
  while (pr.left_base < i && h < (double)L.at(i)) {
    if (TAB && (i & (S - 1)) == S - 1 && i - (S - 1) > pr.left_base && h < (double)L.smin2(i / S)) {
      i -= S;
      continue;
    }
    if (TAB && (i & (B - 1)) == B - 1 && i - (B - 1) > pr.left_base && h < (double)L.bmin(i / B)) {
      i -= B;
      continue;
    }
    --i;
  }
  double ip = (double)i;
  double xi = (double)L.at(i);
  if (xi < h) {
    const double num = h - xi, den = (double)L.at(i + 1) - xi;
    ip += num / den;
  }
  w.left_ip = ip;
  i = p;
  while (i < pr.right_base && h < (double)L.at(i)) {
    if (TAB && (i & (S - 1)) == 0 && L.super_end(i) < pr.right_base && h < (double)L.smin2(i / S)) {
      i = L.super_end(i) + 1;
      continue;
    }
    if (TAB && (i & (B - 1)) == 0 && L.block_end(i) < pr.right_base && h < (double)L.bmin(i / B)) {
      i = L.block_end(i) + 1;
      continue;
    }
    ++i;
  }
  ip = (double)i;
  xi = (double)L.at(i);
  if (xi < h) {
    const double num = h - xi, den = (double)L.at(i - 1) - xi;
    ip -= num / den;
  }
  w.right_ip = ip;
  w.width = w.right_ip - w.left_ip;
  return w;
}

// ---- rule 3.  The visiting order: higher first, among equal heights the larger index first — a total order
template <typename T>
NXSIG_FP_HD bool fp_precedes(T hq, int64_t q, T hp, int64_t p) {
  return hq > hp || (hq == hp && q > p);
}

// the sequential rule on one line: pos ascending, h the heights; keep[k] = 1 for the survivors
inline void find_peaks_distance_sequential(const double* h, const int64_t* pos, int64_t m, int64_t d, uint8_t* keep) {
  std::vector<int64_t> order(m);
  for (int64_t k = 0; k < m; ++k) order[k] = k;
  for (int64_t a = 1; a < m; ++a)   // insertion sort by the visiting order (the program's lines are short)
    for (int64_t b = a; b > 0 && fp_precedes(h[order[b]], pos[order[b]], h[order[b - 1]], pos[order[b - 1]]); --b) {
      const int64_t t = order[b];
      order[b] = order[b - 1];
      order[b - 1] = t;
    }
  for (int64_t k = 0; k < m; ++k) keep[k] = 1;
  for (int64_t a = 0; a < m; ++a) {
    const int64_t j = order[a];
    if (!keep[j]) continue;
    for (int64_t k = j - 1; k >= 0 && pos[j] - pos[k] < d; --k) keep[k] = 0;
    for (int64_t k = j + 1; k < m && pos[k] - pos[j] < d; ++k) keep[k] = 0;
  }
}

// the rounds the kernels play, on one line: in a round every candidate that is alive and not yet kept is kept when no alive candidate
// within d precedes it (all decisions of a round are taken on the state the round began with); then every kept candidate removes the
// alive ones within d.  Ends after the first round that left no candidate undecided; returns the number of rounds
inline int64_t find_peaks_distance_rounds(const double* h, const int64_t* pos, int64_t m, int64_t d, uint8_t* keep) {
  std::vector<uint8_t> alive(m, 1), kept(m, 0);
  int64_t rounds = 0;
  for (;;) {
    ++rounds;
    bool undecided = false;
    std::vector<uint8_t> now(kept);
    for (int64_t j = 0; j < m; ++j) {
      if (!alive[j] || kept[j]) continue;
      bool first = true;
      for (int64_t k = j - 1; first && k >= 0 && pos[j] - pos[k] < d; --k) first = !(alive[k] && fp_precedes(h[k], pos[k], h[j], pos[j]));
      for (int64_t k = j + 1; first && k < m && pos[k] - pos[j] < d; ++k) first = !(alive[k] && fp_precedes(h[k], pos[k], h[j], pos[j]));
      if (first) now[j] = 1;
      else undecided = true;
    }
    kept = now;
    for (int64_t j = 0; j < m; ++j) {
      if (!kept[j]) continue;
      for (int64_t k = j - 1; k >= 0 && pos[j] - pos[k] < d; --k) alive[k] = 0;
      for (int64_t k = j + 1; k < m && pos[k] - pos[j] < d; ++k) alive[k] = 0;
    }
    if (!undecided) break;
  }
  for (int64_t j = 0; j < m; ++j) keep[j] = alive[j];
  return rounds;
}

}  // namespace nxsig
