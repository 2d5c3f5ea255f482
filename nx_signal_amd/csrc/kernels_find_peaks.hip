// PeakFinding.find_peaks: scipy.signal.find_peaks 1.15 on every line of an n-D tensor along one axis (DESIGN.md section 3.14;
// include/nxsig.h states the rules).  The tensor is viewed as [outer][n][inner]; a line is one (outer, inner) pair.
//
// The survivors are a bit mask over the flat tensor, one bit at each peak's own position, so the compaction is in row-major order:
//   summary   (find_peaks.tables only) min and max of every block of kFindPeaksBlock axis positions of every line: the streaming pass;
//             then of every super-block of kFindPeaksFan blocks, from the first level
//   mark      an element that starts a plateau (x[i - 1] < x[i]) walks to its end; a peak that passes plateau_size, height and threshold
//             sets the bit of its middle sample (a wave ors its own lanes' bits in as one word; a middle elsewhere is or'ed in alone)
//   distance  rounds of two launches over the mask (keep: an undecided peak with no alive peak within d ahead of it in the visiting
//             order is kept; remove: every kept peak clears the alive bits within d); the host reads a flag after each round.  Axis
//             last: the bits of a line are consecutive, so both work on whole mask words; any other axis: position by position
//   filter    prominence / width conditions on what is left, one wave per mask word
//   count, scan, place   tile counts, their exclusive offsets and the total (valid), the flat position of every survivor below capacity
//   properties           one thread per output row: coordinates and the requested properties, or -1 / NaN at and past valid
// The only atomics are integer or / and on mask words, whose result does not depend on their order; the walks are those of
// find_peaks_plan.hpp, with the summary (find_peaks.tables) or element by element (find_peaks.generic, NXSIG_DISABLE_FIND_PEAKS_TABLES).
// No FMA contraction anywhere in this file: SciPy's compiled code rounds the product in the width height on its own.
#pragma clang fp contract(off)

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kThreads = 256, kItems = 16, kTile = kThreads * kItems;   // the tile of kernels_peaks.hip: 4096 flat elements, 64 mask words
constexpr int kB = kFindPeaksBlock;
typedef unsigned long long u64;

struct Geom {
  uint64_t total, nwords;   // elements (< 2^32), mask words
  uint32_t n, inner, nblk, nsup;   // axis length, elements after the axis, summary blocks and super-blocks per line
  uint32_t conditions;
  double lo[kFpBounds], hi[kFpBounds];
  int64_t d;                // distance in samples, 1 .. n
  int64_t half;             // wlen // 2, or -1: the whole line
  double rel_height;
};

// the two levels of the line summary, [outer][block][inner] and [outer][super-block][inner]; all null on find_peaks.generic
template <typename T>
struct Summary {
  T *smin, *smax, *tmin, *tmax;
};

// the line of flat element e at axis coordinate i
template <typename T>
__device__ __forceinline__ FpLine<T> line_of(const T* __restrict__ x, const Summary<T>& M, const Geom& G, uint64_t e, int64_t i) {
  FpLine<T> L;
  L.x = x + (e - (uint64_t)i * G.inner);
  L.st = G.inner;
  L.n = G.n;
  const uint64_t c = e % G.inner, o = e / ((uint64_t)G.inner * G.n);
  L.smin = M.smin ? M.smin + (o * G.nblk * G.inner + c) : nullptr;
  L.smax = M.smin ? M.smax + (o * G.nblk * G.inner + c) : nullptr;
  L.tmin = M.smin ? M.tmin + (o * G.nsup * G.inner + c) : nullptr;
  L.tmax = M.smin ? M.tmax + (o * G.nsup * G.inner + c) : nullptr;
  L.sst = G.inner;
  return L;
}

__device__ __forceinline__ bool bit_of(const u64* __restrict__ words, uint64_t e) { return (words[e >> 6] >> (e & 63)) & 1; }

// ---- summary, axis last: a 16-lane group per block, four elements per lane (16-byte loads where the address allows)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp_summary_rows(const T* __restrict__ x, T* __restrict__ smin, T* __restrict__ smax, uint64_t jobs,
                                                              uint32_t n, uint32_t nblk) {
  const int sub = threadIdx.x & 15;
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 16);
  const uint64_t rounds = (jobs + step - 1) / step;   // every lane of a wave makes the same number of trips: the shuffles below see whole groups
  uint64_t job = (uint64_t)blockIdx.x * (kThreads / 16) + (threadIdx.x >> 4);
  for (uint64_t t = 0; t < rounds; ++t, job += step) {
    const bool live = job < jobs;
    const uint64_t line = live ? job / nblk : 0, b = live ? job % nblk : 0;
    const uint64_t q0 = b * kB + sub * 4;   // first axis position of this lane
    const T* src = x + line * n + q0;
    T v[4];
    int have = 0;
    if (live && q0 < n) have = n - q0 < 4 ? (int)(n - q0) : 4;
    if (have == 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      if constexpr (sizeof(T) == 4) {
        const float4 f = *reinterpret_cast<const float4*>(src);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {
        const double2 a = *reinterpret_cast<const double2*>(src), c = *reinterpret_cast<const double2*>(src + 2);
        v[0] = a.x; v[1] = a.y; v[2] = c.x; v[3] = c.y;
      }
    } else {
      for (int k = 0; k < have; ++k) v[k] = src[k];
    }
    // sub 0 always holds an element of a live block
    T lo = have ? v[0] : (T)INFINITY, hi = have ? v[0] : (T)-INFINITY;
    int nan = 0;
    for (int k = 0; k < have; ++k) {
      nan |= v[k] != v[k];
      lo = v[k] < lo ? v[k] : lo;
      hi = v[k] > hi ? v[k] : hi;
    }
    for (int m = 1; m < 16; m <<= 1) {
      const T ol = __shfl_xor(lo, m, 16), oh = __shfl_xor(hi, m, 16);
      nan |= __shfl_xor(nan, m, 16);
      lo = ol < lo ? ol : lo;
      hi = oh > hi ? oh : hi;
    }
    if (live && sub == 0) {
      smin[job] = nan ? (T)NAN : lo;
      smax[job] = nan ? (T)NAN : hi;
    }
  }
}

// ---- summary, any other axis: a thread per (outer, block, inner), neighbours in a wave read neighbouring addresses
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp_summary_strided(const T* __restrict__ x, T* __restrict__ smin, T* __restrict__ smax, uint64_t jobs,
                                                                 uint32_t n, uint32_t inner, uint32_t nblk) {
  for (uint64_t id = (uint64_t)blockIdx.x * kThreads + threadIdx.x; id < jobs; id += (uint64_t)gridDim.x * kThreads) {
    const uint64_t c = id % inner, rest = id / inner, b = rest % nblk, o = rest / nblk;
    T lo, hi;
    fp_block_summary<T>(x + (o * n) * inner + c, inner, n, (int64_t)b, &lo, &hi);
    smin[id] = lo;
    smax[id] = hi;
  }
}

// ---- the second level from the first: a thread per (outer, super-block, inner)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fp_summary_super(Summary<T> M, uint64_t jobs, uint32_t inner, uint32_t nblk, uint32_t nsup) {
  for (uint64_t id = (uint64_t)blockIdx.x * kThreads + threadIdx.x; id < jobs; id += (uint64_t)gridDim.x * kThreads) {
    const uint64_t c = id % inner, rest = id / inner, sb = rest % nsup, o = rest / nsup;
    const uint64_t base = o * nblk * inner + c;
    T lo, hi;
    fp_super_summary<T>(M.smin + base, M.smax + base, inner, nblk, (int64_t)sb, &lo, &hi);
    M.tmin[id] = lo;
    M.tmax[id] = hi;
  }
}

// ---- mark: rule 1 and the conditions ahead of the distance
template <typename T, bool TAB>
__global__ __launch_bounds__(kThreads) void k_fp_mark(const T* __restrict__ x, Summary<T> M, Geom G, u64* __restrict__ words) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTile;
  for (int j = 0; j < kItems; ++j) {
    const uint64_t e = b0 + j * kThreads + tid;
    bool own = false;   // a peak whose middle is this very element
    if (e < G.total) {
      const int64_t i = (int64_t)(e / G.inner % G.n);
      if (i >= 1 && i <= (int64_t)G.n - 2) {
        const FpLine<T> L = line_of<T>(x, M, G, e, i);
        int64_t right;
        if (fp_peak_at<T, TAB>(L, i, &right)) {
          const int64_t p = (i + right) / 2;
          bool keep = true;
          if (G.conditions & kFpPlateauSize) keep = fp_within((double)(right - i + 1), G.lo[kFpBoundPlateau], G.hi[kFpBoundPlateau]);
          if (keep && (G.conditions & kFpHeight)) keep = fp_within((double)L.at(p), G.lo[kFpBoundHeight], G.hi[kFpBoundHeight]);
          if (keep && (G.conditions & kFpThreshold)) {
            const double v = (double)L.at(p), l = v - (double)L.at(p - 1), r = v - (double)L.at(p + 1);
            const double mn = l < r ? l : r, mx = l > r ? l : r;
            keep = fp_within(mn, G.lo[kFpBoundThreshold], INFINITY) && fp_within(mx, -INFINITY, G.hi[kFpBoundThreshold]);
          }
          if (keep) {
            if (p == i) {
              own = true;
            } else {
              const uint64_t f = e + (uint64_t)(p - i) * G.inner;
              atomicOr(&words[f >> 6], (u64)1 << (f & 63));
            }
          }
        }
      }
    }
    const u64 bal = __ballot(own);
    const uint64_t w = (b0 + j * kThreads) / 64 + wave;
    if (lane == 0 && bal && w < G.nwords) atomicOr(&words[w], bal);
  }
}

// ---- distance, first half of a round: alive and not kept, and nobody alive within d comes ahead of it -> kept.  Nearest first: on
// noise-like data the walk ends at the first higher neighbour
// the mask word w cut to the flat range [lo, hi] of a line (axis last: the bits of a line are consecutive), without the bit of e
__device__ __forceinline__ u64 window_bits(uint64_t w, uint64_t lo, uint64_t hi, uint64_t e) {
  u64 m = ~0ull;
  if (w == lo >> 6) m &= ~0ull << (lo & 63);
  if (w == hi >> 6) m &= ~0ull >> (63 - (hi & 63));
  if (w == e >> 6) m &= ~((u64)1 << (e & 63));
  return m;
}

template <typename T, bool ROWS>
__global__ __launch_bounds__(kThreads) void k_fp_keep(const T* __restrict__ x, Geom G, const u64* __restrict__ alive, u64* __restrict__ kept,
                                                      uint32_t* __restrict__ flag) {
  for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < G.total; e += (uint64_t)gridDim.x * kThreads) {
    if (!bit_of(alive, e) || bit_of(kept, e)) continue;
    const int64_t i = (int64_t)(e / G.inner % G.n), n = G.n;
    const T v = x[e];
    const int64_t reach = i > n - 1 - i ? i : n - 1 - i;
    bool first = true;
    if constexpr (ROWS) {   // axis last: whole mask words, from the peak's own outwards; only alive neighbours are loaded
      const uint64_t lo = e - (uint64_t)(i < G.d - 1 ? i : G.d - 1), hi = e + (uint64_t)(n - 1 - i < G.d - 1 ? n - 1 - i : G.d - 1);
      const uint64_t w0 = e >> 6, wl = lo >> 6, wh = hi >> 6;
      for (uint64_t k = 0; first && (w0 >= wl + k || w0 + k <= wh); ++k) {
        for (int up = 0; up < 2 && first; ++up) {
          if (up ? (k == 0 || w0 + k > wh) : w0 < wl + k) continue;
          const uint64_t w = up ? w0 + k : w0 - k;
          u64 m = alive[w] & window_bits(w, lo, hi, e);
          while (m && first) {
            const uint64_t q = (w << 6) + (uint64_t)(__ffsll(m) - 1);
            m &= m - 1;
            const T xq = x[q];
            if (q < e ? xq > v : xq >= v) first = false;
          }
        }
      }
      if (first) atomicOr(&kept[e >> 6], (u64)1 << (e & 63));
      else *flag = 1;
      continue;
    }
    for (int64_t k = 1; k < G.d && k <= reach && first; ++k) {
      if (i - k >= 0) {
        const uint64_t q = e - (uint64_t)k * G.inner;
        if (bit_of(alive, q) && x[q] > v) first = false;   // a lower index comes ahead only when it is higher
      }
      if (i + k <= n - 1) {
        const uint64_t q = e + (uint64_t)k * G.inner;
        if (bit_of(alive, q) && x[q] >= v) first = false;  // a larger index comes ahead when it is as high
      }
    }
    if (first) atomicOr(&kept[e >> 6], (u64)1 << (e & 63));
    else *flag = 1;
  }
}

// ---- distance, second half: every kept peak clears the alive bits within d (again in later rounds, which changes nothing)
template <bool ROWS>
__global__ __launch_bounds__(kThreads) void k_fp_remove(Geom G, u64* __restrict__ alive, const u64* __restrict__ kept) {
  for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < G.total; e += (uint64_t)gridDim.x * kThreads) {
    if (!bit_of(kept, e)) continue;
    const int64_t i = (int64_t)(e / G.inner % G.n), n = G.n;
    if constexpr (ROWS) {
      const uint64_t lo = e - (uint64_t)(i < G.d - 1 ? i : G.d - 1), hi = e + (uint64_t)(n - 1 - i < G.d - 1 ? n - 1 - i : G.d - 1);
      for (uint64_t w = lo >> 6; w <= hi >> 6; ++w) {
        const u64 m = window_bits(w, lo, hi, e);
        if (alive[w] & m) atomicAnd(&alive[w], ~m);
      }
      continue;
    }
    const int64_t reach = i > n - 1 - i ? i : n - 1 - i;
    for (int64_t k = 1; k < G.d && k <= reach; ++k) {
      if (i - k >= 0) {
        const uint64_t q = e - (uint64_t)k * G.inner;
        if (bit_of(alive, q)) atomicAnd(&alive[q >> 6], ~((u64)1 << (q & 63)));
      }
      if (i + k <= n - 1) {
        const uint64_t q = e + (uint64_t)k * G.inner;
        if (bit_of(alive, q)) atomicAnd(&alive[q >> 6], ~((u64)1 << (q & 63)));
      }
    }
  }
}

// ---- the conditions after the distance: prominence, width.  A wave owns a mask word
template <typename T, bool TAB>
__global__ __launch_bounds__(kThreads) void k_fp_filter(const T* __restrict__ x, Summary<T> M, Geom G, u64* __restrict__ words) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTile;
  for (int j = 0; j < kItems; ++j) {
    const uint64_t e = b0 + j * kThreads + tid, w = (b0 + j * kThreads) / 64 + wave;
    const u64 word = w < G.nwords ? words[w] : 0;
    if (!word) continue;   // wave-uniform
    bool keep = (word >> lane) & 1;
    if (keep) {
      const int64_t p = (int64_t)(e / G.inner % G.n);
      const FpLine<T> L = line_of<T>(x, M, G, e, p);
      const FpProminence pr = fp_prominence<T, TAB>(L, p, G.half);
      if (G.conditions & kFpProminence) keep = fp_within(pr.prominence, G.lo[kFpBoundProminence], G.hi[kFpBoundProminence]);
      if (keep && (G.conditions & kFpWidth))
        keep = fp_within(fp_width<T, TAB>(L, p, pr, G.rel_height).width, G.lo[kFpBoundWidth], G.hi[kFpBoundWidth]);
    }
    const u64 bal = __ballot(keep);
    if (lane == 0) words[w] = bal;
  }
}

// ---- compaction: marks per tile, the scan of kernels_peaks.hip, the survivors' flat positions
__global__ __launch_bounds__(64) void k_fp_count(const u64* __restrict__ words, uint64_t nwords, uint32_t* __restrict__ counts) {
  const uint64_t w = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  uint32_t c = w < nwords ? (uint32_t)__popcll(words[w]) : 0;
  for (int m = 32; m; m >>= 1) c += __shfl_xor(c, m, 64);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(1024) void k_fp_scan(const uint32_t* __restrict__ counts, uint64_t ntiles, uint64_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ valid) {
  __shared__ uint64_t part[1024];
  const int tid = threadIdx.x;
  const uint64_t run = (ntiles + 1023) / 1024, q0 = tid * run < ntiles ? tid * run : ntiles, q1 = q0 + run < ntiles ? q0 + run : ntiles;
  uint64_t s = 0;
  for (uint64_t q = q0; q < q1; ++q) s += counts[q];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  uint64_t off = part[tid] - s;
  for (uint64_t q = q0; q < q1; ++q) {
    offsets[q] = off;
    off += counts[q];
  }
  if (tid == 1023) *valid = (uint32_t)part[1023];
}

__global__ __launch_bounds__(kThreads) void k_fp_place(const u64* __restrict__ words, const uint64_t* __restrict__ offsets, uint64_t nwords,
                                                       uint64_t capacity, uint32_t* __restrict__ pos) {
  __shared__ u64 bits[kTile / 64];
  __shared__ uint32_t before[kTile / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTile, w0 = b0 / 64;
  if (tid < kTile / 64) {
    const u64 b = w0 + tid < nwords ? words[w0 + tid] : 0;
    bits[tid] = b;
    uint32_t inc = (uint32_t)__popcll(b);
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    before[tid] = inc - (uint32_t)__popcll(b);
  }
  __syncthreads();
  const uint64_t off = offsets[blockIdx.x];
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int j = 0; j < kItems; ++j) {
    const int wi = j * (kThreads / 64) + wave;
    const u64 b = bits[wi];
    if (!((b >> lane) & 1)) continue;
    const uint64_t slot = off + before[wi] + (uint64_t)__popcll(b & below);
    if (slot < capacity) pos[slot] = (uint32_t)(b0 + j * kThreads + tid);
  }
}

struct Out {
  uint64_t capacity;
  uint32_t dims[8];
  int32_t rank;
  uint32_t want;
  int32_t row[kFpProperties];   // row of fprops / iprops that holds the property, -1 when it is not wanted
  int32_t* indices;
  double* fprops;
  int32_t* iprops;
};

// ---- one thread per output row
template <typename T, bool TAB>
__global__ __launch_bounds__(kThreads) void k_fp_properties(const T* __restrict__ x, Summary<T> M, Geom G, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ valid, Out O) {
  const uint64_t v = *valid;
  for (uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x; s < O.capacity; s += (uint64_t)gridDim.x * kThreads) {
    int32_t* row = O.indices + s * O.rank;
    double f[kFpF64Properties];
    int32_t q[kFpS32Properties];
    for (int k = 0; k < kFpF64Properties; ++k) f[k] = NAN;
    for (int k = 0; k < kFpS32Properties; ++k) q[k] = -1;
    if (s < v) {
      const uint64_t e = pos[s];
      uint32_t r = (uint32_t)e;
      for (int d = O.rank - 1; d >= 0; --d) {
        row[d] = (int32_t)(r % O.dims[d]);
        r /= O.dims[d];
      }
      const int64_t p = (int64_t)(e / G.inner % G.n);
      const FpLine<T> L = line_of<T>(x, M, G, e, p);
      const double h = (double)L.at(p);
      f[kFpPeakHeights] = h;
      f[kFpLeftThresholds] = h - (double)L.at(p - 1);
      f[kFpRightThresholds] = h - (double)L.at(p + 1);
      if (O.want & ((1u << kFpProminences) | (1u << kFpLeftBases) | (1u << kFpRightBases) | (1u << kFpWidthHeights) | (1u << kFpLeftIps) |
                    (1u << kFpRightIps) | (1u << kFpWidths))) {
        const FpProminence pr = fp_prominence<T, TAB>(L, p, G.half);
        f[kFpProminences] = pr.prominence;
        q[kFpLeftBases - kFpF64Properties] = (int32_t)pr.left_base;
        q[kFpRightBases - kFpF64Properties] = (int32_t)pr.right_base;
        if (O.want & ((1u << kFpWidthHeights) | (1u << kFpLeftIps) | (1u << kFpRightIps) | (1u << kFpWidths))) {
          const FpWidth w = fp_width<T, TAB>(L, p, pr, G.rel_height);
          f[kFpWidthHeights] = w.width_height;
          f[kFpLeftIps] = w.left_ip;
          f[kFpRightIps] = w.right_ip;
          f[kFpWidths] = w.width;
        }
      }
      if (O.want & ((1u << kFpLeftEdges) | (1u << kFpRightEdges) | (1u << kFpPlateauSizes))) {
        const T pv = L.at(p);
        const int64_t le = fp_plateau_start<T, TAB>(L, p, pv), re = fp_plateau_end<T, TAB>(L, p, pv) - 1;
        q[kFpLeftEdges - kFpF64Properties] = (int32_t)le;
        q[kFpRightEdges - kFpF64Properties] = (int32_t)re;
        q[kFpPlateauSizes - kFpF64Properties] = (int32_t)(re - le + 1);
      }
    } else {
      for (int d = 0; d < O.rank; ++d) row[d] = -1;
    }
    for (int k = 0; k < kFpF64Properties; ++k)
      if (O.row[k] >= 0) O.fprops[(uint64_t)O.row[k] * O.capacity + s] = f[k];
    for (int k = 0; k < kFpS32Properties; ++k)
      if (O.row[kFpF64Properties + k] >= 0) O.iprops[(uint64_t)O.row[kFpF64Properties + k] * O.capacity + s] = q[k];
  }
}

thread_local int32_t g_last_rounds = 0;

unsigned grid_for(const Ctx* c, uint64_t work) {
  const uint64_t want = (work + kThreads - 1) / kThreads, most = (uint64_t)c->num_cus * 32;
  return (unsigned)(want < most ? (want ? want : 1) : most);
}

template <typename T, bool TAB>
int run(Ctx* c, const FindPeaksLaunch& a, const Geom& G, const Out& O0) {
  const T* x = static_cast<const T*>(a.x);
  const uint64_t ntiles = (G.total + kTile - 1) / kTile, lines = G.total / G.n, nsum = lines * G.nblk, nsum2 = lines * G.nsup;
  // kScratchPeakTiles: alive words, kept words, tile offsets, tile counts, the flag of the distance rounds
  void* sc = nullptr;
  int rc = ctx_scratch(c, kScratchPeakTiles, (size_t)(G.nwords * 16 + ntiles * 12 + 16), &sc);
  if (rc) return rc;
  u64* words = static_cast<u64*>(sc);
  u64* kept = words + G.nwords;
  uint64_t* offsets = reinterpret_cast<uint64_t*>(kept + G.nwords);
  uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + ntiles);
  uint32_t* flag = counts + ntiles;
  // kScratchPeakExtremes: the summary, the survivors' positions, the s32 properties of a host call
  const size_t sum1 = TAB ? ((size_t)nsum * sizeof(T) + 15) & ~(size_t)15 : 0, sum2 = TAB ? ((size_t)nsum2 * sizeof(T) + 15) & ~(size_t)15 : 0;
  const size_t sum_bytes = sum1 + sum2;
  const size_t pos_bytes = ((size_t)a.capacity * 4 + 15) & ~(size_t)15;
  const size_t ip_bytes = a.iprops ? 0 : (size_t)a.capacity * 4 * find_peaks_s32_rows(a.want);
  if ((rc = ctx_scratch(c, kScratchPeakExtremes, 2 * sum_bytes + pos_bytes + ip_bytes + 16, &sc))) return rc;
  unsigned char* base = static_cast<unsigned char*>(sc);
  Summary<T> M{nullptr, nullptr, nullptr, nullptr};
  if (TAB) {
    M.smin = reinterpret_cast<T*>(base);
    M.tmin = reinterpret_cast<T*>(base + sum1);
    M.smax = reinterpret_cast<T*>(base + sum_bytes);
    M.tmax = reinterpret_cast<T*>(base + sum_bytes + sum1);
  }
  uint32_t* pos = reinterpret_cast<uint32_t*>(base + 2 * sum_bytes);
  Out O = O0;
  if (!O.iprops) O.iprops = reinterpret_cast<int32_t*>(base + 2 * sum_bytes + pos_bytes);
  if (a.iprops_used) *a.iprops_used = O.iprops;

  NXSIG_HIP_TRY(hipMemsetAsync(words, 0, (size_t)G.nwords * 16, c->stream));
  if (TAB) {
    if (G.inner == 1) {
      const uint64_t groups = (nsum + 15) / 16, most = (uint64_t)c->num_cus * 32;
      hipLaunchKernelGGL((k_fp_summary_rows<T>), dim3((unsigned)(groups < most ? groups : most)), dim3(kThreads), 0, c->stream, x, M.smin, M.smax, nsum,
                         G.n, G.nblk);
    } else {
      hipLaunchKernelGGL((k_fp_summary_strided<T>), dim3(grid_for(c, nsum)), dim3(kThreads), 0, c->stream, x, M.smin, M.smax, nsum, G.n, G.inner,
                         G.nblk);
    }
    NXSIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_fp_summary_super<T>), dim3(grid_for(c, nsum2)), dim3(kThreads), 0, c->stream, M, nsum2, G.inner, G.nblk, G.nsup);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL((k_fp_mark<T, TAB>), dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, x, M, G, words);
  NXSIG_HIP_TRY(hipGetLastError());
  g_last_rounds = 0;
  if ((G.conditions & kFpDistance) && G.d > 1) {
    const unsigned grid = grid_for(c, G.total);
    for (;;) {
      uint32_t undecided = 0;
      NXSIG_HIP_TRY(hipMemsetAsync(flag, 0, 4, c->stream));
      if (G.inner == 1) hipLaunchKernelGGL((k_fp_keep<T, true>), dim3(grid), dim3(kThreads), 0, c->stream, x, G, (const u64*)words, kept, flag);
      else hipLaunchKernelGGL((k_fp_keep<T, false>), dim3(grid), dim3(kThreads), 0, c->stream, x, G, (const u64*)words, kept, flag);
      NXSIG_HIP_TRY(hipGetLastError());
      if (G.inner == 1) hipLaunchKernelGGL(k_fp_remove<true>, dim3(grid), dim3(kThreads), 0, c->stream, G, words, (const u64*)kept);
      else hipLaunchKernelGGL(k_fp_remove<false>, dim3(grid), dim3(kThreads), 0, c->stream, G, words, (const u64*)kept);
      NXSIG_HIP_TRY(hipGetLastError());
      NXSIG_HIP_TRY(hipMemcpyAsync(&undecided, flag, 4, hipMemcpyDeviceToHost, c->stream));
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      ++g_last_rounds;
      if (!undecided) break;
    }
  }
  if (G.conditions & (kFpProminence | kFpWidth)) {
    hipLaunchKernelGGL((k_fp_filter<T, TAB>), dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, x, M, G, words);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_fp_count, dim3((unsigned)ntiles), dim3(64), 0, c->stream, (const u64*)words, G.nwords, counts);
  NXSIG_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fp_scan, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)counts, ntiles, offsets, a.valid);
  NXSIG_HIP_TRY(hipGetLastError());
  if (a.capacity == 0) return NXSIG_OK;
  hipLaunchKernelGGL(k_fp_place, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, (const u64*)words, (const uint64_t*)offsets, G.nwords,
                     (uint64_t)a.capacity, pos);
  NXSIG_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((k_fp_properties<T, TAB>), dim3(grid_for(c, (uint64_t)a.capacity)), dim3(kThreads), 0, c->stream, x, M, G,
                     (const uint32_t*)pos, (const uint32_t*)a.valid, O);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace

int32_t find_peaks_last_rounds() { return g_last_rounds; }

int launch_find_peaks(Ctx* c, const FindPeaksLaunch& a) {
  Geom G{};
  G.total = 1;
  for (int d = 0; d < a.rank; ++d) G.total *= (uint64_t)a.shape[d];
  G.nwords = (G.total + 63) / 64;
  G.n = (uint32_t)a.shape[a.axis];
  G.inner = 1;
  for (int d = a.axis + 1; d < a.rank; ++d) G.inner *= (uint32_t)a.shape[d];
  G.nblk = (uint32_t)find_peaks_blocks(G.n);
  G.nsup = (uint32_t)find_peaks_supers(G.n);
  G.conditions = a.conditions;
  for (int k = 0; k < kFpBounds; ++k) {
    G.lo[k] = a.bounds ? a.bounds[2 * k] : -INFINITY;
    G.hi[k] = a.bounds ? a.bounds[2 * k + 1] : INFINITY;
  }
  G.d = (a.conditions & kFpDistance) ? find_peaks_d(a.distance, G.n) : 1;
  G.half = a.wlen >= 2 ? a.wlen / 2 : -1;
  G.rel_height = a.rel_height;
  Out O{};
  O.capacity = (uint64_t)a.capacity;
  O.rank = a.rank;
  for (int d = 0; d < a.rank; ++d) O.dims[d] = (uint32_t)a.shape[d];
  O.want = a.want;
  int nf = 0, ni = 0;
  for (int k = 0; k < kFpProperties; ++k) {
    O.row[k] = -1;
    if (a.want & (1u << k)) O.row[k] = k < kFpF64Properties ? nf++ : ni++;
  }
  O.indices = a.indices;
  O.fprops = a.fprops;
  O.iprops = a.iprops;
  const bool tab = tune(c, kT_DISABLE_FIND_PEAKS_TABLES, 0) == 0;
  dispatch_note(tab ? "find_peaks.tables" : "find_peaks.generic");
  if (a.f64) return tab ? run<double, true>(c, a, G, O) : run<double, false>(c, a, G, O);
  return tab ? run<float, true>(c, a, G, O) : run<float, false>(c, a, G, O);
}

}  // namespace nxsig
