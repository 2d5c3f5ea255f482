// NxSignal.PeakFinding.argrelmin/2, argrelmax/2, argrelextrema/3 (lib/nx_signal/peak_finding.ex): a neighbourhood compare along one
// axis of an n-D tensor, then an ordered stream compaction of the marked elements' coordinates.
//
// The tensor is viewed as [outer][n][inner] around the axis.  An element at axis coordinate i is marked when cmp(x[i], x[clip(i +- s)])
// holds for s = 1 .. shifts (shifts = 0 marks everything).  The clipped neighbours of i form two windows, [max(i - S, 0), i - 1] and
// [i + 1, min(i + S, n - 1)] (the element itself at the two ends of a line), so the test is also "x cmp extreme(window)" with a
// NaN-absorbing min (less, less_equal) or max (greater, greater_equal): a NaN anywhere in the window unmarks x, a NaN x is never marked.
//
// Three launches, no inter-workgroup communication inside any of them, no atomics:
//   mark    per tile of kTile flat elements: the mask as 64-bit ballot words (one wave owns a word) and the tile's mark count
//   scan    one workgroup: exclusive offsets of the tile counts (64-bit) and the total, which is valid_indices
//   write   per tile: coordinates of the marked elements at offset + (words before) + popcount(word & lanes below); the rows
//           [valid, size) of the tile's row range are filled with -1 in 16-byte stores
// Families of the mark launch (recorded by dispatch_note):
//   peaks.rows     axis is the last one: the tile and an S-element halo in LDS (16-byte loads); S <= kBruteMax compares each
//                  neighbour, larger S takes window extremes off an in-place doubling table (log2 S LDS passes, O(1) per query)
//   peaks.strided  any other axis: the neighbours of a tile are contiguous runs +-s*inner away (coalesced); larger S: van Herk /
//                  Gil-Werman block prefix / suffix extremes (one pre-pass, blocks of S along the axis) and two reads per window
//   peaks.generic  any axis, any order: each neighbour in turn, stopping at the first failed compare (the correctness path)
//   nonzero        the mark is a given u8 mask
#include <type_traits>

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kThreads = 256, kItems = 16, kTile = kThreads * kItems;   // 4096 flat elements, 64 mask words per tile
constexpr int kBruteMax = 8;                                             // shifts above this take window extremes
constexpr size_t kRowsLds = 64 * 1024 - 256;                             // dynamic LDS of peaks.rows (tile + halo)
enum { kLess = 0, kGreater = 1, kLessEq = 2, kGreaterEq = 3 };           // NXSIG_CMP_*
enum { kGeneric = 0, kStrided = 1, kRows = 2, kNonzero = 3 };

template <int C, typename T> __device__ __forceinline__ bool cmp(T a, T b) {
  if constexpr (C == kLess) return a < b;
  else if constexpr (C == kGreater) return a > b;
  else if constexpr (C == kLessEq) return a <= b;
  else return a >= b;
}

// the window extreme cmp is tested against; a NaN absorbs (cmp with it is false, as with every member of the window)
template <int C, typename T> __device__ __forceinline__ T ext(T a, T b) {
  if constexpr (std::is_floating_point<T>::value) {
    if (a != a) return a;
    if (b != b) return b;
  }
  if constexpr (C == kLess || C == kLessEq) return b < a ? b : a;
  else return b > a ? b : a;
}

struct Line {
  uint64_t total, nwords;   // elements (< 2^32), mask words
  uint32_t n, inner;        // axis length (< 2^31), elements after the axis
  uint32_t shifts;          // min(shifts, max(n - 1, 1)): more shifts clip to the same neighbours; 0 marks everything
  uint32_t log2p;           // peaks.rows doubling table level: 2^log2p <= shifts
};

// extreme of the line's elements [a, b] (axis coordinates) of element e at coordinate i, one by one
template <int C, typename T>
__device__ __forceinline__ T ext_run(const T* __restrict__ x, uint64_t e, int64_t i, int64_t a, int64_t b, int64_t st) {
  T m = x[e + (a - i) * st];
  for (int64_t q = a + 1; q <= b; ++q) m = ext<C>(m, x[e + (q - i) * st]);
  return m;
}

// van Herk / Gil-Werman: extreme of [a, b] (length <= S, a block start, or b a block end, when both lie in one block of S)
template <int C, typename T>
__device__ __forceinline__ T ext_vh(const T* __restrict__ g, const T* __restrict__ h, uint64_t e, int64_t i, int64_t a, int64_t b, int64_t S,
                                    int64_t st) {
  const int64_t ba = a / S, bb = b / S;
  if (ba != bb) return ext<C>(h[e + (a - i) * st], g[e + (b - i) * st]);
  return a == ba * S ? g[e + (b - i) * st] : h[e + (a - i) * st];
}

// pre-pass of peaks.strided for S > kBruteMax: g = extreme from the block's start, h = extreme to the block's end, blocks of S along
// the axis starting at 0 (the last one ends at n - 1)
template <typename T, int C>
__global__ __launch_bounds__(256) void k_peaks_vh(const T* __restrict__ x, T* __restrict__ g, T* __restrict__ h, Line L) {
  const uint64_t S = L.shifts, nblk = (L.n + S - 1) / S;
  const uint64_t jobs = L.total / L.n * nblk;
  for (uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x; id < jobs; id += (uint64_t)gridDim.x * 256) {
    const uint64_t c = id % L.inner, rest = id / L.inner, blk = rest % nblk, o = rest / nblk;
    const uint64_t q0 = blk * S, q1 = q0 + S < L.n ? q0 + S : L.n;
    const uint64_t base = (o * L.n) * L.inner + c;
    T m = x[base + q0 * L.inner];
    g[base + q0 * L.inner] = m;
    for (uint64_t q = q0 + 1; q < q1; ++q) {
      m = ext<C>(m, x[base + q * L.inner]);
      g[base + q * L.inner] = m;
    }
    m = x[base + (q1 - 1) * L.inner];
    h[base + (q1 - 1) * L.inner] = m;
    for (uint64_t q = q1 - 1; q > q0; --q) {
      m = ext<C>(m, x[base + (q - 1) * L.inner]);
      h[base + (q - 1) * L.inner] = m;
    }
  }
}

// pass 1: marks of one tile as ballot words, and the tile's count
template <typename T, int C, int MODE>
__global__ __launch_bounds__(kThreads) void k_peaks_mark(const T* __restrict__ x, const T* __restrict__ g, const T* __restrict__ h, Line L,
                                                         uint64_t* __restrict__ words, uint32_t* __restrict__ counts) {
  extern __shared__ __align__(16) unsigned char peaks_lds[];
  __shared__ uint32_t wave_count[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTile;
  const int64_t S = L.shifts, n = L.n, st = L.inner;
  T* M = reinterpret_cast<T*>(peaks_lds);
  uint64_t lo = 0;   // first element held in LDS (peaks.rows)
  if constexpr (MODE == kRows) {
    constexpr int V = 16 / sizeof(T);
    const uint64_t want = b0 > (uint64_t)S ? b0 - S : 0;
    lo = want - want % V;
    const uint64_t hi = b0 + kTile + S < L.total ? b0 + kTile + S : L.total;
    const uint64_t groups = (hi - lo + V - 1) / V;
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    for (uint64_t q = tid; q < groups; q += kThreads) {
      const uint64_t e0 = lo + q * V;
      if (aligned && e0 + V <= L.total) {
        *reinterpret_cast<uint4*>(M + q * V) = *reinterpret_cast<const uint4*>(x + e0);
      } else {
        for (int v = 0; v < V && e0 + v < L.total; ++v) M[q * V + v] = x[e0 + v];
      }
    }
    __syncthreads();
    if (S > kBruteMax) {   // in-place doubling: after level t, M[j] = extreme of x[j, j + 2^(t+1))
      const int64_t cnt = (int64_t)(groups * V);
      for (uint32_t t = 0; t < L.log2p; ++t) {
        const int64_t d = (int64_t)1 << t;
        for (int64_t cb = 0; cb < cnt; cb += 8 * kThreads) {   // chunks in increasing order: a chunk reads only what is not yet written
          T r[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int64_t jj = cb + k * kThreads + tid;
            r[k] = jj + d < cnt ? ext<C>(M[jj], M[jj + d]) : T(0);
          }
          __syncthreads();
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int64_t jj = cb + k * kThreads + tid;
            if (jj + d < cnt) M[jj] = r[k];
          }
          __syncthreads();
        }
      }
    }
  }
  uint32_t count = 0;   // wave-uniform
#pragma unroll 2
  for (int j = 0; j < kItems; ++j) {
    const uint64_t e = b0 + j * kThreads + tid;
    bool m = false;
    if (e < L.total) {
      if constexpr (MODE == kNonzero) {
        m = reinterpret_cast<const uint8_t*>(x)[e] != 0;
      } else {
        const int64_t i = (int64_t)((uint32_t)e / L.inner % L.n);   // total < 2^32
        const T v = MODE == kRows && S <= kBruteMax ? M[e - lo] : x[e];   // the doubling table has overwritten the tile (L2 still holds it)
        const int64_t lo_w = i - (S < i ? S : i), hi_w = i + (S < n - 1 - i ? S : n - 1 - i);   // the two windows' far ends
        m = true;
        if (S == 0) {
        } else if (MODE == kGeneric || S <= kBruteMax) {   // each neighbour in turn
          const T* xe = MODE == kRows ? M + (e - lo) : x + e;
          for (int64_t s = 1; s <= S && (MODE != kGeneric || m); ++s) {
            const int64_t ip = i + s < n - 1 ? i + s : n - 1, im = i - s > 0 ? i - s : 0;
            m = m && cmp<C>(v, xe[(ip - i) * st]) && cmp<C>(v, xe[(im - i) * st]);
          }
        } else {
          T el = v, er = v;   // the ends of a line compare with themselves
          if (MODE == kRows) {
            const int64_t P = (int64_t)1 << L.log2p, le = (int64_t)(e - lo);
            if (i > 0) el = i - lo_w >= P ? ext<C>(M[le - (i - lo_w)], M[le - P]) : ext_run<C>(x, e, i, lo_w, i - 1, 1);
            if (i < n - 1) er = hi_w - i >= P ? ext<C>(M[le + 1], M[le + (hi_w - i) - P + 1]) : ext_run<C>(x, e, i, i + 1, hi_w, 1);
          } else {
            if (i > 0) el = ext_vh<C>(g, h, e, i, lo_w, i - 1, S, st);
            if (i < n - 1) er = ext_vh<C>(g, h, e, i, i + 1, hi_w, S, st);
          }
          m = cmp<C>(v, el) && cmp<C>(v, er);
        }
      }
    }
    const uint64_t bal = __ballot(m);
    const uint64_t w = (b0 + j * kThreads) / 64 + wave;
    if (lane == 0 && w < L.nwords) words[w] = bal;
    count += (uint32_t)__popcll(bal);
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
    for (int q = 0; q < kThreads / 64; ++q) s += wave_count[q];
    counts[blockIdx.x] = s;
  }
}

// pass 2: one workgroup; each thread sums a contiguous run of tiles, an LDS scan of the run sums, then the run's offsets in order
__global__ __launch_bounds__(1024) void k_peaks_scan(const uint32_t* __restrict__ counts, uint64_t ntiles, uint64_t* __restrict__ offsets,
                                                     uint32_t* __restrict__ valid) {
  __shared__ uint64_t part[1024];
  const int tid = threadIdx.x;
  const uint64_t run = (ntiles + 1023) / 1024, q0 = tid * run, q1 = q0 + run < ntiles ? q0 + run : ntiles;
  uint64_t s = 0;
  for (uint64_t q = q0; q < q1; ++q) s += counts[q];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele
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

struct Coords {
  uint64_t total, nwords;
  uint32_t dims[8];
  int32_t rank;
};

// pass 3: coordinates of the tile's marks, then -1 over the tile's rows at or past valid
__global__ __launch_bounds__(kThreads) void k_peaks_write(const uint64_t* __restrict__ words, const uint64_t* __restrict__ offsets,
                                                          const uint32_t* __restrict__ valid, Coords G, int32_t* __restrict__ indices) {
  __shared__ uint64_t bits[kTile / 64];
  __shared__ uint32_t before[kTile / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * kTile, w0 = b0 / 64;
  if (tid < kTile / 64) {   // wave 0: the tile's words and an exclusive scan of their popcounts
    const uint64_t b = w0 + tid < G.nwords ? words[w0 + tid] : 0;
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
  const int rank = G.rank;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int j = 0; j < kItems; ++j) {
    const int wi = j * (kThreads / 64) + wave;
    const uint64_t b = bits[wi];
    if (!((b >> lane) & 1)) continue;
    const uint64_t pos = off + before[wi] + (uint64_t)__popcll(b & below);
    uint32_t e = (uint32_t)(b0 + j * kThreads + tid);
    int32_t* row = indices + pos * rank;
    for (int d = rank - 1; d >= 0; --d) {
      const uint32_t nd = G.dims[d];
      row[d] = (int32_t)(e % nd);
      e /= nd;
    }
  }
  // the -1 rows: [max(b0, valid), min(b0 + kTile, total)) as int32 elements [s0, s1)
  const uint64_t v = *valid, r0 = b0 > v ? b0 : v, r1 = b0 + kTile < G.total ? b0 + kTile : G.total;
  if (r0 >= r1) return;
  const uint64_t s0 = r0 * rank, s1 = r1 * rank;
  uint64_t a0 = s1, a1 = s1;   // the 16-byte aligned middle
  if ((reinterpret_cast<uintptr_t>(indices) & 15) == 0) {
    a0 = (s0 + 3) & ~3ull;
    a1 = s1 & ~3ull;
    if (a0 > a1) a0 = a1 = s1;
  }
  for (uint64_t q = s0 + tid; q < a0; q += kThreads) indices[q] = -1;
  for (uint64_t q = a0 / 4 + tid; q < a1 / 4; q += kThreads) reinterpret_cast<int4*>(indices)[q] = make_int4(-1, -1, -1, -1);
  for (uint64_t q = a1 + tid; q < s1; q += kThreads) indices[q] = -1;
}

// peaks.rows LDS: the tile, S on either side, and up to two partial 16-byte groups at the ends
size_t rows_lds(uint64_t S, size_t es) { return ((size_t)kTile + 2 * S + 2 * (16 / es)) * es; }

template <typename T, int C>
int mark_typed(Ctx* c, const void* xv, const Line& L, int family, uint64_t ntiles, uint64_t* words, uint32_t* counts) {
  const T* x = static_cast<const T*>(xv);
  const T *g = nullptr, *h = nullptr;
  if (family == kStrided && L.shifts > kBruteMax) {
    void* sc = nullptr;
    int rc = ctx_scratch(c, kScratchPeakExtremes, (size_t)L.total * 2 * sizeof(T), &sc);
    if (rc) return rc;
    T* gw = static_cast<T*>(sc);
    T* hw = gw + L.total;
    const uint64_t jobs = L.total / L.n * ((L.n + L.shifts - 1) / L.shifts);
    const uint64_t blocks = (jobs + 255) / 256 < (uint64_t)c->num_cus * 32 ? (jobs + 255) / 256 : (uint64_t)c->num_cus * 32;
    hipLaunchKernelGGL((k_peaks_vh<T, C>), dim3((unsigned)blocks), dim3(256), 0, c->stream, x, gw, hw, L);
    NXSIG_HIP_TRY(hipGetLastError());
    g = gw;
    h = hw;
  }
  const dim3 grid((unsigned)ntiles);
  switch (family) {
    case kRows: {
      const size_t lds = rows_lds(L.shifts, sizeof(T));
      hipLaunchKernelGGL((k_peaks_mark<T, C, kRows>), grid, dim3(kThreads), lds, c->stream, x, g, h, L, words, counts);
      break;
    }
    case kStrided: hipLaunchKernelGGL((k_peaks_mark<T, C, kStrided>), grid, dim3(kThreads), 0, c->stream, x, g, h, L, words, counts); break;
    default: hipLaunchKernelGGL((k_peaks_mark<T, C, kGeneric>), grid, dim3(kThreads), 0, c->stream, x, g, h, L, words, counts); break;
  }
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <typename T>
int mark_cmp(Ctx* c, const void* x, int comparator, const Line& L, int family, uint64_t ntiles, uint64_t* words, uint32_t* counts) {
  switch (comparator) {
    case kLess: return mark_typed<T, kLess>(c, x, L, family, ntiles, words, counts);
    case kGreater: return mark_typed<T, kGreater>(c, x, L, family, ntiles, words, counts);
    case kLessEq: return mark_typed<T, kLessEq>(c, x, L, family, ntiles, words, counts);
    default: return mark_typed<T, kGreaterEq>(c, x, L, family, ntiles, words, counts);
  }
}

size_t elem_size(int dtype) { return dtype == NXSIG_DT_F64 || dtype == NXSIG_DT_S64 || dtype == NXSIG_DT_U64 ? 8 : 4; }

// passes 2 and 3 over the words and counts pass 1 left in the kScratchPeakTiles slot
int compact(Ctx* c, uint64_t total, const int64_t* shape, int rank, uint64_t ntiles, const uint64_t* words, const uint32_t* counts,
            uint64_t* offsets, int32_t* indices, uint32_t* valid) {
  hipLaunchKernelGGL(k_peaks_scan, dim3(1), dim3(1024), 0, c->stream, counts, ntiles, offsets, valid);
  NXSIG_HIP_TRY(hipGetLastError());
  Coords G{};
  G.total = total;
  G.nwords = (total + 63) / 64;
  G.rank = rank;
  for (int d = 0; d < rank; ++d) G.dims[d] = (uint32_t)shape[d];
  hipLaunchKernelGGL(k_peaks_write, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, words, (const uint64_t*)offsets, (const uint32_t*)valid,
                     G, indices);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

int workspace(Ctx* c, uint64_t total, uint64_t ntiles, uint64_t** words, uint32_t** counts, uint64_t** offsets) {
  const uint64_t nwords = (total + 63) / 64;
  void* sc = nullptr;
  int rc = ctx_scratch(c, kScratchPeakTiles, (size_t)(ntiles * 8 + nwords * 8 + ntiles * 4), &sc);
  if (rc) return rc;
  *offsets = static_cast<uint64_t*>(sc);
  *words = *offsets + ntiles;
  *counts = reinterpret_cast<uint32_t*>(*words + nwords);
  return NXSIG_OK;
}

}  // namespace

int launch_argrelextrema(Ctx* c, const void* x, int dtype, const int64_t* shape, int rank, int axis, int64_t shifts, int comparator,
                         int32_t* indices, uint32_t* valid) {
  Line L{};
  L.total = 1;
  for (int d = 0; d < rank; ++d) L.total *= (uint64_t)shape[d];
  L.nwords = (L.total + 63) / 64;
  L.n = (uint32_t)shape[axis];
  L.inner = 1;
  for (int d = axis + 1; d < rank; ++d) L.inner *= (uint32_t)shape[d];
  const int64_t cap = L.n > 1 ? (int64_t)L.n - 1 : 1;
  L.shifts = (uint32_t)(shifts < cap ? shifts : cap);
  while (L.log2p < 31 && ((uint64_t)2 << L.log2p) <= L.shifts) ++L.log2p;
  const size_t es = elem_size(dtype);
  int family = kGeneric;
  if (tune(c, kT_DISABLE_PEAK_TILES, 0) == 0) {
    family = kStrided;   // also the last axis when the tile and its halo do not fit in LDS
    if (L.inner == 1 && rows_lds(L.shifts, es) <= kRowsLds) family = kRows;
  }
  dispatch_note(family == kGeneric ? "peaks.generic" : (L.inner == 1 ? "peaks.rows" : "peaks.strided"));
  const uint64_t ntiles = (L.total + kTile - 1) / kTile;
  uint64_t *words, *offsets;
  uint32_t* counts;
  int rc = workspace(c, L.total, ntiles, &words, &counts, &offsets);
  if (rc) return rc;
  switch (dtype) {
    case NXSIG_DT_F32: rc = mark_cmp<float>(c, x, comparator, L, family, ntiles, words, counts); break;
    case NXSIG_DT_F64: rc = mark_cmp<double>(c, x, comparator, L, family, ntiles, words, counts); break;
    case NXSIG_DT_S32: rc = mark_cmp<int32_t>(c, x, comparator, L, family, ntiles, words, counts); break;
    case NXSIG_DT_S64: rc = mark_cmp<int64_t>(c, x, comparator, L, family, ntiles, words, counts); break;
    case NXSIG_DT_U32: rc = mark_cmp<uint32_t>(c, x, comparator, L, family, ntiles, words, counts); break;
    default: rc = mark_cmp<uint64_t>(c, x, comparator, L, family, ntiles, words, counts); break;
  }
  if (rc) return rc;
  return compact(c, L.total, shape, rank, ntiles, words, counts, offsets, indices, valid);
}

int launch_nonzero(Ctx* c, const uint8_t* mask, const int64_t* shape, int rank, int32_t* indices, uint32_t* valid) {
  Line L{};
  L.total = 1;
  for (int d = 0; d < rank; ++d) L.total *= (uint64_t)shape[d];
  L.nwords = (L.total + 63) / 64;
  L.n = 1;
  L.inner = 1;
  dispatch_note("nonzero");
  const uint64_t ntiles = (L.total + kTile - 1) / kTile;
  uint64_t *words, *offsets;
  uint32_t* counts;
  int rc = workspace(c, L.total, ntiles, &words, &counts, &offsets);
  if (rc) return rc;
  hipLaunchKernelGGL((k_peaks_mark<uint8_t, kLess, kNonzero>), dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, mask, nullptr, nullptr, L,
                     words, counts);
  NXSIG_HIP_TRY(hipGetLastError());
  return compact(c, L.total, shape, rank, ntiles, words, counts, offsets, indices, valid);
}

}  // namespace nxsig
