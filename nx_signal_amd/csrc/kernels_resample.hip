// Filters.resample_poly: polyphase rational resampling of f32 / c64 rows by up / down (reduced, up != down); include/nxsig.h states the
// definition, DESIGN.md section 3.11 the design.  Output m of a row of n samples, with c = m down + half, q = c div up, r = c mod up:
//     y[m] = sum_t x[q - t] h[r + t up]      over t in [max(0, q - (n - 1)), min(T_r - 1, q)], T_r = taps of branch r
// accumulated from +0.0 by ONE fmaf chain in ascending t (c64: a chain per component, the taps are real).  A term outside that range
// is never multiplied in: the loops are bounded, or the finished fmaf is dropped by a select — never 0 * x.
//
//   resample.poly.lds      phase table g[r][t] = h[r + t up] (row pitch T | 1, zero where r + t up >= L) and the input span of a tile
//                          of kResampleTile outputs in LDS; 256 lanes x 4 outputs each (output i of the tile on lane i % 256: stores
//                          and, for odd down / up, LDS reads are conflict-free); a workgroup keeps its table over several tiles.
//                          up == 1 has one branch: its taps are wave-uniform scalar loads
//   resample.poly.generic  any L, up, down: one output per lane, samples and taps from global memory
//   resample.copy          up == down: the rows copied
// Both polyphase tiers form the same chain in the same order: the same bits.
#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = kResampleTile / kThreads;   // register block: outputs per lane, independent fmaf chains
constexpr size_t kLdsTableMax = 64 * 1024;           // phase table up x T floats of the LDS tier
constexpr size_t kLdsBudget = 96 * 1024;             // table + tile per workgroup (one workgroup per CU at the worst)

typedef float gf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float zero_of(const float*) { return 0.0f; }
__device__ __forceinline__ float2 zero_of(const float2*) { return make_float2(0.0f, 0.0f); }
__device__ __forceinline__ float mac(float x, float h, float a) { return __builtin_fmaf(x, h, a); }
__device__ __forceinline__ float2 mac(float2 x, float h, float2 a) { return make_float2(__builtin_fmaf(x.x, h, a.x), __builtin_fmaf(x.y, h, a.y)); }
__device__ __forceinline__ float pick(bool k, float v, float a) { return k ? v : a; }
__device__ __forceinline__ float2 pick(bool k, float2 v, float2 a) { return make_float2(k ? v.x : a.x, k ? v.y : a.y); }
__device__ __forceinline__ void store_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_nt(float2* p, float2 v) {
  __builtin_nontemporal_store(v.x, &p->x);
  __builtin_nontemporal_store(v.y, &p->y);
}

struct Geom {
  int64_t n, n_out, x_stride;   // samples and outputs per row; elements between rows of x
  int32_t up, down, half, L, T, Tp;   // T = ceil(L / up); Tp = T | 1, the row pitch of the phase table
  int32_t tiles, tiles_per_wg;        // tiles per row; consecutive tiles of one row a workgroup runs
};

// LDS index of tile sample i.  PAD (even lane stride down / up into the tile: 2-, 4-, ... way conflicts on the 32 banks of a
// ds_read_b32) skips one dword after every 32, which spreads such a stride over all banks
template <bool PAD> __device__ __forceinline__ int lidx(int i) { return PAD ? i + (i >> 5) : i; }

template <class S, bool PAD, bool UP1>
__global__ __launch_bounds__(kThreads) void k_resample_lds(const S* __restrict__ x, const float* __restrict__ g, S* __restrict__ y, Geom p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int V = 16 / (int)sizeof(S);
  const int table_elems = UP1 ? 0 : (p.up * p.Tp + 3) & ~3;   // pure decimation reads its taps from g: no table in LDS
  float* gs = reinterpret_cast<float*>(lds_raw);
  S* xs = reinterpret_cast<S*>(lds_raw + (size_t)table_elems * sizeof(float));
  const int tid = threadIdx.x;
  const int wg_per_row = (p.tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
  const int row = blockIdx.x / wg_per_row;
  const int tile_first = (blockIdx.x % wg_per_row) * p.tiles_per_wg;
  const int tile_end = tile_first + p.tiles_per_wg < p.tiles ? tile_first + p.tiles_per_wg : p.tiles;
  const S* xrow = x + (int64_t)row * p.x_stride;
  S* yrow = y + (int64_t)row * p.n_out;

  for (int i = tid; i < table_elems / 4; i += kThreads) reinterpret_cast<gf4*>(gs)[i] = reinterpret_cast<const gf4*>(g)[i];

  for (int tile = tile_first; tile < tile_end; ++tile) {
    const int64_t m0 = (int64_t)tile * kResampleTile;
    const int cnt = p.n_out - m0 < kResampleTile ? (int)(p.n_out - m0) : kResampleTile;
    const int64_t c0 = m0 * p.down + p.half;
    const int64_t q0 = c0 / p.up;
    const int r0 = (int)(c0 - q0 * p.up);
    const int dq_last = UP1 ? (cnt - 1) * p.down : (r0 + (cnt - 1) * p.down) / p.up;
    const int64_t s0 = q0 - (p.T - 1);                     // first sample the tile's outputs can touch
    const int span = dq_last + p.T;
    // stage [s0, s0 + span): whole 16-byte words of the row wherever one lies inside it (a row may start anywhere: the words are
    // aligned in memory, `lead` elements ahead of s0), element by element with zeros outside [0, n) at the ends
    const int lead = (int)(((int64_t)(reinterpret_cast<uintptr_t>(xrow) / sizeof(S)) + s0) & (V - 1));
    const int64_t j0 = s0 - lead;
    const int nvec = (span + lead + V - 1) / V;
    __syncthreads();   // the previous tile's reads are done (first trip: nothing to wait for but the table's writers)
    for (int v = tid; v < nvec; v += kThreads) {
      const int64_t j = j0 + (int64_t)v * V;
      S e[V];
      if (j >= 0 && j + V <= p.n) {
        const gf4 w = *reinterpret_cast<const gf4*>(xrow + j);
        __builtin_memcpy(e, &w, 16);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) e[k] = (j + k >= 0 && j + k < p.n) ? xrow[j + k] : zero_of((const S*)nullptr);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) xs[lidx<PAD>(v * V + k)] = e[k];
    }
    __syncthreads();

    const bool interior = cnt == kResampleTile && s0 >= 0 && q0 + dq_last <= p.n - 1;   // every lo is 0, every hi is T_r - 1
    // per output: LDS index of x[q] (tap t reads xi - t), its branch's table row, the live range [lo, hi] of t
    int xi[kPerLane], gi[kPerLane], lo[kPerLane], hi[kPerLane];
    S acc[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const int i = k * kThreads + tid;
      const bool live = i < cnt;
      int dq = 0, r = 0;
      if (live) {
        if (UP1) { dq = i * p.down; }
        else { const int ci = r0 + i * p.down; dq = ci / p.up; r = ci - dq * p.up; }
      }
      const int64_t q = q0 + dq;
      const int Tr = r + (p.T - 1) * p.up < p.L ? p.T : p.T - 1;
      xi[k] = lead + (p.T - 1) + dq;
      gi[k] = r * p.Tp;
      const int64_t l = q - (p.n - 1);
      lo[k] = live ? (l > 0 ? (int)(l < p.T ? l : p.T) : 0) : 1;
      hi[k] = live ? (q < Tr - 1 ? (int)q : Tr - 1) : 0;
      acc[k] = zero_of((const S*)nullptr);
    }
    // tap t of output k's branch; pure decimation has one branch and a wave-uniform tap per step: a scalar load, no LDS read
    auto tap = [&](int k, int t) { return UP1 ? g[t] : gs[gi[k] + t]; };
    if (interior) {
      for (int t = 0; t < p.T - 1; ++t) {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) acc[k] = mac(xs[lidx<PAD>(xi[k] - t)], tap(k, t), acc[k]);
      }
      const int t = p.T - 1;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) acc[k] = pick(hi[k] == t, mac(xs[lidx<PAD>(xi[k] - t)], tap(k, t), acc[k]), acc[k]);
    } else {
      for (int t = 0; t < p.T; ++t) {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          acc[k] = pick(t >= lo[k] && t <= hi[k], mac(xs[lidx<PAD>(xi[k] - t)], tap(k, t), acc[k]), acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const int i = k * kThreads + tid;
      if (i < cnt) store_nt(yrow + m0 + i, acc[k]);
    }
  }
}

template <class S>
__global__ __launch_bounds__(kThreads) void k_resample_generic(const S* __restrict__ x, const float* __restrict__ h, S* __restrict__ y, Geom p) {
  const int64_t blocks_per_row = (p.n_out + kThreads - 1) / kThreads;
  const int64_t row = blockIdx.x / blocks_per_row;
  const int64_t m = (blockIdx.x % blocks_per_row) * kThreads + threadIdx.x;
  if (m >= p.n_out) return;
  const S* xrow = x + row * p.x_stride;
  const int64_t c = m * p.down + p.half;
  const int64_t q = c / p.up;
  const int64_t r = c - q * p.up;
  const int64_t Tr = r < p.L ? (p.L - r + p.up - 1) / p.up : 0;
  const int64_t lo = q - (p.n - 1) > 0 ? q - (p.n - 1) : 0;
  const int64_t hi = q < Tr - 1 ? q : Tr - 1;
  S acc = zero_of((const S*)nullptr);
  for (int64_t t = lo; t <= hi; ++t) acc = mac(xrow[q - t], h[r + t * p.up], acc);
  y[row * p.n_out + m] = acc;
}

template <class S>
__global__ __launch_bounds__(kThreads) void k_resample_copy(const S* __restrict__ x, S* __restrict__ y, int64_t n, int64_t x_stride) {
  const int64_t blocks_per_row = (n + kThreads - 1) / kThreads;
  const int64_t row = blockIdx.x / blocks_per_row;
  const int64_t j = (blockIdx.x % blocks_per_row) * kThreads + threadIdx.x;
  if (j < n) y[row * n + j] = x[row * x_stride + j];
}

template <class S, bool PAD, bool UP1>
int run_lds(Ctx* c, const ResampleLaunch& a, const Geom& p, const float* g, size_t lds, int64_t blocks) {
  auto kernel = k_resample_lds<S, PAD, UP1>;
  if (lds > 64 * 1024)
    NXSIG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, c->stream, static_cast<const S*>(a.x), g, static_cast<S*>(a.y), p);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <class S>
int run_lds_s(Ctx* c, const ResampleLaunch& a, const Geom& p, const float* g, size_t lds, int64_t blocks, bool pad) {
  if (p.up == 1) return pad ? run_lds<S, true, true>(c, a, p, g, lds, blocks) : run_lds<S, false, true>(c, a, p, g, lds, blocks);
  return pad ? run_lds<S, true, false>(c, a, p, g, lds, blocks) : run_lds<S, false, false>(c, a, p, g, lds, blocks);
}

}  // namespace

int launch_resample_copy(Ctx* c, const ResampleLaunch& a) {
  const int64_t blocks = ((a.n + kThreads - 1) / kThreads) * a.batch;
  if (blocks >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_UNSUPPORTED, "resample_poly: 2^31 or more tiles in one call");
  dispatch_note("resample.copy");
  if (a.is_complex)
    hipLaunchKernelGGL(k_resample_copy<float2>, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, static_cast<const float2*>(a.x),
                       static_cast<float2*>(a.y), a.n, a.batch_stride);
  else
    hipLaunchKernelGGL(k_resample_copy<float>, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, static_cast<const float*>(a.x),
                       static_cast<float*>(a.y), a.n, a.batch_stride);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

int launch_resample_poly(Ctx* c, const ResampleLaunch& a) {
  Geom p;
  p.n = a.n; p.n_out = a.n_out; p.x_stride = a.batch_stride;
  p.up = a.up; p.down = a.down; p.L = a.taps; p.half = (a.taps - 1) / 2;
  const int64_t T = ((int64_t)a.taps + a.up - 1) / a.up;
  p.T = (int32_t)T; p.Tp = (int32_t)(T | 1);
  const int64_t tiles = (a.n_out + kResampleTile - 1) / kResampleTile;
  const size_t elem = a.is_complex ? sizeof(float2) : sizeof(float);
  const int V = 16 / (int)elem;
  // LDS tier: the table up x T floats within 64 KiB, and table + the longest tile within the budget (a long decimation's tile —
  // about kResampleTile down / up samples — does not fit: that ratio runs the generic tier)
  const size_t table_elems = (((size_t)a.up * (size_t)p.Tp) + 3) & ~(size_t)3;
  const int64_t span_max = ((int64_t)(a.up - 1) + (int64_t)(kResampleTile - 1) * a.down) / a.up + T;
  int64_t tile_elems = (span_max + 2 * V - 2) / V * V;   // + the lead of up to V - 1 elements, in whole 16-byte words
  // an even whole-number lane stride into the tile: padded indices
  const bool pad = a.down % a.up == 0 && (a.down / a.up) % 2 == 0;
  if (pad) tile_elems += tile_elems / 32 + 1;
  const size_t lds = (a.up == 1 ? 0 : table_elems * sizeof(float)) + (size_t)tile_elems * elem;   // up == 1: taps by scalar loads
  const bool lds_tier = !tune(c, kT_DISABLE_RESAMPLE_LDS, 0) && (size_t)a.up * (size_t)T * sizeof(float) <= kLdsTableMax &&
                        a.down <= (1 << 20) && span_max < ((int64_t)1 << 24) && lds <= kLdsBudget;   // (tile-local indices stay in 32 bits)
  if (lds_tier) {
    // a workgroup keeps its table over consecutive tiles of one row, as many as still leave four workgroups per CU
    const int64_t want = (tiles * a.batch) / ((int64_t)c->num_cus * 4);
    const int64_t tpw = want < 1 ? 1 : (want > 16 ? 16 : want);
    const int64_t wg_per_row = (tiles + tpw - 1) / tpw;
    const int64_t blocks = wg_per_row * a.batch;
    if (tiles >= ((int64_t)1 << 31) || blocks >= ((int64_t)1 << 31))
      return set_error(NXSIG_ERR_UNSUPPORTED, "resample_poly: 2^31 or more tiles in one call");
    p.tiles = (int32_t)tiles; p.tiles_per_wg = (int32_t)tpw;
    std::vector<float> g(table_elems, 0.0f);
    for (int32_t r = 0; r < a.up; ++r)
      for (int64_t t = 0; r + t * a.up < a.taps; ++t) g[(size_t)r * p.Tp + t] = a.h_host[r + t * a.up];
    const void* gd = nullptr;
    int rc = ctx_table(c, 0x2E5A3B1Eull ^ ((uint64_t)a.up << 32) ^ (uint64_t)a.taps, g.data(), g.size() * sizeof(float), &gd);
    if (rc) return rc;
    dispatch_note("resample.poly.lds");
    return a.is_complex ? run_lds_s<float2>(c, a, p, static_cast<const float*>(gd), lds, blocks, pad)
                        : run_lds_s<float>(c, a, p, static_cast<const float*>(gd), lds, blocks, pad);
  }
  const int64_t blocks = ((a.n_out + kThreads - 1) / kThreads) * a.batch;
  if (blocks >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_UNSUPPORTED, "resample_poly: 2^31 or more tiles in one call");
  p.tiles = 0; p.tiles_per_wg = 1;
  const void* hd = nullptr;
  int rc = ctx_table(c, 0x2E5A3B1Dull ^ ((uint64_t)a.taps << 24), a.h_host, (size_t)a.taps * sizeof(float), &hd);
  if (rc) return rc;
  dispatch_note("resample.poly.generic");
  if (a.is_complex)
    hipLaunchKernelGGL(k_resample_generic<float2>, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, static_cast<const float2*>(a.x),
                       static_cast<const float*>(hd), static_cast<float2*>(a.y), p);
  else
    hipLaunchKernelGGL(k_resample_generic<float>, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, static_cast<const float*>(a.x),
                       static_cast<const float*>(hd), static_cast<float*>(a.y), p);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace nxsig
