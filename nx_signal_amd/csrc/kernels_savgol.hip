// Filters.savgol_filter (include/nxsig.h states the definition, DESIGN.md section 3.15 the design): y[i] = sum_j k[j] ext(i - L + j)
// over f32 or f64 rows, samples widened to double, one fused multiply-add per weight in ascending j, the sum rounded once.
//
//   savgol.tiles    one workgroup of 256 lanes per tile of T = 2048 consecutive outputs of a row.  The T + W - 1 samples around the tile
//                   come in as aligned 16-byte vectors (a vector that leaves the row goes element by element through savgol_ext, so the
//                   extension rule is applied once, at load time) and are kept in LDS as doubles.  A lane owns 8 consecutive outputs: it
//                   holds a window of 16 samples in registers, reads 8 new ones per 8 weights and spends 64 multiply-adds on them.  The
//                   LDS image skips one double after every 32: lanes 8 doubles apart would otherwise all start on the same four
//                   bank pairs, and with the skip the 32 lanes of an 8-byte read group start on 32 different ones.  That is the
//                   arithmetic of the layout, not a measurement: the compiler merges most of a lane's 8 consecutive reads into
//                   ds_read2_b64 (the rest stay ds_read_b64), whose lane groups differ, and the LDS conflict counters of this kernel
//                   have not been read.  The weights are a table in device memory read with a uniform index (scalar loads).
//   savgol.generic  one lane per output, every sample from global memory through savgol_ext: the same products in the same order, so
//                   the same bits.  Takes rows shorter than one tile and everything under NXSIG_DISABLE_SAVGOL_TILES.
//   edges           mode "interp" only, after either tier on the same stream: one lane per edge output, the transposed edge table
//                   Et[j][i] read coalesced, the first / last W samples of the row read uniformly.
// No atomics, no scratch.  The tables (weights, Et) are formed on the host once per context and parameter set (savgol_plan.hpp).
#include <cstring>

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kLanes = kSavgolLanes, kPer = kSavgolPer, kTile = kSavgolTile;
// doubles a tile keeps: the samples of its outputs, the window around them, and the reads of the last (partial) group of weights
constexpr int kLdsLogical = kTile + kSavgolMaxWindow - 1 + 2 * kPer;
__host__ __device__ constexpr int phys(int i) { return i + (i >> 5); }
constexpr int kLdsDoubles = phys(kLdsLogical) + 1;

struct Geom {
  int64_t n, x_stride, per_row;   // per_row: tiles (savgol.tiles) or 256-output blocks (savgol.generic) of a row
  int32_t W, L, h, mode, deriv;
  double fill;                    // what the extension holds where savgol_ext says -1
};

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

template <typename T>
__global__ __launch_bounds__(kLanes) void k_savgol_tiles(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ k, Geom g) {
  __shared__ double lds[kLdsDoubles];
  constexpr int V = 16 / (int)sizeof(T);
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / g.per_row, t0 = (blockIdx.x % g.per_row) * kTile;
  const T* xrow = x + row * g.x_stride;
  const int cnt = (int)(g.n - t0 < kTile ? g.n - t0 : kTile);   // outputs of this tile
  const int span = cnt + g.W - 1;                               // samples they cover
  const int64_t start = t0 - g.L;                               // index of the first one in the extended row
  // elements between the 16-byte boundary at or below &xrow[start] and that address (the pointer is never formed: start may be < 0)
  const int lead = (int)((((uintptr_t)xrow + (uintptr_t)(start * (int64_t)sizeof(T))) / sizeof(T)) & (V - 1));
  const int groups = (lead + span + V - 1) / V;
  for (int q = tid; q < groups; q += kLanes) {
    const int64_t e0 = start - lead + (int64_t)q * V;
    T e[V];
    if (e0 >= 0 && e0 + V <= g.n) {
      const typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(xrow + e0);
      __builtin_memcpy(e, &v, sizeof v);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const int li = q * V + c - lead;
        if (li >= 0 && li < span) lds[phys(li)] = (double)e[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const int li = q * V + c - lead;
        if (li >= 0 && li < span) {
          const int64_t s = savgol_ext(e0 + c, g.n, g.mode);
          lds[phys(li)] = s < 0 ? g.fill : (double)xrow[s];
        }
      }
    }
  }
  __syncthreads();

  const int base = tid * kPer;
  double win[2 * kPer], acc[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    acc[r] = 0.0;
    win[r] = lds[phys(base) + r];   // base is a multiple of 8: the 8 doubles lie inside one run of 32
  }
  int j0 = 0;
  for (; j0 + kPer <= g.W; j0 += kPer) {
    const double* next = lds + phys(base + j0 + kPer);
#pragma unroll
    for (int r = 0; r < kPer; ++r) win[kPer + r] = next[r];
#pragma unroll
    for (int jj = 0; jj < kPer; ++jj) {
      const double kj = k[j0 + jj];
#pragma unroll
      for (int r = 0; r < kPer; ++r) acc[r] = __builtin_fma(kj, win[jj + r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) win[r] = win[kPer + r];
  }
  if (j0 < g.W) {   // the last W % 8 weights: the reads beyond the tile's samples stay inside the array and reach no sum
    const double* next = lds + phys(base + j0 + kPer);
#pragma unroll
    for (int r = 0; r < kPer; ++r) win[kPer + r] = next[r];
#pragma unroll
    for (int jj = 0; jj < kPer - 1; ++jj) {
      if (j0 + jj < g.W) {
        const double kj = k[j0 + jj];
#pragma unroll
        for (int r = 0; r < kPer; ++r) acc[r] = __builtin_fma(kj, win[jj + r], acc[r]);
      }
    }
  }
  __syncthreads();
  // through LDS once more, so that the stores of a wave are consecutive
#pragma unroll
  for (int r = 0; r < kPer; ++r) lds[phys(base) + r] = acc[r];
  __syncthreads();
  T* yrow = y + row * g.n + t0;
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const int i = tid + r * kLanes;
    if (i < cnt) yrow[i] = (T)lds[phys(i)];
  }
}

template <typename T>
__global__ __launch_bounds__(kLanes) void k_savgol_generic(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ k, Geom g) {
  const int64_t row = blockIdx.x / g.per_row, i = (blockIdx.x % g.per_row) * kLanes + threadIdx.x;
  if (i >= g.n) return;
  const T* xrow = x + row * g.x_stride;
  double acc = 0.0;
  for (int j = 0; j < g.W; ++j) {
    const int64_t s = savgol_ext(i - g.L + j, g.n, g.mode);
    acc = __builtin_fma(k[j], s < 0 ? g.fill : (double)xrow[s], acc);
  }
  y[row * g.n + i] = (T)acc;
}

// the first and last h outputs of every row in mode "interp": blocks = rows * 2 sides * ceil(h / 64)
template <typename T>
__global__ __launch_bounds__(64) void k_savgol_edges(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ Et, Geom g) {
  const int64_t per_side = (g.h + 63) / 64;
  const int64_t row = blockIdx.x / (2 * per_side);
  const int rest = (int)(blockIdx.x % (2 * per_side));
  const int side = rest / (int)per_side, i = (rest % (int)per_side) * 64 + (int)threadIdx.x;
  if (i >= g.h) return;
  const T* xrow = x + row * g.x_stride;
  double acc = 0.0;
  for (int j = 0; j < g.W; ++j) acc = __builtin_fma(Et[(size_t)j * g.h + i], (double)xrow[side ? g.n - 1 - j : j], acc);
  y[row * g.n + (side ? g.n - 1 - i : i)] = (T)((side && (g.deriv & 1)) ? -acc : acc);
}

template <typename T> int run(Ctx* c, const SavgolLaunch& a, const double* k, const double* Et, bool tiles) {
  Geom g;
  g.n = a.n; g.x_stride = a.x_stride;
  g.W = a.W; g.L = savgol_left(a.W); g.h = a.W / 2; g.mode = a.mode; g.deriv = a.deriv;
  g.fill = a.mode == kSgConstant ? a.cval : 0.0;
  g.per_row = tiles ? savgol_tiles(a.n) : (a.n + kLanes - 1) / kLanes;
  if (g.per_row >= ((int64_t)1 << 31) / a.batch) return set_error(NXSIG_ERR_UNSUPPORTED, "savgol_filter: 2^31 or more workgroups in one call");
  const T* x = static_cast<const T*>(a.x);
  T* y = static_cast<T*>(a.y);
  const dim3 grid((unsigned)(g.per_row * a.batch));
  if (tiles) {
    dispatch_note("savgol.tiles");
    hipLaunchKernelGGL(k_savgol_tiles<T>, grid, dim3(kLanes), 0, c->stream, x, y, k, g);
  } else {
    dispatch_note("savgol.generic");
    hipLaunchKernelGGL(k_savgol_generic<T>, grid, dim3(kLanes), 0, c->stream, x, y, k, g);
  }
  NXSIG_HIP_TRY(hipGetLastError());
  if (a.mode == kSgInterp && g.h > 0) {
    const int64_t blocks = (int64_t)a.batch * 2 * ((g.h + 63) / 64);
    if (blocks >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_UNSUPPORTED, "savgol_filter: 2^31 or more workgroups in one call");
    hipLaunchKernelGGL(k_savgol_edges<T>, dim3((unsigned)blocks), dim3(64), 0, c->stream, x, y, Et, g);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_savgol(Ctx* c, const SavgolLaunch& a) {
  // the tables of a parameter set are formed once per context: the memo keeps the device pointers beside the parameters, so a later
  // call neither solves the fit again (tens of milliseconds of extended precision for the edge table of a 1025-sample window) nor
  // hashes 4 MB.  Dropped together with the table cache (DeviceGuard, api.cpp)
  const bool interp = a.mode == kSgInterp && a.W / 2 > 0;
  uint64_t dbits;
  std::memcpy(&dbits, &a.delta, sizeof dbits);
  std::vector<uint64_t> want = {0, 0, (uint64_t)a.W, (uint64_t)a.p, (uint64_t)a.deriv, (uint64_t)interp, dbits};
  const uint64_t key = fnv1a(0x5A760C0Full, want.data() + 2, (want.size() - 2) * sizeof(uint64_t));
  const void *kd = nullptr, *ed = nullptr;
  auto hit = c->memo.find(key);
  if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 2, want.end(), hit->second.begin() + 2)) {
    kd = reinterpret_cast<const void*>((uintptr_t)hit->second[0]);
    ed = reinterpret_cast<const void*>((uintptr_t)hit->second[1]);
  } else {
    int rc;
    std::vector<double> k(a.W);
    savgol_coeffs(a.W, a.p, a.deriv, a.delta, -1.0, kSgDot, k.data());
    if ((rc = ctx_table(c, 0x5A764B00ull, k.data(), k.size() * sizeof(double), &kd))) return rc;
    if (interp) {
      const std::vector<double> Et = savgol_edge_table(a.W, a.p, a.deriv, a.delta);
      if ((rc = ctx_table(c, 0x5A764500ull, Et.data(), Et.size() * sizeof(double), &ed))) return rc;
    }
    want[0] = (uint64_t)(uintptr_t)kd;
    want[1] = (uint64_t)(uintptr_t)ed;
    c->memo[key] = want;
  }
  const bool tiles = !tune(c, kT_DISABLE_SAVGOL_TILES, 0) && a.n >= kSavgolTile;
  return a.f64 ? run<double>(c, a, static_cast<const double*>(kd), static_cast<const double*>(ed), tiles)
               : run<float>(c, a, static_cast<const double*>(kd), static_cast<const double*>(ed), tiles);
}

}  // namespace nxsig
