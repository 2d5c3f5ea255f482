// The recurrence scan: a linear recurrence s[m + 1] = A s[m] + B x[m] with NP states in double, run over real f32 rows side by side in
// time.  Filters.sosfilt / sosfiltfilt (kernels_iir.hip) and Filters.lfilter / filtfilt (kernels_lfilter.hip) are its two families;
// DESIGN.md section 3.13 has the design.  A sample is widened on load and an output rounded to f32 once.
//
//   scan     a row is cut into chunks of C samples, one per lane, and tiles of 64 chunks, one per single-wave workgroup.
//              pass 1   every chunk runs the filter from a zero state; a scan over the 64 lanes with A^C, A^2C, ... A^32C turns
//                       the end states into P_i = the state at the end of chunk i of a tile that started at zero; P goes to memory
//              carry    one wave per row: lane j walks R consecutive tiles with A^T from zero, a scan over the lanes with
//                       A^(T R 2^k) joins the runs (the row's start state, zi or zero, enters at lane 0), a second walk writes
//                       every tile's true start state
//              pass 2   a scan of the tile's start state gives lane i its A^(i C) s_tile; with P_(i-1) that is the chunk's true
//                       start state; the chunk runs again and writes y
//            This is exact algebra, not a run-in: a pole on or outside the unit circle is as good as any.  The matrices are built on
//            the host.  Every sum has one fixed order and one writer.  Samples travel through LDS in pieces of 32 per chunk so that
//            global loads and stores are 16 bytes per lane.
//   generic  one lane per row, the plain recurrence
// direction 1 runs the same kernels over the row read backwards.
//
// A family is a struct F of types, constants and static functions; the kernels and the driver below take it as a template argument.
//   device   F::NP                       the padded state count a kernel is instantiated for
//            F::Coefs                    the coefficients, passed to a kernel by value
//            F::step(cf, s, x)           one sample through the filter: advances s, returns y
//            F::matvec_add(v, M, w)      v += M w over the columns in which a power of the family's A can be non-zero, ascending
//   host     F::Launch                   the family's launch struct, a ScanLaunch and its coefficients
//            F::fill(a)                  -> F::Coefs
//            F::states(a)                states per row of zi / zf
//            F::chunk(a), F::tiles(a)    C and the tiles of a row
//            F::kTooManyTiles            the text of the error; F::kTooManyBlocks: the forward-backward filter's
//            F::launch(c, a)             the family's launcher: its tier choice, then run_padded
//            F::note(scan)               dispatch_note of the tier
//            F::tables(c, a, R, &mc, &mt, &scan_ok)   the device matrices of pass 1 / 2 and of the carry; may take the filter off the scan
//            F::zi_table(c, padded, &d)  zi as a cached table: the zi of a forward-backward filter is a function of the coefficients
#pragma once
#include <algorithm>
#include <cstring>

#include "nxsig_internal.h"

namespace nxsig {
namespace rscan {

constexpr int kLanes = kIirLanes;
constexpr int kSub = kIirSub;
constexpr int kWords = kSub / 4 + 1;   // 16-byte words that cover a piece wherever it starts
constexpr int kPitch = 4 * kWords + 1; // LDS floats per chunk: odd, so the lanes' reads fall on different banks

typedef float gf4 __attribute__((ext_vector_type(4)));

struct Geom {
  int64_t n, x_stride, y_stride, out_off, out_len, tiles, R;
  int32_t C, dir, batch, zi_rows, zi_times_first;
};

// inclusive scan over the lanes of the wave: v_i <- sum over j <= i of B^(i - j) v_j, with M[k] = B^(2^k)
template <class F> __device__ __forceinline__ void scan_wave(double (&v)[F::NP], const double* __restrict__ M, int lane) {
  constexpr int NP = F::NP;
#pragma unroll 1
  for (int k = 0; k < kIirLevels; ++k) {
    double w[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) w[r] = __shfl_up(v[r], 1u << k, kLanes);
    if (lane >= (1 << k)) F::matvec_add(v, M + (size_t)k * NP * NP, w);
  }
}

// physical start of the piece of kSub samples whose logical start is l0 (negative when a backward piece hangs over the row's start)
__device__ __forceinline__ int64_t piece_start(const Geom& g, int64_t l0) { return g.dir ? g.n - l0 - kSub : l0; }

template <class F, bool PASS2>
__global__ __launch_bounds__(kLanes) void k_scan_pass(const float* __restrict__ x, float* __restrict__ y, typename F::Coefs cf,
                                                      const double* __restrict__ M, double* __restrict__ P,
                                                      const double* __restrict__ tile_start, double* __restrict__ zf, Geom g) {
  constexpr int NP = F::NP;
  __shared__ float lds[kLanes * kPitch];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x / g.tiles, tile = blockIdx.x - row * g.tiles;
  const float* xrow = x + row * g.x_stride;
  const int64_t xbase = (int64_t)(reinterpret_cast<uintptr_t>(xrow) >> 2);
  const int64_t l_chunk = (tile * kLanes + lane) * g.C;
  const int cnt = g.n - l_chunk >= g.C ? g.C : (g.n - l_chunk > 0 ? (int)(g.n - l_chunk) : 0);
  double* Pt = P + ((row * g.tiles + tile) * NP) * kLanes;

  double s[NP];
  if (PASS2) {
    const double* ts = tile_start + (row * g.tiles + tile) * NP;
#pragma unroll
    for (int r = 0; r < NP; ++r) s[r] = lane == 0 ? ts[r] : 0.0;
    scan_wave<F>(s, M, lane);
    if (lane > 0) {
#pragma unroll
      for (int r = 0; r < NP; ++r) s[r] += Pt[r * kLanes + lane - 1];
    }
  } else {
#pragma unroll
    for (int r = 0; r < NP; ++r) s[r] = 0.0;
  }

  for (int b = 0; b < g.C / kSub; ++b) {
    __syncthreads();   // the previous piece's readers are done
    for (int u = lane; u < kLanes * kWords; u += kLanes) {
      const int i = u / kWords, w = u - i * kWords;
      const int64_t p0 = piece_start(g, (tile * kLanes + i) * g.C + b * kSub);
      const int64_t p = p0 - ((xbase + p0) & 3) + 4 * w;
      float e[4];
      if (p >= 0 && p + 4 <= g.n) {
        const gf4 v = *reinterpret_cast<const gf4*>(xrow + p);
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = (p + k >= 0 && p + k < g.n) ? xrow[p + k] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) lds[i * kPitch + 4 * w + k] = e[k];
    }
    __syncthreads();
    {
      const int64_t p0 = piece_start(g, l_chunk + b * kSub);
      float* mine = lds + lane * kPitch + (int)((xbase + p0) & 3);
      const int live = cnt - b * kSub;   // samples of this piece that exist
#pragma unroll 4
      for (int j = 0; j < kSub; ++j) {
        if (j < live) {
          const int slot = g.dir ? kSub - 1 - j : j;
          const double yv = F::step(cf, s, (double)mine[slot]);
          if (PASS2) mine[slot] = (float)yv;
        }
      }
    }
    if (PASS2) {
      __syncthreads();
      float* yrow = y + row * g.y_stride;
      const int64_t ybase = (int64_t)(reinterpret_cast<uintptr_t>(yrow) >> 2);
      for (int u = lane; u < kLanes * kWords; u += kLanes) {
        const int i = u / kWords, w = u - i * kWords;
        const int64_t p0 = piece_start(g, (tile * kLanes + i) * g.C + b * kSub);
        const int lead_x = (int)((xbase + p0) & 3);
        const int64_t q0 = p0 - g.out_off;
        const int e0 = 4 * w - (int)((ybase + q0) & 3);   // element of the piece the word starts at
        const float* src = lds + i * kPitch + lead_x;
        bool ok[4], all = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = e0 + k;
          ok[k] = e >= 0 && e < kSub && p0 + e >= 0 && p0 + e < g.n && q0 + e >= 0 && q0 + e < g.out_len;
          all = all && ok[k];
        }
        if (all) {
          gf4 v;
          v.x = src[e0]; v.y = src[e0 + 1]; v.z = src[e0 + 2]; v.w = src[e0 + 3];
          *reinterpret_cast<gf4*>(yrow + q0 + e0) = v;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (ok[k]) yrow[q0 + e0 + k] = src[e0 + k];
        }
      }
    }
  }

  if (PASS2) {
    if (zf && cnt > 0 && l_chunk + cnt == g.n) {
#pragma unroll
      for (int r = 0; r < NP; ++r) zf[row * NP + r] = s[r];
    }
  } else {
    scan_wave<F>(s, M, lane);
#pragma unroll
    for (int r = 0; r < NP; ++r) Pt[r * kLanes + lane] = s[r];
  }
}

// the start state of a row: zero, zi, or zi * (the row's first logical sample)
template <int NP>
__device__ __forceinline__ void row_start(double (&s0)[NP], const float* __restrict__ x, const double* __restrict__ zi, int64_t row, const Geom& g) {
  if (zi) {
    const double* zr = zi + (g.zi_rows == 1 ? 0 : row) * NP;
    const double scale = g.zi_times_first ? (double)x[row * g.x_stride + (g.dir ? g.n - 1 : 0)] : 1.0;
#pragma unroll
    for (int r = 0; r < NP; ++r) s0[r] = zr[r] * scale;
  } else {
#pragma unroll
    for (int r = 0; r < NP; ++r) s0[r] = 0.0;
  }
}

// M: [0 .. 5] A^(T R 2^k), [6] A^T
template <class F>
__global__ __launch_bounds__(kLanes) void k_scan_carry(const float* __restrict__ x, const double* __restrict__ P, const double* __restrict__ M,
                                                       const double* __restrict__ zi, double* __restrict__ tile_start, Geom g) {
  constexpr int NP = F::NP;
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const double* MT = M + (size_t)kIirLevels * NP * NP;
  const int64_t t0 = lane * g.R < g.tiles ? lane * g.R : g.tiles;
  const int64_t t1 = t0 + g.R < g.tiles ? t0 + g.R : g.tiles;
  // the end state of tile t run from zero: P of its last lane
  auto tile_end = [&](int64_t t, double (&z)[NP]) {
    const double* Pt = P + ((row * g.tiles + t) * NP) * kLanes;
#pragma unroll
    for (int r = 0; r < NP; ++r) z[r] = Pt[r * kLanes + kLanes - 1];
  };
  double s0[NP], acc[NP], z[NP];
  row_start<NP>(s0, x, zi, row, g);
#pragma unroll
  for (int r = 0; r < NP; ++r) acc[r] = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    tile_end(t, z);
    F::matvec_add(z, MT, acc);
#pragma unroll
    for (int r = 0; r < NP; ++r) acc[r] = z[r];
  }
  if (lane == 0) F::matvec_add(acc, M, s0);   // lane 0 walks R tiles (R <= tiles): the row's start state travels A^(T R)
  scan_wave<F>(acc, M, lane);
  double s[NP];
#pragma unroll
  for (int r = 0; r < NP; ++r) {
    const double below = __shfl_up(acc[r], 1u, kLanes);
    s[r] = lane == 0 ? s0[r] : below;
  }
  for (int64_t t = t0; t < t1; ++t) {
    double* ts = tile_start + (row * g.tiles + t) * NP;
#pragma unroll
    for (int r = 0; r < NP; ++r) ts[r] = s[r];
    tile_end(t, z);
    F::matvec_add(z, MT, s);
#pragma unroll
    for (int r = 0; r < NP; ++r) s[r] = z[r];
  }
}

template <class F>
__global__ __launch_bounds__(kLanes) void k_scan_generic(const float* __restrict__ x, float* __restrict__ y, typename F::Coefs cf,
                                                         const double* __restrict__ zi, double* __restrict__ zf, Geom g) {
  constexpr int NP = F::NP;
  const int64_t row = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (row >= g.batch) return;
  double s[NP];
  row_start<NP>(s, x, zi, row, g);
  const float* xrow = x + row * g.x_stride;
  float* yrow = y + row * g.y_stride;
  for (int64_t i = 0; i < g.n; ++i) {
    const int64_t p = g.dir ? g.n - 1 - i : i;
    const double yv = F::step(cf, s, (double)xrow[p]);
    const int64_t q = p - g.out_off;
    if (q >= 0 && q < g.out_len) yrow[q] = (float)yv;
  }
  if (zf) {
#pragma unroll
    for (int r = 0; r < NP; ++r) zf[row * NP + r] = s[r];
  }
}

// the extension of a forward-backward filter: ext[row][j], j in [0, n + 2 e); the odd form 2 x_end - x is rounded to f32 once, as scipy
// forms it on f32 rows
static __global__ __launch_bounds__(256) void k_scan_extend(const float* __restrict__ x, float* __restrict__ ext, int64_t n, int64_t x_stride,
                                                            int64_t e, int32_t padtype, int64_t blocks_per_row) {
  const int64_t row = blockIdx.x / blocks_per_row;
  const int64_t j = (blockIdx.x - row * blocks_per_row) * 256 + threadIdx.x;
  const int64_t m = n + 2 * e;
  if (j >= m) return;
  const float* xr = x + row * x_stride;
  float v;
  if (j >= e && j < e + n) v = xr[j - e];
  else {
    const bool left = j < e;
    const float end = left ? xr[0] : xr[n - 1];
    const float in = left ? xr[e - j] : xr[n - 2 - (j - (e + n))];
    v = padtype == 1 ? (float)(2.0 * (double)end - (double)in) : (padtype == 2 ? in : end);
  }
  ext[row * m + j] = v;
}

// one run of family F's filter over the rows of `a`; scan: the family's tier choice, which F::tables may still turn down
template <class F> int run(Ctx* c, const typename F::Launch& a, bool scan) {
  constexpr int NP = F::NP;
  const int ns = F::states(a);
  const typename F::Coefs cf = F::fill(a);
  Geom g;
  g.n = a.n; g.x_stride = a.x_stride; g.y_stride = a.y_stride; g.out_off = a.out_off; g.out_len = a.out_len;
  g.C = F::chunk(a); g.dir = a.direction; g.batch = a.batch; g.zi_rows = a.zi_rows; g.zi_times_first = a.zi_times_first ? 1 : 0;
  g.tiles = F::tiles(a);
  g.R = iir_tiles_per_lane(g.tiles);
  int rc;
  const void *mcd = nullptr, *mtd = nullptr;
  if (scan) {
    if (g.tiles >= ((int64_t)1 << 31) / a.batch) return set_error(NXSIG_ERR_UNSUPPORTED, F::kTooManyTiles);
    if ((rc = F::tables(c, a, g.R, &mcd, &mtd, &scan))) return rc;
  }

  // one allocation: chunk states P, tile start states, zi rows, zf rows
  const size_t p_elems = scan ? (size_t)a.batch * g.tiles * NP * kLanes : 0;
  const size_t ts_elems = scan ? (size_t)a.batch * g.tiles * NP : 0;
  const bool has_zi = a.zi_host && ns > 0;
  const bool zi_table = has_zi && a.zi_times_first;   // a function of the coefficients: one cached table per filter (F::zi_table)
  const size_t zi_elems = has_zi && !zi_table ? (size_t)a.zi_rows * NP : 0;
  const size_t zf_elems = a.zf_host ? (size_t)a.batch * NP : 0;
  void* base = nullptr;
  if ((rc = ctx_scratch(c, kScratchLongStftFrames, (p_elems + ts_elems + zi_elems + zf_elems + 1) * sizeof(double), &base))) return rc;
  double* P = static_cast<double*>(base);
  double* ts = P + p_elems;
  double* zi_scratch = ts + ts_elems;
  double* zf = a.zf_host ? zi_scratch + zi_elems : nullptr;

  // zi padded to NP states per row; a row with a non-finite entry is NaN throughout, so that output 0 is non-finite already
  const double* zi = nullptr;
  if (has_zi) {
    std::vector<double> padded((size_t)a.zi_rows * NP, 0.0);
    for (int32_t r = 0; r < a.zi_rows; ++r) {
      bool finite = true;
      for (int k = 0; k < ns; ++k) finite = finite && std::isfinite(a.zi_host[(size_t)r * ns + k]);
      for (int k = 0; k < NP; ++k) padded[(size_t)r * NP + k] = finite ? (k < ns ? a.zi_host[(size_t)r * ns + k] : 0.0) : NAN;
    }
    if (zi_table) {
      const void* d = nullptr;
      if ((rc = F::zi_table(c, padded, &d))) return rc;
      zi = static_cast<const double*>(d);
    } else {   // a caller's zi changes from call to call (zf fed back as zi): through the scratch slot, never a cached table
      NXSIG_HIP_TRY(hipMemcpyAsync(zi_scratch, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));   // `padded` goes away
      zi = zi_scratch;
    }
  }

  F::note(scan);
  if (!scan) {
    hipLaunchKernelGGL(k_scan_generic<F>, dim3((unsigned)(((int64_t)a.batch + kLanes - 1) / kLanes)), dim3(kLanes), 0, c->stream, a.x, a.y, cf, zi, zf, g);
    NXSIG_HIP_TRY(hipGetLastError());
  } else {
    const unsigned blocks = (unsigned)(g.tiles * a.batch);
    hipLaunchKernelGGL((k_scan_pass<F, false>), dim3(blocks), dim3(kLanes), 0, c->stream, a.x, static_cast<float*>(nullptr), cf,
                       static_cast<const double*>(mcd), P, static_cast<const double*>(nullptr), static_cast<double*>(nullptr), g);
    NXSIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_scan_carry<F>, dim3((unsigned)a.batch), dim3(kLanes), 0, c->stream, a.x, P, static_cast<const double*>(mtd), zi, ts, g);
    NXSIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_scan_pass<F, true>), dim3(blocks), dim3(kLanes), 0, c->stream, a.x, a.y, cf, static_cast<const double*>(mcd), P,
                       static_cast<const double*>(ts), zf, g);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  if (a.zf_host) {
    std::vector<double> back((size_t)a.batch * NP);
    NXSIG_HIP_TRY(hipMemcpyAsync(back.data(), zf, back.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
    for (int32_t r = 0; r < a.batch; ++r)
      for (int k = 0; k < ns; ++k) a.zf_host[(size_t)r * ns + k] = back[(size_t)r * NP + k];
  }
  return NXSIG_OK;
}

// the run of the kernel instantiated for the family's padded size
template <template <int> class F, class L> int run_padded(Ctx* c, const L& a, int padded, bool scan) {
  switch (padded) {
    case 1: return run<F<1>>(c, a, scan);
    case 2: return run<F<2>>(c, a, scan);
    case 4: return run<F<4>>(c, a, scan);
    case 8: return run<F<8>>(c, a, scan);
    default: return run<F<16>>(c, a, scan);
  }
}

// a forward-backward filter: x rows -> extended rows (padtype 1 odd, 2 even, 3 constant; edge samples each side), forward with
// zi * (the first sample), backward likewise, the middle slice to y (dense [batch][n]).  `a` brings the coefficients and zi (one row)
template <class F>
int forward_backward(Ctx* c, const float* x, int64_t n, int64_t x_stride, int32_t batch, int32_t padtype, int64_t edge, float* y, typename F::Launch a) {
  const int64_t m = n + 2 * edge;
  void* base = nullptr;
  // the extended rows (when there is an edge) and the forward result, both f32 [batch][m]
  int rc = ctx_scratch(c, kScratchFirLong, (size_t)batch * m * sizeof(float) * (edge > 0 ? 2 : 1), &base);
  if (rc) return rc;
  float* fwd = static_cast<float*>(base);
  const float* in = x;
  int64_t in_stride = x_stride;
  if (edge > 0) {
    float* ext = fwd + (size_t)batch * m;
    const int64_t bpr = (m + 255) / 256;
    if (bpr >= ((int64_t)1 << 31) / batch) return set_error(NXSIG_ERR_UNSUPPORTED, F::kTooManyBlocks);
    hipLaunchKernelGGL(k_scan_extend, dim3((unsigned)(bpr * batch)), dim3(256), 0, c->stream, x, ext, n, x_stride, edge, padtype, bpr);
    NXSIG_HIP_TRY(hipGetLastError());
    in = ext; in_stride = m;
  }
  a.x = in; a.n = m; a.x_stride = in_stride; a.batch = batch;
  a.zi_rows = 1; a.zi_times_first = true; a.zf_host = nullptr;
  a.direction = 0; a.y = fwd; a.y_stride = m; a.out_off = 0; a.out_len = m;
  if ((rc = F::launch(c, a))) return rc;
  a.x = fwd; a.x_stride = m; a.direction = 1; a.y = y; a.y_stride = n; a.out_off = edge; a.out_len = n;
  return F::launch(c, a);
}

}  // namespace rscan
}  // namespace nxsig
