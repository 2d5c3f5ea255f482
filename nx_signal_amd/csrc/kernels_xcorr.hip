// Convolution.correlate_rows / convolve_rows: scipy.signal.correlate / convolve on row pairs, row r of one tensor with row r of
// another (or with one shared template), real f32 or c64.  include/nxsig.h states the definition, DESIGN.md section 3.22 the design; the
// argument checks, the tier choice, the transform length P, the index maps, the mirror-bin map, the row scale and the slab arithmetic
// are csrc/xcorr_plan.hpp.  Both tiers form the circular result c = IDFT_P(X conj(Y)) (correlate) or IDFT_P(X Y) (convolve) at
// P = max(1024, next power of two >= n1 + n2 - 1) and hand out the mode's window of it, c[(circ_start + i) mod P].
//   xcorr.wave     n1 + n2 - 1 <= 1024, real pairs up to 2048: one wave per pair on the wave-private cores, in czt.wave's layout, LDS
//                  budget and rows-per-wave geometry; the next pair's loads are in flight during the butterflies.  A real pair is packed
//                  as z = x + i y (each row first scaled by a power of two into [0.5, 1), undone at the sink) into one wave_fft_core_T;
//                  bin K - k comes through the wave's LDS strip; the product, the optional PHAT (one wave max-reduction), the unscaled
//                  inverse core, and the sink: 8 / 16-byte stores of two adjacent results (element by element where a row starts off
//                  the wide boundary) or a wave argmax.  A c64 pair takes two forward cores; at 2048 points the two spectra do not fit
//                  the register file, so those pairs are xcorr.generic's
//   xcorr.generic  everything else and everything under NXSIG_XCORR_WAVE=0 / NXSIG_DISABLE_WAVE: pad both operands into dense c64 rows
//                  (a shared template once per call), launch_fft forward on both, the product (PHAT: one workgroup per pair, after
//                  its maximum), launch_fft inverse, a sink kernel (the window, or one workgroup's argmax per pair).  The batch runs in
//                  slabs so that the four temporaries (Ctx::xcorr_a, _b, _sa, _sb) stay within kXcorrSlabBytes
// Non-finite rule, the same in both tiers: bin 0 of a forward transform is the sum of the samples, so it is not finite when a sample
// is not; such a pair's cross spectrum is replaced by NaN before the inverse and the pair leaves without a finite element (peak sink:
// value NaN, lag 0).  No atomics; a pair's bits depend neither on the batch nor on its neighbours in a wave or slab.
#include "wave_stft.hpp"

namespace nxsig {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool xc_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ float xc_qnan() { return __uint_as_float(0x7fc00000u); }
// the modulus the peak sink ranks c64 results by (include/nxsig.h): the f32 rounding of sqrt(re^2 + im^2) evaluated in double
__device__ __forceinline__ float xc_modulus(float re, float im) { return (float)sqrt((double)re * (double)re + (double)im * (double)im); }
// np.argmax's order: the larger key, the smaller index among equals
__device__ __forceinline__ bool xc_better(float key, int idx, float best_key, int best_idx) {
  return key > best_key || (key == best_key && idx < best_idx);
}
__device__ __forceinline__ float xc_lane0(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

struct XcWaveArgs {
  const void* a;
  const void* b;
  int64_t a_stride, b_stride, rows, chunk;   // chunk: pairs per workgroup
  int32_t n1, n2, n_out, circ_start, first_lag;
  int32_t correlate, phat, peak;
  float floor;
  const v2f* twB;
  const v2f* twC;
  void* out;
  int32_t* lags;
};

template <int K, int W, bool CPLX>
__global__ __launch_bounds__(64 * W) void k_xcorr_wave(XcWaveArgs a) {
  constexpr int P = K / 64, R3 = K / 256, NQ = K / 128, XCH = K + K / 16 + 16, LOGK = K == 1024 ? 10 : 11;
  typedef typename std::conditional<CPLX, v4f, v2f>::type pair_t;   // two adjacent samples
  typedef typename std::conditional<CPLX, v2f, float>::type elem_t;
  v2f* s_twB = reinterpret_cast<v2f*>(g_wave_smem);
  v2f* s_twC = s_twB + 256;
  v2f* s_x = s_twC + R3 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 256; i += 64 * W) s_twB[i] = a.twB[i];
  for (int i = tid; i < R3 * 256; i += 64 * W) s_twC[i] = a.twC[i];
  __syncthreads();
  v2f* xb = s_x + wave * XCH;
  const int64_t r_begin = (int64_t)blockIdx.x * a.chunk;
  int64_t r_end = r_begin + a.chunk;
  if (r_end > a.rows) r_end = a.rows;
  pair_t na[NQ], nb[NQ];   // n?[q] = (row[i0], row[i0 + 1]), i0 = 2 lane + 128 q; zero at and past the row's length
  auto load = [&](const void* base, int64_t stride, int64_t r, int n, pair_t* dst) {
    const elem_t* row = static_cast<const elem_t*>(base) + (size_t)r * stride;
    const bool wide = czt_wide(reinterpret_cast<uintptr_t>(row), (int)sizeof(elem_t));   // wave-uniform: a row may start at any element
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i0 = czt_slot_sample(lane, q), st = czt_pair_state(i0, n);
      if constexpr (CPLX) {
        v4f v = v4f{0.f, 0.f, 0.f, 0.f};
        if (wide) {
          if (st == 2) v = *reinterpret_cast<const v4f*>(row + i0);
          else if (st == 1) { const v2f t = row[i0]; v.x = t.x; v.y = t.y; }
        } else {
          if (st >= 1) { const v2f t = row[i0]; v.x = t.x; v.y = t.y; }
          if (st == 2) { const v2f t = row[i0 + 1]; v.z = t.x; v.w = t.y; }
        }
        dst[q] = v;
      } else {
        v2f v = v2f{0.f, 0.f};
        if (wide) {
          if (st == 2) v = *reinterpret_cast<const v2f*>(row + i0);
          else if (st == 1) v.x = row[i0];
        } else {
          if (st >= 1) v.x = row[i0];
          if (st == 2) v.y = row[i0 + 1];
        }
        dst[q] = v;
      }
    }
  };
  auto issue = [&](int64_t r) {
    load(a.a, a.a_stride, r, a.n1, na);
    load(a.b, a.b_stride, r, a.n2, nb);
  };
  if (r_begin + wave < r_end) issue(r_begin + wave);
  for (int64_t r = r_begin + wave; r < r_end; r += W) {
    v2f d[P];        // the cross spectrum: d[s] = R[lane + 64 s]
    int shift = -LOGK;   // the result is u 2^shift: the inverse core's 1 / K and, for a packed pair, the two row scales undone
    bool poisoned;
    if constexpr (CPLX) {
      v2f zz[2][NQ], da[P];
#pragma unroll
      for (int q = 0; q < NQ; ++q) { zz[0][q] = v2f{na[q].x, na[q].y}; zz[1][q] = v2f{na[q].z, na[q].w}; }
      wave_fft_core_T<K>(zz, da, xb, s_twB, s_twC, lane);
#pragma unroll
      for (int q = 0; q < NQ; ++q) { zz[0][q] = v2f{nb[q].x, nb[q].y}; zz[1][q] = v2f{nb[q].z, nb[q].w}; }
      issue(r + W < r_end ? r + W : r);   // unconditional prefetch (the last iteration re-reads its own pair)
      __builtin_amdgcn_sched_barrier(0);
      wave_fft_core_T<K>(zz, d, xb, s_twB, s_twC, lane);
      // lane 0 holds bin 0 of either transform, the sum of the samples, in register 0: not finite when a sample is not
      poisoned = xc_nonfinite(xc_lane0(da[0].x)) || xc_nonfinite(xc_lane0(da[0].y)) || xc_nonfinite(xc_lane0(d[0].x)) || xc_nonfinite(xc_lane0(d[0].y));
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = a.correlate ? wcmul_conj(da[s], d[s]) : wcmul(da[s], d[s]);
    } else {
      // each row's largest magnitude (the IEEE bits order as the magnitudes do; Inf and NaN sort last), one wave reduction per operand
      uint32_t ma = 0, mb = 0;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const uint32_t a0 = __float_as_uint(na[q].x) & 0x7fffffffu, a1 = __float_as_uint(na[q].y) & 0x7fffffffu;
        const uint32_t b0 = __float_as_uint(nb[q].x) & 0x7fffffffu, b1 = __float_as_uint(nb[q].y) & 0x7fffffffu;
        ma = max(ma, max(a0, a1)); mb = max(mb, max(b0, b1));
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) { ma = max(ma, (uint32_t)__shfl_xor((int)ma, off)); mb = max(mb, (uint32_t)__shfl_xor((int)mb, off)); }
      const int ea = xcorr_scale_exponent(ma), eb = xcorr_scale_exponent(mb);
      if (!a.phat) shift += ea + eb;   // the PHAT spectrum does not change with the scale of the operands
      v2f zz[2][NQ];   // z = x 2^-ea + i y 2^-eb
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        zz[0][q] = v2f{ldexpf(na[q].x, -ea), ldexpf(nb[q].x, -eb)};
        zz[1][q] = v2f{ldexpf(na[q].y, -ea), ldexpf(nb[q].y, -eb)};
      }
      issue(r + W < r_end ? r + W : r);   // unconditional prefetch (the last iteration re-reads its own pair)
      __builtin_amdgcn_sched_barrier(0);
      wave_fft_core_T<K>(zz, d, xb, s_twB, s_twC, lane);   // d[s] = Z[lane + 64 s]
      // lane 0 holds bin 0, sum x + i sum y, in register 0: not finite when a sample of either row is not
      poisoned = xc_nonfinite(xc_lane0(d[0].x)) || xc_nonfinite(xc_lane0(d[0].y));
      // the split: bin K - k lives in lane xcorr_mirror_lane, register xcorr_mirror_reg; it comes through the wave's LDS strip
#pragma unroll
      for (int s = 0; s < P; ++s) xb[czt_bin(lane, s)] = d[s];
      wave_lds_fence();
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const v2f z = d[s], m = xb[xcorr_mirror_bin(czt_bin(lane, s), K)];
        const v2f X = v2f{0.5f * (z.x + m.x), 0.5f * (z.y - m.y)};    // (Z + conj Zm) / 2
        const v2f Y = v2f{0.5f * (z.y + m.y), -0.5f * (z.x - m.x)};   // (Z - conj Zm) / 2i
        d[s] = a.correlate ? wcmul_conj(X, Y) : wcmul(X, Y);
      }
      wave_lds_fence();   // every mirror read is issued before the inverse core writes the strip
      // an all-zero row: its recovered spectrum is the rounding of the other row's, not zero; the pair's result is exact zeros (wave-uniform)
      if (ma == 0 || mb == 0) {
#pragma unroll
        for (int s = 0; s < P; ++s) d[s] = v2f{0.f, 0.f};
      }
    }
    if (a.phat) {   // wave-uniform
      // G does not change with the scale of R: R is first brought under 1 by a power of two, so that no |R|^2 overflows (c64 operands
      // near 1e10 would) or vanishes
      float mc = 0.f;
#pragma unroll
      for (int s = 0; s < P; ++s) mc = fmaxf(mc, fmaxf(fabsf(d[s].x), fabsf(d[s].y)));
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) mc = fmaxf(mc, __shfl_xor(mc, off));
      const int er = xcorr_scale_exponent(__float_as_uint(mc));
      float mx = 0.f;
#pragma unroll
      for (int s = 0; s < P; ++s) {
        d[s] = v2f{ldexpf(d[s].x, -er), ldexpf(d[s].y, -er)};
        mx = fmaxf(mx, d[s].x * d[s].x + d[s].y * d[s].y);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float thr = a.floor * sqrtf(mx);
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const float den = fmaxf(sqrtf(d[s].x * d[s].x + d[s].y * d[s].y), thr);
        d[s] = den > 0.f ? v2f{d[s].x / den, d[s].y / den} : v2f{0.f, 0.f};
      }
    }
    if (poisoned) {
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = v2f{xc_qnan(), xc_qnan()};
    }
    v2f u[2][NQ];
    wave_fft_core<K, true, true>(d, u, xb, s_twB, s_twC, lane);   // unscaled inverse: u[par][q] = c[2 lane + par + 128 q]
    __builtin_amdgcn_sched_barrier(0);
    const float scale = ldexpf(1.0f, -LOGK);
    auto value = [&](v2f v) -> elem_t {
      if constexpr (CPLX) return v2f{v.x * scale, v.y * scale};
      else return ldexpf(v.x, shift);
    };
    if (!a.peak) {
      elem_t* orow = static_cast<elem_t*>(a.out) + (size_t)r * a.n_out;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i0 = (int)xcorr_out_index(a.circ_start, czt_slot_sample(lane, q), K), i1 = (i0 + 1) & (K - 1);
        const int st = xcorr_store_state(i0, i1, a.n_out);
        if (st == 0) continue;
        const elem_t y0 = value(u[0][q]), y1 = value(u[1][q]);
        if ((st & 4) && czt_wide(reinterpret_cast<uintptr_t>(orow + i0), (int)sizeof(elem_t))) {
          if constexpr (CPLX) __builtin_nontemporal_store(v4f{y0.x, y0.y, y1.x, y1.y}, (gv4f*)(orow + i0));
          else __builtin_nontemporal_store(v2f{y0, y1}, (gv2f*)(orow + i0));
        } else {
          if (st & 1) orow[i0] = y0;
          if (st & 2) orow[i1] = y1;
        }
      }
    } else {
      // the first maximum of the window in lag order: every lane ranks its own elements, the wave the lanes; the owner stores
      float best = -INFINITY;
      int best_i = 0x7fffffff;
      elem_t best_v = value(v2f{0.f, 0.f});
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int par = 0; par < 2; ++par) {
          const int i = (int)xcorr_out_index(a.circ_start, czt_slot_sample(lane, q) + par, K);
          if (i >= a.n_out) continue;
          const elem_t y = value(u[par][q]);
          float key;
          if constexpr (CPLX) key = xc_modulus(y.x, y.y);
          else key = y;
          if (xc_better(key, i, best, best_i)) { best = key; best_i = i; best_v = y; }
        }
      }
      float wbest = best;
      int wbest_i = best_i;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ok = __shfl_xor(wbest, off);
        const int oi = __shfl_xor(wbest_i, off);
        if (xc_better(ok, oi, wbest, wbest_i)) { wbest = ok; wbest_i = oi; }
      }
      elem_t* o = static_cast<elem_t*>(a.out) + r;
      if (poisoned) {
        if (lane == 0) {
          if constexpr (CPLX) *o = v2f{xc_qnan(), xc_qnan()};
          else *o = xc_qnan();
          a.lags[r] = 0;
        }
      } else if (wbest_i == 0x7fffffff) {   // no element ranks: the window is NaN throughout (a product that overflowed to Inf - Inf)
        if (lane == 0) {
          if constexpr (CPLX) *o = v2f{xc_qnan(), xc_qnan()};
          else *o = xc_qnan();
          a.lags[r] = 0;
        }
      } else if (best_i == wbest_i) {   // an index belongs to one lane
        *o = best_v;
        a.lags[r] = a.first_lag + best_i;
      }
    }
  }
}

template <int K, bool CPLX>
int run_wave(Ctx* c, const XcorrLaunch& l) {
  constexpr int W = K == 2048 ? 2 : 4;
  int rc = ensure_wave_tables(c, K);
  if (rc) return rc;
  Ctx::WaveTables& wt = c->wave_tables[K];
  XcWaveArgs w;
  w.a = l.a; w.b = l.b; w.a_stride = l.a_stride; w.b_stride = l.b_stride; w.rows = l.batch;
  w.n1 = (int32_t)l.n1; w.n2 = (int32_t)l.n2; w.n_out = (int32_t)xcorr_out_length(l.n1, l.n2, l.mode);
  w.circ_start = (int32_t)xcorr_circ_start(l.n1, l.n2, l.op, l.mode, K); w.first_lag = (int32_t)xcorr_first_lag(l.n1, l.n2, l.mode);
  w.correlate = l.op == kXcCorrelate; w.phat = l.weighting == kXcPhat; w.peak = l.sink == kXcPeak; w.floor = l.phat_floor;
  w.twB = reinterpret_cast<const v2f*>(wt.twB); w.twC = reinterpret_cast<const v2f*>(wt.twC);
  w.out = l.out; w.lags = l.out_lags;
  const int rpw = tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, l.batch, W, 4);
  w.chunk = (int64_t)W * (rpw < 1 ? 1 : rpw);
  const int64_t blocks = czt_blocks(l.batch, w.chunk);
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "xcorr: too many rows for one launch");
  dispatch_note("xcorr.wave");
  hipLaunchKernelGGL((k_xcorr_wave<K, W, CPLX>), dim3((unsigned)blocks), dim3(64 * W), (size_t)czt_lds_bytes(K), c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

// ---- xcorr.generic
// rows `stride` elements apart -> dense zero-padded c64 [rows][P]; nothing at or past n is read
template <bool CPLX>
__global__ __launch_bounds__(kThreads) void k_xc_pad(const void* __restrict__ x, int64_t stride, int64_t rows, int64_t n, int64_t P,
                                                    float2* __restrict__ out) {
  const int64_t total = rows * P;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / P, j = i - r * P;
    float2 v = make_float2(0.f, 0.f);
    if (j < n) {
      if (CPLX) v = static_cast<const float2*>(x)[(size_t)r * stride + j];
      else v.x = static_cast<const float*>(x)[(size_t)r * stride + j];
    }
    out[i] = v;
  }
}

__device__ __forceinline__ float2 xc_product(float2 x, float2 y, int correlate) {
  return correlate ? make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y) : make_float2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x);
}
__device__ __forceinline__ bool xc_poisoned(const float2* __restrict__ sa, const float2* __restrict__ sb, int64_t r, int64_t b_rows, int64_t P) {
  const float2 a0 = sa[(size_t)r * P], b0 = sb[(size_t)r * b_rows];
  return xc_nonfinite(a0.x) || xc_nonfinite(a0.y) || xc_nonfinite(b0.x) || xc_nonfinite(b0.y);
}

// out[r][k] = X[r][k] conj(Y[r][k]) (correlate) or X[r][k] Y[r][k]; b_rows: P, or 0 for a shared template.  A pair whose bin 0 of either
// spectrum is not finite becomes NaN throughout.  Out of place: every lane of a row reads its bins 0
__global__ __launch_bounds__(kThreads) void k_xc_mul(const float2* __restrict__ sa, const float2* __restrict__ sb, int64_t b_rows, int64_t rows,
                                                    int64_t P, int correlate, float2* __restrict__ out) {
  const int64_t total = rows * P;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / P, k = i - r * P;
    if (xc_poisoned(sa, sb, r, b_rows, P)) { out[i] = make_float2(xc_qnan(), xc_qnan()); continue; }
    out[i] = xc_product(sa[i], sb[(size_t)r * b_rows + k], correlate);
  }
}

// the largest value of a workgroup, handed to every lane (s_cells: kThreads floats, free again on return)
__device__ __forceinline__ float xc_block_max(float v, float* s_cells) {
  s_cells[threadIdx.x] = v;
  __syncthreads();
  for (int w = kThreads / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s_cells[threadIdx.x] = fmaxf(s_cells[threadIdx.x], s_cells[threadIdx.x + w]);
    __syncthreads();
  }
  const float top = s_cells[0];
  __syncthreads();
  return top;
}

// the PHAT product, one workgroup per pair at a time: R into out with its largest component, which gives the power of two that brings
// R under 1 (G does not change with the scale of R, and no |R|^2 overflows or vanishes then); the largest |R|; then
// G = R / max(|R|, floor max|R|) (0 where the denominator is 0).  A lane reads back only what it wrote itself
__global__ __launch_bounds__(kThreads) void k_xc_phat(const float2* __restrict__ sa, const float2* __restrict__ sb, int64_t b_rows, int64_t rows,
                                                     int64_t P, float floor, float2* __restrict__ out) {
  __shared__ float s_max[kThreads];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    float2* o = out + (size_t)r * P;
    if (xc_poisoned(sa, sb, r, b_rows, P)) {   // workgroup-uniform
      for (int64_t k = threadIdx.x; k < P; k += kThreads) o[k] = make_float2(xc_qnan(), xc_qnan());
      continue;
    }
    float mc = 0.f;
    for (int64_t k = threadIdx.x; k < P; k += kThreads) {
      const float2 v = xc_product(sa[(size_t)r * P + k], sb[(size_t)r * b_rows + k], 1);
      o[k] = v;
      mc = fmaxf(mc, fmaxf(fabsf(v.x), fabsf(v.y)));
    }
    const int er = xcorr_scale_exponent(__float_as_uint(xc_block_max(mc, s_max)));
    float mx = 0.f;
    for (int64_t k = threadIdx.x; k < P; k += kThreads) {
      const float2 v = make_float2(ldexpf(o[k].x, -er), ldexpf(o[k].y, -er));
      o[k] = v;
      mx = fmaxf(mx, v.x * v.x + v.y * v.y);
    }
    const float thr = floor * sqrtf(xc_block_max(mx, s_max));
    for (int64_t k = threadIdx.x; k < P; k += kThreads) {
      const float2 v = o[k];
      const float den = fmaxf(sqrtf(v.x * v.x + v.y * v.y), thr);
      o[k] = den > 0.f ? make_float2(v.x / den, v.y / den) : make_float2(0.f, 0.f);
    }
  }
}

// the mode's window of the circular result [rows][P] -> the result [rows][n_out]; the real part for real pairs
template <bool CPLX>
__global__ __launch_bounds__(kThreads) void k_xc_rows(const float2* __restrict__ cc, int64_t rows, int64_t P, int64_t n_out, int64_t circ_start,
                                                     void* __restrict__ out) {
  const int64_t total = rows * n_out;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / n_out, k = i - r * n_out;
    const float2 v = cc[(size_t)r * P + xcorr_circ_index(circ_start, k, P)];
    if (CPLX) static_cast<float2*>(out)[i] = v;
    else static_cast<float*>(out)[i] = v.x;
  }
}

// the peak sink, one workgroup per pair at a time: the first maximum of the window in lag order
template <bool CPLX>
__global__ __launch_bounds__(kThreads) void k_xc_peak(const float2* __restrict__ cc, int64_t rows, int64_t P, int64_t n_out, int64_t circ_start,
                                                     int32_t first_lag, void* __restrict__ out, int32_t* __restrict__ lags) {
  __shared__ float s_key[kThreads];
  __shared__ int s_idx[kThreads];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const float2* row = cc + (size_t)r * P;
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int64_t k = threadIdx.x; k < n_out; k += kThreads) {
      const float2 v = row[xcorr_circ_index(circ_start, k, P)];
      const float key = CPLX ? xc_modulus(v.x, v.y) : v.x;
      if (xc_better(key, (int)k, best, best_i)) { best = key; best_i = (int)k; }
    }
    s_key[threadIdx.x] = best; s_idx[threadIdx.x] = best_i;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) {
      if ((int)threadIdx.x < w && xc_better(s_key[threadIdx.x + w], s_idx[threadIdx.x + w], s_key[threadIdx.x], s_idx[threadIdx.x])) {
        s_key[threadIdx.x] = s_key[threadIdx.x + w]; s_idx[threadIdx.x] = s_idx[threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const int at = s_idx[0];
      // a poisoned pair is NaN throughout: no element ranks, or (real pairs) none compares
      const float2 first = row[xcorr_circ_index(circ_start, 0, P)];
      const bool poisoned = at == 0x7fffffff || first.x != first.x || first.y != first.y;
      const float2 v = poisoned ? make_float2(xc_qnan(), xc_qnan()) : row[xcorr_circ_index(circ_start, at, P)];
      if (CPLX) static_cast<float2*>(out)[r] = v;
      else static_cast<float*>(out)[r] = v.x;
      lags[r] = poisoned ? 0 : first_lag + at;
    }
    __syncthreads();   // the cells are written again for the next pair
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}
unsigned row_blocks(const Ctx* c, int64_t rows) {
  const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 8;
  return (unsigned)(rows < cap ? (rows < 1 ? 1 : rows) : cap);
}

// one of the tier's own temporaries, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does)
int own_buffer(Ctx* c, Ctx::OwnedBuffer& b, size_t bytes, float2** out) {
  if (b.bytes < bytes) {
    if (b.ptr) {
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      NXSIG_HIP_TRY(hipFree(b.ptr));
      b.ptr = nullptr; b.bytes = 0;
    }
    NXSIG_HIP_TRY(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
  }
  *out = static_cast<float2*>(b.ptr);
  return NXSIG_OK;
}

int pad_and_transform(Ctx* c, bool is_complex, const void* x, int64_t stride, int64_t rows, int64_t n, int64_t P, float2* padded, float2* spectra) {
  if (is_complex) hipLaunchKernelGGL(k_xc_pad<true>, dim3(stream_blocks(c, rows * P)), dim3(kThreads), 0, c->stream, x, stride, rows, n, P, padded);
  else hipLaunchKernelGGL(k_xc_pad<false>, dim3(stream_blocks(c, rows * P)), dim3(kThreads), 0, c->stream, x, stride, rows, n, P, padded);
  NXSIG_HIP_TRY(hipGetLastError());
  return launch_fft(c, padded, false, rows, (int32_t)P, (int32_t)P, false, spectra, false);
}

int run_generic(Ctx* c, const XcorrLaunch& l) {
  const int64_t P = xcorr_fft_length(l.n1, l.n2), n_out = xcorr_out_length(l.n1, l.n2, l.mode);
  const int64_t circ_start = xcorr_circ_start(l.n1, l.n2, l.op, l.mode, P), first_lag = xcorr_first_lag(l.n1, l.n2, l.mode);
  const int64_t slab = xcorr_slab_rows(l.batch, P, tune(c, kT_XCORR_SLAB_ROWS, 0));
  const bool shared = l.b_stride == 0, correlate = l.op == kXcCorrelate;
  const size_t es = l.is_complex ? sizeof(float2) : sizeof(float), bytes = (size_t)slab * P * sizeof(float2);
  float2 *A = nullptr, *B = nullptr, *SA = nullptr, *SB = nullptr;
  int rc;
  if ((rc = own_buffer(c, c->xcorr_a, bytes, &A))) return rc;
  if ((rc = own_buffer(c, c->xcorr_sa, bytes, &SA))) return rc;
  if ((rc = own_buffer(c, c->xcorr_b, shared ? (size_t)P * sizeof(float2) : bytes, &B))) return rc;
  if ((rc = own_buffer(c, c->xcorr_sb, shared ? (size_t)P * sizeof(float2) : bytes, &SB))) return rc;
  dispatch_note("xcorr.generic");
  if (shared && (rc = pad_and_transform(c, l.is_complex, l.b, l.n2, 1, l.n2, P, B, SB))) return rc;   // a shared template: once per call
  for (int64_t r0 = 0; r0 < l.batch; r0 += slab) {
    const int64_t rows = l.batch - r0 < slab ? l.batch - r0 : slab;
    if ((rc = pad_and_transform(c, l.is_complex, static_cast<const char*>(l.a) + (size_t)r0 * l.a_stride * es, l.a_stride, rows, l.n1, P, A, SA))) return rc;
    if (!shared && (rc = pad_and_transform(c, l.is_complex, static_cast<const char*>(l.b) + (size_t)r0 * l.b_stride * es, l.b_stride, rows, l.n2, P, B, SB)))
      return rc;
    if (l.weighting == kXcPhat) hipLaunchKernelGGL(k_xc_phat, dim3(row_blocks(c, rows)), dim3(kThreads), 0, c->stream, SA, SB, shared ? 0 : P, rows, P, l.phat_floor, A);
    else hipLaunchKernelGGL(k_xc_mul, dim3(stream_blocks(c, rows * P)), dim3(kThreads), 0, c->stream, SA, SB, shared ? 0 : P, rows, P, (int)correlate, A);
    NXSIG_HIP_TRY(hipGetLastError());
    if ((rc = launch_fft(c, A, false, rows, (int32_t)P, (int32_t)P, true, SA, false))) return rc;   // with its 1 / P
    if (l.sink == kXcPeak) {
      void* o = static_cast<char*>(l.out) + (size_t)r0 * es;
      if (l.is_complex) hipLaunchKernelGGL(k_xc_peak<true>, dim3(row_blocks(c, rows)), dim3(kThreads), 0, c->stream, SA, rows, P, n_out, circ_start, (int32_t)first_lag, o, l.out_lags + r0);
      else hipLaunchKernelGGL(k_xc_peak<false>, dim3(row_blocks(c, rows)), dim3(kThreads), 0, c->stream, SA, rows, P, n_out, circ_start, (int32_t)first_lag, o, l.out_lags + r0);
    } else {
      void* o = static_cast<char*>(l.out) + (size_t)r0 * n_out * es;
      if (l.is_complex) hipLaunchKernelGGL(k_xc_rows<true>, dim3(stream_blocks(c, rows * n_out)), dim3(kThreads), 0, c->stream, SA, rows, P, n_out, circ_start, o);
      else hipLaunchKernelGGL(k_xc_rows<false>, dim3(stream_blocks(c, rows * n_out)), dim3(kThreads), 0, c->stream, SA, rows, P, n_out, circ_start, o);
    }
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_xcorr(Ctx* c, const XcorrLaunch& l) {
  if (l.batch == 0) return NXSIG_OK;
  const bool wave_off = tune(c, kT_XCORR_WAVE, 1) == 0 || tune(c, kT_DISABLE_WAVE, 0) != 0;
  if (xcorr_tier(l.n1, l.n2, l.is_complex, wave_off) == kXcGeneric) return run_generic(c, l);
  if (xcorr_fft_length(l.n1, l.n2) == 1024) return l.is_complex ? run_wave<1024, true>(c, l) : run_wave<1024, false>(c, l);
  return run_wave<2048, false>(c, l);
}

}  // namespace nxsig
