// Filters.hilbert: the analytic signal a = IDFT_N(h DFT_N(row)) of real f32 rows, its magnitude (the envelope) or its imaginary part
// (the Hilbert transform proper).  include/nxsig.h states the definition, DESIGN.md section 3.16 the design; the multiplier rule, the
// tier choice and the lane arithmetic are csrc/hilbert_plan.hpp.
//   hilbert.wave     N = 1024, 2048: one wave per row on the wave-private cores.  8-byte loads in the layout wave_fft_core produces
//                    (zero beyond the samples the row provides), wave_fft_core_T, the gain as a condition on the register index with
//                    1 / N folded in, the unscaled inverse core, and the sink: 16-byte stores of two adjacent c64, or 8-byte stores of
//                    two adjacent f32.  The row is read once and the result written once: 4 + 8 (4 + 4) bytes per sample
//   hilbert.generic  every other N and everything under NXSIG_DISABLE_HILBERT_WAVE: launch_fft into kScratchFusedSpectrum, the gain in
//                    place, launch_fft back — straight into the result only for the analytic signal of a ZERO-PADDED row (L < N); every
//                    row that fills the transform (L >= N, truncated ones included) is centred, and it and every f32 output go into
//                    kScratchIstftProduct and through an elementwise sink.  Bluestein and the four-step rows come with launch_fft
// Centring, the same in both tiers: a row that fills the transform (no zero padding) is transformed as row - c, c its mean, and c is
// added back to the real part afterwards.  Algebraically nothing changes — only X[0] moves, and h[0] = 1 — but a plain single-precision
// transform of a 1000 + N(0, 1) row leaves 6e-5 of max|Im a| in the imaginary part; centred, the error scales with the variation.
// Non-finite rule, the same in both tiers: bin 0 of the forward transform is the sum of the row's samples, so it is not finite when a
// sample is not; such a row's spectrum is replaced by NaN before the inverse transform and the row leaves without a finite element.
// No atomics.
#include "wave_stft.hpp"

namespace nxsig {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool hb_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
// |a| of the envelope: the expression of launch_mag_from_spectrum's kind "magnitude"
__device__ __forceinline__ float hb_mag(float re, float im) { return sqrtf(re * re + im * im); }

struct HilbertWaveArgs {
  const float* x;
  int64_t x_stride, rows, chunk;   // chunk: rows per workgroup
  int32_t n_used, kind;
  const v2f* twB;
  const v2f* twC;
  void* out;
};

template <int K, int W>
__global__ __launch_bounds__(64 * W) void k_hilbert_wave(HilbertWaveArgs a) {
  constexpr int P = K / 64, R3 = K / 256, NQ = K / 128, XCH = K + K / 16 + 16;
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
  // the result rows are K elements apart, so every row shares the alignment of the base (wave-uniform)
  const bool out16 = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0, out8 = (reinterpret_cast<uintptr_t>(a.out) & 7) == 0;
  const bool centre = a.n_used == K;   // no zero padding
  v2f nx[NQ];   // nx[q] = (x[i0], x[i0 + 1]), i0 = 2 lane + 128 q; zero at and past n_used
  auto issue = [&](int64_t r) {
    const float* row = a.x + (size_t)r * a.x_stride;
    const bool al8 = (reinterpret_cast<uintptr_t>(row) & 7) == 0;   // wave-uniform: a row may start at any 4-byte address
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i0 = hilbert_slot_sample(lane, q), st = hilbert_pair_state(i0, a.n_used);
      v2f v = v2f{0.f, 0.f};
      if (al8) {
        if (st == 2) v = *reinterpret_cast<const v2f*>(row + i0);
        else if (st == 1) v.x = row[i0];
      } else {
        if (st >= 1) v.x = row[i0];
        if (st == 2) v.y = row[i0 + 1];
      }
      nx[q] = v;
    }
  };
  if (r_begin + wave < r_end) issue(r_begin + wave);
  for (int64_t r = r_begin + wave; r < r_end; r += W) {
    // a row that fills the transform is transformed as row - c, c its mean as f32 sums give it, and c goes back into the real part at
    // the sink: the same a (only X[0] changes, and h[0] = 1), but the rounding of both transforms then scales with the row's variation
    float c0 = 0.0f;
    if (centre) {
      float sum = 0.0f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) sum += nx[q].x + nx[q].y;
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      c0 = sum * (1.0f / (float)K);
    }
    v2f zz[2][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { zz[0][q] = v2f{nx[q].x - c0, 0.f}; zz[1][q] = v2f{nx[q].y - c0, 0.f}; }
    issue(r + W < r_end ? r + W : r);   // unconditional prefetch (the last iteration re-reads its own row)
    __builtin_amdgcn_sched_barrier(0);
    v2f d[P];
    wave_fft_core_T<K>(zz, d, xb, s_twB, s_twC, lane);   // d[s] = X[lane + 64 s]
    // lane 0 holds X[0], the sum of the samples, in register 0: not finite when a sample is not
    const float x0r = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(d[0].x)));
    const float x0i = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(d[0].y)));
    const bool poisoned = hb_nonfinite(x0r) || hb_nonfinite(x0i);   // wave-uniform
    constexpr float g1 = 1.0f / (float)K, g2 = 2.0f / (float)K;      // the gain with the inverse transform's 1 / N (exact)
#pragma unroll
    for (int s = 0; s < P; ++s) {
      if (s < P / 2) d[s] = d[s] * ((s == 0 && lane == 0) ? g1 : g2);
      else if (s == P / 2) d[s] = lane == 0 ? d[s] * g1 : v2f{0.f, 0.f};
      else d[s] = v2f{0.f, 0.f};
    }
    if (poisoned) {
      const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = v2f{qnan, qnan};
    }
    v2f u[2][NQ];
    wave_fft_core<K, true, true>(d, u, xb, s_twB, s_twC, lane);   // unscaled inverse: u[par][q] = a[2 lane + par + 128 q]
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) { u[0][q].x += c0; u[1][q].x += c0; }
    if (a.kind == kHbAnalytic) {
      v2f* orow = static_cast<v2f*>(a.out) + (size_t)r * K + 2 * lane;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (out16) __builtin_nontemporal_store(v4f{u[0][q].x, u[0][q].y, u[1][q].x, u[1][q].y}, (gv4f*)(orow + 128 * q));
        else { orow[128 * q] = u[0][q]; orow[128 * q + 1] = u[1][q]; }
      }
    } else {
      float* orow = static_cast<float*>(a.out) + (size_t)r * K + 2 * lane;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const v2f o = a.kind == kHbEnvelope ? v2f{hb_mag(u[0][q].x, u[0][q].y), hb_mag(u[1][q].x, u[1][q].y)} : v2f{u[0][q].y, u[1][q].y};
        if (out8) __builtin_nontemporal_store(o, reinterpret_cast<v2f*>(orow + 128 * q));
        else { orow[128 * q] = o.x; orow[128 * q + 1] = o.y; }
      }
    }
  }
}

template <int K>
int run_wave(Ctx* c, const HilbertLaunch& a) {
  constexpr int W = K == 2048 ? 2 : 4;
  int rc = ensure_wave_tables(c, K);
  if (rc) return rc;
  Ctx::WaveTables& wt = c->wave_tables[K];
  HilbertWaveArgs w;
  w.x = a.x; w.x_stride = a.x_stride; w.rows = a.batch;
  w.n_used = (int32_t)hilbert_used(a.length, K); w.kind = a.kind;
  w.twB = reinterpret_cast<const v2f*>(wt.twB); w.twC = reinterpret_cast<const v2f*>(wt.twC);
  w.out = a.out;
  const int rpw = tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, a.batch, W, 4);
  w.chunk = (int64_t)W * (rpw < 1 ? 1 : rpw);
  const int64_t blocks = hilbert_blocks(a.batch, w.chunk);
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "hilbert: too many rows for one launch");
  dispatch_note("hilbert.wave");
  hipLaunchKernelGGL((k_hilbert_wave<K, W>), dim3((unsigned)blocks), dim3(64 * W), (size_t)hilbert_lds_bytes(K), c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

// ---- hilbert.generic
// rows x_stride apart -> dense [rows][n_used], one workgroup per row.  means != nullptr (a row that fills the transform): the row
// leaves as row - c, c its mean as f32 sums give it, and c is kept for the sink (see k_hilbert_wave)
__global__ __launch_bounds__(kThreads) void k_hilbert_rows(const float* __restrict__ x, int64_t x_stride, int64_t n_used, float* __restrict__ out,
                                                          float* __restrict__ means) {
  __shared__ float s_part[kThreads / 64];
  const float* row = x + (size_t)blockIdx.x * x_stride;
  float* orow = out + (size_t)blockIdx.x * n_used;
  float c0 = 0.0f;
  if (means) {
    float sum = 0.0f;
    for (int64_t i = threadIdx.x; i < n_used; i += kThreads) sum += row[i];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    sum = 0.0f;
    for (int w = 0; w < kThreads / 64; ++w) sum += s_part[w];
    c0 = sum / (float)n_used;
    if (threadIdx.x == 0) means[blockIdx.x] = c0;
  }
  for (int64_t i = threadIdx.x; i < n_used; i += kThreads) orow[i] = row[i] - c0;
}

// z[r][k] *= h[k] in place (gains 0, 1, 2: exact); a row whose bin 0 is not finite becomes NaN throughout.  Bin 0 itself is written
// only in that case, and stays non-finite for every reader either way
__global__ __launch_bounds__(kThreads) void k_hilbert_gain(float2* __restrict__ z, int64_t rows, int64_t N) {
  const int64_t total = rows * N;
  const float qnan = __uint_as_float(0x7fc00000u);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / N, k = i - r * N;
    const float2 z0 = z[(size_t)r * N];
    if (hb_nonfinite(z0.x) || hb_nonfinite(z0.y)) { z[i] = make_float2(qnan, qnan); continue; }
    const int g = hilbert_gain(k, N);
    if (g == 1) continue;
    const float2 v = z[i];
    z[i] = g == 2 ? make_float2(v.x * 2.0f, v.y * 2.0f) : make_float2(0.f, 0.f);
  }
}

// the complex signal [rows][N] -> the result, the mean of a centred row back in the real part
__global__ __launch_bounds__(kThreads) void k_hilbert_sink(const float2* __restrict__ a, int64_t rows, int64_t N, const float* __restrict__ means,
                                                          int32_t kind, void* __restrict__ out) {
  const int64_t n = rows * N;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    float2 v = a[i];
    if (means) v.x += means[i / N];
    if (kind == kHbAnalytic) static_cast<float2*>(out)[i] = v;
    else static_cast<float*>(out)[i] = kind == kHbEnvelope ? hb_mag(v.x, v.y) : v.y;
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

int run_generic(Ctx* c, const HilbertLaunch& a) {
  const int64_t rows = a.batch, N = a.n_fft, n_used = hilbert_used(a.length, N);
  // a row that fills the transform is centred on its way in (k_hilbert_rows), which also makes it dense; its mean returns in the sink
  const bool centre = n_used == N, copy = centre || (a.x_stride != n_used && rows > 1), through_sink = centre || a.kind != kHbAnalytic;
  void *spec = nullptr, *tmp = nullptr;
  int rc = ctx_scratch(c, kScratchFusedSpectrum, (size_t)rows * N * sizeof(float2), &spec);
  if (rc) return rc;
  // one temporary: the means | the dense rows, later the complex signal (the rows are spent once the forward transform has run)
  const size_t mean_bytes = centre ? (((size_t)rows * sizeof(float) + 255) & ~(size_t)255) : 0;
  const size_t copy_bytes = copy ? (size_t)rows * n_used * sizeof(float) : 0, signal_bytes = through_sink ? (size_t)rows * N * sizeof(float2) : 0;
  if (copy || through_sink)
    if ((rc = ctx_scratch(c, kScratchIstftProduct, mean_bytes + (copy_bytes > signal_bytes ? copy_bytes : signal_bytes), &tmp))) return rc;
  float* means = centre ? static_cast<float*>(tmp) : nullptr;
  void* region = tmp ? static_cast<char*>(tmp) + mean_bytes : nullptr;
  dispatch_note("hilbert.generic");
  const float* src = a.x;
  if (copy) {
    hipLaunchKernelGGL(k_hilbert_rows, dim3((unsigned)rows), dim3(kThreads), 0, c->stream, a.x, a.x_stride, n_used, static_cast<float*>(region), means);
    NXSIG_HIP_TRY(hipGetLastError());
    src = static_cast<const float*>(region);
  }
  if ((rc = launch_fft(c, src, true, rows, (int32_t)n_used, (int32_t)N, false, static_cast<float2*>(spec), false))) return rc;
  hipLaunchKernelGGL(k_hilbert_gain, dim3(stream_blocks(c, rows * N)), dim3(kThreads), 0, c->stream, static_cast<float2*>(spec), rows, N);
  NXSIG_HIP_TRY(hipGetLastError());
  float2* sig = through_sink ? static_cast<float2*>(region) : static_cast<float2*>(a.out);
  if ((rc = launch_fft(c, spec, false, rows, (int32_t)N, (int32_t)N, true, sig, false))) return rc;
  if (through_sink) {
    hipLaunchKernelGGL(k_hilbert_sink, dim3(stream_blocks(c, rows * N)), dim3(kThreads), 0, c->stream, sig, rows, N, means, a.kind, a.out);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_hilbert(Ctx* c, const HilbertLaunch& a) {
  if (a.batch == 0) return NXSIG_OK;
  const bool wave_off = tune(c, kT_DISABLE_HILBERT_WAVE, 0) != 0 || tune(c, kT_DISABLE_WAVE, 0) != 0;
  if (hilbert_tier(a.n_fft, wave_off) == kHbWave) return a.n_fft == 1024 ? run_wave<1024>(c, a) : run_wave<2048>(c, a);
  return run_generic(c, a);
}

}  // namespace nxsig
