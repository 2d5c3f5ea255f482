// Spectral.welch / csd: Welch's averaged periodogram of real f32 rows; include/nxsig.h states the definition, DESIGN.md section 3.12
// the design.  The spectrum of a frame never reaches memory in the wave tier: a wave transforms a run of consecutive frames of ONE row
// on the wave-private core of wave_stft.hpp and keeps the sums over frames in registers.
//
//   welch.pair     fft_length 1024 / 2048.  Frames 2u and 2u + 1 of a row as re / im of one complex transform z = a + i b (an odd last
//                  frame goes alone, b = 0).  No Hermitian untangle:  |A[k]|^2 + |B[k]|^2 = (|Z[k]|^2 + |Z[K - k]|^2) / 2,  so a lane
//                  adds |Z|^2 of its own K / 64 bins and the fold k <-> K - k happens once, in the finishing kernel
//   csd.pair       frame m of x and of y as re / im.  The mirrored bin comes through the wave's LDS buffer:
//                  X = (Z_k + conj Z_-k) / 2,  Y = -i (Z_k - conj Z_-k) / 2;  sums of |X|^2, |Y|^2, Re and Im of conj(X) Y for the
//                  bins of q <= K / 256 (bins 0 .. K / 2 + 127; the finishing kernel reads 0 .. K / 2)
//   welch.generic  every other fft_length, and NXSIG_DISABLE_WELCH_WAVE: detrended windowed frames of a chunk of runs -> launch_fft
//   csd.generic    (the row transforms of Nx.fft, no clean-up) -> a reduce kernel that forms the same partial sums
//   k_welch_finish both tiers: a row's runs added in ascending order in double, fold, one-sided doubling, scale / M, and a quiet NaN
//                  in every bin of a row whose flag is set
//
// Detrend: the mean of a frame is removed twice (m1 = mean(x), r = x - m1, r -= mean(r)): one f32 pass leaves 3.9e-4 of the row maximum
// on 1000 + N(0, 1), two leave 2.5e-7.  The wave reduction (wave_sum1) is wave-uniform and its order is fixed.
// Non-finite: every loaded sample is tested; a wave that saw one sets its row's flag (a plain store of 1: no ordering needed, the
// finishing kernel runs after the launch).  Nothing relies on the arithmetic to carry a NaN.
#include "wave_stft.hpp"

namespace nxsig {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// Wave-wide sum whose result is wave-uniform: four DPP adds leave the total of each row of 16 lanes in that row (quad swaps, then
// rotations by 4 and 8: VALU, no LDS traffic), and the four row totals are read off lanes 0, 16, 32, 48 and added in one fixed order —
// every lane gets the same bits, and the same bits every time
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum1(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm:[1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm:[2,3,0,1]
  v = dpp_add<0x124>(v);   // row_ror:4
  v = dpp_add<0x128>(v);   // row_ror:8
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ v2f wave_sum2(v2f v) { return v2f{wave_sum1(v.x), wave_sum1(v.y)}; }

struct WelchWaveArgs {
  const float* x;
  const float* y;            // csd only
  int64_t x_stride;
  int32_t N, hop, detrend;
  float inv_n;
  int64_t M, units_per_row, run_len, runs_per_row, total_runs;
  const float* wK;           // f32[K]: the window, zero beyond N
  const v2f* twB;
  const v2f* twC;
  float* part;               // [run][planes][plane_floats]
  int64_t plane_floats;
  int* flags;                // int[rows]
};

// FULL: N == K, no lane holds padding.  PF: the next unit's samples are loaded ahead of the current unit's transform (welch at 1024
// points: the registers are there, the LDS buffers bound the occupancy anyway)
template <int K, int W, bool CSD, bool FULL, bool PF>
__global__ __launch_bounds__(64 * W) void k_welch_wave(WelchWaveArgs a) {
  constexpr int P = K / 64;
  constexpr int R3 = K / 256;
  constexpr int NQ = K / 128;
  constexpr int QH = NQ / 2 + 1;   // csd: the q whose bins reach K / 2
  constexpr int XCH = K + K / 16 + 16;
  v2f* s_twB = reinterpret_cast<v2f*>(g_wave_smem);
  v2f* s_twC = s_twB + 256;
  v2f* s_x = s_twC + R3 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 256; i += 64 * W) s_twB[i] = a.twB[i];
  for (int i = tid; i < R3 * 256; i += 64 * W) s_twC[i] = a.twC[i];
  __syncthreads();
  v2f* xb = s_x + wave * XCH;
  const int64_t run = (int64_t)blockIdx.x * W + wave;
  if (run >= a.total_runs) return;   // the whole wave leaves; no barrier follows
  const int64_t row = run / a.runs_per_row;
  const int64_t u0 = (run - row * a.runs_per_row) * a.run_len;
  const int64_t u1 = u0 + a.run_len < a.units_per_row ? u0 + a.run_len : a.units_per_row;
  const float* xr = a.x + row * a.x_stride;
  const float* yr = CSD ? a.y + row * a.x_stride : nullptr;

  float wv[P];
#pragma unroll
  for (int s = 0; s < P; ++s) wv[s] = a.wK[lane + 64 * s];
  constexpr int NA = CSD ? 4 * QH : NQ;
  float acc[NA][2];   // welch: [q][parity]; csd: [4 q + {Pxx, Pyy, Re Pxy, Im Pxy}][parity]
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i][0] = acc[i][1] = 0.0f;
  bool bad = false;

  // the samples of unit u: frame m covers [m hop, m hop + N), inside the row for every m < M
  auto load = [&](int64_t u, v2f* dst) {
    const float* pa;
    const float* pb;
    bool have_b = true;
    if (CSD) { pa = xr + u * a.hop; pb = yr + u * a.hop; }
    else { pa = xr + 2 * u * a.hop; have_b = 2 * u + 1 < a.M; pb = have_b ? pa + a.hop : pa; }
#pragma unroll
    for (int s = 0; s < P; ++s) {
      const int i = lane + 64 * s;
      const bool live = FULL || i < a.N;
      const float fa = live ? pa[i] : 0.0f;
      float fb = live ? pb[i] : 0.0f;   // pb == pa for a lone last frame: a covered sample either way
      fb = have_b ? fb : 0.0f;
      dst[s] = v2f{fa, fb};
    }
  };
  v2f nxt[PF ? P : 1];
  if (PF) load(u0, nxt);

  for (int64_t u = u0; u < u1; ++u) {
    v2f d[P];
    if (PF) {
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = nxt[s];
      load(u + 1 < u1 ? u + 1 : u, nxt);   // unconditional: the loop stays branch-free
      __builtin_amdgcn_sched_barrier(0);
    } else {
      load(u, d);
    }
#pragma unroll
    for (int s = 0; s < P; ++s) bad = bad || nonfinite(d[s].x) || nonfinite(d[s].y);
    if (a.detrend) {
      v2f sum = v2f{0.f, 0.f};
#pragma unroll
      for (int s = 0; s < P; ++s) sum += d[s];
      const v2f m1 = wave_sum2(sum) * a.inv_n;
      sum = v2f{0.f, 0.f};
#pragma unroll
      for (int s = 0; s < P; ++s) {
        d[s] = FULL || lane + 64 * s < a.N ? d[s] - m1 : v2f{0.f, 0.f};
        sum += d[s];
      }
      const v2f m2 = wave_sum2(sum) * a.inv_n;
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = FULL || lane + 64 * s < a.N ? d[s] - m2 : v2f{0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < P; ++s) d[s] = d[s] * wv[s];

    v2f zz[2][NQ];
    wave_fft_core<K>(d, zz, xb, s_twB, s_twC, lane);

    if (!CSD) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        acc[q][0] = __builtin_fmaf(zz[0][q].x, zz[0][q].x, __builtin_fmaf(zz[0][q].y, zz[0][q].y, acc[q][0]));
        acc[q][1] = __builtin_fmaf(zz[1][q].x, zz[1][q].x, __builtin_fmaf(zz[1][q].y, zz[1][q].y, acc[q][1]));
      }
    } else {
      // the core's last fence is behind us: its exchange buffer is free.  Bin k at xb[k], the mirrored bin read back from xb[(K - k) % K]
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        *reinterpret_cast<v4f*>(&xb[2 * lane + 128 * q]) = v4f{zz[0][q].x, zz[0][q].y, zz[1][q].x, zz[1][q].y};
      wave_lds_fence();
#pragma unroll
      for (int q = 0; q < QH; ++q) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int k = 2 * lane + e + 128 * q;
          const v2f z = zz[e][q];
          const v2f zm = xb[(K - k) & (K - 1)];
          const float xre = 0.5f * (z.x + zm.x), xim = 0.5f * (z.y - zm.y);
          const float yre = 0.5f * (z.y + zm.y), yim = -0.5f * (z.x - zm.x);
          acc[4 * q + 0][e] = __builtin_fmaf(xre, xre, __builtin_fmaf(xim, xim, acc[4 * q + 0][e]));
          acc[4 * q + 1][e] = __builtin_fmaf(yre, yre, __builtin_fmaf(yim, yim, acc[4 * q + 1][e]));
          acc[4 * q + 2][e] = __builtin_fmaf(xre, yre, __builtin_fmaf(xim, yim, acc[4 * q + 2][e]));     // conj(X) Y
          acc[4 * q + 3][e] = __builtin_fmaf(xre, yim, __builtin_fmaf(-xim, yre, acc[4 * q + 3][e]));
        }
      }
      wave_lds_fence();   // the next frame's pass A writes come after these reads
    }
  }

  if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) a.flags[row] = 1;
  float* out = a.part + (size_t)run * (CSD ? 4 : 1) * a.plane_floats + 2 * lane;
  if (!CSD) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) *reinterpret_cast<v2f*>(out + 128 * q) = v2f{acc[q][0], acc[q][1]};
  } else {
#pragma unroll
    for (int q = 0; q < QH; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<v2f*>(out + (size_t)j * a.plane_floats + 128 * q) = v2f{acc[4 * q + j][0], acc[4 * q + j][1]};
  }
}

// ---- generic tier
struct WelchGenArgs {
  const float* x;
  int64_t x_stride;
  int32_t N, hop, K, detrend;
  float inv_n;
  int64_t M, run_len, runs_per_row;
  int64_t run0, runs;        // this chunk's runs [run0, run0 + runs) of the slab
  const float* w;            // f32[N]
  int* flags;
};

// frame slot t of the chunk = unit t % run_len of run run0 + t / run_len; a slot past the row's last frame holds zeros.  One wave per slot
__global__ __launch_bounds__(kThreads) void k_welch_frames(WelchGenArgs a, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= a.runs * a.run_len) return;
  const int64_t run = a.run0 + t / a.run_len;
  const int64_t row = run / a.runs_per_row;
  const int64_t m = (run - row * a.runs_per_row) * a.run_len + t % a.run_len;
  float* o = out + (size_t)t * a.N;
  if (m >= a.M) {
    for (int i = lane; i < a.N; i += 64) o[i] = 0.0f;
    return;
  }
  const float* p = a.x + row * a.x_stride + m * a.hop;
  float m1 = 0.0f, m2 = 0.0f;
  bool bad = false;
  float sum = 0.0f;
  for (int i = lane; i < a.N; i += 64) { const float v = p[i]; bad = bad || nonfinite(v); sum += v; }
  if (a.detrend) {
    m1 = wave_sum1(sum) * a.inv_n;
    sum = 0.0f;
    for (int i = lane; i < a.N; i += 64) sum += p[i] - m1;
    m2 = wave_sum1(sum) * a.inv_n;
  }
  for (int i = lane; i < a.N; i += 64) o[i] = ((p[i] - m1) - m2) * a.w[i];
  if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) a.flags[row] = 1;
}

// partial sums of the chunk's runs from the frames' spectra: one thread per (run, bin), frames in ascending order
template <bool CSD>
__global__ __launch_bounds__(kThreads) void k_welch_reduce(WelchGenArgs a, const float2* __restrict__ sx, const float2* __restrict__ sy,
                                                          int32_t nb, float* __restrict__ part) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= a.runs * nb) return;
  const int64_t rl = idx / nb;
  const int32_t k = (int32_t)(idx - rl * nb);
  const int64_t run = a.run0 + rl;
  const int64_t row = run / a.runs_per_row;
  const int64_t m0 = (run - row * a.runs_per_row) * a.run_len;
  const int64_t cnt = a.M - m0 < a.run_len ? a.M - m0 : a.run_len;
  float pxx = 0.f, pyy = 0.f, pre = 0.f, pim = 0.f;
  for (int64_t j = 0; j < cnt; ++j) {
    const size_t at = (size_t)(rl * a.run_len + j) * a.K + k;
    const float2 X = sx[at];
    pxx = __builtin_fmaf(X.x, X.x, __builtin_fmaf(X.y, X.y, pxx));
    if (CSD) {
      const float2 Y = sy[at];
      pyy = __builtin_fmaf(Y.x, Y.x, __builtin_fmaf(Y.y, Y.y, pyy));
      pre = __builtin_fmaf(X.x, Y.x, __builtin_fmaf(X.y, Y.y, pre));
      pim = __builtin_fmaf(X.x, Y.y, __builtin_fmaf(-X.y, Y.x, pim));
    }
  }
  float* o = part + (size_t)run * (CSD ? 4 : 1) * nb + k;
  o[0] = pxx;
  if (CSD) { o[nb] = pyy; o[2 * (size_t)nb] = pre; o[3 * (size_t)nb] = pim; }
}

struct WelchFinishArgs {
  const float* part;
  const int* flags;
  int64_t rows, runs_per_row, plane_floats;
  int32_t K, nb, planes, fold;   // fold: a plane holds |Z|^2 of all K bins of a frame PAIR (welch.pair)
  double scale;                  // definition's scale / M
  float* pxx;
  float* pyy;
  float2* pxy;
};

__global__ __launch_bounds__(kThreads) void k_welch_finish(WelchFinishArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= a.rows * a.nb) return;
  const int64_t row = idx / a.nb;
  const int32_t k = (int32_t)(idx - row * a.nb);
  const float* p = a.part + (size_t)row * a.runs_per_row * a.planes * a.plane_floats;
  const size_t run_stride = (size_t)a.planes * a.plane_floats;
  const double d = (k == 0 || ((a.K & 1) == 0 && k == a.K / 2)) ? 1.0 : 2.0;
  const float qnan = __uint_as_float(0x7fc00000u);
  const bool bad = a.flags[row] != 0;
  if (a.planes == 1) {
    double s = 0.0;
    if (a.fold) {
      const int32_t km = (a.K - k) % a.K;
      for (int64_t r = 0; r < a.runs_per_row; ++r) s += (double)p[r * run_stride + k] + (double)p[r * run_stride + km];
      s *= 0.5;
    } else {
      for (int64_t r = 0; r < a.runs_per_row; ++r) s += (double)p[r * run_stride + k];
    }
    a.pxx[idx] = bad ? qnan : (float)(s * a.scale * d);
    return;
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = 0; r < a.runs_per_row; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += (double)p[r * run_stride + (size_t)j * a.plane_floats + k];
  const double f = a.scale * d;
  if (a.pxx) a.pxx[idx] = bad ? qnan : (float)(s[0] * f);
  if (a.pyy) a.pyy[idx] = bad ? qnan : (float)(s[1] * f);
  a.pxy[idx] = bad ? make_float2(qnan, qnan) : make_float2((float)(s[2] * f), (float)(s[3] * f));
}

struct Slab {
  const float* x;
  const float* y;
  int64_t rows;
  int* flags;
  float* part;
  void* frames;   // generic tier: what follows the partial sums in the slot
};

template <int K, int W, bool CSD, bool FULL>
int run_wave(Ctx* c, const WelchLaunch& a, const WelchPlan& p, const Slab& s, const float* wK) {
  constexpr int R3 = K / 256, XCH = K + K / 16 + 16;
  int rc = ensure_wave_tables(c, K);
  if (rc) return rc;
  Ctx::WaveTables& wt = c->wave_tables[K];
  WelchWaveArgs w;
  w.x = s.x; w.y = s.y; w.x_stride = a.batch_stride; w.N = a.N; w.hop = a.hop; w.detrend = a.detrend ? 1 : 0;
  w.inv_n = (float)(1.0 / (double)a.N);
  w.M = p.M; w.units_per_row = p.units_per_row; w.run_len = p.run_len; w.runs_per_row = p.runs_per_row;
  w.total_runs = p.runs_per_row * s.rows;
  w.wK = wK; w.twB = reinterpret_cast<const v2f*>(wt.twB); w.twC = reinterpret_cast<const v2f*>(wt.twC);
  w.part = s.part; w.plane_floats = p.plane_floats; w.flags = s.flags;
  const int64_t blocks = (w.total_runs + W - 1) / W;
  if (blocks >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_UNSUPPORTED, "welch: 2^31 or more workgroups in one launch");
  const size_t lds = (size_t)256 * 8 + (size_t)R3 * 256 * 8 + (size_t)W * XCH * 8;
  auto kernel = k_welch_wave<K, W, CSD, FULL, (K == 1024 && !CSD)>;
  dispatch_note(CSD ? "csd.pair" : "welch.pair");
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * W), lds, c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <int K, int W>
int run_wave_k(Ctx* c, const WelchLaunch& a, const WelchPlan& p, const Slab& s, const float* wK) {
  const bool csd = a.y != nullptr, full = a.N == K;
  if (csd) return full ? run_wave<K, W, true, true>(c, a, p, s, wK) : run_wave<K, W, true, false>(c, a, p, s, wK);
  return full ? run_wave<K, W, false, true>(c, a, p, s, wK) : run_wave<K, W, false, false>(c, a, p, s, wK);
}

int run_generic(Ctx* c, const WelchLaunch& a, const WelchPlan& p, const Slab& s, const float* wN) {
  const bool csd = a.y != nullptr;
  const int32_t nb = a.K / 2 + 1;
  const int64_t total_runs = p.runs_per_row * s.rows;
  const int64_t slots_max = p.chunk_runs * p.run_len;
  void* spec = nullptr;
  int rc = ctx_scratch(c, kScratchFusedSpectrum, (size_t)slots_max * a.K * sizeof(float2) * (csd ? 2 : 1), &spec);
  if (rc) return rc;
  float* fx = static_cast<float*>(s.frames);
  float* fy = fx + (size_t)slots_max * a.N;
  float2* sx = static_cast<float2*>(spec);
  float2* sy = sx + (size_t)slots_max * a.K;
  WelchGenArgs g;
  g.x_stride = a.batch_stride; g.N = a.N; g.hop = a.hop; g.K = a.K; g.detrend = a.detrend ? 1 : 0;
  g.inv_n = (float)(1.0 / (double)a.N);
  g.M = p.M; g.run_len = p.run_len; g.runs_per_row = p.runs_per_row; g.w = wN; g.flags = s.flags;
  dispatch_note(csd ? "csd.generic" : "welch.generic");
  for (int64_t r0 = 0; r0 < total_runs; r0 += p.chunk_runs) {
    g.run0 = r0;
    g.runs = total_runs - r0 < p.chunk_runs ? total_runs - r0 : p.chunk_runs;
    const int64_t slots = g.runs * p.run_len;
    const unsigned fblocks = (unsigned)((slots + kThreads / 64 - 1) / (kThreads / 64));
    g.x = s.x;
    hipLaunchKernelGGL(k_welch_frames, dim3(fblocks), dim3(kThreads), 0, c->stream, g, fx);
    NXSIG_HIP_TRY(hipGetLastError());
    if ((rc = launch_fft(c, fx, true, slots, a.N, a.K, false, sx, false))) return rc;
    if (csd) {
      g.x = s.y;
      hipLaunchKernelGGL(k_welch_frames, dim3(fblocks), dim3(kThreads), 0, c->stream, g, fy);
      NXSIG_HIP_TRY(hipGetLastError());
      if ((rc = launch_fft(c, fy, true, slots, a.N, a.K, false, sy, false))) return rc;
    }
    const unsigned rblocks = (unsigned)((g.runs * nb + kThreads - 1) / kThreads);
    if (csd) hipLaunchKernelGGL(k_welch_reduce<true>, dim3(rblocks), dim3(kThreads), 0, c->stream, g, sx, sy, nb, s.part);
    else hipLaunchKernelGGL(k_welch_reduce<false>, dim3(rblocks), dim3(kThreads), 0, c->stream, g, sx, sx, nb, s.part);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_welch(Ctx* c, const WelchLaunch& a) {
  const bool csd = a.y != nullptr;
  // fft_length 2048 runs on wave_fft_core<2048> with two waves per workgroup (its exchange buffers are twice the size)
  const bool fused = (a.K == 1024 || a.K == 2048) && !tune(c, kT_DISABLE_WELCH_WAVE, 0) && !tune(c, kT_DISABLE_WAVE, 0);
  const int64_t M = welch_frames(a.L, a.N, a.hop);
  // the wave tier's runs fill the chip ONCE: its 45 / 53 KB of LDS per workgroup leave three workgroups per compute unit, so 12 waves
  // (1024 points, four per workgroup) or 6 (2048 points, two; csd.pair's 256 registers leave 4) are resident — more runs than that would queue for a second, partly
  // empty round
  const int64_t slots = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * (a.K == 1024 ? 12 : csd ? 4 : 6);
  const WelchPlan p = welch_plan(M, a.batch, a.K, csd, fused, slots);
  const int32_t nb = a.K / 2 + 1;
  const float *wN = nullptr, *wK = nullptr;
  int rc = ctx_window(c, a.window_host, a.N, a.K, &wN, &wK);
  if (rc) return rc;
  // one slot: flags | partial sums of a slab | (generic) the frames of a chunk, each part on a 256-byte boundary
  const size_t flag_bytes = ((size_t)p.slab_rows * sizeof(int) + 255) & ~(size_t)255;
  const size_t part_bytes = ((size_t)p.slab_rows * p.runs_per_row * p.planes * p.plane_floats * sizeof(float) + 255) & ~(size_t)255;
  const size_t frame_bytes = fused ? 0 : (size_t)p.chunk_runs * p.run_len * a.N * sizeof(float) * (csd ? 2 : 1);
  void* base = nullptr;
  if ((rc = ctx_scratch(c, kScratchLongStftFrames, flag_bytes + part_bytes + frame_bytes, &base))) return rc;
  for (int64_t r0 = 0; r0 < a.batch; r0 += p.slab_rows) {
    Slab s;
    s.rows = a.batch - r0 < p.slab_rows ? a.batch - r0 : p.slab_rows;
    s.x = a.x + (size_t)r0 * a.batch_stride;
    s.y = csd ? a.y + (size_t)r0 * a.batch_stride : nullptr;
    s.flags = static_cast<int*>(base);
    s.part = reinterpret_cast<float*>(static_cast<char*>(base) + flag_bytes);
    s.frames = static_cast<char*>(base) + flag_bytes + part_bytes;
    NXSIG_HIP_TRY(hipMemsetAsync(s.flags, 0, (size_t)s.rows * sizeof(int), c->stream));
    if (fused) {
      rc = a.K == 1024 ? run_wave_k<1024, 4>(c, a, p, s, wK) : run_wave_k<2048, 2>(c, a, p, s, wK);
    } else {
      rc = run_generic(c, a, p, s, wN);
    }
    if (rc) return rc;
    WelchFinishArgs f;
    f.part = s.part; f.flags = s.flags; f.rows = s.rows; f.runs_per_row = p.runs_per_row; f.plane_floats = p.plane_floats;
    f.K = a.K; f.nb = nb; f.planes = p.planes; f.fold = fused && !csd ? 1 : 0;
    f.scale = a.scale / (double)M;
    f.pxx = a.pxx ? a.pxx + (size_t)r0 * nb : nullptr;
    f.pyy = a.pyy ? a.pyy + (size_t)r0 * nb : nullptr;
    f.pxy = a.pxy ? a.pxy + (size_t)r0 * nb : nullptr;
    const int64_t blocks = (s.rows * nb + kThreads - 1) / kThreads;
    if (blocks >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_UNSUPPORTED, "welch: 2^31 or more workgroups in one launch");
    hipLaunchKernelGGL(k_welch_finish, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, f);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace nxsig
