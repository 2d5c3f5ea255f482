// Wave-private FFT kernels: the inverse STFT with a TIME-FREQUENCY MASK fused in — opt-in extension (nxsig_istft_masked_c64).
//
// stft -> a model or a rule produces a mask per (frame, bin) -> istft(Nx.multiply(z, mask)) is the denoising / source-separation /
// spectral-gating workflow.  As two calls the masked spectrogram is written to HBM and read back: 8 (z) + 4 (mask) + 8 + 8 + 2 (y) =
// 30 KB per frame at N = 1024, hop 256.  Here every frame's mask row streams in next to its spectrum: 8 + 4 + 2 = 14 KB (12 with a
// one-sided real mask).
//
// k_istft_wave_mask<R, SCALE, W, CPLX> is k_istft_wave (kernels_wave.hip) in its one-frame-ahead form, N = K = 1024, hop = 1024 / R:
// same run / halo geometry, same core, same overlap-add in registers, same rounding order, so the result equals the two-step form
// bit for bit.  What differs: a lane's 16 mask values (f32, or c64 when CPLX) are prefetched together with the 16 bins they belong
// to, and the product — Nx.BinaryBackend's: in double, one rounding per component — is formed where the prefetched frame becomes
// the core's input.  z and the mask are addressed through row strides of their own (0: one row read for every output row).
// The one-sided real mask f32[K/2 + 1] is only another address: bin k > K/2 reads mask[K - k], i.e. the lane's upper eight values
// walk DOWN from mask[512 - lane]; the loads are 4-byte ones, so the odd row stride of 513 floats needs no alignment path.
// Tail-flush frames m >= M read a spectrum AND a mask of zeros (a non-finite mask value of the last frame must not reach them).
#include "wave_stft.hpp"

namespace nxsig {

struct IstftMaskArgs {
  const v2f* z;               // c64[z rows][M][K]
  const void* mask;           // f32[mask rows][M][mlen] or c64[mask rows][M][K]
  int64_t z_row_stride;       // c64 between rows of z (0: broadcast)
  int64_t mask_row_stride;    // mask elements between rows of the mask (0: broadcast)
  int32_t mlen;               // mask elements per frame: K, or K/2 + 1 (one-sided)
  int32_t onesided;
  int64_t M;
  int32_t batch, hop;
  int64_t segs_per_row;       // M + R - 1  (out_len = segs_per_row * hop)
  int64_t run_len, runs_per_row, total_runs;
  const float* wtab;          // f32[K]
  const v2f* twB;             // conjugated tables: the core runs in inverse direction
  const v2f* twC;
  float scale;
  const float* den;           // f32[2R-1][hop]: reciprocal of the guarded OLA normaliser (istft_den_table)
  v2f* y;                     // c64[batch][segs_per_row * hop]
  v2f* dummy;
  const v2f* zeros;           // c64[K] of zeros: spectrum and mask of the tail-flush frames
};

template <int R, bool SCALE, int W, bool CPLX>
__global__ __launch_bounds__(64 * W) void k_istft_wave_mask(IstftMaskArgs a) {
  constexpr int K = 1024;
  constexpr int P = K / 64;
  constexpr int R3 = K / 256;
  constexpr int NQ = K / 128;
  constexpr int QS = NQ / R;            // q values (of 128 samples each) per hop segment, per parity
  constexpr int XCH = K + K / 16 + 16;
  static_assert(NQ % R == 0, "hop must be a multiple of 128");
  using MT = typename std::conditional<CPLX, v2f, float>::type;
  float* s_w = reinterpret_cast<float*>(g_wave_smem);
  v2f* s_twB = reinterpret_cast<v2f*>(s_w + K);
  v2f* s_twC = s_twB + 256;
  v2f* s_x = s_twC + R3 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K; i += 64 * W) s_w[i] = a.wtab[i];
  for (int i = tid; i < 256; i += 64 * W) s_twB[i] = a.twB[i];
  for (int i = tid; i < R3 * 256; i += 64 * W) s_twC[i] = a.twC[i];
  __syncthreads();
  v2f* xb = s_x + wave * XCH;
  const int64_t run = (int64_t)blockIdx.x * W + wave;
  if (run >= a.total_runs) return;  // whole wave leaves; no barrier follows
  const int64_t row = run / a.runs_per_row;
  const int64_t j0 = (run - row * a.runs_per_row) * a.run_len;
  int64_t j1 = j0 + a.run_len;
  if (j1 > a.segs_per_row) j1 = a.segs_per_row;
  const int64_t m_start = j0 >= (R - 1) ? j0 - (R - 1) : 0;   // the run's R - 1 halo frames are recomputed, masks included

  float wv[2][NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const v2f w = *reinterpret_cast<const v2f*>(&s_w[2 * lane + 128 * q]);
    wv[0][q] = w.x; wv[1][q] = w.y;
  }
  const float invK = 1.0f / (float)K;
  v2f pend[R - 1 > 0 ? R - 1 : 1][2][QS];
#pragma unroll
  for (int i = 0; i < R - 1; ++i)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int qq = 0; qq < QS; ++qq) pend[i][e][qq] = v2f{0.f, 0.f};

  const v2f* zrow = a.z + (size_t)row * a.z_row_stride + lane;
  const MT* mrow = reinterpret_cast<const MT*>(a.mask) + (size_t)row * a.mask_row_stride;
  // mask element of bin lane + 64 s: s < 8 at lane + 64 s; s >= 8 the same, or (one-sided) K - (lane + 64 s) = (K - lane) - 64 s
  const int hi0 = a.onesided ? K - lane : lane;
  const int histep = a.onesided ? -64 : 64;
  v2f r[P];
  MT g[P];
  auto issue = [&](int64_t m) {
    const bool live = m < a.M;
    const v2f* pz = live ? zrow + (size_t)m * K : a.zeros + lane;   // frames past the end (tail flush): zeros times zeros
    const MT* pm = live ? mrow + (size_t)m * a.mlen : reinterpret_cast<const MT*>(a.zeros);
#pragma unroll
    for (int s = 0; s < P; ++s) r[s] = __builtin_nontemporal_load(pz + 64 * s);
#pragma unroll
    for (int s = 0; s < P; ++s) g[s] = __builtin_nontemporal_load(s < P / 2 ? pm + lane + 64 * s : pm + hi0 + histep * s);
  };
  v2f d[P];
  auto take = [&]() {   // the prefetched spectrum times its mask becomes the core's input
#pragma unroll
    for (int s = 0; s < P; ++s) {
      if constexpr (CPLX) {
        const double re = (double)r[s].x * (double)g[s].x - (double)r[s].y * (double)g[s].y;
        const double im = (double)r[s].x * (double)g[s].y + (double)r[s].y * (double)g[s].x;
        d[s] = v2f{(float)re, (float)im};
      } else {
        d[s] = v2f{(float)((double)r[s].x * (double)g[s]), (float)((double)r[s].y * (double)g[s])};
      }
    }
  };
  issue(m_start);
  take();

  for (int64_t m = m_start; m < j1; ++m) {
    issue(m + 1 < j1 ? m + 1 : m);  // unconditional prefetch keeps the loop branch-free
    __builtin_amdgcn_sched_barrier(0);
    v2f zz[2][NQ];
    wave_fft_core<K, true>(d, zz, xb, s_twB, s_twC, lane);  // inverse direction (tables are conjugated)
    __builtin_amdgcn_sched_barrier(0);
    take();
    __builtin_amdgcn_sched_barrier(0);

    const int64_t j = m;                        // segment j is complete once frame j has been folded in
    const int64_t trow = j < R - 1 ? j : (j >= a.M ? R + (j - a.M) : R - 1);
    const float* dp = a.den + trow * a.hop + 2 * lane;
    v2f den[QS];
#pragma unroll
    for (int qq = 0; qq < QS; ++qq) den[qq] = *reinterpret_cast<const v2f*>(dp + 128 * qq);
    // frame samples ((IDFT / K) * scale) * window (lib/nx_signal.ex:609-628, same rounding order as k_istft_wave) folded into the
    // pending overlap sums in ascending frame order
    v2f out[2][QS];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int qq = 0; qq < QS; ++qq) {
        v2f f[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          v2f v = fft_eps0(zz[e][i * QS + qq] * invK);  // Nx.ifft's clean-up (:609) precedes scale and window
          if (SCALE) v = v * a.scale;
          f[i] = v * wv[e][i * QS + qq];
        }
        if (R == 1) { out[e][qq] = f[0]; }
        else {
          out[e][qq] = pend[0][e][qq] + f[0];
#pragma unroll
          for (int i = 0; i + 1 < R - 1; ++i) pend[i][e][qq] = pend[i + 1][e][qq] + f[i + 1];
          pend[R - 2][e][qq] = f[R - 1];
        }
      }
    v2f* yp = (j >= j0) ? a.y + (size_t)row * a.segs_per_row * a.hop + j * a.hop + 2 * lane : a.dummy + 2 * lane;
#pragma unroll
    for (int qq = 0; qq < QS; ++qq) {
      const v4f o = v4f{out[0][qq].x * den[qq].x, out[0][qq].y * den[qq].x, out[1][qq].x * den[qq].y, out[1][qq].y * den[qq].y};
      __builtin_nontemporal_store(o, (gv4f*)(yp + 128 * qq));
    }
  }
}

int istft_den_table(Ctx* c, int R, int hop, const float* window_host, const float** out);   // kernels_wave.hip

template <int R>
static int launch_istft_mask_R(Ctx* c, const IstftLaunch& s, const float* window_host) {
  constexpr int K = 1024, W = 4, R3 = K / 256, XCH = K + K / 16 + 16;
  IstftMaskArgs a;
  a.z = reinterpret_cast<const v2f*>(s.z); a.mask = s.mask;
  a.mlen = (int32_t)mask_row_len(s.mask_kind, K);
  a.onesided = s.mask_kind == NXSIG_MASK_ONESIDED ? 1 : 0;
  a.z_row_stride = s.z_bcast ? 0 : s.M * (int64_t)K;
  a.mask_row_stride = s.mask_bcast ? 0 : s.M * (int64_t)a.mlen;
  a.M = s.M; a.batch = s.batch; a.hop = s.hop;
  a.segs_per_row = s.M + R - 1;
  a.wtab = s.window;   // the raw window (N == K)
  Ctx::WaveTables& wt = c->wave_tables[K];
  if (!wt.twB) return NXSIG_ERR_UNSUPPORTED;
  a.twB = reinterpret_cast<const v2f*>(wt.twBi);
  a.twC = reinterpret_cast<const v2f*>(wt.twCi);
  a.scale = s.scale_mul;
  { int rc = istft_den_table(c, R, s.hop, window_host, &a.den); if (rc) return rc; }
  a.y = reinterpret_cast<v2f*>(s.y);
  {
    const void* dz = nullptr;
    auto hit = c->memo.find(0x2E2000000000ull ^ (uint64_t)K);   // shared with launch_istft_wave_R: built once per context
    if (hit != c->memo.end()) dz = reinterpret_cast<const void*>(hit->second[0]);
    else {
      static const std::vector<float2> zero_row((size_t)K, make_float2(0.f, 0.f));
      int rc = ctx_table(c, 0x2E20ull, zero_row.data(), zero_row.size() * sizeof(float2), &dz);
      if (rc) return rc;
      c->memo[0x2E2000000000ull ^ (uint64_t)K] = {reinterpret_cast<uint64_t>(dz)};
    }
    a.zeros = reinterpret_cast<const v2f*>(dz);
  }
  void* dummy = nullptr;
  { int rc = ctx_scratch(c, kScratchWaveSink, (size_t)8192 * sizeof(float2), &dummy); if (rc) return rc; }
  a.dummy = reinterpret_cast<v2f*>(dummy);
  const int64_t total_segs = a.segs_per_row * s.batch;
  const int waves_per_cu = tune(c, kT_ISTFT_RUNS_PER_CU, 8);   // two waves per SIMD
  int64_t run_len = (total_segs + (int64_t)c->num_cus * waves_per_cu - 1) / ((int64_t)c->num_cus * waves_per_cu);
  const int min_run = istft_min_run(c, total_segs, (int64_t)c->num_cus * waves_per_cu, 4);
  if (run_len < min_run) run_len = min_run;
  a.run_len = run_len;
  a.runs_per_row = (a.segs_per_row + run_len - 1) / run_len;
  a.total_runs = a.runs_per_row * s.batch;
  const int64_t blocks = (a.total_runs + W - 1) / W;
  const size_t lds = (size_t)K * 4 + 256 * 8 + (size_t)R3 * 256 * 8 + (size_t)W * XCH * 8;
  dispatch_note("istft.wave.mask");
  const bool cplx = s.mask_kind == NXSIG_MASK_COMPLEX;
  if (cplx) {
    if (s.has_scale) hipLaunchKernelGGL((k_istft_wave_mask<R, true, W, true>), dim3((unsigned)blocks), dim3(64 * W), lds, c->stream, a);
    else hipLaunchKernelGGL((k_istft_wave_mask<R, false, W, true>), dim3((unsigned)blocks), dim3(64 * W), lds, c->stream, a);
  } else if (s.has_scale) hipLaunchKernelGGL((k_istft_wave_mask<R, true, W, false>), dim3((unsigned)blocks), dim3(64 * W), lds, c->stream, a);
  else hipLaunchKernelGGL((k_istft_wave_mask<R, false, W, false>), dim3((unsigned)blocks), dim3(64 * W), lds, c->stream, a);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

// s.mask set.  Fused for N = fft_length = 1024, hop 128 ... 1024 and M >= 2R - 1 (k_istft_wave's conditions); everything else is
// declined and launch_istft materialises the product first
int launch_istft_wave_mask(Ctx* c, const IstftLaunch& s, const float* window_host, bool* handled) {
  *handled = false;
  if (s.M == 0 || s.batch == 0 || window_host == nullptr || !s.mask || s.filt || s.onesided) return NXSIG_OK;
  if (tune(c, kT_DISABLE_WAVE, 0) || tune(c, kT_DISABLE_FUSED_MASK, 0)) return NXSIG_OK;
  if (s.K != 1024 || s.N != 1024) return NXSIG_OK;
  if (s.hop != 128 && s.hop != 256 && s.hop != 512 && s.hop != 1024) return NXSIG_OK;
  if (s.M < 2 * (1024 / s.hop) - 1) return NXSIG_OK;  // head and tail rows must not overlap
  int rc = ensure_wave_tables_1024(c);
  if (rc) return rc;
  *handled = true;
  switch (1024 / s.hop) {
    case 1: return launch_istft_mask_R<1>(c, s, window_host);
    case 2: return launch_istft_mask_R<2>(c, s, window_host);
    case 4: return launch_istft_mask_R<4>(c, s, window_host);
    default: return launch_istft_mask_R<8>(c, s, window_host);
  }
}

}  // namespace nxsig
