// Transforms.czt / zoom_fft: the chirp z-transform X[k] = sum_j x[j] a^(-j) w^(j k) of real f32 or c64 rows, m points from any start a
// at any step w.  include/nxsig.h states the definition, DESIGN.md section 3.20 the design; the argument checks, the tier choice, the
// exact phase reduction, the table builder and the lane arithmetic are csrc/czt_plan.hpp.  Both tiers are Bluestein's identity over the
// three host tables A (n), F (L) and W (m): X = W . IDFT_L(DFT_L(x A) F), the inverse without its 1 / L (F carries it).
//   czt.wave     n + m - 1 <= 2048, L = 1024 or 2048: one wave per row on the wave-private cores, in the layout and LDS budget of
//                hilbert.wave.  8-byte loads of two adjacent f32 (16-byte loads of two adjacent c64) in the layout wave_fft_core
//                produces, zero at and past n; the product with A; wave_fft_core_T; the product with F in registers; the unscaled
//                inverse core; the product with W; 16-byte stores of two adjacent c64 for the first m points.  A row that starts off
//                the wide boundary is loaded / stored element by element.  The next row's loads are in flight during the butterflies.
//                The row is read once and the result written once; the tables (zero-padded to L) are read from L2
//   czt.generic  everything else and everything under NXSIG_CZT_WAVE=0 / NXSIG_DISABLE_WAVE, L the next power of two: a pre-multiply
//                writes dense zero-padded c64 rows (which also makes strided rows dense), launch_fft forward, the product with F,
//                launch_fft inverse, a post-multiply sink.  The LDS, tiled four-step and long-row transforms come with launch_fft.
//                Its two temporaries are the tier's own (Ctx::czt_rows, Ctx::czt_spectra): grown on demand, kept from call to call
// Non-finite rule, the same in both tiers: bin 0 of the forward transform is the sum of the chirped samples, so it is not finite when a
// sample is not; such a row's spectrum is replaced by NaN before the inverse transform and the row leaves without a finite element.
// No atomics.
#include "wave_stft.hpp"

namespace nxsig {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool cz_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

struct CztWaveArgs {
  const void* x;
  int64_t x_stride, rows, chunk;   // chunk: rows per workgroup
  int32_t n, m;
  const v2f* A;                    // [L], zero at and past n
  const v2f* F;                    // [L]
  const v2f* W;                    // [L], zero at and past m
  const v2f* twB;
  const v2f* twC;
  v2f* out;
};

template <int K, int W, bool CPLX>
__global__ __launch_bounds__(64 * W) void k_czt_wave(CztWaveArgs a) {
  constexpr int P = K / 64, R3 = K / 256, NQ = K / 128, XCH = K + K / 16 + 16;
  typedef typename std::conditional<CPLX, v4f, v2f>::type pair_t;   // two adjacent samples
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
  pair_t nx[NQ];   // nx[q] = (x[i0], x[i0 + 1]), i0 = 2 lane + 128 q; zero at and past n
  auto issue = [&](int64_t r) {
    if constexpr (CPLX) {
      const v2f* row = static_cast<const v2f*>(a.x) + (size_t)r * a.x_stride;
      const bool wide = czt_wide(reinterpret_cast<uintptr_t>(row), 8);   // wave-uniform: a row may start at any 8-byte address
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i0 = czt_slot_sample(lane, q), st = czt_pair_state(i0, a.n);
        v4f v = v4f{0.f, 0.f, 0.f, 0.f};
        if (wide) {
          if (st == 2) v = *reinterpret_cast<const v4f*>(row + i0);
          else if (st == 1) { const v2f t = row[i0]; v.x = t.x; v.y = t.y; }
        } else {
          if (st >= 1) { const v2f t = row[i0]; v.x = t.x; v.y = t.y; }
          if (st == 2) { const v2f t = row[i0 + 1]; v.z = t.x; v.w = t.y; }
        }
        nx[q] = v;
      }
    } else {
      const float* row = static_cast<const float*>(a.x) + (size_t)r * a.x_stride;
      const bool wide = czt_wide(reinterpret_cast<uintptr_t>(row), 4);   // wave-uniform: a row may start at any 4-byte address
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i0 = czt_slot_sample(lane, q), st = czt_pair_state(i0, a.n);
        v2f v = v2f{0.f, 0.f};
        if (wide) {
          if (st == 2) v = *reinterpret_cast<const v2f*>(row + i0);
          else if (st == 1) v.x = row[i0];
        } else {
          if (st >= 1) v.x = row[i0];
          if (st == 2) v.y = row[i0 + 1];
        }
        nx[q] = v;
      }
    }
  };
  if (r_begin + wave < r_end) issue(r_begin + wave);
  for (int64_t r = r_begin + wave; r < r_end; r += W) {
    // the samples times A, the two entries of a lane's pair in one 16-byte load (the table is zero-padded to K and 16-byte aligned)
    v2f zz[2][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const v4f t = *reinterpret_cast<const v4f*>(a.A + czt_slot_sample(lane, q));
      if constexpr (CPLX) {
        zz[0][q] = wcmul(v2f{nx[q].x, nx[q].y}, v2f{t.x, t.y});
        zz[1][q] = wcmul(v2f{nx[q].z, nx[q].w}, v2f{t.z, t.w});
      } else {
        zz[0][q] = v2f{nx[q].x * t.x, nx[q].x * t.y};
        zz[1][q] = v2f{nx[q].y * t.z, nx[q].y * t.w};
      }
    }
    issue(r + W < r_end ? r + W : r);   // unconditional prefetch (the last iteration re-reads its own row)
    __builtin_amdgcn_sched_barrier(0);
    v2f d[P];
    wave_fft_core_T<K>(zz, d, xb, s_twB, s_twC, lane);   // d[s] = X[lane + 64 s]
    // lane 0 holds bin 0, the sum of the chirped samples, in register 0: not finite when a sample is not
    const float x0r = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(d[0].x)));
    const float x0i = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(d[0].y)));
    const bool poisoned = cz_nonfinite(x0r) || cz_nonfinite(x0i);   // wave-uniform
#pragma unroll
    for (int s = 0; s < P; ++s) d[s] = wcmul(d[s], a.F[czt_bin(lane, s)]);
    if (poisoned) {
      const float qnan = __uint_as_float(0x7fc00000u);
#pragma unroll
      for (int s = 0; s < P; ++s) d[s] = v2f{qnan, qnan};
    }
    v2f u[2][NQ];
    wave_fft_core<K, true, true>(d, u, xb, s_twB, s_twC, lane);   // unscaled inverse: u[par][q] = y[2 lane + par + 128 q]
    __builtin_amdgcn_sched_barrier(0);
    v2f* orow = a.out + (size_t)r * a.m;
    const bool wide = czt_wide(reinterpret_cast<uintptr_t>(orow), 8);   // wave-uniform: with an odd m every other row starts off 16 bytes
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k0 = czt_slot_sample(lane, q), st = czt_pair_state(k0, a.m);
      if (st == 0) continue;
      const v4f t = *reinterpret_cast<const v4f*>(a.W + k0);
      const v2f y0 = wcmul(u[0][q], v2f{t.x, t.y}), y1 = wcmul(u[1][q], v2f{t.z, t.w});
      if (st == 2 && wide) __builtin_nontemporal_store(v4f{y0.x, y0.y, y1.x, y1.y}, (gv4f*)(orow + k0));
      else {
        orow[k0] = y0;
        if (st == 2) orow[k0 + 1] = y1;
      }
    }
  }
}

// ---- the three tables of a contour on the device, f32, formed once per context and parameter set: the memo keeps the pointers beside
// the parameters, so a repeated call makes no table request.  pad: A and W are zero-padded to L entries (czt.wave reads whole pairs)
struct CztTables { const float2 *A, *F, *W; };
uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, sizeof b); return b; }

int czt_device_tables(Ctx* c, const CztLaunch& a, int64_t L, bool pad, CztTables* t) {
  const CztContour& k = a.contour;
  std::vector<uint64_t> want = {0, 0, 0, (uint64_t)pad, (uint64_t)a.length, (uint64_t)a.m, (uint64_t)L, bits_of(k.w_abs), bits_of(k.w_step),
                                (uint64_t)k.w_den, bits_of(k.a_abs), bits_of(k.a_turns)};
  const uint64_t key = fnv1a(0xC2770000ull, want.data() + 3, (want.size() - 3) * sizeof(uint64_t));
  auto hit = c->memo.find(key);
  if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 3, want.end(), hit->second.begin() + 3)) {
    t->A = reinterpret_cast<const float2*>((uintptr_t)hit->second[0]);
    t->F = reinterpret_cast<const float2*>((uintptr_t)hit->second[1]);
    t->W = reinterpret_cast<const float2*>((uintptr_t)hit->second[2]);
    return NXSIG_OK;
  }
  const int64_t n = a.length, m = a.m, na = pad ? L : n, nw = pad ? L : m;
  std::vector<double> A((size_t)2 * n), F((size_t)2 * L), W((size_t)2 * m);
  if (const char* what = czt_tables(n, m, L, k, A.data(), F.data(), W.data(), nullptr)) return set_error(NXSIG_ERR_UNSUPPORTED, std::string("czt: ") + what);
  std::vector<float> Af((size_t)2 * na, 0.0f), Ff((size_t)2 * L), Wf((size_t)2 * nw, 0.0f);
  for (int64_t i = 0; i < 2 * n; ++i) Af[i] = (float)A[i];
  for (int64_t i = 0; i < 2 * L; ++i) Ff[i] = (float)F[i];
  for (int64_t i = 0; i < 2 * m; ++i) Wf[i] = (float)W[i];
  const void *dA = nullptr, *dF = nullptr, *dW = nullptr;
  int rc = ctx_table(c, 0xC2770A00ull, Af.data(), Af.size() * sizeof(float), &dA);
  if (rc) return rc;
  if ((rc = ctx_table(c, 0xC2770F00ull, Ff.data(), Ff.size() * sizeof(float), &dF))) return rc;
  if ((rc = ctx_table(c, 0xC2770B00ull, Wf.data(), Wf.size() * sizeof(float), &dW))) return rc;
  want[0] = (uint64_t)(uintptr_t)dA; want[1] = (uint64_t)(uintptr_t)dF; want[2] = (uint64_t)(uintptr_t)dW;
  c->memo[key] = want;
  t->A = static_cast<const float2*>(dA); t->F = static_cast<const float2*>(dF); t->W = static_cast<const float2*>(dW);
  return NXSIG_OK;
}

template <int K, bool CPLX>
int run_wave(Ctx* c, const CztLaunch& a) {
  constexpr int W = K == 2048 ? 2 : 4;
  int rc = ensure_wave_tables(c, K);
  if (rc) return rc;
  CztTables t;
  if ((rc = czt_device_tables(c, a, K, true, &t))) return rc;
  Ctx::WaveTables& wt = c->wave_tables[K];
  CztWaveArgs w;
  w.x = a.x; w.x_stride = a.x_stride; w.rows = a.batch; w.n = (int32_t)a.length; w.m = (int32_t)a.m;
  w.A = reinterpret_cast<const v2f*>(t.A); w.F = reinterpret_cast<const v2f*>(t.F); w.W = reinterpret_cast<const v2f*>(t.W);
  w.twB = reinterpret_cast<const v2f*>(wt.twB); w.twC = reinterpret_cast<const v2f*>(wt.twC);
  w.out = static_cast<v2f*>(a.out);
  const int rpw = tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, a.batch, W, 4);
  w.chunk = (int64_t)W * (rpw < 1 ? 1 : rpw);
  const int64_t blocks = czt_blocks(a.batch, w.chunk);
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "czt: too many rows for one launch");
  dispatch_note("czt.wave");
  hipLaunchKernelGGL((k_czt_wave<K, W, CPLX>), dim3((unsigned)blocks), dim3(64 * W), (size_t)czt_lds_bytes(K), c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

// ---- czt.generic
// rows x_stride apart times A -> dense zero-padded c64 [rows][L]
template <bool CPLX>
__global__ __launch_bounds__(kThreads) void k_czt_pre(const void* __restrict__ x, int64_t x_stride, int64_t rows, int64_t n, int64_t L,
                                                     const float2* __restrict__ A, float2* __restrict__ out) {
  const int64_t total = rows * L;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / L, j = i - r * L;
    float2 v = make_float2(0.f, 0.f);
    if (j < n) {   // nothing at or past n is read
      const float2 t = A[j];
      if (CPLX) {
        const float2 s = static_cast<const float2*>(x)[(size_t)r * x_stride + j];
        v = make_float2(s.x * t.x - s.y * t.y, s.x * t.y + s.y * t.x);
      } else {
        const float s = static_cast<const float*>(x)[(size_t)r * x_stride + j];
        v = make_float2(s * t.x, s * t.y);
      }
    }
    out[i] = v;
  }
}

// out[r][k] = z[r][k] F[k]; a row whose bin 0 is not finite becomes NaN throughout.  Out of place: every lane of a row reads its bin 0
__global__ __launch_bounds__(kThreads) void k_czt_mul(const float2* __restrict__ z, const float2* __restrict__ F, int64_t rows, int64_t L,
                                                     float2* __restrict__ out) {
  const int64_t total = rows * L;
  const float qnan = __uint_as_float(0x7fc00000u);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / L, k = i - r * L;
    const float2 z0 = z[(size_t)r * L];
    if (cz_nonfinite(z0.x) || cz_nonfinite(z0.y)) { out[i] = make_float2(qnan, qnan); continue; }
    const float2 v = z[i], t = F[k];
    out[i] = make_float2(v.x * t.x - v.y * t.y, v.x * t.y + v.y * t.x);
  }
}

// the first m points of the convolution [rows][L] times W -> the result [rows][m].  scale = L: launch_fft's inverse divides by L, and
// F carries that 1 / L already (a power of two: exact)
__global__ __launch_bounds__(kThreads) void k_czt_post(const float2* __restrict__ y, const float2* __restrict__ W, int64_t rows, int64_t L, int64_t m,
                                                      float scale, float2* __restrict__ out) {
  const int64_t total = rows * m;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / m, k = i - r * m;
    const float2 v = y[(size_t)r * L + k], t = W[k];
    out[i] = make_float2((v.x * t.x - v.y * t.y) * scale, (v.x * t.y + v.y * t.x) * scale);
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

int enqueue_generic(Ctx* c, const CztLaunch& a, int64_t L, const CztTables& t, float2* rows_buf, float2* spec) {
  const int64_t rows = a.batch, n = a.length, m = a.m;
  int rc;
  if (a.is_complex) hipLaunchKernelGGL(k_czt_pre<true>, dim3(stream_blocks(c, rows * L)), dim3(kThreads), 0, c->stream, a.x, a.x_stride, rows, n, L, t.A, rows_buf);
  else hipLaunchKernelGGL(k_czt_pre<false>, dim3(stream_blocks(c, rows * L)), dim3(kThreads), 0, c->stream, a.x, a.x_stride, rows, n, L, t.A, rows_buf);
  NXSIG_HIP_TRY(hipGetLastError());
  if ((rc = launch_fft(c, rows_buf, false, rows, (int32_t)L, (int32_t)L, false, spec, false))) return rc;
  hipLaunchKernelGGL(k_czt_mul, dim3(stream_blocks(c, rows * L)), dim3(kThreads), 0, c->stream, spec, t.F, rows, L, rows_buf);
  NXSIG_HIP_TRY(hipGetLastError());
  if ((rc = launch_fft(c, rows_buf, false, rows, (int32_t)L, (int32_t)L, true, spec, false))) return rc;
  hipLaunchKernelGGL(k_czt_post, dim3(stream_blocks(c, rows * m)), dim3(kThreads), 0, c->stream, spec, t.W, rows, L, m, (float)L, static_cast<float2*>(a.out));
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

// one of the tier's own temporaries, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does)
int own_buffer(Ctx* c, Ctx::OwnedBuffer& b, size_t bytes, void** out) {
  if (b.bytes < bytes) {
    if (b.ptr) {
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      NXSIG_HIP_TRY(hipFree(b.ptr));
      b.ptr = nullptr; b.bytes = 0;
    }
    NXSIG_HIP_TRY(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
  }
  *out = b.ptr;
  return NXSIG_OK;
}

int run_generic(Ctx* c, const CztLaunch& a) {
  const int64_t L = czt_conv_length(a.length, a.m, true);
  CztTables t;
  int rc = czt_device_tables(c, a, L, false, &t);
  if (rc) return rc;
  const size_t bytes = (size_t)a.batch * L * sizeof(float2);
  void *rows_buf = nullptr, *spec = nullptr;
  if ((rc = own_buffer(c, c->czt_rows, bytes, &rows_buf))) return rc;
  if ((rc = own_buffer(c, c->czt_spectra, bytes, &spec))) return rc;
  dispatch_note("czt.generic");
  return enqueue_generic(c, a, L, t, static_cast<float2*>(rows_buf), static_cast<float2*>(spec));
}

}  // namespace

int launch_czt(Ctx* c, const CztLaunch& a) {
  if (a.batch == 0) return NXSIG_OK;
  const bool wave_off = tune(c, kT_CZT_WAVE, 1) == 0 || tune(c, kT_DISABLE_WAVE, 0) != 0;
  if (czt_tier(a.length, a.m, wave_off) == kCzGeneric) return run_generic(c, a);
  if (czt_conv_length(a.length, a.m, false) == 1024) return a.is_complex ? run_wave<1024, true>(c, a) : run_wave<1024, false>(c, a);
  return a.is_complex ? run_wave<2048, true>(c, a) : run_wave<2048, false>(c, a);
}

}  // namespace nxsig
