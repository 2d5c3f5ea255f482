// Filters.fir_bank / Transforms.cwt: S filters of different lengths applied to every real f32 row in "same" alignment,
// out[row][s][n] = full_s[n + (N_s - 1) / 2], full_s = x * h_s.  include/nxsig.h states the definition, DESIGN.md section 3.21 the
// design; the support rule, the class split, the block geometry, the spectrum builder and the lane arithmetic are csrc/cwt_plan.hpp.
// The bank is split by support and one launch group runs per non-empty class:
//   cwt.wave     N <= 513 at K = 1024, 514 <= N <= 1025 at K = 2048: overlap-save on the wave-private cores.  A wave loads a block of K
//                real samples in the layout wave_fft_core_T consumes (zero beyond the row's ends; 8-byte loads where the block starts
//                on 8 bytes, element by element otherwise), transforms it ONCE as a complex block with a zero imaginary part (the form
//                hilbert.wave uses, for real and complex banks alike) and then, per filter of the class, multiplies the spectrum held
//                in registers by H_s / K (read from L2), runs the unscaled inverse core and stores the block's valid run of
//                out[row][s] through the sink of `kind`.  The block step K - Nmax + 1 is one per class.  The next block's loads are
//                in flight during the butterflies.  The input is read once per class, the result written once
//   cwt.generic  N > 1025 and everything under NXSIG_CWT_WAVE=0 / NXSIG_DISABLE_WAVE: the rows zero-padded to the next power of two
//                >= L + Nmax - 1 and transformed once by launch_fft; per filter a product kernel, launch_fft back and a slice-and-sink
//                kernel.  Three temporaries of the family's own (Ctx::cwt_rows, cwt_spectra, cwt_conv)
// Non-finite rule (FIR's): a kernel that loads an Inf / NaN sample raises its row's flag (Ctx::cwt_flags) with a plain store; a last
// pass writes NaN over every output of a flagged row and the flags are cleared.  No atomics.
#include "wave_stft.hpp"

namespace nxsig {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool cw_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ float cw_mag(float re, float im) { return sqrtf(re * re + im * im); }
template <int KIND>
__device__ __forceinline__ float cw_sink(v2f y) {
  return KIND == kCwReal ? y.x : KIND == kCwMagnitude ? cw_mag(y.x, y.y) : y.x * y.x + y.y * y.y;
}

struct CwtWaveArgs {
  const float* x;
  int64_t x_stride, length, units, chunk;   // units: rows x blocks per row; chunk: units per workgroup
  int32_t bpr, step, lead, nf;              // blocks per row, block step, first valid position, filters of this class
  int64_t bank;                             // filters of the whole bank (the row pitch of out is bank * length)
  const v2f* H;                             // [nf][K], H_s / K
  const int32_t* member;                    // [nf]: the filter's index in the bank
  const v2f* twB;
  const v2f* twC;
  void* out;
  int32_t* flags;                           // [rows]
};

template <int K, int W, int KIND>
__global__ __launch_bounds__(64 * W) void k_cwt_wave(CwtWaveArgs a) {
  constexpr int P = K / 64, R3 = K / 256, NQ = K / 128, XCH = K + K / 16 + 16;
  v2f* s_twB = reinterpret_cast<v2f*>(g_wave_smem);
  v2f* s_twC = s_twB + 256;
  v2f* s_x = s_twC + R3 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 256; i += 64 * W) s_twB[i] = a.twB[i];
  for (int i = tid; i < R3 * 256; i += 64 * W) s_twC[i] = a.twC[i];
  __syncthreads();
  v2f* xb = s_x + wave * XCH;
  const int64_t u_begin = (int64_t)blockIdx.x * a.chunk;
  int64_t u_end = u_begin + a.chunk;
  if (u_end > a.units) u_end = a.units;
  v2f nx[NQ];   // nx[q] = (x[base + t0], x[base + t0 + 1]), t0 = 2 lane + 128 q; zero outside the row
  auto issue = [&](int64_t u) {
    const int64_t r = u / a.bpr, base = cwt_block_base(u - r * a.bpr, a.step, a.lead);
    const float* row = a.x + (size_t)r * a.x_stride;
    const bool wide = ((reinterpret_cast<uintptr_t>(row) + (uintptr_t)(base * 4)) & 7) == 0;   // wave-uniform
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t i = base + cwt_slot_pos(lane, q);
      const bool ok0 = i >= 0 && i < a.length, ok1 = i + 1 >= 0 && i + 1 < a.length;
      v2f v = v2f{0.f, 0.f};
      if (wide && ok0 && ok1) v = *reinterpret_cast<const v2f*>(row + i);
      else {
        if (ok0) v.x = row[i];
        if (ok1) v.y = row[i + 1];
      }
      nx[q] = v;
    }
  };
  if (u_begin + wave < u_end) issue(u_begin + wave);
  for (int64_t u = u_begin + wave; u < u_end; u += W) {
    const int64_t r = u / a.bpr, base = cwt_block_base(u - r * a.bpr, a.step, a.lead);
    v2f zz[2][NQ];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      bad = bad || cw_nonfinite(nx[q].x) || cw_nonfinite(nx[q].y);
      zz[0][q] = v2f{nx[q].x, 0.f};
      zz[1][q] = v2f{nx[q].y, 0.f};
    }
    if (bad) a.flags[r] = 1;   // a plain vector store; every lane that raises it writes the same value
    issue(u + W < u_end ? u + W : u);   // unconditional prefetch (the last iteration re-reads its own block)
    __builtin_amdgcn_sched_barrier(0);
    v2f d[P];
    wave_fft_core_T<K>(zz, d, xb, s_twB, s_twC, lane);   // d[s] = X[lane + 64 s], kept across the filters
    for (int f = 0; f < a.nf; ++f) {
      const v2f* Hf = a.H + (size_t)f * K;
      v2f e[P];
#pragma unroll
      for (int s = 0; s < P; ++s) e[s] = wcmul(d[s], Hf[cwt_bin(lane, s)]);
      v2f y[2][NQ];
      wave_fft_core<K, true, true>(e, y, xb, s_twB, s_twC, lane);   // unscaled inverse: y[par][q] = position 2 lane + par + 128 q
      __builtin_amdgcn_sched_barrier(0);
      const size_t orow = ((size_t)r * a.bank + (size_t)a.member[f]) * (size_t)a.length;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int t0 = cwt_slot_pos(lane, q);
        const bool v0 = cwt_pos_valid(t0, base, a.lead, a.step, a.length), v1 = cwt_pos_valid(t0 + 1, base, a.lead, a.step, a.length);
        if (!v0 && !v1) continue;
        const size_t at = orow + (size_t)(base + t0);   // of position t0 (not formed into a pointer unless v0)
        if constexpr (KIND == kCwComplex) {
          v2f* o = static_cast<v2f*>(a.out);
          if (v0 && v1 && ((reinterpret_cast<uintptr_t>(o + at) & 15) == 0))
            __builtin_nontemporal_store(v4f{y[0][q].x, y[0][q].y, y[1][q].x, y[1][q].y}, (gv4f*)(o + at));
          else {
            if (v0) o[at] = y[0][q];
            if (v1) o[at + 1] = y[1][q];
          }
        } else {
          float* o = static_cast<float*>(a.out);
          const float s0 = cw_sink<KIND>(y[0][q]), s1 = cw_sink<KIND>(y[1][q]);
          if (v0 && v1 && ((reinterpret_cast<uintptr_t>(o + at) & 7) == 0)) __builtin_nontemporal_store(v2f{s0, s1}, (gv2f*)(o + at));
          else {
            if (v0) o[at] = s0;
            if (v1) o[at + 1] = s1;
          }
        }
      }
    }
  }
}

// ---- the last pass: NaN over every output of a flagged row.  grid (blocks, rows); per_row counts f32 words
__global__ __launch_bounds__(kThreads) void k_cwt_poison(const int32_t* __restrict__ flags, int64_t per_row, float* __restrict__ out) {
  const int64_t r = blockIdx.y;
  if (flags[r] == 0) return;
  const float qnan = __uint_as_float(0x7fc00000u);
  float* o = out + (size_t)r * per_row;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < per_row; i += (int64_t)gridDim.x * kThreads) o[i] = qnan;
}

// ---- cwt.generic
// rows x_stride apart -> dense zero-padded c64 [rows][P]; raises the flag of a row that holds a non-finite sample
__global__ __launch_bounds__(kThreads) void k_cwt_pad(const float* __restrict__ x, int64_t x_stride, int64_t rows, int64_t n, int64_t P,
                                                     float2* __restrict__ out, int32_t* __restrict__ flags) {
  const int64_t total = rows * P;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / P, j = i - r * P;
    float v = 0.f;
    if (j < n) {   // nothing at or past n is read
      v = x[(size_t)r * x_stride + j];
      if (cw_nonfinite(v)) flags[r] = 1;
    }
    out[i] = make_float2(v, 0.f);
  }
}

// out[r][k] = z[r][k] H[k]
__global__ __launch_bounds__(kThreads) void k_cwt_mul(const float2* __restrict__ z, const float2* __restrict__ H, int64_t rows, int64_t P,
                                                     float2* __restrict__ out) {
  const int64_t total = rows * P;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t k = i % P;
    const float2 v = z[i], t = H[k];
    out[i] = make_float2(v.x * t.x - v.y * t.y, v.x * t.y + v.y * t.x);
  }
}

// out[r][s][n] = sink(y[r][n + center]): the "same" slice of filter s's full convolution [rows][P]
template <int KIND>
__global__ __launch_bounds__(kThreads) void k_cwt_slice(const float2* __restrict__ y, int64_t rows, int64_t P, int64_t n, int64_t center,
                                                       int64_t bank, int64_t s, void* __restrict__ out) {
  const int64_t total = rows * n;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / n, j = i - r * n;
    const float2 v = y[(size_t)r * P + j + center];
    const size_t at = ((size_t)r * bank + s) * n + j;
    if constexpr (KIND == kCwComplex) static_cast<float2*>(out)[at] = v;
    else static_cast<float*>(out)[at] = cw_sink<KIND>(v2f{v.x, v.y});
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// one of the family's own buffers, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does).
// zero: a fresh buffer is cleared (the flags, which every call leaves cleared)
int own_buffer(Ctx* c, Ctx::OwnedBuffer& b, size_t bytes, bool zero, void** out) {
  if (b.bytes < bytes) {
    if (b.ptr) {
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      NXSIG_HIP_TRY(hipFree(b.ptr));
      b.ptr = nullptr; b.bytes = 0;
    }
    NXSIG_HIP_TRY(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    if (zero) NXSIG_HIP_TRY(hipMemsetAsync(b.ptr, 0, bytes, c->stream));
  }
  *out = b.ptr;
  return NXSIG_OK;
}

// ---- the spectra of a class's filters on the device, f32 [nf][K], and the filters' bank indices, formed once per context, class and
// bank: the memo keeps the two pointers beside two independent hashes of the taps, so a repeated call makes no table request
struct CwtTables { const float2* H; const int32_t* member; };

int cwt_device_tables(Ctx* c, const CwtLaunch& a, const std::vector<int64_t>& offs, const std::vector<int32_t>& members, int64_t K, bool wave,
                      CwtTables* t) {
  uint64_t h1 = 0xC3770001ull, h2 = 0x9E3779B97F4A7C15ull;
  for (int32_t s : members) {
    const uint64_t head[2] = {(uint64_t)s, (uint64_t)a.tap_counts[s]};
    h1 = fnv1a(h1, head, sizeof head); h2 = fnv1a(h2, head, sizeof head);
    h1 = fnv1a(h1, a.taps_host + 2 * offs[s], (size_t)a.tap_counts[s] * 16);
    h2 = fnv1a(h2, a.taps_host + 2 * offs[s], (size_t)a.tap_counts[s] * 16);
  }
  std::vector<uint64_t> want = {0, 0, h2, (uint64_t)members.size(), (uint64_t)K, (uint64_t)wave};
  const uint64_t key = fnv1a(0xC3770000ull ^ h1, want.data() + 2, (want.size() - 2) * sizeof(uint64_t));
  auto hit = c->memo.find(key);
  if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 2, want.end(), hit->second.begin() + 2)) {
    t->H = reinterpret_cast<const float2*>((uintptr_t)hit->second[0]);
    t->member = reinterpret_cast<const int32_t*>((uintptr_t)hit->second[1]);
    return NXSIG_OK;
  }
  std::vector<float> Hf((size_t)2 * K * members.size());
  std::vector<double> work;
  for (size_t f = 0; f < members.size(); ++f) {
    const int64_t N = a.tap_counts[members[f]];
    cwt_spectrum(a.taps_host + 2 * offs[members[f]], N, K, wave ? cwt_center(N) : 0, wave ? 1.0 / (double)K : 1.0, work, Hf.data() + 2 * K * f);
  }
  const void *dH = nullptr, *dM = nullptr;
  int rc = ctx_table(c, 0xC3770A00ull, Hf.data(), Hf.size() * sizeof(float), &dH);
  if (rc) return rc;
  if ((rc = ctx_table(c, 0xC3770B00ull, members.data(), members.size() * sizeof(int32_t), &dM))) return rc;
  want[0] = (uint64_t)(uintptr_t)dH; want[1] = (uint64_t)(uintptr_t)dM;
  c->memo[key] = want;
  t->H = static_cast<const float2*>(dH); t->member = static_cast<const int32_t*>(dM);
  return NXSIG_OK;
}

template <int K, int KIND>
int run_wave_kind(Ctx* c, const CwtLaunch& a, const CwtTables& t, int64_t nf, int64_t Nmax, int32_t* flags) {
  constexpr int W = K == 2048 ? 2 : 4;
  Ctx::WaveTables& wt = c->wave_tables[K];
  CwtWaveArgs w;
  w.x = a.x; w.x_stride = a.x_stride; w.length = a.length;
  w.step = (int32_t)cwt_step(K, Nmax); w.lead = (int32_t)cwt_lead(Nmax);
  const int64_t bpr = cwt_blocks_per_row(a.length, w.step);
  w.bpr = (int32_t)bpr; w.units = a.batch * bpr; w.nf = (int32_t)nf; w.bank = a.num_filters;
  w.H = reinterpret_cast<const v2f*>(t.H); w.member = t.member;
  w.twB = reinterpret_cast<const v2f*>(wt.twB); w.twC = reinterpret_cast<const v2f*>(wt.twC);
  w.out = a.out; w.flags = flags;
  const int upw = tuned_units_per_wave(c, kT_WAVE_UNITS_PER_WAVE, w.units, W, 4);
  w.chunk = (int64_t)W * (upw < 1 ? 1 : upw);
  const int64_t blocks = (w.units + w.chunk - 1) / w.chunk;
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "cwt: too many blocks for one launch");
  hipLaunchKernelGGL((k_cwt_wave<K, W, KIND>), dim3((unsigned)blocks), dim3(64 * W), (size_t)cwt_lds_bytes(K), c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <int K>
int run_wave(Ctx* c, const CwtLaunch& a, const std::vector<int64_t>& offs, const std::vector<int32_t>& members, int64_t Nmax, int32_t* flags) {
  int rc = ensure_wave_tables(c, K);
  if (rc) return rc;
  CwtTables t;
  if ((rc = cwt_device_tables(c, a, offs, members, K, true, &t))) return rc;
  dispatch_note("cwt.wave");
  const int64_t nf = (int64_t)members.size();
  switch (a.kind) {
    case kCwComplex: return run_wave_kind<K, kCwComplex>(c, a, t, nf, Nmax, flags);
    case kCwReal: return run_wave_kind<K, kCwReal>(c, a, t, nf, Nmax, flags);
    case kCwMagnitude: return run_wave_kind<K, kCwMagnitude>(c, a, t, nf, Nmax, flags);
    default: return run_wave_kind<K, kCwPower>(c, a, t, nf, Nmax, flags);
  }
}

int run_generic(Ctx* c, const CwtLaunch& a, const std::vector<int64_t>& offs, const std::vector<int32_t>& members, int64_t Nmax, int32_t* flags) {
  const int64_t P = cwt_generic_length(a.length, Nmax), rows = a.batch, n = a.length;
  CwtTables t;
  int rc = cwt_device_tables(c, a, offs, members, P, false, &t);
  if (rc) return rc;
  const size_t bytes = (size_t)rows * P * sizeof(float2);
  void *rows_buf = nullptr, *spec = nullptr, *conv = nullptr;
  if ((rc = own_buffer(c, c->cwt_rows, bytes, false, &rows_buf))) return rc;
  if ((rc = own_buffer(c, c->cwt_spectra, bytes, false, &spec))) return rc;
  if ((rc = own_buffer(c, c->cwt_conv, bytes, false, &conv))) return rc;
  dispatch_note("cwt.generic");
  float2 *rb = static_cast<float2*>(rows_buf), *sp = static_cast<float2*>(spec), *cv = static_cast<float2*>(conv);
  hipLaunchKernelGGL(k_cwt_pad, dim3(stream_blocks(c, rows * P)), dim3(kThreads), 0, c->stream, a.x, a.x_stride, rows, n, P, rb, flags);
  NXSIG_HIP_TRY(hipGetLastError());
  if ((rc = launch_fft(c, rb, false, rows, (int32_t)P, (int32_t)P, false, sp, false))) return rc;
  for (size_t f = 0; f < members.size(); ++f) {
    const int64_t s = members[f], center = cwt_center(a.tap_counts[s]);
    hipLaunchKernelGGL(k_cwt_mul, dim3(stream_blocks(c, rows * P)), dim3(kThreads), 0, c->stream, sp, t.H + (size_t)f * P, rows, P, rb);
    NXSIG_HIP_TRY(hipGetLastError());
    if ((rc = launch_fft(c, rb, false, rows, (int32_t)P, (int32_t)P, true, cv, false))) return rc;   // the inverse carries its 1 / P
    const dim3 grid(stream_blocks(c, rows * n)), block(kThreads);
    switch (a.kind) {
      case kCwComplex: hipLaunchKernelGGL(k_cwt_slice<kCwComplex>, grid, block, 0, c->stream, cv, rows, P, n, center, a.num_filters, s, a.out); break;
      case kCwReal: hipLaunchKernelGGL(k_cwt_slice<kCwReal>, grid, block, 0, c->stream, cv, rows, P, n, center, a.num_filters, s, a.out); break;
      case kCwMagnitude: hipLaunchKernelGGL(k_cwt_slice<kCwMagnitude>, grid, block, 0, c->stream, cv, rows, P, n, center, a.num_filters, s, a.out); break;
      default: hipLaunchKernelGGL(k_cwt_slice<kCwPower>, grid, block, 0, c->stream, cv, rows, P, n, center, a.num_filters, s, a.out); break;
    }
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_cwt(Ctx* c, const CwtLaunch& a) {
  if (a.batch == 0 || a.num_filters == 0) return NXSIG_OK;
  const bool wave_off = tune(c, kT_CWT_WAVE, 1) == 0 || tune(c, kT_DISABLE_WAVE, 0) != 0;
  CwtGroups g;
  cwt_split(a.tap_counts, a.num_filters, wave_off, &g);
  std::vector<int64_t> offs((size_t)a.num_filters);
  int64_t at = 0;
  for (int64_t s = 0; s < a.num_filters; ++s) { offs[s] = at; at += a.tap_counts[s]; }
  void* flags = nullptr;
  int rc = own_buffer(c, c->cwt_flags, (size_t)kCwtMaxBatch * sizeof(int32_t), true, &flags);
  if (rc) return rc;
  int32_t* fl = static_cast<int32_t*>(flags);
  if (!g.members[kCwWave1024].empty() && (rc = run_wave<1024>(c, a, offs, g.members[kCwWave1024], g.longest[kCwWave1024], fl))) return rc;
  if (!g.members[kCwWave2048].empty() && (rc = run_wave<2048>(c, a, offs, g.members[kCwWave2048], g.longest[kCwWave2048], fl))) return rc;
  if (!g.members[kCwGeneric].empty() && (rc = run_generic(c, a, offs, g.members[kCwGeneric], g.longest[kCwGeneric], fl))) return rc;
  // the last pass: poison the flagged rows, clear the flags
  const int64_t per_row = a.num_filters * a.length * (a.kind == kCwComplex ? 2 : 1);
  const int64_t need = (per_row + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_cwt_poison, dim3((unsigned)(need < 64 ? need : 64), (unsigned)a.batch), dim3(kThreads), 0, c->stream, fl, per_row,
                     static_cast<float*>(a.out));
  NXSIG_HIP_TRY(hipGetLastError());
  NXSIG_HIP_TRY(hipMemsetAsync(fl, 0, (size_t)a.batch * sizeof(int32_t), c->stream));
  return NXSIG_OK;
}

}  // namespace nxsig
