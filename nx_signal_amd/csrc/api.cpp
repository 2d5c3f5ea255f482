// C-ABI entry points declared in include/nxsig.h.  Validates arguments the way the reference's
// deftransforms do (same failure cases -> NXSIG_ERR_INVALID_ARG, which the host mirrors turn into
// ArgumentError), resolves framing geometry, stages host buffers when asked to, and enqueues the HIP
// kernels on the context's stream.  No C++ exception may leave this file: every entry point is wrapped.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <thread>
#include <vector>
#ifdef __linux__
#include <sys/mman.h>
#endif

#include "nxsig_internal.h"
#include <strings.h>
#include <cstdio>

namespace nxsig {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const char* last_error_cstr() { return g_last_error.c_str(); }

static thread_local std::string g_dispatch;
void dispatch_reset() { g_dispatch.clear(); }
void dispatch_note(const char* family) {
  const std::string f(family);
  size_t at = 0;
  while ((at = g_dispatch.find(f, at)) != std::string::npos) {   // already noted (as a whole '+'-separated item)?
    const bool l = at == 0 || g_dispatch[at - 1] == '+', r = at + f.size() == g_dispatch.size() || g_dispatch[at + f.size()] == '+';
    if (l && r) return;
    at += f.size();
  }
  if (!g_dispatch.empty()) g_dispatch += '+';
  g_dispatch += f;
}
const char* dispatch_cstr() { return g_dispatch.c_str(); }
// one per compute entry point of the C ABI: resets the calling thread's record, and leaves a copy in the context on the way out (the
// BEAM's dirty schedulers move between threads from call to call: the NIF reads the context's copy)
struct DispatchScope {
  Ctx* c;
  explicit DispatchScope(Ctx* ctx) : c(ctx) { dispatch_reset(); }
  ~DispatchScope() { c->last_dispatch = g_dispatch; }
};
void dispatch_member_begin(Ctx* c) {
  std::lock_guard<std::mutex> lock(c->mu);
  dispatch_reset();
  c->last_dispatch.clear();
}

// In-process cache key (never persisted): FNV-1a over the tail bytes, and for the bulk four independent multiply-xor lanes over
// 8-byte words — a byte-at-a-time FNV costs one dependent multiply per byte, 0.7 ms for the 512 KB mel filterbank that
// stft_to_mel / mel_spectrogram look up on every call.
uint64_t fnv1a(uint64_t seed, const void* data, size_t bytes) {
  const uint64_t P = 1099511628211ull;
  uint64_t h = 1469598103934665603ull ^ seed;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  size_t i = 0;
  if (bytes >= 64) {
    uint64_t l0 = h ^ 0x9E3779B97F4A7C15ull, l1 = h ^ 0xC2B2AE3D27D4EB4Full, l2 = h ^ 0x165667B19E3779F9ull, l3 = h ^ 0x27D4EB2F165667C5ull;
    for (; i + 32 <= bytes; i += 32) {
      uint64_t w[4];
      std::memcpy(w, p + i, 32);
      l0 = (l0 ^ w[0]) * P; l0 ^= l0 >> 29;
      l1 = (l1 ^ w[1]) * P; l1 ^= l1 >> 29;
      l2 = (l2 ^ w[2]) * P; l2 ^= l2 >> 29;
      l3 = (l3 ^ w[3]) * P; l3 ^= l3 >> 29;
    }
    h = (((((l0 * P) ^ l1) * P) ^ l2) * P ^ l3) * P;
    h ^= h >> 32;
  }
  for (; i < bytes; ++i) {
    h ^= p[i];
    h *= P;
  }
  return h;
}

int make_framing(int64_t L, int32_t N, int32_t hop, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi, Framing* out) {
  if (N < 1) return set_error(NXSIG_ERR_INVALID_ARG, "window_length must be >= 1");
  if (hop < 1)  // lib/nx_signal.ex:282-284
    return set_error(NXSIG_ERR_INVALID_ARG, "expected an integer >= 1 or a list of integers, got: " + std::to_string(hop));
  if (L < 1) return set_error(NXSIG_ERR_INVALID_ARG, "signal length must be >= 1");
  Framing f;
  f.L = L; f.N = N; f.hop = hop; f.reflect = 0; f.lo = 0; f.hi = 0;
  switch (pad_mode) {
    case NXSIG_PAD_VALID: break;
    case NXSIG_PAD_REFLECT: f.reflect = 1; f.lo = N / 2; f.hi = N / 2; break;                 // :262
    case NXSIG_PAD_SAME: { const int64_t tot = N - 1; f.lo = tot / 2; f.hi = tot - tot / 2; } break;  // :308-312
    case NXSIG_PAD_EXPLICIT: f.lo = pad_lo; f.hi = pad_hi; break;
    default:  // :325-329
      return set_error(NXSIG_ERR_INVALID_ARG,
                       "invalid padding mode specified, padding must be one of :valid, :same, or a padding configuration");
  }
  const int64_t Lp = L + f.lo + f.hi;
  if (Lp < N)
    return set_error(NXSIG_ERR_INVALID_ARG, "window of length " + std::to_string(N) +
                                                " does not fit the (padded) signal of length " + std::to_string(Lp));
  f.M = (Lp - N) / hop + 1;  // pooled shape of Nx.window_max, :289-298
  *out = f;
  return NXSIG_OK;
}

int ctx_twiddles(Ctx* c, int K, const float2** out) {
  auto it = c->twiddles.find(K);
  if (it == c->twiddles.end()) {
    std::vector<float2> tw(K);
    for (int j = 0; j < K; ++j) {
      const double ang = -2.0 * 3.14159265358979323846 * (double)j / (double)K;
      tw[j] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    DeviceTable t;
    t.bytes = (size_t)K * sizeof(float2);
    NXSIG_HIP_TRY(hipMalloc(&t.ptr, t.bytes));
    NXSIG_HIP_TRY(hipMemcpyAsync(t.ptr, tw.data(), t.bytes, hipMemcpyHostToDevice, c->stream));
    NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));  // tw goes out of scope
    it = c->twiddles.emplace(K, t).first;
  }
  *out = reinterpret_cast<const float2*>(it->second.ptr);
  return NXSIG_OK;
}

int ctx_table(Ctx* c, uint64_t tag, const void* host, size_t bytes, const void** out) {
  // content-addressed: key = fnv1a(tag, content) ^ size.  A hit on a table of up to 1 MiB is VERIFIED against the kept host copy
  // (size + content): on a 64-bit collision the next key is probed instead of silently handing out another table (a wrong
  // window / filter).  Larger tables keep no host copy and are matched on hash + size only.
  uint64_t key = fnv1a(tag, host, bytes) ^ (uint64_t)bytes; ++c->table_requests;
  for (int probe = 0; probe < 8; ++probe, key = key * 0x9E3779B97F4A7C15ull + 1) {
    auto it = c->tables.find(key);
    if (it == c->tables.end()) {
      DeviceTable t;
      t.bytes = bytes;
      NXSIG_HIP_TRY(hipMalloc(&t.ptr, bytes ? bytes : 4));
      NXSIG_HIP_TRY(hipMemcpyAsync(t.ptr, host, bytes, hipMemcpyHostToDevice, c->stream));
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      t.has_host = bytes <= ((size_t)1 << 20);
      if (t.has_host) t.host.assign(static_cast<const unsigned char*>(host), static_cast<const unsigned char*>(host) + bytes);
      it = c->tables.emplace(key, std::move(t)).first;
      *out = it->second.ptr;
      return NXSIG_OK;
    }
    const DeviceTable& t = it->second;
    if (t.bytes == bytes && (!t.has_host || bytes == 0 || std::memcmp(t.host.data(), host, bytes) == 0)) {
      *out = t.ptr;
      return NXSIG_OK;
    }
  }
  return set_error(NXSIG_ERR_HIP, "table cache: repeated hash collisions");
}

static thread_local const Ctx* t_mel_defer = nullptr;
MelDeferScope::MelDeferScope(const Ctx* c) { t_mel_defer = c; }
MelDeferScope::~MelDeferScope() { t_mel_defer = nullptr; }
bool mel_deferred(const Ctx* c) { return t_mel_defer == c; }

int ctx_scratch(Ctx* c, ScratchSlot slot, size_t bytes, void** out) {
  if (c->scratch_bytes[slot] < bytes) {
    if (c->scratch[slot]) {
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      NXSIG_HIP_TRY(hipFree(c->scratch[slot]));
      c->scratch[slot] = nullptr;
      c->scratch_bytes[slot] = 0;
    }
    NXSIG_HIP_TRY(hipMalloc(&c->scratch[slot], bytes));
    c->scratch_bytes[slot] = bytes;
  }
  *out = c->scratch[slot];
  return NXSIG_OK;
}

int ctx_window(Ctx* c, const float* w, int N, int K, const float** dev, const float** devK) {
  if (c->memo_dev && c->memo_K == K && (int)c->memo_win.size() == N &&
      std::memcmp(c->memo_win.data(), w, (size_t)N * sizeof(float)) == 0) {
    *dev = c->memo_dev; *devK = c->memo_devK;
    return NXSIG_OK;
  }
  const void *d = nullptr, *dk = nullptr;
  int rc = ctx_table(c, 0x57494Eull, w, (size_t)N * sizeof(float), &d);
  if (rc) return rc;
  std::vector<float> padded((size_t)K, 0.0f);
  for (int i = 0; i < K && i < N; ++i) padded[i] = w[i];
  rc = ctx_table(c, 0x57494E4Bull, padded.data(), padded.size() * sizeof(float), &dk);
  if (rc) return rc;
  c->memo_win.assign(w, w + N);
  c->memo_K = K;
  c->memo_dev = reinterpret_cast<const float*>(d);
  c->memo_devK = reinterpret_cast<const float*>(dk);
  *dev = c->memo_dev; *devK = c->memo_devK;
  return NXSIG_OK;
}

// declared here, implemented in the .hip files
int launch_stft_generic(Ctx* c, const StftLaunch& a);
int launch_istft_generic(Ctx* c, const IstftLaunch& a);
int launch_fir_generic(Ctx* c, const FirLaunch& a);
int launch_stft_wave(Ctx* c, const StftLaunch& a, bool* handled);
int launch_istft_wave(Ctx* c, const IstftLaunch& a, const float* window_host, bool* handled);
int launch_fir_wave(Ctx* c, const FirLaunch& a, bool* handled);

// More rows than one launch takes (the bounds-checked and generic kernels put the row on gridDim.y, <= 65 535) run as slabs of 65 504
// rows — a multiple of 32, so that every slab's rows keep the first slab's alignment (FirWaveArgs::row_mod).  Rows are independent in
// stft / istft / fir; the sinks whose result depends on the whole tensor (log-mel, dBFS) keep the 65 535-row limit.
static constexpr int32_t kSlabRows = 65504;

int launch_stft(Ctx* c, const StftLaunch& a) {
  if (a.batch > kSlabRows) {
    for (int32_t r0 = 0; r0 < a.batch; r0 += kSlabRows) {
      StftLaunch b = a;
      b.batch = a.batch - r0 < kSlabRows ? a.batch - r0 : kSlabRows;
      b.x = a.x + (size_t)r0 * a.batch_stride;
      b.z = a.z + (size_t)r0 * a.fr.M * a.K;
      int rc = launch_stft(c, b);
      if (rc) return rc;
    }
    return NXSIG_OK;
  }
  bool handled = false;
  int rc = launch_stft_wave(c, a, &handled);
  if (rc || handled) return rc;
  return launch_stft_generic(c, a);
}
int launch_istft_packed_wave(Ctx* c, const IstftLaunch& a, const float* window_host, bool* handled);
int launch_istft(Ctx* c, const IstftLaunch& a, const float* window_host) {
  if (a.batch > kSlabRows && !a.onesided) {
    const int64_t out_len = a.M * a.hop + (a.N - a.hop);
    for (int32_t r0 = 0; r0 < a.batch; r0 += kSlabRows) {
      IstftLaunch b = a;
      b.batch = a.batch - r0 < kSlabRows ? a.batch - r0 : kSlabRows;
      b.z = a.z + (a.z_bcast ? 0 : (size_t)r0 * a.M * a.K);
      if (a.mask && !a.mask_bcast)
        b.mask = reinterpret_cast<const char*>(a.mask) +
                 (size_t)r0 * a.M * mask_row_len(a.mask_kind, a.K) * (a.mask_kind == NXSIG_MASK_COMPLEX ? sizeof(float2) : sizeof(float));
      b.y = a.y + (size_t)r0 * out_len;
      int rc2 = launch_istft(c, b, window_host);
      if (rc2) return rc2;
    }
    return NXSIG_OK;
  }
  bool handled = false;
  int rc;
  if (a.onesided) {  // packed half spectrum in, real signal out (nxsig_istft_packed_f32)
    if ((rc = launch_istft_packed_wave(c, a, window_host, &handled))) return rc;
    if (handled) {
      return launch_istft_fix(c, a, window_host);
    }
    // no fused kernel for this geometry: the Hermitian rows are written out, the complex path runs, its real part is kept
    const int64_t out_len = a.M * a.hop + (a.N - a.hop);
    void *zf = nullptr, *yf = nullptr;
    if ((rc = ctx_scratch(c, kScratchPackedSpectrum, (size_t)a.batch * a.M * a.K * sizeof(float2), &zf))) return rc;
    if ((rc = ctx_scratch(c, kScratchPackedSignal, (size_t)a.batch * out_len * sizeof(float2), &yf))) return rc;
    if ((rc = launch_full_from_packed(c, a.z, (int64_t)a.batch * a.M, a.K, reinterpret_cast<float2*>(zf)))) return rc;
    IstftLaunch b = a;
    b.onesided = false; b.z = reinterpret_cast<const float2*>(zf); b.y = reinterpret_cast<float2*>(yf);
    b.nf_list = nullptr; b.nf_frames_per_unit = 0;
    if ((rc = launch_istft(c, b, window_host))) return rc;
    return launch_real_from_c64(c, b.y, (int64_t)a.batch * out_len, reinterpret_cast<float*>(a.y));
  }
  rc = a.mask ? launch_istft_wave_mask(c, a, window_host, &handled) : launch_istft_wave(c, a, window_host, &handled);
  if (rc) return rc;
  if (!handled && a.mask) {
    // no fused kernel for this geometry: the masked spectrogram is materialised once (the two-step chain), then the size's own inverse runs
    void* zf = nullptr;
    if ((rc = ctx_scratch(c, kScratchIstftProduct, (size_t)a.batch * a.M * a.K * sizeof(float2), &zf))) return rc;
    if ((rc = launch_spectrum_mask(c, a.z, a.z_bcast, a.mask, a.mask_kind, a.mask_bcast, a.batch, a.M, a.K, reinterpret_cast<float2*>(zf)))) return rc;
    IstftLaunch b = a;
    b.z = reinterpret_cast<const float2*>(zf);
    b.mask = nullptr; b.z_bcast = false; b.mask_bcast = false;
    return launch_istft(c, b, window_host);
  }
  if (!handled && a.filt) {
    // no fused kernel for this geometry: the filter product is materialised once (the two-step chain), then the plain path runs
    void* zf = nullptr;
    if ((rc = ctx_scratch(c, kScratchIstftProduct, (size_t)a.batch * a.M * a.K * sizeof(float2), &zf))) return rc;
    if ((rc = launch_spectrum_mul(c, a.z, (int64_t)a.batch * a.M, a.K, a.filt, reinterpret_cast<float2*>(zf)))) return rc;
    IstftLaunch b = a;
    b.z = reinterpret_cast<const float2*>(zf);
    b.filt = nullptr;
    return launch_istft(c, b, window_host);
  }
  if (!handled && (rc = launch_istft_generic(c, a))) return rc;
  // ill-conditioned edge samples recomputed in double; kernels that invert several frames per transform reported their non-finite
  // units: those samples again, frame by frame (one launch for both)
  return launch_istft_fix(c, a, window_host);
}
// filters longer than the overlap-save kernels take (> 4096 taps: impulse responses of seconds): one transform of
// next_pow2(L + taps - 1) points per row, the way the reference's fftconvolve does it (lib/nx_signal/convolution.ex:252-329),
// through the device-side fft_nd fold (four-step rows up to 2^26 points); the requested slice is copied out of the full result
static int launch_fir_long(Ctx* c, const FirLaunch& a) {
  dispatch_note("fir.long");
  const int64_t full = a.L + a.taps - 1;
  if (full > ((int64_t)1 << 26))
    return set_error(NXSIG_ERR_UNSUPPORTED, "fir: more than 4096 taps with length + taps - 1 > 2^26 is not supported");
  const void* hd = nullptr;
  int rc = ctx_table(c, 0xF17A95ull ^ ((uint64_t)a.taps << 24), a.h_host, (size_t)a.taps * sizeof(float), &hd);
  if (rc) return rc;
  void* tmp = nullptr;
  if ((rc = ctx_scratch(c, kScratchFirLong, (size_t)full * sizeof(float), &tmp))) return rc;
  const int64_t s1 = a.L, s2 = a.taps;
  for (int32_t row = 0; row < a.batch; ++row) {
    if ((rc = launch_fftconvolve_nd(c, a.x + (size_t)row * a.batch_stride, true, &s1, hd, true, &s2, 1, NXSIG_CONV_FULL, tmp, nullptr))) return rc;
    NXSIG_HIP_TRY(hipMemcpyAsync(a.y + (size_t)row * a.out_len, static_cast<const float*>(tmp) + a.out_start, (size_t)a.out_len * sizeof(float),
                                 hipMemcpyDeviceToDevice, c->stream));
  }
  return NXSIG_OK;
}

int launch_fir_partition_sum(Ctx* c, int n, const float* const* src, const int64_t* i0, const int64_t* len, bool accumulate, bool clean, float scale,
                             float* y, int32_t batch, int64_t out_len);   // kernels_generic.hip

// 1 026 ... 32 768 taps (round 5): the filter is cut into P partitions of <= 1 025 taps (stride 256 ... 1 024), each one a FIR call of the tuned overlap-save
// kernels into a scratch tensor (full convolution of x with h[p S .. p S + taps_p), delayed by p S samples), and one pass sums them into
// y.  P x (8 B per sample at the 1 025-tap kernel's rate) + one (4 P + 4) B pass instead of the 8192-point workgroup kernel (0.05 of
// the roofline) or one 2^k-point transform per row (> 4 096 taps: 0.009).  Non-finite samples poison their row like everywhere else
// (FirLaunch::row_flags, shared by the partitions).  Scratch: at most ~4 GB per round of partitions; later rounds add to y.
// The reference's result is ONE Nx.ifft output: samples with |y| <= 1e-10 are exact zeros (convolution.ex:282).  The overlap-save
// kernels apply that clean-up to what they store — here partial sums, where it does not belong.  So the partitions run with h x 2^20
// (exact: the kernels' threshold then sits at 1e-16 of the true scale, far below what decides a sample of y), the summing pass
// multiplies by 2^-20 and cleans the finished sums.
static int launch_fir_partitioned(Ctx* c, const FirLaunch& a_in) {
  dispatch_note("fir.partitioned");
  FirLaunch a = a_in;
  int rc = fir_row_flags(c, a.batch, &a.row_flags);
  if (rc) return rc;
  constexpr float kUp = 1048576.0f, kDown = 1.0f / 1048576.0f;
  std::vector<float> hs((size_t)a.taps);
  for (int i = 0; i < a.taps; ++i) hs[i] = a.h_host[i] * kUp;
  // partition stride S: a multiple of 256 (the delays p S keep the rows' 16-byte alignment: the stream kernels decline unaligned
  // spans; and taps_p - 1 is what the real-block kernel pads to a multiple of 256 anyway); the last partition takes up to S + 1 taps
  const int P = (a.taps - 1 + 1023) / 1024;
  int S = ((a.taps - 1 + P - 1) / P + 255) / 256 * 256;
  if (S > 1024) S = 1024;
  const int64_t row_bytes = (int64_t)a.batch * (a.out_len + 4) * 4;
  int per_round = (int)(((int64_t)4 << 30) / (row_bytes > 0 ? row_bytes : 1));
  if (per_round < 1) per_round = 1;
  if (per_round > 8) per_round = 8;
  void* tmp = nullptr;
  const int n_parts = (a.taps - 1 + S - 1) / S;
  const int first_round = n_parts < per_round ? n_parts : per_round;
  if ((rc = ctx_scratch(c, kScratchFirLong, (size_t)first_round * (size_t)row_bytes, &tmp))) return rc;
  bool any = false;
  for (int p0 = 0; p0 < n_parts; p0 += per_round) {
    const float* src[8];
    int64_t i0s[8], lens[8];
    int n = 0;
    size_t off = 0;
    for (int p = p0; p < n_parts && p < p0 + per_round; ++p) {
      const int64_t delay = (int64_t)p * S;
      const int32_t taps_p = p == n_parts - 1 ? a.taps - p * S : S;
      const int64_t full_p = a.L + taps_p - 1;                       // length of x * h_p
      int64_t i0 = delay - a.out_start;                              // first output of y this partition reaches
      if (i0 < 0) i0 = 0;
      int64_t i1 = full_p - 1 + delay - a.out_start;                 // last one
      if (i1 > a.out_len - 1) i1 = a.out_len - 1;
      if (i1 < i0) continue;
      FirLaunch q = a;
      q.h_host = hs.data() + (size_t)p * S; q.taps = taps_p;
      q.out_start = a.out_start + i0 - delay;
      q.out_len = (i1 - i0 + 1 + 3) & ~(int64_t)3;   // whole 16-byte groups per row (the stream kernels decline unaligned rows); what lies
                                                      // beyond the partition's full convolution comes out as zeros
      q.y = reinterpret_cast<float*>(static_cast<char*>(tmp) + off);
      off += (size_t)a.batch * (size_t)q.out_len * 4;
      bool handled = false;
      if ((rc = launch_fir_wave(c, q, &handled))) return rc;
      if (!handled && (rc = launch_fir_generic(c, q))) return rc;
      src[n] = q.y; i0s[n] = i0; lens[n] = q.out_len; ++n;
    }
    const bool last = p0 + per_round >= n_parts;
    if (n == 0 && any && !last) continue;
    if ((rc = launch_fir_partition_sum(c, n, src, i0s, lens, any, last, kDown, a.y, a.batch, a.out_len))) return rc;
    any = true;
  }
  return launch_fir_poison(c, a);
}

int launch_fir(Ctx* c, const FirLaunch& a_in) {
  if (a_in.out_len <= 0 || a_in.batch == 0) return NXSIG_OK;
  if (a_in.batch > kSlabRows) {
    for (int32_t r0 = 0; r0 < a_in.batch; r0 += kSlabRows) {
      FirLaunch b = a_in;
      b.batch = a_in.batch - r0 < kSlabRows ? a_in.batch - r0 : kSlabRows;
      b.x = a_in.x + (size_t)r0 * a_in.batch_stride;
      b.y = a_in.y + (size_t)r0 * a_in.out_len;
      int rc = launch_fir(c, b);
      if (rc) return rc;
    }
    return NXSIG_OK;
  }
  if (a_in.taps > 32769) return launch_fir_long(c, a_in);   // one transform per row, like the reference: non-finite rows come out NaN
  if (a_in.taps > 1025 && !tune(c, kT_DISABLE_WAVE, 0) && tune(c, kT_FIR_DLINE, 1)) {
    // round 6: one forward transform per input block, the partitions applied as a frequency-domain delay line, one inverse per output
    // block (kernels_wave_firlong.hip); NXSIG_FIR_DLINE=0 keeps round 5's partition-by-partition form
    FirLaunch a = a_in;
    int rcd = fir_row_flags(c, a.batch, &a.row_flags);
    if (rcd) return rcd;
    bool hd = false;
    if ((rcd = launch_fir_dline(c, a, &hd))) return rcd;
    if (hd) return launch_fir_poison(c, a);
  }
  if (a_in.taps > 32768) return launch_fir_long(c, a_in);
  if (a_in.taps > 1025 && !tune(c, kT_DISABLE_WAVE, 0)) return launch_fir_partitioned(c, a_in);
  if (a_in.taps > 4096) return launch_fir_long(c, a_in);
  FirLaunch a = a_in;
  int rc = fir_row_flags(c, a.batch, &a.row_flags);
  if (rc) return rc;
  bool handled = false;
  rc = launch_fir_wave(c, a, &handled);
  if (rc) return rc;
  if (!handled && (rc = launch_fir_generic(c, a))) return rc;
  return launch_fir_poison(c, a);   // rows that held an Inf / NaN sample: NaN from end to end (FirLaunch::row_flags)
}

struct DeviceGuard {
  explicit DeviceGuard(Ctx* c) : lock(c->mu) {
    ok = (hipSetDevice(c->device) == hipSuccess);
    // bound the content-addressed table cache.  Done at API entry only, never while a call holds table pointers, and never
    // while the stream is being captured (a captured graph bakes table pointers in).  A graph captured EARLIER stays valid as
    // long as its context sees fewer than 1024 (NXSIG_TABLE_CACHE_MAX) distinct tables afterwards; beyond that re-capture it
    // (DESIGN.md section 3.0).  Every cache of pointers into `tables` is dropped with it: DESIGN.md lists them next to that sentence.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (ok && c->tables.size() > (size_t)tune(c, kT_TABLE_CACHE_MAX, kTableCacheMax) && hipStreamIsCapturing(c->stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) {
      (void)hipStreamSynchronize(c->stream);
      for (auto& kv : c->tables) (void)hipFree(kv.second.ptr);
      c->tables.clear();
      c->wave_tables.clear();
      c->f64_tables.clear();
      c->memo_dev = c->memo_devK = nullptr;
      c->memo.clear();
    }
  }
  std::lock_guard<std::mutex> lock;
  bool ok;
};

// the transfers of host signal buffers through scratch slots (convenience path, PCIe-bound); the entry points use it through HostIo
struct Staged {
  Ctx* c;
  explicit Staged(Ctx* ctx) : c(ctx) {}
  // ---- round 6: pinned bounce slots.  A pageable hipMemcpy runs at 13-32 GB/s on this platform (the runtime stages it through its own
  // small pinned buffers, single-threaded); a DMA between HBM and PINNED host memory runs at the link's ~56 GB/s.  So transfers of
  // kPinMin bytes or more go in chunks of kPinChunk through two pinned slots per direction: while the DMA engine moves chunk k + 1,
  // kCopyThreads host threads copy chunk k between the slot and the caller's buffer (which also takes the first-touch page faults of a
  // freshly allocated result, in parallel).  NXSIG_HOST_PIPE=1 selects it (n >= 2: n copy threads).  Results are the same bytes either way.
  static constexpr size_t kPinChunk = (size_t)32 << 20, kPinMin = (size_t)8 << 20;
  static constexpr unsigned kCopyThreads = 8;
  int ensure_pins() {
    if (c->pin_bytes) return NXSIG_OK;
    for (int i = 0; i < 4; ++i) {
      NXSIG_HIP_TRY(hipHostMalloc(&c->pin[i], kPinChunk, hipHostMallocDefault));
      NXSIG_HIP_TRY(hipEventCreateWithFlags(&c->xfer_ev[i], hipEventDisableTiming));
    }
    NXSIG_HIP_TRY(hipEventCreateWithFlags(&c->xfer_ready, hipEventDisableTiming));
    NXSIG_HIP_TRY(hipStreamCreateWithFlags(&c->xfer_stream, hipStreamNonBlocking));
    c->pin_bytes = kPinChunk;
    return NXSIG_OK;
  }
  void parallel_memcpy(char* dst, const char* src, size_t bytes) const {
    unsigned hw = std::thread::hardware_concurrency();
    const int knob = tune(c, kT_HOST_PIPE, 0);   // >= 2: that many copy threads (sweeps)
    const unsigned T = knob >= 2 ? (unsigned)knob : (hw >= 16 ? kCopyThreads : (hw >= 4 ? 2 : 1));
    // whole pages per thread, ROUNDED UP from bytes / T: rounded down, a chunk shorter than T bytes had per = 0 and was not copied at
    // all, and one whose bytes / T is a whole number of pages lost its last bytes % T bytes (32 MiB + 4 bytes of f32: the last sample)
    const size_t per = (((bytes + T - 1) / T) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) {
      const size_t o = (size_t)t * per;
      if (o < bytes) th.emplace_back([=] { std::memcpy(dst + o, src + o, bytes - o < per ? bytes - o : per); });
    }
    std::memcpy(dst, src, bytes < per ? bytes : per);
    for (auto& t : th) t.join();
  }
  // (default OFF: measured on 8 x config 2 — 92 MB up, 737 MB down, link floor 14.5 ms — the direct pageable copies with pre-faulting
  // below take 15.5 ms into a resident result buffer and 17.6 ms into a fresh one, this pipeline 16.3-16.5 / 16.9-17.5 ms: the runtime
  // pins resident user pages on the fly and DMAs straight into them, which the extra host copy cannot beat; profiles/r06/host_path.txt)
  bool piped(size_t bytes) const { return bytes >= kPinMin && tune(c, kT_HOST_PIPE, 0) != 0; }
  int in(ScratchSlot slot, const void* host, size_t bytes, const void** dev) {
    void* d = nullptr;
    int rc = ctx_scratch(c, slot, bytes ? bytes : 4, &d);
    if (rc) return rc;
    *dev = d;
    if (!piped(bytes)) {
      NXSIG_HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream));
      return NXSIG_OK;
    }
    if ((rc = ensure_pins())) return rc;
    // the scratch slot may still be read by work queued on the compute stream: the transfer stream starts behind it
    NXSIG_HIP_TRY(hipEventRecord(c->xfer_ready, c->stream));
    NXSIG_HIP_TRY(hipStreamWaitEvent(c->xfer_stream, c->xfer_ready, 0));
    const char* h = static_cast<const char*>(host);
    char* dd = static_cast<char*>(d);
    int k = 0;
    for (size_t off = 0; off < bytes; off += kPinChunk, ++k) {
      const size_t len = bytes - off < kPinChunk ? bytes - off : kPinChunk;
      const int sl = 2 + (k & 1);
      // the DMA that last read this slot is done — whichever in() queued it: a call's SECOND host operand starts at k = 0 again while
      // the first operand's last chunk may still be on its way out of the same slot (waiting only from k = 2 on let the host copy below
      // overwrite it).  An event nothing was recorded on yet counts as complete.
      NXSIG_HIP_TRY(hipEventSynchronize(c->xfer_ev[sl]));
      parallel_memcpy(static_cast<char*>(c->pin[sl]), h + off, len);
      NXSIG_HIP_TRY(hipMemcpyAsync(dd + off, c->pin[sl], len, hipMemcpyHostToDevice, c->xfer_stream));
      NXSIG_HIP_TRY(hipEventRecord(c->xfer_ev[sl], c->xfer_stream));
    }
    // the compute stream continues once the last chunk has landed
    NXSIG_HIP_TRY(hipEventRecord(c->xfer_ready, c->xfer_stream));
    NXSIG_HIP_TRY(hipStreamWaitEvent(c->stream, c->xfer_ready, 0));
    return NXSIG_OK;
  }
  int out_alloc(ScratchSlot slot, size_t bytes, void** dev) { return ctx_scratch(c, slot, bytes ? bytes : 4, dev); }
  // A pageable device-to-host copy runs at PCIe speed (56 GB/s measured) into RESIDENT pages but at 20-25 GB/s into a
  // freshly allocated result buffer (np.empty, enif_make_new_binary): first-touch page faults, taken one at a time
  // inside the copy.  So the result is copied in chunks, and while chunk k is on the wire a few threads pre-fault the
  // pages of chunk k+1 (MADV_POPULATE_WRITE, or a read-write touch that keeps the contents where madvise refuses).
  static void prefault_parallel(char* p, size_t bytes) {
    const uintptr_t page = 4096;
    uintptr_t a = (reinterpret_cast<uintptr_t>(p) + page - 1) & ~(page - 1);
    const uintptr_t e = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(page - 1);
    if (e <= a) return;
    unsigned hw = std::thread::hardware_concurrency();
    unsigned T = hw >= 8 ? 4 : 1;  // more threads contend on the process' mmap lock: 8 / 16 / 32 measured slower
    const size_t per = (((e - a) / T) + page - 1) & ~(size_t)(page - 1);
    auto work = [](uintptr_t s0, uintptr_t s1) {
      const uintptr_t page = 4096;
      if (s1 <= s0) return;
#ifdef __linux__
      if (madvise(reinterpret_cast<void*>(s0), s1 - s0, 23 /* MADV_POPULATE_WRITE */) == 0) return;
#endif
      for (uintptr_t q = s0; q < s1; q += page) { volatile char* b = reinterpret_cast<volatile char*>(q); *b = *b; }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) {
      const uintptr_t s0 = a + (uintptr_t)t * per, s1 = s0 + per < e ? s0 + per : e;
      if (s0 < e) th.emplace_back(work, s0, s1);
    }
    work(a, a + per < e ? a + per : e);
    for (auto& t : th) t.join();
  }
  int out_copy(void* host, const void* dev, size_t bytes) {
    if (piped(bytes)) return out_copy_piped(host, dev, bytes);
    const size_t CH = (size_t)32 << 20;
    if (bytes < ((size_t)32 << 20) || tune(c, kT_NO_PREFAULT, 0)) {
      NXSIG_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      return NXSIG_OK;
    }
    char* h = static_cast<char*>(host);
    const char* d = static_cast<const char*>(dev);
    prefault_parallel(h, bytes < CH ? bytes : CH);
    for (size_t off = 0; off < bytes; off += CH) {
      const size_t len = bytes - off < CH ? bytes - off : CH;
      std::thread pf;
      if (off + CH < bytes) {
        const size_t nlen = bytes - (off + CH) < CH ? bytes - (off + CH) : CH;
        pf = std::thread(prefault_parallel, h + off + CH, nlen);
      }
      hipError_t e1 = hipMemcpyAsync(h + off, d + off, len, hipMemcpyDeviceToHost, c->stream);
      hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(c->stream) : e1;
      if (pf.joinable()) pf.join();
      NXSIG_HIP_TRY(e2);
    }
    return NXSIG_OK;
  }
  // device -> pinned slot (DMA, transfer stream) -> caller's buffer (host threads), two slots: DMA of chunk k + 1 beside the copy of chunk k
  int out_copy_piped(void* host, const void* dev, size_t bytes) {
    int rc = ensure_pins();
    if (rc) return rc;
    NXSIG_HIP_TRY(hipEventRecord(c->xfer_ready, c->stream));             // the kernels that produce the result
    NXSIG_HIP_TRY(hipStreamWaitEvent(c->xfer_stream, c->xfer_ready, 0));
    char* h = static_cast<char*>(host);
    const char* d = static_cast<const char*>(dev);
    const size_t n = (bytes + kPinChunk - 1) / kPinChunk;
    auto len_of = [&](size_t k) { const size_t off = k * kPinChunk; return bytes - off < kPinChunk ? bytes - off : kPinChunk; };
    NXSIG_HIP_TRY(hipMemcpyAsync(c->pin[0], d, len_of(0), hipMemcpyDeviceToHost, c->xfer_stream));
    NXSIG_HIP_TRY(hipEventRecord(c->xfer_ev[0], c->xfer_stream));
    for (size_t k = 0; k < n; ++k) {
      const int sl = (int)(k & 1);
      if (k + 1 < n) {   // slot (k + 1) & 1 was emptied by the copy of chunk k - 1 (sequential below)
        NXSIG_HIP_TRY(hipMemcpyAsync(c->pin[sl ^ 1], d + (k + 1) * kPinChunk, len_of(k + 1), hipMemcpyDeviceToHost, c->xfer_stream));
        NXSIG_HIP_TRY(hipEventRecord(c->xfer_ev[sl ^ 1], c->xfer_stream));
      }
      NXSIG_HIP_TRY(hipEventSynchronize(c->xfer_ev[sl]));
      parallel_memcpy(h + k * kPinChunk, static_cast<const char*>(c->pin[sl]), len_of(k));
    }
    // later work on the compute stream may overwrite the scratch slot the result came from: it is behind the last DMA already
    // (every DMA was waited for above); nothing else to order
    return NXSIG_OK;
  }
};


// The tensor operands of one call (mem = NXSIG_HOST or NXSIG_DEVICE): device pointers pass through as they are, host pointers go through
// scratch slots — up to three inputs are uploaded by open(), up to three results are written by the kernels into their slots and
// copied back by close(), in the order they were listed.  in[] / out[] are the pointers to launch with either way.  A null input stays
// null (optional operands).  Results that share a slot are packed into it, each at the next 256-byte boundary.
struct HostIo {
  struct In { const void* p; size_t bytes; ScratchSlot slot; };
  // reserve: bytes to set aside when that is more than what is copied back (a result whose size the launcher decides: `bytes` is set
  // after the launch, before close(); the whole 256-byte units of a waveform result)
  struct Out { void* p; size_t bytes; ScratchSlot slot; size_t reserve = 0; };
  static constexpr int kMax = 3;
  Staged st;
  const bool host;
  bool plain_upload = false;   // uploads as one hipMemcpyAsync on the compute stream whatever NXSIG_HOST_PIPE says (the n-D calls)
  const void* in[kMax] = {};
  void* out[kMax] = {};
  Out outs[kMax] = {};
  int nout = 0;
  HostIo(Ctx* c, int32_t mem) : st(c), host(mem == NXSIG_HOST) {}
  int open(std::initializer_list<In> ins, std::initializer_list<Out> results) {
    int rc, j = 0;
    for (const In& i : ins) {
      in[j] = i.p;
      if (host && i.p) {
        if (!plain_upload) {
          if ((rc = st.in(i.slot, i.p, i.bytes, &in[j]))) return rc;
        } else {
          void* d = nullptr;
          if ((rc = ctx_scratch(st.c, i.slot, i.bytes, &d))) return rc;
          NXSIG_HIP_TRY(hipMemcpyAsync(d, i.p, i.bytes, hipMemcpyHostToDevice, st.c->stream));
          in[j] = d;
        }
      }
      ++j;
    }
    for (const Out& o : results) { outs[nout] = o; out[nout] = o.p; ++nout; }
    if (!host) return NXSIG_OK;
    for (int a = 0; a < nout; ++a) {
      bool first = true;
      for (int b = 0; b < a; ++b) first = first && outs[b].slot != outs[a].slot;
      if (!first) continue;
      size_t off[kMax] = {}, total = 0;
      for (int b = a; b < nout; ++b) {
        if (outs[b].slot != outs[a].slot) continue;
        off[b] = total = (total + 255) & ~(size_t)255;
        total += outs[b].reserve > outs[b].bytes ? outs[b].reserve : outs[b].bytes;
      }
      void* base = nullptr;
      if ((rc = st.out_alloc(outs[a].slot, total, &base))) return rc;
      for (int b = a; b < nout; ++b)
        if (outs[b].slot == outs[a].slot) out[b] = static_cast<char*>(base) + off[b];
    }
    return NXSIG_OK;
  }
  int close() {
    if (!host) return NXSIG_OK;
    for (int j = 0; j < nout; ++j) {
      const int rc = st.out_copy(outs[j].p, out[j], outs[j].bytes);
      if (rc) return rc;
    }
    return NXSIG_OK;
  }
  // one device-to-host copy by out_copy's rules (chunked, pre-faulting, piped), for a result that sits elsewhere than in out[]
  int download(void* host_dst, const void* dev, size_t bytes) { return st.out_copy(host_dst, dev, bytes); }
};
}  // namespace nxsig

using namespace nxsig;

#define NXSIG_CHECK_CTX(ctx)                                                            \
  if (!(ctx)) return set_error(NXSIG_ERR_INVALID_ARG, "null context");                  \
  Ctx* c = reinterpret_cast<Ctx*>(ctx);                                                 \
  DeviceGuard guard(c);                                                                 \
  if (!guard.ok) return set_error(NXSIG_ERR_HIP, "hipSetDevice failed");

namespace nxsig {
static const char* const kTuneNames[kTuneCount] = {
#define NXSIG_X(n) "NXSIG_" #n,
    NXSIG_TUNABLES(NXSIG_X)
#undef NXSIG_X
};
const char* tuning_name(int key) { return key >= 0 && key < kTuneCount ? kTuneNames[key] : ""; }
int tuning_index(const char* name) {
  if (!name) return -1;
  for (int k = 0; k < kTuneCount; ++k)
    if (!std::strcmp(name, kTuneNames[k]) || !std::strcmp(name, kTuneNames[k] + 6)) return k;
  return -1;
}
// Admissible values of a switch.  The geometry knobs end up as divisors or loop counts in the launchers (ISTFT_RUNS_PER_CU = 0 was an
// integer division by zero in launch_istft_wave_R), so they are range-checked HERE, once, for both ways in — the environment and
// nxsig_ctx_set_tuning — instead of at every use site; the on / off switches take any non-negative value.
static bool tuning_in_range(int k, long v, long* lo, long* hi) {
  long a = 0, b = 1L << 30;
  switch (k) {
    case kT_ISTFT_RUNS_PER_CU: a = 1; b = 4096; break;         // resident waves per CU the run length is derived from
    case kT_ISTFT_MIN_RUN: a = 1; b = 1 << 20; break;
    case kT_WAVE_UNITS_PER_WAVE: a = 1; b = 4096; break;
    case kT_FIR_UNITS_PER_WAVE: a = 1; b = 4096; break;
    case kT_MEL_LDS_KB: a = 1; b = 160; break;               // LDS per CU on gfx950
    case kT_FFT_TILE_ELEMS: a = 1024; b = 16384; break;
    case kT_FFT_TILE_NT: a = 64; b = 1024; break;
    case kT_FFT_TILED_MIN: a = 2; break;
    case kT_STORE_POLICY: a = 0; b = 2; break;
    case kT_FIR_R2K: a = 0; b = 2; break;
    case kT_TABLE_CACHE_MAX: a = 1; b = 1 << 20; break;       // tables a context keeps before the trim of DeviceGuard
    default: break;
  }
  if (lo) *lo = a;
  if (hi) *hi = b;
  return v >= a && v <= b;
}
// the library's ONE look at the process environment for its switches: at context creation, never in a launch.  A value that is not
// a number ("true", "on", "yes" / "false", "off", "no" aside, which mean 1 / 0) or lies outside the switch's range is IGNORED with
// one line on stderr — never silently read as 0.
void tuning_from_env(Tuning* t) {
  for (int k = 0; k < kTuneCount; ++k) {
    const char* v = std::getenv(kTuneNames[k]);
    if (!v || !*v) continue;
    char* end = nullptr;
    long val = std::strtol(v, &end, 10);
    while (end && (*end == ' ' || *end == '\t')) ++end;
    if (end == v || (end && *end)) {
      if (!strcasecmp(v, "true") || !strcasecmp(v, "on") || !strcasecmp(v, "yes")) val = 1;
      else if (!strcasecmp(v, "false") || !strcasecmp(v, "off") || !strcasecmp(v, "no")) val = 0;
      else { std::fprintf(stderr, "nxsig: %s=%s is not a number: ignored\n", kTuneNames[k], v); continue; }
    }
    long lo, hi;
    if (!tuning_in_range(k, val, &lo, &hi)) {
      std::fprintf(stderr, "nxsig: %s=%ld is outside [%ld, %ld]: ignored\n", kTuneNames[k], val, lo, hi);
      continue;
    }
    t->v[k] = (int32_t)val; t->set[k] = true;
  }
}
bool tuning_value_ok(int key, long value, long* lo, long* hi) { return tuning_in_range(key, value, lo, hi); }
}  // namespace nxsig

static int check_mem(int32_t mem) {
  if (mem != NXSIG_HOST && mem != NXSIG_DEVICE) return set_error(NXSIG_ERR_INVALID_ARG, "mem must be NXSIG_HOST or NXSIG_DEVICE");
  return NXSIG_OK;
}


/* ---------------------------------------------------------------- helpers of the compute entry points */
static int check_scaling(int32_t s) {
  if (s != NXSIG_SCALE_NONE && s != NXSIG_SCALE_SPECTRUM && s != NXSIG_SCALE_PSD)  // lib/nx_signal.ex:124-126, :622-624
    return set_error(NXSIG_ERR_INVALID_ARG, "invalid :scaling, expected one of :spectrum, :psd or nil");
  return NXSIG_OK;
}

// bytes of `batch` rows of `length` elements that lie batch_stride elements apart
static size_t rows_bytes(int32_t batch, int64_t batch_stride, int64_t length, size_t elem) {
  return ((size_t)(batch - 1) * batch_stride + length) * elem;
}

// ---- the prologue of the f32 STFT family (stft, stft_c64, stft_mel, stft_onesided / stft_packed, stft_magnitude), in two parts: a
// checker that needs no context and a planner that fills the launch.  Every entry point keeps its own NXSIG_CHECK_CTX: stft, stft_c64
// and stft_mel look at the context first, the others validate (and write *num_frames_out) first.
struct StftEntry {
  const char* name;             // prefix of the messages
  int32_t max_batch;            // 0 = unbounded (rows beyond one launch run as slabs, see launch_stft)
  int32_t min_fft_length;
  const char* fft_length_msg;   // what follows the prefix when fft_length is too short (or fft_length_also is set)
  bool extra_null = false;      // a pointer of the entry point's own (the mel filterbank) is null
  bool fft_length_also = false; // a condition of the entry point's own that shares the fft_length message (mel_bins < 1)
  const char* after_null = nullptr;  // a failed check of the entry point's own that sits right behind the null check: its whole message
  const char* after_mem = nullptr;   // the same, behind the check of `mem`
};

static int stft_check(const StftEntry& e, const void* x, const float* window, const nxsig_stft_params* p, const void* out, int64_t length,
                      int32_t batch, int64_t batch_stride, int32_t mem, Framing* fr, int64_t* num_frames_out) {
  auto bad = [&](const std::string& what) { return set_error(NXSIG_ERR_INVALID_ARG, std::string(e.name) + what); };
  if (!x || !window || !p || !out || e.extra_null) return bad(": null pointer argument");
  if (e.after_null) return set_error(NXSIG_ERR_INVALID_ARG, e.after_null);
  int rc = check_mem(mem);
  if (rc) return rc;
  if (e.after_mem) return set_error(NXSIG_ERR_INVALID_ARG, e.after_mem);
  if (batch < 1 || (e.max_batch && batch > e.max_batch))
    return bad(e.max_batch ? ": batch must be in [1, " + std::to_string(e.max_batch) + "]" : std::string(": batch must be >= 1"));
  if (batch_stride < length) return bad(": batch_stride < length");
  if (p->fft_length < e.min_fft_length || e.fft_length_also) return bad(e.fft_length_msg);
  if ((rc = check_scaling(p->scaling))) return rc;
  if ((rc = make_framing(length, p->frame_length, p->hop, p->pad_mode, p->pad_lo, p->pad_hi, fr))) return rc;
  if (num_frames_out) *num_frames_out = fr->M;
  return NXSIG_OK;
}

// everything of the launch but the operands: geometry, :scaling divisor, the window's device copies (a.x / a.z are the caller's)
static int stft_plan(Ctx* c, const Framing& fr, int32_t batch, int64_t batch_stride, const float* window, const nxsig_stft_params* p,
                     StftLaunch* a) {
  a->fr = fr; a->batch = batch; a->batch_stride = batch_stride; a->K = p->fft_length;
  a->has_scale = p->scaling != NXSIG_SCALE_NONE;
  a->inv_scale_div = a->has_scale ? scaling_factor(window, p->frame_length, p->scaling, p->sampling_rate) : 1.0f;
  a->x = nullptr; a->z = nullptr;
  return ctx_window(c, window, p->frame_length, p->fft_length, &a->window, &a->window_padK);
}

// nxsig_stft_f32 / nxsig_stft_c64: x_elem bytes per sample, the full spectrum out
static int stft_full(nxsig_ctx* ctx, const void* x, size_t x_elem, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                     const nxsig_stft_params* p, nxsig_c64* z, int64_t* num_frames_out, int32_t mem, int (*launch)(Ctx*, const StftLaunch&)) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  static const StftEntry e{"stft", 0, 1, ": fft_length must be >= 1"};
  Framing fr;
  int rc = stft_check(e, x, window, p, z, length, batch, batch_stride, mem, &fr, num_frames_out);
  if (rc) return rc;
  StftLaunch a;
  if ((rc = stft_plan(c, fr, batch, batch_stride, window, p, &a))) return rc;
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, x_elem), kScratchStageIn}},
                    {{z, (size_t)batch * fr.M * p->fft_length * sizeof(float2), kScratchStageOut}}))) return rc;
  a.x = static_cast<const float*>(io.in[0]); a.z = static_cast<float2*>(io.out[0]);
  if ((rc = launch(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

// The tail of the fused sinks (mel, one-sided / packed, magnitude): out_count results of out_elem bytes.  fused(a, out, &handled) tries
// the wave kernel that reduces in registers; when it declines, the full spectrum goes to a scratch slot and reduce(a, out) runs on it.
template <class Fused, class Reduce>
static int stft_fused_sink(Ctx* c, StftLaunch& a, const float* x, int64_t length, void* out, size_t out_elem, size_t out_count, int32_t mem,
                           Fused fused, Reduce reduce) {
  HostIo io(c, mem);
  int rc = io.open({{x, rows_bytes(a.batch, a.batch_stride, length, sizeof(float)), kScratchStageIn}}, {{out, out_count * out_elem, kScratchStageOut}});
  if (rc) return rc;
  a.x = static_cast<const float*>(io.in[0]);
  bool handled = false;
  if ((rc = fused(a, io.out[0], &handled))) return rc;
  if (!handled) {
    void* zs = nullptr;
    if ((rc = ctx_scratch(c, kScratchFusedSpectrum, (size_t)a.batch * a.fr.M * a.K * sizeof(float2), &zs))) return rc;
    a.z = reinterpret_cast<float2*>(zs);
    if ((rc = launch_stft(c, a))) return rc;
    if ((rc = reduce(a, io.out[0]))) return rc;
  }
  return io.close();
}

// nxsig_stft_onesided_f32 / nxsig_stft_packed_f32 (the messages carry the one-sided prefix for both, the parity check aside)
static int stft_onesided_impl(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                              const nxsig_stft_params* p, nxsig_c64* out, int64_t* num_frames_out, int32_t mem, bool packed) {
  NXSIG_API_BEGIN
  StftEntry e{"stft_onesided", 65535, 2, ": fft_length >= 2 required"};
  if (packed && p && (p->fft_length & 1)) e.after_null = "stft_packed: fft_length must be even";
  Framing fr;
  int rc = stft_check(e, x, window, p, out, length, batch, batch_stride, mem, &fr, num_frames_out);
  if (rc) return rc;
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  StftLaunch a;
  if ((rc = stft_plan(c, fr, batch, batch_stride, window, p, &a))) return rc;
  const int64_t rows = (int64_t)batch * fr.M;
  return stft_fused_sink(
      c, a, x, length, out, sizeof(float2), (size_t)rows * (p->fft_length / 2), mem,
      [&](const StftLaunch& s, void* od, bool* handled) {
        return launch_stft_mag_wave(c, s, packed ? 4 : 3 /* complex bins */, static_cast<float*>(od), handled);
      },
      [&](const StftLaunch& s, void* od) { return launch_half_from_spectrum(c, s.z, rows, s.K, static_cast<float2*>(od), packed); });
  NXSIG_API_END
}

// the operands of a time-frequency mask (nxsig_spectrum_mask_c64 / nxsig_istft_masked_c64)
struct MaskOperand {
  const void* mask = nullptr;
  int32_t kind = 0, z_rows = 1, mask_rows = 1;
};
static int check_mask(const char* fn, const MaskOperand& mo, int32_t K, int32_t* rows) {
  const std::string f(fn);
  if (!mo.mask) return set_error(NXSIG_ERR_INVALID_ARG, f + ": null mask");
  if (mo.kind != NXSIG_MASK_REAL && mo.kind != NXSIG_MASK_ONESIDED && mo.kind != NXSIG_MASK_COMPLEX)
    return set_error(NXSIG_ERR_INVALID_ARG, f + ": mask_kind must be NXSIG_MASK_REAL, NXSIG_MASK_ONESIDED or NXSIG_MASK_COMPLEX");
  if (mo.kind == NXSIG_MASK_ONESIDED && (K & 1)) return set_error(NXSIG_ERR_INVALID_ARG, f + ": a one-sided mask needs an even fft_length");
  if (mo.z_rows < 1 || mo.mask_rows < 1) return set_error(NXSIG_ERR_INVALID_ARG, f + ": z_rows and mask_rows must be >= 1");
  if (mo.z_rows != mo.mask_rows && mo.z_rows != 1 && mo.mask_rows != 1)
    return set_error(NXSIG_ERR_INVALID_ARG, f + ": z_rows and mask_rows must be equal, or one of them 1, got " + std::to_string(mo.z_rows) +
                                                " and " + std::to_string(mo.mask_rows));
  *rows = mo.z_rows > mo.mask_rows ? mo.z_rows : mo.mask_rows;
  if (*rows > 65535) return set_error(NXSIG_ERR_INVALID_ARG, f + ": at most 65535 rows");
  return NXSIG_OK;
}
static size_t mask_bytes(const MaskOperand& mo, int64_t num_frames, int32_t K) {
  return (size_t)mo.mask_rows * num_frames * mask_row_len(mo.kind, K) * (mo.kind == NXSIG_MASK_COMPLEX ? sizeof(float2) : sizeof(float));
}

static int istft_common(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                        const nxsig_stft_params* p, const nxsig_c64* h, nxsig_c64* y, int32_t mem, bool onesided = false,
                        const MaskOperand* mo = nullptr) {
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!z || !window || !p || !y) return set_error(NXSIG_ERR_INVALID_ARG, "istft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || (batch > 65535 && (onesided || h)))
    return set_error(NXSIG_ERR_INVALID_ARG, "istft: batch must be >= 1 (and <= 65535 for the packed and the filtered forms)");
  if (num_frames < 1) return set_error(NXSIG_ERR_INVALID_ARG, "istft: num_frames must be >= 1");
  rc = check_scaling(p->scaling);
  if (rc) return rc;
  const int N = p->frame_length, hop = p->hop, K = p->fft_length;
  if (N < 1 || hop < 1) return set_error(NXSIG_ERR_INVALID_ARG, "istft: frame_length and hop must be >= 1");
  if (hop > N)  // overlap_length < 0 cannot be expressed; overlap >= N -> hop <= 0 handled above (lib/nx_signal.ex:692-695)
    return set_error(NXSIG_ERR_INVALID_ARG, "overlap_length must be a number less than the window size");
  if (K != N)
    return set_error(NXSIG_ERR_INVALID_ARG,
                     "istft: fft_length must equal the window length (the reference broadcasts {M,K} x {N}, lib/nx_signal.ex:628)");
  if (onesided && (K & 1)) return set_error(NXSIG_ERR_INVALID_ARG, "istft_packed: fft_length must be even");
  IstftLaunch a;
  a.M = num_frames; a.batch = batch; a.N = N; a.hop = hop; a.K = K; a.onesided = onesided;
  a.has_scale = p->scaling != NXSIG_SCALE_NONE;
  a.scale_mul = a.has_scale ? scaling_factor(window, N, p->scaling, p->sampling_rate) : 1.0f;
  const void* wdev = nullptr;
  rc = ctx_table(c, 0x57494Eull, window, (size_t)N * sizeof(float), &wdev);
  if (rc) return rc;
  a.window = reinterpret_cast<const float*>(wdev);
  if (h) {  // same table key as spectrum_mul: the two-step and the fused form share the filter's device copy
    const void* hd = nullptr;
    if ((rc = ctx_table(c, 0x5BEC0ull ^ (uint64_t)K, h, (size_t)K * sizeof(float2), &hd))) return rc;
    a.filt = reinterpret_cast<const float2*>(hd);
  }
  const int64_t out_len = num_frames * hop + (N - hop);
  const size_t zbytes = (size_t)(mo ? mo->z_rows : batch) * num_frames * (onesided ? K / 2 : K) * sizeof(float2);
  const size_t ybytes = (size_t)batch * out_len * (onesided ? sizeof(float) : sizeof(float2));
  if (mo) {
    a.mask_kind = mo->kind;
    a.z_bcast = mo->z_rows == 1 && batch > 1; a.mask_bcast = mo->mask_rows == 1 && batch > 1;
  }
  HostIo io(c, mem);
  if ((rc = io.open({{z, zbytes, kScratchStageIn}, {mo ? mo->mask : nullptr, mo ? mask_bytes(*mo, num_frames, K) : 0, kScratchNdStageA}},
                    {{y, ybytes, kScratchStageOut}}))) return rc;
  a.z = static_cast<const float2*>(io.in[0]); a.mask = io.in[1]; a.y = static_cast<float2*>(io.out[0]);
  if ((rc = launch_istft(c, a, window))) return rc;
  return io.close();
}

// ---- what the f32 and the f64 tier of as_windowed / overlap_and_add / fir differ in: the launcher, the names in one message, and the
// FIR's row limit (f32: unbounded, rows beyond one launch run as slabs, see launch_fir)
template <class T> struct Tier;
template <> struct Tier<float> {
  static constexpr const char* kReal = "f32";
  static constexpr const char* kComplex = "c64";
  static constexpr int32_t kFirMaxBatch = 0;
  using Fir = FirLaunch;
  static int as_windowed(Ctx* c, const float* x, int64_t batch_stride, int32_t batch, const Framing& fr, float* out) {
    return launch_as_windowed(c, x, batch_stride, batch, fr, out);
  }
  static int overlap_and_add(Ctx* c, const float* frames, int64_t M, int32_t batch, int32_t N, int32_t hop, int32_t comps, float* out) {
    return launch_overlap_and_add(c, frames, M, batch, N, hop, comps, out);
  }
  static int fir(Ctx* c, const FirLaunch& a) { return launch_fir(c, a); }
};
template <> struct Tier<double> {
  static constexpr const char* kReal = "f64";
  static constexpr const char* kComplex = "c128";
  static constexpr int32_t kFirMaxBatch = 65535;
  using Fir = FirLaunchD;
  static int as_windowed(Ctx* c, const double* x, int64_t batch_stride, int32_t batch, const Framing& fr, double* out) {
    return launch_as_windowed_f64(c, x, batch_stride, batch, fr, out);
  }
  static int overlap_and_add(Ctx* c, const double* frames, int64_t M, int32_t batch, int32_t N, int32_t hop, int32_t comps, double* out) {
    return launch_ola_f64(c, frames, M, batch, N, hop, comps, nullptr, false, false, out);
  }
  static int fir(Ctx* c, const FirLaunchD& a) { return launch_fir_f64(c, a); }
};

template <class T>
static int as_windowed(nxsig_ctx* ctx, const T* x, int64_t length, int32_t batch, int64_t batch_stride, int32_t window_length, int32_t stride,
                       int32_t pad_mode, int64_t pad_lo, int64_t pad_hi, T* out, int64_t* num_frames_out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !out) return set_error(NXSIG_ERR_INVALID_ARG, "as_windowed: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || batch > 65535) return set_error(NXSIG_ERR_INVALID_ARG, "as_windowed: batch must be in [1, 65535]");
  if (batch_stride < length) return set_error(NXSIG_ERR_INVALID_ARG, "as_windowed: batch_stride < length");
  Framing fr;
  rc = make_framing(length, window_length, stride, pad_mode, pad_lo, pad_hi, &fr);
  if (rc) return rc;
  if (num_frames_out) *num_frames_out = fr.M;
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(T)), kScratchStageIn}},
                    {{out, (size_t)batch * fr.M * fr.N * sizeof(T), kScratchStageOut}}))) return rc;
  if ((rc = Tier<T>::as_windowed(c, static_cast<const T*>(io.in[0]), batch_stride, batch, fr, static_cast<T*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

template <class T>
static int overlap_and_add(nxsig_ctx* ctx, const T* frames, int64_t num_frames, int32_t batch, int32_t frame_length, int32_t overlap_length,
                           int32_t components, T* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!frames || !out) return set_error(NXSIG_ERR_INVALID_ARG, "overlap_and_add: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (components != 1 && components != 2)
    return set_error(NXSIG_ERR_INVALID_ARG, std::string("overlap_and_add: components must be 1 (") + Tier<T>::kReal + ") or 2 (" + Tier<T>::kComplex + ")");
  if (batch < 1 || batch > 65535 || num_frames < 1 || frame_length < 1)
    return set_error(NXSIG_ERR_INVALID_ARG, "overlap_and_add: batch, num_frames and frame_length must be >= 1");
  if (overlap_length >= frame_length)  // lib/nx_signal.ex:692-695 (message prints the window size twice, quirk B10)
    return set_error(NXSIG_ERR_INVALID_ARG, "overlap_length must be a number less than the window size " +
                                                std::to_string(frame_length) + ", got: " + std::to_string(frame_length));
  if (overlap_length < 0) return set_error(NXSIG_ERR_INVALID_ARG, "overlap_and_add: overlap_length must be >= 0");
  const int hop = frame_length - overlap_length;
  const int64_t out_len = num_frames * hop + overlap_length;
  HostIo io(c, mem);
  if ((rc = io.open({{frames, (size_t)batch * num_frames * frame_length * components * sizeof(T), kScratchStageIn}},
                    {{out, (size_t)batch * out_len * components * sizeof(T), kScratchStageOut}}))) return rc;
  if ((rc = Tier<T>::overlap_and_add(c, static_cast<const T*>(io.in[0]), num_frames, batch, frame_length, hop, components,
                                     static_cast<T*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

template <class T>
static int fir_common(nxsig_ctx* ctx, const T* x, int64_t length, int32_t batch, int64_t batch_stride, const T* h, int32_t num_taps,
                      int64_t start, int64_t out_len, T* y, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !h || !y) return set_error(NXSIG_ERR_INVALID_ARG, "fir: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || (Tier<T>::kFirMaxBatch && batch > Tier<T>::kFirMaxBatch) || length < 1 || num_taps < 1)
    return set_error(NXSIG_ERR_INVALID_ARG, "fir: batch, length and num_taps must be >= 1");
  if (batch_stride < length) return set_error(NXSIG_ERR_INVALID_ARG, "fir: batch_stride < length");
  if (start < 0 || out_len < 1 || start + out_len > length + num_taps - 1)
    return set_error(NXSIG_ERR_INVALID_ARG, "fir: requested slice lies outside the full convolution");
  typename Tier<T>::Fir a;
  a.L = length; a.batch = batch; a.batch_stride = batch_stride; a.h_host = h; a.taps = num_taps;
  a.out_start = start; a.out_len = out_len;
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(T)), kScratchStageIn}},
                    {{y, (size_t)batch * out_len * sizeof(T), kScratchStageOut}}))) return rc;
  a.x = static_cast<const T*>(io.in[0]); a.y = static_cast<T*>(io.out[0]);
  if ((rc = Tier<T>::fir(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

// the slice of the full 1-D convolution of n1 and n2 samples a mode names (lib/nx_signal/convolution.ex:300-329: centered(out, shape)
// starts at div(full - new, 2); an unknown mode: convolution.ex:41-44)
static int conv_slice(int64_t n1, int64_t n2, int32_t mode, int64_t* start, int64_t* out_len) {
  const int64_t full = n1 + n2 - 1;
  switch (mode) {
    case NXSIG_CONV_FULL: *out_len = full; break;
    case NXSIG_CONV_SAME: *out_len = n1; break;
    case NXSIG_CONV_VALID: *out_len = (n1 >= n2 ? n1 - n2 : n2 - n1) + 1; break;
    default: return set_error(NXSIG_ERR_INVALID_ARG, "expected mode to be one of [:full, :same, :valid]");
  }
  *start = (full - *out_len) / 2;
  return NXSIG_OK;
}

// nxsig_fir_f32 / _f64: the slice of the full convolution a mode names (its length checks come ahead of the context's)
template <class T>
static int fir_mode(nxsig_ctx* ctx, const T* x, int64_t length, int32_t batch, int64_t batch_stride, const T* h, int32_t num_taps, int32_t mode,
                    T* y, int32_t mem) {
  if (length < 1 || num_taps < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fir: batch, length and num_taps must be >= 1");
  int64_t out_len, start;
  const int rc = conv_slice(length, num_taps, mode, &start, &out_len);
  if (rc) return rc;
  return fir_common<T>(ctx, x, length, batch, batch_stride, h, num_taps, start, out_len, y, mem);
}

// nxsig_fftconvolve_nd / nxsig_convolve_direct: the same entry point around two launchers
typedef int (*ConvNdLaunch)(Ctx* c, const void* a, bool a_is_real, const int64_t* s1, const void* b, bool b_is_real, const int64_t* s2, int rank,
                            int mode, void* out, int64_t* out_shape);
static int conv_nd(const char* name, ConvNdLaunch launch, nxsig_ctx* ctx, const void* a, int32_t a_is_real, const int64_t* a_shape, const void* b,
                   int32_t b_is_real, const int64_t* b_shape, int32_t rank, int32_t mode, void* out, int64_t* out_shape, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const std::string f(name);
  if (!a || !b || !out || !a_shape || !b_shape) return set_error(NXSIG_ERR_INVALID_ARG, f + ": null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rank < 1 || rank > 8) return set_error(NXSIG_ERR_INVALID_ARG, f + ": rank must be in [1, 8]");
  if (mem == NXSIG_DEVICE) return launch(c, a, a_is_real != 0, a_shape, b, b_is_real != 0, b_shape, rank, mode, out, out_shape);
  int64_t na = 1, nb = 1, no = 1, osh[8];
  for (int d = 0; d < rank; ++d) {
    if (a_shape[d] < 1 || b_shape[d] < 1) return set_error(NXSIG_ERR_INVALID_ARG, f + ": empty dimension");
    na *= a_shape[d]; nb *= b_shape[d]; no *= a_shape[d] + b_shape[d] - 1;  // upper bound of every mode's result
  }
  const size_t out_elem = a_is_real && b_is_real ? 4 : 8;
  HostIo io(c, mem);
  io.plain_upload = true;
  if ((rc = io.open({{a, (size_t)na * (a_is_real ? 4 : 8), kScratchNdStageA}, {b, (size_t)nb * (b_is_real ? 4 : 8), kScratchNdStageB}},
                    {{out, 0, kScratchNdStageOut, (size_t)no * out_elem}}))) return rc;
  if ((rc = launch(c, io.in[0], a_is_real != 0, a_shape, io.in[1], b_is_real != 0, b_shape, rank, mode, io.out[0], osh))) return rc;
  int64_t nres = 1;
  for (int d = 0; d < rank; ++d) { nres *= osh[d]; if (out_shape) out_shape[d] = osh[d]; }
  io.outs[0].bytes = (size_t)nres * out_elem;
  return io.close();
  NXSIG_API_END
}

// Filters.median / wiener: the shape checks of filters.ex (and of the Nx.slice / Nx.conv they compose)
static int filter_shape(const char* fn, const int64_t* shape, int32_t rank, const int64_t* ks, int64_t* n) {
  if (rank < 1 || rank > 8) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": rank must be in [1, 8]");
  *n = 1;
  for (int d = 0; d < rank; ++d) {
    if (shape[d] < 1) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": empty dimension");
    if (ks[d] < 1) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": window lengths must be >= 1");
    *n *= shape[d];
  }
  return NXSIG_OK;
}

// PeakFinding.argrelextrema / nonzero: the port's limits
static int peaks_shape(const char* fn, const int64_t* shape, int32_t rank, int64_t* n) {
  if (!shape) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": null pointer argument");
  if (rank < 1 || rank > 8) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": rank must be in [1, 8]");
  *n = 1;
  for (int d = 0; d < rank; ++d) {
    if (shape[d] < 1) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": empty dimension");
    if (shape[d] >= ((int64_t)1 << 31)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": a dimension of 2^31 or more");
    *n *= shape[d];
    if (*n >= ((int64_t)1 << 32)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": 2^32 or more elements");
  }
  return NXSIG_OK;
}
// x in; out[0] = valid, out[1] = indices [n][rank] (`valid` travels back first)
static int peaks_open(HostIo& io, const void* x, size_t x_bytes, int64_t n, int32_t rank, int32_t* indices, uint32_t* valid) {
  return io.open({{x, x_bytes, kScratchNdStageA}}, {{valid, 4, kScratchNdStageB}, {indices, (size_t)n * rank * 4, kScratchNdStageOut}});
}

// NxSignal.Waveforms (lib/nx_signal/waveforms.ex): the reference's ArgumentErrors, the scalars that do not
// depend on t computed once under the tier's rounding (f32: every op in double on f32 operands, rounded to f32; f64: no rounding;
// pi() the f32 constant in both)
constexpr double kWavePi = 3.1415927410125732;   // Nx.Constants.pi() as f32
constexpr double kWaveTwoPi = 2.0 * kWavePi;     // 2 * pi(): exact

struct WaveRound {
  bool f64;
  double operator()(double x) const { return f64 ? x : (double)(float)x; }
};

static std::string wave_num(double v) {
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}

static int wave_args(const char* fn, const void* t, const void* out, int64_t n, int32_t mem) {
  if (n < 0) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": n must be >= 0");
  if (n > 0 && (!t || !out)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": null pointer argument");
  return check_mem(mem);
}
// a staged waveform result takes a whole number of 256-byte units of its slot
static size_t wave_span(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// t (and an optional second stream) of in_elem-byte elements in, one result of out_elem-byte elements out
static int wave_open(HostIo& io, const void* t, const void* second, size_t in_elem, int64_t n, void* out, size_t out_elem) {
  return io.open({{t, (size_t)n * in_elem, kScratchNdStageA}, {second, (size_t)n * in_elem, kScratchNdStageB}},
                 {{out, (size_t)n * out_elem, kScratchNdStageOut, wave_span((size_t)n * out_elem)}});
}

extern "C" {

int nxsig_abi_version(void) { return NXSIG_ABI_VERSION; }

const char* nxsig_last_error(void) { return last_error_cstr(); }
const char* nxsig_last_dispatch(void) { return dispatch_cstr(); }

int nxsig_device_count(int* count) {
  NXSIG_API_BEGIN
  if (!count) return set_error(NXSIG_ERR_INVALID_ARG, "count is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return set_error(NXSIG_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  *count = n;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_ctx_set_tuning(nxsig_ctx* ctx, const char* name, int32_t value) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  const int k = tuning_index(name);
  if (k < 0) return set_error(NXSIG_ERR_INVALID_ARG, std::string("no such switch: ") + (name ? name : "(null)"));
  long lo, hi;
  if (!tuning_value_ok(k, value, &lo, &hi))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string(tuning_name(k)) + " must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
  c->tuning.v[k] = value;   // (NXSIG_CHECK_CTX holds the context's mutex)
  c->tuning.set[k] = true;
  if (k == kT_POOL_MAX_MB) c->pool_cap = 0;  // decided again at the next nxsig_free
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_ctx_get_tuning(nxsig_ctx* ctx, const char* name, int32_t* value, int32_t* is_set) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  const int k = tuning_index(name); if (k < 0 && table_requests_query(c, name, value, is_set)) return NXSIG_OK;   // the read-only name
  if (k < 0) return set_error(NXSIG_ERR_INVALID_ARG, std::string("no such switch: ") + (name ? name : "(null)"));
  if (value) *value = c->tuning.v[k];
  if (is_set) *is_set = c->tuning.set[k] ? 1 : 0;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_ctx_clear_tuning(nxsig_ctx* ctx, const char* name) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (name == nullptr) { c->tuning = Tuning(); return NXSIG_OK; }
  const int k = tuning_index(name);
  if (k < 0) return set_error(NXSIG_ERR_INVALID_ARG, std::string("no such switch: ") + name);
  c->tuning.set[k] = false;
  c->tuning.v[k] = 0;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_ctx_create(int device, nxsig_ctx** out) {
  NXSIG_API_BEGIN
  if (!out) return set_error(NXSIG_ERR_INVALID_ARG, "out is null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return set_error(NXSIG_ERR_NO_DEVICE, "no ROCm-capable device: the nxsig hot path has no CPU fallback");
  if (device < 0 || device >= n) return set_error(NXSIG_ERR_INVALID_ARG, "device index out of range");
  NXSIG_HIP_TRY(hipSetDevice(device));
  Ctx* c = new Ctx();
  c->device = device;
  hipDeviceProp_t prop;
  NXSIG_HIP_TRY(hipGetDeviceProperties(&prop, device));
  c->num_cus = prop.multiProcessorCount;
  tuning_from_env(&c->tuning);
  c->dev_name = std::string(prop.name) + " " + prop.gcnArchName + " " + std::to_string(prop.multiProcessorCount) + " CUs";
  NXSIG_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  NXSIG_HIP_TRY(hipEventCreate(&c->ev_start));
  NXSIG_HIP_TRY(hipEventCreate(&c->ev_stop));
  *out = reinterpret_cast<nxsig_ctx*>(c);
  return NXSIG_OK;
  NXSIG_API_END
}

void nxsig_ctx_destroy(nxsig_ctx* ctx) {
  if (!ctx) return;
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  try {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->twiddles) (void)hipFree(kv.second.ptr);
    for (auto& kv : c->tables) (void)hipFree(kv.second.ptr);
    for (auto& s : c->scratch) if (s) (void)hipFree(s);
    for (auto& kv : c->pool_free) (void)hipFree(kv.second);
    for (auto& kv : c->pool_live) (void)hipFree(kv.first);   // blocks the caller never returned die with their context
    (void)hipEventDestroy(c->ev_start);
    (void)hipEventDestroy(c->ev_stop);
    for (auto e : c->lap_events) (void)hipEventDestroy(e);
    for (auto& pp : c->pin) if (pp) (void)hipHostFree(pp);
    for (auto& e : c->xfer_ev) if (e) (void)hipEventDestroy(e);
    if (c->xfer_ready) (void)hipEventDestroy(c->xfer_ready);
    if (c->xfer_stream) (void)hipStreamDestroy(c->xfer_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
  } catch (...) {
  }
  delete c;
}

int nxsig_ctx_last_dispatch(nxsig_ctx* ctx, char* buf, size_t buflen) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!buf || buflen == 0) return set_error(NXSIG_ERR_INVALID_ARG, "last_dispatch: buf is null");
  std::snprintf(buf, buflen, "%s", c->last_dispatch.c_str());
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_device_name(nxsig_ctx* ctx, char* buf, size_t buflen) {
  NXSIG_API_BEGIN
  if (!ctx || !buf || buflen == 0) return set_error(NXSIG_ERR_INVALID_ARG, "bad arguments");
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  std::strncpy(buf, c->dev_name.c_str(), buflen - 1);
  buf[buflen - 1] = 0;
  return NXSIG_OK;
  NXSIG_API_END
}

// ---- caching allocator (see Ctx::pool_free).  Blocks are rounded up to 2 MiB (256 B below 1 MiB) so that results of nearly equal
// sizes share blocks; a cached block serves a request when it is at most 12.5 % + 2 MiB larger.
static size_t pool_round(size_t bytes) {
  if (bytes < 4) bytes = 4;
  const size_t g = bytes < ((size_t)1 << 20) ? 256 : ((size_t)2 << 20);
  return (bytes + g - 1) / g * g;
}
static void pool_trim(Ctx* c, size_t keep) {   // releases cached blocks, largest first, until at most `keep` bytes stay cached
  if (c->pool_cached <= keep) return;
  (void)hipStreamSynchronize(c->stream);
  while (c->pool_cached > keep && !c->pool_free.empty()) {
    auto it = std::prev(c->pool_free.end());
    (void)hipFree(it->second);
    c->pool_cached -= it->first;
    c->pool_free.erase(it);
  }
}

int nxsig_alloc(nxsig_ctx* ctx, size_t bytes, void** dptr) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!dptr) return set_error(NXSIG_ERR_INVALID_ARG, "dptr is null");
  const size_t need = pool_round(bytes);
  auto it = c->pool_free.lower_bound(need);
  if (it != c->pool_free.end() && it->first <= need + need / 8 + ((size_t)2 << 20)) {
    *dptr = it->second;
    c->pool_live[it->second] = it->first;
    c->pool_cached -= it->first;
    c->pool_free.erase(it);
    return NXSIG_OK;
  }
  hipError_t e = hipMalloc(dptr, need);
  if (e != hipSuccess && !c->pool_free.empty()) {  // out of memory with blocks parked in the cache: give them back and retry
    (void)hipGetLastError();
    pool_trim(c, 0);
    e = hipMalloc(dptr, need);
  }
  NXSIG_HIP_TRY(e);
  c->pool_live[*dptr] = need;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_free(nxsig_ctx* ctx, void* dptr) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!dptr) return NXSIG_OK;
  auto it = c->pool_live.find(dptr);
  if (it == c->pool_live.end()) {  // not one of ours (or already released): plain free, after the stream has drained
    NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
    NXSIG_HIP_TRY(hipFree(dptr));
    return NXSIG_OK;
  }
  if (c->pool_cap == 0) {  // NXSIG_POOL_MAX_MB (0 disables caching); default: a quarter of the device memory
    size_t free_b = 0, total_b = 0;
    c->pool_cap = 1;
    if (c->tuning.set[kT_POOL_MAX_MB]) c->pool_cap = (size_t)(c->tuning.v[kT_POOL_MAX_MB] < 0 ? 0 : c->tuning.v[kT_POOL_MAX_MB]) << 20 | 1;
    else if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) c->pool_cap = total_b / 4 | 1;
  }
  const size_t sz = it->second;
  c->pool_live.erase(it);
  if (sz > c->pool_cap) {  // never cacheable
    NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
    NXSIG_HIP_TRY(hipFree(dptr));
    return NXSIG_OK;
  }
  c->pool_free.emplace(sz, dptr);
  c->pool_cached += sz;
  pool_trim(c, c->pool_cap);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_upload(nxsig_ctx* ctx, void* dst_device, const void* src_host, size_t bytes) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  NXSIG_HIP_TRY(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, c->stream));
  NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_download(nxsig_ctx* ctx, void* dst_host, const void* src_device, size_t bytes) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!dst_host || !src_device) return set_error(NXSIG_ERR_INVALID_ARG, "download: null pointer");
  // large results: chunked copy with the next chunk's pages pre-faulted (freshly allocated destinations)
  return HostIo(c, NXSIG_HOST).download(dst_host, src_device, bytes);
  NXSIG_API_END
}

int nxsig_sync(nxsig_ctx* ctx) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_mem_info(nxsig_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  size_t f = 0, t = 0;
  NXSIG_HIP_TRY(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_set_stream(nxsig_ctx* ctx, void* hip_stream) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->own_stream) NXSIG_HIP_TRY(hipStreamDestroy(c->stream));
  if (hip_stream) {
    c->stream = reinterpret_cast<hipStream_t>(hip_stream);
    c->own_stream = false;
  } else {
    NXSIG_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return NXSIG_OK;
  NXSIG_API_END
}

void* nxsig_get_stream(nxsig_ctx* ctx) { return ctx ? reinterpret_cast<Ctx*>(ctx)->stream : nullptr; }

int nxsig_timer_start(nxsig_ctx* ctx) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  NXSIG_HIP_TRY(hipEventRecord(c->ev_start, c->stream));
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_timer_stop(nxsig_ctx* ctx, float* elapsed_ms) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!elapsed_ms) return set_error(NXSIG_ERR_INVALID_ARG, "elapsed_ms is null");
  NXSIG_HIP_TRY(hipEventRecord(c->ev_stop, c->stream));
  NXSIG_HIP_TRY(hipEventSynchronize(c->ev_stop));
  NXSIG_HIP_TRY(hipEventElapsedTime(elapsed_ms, c->ev_start, c->ev_stop));
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_timer_lap(nxsig_ctx* ctx) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (c->laps_used >= 4096) return set_error(NXSIG_ERR_INVALID_ARG, "timer_lap: at most 4096 laps per series");
  if (c->laps_used == c->lap_events.size()) {
    hipEvent_t e;
    NXSIG_HIP_TRY(hipEventCreate(&e));
    c->lap_events.push_back(e);
  }
  NXSIG_HIP_TRY(hipEventRecord(c->lap_events[c->laps_used], c->stream));
  ++c->laps_used;
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_timer_laps(nxsig_ctx* ctx, float* intervals_ms, int32_t capacity, int32_t* count) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  if (!count || (capacity > 0 && !intervals_ms)) return set_error(NXSIG_ERR_INVALID_ARG, "timer_laps: null output");
  const size_t n = c->laps_used;
  c->laps_used = 0;
  *count = 0;
  if (n == 0) return NXSIG_OK;
  NXSIG_HIP_TRY(hipEventSynchronize(c->lap_events[n - 1]));
  for (size_t i = 0; i + 1 < n && (int32_t)i < capacity; ++i) {
    NXSIG_HIP_TRY(hipEventElapsedTime(&intervals_ms[i], c->lap_events[i], c->lap_events[i + 1]));
    *count = (int32_t)i + 1;
  }
  return NXSIG_OK;
  NXSIG_API_END
}

/* ---------------------------------------------------------------- shape helpers */
int32_t nxsig_next_pow2(int32_t n) {
  int32_t p = 1;
  while (p < n && p < (1 << 30)) p <<= 1;
  return p;
}

int64_t nxsig_num_frames(int64_t length, int32_t frame_length, int32_t hop, int32_t pad_mode, int64_t pad_lo,
                         int64_t pad_hi) {
  Framing f;
  int rc = make_framing(length, frame_length, hop, pad_mode, pad_lo, pad_hi, &f);
  return rc ? (int64_t)rc : f.M;
}

int64_t nxsig_ola_length(int64_t num_frames, int32_t frame_length, int32_t hop) {
  if (num_frames < 0 || frame_length < 1 || hop < 1 || hop > frame_length)
    return set_error(NXSIG_ERR_INVALID_ARG, "ola_length: need num_frames >= 0 and 1 <= hop <= frame_length");
  return num_frames * hop + (frame_length - hop);
}

int64_t nxsig_conv_length(int64_t n1, int64_t n2, int32_t mode) {
  if (n1 < 1 || n2 < 1) return set_error(NXSIG_ERR_INVALID_ARG, "conv_length: lengths must be >= 1");
  switch (mode) {
    case NXSIG_CONV_FULL: return n1 + n2 - 1;
    case NXSIG_CONV_SAME: return n1;
    case NXSIG_CONV_VALID: return (n1 >= n2 ? n1 - n2 : n2 - n1) + 1;
    default: return set_error(NXSIG_ERR_INVALID_ARG, "expected mode to be one of [:full, :same, :valid]");
  }
}

static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

int64_t nxsig_resample_length(int64_t length, int32_t up, int32_t down) {
  if (length < 0) return set_error(NXSIG_ERR_INVALID_ARG, "resample_length: length must be >= 0");
  if (up < 1 || down < 1) return set_error(NXSIG_ERR_INVALID_ARG, "resample_length: up and down must be >= 1");
  const int64_t g = gcd64(up, down);
  const unsigned __int128 v = ((unsigned __int128)length * (uint64_t)(up / g) + (uint64_t)(down / g) - 1) / (uint64_t)(down / g);
  if (v > (unsigned __int128)INT64_MAX) return set_error(NXSIG_ERR_INVALID_ARG, "resample_length: the result does not fit 64 bits");
  return (int64_t)v;
}

int32_t nxsig_resample_tile(void) { return kResampleTile; }

/* ---------------------------------------------------------------- host generators */
int nxsig_window_f32(int32_t kind, int32_t n, int32_t is_periodic, double beta, double eps, float* out) {
  NXSIG_API_BEGIN
  return window_f32(kind, n, is_periodic != 0, beta, eps, out);
  NXSIG_API_END
}

int nxsig_sinc_f32(const float* t, int64_t n, float* out) {
  NXSIG_API_BEGIN
  if (n < 0 || (n > 0 && (!t || !out))) return set_error(NXSIG_ERR_INVALID_ARG, "sinc: bad arguments");
  sinc_f32(t, n, out);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_firwin_f32(int32_t num_taps, const double* cutoff, int32_t n_cutoff, int32_t window_kind, double kaiser_beta,
                     int32_t pass_zero, int32_t scale, double sampling_rate, float* out) {
  NXSIG_API_BEGIN
  return firwin_f32(num_taps, cutoff, n_cutoff, window_kind, kaiser_beta, pass_zero != 0, scale != 0, sampling_rate, out);
  NXSIG_API_END
}

int nxsig_fft_frequencies_f32(double sampling_rate, int32_t fft_length, int32_t endpoint, float* out) {
  NXSIG_API_BEGIN
  if (fft_length < 1 || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fft_frequencies: fft_length must be >= 1");
  fft_frequencies_f32(sampling_rate, fft_length, endpoint != 0, out);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_stft_times_f32(int32_t frame_length, double sampling_rate, int64_t num_frames, float* out) {
  NXSIG_API_BEGIN
  if (num_frames < 0 || (num_frames > 0 && !out)) return set_error(NXSIG_ERR_INVALID_ARG, "stft_times: bad arguments");
  stft_times_f32(frame_length, sampling_rate, num_frames, out);
  return NXSIG_OK;
  NXSIG_API_END
}

/* ---------------------------------------------------------------- hot path */
int nxsig_stft_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                   const float* window, const nxsig_stft_params* p, nxsig_c64* z, int64_t* num_frames_out, int32_t mem) {
  return stft_full(ctx, x, sizeof(float), length, batch, batch_stride, window, p, z, num_frames_out, mem, launch_stft);
}

int nxsig_stft_c64(nxsig_ctx* ctx, const nxsig_c64* x, int64_t length, int32_t batch, int64_t batch_stride,
                   const float* window, const nxsig_stft_params* p, nxsig_c64* z, int64_t* num_frames_out, int32_t mem) {
  return stft_full(ctx, x, sizeof(float2), length, batch, batch_stride, window, p, z, num_frames_out, mem, launch_stft_c64);
}

int nxsig_istft_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                    const nxsig_stft_params* p, nxsig_c64* y, int32_t mem) {
  NXSIG_API_BEGIN
  return istft_common(ctx, z, num_frames, batch, window, p, nullptr, y, mem);
  NXSIG_API_END
}

int nxsig_istft_packed_f32(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                           const nxsig_stft_params* p, float* y, int32_t mem) {
  NXSIG_API_BEGIN
  return istft_common(ctx, z, num_frames, batch, window, p, nullptr, reinterpret_cast<nxsig_c64*>(y), mem, true);
  NXSIG_API_END
}

int nxsig_istft_filtered_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                             const nxsig_stft_params* p, const nxsig_c64* h, nxsig_c64* y, int32_t mem) {
  NXSIG_API_BEGIN
  if (!h) return set_error(NXSIG_ERR_INVALID_ARG, "istft_filtered: null filter spectrum");
  return istft_common(ctx, z, num_frames, batch, window, p, h, y, mem);
  NXSIG_API_END
}

int nxsig_istft_masked_c64(nxsig_ctx* ctx, const nxsig_c64* z, int32_t z_rows, int64_t num_frames, const float* window,
                           const nxsig_stft_params* p, const void* mask, int32_t mask_kind, int32_t mask_rows, nxsig_c64* y, int32_t mem) {
  NXSIG_API_BEGIN
  if (!p) return set_error(NXSIG_ERR_INVALID_ARG, "istft: null pointer argument");
  MaskOperand mo;
  mo.mask = mask; mo.kind = mask_kind; mo.z_rows = z_rows; mo.mask_rows = mask_rows;
  int32_t rows = 0;
  int rc = check_mask("istft_masked", mo, p->fft_length, &rows);
  if (rc) return rc;
  return istft_common(ctx, z, num_frames, rows, window, p, nullptr, y, mem, false, &mo);
  NXSIG_API_END
}

int nxsig_spectrum_mask_c64(nxsig_ctx* ctx, const nxsig_c64* z, int32_t z_rows, const void* mask, int32_t mask_kind, int32_t mask_rows,
                            int64_t num_frames, int32_t fft_length, nxsig_c64* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!z || !out) return set_error(NXSIG_ERR_INVALID_ARG, "spectrum_mask: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (num_frames < 1 || fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "spectrum_mask: num_frames and fft_length must be >= 1");
  MaskOperand mo;
  mo.mask = mask; mo.kind = mask_kind; mo.z_rows = z_rows; mo.mask_rows = mask_rows;
  int32_t rows = 0;
  if ((rc = check_mask("spectrum_mask", mo, fft_length, &rows))) return rc;
  const bool zb = z_rows == 1 && rows > 1, mb = mask_rows == 1 && rows > 1;
  HostIo io(c, mem);
  if ((rc = io.open({{z, (size_t)z_rows * num_frames * fft_length * sizeof(float2), kScratchStageIn},
                     {mask, mask_bytes(mo, num_frames, fft_length), kScratchNdStageA}},
                    {{out, (size_t)rows * num_frames * fft_length * sizeof(float2), kScratchStageOut}}))) return rc;
  if ((rc = launch_spectrum_mask(c, static_cast<const float2*>(io.in[0]), zb, io.in[1], mask_kind, mb, rows, num_frames, fft_length,
                                 static_cast<float2*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_as_windowed_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                          int32_t window_length, int32_t stride, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi,
                          float* out, int64_t* num_frames_out, int32_t mem) {
  return as_windowed<float>(ctx, x, length, batch, batch_stride, window_length, stride, pad_mode, pad_lo, pad_hi, out, num_frames_out, mem);
}

int nxsig_overlap_and_add(nxsig_ctx* ctx, const float* frames, int64_t num_frames, int32_t batch, int32_t frame_length,
                          int32_t overlap_length, int32_t components, float* out, int32_t mem) {
  return overlap_and_add<float>(ctx, frames, num_frames, batch, frame_length, overlap_length, components, out, mem);
}

int nxsig_fft(nxsig_ctx* ctx, const void* in, int32_t in_is_real, int64_t rows, int32_t n_in, int32_t fft_length,
              int32_t inverse, nxsig_c64* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!in || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rows < 1 || n_in < 1 || fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fft: rows, n_in and fft_length must be >= 1");
  HostIo io(c, mem);
  if ((rc = io.open({{in, (size_t)rows * n_in * (in_is_real ? sizeof(float) : sizeof(float2)), kScratchStageIn}},
                    {{out, (size_t)rows * fft_length * sizeof(float2), kScratchStageOut}}))) return rc;
  if ((rc = launch_fft(c, io.in[0], in_is_real != 0, rows, n_in, fft_length, inverse != 0, static_cast<float2*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_fir_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* h,
                  int32_t num_taps, int32_t mode, float* y, int32_t mem) {
  return fir_mode<float>(ctx, x, length, batch, batch_stride, h, num_taps, mode, y, mem);
}

int nxsig_fir_slice_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* h,
                        int32_t num_taps, int64_t out_start, int64_t out_len, float* y, int32_t mem) {
  return fir_common<float>(ctx, x, length, batch, batch_stride, h, num_taps, out_start, out_len, y, mem);
}

int nxsig_fft_nd(nxsig_ctx* ctx, const void* in, int32_t in_is_real, const int64_t* shape, int32_t rank, const int32_t* axes,
                 const int64_t* lengths, int32_t n_axes, int32_t inverse, nxsig_c64* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!in || !out || !shape || (n_axes > 0 && (!axes || !lengths))) return set_error(NXSIG_ERR_INVALID_ARG, "fft_nd: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rank < 1 || rank > 8 || n_axes < 0 || n_axes > 16) return set_error(NXSIG_ERR_INVALID_ARG, "fft_nd: rank must be in [1, 8]");
  std::vector<int64_t> osh(shape, shape + rank);
  int64_t n_in = 1, n_out = 1;
  for (int d = 0; d < rank; ++d) { if (shape[d] < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fft_nd: empty dimension"); n_in *= shape[d]; }
  for (int i = 0; i < n_axes; ++i) {
    const int ax = axes[i] < 0 ? axes[i] + rank : axes[i];
    if (ax < 0 || ax >= rank) return set_error(NXSIG_ERR_INVALID_ARG, "fft_nd: axis out of bounds");
    if (lengths[i] < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fft_nd: lengths must be positive");
    osh[ax] = lengths[i];
  }
  for (auto v : osh) n_out *= v;
  HostIo io(c, mem);
  io.plain_upload = true;
  if ((rc = io.open({{in, (size_t)n_in * (in_is_real ? sizeof(float) : sizeof(float2)), kScratchNdStageA}},
                    {{out, (size_t)n_out * sizeof(float2), kScratchNdStageB}}))) return rc;
  if ((rc = launch_fft_nd(c, io.in[0], in_is_real != 0, shape, rank, axes, lengths, n_axes, inverse != 0, static_cast<float2*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_fftconvolve_nd(nxsig_ctx* ctx, const void* a, int32_t a_is_real, const int64_t* a_shape, const void* b, int32_t b_is_real,
                         const int64_t* b_shape, int32_t rank, int32_t mode, void* out, int64_t* out_shape, int32_t mem) {
  return conv_nd("fftconvolve", launch_fftconvolve_nd, ctx, a, a_is_real, a_shape, b, b_is_real, b_shape, rank, mode, out, out_shape, mem);
}

int nxsig_convolve_direct(nxsig_ctx* ctx, const void* a, int32_t a_is_real, const int64_t* a_shape, const void* b, int32_t b_is_real,
                          const int64_t* b_shape, int32_t rank, int32_t mode, void* out, int64_t* out_shape, int32_t mem) {
  return conv_nd("convolve", launch_convolve_direct, ctx, a, a_is_real, a_shape, b, b_is_real, b_shape, rank, mode, out, out_shape, mem);
}

int nxsig_median_filter(nxsig_ctx* ctx, const void* x, int32_t is_f64, const int64_t* shape, int32_t rank, const int64_t* kernel_shape,
                        float* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !out || !shape || !kernel_shape) return set_error(NXSIG_ERR_INVALID_ARG, "median: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  int64_t n = 0;
  if ((rc = filter_shape("median", shape, rank, kernel_shape, &n))) return rc;
  for (int d = 0; d < rank; ++d)   // Nx.slice: a window longer than its axis
    if (kernel_shape[d] > shape[d])
      return set_error(NXSIG_ERR_INVALID_ARG, "median: kernel_shape " + std::to_string(kernel_shape[d]) + " exceeds dimension " +
                                                  std::to_string(shape[d]) + " of axis " + std::to_string(d));
  HostIo io(c, mem);
  if ((rc = io.open({{x, (size_t)n * (is_f64 ? 8 : 4), kScratchNdStageA}}, {{out, (size_t)n * 4, kScratchNdStageOut}}))) return rc;
  if ((rc = launch_median(c, io.in[0], is_f64 != 0, shape, rank, kernel_shape, static_cast<float*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_resample_poly(nxsig_ctx* ctx, const void* x, int32_t is_complex, int64_t length, int32_t batch, int64_t batch_stride,
                        const float* h, int32_t num_taps, int32_t up, int32_t down, void* y, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !h || !y) return set_error(NXSIG_ERR_INVALID_ARG, "resample_poly: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "resample_poly: batch and length must be >= 1");
  if (batch_stride < length) return set_error(NXSIG_ERR_INVALID_ARG, "resample_poly: batch_stride < length");
  if (up < 1 || down < 1) return set_error(NXSIG_ERR_INVALID_ARG, "resample_poly: up and down must be >= 1");
  if (num_taps < 1) return set_error(NXSIG_ERR_INVALID_ARG, "resample_poly: the tap vector is empty");
  const int32_t g = (int32_t)gcd64(up, down);
  const int64_t n_out = nxsig_resample_length(length, up, down);
  if (n_out < 0) return (int)n_out;
  if (n_out > INT64_MAX / batch / 8) return set_error(NXSIG_ERR_UNSUPPORTED, "resample_poly: the result is too large");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const size_t elem = is_complex ? sizeof(float2) : sizeof(float);
  ResampleLaunch a;
  a.is_complex = is_complex != 0; a.n = length; a.batch_stride = batch_stride; a.n_out = n_out; a.batch = batch;
  a.h_host = h; a.taps = num_taps; a.up = up / g; a.down = down / g;
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, elem), kScratchStageIn}},
                    {{y, (size_t)batch * n_out * elem, kScratchStageOut}}))) return rc;
  a.x = io.in[0]; a.y = io.out[0];
  if ((rc = a.up == a.down ? launch_resample_copy(c, a) : launch_resample_poly(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_wiener(nxsig_ctx* ctx, const void* x, int32_t is_f64, const int64_t* shape, int32_t rank, const int64_t* kernel_size, int32_t has_noise,
                 double noise, void* out, double* noise_used, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !out || !shape || !kernel_size) return set_error(NXSIG_ERR_INVALID_ARG, "wiener: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  int64_t n = 0;
  if ((rc = filter_shape("wiener", shape, rank, kernel_size, &n))) return rc;
  const size_t bytes = (size_t)n * (is_f64 ? 8 : 4);
  const double* noise_dev = nullptr;
  HostIo io(c, mem);
  if ((rc = io.open({{x, bytes, kScratchNdStageA}}, {{out, bytes, kScratchNdStageOut}}))) return rc;
  if ((rc = launch_wiener(c, io.in[0], is_f64 != 0, shape, rank, kernel_size, has_noise != 0, noise, io.out[0], &noise_dev))) return rc;
  if ((rc = io.close())) return rc;
  if (noise_used) {
    if (noise_dev) {
      NXSIG_HIP_TRY(hipMemcpyAsync(noise_used, noise_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
      *noise_used = noise;
    }
  }
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_argrelextrema(nxsig_ctx* ctx, const void* x, int32_t dtype, const int64_t* shape, int32_t rank, int32_t axis, int64_t shifts,
                        int32_t comparator, int32_t* indices, uint32_t* valid, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !indices || !valid) return set_error(NXSIG_ERR_INVALID_ARG, "argrelextrema: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  int64_t n = 0;
  if ((rc = peaks_shape("argrelextrema", shape, rank, &n))) return rc;
  if (axis < 0 || axis >= rank)
    return set_error(NXSIG_ERR_INVALID_ARG, "argrelextrema: axis " + std::to_string(axis) + " is out of range for rank " + std::to_string(rank));
  if (dtype < NXSIG_DT_F32 || dtype > NXSIG_DT_U64) return set_error(NXSIG_ERR_INVALID_ARG, "argrelextrema: unknown dtype");
  if (comparator < NXSIG_CMP_LESS || comparator > NXSIG_CMP_GREATER_EQUAL) return set_error(NXSIG_ERR_INVALID_ARG, "argrelextrema: unknown comparator");
  if (shifts < 0) shifts = 0;
  const size_t es = dtype == NXSIG_DT_F64 || dtype == NXSIG_DT_S64 || dtype == NXSIG_DT_U64 ? 8 : 4;
  HostIo io(c, mem);
  if ((rc = peaks_open(io, x, (size_t)n * es, n, rank, indices, valid))) return rc;
  if ((rc = launch_argrelextrema(c, io.in[0], dtype, shape, rank, axis, shifts, comparator, static_cast<int32_t*>(io.out[1]),
                                 static_cast<uint32_t*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_nonzero(nxsig_ctx* ctx, const uint8_t* mask, const int64_t* shape, int32_t rank, int32_t* indices, uint32_t* valid, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!mask || !indices || !valid) return set_error(NXSIG_ERR_INVALID_ARG, "nonzero: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  int64_t n = 0;
  if ((rc = peaks_shape("nonzero", shape, rank, &n))) return rc;
  HostIo io(c, mem);
  if ((rc = peaks_open(io, mask, (size_t)n, n, rank, indices, valid))) return rc;
  if ((rc = launch_nonzero(c, static_cast<const uint8_t*>(io.in[0]), shape, rank, static_cast<int32_t*>(io.out[1]),
                           static_cast<uint32_t*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_sawtooth(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double width, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!(width >= 0.0 && width <= 1.0))   // waveforms.ex:34-36
    return set_error(NXSIG_ERR_INVALID_ARG, "width must be between 0 and 1, inclusive. Got: " + wave_num(width));
  int rc = wave_args("sawtooth", t, out, n, mem);
  if (rc || n == 0) return rc;
  const WaveRound R{is_f64 != 0};
  WaveSaw p;
  // width is an Elixir number: width + 1 and 1 - width are double arithmetic and the number meets pi() unrounded
  p.two_pi = kWaveTwoPi;
  p.thr = R(kWaveTwoPi * width);
  p.d_rise = R(kWavePi * width);
  p.c_fall = R(kWavePi * (width + 1.0));
  p.d_fall = R(kWavePi * (1.0 - width));
  p.mode = width == 1.0 ? 1 : width == 0.0 ? 0 : 2;
  HostIo io(c, mem);
  const size_t es = is_f64 ? 8 : 4;
  if ((rc = wave_open(io, t, nullptr, es, n, out, es))) return rc;
  if ((rc = launch_sawtooth(c, io.in[0], is_f64 != 0, n, p, io.out[0]))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_square(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double duty, const void* duty_tensor, int32_t* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  int rc = wave_args("square", t, out, n, mem);
  if (rc || n == 0) return rc;
  const WaveRound R{is_f64 != 0};
  WaveSquare p;
  p.two_pi = kWaveTwoPi;
  p.pi = kWavePi;
  p.thr = R(R(R(duty) * 2.0) * kWavePi);   // duty * 2 * pi(), duty a tensor argument of square_n
  HostIo io(c, mem);
  if ((rc = wave_open(io, t, duty_tensor, is_f64 ? 8 : 4, n, out, 4))) return rc;
  if ((rc = launch_square(c, io.in[0], is_f64 != 0, n, p, io.in[1], static_cast<int32_t*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_gaussian_pulse(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double center_frequency, double bandwidth,
                         double bandwidth_reference_level, void* envelope, void* in_phase, void* quadrature, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const double fc = center_frequency, bw = bandwidth, bwr = bandwidth_reference_level;
  if (!(fc >= 0.0))   // waveforms.ex:173-186
    return set_error(NXSIG_ERR_INVALID_ARG, "Center frequency must be greater than or equal to 0, got: " + wave_num(fc));
  if (!(bw > 0.0)) return set_error(NXSIG_ERR_INVALID_ARG, "Bandwidth must be greater than 0, got: " + wave_num(bw));
  if (!(bwr < 0.0)) return set_error(NXSIG_ERR_INVALID_ARG, "Bandwidth reference level must be less than 0, got: " + wave_num(bwr));
  int rc = wave_args("gaussian_pulse", t, envelope, n, mem);
  if (rc || n == 0) return rc;
  if (!in_phase || !quadrature) return set_error(NXSIG_ERR_INVALID_ARG, "gaussian_pulse: null pointer argument");
  const WaveRound R{is_f64 != 0};
  // constants fold in double before they meet a tensor: ref = f32(10^(bwr / 20)), a = -f32((pi fc bw)^2) / (4 log(ref))
  const double ref = R(std::pow(10.0, bwr / 20.0));
  const double pfb = 3.141592653589793 * fc * bw;
  const double a = R(-R(pfb * pfb) / R(4.0 * R(std::log(ref))));
  WaveGauss p;
  p.neg_a = R(-a);
  p.w = R(kWaveTwoPi * R(fc));
  HostIo io(c, mem);
  const size_t bytes = (size_t)n * (is_f64 ? 8 : 4);
  if ((rc = io.open({{t, bytes, kScratchNdStageA}},
                    {{envelope, bytes, kScratchNdStageOut, wave_span(bytes)}, {in_phase, bytes, kScratchNdStageOut, wave_span(bytes)},
                     {quadrature, bytes, kScratchNdStageOut, wave_span(bytes)}}))) return rc;
  if ((rc = launch_gaussian_pulse(c, io.in[0], is_f64 != 0, n, p, io.out[0], io.out[1], io.out[2]))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_chirp(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double f0, double t1, double f1, int32_t method, int32_t vertex_zero,
                double phi, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (method < NXSIG_CHIRP_LINEAR || method > NXSIG_CHIRP_HYPERBOLIC)   // waveforms.ex:291-300
    return set_error(NXSIG_ERR_INVALID_ARG, "invalid method, must be one of [:linear, :quadratic, :logarithmic, :hyperbolic], got: " + std::to_string(method));
  int rc = wave_args("chirp", t, out, n, mem);
  if (rc || n == 0) return rc;
  const WaveRound R{is_f64 != 0};
  f0 = R(f0), t1 = R(t1), f1 = R(f1);   // tensor arguments of the defn
  WaveChirp p{};
  p.two_pi = kWaveTwoPi;
  p.phi = R(phi);
  const char* family = "waveform.chirp.linear";
  if (method == NXSIG_CHIRP_LINEAR) {
    p.kind = kChirpLinear;
    p.a = f0;
    p.b = R(0.5 * R(R(f1 - f0) / t1));
  } else if (method == NXSIG_CHIRP_QUADRATIC) {
    family = "waveform.chirp.quadratic";
    const double beta = R(R(f1 - f0) / R(t1 * t1));
    p.kind = vertex_zero ? kChirpQuadratic : kChirpQuadraticT1;
    p.a = vertex_zero ? f0 : f1;
    p.b = beta;
    p.c = t1;
    p.d = R(std::pow(t1, 3.0));
  } else if (method == NXSIG_CHIRP_LOGARITHMIC) {
    family = "waveform.chirp.logarithmic";
    if (f0 * f1 <= 0.0) {
      p.kind = kChirpNan;
    } else if (f0 == f1) {
      p.kind = kChirpConstant;
      p.a = R(kWaveTwoPi * f0);
    } else {
      const double ratio = R(f1 / f0), beta = R(t1 / R(std::log(ratio)));
      p.kind = kChirpLogarithmic;
      p.a = R(beta * f0);
      p.b = ratio;
      p.c = t1;
    }
  } else {
    family = "waveform.chirp.hyperbolic";
    if (f0 == f1) {
      p.kind = kChirpConstant;
      p.a = R(kWaveTwoPi * f0);
    } else {
      const double sp = R(R(R(-f1) * t1) / R(f0 - f1));
      p.kind = kChirpHyperbolic;
      p.a = R(R(-sp) * f0);
      p.b = sp;
    }
  }
  HostIo io(c, mem);
  const size_t es = is_f64 ? 8 : 4;
  if ((rc = wave_open(io, t, nullptr, es, n, out, es))) return rc;
  if ((rc = launch_chirp(c, io.in[0], is_f64 != 0, n, p, family, io.out[0]))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_polynomial_sweep(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, const double* coefs, int32_t ncoefs, double phi,
                           int32_t phi_degrees, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (ncoefs < 1 || ncoefs > NXSIG_SWEEP_MAX_COEFS)
    return set_error(NXSIG_ERR_INVALID_ARG, "polynomial_sweep: coefs must have 1 to " + std::to_string(NXSIG_SWEEP_MAX_COEFS) + " entries, got " +
                                                std::to_string(ncoefs));
  if (!coefs) return set_error(NXSIG_ERR_INVALID_ARG, "polynomial_sweep: null pointer argument");
  int rc = wave_args("polynomial_sweep", t, out, n, mem);
  if (rc || n == 0) return rc;
  const WaveRound R{is_f64 != 0};
  WaveSweep p{};
  p.n = ncoefs;
  p.two_pi = kWaveTwoPi;
  p.phi = phi_degrees ? R(phi * kWavePi / 180.0) : R(phi);   // phi * pi() / 180: constants, folded in double
  for (int k = 0; k < ncoefs; ++k) p.coef[k] = R(R(coefs[k]) / (double)(ncoefs - k));
  HostIo io(c, mem);
  const size_t es = is_f64 ? 8 : 4;
  if ((rc = wave_open(io, t, nullptr, es, n, out, es))) return rc;
  if ((rc = launch_polynomial_sweep(c, io.in[0], is_f64 != 0, n, p, io.out[0]))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_unit_impulse(nxsig_ctx* ctx, int32_t dtype, const int64_t* shape, int32_t rank, const int64_t* index, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  int rc = check_mem(mem);
  if (rc) return rc;
  if (dtype < NXSIG_DT_F32 || dtype > NXSIG_DT_U64) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: unknown dtype");
  if (rank < 0 || rank > 8) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: rank must be in [0, 8]");
  if (rank > 0 && (!shape || !index)) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: null pointer argument");
  int64_t n = 1;
  for (int d = 0; d < rank; ++d) {
    if (shape[d] < 0) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: negative dimension");
    if (shape[d] && n > (((int64_t)1 << 60) / shape[d])) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: shape too large");
    n *= shape[d];
  }
  if (n == 0) return NXSIG_OK;   // an empty dimension: an empty tensor, nothing to put
  if (!out) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: null pointer argument");
  int64_t at = 0;
  for (int d = 0; d < rank; ++d) {
    if (index[d] < 0 || index[d] >= shape[d])
      return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: index " + std::to_string(index[d]) + " is out of range for axis " + std::to_string(d) +
                                                  " of size " + std::to_string(shape[d]));
    at = at * shape[d] + index[d];
  }
  const size_t bytes = (size_t)n * (dtype == NXSIG_DT_F64 || dtype == NXSIG_DT_S64 || dtype == NXSIG_DT_U64 ? 8 : 4);
  HostIo io(c, mem);
  if ((rc = io.open({}, {{out, bytes, kScratchNdStageOut}}))) return rc;
  if ((rc = launch_unit_impulse(c, io.out[0], dtype, n, at))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_fftconvolve_c64(nxsig_ctx* ctx, const nxsig_c64* a, int64_t n1, const nxsig_c64* b, int64_t n2, int32_t mode,
                          nxsig_c64* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!a || !b || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fftconvolve: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (n1 < 1 || n2 < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fftconvolve: lengths must be >= 1");
  int64_t out_len, start;
  if ((rc = conv_slice(n1, n2, mode, &start, &out_len))) return rc;
  // (the launcher works in blocks of 8 192 points: the staged result is never shorter)
  HostIo io(c, mem);
  if ((rc = io.open({{a, (size_t)n1 * sizeof(float2), kScratchStageIn}, {b, (size_t)n2 * sizeof(float2), kScratchStageOut}},
                    {{out, (size_t)out_len * sizeof(float2), kScratchFusedSpectrum, (size_t)8192 * sizeof(float2)}}))) return rc;
  if ((rc = launch_fftconvolve_c64(c, static_cast<const float2*>(io.in[0]), n1, static_cast<const float2*>(io.in[1]), n2, start, out_len,
                                   static_cast<float2*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_mel_filters_f32(int32_t fft_length, int32_t mel_bins, double sampling_rate, double max_mel,
                          double mel_frequency_spacing, float* out) {
  NXSIG_API_BEGIN
  if (fft_length < 2 || mel_bins < 1 || !out || !(mel_frequency_spacing > 0.0))
    return set_error(NXSIG_ERR_INVALID_ARG, "mel_filters: fft_length >= 2, mel_bins >= 1 and a positive spacing are required");
  mel_filters_f32(fft_length, mel_bins, sampling_rate, max_mel, mel_frequency_spacing, out);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_stft_to_mel(nxsig_ctx* ctx, const nxsig_c64* z, int64_t rows, int32_t fft_length, int32_t mel_bins,
                      const float* filters, float* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!z || !filters || !out) return set_error(NXSIG_ERR_INVALID_ARG, "stft_to_mel: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rows < 1 || fft_length < 2 || mel_bins < 1) return set_error(NXSIG_ERR_INVALID_ARG, "stft_to_mel: rows, fft_length, mel_bins must be positive");
  if (fft_length / 2 > 8192) return set_error(NXSIG_ERR_UNSUPPORTED, "stft_to_mel: fft_length > 16384 is not supported");
  HostIo io(c, mem);
  if ((rc = io.open({{z, (size_t)rows * fft_length * sizeof(float2), kScratchStageIn}}, {{out, (size_t)rows * mel_bins * sizeof(float), kScratchStageOut}})))
    return rc;
  if ((rc = launch_stft_to_mel(c, static_cast<const float2*>(io.in[0]), rows, fft_length, mel_bins, filters, static_cast<float*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_spectrum_mul_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t rows, int32_t fft_length, const nxsig_c64* h,
                           nxsig_c64* out, int32_t mem) {
  NXSIG_API_BEGIN
  if (!z || !h || !out) return set_error(NXSIG_ERR_INVALID_ARG, "spectrum_mul: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rows < 0 || fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "spectrum_mul: rows >= 0 and fft_length >= 1 required");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (rows == 0) return NXSIG_OK;
  const void* hd = nullptr;
  if ((rc = ctx_table(c, 0x5BEC0ull ^ (uint64_t)fft_length, h, (size_t)fft_length * sizeof(float2), &hd))) return rc;
  const size_t bytes = (size_t)rows * fft_length * sizeof(float2);
  if (mem == NXSIG_DEVICE)
    return launch_spectrum_mul(c, reinterpret_cast<const float2*>(z), rows, fft_length, reinterpret_cast<const float2*>(hd),
                               reinterpret_cast<float2*>(out));
  HostIo io(c, mem);   // host tensors: the product is formed in place in the staged input
  if ((rc = io.open({{z, bytes, kScratchStageIn}}, {}))) return rc;
  float2* zw = static_cast<float2*>(const_cast<void*>(io.in[0]));
  if ((rc = launch_spectrum_mul(c, zw, rows, fft_length, reinterpret_cast<const float2*>(hd), zw))) return rc;
  return io.download(out, zw, bytes);
  NXSIG_API_END
}

int nxsig_stft_mel_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                       const float* window, const nxsig_stft_params* p, int32_t mel_bins, const float* filters, float* out,
                       int64_t* num_frames_out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  StftEntry e{"stft_mel", 65535, 2, ": fft_length >= 2 and mel_bins >= 1 required"};
  e.extra_null = !filters;
  e.fft_length_also = mel_bins < 1;
  Framing fr;
  int rc = stft_check(e, x, window, p, out, length, batch, batch_stride, mem, &fr, num_frames_out);
  if (rc) return rc;
  StftLaunch a;
  if ((rc = stft_plan(c, fr, batch, batch_stride, window, p, &a))) return rc;
  const int64_t rows = (int64_t)batch * fr.M;
  return stft_fused_sink(
      c, a, x, length, out, sizeof(float), (size_t)rows * mel_bins, mem,
      [&](const StftLaunch& s, void* od, bool* handled) { return launch_stft_mel_wave(c, s, mel_bins, filters, static_cast<float*>(od), handled); },
      [&](const StftLaunch& s, void* od) { return launch_stft_to_mel(c, s.z, rows, s.K, mel_bins, filters, static_cast<float*>(od)); });
  NXSIG_API_END
}

int nxsig_stft_onesided_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                            const nxsig_stft_params* p, nxsig_c64* out, int64_t* num_frames_out, int32_t mem) {
  return stft_onesided_impl(ctx, x, length, batch, batch_stride, window, p, out, num_frames_out, mem, false);
}
int nxsig_stft_packed_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                          const nxsig_stft_params* p, nxsig_c64* out, int64_t* num_frames_out, int32_t mem) {
  return stft_onesided_impl(ctx, x, length, batch, batch_stride, window, p, out, num_frames_out, mem, true);
}

int nxsig_stft_magnitude_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                             const float* window, const nxsig_stft_params* p, int32_t kind, float* out,
                             int64_t* num_frames_out, int32_t mem) {
  NXSIG_API_BEGIN
  StftEntry e{"stft_magnitude", 65535, 2, ": fft_length >= 2 required"};
  if (kind != NXSIG_MAG_ABS && kind != NXSIG_MAG_POWER && kind != NXSIG_MAG_DBFS)
    e.after_mem = "stft_magnitude: kind must be NXSIG_MAG_ABS, NXSIG_MAG_POWER or NXSIG_MAG_DBFS";
  Framing fr;
  int rc = stft_check(e, x, window, p, out, length, batch, batch_stride, mem, &fr, num_frames_out);
  if (rc) return rc;
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  StftLaunch a;
  if ((rc = stft_plan(c, fr, batch, batch_stride, window, p, &a))) return rc;
  const int64_t rows = (int64_t)batch * fr.M;
  return stft_fused_sink(
      c, a, x, length, out, sizeof(float), (size_t)rows * (p->fft_length / 2), mem,
      [&](const StftLaunch& s, void* od, bool* handled) { return launch_stft_mag_wave(c, s, kind, static_cast<float*>(od), handled); },
      [&](const StftLaunch& s, void* od) { return launch_mag_from_spectrum(c, s.z, rows, s.K, kind, static_cast<float*>(od)); });
  NXSIG_API_END
}


/* ---------------------------------------------------------------- f64 / c128 tier (kernels_f64.hip) */
int nxsig_window_f64(int32_t kind, int32_t n, int32_t is_periodic, double beta, double eps, double* out) {
  NXSIG_API_BEGIN
  return window_f64(kind, n, is_periodic != 0, beta, eps, out);
  NXSIG_API_END
}

int nxsig_sinc_f64(const double* t, int64_t n, double* out) {
  NXSIG_API_BEGIN
  if (n < 0 || (n > 0 && (!t || !out))) return set_error(NXSIG_ERR_INVALID_ARG, "sinc: bad arguments");
  sinc_f64(t, n, out);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_firwin_f64(int32_t num_taps, const double* cutoff, int32_t n_cutoff, int32_t window_kind, double kaiser_beta,
                     int32_t pass_zero, int32_t scale, double sampling_rate, double* out) {
  NXSIG_API_BEGIN
  return firwin_f64(num_taps, cutoff, n_cutoff, window_kind, kaiser_beta, pass_zero != 0, scale != 0, sampling_rate, out);
  NXSIG_API_END
}

int nxsig_fft_frequencies_f64(double sampling_rate, int32_t fft_length, int32_t endpoint, double* out) {
  NXSIG_API_BEGIN
  if (fft_length < 1 || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fft_frequencies: fft_length must be >= 1");
  fft_frequencies_f64(sampling_rate, fft_length, endpoint != 0, out);
  return NXSIG_OK;
  NXSIG_API_END
}

// the caller's window as f64 on the device; `wide` receives the exactly widened host copy of an f32 window
static int window_dev_f64(Ctx* c, const void* window, int32_t window_is_f64, int N, std::vector<double>& wide, const double** dev) {
  const double* wh = reinterpret_cast<const double*>(window);
  if (!window_is_f64) {
    wide.resize(N);
    for (int i = 0; i < N; ++i) wide[i] = (double)reinterpret_cast<const float*>(window)[i];
    wh = wide.data();
  }
  const void* d = nullptr;
  int rc = ctx_table(c, 0x57494E3634ull, wh, (size_t)N * sizeof(double), &d);
  if (rc) return rc;
  *dev = reinterpret_cast<const double*>(d);
  return NXSIG_OK;
}
// the scalar of :scaling in the window's own type (Nx.sum(window) / Nx.sqrt(fs * Nx.sum(window ** 2))), widened
static double scaling_of(const void* window, int32_t window_is_f64, int N, int scaling, double fs) {
  if (window_is_f64) return scaling_factor_f64(reinterpret_cast<const double*>(window), N, scaling, fs);
  return (double)scaling_factor(reinterpret_cast<const float*>(window), N, scaling, fs);
}

int nxsig_stft_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const void* window,
                   int32_t window_is_f64, const nxsig_stft_params* p, nxsig_c128* z, int64_t* num_frames_out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !window || !p || !z) return set_error(NXSIG_ERR_INVALID_ARG, "stft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || batch > 65535) return set_error(NXSIG_ERR_INVALID_ARG, "stft: batch must be in [1, 65535]");
  if (batch_stride < length) return set_error(NXSIG_ERR_INVALID_ARG, "stft: batch_stride < length");
  if (p->fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "stft: fft_length must be >= 1");
  if ((rc = check_scaling(p->scaling))) return rc;
  Framing fr;
  if ((rc = make_framing(length, p->frame_length, p->hop, p->pad_mode, p->pad_lo, p->pad_hi, &fr))) return rc;
  if (num_frames_out) *num_frames_out = fr.M;
  StftLaunchD a;
  a.fr = fr; a.batch = batch; a.batch_stride = batch_stride; a.K = p->fft_length;
  a.has_scale = p->scaling != NXSIG_SCALE_NONE;
  a.div = a.has_scale ? scaling_of(window, window_is_f64, p->frame_length, p->scaling, p->sampling_rate) : 1.0;
  std::vector<double> wide;
  if ((rc = window_dev_f64(c, window, window_is_f64, p->frame_length, wide, &a.window))) return rc;
  const size_t zbytes = (size_t)batch * fr.M * p->fft_length * sizeof(double2);
  const size_t xbytes = ((size_t)(batch - 1) * batch_stride + length) * sizeof(double);
  HostIo io(c, mem);
  if ((rc = io.open({{x, xbytes, kScratchStageIn}}, {{z, zbytes, kScratchStageOut}}))) return rc;
  a.x = static_cast<const double*>(io.in[0]); a.z = static_cast<double2*>(io.out[0]);
  if ((rc = launch_stft_f64(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_stft_c128(nxsig_ctx* ctx, const nxsig_c128* x, int64_t length, int32_t batch, int64_t batch_stride, const void* window,
                    int32_t window_is_f64, const nxsig_stft_params* p, nxsig_c128* z, int64_t* num_frames_out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!x || !window || !p || !z) return set_error(NXSIG_ERR_INVALID_ARG, "stft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || batch > 65535) return set_error(NXSIG_ERR_INVALID_ARG, "stft: batch must be in [1, 65535]");
  if (batch_stride < length) return set_error(NXSIG_ERR_INVALID_ARG, "stft: batch_stride < length");
  if (p->fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "stft: fft_length must be >= 1");
  if ((rc = check_scaling(p->scaling))) return rc;
  Framing fr;
  if ((rc = make_framing(length, p->frame_length, p->hop, p->pad_mode, p->pad_lo, p->pad_hi, &fr))) return rc;
  if (num_frames_out) *num_frames_out = fr.M;
  StftLaunchD a;
  a.fr = fr; a.batch = batch; a.batch_stride = batch_stride; a.K = p->fft_length; a.x_is_complex = 1;
  a.has_scale = p->scaling != NXSIG_SCALE_NONE;
  a.div = a.has_scale ? scaling_of(window, window_is_f64, p->frame_length, p->scaling, p->sampling_rate) : 1.0;
  std::vector<double> wide;
  if ((rc = window_dev_f64(c, window, window_is_f64, p->frame_length, wide, &a.window))) return rc;
  dispatch_note("stft.f64.c128");
  const size_t zbytes = (size_t)batch * fr.M * p->fft_length * sizeof(double2);
  const size_t xbytes = ((size_t)(batch - 1) * batch_stride + length) * sizeof(double2);
  HostIo io(c, mem);
  if ((rc = io.open({{x, xbytes, kScratchStageIn}}, {{z, zbytes, kScratchStageOut}}))) return rc;
  a.x = static_cast<const double*>(io.in[0]); a.z = static_cast<double2*>(io.out[0]);
  if ((rc = launch_stft_f64(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_istft_c128(nxsig_ctx* ctx, const nxsig_c128* z, int64_t num_frames, int32_t batch, const void* window, int32_t window_is_f64,
                     const nxsig_stft_params* p, nxsig_c128* y, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!z || !window || !p || !y) return set_error(NXSIG_ERR_INVALID_ARG, "istft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (batch < 1 || batch > 65535) return set_error(NXSIG_ERR_INVALID_ARG, "istft: batch must be in [1, 65535]");
  if (num_frames < 1) return set_error(NXSIG_ERR_INVALID_ARG, "istft: num_frames must be >= 1");
  if ((rc = check_scaling(p->scaling))) return rc;
  const int N = p->frame_length, hop = p->hop, K = p->fft_length;
  if (N < 1 || hop < 1) return set_error(NXSIG_ERR_INVALID_ARG, "istft: frame_length and hop must be >= 1");
  if (hop > N) return set_error(NXSIG_ERR_INVALID_ARG, "overlap_length must be a number less than the window size");
  if (K != N)
    return set_error(NXSIG_ERR_INVALID_ARG,
                     "istft: fft_length must equal the window length (the reference broadcasts {M,K} x {N}, lib/nx_signal.ex:628)");
  IstftLaunchD a;
  a.M = num_frames; a.batch = batch; a.N = N; a.hop = hop; a.K = K; a.window_f32 = window_is_f64 ? 0 : 1;
  a.has_scale = p->scaling != NXSIG_SCALE_NONE;
  a.scale_mul = a.has_scale ? scaling_of(window, window_is_f64, N, p->scaling, p->sampling_rate) : 1.0;
  std::vector<double> wide;
  if ((rc = window_dev_f64(c, window, window_is_f64, N, wide, &a.window))) return rc;
  const int64_t out_len = num_frames * hop + (N - hop);
  const size_t zbytes = (size_t)batch * num_frames * K * sizeof(double2), ybytes = (size_t)batch * out_len * sizeof(double2);
  HostIo io(c, mem);
  if ((rc = io.open({{z, zbytes, kScratchStageIn}}, {{y, ybytes, kScratchStageOut}}))) return rc;
  a.z = static_cast<const double2*>(io.in[0]); a.y = static_cast<double2*>(io.out[0]);
  if ((rc = launch_istft_f64(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_fft_c128(nxsig_ctx* ctx, const void* in, int32_t in_is_real, int64_t rows, int32_t n_in, int32_t fft_length, int32_t inverse,
                   nxsig_c128* out, int32_t mem) {
  NXSIG_API_BEGIN
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (!in || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fft: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (rows < 1 || n_in < 1 || fft_length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "fft: rows, n_in and fft_length must be >= 1");
  const size_t ibytes = (size_t)rows * n_in * (in_is_real ? sizeof(double) : sizeof(double2));
  const size_t obytes = (size_t)rows * fft_length * sizeof(double2);
  HostIo io(c, mem);
  if ((rc = io.open({{in, ibytes, kScratchStageIn}}, {{out, obytes, kScratchStageOut}}))) return rc;
  if ((rc = launch_fft_f64(c, io.in[0], in_is_real != 0, rows, n_in, fft_length, inverse != 0, static_cast<double2*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_as_windowed_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, int32_t window_length,
                          int32_t stride, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi, double* out, int64_t* num_frames_out,
                          int32_t mem) {
  return as_windowed<double>(ctx, x, length, batch, batch_stride, window_length, stride, pad_mode, pad_lo, pad_hi, out, num_frames_out, mem);
}

int nxsig_overlap_and_add_f64(nxsig_ctx* ctx, const double* frames, int64_t num_frames, int32_t batch, int32_t frame_length,
                              int32_t overlap_length, int32_t components, double* out, int32_t mem) {
  return overlap_and_add<double>(ctx, frames, num_frames, batch, frame_length, overlap_length, components, out, mem);
}

int nxsig_fir_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const double* h,
                  int32_t num_taps, int32_t mode, double* y, int32_t mem) {
  return fir_mode<double>(ctx, x, length, batch, batch_stride, h, num_taps, mode, y, mem);
}

int nxsig_fir_slice_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const double* h,
                        int32_t num_taps, int64_t out_start, int64_t out_len, double* y, int32_t mem) {
  return fir_common<double>(ctx, x, length, batch, batch_stride, h, num_taps, out_start, out_len, y, mem);
}

/* ---------------------------------------------------------------- Spectral.welch / csd */
int32_t nxsig_welch_bins(int32_t fft_length) {
  const int32_t nb = welch_bins(fft_length);
  return nb < 0 ? set_error(NXSIG_ERR_INVALID_ARG, "welch_bins: fft_length must be >= 1") : nb;
}

// welch (y == nullptr, pxx only) and csd: the argument checks need no context and come ahead of it
static int welch_common(const char* fn, nxsig_ctx* ctx, const float* x, const float* y, int64_t length, int32_t batch, int64_t batch_stride,
                        const float* window, int32_t frame_length, int32_t hop, int32_t fft_length, int32_t detrend, int32_t scaling,
                        double sampling_rate, float* pxx_out, float* pyy_out, nxsig_c64* pxy_out, int32_t mem) {
  NXSIG_API_BEGIN
  const bool csd = fn[0] == 'c';
  if (!x || !window || (csd ? !y || !pxy_out : !pxx_out)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (const char* what = welch_check_args(length, batch, batch_stride, frame_length, hop, fft_length, scaling, sampling_rate))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  const int64_t nb = welch_bins(fft_length);
  if (nb > INT64_MAX / batch / 8) return set_error(NXSIG_ERR_UNSUPPORTED, std::string(fn) + ": the result is too large");
  double sw = 0.0, sw2 = 0.0;
  for (int32_t i = 0; i < frame_length; ++i) { sw += (double)window[i]; sw2 += (double)window[i] * (double)window[i]; }
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  WelchLaunch a;
  a.L = length; a.batch_stride = batch_stride; a.batch = batch; a.N = frame_length; a.hop = hop; a.K = fft_length;
  a.window_host = window; a.detrend = detrend != 0;
  a.scale = scaling == NXSIG_WELCH_DENSITY ? 1.0 / (sampling_rate * sw2) : 1.0 / (sw * sw);
  const size_t in_bytes = rows_bytes(batch, batch_stride, length, sizeof(float));
  const size_t rb = (size_t)batch * nb * sizeof(float);
  HostIo io(c, mem);
  // two inputs, the results packed into one slot (pxy first); a result the caller does not want is not listed
  if (!csd) rc = io.open({{x, in_bytes, kScratchNdStageA}}, {{pxx_out, rb, kScratchNdStageOut}});
  else if (pxx_out && pyy_out)
    rc = io.open({{x, in_bytes, kScratchNdStageA}, {y, in_bytes, kScratchNdStageB}},
                 {{pxy_out, 2 * rb, kScratchNdStageOut}, {pxx_out, rb, kScratchNdStageOut}, {pyy_out, rb, kScratchNdStageOut}});
  else if (pxx_out || pyy_out)
    rc = io.open({{x, in_bytes, kScratchNdStageA}, {y, in_bytes, kScratchNdStageB}},
                 {{pxy_out, 2 * rb, kScratchNdStageOut}, {pxx_out ? pxx_out : pyy_out, rb, kScratchNdStageOut}});
  else rc = io.open({{x, in_bytes, kScratchNdStageA}, {y, in_bytes, kScratchNdStageB}}, {{pxy_out, 2 * rb, kScratchNdStageOut}});
  if (rc) return rc;
  a.x = static_cast<const float*>(io.in[0]);
  a.y = csd ? static_cast<const float*>(io.in[1]) : nullptr;
  a.pxx = a.pyy = nullptr; a.pxy = nullptr;
  if (!csd) a.pxx = static_cast<float*>(io.out[0]);
  else {
    a.pxy = static_cast<float2*>(io.out[0]);
    if (pxx_out) a.pxx = static_cast<float*>(io.out[1]);
    if (pyy_out) a.pyy = static_cast<float*>(io.out[pxx_out ? 2 : 1]);
  }
  if ((rc = launch_welch(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_welch_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                    int32_t frame_length, int32_t hop, int32_t fft_length, int32_t detrend, int32_t scaling, double sampling_rate,
                    float* pxx_out, int32_t mem) {
  return welch_common("welch", ctx, x, nullptr, length, batch, batch_stride, window, frame_length, hop, fft_length, detrend, scaling,
                      sampling_rate, pxx_out, nullptr, nullptr, mem);
}

int nxsig_csd_f32(nxsig_ctx* ctx, const float* x, const float* y, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                  int32_t frame_length, int32_t hop, int32_t fft_length, int32_t detrend, int32_t scaling, double sampling_rate,
                  float* pxx_out, float* pyy_out, nxsig_c64* pxy_out, int32_t mem) {
  return welch_common("csd", ctx, x, y, length, batch, batch_stride, window, frame_length, hop, fft_length, detrend, scaling, sampling_rate,
                      pxx_out, pyy_out, pxy_out, mem);
}

/* ---------------------------------------------------------------- Filters.sosfilt / sosfiltfilt */
int32_t nxsig_sosfilt_chunk(int32_t n_sections) {
  const int32_t v = iir_chunk(n_sections);
  return v ? v : set_error(NXSIG_ERR_INVALID_ARG, "sosfilt_chunk: n_sections must be in [1, 16]");
}

int32_t nxsig_sosfilt_tile(int32_t n_sections) {
  const int32_t v = iir_tile(n_sections);
  return v ? v : set_error(NXSIG_ERR_INVALID_ARG, "sosfilt_tile: n_sections must be in [1, 16]");
}

// what the two entry points check alike, ahead of the context: pointers, mem, the cascade, the rows
static int sos_check_common(const char* fn, const void* x, const void* y, const double* sos, int32_t n_sections, int32_t mem, int64_t length,
                            int32_t batch, int64_t batch_stride) {
  if (!x || !sos || !y) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (n_sections > kIirMaxSections)
    return set_error(NXSIG_ERR_UNSUPPORTED, std::string(fn) + ": more than 16 sections in one call (split the cascade)");
  if (const char* what = iir_check_sos(sos, n_sections)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  if (const char* what = iir_check_args(length, batch, batch_stride, 1, false, 0)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  if (length > INT64_MAX / batch / 16) return set_error(NXSIG_ERR_UNSUPPORTED, std::string(fn) + ": the rows are too large");
  return NXSIG_OK;
}

int nxsig_sosfilt_zi(const double* sos, int32_t n_sections, double* zi_out) {
  NXSIG_API_BEGIN
  if (!sos || !zi_out) return set_error(NXSIG_ERR_INVALID_ARG, "sosfilt_zi: null pointer argument");
  if (n_sections > (1 << 20)) return set_error(NXSIG_ERR_INVALID_ARG, "sosfilt_zi: too many sections");
  if (const char* what = iir_check_sos(sos, n_sections)) return set_error(NXSIG_ERR_INVALID_ARG, std::string("sosfilt_zi: ") + what);
  if (!iir_sosfilt_zi(sos, n_sections, zi_out))
    return set_error(NXSIG_ERR_INVALID_ARG, "sosfilt_zi: singular matrix (a section has a pole at z = 1)");
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_sosfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* sos,
                      int32_t n_sections, const double* zi, int32_t zi_rows, double* zf_out, int32_t direction, float* y, int32_t mem) {
  NXSIG_API_BEGIN
  int rc = sos_check_common("sosfilt", x, y, sos, n_sections, mem, length, batch, batch_stride);
  if (rc) return rc;
  if (const char* what = iir_check_args(length, batch, batch_stride, zi_rows, zi != nullptr, direction))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string("sosfilt: ") + what);
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(float)), kScratchNdStageA}},
                    {{y, (size_t)batch * length * sizeof(float), kScratchNdStageOut}}))) return rc;
  IirLaunch a;
  a.x = static_cast<const float*>(io.in[0]); a.n = length; a.x_stride = batch_stride; a.batch = batch;
  a.sos_host = sos; a.n_sections = n_sections; a.zi_host = zi; a.zi_rows = zi ? zi_rows : 1; a.zi_times_first = false;
  a.zf_host = zf_out; a.direction = direction;
  a.y = static_cast<float*>(io.out[0]); a.y_stride = length; a.out_off = 0; a.out_len = length;
  if ((rc = launch_sosfilt(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_sosfiltfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* sos,
                          int32_t n_sections, int32_t padtype, int64_t padlen, float* y, int32_t mem) {
  NXSIG_API_BEGIN
  int rc = sos_check_common("sosfiltfilt", x, y, sos, n_sections, mem, length, batch, batch_stride);
  if (rc) return rc;
  const int64_t edge = iir_edge(sos, n_sections, padtype, padlen, length);
  if (edge == -1) return set_error(NXSIG_ERR_INVALID_ARG, "sosfiltfilt: padtype must be NXSIG_SOS_PAD_NONE, _ODD, _EVEN or _CONSTANT");
  if (edge == -2)
    return set_error(NXSIG_ERR_INVALID_ARG, "sosfiltfilt: the length of the input vector x must be greater than padlen, which is " +
                                                std::to_string(padlen < 0 ? iir_default_padlen(sos, n_sections) : padlen));
  if (length + 2 * edge > INT64_MAX / batch / 16) return set_error(NXSIG_ERR_UNSUPPORTED, "sosfiltfilt: the rows are too large");
  double zi_probe[2 * kIirMaxSections];
  if (!iir_sosfilt_zi(sos, n_sections, zi_probe))
    return set_error(NXSIG_ERR_INVALID_ARG, "sosfiltfilt: singular matrix (a section has a pole at z = 1)");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(float)), kScratchNdStageA}},
                    {{y, (size_t)batch * length * sizeof(float), kScratchNdStageOut}}))) return rc;
  if ((rc = launch_sosfiltfilt(c, static_cast<const float*>(io.in[0]), length, batch_stride, batch, sos, n_sections, padtype, edge,
                               static_cast<float*>(io.out[0])))) return rc;
  return io.close();
  NXSIG_API_END
}

/* ---------------------------------------------------------------- Filters.lfilter / filtfilt */
int32_t nxsig_lfilter_chunk(int32_t order) {
  const int32_t v = lf_chunk(order);
  return v ? v : set_error(NXSIG_ERR_INVALID_ARG, "lfilter_chunk: order must be in [0, 16]");
}

int32_t nxsig_lfilter_tile(int32_t order) {
  const int32_t v = lf_tile(order);
  return v ? v : set_error(NXSIG_ERR_INVALID_ARG, "lfilter_tile: order must be in [0, 16]");
}

// what the two entry points check alike, ahead of the context: pointers, mem, the coefficients, the rows
static int lf_check_common(const char* fn, const void* x, const void* y, const double* b, int32_t nb, const double* a, int32_t na, int32_t mem,
                           int64_t length, int32_t batch, int64_t batch_stride) {
  if (!x || !b || !a || !y) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = lf_check_ba(b, nb, a, na, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  if (const char* what = lf_check_args(length, batch, batch_stride, 1, false, 0)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  if (length > INT64_MAX / batch / 16) return set_error(NXSIG_ERR_UNSUPPORTED, std::string(fn) + ": the rows are too large");
  return NXSIG_OK;
}

int nxsig_lfilter_zi(const double* b, int32_t nb, const double* a, int32_t na, double* zi_out) {
  NXSIG_API_BEGIN
  if (!b || !a || !zi_out) return set_error(NXSIG_ERR_INVALID_ARG, "lfilter_zi: null pointer argument");
  bool unsupported = false;
  if (const char* what = lf_check_ba(b, nb, a, na, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("lfilter_zi: ") + what);
  if (!lf_zi(lf_normalise(b, nb, a, na), zi_out)) return set_error(NXSIG_ERR_INVALID_ARG, "lfilter_zi: singular matrix (the filter has a pole at z = 1)");
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_lfilter_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* b, int32_t nb,
                      const double* a, int32_t na, const double* zi, int32_t zi_rows, double* zf_out, int32_t direction, float* y, int32_t mem) {
  NXSIG_API_BEGIN
  int rc = lf_check_common("lfilter", x, y, b, nb, a, na, mem, length, batch, batch_stride);
  if (rc) return rc;
  if (const char* what = lf_check_args(length, batch, batch_stride, zi_rows, zi != nullptr, direction))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string("lfilter: ") + what);
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(float)), kScratchNdStageA}},
                    {{y, (size_t)batch * length * sizeof(float), kScratchNdStageOut}}))) return rc;
  LfLaunch l;
  l.x = static_cast<const float*>(io.in[0]); l.n = length; l.x_stride = batch_stride; l.batch = batch;
  l.cf = lf_normalise(b, nb, a, na);
  const bool states = l.cf.n > 0;   // a gain has no state: zi and zf_out are empty arrays
  l.zi_host = states ? zi : nullptr; l.zi_rows = zi ? zi_rows : 1; l.zi_times_first = false;
  l.zf_host = states ? zf_out : nullptr; l.direction = direction;
  l.y = static_cast<float*>(io.out[0]); l.y_stride = length; l.out_off = 0; l.out_len = length;
  if ((rc = launch_lfilter(c, l))) return rc;
  return io.close();
  NXSIG_API_END
}

int nxsig_filtfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* b, int32_t nb,
                       const double* a, int32_t na, int32_t padtype, int64_t padlen, float* y, int32_t mem) {
  NXSIG_API_BEGIN
  int rc = lf_check_common("filtfilt", x, y, b, nb, a, na, mem, length, batch, batch_stride);
  if (rc) return rc;
  const int64_t edge = lf_edge(nb, na, padtype, padlen, length);
  if (edge == -1) return set_error(NXSIG_ERR_INVALID_ARG, "filtfilt: padtype must be NXSIG_SOS_PAD_NONE, _ODD, _EVEN or _CONSTANT");
  if (edge == -2)
    return set_error(NXSIG_ERR_INVALID_ARG, "filtfilt: the length of the input vector x must be greater than padlen, which is " +
                                                std::to_string(padlen < 0 ? lf_default_padlen(nb, na) : padlen));
  if (length + 2 * edge > INT64_MAX / batch / 16) return set_error(NXSIG_ERR_UNSUPPORTED, "filtfilt: the rows are too large");
  const LfCoefs cf = lf_normalise(b, nb, a, na);
  double zi_probe[kLfMaxOrder];
  if (!lf_zi(cf, zi_probe)) return set_error(NXSIG_ERR_INVALID_ARG, "filtfilt: singular matrix (the filter has a pole at z = 1)");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(float)), kScratchNdStageA}},
                    {{y, (size_t)batch * length * sizeof(float), kScratchNdStageOut}}))) return rc;
  if ((rc = launch_filtfilt(c, static_cast<const float*>(io.in[0]), length, batch_stride, batch, cf, padtype, edge, static_cast<float*>(io.out[0]))))
    return rc;
  return io.close();
  NXSIG_API_END
}

/* ---------------------------------------------------------------- PeakFinding.find_peaks */
int32_t nxsig_find_peaks_block(void) { return kFindPeaksBlock; }

int32_t nxsig_find_peaks_rounds(void) { return find_peaks_last_rounds(); }

int nxsig_find_peaks(nxsig_ctx* ctx, const void* x, int32_t dtype, const int64_t* shape, int32_t rank, int32_t axis, const double* bounds,
                     uint32_t conditions, double distance, int64_t wlen, double rel_height, int64_t capacity, uint32_t want,
                     int32_t* indices, uint32_t* valid, double* fprops, int32_t* iprops, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !valid) return set_error(NXSIG_ERR_INVALID_ARG, "find_peaks: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = peaks_shape("find_peaks", shape, rank, &total))) return rc;
  if (axis < 0 || axis >= rank)
    return set_error(NXSIG_ERR_INVALID_ARG, "find_peaks: axis " + std::to_string(axis) + " is out of range for rank " + std::to_string(rank));
  if (dtype != NXSIG_DT_F32 && dtype != NXSIG_DT_F64) return set_error(NXSIG_ERR_INVALID_ARG, "find_peaks: dtype must be NXSIG_DT_F32 or NXSIG_DT_F64");
  const int64_t n = shape[axis], most = find_peaks_capacity(total / n, n);
  char msg[96];
  if (const char* what = find_peaks_check(conditions, bounds, distance, wlen, rel_height, want, capacity, most, msg, sizeof msg))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string("find_peaks: ") + what);
  const int nf = find_peaks_f64_rows(want), ni = find_peaks_s32_rows(want);
  if (capacity > 0 && (!indices || (nf && !fprops) || (ni && !iprops))) return set_error(NXSIG_ERR_INVALID_ARG, "find_peaks: null pointer argument");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const size_t es = dtype == NXSIG_DT_F64 ? 8 : 4;
  FindPeaksLaunch a{};
  a.f64 = dtype == NXSIG_DT_F64; a.shape = shape; a.rank = rank; a.axis = axis; a.conditions = conditions; a.bounds = bounds;
  a.distance = distance; a.wlen = wlen; a.rel_height = rel_height; a.capacity = capacity; a.want = want;
  HostIo io(c, mem);
  // x in; out[0] = valid, out[1] = indices, out[2] = the f64 properties (a host call's s32 properties stay in the launcher's scratch)
  const size_t ib = (size_t)capacity * rank * 4, fb = (size_t)capacity * nf * 8;
  if (capacity == 0 || mem == NXSIG_DEVICE) rc = io.open({{x, (size_t)total * es, kScratchNdStageA}}, {{valid, 4, kScratchNdStageB}});
  else if (nf) rc = io.open({{x, (size_t)total * es, kScratchNdStageA}}, {{valid, 4, kScratchNdStageB}, {indices, ib, kScratchNdStageOut}, {fprops, fb, kScratchNdStageOut}});
  else rc = io.open({{x, (size_t)total * es, kScratchNdStageA}}, {{valid, 4, kScratchNdStageB}, {indices, ib, kScratchNdStageOut}});
  if (rc) return rc;
  const bool staged = mem == NXSIG_HOST && capacity > 0;
  int32_t* ip_dev = nullptr;
  a.x = io.in[0];
  a.valid = static_cast<uint32_t*>(io.out[0]);
  a.indices = staged ? static_cast<int32_t*>(io.out[1]) : indices;
  a.fprops = staged ? (nf ? static_cast<double*>(io.out[2]) : nullptr) : fprops;
  a.iprops = staged ? nullptr : iprops;
  a.iprops_used = &ip_dev;
  if ((rc = launch_find_peaks(c, a))) return rc;
  if ((rc = io.close())) return rc;
  if (staged && ni) return io.download(iprops, ip_dev, (size_t)capacity * ni * 4);
  return NXSIG_OK;
  NXSIG_API_END
}

/* ---------------------------------------------------------------- Filters.savgol_filter / savgol_coeffs */
int32_t nxsig_savgol_tile(void) { return kSavgolTile; }

static int savgol_check_common(const char* fn, int32_t window_length, int32_t polyorder, int32_t deriv, double delta) {
  bool unsupported = false;
  if (const char* what = savgol_check_design(window_length, polyorder, deriv, delta, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string(fn) + ": " + what);
  return NXSIG_OK;
}

int nxsig_savgol_coeffs(int32_t window_length, int32_t polyorder, int32_t deriv, double delta, double pos, int32_t use, double* out) {
  NXSIG_API_BEGIN
  if (!out) return set_error(NXSIG_ERR_INVALID_ARG, "savgol_coeffs: null pointer argument");
  int rc = savgol_check_common("savgol_coeffs", window_length, polyorder, deriv, delta);
  if (rc) return rc;
  if (pos != -1.0 && !(pos >= 0.0 && pos < (double)window_length))
    return set_error(NXSIG_ERR_INVALID_ARG, "savgol_coeffs: pos must be nonnegative and less than window_length.");
  if (use != kSgConv && use != kSgDot) return set_error(NXSIG_ERR_INVALID_ARG, "savgol_coeffs: `use` must be 'conv' or 'dot'.");
  savgol_coeffs(window_length, polyorder, deriv, delta, pos, use, out);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_savgol_filter(nxsig_ctx* ctx, const void* x, int32_t is_f64, int64_t length, int32_t batch, int64_t batch_stride, int32_t window_length,
                        int32_t polyorder, int32_t deriv, double delta, int32_t mode, double cval, void* y, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !y) return set_error(NXSIG_ERR_INVALID_ARG, "savgol_filter: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  if (is_f64 != 0 && is_f64 != 1) return set_error(NXSIG_ERR_INVALID_ARG, "savgol_filter: is_f64 must be 0 or 1");
  if ((rc = savgol_check_common("savgol_filter", window_length, polyorder, deriv, delta))) return rc;
  if (const char* what = savgol_check_rows(window_length, mode, cval, length, batch, batch_stride))
    return set_error(NXSIG_ERR_INVALID_ARG, std::string("savgol_filter: ") + what);
  if (batch_stride > INT64_MAX / batch / 16) return set_error(NXSIG_ERR_UNSUPPORTED, "savgol_filter: the rows are too large");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const size_t es = is_f64 ? sizeof(double) : sizeof(float);
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, es), kScratchNdStageA}},
                    {{y, (size_t)batch * length * es, kScratchNdStageOut}}))) return rc;
  SavgolLaunch a;
  a.x = io.in[0]; a.f64 = is_f64 != 0; a.n = length; a.x_stride = batch_stride; a.batch = batch;
  a.W = window_length; a.p = polyorder; a.deriv = deriv; a.delta = delta; a.mode = mode; a.cval = cval;
  a.y = io.out[0];
  if ((rc = launch_savgol(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

/* ---------------------------------------------------------------- Filters.hilbert */
int nxsig_hilbert_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, int64_t n_fft, int32_t kind,
                      void* out, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !out) return set_error(NXSIG_ERR_INVALID_ARG, "hilbert: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = hilbert_check(length, batch, batch_stride, n_fft, kind, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("hilbert: ") + what);
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (batch == 0) return NXSIG_OK;
  HostIo io(c, mem);
  if ((rc = io.open({{x, rows_bytes(batch, batch_stride, length, sizeof(float)), kScratchNdStageA}},
                    {{out, (size_t)batch * n_fft * hilbert_out_elem(kind), kScratchNdStageOut}}))) return rc;
  HilbertLaunch a;
  a.x = static_cast<const float*>(io.in[0]); a.length = length; a.x_stride = batch_stride; a.batch = batch; a.n_fft = n_fft; a.kind = kind;
  a.out = io.out[0];
  if ((rc = launch_hilbert(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

/* ---------------------------------------------------------------- Transforms.dct / idct */
int nxsig_dct_f32(nxsig_ctx* ctx, const float* x, int64_t length, int64_t batch, int64_t batch_stride, int64_t n, int32_t type, int32_t norm,
                  int64_t keep, float* out, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !out) return set_error(NXSIG_ERR_INVALID_ARG, "dct: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = dct_check(length, batch, batch_stride, n, type, norm, keep, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("dct: ") + what);
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (batch == 0) return NXSIG_OK;
  HostIo io(c, mem);
  if ((rc = io.open({{x, ((size_t)(batch - 1) * batch_stride + length) * sizeof(float), kScratchNdStageA}},
                    {{out, (size_t)batch * keep * sizeof(float), kScratchNdStageOut}}))) return rc;
  DctLaunch a;
  a.x = static_cast<const float*>(io.in[0]); a.length = length; a.x_stride = batch_stride; a.batch = batch; a.n = n; a.type = type; a.norm = norm;
  a.keep = keep; a.out = static_cast<float*>(io.out[0]);
  if ((rc = launch_dct(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

}  // extern "C"

namespace nxsig {
bool table_requests_query(const Ctx* c, const char* name, int32_t* value, int32_t* is_set) {
  if (!name || (std::strcmp(name, "TABLE_REQUESTS") != 0 && std::strcmp(name, "NXSIG_TABLE_REQUESTS") != 0)) return false;
  if (value) *value = (int32_t)(c->table_requests & 0x7fffffff);
  if (is_set) *is_set = 0;
  return true;
}
}  // namespace nxsig

/* ---------------------------------------------------------------- Spectral.lombscargle */
extern "C" {

int32_t nxsig_lombscargle_block(int32_t which) {
  const int32_t v = ls_block(which);
  return v ? v : set_error(NXSIG_ERR_INVALID_ARG, "lombscargle_block: which must be 0 (frequencies), 1 (rows) or 2 (samples per tile)");
}

int nxsig_lombscargle(nxsig_ctx* ctx, const void* y, int32_t dtype, int64_t n, int32_t batch, int64_t batch_stride, const double* x,
                      const double* freqs, int64_t num_freqs, const double* weights, int32_t precenter, int32_t normalize, int32_t floating_mean,
                      void* out, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!y || !x || !freqs || !out) return set_error(NXSIG_ERR_INVALID_ARG, "lombscargle: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = ls_check_shape(dtype, n, batch, batch_stride, num_freqs, precenter, normalize, floating_mean, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("lombscargle: ") + what);
  if (const char* what = ls_check_arrays(x, n, freqs, num_freqs, weights)) return set_error(NXSIG_ERR_INVALID_ARG, std::string("lombscargle: ") + what);
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  const size_t es = dtype == NXSIG_DT_F64 ? sizeof(double) : sizeof(float);
  HostIo io(c, mem);
  if ((rc = io.open({{y, rows_bytes(batch, batch_stride, n, es), kScratchNdStageA}},
                    {{out, (size_t)batch * num_freqs * ls_out_elem(dtype, normalize), kScratchNdStageOut}}))) return rc;
  LsLaunch a;
  a.y = io.in[0]; a.f64 = dtype == NXSIG_DT_F64; a.n = n; a.y_stride = batch_stride; a.batch = batch;
  a.x_host = x; a.freqs_host = freqs; a.num_freqs = num_freqs; a.weights_host = weights;
  a.precenter = precenter; a.normalize = normalize; a.floating_mean = floating_mean;
  a.out = io.out[0];
  if ((rc = launch_lombscargle(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

}  // extern "C"

/* ---------------------------------------------------------------- Transforms.czt / zoom_fft */
extern "C" {

int64_t nxsig_czt_conv_length(int64_t n, int64_t m) {
  if (n < 1 || m < 1) return set_error(NXSIG_ERR_INVALID_ARG, "czt_conv_length: n and m must be >= 1");
  if (n > ((int64_t)1 << 30) || m > ((int64_t)1 << 30) || czt_need(n, m) > ((int64_t)1 << 30))
    return set_error(NXSIG_ERR_UNSUPPORTED, "czt_conv_length: n + m - 1 must be at most 2^30");
  return czt_conv_length(n, m, false);
}

int nxsig_czt_tables(int64_t n, int64_t m, int64_t L, double w_abs, double w_step, int64_t w_den, double a_abs, double a_turns,
                     double* A, double* F, double* W, double* spread) {
  NXSIG_API_BEGIN
  if (!A || !F || !W) return set_error(NXSIG_ERR_INVALID_ARG, "czt_tables: null pointer argument");
  const CztContour k{w_abs, w_step, w_den, a_abs, a_turns};
  bool unsupported = false;
  if (const char* what = czt_check(0, n, 1, n, m, k, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("czt_tables: ") + what);
  if (!czt_is_pow2(L) || L < czt_need(n, m) || L > ((int64_t)1 << 30))
    return set_error(NXSIG_ERR_INVALID_ARG, "czt_tables: L must be a power of two >= n + m - 1");
  if (const char* what = czt_tables(n, m, L, k, A, F, W, spread)) return set_error(NXSIG_ERR_UNSUPPORTED, std::string("czt: ") + what);
  return NXSIG_OK;
  NXSIG_API_END
}

int nxsig_czt(nxsig_ctx* ctx, const void* x, int32_t is_complex, int64_t length, int64_t batch, int64_t batch_stride, int64_t m,
              double w_abs, double w_step, int64_t w_den, double a_abs, double a_turns, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !out) return set_error(NXSIG_ERR_INVALID_ARG, "czt: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  const CztContour k{w_abs, w_step, w_den, a_abs, a_turns};
  bool unsupported = false;
  if (const char* what = czt_check(is_complex, length, batch, batch_stride, m, k, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("czt: ") + what);
  if (!(czt_spread(length, m, k) <= kCztSpreadGate)) return set_error(NXSIG_ERR_UNSUPPORTED, "czt: the contour leaves single precision");
  const size_t es = is_complex ? sizeof(float2) : sizeof(float);
  const size_t x_bytes = batch ? ((size_t)(batch - 1) * batch_stride + length) * es : 0, out_bytes = (size_t)batch * m * sizeof(float2);
  if (czt_overlap(x, x_bytes, out, out_bytes)) return set_error(NXSIG_ERR_INVALID_ARG, "czt: x and out must not overlap");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (batch == 0) return NXSIG_OK;
  HostIo io(c, mem);
  if ((rc = io.open({{x, x_bytes, kScratchNdStageA}}, {{out, out_bytes, kScratchNdStageOut}}))) return rc;
  CztLaunch a;
  a.x = io.in[0]; a.is_complex = is_complex != 0; a.length = length; a.x_stride = batch_stride; a.batch = batch; a.m = m; a.contour = k;
  a.out = io.out[0];
  if ((rc = launch_czt(c, a))) return rc;
  return io.close();
  NXSIG_API_END
}

}  // extern "C"

/* ---------------------------------------------------------------- Filters.fir_bank / Transforms.cwt */
extern "C" {

int64_t nxsig_cwt_support(double width, int64_t length) {
  if (!std::isfinite(width) || !(width > 0.0)) return set_error(NXSIG_ERR_INVALID_ARG, "cwt_support: width must be positive and finite");
  if (length < 1) return set_error(NXSIG_ERR_INVALID_ARG, "cwt_support: length must be >= 1");
  return cwt_support(width, length);
}

int nxsig_cwt_wavelet(int32_t wavelet, double width, double w, int64_t N, double* out_f64) {
  NXSIG_API_BEGIN
  if (!out_f64) return set_error(NXSIG_ERR_INVALID_ARG, "cwt_wavelet: null pointer argument");
  if (const char* what = cwt_widths_check(wavelet, &width, 1, w)) return set_error(NXSIG_ERR_INVALID_ARG, std::string("cwt_wavelet: ") + what);
  if (N < 1) return set_error(NXSIG_ERR_INVALID_ARG, "cwt_wavelet: N must be >= 1");
  if (N > kCwtMaxExtent) return set_error(NXSIG_ERR_UNSUPPORTED, "cwt_wavelet: N must be at most 2^24");
  cwt_wavelet(wavelet, width, w, N, out_f64);
  return NXSIG_OK;
  NXSIG_API_END
}

}  // extern "C"

// the part the two entry points share, once the bank is a list of interleaved complex doubles and every argument but the context is checked
static int cwt_run(const char* name, nxsig_ctx* ctx, const void* x, int64_t length, int64_t batch, int64_t batch_stride,
                   const std::vector<double>& taps, const int64_t* tap_counts, int64_t num_filters, int32_t kind, void* out, int32_t mem) {
  const size_t x_bytes = ((size_t)(batch - 1) * batch_stride + length) * sizeof(float);
  const size_t out_bytes = (size_t)batch * num_filters * length * (kind == kCwComplex ? sizeof(float2) : sizeof(float));
  if (czt_overlap(x, x_bytes, out, out_bytes)) return set_error(NXSIG_ERR_INVALID_ARG, std::string(name) + ": x and out must not overlap");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  HostIo io(c, mem);
  int rc;
  if ((rc = io.open({{x, x_bytes, kScratchNdStageA}}, {{out, out_bytes, kScratchNdStageOut}}))) return rc;
  CwtLaunch a;
  a.x = static_cast<const float*>(io.in[0]); a.length = length; a.x_stride = batch_stride; a.batch = batch;
  a.taps_host = taps.data(); a.tap_counts = tap_counts; a.num_filters = num_filters; a.kind = kind; a.out = io.out[0];
  if ((rc = launch_cwt(c, a))) return rc;
  return io.close();
}

extern "C" {

int nxsig_fir_bank(nxsig_ctx* ctx, const void* x, int64_t length, int64_t batch, int64_t batch_stride, const void* taps, int32_t taps_complex,
                   const int64_t* tap_counts, int64_t num_filters, int32_t kind, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!x || !taps || !tap_counts || !out) return set_error(NXSIG_ERR_INVALID_ARG, "fir_bank: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = cwt_rows_check(length, batch, batch_stride, kind, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("fir_bank: ") + what);
  int64_t total = 0, longest = 0;
  if (const char* what = cwt_bank_check(length, taps_complex, tap_counts, num_filters, &total, &longest, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("fir_bank: ") + what);
  std::vector<double> h((size_t)2 * total, 0.0);
  const float* tf = static_cast<const float*>(taps);
  for (int64_t i = 0; i < total; ++i) {
    h[2 * i] = taps_complex ? tf[2 * i] : tf[i];
    if (taps_complex) h[2 * i + 1] = tf[2 * i + 1];
  }
  if (!cwt_all_finite(h.data(), 2 * total)) return set_error(NXSIG_ERR_INVALID_ARG, "fir_bank: the taps must be finite");
  return cwt_run("fir_bank", ctx, x, length, batch, batch_stride, h, tap_counts, num_filters, kind, out, mem);
  NXSIG_API_END
}

int nxsig_cwt(nxsig_ctx* ctx, const void* x, int64_t length, int64_t batch, int64_t batch_stride, int32_t wavelet, const double* widths,
              int64_t num_widths, double w, int32_t kind, void* out, int32_t mem) {
  NXSIG_API_BEGIN
  if (!x || !widths || !out) return set_error(NXSIG_ERR_INVALID_ARG, "cwt: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = cwt_rows_check(length, batch, batch_stride, kind, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("cwt: ") + what);
  if (const char* what = cwt_widths_check(wavelet, widths, num_widths, w)) return set_error(NXSIG_ERR_INVALID_ARG, std::string("cwt: ") + what);
  std::vector<int64_t> counts((size_t)num_widths);
  for (int64_t s = 0; s < num_widths; ++s) counts[s] = cwt_support(widths[s], length);
  int64_t total = 0, longest = 0;
  if (const char* what = cwt_bank_check(length, 1, counts.data(), num_widths, &total, &longest, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("cwt: ") + what);
  // the wavelets in double, rounded to f32 once: the bank nxsig_fir_bank would be handed
  std::vector<double> h((size_t)2 * total);
  int64_t at = 0;
  for (int64_t s = 0; s < num_widths; ++s) { cwt_wavelet(wavelet, widths[s], w, counts[s], h.data() + 2 * at); at += counts[s]; }
  for (double& v : h) v = (double)(float)v;
  if (!cwt_all_finite(h.data(), 2 * total)) return set_error(NXSIG_ERR_INVALID_ARG, "cwt: the taps must be finite");
  return cwt_run("cwt", ctx, x, length, batch, batch_stride, h, counts.data(), num_widths, kind, out, mem);
  NXSIG_API_END
}

}  // extern "C"

/* ---------------------------------------------------------------- Convolution.correlate_rows / convolve_rows */
extern "C" {

int64_t nxsig_xcorr_fft_length(int64_t n1, int64_t n2) {
  if (n1 < 1 || n2 < 1) return set_error(NXSIG_ERR_INVALID_ARG, "xcorr_fft_length: lengths must be >= 1");
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30) || xcorr_need(n1, n2) > ((int64_t)1 << 30))
    return set_error(NXSIG_ERR_UNSUPPORTED, "xcorr_fft_length: n1 + n2 - 1 must be at most 2^30");
  return xcorr_fft_length(n1, n2);
}

int nxsig_xcorr(nxsig_ctx* ctx, const void* a, int64_t n1, int64_t a_stride, const void* b, int64_t n2, int64_t b_stride, int64_t batch,
                int32_t is_complex, int32_t op, int32_t mode, int32_t weighting, double phat_floor, int32_t sink, void* out,
                int32_t* out_lags, int32_t mem) {
  NXSIG_API_BEGIN
  // the argument checks need no context and come ahead of it
  if (!a || !b || !out || (sink == kXcPeak && !out_lags)) return set_error(NXSIG_ERR_INVALID_ARG, "xcorr: null pointer argument");
  int rc = check_mem(mem);
  if (rc) return rc;
  bool unsupported = false;
  if (const char* what = xcorr_check(n1, a_stride, n2, b_stride, batch, is_complex, op, mode, weighting, phat_floor, sink, &unsupported))
    return set_error(unsupported ? NXSIG_ERR_UNSUPPORTED : NXSIG_ERR_INVALID_ARG, std::string("xcorr: ") + what);
  const size_t es = is_complex ? sizeof(float2) : sizeof(float);
  const bool peak = sink == kXcPeak;
  const size_t a_bytes = batch ? ((size_t)(batch - 1) * a_stride + n1) * es : 0, b_bytes = batch ? ((size_t)(batch - 1) * b_stride + n2) * es : 0;
  const size_t out_bytes = (size_t)batch * (peak ? 1 : xcorr_out_length(n1, n2, mode)) * es, lag_bytes = peak ? (size_t)batch * sizeof(int32_t) : 0;
  if (czt_overlap(a, a_bytes, out, out_bytes) || czt_overlap(b, b_bytes, out, out_bytes) || czt_overlap(a, a_bytes, out_lags, lag_bytes) ||
      czt_overlap(b, b_bytes, out_lags, lag_bytes) || czt_overlap(out, out_bytes, out_lags, lag_bytes))
    return set_error(NXSIG_ERR_INVALID_ARG, "xcorr: the result must not overlap an operand");
  NXSIG_CHECK_CTX(ctx)
  DispatchScope dispatch_scope(c);
  if (batch == 0) return NXSIG_OK;
  HostIo io(c, mem);
  if (peak) rc = io.open({{a, a_bytes, kScratchNdStageA}, {b, b_bytes, kScratchNdStageB}}, {{out, out_bytes, kScratchNdStageOut}, {out_lags, lag_bytes, kScratchNdStageOut}});
  else rc = io.open({{a, a_bytes, kScratchNdStageA}, {b, b_bytes, kScratchNdStageB}}, {{out, out_bytes, kScratchNdStageOut}});
  if (rc) return rc;
  XcorrLaunch l;
  l.a = io.in[0]; l.b = io.in[1]; l.is_complex = is_complex != 0; l.n1 = n1; l.a_stride = a_stride; l.n2 = n2; l.b_stride = b_stride; l.batch = batch;
  l.op = op; l.mode = mode; l.weighting = weighting; l.sink = sink; l.phat_floor = (float)phat_floor;
  l.out = io.out[0]; l.out_lags = peak ? static_cast<int32_t*>(io.out[1]) : nullptr;
  if ((rc = launch_xcorr(c, l))) return rc;
  return io.close();
  NXSIG_API_END
}

}  // extern "C"
