// Internal declarations shared by the C-ABI layer (api.cpp), the host-side generators
// (host_numerics.cpp) and the HIP launchers (*.hip).  Nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/nxsig.h"

namespace nxsig {

// ---- error plumbing: thread-local message, never throws across the C ABI ----
int set_error(int code, const std::string& msg);
const char* last_error_cstr();

// ---- dispatch record (nxsig_last_dispatch): the kernel FAMILIES the calling thread's last compute call launched, "a+b+c" in launch
// order (each family once).  Every launcher that commits to a kernel family notes it; the compute entry points of the C ABI reset
// the record.  Thread-local like the error message: dirty schedulers calling concurrently see their own call's record.
void dispatch_reset();
void dispatch_note(const char* family);
const char* dispatch_cstr();
struct Ctx;
// group.cpp, where a member's part of a sharded call starts: empties the calling thread's record AND the member context's copy.  The
// compute entry point the group then calls on the member fills both again; a member whose part is empty keeps the empty record
// instead of whatever ran on its context before (include/nxsig.h, nxsig_ctx_last_dispatch).
void dispatch_member_begin(Ctx* c);

#define NXSIG_HIP_TRY(expr)                                                                          \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return ::nxsig::set_error(_e == hipErrorOutOfMemory ? NXSIG_ERR_OOM : NXSIG_ERR_HIP,           \
                                std::string(#expr) + ": " + hipGetErrorString(_e));                  \
  } while (0)

// ---- every extern "C" entry point runs between these two: no C++ exception leaves the library
#define NXSIG_API_BEGIN try {
#define NXSIG_API_END                                                                   \
  }                                                                                     \
  catch (const std::bad_alloc&) { return ::nxsig::set_error(NXSIG_ERR_OOM, "host out of memory"); } \
  catch (const std::exception& e) { return ::nxsig::set_error(NXSIG_ERR_INVALID_ARG, std::string("internal error: ") + e.what()); } \
  catch (...) { return ::nxsig::set_error(NXSIG_ERR_INVALID_ARG, "internal error"); }

// ---- Nx.fft / Nx.ifft clean-up (SURVEY App. A rule 7; call sites lib/nx_signal.ex:102, :609, convolution.ex:282): the
// BinaryBackend zeroes every component of a transform's result whose magnitude is <= eps (1e-10, the default of the :eps
// option) before rounding to c64.  Every forward / inverse kernel applies it to the finished transform, ahead of any scaling
// or window product the reference applies afterwards.  NaN compares false and passes through.
constexpr float kFftEps = 1.0e-10f;
__host__ __device__ __forceinline__ float fft_eps0(float x) { return __builtin_fabsf(x) <= kFftEps ? 0.0f : x; }
__host__ __device__ __forceinline__ float2 fft_eps0(float2 v) { return make_float2(fft_eps0(v.x), fft_eps0(v.y)); }

// ---- host numerics (host_numerics.cpp) ----
int window_f32(int kind, int n, bool periodic, double beta, double eps, float* out);
void sinc_f32(const float* t, int64_t n, float* out);
int firwin_f32(int num_taps, const double* cutoff, int n_cutoff, int window_kind, double beta, bool pass_zero,
               bool scale, double sampling_rate, float* out);
void fft_frequencies_f32(double fs, int K, bool endpoint, float* out);
void stft_times_f32(int N, double fs, int64_t M, float* out);
float scaling_factor(const float* w, int N, int scaling, double fs);
void mel_filters_f32(int K, int mel_bins, double fs, double max_mel, double f_sp, float* out);
// the same generators evaluated in f64 (`type: {:f, 64}` of the reference: every op rounds to double)
int window_f64(int kind, int n, bool periodic, double beta, double eps, double* out);
void sinc_f64(const double* t, int64_t n, double* out);
int firwin_f64(int num_taps, const double* cutoff, int n_cutoff, int window_kind, double beta, bool pass_zero,
               bool scale, double sampling_rate, double* out);
void fft_frequencies_f64(double fs, int K, bool endpoint, double* out);
double scaling_factor_f64(const double* w, int N, int scaling, double fs);

// ---- framing geometry (as_windowed, lib/nx_signal.ex:257-331) ----
struct Framing {
  int64_t L;       // signal length
  int32_t N;       // frame (window) length
  int32_t hop;     // stride
  int32_t reflect; // 1 = mirror padding, 0 = zero padding
  int64_t lo, hi;  // padding (may be negative for explicit crop)
  int64_t M;       // number of frames
};
int make_framing(int64_t L, int32_t N, int32_t hop, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi, Framing* out);

// ---- dispatch / geometry switches ----
// Read from the environment ONCE per context, in nxsig_ctx_create (tuning_from_env: the library's one getenv loop); afterwards a
// launch only reads the context's Tuning struct.  nxsig_ctx_set_tuning changes a switch of one context at run time (the A/B sweep
// tools, tests); nothing in a launch path looks at the process environment.  Names are the NXSIG_<NAME> variables of
// INTEGRATION.md.  The knobs of concluded experiments are gone (round 4): their winning value is a constant at the use site.
#define NXSIG_TUNABLES(X)                                                                                                      \
  X(DISABLE_WAVE) X(DISABLE_WAVE_ROWS) X(DISABLE_BLUE_WAVE) X(DISABLE_R20) X(DISABLE_RAB) X(DISABLE_8K) X(DISABLE_4K) X(DISABLE_FUSED_FILTER) X(DISABLE_FUSED_MASK) \
  X(ISTFT_DEEP) X(ISTFT_HALF_DEEP) X(ISTFT_RUNS_PER_CU) X(ISTFT_MIN_RUN) X(ISTFT_REGOLA)                                                    \
  X(STORE_POLICY) X(WAVE_NO_SPLIT) X(NO_AL8) X(NO_STAGE) X(WAVE_UNITS_PER_WAVE) X(STAGE_PAD) X(NO_HOP4) X(WAVE_SMALL_W) X(WAVE_SMALL_CHUNK) \
  X(FIR32) X(FIR_PAD_TAPS) X(FIR_PHASE) X(FIR_HREG) X(FIR_UNITS_PER_WAVE) X(FIR_R2K) X(FIR_DLINE)                                                    \
  X(MEL_TILE) X(MEL_LDS_KB) X(FFT_TILED) X(FFT_TILE_ELEMS) X(FFT_TILE_NT) X(FFT_COLUMNS) X(FFT_TILED_MIN) X(CONV_POW2)          \
  X(DIRECT_FAST) X(POOL_MAX_MB) X(NO_PREFAULT) X(HOST_PIPE) X(DISABLE_FILTER_TILES) X(DISABLE_PEAK_TILES) X(DISABLE_RESAMPLE_LDS) \
  X(TABLE_CACHE_MAX) X(DISABLE_WELCH_WAVE) X(DISABLE_SOSFILT_SCAN) X(DISABLE_FIND_PEAKS_TABLES) X(DISABLE_SAVGOL_TILES) X(DISABLE_HILBERT_WAVE) X(DISABLE_DCT_DIRECT) X(DISABLE_LFILTER_SCAN) X(CZT_WAVE) X(CWT_WAVE) X(XCORR_WAVE) X(XCORR_SLAB_ROWS) X(LOMBSCARGLE_TILE)
enum TuneKey : int {
#define NXSIG_X(n) kT_##n,
  NXSIG_TUNABLES(NXSIG_X)
#undef NXSIG_X
  kTuneCount
};
struct Tuning {
  int32_t v[kTuneCount] = {};
  bool set[kTuneCount] = {};
};
void tuning_from_env(Tuning* t);       // api.cpp
bool tuning_value_ok(int key, long value, long* lo, long* hi);   // the admissible range of a switch (api.cpp)
int tuning_index(const char* name);    // "NXSIG_FOO" or "FOO" -> TuneKey, -1 when there is no such switch
const char* tuning_name(int key);      // "NXSIG_FOO"

// ---- scratch slots of a context (Ctx::scratch): every user of ctx_scratch owns the slot it names here.  Two users of one slot that are
// live in the same call overwrite each other silently, so a new temporary takes a new enumerator, never a number.
enum ScratchSlot : int {
  kScratchMultiStage = 0,        // generic istft's frames tensor; the three transforms of nxsig_fftconvolve_c64 (kernels_generic.hip)
  kScratchStageIn = 1,           // host staging: the first input of a NXSIG_HOST call (HostIo, api.cpp)
  kScratchStageOut = 2,          // host staging: the result of a NXSIG_HOST call; nxsig_fftconvolve_c64's second input (HostIo, api.cpp)
  kScratchWaveSink = 3,          // dummy sink the wave kernels' unused output pointers aim at (kernels_wave*.hip, wave_stft.hpp, wave_rab.hpp)
  kScratchFusedSpectrum = 4,     // spectrum of the two-step fall-back of the fused sinks (welch.generic / csd.generic: the frames' spectra); staged result of nxsig_fftconvolve_c64 (api.cpp); hilbert.generic: the rows' spectra (kernels_hilbert.hip); dct.fft: the result of its one row transform (kernels_dct.hip)
  kScratchReductionCells = 5,    // running maximum + non-finite flag of the log-mel / dBFS paths (kernels_generic.hip, group.cpp)
  kScratchFourStepA = 6,         // four-step rows: first buffer, also the tiled form's only one (kernels_nd.hip)
  kScratchFourStepB = 7,         // four-step rows: second buffer (kernels_nd.hip)
  kScratchBluesteinA = 8,        // Bluestein rows: chirped input / product (kernels_nd.hip)
  kScratchBluesteinB = 9,        // Bluestein rows: its transform (kernels_nd.hip)
  kScratchFftNdA = 10,           // fft_nd ping-pong buffers (kernels_nd.hip)
  kScratchFftNdB = 11,
  kScratchFftNdC = 12,
  kScratchConvNdA = 13,          // n-D fftconvolve: padded A, later the inverse transform's result (kernels_nd.hip)
  kScratchConvNdB = 14,          // n-D fftconvolve: padded B (kernels_nd.hip)
  kScratchConvNdC = 15,          // n-D fftconvolve: the product (kernels_nd.hip)
  kScratchLongStftFrames = 16,   // frames of the long-transform stft (launch_stft_big, kernels_nd.hip); welch / csd: row flags, partial sums, the generic tier's frames (kernels_welch.hip); sosfilt and lfilter: chunk and tile states, zi, zf (recurrence_scan.hpp)
  kScratchNdStageA = 17,         // host staging of the n-D / filter / peak / waveform calls: first input; the mask of the masked istft (api.cpp)
  kScratchNdStageB = 18,         // the same: second input; peak finding's `valid` cell (api.cpp)
  kScratchNdStageOut = 19,       // the same: results, several packed at a 256-byte stride (api.cpp)
  kScratchIstftProduct = 20,     // z * H / z * mask of the filtered and masked istft's two-step fall-back (launch_istft, api.cpp); hilbert.generic: the means of the rows that fill the transform, the dense (centred or gathered) rows, later the complex signal ahead of the sink — every output of a centred row, the f32 outputs of the others (kernels_hilbert.hip); dct.fft: the input of its one row transform — the row means and the permuted, centred rows (type 2) or the Hermitian spectra (type 3) (kernels_dct.hip)
  kScratchFirLong = 21,          // long FIR: full convolution row, partition outputs, delay-line spectra (api.cpp, kernels_wave_firlong.hip); sosfiltfilt and filtfilt: the extended rows and the forward result (recurrence_scan.hpp)
  kScratchFirRowFlags = 22,      // per-row non-finite flags of the FIR kernels (fir_row_flags, kernels_generic.hip)
  kScratchIstftNfList = 23,      // units with a non-finite bin reported by the multi-frame inverse kernels (istft_nf_list, kernels_generic.hip)
  kScratchPackedSpectrum = 24,   // packed istft fall-back: the Hermitian rows written out (launch_istft, api.cpp)
  kScratchPackedSignal = 25,     // packed istft fall-back: the complex signal before its real part is kept (launch_istft, api.cpp)
  kScratchStftC64Frames = 26,    // windowed frames of the generic complex-input stft (launch_stft_c64, kernels_generic.hip)
  kScratchIstftF64Frames = 27,   // frames of the f64 istft (kernels_f64.hip)
  kScratchWienerSums = 28,       // wiener's noise cell + per-workgroup partial sums (kernels_filters.hip)
  kScratchPeakTiles = 29,        // peak finding: mask words + tile counts / offsets (kernels_peaks.hip)
  kScratchPeakExtremes = 30,     // peak finding over a strided axis: window extremes (kernels_peaks.hip)
  kScratchSlots = 32             // (31 is free)
};

// ---- device tables cached per context ----
// The content-addressed cache (Ctx::tables) is bounded by COUNT: once a context holds more tables than this, the next API entry frees
// them all and forgets every pointer into them (DeviceGuard, api.cpp; DESIGN.md lists those pointer caches).  NXSIG_TABLE_CACHE_MAX
// overrides the bound of one context (tests cross it with a few dozen tables).
constexpr int kTableCacheMax = 1024;
struct DeviceTable {
  void* ptr = nullptr;
  size_t bytes = 0;
  std::vector<unsigned char> host;  // copy of the content (tables <= 1 MiB): a hash hit is verified against it
  bool has_host = false;            // (a zero-byte table has a host copy too: an empty one)
};

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  std::vector<hipEvent_t> lap_events;  // nxsig_timer_lap series: events are created on demand and reused
  size_t laps_used = 0;
  std::mutex mu;
  int num_cus = 0;
  std::string dev_name;
  // twiddle tables w_K^j = exp(-2 pi i j / K), j in [0,K), generated in double, stored as float2
  std::map<int, DeviceTable> twiddles;
  // content-addressed small tables (windows, filter spectra ...): key = fnv1a(tag, bytes)
  std::map<uint64_t, DeviceTable> tables; uint64_t table_requests = 0;   // ... and the calls of ctx_table so far ("TABLE_REQUESTS")
  // f64 tier (kernels_f64.hip): device pointers of its twiddle / chirp tables by (kind << 32 | length); the storage belongs to `tables`
  std::map<int64_t, const void*> f64_tables;
  // device scratch buffers reused from call to call, one per ScratchSlot (the enum names every slot and its owner); grown on demand
  // by ctx_scratch, freed with the context
  void* scratch[kScratchSlots] = {};
  size_t scratch_bytes[kScratchSlots] = {};
  // per-K tables of the tuned wave kernels (pass-B / pass-C twiddles), built once
  struct WaveTables { const void* twB = nullptr; const void* twC = nullptr; const void* twI = nullptr;
                      const void* twBi = nullptr; const void* twCi = nullptr;    // ...i = conjugated (inverse transform)
                      const void* twQ[3] = {nullptr, nullptr, nullptr}; };       // quad front-ends J = 2, 4, 8
  std::map<int, WaveTables> wave_tables;
  // memo of the last window seen (the common case: the same window tensor call after call)
  std::vector<float> memo_win;
  int memo_K = 0;
  const float* memo_dev = nullptr;   // f32[N]
  const float* memo_devK = nullptr;  // f32[K], zero-padded / truncated to the fft length
  // memo of host-side derivations keyed by the content they derive from (filter spectrum of a tap vector, OLA normaliser
  // rows and edge-fix sample list of a window): a few machine words each, dropped together with `tables`
  std::map<uint64_t, std::vector<uint64_t>> memo;
  // caching allocator behind nxsig_alloc / nxsig_free: freed blocks are kept (no hipFree, no device synchronisation) and handed
  // out again to requests of a similar size.  A 3.3 GB hipMalloc costs ~100 ms on this platform — two hundred times the
  // stft that fills it — so a caller that allocates its result per call (the Python mirror, the NIF's *_dev functions) would
  // otherwise spend all its time in the allocator.  Reuse is ordered by the context's stream.
  std::multimap<size_t, void*> pool_free;   // size -> block
  std::map<void*, size_t> pool_live;        // blocks handed out by nxsig_alloc
  size_t pool_cached = 0, pool_cap = 0;     // bytes sitting in pool_free; cap (0 = not yet decided)
  // host-tensor calls (mem = NXSIG_HOST): two pinned bounce slots per direction + a transfer stream.  The result travels in chunks:
  // DMA of chunk k + 1 into one slot while host threads copy chunk k out of the other into the caller's (pageable) buffer
  // (Staged::out_copy, api.cpp); created on the first host-tensor call of at least kPinMin bytes, freed with the context
  void* pin[4] = {nullptr, nullptr, nullptr, nullptr};   // [0, 1] device -> host, [2, 3] host -> device
  size_t pin_bytes = 0; hipStream_t xfer_stream = nullptr;
  hipEvent_t xfer_ev[4] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t xfer_ready = nullptr;
  // czt.generic's two temporaries (kernels_czt.hip), its own: grown on demand like a scratch slot, kept from call to call, freed with the context
  struct OwnedBuffer { void* ptr = nullptr; size_t bytes = 0; OwnedBuffer() = default; OwnedBuffer(const OwnedBuffer&) = delete; OwnedBuffer& operator=(const OwnedBuffer&) = delete; ~OwnedBuffer() { if (ptr) (void)hipFree(ptr); } } czt_rows, czt_spectra; OwnedBuffer cwt_flags, cwt_rows, cwt_spectra, cwt_conv; OwnedBuffer xcorr_a, xcorr_b, xcorr_sa, xcorr_sb;   // ... and cwt's own (kernels_cwt.hip), kept the same way: the per-row non-finite flags (zero between calls), cwt.generic's three temporaries; xcorr.generic's four temporaries (kernels_xcorr.hip), kept the same way: the padded rows of either operand and their spectra, one slab of pairs each
  std::string last_dispatch;                // kernel families of the last compute call on this context (nxsig_ctx_last_dispatch)
  Tuning tuning;                            // dispatch / geometry switches (environment at creation, nxsig_ctx_set_tuning later)
};
// value of a switch for this context, or the launcher's default when nobody set it
static inline int tune(const Ctx* c, TuneKey k, int dflt) { return c->tuning.set[k] ? (int)c->tuning.v[k] : dflt; }

// Units per wave of a short-lived-workgroup launch (round 6): the measured optimum `dflt` of a launch that runs for many rounds of
// workgroups — but a launch with fewer workgroups than three per CU is ONE round, what sets its time is the longest wave, and it should
// spread over the chip instead (a 10 s utterance at 16 kHz in 400 / 512 framing: 250 units = 16 workgroups at 4 units per wave, 24.4 us;
// at one unit per wave 63 workgroups, 15.4 us; config 1's 2048-point twin 23.5 -> 7.2 us: profiles/r06/small_launch_units_per_wave.txt)
static inline int fill_units_per_wave(const Ctx* c, int64_t total_units, int W, int dflt) {
  const int64_t slots = (int64_t)c->num_cus * 3 * W;
  const int64_t fill = (total_units + slots - 1) / slots;
  return fill < dflt ? (fill < 1 ? 1 : (int)fill) : dflt;
}
// ... behind the launcher's geometry switch (NXSIG_WAVE_UNITS_PER_WAVE for the forward and row kernels, NXSIG_FIR_UNITS_PER_WAVE for the
// FIR streams): switch set -> its value (range-checked at the way in, tuning_in_range), else the heuristic above.  Every streaming kernel
// walks its chunk with `for (u = begin + wave; u < end; u += W)`, so any value computes the same result (tests/test_gpu_launch_geometry.py)
static inline int tuned_units_per_wave(const Ctx* c, TuneKey k, int64_t total_units, int W, int dflt) {
  return c->tuning.set[k] ? (int)c->tuning.v[k] : fill_units_per_wave(c, total_units, W, dflt);
}

// Shortest run of the persistent inverse kernels (every run recomputes its halo, so long runs pay less of it — but a launch with fewer
// units than two per wave slot is ONE partial round, and what sets its time is the length of a run: 1 s of audio, 184 frames, ran as 23
// runs of 8 + 3 frames on 23 of 2 048 wave slots).  Such launches take runs of 2: N = 1024 one second 29.8 -> 19.9 us, N = 2048 ten
// seconds 61 -> 40 us, N = 256 36 -> 19 us (profiles/r06/small_launch_istft_min_run.txt).  NXSIG_ISTFT_MIN_RUN overrides.
static inline int istft_min_run(const Ctx* c, int64_t total_units, int64_t slots, int dflt) {
  if (c->tuning.set[kT_ISTFT_MIN_RUN]) return (int)c->tuning.v[kT_ISTFT_MIN_RUN];
  return total_units <= 2 * slots ? 2 : dflt;
}

// Set (for the calling THREAD and one context) by the sharded log-mel of group.cpp while it runs pass 1 on a member: the clamp
// pass of stft_to_mel / the fused mel sink is NOT launched — the running maximum of the member's shard must first be
// all-reduced with the other members'; the group launches the pass afterwards.  Thread-local on purpose: another thread that
// calls nxsig_stft_mel_f32 / stft_to_mel on the same context at the same time keeps its own clamp pass, and the scope guard
// clears the mark on every way out.
struct MelDeferScope {
  explicit MelDeferScope(const Ctx* c);
  ~MelDeferScope();
  MelDeferScope(const MelDeferScope&) = delete;
  MelDeferScope& operator=(const MelDeferScope&) = delete;
};
bool mel_deferred(const Ctx* c);

int ctx_twiddles(Ctx* c, int K, const float2** out);
int ctx_table(Ctx* c, uint64_t tag, const void* host, size_t bytes, const void** out);
int ctx_scratch(Ctx* c, ScratchSlot slot, size_t bytes, void** out);
// device copies of a host window: raw f32[N] and the K-point table (Nx.fft(length: K) pads / truncates rows)
int ctx_window(Ctx* c, const float* window_host, int N, int K, const float** dev, const float** devK);
uint64_t fnv1a(uint64_t seed, const void* data, size_t bytes);

// ---- kernel launchers (implemented in the .hip files; all enqueue on c->stream) ----
struct StftLaunch {
  const float* x;        // device, [batch][L] rows batch_stride apart
  int64_t batch_stride;
  int32_t batch;
  Framing fr;
  int32_t K;             // fft length
  const float* window;   // device f32[N]
  const float* window_padK = nullptr;  // device f32[K] (zero-padded / truncated), used by the wave kernel
  float inv_scale_div;   // spectrum is DIVIDED by this (1.0 = none); division kept exact like the reference
  int32_t has_scale;
  float2* z;             // device c64[batch][M][K]
};
int launch_stft(Ctx* c, const StftLaunch& a);
int launch_stft_c64(Ctx* c, const StftLaunch& a);   // complex samples: a.x holds c64[batch][L] (kernels_generic.hip)

struct IstftLaunch {
  const float2* z;       // device c64[batch][M][K]
  int64_t M;
  int32_t batch;
  int32_t N, hop, K;
  const float* window;   // device f32[N]
  float scale_mul;       // frames are MULTIPLIED by this (istft :614/:617)
  int32_t has_scale;
  float2* y;             // device c64[batch][M*hop + N-hop]
  const float2* filt = nullptr;  // optional device c64[K]: every frame's spectrum is multiplied by it first (z * H of the
                                 // STFT-domain filtering chain, guides/filtering.livemd:141), rounded to c64 like Nx.multiply
  // optional time-frequency mask (nxsig_istft_masked_c64): frame m of row r is z[r][m][k] * mask[r][m][k] rounded to c64 first.
  // mask_kind: nxsig_mask_kind.  z_bcast / mask_bcast: that operand has ONE row, read for every row of the batch (row stride 0)
  const void* mask = nullptr;
  int32_t mask_kind = 0;
  bool z_bcast = false, mask_bcast = false;
  // set by a wave launcher whose kernel inverts several frames with ONE transform: the device list of units that hold a
  // non-finite bin and the frames per unit; launch_istft then recomputes those units' samples frame by frame (k_istft_edge_fix's second role)
  mutable int* nf_list = nullptr;
  mutable int nf_frames_per_unit = 0;
  // packed one-sided form (nxsig_istft_packed_f32): z is c64[batch][M][K / 2] — bins 0 .. K/2 - 1 with Re X[K/2] in the imaginary
  // part of bin 0 — and y is REAL f32[batch][M*hop + N-hop]
  bool onesided = false;
};
// elements (f32 or c64, by kind) of one mask row of one frame
__host__ __device__ __forceinline__ int64_t mask_row_len(int32_t kind, int32_t K) { return kind == NXSIG_MASK_ONESIDED ? K / 2 + 1 : K; }
// one bin of a masked spectrum: the product Nx.multiply forms on the BinaryBackend (double, one rounding per component); a real
// gain multiplies each component on its own.  mrow: the mask row of the bin's (row, frame).  Shared by k_spectrum_mask, the fused
// kernel and the edge fix-up, so that every path rounds alike
__device__ __forceinline__ float2 spectrum_mask_apply(float2 v, const void* mrow, int32_t kind, int32_t k, int32_t K) {
  if (kind == NXSIG_MASK_COMPLEX) {
    const float2 h = reinterpret_cast<const float2*>(mrow)[k];
    return make_float2((float)((double)v.x * (double)h.x - (double)v.y * (double)h.y),
                       (float)((double)v.x * (double)h.y + (double)v.y * (double)h.x));
  }
  const float g = reinterpret_cast<const float*>(mrow)[(kind == NXSIG_MASK_ONESIDED && k > K / 2) ? K - k : k];
  return make_float2((float)((double)v.x * (double)g), (float)((double)v.y * (double)g));
}
int launch_spectrum_mask(Ctx* c, const float2* z, bool z_bcast, const void* mask, int32_t kind, bool mask_bcast, int64_t rows, int64_t M,
                         int32_t K, float2* out);
int launch_istft_wave_mask(Ctx* c, const IstftLaunch& s, const float* window_host, bool* handled);   // kernels_wave_mask.hip
int launch_half_from_spectrum(Ctx* c, const float2* z, int64_t rows, int32_t K, float2* out, bool packed);
int launch_full_from_packed(Ctx* c, const float2* zp, int64_t rows, int32_t K, float2* out);
int launch_real_from_c64(Ctx* c, const float2* in, int64_t n, float* out);
int istft_nf_list(Ctx* c, int64_t capacity, int** list);
int launch_istft_fix(Ctx* c, const IstftLaunch& s, const float* window_host);   // k_istft_edge_fix: edge samples + reported non-finite units
int launch_istft(Ctx* c, const IstftLaunch& a, const float* window_host);

int launch_as_windowed(Ctx* c, const float* x, int64_t batch_stride, int32_t batch, const Framing& fr, float* out);
int launch_overlap_and_add(Ctx* c, const float* frames, int64_t M, int32_t batch, int32_t N, int32_t hop, int32_t comps,
                           float* out);
// clean: apply the Nx.fft / Nx.ifft eps clean-up to the result (false for transforms that are sub-steps of a longer one)
int launch_fft(Ctx* c, const void* in, bool in_is_real, int64_t rows, int32_t n_in, int32_t K, bool inverse, float2* out, bool clean = true);

struct FirLaunch {
  const float* x;
  int64_t L, batch_stride;
  int32_t batch;
  const float* h_host;
  int32_t taps;
  int64_t out_start, out_len;  // requested slice of the full convolution
  float* y;                    // device f32[batch][out_len]
  // device int[batch], zero on entry: a kernel that loads a non-finite sample of row r sets row_flags[r]; launch_fir's last
  // pass (k_fir_poison) then makes the whole row NaN and clears the flag.  The reference filters by ONE transform of the whole
  // row (Convolution.fftconvolve, lib/nx_signal/convolution.ex:276-284), so an Inf / NaN sample anywhere leaves no finite
  // output in that row; block-wise overlap-save would otherwise confine it to the blocks (and block pairs) that hold it.
  int* row_flags = nullptr;
};
int launch_fir(Ctx* c, const FirLaunch& a);
int launch_fir_dline(Ctx* c, const FirLaunch& a, bool* handled);   // kernels_wave_firlong.hip: 1 026 ... 32 769 taps
int fir_row_flags(Ctx* c, int32_t batch, int** out);                                                     // kernels_generic.hip
int launch_fir_poison(Ctx* c, const FirLaunch& a);
int launch_fir_flags_from_output(Ctx* c, const float* y, int32_t rows, int64_t out_len, int* flags);     // sample-sharded FIR, group.cpp
int launch_mag_from_spectrum(Ctx* c, const float2* z, int64_t rows, int32_t K, int kind, float* out);
int launch_stft_mag_wave(Ctx* c, const StftLaunch& s, int kind, float* out, bool* handled);
int launch_spectrum_mul(Ctx* c, const float2* z, int64_t rows, int32_t K, const float2* h_dev, float2* out);
int launch_stft_to_mel(Ctx* c, const float2* z, int64_t rows, int32_t K, int32_t mel_bins, const float* filters_host,
                       float* out);
int launch_stft_mel_wave(Ctx* c, const StftLaunch& s, int mel_bins, const float* filters_host, float* out, bool* handled);
// the two cells {running maximum in ordered-int encoding, non-finite flag} of the log-mel paths and their clamp pass
int launch_mel_init(Ctx* c, int** gmax);
int launch_mel_finish(Ctx* c, float* out, int64_t n, int* gmax);
// kernels_nd.hip: rows of any length (four-step / Bluestein beyond the LDS-resident kernels), device-side fft_nd, n-D fftconvolve
int launch_fft_big(Ctx* c, const void* in, bool in_is_real, int64_t rows, int64_t n_in, int64_t K, bool inverse, float2* out, bool clean = true);
int64_t fft_tiled_min(const Ctx* c);   // power-of-two row lengths from here up run the two-pass tiled four-step of kernels_nd.hip
int launch_rows_post(Ctx* c, float2* a, int64_t rows, int64_t K, const float* window, float scale, bool has_scale, float div, bool has_div);
int launch_fft_nd(Ctx* c, const void* in, bool in_is_real, const int64_t* shape, int rank, const int32_t* axes, const int64_t* lengths,
                  int n_axes, bool inverse, float2* out);
int launch_convolve_direct(Ctx* c, const void* a, bool a_is_real, const int64_t* s1, const void* b, bool b_is_real, const int64_t* s2,
                           int rank, int mode, void* out, int64_t* out_shape);
int launch_fftconvolve_nd(Ctx* c, const void* a, bool a_is_real, const int64_t* s1, const void* b, bool b_is_real, const int64_t* s2,
                          int rank, int mode, void* out, int64_t* out_shape);
int launch_stft_big(Ctx* c, const StftLaunch& s);
// kernels_filters.hip: Filters.median / wiener over device tensors of rank <= 8 (f32, or f64 when f64).  median writes f32; wiener
// writes the input's type and, when it estimates the noise (!has_noise), leaves the estimate in a device cell (*noise_dev)
int launch_median(Ctx* c, const void* x, bool f64, const int64_t* shape, int rank, const int64_t* ks, float* out);
int launch_wiener(Ctx* c, const void* x, bool f64, const int64_t* shape, int rank, const int64_t* ks, bool has_noise, double noise, void* out,
                  const double** noise_dev);
// kernels_resample.hip: Filters.resample_poly (include/nxsig.h states the definition).  up / down are REDUCED, up != down; h_host are
// the taps with the gain included; y is dense [batch][n_out].  The phase table goes through ctx_table; nothing waits
struct ResampleLaunch {
  const void* x;               // device f32 / c64 [batch][n], rows batch_stride elements apart
  bool is_complex;
  int64_t n, batch_stride, n_out;
  int32_t batch;
  const float* h_host;
  int32_t taps, up, down;
  void* y;
};
constexpr int kResampleTile = 1024;   // outputs of one row per workgroup of the LDS tier
int launch_resample_poly(Ctx* c, const ResampleLaunch& a);
int launch_resample_copy(Ctx* c, const ResampleLaunch& a);
// kernels_peaks.hip: PeakFinding.argrelextrema over a device tensor (dtype: nxsig_dtype; the shape checks are the caller's) and the
// nonzero compaction of a u8 mask; indices [size][rank] and *valid on the device, nothing waits
int launch_argrelextrema(Ctx* c, const void* x, int dtype, const int64_t* shape, int rank, int axis, int64_t shifts, int comparator,
                         int32_t* indices, uint32_t* valid);
int launch_nonzero(Ctx* c, const uint8_t* mask, const int64_t* shape, int rank, int32_t* indices, uint32_t* valid);
// kernels_waveforms.hip: NxSignal.Waveforms over n device elements (f32, or f64 when f64).  The scalars are computed by the caller
// under the tier's rounding and passed by value; n == 0 launches nothing; nothing waits
struct WaveSaw {
  double two_pi, thr, d_rise, c_fall, d_fall;   // 2 pi(), 2 pi() width, pi() width, pi() (width + 1), pi() (1 - width)
  int32_t mode;                                 // 1: width == 1 (rise only), 0: width == 0 (fall only), 2: select on tmod < thr
};
struct WaveSquare {
  double two_pi, pi, thr;   // thr = duty * 2 * pi() of a scalar duty
};
struct WaveGauss {
  double neg_a, w;   // -a, 2 pi() fc
};
enum WaveChirpKind { kChirpLinear = 0, kChirpQuadratic, kChirpQuadraticT1, kChirpLogarithmic, kChirpHyperbolic, kChirpConstant, kChirpNan };
struct WaveChirp {
  int32_t kind;
  double two_pi, a, b, c, d, phi;   // per kind: see ChirpOp
};
constexpr int kWaveSweepMaxCoefs = 32;
struct WaveSweep {
  int32_t n;
  double two_pi, phi;
  double coef[kWaveSweepMaxCoefs];   // coefs[k] / (n - k)
};
int launch_sawtooth(Ctx* c, const void* t, bool f64, int64_t n, const WaveSaw& p, void* out);
int launch_square(Ctx* c, const void* t, bool f64, int64_t n, const WaveSquare& p, const void* duty, int32_t* out);
int launch_gaussian_pulse(Ctx* c, const void* t, bool f64, int64_t n, const WaveGauss& p, void* envelope, void* in_phase, void* quadrature);
int launch_chirp(Ctx* c, const void* t, bool f64, int64_t n, const WaveChirp& p, const char* family, void* out);
int launch_polynomial_sweep(Ctx* c, const void* t, bool f64, int64_t n, const WaveSweep& p, void* out);
int launch_unit_impulse(Ctx* c, void* out, int dtype, int64_t n, int64_t at);

// ---- f64 / c128 tier (kernels_f64.hip) ----
struct StftLaunchD {
  const double* x;       // device f64[batch][L], rows batch_stride apart; x_is_complex: c128[batch][L], batch_stride in complex elements
  int32_t x_is_complex = 0;
  int64_t batch_stride;
  int32_t batch;
  Framing fr;
  int32_t K;
  const double* window;  // device f64[N]
  double div;            // the spectrum is DIVIDED by this
  int32_t has_scale;
  double2* z;            // device c128[batch][M][K]
};
struct IstftLaunchD {
  const double2* z;      // device c128[batch][M][K]
  int64_t M;
  int32_t batch, N, hop, K;
  const double* window;  // device f64[N]
  double scale_mul;
  int32_t has_scale;
  int32_t window_f32;    // the caller's window was f32: the |w|^2 normaliser is formed with f32 roundings like the reference's
  double2* y;            // device c128[batch][M*hop + N-hop]
};
struct FirLaunchD {
  const double* x;
  int64_t L, batch_stride;
  int32_t batch;
  const double* h_host;
  int32_t taps;
  int64_t out_start, out_len;
  double* y;
};
int launch_stft_f64(Ctx* c, const StftLaunchD& s);
int launch_istft_f64(Ctx* c, const IstftLaunchD& s);
int launch_fft_f64(Ctx* c, const void* in, bool in_is_real, int64_t rows, int32_t n_in, int32_t K, bool inverse, double2* out,
                   const double* post_window = nullptr, double post_scale = 1.0, bool has_post_scale = false);
int launch_ola_f64(Ctx* c, const double* frames, int64_t M, int32_t batch, int32_t N, int32_t hop, int32_t comps, const double* window,
                   bool norm, bool window_f32, double* out);
int launch_as_windowed_f64(Ctx* c, const double* x, int64_t batch_stride, int32_t batch, const Framing& f, double* out);
int launch_fir_f64(Ctx* c, const FirLaunchD& s);
int launch_fftconvolve_c64(Ctx* c, const float2* a, int64_t n1, const float2* b, int64_t n2, int64_t start, int64_t len,
                           float2* out);

// kernels_welch.hip: Spectral.welch / csd (include/nxsig.h states the definition, DESIGN.md section 3.12 the design).  y == nullptr:
// welch (pxx only).  Temporaries: kScratchLongStftFrames holds the per-row non-finite flags, the partial sums [row][run][plane][bin]
// of one slab of rows and, in the generic tier, a chunk's detrended windowed frames; kScratchFusedSpectrum holds that chunk's spectra.
// Everything is enqueued on c->stream; nothing waits
struct WelchLaunch {
  const float* x;            // device f32[batch][L], rows batch_stride elements apart
  const float* y;            // the same layout, or nullptr
  int64_t L, batch_stride;
  int32_t batch, N, hop, K;
  const float* window_host;  // f32[N]
  bool detrend;
  double scale;              // 1 / (fs sum w^2) or 1 / (sum w)^2
  float* pxx;                // device f32[batch][K / 2 + 1] (csd: may be null)
  float* pyy;                // csd only, may be null
  float2* pxy;               // csd only
};
int launch_welch(Ctx* c, const WelchLaunch& a);

}  // namespace nxsig

#include "iir_plan.hpp"
#include "welch_plan.hpp"

namespace nxsig {
// recurrence_scan.hpp: what one run of a recursive filter over `batch` rows is told, whichever family it belongs to.  Logical sample i of
// a row is physical sample i (direction 0) or n - 1 - i (direction 1); output sample p (physical) goes to y[row * y_stride + p - out_off]
// when 0 <= p - out_off < out_len.  Temporaries (chunk and tile states, zi, zf) live in kScratchLongStftFrames.  Enqueued on c->stream;
// only a call that returns zf or brings a zi of the caller's waits
struct ScanLaunch {
  const float* x;          // device f32[batch][n], rows x_stride elements apart
  int64_t n, x_stride;
  int32_t batch;
  const double* zi_host;   // f64[zi_rows][states of the filter] or nullptr (zero state)
  int32_t zi_rows;         // 1 or batch
  bool zi_times_first;     // the start state of a row is zi * (its first logical sample): the forward-backward filters
  double* zf_host;         // f64[batch][states of the filter] or nullptr
  int32_t direction;
  float* y;                // device
  int64_t y_stride, out_off, out_len;
};
// kernels_iir.hip: Filters.sosfilt / sosfiltfilt (include/nxsig.h states the definition, DESIGN.md section 3.13 the design).  One
// run of the cascade; a row has 2 n_sections states ([n_sections][2])
struct IirLaunch : ScanLaunch {
  const double* sos_host;  // f64[n_sections][6]
  int32_t n_sections;      // 1 .. kIirMaxSections
};
int launch_sosfilt(Ctx* c, const IirLaunch& a);
// sosfiltfilt: x rows -> extended rows (padtype 1 odd, 2 even, 3 constant; edge samples each side) in kScratchFirLong, forward,
// backward, the middle slice to y (dense [batch][n])
int launch_sosfiltfilt(Ctx* c, const float* x, int64_t n, int64_t x_stride, int32_t batch, const double* sos_host, int32_t n_sections,
                       int32_t padtype, int64_t edge, float* y);
}  // namespace nxsig

#include "find_peaks_plan.hpp"

namespace nxsig {
// kernels_find_peaks.hip: PeakFinding.find_peaks over a device tensor (include/nxsig.h states the rules, DESIGN.md section 3.14 the
// design; the argument checks are the caller's).  The mask words live in kScratchPeakTiles, the line summary and the survivors' positions
// in kScratchPeakExtremes: find_peaks and argrelextrema never overlap on one stream.  A call with a distance condition waits once per
// round of the distance stage; every other call only enqueues on c->stream
struct FindPeaksLaunch {
  const void* x;           // device f32, or f64 when f64
  bool f64;
  const int64_t* shape;
  int32_t rank, axis;
  uint32_t conditions;     // FindPeaksCondition bits
  const double* bounds;    // host f64[5][2] or nullptr
  double distance;
  int64_t wlen;            // -1: none
  double rel_height;
  int64_t capacity;
  uint32_t want;           // FindPeaksProperty bits
  int32_t* indices;        // device s32[capacity][rank]
  uint32_t* valid;         // device
  double* fprops;          // device f64[f64 rows wanted][capacity]
  int32_t* iprops;         // device s32[s32 rows wanted][capacity], or nullptr: the launcher keeps them in its scratch ...
  int32_t** iprops_used;   // ... and says where (may be nullptr)
};
int launch_find_peaks(Ctx* c, const FindPeaksLaunch& a);
int32_t find_peaks_last_rounds();   // rounds of the distance stage in the calling thread's last launch_find_peaks
}  // namespace nxsig

#include "savgol_plan.hpp"

namespace nxsig {
// kernels_savgol.hip: Filters.savgol_filter over device rows (include/nxsig.h states the definition, DESIGN.md section 3.15 the design;
// the argument checks are the caller's).  The weights and the edge table of mode "interp" are cached tables of the context, formed once
// per parameter set.  No scratch; everything is enqueued on c->stream and nothing waits (the first call of a parameter set uploads)
struct SavgolLaunch {
  const void* x;           // device f32, or f64 when f64: [batch][n], rows x_stride elements apart
  bool f64;
  int64_t n, x_stride;
  int32_t batch;
  int32_t W, p, deriv;     // window_length, polyorder, deriv
  double delta;
  int32_t mode;            // SavgolMode
  double cval;
  void* y;                 // device, dense [batch][n]
};
int launch_savgol(Ctx* c, const SavgolLaunch& a);
}  // namespace nxsig

#include "hilbert_plan.hpp"

namespace nxsig {
// kernels_hilbert.hip: Filters.hilbert over device rows (include/nxsig.h states the definition, DESIGN.md section 3.16 the design; the
// argument checks are the caller's).  hilbert.wave uses no scratch; hilbert.generic keeps the spectra in kScratchFusedSpectrum and, for
// every row that fills the transform (length >= n_fft: it is centred, whatever the output), for strided rows and for an f32 result, a
// second temporary in kScratchIstftProduct: the row means | the dense rows, later the complex signal ahead of the sink.  Everything is enqueued on c->stream and nothing waits
struct HilbertLaunch {
  const float* x;          // device f32[batch][length], rows x_stride elements apart
  int64_t length, x_stride;
  int32_t batch;
  int64_t n_fft;
  int32_t kind;            // HilbertKind
  void* out;               // device, dense [batch][n_fft]: c64 (analytic) or f32 (envelope, quadrature)
};
int launch_hilbert(Ctx* c, const HilbertLaunch& a);
}  // namespace nxsig

namespace nxsig {
// nxsig_ctx_get_tuning's read-only name "TABLE_REQUESTS" (or "NXSIG_TABLE_REQUESTS"): how often ctx_table was called on the context,
// modulo 2^31, is_set = 0.  A call served from a memo of table pointers makes no request, which is how the tests see that a repeated
// call formed nothing again.  False for any other name (api.cpp)
bool table_requests_query(const Ctx* c, const char* name, int32_t* value, int32_t* is_set);
}  // namespace nxsig

#include "dct_plan.hpp"

namespace nxsig {
// kernels_dct.hip: Transforms.dct / idct over device rows (include/nxsig.h states the definition, DESIGN.md section 3.17 the design; the
// argument checks are the caller's).  dct.direct uses no scratch; dct.fft keeps the input of its row transform (type 2: behind the row means) in
// kScratchIstftProduct and the transform's result in kScratchFusedSpectrum.  The cosine / twiddle table goes through ctx_table once per context and
// parameter set.  Everything is enqueued on c->stream and nothing waits
struct DctLaunch {
  const float* x;          // device f32[batch][length], rows x_stride elements apart
  int64_t length, x_stride, batch;
  int64_t n;               // points of the transform: the row is truncated or zero-padded
  int32_t type, norm;      // 2 or 3; DctNorm
  int64_t keep;            // leading coefficients stored, 1 <= keep <= n
  float* out;              // device, dense [batch][keep]
};
int launch_dct(Ctx* c, const DctLaunch& a);
}  // namespace nxsig

#include "lfilter_plan.hpp"

namespace nxsig {
// kernels_lfilter.hip: Filters.lfilter / filtfilt (include/nxsig.h states the definition, DESIGN.md section 3.18 the design; the argument
// checks are the caller's).  One run of the filter; a row has cf.n states, none when the filter is a gain
struct LfLaunch : ScanLaunch {
  LfCoefs cf;              // b and a divided by a[0], zero-padded; cf.n the order 0 .. kLfMaxOrder
};
int launch_lfilter(Ctx* c, const LfLaunch& a);
// filtfilt: x rows -> extended rows (padtype 1 odd, 2 even, 3 constant; edge samples each side) in kScratchFirLong, forward, backward,
// the middle slice to y (dense [batch][n])
int launch_filtfilt(Ctx* c, const float* x, int64_t n, int64_t x_stride, int32_t batch, const LfCoefs& cf, int32_t padtype, int64_t edge, float* y);
}  // namespace nxsig

#include "lombscargle_plan.hpp"

namespace nxsig {
// kernels_lombscargle.hip: Spectral.lombscargle (include/nxsig.h states the definition, DESIGN.md section 3.19 the design; the argument
// checks are the caller's).  x, freqs and the weights are HOST arrays: they reach the device through ctx_table, the weights normalised
// to sum 1 (ones where weights_host is null).  No scratch.  Enqueued on c->stream; nothing waits once the tables are cached
struct LsLaunch {
  const void* y;             // device f32 / f64 [batch][n], rows y_stride elements apart
  bool f64;
  int64_t n, y_stride;
  int32_t batch;
  const double* x_host;      // f64[n]
  const double* freqs_host;  // f64[num_freqs], angular
  int64_t num_freqs;
  const double* weights_host;   // f64[n] or nullptr
  int32_t precenter, normalize, floating_mean;
  void* out;                 // device, dense [batch][num_freqs]: f32 / f64, c64 / c128 under kLsAmplitude
};
int launch_lombscargle(Ctx* c, const LsLaunch& a);
}  // namespace nxsig

#include "czt_plan.hpp"

namespace nxsig {
// kernels_czt.hip: Transforms.czt / zoom_fft over device rows (include/nxsig.h states the definition, DESIGN.md section 3.20 the design;
// the argument checks are the caller's).  czt.wave uses no temporary; czt.generic keeps two of its own (Ctx::czt_rows: the chirped
// zero-padded rows, later their spectra times F; Ctx::czt_spectra: the two transforms' results).  The three tables go through ctx_table once per
// context and parameter set (a memo keeps the pointers: a repeated call makes no table request).  Everything is enqueued on c->stream
// and nothing waits once the tables are cached
struct CztLaunch {
  const void* x;           // device f32 / c64 [batch][length], rows x_stride elements apart
  bool is_complex;
  int64_t length, x_stride, batch;
  int64_t m;               // output points
  CztContour contour;
  void* out;               // device, dense c64 [batch][m]
};
int launch_czt(Ctx* c, const CztLaunch& a);
}  // namespace nxsig

#include "cwt_plan.hpp"

namespace nxsig {
// kernels_cwt.hip: Filters.fir_bank / Transforms.cwt over device rows (include/nxsig.h states the definition, DESIGN.md section 3.21
// the design; the argument checks are the caller's).  The bank is split by support and one launch group runs per non-empty class.  The
// filters' spectra go through ctx_table once per context, class and bank (a memo keeps the pointers: a repeated call makes no table
// request).  Temporaries are the family's own (Ctx::cwt_flags and, for cwt.generic, cwt_rows / cwt_spectra / cwt_conv).  Everything is
// enqueued on c->stream and nothing waits once the tables are cached
struct CwtLaunch {
  const float* x;             // device f32 [batch][length], rows x_stride elements apart
  int64_t length, x_stride, batch;
  const double* taps_host;    // the filters concatenated, interleaved complex doubles
  const int64_t* tap_counts;  // host [num_filters]
  int64_t num_filters;
  int32_t kind;               // CwtKind
  void* out;                  // device, dense [batch][num_filters][length]: c64 (kCwComplex) or f32
};
int launch_cwt(Ctx* c, const CwtLaunch& a);
}  // namespace nxsig

#include "xcorr_plan.hpp"

namespace nxsig {
// kernels_xcorr.hip: Convolution.correlate_rows / convolve_rows over device rows (include/nxsig.h states the definition, DESIGN.md
// section 3.22 the design; the argument checks are the caller's).  xcorr.wave uses no temporary and no table beyond the wave twiddles;
// xcorr.generic keeps four temporaries of its own (Ctx::xcorr_a / xcorr_b: the zero-padded rows, later the cross spectrum;
// Ctx::xcorr_sa / xcorr_sb: the spectra, later the circular result) and walks the batch in slabs.  Everything is enqueued on c->stream
struct XcorrLaunch {
  const void* a;           // device f32 / c64 [batch][n1], rows a_stride elements apart
  const void* b;           // device f32 / c64 [batch][n2], rows b_stride elements apart; b_stride 0: one row for every pair
  bool is_complex;
  int64_t n1, a_stride, n2, b_stride, batch;
  int32_t op, mode, weighting, sink;
  float phat_floor;
  void* out;               // device, dense: [batch][n_out] (rows) or [batch] (peak), f32 or c64 as the operands
  int32_t* out_lags;       // device s32 [batch] (peak), else unused
};
int launch_xcorr(Ctx* c, const XcorrLaunch& a);
}  // namespace nxsig
