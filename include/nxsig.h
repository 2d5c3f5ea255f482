/*
 * nxsig.h — C ABI of the MI355X-native STFT / iSTFT / FIR hot path behind the NxSignal API.
 *
 * This is the drop-in boundary: everything a host language needs
 * (the Elixir dirty-NIF shim in nif/nxsig_nif.c, the Python mirror in nx_signal_amd/, the C++
 * tests) goes through these `extern "C"` entry points — plain pointers and sizes, no torch /
 * C++ types.  The reference has no native code; each entry point replaces the Nx primitives
 * the cited reference lines compose on Nx.BinaryBackend (file:line are relative to the
 * reference root, elixir-nx/nx_signal v0.3.0).
 *
 * Conventions
 *   - every function returns NXSIG_OK (0) or a negative nxsig_status; a human readable message
 *     for the calling thread is available from nxsig_last_error().  Nothing aborts, throws or
 *     longjmps across this boundary (dirty-NIF safe).
 *   - buffers are caller-allocated and never retained after the call returns.
 *   - `mem` says where the SIGNAL buffers (x, z, y ...) live: NXSIG_HOST (the library stages
 *     them through HBM — PCIe-bound, convenience path) or NXSIG_DEVICE (HBM pointers from
 *     nxsig_alloc or any other HIP allocator — the hot path; the call is asynchronous on the
 *     context's stream and returns once the kernels are enqueued).
 *   - small parameter tables (window, FIR taps) are ALWAYS host pointers: they are user-built
 *     tensors of a few KB, hashed and cached in HBM per context.
 *   - c64 = interleaved little-endian (f32 re, f32 im), row-major — Nx's native layout.
 *   - a context is bound to one GPU and one HIP stream; calls on one context are serialised
 *     by an internal mutex, different contexts may be used concurrently from any OS thread.
 */
#ifndef NXSIG_H
#define NXSIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NXSIG_ABI_VERSION 1

typedef struct nxsig_ctx nxsig_ctx;

typedef struct nxsig_c64 {
  float re, im;
} nxsig_c64;

typedef struct nxsig_c128 {
  double re, im;
} nxsig_c128;

typedef enum nxsig_status {
  NXSIG_OK = 0,
  NXSIG_ERR_INVALID_ARG = -1, /* maps to ArgumentError on the Elixir side */
  NXSIG_ERR_UNSUPPORTED = -2, /* valid in the reference, not built here yet (message says what) */
  NXSIG_ERR_HIP = -3,         /* a HIP runtime call failed */
  NXSIG_ERR_NO_DEVICE = -4,
  NXSIG_ERR_OOM = -5
} nxsig_status;

typedef enum nxsig_mem { NXSIG_HOST = 0, NXSIG_DEVICE = 1 } nxsig_mem;

/* as_windowed padding modes — lib/nx_signal.ex:303-331, :343-352 */
typedef enum nxsig_pad {
  NXSIG_PAD_VALID = 0,    /* :valid (default of stft, :76) */
  NXSIG_PAD_REFLECT = 1,  /* :reflect — div(N,2) each side, mirror without edge repeat (:262, :348-349) */
  NXSIG_PAD_SAME = 2,     /* :same — k-1 total, floor left / ceil right (:308-312) */
  NXSIG_PAD_EXPLICIT = 3  /* [{lo, hi}] zero padding (negative = crop, as Nx.pad) (:314-323) */
} nxsig_pad;

/* stft/istft :scaling — lib/nx_signal.ex:113-127, :611-625 */
typedef enum nxsig_scaling { NXSIG_SCALE_NONE = 0, NXSIG_SCALE_SPECTRUM = 1, NXSIG_SCALE_PSD = 2 } nxsig_scaling;

/* NxSignal.Windows — lib/nx_signal/windows.ex */
typedef enum nxsig_window_kind {
  NXSIG_WIN_RECTANGULAR = 0, /* :33  */
  NXSIG_WIN_BARTLETT = 1,    /* :57  */
  NXSIG_WIN_TRIANGULAR = 2,  /* :98  */
  NXSIG_WIN_BLACKMAN = 3,    /* :160 */
  NXSIG_WIN_HAMMING = 4,     /* :225 */
  NXSIG_WIN_HANN = 5,        /* :278 */
  NXSIG_WIN_KAISER = 6       /* :341 */
} nxsig_window_kind;

/* Convolution modes — lib/nx_signal/convolution.ex:300-329 */
typedef enum nxsig_conv_mode { NXSIG_CONV_FULL = 0, NXSIG_CONV_SAME = 1, NXSIG_CONV_VALID = 2 } nxsig_conv_mode;

/* options of NxSignal.stft/3 (lib/nx_signal.ex:71-85) and istft/3 (:583) after default resolution */
typedef struct nxsig_stft_params {
  int32_t frame_length;  /* N = size of the window tensor (:69) */
  int32_t hop;           /* N - overlap_length (:99, :702) */
  int32_t fft_length;    /* K; :power_of_two already resolved by the caller (nxsig_next_pow2) */
  int32_t pad_mode;      /* nxsig_pad (stft only) */
  int64_t pad_lo, pad_hi;/* NXSIG_PAD_EXPLICIT only */
  int32_t scaling;       /* nxsig_scaling */
  int32_t reserved;
  double sampling_rate;  /* used by :psd scaling only */
} nxsig_stft_params;

/* ---------------------------------------------------------------- context / errors ---- */
int nxsig_abi_version(void);
int nxsig_device_count(int* count);
int nxsig_ctx_create(int device, nxsig_ctx** out);
void nxsig_ctx_destroy(nxsig_ctx* ctx);
/* Dispatch / geometry switches of ONE context ("Switches").  nxsig_ctx_create reads the NXSIG_<NAME> variables of
 * the process environment once; after that no call looks at the environment — a launch only reads the context's switches, and
 * these three functions change them at run time (A/B sweeps, tests).  `name` is "NXSIG_FOO" or "FOO"; unknown names are
 * NXSIG_ERR_INVALID_ARG.  clear(name = NULL) returns every switch to the launchers' defaults.  get alone also answers the read-only
 * name "TABLE_REQUESTS": how often this context was asked for a cached device table so far, modulo 2^31 (is_set = 0) — a call served
 * from a memo of table pointers asks for none, which is how the tests see that it formed nothing again. */
int nxsig_ctx_set_tuning(nxsig_ctx* ctx, const char* name, int32_t value);
int nxsig_ctx_get_tuning(nxsig_ctx* ctx, const char* name, int32_t* value, int32_t* is_set);
int nxsig_ctx_clear_tuning(nxsig_ctx* ctx, const char* name);
const char* nxsig_last_error(void); /* thread-local, valid until the next call on this thread */
/* Which kernel families did the calling thread's LAST compute call (stft / istft / fir / fft / convolve / mel ...) launch?  A
 * '+'-separated list in launch order, each family once, e.g. "stft.pair", "stft.pair.1r+stft.pair.edge", "istft.wave+istft.edge_chunks",
 * "fir.pair+fir.poison", "stft.generic".  The names are the kernel families of DESIGN.md section 3; a shape that silently falls from a tuned
 * kernel to the generic ones shows here (tests/test_gpu_dispatch_table.py pins the family of every documented shape).  Thread-local,
 * valid until the next compute call on this thread; "" before the first one.  Diagnostic only: nothing in the library reads it. */
const char* nxsig_last_dispatch(void);
/* the same record of the last compute call made on THIS CONTEXT by any thread, copied into buf (truncated to buflen - 1 characters): what a
 * host whose calls hop between threads (the BEAM's dirty schedulers) reads.
 * A GROUP MEMBER's context (nxsig_group_ctx): after a *_sharded call the record names the families the member's OWN part of that call ran
 * on — the record of the compute entry point the group called on it — and is "" for a member whose part was empty (more members than
 * rows).  The helper passes the group itself adds afterwards (the row poisoning of sample-sharded FIR, the clamp of the sharded log-mel)
 * are not noted.  The thread-local record after a *_sharded call is that of the last member the calling thread served: read the members'. */
int nxsig_ctx_last_dispatch(nxsig_ctx* ctx, char* buf, size_t buflen);
/* human readable device line ("AMD Instinct MI355X gfx950 256 CUs") into buf */
int nxsig_device_name(nxsig_ctx* ctx, char* buf, size_t buflen);

/* ---------------------------------------------------------------- memory / stream ----- */
/* Device memory of the context's GPU through a caching allocator: nxsig_free parks the block (no hipFree, no device
 * synchronisation) and a later nxsig_alloc of a similar size gets it back — a fresh 3.3 GB hipMalloc costs ~100 ms here, two
 * hundred times the stft that fills it.  Reuse is ordered by the context's stream; callers that touch a buffer on another
 * stream synchronise before freeing it.  The cache holds at most NXSIG_POOL_MAX_MB (default: a quarter of the device memory,
 * 0 = no caching) and is emptied when an allocation fails.  Blocks belong to their context and die with it.  nxsig_free also
 * accepts pointers from other HIP allocators (plain hipFree after the stream has drained). */
int nxsig_alloc(nxsig_ctx* ctx, size_t bytes, void** dptr);
int nxsig_free(nxsig_ctx* ctx, void* dptr);
int nxsig_upload(nxsig_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);   /* synchronous */
int nxsig_download(nxsig_ctx* ctx, void* dst_host, const void* src_device, size_t bytes); /* synchronous */
int nxsig_sync(nxsig_ctx* ctx);                       /* wait for everything enqueued on the ctx stream */
/* free / total memory of the context's GPU right now (hipMemGetInfo): bench.py's preflight reads the high-water mark off it */
int nxsig_mem_info(nxsig_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int nxsig_set_stream(nxsig_ctx* ctx, void* hip_stream); /* adopt a caller-owned hipStream_t (NULL = own stream) */
void* nxsig_get_stream(nxsig_ctx* ctx);
/* HIP-event stopwatch on the ctx stream (used by bench.py: events live on the stream the kernels run on) */
int nxsig_timer_start(nxsig_ctx* ctx);
int nxsig_timer_stop(nxsig_ctx* ctx, float* elapsed_ms); /* records + synchronises the stop event */

/* ---------------------------------------------------------------- shape helpers (pure) - */
int32_t nxsig_next_pow2(int32_t n); /* :power_of_two of Nx.fft */
/* number of frames of as_windowed — lib/nx_signal.ex:289-298; negative status on error */
int64_t nxsig_num_frames(int64_t length, int32_t frame_length, int32_t hop, int32_t pad_mode, int64_t pad_lo,
                         int64_t pad_hi);
/* output length of overlap_and_add / istft: M*hop + (N-hop) — lib/nx_signal.ex:703 */
int64_t nxsig_ola_length(int64_t num_frames, int32_t frame_length, int32_t hop);
/* output length of convolve for a mode — lib/nx_signal/convolution.ex:300-347 */
int64_t nxsig_conv_length(int64_t n1, int64_t n2, int32_t mode);
/* rows of nxsig_resample_poly: ceil(length * up / down) (the ratio need not be reduced); negative status when length < 0 or
 * up, down < 1 */
int64_t nxsig_resample_length(int64_t length, int32_t up, int32_t down);
/* outputs of one row a workgroup of the resample.poly.lds tier owns (the tile whose edges the tests straddle) */
int32_t nxsig_resample_tile(void);

/* ------------------------------------------ host-side generators (BinaryBackend rounding) */
/* NxSignal.Windows.* (n, is_periodic:, type: f32) — lib/nx_signal/windows.ex; beta/eps: kaiser only */
int nxsig_window_f32(int32_t kind, int32_t n, int32_t is_periodic, double beta, double eps, float* out);
/* NxSignal.Waveforms.sinc — lib/nx_signal/waveforms.ex:451-457 */
int nxsig_sinc_f32(const float* t, int64_t n, float* out);
/* NxSignal.Filters.firwin/3 — lib/nx_signal/filters.ex:147-279 (cutoff in sampling_rate units) */
int nxsig_firwin_f32(int32_t num_taps, const double* cutoff, int32_t n_cutoff, int32_t window_kind, double kaiser_beta,
                     int32_t pass_zero, int32_t scale, double sampling_rate, float* out);
/* NxSignal.fft_frequencies/2 — lib/nx_signal.ex:154-166 */
int nxsig_fft_frequencies_f32(double sampling_rate, int32_t fft_length, int32_t endpoint, float* out);
/* the `times` output of stft — lib/nx_signal.ex:108-111 */
int nxsig_stft_times_f32(int32_t frame_length, double sampling_rate, int64_t num_frames, float* out);

/* ---------------------------------------------------------------- the hot path -------- */
/*
 * NxSignal.stft/3 — lib/nx_signal.ex:68-130 (as_windowed :94-100, Nx.multiply :101, Nx.fft :102,
 * scaling :113-127) fused in one launch.
 *   x      f32[batch][length], rows `batch_stride` elements apart (batch = vectorized channels, B16)
 *   window f32[N] HOST
 *   z      c64[batch][M][K]
 *   M      = nxsig_num_frames(length, N, hop, pad...) written to *num_frames_out (may be NULL)
 */
int nxsig_stft_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                   const float* window, const nxsig_stft_params* params, nxsig_c64* z, int64_t* num_frames_out,
                   int32_t mem);

/*
 * NxSignal.stft/3 of COMPLEX samples (c64 IQ data) — lib/nx_signal.ex:94-102 frames, multiplies (:101, c64 x f32 componentwise) and
 * transforms (:102, one Nx.fft row per frame: no pair packing) whatever tensor it is given.  Same parameters and outputs as
 * nxsig_stft_f32 with x c64[batch][length] (interleaved re, im), rows `batch_stride` COMPLEX elements apart.
 */
int nxsig_stft_c64(nxsig_ctx* ctx, const nxsig_c64* x, int64_t length, int32_t batch, int64_t batch_stride,
                   const float* window, const nxsig_stft_params* params, nxsig_c64* z, int64_t* num_frames_out,
                   int32_t mem);

/*
 * NxSignal.istft/3 — lib/nx_signal.ex:582-638 (Nx.ifft :609, inverse scaling :611-625, x window and
 * overlap_and_add :627-628, OLA(|w|^2) normaliser with the 1e-10 guard :630-637).
 *   z c64[batch][M][K]  ->  y c64[batch][M*hop + N-hop]   (complex output)
 *   requires fft_length == frame_length (the reference's broadcast {M,K} x {N} requires it too).
 */
int nxsig_istft_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                    const nxsig_stft_params* params, nxsig_c64* y, int32_t mem);

/* NxSignal.as_windowed/2 — lib/nx_signal.ex:249-364: f32[batch][length] -> f32[batch][M][N] */
int nxsig_as_windowed_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                          int32_t window_length, int32_t stride, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi,
                          float* out, int64_t* num_frames_out, int32_t mem);

/* NxSignal.overlap_and_add/2 — lib/nx_signal.ex:684-736: [batch][M][N] -> [batch][M*hop + N-hop].
 * `components` = 1 for f32 tensors, 2 for c64 (interleaved); deterministic (fixed frame order). */
int nxsig_overlap_and_add(nxsig_ctx* ctx, const float* frames, int64_t num_frames, int32_t batch, int32_t frame_length,
                          int32_t overlap_length, int32_t components, float* out, int32_t mem);

/* Nx.fft / Nx.ifft(length: K) over the last axis as NxSignal.Transforms.fft_nd / ifft_nd reach them
 * (lib/nx_signal/transforms.ex:5-21): rows of n_in elements are zero-padded / truncated to K.
 * in: c64[rows][n_in] (in_is_real = 0) or f32[rows][n_in] (in_is_real = 1); out: c64[rows][K]. */
int nxsig_fft(nxsig_ctx* ctx, const void* in, int32_t in_is_real, int64_t rows, int32_t n_in, int32_t fft_length,
              int32_t inverse, nxsig_c64* out, int32_t mem);

/*
 * NxSignal.Transforms.fft_nd / ifft_nd — lib/nx_signal/transforms.ex:5-21: Enum.zip_reduce(axes, lengths, t, &Nx.fft(&3, axis: &1,
 * length: &2)) (or Nx.ifft), entirely in HBM: an axis other than the last is brought to the back by a tiled transpose kernel,
 * transformed by the row kernels and moved back.  in: f32 (in_is_real) or c64 tensor of `rank` <= 8 dims, row-major; out: c64 tensor
 * whose dims at `axes` are `lengths` (zero-pad / truncate like Nx.fft(length:)).  Row lengths: any power of two up to 2^26
 * (four-step beyond 8192), any other length up to 2^22 (Bluestein).  `out` must not alias `in`.
 */
int nxsig_fft_nd(nxsig_ctx* ctx, const void* in, int32_t in_is_real, const int64_t* shape, int32_t rank, const int32_t* axes,
                 const int64_t* lengths, int32_t n_axes, int32_t inverse, nxsig_c64* out, int32_t mem);

/*
 * n-D Convolution.fftconvolve/3 — lib/nx_signal/convolution.ex:252-347: fft_nd of both operands over the axes where neither
 * dimension is 1 (lengths s1 + s2 - 1), broadcast product, ifft_nd, Nx.real for real operands, `centered` slice per mode
 * (:valid needs one operand at least as large as the other in every dimension, :335-347).  a, b: tensors of equal rank <= 8
 * (f32 when *_is_real, else c64).  out: f32 when both are real, else c64; its shape is written to out_shape[rank] (may be
 * NULL): full s1 + s2 - 1, same s1, valid |s1 - s2| + 1.
 */
int nxsig_fftconvolve_nd(nxsig_ctx* ctx, const void* a, int32_t a_is_real, const int64_t* a_shape, const void* b, int32_t b_is_real,
                         const int64_t* b_shape, int32_t rank, int32_t mode, void* out, int64_t* out_shape, int32_t mem);

/*
 * Convolution.convolve/3 with `method: :direct` (the reference's DEFAULT method) — lib/nx_signal/convolution.ex:38-58, :95-218:
 * Nx.conv of in1, zero-padded per mode (:full k-1 on both sides; :same (k-1) - div(k-1, 2) left, div(k-1, 2) right; :valid none,
 * the larger operand becomes the volume, :120-135), with in2 reversed along every axis.  Time-domain sums, products accumulated
 * in double in the BinaryBackend's window order and rounded once: integer-valued inputs come out exact (the reference's tests
 * compare with ==).  O(output x kernel) work — meant for short kernels; long filters belong to nxsig_fir_f32 / the FFT method.
 * Same argument convention as nxsig_fftconvolve_nd; out shape: full s1 + s2 - 1, same s1, valid |s1 - s2| + 1.
 */
int nxsig_convolve_direct(nxsig_ctx* ctx, const void* a, int32_t a_is_real, const int64_t* a_shape, const void* b, int32_t b_is_real,
                          const int64_t* b_shape, int32_t rank, int32_t mode, void* out, int64_t* out_shape, int32_t mem);

/*
 * Filters.median/2 — lib/nx_signal/filters.ex:17-55: every output is the median of the window of kernel_shape that starts at
 * min(i_d, n_d - k_d) on every axis (Nx.slice clamps its start indices: no padding, outputs near the high edge reuse the last full
 * window).  x: f32, or f64 when is_f64 (integer tensors are converted to f64 by the caller); rank <= 8; 1 <= k_d <= n_d.  Values are
 * ordered like np.sort (NaN above +Inf, -0.0 == +0.0, a zero median comes out +0.0).  Odd windows: the middle value; even windows:
 * (a + b) / 2 of the two middle values in the input's type.  out: f32, the input's shape.  Dispatch: median.rows (window on the last
 * axis, k <= 31), median.plane (last two axes, k_h, k_w <= 7), median.generic (any window) — the same bits from every tier.
 */
int nxsig_median_filter(nxsig_ctx* ctx, const void* x, int32_t is_f64, const int64_t* shape, int32_t rank, const int64_t* kernel_shape,
                        float* out, int32_t mem);

/*
 * Filters.resample_poly: the last axis of real f32 (or c64 when is_complex) rows resampled by the rational factor up / down with a
 * polyphase FIR — scipy.signal.resample_poly(x, up, down, window: h / up, padtype: "constant").  The reference has no resampler.
 * Definition: the ratio is reduced first (g = gcd(up, down), up /= g, down /= g); a row of n = length samples gives
 * n_out = nxsig_resample_length(n, up, down) = ceil(n up / down) outputs; with the taps h[0 .. L), real, GAIN INCLUDED (scipy's
 * up * window), and half = (L - 1) / 2,
 *     y[m] = sum_j x[j] h[m down + half - j up]      over every j in [0, n) whose tap index lies in [0, L), and nothing else
 * — with c = m down + half, q = c div up, r = c mod up:  y[m] = sum_{t >= 0} x[q - t] h[r + t up], one polyphase branch r of at
 * most T = ceil(L / up) taps per output, accumulated from +0.0 by one fmaf per term in ascending t (c64: each component on its
 * own).  Samples outside the row and taps outside [0, L) are never multiplied in: an Inf / NaN reaches exactly the outputs whose
 * branch covers it, and no other row (this is NOT nxsig_fir_f32's whole-row rule).  up == down after reduction: y is a copy of x,
 * no filter applied (dispatch resample.copy).
 *   x [batch][length] rows batch_stride >= length elements apart, h f32[num_taps] HOST, y [batch][n_out] dense.
 * Dispatch: resample.poly.lds while the phase table up x T floats is at most 64 KiB (and it fits the LDS next to a tile's input
 * span), resample.poly.generic otherwise and under NXSIG_DISABLE_RESAMPLE_LDS — the same bits from both.  NXSIG_ERR_UNSUPPORTED:
 * 2^31 or more tiles in one call.
 */
int nxsig_resample_poly(nxsig_ctx* ctx, const void* x, int32_t is_complex, int64_t length, int32_t batch, int64_t batch_stride,
                        const float* h, int32_t num_taps, int32_t up, int32_t down, void* y, int32_t mem);

/*
 * Filters.wiener/2 — lib/nx_signal/filters.ex:81-110, :281-303, computed in f64: S1 / S2 = correlate(t, ones(kernel_size)) and
 * correlate(t^2, ...) with mode :same (zero padding (k-1) - div(k-1, 2) low, div(k-1, 2) high), each accumulated from 0.0 over the window
 * in row-major order; l_mean = S1 / size, l_var = S2 / size - l_mean^2; noise = has_noise ? noise : mean(l_var);
 * out = l_var < noise ? l_mean : (t - l_mean) * (1 - noise / l_var) + l_mean, rounded to the input's type.  x, out: f32, or f64 when
 * is_f64; rank <= 8; kernel_size[rank] >= 1.  noise_used (may be NULL): the noise the formula used (the estimate when !has_noise; the
 * call then waits for the device).  The estimate's sum runs in a fixed order: the result is the same from run to run.
 */
int nxsig_wiener(nxsig_ctx* ctx, const void* x, int32_t is_f64, const int64_t* shape, int32_t rank, const int64_t* kernel_size, int32_t has_noise,
                 double noise, void* out, double* noise_used, int32_t mem);

/* element types of nxsig_argrelextrema (narrower integers and bool are widened to s32, f16 to f32, by the caller) */
typedef enum nxsig_dtype {
  NXSIG_DT_F32 = 0, NXSIG_DT_F64 = 1, NXSIG_DT_S32 = 2, NXSIG_DT_S64 = 3, NXSIG_DT_U32 = 4, NXSIG_DT_U64 = 5
} nxsig_dtype;

/* the comparators of PeakFinding.argrelextrema/3 that run fused: Nx.less/2, greater/2, less_equal/2, greater_equal/2 */
typedef enum nxsig_comparator {
  NXSIG_CMP_LESS = 0, NXSIG_CMP_GREATER = 1, NXSIG_CMP_LESS_EQUAL = 2, NXSIG_CMP_GREATER_EQUAL = 3
} nxsig_comparator;

/*
 * PeakFinding.argrelextrema/3 — lib/nx_signal/peak_finding.ex (argrelmin/2 = NXSIG_CMP_LESS, argrelmax/2 = NXSIG_CMP_GREATER):
 * x[i] is marked when cmp(x[i], x[clip(i + s, 0, n - 1)]) and cmp(x[i], x[clip(i - s, 0, n - 1)]) hold for s = 1 .. shifts along
 * `axis` (n its length; shifts = max(0, ceil(order)), so 0 marks every element).  Plain IEEE compares in the input's type: NaN
 * compares false, -0.0 == +0.0, integers exactly.  x: dtype (nxsig_dtype) of prod(shape) elements; rank 1 .. 8, no empty dimension,
 * fewer than 2^32 elements, every dimension below 2^31.  indices: s32 [size][rank], the coordinates of the marked elements in
 * row-major order of their flat index (np.argwhere's order), then -1 rows; *valid: their count (u32; on the device when mem is
 * NXSIG_DEVICE, and the call then returns without waiting).  The same bits from run to run and from every dispatch family:
 * peaks.rows (axis is the last one), peaks.strided (any other axis), peaks.generic (NXSIG_DISABLE_PEAK_TILES).
 */
int nxsig_argrelextrema(nxsig_ctx* ctx, const void* x, int32_t dtype, const int64_t* shape, int32_t rank, int32_t axis, int64_t shifts,
                        int32_t comparator, int32_t* indices, uint32_t* valid, int32_t mem);

/*
 * The nonzero step of PeakFinding.argrelextrema/3 for a mask built elsewhere (a custom comparator): the coordinates of the
 * non-zero bytes of mask (u8, prod(shape) elements) in row-major order, then -1 rows, as nxsig_argrelextrema writes them
 * (dispatch family nonzero).  The same limits on shape and rank.
 */
int nxsig_nonzero(nxsig_ctx* ctx, const uint8_t* mask, const int64_t* shape, int32_t rank, int32_t* indices, uint32_t* valid, int32_t mem);

/*
 * NxSignal.Waveforms — lib/nx_signal/waveforms.ex.  t: n elements, f32, or f64 when is_f64; the results have
 * t's type unless stated.  f32: every Nx op is evaluated in double on f32 operands and rounded to f32 (the reference's literals come
 * out bit for bit); f64: the same expressions unrounded.  pi() is the f32 constant in both.  mem: NXSIG_HOST or NXSIG_DEVICE for every
 * tensor pointer; device calls return without waiting; n == 0 returns NXSIG_OK and launches nothing.  A device pointer needs only the
 * alignment of its element type.  Dispatch families: waveform.<function> (waveform.chirp.<method>).
 */

/* sawtooth/2 — waveforms.ex:29-54: tmod = fmod(t, 2 pi()); width == 1: tmod / (pi() width) - 1; width == 0: the falling ramp;
 * otherwise a select on tmod < 2 pi() width.  width outside [0, 1] (or NaN): NXSIG_ERR_INVALID_ARG (:34-36). */
int nxsig_sawtooth(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double width, void* out, int32_t mem);

/* square/2 — waveforms.ex:96-104: fmod(t, 2 pi()) < duty * 2 * pi() ? 1 : -1 as s32.  duty_tensor (n elements of t's type, same mem)
 * replaces the scalar duty when it is not NULL. */
int nxsig_square(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double duty, const void* duty_tensor, int32_t* out, int32_t mem);

/* gaussian_pulse/2 — waveforms.ex:161-198: envelope = exp(-a t^2), in_phase = envelope cos(2 pi() fc t), quadrature = envelope
 * sin(2 pi() fc t), a = -(pi fc bw)^2 / (4 log(10^(bwr / 20))); one pass writes the three outputs, which must not overlap.
 * fc < 0, bw <= 0, bwr >= 0: NXSIG_ERR_INVALID_ARG (:173-186). */
int nxsig_gaussian_pulse(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double center_frequency, double bandwidth,
                         double bandwidth_reference_level, void* envelope, void* in_phase, void* quadrature, int32_t mem);

/* the :method of chirp/5 */
typedef enum nxsig_chirp_method {
  NXSIG_CHIRP_LINEAR = 0, NXSIG_CHIRP_QUADRATIC = 1, NXSIG_CHIRP_LOGARITHMIC = 2, NXSIG_CHIRP_HYPERBOLIC = 3
} nxsig_chirp_method;

/* chirp/5 — waveforms.ex:249-289: cos(phase + phi), phase by method (:254-285; vertex_zero only matters to NXSIG_CHIRP_QUADRATIC).
 * :logarithmic with f0 f1 <= 0 gives NaN everywhere, f0 == f1 of :logarithmic / :hyperbolic is 2 pi() f0 t.  An unknown method:
 * NXSIG_ERR_INVALID_ARG (:291-300). */
int nxsig_chirp(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, double f0, double t1, double f1, int32_t method, int32_t vertex_zero,
                double phi, void* out, int32_t mem);

#define NXSIG_SWEEP_MAX_COEFS 32
/* polynomial_sweep/3 — waveforms.ex:343-361: cos(2 pi() sum_k (coefs[k] / (n - k)) t^(n - k) + phi), coefs (host, ncoefs in
 * [1, NXSIG_SWEEP_MAX_COEFS]) from the highest power down, the sum in f64 rounded once; phi in degrees when phi_degrees (:354-358). */
int nxsig_polynomial_sweep(nxsig_ctx* ctx, const void* t, int32_t is_f64, int64_t n, const double* coefs, int32_t ncoefs, double phi,
                           int32_t phi_degrees, void* out, int32_t mem);

/* unit_impulse/2 — waveforms.ex:406-437: prod(shape) zeros of dtype (nxsig_dtype) and a single one at index (rank entries, host; the
 * caller resolves :midpoint and a scalar index); rank 0 .. 8.  An empty dimension gives NXSIG_OK and writes nothing.  An index
 * outside the shape is NXSIG_ERR_INVALID_ARG (a deliberate deviation: what Nx.indexed_put does with it is not specified here). */
int nxsig_unit_impulse(nxsig_ctx* ctx, int32_t dtype, const int64_t* shape, int32_t rank, const int64_t* index, void* out, int32_t mem);

/*
 * FIR filtering: y = Convolution.convolve(x, h, method: :fft, mode:) for real 1-D x (per batch row) and
 * real taps h — lib/nx_signal/convolution.ex:252-329 as used by guides/filtering.livemd:126-128 —
 * computed by overlap-save block FFT convolution (the `Filters.fir` of BASELINE config 5; the reference
 * does one length-(L+K-1) FFT, results agree to fp32 rounding).  Filters of any length: up to 1025 taps the tuned wave kernels,
 * up to 4096 taps the generic overlap-save kernel, beyond that (impulse responses of seconds) one transform of
 * next_pow2(length + num_taps - 1) <= 2^26 points per row like the reference.
 *   x f32[batch][length], h f32[num_taps] HOST, y f32[batch][nxsig_conv_length(length, num_taps, mode)]
 */
int nxsig_fir_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* h,
                  int32_t num_taps, int32_t mode, float* y, int32_t mem);

/* Any slice [out_start, out_start + out_len) of the FULL convolution of every row with h (the modes of nxsig_fir_f32 are
 * three such slices; sharded filtering asks for the slice a rank owns): y f32[batch][out_len].
 * Non-finite samples: the reference filters a row by ONE transform (convolution.ex:276-284), so a row that holds an Inf / NaN has no
 * finite output, and nxsig_fir_f32 returns such a row as NaN from end to end.  A SLICE call only looks at the blocks its outputs
 * need: it returns NaN for the whole slice when one of THOSE samples is not finite, and finite values when the non-finite sample
 * lies elsewhere in the row — so the slices of a row assembled BY THE CALLER can be finite where the unsliced call is NaN
 * (nxsig_fir_sharded_f32 on the samples axis closes that itself: its members exchange one flag per row).  Callers that need the reference's whole-row behaviour for sliced rows test the row
 * themselves; finite rows are unaffected. */
int nxsig_fir_slice_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* h,
                        int32_t num_taps, int64_t out_start, int64_t out_len, float* y, int32_t mem);

/*
 * NxSignal.mel_filters/4 — lib/nx_signal.ex:397-445 (Slaney-style filterbank, host-side with BinaryBackend rounding):
 * out f32[mel_bins][fft_length].  Defaults of the reference: max_mel 3016, mel_frequency_spacing 200/3.
 */
int nxsig_mel_filters_f32(int32_t fft_length, int32_t mel_bins, double sampling_rate, double max_mel,
                          double mel_frequency_spacing, float* out);

/*
 * NxSignal.stft_to_mel/3 — lib/nx_signal.ex:486-513: |z|^2 of the first fft_length/2 bins x filterbank
 * -> log10(max(., 1e-10)) -> max(., global max - 8) -> (. + 4) / 4.   z c64[rows][fft_length] (rows = every frame of
 * every batch element: the reference's reduce_max runs over the whole tensor) -> out f32[rows][mel_bins].
 * `filters` f32[mel_bins][fft_length] is a HOST table (nxsig_mel_filters_f32 or user supplied).
 */
int nxsig_stft_to_mel(nxsig_ctx* ctx, const nxsig_c64* z, int64_t rows, int32_t fft_length, int32_t mel_bins,
                      const float* filters, float* out, int32_t mem);

/*
 * Fused NxSignal.stft/3 -> NxSignal.stft_to_mel/3: the log-mel spectrogram of x without ever writing the
 * complex spectrum to HBM (mel_bins * 4 B/frame leave the chip instead of fft_length * 8).  Same result as
 * nxsig_stft_f32 followed by nxsig_stft_to_mel, to fp32 rounding.  x f32[batch][length] -> out f32[batch][M][mel_bins];
 * the global maximum runs over the whole output.  Shapes the fused kernel does not cover run the two-step path.
 */
int nxsig_stft_mel_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                       const float* window, const nxsig_stft_params* params, int32_t mel_bins, const float* filters,
                       float* out, int64_t* num_frames_out, int32_t mem);

/*
 * One-sided complex spectrum (opt-in; not in the reference API): the bins 0 .. fft_length/2 - 1 of NxSignal.stft/3 —
 * the slice the reference's own downstream code keeps for real signals (stft_to_mel: lib/nx_signal.ex:493-496; the spectrogram
 * guide: guides/spectrogram.livemd:80-82) — written straight from the transform: 4 KB per frame instead of 8 at fft_length 1024,
 * identical bits to the first half of nxsig_stft_f32's rows.  out c64[batch][M][fft_length / 2].
 */
int nxsig_stft_onesided_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                            const nxsig_stft_params* params, nxsig_c64* out, int64_t* num_frames_out, int32_t mem);

/*
 * The PACKED one-sided pair (opt-in; not in the reference API): the reference's STFT-domain filtering chain
 * stft -> z * H -> istft (guides/filtering.livemd:137-159) moves the full two-sided spectrum, 8 KB + 2 KB of HBM traffic per
 * frame at fft_length 1024, although for a real signal half of z mirrors the other half and the imaginary part of the istft
 * result is round-off (callers take Nx.real / Nx.as_type, lib/nx_signal.ex:550).  The packed pair keeps what is independent:
 *   nxsig_stft_packed_f32    out c64[batch][M][fft_length / 2]: bins 0 .. fft_length/2 - 1 exactly as nxsig_stft_onesided_f32
 *                            writes them, except that the imaginary part of bin 0 (zero for a real frame) carries
 *                            Re X[fft_length / 2], the Nyquist bin (real for a real frame) — nothing of a real frame's
 *                            spectrum is lost.  fft_length even.  4 KB per frame.
 *   nxsig_istft_packed_f32   the inverse of exactly that layout (a pointwise product z * H of two packed tensors must treat
 *                            bin 0 as the two reals it is): y REAL f32[batch][M * hop + frame_length - hop], equal to the real part
 *                            of nxsig_istft_c64 on the full Hermitian spectrum to fp32 round-off.  1 KB per frame.
 * frame_length == fft_length as for istft; fused kernel for 1024 / hop 128 ... 1024, other shapes go through the full layout.
 */
int nxsig_stft_packed_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                          const nxsig_stft_params* params, nxsig_c64* out, int64_t* num_frames_out, int32_t mem);
int nxsig_istft_packed_f32(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                           const nxsig_stft_params* params, float* y, int32_t mem);

/*
 * Magnitude spectrogram fused with the STFT (opt-in, not in the reference API): what
 * guides/spectrogram.livemd:76-92 computes from NxSignal.stft/3 — Nx.abs(s) of the bins below fft_length / 2, optionally
 * as dBFS 20 * log(|s| / reduce_max|s|) / log(10) — without writing the complex spectrum to HBM: fft_length * 2 bytes per
 * frame leave the chip instead of fft_length * 8.   x f32[batch][length] -> out f32[batch][M][fft_length / 2].
 * kind: NXSIG_MAG_ABS |s|, NXSIG_MAG_POWER |s|^2, NXSIG_MAG_DBFS (the maximum runs over the whole output).
 */
#define NXSIG_MAG_ABS 0
#define NXSIG_MAG_POWER 1
#define NXSIG_MAG_DBFS 2
int nxsig_stft_magnitude_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride,
                             const float* window, const nxsig_stft_params* params, int32_t kind, float* out,
                             int64_t* num_frames_out, int32_t mem);

/*
 * STFT-domain filtering kept on the device: the `Nx.multiply(z, hfft)` step of the reference's documented
 * workflow stft -> z * H -> istft (guides/filtering.livemd:137-159).  out[r][k] = z[r][k] * h[k], each component
 * computed in double and rounded once like Nx.BinaryBackend's complex multiply.  z, out c64[rows][fft_length] (out may
 * alias z); `h` c64[fft_length] is a HOST table (the DFT of the filter, e.g. from nxsig_fft).
 */
int nxsig_spectrum_mul_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t rows, int32_t fft_length, const nxsig_c64* h,
                           nxsig_c64* out, int32_t mem);

/*
 * The last two steps of that workflow in one call: NxSignal.istft(Nx.multiply(z, hfft), window, opts)
 * (guides/filtering.livemd:141 + :150-157).  Same result, bit for bit, as nxsig_spectrum_mul_c64 followed by nxsig_istft_c64
 * (the product is formed in double and rounded to c64 before the inverse transform sees it), but for N = 1024 the filter
 * values ride in the registers of the inverse-STFT kernel and the filtered spectrogram is never written to or re-read from
 * HBM (26 KB of traffic per frame -> 10 at hop 256).  Other sizes run the two steps behind this entry.  z is not modified.
 *   z c64[batch][M][K], h c64[K] HOST  ->  y c64[batch][M*hop + N-hop]
 */
int nxsig_istft_filtered_c64(nxsig_ctx* ctx, const nxsig_c64* z, int64_t num_frames, int32_t batch, const float* window,
                             const nxsig_stft_params* params, const nxsig_c64* h, nxsig_c64* y, int32_t mem);

/*
 * Time-frequency masks (denoising, source separation, spectral gating): a mask that differs from frame to frame, unlike the
 * filter `h` above.  The layout of one mask row (one frame):
 *   NXSIG_MASK_REAL      f32[K]        real gain per bin
 *   NXSIG_MASK_ONESIDED  f32[K/2 + 1]  real gain of bins 0 .. K/2; bin k > K/2 takes mask[K - k] (K even)
 *   NXSIG_MASK_COMPLEX   c64[K]
 * A real gain multiplies each component on its own, (float)((double)z.c * (double)m); a complex one is the product of
 * nxsig_spectrum_mul_c64.  z has z_rows rows of [num_frames][K], the mask mask_rows rows of [num_frames][row length]: the two
 * counts are equal, or one of them is 1 and that operand is read again for every row of the other (one mixture and S masks:
 * z_rows == 1, mask_rows == S).  The result has max(z_rows, mask_rows) rows, at most 65 535 (the limit of the filtered form).
 * `mem` covers z, the mask and the result alike.
 */
typedef enum nxsig_mask_kind { NXSIG_MASK_REAL = 0, NXSIG_MASK_ONESIDED = 1, NXSIG_MASK_COMPLEX = 2 } nxsig_mask_kind;

/* out[r][m][k] = z[r or 0][m][k] * mask[r or 0][m][k]: c64[max(z_rows, mask_rows)][num_frames][fft_length].  out must not
 * alias z or the mask when one of them is broadcast. */
int nxsig_spectrum_mask_c64(nxsig_ctx* ctx, const nxsig_c64* z, int32_t z_rows, const void* mask, int32_t mask_kind,
                            int32_t mask_rows, int64_t num_frames, int32_t fft_length, nxsig_c64* out, int32_t mem);

/*
 * NxSignal.istft(Nx.multiply(z, mask), window, opts) in one call: the same bits as nxsig_spectrum_mask_c64 followed by
 * nxsig_istft_c64.  For N = fft_length = 1024 and hop 128 / 256 / 512 / 1024 every frame's mask row streams into the inverse
 * kernel next to its spectrum and the masked spectrogram never exists in HBM (30 KB of traffic per frame -> 14 with a full real
 * mask, 12 with a one-sided one, at hop 256); other geometries run the two steps behind this entry.  z and the mask are not
 * modified.  y c64[max(z_rows, mask_rows)][M*hop + N-hop].
 */
int nxsig_istft_masked_c64(nxsig_ctx* ctx, const nxsig_c64* z, int32_t z_rows, int64_t num_frames, const float* window,
                           const nxsig_stft_params* params, const void* mask, int32_t mask_kind, int32_t mask_rows,
                           nxsig_c64* y, int32_t mem);

/*
 * 1-D complex case of Convolution.fftconvolve/3 — lib/nx_signal/convolution.ex:252-329 (tests: "FFT complex",
 * test/nx_signal/convolutions_test.exs:473-487): out = ifft(fft(a, P) * fft(b, P)) sliced per mode, with
 * P = next power of two >= n1 + n2 - 1 (same linear convolution as the reference's length n1 + n2 - 1).
 *   a c64[n1], b c64[n2], out c64[nxsig_conv_length(n1, n2, mode)]; n1 + n2 - 1 <= 2^26 (four-step transforms beyond 8192 points).
 */
int nxsig_fftconvolve_c64(nxsig_ctx* ctx, const nxsig_c64* a, int64_t n1, const nxsig_c64* b, int64_t n2, int32_t mode,
                          nxsig_c64* out, int32_t mem);

/* ---------------------------------------------------------------- f64 / c128 tier --------
 * The reference computes in the type of its operands: f64 samples or an f64 window promote the product of lib/nx_signal.ex:101
 * to f64 and Nx.fft returns c128 (:102); a c128 spectrum is inverted in c128 (:609); Windows.* / firwin / fft_frequencies take
 * `type: {:f, 64}` (lib/nx_signal/windows.ex:58, :99 ..., filters.ex:154, nx_signal.ex:155).  These entry points are that
 * tier: the argument conventions of their f32 namesakes with double / nxsig_c128 payloads, double arithmetic on the device
 * (workgroup-per-frame kernels, kernels_f64.hip — the tuned wave kernels stay the f32 path).  Limits: fft_length a power of two
 * <= 8192, any other length <= 4096 (Bluestein) or <= 65536 with at most 8192 samples per row (table DFT); FIR up to 4097 taps.
 * NXSIG_ERR_UNSUPPORTED beyond.  `window` is f64[N] when window_is_f64, else f32[N]: the reference forms the :scaling
 * scalar and the |w|^2 normaliser in the window's OWN type before promoting (Nx.sum(window) :116, :614; :630-633).
 */
/* NxSignal.Windows.*(n, type: {:f, 64}) — lib/nx_signal/windows.ex: every op of the f32 generator rounded to double instead */
int nxsig_window_f64(int32_t kind, int32_t n, int32_t is_periodic, double beta, double eps, double* out);
/* NxSignal.Waveforms.sinc on an f64 tensor — lib/nx_signal/waveforms.ex:451-457 (its pi() stays the f32 constant) */
int nxsig_sinc_f64(const double* t, int64_t n, double* out);
/* NxSignal.Filters.firwin(..., type: {:f, 64}) — lib/nx_signal/filters.ex:147-279 */
int nxsig_firwin_f64(int32_t num_taps, const double* cutoff, int32_t n_cutoff, int32_t window_kind, double kaiser_beta,
                     int32_t pass_zero, int32_t scale, double sampling_rate, double* out);
/* NxSignal.fft_frequencies(fs, type: {:f, 64}) — lib/nx_signal.ex:154-166 */
int nxsig_fft_frequencies_f64(double sampling_rate, int32_t fft_length, int32_t endpoint, double* out);
/* NxSignal.stft/3 on f64 samples — lib/nx_signal.ex:68-130: x f64[batch][length] -> z c128[batch][M][K] */
int nxsig_stft_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const void* window,
                   int32_t window_is_f64, const nxsig_stft_params* params, nxsig_c128* z, int64_t* num_frames_out, int32_t mem);
/* NxSignal.stft/3 on COMPLEX f64 samples (c128 IQ data) — lib/nx_signal.ex:94-102 on whatever tensor it is given: frames, c128 x window
 * componentwise (:101), one Nx.fft row per frame (:102).  x c128[batch][length], rows `batch_stride` COMPLEX elements apart; the other
 * arguments as nxsig_stft_f64 */
int nxsig_stft_c128(nxsig_ctx* ctx, const nxsig_c128* x, int64_t length, int32_t batch, int64_t batch_stride, const void* window,
                    int32_t window_is_f64, const nxsig_stft_params* params, nxsig_c128* z, int64_t* num_frames_out, int32_t mem);
/* NxSignal.istft/3 on a c128 spectrum — lib/nx_signal.ex:582-638: z c128[batch][M][K] -> y c128[batch][M*hop + N-hop] */
int nxsig_istft_c128(nxsig_ctx* ctx, const nxsig_c128* z, int64_t num_frames, int32_t batch, const void* window, int32_t window_is_f64,
                     const nxsig_stft_params* params, nxsig_c128* y, int32_t mem);
/* Nx.fft / Nx.ifft(length: K) over rows in c128 — lib/nx_signal/transforms.ex:5-21: in f64 (in_is_real) or c128 */
int nxsig_fft_c128(nxsig_ctx* ctx, const void* in, int32_t in_is_real, int64_t rows, int32_t n_in, int32_t fft_length, int32_t inverse,
                   nxsig_c128* out, int32_t mem);
/* NxSignal.as_windowed/2 of an f64 tensor — lib/nx_signal.ex:249-364 */
int nxsig_as_windowed_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, int32_t window_length,
                          int32_t stride, int32_t pad_mode, int64_t pad_lo, int64_t pad_hi, double* out, int64_t* num_frames_out,
                          int32_t mem);
/* NxSignal.overlap_and_add/2 of an f64 (components = 1) or c128 (2) tensor — lib/nx_signal.ex:684-736 */
int nxsig_overlap_and_add_f64(nxsig_ctx* ctx, const double* frames, int64_t num_frames, int32_t batch, int32_t frame_length,
                              int32_t overlap_length, int32_t components, double* out, int32_t mem);
/* Convolution.convolve(x, h, method: :fft, mode:) of f64 rows with f64 taps — lib/nx_signal/convolution.ex:252-329 */
int nxsig_fir_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const double* h,
                  int32_t num_taps, int32_t mode, double* y, int32_t mem);
int nxsig_fir_slice_f64(nxsig_ctx* ctx, const double* x, int64_t length, int32_t batch, int64_t batch_stride, const double* h,
                        int32_t num_taps, int64_t out_start, int64_t out_len, double* y, int32_t mem);

/* ============================================================== multi-GPU groups ====
 * The path shards with NO data-path exchange: channels (the reference's vectorized axes,
 * lib/nx_signal.ex:358-363) are independent and frames are independent given their samples, so rank r owns a
 * contiguous block of channels, or a contiguous frame range of one long stream plus an (N - hop)-sample input halo it
 * reads redundantly.  The only collective is the OPTIONAL final assembly: an RCCL all-gather over xGMI of the output
 * shards.  A group is either
 *   - LOCAL: one process drives every GPU of the node (the Elixir / dirty-NIF host): one nxsig_ctx + stream per device,
 *     communicators from ncclCommInitAll, collectives fused with ncclGroupStart / ncclGroupEnd; or
 *   - RANKED: one process per GPU (bench.py under a process launcher): ncclCommInitRank, the 128-byte ncclUniqueId
 *     travelling from rank 0 through a file on the node (nxsig_rendezvous_*).
 * librccl is dlopen()ed when the first group is created; a process that never creates a group never loads it.
 * Members that share one device (testing / replicas on a single GPU) get no communicator: their assembly runs as
 * device-to-device copies (LOCAL groups only).
 */
typedef struct nxsig_group nxsig_group;

typedef enum nxsig_shard_axis {
  NXSIG_SHARD_CHANNELS = 0, /* batch rows split into contiguous blocks (BASELINE configs 4 / 5) */
  NXSIG_SHARD_FRAMES = 1    /* frame ranges of each row, input halo read redundantly (one long stream) */
} nxsig_shard_axis;

/* contiguous near-equal split of range(total): the first total % parts members get one extra item (pure) */
int nxsig_shard_range(int64_t total, int32_t parts, int32_t index, int64_t* begin, int64_t* end);
/* frame range [m0, m1) of member `index` of a :valid-framed stream of `num_frames` frames and the sample span
 * [s0, s1) it reads: s0 = m0 * hop, s1 = (m1 - 1) * hop + frame_length (pure) */
int nxsig_shard_frames(int64_t num_frames, int32_t frame_length, int32_t hop, int32_t parts, int32_t index, int64_t* m0,
                       int64_t* m1, int64_t* s0, int64_t* s1);
/* output range [n0, n1) of member `index` of a FIR whose full-convolution slice starts at `out_start` (mode offset) and
 * the input span [s0, s1), clamped to [0, length), it reads: num_taps - 1 samples of halo (pure) */
int nxsig_shard_fir(int64_t length, int32_t num_taps, int32_t mode, int32_t parts, int32_t index, int64_t* n0, int64_t* n1,
                    int64_t* s0, int64_t* s1);

/* iSTFT over frame ranges: member `index` keeps output samples [n0, n1) = [m0 hop, m1 hop) of its frame share (the last member
 * also the tail up to M hop + N - hop) and needs input frames [f0, f1) = [m0 - (ceil(N / hop) - 1), m1) widened to multiples of
 * 8 frames (the kernels' frame groups): the halo FRAMES are recomputed instead of exchanging partial overlap-add sums (pure) */
int nxsig_shard_istft(int64_t num_frames, int32_t frame_length, int32_t hop, int32_t parts, int32_t index, int64_t* f0, int64_t* f1,
                      int64_t* n0, int64_t* n1);

/* file rendezvous on one node (pure host code): publish writes `bytes` bytes atomically (tmp file + rename), fetch polls
 * until the file exists, is complete and is younger than `max_age_s` seconds (stale files of earlier runs are ignored) */
int nxsig_rendezvous_publish(const char* path, const void* data, size_t bytes);
int nxsig_rendezvous_fetch(const char* path, void* data, size_t bytes, int32_t timeout_ms, int32_t max_age_s);

/* LOCAL group over `n` devices of this process (device_ids NULL = 0 .. n-1) */
int nxsig_group_create_local(int32_t n, const int32_t* device_ids, nxsig_group** out);
/* RANKED group: this process is rank `rank` of `world` and drives `device`.  Rank 0 creates the ncclUniqueId and
 * publishes it at `rendezvous_path`, the other ranks fetch it there (timeout_ms); world == 1 needs no path. */
int nxsig_group_create_rank(int32_t world, int32_t rank, int32_t device, const char* rendezvous_path, int32_t timeout_ms,
                            nxsig_group** out);
void nxsig_group_destroy(nxsig_group* g);
int32_t nxsig_group_world(const nxsig_group* g);        /* ranks in the group */
int32_t nxsig_group_local_count(const nxsig_group* g);  /* members driven by this process */
int32_t nxsig_group_rank(const nxsig_group* g, int32_t local_index);   /* global rank of a local member */
nxsig_ctx* nxsig_group_ctx(nxsig_group* g, int32_t local_index);       /* its context (owned by the group) */
int32_t nxsig_group_has_rccl(const nxsig_group* g);     /* 1 when the members hold RCCL communicators */
/* The RCCL library the groups of this process dlopen()ed (group.cpp looks for NXSIG_RCCL_LIB, librccl.so.1, /opt/rocm/lib/librccl.so.1,
 * librccl.so in that order — a process that imported torch finds torch's bundled copy first): *version = ncclGetVersion's code
 * (e.g. 22606 = 2.26.6; 0: no library / no such symbol), path_buf = the shared object's path.  Loads the library if nobody has yet. */
int nxsig_rccl_info(int32_t* version, char* path_buf, size_t buflen);
/* waits for every local stream, then (RCCL) all-reduces one word across the group and waits again */
int nxsig_group_barrier(nxsig_group* g);
/* element-wise reduction of `n` (<= 64) host doubles over the PROCESSES of the group; op 0 = max, 1 = sum */
int nxsig_group_allreduce_f64(nxsig_group* g, double* values, int32_t n, int32_t op);
/*
 * Final assembly of sharded device buffers: member r contributes `counts[r]` bytes (counts has nxsig_group_world
 * entries and is the same on every member).  For each local member i: send[i] = its shard (device), recv[i] = a device
 * buffer of sum(counts) bytes receiving the shards in rank order; send[i] may point into recv[i] at its own offset (in
 * place).  RCCL: one ncclBroadcast per rank inside ncclGroupStart / End (ncclAllGather when all counts are equal), on the
 * members' streams; asynchronous.  Members sharing a device: device-to-device copies.
 */
int nxsig_group_allgather(nxsig_group* g, const void* const* send, const int64_t* counts, void* const* recv);

/*
 * NxSignal.stft/3 sharded over the group (window_padding must be :valid — padding belongs to the stream ends).
 *   mem == NXSIG_HOST  : x[0] is the whole host tensor f32[batch][length], z[0] the whole host result c64[batch][M][K];
 *                        every local member uploads its part, computes it, and the result is assembled either by per-shard
 *                        downloads (gather == 0) or by the RCCL all-gather followed by one download (gather == 1).
 *                        RANKED groups (one process per GPU): every process passes the whole tensor and a full-size result;
 *                        gather == 0 writes only the process' own part of it, gather == 1 the whole result in every process.
 *   mem == NXSIG_DEVICE: x[i] is local member i's INPUT SHARD on its own device — rows [c0, c1) of the tensor
 *                        (channels axis: f32[c1 - c0][length], rows batch_stride apart) or the sample span [s0, s1) of
 *                        every row (frames axis: f32[batch][s1 - s0]).  batch_stride == 0 means DENSE per-member shards
 *                        (row stride = the member's own row length) and is what frame shards should pass: their spans
 *                        differ from member to member whenever the frame count does not divide evenly, so one stride
 *                        cannot describe them; a non-zero batch_stride applies to every member and must be at least
 *                        the member's row length (NXSIG_ERR_INVALID_ARG otherwise).  gather == 0: z[i] receives
 *                        the member's output shard (c64[c1 - c0][M][K] / c64[batch][m1 - m0][K]) and stays on its device.
 *                        gather == 1: z[i] is a full c64[batch][M][K] buffer on every member's device; shards are
 *                        computed in place and all-gathered (frames axis: batch must be 1).  Asynchronous.
 * `length`, `batch` always describe the WHOLE tensor; ranges come from nxsig_shard_range / nxsig_shard_frames.
 */
int nxsig_stft_sharded_f32(nxsig_group* g, const float* const* x, int64_t length, int32_t batch, int64_t batch_stride,
                           const float* window, const nxsig_stft_params* params, int32_t axis, int32_t gather,
                           nxsig_c64* const* z, int32_t mem);
/* NxSignal.istft/3 (nxsig_istft_c64) sharded over the group; same conventions.  Channels axis: rows of z c64[batch][M][K] split.
 * Frames axis: output sample ranges with halo frames (nxsig_shard_istft); DEVICE shards are dense c64[batch][f1 - f0][K] and
 * c64[batch][n1 - n0].  The result equals the unsharded call bit for bit: every frame that touches a kept sample is present on
 * the member that keeps it, and is added in the same order. */
int nxsig_istft_sharded_c64(nxsig_group* g, const nxsig_c64* const* z, int64_t num_frames, int32_t batch, const float* window,
                            const nxsig_stft_params* params, int32_t axis, int32_t gather, nxsig_c64* const* y, int32_t mem);
/* FIR filtering (nxsig_fir_f32) sharded over the group; same conventions.  Channels axis: rows split.  Frames axis here
 * means OUTPUT SAMPLE ranges of every row with a (num_taps - 1)-sample input halo (nxsig_shard_fir); it has ONE exchange step:
 * a row that holds an Inf / NaN anywhere has no finite output in the reference (one transform per row, convolution.ex:276-284),
 * so every member reads off its slice which rows its own samples poisoned, the flags (int32[batch]) are all-reduced with a maximum
 * (ncclAllReduce; members of one process that share a device: through the host) and every member turns the flagged rows NaN —
 * the sharded result equals the unsharded one for such rows too.  A ranked group without RCCL cannot do that: unsupported. */
int nxsig_fir_sharded_f32(nxsig_group* g, const float* const* x, int64_t length, int32_t batch, int64_t batch_stride,
                          const float* h, int32_t num_taps, int32_t mode, int32_t axis, int32_t gather, float* const* y,
                          int32_t mem);

/*
 * NxSignal.stft/3 |> NxSignal.stft_to_mel/3 (lib/nx_signal.ex:68-130, :486-513) sharded over the group — the one sharded entry
 * point with an EXCHANGE step: the clamp `max(log_spec, reduce_max(log_spec) - 8)` (:511) needs the maximum over the whole
 * tensor.  Every member runs the fused stft -> mel kernel on its shard (device-resident, laid out as for nxsig_stft_sharded_f32
 * with mem == NXSIG_DEVICE: rows [c0, c1) for the channels axis, the sample span [s0, s1) of every row for the frames axis),
 * or — mem == NXSIG_HOST, LOCAL groups — on the part of the host tensor x[0] the call uploads to it;
 * the members' running maxima (one int32 pair: ordered-int maximum, non-finite flag) are all-reduced — ncclAllReduce / ncclMax
 * on the members' streams inside one ncclGroupStart / End; members of one process that share a device reduce through the
 * host — and every member then clamps its own shard.  mem == NXSIG_DEVICE: out[i] is f32[c1 - c0][M][mel_bins] /
 * f32[batch][m1 - m0][mel_bins] on member i's device and the results stay sharded (assemble with nxsig_group_allgather if
 * needed); mem == NXSIG_HOST: out[0] is the whole host result f32[batch][M][mel_bins].  window_padding must be :valid.
 * `filters`: host f32[mel_bins][fft_length] (nxsig_mel_filters_f32).  Asynchronous on the members' streams.
 */
int nxsig_stft_mel_sharded_f32(nxsig_group* g, const float* const* x, int64_t length, int32_t batch, int64_t batch_stride,
                               const float* window, const nxsig_stft_params* params, int32_t mel_bins, const float* filters,
                               int32_t axis, float* const* out, int64_t* num_frames_out, int32_t mem);

/* per-launch stopwatch on the ctx stream: lap() records an event (at most 4096 per series), laps() synchronises and
 * returns the n - 1 intervals in milliseconds and clears the series */
int nxsig_timer_lap(nxsig_ctx* ctx);
int nxsig_timer_laps(nxsig_ctx* ctx, float* intervals_ms, int32_t capacity, int32_t* count);

/* ---------------------------------------------------------------- spectral estimation --- */
/*
 * Spectral.welch / csd / coherence: Welch's averaged periodogram of real f32 rows — scipy.signal.welch / csd with
 * return_onesided = True, average = "mean", nperseg = frame_length, noverlap = frame_length - hop, nfft = fft_length (the reference has
 * no spectral estimator).  Frame m of a row covers samples [m hop, m hop + N), M = (length - N) / hop + 1
 * frames, no padding, a ragged tail is dropped; K = fft_length >= N (zero padded).  For bin k in [0, K / 2]
 *     Pxy[k] = scale * d_k * (1 / M) sum_m conj(X_m[k]) Y_m[k],      X_m = DFT_K(w * (x_m - mean(x_m)))      (detrend != 0)
 * with scale = 1 / (sampling_rate * sum w^2) (NXSIG_WELCH_DENSITY) or 1 / (sum w)^2 (NXSIG_WELCH_SPECTRUM), both formed in double
 * from the f32 window, and d_k = 2 except d_0 = 1 and, for even K, d_{K/2} = 1.  welch is csd(x, x): real.  The mean of a frame is
 * removed twice (the mean, then the mean of the residual) so that a large offset leaves no f32 round-off at bin 0 and its neighbours.
 * No |x| <= 1e-10 clean-up: this is not an Nx.fft result.
 *   x, y [batch][length] rows batch_stride >= length elements apart (one stride for both), window f32[frame_length] HOST,
 *   pxx_out / pyy_out f32[batch][bins], pxy_out c64[batch][bins], bins = nxsig_welch_bins(fft_length), dense.  In nxsig_csd_f32
 *   pxx_out and pyy_out may be NULL (not wanted).
 * Non-finite rule: a row (for csd: the pair x_r, y_r) with an Inf / NaN inside the samples its M frames cover gives NaN in EVERY bin
 * of every result of that row — Pxx of a row whose y holds the NaN included; a non-finite sample in the dropped tail, in the gap
 * between rows or in another row reaches nothing.
 * Deterministic: partial sums per (row, run of frames) are stored and added in ascending run order, no atomics.  The same call gives
 * the same bits every time, and rows of equal content within one call get equal bits.  Across batch sizes welch.generic / csd.generic
 * keep a row's bits (their runs are 64 frames whatever the batch); welch.pair / csd.pair size their runs from rows x frames of the
 * whole call and sum a run in f32, so there a row of another batch size agrees within tolerance, not bit for bit — unless its
 * frames fit one run or the runs are the shortest ones (four units) in both calls.
 * Dispatch: welch.pair / csd.pair (fft_length 1024 and 2048: wave-private transforms, the spectrum never reaches memory),
 * welch.generic / csd.generic for every other length and under NXSIG_DISABLE_WELCH_WAVE.  The tiers agree within tolerance, not bit
 * for bit.
 */
typedef enum nxsig_welch_scaling { NXSIG_WELCH_DENSITY = 0, NXSIG_WELCH_SPECTRUM = 1 } nxsig_welch_scaling;
/* bins of a one-sided estimate: fft_length / 2 + 1 (even and odd lengths alike, as rfft); negative status when fft_length < 1 */
int32_t nxsig_welch_bins(int32_t fft_length);
int nxsig_welch_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                    int32_t frame_length, int32_t hop, int32_t fft_length, int32_t detrend, int32_t scaling, double sampling_rate,
                    float* pxx_out, int32_t mem);
int nxsig_csd_f32(nxsig_ctx* ctx, const float* x, const float* y, int64_t length, int32_t batch, int64_t batch_stride, const float* window,
                  int32_t frame_length, int32_t hop, int32_t fft_length, int32_t detrend, int32_t scaling, double sampling_rate,
                  float* pxx_out, float* pyy_out, nxsig_c64* pxy_out, int32_t mem);

/* ---------------------------------------------------------------- recursive filters --- */
/*
 * Filters.sosfilt / sosfilt_zi / sosfiltfilt: cascades of second-order sections over real f32 rows — scipy.signal 1.15's definition
 * (the reference has no recursive filter).  sos is f64[n_sections][6] = b0 b1 b2 a0 a1 a2 per section with
 * a0 == 1, always a HOST pointer.  Each section runs in transposed direct form II on its predecessor's output,
 *     y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y
 * and (z0, z1) per section is scipy's state.  Coefficients, states and the recurrence are double on the device; a sample is widened
 * on load and an output rounded to f32 once.
 *   x [batch][length] rows batch_stride >= length elements apart, y f32[batch][length] dense; x and y must not overlap.
 *   zi   f64[zi_rows][n_sections][2] HOST or NULL (zero state); zi_rows is 1 (every row starts alike) or batch; a call that brings it
 *        synchronises (it is uploaded through scratch, never cached: feeding zf back as zi block after block keeps no table)
 *   zf_out f64[batch][n_sections][2] HOST or NULL: the states after the last sample; a call that asks for it synchronises
 *   direction 0: samples in order; 1: the same filter run from the end of each row towards its start (y[i] still belongs to x[i])
 *   n_sections 1 .. 16; more returns NXSIG_ERR_UNSUPPORTED (run the cascade in groups)
 * nxsig_sosfiltfilt_f32: scipy.signal.sosfiltfilt in one call, device resident: each row is extended by `edge` samples per side
 * (padlen < 0: scipy's default 3 * (2 n_sections + 1 - min(#(b2 == 0), #(a2 == 0))); NXSIG_SOS_PAD_NONE: 0), filtered forward from
 * the state sosfilt_zi * x_ext[0], filtered backward from sosfilt_zi * y_fwd[last], and the middle `length` samples are kept.  The
 * extension and the forward result are f32 rows.  padlen >= length is an error, worded as scipy's.
 * Non-finite rule: outputs ahead of the first Inf / NaN sample of a row are bit for bit those of the row with that sample and
 * everything after it zeroed; every output from it on is non-finite.  Other rows and the gaps between strided rows are untouched.
 * A zi row with a non-finite entry counts as a non-finite sample 0.  Under sosfiltfilt such a row is non-finite everywhere.
 * Deterministic: no atomics, one order of additions; chunk and tile depend on n_sections only, a row's bits do not depend on the
 * batch.  Dispatch: sosfilt.scan (a time-parallel scan: chunks of nxsig_sosfilt_chunk samples per lane, tiles of nxsig_sosfilt_tile
 * samples per workgroup), sosfilt.generic (one lane per row) for rows of at most one chunk and under NXSIG_DISABLE_SOSFILT_SCAN.  The
 * tiers agree within tolerance, not bit for bit.
 */
typedef enum nxsig_sos_padtype { NXSIG_SOS_PAD_NONE = 0, NXSIG_SOS_PAD_ODD = 1, NXSIG_SOS_PAD_EVEN = 2, NXSIG_SOS_PAD_CONSTANT = 3 } nxsig_sos_padtype;
/* samples per lane / per workgroup tile of sosfilt.scan for a cascade of n_sections (1 .. 16); negative status otherwise */
int32_t nxsig_sosfilt_chunk(int32_t n_sections);
int32_t nxsig_sosfilt_tile(int32_t n_sections);
/* scipy.signal.sosfilt_zi: the state of a settled step response, f64[n_sections][2]; host only */
int nxsig_sosfilt_zi(const double* sos, int32_t n_sections, double* zi_out);
int nxsig_sosfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* sos,
                      int32_t n_sections, const double* zi, int32_t zi_rows, double* zf_out, int32_t direction, float* y, int32_t mem);
int nxsig_sosfiltfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* sos,
                          int32_t n_sections, int32_t padtype, int64_t padlen, float* y, int32_t mem);

/*
 * PeakFinding.find_peaks — scipy.signal.find_peaks 1.15 on every line of x along `axis`.  x: f32
 * (NXSIG_DT_F32) or f64 (NXSIG_DT_F64), the shape limits of nxsig_argrelextrema.  All compares are plain IEEE compares in double on
 * the exactly widened samples.
 *   peaks       i in [1, n - 2] with x[i - 1] < x[i]; j the first index > i with x[j] != x[i] (or n - 1); x[j] < x[i].  Edges i and
 *               j - 1, the peak their mean rounded down.  A plateau that reaches the end of a line is no peak.
 *   conditions  one bit per condition given: 1 plateau_size, 2 height, 4 threshold, 8 distance, 16 prominence, 32 width; applied in
 *               that order.  bounds: f64[5][2] HOST, the (min, max) of plateau_size, height, threshold, prominence, width, with
 *               -inf / +inf for an open side; may be NULL when only the distance is given.  threshold: min <= min(left, right) and
 *               max(left, right) <= max.
 *   distance    d = ceil(distance) >= 1.  The peaks of a line are visited from the highest to the lowest, AMONG EQUAL HEIGHTS THE
 *               LARGER INDEX FIRST (the library's own rule: SciPy leaves ties to an unstable sort); a peak still kept removes every
 *               other within less than d.  The device plays rounds that give exactly this result; the call waits once per round.
 *   prominence  wlen: ceil of the caller's window, >= 2, or -1 for the whole line; the walk covers peak -+ wlen / 2.  The base of a
 *               side is the position of its minimum nearest to the peak.
 *   width       at x[peak] - prominence * rel_height (rel_height >= 0), linear interpolation at both crossings, no fused
 *               multiply-add.
 * Results: indices s32[capacity][rank], the coordinates of the surviving peaks in row-major order, then -1 rows; *valid the true
 * count, also when it exceeds capacity (0 <= capacity <= lines * ((n - 1) / 2), the most a tensor holds; only the first `capacity`
 * rows are written).  want: one bit per property returned — bits 0 .. 7 peak_heights, left_thresholds, right_thresholds, prominences,
 * width_heights, left_ips, right_ips, widths (f64); bits 8 .. 12 left_bases, right_bases, left_edges, right_edges, plateau_sizes (s32
 * axis coordinates).  fprops: f64[rows][capacity], one row per f64 bit set, in bit order; iprops: s32[rows][capacity] likewise; NaN /
 * -1 at and past valid.  Either may be NULL when it has no row.  The same bits from run to run and from both dispatch families:
 * find_peaks.tables (min / max of every block of nxsig_find_peaks_block axis positions bound every walk) and find_peaks.generic
 * (NXSIG_DISABLE_FIND_PEAKS_TABLES: the same walks element by element).  The only atomics are integer or / and on mask words.
 */
int32_t nxsig_find_peaks_block(void);
/* rounds the distance stage of the calling thread's last nxsig_find_peaks took (0: it did not run) */
int32_t nxsig_find_peaks_rounds(void);
int nxsig_find_peaks(nxsig_ctx* ctx, const void* x, int32_t dtype, const int64_t* shape, int32_t rank, int32_t axis, const double* bounds,
                     uint32_t conditions, double distance, int64_t wlen, double rel_height, int64_t capacity, uint32_t want,
                     int32_t* indices, uint32_t* valid, double* fprops, int32_t* iprops, int32_t mem);

/*
 * Filters.savgol_filter / savgol_coeffs — scipy.signal 1.15's Savitzky-Golay smoothing and smoothed derivatives over real f32 or f64
 * rows (the reference has neither).  THE DEFINITION: with W = window_length, h = W / 2 (rounded down), L = h for
 * an odd W and h - 1 for an even one, k[0 .. W) the correlation weights (nxsig_savgol_coeffs with pos = -1 and NXSIG_SAVGOL_DOT) and
 * ext(i) the row extended by `mode`,
 *     y[i] = sum over j = 0 .. W - 1 of k[j] * ext(i - L + j)
 *   NXSIG_SAVGOL_MIRROR    period 2 (n - 1), the edge sample not repeated; n = 1 gives the sample itself
 *   NXSIG_SAVGOL_NEAREST   the index clamped to [0, n - 1]
 *   NXSIG_SAVGOL_WRAP      the index modulo n
 *   NXSIG_SAVGOL_CONSTANT  cval outside the row
 *   NXSIG_SAVGOL_INTERP    zero outside the row; then y[0 .. h) and y[n - h .. n) are replaced by the deriv-th derivative, divided by
 *                          delta^deriv, of the degree-polyorder least-squares polynomial through the first / last W samples, evaluated
 *                          at those positions: a fixed linear map E[h][W], y[i] = sum_j E[i][j] x[j] and
 *                          y[n - 1 - i] = (-1)^deriv sum_j E[i][j] x[n - 1 - j].  Needs W <= n; the other modes take any n >= 1.
 * Weights: k[j] is the weight of window sample j in the deriv-th derivative at window position pos (default: the centre, h for an odd
 * W, h - 0.5 for an even one) of the least-squares polynomial of degree polyorder through W samples `delta` apart.  THEY ARE THE EXACT
 * LEAST-SQUARES WEIGHTS ROUNDED TO DOUBLE, NOT SCIPY'S: each lies within 1e-12 max|k| of the rational solution (formed in long double on
 * the polynomials orthogonal over the window); scipy's lstsq on the uncentred Vandermonde matrix loses digits as W grows (4.5e-6 at
 * W = 512, polyorder 7, deriv 3).  At the default pos an even (odd) derivative has exactly symmetric (antisymmetric) weights and an odd
 * derivative over an odd window a centre weight of exactly zero.  deriv > polyorder gives all-zero weights.  NXSIG_SAVGOL_CONV returns
 * them reversed (scipy's default order).
 * Limits: 1 <= W <= 1025, polyorder < W, polyorder <= 15 (beyond: NXSIG_ERR_UNSUPPORTED), deriv >= 0, delta finite and non-zero, cval
 * finite.  x [batch][length] rows batch_stride >= length elements apart, f32 (is_f64 = 0) or f64 (1); y the same type, dense
 * [batch][length]; x and y must not overlap.
 * Arithmetic: every sample is widened to double; the sum is ONE chain acc = fma(k[j], ext(i - L + j), acc) from acc = 0 in ascending j,
 * every weight included, zero ones too; an edge output of INTERP the same chain over E[i][j] in ascending j (the sign applied last); the
 * result is rounded to the row type once.  Both dispatch families follow it, so they return the same bits: savgol.tiles (a workgroup per
 * tile of nxsig_savgol_tile() outputs, samples in LDS) and savgol.generic (one lane per output; rows shorter than one tile and
 * everything under NXSIG_DISABLE_SAVGOL_TILES).  No atomics; a row's bits do not depend on the batch.
 * Non-finite rule: an output is non-finite exactly when its window, after extension, covers an Inf / NaN sample (under WRAP and MIRROR
 * that includes the samples the extension brings in); under INTERP all h edge outputs of a side are non-finite when the first / last W
 * samples hold one.  Which of NaN / Inf comes out is not specified.  Other outputs and other rows keep their bits.
 * Every argument check comes ahead of the context; a device call returns without waiting (the first call of a parameter set on a
 * context forms and uploads its tables).
 */
typedef enum nxsig_savgol_mode { NXSIG_SAVGOL_MIRROR = 0, NXSIG_SAVGOL_CONSTANT = 1, NXSIG_SAVGOL_NEAREST = 2, NXSIG_SAVGOL_WRAP = 3,
                                 NXSIG_SAVGOL_INTERP = 4 } nxsig_savgol_mode;
typedef enum nxsig_savgol_use { NXSIG_SAVGOL_CONV = 0, NXSIG_SAVGOL_DOT = 1 } nxsig_savgol_use;
/* outputs per workgroup tile of savgol.tiles */
int32_t nxsig_savgol_tile(void);
/* out: f64[window_length]; pos = -1: the default; host only */
int nxsig_savgol_coeffs(int32_t window_length, int32_t polyorder, int32_t deriv, double delta, double pos, int32_t use, double* out);
int nxsig_savgol_filter(nxsig_ctx* ctx, const void* x, int32_t is_f64, int64_t length, int32_t batch, int64_t batch_stride,
                        int32_t window_length, int32_t polyorder, int32_t deriv, double delta, int32_t mode, double cval, void* y, int32_t mem);

/*
 * Filters.hilbert — scipy.signal.hilbert(x, N=None, axis=-1) of SciPy 1.15 over real f32 rows: the analytic signal, its magnitude (the
 * envelope) or its imaginary part (the Hilbert transform proper).  The reference has none of them; DESIGN.md section 3.16.
 * THE DEFINITION: a row of `length` samples is truncated or zero-padded to N = n_fft points (SciPy's default is N = length),
 *     X = DFT_N(row),   a = IDFT_N(X h) with its 1 / N,
 *     h[0] = 1;  N even: h[N / 2] = 1 and h[k] = 2 for 0 < k < N / 2;  N odd: h[k] = 2 for 0 < k < (N + 1) / 2;  every other h[k] = 0.
 * The gains of a row sum to N.  No Nx.fft-style clean-up of small values is applied, to either transform.
 *   NXSIG_HILBERT_ANALYTIC    out = a, c64 [batch][n_fft]
 *   NXSIG_HILBERT_ENVELOPE    out = |a| = sqrtf(re * re + im * im) in f32 on the rounded components of a, f32 [batch][n_fft] (the expression
 *                             of nxsig_stft_magnitude_f32's NXSIG_MAG_ABS, the same in both dispatch families)
 *   NXSIG_HILBERT_QUADRATURE  out = Im a, f32 [batch][n_fft]
 * x [batch][length] rows batch_stride >= length elements apart, of which the first min(length, n_fft) samples are read; out dense; x
 * and out must not overlap.  batch = 0 succeeds and launches nothing.  Limits: length >= 1, 1 <= n_fft < 2^31; lengths the row
 * transforms of nxsig_fft refuse, rows whose byte counts overflow and f64 rows (there is no f64 entry point) are
 * NXSIG_ERR_UNSUPPORTED.
 * Dispatch families: hilbert.wave (n_fft = 1024, 2048: one wave per row, both transforms and the gain in registers and LDS, the row
 * read once and the result written once) and hilbert.generic (every other n_fft, and every n_fft under NXSIG_DISABLE_HILBERT_WAVE or
 * NXSIG_DISABLE_WAVE: nxsig_fft's row transforms around an in-place gain, the spectrum in scratch memory).  Both are single-precision
 * transforms: a row is within 1e-5 max|a| of the definition evaluated in double; the two families need not agree to the bit.  No
 * atomics; a row's bits do not depend on the batch.
 * Arithmetic: a row that fills the transform (length >= n_fft: no zero padding) is transformed as row - c, c the row's mean as f32 sums
 * give it, and c is added to Re a afterwards.  Algebraically that is the same a (only X[0] changes, and h[0] = 1); numerically the
 * rounding of the two transforms then scales with the row's variation, not with its offset: Im a of a 1000 + N(0, 1) row stays within
 * 1e-5 max|Im a|, where the plain transforms leave 6e-5.  A zero-padded row is transformed as it stands.
 * Non-finite rule: a row that holds an Inf / NaN among the min(length, n_fft) samples read has no finite output element (SciPy's
 * transforms behave alike); which of NaN / Inf comes out is not specified.  The rule is carried out on X[0], the sum of the samples as the
 * forward transform forms it: when it is not finite the whole spectrum of the row is replaced by NaN.  (Finite samples whose sum
 * overflows f32 therefore poison their row, whose outputs overflow anyway.)  No other row of the batch is affected, and samples at or
 * past min(length, n_fft) are not read.
 * Every argument check comes ahead of the context; a device call returns without waiting.
 */
typedef enum nxsig_hilbert_kind { NXSIG_HILBERT_ANALYTIC = 0, NXSIG_HILBERT_ENVELOPE = 1, NXSIG_HILBERT_QUADRATURE = 2 } nxsig_hilbert_kind;
int nxsig_hilbert_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, int64_t n_fft, int32_t kind,
                      void* out, int32_t mem);

/*
 * Transforms.dct / idct — scipy.fft.dct(x, type, n, axis, norm) and idct of SciPy 1.15 over real f32 rows, types 2 and 3, and the mfcc
 * front end built on them.  The reference has neither; DESIGN.md section 3.17.
 * THE DEFINITION: a row of `length` samples is truncated or zero-padded to n points (SciPy's default is n = length), then
 *   type 2   y[k] = 2 sum_{j=0}^{n-1} x[j] cos(pi k (2 j + 1) / (2 n))
 *            norm NXSIG_DCT_ORTHO: y[0] * sqrt(1 / (4 n)), y[k > 0] * sqrt(1 / (2 n));  NXSIG_DCT_FORWARD: y / (2 n)
 *   type 3   y[k] = x[0] + 2 sum_{j=1}^{n-1} x[j] cos(pi (2 k + 1) j / (2 n))
 *            norm NXSIG_DCT_ORTHO: y[k] = x[0] / sqrt(n) + sqrt(2 / n) sum_{j>=1} x[j] cos(...);  NXSIG_DCT_FORWARD: y / (2 n)
 * idct(x, type t, norm) is the transform of the other type (2 <-> 3) with NXSIG_DCT_BACKWARD and NXSIG_DCT_FORWARD exchanged and
 * NXSIG_DCT_ORTHO kept, so idct(dct(x)) = x for every norm; the caller makes the exchange (there is no inverse flag).  Types 1 and 4
 * are valid in SciPy and not built: NXSIG_ERR_UNSUPPORTED; any other type is an argument error.  SciPy's orthogonalize=, overwrite_x= and
 * workers= are not offered.  No Nx.fft-style clean-up of small values is applied.
 * keep (the one extension): only the leading keep coefficients y[0 .. keep) are computed and stored, 1 <= keep <= n; they carry the
 * bits of the leading slice of the full result.
 * x [batch][length] rows batch_stride >= length elements apart, of which the first min(length, n) samples are read; out dense
 * [batch][keep]; x and out must not overlap.  batch = 0 succeeds and launches nothing.  Limits: length >= 1, 1 <= n < 2^31; lengths the
 * row transforms of nxsig_fft refuse, rows whose byte counts overflow and f64 rows (there is no f64 entry point) are
 * NXSIG_ERR_UNSUPPORTED.
 * Dispatch families: dct.direct (n <= 256, any keep — the cepstral path: every output is one sum over ascending j against a cosine
 * table, several rows per workgroup through LDS) and dct.fft (every other n, and every n under NXSIG_DISABLE_DCT_DIRECT: Makhoul's
 * n-point form — a permutation, one row transform of nxsig_fft, a twiddle; the other way round for type 3).  The tables are built on the
 * host in double from an integer argument reduced mod 4 n, so no argument of cos is rounded and cos of an odd multiple of pi / 2 is an
 * exact zero.  Both families are single precision: a row is within 1e-5 max_k |y[k]| of the definition evaluated in double; the two
 * families need not agree to the bit.  No atomics: a row's bits depend neither on the batch nor on where the tensors live.
 * Arithmetic: both families compute type 2 on row - c, c the mean of the n points as f32 sums give it, and add c * 2 n (times the
 * norm's factor of y[0]) to y[0].  Algebraically nothing changes (sum_j cos(pi k (2 j + 1) / (2 n)) = 0 for 0 < k < n); numerically the
 * coefficients k >= 1 of a 1000 + N(0, 1) row then stay within 1e-5 max_{k>=1} |y[k]|, where plain f32 sums against an f32 table
 * leave 5e-4 to 1e-3 and a plain single-precision transform of Makhoul's form 2.5e-4.  Type 3 is computed as it stands.
 * Non-finite rule: a row that holds an Inf / NaN among the min(length, n) samples read has no finite output element (SciPy's
 * transforms behave alike); which of NaN / Inf comes out is not specified.  dct.direct: every output is a sum over every sample.
 * dct.fft: when bin 0 of the forward transform (type 2: the sum of the samples) or point 0 of the inverse one (type 3: the sum of the
 * spectrum) is not finite, the row leaves as NaN.  No other row of the batch is affected, and samples at or past min(length, n) are
 * not read.
 * Every argument check comes ahead of the context; a device call returns without waiting.
 */
typedef enum nxsig_dct_norm { NXSIG_DCT_BACKWARD = 0, NXSIG_DCT_ORTHO = 1, NXSIG_DCT_FORWARD = 2 } nxsig_dct_norm;
int nxsig_dct_f32(nxsig_ctx* ctx, const float* x, int64_t length, int64_t batch, int64_t batch_stride, int64_t n, int32_t type, int32_t norm,
                  int64_t keep, float* out, int32_t mem);

/*
 * Filters.lfilter / lfilter_zi / filtfilt — scipy.signal 1.15's transfer-function filter over real f32 rows (the reference has no
 * recursive filter).  b = f64[nb] and a = f64[na] are HOST pointers, finite, a[0] != 0; both are divided by a[0]
 * and the shorter is filled up with zeros.  The order is n = max(nb, na) - 1, and a row runs in transposed direct form II,
 *     y = b0 x + z[0];   z[i] = z[i + 1] + b[i + 1] x - a[i + 1] y  (i < n - 1);   z[n - 1] = b[n] x - a[n] y
 * with z, n doubles, scipy's zi / zf.  Coefficients, states and the recurrence are double on the device; a sample is widened on load
 * and an output rounded to f32 once.  n = 0 is a gain.  n > 16 returns NXSIG_ERR_UNSUPPORTED: a recursive filter of such an order belongs
 * in second-order sections (nxsig_sosfilt_f32), an FIR one (na == 1) in nxsig_fir_f32.
 *   x [batch][length] rows batch_stride >= length elements apart, y f32[batch][length] dense; x and y must not overlap.
 *   zi   f64[zi_rows][n] HOST or NULL (zero state); zi_rows is 1 (every row starts alike) or batch; a call that brings it synchronises
 *        (it is uploaded through scratch, never cached: feeding zf back as zi block after block keeps no table)
 *   zf_out f64[batch][n] HOST or NULL: the states after the last sample; a call that asks for it synchronises
 *   direction 0: samples in order; 1: the same filter run from the end of each row towards its start (y[i] still belongs to x[i])
 * nxsig_filtfilt_f32: scipy.signal.filtfilt(b, a, x, method="pad") in one call, device resident: each row is extended by `edge` samples
 * per side (padlen < 0: scipy's default 3 max(na, nb); NXSIG_SOS_PAD_NONE: 0), filtered forward from the state lfilter_zi * x_ext[0],
 * filtered backward from lfilter_zi * y_fwd[last], and the middle `length` samples are kept.  The extension and the forward result are
 * f32 rows.  padlen >= length is an error, worded as scipy's; so is a filter with a pole at z = 1 (lfilter_zi is singular).
 * Non-finite rule: outputs ahead of the first Inf / NaN sample of a row are bit for bit those of the row with that sample and
 * everything after it zeroed; every output from it on is non-finite, because 0 * Inf and 0 * NaN keep every state NaN; a gain (n = 0) runs as an
 * order-1 filter with zero coefficients and follows the same rule (scipy's gain touches that one sample only).  THAT IS THE
 * RECURRENCE'S BEHAVIOUR, ALSO FOR na == 1, NOT SCIPY'S: scipy runs such a filter as a convolution, after which a non-finite sample
 * reaches only the nb outputs whose taps cover it.  Other rows and the gaps between strided rows are untouched.  A zi row with a
 * non-finite entry counts as a non-finite sample 0.  Under filtfilt such a row is non-finite everywhere.
 * Deterministic: no atomics, one order of additions; chunk and tile depend on the order only, a row's bits do not depend on the batch.
 * Dispatch: lfilter.scan (sosfilt's time-parallel scan on the dense n x n companion matrix: chunks of nxsig_lfilter_chunk samples per
 * lane, tiles of nxsig_lfilter_tile samples per workgroup) and lfilter.generic (one lane per row, the plain recurrence) for rows of at
 * most one chunk, under NXSIG_DISABLE_LFILTER_SCAN, and for every filter the conditioning guard keeps off the scan: a direct form with
 * clustered poles (a 20 Hz high-pass of order 4 at 48 kHz, a Bessel low-pass of order 14) has matrix powers too badly conditioned for
 * the scan while the plain recurrence is still accurate.  The guard is a rule of the normalised (b, a) and the tiles per lane alone:
 * with G the largest |entry| among A^1 .. A^chunk of the companion matrix A and among the tables, every entry finite,
 * G x sum |a[k]| <= 1e4, and the table's A^chunk within 1e-11 G of chunk steps of the recurrence.  The tiers agree within tolerance,
 * not bit for bit.
 * Every argument check comes ahead of the context.
 */
/* samples per lane / per workgroup tile of lfilter.scan for a filter of `order` (0 .. 16); negative status otherwise */
int32_t nxsig_lfilter_chunk(int32_t order);
int32_t nxsig_lfilter_tile(int32_t order);
/* scipy.signal.lfilter_zi: the state of a settled step response, f64[max(nb, na) - 1]; host only */
int nxsig_lfilter_zi(const double* b, int32_t nb, const double* a, int32_t na, double* zi_out);
int nxsig_lfilter_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* b, int32_t nb,
                      const double* a, int32_t na, const double* zi, int32_t zi_rows, double* zf_out, int32_t direction, float* y, int32_t mem);
int nxsig_filtfilt_f32(nxsig_ctx* ctx, const float* x, int64_t length, int32_t batch, int64_t batch_stride, const double* b, int32_t nb,
                       const double* a, int32_t na, int32_t padtype, int64_t padlen, float* y, int32_t mem);

/*
 * Spectral.lombscargle — scipy.signal.lombscargle of SciPy 1.15 (the generalised Lomb-Scargle periodogram, with weights, floating_mean
 * and the three normalisations), batched over real f32 / f64 rows that share one time base (the reference has no such estimator;
 * DESIGN.md section 3.19).  x = f64[n] sample times (unsorted is fine), freqs = f64[num_freqs] ANGULAR frequencies (0 allowed) and
 * weights = f64[n] or NULL (ones) are always HOST pointers and must be finite; weights >= 0 with a positive sum, normalised to sum 1 as
 * scipy does.  `mem` describes y and out only.
 *   y [batch][n] rows batch_stride >= n elements apart, dtype NXSIG_DT_F32 or NXSIG_DT_F64
 *   out [batch][num_freqs] dense: f32 for f32 rows, f64 for f64 rows; c64 / c128 when normalize == 2
 *   precenter 1: the plain mean of a row is subtracted from it first (on load, never as a correction of finished sums)
 *   normalize 0 "power": 2 (a YC + b YS) n / 4;  1 "normalize": 2 (a YC + b YS) 0.5 / YY;  2 "amplitude": (a + i b) e^{i tau}
 *   floating_mean 1: the fitted model carries a constant (the corrections by C, S and Y of scipy's Eq. 8 - 15)
 * With w the normalised weights and every sum over the row's samples: Y = sum w y, YY = sum w y y, C = sum w cos(wt), S = sum w sin(wt),
 * CC = sum w cos^2, SS = 1 - CC, CS = sum w cos sin; tau = atan2(2 CS, CC - SS) / 2; YC, YS, CC, SS at the phase wt - tau;
 * CC and SS are clamped from below at 2^-53 (numpy's finfo(float64).epsneg, for both result types); a = YC / CC, b = YS / SS.
 * Every sum, tau, the divisions and the normalisation are double on the device; a sample is widened on load and a result rounded to
 * its type once.  The phase is fl(freqs[k] * x[i]) in double, fed to the double sincos, as numpy does: no f32 phase, no fast intrinsic.
 * Non-finite rule: a row of y that holds an Inf / NaN is NaN at every frequency (both parts under "amplitude"); a zero weight does
 * not shield it.  Other rows keep their bits; the gaps between strided rows and everything outside the result are untouched.
 * Deterministic: no atomics, one order of additions per tier; within a tier the bits of out[r][k] depend neither on the batch nor on
 * which other rows run beside row r.
 * Dispatch: lombscargle.tile (a workgroup owns nxsig_lombscargle_block(0) frequencies and (1) rows, walks the time axis in tiles of (2)
 * samples staged through LDS, one sincos per (t, w) for all its rows; tau from the unshifted sums, which are then rotated by tau
 * instead of summed again) on every shape and option set; lombscargle.generic (one lane per (row, frequency), scipy's two passes as
 * written) under NXSIG_LOMBSCARGLE_TILE=0.  A rule of the switch alone, never of the batch.  The tiers agree within tolerance, not bit
 * for bit.  x, freqs and the normalised weights go through the context's table cache: a repeated call uploads nothing.
 * Every argument check comes ahead of the context.
 */
/* 0: frequencies per workgroup, 1: rows per workgroup, 2: samples per staged tile of lombscargle.tile; negative status otherwise */
int32_t nxsig_lombscargle_block(int32_t which);
int nxsig_lombscargle(nxsig_ctx* ctx, const void* y, int32_t dtype, int64_t n, int32_t batch, int64_t batch_stride,
                      const double* x, const double* freqs, int64_t num_freqs, const double* weights /* or NULL */,
                      int32_t precenter, int32_t normalize, int32_t floating_mean, void* out, int32_t mem);

/*
 * Transforms.czt / zoom_fft — scipy.signal.czt and zoom_fft of SciPy 1.15 over real f32 or c64 rows: the chirp z-transform, a DFT of
 * any length, any start and any step, and the narrow-band zoom built on it.  The reference has neither; DESIGN.md section 3.20.
 * THE DEFINITION: for a row x[0 .. n) (n = length) and m output points
 *     X[k] = sum_{j<n} x[j] a^(-j) w^(j k),   k = 0 .. m - 1,
 *     w = w_abs exp(-2 pi i w_step / w_den),   a = a_abs exp(2 pi i a_turns).
 * Angles are carried as turns, and the step as a double over a positive integer, so that every phase the transform needs, such as
 * k^2 w_step / (2 w_den), is reduced mod 1 in integer arithmetic before it meets a sine (csrc/czt_plan.hpp: a 128-bit binary fraction
 * and a wrapping product; what is lost is under 2^-66 of a turn).  SciPy's ZoomFFT forms exp(-i pi scale k^2 / m) from an unreduced
 * double and loses the tail of long rows; that is not copied.  How SciPy's three calls map onto the definition:
 *     czt(x, m)                        w_abs 1, w_step 1, w_den m, a_abs 1, a_turns 0
 *     czt(x, m, w, a)                  w_abs |w|, w_step -arg(w) / 2 pi, w_den 1, a_abs |a|, a_turns arg(a) / 2 pi
 *     zoom_fft(x, [f1, f2], m, fs)     w_abs 1, w_step scale, w_den m, a_abs 1, a_turns f1 / fs;  scale = (f2 - f1) / fs, or
 *                                      (f2 - f1) m / (fs (m - 1)) with endpoint, exactly as SciPy computes it
 * x [batch][length] rows batch_stride >= length elements apart, f32 (is_complex 0) or c64 (is_complex 1); out c64 [batch][m], dense;
 * x and out must not overlap.  batch = 0 succeeds and launches nothing.
 * Both dispatch families are Bluestein's identity j k = (j^2 + k^2 - (k - j)^2) / 2 over three tables formed on the host in double and
 * rounded to f32 once (nxsig_czt_tables returns them as doubles):
 *     A[j] = a^(-j) w^(j^2 / 2), j < n         applied to the samples
 *     F    = DFT_L(v) / L,  v[j mod L] = w^(-j^2 / 2) for j in (-n, m), zero elsewhere;  L a power of two >= n + m - 1
 *     W[k] = w^(k^2 / 2), k < m                applied to the first m points of IDFT_L(DFT_L(x A) F) (the inverse without its 1 / L)
 * czt.wave (n + m - 1 <= 2048: L = 1024 when n + m - 1 fits, else 2048; one wave per row, both transforms and the three products in
 * registers and LDS, the row read once and the result written once) and czt.generic (everything else, and everything under
 * NXSIG_CZT_WAVE=0 or NXSIG_DISABLE_WAVE: L the next power of two, nxsig_fft's row transforms around the three products, the padded rows
 * in two temporaries the context keeps).  Both are single-precision transforms: a row is within 1e-5 max|X| of the definition
 * evaluated in double; the two families need not agree to the bit.  No atomics; a row's bits do not depend on the batch.  The tables
 * are cached per context by content; a repeated call forms nothing again.
 * Spirals: |w| != 1 or |a| != 1 is accepted while the spread max|t| / min|t| of each of A, v and W stays within 32 (the gate is
 * measured: csrc/czt_plan.hpp); beyond it the call is NXSIG_ERR_UNSUPPORTED, "czt: the contour leaves single
 * precision".
 * Non-finite rule: a row that holds an Inf / NaN among its n samples has no finite output element; which of NaN / Inf comes out is not
 * specified.  The rule is carried out on bin 0 of the forward transform, the sum of the chirped samples: when it is not finite the
 * whole spectrum of the row is replaced by NaN.  No other row of the batch is affected; rows never share a transform.
 * Limits: n, m >= 1, w_den >= 1, w_abs and a_abs positive and finite, w_step and a_turns finite, batch_stride >= length.  n + m - 1 over
 * 2^30, w_den over 2^61, lengths the row transforms of nxsig_fft refuse and rows whose byte counts overflow are NXSIG_ERR_UNSUPPORTED.
 * Not built: f64 / c128 rows (there is no double tier), device tensors along another axis than the last, sharded entry points, NIF
 * and Elixir functions.
 * Every argument check comes ahead of the context; a device call returns without waiting.
 */
/* L of the family the shape takes by default (1024 or 2048 while n + m - 1 <= 2048, else the next power of two); negative status
 * for n < 1, m < 1 or n + m - 1 > 2^30.  Host only, no context */
int64_t nxsig_czt_conv_length(int64_t n, int64_t m);
/* the three tables as interleaved complex doubles: A f64[2 n], F f64[2 L], W f64[2 m]; L a power of two >= n + m - 1; *spread (or
 * NULL) receives the contour's spread, also when it is refused.  Host only, no context */
int nxsig_czt_tables(int64_t n, int64_t m, int64_t L, double w_abs, double w_step, int64_t w_den, double a_abs, double a_turns,
                     double* A, double* F, double* W, double* spread);
int nxsig_czt(nxsig_ctx* ctx, const void* x, int32_t is_complex, int64_t length, int64_t batch, int64_t batch_stride, int64_t m,
              double w_abs, double w_step, int64_t w_den, double a_abs, double a_turns, void* out, int32_t mem);

/*
 * Filters.fir_bank / Transforms.cwt — a bank of S FIR filters of different lengths over real f32 rows, and the continuous wavelet
 * transform that is one instance of it: scipy.signal.cwt, morlet2 and ricker as SciPy <= 1.14 had them (1.15 removed them, so the
 * definition is written down here).  The reference has neither; DESIGN.md section 3.21.
 * THE DEFINITION: for a row x[0 .. L) (L = length) and a filter h of N taps
 *     full[n] = sum_k x[k] h[n - k],          out[s][n] = full[n + (N - 1) / 2],  0 <= n < L   ("same" alignment, integer division)
 * which for N <= L is numpy.convolve(x, h, "same").  nxsig_fir_bank takes the filters as they are.  nxsig_cwt builds, per width a,
 *     N   = min(ceil(10 a), L)                (SciPy passed the unrounded 10 a to arange: the same count)
 *     h_a = conj(wavelet(N, a))[::-1]
 *     morlet2(M, s, w): t = (arange(M) - (M - 1) / 2) / s,  sqrt(1 / s) pi^(-1/4) exp(i w t) exp(-t^2 / 2)             complex
 *     ricker(M, a):     v = arange(M) - (M - 1) / 2,        2 / (sqrt(3 a) pi^(1/4)) (1 - v^2 / a^2) exp(-v^2 / (2 a^2))  real
 * evaluated on the host in double and rounded to f32 once (nxsig_cwt_wavelet returns the doubles), and runs the same launcher.
 * x [batch][length] rows batch_stride >= length elements apart, any 4-byte address; taps a HOST array, the S filters concatenated, f32
 * (taps_complex 0) or c64 (1); tap_counts HOST int64[S]; out dense [batch][S][length], c64 for NXSIG_CWT_COMPLEX, f32 for
 * NXSIG_CWT_REAL (the real part), NXSIG_CWT_MAGNITUDE (sqrtf(re re + im im), the expression of nxsig_hilbert's envelope) and
 * NXSIG_CWT_POWER (re re + im im).  x and out must not overlap.
 * The bank is split by support and one launch group runs per non-empty class; nxsig_last_dispatch names the classes that ran:
 *     cwt.wave     N <= 513 at K = 1024 points, 514 <= N <= 1025 at K = 2048: overlap-save inside one wave.  A block of K samples is
 *                  loaded and transformed ONCE; per filter of the class the spectrum is multiplied by H_s / K, inverted and the
 *                  block's valid run of out[row][s] stored through the sink.  Block step K - Nmax + 1, one per class.  H_s is the
 *                  K-point spectrum of the taps, formed in double and rounded once, cached per context (a repeated call forms nothing)
 *     cwt.generic  N > 1025, and everything under NXSIG_CWT_WAVE=0 or NXSIG_DISABLE_WAVE: the rows zero-padded to the next power of
 *                  two >= L + Nmax - 1 and transformed once by nxsig_fft's row transforms; per filter a product, the transform back and
 *                  a slice-and-sink kernel; three temporaries the context keeps
 * Both are single-precision: per (row, filter) the result is within 1e-5 max|out| of the definition in double, except where the output
 * cancels against a large offset of the row (then 1e-5 max|x| sum|h_s|).  The classes need not agree to the bit.  No atomics.
 * Non-finite rule (nxsig_fir's): a row that holds an Inf / NaN has no finite output element at any filter; every other row of the
 * batch keeps its bits.  A kernel that loads such a sample raises the row's flag; a last pass writes NaN over flagged rows.
 * Limits, each refused with its own message ahead of the context: batch in [1, 65535], num_filters in [1, 4096], every tap count >= 1,
 * length + max taps - 1 <= 2^24 (NXSIG_ERR_UNSUPPORTED), widths positive and finite, taps finite, batch_stride >= length.
 * Not built: f64 or complex rows, "full" / "valid" alignment (ragged), a 4096-point wave class, sharded entry points, NIF and Elixir
 * functions.  A device call returns without waiting.
 */
#define NXSIG_CWT_COMPLEX 0
#define NXSIG_CWT_REAL 1
#define NXSIG_CWT_MAGNITUDE 2
#define NXSIG_CWT_POWER 3
#define NXSIG_CWT_MORLET2 0
#define NXSIG_CWT_RICKER 1
/* N = min(ceil(10 width), length); negative status for a width that is not positive and finite or length < 1.  Host only, no context */
int64_t nxsig_cwt_support(double width, int64_t length);
/* conj(wavelet(N, width))[::-1] as N interleaved complex doubles (w: morlet2's omega, ignored by ricker).  Host only, no context */
int nxsig_cwt_wavelet(int32_t wavelet, double width, double w, int64_t N, double* out_f64);
int nxsig_fir_bank(nxsig_ctx* ctx, const void* x, int64_t length, int64_t batch, int64_t batch_stride, const void* taps, int32_t taps_complex,
                   const int64_t* tap_counts, int64_t num_filters, int32_t kind, void* out, int32_t mem);
int nxsig_cwt(nxsig_ctx* ctx, const void* x, int64_t length, int64_t batch, int64_t batch_stride, int32_t wavelet, const double* widths,
              int64_t num_widths, double w, int32_t kind, void* out, int32_t mem);

/*
 * Convolution.correlate_rows / convolve_rows — scipy.signal.correlate / convolve of SciPy 1.15.3 on row PAIRS: row r of one device (or
 * host) tensor with row r of another, both real f32 or both c64.  The reference has no pairwise call; DESIGN.md section 3.22.
 * THE DEFINITION: for rows x[0 .. n1) and y[0 .. n2)
 *     correlate   full[k] = sum_l x[l] conj(y[l - k + n2 - 1]),   k = 0 .. n1 + n2 - 2   (the lag of full[k] is k - (n2 - 1))
 *     convolve    full[k] = sum_l x[l] y[k - l].
 * mode (nxsig_conv_mode) selects a window of full: FULL all of it; SAME the n1 elements from (n2 - 1) / 2 (centred on full); VALID the
 * max(n1, n2) - min(n1, n2) + 1 elements from min(n1, n2) - 1, n2 > n1 included.  nxsig_conv_length(n1, n2, mode) is the window's
 * length n_out; the result is SciPy's per pair for every op and mode.
 * a [batch][n1] rows a_stride >= n1 elements apart; b [batch][n2] rows b_stride >= n2 apart, or b_stride = 0: ONE row b for every
 * pair (a shared template).  is_complex 0: f32 operands and result; 1: c64 operands and result.  a and b may be the same memory
 * (autocorrelation); out (and out_lags) must not overlap an operand or each other.  batch = 0 succeeds and launches nothing.
 * weighting NXSIG_XCORR_PHAT (correlate only) replaces the cross spectrum R[k] = X[k] conj(Y[k]) by
 *     G[k] = R[k] / max(|R[k]|, phat_floor max_j |R[j]|),   G[k] = 0 where that denominator is 0 (a pair whose cross spectrum is zero),
 * phat_floor in [0, 1).  G is not linear in the operands, so its inverse depends on the transform length: the contract fixes
 *     P = nxsig_xcorr_fft_length(n1, n2) = max(1024, the next power of two >= n1 + n2 - 1)      for BOTH dispatch families,
 * X = DFT_P(x), Y = DFT_P(y) of the zero-padded rows, and the weighted result is the mode's window of IDFT_P(G) (with its 1 / P).
 * sink NXSIG_XCORR_PEAK (correlate only) writes per pair, instead of the row, out_lags[r] = scipy.signal.correlation_lags(n1, n2,
 * mode)[i] and out[r] = window[i] at i = the first maximum in lag order (np.argmax) of the window's values (real pairs) or of their
 * moduli (c64 pairs: the f32 rounding of sqrt(re^2 + im^2) evaluated in double); out is then [batch], the [batch][n_out] rows are
 * never written.  SciPy's "same" lags are not always the lags of the "same" values (odd n1 with even n2 differ by one); the sink
 * reports correlation_lags' entry as it stands.
 * Dispatch families:
 *   xcorr.wave     n1 + n2 - 1 <= 1024, and real pairs up to 2048: one wave per pair on the wave-private transform cores, in czt.wave's
 *                  layout, LDS budget and rows-per-wave geometry.  A real pair is packed as z = x + i y into ONE forward transform,
 *                  X and Y recovered from Z[k] and Z[P - k] (fetched through the wave's LDS strip); each row is first scaled by the power
 *                  of two that brings its largest magnitude into [0.5, 1) and the scale is undone at the sink — exact, and needed: the
 *                  packed transform's error is relative to the larger row (rows of 1e4 against 1e-4 lose everything without it).  A c64
 *                  pair takes two forward transforms; at 2048 points that does not fit the register file, so c64 pairs with
 *                  n1 + n2 - 1 > 1024 run on xcorr.generic.  The operands are read once and the result written once
 *   xcorr.generic  everything else and everything under NXSIG_XCORR_WAVE=0 / NXSIG_DISABLE_WAVE: a pad kernel writes dense zero-padded
 *                  c64 rows [rows][P] of both operands (a shared template once), nxsig_fft's row transforms forward on both, the
 *                  product (PHAT after a per-row maximum), the inverse transform, a sink kernel.  Its four temporaries are its own,
 *                  kept by the context; the batch runs in slabs of pairs so that they stay within 256 MiB together (one pair when a
 *                  single pair is larger); NXSIG_XCORR_SLAB_ROWS (0 = automatic) forces the slab
 * Both are single-precision transforms: an element is within 1e-5 ||x||_2 ||y||_2 of the definition in double (the Cauchy-Schwarz
 * bound of any element), and a row of noise within 1e-5 of its maximum; the families need not agree to the bit.  No atomics; a
 * pair's bits depend neither on the batch nor on its neighbours in a wave or slab.
 * Non-finite rule: a pair in which either row holds an Inf / NaN has no finite output element; under the peak sink its value is NaN
 * and its lag 0.  Carried out on bin 0 of the forward transforms (the sum of the samples): when it is not finite the pair's cross
 * spectrum is replaced by NaN.  No other pair changes.  A pair of finite samples whose products overflow single precision (c64 rows near
 * 1e19) comes out Inf / NaN as any f32 arithmetic would; when its whole window is NaN the peak sink writes NaN and lag 0 as well.  The
 * PHAT weighting is formed on the cross spectrum scaled under 1 by a power of two, so it neither overflows nor vanishes where R is finite.
 * Limits: n1, n2 >= 1, a_stride >= n1, b_stride = 0 or >= n2, phat_floor in [0, 1); PHAT and the peak sink with convolve are refused.
 * n1 + n2 - 1 over 2^30, lengths the row transforms of nxsig_fft refuse and rows whose byte counts overflow are NXSIG_ERR_UNSUPPORTED.
 * Not built: f64 / c128 pairs (there is no double tier), mixed real / complex pairs, n-D correlation, device tensors along another axis
 * than the last, max_lag windows, "coeff" normalisation, sharded entry points, NIF and Elixir functions.
 * Every argument check comes ahead of the context; a device call returns without waiting.
 */
#define NXSIG_XCORR_CONVOLVE 0
#define NXSIG_XCORR_CORRELATE 1
#define NXSIG_XCORR_PLAIN 0
#define NXSIG_XCORR_PHAT 1
#define NXSIG_XCORR_ROWS 0
#define NXSIG_XCORR_PEAK 1
/* out_lags: s32 [batch] under NXSIG_XCORR_PEAK, else NULL (ignored) */
/* P of the contract: max(1024, the next power of two >= n1 + n2 - 1); negative status for n1 < 1, n2 < 1 or n1 + n2 - 1 > 2^30.
 * Host only, no context */
int64_t nxsig_xcorr_fft_length(int64_t n1, int64_t n2);
int nxsig_xcorr(nxsig_ctx* ctx, const void* a, int64_t n1, int64_t a_stride, const void* b, int64_t n2, int64_t b_stride, int64_t batch,
                int32_t is_complex, int32_t op, int32_t mode, int32_t weighting, double phat_floor, int32_t sink, void* out,
                int32_t* out_lags, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif /* NXSIG_H */
