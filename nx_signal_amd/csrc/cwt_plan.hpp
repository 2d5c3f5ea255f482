// Transforms.cwt / Filters.fir_bank: everything of it that is plain C++ — the support rule, the two wavelets,
// the argument checks, the split of a bank into launch classes, the block step and alignment of the overlap-save scheme, the builder of
// a filter's spectrum and the lane / slot arithmetic of the fused kernel.  The C entry points, the kernels of kernels_cwt.hip and the
// stand-alone program tests/san_cwt.cpp (ASan / UBSan on the host) all use this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "czt_plan.hpp"   // czt_fft_f64 (the double transform the tables are formed with), czt_overlap

#if defined(__HIPCC__)
#define NXSIG_CW_HD __host__ __device__ __forceinline__
#else
#define NXSIG_CW_HD inline
#endif

namespace nxsig {

enum CwtKind : int32_t { kCwComplex = 0, kCwReal = 1, kCwMagnitude = 2, kCwPower = 3 };
enum CwtWavelet : int32_t { kCwMorlet2 = 0, kCwRicker = 1 };
// the launch classes of a bank, by support N: cwt.wave at K = 1024 (N <= 513) and K = 2048 (514 <= N <= 1025), cwt.generic beyond
enum CwtClass : int32_t { kCwWave1024 = 0, kCwWave2048 = 1, kCwGeneric = 2, kCwClasses = 3 };

constexpr int64_t kCwtMaxBatch = 65535, kCwtMaxFilters = 4096, kCwtMaxExtent = (int64_t)1 << 24;

// ---- the definition (include/nxsig.h).  N = min(ceil(10 a), L): SciPy passed the unrounded 10 a to arange, the same count
inline int64_t cwt_support(double width, int64_t length) {
  const double n = std::ceil(10.0 * width);
  if (!(n < (double)length)) return length;
  return n < 1.0 ? 1 : (int64_t)n;
}
// h = conj(wavelet(N, a))[::-1] as N interleaved complex doubles.  morlet2: sqrt(1 / s) pi^(-1/4) exp(i w t) exp(-t^2 / 2),
// t = (j - (N - 1) / 2) / s; ricker: 2 / (sqrt(3 a) pi^(1/4)) (1 - v^2 / a^2) exp(-v^2 / (2 a^2)), v = j - (N - 1) / 2
inline void cwt_wavelet(int32_t wavelet, double a, double w, int64_t N, double* out) {
  const double pi = 3.14159265358979323846;
  const double mid = (double)(N - 1) / 2.0;
  for (int64_t j = 0; j < N; ++j) {
    const int64_t src = N - 1 - j;   // reversed
    if (wavelet == kCwMorlet2) {
      const double t = ((double)src - mid) / a;
      const double g = std::sqrt(1.0 / a) * std::pow(pi, -0.25) * std::exp(-0.5 * t * t);
      out[2 * j] = g * std::cos(w * t);
      out[2 * j + 1] = -(g * std::sin(w * t));   // conjugated
    } else {
      const double v = (double)src - mid;
      const double A = 2.0 / (std::sqrt(3.0 * a) * std::pow(pi, 0.25));
      const double wsq = a * a, xsq = v * v;
      out[2 * j] = A * (1.0 - xsq / wsq) * std::exp(-xsq / (2.0 * wsq));
      out[2 * j + 1] = 0.0;
    }
  }
}

// ---- "same" alignment: out[n] = full[n + (N - 1) / 2], full[m] = sum_k x[k] h[m - k]
NXSIG_CW_HD int64_t cwt_center(int64_t N) { return (N - 1) / 2; }

// ---- the classes
inline int cwt_class(int64_t N, bool wave_off) { return (wave_off || N > 1025) ? kCwGeneric : (N <= 513 ? kCwWave1024 : kCwWave2048); }
inline int cwt_class_points(int cls) { return cls == kCwWave1024 ? 1024 : 2048; }
inline const char* cwt_class_name(int cls) { return cls == kCwGeneric ? "cwt.generic" : "cwt.wave"; }

// ---- overlap-save on K points, one geometry per class (Nmax: the longest support of the class).  Written as
// out[n] = sum_i g[i] x[n - i], g[i] = h[i + c], -c <= i <= N - 1 - c, c = cwt_center(N), every filter is a two-sided one placed
// circularly in the K points (cwt_spectrum).  A block that holds the samples base .. base + K - 1 then yields position t of the circular
// result free of wrap-around for N - 1 - c <= t <= K - 1 - c; N - 1 - c = ceil((N - 1) / 2) and c both grow with N, so the run
// cwt_lead(Nmax) <= t < cwt_lead(Nmax) + cwt_step(K, Nmax) is valid for every filter of the class, and out[base + t] is its value
NXSIG_CW_HD int64_t cwt_step(int64_t K, int64_t Nmax) { return K - Nmax + 1; }
NXSIG_CW_HD int64_t cwt_lead(int64_t Nmax) { return Nmax - 1 - cwt_center(Nmax); }
NXSIG_CW_HD int64_t cwt_blocks_per_row(int64_t length, int64_t step) { return (length + step - 1) / step; }
// first sample of block b (negative in the first block: zeros stand in for what lies before the row)
NXSIG_CW_HD int64_t cwt_block_base(int64_t b, int64_t step, int64_t lead) { return b * step - lead; }

// the fused kernel, K = 64 P points per wave: lane l holds the ADJACENT positions t0 and t0 + 1 of each 128-position slot q going in and
// coming out (what wave_fft_core_T consumes and wave_fft_core produces), and bin cwt_bin(l, s) in register s in between
NXSIG_CW_HD int cwt_slot_pos(int lane, int q) { return 2 * lane + 128 * q; }
NXSIG_CW_HD int cwt_bin(int lane, int s) { return lane + 64 * s; }
// position t of a block is output n = base + t when it lies in the valid run and inside the row
NXSIG_CW_HD bool cwt_pos_valid(int64_t t, int64_t base, int64_t lead, int64_t step, int64_t length) {
  return t >= lead && t < lead + step && base + t >= 0 && base + t < length;
}
inline int cwt_waves(int K) { return K == 2048 ? 2 : 4; }
inline int64_t cwt_lds_bytes(int K) { return (int64_t)(256 + (K / 256) * 256 + cwt_waves(K) * (K + K / 16 + 16)) * 8; }
// cwt.generic: the rows are zero-padded to the next power of two >= L + Nmax - 1
inline int64_t cwt_generic_length(int64_t length, int64_t Nmax) {
  int64_t P = 1;
  while (P < length + Nmax - 1) P <<= 1;
  return P;
}

// ---- the K-point spectrum of one filter, f32 interleaved: the taps (N interleaved complex doubles) placed at (j - shift) mod K,
// transformed in double, times `scale`, rounded once.  cwt.wave: shift = cwt_center(N), scale = 1 / K (its inverse core is unscaled);
// cwt.generic: shift = 0, scale = 1
inline void cwt_spectrum(const double* taps, int64_t N, int64_t K, int64_t shift, double scale, std::vector<double>& work, float* out) {
  work.assign((size_t)2 * K, 0.0);
  for (int64_t j = 0; j < N; ++j) {
    const int64_t at = ((j - shift) % K + K) % K;
    work[2 * at] += taps[2 * j]; work[2 * at + 1] += taps[2 * j + 1];
  }
  czt_fft_f64(work.data(), K);
  for (int64_t i = 0; i < 2 * K; ++i) out[i] = (float)(work[i] * scale);
}

// ---- the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: well formed but
// beyond what is built
inline const char* cwt_rows_check(int64_t length, int64_t batch, int64_t batch_stride, int32_t kind, bool* unsupported) {
  *unsupported = false;
  if (kind < kCwComplex || kind > kCwPower) return "kind must be NXSIG_CWT_COMPLEX, _REAL, _MAGNITUDE or _POWER";
  if (length < 1) return "length must be >= 1";
  if (batch < 1 || batch > kCwtMaxBatch) return "batch must be in [1, 65535]";
  if (batch_stride < length) return "batch_stride must be >= length";
  return nullptr;
}
inline const char* cwt_bank_check(int64_t length, int32_t taps_complex, const int64_t* tap_counts, int64_t num_filters, int64_t* total,
                                  int64_t* longest, bool* unsupported) {
  *unsupported = false;
  if (taps_complex != 0 && taps_complex != 1) return "taps_complex must be 0 or 1";
  if (num_filters < 1 || num_filters > kCwtMaxFilters) return "num_filters must be in [1, 4096]";
  int64_t sum = 0, top = 0;
  for (int64_t s = 0; s < num_filters; ++s) {
    if (tap_counts[s] < 1) return "every tap count must be >= 1";
    if (tap_counts[s] > kCwtMaxExtent) { *unsupported = true; return "length + max taps - 1 must be at most 2^24"; }
    sum += tap_counts[s];
    if (tap_counts[s] > top) top = tap_counts[s];
  }
  if (length + top - 1 > kCwtMaxExtent) { *unsupported = true; return "length + max taps - 1 must be at most 2^24"; }
  *total = sum; *longest = top;
  return nullptr;
}
inline bool cwt_all_finite(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
inline const char* cwt_widths_check(int32_t wavelet, const double* widths, int64_t num_widths, double w) {
  if (wavelet != kCwMorlet2 && wavelet != kCwRicker) return "wavelet must be NXSIG_CWT_MORLET2 or NXSIG_CWT_RICKER";
  if (num_widths < 1 || num_widths > kCwtMaxFilters) return "num_widths must be in [1, 4096]";
  for (int64_t s = 0; s < num_widths; ++s)
    if (!std::isfinite(widths[s]) || !(widths[s] > 0.0)) return "every width must be positive and finite";
  if (wavelet == kCwMorlet2 && !std::isfinite(w)) return "w must be finite";
  return nullptr;
}

// ---- a bank split into its classes: the filters of class k, in bank order, and the longest support among them
struct CwtGroups {
  std::vector<int32_t> members[kCwClasses];
  int64_t longest[kCwClasses] = {0, 0, 0};
};
inline void cwt_split(const int64_t* tap_counts, int64_t num_filters, bool wave_off, CwtGroups* g) {
  for (int k = 0; k < kCwClasses; ++k) { g->members[k].clear(); g->longest[k] = 0; }
  for (int64_t s = 0; s < num_filters; ++s) {
    const int k = cwt_class(tap_counts[s], wave_off);
    g->members[k].push_back((int32_t)s);
    if (tap_counts[s] > g->longest[k]) g->longest[k] = tap_counts[s];
  }
}

}  // namespace nxsig
