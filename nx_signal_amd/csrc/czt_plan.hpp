// Transforms.czt / zoom_fft: everything of it that is plain C++ — the argument checks, the tier choice, the
// convolution length L, the exact phase reduction, the builder of the three tables A, F and W, and the row and lane arithmetic of the
// fused kernel.  The C entry points, the kernels of kernels_czt.hip and the stand-alone program tests/san_czt.cpp (ASan / UBSan on the
// host) all use this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NXSIG_CZ_HD __host__ __device__ __forceinline__
#else
#define NXSIG_CZ_HD inline
#endif

namespace nxsig {

enum CztTier : int32_t { kCzWave = 0, kCzGeneric = 1 };

// ---- the definition (include/nxsig.h): X[k] = sum_{j<n} x[j] a^(-j) w^(j k), w = w_abs exp(-2 pi i w_step / w_den),
// a = a_abs exp(2 pi i a_turns).  Angles are turns; the step is a double over a positive integer
struct CztContour {
  double w_abs, w_step;
  int64_t w_den;
  double a_abs, a_turns;
};

// The spiral gate: a contour with |w| != 1 or |a| != 1 is accepted while the spread max|t| / min|t| of each of the three chirps (A, W
// and the kernel v that F is the transform of) stays at or under this.  Measured on the host emulation (tests/test_czt_host.py,
// test_the_spiral_gate_is_the_measured_one: the single-precision scheme built from the tables against the definition in double, on the
// recorded spiral sweep: sixteen rows each of n = m = 64 and n = 600, m = 300, |w| on either side of 1 at spreads 4, 8, 16, 32, 64).
// The worst row stays under 1e-6 of the row maximum, a decade under the 1e-5 bar, up to a spread of 32 (4.7e-7 at 16, 8.3e-7 at 32,
// both n = 600 with |w| < 1) and is over it at 64 (1.6e-6, the same case; other rows read 1.0e-5 at 512).  The error grows in
// proportion to the spread on the |w| < 1 side, where the convolution is formed at the scale of the largest chirp entry and handed out
// at the scale of the smallest; |w| > 1 stays at 2e-7 to 4e-7 throughout, but one gate serves both.  DESIGN.md section 3.20 keeps the sweep
constexpr double kCztSpreadGate = 32.0;

// ---- the tier and the convolution length.  czt.wave runs both transforms of a row inside one wave at L = 1024 or 2048 points, so it
// takes n + m - 1 <= 2048; everything else, and everything with the wave tier switched off, is czt.generic at the next power of two
inline int64_t czt_need(int64_t n, int64_t m) { return n + m - 1; }
inline int czt_tier(int64_t n, int64_t m, bool wave_off) { return (!wave_off && czt_need(n, m) <= 2048) ? kCzWave : kCzGeneric; }
inline int64_t czt_conv_length(int64_t n, int64_t m, bool wave_off) {
  const int64_t need = czt_need(n, m);
  if (czt_tier(n, m, wave_off) == kCzWave) return need <= 1024 ? 1024 : 2048;
  int64_t L = 1;
  while (L < need) L <<= 1;
  return L;
}
inline bool czt_is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
// waves per workgroup, LDS and workgroups of czt.wave: the layout and the budget of hilbert.wave (hilbert_plan.hpp)
inline int czt_waves(int L) { return L == 2048 ? 2 : 4; }
inline int64_t czt_lds_bytes(int L) { return (int64_t)(256 + (L / 256) * 256 + czt_waves(L) * (L + L / 16 + 16)) * 8; }
inline int64_t czt_blocks(int64_t rows, int64_t chunk) { return (rows + chunk - 1) / chunk; }

// ---- the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: the arguments are well
// formed but beyond what is built
inline const char* czt_check(int32_t is_complex, int64_t length, int64_t batch, int64_t batch_stride, int64_t m, const CztContour& c,
                             bool* unsupported) {
  *unsupported = false;
  if (is_complex != 0 && is_complex != 1) return "is_complex must be 0 or 1";
  if (length < 1) return "length must be >= 1";
  if (m < 1) return "m must be >= 1";
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < length) return "batch_stride must be >= length";
  if (c.w_den < 1) return "w_den must be >= 1";
  if (!(c.w_abs > 0.0) || !std::isfinite(c.w_abs)) return "w_abs must be positive and finite";
  if (!(c.a_abs > 0.0) || !std::isfinite(c.a_abs)) return "a_abs must be positive and finite";
  if (!std::isfinite(c.w_step)) return "w_step must be finite";
  if (!std::isfinite(c.a_turns)) return "a_turns must be finite";
  *unsupported = true;
  if (length > ((int64_t)1 << 30) || m > ((int64_t)1 << 30) || czt_need(length, m) > ((int64_t)1 << 30)) return "n + m - 1 must be at most 2^30";
  if (c.w_den > ((int64_t)1 << 61)) return "w_den must be at most 2^61";
  // the byte counts: the input rows (c64 at the widest), and batch padded rows of L <= 2^30 c64, twice, with room to spare
  if (batch > 0 && (batch_stride > INT64_MAX / batch / 16 || ((int64_t)1 << 31) > INT64_MAX / batch / 32)) return "the rows are too large";
  *unsupported = false;
  return nullptr;
}
// two byte ranges share a byte
inline bool czt_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uint64_t pa = (uint64_t)reinterpret_cast<uintptr_t>(a), pb = (uint64_t)reinterpret_cast<uintptr_t>(b);
  return a_bytes > 0 && b_bytes > 0 && pa < pb + b_bytes && pb < pa + a_bytes;
}

// ---- the phase reduction.  Every phase of the three tables is an integer multiple (j, j^2 < 2^62) of a fixed fraction of a turn, so
// the fraction is kept as a 128-bit binary fraction F = floor(frac(value / den) 2^128) and the multiple is a wrapping 128-bit product:
// (j^2 F) mod 2^128 IS frac(j^2 F / 2^128) 2^128, exactly.  What is lost is the tail of F alone: under 2^62 2^-128 = 2^-66 of a turn
typedef unsigned __int128 czt_u128;

inline uint64_t czt_pow2_mod(int e, uint64_t den) {   // 2^e mod den, e >= 0
  czt_u128 r = 1 % den, b = 2 % den;
  for (; e > 0; e >>= 1) {
    if (e & 1) r = r * b % den;
    b = b * b % den;
  }
  return (uint64_t)r;
}

inline czt_u128 czt_turn_fraction(double value, uint64_t den) {
  if (value == 0.0 || !std::isfinite(value) || den == 0) return 0;
  int e = 0;
  const double mant = std::frexp(std::fabs(value), &e);     // |value| = mant 2^e, mant in [0.5, 1)
  const uint64_t M = (uint64_t)std::ldexp(mant, 53);        // |value| = M 2^(e - 53), exactly
  e -= 53;
  // Q = floor(N 2^128 / den) in three 64-bit limbs, N = M (e < 0: the shift comes afterwards) or (M 2^e) mod den
  uint64_t limb[5] = {0, 0, 0, 0, 0};
  czt_u128 r;
  if (e >= 0) {
    r = (czt_u128)(M % den) * czt_pow2_mod(e, den) % den;
  } else {
    limb[2] = M / den;
    r = M % den;
  }
  limb[1] = (uint64_t)((r << 64) / den); r = (r << 64) % den;
  limb[0] = (uint64_t)((r << 64) / den);
  uint64_t lo = limb[0], hi = limb[1];
  if (e < 0) {
    const int t = -e;
    if (t >= 192) return 0;
    const int ws = t / 64, bs = t % 64;
    lo = limb[ws] >> bs; hi = limb[ws + 1] >> bs;
    if (bs) { lo |= limb[ws + 1] << (64 - bs); hi |= limb[ws + 2] << (64 - bs); }
  }
  const czt_u128 f = ((czt_u128)hi << 64) | lo;
  return value < 0.0 ? (czt_u128)0 - f : f;
}
// a reduced phase as an angle in [-pi, pi): the leading 64 bits, signed
inline double czt_angle(czt_u128 p) {
  return 6.283185307179586476925286766559 * ((double)(int64_t)(uint64_t)(p >> 64) * 5.421010862427522170037264004349e-20);   // 2^-64
}
inline void czt_polar(double mag, czt_u128 phase, double* re, double* im) {
  const double ang = czt_angle(phase);
  *re = mag * std::cos(ang); *im = mag * std::sin(ang);
}

// in-place radix-2 transform of L = 2^k interleaved complex doubles, exp(-2 pi i j k / L); the twiddles are evaluated one by one
inline void czt_fft_f64(double* z, int64_t L) {
  for (int64_t i = 1, j = 0; i < L; ++i) {
    int64_t bit = L >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { const double tr = z[2 * i], ti = z[2 * i + 1]; z[2 * i] = z[2 * j]; z[2 * i + 1] = z[2 * j + 1]; z[2 * j] = tr; z[2 * j + 1] = ti; }
  }
  std::vector<double> tw((size_t)(L > 1 ? L : 2));
  for (int64_t k = 0; k < L / 2; ++k) {
    const double ang = -6.283185307179586476925286766559 * (double)k / (double)L;
    tw[2 * k] = std::cos(ang); tw[2 * k + 1] = std::sin(ang);
  }
  for (int64_t len = 2; len <= L; len <<= 1) {
    const int64_t half = len / 2, step = L / len;
    for (int64_t i = 0; i < L; i += len)
      for (int64_t k = 0; k < half; ++k) {
        const double wr = tw[2 * k * step], wi = tw[2 * k * step + 1];
        double* u = z + 2 * (i + k);
        double* v = z + 2 * (i + k + half);
        const double xr = v[0] * wr - v[1] * wi, xi = v[0] * wi + v[1] * wr;
        v[0] = u[0] - xr; v[1] = u[1] - xi; u[0] += xr; u[1] += xi;
      }
  }
}

// ---- the spread of a contour: the largest max|t| / min|t| among A, W and the kernel v (entry 0 of each is 1, so a spread within the
// gate keeps every entry finite and normal in f32).  ln|W[k]| = k^2 ln|w| / 2 and ln|v[j]| = -j^2 ln|w| / 2 are monotonic in |j|;
// ln|A[j]| = j^2 ln|w| / 2 - j ln|a| is a parabola, whose extremes over the integers lie at the ends or beside its vertex
inline double czt_spread(int64_t n, int64_t m, const CztContour& c) {
  const double lw = c.w_abs == 1.0 ? 0.0 : std::log(c.w_abs), la = c.a_abs == 1.0 ? 0.0 : std::log(c.a_abs);
  if (lw == 0.0 && la == 0.0) return 1.0;
  const double top = (double)((n > m ? n : m) - 1);
  double worst = std::fabs(0.5 * top * top * lw);        // v over (-n, m), and W within it
  double lo = 0.0, hi = 0.0;
  auto visit = [&](double j) {
    if (j < 0.0 || j > (double)(n - 1)) return;
    const double g = 0.5 * j * j * lw - j * la;
    if (g < lo) lo = g;
    if (g > hi) hi = g;
  };
  visit((double)(n - 1));
  if (lw != 0.0) { const double v = std::floor(la / lw); visit(v); visit(v + 1.0); }
  if (hi - lo > worst) worst = hi - lo;
  return std::exp(worst);   // Inf or NaN beyond double: refused like any spread over the gate
}

// ---- the three tables, interleaved complex doubles:
//   A[j] = a^(-j) w^(j^2 / 2), j < n        applied to the samples
//   F    = DFT_L(v) / L, v[j mod L] = w^(-j^2 / 2) for j in (-n, m), zero elsewhere (L >= n + m - 1, a power of two)
//   W[k] = w^(k^2 / 2), k < m               applied to the first m points of the convolution
// *spread: the largest max|t| / min|t| among A, v and W.  Returns nullptr, or the reason the contour is not served
inline const char* czt_tables(int64_t n, int64_t m, int64_t L, const CztContour& c, double* A, double* F, double* W, double* spread) {
  const czt_u128 fw = czt_turn_fraction(c.w_step, 2 * (uint64_t)c.w_den);   // w_step / (2 w_den) of a turn, per unit of j^2
  const czt_u128 fa = czt_turn_fraction(c.a_turns, 1);
  const double lw = c.w_abs == 1.0 ? 0.0 : std::log(c.w_abs), la = c.a_abs == 1.0 ? 0.0 : std::log(c.a_abs);
  const double worst = czt_spread(n, m, c);
  if (spread) *spread = worst;
  if (!(worst <= kCztSpreadGate)) return "the contour leaves single precision";
  for (int64_t j = 0; j < n; ++j) {
    const czt_u128 j2 = (czt_u128)(uint64_t)j * (uint64_t)j;
    const double mag = (lw == 0.0 && la == 0.0) ? 1.0 : std::exp(0.5 * (double)j * (double)j * lw - (double)j * la);
    czt_polar(mag, (czt_u128)0 - (czt_u128)(uint64_t)j * fa - j2 * fw, &A[2 * j], &A[2 * j + 1]);
  }
  for (int64_t k = 0; k < m; ++k) {
    const czt_u128 k2 = (czt_u128)(uint64_t)k * (uint64_t)k;
    const double mag = lw == 0.0 ? 1.0 : std::exp(0.5 * (double)k * (double)k * lw);
    czt_polar(mag, (czt_u128)0 - k2 * fw, &W[2 * k], &W[2 * k + 1]);
  }
  for (int64_t i = 0; i < 2 * L; ++i) F[i] = 0.0;
  for (int64_t j = -(n - 1); j < m; ++j) {
    const uint64_t aj = (uint64_t)(j < 0 ? -j : j);
    const czt_u128 j2 = (czt_u128)aj * aj;
    const double mag = lw == 0.0 ? 1.0 : std::exp(-0.5 * (double)aj * (double)aj * lw);
    const int64_t at = j < 0 ? j + L : j;
    czt_polar(mag, j2 * fw, &F[2 * at], &F[2 * at + 1]);
  }
  czt_fft_f64(F, L);
  const double inv = 1.0 / (double)L;
  for (int64_t i = 0; i < 2 * L; ++i) F[i] *= inv;
  return nullptr;
}

// ---- the fused kernel, L = 64 P points per wave.  Going in, lane l holds the ADJACENT samples i0 and i0 + 1 of each 128-sample slot q:
// i0 = czt_slot_sample(l, q) (what wave_fft_core_T consumes and wave_fft_core produces, so the results leave in the same layout)
NXSIG_CZ_HD int czt_slot_sample(int lane, int q) { return 2 * lane + 128 * q; }
// how many of the two elements lie inside the `count` elements a row holds (n going in, m going out): 2 both, 1 the first alone,
// 0 neither; nothing at or past `count` is ever read or written
NXSIG_CZ_HD int czt_pair_state(int i0, int count) { return i0 + 1 < count ? 2 : (i0 < count ? 1 : 0); }
// between the two transforms lane l holds bin czt_bin(l, s) in register s, and multiplies it by F[czt_bin(l, s)]
NXSIG_CZ_HD int czt_bin(int lane, int s) { return lane + 64 * s; }
// a row may start at any multiple of its element size: the wide access (one load or store of two adjacent elements) is taken when the
// row starts on twice the element size, the narrow one (element by element) otherwise.  elem: 4 (f32 in), 8 (c64 in or out)
NXSIG_CZ_HD bool czt_wide(uint64_t row_address, int elem) { return (row_address & (uint64_t)(2 * elem - 1)) == 0; }

}  // namespace nxsig
