// Filters.sosfilt / sosfiltfilt: the host side, free of HIP so that a stand-alone program can drive it under a sanitizer
// (tests/san_iir.cpp): the argument checks, the chunk / tile geometry, the state matrix A of a cascade and its powers, scipy's
// sosfilt_zi, the padding of sosfiltfilt.  A cascade of S biquads in transposed direct form II is the linear system
//     s[n + 1] = A s[n] + B x[n],      s = (z0, z1) of section 0, (z0, z1) of section 1, ...            (2 S states)
// A is block lower triangular (a section sees the sections before it only).  Everything is double.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace nxsig {

constexpr int32_t kIirMaxSections = 16;   // one call; longer cascades are split by the caller
constexpr int32_t kIirLanes = 64;         // chunks per tile: one chunk per lane of a wave
constexpr int32_t kIirSub = 32;           // samples of a chunk staged through LDS at a time

// sections a kernel is instantiated for: the cascade is filled up with identity sections (b = a = 1, 0, 0: exact, their state stays 0)
inline int32_t iir_padded_sections(int32_t s) { return s <= 1 ? 1 : s <= 2 ? 2 : s <= 4 ? 4 : s <= 8 ? 8 : 16; }
// samples per lane and per workgroup tile: functions of n_sections only (0 outside 1 .. 16)
inline int32_t iir_chunk(int32_t s) { return s < 1 || s > kIirMaxSections ? 0 : (s <= 2 ? 32 : 64); }
inline int32_t iir_tile(int32_t s) { return iir_chunk(s) * kIirLanes; }

// nullptr, or what is wrong with sos = f64[n_sections][6] (worded after scipy's _validate_sos)
inline const char* iir_check_sos(const double* sos, int32_t n_sections) {
  if (n_sections < 1) return "sos must have at least one section (shape (n_sections, 6))";
  for (int32_t s = 0; s < n_sections; ++s) {
    if (!(sos[6 * s + 3] == 1.0)) return "sos[:, 3] should be all ones";
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(sos[6 * s + k])) return "sos must be finite";
  }
  return nullptr;
}

// nullptr, or what is wrong with the shape arguments of nxsig_sosfilt_f32 (after the null, mem and sos checks)
inline const char* iir_check_args(int64_t length, int32_t batch, int64_t batch_stride, int32_t zi_rows, bool has_zi, int32_t direction) {
  if (batch < 1 || length < 1) return "batch and length must be >= 1";
  if (batch_stride < length) return "batch_stride < length";
  if (has_zi && zi_rows != 1 && zi_rows != batch) return "zi_rows must be 1 or batch";
  if (direction != 0 && direction != 1) return "direction must be 0 (forward) or 1 (backward)";
  return nullptr;
}

// ---- sosfiltfilt: padtype 0 none, 1 odd, 2 even, 3 constant; padlen < 0 asks for scipy's default
inline int32_t iir_default_padlen(const double* sos, int32_t n_sections) {
  int32_t zb = 0, za = 0;
  for (int32_t s = 0; s < n_sections; ++s) { zb += sos[6 * s + 2] == 0.0; za += sos[6 * s + 5] == 0.0; }
  return 3 * (2 * n_sections + 1 - (zb < za ? zb : za));
}
// the edge scipy pads with (>= 0), or -1: padtype unknown, -2: padlen >= length
inline int64_t iir_edge(const double* sos, int32_t n_sections, int32_t padtype, int64_t padlen, int64_t length) {
  if (padtype < 0 || padtype > 3) return -1;
  const int64_t edge = padtype == 0 ? 0 : (padlen < 0 ? iir_default_padlen(sos, n_sections) : padlen);
  return length <= edge ? -2 : edge;
}

// ---- one sample through the cascade, scipy's recurrence; s holds 2 n_sections states
inline double iir_step(const double* sos, int32_t n_sections, double* s, double x) {
  for (int32_t k = 0; k < n_sections; ++k) {
    const double* c = sos + 6 * k;
    const double y = c[0] * x + s[2 * k];
    s[2 * k] = c[1] * x - c[4] * y + s[2 * k + 1];
    s[2 * k + 1] = c[2] * x - c[5] * y;
    x = y;
  }
  return x;
}

// A as a dense row-major n x n matrix, n = 2 n_sections: column c is one step from the unit state e_c with x = 0
inline std::vector<double> iir_state_matrix(const double* sos, int32_t n_sections) {
  const int n = 2 * n_sections;
  std::vector<double> A((size_t)n * n, 0.0), s((size_t)n);
  for (int c = 0; c < n; ++c) {
    for (int r = 0; r < n; ++r) s[r] = r == c ? 1.0 : 0.0;
    iir_step(sos, n_sections, s.data(), 0.0);
    for (int r = 0; r < n; ++r) A[(size_t)r * n + c] = s[r];
  }
  return A;
}

// Powers of A are formed in extended precision (long double: a 64-bit mantissa on x86-64) and rounded to double once.  In double,
// squaring loses about (exponent) x (eigenvector condition) ulps, and a high-pass at 20 Hz / 48 kHz has pole pairs so close to z = 1
// that A is nearly defective: A^2048 came out with 1e-10 relative error, which the zero-state responses it is multiplied with (far
// larger than the settled states they cancel to) turned into 3e-8 in a state.  With the wide powers the scheme stays within 1e-11 of
// the recurrence (tests/san_iir.cpp).
typedef long double iir_wide;

inline std::vector<iir_wide> iir_matmul(const std::vector<iir_wide>& X, const std::vector<iir_wide>& Y, int n) {
  std::vector<iir_wide> Z((size_t)n * n, 0.0L);
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < n; ++k) {
      const iir_wide x = X[(size_t)r * n + k];
      if (x == 0.0L) continue;   // the zero blocks above the diagonal (and 0 * Inf of an overflowed power stays out of them)
      for (int c = 0; c < n; ++c) Z[(size_t)r * n + c] += x * Y[(size_t)k * n + c];
    }
  return Z;
}

// A^e by squaring, e >= 0
inline std::vector<iir_wide> iir_matpow_wide(const std::vector<double>& A0, int n, uint64_t e) {
  std::vector<iir_wide> A(A0.begin(), A0.end()), R((size_t)n * n, 0.0L);
  for (int i = 0; i < n; ++i) R[(size_t)i * n + i] = 1.0L;
  while (e) {
    if (e & 1) R = iir_matmul(R, A, n);
    e >>= 1;
    if (e) A = iir_matmul(A, A, n);
  }
  return R;
}
inline std::vector<double> iir_matpow(const std::vector<double>& A, int n, uint64_t e) {
  const std::vector<iir_wide> R = iir_matpow_wide(A, n, e);
  return std::vector<double>(R.begin(), R.end());
}

// levels of a scan over the 64 lanes of a wave: level k combines with the lane 2^k below through base^(2^k)
constexpr int kIirLevels = 6;

// The matrices a kernel reads, each padded to np x np (np = 2 * padded sections, the padding rows and columns are zero), row-major:
// [0 .. 5] base^(2^k) for k = 0 .. 5, [6] `single`.  For the tile passes base = A^C (single unused: identity);
// for the carry over the tiles of a row base = A^(T R) with R tiles per lane and single = A^T.
inline std::vector<double> iir_scan_matrices(const std::vector<double>& A, int n, int np, uint64_t base_exp, uint64_t single_exp) {
  std::vector<double> out((size_t)(kIirLevels + 1) * np * np, 0.0);
  auto put = [&](int slot, const std::vector<iir_wide>& M) {
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) out[((size_t)slot * np + r) * np + c] = (double)M[(size_t)r * n + c];
  };
  std::vector<iir_wide> P = iir_matpow_wide(A, n, base_exp);
  for (int k = 0; k < kIirLevels; ++k) {
    put(k, P);
    if (k + 1 < kIirLevels) P = iir_matmul(P, P, n);
  }
  put(kIirLevels, iir_matpow_wide(A, n, single_exp));
  return out;
}

// scipy.signal.sosfilt_zi: zi[s] = (running DC gain) * lfilter_zi(b_s, a_s); zi = f64[n_sections][2].  lfilter_zi solves
// (I - A^T) z = B with A the companion matrix of a, i.e. [[1 + a1, -1], [a2, 1]] z = [b1 - a1 b0, b2 - a2 b0]; done here as LAPACK
// does it for scipy, by elimination with partial pivoting (the system of a 20 Hz high-pass has a condition of 1e6, so the order of
// operations shows).  false: a section has a pole at z = 1 (1 + a1 + a2 == 0): the system is singular and there is no settled step
// response (scipy raises LinAlgError)
inline bool iir_sosfilt_zi(const double* sos, int32_t n_sections, double* zi) {
  double scale = 1.0;
  for (int32_t s = 0; s < n_sections; ++s) {
    const double* c = sos + 6 * s;
    const double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[4], a2 = c[5];
    if ((1.0 + a1) + a2 == 0.0) return false;
    double m00 = 1.0 + a1, m01 = -1.0, m10 = a2, m11 = 1.0, r0 = b1 - a1 * b0, r1 = b2 - a2 * b0;
    if (std::fabs(m10) > std::fabs(m00)) {
      double t = m00; m00 = m10; m10 = t;
      t = m01; m01 = m11; m11 = t;
      t = r0; r0 = r1; r1 = t;
    }
    const double l = m10 / m00, u11 = m11 - l * m01;
    if (u11 == 0.0) return false;
    const double z1 = (r1 - l * r0) / u11;
    const double z0 = (r0 - m01 * z1) / m00;
    zi[2 * s] = scale * z0;
    zi[2 * s + 1] = scale * z1;
    scale *= ((b0 + b1) + b2) / ((1.0 + a1) + a2);
  }
  return true;
}

// tiles of a row and the tiles each lane of the carry kernel walks
inline int64_t iir_tiles(int64_t length, int32_t n_sections) { const int64_t T = iir_tile(n_sections); return (length + T - 1) / T; }
inline int64_t iir_tiles_per_lane(int64_t tiles) { return (tiles + kIirLanes - 1) / kIirLanes; }

}  // namespace nxsig
