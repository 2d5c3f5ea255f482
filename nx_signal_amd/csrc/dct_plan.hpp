// Transforms.dct / idct: everything of them that is plain C++ — the argument checks, the norm factors, the tier
// choice, the cosine and twiddle tables (built in double from an integer argument that is reduced before cos is taken) and the launch
// geometry of the direct kernel.  The C entry point, the kernels of kernels_dct.hip and the stand-alone program tests/san_dct.cpp
// (ASan / UBSan on the host) all use this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NXSIG_DCT_HD __host__ __device__ __forceinline__
#else
#define NXSIG_DCT_HD inline
#endif

namespace nxsig {

// norm: 0 None / "backward", 1 "ortho", 2 "forward" (scipy.fft's names)
enum DctNorm : int32_t { kDctBackward = 0, kDctOrtho = 1, kDctForward = 2, kDctNorms = 3 };
enum DctTier : int32_t { kDctDirect = 0, kDctFft = 1 };
constexpr int64_t kDctDirectMax = 256;   // dct.direct takes n <= 256
constexpr int kDctThreads = 256;         // threads of a workgroup of the direct kernel
constexpr int kDctRR = 8;                // rows a thread of the direct kernel accumulates at once
constexpr int kDctLdsFloats = 8192;      // LDS image of a tile of rows, in floats (32 KB)

// samples of a row the transform takes: the row is truncated or zero-padded to n
NXSIG_DCT_HD int64_t dct_used(int64_t length, int64_t n) { return length < n ? length : n; }

// the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: the arguments are well
// formed but beyond what is built (types 1 and 4, n of 2^31 and more, byte counts that overflow)
inline const char* dct_check(int64_t length, int64_t batch, int64_t batch_stride, int64_t n, int32_t type, int32_t norm, int64_t keep,
                             bool* unsupported) {
  *unsupported = false;
  if (length < 1) return "length must be >= 1";
  if (n < 1) return "n must be >= 1";
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < length) return "batch_stride must be >= length";
  if (type == 1 || type == 4) { *unsupported = true; return type == 1 ? "type 1 is not built (types 2 and 3 are)" : "type 4 is not built (types 2 and 3 are)"; }
  if (type != 2 && type != 3) return "type must be 2 or 3";
  if (norm < 0 || norm >= kDctNorms) return "norm must be 0 (backward), 1 (ortho) or 2 (forward)";
  if (keep < 1 || keep > n) return "keep must be in [1, n]";
  *unsupported = true;
  if (n > 0x7fffffffLL) return "n must be below 2^31";
  // the byte counts: the input rows, and batch spectra of n c64 (the widest temporary) with room to spare
  if (batch > 0 && (batch_stride > INT64_MAX / batch / 16 || n > INT64_MAX / batch / 32)) return "the rows are too large";
  *unsupported = false;
  return nullptr;
}

inline int dct_tier(int64_t n, bool direct_off) { return (!direct_off && n <= kDctDirectMax) ? kDctDirect : kDctFft; }

// ---- the norm.  Type 2 scales its OUTPUTS: y[0] by out0, y[k > 0] by out1.  Type 3 scales its INPUTS: x[0] by in0, x[j > 0] by in1
struct DctScale { double a0, a1; };
inline DctScale dct_scale(int64_t n, int32_t norm) {
  const double N = (double)n;
  if (norm == kDctOrtho) return {std::sqrt(1.0 / (4.0 * N)), std::sqrt(1.0 / (2.0 * N))};   // type 3: x[0] / sqrt(n) = 2 a0 x[0], sqrt(2 / n) = 2 a1
  if (norm == kDctForward) return {1.0 / (2.0 * N), 1.0 / (2.0 * N)};
  return {1.0, 1.0};
}

// cos(pi m / (2 n)) for an integer m >= 0: m is reduced mod 4 n and folded into [0, n] before the one call of cos, so the argument
// of cos is never the rounded product of a large k (2 j + 1) — and m = n, an odd multiple of pi / 2, gives an exact zero
inline double dct_cos(int64_t m, int64_t n) {
  m %= 4 * n;
  if (m > 2 * n) m = 4 * n - m;
  double sign = 1.0;
  if (m > n) { sign = -1.0; m = 2 * n - m; }
  if (m == n) return 0.0;
  if (m == 0) return sign;
  return sign * std::cos(M_PI * (double)m / (2.0 * (double)n));
}

// ---- dct.direct: the table Tt[j][k], j < n, k < keep (k fastest: the lanes of a wave hold consecutive k), norm folded in
//   type 2   Tt[j][k] = 2 a_k cos(pi k (2 j + 1) / (2 n))
//   type 3   Tt[0][k] = a0' and Tt[j][k] = 2 a1' cos(pi (2 k + 1) j / (2 n)), with a0' = 2 a0 (ortho), a0 (otherwise): x[0] enters once
inline std::vector<float> dct_direct_table(int64_t n, int64_t keep, int32_t type, int32_t norm) {
  std::vector<float> t((size_t)n * (size_t)keep);
  const DctScale s = dct_scale(n, norm);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t k = 0; k < keep; ++k) {
      double v;
      if (type == 2) v = 2.0 * (k == 0 ? s.a0 : s.a1) * dct_cos(k * (2 * j + 1), n);
      else if (j == 0) v = norm == kDctOrtho ? 2.0 * s.a0 : s.a0;
      else v = 2.0 * s.a1 * dct_cos((2 * k + 1) * j, n);
      t[(size_t)j * keep + k] = (float)v;
    }
  return t;
}
// type 2 transforms row - c and adds c times this to y[0]: the sum of the table's k = 0 column is 2 n a0 (every other column sums to 0)
inline float dct_dc_gain(int64_t n, int32_t norm) { return (float)(2.0 * (double)n * dct_scale(n, norm).a0); }

// ---- dct.fft: the twiddles e^{i pi k / (2 n)} = (cos, sin), k < n, as interleaved f32 pairs, norm folded in
//   type 2   tw[k] = 2 a_k (cos, sin):            y[k] = tw[k].x Re V[k] + tw[k].y Im V[k]           (2 Re(e^{-i pi k / 2n} V[k]))
//   type 3   W[0] = tw[0].x x[0] and W[k] = tw[k] (x[k] - i x[n - k]): a Hermitian spectrum whose inverse transform, un-permuted, is y.
//            tw[0] = (n a0', 0), tw[k > 0] = n a1 (cos, sin): the n undoes the inverse transform's 1 / n, and the definition's
//            2 x[j] cos is what the pair W[j], W[n - j] adds up to
inline std::vector<float> dct_fft_table(int64_t n, int32_t type, int32_t norm) {
  std::vector<float> t((size_t)n * 2);
  const DctScale s = dct_scale(n, norm);
  for (int64_t k = 0; k < n; ++k) {
    double g;
    if (type == 2) g = 2.0 * (k == 0 ? s.a0 : s.a1);
    else if (k == 0) g = (double)n * (norm == kDctOrtho ? 2.0 * s.a0 : s.a0);
    else g = (double)n * s.a1;
    t[(size_t)2 * k] = (float)(g * dct_cos(k, n));
    t[(size_t)2 * k + 1] = (float)(g * dct_cos(n - k, n));   // sin(pi k / 2n) = cos(pi (n - k) / 2n)
  }
  return t;
}

// Makhoul's permutation: v[i] = x[dct_perm(i, n)], i.e. v[j] = x[2 j], v[n - 1 - j] = x[2 j + 1]; type 3 leaves through its inverse,
// y[m] = u[dct_unperm(m, n)]
NXSIG_DCT_HD int64_t dct_perm(int64_t i, int64_t n) { return i < (n + 1) / 2 ? 2 * i : 2 * (n - 1 - i) + 1; }

NXSIG_DCT_HD int64_t dct_unperm(int64_t m, int64_t n) { return (m & 1) ? n - 1 - (m - 1) / 2 : m / 2; }

// ---- dct.direct: the geometry.  A workgroup takes a tile of groups * kDctRR rows into LDS, row r at r * pitch; thread t < groups *
// keep owns coefficient k = t % keep of the rows g + groups * rr, g = t / keep, rr < kDctRR.  pitch: at least n + 1 (the float after a
// row keeps its mean), a multiple of 4 (16-byte LDS reads) and an odd number of 16-byte units (the groups a wave spans read different
// banks)
// the direct kernel's row mean: lane q of four sums the units [dct_quarter(q), dct_quarter(q + 1)) of a row (16-byte units when n is
// a multiple of 4, single samples otherwise), and the four partial sums add up as (p0 + p1) + (p2 + p3)
NXSIG_DCT_HD int dct_quarter(int q, int units) { return (q * units) >> 2; }
struct DctGeom { int32_t pitch, groups, tile_rows; int64_t tiles; };
inline DctGeom dct_geom(int64_t n, int64_t keep, int64_t batch) {
  DctGeom g;
  int64_t p = (n + 1 + 3) / 4 * 4;
  if (((p / 4) & 1) == 0) p += 4;
  g.pitch = (int32_t)p;
  int64_t by_threads = kDctThreads / keep, by_lds = kDctLdsFloats / (kDctRR * p);
  int64_t groups = by_threads < by_lds ? by_threads : by_lds;
  if (groups < 1) groups = 1;
  g.groups = (int32_t)groups;
  g.tile_rows = (int32_t)(groups * kDctRR);
  g.tiles = (batch + g.tile_rows - 1) / g.tile_rows;
  return g;
}

}  // namespace nxsig
