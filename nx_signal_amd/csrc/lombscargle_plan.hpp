// Spectral.lombscargle: everything of it that is plain C++ — the blocking sizes, the argument checks, the
// normalised weights, the tier choice and the grid arithmetic.  The C entry point and the kernels of kernels_lombscargle.hip use this
// one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace nxsig {

// normalize: scipy's False / "power", True / "normalize", "amplitude"
enum LsNormalize : int32_t { kLsPower = 0, kLsNormalize = 1, kLsAmplitude = 2, kLsNormalizes = 3 };
enum LsTier : int32_t { kLsTile = 0, kLsGeneric = 1 };

constexpr int kLsFB = 64;       // frequencies per workgroup of lombscargle.tile: one per lane of its one wave
constexpr int kLsRB = 8;        // rows per workgroup: two running sums per row and lane stay in registers
constexpr int kLsTT = 128;      // samples per staged tile: (2 + kLsRB) * kLsTT doubles of LDS = 10 KB, four workgroups per SIMD
constexpr int kLsGenericThreads = 256;
// scipy: np.finfo(np.float64).epsneg, the floor of the shifted CC and SS
constexpr double kLsEpsNeg = 1.1102230246251565e-16;

inline int32_t ls_block(int32_t which) { return which == 0 ? kLsFB : which == 1 ? kLsRB : which == 2 ? kLsTT : 0; }

// the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: well formed but beyond
// what is built (byte counts or grids that overflow)
inline const char* ls_check_shape(int32_t dtype, int64_t n, int32_t batch, int64_t batch_stride, int64_t num_freqs, int32_t precenter,
                                  int32_t normalize, int32_t floating_mean, bool* unsupported) {
  *unsupported = false;
  if (dtype != 0 && dtype != 1) return "dtype must be NXSIG_DT_F32 or NXSIG_DT_F64";
  if (n < 1) return "Parameters x, y, weights must be 1-D arrays of equal non-zero length!";
  if (num_freqs < 1) return "Parameter freqs must be a 1-D array of non-zero length!";
  if (batch < 1) return "batch must be >= 1";
  if (batch_stride < n) return "batch_stride must be >= n";
  if (precenter != 0 && precenter != 1) return "precenter must be 0 or 1";
  if (normalize < 0 || normalize >= kLsNormalizes) return "Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'.";
  if (floating_mean != 0 && floating_mean != 1) return "floating_mean must be 0 or 1";
  *unsupported = true;
  if (n > INT64_MAX / 16 || num_freqs > INT64_MAX / 16) return "the rows are too large";
  if (batch_stride > INT64_MAX / batch / 16 || num_freqs > INT64_MAX / batch / 32) return "the rows are too large";
  const int64_t fblocks = (num_freqs + kLsFB - 1) / kLsFB, rblocks = ((int64_t)batch + kLsRB - 1) / kLsRB;
  if (fblocks > 0x7fffffffLL / rblocks) return "the result is too large for one launch";
  *unsupported = false;
  return nullptr;
}

// the three host arrays: finite times and frequencies; finite, non-negative weights with a positive sum (scipy's sentence)
inline const char* ls_check_arrays(const double* x, int64_t n, const double* freqs, int64_t num_freqs, const double* weights) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return "x must be finite";
  for (int64_t i = 0; i < num_freqs; ++i)
    if (!std::isfinite(freqs[i])) return "freqs must be finite";
  if (weights) {
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      if (!std::isfinite(weights[i])) return "weights must be finite";
      if (!(weights[i] >= 0.0)) return "Parameter weights must have only non-negative entries which sum to a positive value!";
      sum += weights[i];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return "Parameter weights must have only non-negative entries which sum to a positive value!";
  }
  return nullptr;
}

// scipy: weights *= 1.0 / weights.sum(), ones where none are given.  The sum runs in ascending order
inline std::vector<double> ls_weights(const double* weights, int64_t n) {
  std::vector<double> w((size_t)n);
  double sum = 0.0;
  for (int64_t i = 0; i < n; ++i) sum += (w[(size_t)i] = weights ? weights[i] : 1.0);
  const double inv = 1.0 / sum;
  for (int64_t i = 0; i < n; ++i) w[(size_t)i] *= inv;
  return w;
}

// the tier is a rule of the shape, the options and the switch alone, never of the batch: lombscargle.tile takes every shape and
// option set, lombscargle.generic runs under NXSIG_LOMBSCARGLE_TILE=0
inline int ls_tier(int64_t /*n*/, int64_t /*num_freqs*/, int32_t /*normalize*/, int32_t /*floating_mean*/, bool tile_on) {
  return tile_on ? kLsTile : kLsGeneric;
}

inline size_t ls_out_elem(int32_t dtype, int32_t normalize) { return (dtype ? 8u : 4u) * (normalize == kLsAmplitude ? 2u : 1u); }

}  // namespace nxsig
