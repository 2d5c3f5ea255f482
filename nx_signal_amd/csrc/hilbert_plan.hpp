// Filters.hilbert: everything of it that is plain C++ — the argument checks, the multiplier rule of the analytic
// signal, the tier choice, and the row and lane arithmetic of the fused kernel.  The C entry point, the kernels of kernels_hilbert.hip
// and the stand-alone program tests/san_hilbert.cpp (ASan / UBSan on the host) all use this one copy.  No HIP types.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NXSIG_HB_HD __host__ __device__ __forceinline__
#else
#define NXSIG_HB_HD inline
#endif

namespace nxsig {

// nxsig_hilbert_kind of include/nxsig.h
enum HilbertKind : int32_t { kHbAnalytic = 0, kHbEnvelope = 1, kHbQuadrature = 2, kHbKinds = 3 };
enum HilbertTier : int32_t { kHbWave = 0, kHbGeneric = 1 };

// ---- the definition: a = IDFT_N(h DFT_N(row)), h[k] = hilbert_gain(k, N).  The gains of a row sum to N
NXSIG_HB_HD int hilbert_gain(int64_t k, int64_t N) {
  if (k == 0) return 1;
  if ((N & 1) == 0 && k == N / 2) return 1;
  return k < (N + 1) / 2 ? 2 : 0;
}

// samples of a row the transform takes: the row is truncated or zero-padded to n_fft
NXSIG_HB_HD int64_t hilbert_used(int64_t length, int64_t n_fft) { return length < n_fft ? length : n_fft; }
// bytes of one result element
inline int64_t hilbert_out_elem(int32_t kind) { return kind == kHbAnalytic ? 8 : 4; }

// the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: the arguments are well
// formed but beyond what is built
inline const char* hilbert_check(int64_t length, int64_t batch, int64_t batch_stride, int64_t n_fft, int32_t kind, bool* unsupported) {
  *unsupported = false;
  if (length < 1) return "length must be >= 1";
  if (n_fft < 1) return "n_fft must be >= 1";
  if (batch < 0) return "batch must be >= 0";
  if (batch_stride < length) return "batch_stride must be >= length";
  if (kind < 0 || kind >= kHbKinds) return "kind must be NXSIG_HILBERT_ANALYTIC, NXSIG_HILBERT_ENVELOPE or NXSIG_HILBERT_QUADRATURE";
  *unsupported = true;
  if (n_fft > 0x7fffffffLL) return "n_fft must be below 2^31";
  // the byte counts: the input rows, and batch spectra of n_fft c64 (the widest temporary) with room to spare
  if (batch > 0 && (batch_stride > INT64_MAX / batch / 16 || n_fft > INT64_MAX / batch / 32)) return "the rows are too large";
  *unsupported = false;
  return nullptr;
}

// ---- the tier: hilbert.wave transforms 1024 and 2048 points inside one wave; every other length, and every length with the wave tier
// switched off, takes hilbert.generic
inline int hilbert_tier(int64_t n_fft, bool wave_off) { return (!wave_off && (n_fft == 1024 || n_fft == 2048)) ? kHbWave : kHbGeneric; }
// waves per workgroup of hilbert.wave: 45 KB (1024 points, four waves) and 53 KB (2048 points, two) of LDS leave three workgroups per
// compute unit
inline int hilbert_waves(int n_fft) { return n_fft == 2048 ? 2 : 4; }
inline int64_t hilbert_lds_bytes(int n_fft) {
  return (int64_t)(256 + (n_fft / 256) * 256 + hilbert_waves(n_fft) * (n_fft + n_fft / 16 + 16)) * 8;
}
// workgroups of a launch whose workgroups take `chunk` consecutive rows each
inline int64_t hilbert_blocks(int64_t rows, int64_t chunk) { return (rows + chunk - 1) / chunk; }

// ---- the fused kernel, K = 64 P points per wave.  Going in, lane l holds the ADJACENT samples i0 and i0 + 1 of each 128-sample slot q:
// i0 = hilbert_slot_sample(l, q) (what wave_fft_core_T consumes and wave_fft_core produces, so the results leave in the same layout)
NXSIG_HB_HD int hilbert_slot_sample(int lane, int q) { return 2 * lane + 128 * q; }
// how many of the two samples lie inside the n_used samples the row provides: 2 both (one 8-byte load), 1 the first alone, 0 neither;
// nothing at or past n_used is ever read
NXSIG_HB_HD int hilbert_pair_state(int i0, int n_used) { return i0 + 1 < n_used ? 2 : (i0 < n_used ? 1 : 0); }
// between the two transforms lane l holds bin l + 64 s in register s, so the gain is a condition on the register index: 2 below P / 2,
// 0 above, and 1 only on lane 0 in registers 0 and P / 2.  Equal to hilbert_gain(l + 64 s, 64 P) (tests/san_hilbert.cpp walks every lane)
NXSIG_HB_HD int hilbert_wave_gain(int lane, int s, int P) {
  if (s < P / 2) return (lane == 0 && s == 0) ? 1 : 2;
  if (s == P / 2) return lane == 0 ? 1 : 0;
  return 0;
}

}  // namespace nxsig
