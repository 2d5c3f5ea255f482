// Convolution.correlate_rows / convolve_rows: everything of it that is plain C++ — the argument checks, the
// tier choice, the transform length P, the index maps from the full result to the circular one for each op and mode, the mirror-bin
// map of the packed split, the power-of-two row scale, the slab arithmetic of xcorr.generic and the lane and slot arithmetic of
// xcorr.wave.  The C entry points, the kernels of kernels_xcorr.hip and the stand-alone program tests/san_xcorr.cpp (ASan / UBSan on
// the host) all use this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "czt_plan.hpp"   // the wave layout shared with czt.wave: czt_slot_sample, czt_pair_state, czt_wide, czt_lds_bytes, czt_blocks, czt_overlap

namespace nxsig {

enum XcorrTier : int32_t { kXcWave = 0, kXcGeneric = 1 };
// the values of include/nxsig.h
enum XcorrOp : int32_t { kXcConvolve = 0, kXcCorrelate = 1 };
enum XcorrMode : int32_t { kXcFull = 0, kXcSame = 1, kXcValid = 2 };
enum XcorrWeighting : int32_t { kXcPlain = 0, kXcPhat = 1 };
enum XcorrSink : int32_t { kXcRows = 0, kXcPeak = 1 };

// ---- the definition (include/nxsig.h).  full[k], k = 0 .. n1 + n2 - 2:
//   correlate   full[k] = sum_l x[l] conj(y[l - k + n2 - 1])      (the lag of full[k] is k - (n2 - 1))
//   convolve    full[k] = sum_l x[l] y[k - l]
inline int64_t xcorr_need(int64_t n1, int64_t n2) { return n1 + n2 - 1; }
// the mode's window of full: its first element and its length (SciPy's for all three modes, n2 > n1 included)
inline int64_t xcorr_out_start(int64_t n1, int64_t n2, int32_t mode) {
  return mode == kXcFull ? 0 : mode == kXcSame ? (n2 - 1) / 2 : (n1 < n2 ? n1 : n2) - 1;
}
inline int64_t xcorr_out_length(int64_t n1, int64_t n2, int32_t mode) {
  return mode == kXcFull ? n1 + n2 - 1 : mode == kXcSame ? n1 : (n1 >= n2 ? n1 - n2 : n2 - n1) + 1;
}
// scipy.signal.correlation_lags(n1, n2, mode)[0]; the lags count up by one from it.  SciPy's "same" window of the lags is NOT always
// the window of the values (n1 odd and n2 even differ by one): the peak sink reports correlation_lags(...)[argmax], as the contract says
inline int64_t xcorr_first_lag(int64_t n1, int64_t n2, int32_t mode) {
  if (mode == kXcFull) return -(n2 - 1);
  if (mode == kXcSame) return -(n2 - 1) + (n1 + n2 - 1) / 2 - n1 / 2;
  return n1 >= n2 ? 0 : n1 - n2;
}

// ---- the transform length of the contract, for BOTH tiers (the PHAT weighting is not linear in the operands, so its inverse depends
// on the length): P = max(1024, the next power of two >= n1 + n2 - 1)
inline int64_t xcorr_fft_length(int64_t n1, int64_t n2) {
  int64_t P = 1024;
  while (P < xcorr_need(n1, n2)) P <<= 1;
  return P;
}
// xcorr.wave keeps a pair inside one wave at P = 1024 (real and c64 pairs) or 2048 (real pairs only: a c64 pair holds two spectra and
// does not fit the register file at 2048 points); everything else, and everything with the wave tier switched off, is xcorr.generic
inline int xcorr_tier(int64_t n1, int64_t n2, bool is_complex, bool wave_off) {
  const int64_t need = xcorr_need(n1, n2);
  return (!wave_off && (need <= 1024 || (need <= 2048 && !is_complex))) ? kXcWave : kXcGeneric;
}

// ---- full -> circular.  Both tiers form c = IDFT_P(X conj(Y)) (correlate: c[j mod P] is lag j) or IDFT_P(X Y) (convolve: c[k] = full[k]);
// output element i of the mode's window is c[(xcorr_circ_start + i) mod P]
inline int64_t xcorr_circ_start(int64_t n1, int64_t n2, int32_t op, int32_t mode, int64_t P) {
  const int64_t s = xcorr_out_start(n1, n2, mode) - (op == kXcCorrelate ? n2 - 1 : 0);
  return ((s % P) + P) % P;
}
NXSIG_CZ_HD int64_t xcorr_circ_index(int64_t circ_start, int64_t i, int64_t P) { return (circ_start + i) & (P - 1); }
// the other way round: the output element the circular index j belongs to (>= n_out: none)
NXSIG_CZ_HD int64_t xcorr_out_index(int64_t circ_start, int64_t j, int64_t P) { return (j - circ_start) & (P - 1); }

// ---- the packed split.  A real pair goes through ONE forward transform as z = x + i y; with Zm = Z[(K - k) mod K]
//   X[k] = (Z[k] + conj(Zm)) / 2,   Y[k] = (Z[k] - conj(Zm)) / (2 i).
// After wave_fft_core_T lane l holds bin l + 64 s in register s (s < K / 64); the mirror bin of (l, s) is held by
NXSIG_CZ_HD int xcorr_mirror_lane(int lane) { return (64 - lane) & 63; }
NXSIG_CZ_HD int xcorr_mirror_reg(int lane, int s, int regs) { return lane == 0 ? (regs - s) % regs : regs - 1 - s; }
NXSIG_CZ_HD int xcorr_mirror_bin(int k, int K) { return (K - k) & (K - 1); }

// ---- the row scale.  Packing couples the rounding errors of the two rows (the error of either recovered spectrum is relative to the
// larger one), so each row is first scaled by the power of two that brings its largest magnitude into [0.5, 1): 2^-e with
// max = f 2^e, f in [0.5, 1).  Exact; undone at the sink by 2^(ea + eb).  An all-zero row, and a row whose maximum is not finite (it
// is poisoned anyway), keep scale 1.  max_bits: the IEEE bits of the row's largest |sample|
NXSIG_CZ_HD int xcorr_scale_exponent(uint32_t max_bits) {
  max_bits &= 0x7fffffffu;
  if (max_bits == 0 || max_bits >= 0x7f800000u) return 0;
  const int field = (int)(max_bits >> 23);
  if (field != 0) return field - 126;
  int lead = 0;                                  // subnormal: max = m 2^-149, m < 2^23
  for (uint32_t m = max_bits; m >>= 1;) ++lead;  // floor(log2 m)
  return lead - 148;
}

// ---- the argument errors that need neither the tensors nor a context; nullptr when all is well.  *unsupported: the arguments are
// well formed but beyond what is built
inline const char* xcorr_check(int64_t n1, int64_t a_stride, int64_t n2, int64_t b_stride, int64_t batch, int32_t is_complex, int32_t op,
                               int32_t mode, int32_t weighting, double phat_floor, int32_t sink, bool* unsupported) {
  *unsupported = false;
  if (is_complex != 0 && is_complex != 1) return "is_complex must be 0 or 1";
  if (op != kXcConvolve && op != kXcCorrelate) return "op must be 0 (convolve) or 1 (correlate)";
  if (mode != kXcFull && mode != kXcSame && mode != kXcValid) return "expected mode to be one of [:full, :same, :valid]";
  if (weighting != kXcPlain && weighting != kXcPhat) return "weighting must be 0 (none) or 1 (phat)";
  if (sink != kXcRows && sink != kXcPeak) return "sink must be 0 (rows) or 1 (peak)";
  if (weighting == kXcPhat && op != kXcCorrelate) return "the phat weighting belongs to correlate";
  if (sink == kXcPeak && op != kXcCorrelate) return "the peak sink belongs to correlate";
  if (!(phat_floor >= 0.0 && phat_floor < 1.0)) return "phat_floor must be in [0, 1)";
  if (n1 < 1 || n2 < 1) return "lengths must be >= 1";
  if (batch < 0) return "batch must be >= 0";
  if (a_stride < n1) return "a_stride must be >= n1";
  if (b_stride != 0 && b_stride < n2) return "b_stride must be 0 or >= n2";
  *unsupported = true;
  if (n1 > ((int64_t)1 << 30) || n2 > ((int64_t)1 << 30) || xcorr_need(n1, n2) > ((int64_t)1 << 30)) return "n1 + n2 - 1 must be at most 2^30";
  // the byte counts: the operands (c64 at the widest) and the result
  if (batch > 0 && (a_stride > INT64_MAX / batch / 16 || b_stride > INT64_MAX / batch / 16 || ((int64_t)1 << 31) > INT64_MAX / batch / 16))
    return "the rows are too large";
  *unsupported = false;
  return nullptr;
}

// ---- xcorr.generic's slabs.  Its four temporaries (the padded rows and the spectra of either operand, c64 [rows][P] each) stay within
// kXcorrSlabBytes together, or hold one pair when a single pair is larger: the batch runs in slabs of this many pairs
constexpr int64_t kXcorrSlabBytes = (int64_t)256 << 20;
inline int64_t xcorr_slab_rows(int64_t batch, int64_t P, int64_t forced) {
  int64_t rows = forced > 0 ? forced : kXcorrSlabBytes / (4 * P * 8);
  if (rows < 1) rows = 1;
  return rows < batch ? rows : batch;
}
inline int64_t xcorr_slabs(int64_t batch, int64_t slab_rows) { return slab_rows > 0 ? (batch + slab_rows - 1) / slab_rows : 0; }

// ---- xcorr.wave: czt.wave's layout, LDS budget and rows-per-wave geometry (czt_plan.hpp).  Going in, lane l holds the adjacent
// samples czt_slot_sample(l, q) and + 1 of each 128-sample slot q; the result leaves the inverse core in the same layout, so circular
// index j = czt_slot_sample(l, q) + par is output element xcorr_out_index(circ_start, j, K).  A pair of adjacent circular indices is
// one wide store when both elements are inside the row, adjacent in it (no wrap between them) and the first one lands on twice the
// element size.  Bit 0 / bit 1: the first / second element is inside the row; bit 2: they are adjacent in it
NXSIG_CZ_HD int xcorr_store_state(int64_t i0, int64_t i1, int64_t n_out) {
  const int in0 = i0 < n_out ? 1 : 0, in1 = i1 < n_out ? 2 : 0;
  return in0 | in1 | ((in0 && in1 && i1 == i0 + 1) ? 4 : 0);
}

}  // namespace nxsig
