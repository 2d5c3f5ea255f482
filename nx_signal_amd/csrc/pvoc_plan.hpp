// Transforms.phase_vocoder: everything of it that is plain C++ — the argument checks, the output frame count,
// the step function t -> (i_t, alpha_t) and the chunk geometry of the scan.  The C entry points and the kernels of kernels_pvoc.hip
// share this one copy, so the host's frame count and the device's walk cannot disagree.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NXSIG_PV_HD __host__ __device__ inline
#else
#define NXSIG_PV_HD inline
#endif

namespace nxsig {

// ---- the definition.  n_out = ceil(M / rate), the quotient in double: what len(numpy.arange(0, M, rate)) gives
inline int64_t pvoc_frames(int64_t M, double rate) { return (int64_t)std::ceil((double)M / rate); }

// s_t = t rate as ONE double product (no fused multiply-add: the host and the device must floor the same number), i_t = floor(s_t),
// alpha_t = s_t - i_t.  The last steps of a row can reach i_t = M - 1 (and, by the rounding of the product, M): frames M and M + 1
// count as zeros and are never read
NXSIG_PV_HD void pvoc_step_d(double t, double rate, double* f, double* alpha) {   // t a whole number: floor(s_t) as a double
#pragma clang fp contract(off)
  const double s = t * rate;
  *f = std::floor(s);
  *alpha = s - *f;
}
NXSIG_PV_HD void pvoc_step(int64_t t, double rate, int64_t* i, double* alpha) {
  double f;
  pvoc_step_d((double)t, rate, &f, alpha);
  *i = (int64_t)f;
}

constexpr int64_t kPvMaxFrames = (int64_t)1 << 40;   // input and output frames of a row
inline const char* pvoc_check_rate(int64_t frames, double rate, bool* unsupported) {
  *unsupported = false;
  if (frames < 1) return "frames must be >= 1";
  if (!(rate > 0.0) || !std::isfinite(rate)) return "rate must be a finite number > 0";
  if (frames > kPvMaxFrames || (double)frames / rate > (double)kPvMaxFrames) { *unsupported = true; return "rows of at most 2^40 input and output frames are built"; }
  return nullptr;
}
inline const char* pvoc_check(int64_t batch, int64_t frames, int64_t bins, double rate, bool* unsupported) {
  if (const char* what = pvoc_check_rate(frames, rate, unsupported)) return what;
  if (batch < 0) return "batch must be >= 0";
  if (bins < 1) return "bins must be >= 1";
  if (batch > ((int64_t)1 << 31) || bins > ((int64_t)1 << 31)) { *unsupported = true; return "at most 2^31 rows and 2^31 bins are built"; }
  return nullptr;
}

// ---- geometry.  A lane owns kPvWide = 2 adjacent bins (16-byte accesses) or one (8-byte accesses: odd K, misaligned bases); a wave
// owns a TILE of 64 lanes' bins and walks a CHUNK of C consecutive output frames of one row; kPvWaves waves of a workgroup take
// consecutive units (tile fastest, then chunk, then row)
constexpr int kPvWaves = 4;
constexpr int kPvWide = 2;
constexpr int kPvDepth = 4;              // input frames in flight ahead of the one in use (registers: 4 VGPRs per frame and lane)
constexpr int64_t kPvWalkFrames = 1024;  // a row of at most this many output frames is one chunk: one launch beats three short ones
constexpr int64_t kPvMinChunk = 64;      // the aggregates (16 bytes per chunk and bin) stay <= 2 / 64 of out (8 bytes per frame and bin)
constexpr int64_t kPvTargetWaves = 4096; // 256 CUs x 4 SIMDs x 4 resident waves
inline int64_t pvoc_tiles(int64_t K, bool wide) { const int64_t w = 64 * (wide ? kPvWide : 1); return (K + w - 1) / w; }
// the 16-byte instantiation: K even puts every frame of a 16-byte-aligned base on a 16-byte boundary
inline bool pvoc_wide(int64_t K, uintptr_t z, uintptr_t out) { return K % 2 == 0 && z % 16 == 0 && out % 16 == 0; }
// C: the rows' frames spread over kPvTargetWaves waves, not below kPvMinChunk; `forced` > 0 (NXSIG_PVOC_CHUNK) is taken as it is.
// C >= n_out means one chunk: pvoc.walk
inline int64_t pvoc_chunk_frames(int64_t n_out, int64_t batch, int64_t K, int64_t forced = 0) {
  if (forced > 0) return forced < n_out ? forced : n_out;
  if (n_out <= kPvWalkFrames) return n_out;
  const int64_t columns = (batch < 1 ? 1 : batch) * pvoc_tiles(K, true);
  const int64_t chunks = (kPvTargetWaves + columns - 1) / columns;
  int64_t C = (n_out + chunks - 1) / chunks;
  if (C < kPvMinChunk) C = kPvMinChunk;
  return C < n_out ? C : n_out;
}
inline int64_t pvoc_chunks(int64_t n_out, int64_t C) { return (n_out + C - 1) / C; }

}  // namespace nxsig
