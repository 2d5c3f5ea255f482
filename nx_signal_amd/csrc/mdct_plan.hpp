// Transforms.mdct / imdct: everything of it that is plain C++ — the argument checks, the frame count, the tier
// choice, the run hand-out, the fold / unfold index maps and the table builder.  The C entry points and the kernels of kernels_mdct.hip
// share this one copy.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NXSIG_MD_HD __host__ __device__ inline
#else
#define NXSIG_MD_HD inline
#endif

namespace nxsig {

enum MdctNorm : int32_t { kMdNormNone = 0, kMdNormOrtho = 1 };   // nxsig_mdct_norm of include/nxsig.h
enum MdctTier : int { kMdWave = 0, kMdGeneric = 1 };

// ---- the definition: frame length N = 2 M, hop M.  Frame m covers the half-frame BLOCKS m and m + 1 of the (virtually padded) row;
// block b holds the row's samples (b - pad) M ... (b - pad) M + M - 1, zero outside [0, L) and never read there (pad = pad_edges)
inline int64_t mdct_frames(int64_t L, int64_t N, bool pad) {
  const int64_t M = N / 2;
  return pad ? (L + M - 1) / M + 1 : (L - N) / M + 1;
}
// samples imdct returns by default
inline int64_t imdct_length(int64_t frames, int64_t N, bool pad) { return pad ? (frames - 1) * (N / 2) : (frames + 1) * (N / 2); }

// the factor on the sum: forward 1 or sqrt(2 / M); inverse 2 / M or sqrt(2 / M)
inline double mdct_scale(int64_t M, int32_t norm, bool inverse) {
  return norm == kMdNormOrtho ? std::sqrt(2.0 / (double)M) : (inverse ? 2.0 / (double)M : 1.0);
}

inline const char* mdct_check_frame(int64_t N, int32_t pad, int32_t norm, bool* unsupported) {
  *unsupported = false;
  if (N < 4 || N % 4 != 0) return "frame_length must be a positive multiple of 4";
  if (pad != 0 && pad != 1) return "pad_edges must be 0 or 1";
  if (norm != kMdNormNone && norm != kMdNormOrtho) return "norm must be NXSIG_MDCT_NORM_NONE or NXSIG_MDCT_NORM_ORTHO";
  if (N > ((int64_t)1 << 24)) { *unsupported = true; return "frame_length must be at most 2^24"; }
  return nullptr;
}
inline const char* mdct_check(int64_t L, int64_t batch, int64_t batch_stride, int64_t N, int32_t pad, int32_t norm, bool* unsupported) {
  if (const char* what = mdct_check_frame(N, pad, norm, unsupported)) return what;
  if (batch < 0) return "batch must be >= 0";
  if (L < 1) return "length must be >= 1";
  if (!pad && L < N) return "length must be at least frame_length without pad_edges";
  if (batch_stride < L) return "batch_stride must be >= length";
  if (L > ((int64_t)1 << 40) || batch > ((int64_t)1 << 31)) { *unsupported = true; return "rows of at most 2^40 samples and 2^31 rows are built"; }
  return nullptr;
}
inline const char* imdct_check(int64_t frames, int64_t batch, int64_t N, int32_t pad, int32_t norm, int64_t out_length, bool* unsupported) {
  if (const char* what = mdct_check_frame(N, pad, norm, unsupported)) return what;
  if (batch < 0) return "batch must be >= 0";
  if (frames < 1) return "frames must be >= 1";
  if (frames > ((int64_t)1 << 40) || batch > ((int64_t)1 << 31)) { *unsupported = true; return "at most 2^40 frames and 2^31 rows are built"; }
  const int64_t M = N / 2;
  if (pad ? (out_length < 1 || out_length > frames * M) : out_length != (frames + 1) * M)
    return pad ? "out_length must be in [1, frames * frame_length / 2] with pad_edges" : "out_length must be (frames + 1) * frame_length / 2 without pad_edges";
  return nullptr;
}

// ---- the tier: mdct.wave / imdct.wave run the M / 2-point complex transform inside a wave for M = 256, 512, 1024
inline int mdct_tier(int64_t M, bool wave_off) { return (!wave_off && (M == 256 || M == 512 || M == 1024)) ? kMdWave : kMdGeneric; }

// ---- mdct.wave / imdct.wave geometry.  A wave transforms 512 complex points per iteration, 8 per lane: G = 1024 / M consecutive
// frames of one row, each on its own group of M / 16 lanes.  A wave walks a RUN of consecutive frames of one row; the kMdWaves waves
// of a workgroup take consecutive runs
constexpr int kMdWaves = 4;
constexpr int kMdMinRun = 8;       // frames: the run of the smallest launch (a multiple of every G)
constexpr int kMdMaxRun = 64;
constexpr int kMdBuf = 512 + 64;   // complex slots of a wave's LDS buffer: 512 points, one slot of padding after every 8
inline int64_t mdct_lds_bytes() { return (int64_t)kMdWaves * kMdBuf * 8; }
NXSIG_MD_HD int mdct_pad(int a) { return a + (a >> 3); }
// frames per run: the frames spread over `slots` resident waves, rounded up to whole iterations, within [kMdMinRun, kMdMaxRun]
inline int64_t mdct_run_frames(int64_t frames, int64_t rows, int64_t slots, int64_t M) {
  const int64_t G = 1024 / M;
  int64_t run = (frames * rows + slots - 1) / (slots < 1 ? 1 : slots);
  run = (run + G - 1) / G * G;
  return run < kMdMinRun ? kMdMinRun : (run > kMdMaxRun ? kMdMaxRun : run);
}

// ---- the fold.  The windowed frame f = w x in quarters a, b, c, d of M / 2 samples gives u = [-rev(c) - d, a - rev(b)], and
// X[m, .] is the DCT-IV of u.  A lane that holds samples i and M - 1 - i (i < M / 2) of block b forms, with no other lane's samples,
//   P_i = u_{b-1}[M/2 - 1 - i] = -w[M + i] h[i] - w[2M - 1 - i] h[M - 1 - i]     (block b as the SECOND half of frame b - 1)
//   Q_i = u_b    [M/2 + i]     =  w[i] h[i]     - w[M - 1 - i]  h[M - 1 - i]     (block b as the FIRST half of frame b)
// and the complex point t[n] = u[2n] + i u[M - 1 - 2n] of a frame takes P_i and the frame's carried Q_i of ONE i:
//   i odd : n = (M/2 - 1 - i) / 2,  t[n] = P_i + i Q_i          i even: n = (M/2 + i) / 2,  t[n] = Q_i + i P_i
NXSIG_MD_HD int mdct_fold_point(int i, int M) { return (i & 1) ? (M / 2 - 1 - i) / 2 : (M / 2 + i) / 2; }
// the same fold sample by sample (the generic tier): u[j] = s0 f[p0] + s1 f[p1]
NXSIG_MD_HD void mdct_fold_pair(int64_t j, int64_t M, int64_t* p0, int64_t* p1, float* s0) {
  if (j < M / 2) { *p0 = 3 * M / 2 - 1 - j; *p1 = 3 * M / 2 + j; *s0 = -1.0f; }   // -rev(c) - d
  else { *p0 = j - M / 2; *p1 = 3 * M / 2 - 1 - j; *s0 = 1.0f; }                   // a - rev(b): the second term is always subtracted
}
// the unfold (its transpose): sample n of the frame built from v = DCT-IV(X[m, .]) is s v[j], w[n] and the scale aside
NXSIG_MD_HD int64_t mdct_unfold(int64_t n, int64_t M, float* s) {
  if (n < M / 2) { *s = 1.0f; return M / 2 + n; }
  *s = -1.0f;
  return n < 3 * M / 2 ? 3 * M / 2 - 1 - n : n - 3 * M / 2;
}

// ---- the tables of one (M, scale), Q = M / 2 complex entries each, formed in double:
//   pre[n] = exp(-i pi (4n + 1) / (4M))      post[k] = scale exp(-i pi k / M)      fw[j] = exp(-2 pi i j / Q)
// DCT-IV(u)[2k] = Re y[k], DCT-IV(u)[M - 1 - 2k] = -Im y[k] with y = post . DFT_Q(pre . t)
inline void mdct_tables(int64_t M, double scale, double* pre, double* post, double* fw) {
  const int64_t Q = M / 2;
  const double pi = 3.14159265358979323846;
  for (int64_t n = 0; n < Q; ++n) {
    const double a = -pi * (double)(4 * n + 1) / (double)(4 * M), b = -pi * (double)n / (double)M, c = -2.0 * pi * (double)n / (double)Q;
    pre[2 * n] = std::cos(a); pre[2 * n + 1] = std::sin(a);
    post[2 * n] = scale * std::cos(b); post[2 * n + 1] = scale * std::sin(b);
    fw[2 * n] = std::cos(c); fw[2 * n + 1] = std::sin(c);
  }
}

}  // namespace nxsig
