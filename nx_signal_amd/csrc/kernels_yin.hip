// Spectral.yin: the YIN pitch estimate of every frame of f32 rows, following librosa.yin (every sum direct and in double).
// include/nxsig.h states the definition, DESIGN.md section 3.26 the design; the checks, the frame count and the geometry are
// csrc/yin_plan.hpp.
// A frame's hot loop is the difference function d(tau) = sum_{j = 1 .. W} (x[j] - x[j + tau])^2, tau = 0 ... T: W (T + 1) pairs of one
// double subtraction and one double FMA.
//   yin.tile   the frame's used samples x[1 ... W + T] are converted to double once and staged in LDS (out-of-row samples as zeros,
//              the non-finite flag taken on the way).  A thread owns R consecutive lags tau0 = t R ... in R accumulators; 64 threads
//              serve a frame when 64 R covers the lags (then the waves of a workgroup take consecutive frames), 256 otherwise.  The
//              thread walks j in blocks of B: per block it reads B template values x[j ...] (one address for the whole wave: an LDS
//              broadcast) and B NEW window values; the other B of the 2 B values x[j + tau0 ...] a block touches are the ones the
//              block before read last, kept in registers (the loop is unrolled twice so that the two halves swap names, not
//              contents): 2 B LDS reads per R B pairs.  Staged samples lie in groups of R with one spare double after each (even R),
//              so the window reads of neighbouring lanes, R samples apart, fall into different banks, and every offset inside a block
//              is a compile-time immediate.
//              The tail runs in the same launch: an inclusive prefix sum of d over tau (per thread over its R lags, across the wave
//              by lane shifts, across waves through LDS, all in a fixed order), c = d / (prefix / tau + tiny) into LDS over the
//              samples (no longer needed), the coalesced f32 store of c if asked for, two first-index reductions (the first trough
//              under the threshold; the minimum with the lowest index), the three-point shift and one store of f0 and v per frame.
// Deterministic: a frame's bits depend on (L, pmin, pmax, threshold, sr) and its samples; no atomics, no temporary.
#include <cfloat>
#include <climits>

#include "nxsig_internal.h"

namespace nxsig {

namespace {

struct YinArgs {
  const float* x;       // f32 rows, `stride` elements apart
  float* f0;            // f32 [batch F] or null
  float* v;             // f32 [batch F] or null
  float* cm;            // f32 [batch F][m] or null
  int64_t stride, n, hop, F;   // F: frames per row
  int64_t total;        // batch F
  double sr, thr;
  int32_t W, T, pmin, m;       // the window, the largest lag, the smallest period, pmax - pmin + 1
  int32_t lead;         // samples ahead of the row that frame 0 starts at: L / 2 with center, else 0
  int32_t groups;       // groups of R staged samples per frame
  int32_t per_wg;       // frames per workgroup
};

// what one frame's threads wait on: the workgroup's barrier for 256 threads, nothing but program order for one wave
template <int TPF>
__device__ __forceinline__ void frame_sync() {
  if constexpr (TPF == 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}
template <int TPF>
__device__ __forceinline__ bool frame_any(bool p) {
  if constexpr (TPF == 64) {
    frame_sync<64>();
    return __any(p) != 0;
  } else {
    return __syncthreads_or(p) != 0;
  }
}

// one block of the walk: the B template values at tp, the window's upper half read into `hi` (the lower one, `lo`, is the upper half of
// the block before), R B pairs.  Every index is a compile-time constant once unrolled
template <int R, int B, int GS>
__device__ __forceinline__ void yin_block_step(const double* tp, const double* win, const double (&lo)[B], double (&hi)[B], double (&acc)[R]) {
  double tv[B];
#pragma unroll
  for (int k = 0; k < B; ++k) {
    hi[k] = win[(B + k) / R * GS + (B + k) % R];
    tv[k] = tp[k / R * GS + k % R];
  }
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double diff = tv[b] - (b + r < B ? lo[b + r < B ? b + r : 0] : hi[b + r < B ? 0 : b + r - B]);
      acc[r] = __builtin_fma(diff, diff, acc[r]);
    }
}

template <int R, int TPF>
__global__ __launch_bounds__(256) void k_yin_tile(YinArgs g) {
  constexpr int B = R < 4 ? 4 : R, GS = R == 1 ? 1 : R + 1, kStep = B / R * GS;   // kStep: doubles between two blocks
  extern __shared__ double yin_lds[];
  __shared__ double s_sum[kYinWaves], s_minv[kYinWaves];
  __shared__ int s_first[kYinWaves], s_mini[kYinWaves];
  const int t = (int)threadIdx.x % TPF, slot = (int)threadIdx.x / TPF, lane = t & 63, wave = t >> 6;
  const int64_t frame = (int64_t)blockIdx.x * g.per_wg + slot;
  if (frame >= g.total) return;   // a whole wave of a 64-thread frame; a 256-thread frame has the workgroup to itself
  double* s = yin_lds + (size_t)slot * g.groups * GS;
  const float* xr = g.x + (frame / g.F) * g.stride;
  const int64_t first_pos = (frame % g.F) * g.hop - g.lead + 1;   // the row index of x[1], the first used sample
  const int used = g.W + g.T, cap = g.groups * R;

  // stage x[1 ... W + T] in double, zeros where the row has no sample and from W + T on (unused lags read there)
  bool bad = false;
  for (int u = t; u < cap; u += TPF) {
    const int64_t pos = first_pos + u;
    float val = 0.0f;
    if (u < used && pos >= 0 && pos < g.n) val = xr[pos];
    bad = bad || !(__builtin_fabsf(val) <= FLT_MAX);
    s[u / R * GS + u % R] = (double)val;
  }
  bad = frame_any<TPF>(bad);

  // the difference function: acc[r] = d(t R + r)
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  if ((t & ~63) * R <= g.T) {   // a wave whose lags all lie beyond T has nothing to add
    const double* tp = s;
    const double* win = s + t * GS;
    double c0[B], c1[B];
#pragma unroll
    for (int k = 0; k < B; ++k) c0[k] = win[k / R * GS + k % R];
    const int blocks = g.W / B;
    int jb = 0;
    for (; jb + 2 <= blocks; jb += 2) {
      yin_block_step<R, B, GS>(tp, win, c0, c1, acc);
      yin_block_step<R, B, GS>(tp + kStep, win + kStep, c1, c0, acc);
      tp += 2 * kStep; win += 2 * kStep;
    }
    if (jb < blocks) yin_block_step<R, B, GS>(tp, win, c0, c1, acc);
    for (int j = blocks * B; j < g.W; ++j) {   // the last W % B template values, one at a time
      const double tv = s[j / R * GS + j % R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = j + t * R + r;
        const double diff = tv - s[i / R * GS + i % R];
        acc[r] = __builtin_fma(diff, diff, acc[r]);
      }
    }
  }

  // the prefix sum of d over tau: the thread's own lags, then the threads below it in the wave, then the waves below
  double inc = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) inc += acc[r];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  double run = __shfl_up(inc, 1, 64);
  if (lane == 0) run = 0.0;
  if constexpr (TPF == 256) {
    if (lane == 63) s_sum[wave] = inc;
    __syncthreads();   // also: every wave has left the walk, the samples may be overwritten
    double carry = 0.0;
    for (int w = 0; w < wave; ++w) carry += s_sum[w];
    run += carry;
  } else {
    frame_sync<64>();
  }
  double* cc = s;   // c[i], i = tau - pmin
#pragma unroll
  for (int r = 0; r < R; ++r) {
    run += acc[r];
    const int tau = t * R + r;
    if (tau >= g.pmin && tau <= g.T) cc[tau - g.pmin] = acc[r] / (run / (double)tau + DBL_MIN);
  }
  frame_sync<TPF>();

  const int m = g.m;
  const float nanf32 = __builtin_nanf("");
  if (g.cm) {
    float* co = g.cm + frame * m;
    for (int i = t; i < m; i += TPF) co[i] = bad ? nanf32 : (float)cc[i];
  }
  // the first trough under the threshold, and the minimum with the lowest index
  int first = INT_MAX, mini = INT_MAX;
  double minv = __builtin_inf();
  if (!bad)
    for (int i = t; i < m; i += TPF) {
      const double ci = cc[i];
      const bool trough = i == 0 ? ci < cc[1] : i == m - 1 ? ci < cc[m - 2] : ci < cc[i - 1] && ci <= cc[i + 1];
      if (trough && ci < g.thr && first == INT_MAX) first = i;
      if (ci < minv) { minv = ci; mini = i; }
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int of = __shfl_xor(first, off, 64), oi = __shfl_xor(mini, off, 64);
    const double ov = __shfl_xor(minv, off, 64);
    first = of < first ? of : first;
    if (ov < minv || (ov == minv && oi < mini)) { minv = ov; mini = oi; }
  }
  if constexpr (TPF == 256) {
    if (lane == 0) { s_first[wave] = first; s_minv[wave] = minv; s_mini[wave] = mini; }
    __syncthreads();
    first = s_first[0]; minv = s_minv[0]; mini = s_mini[0];
    for (int w = 1; w < kYinWaves; ++w) {
      first = s_first[w] < first ? s_first[w] : first;
      if (s_minv[w] < minv || (s_minv[w] == minv && s_mini[w] < mini)) { minv = s_minv[w]; mini = s_mini[w]; }
    }
  }
  if (t == 0) {
    const int is = first != INT_MAX ? first : mini < m ? mini : 0;
    const double ci = cc[is];
    double shift = 0.0;
    if (is > 0 && is < m - 1) {
      const double a = cc[is + 1] + cc[is - 1] - 2.0 * ci, b = (cc[is + 1] - cc[is - 1]) / 2.0;
      if (__builtin_fabs(b) < __builtin_fabs(a)) shift = -b / a;
    }
    const double f0 = g.sr / ((double)(g.pmin + is) + shift);
    if (g.f0) g.f0[frame] = bad ? nanf32 : (float)f0;
    if (g.v) g.v[frame] = bad ? nanf32 : (float)ci;
  }
}

template <int R, int TPF>
int run_tile(Ctx* c, YinArgs g, const YinGeometry& geo) {
  g.groups = (int32_t)geo.groups; g.per_wg = geo.frames;
  const int64_t blocks = (g.total + geo.frames - 1) / geo.frames;
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "yin: too many frames for one launch");
  hipLaunchKernelGGL((k_yin_tile<R, TPF>), dim3((unsigned)blocks), dim3((unsigned)(TPF * geo.frames)), geo.frames * geo.frame_bytes, c->stream, g);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <int TPF>
int run_threads(Ctx* c, const YinArgs& g, const YinGeometry& geo) {
  switch (geo.lags) {
    case 1: return run_tile<1, TPF>(c, g, geo);
    case 2: return run_tile<2, TPF>(c, g, geo);
    case 4: return run_tile<4, TPF>(c, g, geo);
    default: return run_tile<8, TPF>(c, g, geo);
  }
}

}  // namespace

int launch_yin(Ctx* c, const YinLaunch& l) {
  YinArgs g = {};
  g.x = static_cast<const float*>(l.x); g.f0 = static_cast<float*>(l.f0); g.v = static_cast<float*>(l.v); g.cm = static_cast<float*>(l.cmnd);
  g.stride = l.x_stride; g.n = l.n; g.hop = l.hop; g.sr = l.sr; g.thr = l.threshold;
  g.W = (int32_t)yin_window(l.frame_length); g.T = (int32_t)l.max_period; g.pmin = (int32_t)l.min_period;
  g.m = (int32_t)(l.max_period - l.min_period + 1);
  g.lead = l.center ? (int32_t)(l.frame_length / 2) : 0;
  g.F = yin_frames(l.n, l.frame_length, l.hop, l.center);
  g.total = l.batch * g.F;
  if (g.total == 0) return NXSIG_OK;
  dispatch_note("yin.tile");
  const YinGeometry geo = yin_geometry(l.frame_length, l.max_period, tune(c, kT_YIN_LAGS, 0));
  return geo.threads == kYinThreads[0] ? run_threads<64>(c, g, geo) : run_threads<256>(c, g, geo);
}

}  // namespace nxsig
