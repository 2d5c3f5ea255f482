// Transforms.mdct / imdct: the lapped cosine transform of real f32 rows, frame length N = 2 M, hop M, M real coefficients per frame.
// include/nxsig.h states the definition, DESIGN.md section 3.23 the design; the checks, the tier choice, the run hand-out, the fold
// maps and the table builder are csrc/mdct_plan.hpp.  Both tiers compute a frame's DCT-IV as ONE complex transform of Q = M / 2 points
// between a pre- and a post-twiddle:  t[n] = u[2n] + i u[M - 1 - 2n],  y = post . DFT_Q(pre . t),  X[2k] = Re y[k],  X[M - 1 - 2k] = -Im y[k].
//   mdct.wave / imdct.wave        M = 256, 512, 1024.  A wave walks a run of consecutive frames of one row, G = 1024 / M frames per
//                    iteration, each frame on its own group of M / 16 lanes, 8 complex points per lane.
//                    Forward: a lane loads samples i and M - 1 - i (8 values of i, 16-byte loads) of ONE half-frame block and forms
//                    in registers both of the block's folded halves: P (the block as the second half of the frame that ends there)
//                    and Q (as the first half of the frame that starts there).  Q is carried in registers to the next frame — to the
//                    next lane group by one lane permute, from the last group to the first across iterations — so every sample is
//                    loaded once.  Pre-twiddle, three register passes (radix 8 . 8 . 8, 8 . 8 . 4, 8 . 4 . 4) with two in-place LDS
//                    exchanges, post-twiddle, and a last LDS turn that puts the coefficients in order for 16-byte stores.
//                    Inverse: the same passes; a lane reads v[M/2 + i] and v[M/2 - 1 - i] back, carries the second (the frame's
//                    contribution to the NEXT block) the same way, and stores every output sample once: no atomics, no second pass.
//                    The first frame of a run that does not start a row loads its first block (forward) or recomputes the frame
//                    before it (inverse) without storing; pad_edges halves are zeros and are never read.
//   mdct.generic / imdct.generic  every other even M and everything under NXSIG_MDCT_WAVE=0 / NXSIG_DISABLE_WAVE: a fold + pre-twiddle
//                    kernel, launch_fft on rows of Q points (Bluestein and odd Q come with it), and a post-twiddle kernel that for the
//                    inverse also overlap-adds the two frames of every sample.  Its two temporaries are the tier's own.
// Non-finite rule: frames are transformed independently in both tiers (the wave tier's lane groups share nothing but the carried
// halves), and the pre-twiddle (no zero component) spreads an Inf / NaN to both parts of a point and the transform to every bin, so
// exactly the frames that cover a non-finite sample — the blocks a non-finite coefficient's frame covers — lose their finite values.
#include <algorithm>
#include <cstring>
#include <vector>

#include "nxsig_internal.h"

namespace nxsig {

namespace {

constexpr int kThreads = 256;

extern __shared__ __attribute__((aligned(16))) unsigned char md_smem[];
typedef float md_v4f __attribute__((ext_vector_type(4)));   // what the non-temporal store builtin takes

__device__ __forceinline__ float2 md_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 md_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 md_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// natural-order forward DFTs on registers
__device__ __forceinline__ void md_dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 s02 = md_add(a0, a2), d02 = md_sub(a0, a2), s13 = md_add(a1, a3), d13 = md_sub(a1, a3);
  a0 = md_add(s02, s13); a2 = md_sub(s02, s13);
  a1 = make_float2(d02.x + d13.y, d02.y - d13.x);   // d02 - i d13
  a3 = make_float2(d02.x - d13.y, d02.y + d13.x);   // d02 + i d13
}
template <int R>
__device__ __forceinline__ void md_dft(float2* u) {
  if (R == 4) { md_dft4(u[0], u[1], u[2], u[3]); return; }
  const float h = 0.70710678118654752f;
  float2 a0 = u[0], a1 = u[2], a2 = u[4], a3 = u[6], b0 = u[1], b1 = u[3], b2 = u[5], b3 = u[7];
  md_dft4(a0, a1, a2, a3);
  md_dft4(b0, b1, b2, b3);
  b1 = make_float2((b1.x + b1.y) * h, (b1.y - b1.x) * h);    // W8^1
  b2 = make_float2(b2.y, -b2.x);                             // W8^2
  b3 = make_float2((b3.y - b3.x) * h, -(b3.x + b3.y) * h);   // W8^3
  u[0] = md_add(a0, b0); u[4] = md_sub(a0, b0);
  u[1] = md_add(a1, b1); u[5] = md_sub(a1, b1);
  u[2] = md_add(a2, b2); u[6] = md_sub(a2, b2);
  u[3] = md_add(a3, b3); u[7] = md_sub(a3, b3);
}

// this wave's LDS traffic in program order (the hardware runs a wave's DS operations in order)
__device__ __forceinline__ void md_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct MdWaveArgs {
  const float* in;
  float* out;
  const float* w;       // f32[2 M]
  const float2* tab;    // pre[Q] | post[Q] | fw[Q]
  int64_t in_stride;    // forward: elements between rows
  int64_t L;            // forward: samples of a row; inverse: samples of an output row
  int64_t F, run, runs_per_row, total_runs;
  int32_t pad;
};

// the three passes of G independent Q-point transforms, 8 points per lane.  Pass 1 (radix 8 over n = LF r + lf) takes its points in
// u; passes 2 and 3 (radix R2, R3 with R2 R3 = LF) exchange through zb in place, so a butterfly reads and writes the same slots and
// one fence per exchange is enough.  y[s][k3] leaves as bin k = k1 + 8 (k2 + R2 k3) of butterfly b = lf + LF s = k1 R2 + k2, times post
template <int M>
struct MdCore {
  static constexpr int Q = M / 2, LF = M / 16, G = 64 / LF, R2 = M == 256 ? 4 : 8, R3 = LF / R2, S2 = 8 / R2, S3 = 8 / R3;
  float2 tw1[8], tw2[S2][R2], post[S3][R3];
  int kout[S3][R3];
  __device__ __forceinline__ void init(const float2* tab, int lf) {
    const float2* fw = tab + 2 * Q;
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) tw1[k1] = fw[lf * k1];
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      const int n3 = (lf + LF * s) % R3;
#pragma unroll
      for (int k2 = 0; k2 < R2; ++k2) tw2[s][k2] = fw[8 * n3 * k2];
    }
#pragma unroll
    for (int s = 0; s < S3; ++s) {
      const int b = lf + LF * s, k1 = b / R2, k2 = b % R2;
#pragma unroll
      for (int k3 = 0; k3 < R3; ++k3) { kout[s][k3] = k1 + 8 * (k2 + R2 * k3); post[s][k3] = tab[Q + kout[s][k3]]; }
    }
  }
  __device__ __forceinline__ void run(float2* u, float2* zb, int g, int lf, float2 (*y)[R3]) const {
    md_dft<8>(u);
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) zb[mdct_pad(g * Q + k1 * LF + lf)] = k1 ? md_cmul(u[k1], tw1[k1]) : u[0];
    md_fence();
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      const int b = lf + LF * s, base = g * Q + (b / R3) * LF + b % R3;
      float2 v[R2];
#pragma unroll
      for (int n2 = 0; n2 < R2; ++n2) v[n2] = zb[mdct_pad(base + R3 * n2)];
      md_dft<R2>(v);
#pragma unroll
      for (int k2 = 0; k2 < R2; ++k2) zb[mdct_pad(base + R3 * k2)] = k2 ? md_cmul(v[k2], tw2[s][k2]) : v[0];
    }
    md_fence();
#pragma unroll
    for (int s = 0; s < S3; ++s) {
      const int base = g * Q + R3 * (lf + LF * s);
      float2 v[R3];
#pragma unroll
      for (int n3 = 0; n3 < R3; ++n3) v[n3] = zb[mdct_pad(base + n3)];
      md_dft<R3>(v);
#pragma unroll
      for (int k3 = 0; k3 < R3; ++k3) y[s][k3] = md_cmul(v[k3], post[s][k3]);
    }
    md_fence();   // every read of the exchange is issued before the caller reuses the buffer
  }
};

// the run of this wave: row, first frame, one past the last
__device__ __forceinline__ bool md_run(const MdWaveArgs& a, int wave, int64_t* row, int64_t* m0, int64_t* m_end) {
  const int64_t rid = (int64_t)blockIdx.x * kMdWaves + wave;
  if (rid >= a.total_runs) return false;
  *row = rid / a.runs_per_row;
  *m0 = (rid - *row * a.runs_per_row) * a.run;
  *m_end = *m0 + a.run < a.F ? *m0 + a.run : a.F;
  return true;
}

template <int M>
__global__ __launch_bounds__(64 * kMdWaves) void k_mdct_wave(MdWaveArgs a) {
  using Core = MdCore<M>;
  constexpr int Q = Core::Q, LF = Core::LF, G = Core::G, R3 = Core::R3, S3 = Core::S3;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / LF, lf = lane % LF;
  float2* zb = reinterpret_cast<float2*>(md_smem) + wave * kMdBuf;
  float* ob = reinterpret_cast<float*>(zb);
  int64_t r, m0, m_end;
  if (!md_run(a, wave, &r, &m0, &m_end)) return;   // no workgroup barrier anywhere below
  const float* row = a.in + (size_t)r * a.in_stride;
  const bool row16 = (reinterpret_cast<uintptr_t>(row) & 15) == 0, out16 = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
  float wa[8], wb[8], wc[8], wd[8];
  float2 pre[8];
  int zaddr[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int i = 8 * lf + e, n = mdct_fold_point(i, M);
    wa[e] = a.w[i]; wb[e] = a.w[M - 1 - i]; wc[e] = a.w[M + i]; wd[e] = a.w[2 * M - 1 - i];
    pre[e] = a.tab[n];
    zaddr[e] = mdct_pad(g * Q + n);
  }
  Core core;
  core.init(a.tab, lf);
  // samples i = 8 lf + e (hf) and M - 1 - i (hb) of block b; outside the row they are zeros that are never read
  auto load_block = [&](int64_t b, float* hf, float* hb) {
    const int64_t base = (b - a.pad) * M;
    if (base >= 0 && base + M <= a.L) {
      const float* p = row + base;
      if (row16) {
        const float4 f0 = *reinterpret_cast<const float4*>(p + 8 * lf), f1 = *reinterpret_cast<const float4*>(p + 8 * lf + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(p + M - 8 - 8 * lf), b1 = *reinterpret_cast<const float4*>(p + M - 4 - 8 * lf);
        hf[0] = f0.x; hf[1] = f0.y; hf[2] = f0.z; hf[3] = f0.w; hf[4] = f1.x; hf[5] = f1.y; hf[6] = f1.z; hf[7] = f1.w;
        hb[7] = b0.x; hb[6] = b0.y; hb[5] = b0.z; hb[4] = b0.w; hb[3] = b1.x; hb[2] = b1.y; hb[1] = b1.z; hb[0] = b1.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { hf[e] = p[8 * lf + e]; hb[e] = p[M - 1 - 8 * lf - e]; }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t of = base + 8 * lf + e, ob2 = base + M - 1 - 8 * lf - e;
        hf[e] = (of >= 0 && of < a.L) ? row[of] : 0.0f;
        hb[e] = (ob2 >= 0 && ob2 < a.L) ? row[ob2] : 0.0f;
      }
    }
  };
  float hf[8], hb[8], qprev[8];
  // the seam: the carried half of the run's first frame is block m0's, which the last lane group loads for itself
  load_block(m0 - (G - 1) + g, hf, hb);
#pragma unroll
  for (int e = 0; e < 8; ++e) qprev[e] = wa[e] * hf[e] - wb[e] * hb[e];
  load_block(m0 + g + 1, hf, hb);
  for (int64_t m_it = m0; m_it < m_end; m_it += G) {
    float P[8], qn[8], qc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      P[e] = -wc[e] * hf[e] - wd[e] * hb[e];
      qn[e] = wa[e] * hf[e] - wb[e] * hb[e];
    }
    if (m_it + G < m_end) load_block(m_it + G + g + 1, hf, hb);   // the next iteration's samples fly during this one's transform
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qc[e] = G == 1 ? qprev[e] : __shfl(g == G - 1 ? qprev[e] : qn[e], (lane - LF) & 63);
      qprev[e] = qn[e];
      const float2 t = (e & 1) ? make_float2(P[e], qc[e]) : make_float2(qc[e], P[e]);
      zb[zaddr[e]] = md_cmul(t, pre[e]);
    }
    md_fence();
    float2 u[8], y[S3][R3];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) u[rr] = zb[mdct_pad(g * Q + LF * rr + lf)];
    core.run(u, zb, g, lf, y);
#pragma unroll
    for (int s = 0; s < S3; ++s)
#pragma unroll
      for (int k3 = 0; k3 < R3; ++k3) {
        const int k = core.kout[s][k3];
        ob[g * M + 2 * k] = y[s][k3].x;
        ob[g * M + M - 1 - 2 * k] = -y[s][k3].y;
      }
    md_fence();
    float* orow = a.out + ((size_t)r * a.F + m_it) * M;
#pragma unroll
    for (int cch = 0; cch < 4; ++cch) {
      const int idx = 4 * (lane + 64 * cch);
      const float4 v = *reinterpret_cast<const float4*>(ob + idx);
      if (m_it + idx / M < m_end) {
        if (out16) __builtin_nontemporal_store(md_v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<md_v4f*>(orow + idx));
        else { orow[idx] = v.x; orow[idx + 1] = v.y; orow[idx + 2] = v.z; orow[idx + 3] = v.w; }
      }
    }
    md_fence();
  }
}

template <int M>
__global__ __launch_bounds__(64 * kMdWaves) void k_imdct_wave(MdWaveArgs a) {
  using Core = MdCore<M>;
  constexpr int LF = Core::LF, G = Core::G, R3 = Core::R3, S3 = Core::S3;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / LF, lf = lane % LF;
  float2* zb = reinterpret_cast<float2*>(md_smem) + wave * kMdBuf;
  float* ob = reinterpret_cast<float*>(zb);
  int64_t r, m0, m_end;
  if (!md_run(a, wave, &r, &m0, &m_end)) return;   // no workgroup barrier anywhere below
  const float* irow = a.in + (size_t)r * a.F * M;
  float* orow = a.out + (size_t)r * a.L;
  const bool in16 = (reinterpret_cast<uintptr_t>(a.in) & 15) == 0, orow16 = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;
  float wa[8], wb[8], wc[8], wd[8];
  float2 pre[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int i = 8 * lf + e;
    wa[e] = a.w[i]; wb[e] = a.w[M - 1 - i]; wc[e] = a.w[M + i]; wd[e] = a.w[2 * M - 1 - i];
    pre[e] = a.tab[LF * e + lf];
  }
  Core core;
  core.init(a.tab, lf);
  // the run stores blocks m0 .. last; the block after a row's last frame has one contribution only.  A run that does not start its
  // row first recomputes the frame before it (one iteration that stores nothing) for that frame's half of block m0
  const int64_t last = m_end == a.F ? a.F : m_end - 1;
  float v2prev[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v2prev[e] = 0.0f;
  for (int64_t m_it = m0 > 0 ? m0 - G : m0; m_it <= last; m_it += G) {
#pragma unroll
    for (int cch = 0; cch < 4; ++cch) {
      const int idx = 4 * (lane + 64 * cch);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // frames at and past the run's end count as zeros and are not read
      if (m_it + idx / M < m_end) {
        const float* p = irow + (size_t)m_it * M + idx;
        if (in16) v = *reinterpret_cast<const float4*>(p);
        else v = make_float4(p[0], p[1], p[2], p[3]);
      }
      *reinterpret_cast<float4*>(ob + idx) = v;
    }
    md_fence();
    float2 u[8], y[S3][R3];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int n = LF * rr + lf;
      u[rr] = md_cmul(make_float2(ob[g * M + 2 * n], ob[g * M + M - 1 - 2 * n]), pre[rr]);
    }
    md_fence();
    core.run(u, zb, g, lf, y);
#pragma unroll
    for (int s = 0; s < S3; ++s)
#pragma unroll
      for (int k3 = 0; k3 < R3; ++k3) {
        const int k = core.kout[s][k3];
        ob[g * M + 2 * k] = y[s][k3].x;
        ob[g * M + M - 1 - 2 * k] = -y[s][k3].y;
      }
    md_fence();
    float v1[8], v2n[8], v2c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { v1[e] = ob[g * M + M / 2 + 8 * lf + e]; v2n[e] = ob[g * M + M / 2 - 1 - 8 * lf - e]; }
    md_fence();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v2c[e] = G == 1 ? v2prev[e] : __shfl(g == G - 1 ? v2prev[e] : v2n[e], (lane - LF) & 63);
      v2prev[e] = v2n[e];
    }
    const int64_t b = m_it + g;
    if (b >= m0 && b <= last) {
      float of[8], obk[8];   // samples i = 8 lf + e and M - 1 - i of block b
  #pragma unroll
      for (int e = 0; e < 8; ++e) {
        of[e] = wa[e] * v1[e] - wc[e] * v2c[e];
        obk[e] = -wb[e] * v1[e] - wd[e] * v2c[e];
      }
      const int64_t base = (b - a.pad) * M;
      if (base >= 0 && base + M <= a.L && orow16) {
        float* p = orow + base;
        __builtin_nontemporal_store(md_v4f{of[0], of[1], of[2], of[3]}, reinterpret_cast<md_v4f*>(p + 8 * lf));
        __builtin_nontemporal_store(md_v4f{of[4], of[5], of[6], of[7]}, reinterpret_cast<md_v4f*>(p + 8 * lf + 4));
        __builtin_nontemporal_store(md_v4f{obk[7], obk[6], obk[5], obk[4]}, reinterpret_cast<md_v4f*>(p + M - 8 - 8 * lf));
        __builtin_nontemporal_store(md_v4f{obk[3], obk[2], obk[1], obk[0]}, reinterpret_cast<md_v4f*>(p + M - 4 - 8 * lf));
      } else {
  #pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int64_t p0 = base + 8 * lf + e, p1 = base + M - 1 - 8 * lf - e;
          if (p0 >= 0 && p0 < a.L) orow[p0] = of[e];
          if (p1 >= 0 && p1 < a.L) orow[p1] = obk[e];
        }
      }
    }
  }
}

// ---- the generic tier: one lane per complex point
// forward: rows in_stride apart -> z[(r F + m) Q + n] = pre[n] (u[2n] + i u[M - 1 - 2n]), u the fold of the windowed frame
__global__ __launch_bounds__(kThreads) void k_mdct_fold(const float* __restrict__ x, int64_t x_stride, int64_t L, int64_t rows, int64_t F, int64_t M,
                                                       int32_t pad, const float* __restrict__ w, const float2* __restrict__ pre, float2* __restrict__ z) {
  const int64_t Q = M / 2, total = rows * F * Q;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t n = i % Q, fm = i / Q, m = fm % F, r = fm / F;
    const float* row = x + (size_t)r * x_stride;
    const int64_t start = (m - pad) * M;
    auto f = [&](int64_t p) { const int64_t at = start + p; return (at >= 0 && at < L) ? w[p] * row[at] : 0.0f; };
    auto u = [&](int64_t j) { int64_t p0, p1; float s0; mdct_fold_pair(j, M, &p0, &p1, &s0); return s0 * f(p0) - f(p1); };
    const float2 t = make_float2(u(2 * n), u(M - 1 - 2 * n)), c = pre[n];
    z[i] = make_float2(t.x * c.x - t.y * c.y, t.x * c.y + t.y * c.x);
  }
}
// inverse: dense coefficient frames -> z[f Q + n] = pre[n] (X[2n] + i X[M - 1 - 2n])
__global__ __launch_bounds__(kThreads) void k_imdct_points(const float* __restrict__ X, int64_t frames, int64_t M, const float2* __restrict__ pre,
                                                          float2* __restrict__ z) {
  const int64_t Q = M / 2, total = frames * Q;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t n = i % Q, fm = i / Q;
    const float2 t = make_float2(X[(size_t)fm * M + 2 * n], X[(size_t)fm * M + M - 1 - 2 * n]), c = pre[n];
    z[i] = make_float2(t.x * c.x - t.y * c.y, t.x * c.y + t.y * c.x);
  }
}
// forward: Z[f Q + k] -> out[f M + 2k] = Re y, out[f M + M - 1 - 2k] = -Im y, y = post[k] Z[k]
__global__ __launch_bounds__(kThreads) void k_mdct_post(const float2* __restrict__ Z, int64_t frames, int64_t M, const float2* __restrict__ post,
                                                       float* __restrict__ out) {
  const int64_t Q = M / 2, total = frames * Q;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t k = i % Q, fm = i / Q;
    const float2 v = Z[i], c = post[k];
    out[(size_t)fm * M + 2 * k] = v.x * c.x - v.y * c.y;
    out[(size_t)fm * M + M - 1 - 2 * k] = -(v.x * c.y + v.y * c.x);
  }
}
// inverse: one lane per output sample adds the (at most) two frames that cover it
__global__ __launch_bounds__(kThreads) void k_imdct_ola(const float2* __restrict__ Z, int64_t rows, int64_t F, int64_t M, int32_t pad, int64_t Lout,
                                                       const float* __restrict__ w, const float2* __restrict__ post, float* __restrict__ out) {
  const int64_t Q = M / 2, total = rows * Lout;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / Lout, s = i - r * Lout + (int64_t)pad * M, b = s / M, rr = s - b * M;
    auto term = [&](int64_t m, int64_t n) {   // w[n] times sample n of frame m
      float sg;
      const int64_t j = mdct_unfold(n, M, &sg), k = (j & 1) ? (M - 1 - j) / 2 : j / 2;
      const float2 v = Z[((size_t)r * F + m) * Q + k], c = post[k];
      const float val = (j & 1) ? -(v.x * c.y + v.y * c.x) : v.x * c.x - v.y * c.y;
      return w[n] * (sg * val);
    };
    float acc = 0.0f;
    if (b < F) acc = term(b, rr);
    if (b >= 1 && b - 1 < F) acc += term(b - 1, M + rr);
    out[i] = acc;
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// one of the tier's own temporaries, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does)
int own_buffer(Ctx* c, Ctx::OwnedBuffer& b, size_t bytes, void** out) {
  if (b.bytes < bytes) {
    if (b.ptr) {
      NXSIG_HIP_TRY(hipStreamSynchronize(c->stream));
      NXSIG_HIP_TRY(hipFree(b.ptr));
      b.ptr = nullptr; b.bytes = 0;
    }
    NXSIG_HIP_TRY(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
  }
  *out = b.ptr;
  return NXSIG_OK;
}

// the window and the twiddles of (M, norm, direction) on the device: double on the host, rounded once; a memo keeps the twiddles' pointer
struct MdTables { const float* w; const float2* tab; };
int device_tables(Ctx* c, const MdctLaunch& a, MdTables* t) {
  const int64_t M = a.N / 2, Q = M / 2;
  const void* dw = nullptr;
  int rc = ctx_table(c, 0x3DC70A00ull, a.window_host, (size_t)a.N * sizeof(float), &dw);
  if (rc) return rc;
  t->w = static_cast<const float*>(dw);
  std::vector<uint64_t> want = {0, (uint64_t)M, (uint64_t)a.norm, (uint64_t)a.inverse};
  const uint64_t key = fnv1a(0x3DC70000ull, want.data() + 1, 3 * sizeof(uint64_t));
  auto hit = c->memo.find(key);
  if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 1, want.end(), hit->second.begin() + 1)) {
    t->tab = reinterpret_cast<const float2*>((uintptr_t)hit->second[0]);
    return NXSIG_OK;
  }
  std::vector<double> d((size_t)6 * Q);
  mdct_tables(M, mdct_scale(M, a.norm, a.inverse), d.data(), d.data() + 2 * Q, d.data() + 4 * Q);
  std::vector<float> f(d.size());
  for (size_t i = 0; i < d.size(); ++i) f[i] = (float)d[i];
  const void* dt = nullptr;
  if ((rc = ctx_table(c, 0x3DC70B00ull, f.data(), f.size() * sizeof(float), &dt))) return rc;
  want[0] = (uint64_t)(uintptr_t)dt;
  c->memo[key] = want;
  t->tab = static_cast<const float2*>(dt);
  return NXSIG_OK;
}

template <int M>
int run_wave(Ctx* c, const MdctLaunch& a, const MdTables& t) {
  MdWaveArgs w;
  w.in = a.in; w.out = a.out; w.w = t.w; w.tab = t.tab;
  w.in_stride = a.in_stride; w.L = a.length; w.F = a.frames; w.pad = a.pad;
  w.run = mdct_run_frames(a.frames, a.batch, (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 2 * kMdWaves, M);   // two workgroups per CU are resident (190-odd VGPRs)
  w.runs_per_row = (a.frames + w.run - 1) / w.run;
  w.total_runs = w.runs_per_row * a.batch;
  const int64_t blocks = (w.total_runs + kMdWaves - 1) / kMdWaves;
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "mdct: too many frames for one launch");
  dispatch_note(a.inverse ? "imdct.wave" : "mdct.wave");
  if (a.inverse) hipLaunchKernelGGL(k_imdct_wave<M>, dim3((unsigned)blocks), dim3(64 * kMdWaves), (size_t)mdct_lds_bytes(), c->stream, w);
  else hipLaunchKernelGGL(k_mdct_wave<M>, dim3((unsigned)blocks), dim3(64 * kMdWaves), (size_t)mdct_lds_bytes(), c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

int run_generic(Ctx* c, const MdctLaunch& a, const MdTables& t) {
  const int64_t M = a.N / 2, Q = M / 2, frames = a.batch * a.frames;
  if (Q > 0x7fffffffLL || frames > ((int64_t)1 << 40)) return set_error(NXSIG_ERR_UNSUPPORTED, "mdct: too many points for the row transforms");
  const size_t bytes = (size_t)frames * Q * sizeof(float2);
  void *pts = nullptr, *spec = nullptr;
  int rc = own_buffer(c, c->mdct_points, bytes, &pts);
  if (rc) return rc;
  if (Q > 1 && (rc = own_buffer(c, c->mdct_spectra, bytes, &spec))) return rc;
  float2* z = static_cast<float2*>(pts);
  dispatch_note(a.inverse ? "imdct.generic" : "mdct.generic");
  const unsigned pb = stream_blocks(c, frames * Q);
  if (a.inverse) hipLaunchKernelGGL(k_imdct_points, dim3(pb), dim3(kThreads), 0, c->stream, a.in, frames, M, t.tab, z);
  else hipLaunchKernelGGL(k_mdct_fold, dim3(pb), dim3(kThreads), 0, c->stream, a.in, a.in_stride, a.length, a.batch, a.frames, M, a.pad, t.w, t.tab, z);
  NXSIG_HIP_TRY(hipGetLastError());
  const float2* Z = z;   // a one-point transform is the point itself
  if (Q > 1) {
    if ((rc = launch_fft(c, z, false, frames, (int32_t)Q, (int32_t)Q, false, static_cast<float2*>(spec), false))) return rc;
    Z = static_cast<const float2*>(spec);
  }
  if (a.inverse) hipLaunchKernelGGL(k_imdct_ola, dim3(stream_blocks(c, a.batch * a.length)), dim3(kThreads), 0, c->stream, Z, a.batch, a.frames, M, a.pad,
                                    a.length, t.w, t.tab + Q, a.out);
  else hipLaunchKernelGGL(k_mdct_post, dim3(pb), dim3(kThreads), 0, c->stream, Z, frames, M, t.tab + Q, a.out);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace

int launch_mdct(Ctx* c, const MdctLaunch& a) {
  if (a.batch == 0) return NXSIG_OK;
  MdTables t;
  const int rc = device_tables(c, a, &t);
  if (rc) return rc;
  const bool wave_off = tune(c, kT_MDCT_WAVE, 1) == 0 || tune(c, kT_DISABLE_WAVE, 0) != 0;
  const int64_t M = a.N / 2;
  if (mdct_tier(M, wave_off) == kMdGeneric) return run_generic(c, a, t);
  return M == 256 ? run_wave<256>(c, a, t) : (M == 512 ? run_wave<512>(c, a, t) : run_wave<1024>(c, a, t));
}

}  // namespace nxsig
