// Spectral.lpc: Burg's linear prediction of every frame of f32 rows, what librosa.lpc computes (in double, the denominator summed afresh
// at every stage).  include/nxsig.h states the definition, DESIGN.md section 3.25 the design; the checks, the frame count, the tier
// choice and the geometry are csrc/lpc_plan.hpp.
// A frame of L samples is L - 1 pairs (f[j], b[j]) = (x[j + 1], x[j]); stage m forms k_m = -2 sum f b / (sum f f + sum b b + tiny) over
// the L - 1 - m pairs left and replaces pair j by (f[j + 1] + k b[j + 1], b[j] + k f[j]): f moves one place against b per stage.
//   lpc.wave   one wave owns one frame from load to store (L <= 2048), the pairs BLOCKED over its lanes: lane l holds pairs
//              l R ... l R + R - 1 in 2 R double registers (R = 2, 8, 16 or 32).  The shift costs no instruction: the update of slot s
//              is WRITTEN to slot s - 1 (F[s - 1] = fma(k, B[s], F[s]) while B[s] = fma(k, F[s], B[s]) stays), and the one value
//              that leaves a lane at slot 0 is fetched by the lane below it (one 64-bit lane shift per stage).  Pairs past the end
//              hold zeros, so the sums need no mask; the update makes exactly one of them non-zero (b of the pair that just
//              left), and that one is put back to zero: its slot is the same in every lane, so a scalar branch finds it.
//              The two sums cross the wave in double in a fixed order (four DPP steps inside a row of 16 lanes, then the four
//              rows' sums through scalar registers).  No LDS in the stage loop; the k_m wait in LDS for the step-up of a, which
//              the same wave does at the end (a in three registers per lane, the reversed operand through LDS).
//   lpc.rows   every longer frame and everything under NXSIG_LPC_WAVE=0: f and b in double in a temporary of the context, one launch
//              per stage over (frame, chunk of 4096 pairs) units.  f stays where it is and is READ at a moving offset (pair j of
//              stage m is (F[j + m], B[j])), so nothing is shifted; a stage reads one copy of (F, B) and writes the other, because
//              a pair's new f comes from its neighbour's old values.  Launch m applies stage m - 1 and writes the chunk's two
//              partial sums of stage m; every workgroup of launch m + 1 adds its frame's partials in the same fixed order to get
//              k_m: no atomics, no host round trip, and the same bits on any grid.  A last launch steps a up.
// Non-finite rule: an Inf / NaN sample makes the sums of its frames non-finite, hence k_0 and with it every output of those frames,
// a[0] included (1 + k 0); frames share no arithmetic.
#include <cfloat>

#include "nxsig_internal.h"

namespace nxsig {

namespace {

constexpr int kThreads = 64 * kLpcWaves;
constexpr int kLpcASlots = (kLpcMaxOrder + 64) / 64;   // coefficients a[lane + 64 q] per lane: 3

struct LpcArgs {
  const float* x;       // f32 rows, `stride` elements apart
  float* a;             // f32 [batch F][p + 1]
  float* k;             // f32 [batch F][p] or null
  float* e;             // f32 [batch F] or null
  double* tmp;          // lpc.rows: the slab's temporary
  int64_t stride, L, hop, F;   // F: frames per row
  int64_t total;        // batch F
  int64_t frame0, frames, chunks;   // lpc.rows: the slab's first frame (of `total`), its frames, chunks per frame
  int32_t p;
};

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// the sum of a value over the 64 lanes, the same bits in every lane: partners exchange inside quads, half rows and rows of 16 (each
// step adds the two halves of a group, so both partners form the same sum), then ((r0 + r1) + (r2 + r3)) of the four rows.  All 64
// lanes must be active
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return (lane_f64(v, 0) + lane_f64(v, 16)) + (lane_f64(v, 32) + lane_f64(v, 48));
}
// the value of the lane above; `last` in lane 63
__device__ __forceinline__ double from_lane_above(double v, int lane, double last) {
  const double o = __shfl_down(v, 1, 64);
  return lane == 63 ? last : o;
}

__device__ __forceinline__ double lpc_reflection(double num, double den) { return -2.0 * num / (den + DBL_MIN); }

// the end of a frame, by one wave: a stepped up from the p reflection coefficients in s_k (a[i] in lane i % 64, register i / 64; the
// reversed operand a[m + 1 - i] goes through s_a), e = e0 prod (1 - k^2), and the stores
__device__ __forceinline__ void lpc_finish(double* s_a, const double* s_k, int p, int lane, double e0, const LpcArgs& g, int64_t frame) {
  double av[kLpcASlots];
#pragma unroll
  for (int q = 0; q < kLpcASlots; ++q) av[q] = lane + 64 * q == 0 ? 1.0 : 0.0;
  double shrink = 1.0;
  for (int m = 0; m < p; ++m) {
#pragma unroll
    for (int q = 0; q < kLpcASlots; ++q) s_a[lane + 64 * q] = av[q];
    __builtin_amdgcn_wave_barrier();
    const double k = s_k[m];
#pragma unroll
    for (int q = 0; q < kLpcASlots; ++q) {
      const int i = lane + 64 * q;
      if (i <= m + 1) av[q] = __builtin_fma(k, s_a[m + 1 - i], av[q]);
    }
    __builtin_amdgcn_wave_barrier();
    shrink *= 1.0 - k * k;
  }
  float* ao = g.a + frame * (p + 1);
#pragma unroll
  for (int q = 0; q < kLpcASlots; ++q)
    if (lane + 64 * q <= p) ao[lane + 64 * q] = (float)av[q];
  if (g.k)
    for (int i = lane; i < p; i += 64) g.k[frame * p + i] = (float)s_k[i];
  if (g.e && lane == 0) g.e[frame] = (float)(e0 * shrink);
}

// ---------------------------------------------------------------- lpc.wave
template <int R>
__global__ __launch_bounds__(kThreads) void k_lpc_wave(LpcArgs g) {
  __shared__ double s_a[kLpcWaves][64 * kLpcASlots];
  __shared__ double s_k[kLpcWaves][kLpcMaxOrder];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int64_t frame = (int64_t)blockIdx.x * kLpcWaves + wave;
  if (frame >= g.total) return;   // the whole wave
  const float* xf = g.x + (frame / g.F) * g.stride + (frame % g.F) * g.hop;
  const int L = (int)g.L, p = g.p, base = lane * R;

  // the lane's R samples x[base ... base + R - 1], zeros from L on: 16-byte loads where the frame starts on a 16-byte boundary
  float xs[R];
  constexpr int V = R % 4 == 0 ? 4 : 1;
  const bool wide = V == 4 && reinterpret_cast<uintptr_t>(xf) % 16 == 0;
#pragma unroll
  for (int v = 0; v < R; v += V) {
    const int i = base + v;
    if (wide && i + V <= L) {
      const float4 q = *reinterpret_cast<const float4*>(xf + i);
      xs[v] = q.x; xs[v + V / 4] = q.y; xs[v + V / 2] = q.z; xs[v + V - 1] = q.w;
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u) xs[v + u] = i + u < L ? xf[i + u] : 0.0f;
    }
  }
  const double tail = 64 * R < L ? (double)xf[64 * R] : 0.0;   // L - 1 = 64 R: the last pair's f is a sample no lane holds
  double F[R], B[R], xx = lane == 63 ? tail * tail : 0.0;
  const double next = from_lane_above((double)xs[0], lane, tail);
#pragma unroll
  for (int s = 0; s < R; ++s) {
    xx = __builtin_fma((double)xs[s], (double)xs[s], xx);
    F[s] = s + 1 < R ? (double)xs[s + 1 < R ? s + 1 : s] : next;   // x[j + 1]: zero from pair L - 1 on by the load
    B[s] = base + s < L - 1 ? (double)xs[s] : 0.0;                 // x[j]: pair L - 1 does not exist
  }
  const double e0 = wave_sum(xx) / (double)L;

  for (int m = 0; m < p; ++m) {
    double num = 0.0, ff = 0.0, bb = 0.0;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      num = __builtin_fma(F[s], B[s], num);
      ff = __builtin_fma(F[s], F[s], ff);
      bb = __builtin_fma(B[s], B[s], bb);
    }
    const double k = lpc_reflection(wave_sum(num), wave_sum(ff + bb));
    if (lane == 0) s_k[wave][m] = k;
    if (m + 1 == p) break;   // the pairs are not needed again
    const double out = __builtin_fma(k, B[0], F[0]);   // leaves the lane: the new f of the lane below's last slot
    B[0] = __builtin_fma(k, F[0], B[0]);
#pragma unroll
    for (int s = 1; s < R; ++s) {
      const double nf = __builtin_fma(k, B[s], F[s]);
      B[s] = __builtin_fma(k, F[s], B[s]);
      F[s - 1] = nf;
    }
    F[R - 1] = from_lane_above(out, lane, 0.0);
    // pair L - 2 - m has just left: its f is zero already (it came from a zero pair), its b is not
    const int gone = L - 2 - m;
    const int slot = __builtin_amdgcn_readfirstlane(gone % R), owner = gone / R;
#pragma unroll
    for (int s = 0; s < R; ++s)
      if (s == slot) {
        asm volatile("");   // keeps this a scalar branch: as a select it would cost two moves per slot and stage
        B[s] = lane == owner ? 0.0 : B[s];
      }
  }
  __builtin_amdgcn_wave_barrier();
  lpc_finish(s_a[wave], s_k[wave], p, lane, e0, g, frame);
}

// ---------------------------------------------------------------- lpc.rows
// the temporary of a slab of `frames` frames, in doubles (lpc_frame_doubles() per frame): (F, B) of P = L - 1 pairs per frame and stage
// parity, the chunks' (num, den) per parity, the chunks' sums of x^2, the reflection coefficients
struct LpcTmp {
  double *fb0, *part0, *xx, *kb;
  int64_t fb_step, part_step;
  __device__ LpcTmp(const LpcArgs& g, int64_t fs) {
    const int64_t P = g.L - 1;
    double* t = g.tmp;
    fb0 = t + fs * 2 * P; fb_step = g.frames * 2 * P; t += 4 * g.frames * P;
    part0 = t + fs * 2 * g.chunks; part_step = g.frames * 2 * g.chunks; t += 4 * g.frames * g.chunks;
    xx = t + fs * g.chunks; t += g.frames * g.chunks;
    kb = t + fs * g.p;
  }
  __device__ double* fb(int stage) const { return fb0 + (stage & 1) * fb_step; }       // F at [0, P), B at [P, 2 P)
  __device__ double* part(int stage) const { return part0 + (stage & 1) * part_step; }  // (num, den) per chunk
};

// the sum of one value per thread over the workgroup in a fixed order, the same bits in every thread
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = (int)threadIdx.x;
  __syncthreads();   // sh may still be read from the sum before
  sh[t] = v;
  __syncthreads();
  for (int off = kLpcRowsThreads / 2; off > 0; off >>= 1) {
    if (t < off) sh[t] += sh[t + off];
    __syncthreads();
  }
  return sh[0];
}

// launch m of a slab: k_{m - 1} from the partial sums of stage m - 1, its update applied to the chunk's pairs of stage m (launch 0 forms
// them from x), the chunk's partial sums of stage m
__global__ __launch_bounds__(kLpcRowsThreads) void k_lpc_rows_stage(LpcArgs g, int m) {
  __shared__ double sh[kLpcRowsThreads];
  const int t = (int)threadIdx.x;
  const int64_t fs = (int64_t)blockIdx.x / g.chunks, chunk = (int64_t)blockIdx.x % g.chunks;
  const int64_t frame = g.frame0 + fs, P = g.L - 1;
  const LpcTmp tmp(g, fs);
  const int64_t left = P - m;   // pairs of stage m
  const int64_t j0 = chunk * kLpcChunk, j1 = j0 + kLpcChunk < left ? j0 + kLpcChunk : left;
  double* dst = tmp.fb(m);
  double num = 0.0, den = 0.0;
  if (m == 0) {
    const float* xf = g.x + (frame / g.F) * g.stride + (frame % g.F) * g.hop;
    double xx = 0.0;
    for (int64_t j = j0 + t; j < j1; j += kLpcRowsThreads) {
      const double b = (double)xf[j], f = (double)xf[j + 1];
      dst[j] = f; dst[P + j] = b;
      num = __builtin_fma(f, b, num); den = __builtin_fma(f, f, den); den = __builtin_fma(b, b, den);
      xx = __builtin_fma(b, b, xx);
      if (j == P - 1) xx = __builtin_fma(f, f, xx);   // the last sample is no pair's b
    }
    xx = block_sum(xx, sh);
    if (t == 0) tmp.xx[chunk] = xx;
  } else {
    const double* pp = tmp.part(m - 1);
    double pn = 0.0, pd = 0.0;
    for (int64_t c = t; c < g.chunks; c += kLpcRowsThreads) { pn += pp[2 * c]; pd += pp[2 * c + 1]; }
    pn = block_sum(pn, sh);
    pd = block_sum(pd, sh);
    const double k = lpc_reflection(pn, pd);
    if (chunk == 0 && t == 0) tmp.kb[m - 1] = k;
    const double* src = tmp.fb(m - 1);
    for (int64_t j = j0 + t; j < j1; j += kLpcRowsThreads) {   // pair j of stage m - 1 is (src[j + m - 1], src[P + j])
      const double f = __builtin_fma(k, src[P + j + 1], src[j + m]);
      const double b = __builtin_fma(k, src[j + m - 1], src[P + j]);
      dst[j + m] = f; dst[P + j] = b;
      num = __builtin_fma(f, b, num); den = __builtin_fma(f, f, den); den = __builtin_fma(b, b, den);
    }
  }
  num = block_sum(num, sh);
  den = block_sum(den, sh);
  if (t == 0) { double* po = tmp.part(m); po[2 * chunk] = num; po[2 * chunk + 1] = den; }
}

// the last launch of a slab, one wave per frame: k_{p - 1}, the energy, the step-up, the stores
__global__ __launch_bounds__(64) void k_lpc_rows_final(LpcArgs g) {
  __shared__ double s_a[64 * kLpcASlots];
  __shared__ double s_k[kLpcMaxOrder];
  const int lane = (int)threadIdx.x, p = g.p;
  const int64_t fs = blockIdx.x;
  const LpcTmp tmp(g, fs);
  const double* pp = tmp.part(p - 1);
  double pn = 0.0, pd = 0.0, xx = 0.0;
  for (int64_t c = lane; c < g.chunks; c += 64) { pn += pp[2 * c]; pd += pp[2 * c + 1]; xx += tmp.xx[c]; }
  const double k = lpc_reflection(wave_sum(pn), wave_sum(pd));
  xx = wave_sum(xx);
  for (int i = lane; i < p; i += 64) s_k[i] = i == p - 1 ? k : tmp.kb[i];
  __builtin_amdgcn_wave_barrier();
  lpc_finish(s_a, s_k, p, lane, xx / (double)g.L, g, g.frame0 + fs);
}

// the family's own temporary, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does)
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

template <int R>
int run_wave(Ctx* c, const LpcArgs& g) {
  const int64_t blocks = (g.total + kLpcWaves - 1) / kLpcWaves;
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "lpc: too many frames for one launch");
  hipLaunchKernelGGL(k_lpc_wave<R>, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, g);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

int run_rows(Ctx* c, LpcArgs g) {
  g.chunks = lpc_chunks(g.L);
  const int64_t slab = lpc_slab_frames(g.total, g.L, g.p);
  void* tmp = nullptr;
  int rc = own_buffer(c, c->lpc_tmp, (size_t)slab * lpc_frame_doubles(g.L, g.p) * sizeof(double), &tmp);
  if (rc) return rc;
  g.tmp = static_cast<double*>(tmp);
  for (g.frame0 = 0; g.frame0 < g.total; g.frame0 += slab) {
    g.frames = g.total - g.frame0 < slab ? g.total - g.frame0 : slab;
    for (int m = 0; m < g.p; ++m) {
      hipLaunchKernelGGL(k_lpc_rows_stage, dim3((unsigned)(g.frames * g.chunks)), dim3(kLpcRowsThreads), 0, c->stream, g, m);
      NXSIG_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lpc_rows_final, dim3((unsigned)g.frames), dim3(64), 0, c->stream, g);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

}  // namespace

int launch_lpc(Ctx* c, const LpcLaunch& l) {
  LpcArgs g = {};
  g.x = static_cast<const float*>(l.x); g.a = static_cast<float*>(l.a); g.k = static_cast<float*>(l.k); g.e = static_cast<float*>(l.e);
  g.stride = l.x_stride; g.L = l.frame_length; g.hop = l.hop; g.p = (int32_t)l.order;
  g.F = lpc_frames(l.n, l.frame_length, l.hop);
  g.total = l.batch * g.F;
  if (g.total == 0) return NXSIG_OK;
  const bool wave_on = tune(c, kT_LPC_WAVE, 1) != 0 && tune(c, kT_DISABLE_WAVE, 0) == 0;
  if (lpc_tier(g.L, wave_on) == kLpcRows) {
    dispatch_note("lpc.rows");
    return run_rows(c, g);
  }
  dispatch_note("lpc.wave");
  switch (lpc_slots(g.L)) {
    case 2: return run_wave<2>(c, g);
    case 8: return run_wave<8>(c, g);
    case 16: return run_wave<16>(c, g);
    default: return run_wave<32>(c, g);
  }
}

}  // namespace nxsig
