// Transforms.phase_vocoder: the time base of a c64 spectrogram [batch][M][K] changed by `rate`, as librosa.phase_vocoder and
// torchaudio.functional.phase_vocoder do.  include/nxsig.h states the definition, DESIGN.md section 3.24 the design; the checks, the
// frame count, the step function t -> (i_t, alpha_t) and the chunk geometry are csrc/pvoc_plan.hpp.
// The accumulated phase is carried as a unit PHASOR in double, U[t + 1] = U[t] u(z[i_t + 1]) conj(u(z[i_t])) with u(z) = z / |z|: an
// associative product with no transcendental, so a row's time axis can be cut into chunks.
//   work split       a lane owns two adjacent bins (16-byte loads and non-temporal stores; the W = 1 instantiation owns one bin with
//                    8-byte accesses, for odd K and misaligned bases) and a wave walks time: nothing crosses a lane, so there is no
//                    LDS, no DPP and no matrix instruction here.  A unit is (row, chunk of C output frames, tile of 64 lanes' bins).
//   registers        the pair (z[i], z[i + 1]) with |z| and u(z) formed ONCE per loaded frame, the rotor u(z[i + 1]) conj(u(z[i])) of
//                    the pair, the phasor, and the next kPvDepth input frames the walk will need, loaded ahead of use (the index
//                    sequence is arithmetic).  An unchanged i_t loads nothing; i_t + 1 turns the second frame into the first.
//   pvoc.walk        n_out <= C: one launch, a unit starts at u(z[0]).
//   pvoc.scan        (A) k_pvoc_aggregate: the product of a chunk's rotors, c128 [batch][chunks][K] (the last chunk's is
//                    never needed and not formed); (B) k_pvoc_carry: one thread per (row, bin) turns them in place into the
//                    exclusive prefix that starts at u(z[0, k]), sequentially over the chunks, so every run gives the same bits;
//                    (C) k_pvoc_emit: a unit starts from its carry and writes its C frames.  Three launches on one stream:
//                    no workgroup waits on another.  The price is that z is read twice.
// Non-finite rule: an Inf / NaN in the pair of step t makes the interpolated magnitude and the rotor non-finite, so that bin's
// output is non-finite at t and its phasor (and every later chunk's carry) from t + 1 on; bins share no arithmetic.
#include "nxsig_internal.h"

namespace nxsig {

namespace {

constexpr int kThreads = 64 * kPvWaves;
enum PvMode : int { kPvWalk = 0, kPvAggregate = 1, kPvEmit = 2 };

typedef float pv_v4f __attribute__((ext_vector_type(4)));   // what the non-temporal store builtin takes
typedef float pv_v2f __attribute__((ext_vector_type(2)));

struct PvArgs {
  const float* z;       // c64 [batch][M][K]
  float* out;           // c64 [batch][n_out][K]
  double* carry;        // c128 [batch][chunks][K]
  int64_t batch, M, K, n_out, C, chunks, tiles;
  int64_t chunks_run;   // chunks of a row this launch covers: `chunks`, or chunks - 1 for the aggregates
  double rate;
};

// one loaded input frame of one bin: |z| and u(z) = z / |z|, u(0) = 1 for a zero of either sign.  s = x^2 + y^2 of f32 values neither
// overflows nor underflows in double (2e-90 ... 2.4e77), so ONE reciprocal square root serves both: r = 1 / sqrt(s) from the
// hardware's estimate and two Newton steps (its error squared twice is below a double's rounding), |z| = s r, u = z r.  An Inf gives
// r = 0 and NaNs, a NaN stays one: the bin is non-finite either way
struct PvBin { double m, ux, uy; };
__device__ __forceinline__ PvBin pv_form(float re, float im) {
  const double x = (double)re, y = (double)im;
  const double s = x * x + y * y;
  double r = __builtin_amdgcn_rsq(s);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double h = __builtin_fma(-0.5 * (s * r), r, 0.5);
    r = __builtin_fma(r, h, r);
  }
  const bool zero = s == 0.0;
  PvBin b;
  b.m = zero ? 0.0 : s * r;
  b.ux = zero ? 1.0 : x * r;
  b.uy = zero ? 0.0 : y * r;
  return b;
}

template <int W> struct PvRaw { float v[2 * W]; };
// frame f of the lane's bins, zeros past `flast` (the last frame the unit uses; frames M and M + 1 count as zeros and are never read)
template <int W>
__device__ __forceinline__ PvRaw<W> pv_load(const float* col, int64_t f, int64_t flast, int64_t K, bool lane_ok) {
  PvRaw<W> r;
#pragma unroll
  for (int j = 0; j < 2 * W; ++j) r.v[j] = 0.0f;
  if (lane_ok && f <= flast) {
    const float* p = col + 2 * f * K;
    if (W == 2) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      r.v[0] = v.x; r.v[1] = v.y; r.v[W] = v.z; r.v[2 * W - 1] = v.w;
    } else {
      const float2 v = *reinterpret_cast<const float2*>(p);
      r.v[0] = v.x; r.v[1] = v.y;
    }
  }
  return r;
}

template <int W, int MODE>
__device__ __forceinline__ void pv_unit(const PvArgs& a) {
  // the unit of this wave: tile fastest, then chunk, then row.  Everything about time is the same in all 64 lanes
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int64_t unit = (int64_t)blockIdx.x * kPvWaves + wave;
  const int64_t tile = unit % a.tiles, chunk = (unit / a.tiles) % a.chunks_run, row = unit / (a.tiles * a.chunks_run);
  if (row >= a.batch) return;
  const int64_t bin = (tile * 64 + lane) * W;
  const bool lane_ok = bin + W <= a.K;
  const int64_t t0 = chunk * a.C, t1 = t0 + a.C < a.n_out ? t0 + a.C : a.n_out;
  const double rate = a.rate;
  const float* col = a.z + 2 * (row * a.M * a.K + bin);

  int64_t cur, flast;   // cur: the frame held as the pair's first
  double alpha;
  pvoc_step(t1 - 1, rate, &flast, &alpha);
  flast = flast + 1 < a.M - 1 ? flast + 1 : a.M - 1;
  pvoc_step(t0, rate, &cur, &alpha);

  // the frames the walk needs, in order: for t = t0, t0 + 1, ... those of {i_t, i_t + 1} above the last one taken
  int64_t made = cur - 1, tp = t0;
  auto next_frame = [&]() -> int64_t {
    while (tp < t1) {
      int64_t i; double al;
      pvoc_step(tp, rate, &i, &al);
      if (made < i) return made = i;
      if (made < i + 1) return made = i + 1;
      ++tp;
    }
    return ++made;   // past the unit's last pair: above flast, so never loaded and never used
  };
  PvRaw<W> q[kPvDepth];
#pragma unroll
  for (int d = 0; d < kPvDepth; ++d) q[d] = pv_load<W>(col, next_frame(), flast, a.K, lane_ok);
  auto pop = [&](PvBin* dst) {
#pragma unroll
    for (int j = 0; j < W; ++j) dst[j] = pv_form(q[0].v[2 * j], q[0].v[2 * j + 1]);
#pragma unroll
    for (int d = 0; d + 1 < kPvDepth; ++d) q[d] = q[d + 1];
    q[kPvDepth - 1] = pv_load<W>(col, next_frame(), flast, a.K, lane_ok);
  };

  PvBin A[W], B[W];
  double Rx[W], Ry[W], Ux[W], Uy[W];
  pop(A);
  pop(B);
  auto rotor = [&]() {
#pragma unroll
    for (int j = 0; j < W; ++j) {   // u(B) conj(u(A))
      Rx[j] = B[j].ux * A[j].ux + B[j].uy * A[j].uy;
      Ry[j] = B[j].uy * A[j].ux - B[j].ux * A[j].uy;
    }
  };
  rotor();
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (MODE == kPvWalk) { Ux[j] = A[j].ux; Uy[j] = A[j].uy; }   // t0 = 0: the pair's first frame is z[0]
    else if (MODE == kPvAggregate) { Ux[j] = 1.0; Uy[j] = 0.0; }
    else {
      Ux[j] = 1.0; Uy[j] = 0.0;
      if (lane_ok) {
        const double2 u = *reinterpret_cast<const double2*>(a.carry + 2 * ((row * a.chunks + chunk) * a.K + bin + j));
        Ux[j] = u.x; Uy[j] = u.y;
      }
    }
  }

  float* op = a.out + 2 * ((row * a.n_out + t0) * a.K + bin);
  double td = (double)t0, curd = (double)cur;   // the walk's own steps stay in double: whole numbers below 2^53 are exact
  for (int64_t n = t1 - t0; n > 0; --n, td += 1.0, op += 2 * a.K) {
    double fd;
    pvoc_step_d(td, rate, &fd, &alpha);
    if (fd != curd) {
      if (fd == curd + 1.0) {
#pragma unroll
        for (int j = 0; j < W; ++j) A[j] = B[j];
      } else {
        pop(A);
      }
      pop(B);
      curd = fd;
      rotor();
    }
    if (MODE != kPvAggregate) {
      float o[2 * W];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double mag = (1.0 - alpha) * A[j].m + alpha * B[j].m;
        o[2 * j] = (float)(mag * Ux[j]);
        o[2 * j + 1] = (float)(mag * Uy[j]);
      }
      if (lane_ok) {
        if (W == 2) {
          pv_v4f v = {o[0], o[1], o[W], o[2 * W - 1]};
          __builtin_nontemporal_store(v, reinterpret_cast<pv_v4f*>(op));
        } else {
          pv_v2f v = {o[0], o[1]};
          __builtin_nontemporal_store(v, reinterpret_cast<pv_v2f*>(op));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double nx = Ux[j] * Rx[j] - Uy[j] * Ry[j], ny = Ux[j] * Ry[j] + Uy[j] * Rx[j];
      Ux[j] = nx; Uy[j] = ny;
    }
  }
  if (MODE == kPvAggregate && lane_ok) {
#pragma unroll
    for (int j = 0; j < W; ++j)
      *reinterpret_cast<double2*>(a.carry + 2 * ((row * a.chunks + chunk) * a.K + bin + j)) = make_double2(Ux[j], Uy[j]);
  }
}

template <int W> __global__ __launch_bounds__(kThreads) void k_pvoc_walk(PvArgs a) { pv_unit<W, kPvWalk>(a); }
template <int W> __global__ __launch_bounds__(kThreads) void k_pvoc_aggregate(PvArgs a) { pv_unit<W, kPvAggregate>(a); }
template <int W> __global__ __launch_bounds__(kThreads) void k_pvoc_emit(PvArgs a) { pv_unit<W, kPvEmit>(a); }

// (B) of pvoc.scan: the aggregates of a (row, bin) become, in place, the phasor each chunk starts from.  One thread walks the chunks
// of its bin in order; neighbouring threads hold neighbouring bins, so every access is coalesced
__global__ __launch_bounds__(256) void k_pvoc_carry(const float* __restrict__ z, double* carry, int64_t batch, int64_t M, int64_t K, int64_t chunks) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * K) return;
  const int64_t row = idx / K, k = idx % K;
  const float2 z0 = *reinterpret_cast<const float2*>(z + 2 * (row * M * K + k));
  const PvBin s = pv_form(z0.x, z0.y);
  double ux = s.ux, uy = s.uy;
  double2* p = reinterpret_cast<double2*>(carry) + row * chunks * K + k;
  for (int64_t c = 0; c < chunks; ++c, p += K) {
    double2 g = make_double2(1.0, 0.0);
    if (c + 1 < chunks) g = *p;   // the last chunk has no aggregate
    *p = make_double2(ux, uy);
    const double nx = ux * g.x - uy * g.y, ny = ux * g.y + uy * g.x;
    ux = nx; uy = ny;
  }
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

template <int W, int MODE>
int run_walk(Ctx* c, const PvArgs& w) {
  const int64_t blocks = (w.batch * w.chunks_run * w.tiles + kPvWaves - 1) / kPvWaves;
  if (blocks > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "phase_vocoder: too many units for one launch");
  auto* kernel = MODE == kPvWalk ? k_pvoc_walk<W> : (MODE == kPvAggregate ? k_pvoc_aggregate<W> : k_pvoc_emit<W>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, w);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <int W>
int run(Ctx* c, PvArgs w) {
  if (w.chunks == 1) {
    dispatch_note("pvoc.walk");
    return run_walk<W, kPvWalk>(c, w);
  }
  void* carry = nullptr;
  int rc = own_buffer(c, c->pvoc_carry, (size_t)w.batch * w.chunks * w.K * 2 * sizeof(double), &carry);
  if (rc) return rc;
  w.carry = static_cast<double*>(carry);
  dispatch_note("pvoc.scan");
  w.chunks_run = w.chunks - 1;
  if ((rc = run_walk<W, kPvAggregate>(c, w))) return rc;
  const int64_t cb = (w.batch * w.K + 255) / 256;
  if (cb > 0x7fffffffLL) return set_error(NXSIG_ERR_UNSUPPORTED, "phase_vocoder: too many bins for one launch");
  hipLaunchKernelGGL(k_pvoc_carry, dim3((unsigned)cb), dim3(256), 0, c->stream, w.z, w.carry, w.batch, w.M, w.K, w.chunks);
  NXSIG_HIP_TRY(hipGetLastError());
  w.chunks_run = w.chunks;
  return run_walk<W, kPvEmit>(c, w);
}

}  // namespace

int launch_pvoc(Ctx* c, const PvocLaunch& a) {
  if (a.batch == 0) return NXSIG_OK;
  PvArgs w;
  w.z = static_cast<const float*>(a.z); w.out = static_cast<float*>(a.out); w.carry = nullptr;
  w.batch = a.batch; w.M = a.frames; w.K = a.bins; w.rate = a.rate;
  w.n_out = pvoc_frames(a.frames, a.rate);
  w.C = pvoc_chunk_frames(w.n_out, a.batch, a.bins, tune(c, kT_PVOC_CHUNK, 0));
  w.chunks = w.chunks_run = pvoc_chunks(w.n_out, w.C);
  const bool wide = pvoc_wide(a.bins, reinterpret_cast<uintptr_t>(a.z), reinterpret_cast<uintptr_t>(a.out));
  w.tiles = pvoc_tiles(a.bins, wide);
  return wide ? run<kPvWide>(c, w) : run<1>(c, w);
}

}  // namespace nxsig
