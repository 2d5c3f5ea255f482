// NxSignal.Waveforms: sawtooth/2, square/2, gaussian_pulse/2, chirp/5, polynomial_sweep/3 and unit_impulse/2
// (lib/nx_signal/waveforms.ex) as elementwise kernels.
//
// Numbers.  The f32 tier evaluates every Nx op in double on f32-rounded operands and rounds the result back to f32 (Rnd<float>: the
// BinaryBackend rule of host_numerics.cpp / SURVEY Appendix A); the f64 tier is the same expression with Rnd<double>, the identity.
// Transcendentals are the double functions.  No FMA contraction in this file: the reference rounds between a multiply and an add.
// Every scalar that does not depend on t (thresholds, a of gaussian_pulse, the chirp factors, the integrated coefficients of
// polynomial_sweep) is computed once by the caller in api.cpp and arrives by value.
//
// One driver, k_wave_elem<Op>: 64-bit element indices, a grid-stride loop over groups of four elements.  The group boundary is put
// where the first output is 16-byte aligned; the elements before it (at most three) and after the last whole group are done one by
// one.  Every stream whose pointer is 16-byte aligned at that boundary moves in 16-byte loads / stores, any other (a view offset by
// one element) element by element; both give the same bits.  No atomics, no LDS, no scratch.
// Dispatch families: waveform.sawtooth, waveform.square, waveform.gaussian_pulse, waveform.chirp.<method>, waveform.polynomial_sweep,
// waveform.unit_impulse.
#pragma clang fp contract(off)

#include <type_traits>

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kThreads = 256, kGroup = 4;   // elements per group: one 16-byte access of f32 / s32, two of f64
constexpr int kBlocksPerCu = 8;             // 2048 threads per CU, the grid-stride loop takes the rest

template <typename T> struct Rnd {
  __device__ static __forceinline__ double r(double x) {
    if constexpr (std::is_same<T, float>::value) return (double)(float)x;
    else return x;
  }
};

template <typename T> using Pack = T __attribute__((ext_vector_type(16 / sizeof(T))));   // one 16-byte access

// kGroup elements from / to p, in 16-byte accesses when p is 16-byte aligned (al)
template <typename T> __device__ __forceinline__ void load_group(const T* __restrict__ p, bool al, T (&v)[kGroup]) {
  constexpr int W = 16 / sizeof(T);
  if (al) {
#pragma unroll
    for (int q = 0; q < kGroup / W; ++q) {
      const Pack<T> pk = reinterpret_cast<const Pack<T>*>(p)[q];
#pragma unroll
      for (int k = 0; k < W; ++k) v[q * W + k] = pk[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGroup; ++k) v[k] = p[k];
  }
}

template <typename T> __device__ __forceinline__ void store_group(T* __restrict__ p, bool al, const T (&v)[kGroup]) {
  constexpr int W = 16 / sizeof(T);
  if (al) {
#pragma unroll
    for (int q = 0; q < kGroup / W; ++q) {
      Pack<T> pk;
#pragma unroll
      for (int k = 0; k < W; ++k) pk[k] = v[q * W + k];
      reinterpret_cast<Pack<T>*>(p)[q] = pk;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGroup; ++k) p[k] = v[k];
  }
}

template <typename Out, int N> struct Outs {
  Out* p[N];
};

// bits of `al`: 1 first input, 2 second input, 4 << j output j (aligned to 16 bytes at element `head`)
template <typename Op>
__global__ __launch_bounds__(kThreads) void k_wave_elem(Op op, const typename Op::In* __restrict__ a, const typename Op::In* __restrict__ b,
                                                        Outs<typename Op::Out, Op::kOut> o, uint64_t n, uint64_t head, uint32_t al) {
  using In = typename Op::In;
  using Out = typename Op::Out;
  const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, nth = (uint64_t)gridDim.x * kThreads;
  const uint64_t groups = (n - head) / kGroup, tail = head + groups * kGroup;
  // head [0, head) and tail [tail, n): fewer than kGroup elements each
  if (tid < 2 * kGroup) {
    const uint64_t e = tid < kGroup ? tid : tail + (tid - kGroup);
    if (tid < kGroup ? e < head : e < n) {
      Out r[Op::kOut];
      op(a[e], Op::kTwo ? b[e] : In(0), r);
#pragma unroll
      for (int j = 0; j < Op::kOut; ++j) o.p[j][e] = r[j];
    }
  }
  for (uint64_t g = tid; g < groups; g += nth) {
    const uint64_t e = head + g * kGroup;
    In ta[kGroup], tb[kGroup] = {};
    load_group(a + e, al & 1u, ta);
    if constexpr (Op::kTwo) load_group(b + e, al & 2u, tb);
    Out res[Op::kOut][kGroup];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      Out r[Op::kOut];
      op(ta[k], tb[k], r);
#pragma unroll
      for (int j = 0; j < Op::kOut; ++j) res[j][k] = r[j];
    }
#pragma unroll
    for (int j = 0; j < Op::kOut; ++j) store_group(o.p[j] + e, al & (4u << j), res[j]);
  }
}

// ---- the functions -------------------------------------------------------------------------------------------------------------
// waveforms.ex:29-54.  rise = tmod / (pi() width) - 1, fall = (pi() (width + 1) - tmod) / (pi() (1 - width)); Nx.remainder is fmod
template <typename T> struct SawOp {
  using In = T;
  using Out = T;
  static constexpr int kOut = 1;
  static constexpr bool kTwo = false;
  WaveSaw p;
  __device__ __forceinline__ void operator()(T t, T, T (&o)[1]) const {
    using R = Rnd<T>;
    const double tmod = R::r(fmod((double)t, p.two_pi));
    const double rise = R::r(R::r(tmod / p.d_rise) - 1.0);
    const double fall = R::r(R::r(p.c_fall - tmod) / p.d_fall);
    o[0] = (T)(p.mode == 1 ? rise : p.mode == 0 ? fall : (tmod < p.thr ? rise : fall));
  }
};

// waveforms.ex:101-104.  tmod < duty * 2 * pi() ? 1 : -1; a tensor duty is the second stream
template <typename T, bool TENSOR> struct SquareOp {
  using In = T;
  using Out = int32_t;
  static constexpr int kOut = 1;
  static constexpr bool kTwo = TENSOR;
  WaveSquare p;
  __device__ __forceinline__ void operator()(T t, T d, int32_t (&o)[1]) const {
    using R = Rnd<T>;
    const double tmod = R::r(fmod((double)t, p.two_pi));
    const double thr = TENSOR ? R::r(R::r((double)d * 2.0) * p.pi) : p.thr;
    o[0] = tmod < thr ? 1 : -1;
  }
};

// waveforms.ex:192-197.  envelope = exp((-a) (t t)), yarg = (2 pi() fc) t
template <typename T> struct GaussOp {
  using In = T;
  using Out = T;
  static constexpr int kOut = 3;
  static constexpr bool kTwo = false;
  WaveGauss p;
  __device__ __forceinline__ void operator()(T tt, T, T (&o)[3]) const {
    using R = Rnd<T>;
    const double t = (double)tt;
    const double env = R::r(exp(R::r(p.neg_a * R::r(t * t))));
    const double yarg = R::r(p.w * t);
    o[0] = (T)env;
    o[1] = (T)R::r(env * R::r(cos(yarg)));
    o[2] = (T)R::r(env * R::r(sin(yarg)));
  }
};

// waveforms.ex:252-288.  The phase per kind (WaveChirp names the scalars); the factor 2 pi() multiplies last
template <typename T, int KIND> struct ChirpOp {
  using In = T;
  using Out = T;
  static constexpr int kOut = 1;
  static constexpr bool kTwo = false;
  WaveChirp p;
  __device__ __forceinline__ void operator()(T tt, T, T (&o)[1]) const {
    using R = Rnd<T>;
    const double t = (double)tt;
    double phase;
    if constexpr (KIND == kChirpLinear) {   // 2pi (f0 t + (0.5 beta) t^2): a = f0, b = 0.5 beta
      phase = R::r(p.two_pi * R::r(R::r(p.a * t) + R::r(p.b * R::r(pow(t, 2.0)))));
    } else if constexpr (KIND == kChirpQuadratic) {   // 2pi (f0 t + beta t^3 / 3): a = f0, b = beta
      phase = R::r(p.two_pi * R::r(R::r(p.a * t) + R::r(R::r(p.b * R::r(pow(t, 3.0))) / 3.0)));
    } else if constexpr (KIND == kChirpQuadraticT1) {   // 2pi (f1 t + beta ((t1 - t)^3 - t1^3) / 3): a = f1, b = beta, c = t1, d = t1^3
      phase = R::r(p.two_pi * R::r(R::r(p.a * t) + R::r(R::r(p.b * R::r(R::r(pow(R::r(p.c - t), 3.0)) - p.d)) / 3.0)));
    } else if constexpr (KIND == kChirpLogarithmic) {   // 2pi ((beta f0) ((f1 / f0)^(t / t1) - 1)): a = beta f0, b = f1 / f0, c = t1
      phase = R::r(p.two_pi * R::r(p.a * R::r(R::r(pow(p.b, R::r(t / p.c))) - 1.0)));
    } else if constexpr (KIND == kChirpHyperbolic) {   // 2pi ((-sp f0) log|1 - t / sp|): a = -sp f0, b = sp
      phase = R::r(p.two_pi * R::r(p.a * R::r(log(R::r(fabs(R::r(1.0 - R::r(t / p.b))))))));
    } else if constexpr (KIND == kChirpConstant) {   // f0 == f1 of :logarithmic / :hyperbolic: (2pi f0) t, a = 2pi f0
      phase = R::r(p.a * t);
    } else {   // :logarithmic with f0 f1 <= 0: Nx.broadcast(:nan, shape)
      phase = __builtin_nan("");
    }
    o[0] = (T)R::r(cos(R::r(phase + p.phi)));
  }
};

// waveforms.ex:343-361.  t^(n - k) as one pow each, the dot product summed in f64 and rounded once
template <typename T> struct SweepOp {
  using In = T;
  using Out = T;
  static constexpr int kOut = 1;
  static constexpr bool kTwo = false;
  WaveSweep p;
  __device__ __forceinline__ void operator()(T tt, T, T (&o)[1]) const {
    using R = Rnd<T>;
    const double t = (double)tt;
    double acc = 0.0;
    for (int k = 0; k < p.n; ++k) acc = acc + p.coef[k] * R::r(pow(t, (double)(p.n - k)));
    const double phase = R::r(acc);
    o[0] = (T)R::r(cos(R::r(R::r(p.two_pi * phase) + p.phi)));
  }
};

// waveforms.ex:413-422.  zeros, then one at flat element `at`, in words of the element's size
template <typename U>
__global__ __launch_bounds__(kThreads) void k_wave_impulse(U* __restrict__ out, uint64_t n, uint64_t head, uint64_t at, U one) {
  constexpr int W = 16 / sizeof(U);
  const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, nth = (uint64_t)gridDim.x * kThreads;
  const uint64_t groups = (n - head) / W, tail = head + groups * W;
  if (tid < 2 * W) {
    const uint64_t e = tid < W ? tid : tail + (tid - W);
    if (tid < W ? e < head : e < n) out[e] = e == at ? one : U(0);
  }
  for (uint64_t g = tid; g < groups; g += nth) {
    const uint64_t e = head + g * W;
    Pack<U> pk;
#pragma unroll
    for (int k = 0; k < W; ++k) pk[k] = e + k == at ? one : U(0);
    *reinterpret_cast<Pack<U>*>(out + e) = pk;
  }
}

bool misaligned(const void* p, size_t es) { return p && (reinterpret_cast<uintptr_t>(p) % es) != 0; }

// elements before the first 16-byte boundary of p
uint64_t head_of(const void* p, size_t es, uint64_t n) {
  const uint64_t h = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / es;
  return h < n ? h : n;
}

bool aligned_at(const void* p, size_t es, uint64_t head) { return ((reinterpret_cast<uintptr_t>(p) + head * es) & 15) == 0; }

unsigned grid_for(const Ctx* c, uint64_t groups) {
  const uint64_t want = (groups + kThreads - 1) / kThreads, cap = (uint64_t)(c->num_cus > 0 ? c->num_cus : 1) * kBlocksPerCu;
  return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

template <typename Op>
int launch_elem(Ctx* c, const Op& op, const void* a, const void* b, void* const* outs, int64_t n) {
  using In = typename Op::In;
  using Out = typename Op::Out;
  if (n <= 0) return NXSIG_OK;
  Outs<Out, Op::kOut> o;
  bool bad = misaligned(a, sizeof(In)) || misaligned(b, sizeof(In));
  for (int j = 0; j < Op::kOut; ++j) {
    o.p[j] = static_cast<Out*>(outs[j]);
    bad = bad || misaligned(outs[j], sizeof(Out));
  }
  if (bad) return set_error(NXSIG_ERR_INVALID_ARG, "waveforms: a pointer is not aligned to its element type");
  const uint64_t head = head_of(outs[0], sizeof(Out), (uint64_t)n);
  uint32_t al = aligned_at(a, sizeof(In), head) ? 1u : 0u;
  if (Op::kTwo && aligned_at(b, sizeof(In), head)) al |= 2u;
  for (int j = 0; j < Op::kOut; ++j)
    if (aligned_at(outs[j], sizeof(Out), head)) al |= 4u << j;
  hipLaunchKernelGGL(k_wave_elem<Op>, dim3(grid_for(c, ((uint64_t)n - head) / kGroup)), dim3(kThreads), 0, c->stream, op, static_cast<const In*>(a),
                     static_cast<const In*>(b), o, (uint64_t)n, head, al);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

template <typename T, int KIND> int launch_chirp_kind(Ctx* c, const WaveChirp& p, const void* t, void* out, int64_t n) {
  ChirpOp<T, KIND> op{p};
  return launch_elem(c, op, t, nullptr, &out, n);
}

template <typename T> int launch_chirp_t(Ctx* c, const WaveChirp& p, const void* t, void* out, int64_t n) {
  switch (p.kind) {
    case kChirpLinear: return launch_chirp_kind<T, kChirpLinear>(c, p, t, out, n);
    case kChirpQuadratic: return launch_chirp_kind<T, kChirpQuadratic>(c, p, t, out, n);
    case kChirpQuadraticT1: return launch_chirp_kind<T, kChirpQuadraticT1>(c, p, t, out, n);
    case kChirpLogarithmic: return launch_chirp_kind<T, kChirpLogarithmic>(c, p, t, out, n);
    case kChirpHyperbolic: return launch_chirp_kind<T, kChirpHyperbolic>(c, p, t, out, n);
    case kChirpConstant: return launch_chirp_kind<T, kChirpConstant>(c, p, t, out, n);
    case kChirpNan: return launch_chirp_kind<T, kChirpNan>(c, p, t, out, n);
  }
  return set_error(NXSIG_ERR_INVALID_ARG, "chirp: unknown kind");
}

}  // namespace

int launch_sawtooth(Ctx* c, const void* t, bool f64, int64_t n, const WaveSaw& p, void* out) {
  dispatch_note("waveform.sawtooth");
  if (f64) return launch_elem(c, SawOp<double>{p}, t, nullptr, &out, n);
  return launch_elem(c, SawOp<float>{p}, t, nullptr, &out, n);
}

int launch_square(Ctx* c, const void* t, bool f64, int64_t n, const WaveSquare& p, const void* duty, int32_t* out) {
  dispatch_note("waveform.square");
  void* o = out;
  if (duty) {
    if (f64) return launch_elem(c, SquareOp<double, true>{p}, t, duty, &o, n);
    return launch_elem(c, SquareOp<float, true>{p}, t, duty, &o, n);
  }
  if (f64) return launch_elem(c, SquareOp<double, false>{p}, t, nullptr, &o, n);
  return launch_elem(c, SquareOp<float, false>{p}, t, nullptr, &o, n);
}

int launch_gaussian_pulse(Ctx* c, const void* t, bool f64, int64_t n, const WaveGauss& p, void* envelope, void* in_phase, void* quadrature) {
  dispatch_note("waveform.gaussian_pulse");
  void* outs[3] = {envelope, in_phase, quadrature};
  if (f64) return launch_elem(c, GaussOp<double>{p}, t, nullptr, outs, n);
  return launch_elem(c, GaussOp<float>{p}, t, nullptr, outs, n);
}

int launch_chirp(Ctx* c, const void* t, bool f64, int64_t n, const WaveChirp& p, const char* family, void* out) {
  dispatch_note(family);
  return f64 ? launch_chirp_t<double>(c, p, t, out, n) : launch_chirp_t<float>(c, p, t, out, n);
}

int launch_polynomial_sweep(Ctx* c, const void* t, bool f64, int64_t n, const WaveSweep& p, void* out) {
  dispatch_note("waveform.polynomial_sweep");
  if (f64) return launch_elem(c, SweepOp<double>{p}, t, nullptr, &out, n);
  return launch_elem(c, SweepOp<float>{p}, t, nullptr, &out, n);
}

int launch_unit_impulse(Ctx* c, void* out, int dtype, int64_t n, int64_t at) {
  dispatch_note("waveform.unit_impulse");
  if (n <= 0) return NXSIG_OK;
  const bool wide = dtype == NXSIG_DT_F64 || dtype == NXSIG_DT_S64 || dtype == NXSIG_DT_U64;
  const size_t es = wide ? 8 : 4;
  if (misaligned(out, es)) return set_error(NXSIG_ERR_INVALID_ARG, "unit_impulse: out is not aligned to its element type");
  const uint64_t head = head_of(out, es, (uint64_t)n);
  const unsigned grid = grid_for(c, ((uint64_t)n - head) / (16 / es));
  if (wide) {
    const uint64_t one = dtype == NXSIG_DT_F64 ? 0x3ff0000000000000ull : 1ull;
    hipLaunchKernelGGL(k_wave_impulse<uint64_t>, dim3(grid), dim3(kThreads), 0, c->stream, static_cast<uint64_t*>(out), (uint64_t)n, head, (uint64_t)at, one);
  } else {
    const uint32_t one = dtype == NXSIG_DT_F32 ? 0x3f800000u : 1u;
    hipLaunchKernelGGL(k_wave_impulse<uint32_t>, dim3(grid), dim3(kThreads), 0, c->stream, static_cast<uint32_t*>(out), (uint64_t)n, head, (uint64_t)at, one);
  }
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace nxsig
