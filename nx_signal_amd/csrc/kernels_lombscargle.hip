// Spectral.lombscargle: the generalised Lomb-Scargle periodogram of scipy.signal 1.15 over real f32 / f64 rows that share one time
// base.  include/nxsig.h states the definition, DESIGN.md section 3.19 the design; the argument checks, the blocking sizes and the tier
// choice are csrc/lombscargle_plan.hpp.  Every sum, tau, the divisions and the normalisation are double; a sample is widened on load
// and a result rounded to its type once.  The phase is fl(w * t) in double, fed to the double sincos: no f32 phase, no fast intrinsic.
//   lombscargle.tile     a workgroup (one wave) owns kLsFB frequencies, one per lane, and kLsRB rows.  Prologue: per row the plain
//                        mean (precenter), Y = sum w (y - mean), YY = sum w (y - mean)^2 and the non-finite flag: lane l sums the
//                        samples l, l + 64, ... in ascending order, then a butterfly over the wave — a shape of n alone.  Then the
//                        time axis in order, kLsTT samples per tile: (t, w) pairs and w (y - mean) of the kLsRB rows go through LDS
//                        (the mean is subtracted on load), every lane reads them at the same address (a broadcast), and one
//                        sincos(w t) per sample feeds the four row-independent sums C, S, CC, CS and the rows' YC, YS, all in
//                        registers.  tau comes from the unshifted sums, which are then ROTATED by tau instead of summed again at
//                        the shifted phase (half the sincos of scipy's two passes).
//   lombscargle.generic  one lane per (row, frequency): scipy's two passes as written, from global memory.  Everything under
//                        NXSIG_LOMBSCARGLE_TILE=0.
// Non-finite rule: a row of y that holds an Inf / NaN is NaN at every frequency (a zero weight does not shield it); the sums of the
// other rows never see its samples.  No atomics, no scratch: the bits of out[r][k] depend on n, the options and the tier alone.
#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int FB = kLsFB, RB = kLsRB, TT = kLsTT;

struct LsArgs {
  const void* y;          // device f32 / f64 [batch][n], rows y_stride elements apart
  int64_t y_stride, n, F;
  int32_t batch, precenter, normalize, fm;
  const double *x, *freqs, *w;   // device tables: times [n], angular frequencies [F], weights [n] that sum to 1
  void* out;              // [batch][F] of f32 / f64, or of c64 / c128 under "amplitude"
};

__device__ __forceinline__ bool ls_nonfinite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL; }

template <typename T>
__device__ __forceinline__ void ls_put(void* out, int64_t idx, bool amplitude, double re, double im);
template <>
__device__ __forceinline__ void ls_put<float>(void* out, int64_t idx, bool amplitude, double re, double im) {
  if (amplitude) static_cast<float2*>(out)[idx] = make_float2((float)re, (float)im);
  else static_cast<float*>(out)[idx] = (float)re;
}
template <>
__device__ __forceinline__ void ls_put<double>(void* out, int64_t idx, bool amplitude, double re, double im) {
  if (amplitude) static_cast<double2*>(out)[idx] = make_double2(re, im);
  else static_cast<double*>(out)[idx] = re;
}

// From the shifted sums to the result, scipy's last lines: CC and SS clamped at epsneg, a = YC / CC, b = YS / SS,
// 2 (a YC + b YS) scaled by n / 4 ("power") or 0.5 / YY ("normalize"), or (a + i b) e^{i tau} ("amplitude").  (ct, st) = (cos, sin) tau
template <typename T>
__device__ __forceinline__ void ls_finish(void* out, int64_t idx, int32_t normalize, bool bad, double CC, double SS, double YC, double YS,
                                          double ct, double st, double n, double YY) {
  if (bad) {
    const double q = __longlong_as_double(0x7ff8000000000000LL);
    ls_put<T>(out, idx, normalize == kLsAmplitude, q, q);
    return;
  }
  if (CC < kLsEpsNeg) CC = kLsEpsNeg;
  if (SS < kLsEpsNeg) SS = kLsEpsNeg;
  const double a = YC / CC, b = YS / SS;
  double p = 2.0 * (a * YC + b * YS);
  if (normalize == kLsPower) {
    p *= n / 4.0;
  } else if (normalize == kLsNormalize) {
    p *= 0.5 / YY;
  } else {
    ls_put<T>(out, idx, true, a * ct - b * st, a * st + b * ct);
    return;
  }
  ls_put<T>(out, idx, false, p, 0.0);
}

// ---- lombscargle.tile
template <typename T>
__global__ __launch_bounds__(FB) void k_ls_tile(LsArgs a, int32_t fblocks) {
  __shared__ __attribute__((aligned(16))) double2 s_tw[TT];        // (t, w) of the tile's samples
  __shared__ __attribute__((aligned(16))) double s_wy[TT * RB];    // w (y - mean) of sample j, row r at [j * RB + r]
  __shared__ double s_mean[RB], s_Y[RB], s_YY[RB];
  __shared__ int s_bad[RB];
  const int lane = threadIdx.x;
  const int64_t fb = blockIdx.x % fblocks, row0 = (int64_t)(blockIdx.x / fblocks) * RB;
  const int64_t left = a.batch - row0;
  const int here = left < RB ? (int)left : RB;   // rows of this block that exist (>= 1)
  const T* ybase = static_cast<const T*>(a.y) + (size_t)row0 * a.y_stride;
  const int64_t n = a.n;

  // ---- prologue: what a row needs that does not depend on the frequency.  Lane l takes the samples l, l + FB, ... in ascending
  // order, the wave adds the 64 partial sums in a butterfly: the same shape for every row, batch and launch
  for (int r = 0; r < here; ++r) {
    const T* row = ybase + (size_t)r * a.y_stride;
    double sum = 0.0;
    int bad = 0;
    for (int64_t i = lane; i < n; i += FB) {
      const double v = (double)row[i];
      bad |= ls_nonfinite(v) ? 1 : 0;
      sum += v;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const double mean = a.precenter ? sum / (double)n : 0.0;
    double Y = 0.0, YY = 0.0;
    for (int64_t i = lane; i < n; i += FB) {
      const double d = (double)row[i] - mean, wy = a.w[i] * d;
      Y += wy;
      YY = fma(wy, d, YY);
    }
    for (int off = 32; off > 0; off >>= 1) { Y += __shfl_xor(Y, off); YY += __shfl_xor(YY, off); }
    bad = __any(bad);
    if (lane == 0) { s_mean[r] = mean; s_Y[r] = Y; s_YY[r] = YY; s_bad[r] = bad; }
  }

  const int64_t k = fb * FB + lane;
  const bool active = k < a.F;
  const double omega = active ? a.freqs[k] : 0.0;
  double C = 0.0, S = 0.0, CC = 0.0, CS = 0.0, YC[RB], YS[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) YC[r] = YS[r] = 0.0;

  // ---- the time axis, in order
  for (int64_t t0 = 0; t0 < n; t0 += TT) {
    const int cnt = n - t0 < TT ? (int)(n - t0) : TT;
    __syncthreads();   // the previous tile's readers are done (and, the first time, the prologue's writes are visible)
    for (int j = lane; j < cnt; j += FB) {
      const double wj = a.w[t0 + j];
      s_tw[j] = make_double2(a.x[t0 + j], wj);
#pragma unroll
      for (int r = 0; r < RB; ++r)
        s_wy[j * RB + r] = r < here ? wj * ((double)ybase[(size_t)r * a.y_stride + t0 + j] - s_mean[r]) : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const double2 tw = s_tw[j];
      const double ph = omega * tw.x;
      double s, c;
      sincos(ph, &s, &c);
      const double wc = tw.y * c;
      C += wc;
      S = fma(tw.y, s, S);
      CC = fma(wc, c, CC);
      CS = fma(wc, s, CS);
#pragma unroll
      for (int r = 0; r < RB; r += 2) {
        const double2 v = *reinterpret_cast<const double2*>(&s_wy[j * RB + r]);
        YC[r] = fma(v.x, c, YC[r]);
        YS[r] = fma(v.x, s, YS[r]);
        YC[r + 1] = fma(v.y, c, YC[r + 1]);
        YS[r + 1] = fma(v.y, s, YS[r + 1]);
      }
    }
  }
  if (!active) return;

  // ---- tau from the unshifted sums (the floating mean's corrections first), then the rotation by tau
  double SS = 1.0 - CC;
  if (a.fm) {
    CC -= C * C;
    SS -= S * S;
    CS -= C * S;
  }
  const double tau = 0.5 * atan2(2.0 * CS, CC - SS);
  double st, ct;
  sincos(tau, &st, &ct);
  const double c2 = ct * ct, s2 = st * st, sc2 = 2.0 * CS * (st * ct);
  const double CCt = CC * c2 + sc2 + SS * s2, SSt = SS * c2 - sc2 + CC * s2;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r >= here) continue;
    const double Y = s_Y[r];
    double yc = YC[r], ys = YS[r], yy = s_YY[r];
    if (a.fm) {
      yc -= Y * C;
      ys -= Y * S;
      yy -= Y * Y;
    }
    ls_finish<T>(a.out, (row0 + r) * a.F + k, a.normalize, s_bad[r] != 0, CCt, SSt, yc * ct + ys * st, ys * ct - yc * st, ct, st, (double)n, yy);
  }
}

// ---- lombscargle.generic: scipy's two passes, one lane per (row, frequency)
template <typename T>
__global__ __launch_bounds__(kLsGenericThreads) void k_ls_generic(LsArgs a) {
  const int64_t total = (int64_t)a.batch * a.F, n = a.n;
  for (int64_t idx = (int64_t)blockIdx.x * kLsGenericThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kLsGenericThreads) {
    const int64_t r = idx / a.F, k = idx - r * a.F;
    const T* row = static_cast<const T*>(a.y) + (size_t)r * a.y_stride;
    const double omega = a.freqs[k];
    bool bad = false;
    double mean = 0.0;
    if (a.precenter) {
      double sum = 0.0;
      for (int64_t i = 0; i < n; ++i) sum += (double)row[i];
      mean = sum / (double)n;
    }
    double Y = 0.0, YY = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double v = (double)row[i], d = v - mean, wy = a.w[i] * d;
      bad = bad || ls_nonfinite(v);
      Y += wy;
      YY += wy * d;
    }
    // first pass: tau
    double C = 0.0, S = 0.0, CC = 0.0, CS = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      double s, c;
      sincos(omega * a.x[i], &s, &c);
      const double w = a.w[i];
      CC += w * (c * c);
      CS += w * (c * s);
      C += w * c;
      S += w * s;
    }
    double SS = 1.0 - CC;
    if (a.fm) {
      CC -= C * C;
      SS -= S * S;
      CS -= C * S;
    }
    const double tau = 0.5 * atan2(2.0 * CS, CC - SS);
    // second pass: every sum again at the phase shifted by tau
    double YC = 0.0, YS = 0.0;
    CC = C = S = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      double s, c;
      sincos(omega * a.x[i] - tau, &s, &c);
      const double w = a.w[i], wy = w * ((double)row[i] - mean);
      YC += wy * c;
      YS += wy * s;
      CC += w * (c * c);
      C += w * c;
      S += w * s;
    }
    SS = 1.0 - CC;
    if (a.fm) {
      YC -= Y * C;
      YS -= Y * S;
      CC -= C * C;
      SS -= S * S;
      YY -= Y * Y;
    }
    double st, ct;
    sincos(tau, &st, &ct);
    ls_finish<T>(a.out, idx, a.normalize, bad, CC, SS, YC, YS, ct, st, (double)n, YY);
  }
}

}  // namespace

int launch_lombscargle(Ctx* c, const LsLaunch& l) {
  if (l.batch == 0) return NXSIG_OK;
  // the three host arrays go through the content-addressed table cache: a repeated call uploads nothing
  const std::vector<double> w = ls_weights(l.weights_host, l.n);
  const void *dx = nullptr, *df = nullptr, *dw = nullptr;
  int rc;
  if ((rc = ctx_table(c, 0x4C53434100000001ull, l.x_host, (size_t)l.n * sizeof(double), &dx))) return rc;
  if ((rc = ctx_table(c, 0x4C53434100000002ull, l.freqs_host, (size_t)l.num_freqs * sizeof(double), &df))) return rc;
  if ((rc = ctx_table(c, 0x4C53434100000003ull, w.data(), (size_t)l.n * sizeof(double), &dw))) return rc;
  LsArgs a;
  a.y = l.y; a.y_stride = l.y_stride; a.n = l.n; a.F = l.num_freqs;
  a.batch = l.batch; a.precenter = l.precenter; a.normalize = l.normalize; a.fm = l.floating_mean;
  a.x = static_cast<const double*>(dx); a.freqs = static_cast<const double*>(df); a.w = static_cast<const double*>(dw);
  a.out = l.out;
  if (ls_tier(l.n, l.num_freqs, l.normalize, l.floating_mean, tune(c, kT_LOMBSCARGLE_TILE, 1) != 0) == kLsTile) {
    dispatch_note("lombscargle.tile");
    const int64_t fblocks = (l.num_freqs + FB - 1) / FB, rblocks = ((int64_t)l.batch + RB - 1) / RB;   // fblocks * rblocks < 2^31: ls_check_shape
    if (l.f64) hipLaunchKernelGGL(k_ls_tile<double>, dim3((unsigned)(fblocks * rblocks)), dim3(FB), 0, c->stream, a, (int32_t)fblocks);
    else hipLaunchKernelGGL(k_ls_tile<float>, dim3((unsigned)(fblocks * rblocks)), dim3(FB), 0, c->stream, a, (int32_t)fblocks);
  } else {
    dispatch_note("lombscargle.generic");
    const int64_t total = (int64_t)l.batch * l.num_freqs, need = (total + kLsGenericThreads - 1) / kLsGenericThreads;
    const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
    const unsigned blocks = (unsigned)(need < cap ? need : cap);
    if (l.f64) hipLaunchKernelGGL(k_ls_generic<double>, dim3(blocks), dim3(kLsGenericThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(k_ls_generic<float>, dim3(blocks), dim3(kLsGenericThreads), 0, c->stream, a);
  }
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace nxsig
