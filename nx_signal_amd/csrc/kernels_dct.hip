// Transforms.dct / idct: the cosine transforms of type 2 and 3 over real f32 rows (scipy.fft.dct / idct).  include/nxsig.h states the
// definition, DESIGN.md section 3.17 the design; the argument checks, the norm factors, the tables, the tier choice and the direct
// kernel's geometry are csrc/dct_plan.hpp.
//   dct.direct  n <= 256, any keep (the MFCC path): every output is one sum over ascending j of fmaf(x[j], Tt[j][k], .) against a
//               cosine table built in double on the host, the norm folded in.  A workgroup copies a tile of rows into LDS (16-byte
//               loads where the rows are dense, full and 16-byte aligned; element by element otherwise: strided rows, padding,
//               truncation, n = 13), thread t owns coefficient k = t % keep of kDctRR rows and reads the table coalesced (k fastest)
//               and the samples as 16-byte LDS broadcasts; the stores of a workgroup are one contiguous run.  Rows live on
//               gridDim.x, in slabs of 2^30 tiles.
//   dct.fft     every other n and every n under NXSIG_DISABLE_DCT_DIRECT: Makhoul's n-point form.  Type 2: gather v[j] = x[2 j],
//               v[n - 1 - j] = x[2 j + 1] (pads, truncates, takes strided rows, centres) into kScratchIstftProduct behind the row
//               means, one real-input launch_fft_big (clean = false) into kScratchFusedSpectrum, y[k] = 2 Re(e^{-i pi k / 2n} V[k])
//               with the norm, keep outputs stored.  Type 3 in reverse: W[k] = e^{i pi k / 2n} (x[k] - i x[n - k]) into
//               kScratchIstftProduct, one inverse launch_fft_big into kScratchFusedSpectrum, y[m] = Re u[dct_unperm(m)].  The
//               twiddles are a double-built table.
// Centring (type 2, both families): a row is transformed as row - c, c the mean of its n points as f32 sums give it, and
// c * 2 n a_0 goes back into y[0]: algebraically nothing changes (every column k >= 1 of the cosine matrix sums to zero), numerically
// the rounding — of the table in dct.direct, of the butterflies in dct.fft — then scales with the row's variation, not its offset.
// Measured on 1000 + N(0, 1) rows of 80 points, error of the coefficients k >= 1 over their maximum: 5e-4 for plain f32 sums against
// an f32 table (host emulation), 2.5e-4 for the plain single-precision transform of dct.fft (MI355X); centred, both stay below 1e-6.
// Non-finite rule: a row that holds an Inf / NaN among the samples read has no finite output.  dct.direct: every output sums every
// sample (Inf * 0 = NaN).  dct.fft: bin 0 of the forward transform (type 2) and point 0 of the inverse one (type 3) are plain sums
// over the whole row; when they are not finite the row leaves as NaN.
// No atomics: a row's bits depend neither on the batch nor on the launch geometry.
#include <cstring>

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kThreads = kDctThreads, kRR = kDctRR;

__device__ __forceinline__ bool dct_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

struct DctDirectArgs {
  const float* x;
  int64_t x_stride, rows, tile0;   // tile0: the first tile of this launch (slabs)
  int32_t n, n_used, keep, pitch, groups, tile_rows, centre;
  float dc_gain;
  const float* table;              // Tt[n][keep]
  float* out;                      // [rows][keep]
};

__global__ __launch_bounds__(kThreads) void k_dct_direct(DctDirectArgs a) {
  __shared__ __attribute__((aligned(16))) float s[kDctLdsFloats];
  const int tid = threadIdx.x, n = a.n, P = a.pitch, keep = a.keep;
  const int64_t row0 = ((int64_t)blockIdx.x + a.tile0) * a.tile_rows;
  const int64_t left = a.rows - row0;
  const int here = left < a.tile_rows ? (int)left : a.tile_rows;   // rows of this tile that exist (>= 1)
  const float* base = a.x + (size_t)row0 * a.x_stride;
  // ---- the tile into LDS, row r at r * P; rows that do not exist and points past n_used are zero
  const bool wide = a.x_stride == n && a.n_used == n && (n & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;   // uniform
  if (wide) {
    const int Q = n >> 2, total = a.tile_rows * Q;
    const float4* b4 = reinterpret_cast<const float4*>(base);
#pragma unroll 4
    for (int i = tid; i < total; i += kThreads) {
      const int r = i / Q, c4 = i - r * Q;
      const float4 v = r < here ? b4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&s[r * P + 4 * c4]) = v;
    }
  } else {
    const int total = a.tile_rows * n;
    for (int i = tid; i < total; i += kThreads) {
      const int r = i / n, j = i - r * n;
      s[r * P + j] = (r < here && j < a.n_used) ? base[(size_t)r * a.x_stride + j] : 0.0f;
    }
  }
  __syncthreads();
  // ---- type 2: centre every row on the mean of its n points.  Four adjacent lanes per row: lane q sums the q-th quarter of the row
  // (dct_quarter; ascending j), the row's sum is (p0 + p1) + (p2 + p3) on all four, and each subtracts c from its own quarter.  The
  // order depends on n alone.  The mean stays in s[r * P + n]
  if (a.centre) {
    const bool quads = (n & 3) == 0;               // whole 16-byte units
    const int units = quads ? n >> 2 : n;
    for (int slot = tid; slot < 4 * here; slot += kThreads) {
      const int r = slot >> 2, q = slot & 3, lo = dct_quarter(q, units), hi = dct_quarter(q + 1, units);
      float* row = s + r * P;
      float sum = 0.0f;
      if (quads) {
        for (int u = lo; u < hi; ++u) { const float4 v = *reinterpret_cast<const float4*>(row + 4 * u); sum += v.x; sum += v.y; sum += v.z; sum += v.w; }
      } else {
        for (int u = lo; u < hi; ++u) sum += row[u];
      }
      sum += __shfl_xor(sum, 1);   // the partners are the lanes of the same row, in this trip of the slot loop together
      sum += __shfl_xor(sum, 2);
      const float c = sum / (float)n;
      if (quads) {
        for (int u = lo; u < hi; ++u) {
          float4 v = *reinterpret_cast<const float4*>(row + 4 * u);
          v.x -= c; v.y -= c; v.z -= c; v.w -= c;
          *reinterpret_cast<float4*>(row + 4 * u) = v;
        }
      } else {
        for (int u = lo; u < hi; ++u) row[u] -= c;
      }
      if (q == 0) row[n] = c;
    }
    __syncthreads();
  }
  // ---- the sums: thread t owns coefficient k of the rows g + groups * rr
  if (tid >= a.groups * keep) return;
  const int g = tid / keep, k = tid - g * keep;
  const float* tk = a.table + k;
  float acc[kRR];
#pragma unroll
  for (int rr = 0; rr < kRR; ++rr) acc[rr] = 0.0f;
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    const float t0 = tk[(size_t)j * keep], t1 = tk[(size_t)(j + 1) * keep], t2 = tk[(size_t)(j + 2) * keep], t3 = tk[(size_t)(j + 3) * keep];
#pragma unroll
    for (int rr = 0; rr < kRR; ++rr) {
      const float4 v = *reinterpret_cast<const float4*>(&s[(g + a.groups * rr) * P + j]);
      acc[rr] = fmaf(v.x, t0, acc[rr]);
      acc[rr] = fmaf(v.y, t1, acc[rr]);
      acc[rr] = fmaf(v.z, t2, acc[rr]);
      acc[rr] = fmaf(v.w, t3, acc[rr]);
    }
  }
  for (; j < n; ++j) {
    const float t0 = tk[(size_t)j * keep];
#pragma unroll
    for (int rr = 0; rr < kRR; ++rr) acc[rr] = fmaf(s[(g + a.groups * rr) * P + j], t0, acc[rr]);
  }
#pragma unroll
  for (int rr = 0; rr < kRR; ++rr) {
    const int r = g + a.groups * rr;
    if (r >= here) continue;
    float y = acc[rr];
    if (a.centre && k == 0) y = fmaf(s[r * P + n], a.dc_gain, y);
    a.out[(size_t)(row0 + r) * keep + k] = y;
  }
}

// ---- dct.fft, type 2
// v[r][i] = x[r][dct_perm(i)] - c, zero for x where the row has no sample; c = means[r] is the mean of the row's n points as f32 sums
// give it (one workgroup per row: a fixed order, whatever the batch).  See "Centring" at the top: a plain single-precision transform
// of a 1000 + N(0, 1) row leaves 2.5e-4 of max_{k>=1} |y[k]| in the coefficients k >= 1
__global__ __launch_bounds__(kThreads) void k_dct2_gather(const float* __restrict__ x, int64_t x_stride, int64_t n_used, int64_t n, int64_t rows,
                                                         float* __restrict__ v, float* __restrict__ means) {
  __shared__ float s_part[kThreads / 64];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const float* row = x + (size_t)r * x_stride;
    float sum = 0.0f;
    for (int64_t i = threadIdx.x; i < n_used; i += kThreads) sum += row[i];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();   // the previous row's readers of s_part are done
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    sum = 0.0f;
    for (int w = 0; w < kThreads / 64; ++w) sum += s_part[w];
    const float c = sum / (float)n;
    if (threadIdx.x == 0) means[r] = c;
    float* vrow = v + (size_t)r * n;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
      const int64_t src = dct_perm(i, n);
      vrow[i] = (src < n_used ? row[src] : 0.0f) - c;
    }
  }
}

// y[r][k] = tw[k].x Re V[r][k] + tw[k].y Im V[r][k], k < keep, and the mean's share c * dc_gain back in y[r][0]; a row whose V[0] (the
// sum of its centred samples) is not finite leaves as NaN
__global__ __launch_bounds__(kThreads) void k_dct2_post(const float2* __restrict__ V, const float2* __restrict__ tw, const float* __restrict__ means,
                                                       float dc_gain, int64_t rows, int64_t n, int64_t keep, float* __restrict__ out) {
  const int64_t total = rows * keep;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / keep, k = i - r * keep;
    const float2 v0 = V[(size_t)r * n], v = V[(size_t)r * n + k], t = tw[k];
    const bool bad = dct_nonfinite(v0.x) || dct_nonfinite(v0.y);
    float y = fmaf(t.x, v.x, t.y * v.y);
    if (k == 0) y = fmaf(means[r], dc_gain, y);
    out[i] = bad ? __uint_as_float(0x7fc00000u) : y;
  }
}

// ---- dct.fft, type 3
// W[r][0] = tw[0].x x[0], W[r][k] = tw[k] (x[k] - i x[n - k]); zero where the row has no sample
__global__ __launch_bounds__(kThreads) void k_dct3_pre(const float* __restrict__ x, int64_t x_stride, int64_t n_used, int64_t n, int64_t rows,
                                                      const float2* __restrict__ tw, float2* __restrict__ W) {
  const int64_t total = rows * n;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / n, k = i - r * n;
    const float* row = x + (size_t)r * x_stride;
    const float2 t = tw[k];
    if (k == 0) { W[i] = make_float2(t.x * row[0], 0.0f); continue; }
    const float p = k < n_used ? row[k] : 0.0f, q = n - k < n_used ? row[n - k] : 0.0f;
    W[i] = make_float2(fmaf(t.x, p, t.y * q), fmaf(t.y, p, -(t.x * q)));
  }
}

// y[r][m] = Re u[r][dct_unperm(m)], m < keep; a row whose u[0] (the sum of its spectrum) is not finite leaves as NaN
__global__ __launch_bounds__(kThreads) void k_dct3_sink(const float2* __restrict__ u, int64_t rows, int64_t n, int64_t keep, float* __restrict__ out) {
  const int64_t total = rows * keep;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / keep, m = i - r * keep;
    const float2 u0 = u[(size_t)r * n];
    const bool bad = dct_nonfinite(u0.x) || dct_nonfinite(u0.y);
    out[i] = bad ? __uint_as_float(0x7fc00000u) : u[(size_t)r * n + dct_unperm(m, n)].x;
  }
}

unsigned stream_blocks(const Ctx* c, int64_t n) {
  const int64_t need = (n + kThreads - 1) / kThreads, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  return (unsigned)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// the table of a parameter set is formed once per context: the memo keeps the device pointer beside the parameters, so a repeated call
// makes no table request.  Dropped together with the table cache (DeviceGuard, api.cpp)
int dct_table(Ctx* c, int tier, const DctLaunch& a, const float** out) {
  const int64_t keep = tier == kDctDirect ? a.keep : 0;   // the fft tier's twiddles do not depend on keep
  std::vector<uint64_t> want = {0, (uint64_t)tier, (uint64_t)a.n, (uint64_t)keep, (uint64_t)a.type, (uint64_t)a.norm};
  const uint64_t key = fnv1a(0xDC7D1EC7ull, want.data() + 1, (want.size() - 1) * sizeof(uint64_t));
  auto hit = c->memo.find(key);
  if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 1, want.end(), hit->second.begin() + 1)) {
    *out = reinterpret_cast<const float*>((uintptr_t)hit->second[0]);
    return NXSIG_OK;
  }
  const std::vector<float> t = tier == kDctDirect ? dct_direct_table(a.n, a.keep, a.type, a.norm) : dct_fft_table(a.n, a.type, a.norm);
  const void* d = nullptr;
  int rc = ctx_table(c, 0xDC700000ull ^ key, t.data(), t.size() * sizeof(float), &d);
  if (rc) return rc;
  want[0] = (uint64_t)(uintptr_t)d;
  c->memo[key] = want;
  *out = static_cast<const float*>(d);
  return NXSIG_OK;
}

int run_direct(Ctx* c, const DctLaunch& a) {
  const float* table = nullptr;
  int rc = dct_table(c, kDctDirect, a, &table);
  if (rc) return rc;
  const DctGeom g = dct_geom(a.n, a.keep, a.batch);
  DctDirectArgs d;
  d.x = a.x; d.x_stride = a.x_stride; d.rows = a.batch;
  d.n = (int32_t)a.n; d.n_used = (int32_t)dct_used(a.length, a.n); d.keep = (int32_t)a.keep;
  d.pitch = g.pitch; d.groups = g.groups; d.tile_rows = g.tile_rows;
  d.centre = a.type == 2 ? 1 : 0;
  d.dc_gain = dct_dc_gain(a.n, a.norm);
  d.table = table; d.out = a.out;
  dispatch_note("dct.direct");
  constexpr int64_t kSlab = (int64_t)1 << 30;
  for (int64_t t0 = 0; t0 < g.tiles; t0 += kSlab) {
    const int64_t count = g.tiles - t0 < kSlab ? g.tiles - t0 : kSlab;
    d.tile0 = t0;
    hipLaunchKernelGGL(k_dct_direct, dim3((unsigned)count), dim3(kThreads), 0, c->stream, d);
    NXSIG_HIP_TRY(hipGetLastError());
  }
  return NXSIG_OK;
}

int run_fft(Ctx* c, const DctLaunch& a) {
  const int64_t rows = a.batch, n = a.n, n_used = dct_used(a.length, n);
  const float* table = nullptr;
  int rc = dct_table(c, kDctFft, a, &table);
  if (rc) return rc;
  const float2* tw = reinterpret_cast<const float2*>(table);
  void *spec = nullptr, *tmp = nullptr;
  if ((rc = ctx_scratch(c, kScratchFusedSpectrum, (size_t)rows * n * sizeof(float2), &spec))) return rc;
  // one temporary: type 2 the row means | the permuted, centred rows; type 3 the Hermitian spectra
  const size_t mean_bytes = a.type == 2 ? (((size_t)rows * sizeof(float) + 255) & ~(size_t)255) : 0;
  if ((rc = ctx_scratch(c, kScratchIstftProduct, mean_bytes + (size_t)rows * n * (a.type == 2 ? sizeof(float) : sizeof(float2)), &tmp))) return rc;
  dispatch_note("dct.fft");
  if (a.type == 2) {
    float* means = static_cast<float*>(tmp);
    float* v = reinterpret_cast<float*>(static_cast<char*>(tmp) + mean_bytes);
    const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 64;   // one workgroup per row, the rows dealt round robin beyond that
    hipLaunchKernelGGL(k_dct2_gather, dim3((unsigned)(rows < cap ? rows : cap)), dim3(kThreads), 0, c->stream, a.x, a.x_stride, n_used, n, rows, v,
                       means);
    NXSIG_HIP_TRY(hipGetLastError());
    if ((rc = launch_fft_big(c, v, true, rows, n, n, false, static_cast<float2*>(spec), false))) return rc;
    hipLaunchKernelGGL(k_dct2_post, dim3(stream_blocks(c, rows * a.keep)), dim3(kThreads), 0, c->stream, static_cast<const float2*>(spec), tw, means,
                       dct_dc_gain(n, a.norm), rows, n, a.keep, a.out);
    NXSIG_HIP_TRY(hipGetLastError());
    return NXSIG_OK;
  }
  hipLaunchKernelGGL(k_dct3_pre, dim3(stream_blocks(c, rows * n)), dim3(kThreads), 0, c->stream, a.x, a.x_stride, n_used, n, rows, tw,
                     static_cast<float2*>(tmp));
  NXSIG_HIP_TRY(hipGetLastError());
  if ((rc = launch_fft_big(c, tmp, false, rows, n, n, true, static_cast<float2*>(spec), false))) return rc;
  hipLaunchKernelGGL(k_dct3_sink, dim3(stream_blocks(c, rows * a.keep)), dim3(kThreads), 0, c->stream, static_cast<const float2*>(spec), rows, n,
                     a.keep, a.out);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace

int launch_dct(Ctx* c, const DctLaunch& a) {
  if (a.batch == 0) return NXSIG_OK;
  if (dct_tier(a.n, tune(c, kT_DISABLE_DCT_DIRECT, 0) != 0) == kDctDirect) return run_direct(c, a);
  return run_fft(c, a);
}

}  // namespace nxsig
