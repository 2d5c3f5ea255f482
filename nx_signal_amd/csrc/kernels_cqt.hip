// Spectral.cqt / vqt: C[k, t] = sum_n x~[t hop + n] A_k[n] on every row, A_k = g_k conj(b_k) a bank of centred complex kernels of
// different lengths, handed over as data.  include/nxsig.h states the definition, DESIGN.md section 3.27 the design; the argument checks,
// the bin tiles and the table layout are csrc/cqt_plan.hpp.
//   cqt.mfma    a banded real-by-complex GEMM on v_mfma_f32_16x16x4_f32: 16 bins (sorted by length) on M, 16 frames on N, samples on
//               K.  A workgroup of 4 waves serves (row, bin tile, 128 frames), a wave 2 frame tiles.  The tile's n range is walked in
//               sub-panels of 64 samples: the basis sub-panel (8 KB, one contiguous piece of the table, zero where a bin is shorter)
//               goes to LDS once for the 128 frames, every wave stages its own 32 frames' 64 samples frame-major at a pitch of 68
//               words (lane = sample: coalesced loads, conflict-free writes for ANY hop), and a lane then reads its 16 K values of a
//               frame as four 16-byte LDS reads (the table's cell order makes them consecutive samples).  Real and imaginary parts are
//               two accumulator sets that share the signal operand; a step's basis operand serves both frame tiles.  After every 8
//               sub-panels (a panel of 512 samples) the f32 accumulators are added to double ones and cleared, in that fixed order.
//   cqt.direct  one wave per (bin, 8 frames): taps in chunks of 256, each frame's samples of the chunk through LDS, products and sums
//               in double, lane sums reduced by lane shuffles in a fixed order.  No padding, no table but the bank itself.
// Non-finite rule: both tiers load a non-finite sample as +0 and decide NaN at the store from the row's non-finite prefix counts
// (Ctx::cqt_mask: one bit per sample; Ctx::cqt_count: non-finite samples ahead of each 64-sample word), formed by two small launches
// ahead of either tier: output (k, t) is NaN exactly when [t hop + lo_k, t hop + lo_k + N_k - 1] holds one.
// Deterministic: an output's bits depend on its row's samples, hop and the bank alone; no atomics.
#include <cstring>

#include "nxsig_internal.h"

namespace nxsig {

namespace {

typedef float cq4 __attribute__((ext_vector_type(4)));

struct CqtArgs {
  const float* x;                // f32 rows, `stride` elements apart
  int64_t stride, len, hop, F, batch;
  const int64_t* meta;           // [3][n_bins]: lo, offset into the concatenated taps, count
  const float2* const* pieces;   // the table (cqt.mfma: 128 sub-panels per piece) or the taps (cqt.direct: 2^17 per piece)
  const int64_t* plan;           // cqt.mfma: [tiles][5] (CqtTile), then the sorted bins [n_bins]
  const uint64_t* mask;          // [batch][words] non-finite bits
  const uint32_t* count;         // [batch][words] non-finite samples ahead of the word
  int64_t words;
  void* out;                     // c64 or f32 [batch][n_bins][F]
  int64_t fblocks;               // frame blocks per row
  int32_t n_bins, tiles;
};

constexpr int kTablePieceSubs = 128;          // 128 sub-panels of 8 KB: every piece of a table stays within the cache's verified 1 MiB
constexpr int kTapsPieceShift = 17;           // 2^17 complex taps likewise

__device__ __forceinline__ bool cq_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ float cq_load(const float* xr, int64_t pos, int64_t len, bool frame_ok) {
  float v = 0.0f;
  if (frame_ok && pos >= 0 && pos < len) v = xr[pos];
  return cq_nonfinite(v) ? 0.0f : v;
}
// non-finite samples in [0, p) of the row, p <= len
__device__ __forceinline__ uint32_t cq_below(const uint64_t* mask, const uint32_t* count, int64_t p) {
  const int64_t w = p >> 6;
  return count[w] + (uint32_t)__popcll(mask[w] & ((1ull << (p & 63)) - 1ull));
}
template <int KIND>
__device__ __forceinline__ void cq_store(const CqtArgs& a, int64_t row, int64_t k, int64_t t, double re, double im) {
  int64_t s0 = t * a.hop + a.meta[k], s1 = s0 + a.meta[2 * a.n_bins + k] - 1;
  s0 = s0 < 0 ? 0 : s0; s1 = s1 >= a.len ? a.len - 1 : s1;
  bool bad = false;
  if (s0 <= s1) {
    const uint64_t* m = a.mask + row * a.words;
    const uint32_t* c = a.count + row * a.words;
    bad = cq_below(m, c, s1 + 1) != cq_below(m, c, s0);
  }
  const int64_t at = (row * a.n_bins + k) * a.F + t;
  const float nan32 = __builtin_nanf("");
  if constexpr (KIND == kCqComplex) static_cast<float2*>(a.out)[at] = bad ? make_float2(nan32, nan32) : make_float2((float)re, (float)im);
  else if constexpr (KIND == kCqMagnitude) static_cast<float*>(a.out)[at] = bad ? nan32 : (float)__builtin_sqrt(re * re + im * im);
  else static_cast<float*>(a.out)[at] = bad ? nan32 : (float)(re * re + im * im);
}

// ---- the non-finite bits of every row, then the counts ahead of each word (one workgroup per row)
__global__ __launch_bounds__(256) void k_cqt_mask(const float* __restrict__ x, int64_t stride, int64_t len, int64_t words, int64_t units,
                                                  uint64_t* __restrict__ mask) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6); u < units; u += waves) {
    const int64_t row = u / words, pos = (u - row * words) * 64 + lane;
    const float v = pos < len ? x[row * stride + pos] : 0.0f;
    const uint64_t m = __ballot(cq_nonfinite(v));
    if (lane == 0) mask[u] = m;
  }
}
__global__ __launch_bounds__(256) void k_cqt_count(const uint64_t* __restrict__ mask, int64_t words, uint32_t* __restrict__ count) {
  __shared__ uint32_t part[256];
  const int t = (int)threadIdx.x;
  const uint64_t* m = mask + (int64_t)blockIdx.x * words;
  uint32_t* c = count + (int64_t)blockIdx.x * words;
  const int64_t per = (words + 255) / 256, b = t * per, e = b + per < words ? b + per : words;
  uint32_t s = 0;
  for (int64_t i = b; i < e; ++i) s += (uint32_t)__popcll(m[i]);
  part[t] = s;
  __syncthreads();
  uint32_t run = 0;
  for (int j = 0; j < t; ++j) run += part[j];
  for (int64_t i = b; i < e; ++i) { c[i] = run; run += (uint32_t)__popcll(m[i]); }
}

// ---- cqt.mfma
template <int KIND>
__global__ __launch_bounds__(64 * kCqtWaves) void k_cqt_mfma(CqtArgs a) {
  __shared__ __attribute__((aligned(16))) float sB[kCqtBlockFrames * kCqtPitch];
  __shared__ __attribute__((aligned(16))) float2 sA[kCqtSub / 4 * 64];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
  int64_t b = blockIdx.x;
  const int64_t fb = b % a.fblocks; b /= a.fblocks;
  const int64_t row = b % a.batch, tile = b / a.batch;   // the longest tile's workgroups come first
  const int64_t* tp = a.plan + tile * 5;
  const int64_t first = tp[0], bins = tp[1], n_lo = tp[2], subs = tp[3], sub_off = tp[4];
  const float* xr = a.x + row * a.stride;
  constexpr int kWaveFrames = kCqtWaveTiles * kCqtTileFrames;
  const int64_t t0 = fb * kCqtBlockFrames + wave * kWaveFrames;   // the wave's first frame
  const bool live = t0 < a.F;                                     // per wave
  float* mine = sB + wave * kWaveFrames * kCqtPitch;

  cq4 acc[kCqtWaveTiles][2];
  double sum[kCqtWaveTiles][2][4];
#pragma unroll
  for (int ft = 0; ft < kCqtWaveTiles; ++ft)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      acc[ft][p] = cq4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int v = 0; v < 4; ++v) sum[ft][p][v] = 0.0;
    }

  for (int64_t u = 0; u < subs; ++u) {
    __syncthreads();   // every wave has read the sub-panel before
    {   // the basis sub-panel: 8 KB, once for the workgroup's 128 frames
      const int64_t s = sub_off + u;
      const float4* src = reinterpret_cast<const float4*>(a.pieces[s / kTablePieceSubs] + (s % kTablePieceSubs) * (kCqtSub / 4 * 64));
      float4* dst = reinterpret_cast<float4*>(sA);
      dst[tid] = src[tid];
      dst[tid + 256] = src[tid + 256];
    }
    if (live) {   // the wave's own frames: lane = sample of the sub-panel
      const int64_t nb = n_lo + u * kCqtSub + lane;
#pragma unroll 8
      for (int f = 0; f < kWaveFrames; ++f) {
        const int64_t t = t0 + f;
        mine[f * kCqtPitch + lane] = cq_load(xr, t * a.hop + nb, a.len, t < a.F);
      }
    }
    __syncthreads();
    if (live) {
      const float* b0 = mine + col * kCqtPitch + g * 16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cq4 bv[kCqtWaveTiles];
#pragma unroll
        for (int ft = 0; ft < kCqtWaveTiles; ++ft) bv[ft] = *reinterpret_cast<const cq4*>(b0 + ft * kCqtTileFrames * kCqtPitch + 4 * j);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float2 w = sA[(4 * j + s) * 64 + lane];
#pragma unroll
          for (int ft = 0; ft < kCqtWaveTiles; ++ft) {
            acc[ft][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, bv[ft][s], acc[ft][0], 0, 0, 0);
            acc[ft][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, bv[ft][s], acc[ft][1], 0, 0, 0);
          }
        }
      }
      if ((u + 1) % kCqtPanelSubs == 0 || u + 1 == subs) {   // the panel's end: into the double sums, in the order of the panels
#pragma unroll
        for (int ft = 0; ft < kCqtWaveTiles; ++ft)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int v = 0; v < 4; ++v) sum[ft][p][v] += (double)acc[ft][p][v];
            acc[ft][p] = cq4{0.0f, 0.0f, 0.0f, 0.0f};
          }
      }
    }
  }
  if (!live) return;
  // lane (g, col) holds bins 4 g + v of the tile at frame col of each frame tile: 16 lanes write 16 consecutive frames of a bin
  const int64_t* order = a.plan + (int64_t)a.tiles * 5;
#pragma unroll
  for (int ft = 0; ft < kCqtWaveTiles; ++ft)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t m = 4 * g + v, t = t0 + ft * kCqtTileFrames + col;
      if (m < bins && t < a.F) cq_store<KIND>(a, row, order[first + m], t, sum[ft][0][v], sum[ft][1][v]);
    }
}

// ---- cqt.direct
template <int KIND>
__global__ __launch_bounds__(64) void k_cqt_direct(CqtArgs a) {
  __shared__ float s[kCqtDirectFrames][kCqtDirectChunk];
  const int lane = (int)threadIdx.x;
  int64_t b = blockIdx.x;
  const int64_t fb = b % a.fblocks; b /= a.fblocks;
  const int64_t row = b % a.batch, k = b / a.batch;
  const int64_t lo = a.meta[k], off = a.meta[a.n_bins + k], N = a.meta[2 * a.n_bins + k], t0 = fb * kCqtDirectFrames;
  const float* xr = a.x + row * a.stride;
  double re[kCqtDirectFrames], im[kCqtDirectFrames];
#pragma unroll
  for (int f = 0; f < kCqtDirectFrames; ++f) re[f] = im[f] = 0.0;
  for (int64_t c0 = 0; c0 < N; c0 += kCqtDirectChunk) {
    const int clen = (int)(N - c0 < kCqtDirectChunk ? N - c0 : kCqtDirectChunk);
    __syncthreads();
#pragma unroll
    for (int f = 0; f < kCqtDirectFrames; ++f)
      for (int i = lane; i < clen; i += 64) s[f][i] = cq_load(xr, (t0 + f) * a.hop + lo + c0 + i, a.len, t0 + f < a.F);
    __syncthreads();
    for (int i = lane; i < clen; i += 64) {
      const int64_t j = off + c0 + i;
      const float2 w = a.pieces[j >> kTapsPieceShift][j & ((1 << kTapsPieceShift) - 1)];
      const double wr = (double)w.x, wi = (double)w.y;
#pragma unroll
      for (int f = 0; f < kCqtDirectFrames; ++f) {
        const double xv = (double)s[f][i];
        re[f] = __builtin_fma(wr, xv, re[f]);
        im[f] = __builtin_fma(wi, xv, im[f]);
      }
    }
  }
#pragma unroll
  for (int f = 0; f < kCqtDirectFrames; ++f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      re[f] += __shfl_xor(re[f], o, 64);
      im[f] += __shfl_xor(im[f], o, 64);
    }
    if (lane == f && t0 + f < a.F) cq_store<KIND>(a, row, k, t0 + f, re[f], im[f]);
  }
}

// ---- the bank on the device, formed once per context, bank and tier.  Every table goes through ctx_table in pieces of at most 1 MiB,
// so every hash hit of the table cache is verified against its host copy; the memo that keeps the pointers is matched on two independent
// 64-bit hashes of (lo, count, taps) and on the sizes, as cwt's is
struct CqtTables { const int64_t* meta; const float2* const* pieces; const int64_t* plan; int64_t tiles; };

int cqt_pieces(Ctx* c, uint64_t tag, const float2* host, int64_t cells, int64_t piece, const void** out) {
  std::vector<const void*> ptrs;
  for (int64_t at = 0; at < cells; at += piece) {
    const void* d = nullptr;
    const int rc = ctx_table(c, tag, host + at, (size_t)std::min(piece, cells - at) * sizeof(float2), &d);
    if (rc) return rc;
    ptrs.push_back(d);
  }
  return ctx_table(c, tag ^ 0xFFull, ptrs.data(), ptrs.size() * sizeof(void*), out);
}

int cqt_device_tables(Ctx* c, const CqtLaunch& l, bool mfma, CqtTables* t) {
  const int64_t n = l.n_bins;
  uint64_t h1 = 0xC0710001ull, h2 = 0x9E3779B97F4A7C15ull;
  h1 = fnv1a(h1, l.lo_host, (size_t)n * 8); h2 = fnv1a(h2, l.lo_host, (size_t)n * 8);
  h1 = fnv1a(h1, l.count_host, (size_t)n * 4); h2 = fnv1a(h2, l.count_host, (size_t)n * 4);
  h1 = fnv1a(h1, l.taps_host, (size_t)l.total * 8); h2 = fnv1a(h2, l.taps_host, (size_t)l.total * 8);
  std::vector<uint64_t> want = {0, 0, 0, 0, h2, (uint64_t)n, (uint64_t)l.total, (uint64_t)mfma};
  const uint64_t key = fnv1a(0xC0710000ull ^ h1, want.data() + 4, (want.size() - 4) * sizeof(uint64_t));
  auto hit = c->memo.find(key);
  if (hit == c->memo.end() || hit->second.size() != want.size() || !std::equal(want.begin() + 4, want.end(), hit->second.begin() + 4)) {
    std::vector<int64_t> meta((size_t)3 * n);
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k) { meta[k] = l.lo_host[k]; meta[n + k] = at; meta[2 * n + k] = l.count_host[k]; at += l.count_host[k]; }
    const void *dm = nullptr, *dp = nullptr, *dl = nullptr;
    int rc = ctx_table(c, 0xC0710A00ull, meta.data(), meta.size() * sizeof(int64_t), &dm);
    if (rc) return rc;
    const float2* taps = static_cast<const float2*>(l.taps_host);
    if (mfma) {
      CqtPlan p;
      cqt_plan(n, l.lo_host, l.count_host, &p);
      std::vector<float2> table((size_t)p.subs_total * (kCqtSub / 4 * 64), make_float2(0.0f, 0.0f));
      std::vector<int64_t> plan;
      for (const CqtTile& tl : p.tiles) {
        plan.insert(plan.end(), {tl.first, tl.bins, tl.n_lo, tl.subs, tl.sub_off});
        for (int64_t m = 0; m < tl.bins; ++m) {
          const int64_t k = p.order[(size_t)(tl.first + m)];
          for (int64_t i = 0; i < l.count_host[k]; ++i) table[(size_t)cqt_cell(tl, m, l.lo_host[k] + i)] = taps[meta[n + k] + i];
        }
      }
      for (int32_t k : p.order) plan.push_back(k);
      if ((rc = cqt_pieces(c, 0xC0710B00ull, table.data(), (int64_t)table.size(), (int64_t)kTablePieceSubs * (kCqtSub / 4 * 64), &dp))) return rc;
      if ((rc = ctx_table(c, 0xC0710C00ull, plan.data(), plan.size() * sizeof(int64_t), &dl))) return rc;
      want[3] = (uint64_t)p.tiles.size();
    } else {
      if ((rc = cqt_pieces(c, 0xC0710D00ull, taps, l.total, (int64_t)1 << kTapsPieceShift, &dp))) return rc;
    }
    want[0] = (uint64_t)(uintptr_t)dm; want[1] = (uint64_t)(uintptr_t)dp; want[2] = (uint64_t)(uintptr_t)dl;
    c->memo[key] = want;
    hit = c->memo.find(key);
  }
  const std::vector<uint64_t>& got = hit->second;
  t->meta = reinterpret_cast<const int64_t*>((uintptr_t)got[0]);
  t->pieces = reinterpret_cast<const float2* const*>((uintptr_t)got[1]);
  t->plan = reinterpret_cast<const int64_t*>((uintptr_t)got[2]);
  t->tiles = (int64_t)got[3];
  return NXSIG_OK;
}

// one of the family's own buffers, grown on demand (the stream is drained before a buffer in use is replaced, as ctx_scratch does)
int cqt_buffer(Ctx* c, Ctx::OwnedBuffer& b, size_t bytes, void** out) {
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

template <int KIND>
int run_kind(Ctx* c, CqtArgs& g, bool mfma) {
  const int64_t per = mfma ? kCqtBlockFrames : kCqtDirectFrames;
  g.fblocks = (g.F + per - 1) / per;
  const int64_t units = mfma ? g.tiles : g.n_bins;
  if (g.fblocks > 0x7fffffffLL / units / g.batch) return set_error(NXSIG_ERR_UNSUPPORTED, "cqt: too many blocks for one launch");
  const dim3 grid((unsigned)(g.fblocks * g.batch * units));
  if (mfma) hipLaunchKernelGGL(k_cqt_mfma<KIND>, grid, dim3(64 * kCqtWaves), 0, c->stream, g);
  else hipLaunchKernelGGL(k_cqt_direct<KIND>, grid, dim3(64), 0, c->stream, g);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace

int launch_cqt(Ctx* c, const CqtLaunch& l) {
  if (l.batch == 0) return NXSIG_OK;
  const bool mfma = tune(c, kT_CQT_MFMA, 1) != 0;
  CqtTables t;
  int rc = cqt_device_tables(c, l, mfma, &t);
  if (rc) return rc;
  CqtArgs g = {};
  g.x = static_cast<const float*>(l.x); g.stride = l.x_stride; g.len = l.length; g.hop = l.hop; g.batch = l.batch;
  g.F = cqt_frames(l.length, l.hop);
  g.meta = t.meta; g.pieces = t.pieces; g.plan = t.plan; g.tiles = (int32_t)t.tiles; g.n_bins = (int32_t)l.n_bins; g.out = l.out;
  g.words = (l.length >> 6) + 1;   // the word that position `length` falls into is there too
  void *mask = nullptr, *count = nullptr;
  if ((rc = cqt_buffer(c, c->cqt_mask, (size_t)l.batch * g.words * sizeof(uint64_t), &mask))) return rc;
  if ((rc = cqt_buffer(c, c->cqt_count, (size_t)l.batch * g.words * sizeof(uint32_t), &count))) return rc;
  g.mask = static_cast<const uint64_t*>(mask); g.count = static_cast<const uint32_t*>(count);
  const int64_t units = l.batch * g.words, need = (units + 3) / 4, cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 1) * 32;
  hipLaunchKernelGGL(k_cqt_mask, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, c->stream, g.x, g.stride, g.len, g.words, units,
                     static_cast<uint64_t*>(mask));
  NXSIG_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_cqt_count, dim3((unsigned)l.batch), dim3(256), 0, c->stream, g.mask, g.words, static_cast<uint32_t*>(count));
  NXSIG_HIP_TRY(hipGetLastError());
  dispatch_note(mfma ? "cqt.mfma" : "cqt.direct");
  switch (l.kind) {
    case kCqComplex: return run_kind<kCqComplex>(c, g, mfma);
    case kCqMagnitude: return run_kind<kCqMagnitude>(c, g, mfma);
    default: return run_kind<kCqPower>(c, g, mfma);
  }
}

}  // namespace nxsig
