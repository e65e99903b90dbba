// The row LayerNorms of the Transformer's PrePostProcessingWrapper / output_normalization
// (parts/transformer/common.py:41-106, norm_params "type"), on PACKED token-major bf16 [N, D] tensors, fp32
// statistics, one wave per row. kL1 picks the kind:
//   * "layernorm_L2" (common.py:41-68, kL1 = false): y = (x - mean) * rsqrt(var + eps) * scale + bias;
//   * "layernorm_L1" (common.py:69-80, kL1 = true): c = x - mean(x), a = mean(|c|), y = c / (a + eps) * scale + bias.
//     The reference's fp16 saturate_cast has no counterpart: activations here are bf16, whose range is fp32's, so
//     the cast back cannot overflow.
// The backward also adds the residual-branch gradient of the pre-norm wrapper (common.py:99-106) and writes
// [num_parts, 2, D] parameter-gradient partials. D = 512 / 1024 are the tuned fixed-width instantiations; every
// other width D % 8 == 0, 8 <= D <= 4096 takes the any-width kernels at the end.
#include "os2s_common.hpp"

namespace os2s {

// ---------------------------------------------------------------------------
// fixed width: the row in registers
// ---------------------------------------------------------------------------
// L2 saves mean and rstd = rsqrt(var + eps), L1 mean and r = 1 / (mean|x - mean| + eps) per row; both reductions
// run on the row held in registers
template <bool kL1, int VPL>  // 16-byte vectors per lane: D = 64 * 8 * VPL
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, long long N, bf16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ r_out) {
  constexpr int D = 64 * 8 * VPL;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float v[VPL][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    unpack8(*reinterpret_cast<const u32x4*>(x + row * D + (u * 64 + lane) * 8), v[u]);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[u][e];
  }
  const float mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = v[u][e] - mean; q += kL1 ? fabsf(d) : d * d; }
  q = wave_sum(q) * (1.f / D) + eps;
  const float r = kL1 ? 1.f / q : rsqrtf(q);
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int c0 = (u * 64 + lane) * 8;
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (v[u][e] - mean) * r * gamma[c0 + e] + beta[c0 + e];
    *reinterpret_cast<u32x4*>(y + row * D + c0) = pack8(o8);
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (r_out) r_out[row] = r;
  }
}

// A buffer descriptor over the n rows of D bf16 a workgroup of the backward owns, so the prefetch past the last
// row needs no branch (out of range: zeros, no memory request).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ln_rows_rsrc(const void* base, long long r0, int n, int D) {
  const unsigned long long a = (unsigned long long)base + (unsigned long long)r0 * (unsigned)D * 2ull;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane(base ? n * D * 2 : 0);   // null tensor: everything is out of range
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}

// the registers of one prefetched row: dy, x, residual gradient (16 bytes per lane per vector) and the row's two
// saved statistics
template <int VPL>
struct LnRow {
  u32x4 a[VPL], t[VPL], r[VPL];
  float mu, rs;
};

// L2: dx = dres + rstd * (g*dy - mean_D(g*dy) - xhat * mean_D(g*dy*xhat));
//     per-block partial sums of dbeta = sum dy, dgamma = sum dy*xhat -> partial[blk][2][D].
// L1: with g = dy * scale, c = x - mean, s = sign(c) (0 at 0), r = 1 / (a + eps), a = mean|c|:
//       dc = g r - (r^2 / D) sum(g c) s,   dx = dc - mean(dc) + dres,
//     and mean(dc) = (r sum(g) - (r^2 / D) sum(g c) sum(s)) / D: the three sums are ONE reduction step per row.
//     Per-block partial sums of dbias = sum dy, dscale = sum dy * c r -> partial[blk][2][D].
//
// One wave per row, kLnWaves rows of a workgroup's block at a time. A row is two dependent steps (two
// wave reductions between its loads and its stores), so the kernel is a latency chain per wave:
// the first version (4 waves x 8 rows, loads of a row issued after the stores of the previous one,
// the residual gradient loaded after the reductions) ran at 1.1 TB/s. Now every load of row i + kLnWaves
// (dy, x, dres, mean, rstd) is issued before row i is reduced — through buffer descriptors over the
// block's rows, so the prefetch past the last row needs no branch: it is out of range, returns zeros
// and costs no memory request — and a workgroup has 8 waves.
constexpr int kLnWaves = 8;
// rows per workgroup (8 / 16 / 32 measured equal on a Transformer-big step: the step is bound by the sum of kernel
// times, not by this kernel's latency)
constexpr int kLnRowsPerBlock = 32;

__device__ __forceinline__ float sign0(float c) { return c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f); }

template <bool kL1, int VPL>
__global__ __launch_bounds__(64 * kLnWaves) void layernorm_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rsave,
    const bf16_t* __restrict__ dres, long long N, int rows_per_block, bf16_t* __restrict__ dx,
    float* __restrict__ partial) {
  constexpr int D = 64 * 8 * VPL;
  constexpr int kOob = 0x7fffffff;
  __shared__ float red[kLnWaves][D];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float gb[VPL][8], gg[VPL][8], gm[VPL][8];
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    load8(gamma + (u * 64 + lane) * 8, gm[u]);
#pragma unroll
    for (int e = 0; e < 8; ++e) { gb[u][e] = 0.f; gg[u][e] = 0.f; }
  }
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long left = N - r0;
  const int n = (int)(left < rows_per_block ? left : rows_per_block);
  const __amdgpu_buffer_rsrc_t dyr = ln_rows_rsrc(dy, r0, n, D);
  const __amdgpu_buffer_rsrc_t xr = ln_rows_rsrc(x, r0, n, D);
  const __amdgpu_buffer_rsrc_t drr = ln_rows_rsrc(dres, r0, n, D);
  const __amdgpu_buffer_rsrc_t dxr = ln_rows_rsrc(dx, r0, n, D);
  auto fetch = [&](int i, LnRow<VPL>& R) {
    const bool in = i < n;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      const int off = in ? i * (D * 2) + (u * 64 + lane) * 16 : kOob;
      R.a[u] = __builtin_amdgcn_raw_buffer_load_b128(dyr, off, 0, 0);
      R.t[u] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
      R.r[u] = __builtin_amdgcn_raw_buffer_load_b128(drr, off, 0, 0);
    }
    const long long gr = r0 + (in ? i : 0);
    R.mu = mean[gr];
    R.rs = rsave[gr];
  };
  auto process = [&](int i, const LnRow<VPL>& cur) {
    const float mu = cur.mu, rs = cur.rs;
    // kept from the sums to the dx of a row — L2: p = dy, q = xhat;  L1: p = g = gamma * dy, q = c = x - mean
    float p[VPL][8], q[VPL][8];
    // L2: s1 = sum g, s2 = sum g * xhat;  L1: s1 = sum g, s2 = sum g * c, s3 = sum sign(c)
    float s1 = 0.f, s2 = 0.f;
    [[maybe_unused]] float s3 = 0.f;
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      float dyv[8];
      unpack8(cur.a[u], dyv);
      unpack8(cur.t[u], q[u]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (kL1) {
          const float c = q[u][e] - mu;
          q[u][e] = c;
          gb[u][e] += dyv[e];
          gg[u][e] += dyv[e] * (c * rs);
          const float g = gm[u][e] * dyv[e];
          p[u][e] = g;
          s1 += g;
          s2 += g * c;
          s3 += sign0(c);
        } else {
          q[u][e] = (q[u][e] - mu) * rs;
          p[u][e] = dyv[e];
          gb[u][e] += dyv[e];
          gg[u][e] += dyv[e] * q[u][e];
          const float gd = gm[u][e] * dyv[e];
          s1 += gd;
          s2 += gd * q[u][e];
        }
      }
    }
    [[maybe_unused]] float k = 0.f, mdc = 0.f;
    if constexpr (kL1) {
      s1 = wave_sum_dpp(s1);
      s2 = wave_sum_dpp(s2);
      s3 = wave_sum_dpp(s3);
      k = rs * rs * (1.f / D) * s2;
      mdc = (rs * s1 - k * s3) * (1.f / D);
    } else {
      s1 = wave_sum_dpp(s1) * (1.f / D);
      s2 = wave_sum_dpp(s2) * (1.f / D);
    }
#pragma unroll
    for (int u = 0; u < VPL; ++u) {
      float o8[8], rv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (kL1) o8[e] = p[u][e] * rs - k * sign0(q[u][e]) - mdc;
        else o8[e] = rs * (gm[u][e] * p[u][e] - s1 - q[u][e] * s2);
      }
      unpack8(cur.r[u], rv);               // zeros without a residual gradient
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] += rv[e];
      __builtin_amdgcn_raw_buffer_store_b128(pack8(o8), dxr, i * (D * 2) + (u * 64 + lane) * 16, 0, 0);
    }
  };
  // two row buffers, used alternately (a register copy `cur = next` would have to wait for the prefetch);
  // sched_barrier: the prefetch is issued where it stands, not where hipcc would sink it to
  LnRow<VPL> ra, rb;
  fetch(wid, ra);
  for (int i = wid; i < n; i += 2 * kLnWaves) {
    fetch(i + kLnWaves, rb);
    __builtin_amdgcn_sched_barrier(0);
    process(i, ra);
    if (i + kLnWaves >= n) break;
    fetch(i + 2 * kLnWaves, ra);
    __builtin_amdgcn_sched_barrier(0);
    process(i + kLnWaves, rb);
  }
  // block reduce the parameter-gradient partials over the waves (fixed order)
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VPL; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        red[wid][(u * 64 + lane) * 8 + e] = pass == 0 ? gb[u][e] : gg[u][e];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 64 * kLnWaves) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < kLnWaves; ++w) acc += red[w][c];
      partial[((long long)blockIdx.x * 2 + pass) * D + c] = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// any width D % 8 == 0, 8 <= D <= 4096
// ---------------------------------------------------------------------------
// One wave per row with a RUNTIME loop over the row's 16-byte pieces. A row (at most 8 KB) is read again from the
// cache for every pass instead of being held in a register array a runtime index would demote to scratch. Same
// results, saved statistics and [num_parts, 2, D] partial layout as the fixed-width kernels. Not tuned.
constexpr int kLnAnyMaxD = 4096;
static inline bool ln_any_width_ok(int D) { return D >= 8 && D <= kLnAnyMaxD && D % 8 == 0; }

template <bool kL1>
__global__ __launch_bounds__(256) void layernorm_any_fwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, long long N, int D, bf16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ r_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int D8 = D >> 3;
  const bf16_t* xr = x + row * D;
  const float fD = (float)D;      // divisions, not a reciprocal: 1 / D is inexact when D is no power of two, and a
  float s = 0.f;                  // constant row must come out with mean == x exactly (L1: mean|x - mean| = 0)
  for (int c = lane; c < D8; c += 64) {
    float v[8];
    unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  }
  const float mean = wave_sum(s) / fD;
  float q = 0.f;
  for (int c = lane; c < D8; c += 64) {
    float v[8];
    unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; q += kL1 ? fabsf(d) : d * d; }
  }
  q = wave_sum(q) / fD;
  const float r = kL1 ? 1.f / (q + eps) : rsqrtf(q + eps);
  for (int c = lane; c < D8; c += 64) {
    float v[8], o8[8];
    unpack8(*reinterpret_cast<const u32x4*>(xr + c * 8), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (v[e] - mean) * r * gamma[c * 8 + e] + beta[c * 8 + e];
    *reinterpret_cast<u32x4*>(y + row * D + c * 8) = pack8(o8);
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (r_out) r_out[row] = r;
  }
}

// One workgroup per block of rows_per_block rows (the num_parts of the fixed-width kernels). First the
// parameter-gradient partials, one column per thread over the block's rows in a fixed order:
//   partial[blk][0][c] = sum dy, partial[blk][1][c] = sum dy * (x - mean) * r;
// then one wave per row: dx = dres + (the formulas of layernorm_bwd_kernel).
template <bool kL1>
__global__ __launch_bounds__(512) void layernorm_any_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rsave,
    const bf16_t* __restrict__ dres, long long N, int D, int rows_per_block, bf16_t* __restrict__ dx,
    float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long left = N - r0;
  const int n = (int)(left < rows_per_block ? left : rows_per_block);
  for (int c = threadIdx.x; c < D; c += 512) {
    float sb = 0.f, sg = 0.f;
    for (int i = 0; i < n; ++i) {
      const float d = bf2f(dy[(r0 + i) * D + c]);
      sb += d;
      sg += d * ((bf2f(x[(r0 + i) * D + c]) - mean[r0 + i]) * rsave[r0 + i]);
    }
    partial[((long long)blockIdx.x * 2) * D + c] = sb;
    partial[((long long)blockIdx.x * 2 + 1) * D + c] = sg;
  }
  const int D8 = D >> 3;
  const float invD = 1.f / (float)D;
  for (int i = wid; i < n; i += 8) {
    const long long ro = (r0 + i) * D;
    const float mu = mean[r0 + i], rs = rsave[r0 + i];
    // L2: s1 = sum g, s2 = sum g * xhat;  L1: s1 = sum g, s2 = sum g * c, s3 = sum sign(c)   (g = gamma * dy)
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = lane; c < D8; c += 64) {
      float dv[8], xv[8];
      unpack8(*reinterpret_cast<const u32x4*>(dy + ro + c * 8), dv);
      unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = gamma[c * 8 + e] * dv[e];
        const float cc = xv[e] - mu;
        s1 += g;
        s2 += g * (kL1 ? cc : cc * rs);
        if (kL1) s3 += cc > 0.f ? 1.f : (cc < 0.f ? -1.f : 0.f);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (kL1) s3 = wave_sum(s3);
    const float k = rs * rs * invD * s2;                 // L1
    const float mdc = (rs * s1 - k * s3) * invD;         // L1
    for (int c = lane; c < D8; c += 64) {
      float dv[8], xv[8], rv[8], o8[8];
      unpack8(*reinterpret_cast<const u32x4*>(dy + ro + c * 8), dv);
      unpack8(*reinterpret_cast<const u32x4*>(x + ro + c * 8), xv);
      u32x4 t = {0u, 0u, 0u, 0u};
      if (dres) t = *reinterpret_cast<const u32x4*>(dres + ro + c * 8);
      unpack8(t, rv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = gamma[c * 8 + e] * dv[e];
        const float cc = xv[e] - mu;
        if (kL1) {
          const float sgn = cc > 0.f ? 1.f : (cc < 0.f ? -1.f : 0.f);
          o8[e] = g * rs - k * sgn - mdc + rv[e];
        } else {
          o8[e] = rs * (g - s1 * invD - cc * rs * (s2 * invD)) + rv[e];
        }
      }
      *reinterpret_cast<u32x4*>(dx + ro + c * 8) = pack8(o8);
    }
  }
}

// ---------------------------------------------------------------------------
// launch choice: 1024 and 512 are the tuned instantiations, every other width the runtime column loop
// ---------------------------------------------------------------------------
template <bool kL1>
static int layernorm_fwd(os2s_stream_t stream, const uint16_t* x, const float* gamma, const float* beta, float eps,
                         long long N, int D, uint16_t* y, float* mean, float* rsave) {
  OS2S_REQUIRE(x && gamma && beta && y && N >= 0);
  if (N == 0) return OS2S_OK;
  const dim3 grid(ceil_div(N, 4));
  if (D == 1024) {
    OS2S_LAUNCH((layernorm_fwd_kernel<kL1, 2>), grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, N, y,
                mean, rsave);
  } else if (D == 512) {
    OS2S_LAUNCH((layernorm_fwd_kernel<kL1, 1>), grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, N, y,
                mean, rsave);
  } else if (ln_any_width_ok(D)) {
    OS2S_LAUNCH(layernorm_any_fwd_kernel<kL1>, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, N, D, y,
                mean, rsave);
  } else {
    return OS2S_ERR_UNSUPPORTED;
  }
  return OS2S_OK;
}

// partial: [num_parts, 2, D] (row 0: sum dy = dbeta, row 1: sum dy*xhat = dgamma); reduce it
// with os2s_bn_bwd_finalize(partial, nparts, nq=2, q=1, C=D, ...).
template <bool kL1>
static int layernorm_bwd(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x, const float* gamma,
                         const float* mean, const float* rsave, const uint16_t* dres, long long N, int D,
                         uint16_t* dx, float* partial) {
  OS2S_REQUIRE(dy && x && gamma && mean && rsave && dx && partial && N >= 0);
  if (N == 0) return OS2S_OK;
  const dim3 grid(ceil_div(N, kLnRowsPerBlock));
  if (D == 1024) {
    OS2S_LAUNCH((layernorm_bwd_kernel<kL1, 2>), grid, dim3(64 * kLnWaves), 0, (hipStream_t)stream, dy, x, gamma, mean,
                rsave, dres, N, kLnRowsPerBlock, dx, partial);
  } else if (D == 512) {
    OS2S_LAUNCH((layernorm_bwd_kernel<kL1, 1>), grid, dim3(64 * kLnWaves), 0, (hipStream_t)stream, dy, x, gamma, mean,
                rsave, dres, N, kLnRowsPerBlock, dx, partial);
  } else if (ln_any_width_ok(D)) {
    OS2S_LAUNCH(layernorm_any_bwd_kernel<kL1>, grid, dim3(512), 0, (hipStream_t)stream, dy, x, gamma, mean, rsave,
                dres, N, D, kLnRowsPerBlock, dx, partial);
  } else {
    return OS2S_ERR_UNSUPPORTED;
  }
  return OS2S_OK;
}

}  // namespace os2s

using namespace os2s;

extern "C" int os2s_layernorm_fwd(os2s_stream_t stream, const uint16_t* x, const float* gamma,
                                  const float* beta, float eps, long long N, int D, uint16_t* y,
                                  float* mean, float* rstd) {
  return layernorm_fwd<false>(stream, x, gamma, beta, eps, N, D, y, mean, rstd);
}

extern "C" int os2s_layernorm_bwd_num_parts(long long N) { return ceil_div(N, kLnRowsPerBlock); }

extern "C" int os2s_layernorm_bwd(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x,
                                  const float* gamma, const float* mean, const float* rstd,
                                  const uint16_t* dres, long long N, int D, uint16_t* dx,
                                  float* partial) {
  return layernorm_bwd<false>(stream, dy, x, gamma, mean, rstd, dres, N, D, dx, partial);
}

extern "C" int os2s_layernorm_l1_fwd(os2s_stream_t stream, const uint16_t* x, const float* gamma,
                                     const float* beta, float eps, long long N, int D, uint16_t* y,
                                     float* mean, float* rinv) {
  return layernorm_fwd<true>(stream, x, gamma, beta, eps, N, D, y, mean, rinv);
}

extern "C" int os2s_layernorm_l1_bwd_num_parts(long long N) { return ceil_div(N, kLnRowsPerBlock); }

extern "C" int os2s_layernorm_l1_bwd(os2s_stream_t stream, const uint16_t* dy, const uint16_t* x,
                                     const float* gamma, const float* mean, const float* rinv,
                                     const uint16_t* dres, long long N, int D, uint16_t* dx,
                                     float* partial) {
  return layernorm_bwd<true>(stream, dy, x, gamma, mean, rinv, dres, N, D, dx, partial);
}
